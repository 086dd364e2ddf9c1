"""Warp, WarpV2, invert_flow and occlusion_map on the GPU under non-finite and beyond-`int` flows, against the rule of
include/qpwc.h as tests/test_nonfinite_flow_cpu.py restates it (explicit sat_trunc, pixel by pixel), on that module's
fixtures: 2 x 9 x 14, a smooth flow within 0.75 px with one planted value a pixel -- NaN, +-Inf, +-3e9, +-2147483648,
2147483520, 1e10 and flows that land exactly on W - 1, W and -1 (fp16 storage: NaN, +-Inf, +-65504 and the landings).

These are value tests: that module's docstring lists the lines that clamp every address derived from a flow value after
the conversion.  Asserted for every op, layout and dtype:
  * an output element that reads no planted pixel has the bits of the run on the clean flow;
  * every element equals the restatement: NaN exactly where it has NaN, the same bits elsewhere;
  * the map equals the restatement's everywhere;
  * two runs are bit-identical;
  * every planted value reached the op (the tensor handed over is read back, after the fp16 cast).
Mutation, on paper: `x0 == INT32_MAX ? x0 : x0 + 1` to `x0 + 1` in taps_tfwarp makes the second corner of the planted
2147483648 wrap to INT32_MIN and clamp to column 0: Warp and invert_flow then differ from the restatement at those pixels
(tests/test_nonfinite_flow_cpu.py::test_the_guard_is_visible shows the two readings differ on this fixture)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_nonfinite_flow_cpu import fixture, ref_invert_flow, ref_occlusion, ref_warp, same, where_differs  # noqa: E402

from qpwcnet_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYOUTS = ["channels_last", "channels_first"]
_REFS = {}


def refs(half):
    """The restatement's answers for a dtype, computed once: {(what, planted?): array} in channels-last float32."""
    if half not in _REFS:
        img, clean, planted, mask = fixture(half)
        out = {}
        for tag, flo in (("clean", clean), ("planted", planted)):
            for mode in ("tfwarp", "clamp"):
                for C in (3, 8):
                    out["warp", mode, C, tag] = ref_warp(img[..., :C], flo, mode)
            out["inv", tag], out["reads", tag] = ref_invert_flow(flo)
            out["occ", tag] = ref_occlusion(flo)
        _REFS[half] = out
    return _REFS[half]


def to_dev(a, layout, half):
    """A channels-last float32 array as a dense device tensor of the layout and dtype."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = t.half() if half else t
    return t.permute(0, 3, 1, 2).contiguous() if layout == "channels_first" else t


def to_host(t, layout):
    """-> channels-last numpy of the tensor's own dtype."""
    t = t.permute(0, 2, 3, 1) if layout == "channels_first" and t.dim() == 4 else t
    return np.ascontiguousarray(t.cpu().numpy())


def storage(a, half):
    return a.astype(np.float16) if half else a


def reached(t, layout, want, half):
    """The tensor handed to the op holds the planted values: NaN where planted, the same bits elsewhere."""
    return same(to_host(t, layout), storage(want, half))


@pytest.mark.parametrize("C", [3, 8], ids=["C3", "C8"])             # the element-wise kernels; the 16-byte ones
@pytest.mark.parametrize("mode", ["tfwarp", "clamp"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_warp(half, layout, mode, C):
    img, clean, planted, mask = fixture(half)
    r = refs(half)
    ti = to_dev(img[..., :C], layout, half)
    got = {}
    for tag, flo in (("clean", clean), ("planted", planted)):
        tf = to_dev(flo, layout, half)                               # fp16 storage: an fp16 flow, cast by ops.warp
        assert reached(tf, layout, flo, half)
        one, two = ops.warp(ti, tf, mode, layout), ops.warp(ti, tf, mode, layout)
        assert one.dtype == ti.dtype and same(to_host(one, layout), to_host(two, layout))
        got[tag] = to_host(one, layout)
        with np.errstate(all="ignore"):
            want = storage(r["warp", mode, C, tag], half)
        assert same(got[tag], want), (tag, where_differs(got[tag].astype(np.float32), want.astype(np.float32))[:5])
    # a pixel's output reads the flow of that pixel only
    assert same(got["planted"][~mask], got["clean"][~mask])
    assert np.isfinite(got["clean"]).all() and np.isnan(got["planted"].astype(np.float32)[mask]).any() == (mode == "tfwarp")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_invert_flow_and_occlusion_map(half, layout):
    img, clean, planted, mask = fixture(half)
    r = refs(half)
    got = {}
    for tag, flo in (("clean", clean), ("planted", planted)):
        tf = to_dev(flo, layout, half)
        assert reached(tf, layout, flo, half)
        inv, inv2 = ops.invert_flow(tf, layout), ops.invert_flow(tf, layout)
        occ, occ2 = ops.occlusion_map(tf, layout), ops.occlusion_map(tf, layout)
        assert inv.dtype == tf.dtype and occ.dtype == torch.float32
        assert same(to_host(inv, layout), to_host(inv2, layout)) and torch.equal(occ, occ2)
        got[tag] = (to_host(inv, layout), occ.cpu().numpy())
        with np.errstate(all="ignore"):
            want = storage(r["inv", tag], half)
        assert same(got[tag][0], want), (tag, where_differs(got[tag][0].astype(np.float32), want.astype(np.float32))[:5])
        assert np.array_equal(got[tag][1], r["occ", tag]), (tag, np.argwhere(got[tag][1] != r["occ", tag]).tolist()[:5])
        assert set(np.unique(got[tag][1])) == {0.0, 1.0}
    # an inverse-flow pixel that is not planted and whose four corners are not planted has the clean run's bits
    reads = r["reads", "clean"]
    B, H, W = mask.shape
    free = ~mask & ~np.array([[[any(mask[b, ty, tx] for ty, tx in reads[b, y, x]) for x in range(W)] for y in range(H)]
                              for b in range(B)])
    assert 0.3 * mask.size < free.sum() < mask.size - mask.sum()
    assert same(got["planted"][0][free], got["clean"][0][free])
    assert not same(got["planted"][0], got["clean"][0]) and np.isfinite(got["clean"][0].astype(np.float32)).all()

"""Non-finite and beyond-`int` flows: the rule of include/qpwc.h (qpwc_warp_fwd, qpwc_invert_flow_fwd,
qpwc_occlusion_fwd), restated here pixel by pixel with an explicit ``sat_trunc``, and every CPU chain held to it.

A diverged model produces NaN and Inf flows, a .flo file marks "unknown" with 1e10.  What the kernels do with them
(csrc/common.h, csrc/occlusion.hip) is the shipped behaviour:
  * the float -> int conversion of tf_warp's corner (`(int)xf`, v_cvt_i32_f32) truncates toward zero, saturates at
    INT32_MIN / INT32_MAX and turns NaN into 0;
  * the second corner of a corner saturated at INT32_MAX is that corner (`x0 == INT32_MAX ? x0 : x0 + 1`), not the
    wrapped INT32_MIN;
  * the corners are clamped into the image AFTER the conversion, the weights use the clamped corners and the raw sum;
  * WarpV2's taps clamp in floating point first, with fmaxf / fminf, which return their other operand for a NaN: a NaN
    coordinate gives corner 0 and alpha 0, +Inf the last corner pair and alpha 1, -Inf corner 0 and alpha 0;
  * the occlusion target `(int)((float)y + inv.y)` converts the same way and is clamped into the image.
Every address derived from a flow value is clamped after the conversion -- read in the sources, and listed here so
that a change to one of these lines is looked at with this file open:
  csrc/common.h  taps_clamp   fl_y / fl_x = fminf(fmaxf(0, floorf(q)), size - 2) before `(int)`; y1 = y0 + 1 <= size - 1
                              (qpwc_warp_fwd and the fused entry points refuse H < 2 or W < 2 in this mode)
  csrc/common.h  taps_tfwarp  x0, x1, y0, y1 = clampi(.., 0, size - 1) after `(int)` and the INT32_MAX guard
  csrc/warp.hip               both kernels address img with t.y0, t.y1, t.x0, t.x1 of make_taps only; the output index
                              and the flow index come from the thread index
  csrc/occlusion.hip          FlowField::at(b, t.y0 / t.y1, t.x0 / t.x1) from taps_tfwarp; ti, tj = clampi((int)(..), 0,
                              size - 1); the second f.at(b, ti, tj) and the store out[(b * H + ti) * W + tj] use those
These are value tests on inputs that training and data files produce, not memory probes.

Departures found in the CPU chains when this file was written, all brought to the rule (DESIGN.md lists them):
  oracle.np_ref.tf_warp / estimate_occlusion_map  `astype(np.int32)` of NaN, +Inf and values >= 2^31 gives INT32_MIN on
        x86 (the first column, not the last), and whatever the platform gives elsewhere;
  oracle.np_ref.interpolate_bilinear               np.maximum / np.minimum propagate NaN into `astype(np.int32)`: an index
        of INT32_MIN, an IndexError; the kernel's fmaxf / fminf give corner 0, alpha 0;
  oracle.torch_ref.tf_warp / _interpolate_bilinear the same two, through `.to(torch.int32)` and torch.clamp;
  oracle/c/qpwc_oracle.c oracle_warp               `(int)xf` of an out-of-range float is undefined behaviour in C.
tests/test_gpu_nonfinite_flow.py holds the kernels to the same restatement on the same fixtures.

Mutation, on paper: `x0 == INT32_MAX ? x0 : x0 + 1` to `x0 + 1` in the restatement's taps_tfwarp makes the second corner
of a flow of 2147483648 wrap to INT32_MIN and clamp to column 0 instead of W - 1: the weights -A and +A then meet two
different pixels and the output is their difference times 2^31 instead of rounding noise --
test_the_guard_is_visible asserts that the two readings differ on the fixture."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import np_ref  # noqa: E402

F = np.float32
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
SHAPE = (2, 9, 14)                                    # B, H, W


# ---- the rule --------------------------------------------------------------------------------------------------------
def sat_trunc(v):
    """float32 -> int as v_cvt_i32_f32 converts: toward zero, saturating, NaN -> 0."""
    v = F(v)
    if v != v:
        return 0
    if v >= F(2147483648.0):
        return INT32_MAX
    if v <= F(-2147483648.0):
        return INT32_MIN
    return int(v)                                     # Python's int() truncates toward zero


def clampi(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def fmaxf(a, b):
    """C's fmaxf: the other operand for a NaN."""
    a, b = F(a), F(b)
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def fminf(a, b):
    a, b = F(a), F(b)
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def taps_tfwarp(y, x, fx, fy, H, W, guard=True):
    """-> ((y0, y1, x0, x1), (w00, w01, w10, w11)); guard=False: the reading without the INT32_MAX guard, as 32-bit
    arithmetic would wrap it."""
    xf, yf = F(x) + F(fx), F(y) + F(fy)
    x0, y0 = sat_trunc(xf), sat_trunc(yf)

    def second(c):
        if c == INT32_MAX:
            return c if guard else INT32_MIN
        return c + 1
    x1, y1 = second(x0), second(y0)
    x0, x1, y0, y1 = clampi(x0, 0, W - 1), clampi(x1, 0, W - 1), clampi(y0, 0, H - 1), clampi(y1, 0, H - 1)
    x0f, x1f, y0f, y1f = F(x0), F(x1), F(y0), F(y1)
    return (y0, y1, x0, x1), ((x1f - xf) * (y1f - yf), (xf - x0f) * (y1f - yf), (x1f - xf) * (yf - y0f), (xf - x0f) * (yf - y0f))


def blend_tfwarp(w, tl, tr, bl, br):
    w00, w01, w10, w11 = w
    return ((w00 * F(tl) + w10 * F(bl)) + w01 * F(tr)) + w11 * F(br)


def taps_clamp(y, x, fx, fy, H, W):
    """-> ((y0, y1, x0, x1), (ay, ax))"""
    qy, qx = F(y) - (-F(fy)), F(x) - (-F(fx))
    fl_y = fminf(fmaxf(F(0), np.floor(qy)), F(H - 2))
    fl_x = fminf(fmaxf(F(0), np.floor(qx)), F(W - 2))
    y0, x0 = int(fl_y), int(fl_x)
    return (y0, y0 + 1, x0, x0 + 1), (fminf(fmaxf(F(0), qy - fl_y), F(1)), fminf(fmaxf(F(0), qx - fl_x), F(1)))


def blend_clamp(a, tl, tr, bl, br):
    ay, ax = a
    tl, tr, bl, br = F(tl), F(tr), F(bl), F(br)
    top = ax * (tr - tl) + tl
    bot = ax * (br - bl) + bl
    return ay * (bot - top) + top


def ref_warp(img, flo, mode, guard=True):
    """Warp (mode 'tfwarp') / WarpV2 ('clamp') of img (B,H,W,C) under flo (B,H,W,2), float32, pixel by pixel."""
    B, H, W, C = img.shape
    out = np.empty((B, H, W, C), F)
    with np.errstate(all="ignore"):
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    fx, fy = flo[b, y, x]
                    if mode == "tfwarp":
                        (y0, y1, x0, x1), w = taps_tfwarp(y, x, fx, fy, H, W, guard)
                        mix = blend_tfwarp
                    else:
                        (y0, y1, x0, x1), w = taps_clamp(y, x, fx, fy, H, W)
                        mix = blend_clamp
                    assert min(y0, y1, x0, x1) >= 0 and max(y0, y1) < H and max(x0, x1) < W
                    for c in range(C):
                        out[b, y, x, c] = mix(w, img[b, y0, x0, c], img[b, y0, x1, c], img[b, y1, x0, c], img[b, y1, x1, c])
    return out


def ref_invert_flow(flo, guard=True):
    """-> (-tf_warp(flo, flo) float32 (B,H,W,2), reads (B,H,W,4,2): the (y, x) of the four flow pixels each one read)."""
    B, H, W, _ = flo.shape
    out, reads = np.empty((B, H, W, 2), F), np.empty((B, H, W, 4, 2), np.int64)
    with np.errstate(all="ignore"):
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    (y0, y1, x0, x1), w = taps_tfwarp(y, x, flo[b, y, x, 0], flo[b, y, x, 1], H, W, guard)
                    reads[b, y, x] = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
                    for c in range(2):
                        out[b, y, x, c] = -blend_tfwarp(w, flo[b, y0, x0, c], flo[b, y0, x1, c], flo[b, y1, x0, c], flo[b, y1, x1, c])
    return out, reads


def ref_occlusion(flo):
    """estimate_occlusion_map as occlusion_scatter_kernel computes it: every pixel writes the out-of-bounds test of its
    clamped, saturating target to that target; a pixel no one writes keeps 1."""
    B, H, W, _ = flo.shape
    inv, _ = ref_invert_flow(flo)
    out = np.ones((B, H, W), F)
    with np.errstate(all="ignore"):
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    ti = clampi(sat_trunc(F(y) + inv[b, y, x, 1]), 0, H - 1)
                    tj = clampi(sat_trunc(F(x) + inv[b, y, x, 0]), 0, W - 1)
                    i2, j2 = F(ti) + flo[b, ti, tj, 1], F(tj) + flo[b, ti, tj, 0]
                    oob = bool(i2 < 0) or bool(i2 >= H) or bool(j2 < 0) or bool(j2 >= W)      # a NaN compares false
                    out[b, ti, tj] = 1.0 if oob else 0.0
    return out


# ---- the fixtures (shared with tests/test_gpu_nonfinite_flow.py) -----------------------------------------------------
NAN, INF = float("nan"), float("inf")
PLANT_F32 = [(0, NAN), (1, NAN), (0, INF), (1, -INF), (0, -INF), (1, INF), (0, 3e9), (1, -3e9), (0, -3e9), (1, 3e9),
             (0, 2147483648.0), (1, -2147483648.0), (0, -2147483648.0), (1, 2147483648.0), (0, 2147483520.0),
             (1, 2147483520.0), (0, 1e10), (1, 1e10), (0, "last"), (0, "size"), (0, "-1"), (1, "last"), (1, "size"), (1, "-1")]
PLANT_F16 = [(0, NAN), (1, NAN), (0, INF), (1, -INF), (0, -INF), (1, INF), (0, 65504.0), (1, -65504.0), (0, -65504.0),
             (1, 65504.0), (0, "last"), (0, "size"), (0, "-1"), (1, "last"), (1, "size"), (1, "-1")]
PLACES = [(b, y, x) for b in range(2) for y in (1, 4, 7) for x in (1, 5, 9, 12)]     # 3 rows, 3 to 4 columns apart
_FIXTURES = {}


def fixture(half):
    """(img (B,H,W,8) float32, clean flow, planted flow, planted (B,H,W) bool), computed once; fp16 storage: every
    value is an fp16 number.  The base flow is smooth and within 0.75 px: a clean pixel reads flows within 2 pixels."""
    if half not in _FIXTURES:
        B, H, W = SHAPE
        rng = np.random.default_rng(17)
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        flo = np.empty((B, H, W, 2), np.float64)
        for b in range(B):
            flo[b, ..., 0] = 0.75 * np.sin(2 * np.pi * yy / H + b) * np.cos(2 * np.pi * xx / W)
            flo[b, ..., 1] = 0.75 * np.cos(2 * np.pi * yy / H) * np.sin(2 * np.pi * xx / W + 0.5 * b)
        img = np.sin(0.7 * yy + 0.3 * xx)[None, ..., None] + 0.25 * rng.standard_normal((B, H, W, 8))
        cast = (lambda a: a.astype(np.float16).astype(F)) if half else (lambda a: a.astype(F))
        img, clean = cast(img), cast(flo)
        planted, mask = clean.copy(), np.zeros((B, H, W), bool)
        plants = PLANT_F16 if half else PLANT_F32
        assert len(plants) <= len(PLACES)
        for (b, y, x), (ch, v) in zip(PLACES, plants):
            if isinstance(v, str):                    # x + fx (or y + fy) lands exactly on size - 1, size or -1
                v = {"last": (W, H)[ch] - 1, "size": (W, H)[ch], "-1": -1}[v] - (x, y)[ch]
            planted[b, y, x, ch] = v
            mask[b, y, x] = True
        assert np.array_equal(cast(planted), planted, equal_nan=True) and np.abs(clean).max() <= 0.75
        _FIXTURES[half] = (img, clean, planted, mask)
    return _FIXTURES[half]


def same(a, b):
    """NaN exactly where the other has NaN, the same bits elsewhere (0 and -0 are told apart)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    ints = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(ints)[~na], b.view(ints)[~nb]))


def where_differs(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.argwhere((na != nb) | (~na & ~nb & (a != b))).tolist()


# ---- the rule's own known answers --------------------------------------------------------------------------------------
def test_sat_trunc_known_answers():
    for v, want in ((NAN, 0), (INF, INT32_MAX), (-INF, INT32_MIN), (3e9, INT32_MAX), (-3e9, INT32_MIN), (1e10, INT32_MAX),
                    (2147483648.0, INT32_MAX), (-2147483648.0, INT32_MIN), (2147483520.0, 2147483520),
                    (-2147483520.0, -2147483520), (2.9, 2), (-2.9, -2), (-0.5, 0), (0.999, 0), (-0.0, 0), (13.0, 13)):
        assert sat_trunc(v) == want, v
    assert fmaxf(0.0, NAN) == 0 and fmaxf(NAN, 2.0) == 2 and fminf(NAN, 1.0) == 1 and fminf(INF, 7.0) == 7


def test_taps_under_the_rule():
    H, W = 9, 14
    # tfwarp: NaN -> corners (0, 1); +huge -> the last column twice; -huge -> the first twice; exact landings
    for fx, want in ((NAN, (0, 1)), (INF, (W - 1, W - 1)), (-INF, (0, 0)), (3e9, (W - 1, W - 1)), (-3e9, (0, 0)),
                     (2147483648.0, (W - 1, W - 1)), (2147483520.0, (W - 1, W - 1)), (1e10, (W - 1, W - 1)),
                     (W - 1 - 5, (W - 1, W - 1)), (W - 5, (W - 1, W - 1)), (-1 - 5, (0, 0)), (-5.5, (0, 1)), (0.25, (5, 6))):
        with np.errstate(all="ignore"):
            (y0, y1, x0, x1), w = taps_tfwarp(4, 5, fx, 0.0, H, W)
        assert (x0, x1) == want and (y0, y1) == (4, 5), fx
    with np.errstate(all="ignore"):
        assert taps_tfwarp(4, 5, 2147483648.0, 0.0, H, W, guard=False)[0][2:] == (W - 1, 0)      # what the guard prevents
        # clamp: a NaN coordinate -> corner 0, alpha 0; +Inf -> the last pair, alpha 1; -Inf -> corner 0, alpha 0
        for fy, want in ((NAN, (0, 1, 0.0)), (INF, (H - 2, H - 1, 1.0)), (-INF, (0, 1, 0.0)), (1e10, (H - 2, H - 1, 1.0)),
                         (-3e9, (0, 1, 0.0)), (H - 1 - 4, (H - 2, H - 1, 1.0)), (0.5, (4, 5, 0.5))):
            (y0, y1, x0, x1), (ay, ax) = taps_clamp(4, 5, 0.0, fy, H, W)
            assert (y0, y1, float(ay)) == want and (x0, x1, float(ax)) == (5, 6, 0.0), fy


def test_the_guard_is_visible():
    """Without the INT32_MAX guard the planted flows of 2147483648 read column 0 beside column W - 1: Warp and the
    inverse flow change there, so the equality of the other tests catches a missing guard."""
    img, clean, planted, mask = fixture(False)
    assert not same(ref_warp(img, planted, "tfwarp"), ref_warp(img, planted, "tfwarp", guard=False))
    assert not same(ref_invert_flow(planted)[0], ref_invert_flow(planted, guard=False)[0])


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_fixture_plants_what_it_says(half):
    img, clean, planted, mask = fixture(half)
    plants = PLANT_F16 if half else PLANT_F32
    assert mask.sum() == len(plants) and np.isfinite(clean).all() and np.isfinite(img).all()
    assert np.array_equal(planted[~mask], clean[~mask])
    assert np.isnan(planted).sum() == 2 and np.isinf(planted).sum() == 4
    assert (np.abs(planted[np.isfinite(planted)]) >= (65504.0 if half else 2147483520.0)).sum() == (4 if half else 12)
    B, H, W = SHAPE
    xs = np.arange(W)[None, None, :] + planted[..., 0]
    ys = np.arange(H)[None, :, None] + planted[..., 1]
    for v, grid in ((W - 1, xs), (W, xs), (-1, xs), (H - 1, ys), (H, ys), (-1, ys)):
        assert (grid[mask] == v).sum() >= 1, v
    # planted pixels are further apart than a clean pixel reads: no clean pixel depends on two of them
    _, reads = ref_invert_flow(clean)
    hits = np.zeros(SHAPE, int)
    for b, y, x in np.argwhere(~mask):
        hits[b, y, x] = sum(mask[b, ty, tx] for ty, tx in reads[b, y, x])
    assert hits.max() == 1 or hits.max() == 2 and all(len({tuple(t) for t in reads[b, y, x] if mask[b, t[0], t[1]]}) == 1
                                                      for b, y, x in np.argwhere(hits == 2))


# ---- the CPU chains against the rule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["tfwarp", "clamp"])
def test_np_ref_warp_follows_the_rule(mode):
    img, clean, planted, mask = fixture(False)
    fn = np_ref.tf_warp if mode == "tfwarp" else np_ref.warp_v2
    with np.errstate(all="ignore"):
        for flo in (clean, planted):
            got, want = fn(img, flo), ref_warp(img, flo, mode)
            assert same(got, want), where_differs(got, want)[:5]
            nchw = fn(np.ascontiguousarray(np.moveaxis(img, 3, 1)), np.ascontiguousarray(np.moveaxis(flo, 3, 1)), "channels_first")
            assert same(np.moveaxis(nchw, 1, 3), want)
    # Warp turns a non-finite flow into NaN at its own pixel; WarpV2 clamps it to a border sample and stays finite
    assert np.isfinite(want[~mask]).all() and np.isnan(want[mask]).any() == (mode == "tfwarp")


def test_np_ref_occlusion_follows_the_rule():
    for half in (False, True):
        img, clean, planted, mask = fixture(half)
        with np.errstate(all="ignore"):
            for flo in (clean, planted):
                inv, _ = ref_invert_flow(flo)
                got = np_ref.invert_flow(flo)
                assert same(got, inv), where_differs(got, inv)[:5]
                occ = ref_occlusion(flo)
                assert np.array_equal(np_ref.estimate_occlusion_map(flo), occ)
                nchw = np.ascontiguousarray(np.moveaxis(flo, 3, 1))
                assert np.array_equal(np_ref.estimate_occlusion_map(nchw, "channels_first"), occ)
        assert set(np.unique(occ)) == {0.0, 1.0}


@pytest.mark.parametrize("mode", ["tfwarp", "clamp"])
def test_torch_ref_warp_follows_the_rule(mode):
    import torch
    from oracle import torch_ref
    img, clean, planted, mask = fixture(False)
    fn = torch_ref.tf_warp if mode == "tfwarp" else torch_ref.warp_v2
    for flo in (clean, planted):
        got, want = fn(torch.from_numpy(img), torch.from_numpy(flo)).numpy(), ref_warp(img, flo, mode)
        assert same(got, want), where_differs(got, want)[:5]


@pytest.mark.parametrize("mode", ["tfwarp", "clamp"])
def test_c_oracle_warp_follows_the_rule(mode, c_oracle):
    img, clean, planted, mask = fixture(False)
    for flo in (clean, planted):
        want = ref_warp(img, flo, mode)
        got = c_oracle.warp(img, flo, "channels_last", mode)
        assert same(got, want), where_differs(got, want)[:5]
        nchw = c_oracle.warp(np.ascontiguousarray(np.moveaxis(img, 3, 1)), np.ascontiguousarray(np.moveaxis(flo, 3, 1)),
                             "channels_first", mode)
        assert same(np.moveaxis(nchw, 1, 3), want)


def test_the_device_ops_have_no_cpu_path():
    """qpwcnet_amd.warp and qpwcnet_amd.occlusion run on a HIP device only: a CPU tensor is refused by name, there is no
    second implementation that could depart from the rule."""
    import torch
    from qpwcnet_amd import occlusion, warp
    img, clean, planted, mask = fixture(False)
    for call in (lambda: warp.tf_warp(torch.from_numpy(img), torch.from_numpy(planted), "channels_last"),
                 lambda: occlusion.invert_flow(torch.from_numpy(planted), "channels_last"),
                 lambda: occlusion.estimate_occlusion_map(torch.from_numpy(planted), "channels_last")):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()

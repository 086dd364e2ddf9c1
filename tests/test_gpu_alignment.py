"""GPU suite of the forms that only operands off the 16-byte grid reach.

About twenty launchers in qpwcnet_amd/csrc look at the low bits of a pointer and pick between a vector form and an
element-wise one (tests/test_alignment_cpu.py lists the sites and holds the list to the sources).  The C boundary promises
element alignment only, and a dense slice of a larger buffer (`flat[1:1 + n].view(shape)`) is contiguous and 4 bytes off
the grid, so the element-wise forms are reachable from ordinary torch code.  Every case here hands one of them such an
operand, made by `off_grid`: at least 16 bytes of slack on both sides, NaN (0xFF for uint8) around an input, so that a
load in front of the base or past the end poisons the result, and a sentinel around an output that must still be there
afterwards.  A fallback that rounds its address down, keeps a vector store, or reads four elements where one is left
fails here.

Oracles and bounds are the ones the neighbouring files already use for the same operation (named case by case); where
two forms run the same expressions and those files already assert bit equality between them, the off-grid call must also
give the bits of the aligned call.  Data are seeded random values.  Shapes are the smallest that still reach the form."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_optim_cpu import (CASES as OPT_CASES, CLIP, STEPS, assert_within_bounds, errors, make_optimizer,  # noqa: E402
                            set_grads, trajectory)
from test_vis_cpu import BOUND, ref_flow_to_image, ref_nearest, random_flow, to_layout  # noqa: E402

from oracle import c_ref, net_ref, torch_ref  # noqa: E402
from qpwcnet_amd import _hip, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4                      # tests/test_gpu_parity.py: "within 1e-4 fp32 on identical inputs"
F16_EPS = 2.0 ** -11            # ... and its fp16 rule: TOL + 2^-11 |ref|
SENTINEL = {torch.float32: -1234.0, torch.float16: -1234.0, torch.uint8: 0xA5}
MODES = {"clamp": _hip.WARP_CLAMP, "tfwarp": _hip.WARP_TFWARP}
DTYPES = {"f32": torch.float32, "f16": torch.float16}


@pytest.fixture(scope="module", autouse=True)
def _loaded():
    _hip.lib()
    c_ref.build()


# ---- the helper ------------------------------------------------------------------------------------------------------
def off_grid(t, nbytes, sentinel=None):
    """A dense copy of device tensor t that starts nbytes past a 16-byte boundary, with 16 + nbytes bytes of slack in
    front of it and 32 behind.  The slack holds NaN (0xFF bytes for uint8) for an input; for an output pass its dtype's
    SENTINEL, and `guards_intact` says afterwards whether every slack element still holds it."""
    es = t.element_size()
    assert 0 < nbytes < 16 and nbytes % es == 0, (nbytes, es)
    lead, n = (16 + nbytes) // es, t.numel()
    fill = sentinel if sentinel is not None else (0xFF if t.dtype == torch.uint8 else float("nan"))
    buf = torch.full((lead + n + 32 // es,), fill, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[lead:lead + n].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == nbytes and lead * es >= 16
    v._guard = (buf, lead, n, fill)
    return v


def off_grid_out(shape, dtype, nbytes):
    """An output for off_grid: NaN (uint8: 0) where the call must write, the dtype's sentinel around it."""
    blank = torch.full(shape, 0 if dtype == torch.uint8 else float("nan"), dtype=dtype, device=DEV)
    return off_grid(blank, nbytes, SENTINEL[dtype])


def guards_intact(v):
    buf, lead, n, fill = v._guard
    g = torch.cat([buf[:lead], buf[lead + n:]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def one_early(v):
    """The tensor a load that starts one element in front of v's base would see (negative controls)."""
    buf, lead, n, _ = v._guard
    return buf[lead - 1:lead - 1 + n].view(v.shape)


def test_off_grid_helper():
    for dtype, nbytes in ((torch.float32, 4), (torch.float32, 12), (torch.float16, 2), (torch.float16, 8),
                          (torch.uint8, 1)):
        t = torch.arange(24, device=DEV).reshape(2, 3, 4).to(dtype)
        v = off_grid(t, nbytes)
        assert torch.equal(v, t) and v.data_ptr() % 16 == nbytes and guards_intact(v)
        o = off_grid_out((2, 3, 4), dtype, nbytes)
        assert guards_intact(o)
        o._guard[0][o._guard[1] + 24] = 1            # the element behind the view
        assert not guards_intact(o)
        o = off_grid_out((2, 3, 4), dtype, nbytes)
        o._guard[0][o._guard[1] - 1] = 1             # ... and the one in front of it
        assert not guards_intact(o)
        assert torch.equal(one_early(v).reshape(-1)[1:], t.reshape(-1)[:-1])


def _np(t):
    return t.detach().float().cpu().numpy()


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _nanmax(a):
    return float(np.nanmax(np.abs(a)))


# ---- warp forward ----------------------------------------------------------------------------------------------------
_WARP = {}


def _warp_case(dtype, C):
    """(img, flo, {mode: c_ref result}) for B=2, H=5, W=7: flows N(0, 3^2) cross every border.  Computed once."""
    if (dtype, C) not in _WARP:
        rng = np.random.default_rng(100 + C)
        img = rng.standard_normal((2, 5, 7, C)).astype(np.float32)
        flo = (rng.standard_normal((2, 5, 7, 2)) * 3).astype(np.float32)
        img_t = torch.from_numpy(img).to(DEV, dtype)
        img32 = _np(img_t)                              # the fp16-rounded values for fp16
        refs = {m: c_ref.warp(img32, flo, mode=m) for m in MODES}
        for r in refs.values():
            r.setflags(write=False)
        _WARP[dtype, C] = (img_t, torch.from_numpy(flo).to(DEV), refs)
    return _WARP[dtype, C]


def _warp_c(img, flo, out, mode):
    B, H, W, C = img.shape
    _hip.check(_hip.lib().qpwc_warp_fwd(img.data_ptr(), flo.data_ptr(), out.data_ptr(), B, H, W, C, 0, _hip.NHWC,
                                        ops._DTYPES[img.dtype], MODES[mode], ops._stream(img)))


@pytest.mark.parametrize("place", ["img", "out", "both"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("C", [4, 8])
@pytest.mark.parametrize("dt,off", [("f32", 4), ("f16", 2), ("f16", 8)])
def test_warp_forward_off_grid(dt, off, C, mode, place):
    """warp_impl with img and / or out off the grid at C % 4 == 0: warp_generic_kernel<NHWC> instead of the 16- / 8-byte
    gather kernels (fp16 8 bytes off would suit the 8-byte kernel, but `fast` asks for 16).  fp32 equals c_ref.warp
    exactly (test_randomised_shapes_every_kernel_path), fp16 stays within rtol = atol = 1e-3 (test_fp16_storage_path),
    and both give the bits of the aligned call.  Measured on an MI355X: fp32 exact, fp16 max |err| 1.2e-3
    (inside 1e-3 + 1e-3 |ref| at every element)."""
    img, flo, refs = _warp_case(DTYPES[dt], C)
    aligned = _nan_like(img)
    _warp_c(img, flo, aligned, mode)
    src = off_grid(img, off) if place in ("img", "both") else img
    dst = off_grid_out(img.shape, img.dtype, off) if place in ("out", "both") else _nan_like(img)
    _warp_c(src, flo, dst, mode)
    torch.cuda.synchronize()
    assert place == "img" or guards_intact(dst)
    assert torch.equal(dst, aligned)
    got, ref = _np(dst), refs[mode]
    print("warp {} +{} C={} {} {}: max |err| {:.3e}".format(dt, off, C, mode, place, float(np.abs(got - ref).max())))
    if dt == "f32":
        np.testing.assert_array_equal(got, ref)
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-3)


def test_warp_channels_first_off_grid_image():
    """ops.warp in channels_first with an off-grid (B,4,H,W) image: the wrapper's transpose (layout_transpose, element
    loads) takes it as it is and the channels-last gather kernel runs on the aligned copy: equal to the aligned call and to
    c_ref.warp (on an MI355X: both exact)."""
    img, flo, refs = _warp_case(torch.float32, 4)
    img_cf, flo_cf = img.permute(0, 3, 1, 2).contiguous(), flo.permute(0, 3, 1, 2).contiguous()
    for mode in MODES:
        aligned = ops.warp(img_cf, flo_cf, mode, "channels_first")
        got = ops.warp(off_grid(img_cf, 4), flo_cf, mode, "channels_first")
        assert torch.equal(got, aligned)
        np.testing.assert_array_equal(_np(got.permute(0, 2, 3, 1)), refs[mode])


def test_warp_negative_control():
    """The comparison of test_warp_forward_off_grid tells a load one element early apart: c_ref.warp of the buffer read
    from one float in front of the base differs from the kernel's result by more than 1000 x the project's fp32 bound
    (the case itself allows no difference at all).  Measured: 3.4."""
    img, flo, refs = _warp_case(torch.float32, 4)
    src = off_grid(img, 4)
    dst = off_grid_out(img.shape, img.dtype, 4)
    _warp_c(src, flo, dst, "clamp")
    early = c_ref.warp(_np(one_early(src)), _np(flo), mode="clamp")
    d = _nanmax(_np(dst) - early)
    print("warp negative control: {:.3e}".format(d))
    assert d > 1000 * TOL


# ---- cost volume forward ---------------------------------------------------------------------------------------------
_CV = {}


def _cv_case(shape, dtype, seed=7):
    """(prv, nxt, c_ref.cost_volume of the values the device holds), computed once per shape and dtype."""
    if (shape, dtype) not in _CV:
        rng = np.random.default_rng(seed + shape[3] + shape[1])
        prv, nxt = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV, dtype) for _ in range(2))
        ref = c_ref.cost_volume(_np(prv), _np(nxt))
        ref.setflags(write=False)
        _CV[shape, dtype] = (prv, nxt, ref)
    return _CV[shape, dtype]


def _cv_check(got, ref, dtype, what):
    err = np.abs(_np(got) - ref)
    print("cost volume {}: max |err| {:.3e}".format(what, float(err.max())))
    tol = TOL if dtype == torch.float32 else TOL + F16_EPS * np.abs(ref)
    assert np.all(err <= tol), (what, float((err - tol).max()))


@pytest.mark.parametrize("place", ["prv", "nxt", "both"])
@pytest.mark.parametrize("C", [4, 16, 32])
@pytest.mark.parametrize("dt,off", [("f32", 4), ("f16", 2)])
def test_cost_volume_inputs_off_grid(dt, off, C, place):
    """ops.cost_volume with prv and / or nxt off the grid, (2, 9, 11, C): cost_volume_generic_kernel, at C = 16 and 32
    behind the matrix-core launcher's own refusal (cost_volume_mfma_launch returns 1), at C = 4 behind `fast` of
    cost_volume_impl.  Against c_ref.cost_volume at TOL (fp16: TOL + 2^-11 |ref|).  Measured on an MI355X: fp32 max
    |err| 2.4e-7, fp16 9.5e-4 (inside TOL + 2^-11 |ref| at every element)."""
    prv, nxt, ref = _cv_case((2, 9, 11, C), DTYPES[dt])
    p = off_grid(prv, off) if place in ("prv", "both") else prv
    n = off_grid(nxt, off) if place in ("nxt", "both") else nxt
    _cv_check(ops.cost_volume(p, n), ref, DTYPES[dt], "{} +{} C={} {}".format(dt, off, C, place))


@pytest.mark.parametrize("place", ["prv", "nxt", "both"])
@pytest.mark.parametrize("dt,off", [("f32", 4), ("f16", 2)])
def test_cost_volume_channels_first_inputs_off_grid(dt, off, place):
    """The same in channels_first at C = 16: the wrapper transposes the off-grid (B,16,H,W) operands (element loads) into
    aligned channels-last copies: equal to the aligned call, and c_ref within the bound.  Measured on an MI355X: fp32 max
    |err| 1.2e-7, fp16 4.9e-4."""
    prv, nxt, ref = _cv_case((2, 9, 11, 16), DTYPES[dt])
    pc, nc = prv.permute(0, 3, 1, 2).contiguous(), nxt.permute(0, 3, 1, 2).contiguous()
    aligned = ops.cost_volume(pc, nc, 4, "channels_first")
    p = off_grid(pc, off) if place in ("prv", "both") else pc
    n = off_grid(nc, off) if place in ("nxt", "both") else nc
    got = ops.cost_volume(p, n, 4, "channels_first")
    assert torch.equal(got, aligned)
    _cv_check(got.permute(0, 2, 3, 1), ref, DTYPES[dt], "channels_first {} {}".format(dt, place))


def _cv_c(prv, nxt, out):
    B, H, W, C = prv.shape
    _hip.check(_hip.lib().qpwc_cost_volume_fwd(prv.data_ptr(), nxt.data_ptr(), out.data_ptr(), B, H, W, C, 4, _hip.NHWC,
                                               ops._DTYPES[prv.dtype], 0.1, ops._stream(prv)))


@pytest.mark.parametrize("shape,dt,off,kernel", [
    ((2, 8, 16, 32), "f32", 4, "cost_volume_mfma_kernel"), ((2, 8, 16, 16), "f32", 4, "cost_volume_mfma_kernel"),
    ((2, 8, 16, 32), "f16", 2, "cost_volume_mfma_kernel"), ((2, 8, 16, 32), "f16", 4, "cost_volume_mfma_kernel"),
    ((2, 8, 16, 16), "f16", 2, "cost_volume_mfma_kernel"), ((2, 8, 16, 16), "f16", 4, "cost_volume_mfma_kernel"),
    ((4, 64, 64, 32), "f16", 2, "cost_volume_mfma_lds_f16_kernel")])
def test_cost_volume_output_off_grid(shape, dt, off, kernel):
    """qpwc_cost_volume_fwd with only `out` off the grid (as test_cost_volume_output_only_element_aligned, which covers
    the fp32 workgroup-shared kernel): the scalar epilogue of the per-wave matrix-core kernels (store_tile_impl, 32 and 16
    channels: 8 and 4 channels per lane) in both dtypes, and of the fp16 workgroup-shared kernel at its smallest shape
    (256 regions of 8 x 8).  c_ref within the bound, the bits of the aligned call, guards intact.  Measured on an
    MI355X: fp32 max |err| 2.4e-7, fp16 3.6e-4."""
    dtype = DTYPES[dt]
    assert ops.cost_volume_kernel(*shape, dtype=dtype) == kernel
    prv, nxt, ref = _cv_case(shape, dtype)
    out = off_grid_out(shape[:3] + (81,), dtype, off)
    _cv_c(prv, nxt, out)
    torch.cuda.synchronize()
    assert guards_intact(out)
    assert torch.equal(out, ops.cost_volume(prv, nxt))
    _cv_check(out, ref, dtype, "{} out +{} {}".format(kernel, off, shape))


@pytest.mark.parametrize("dt,off", [("f32", 4), ("f16", 2), ("f16", 8)])
@pytest.mark.parametrize("shape", [(4, 64, 64, 32), (2, 8, 16, 32), (1, 12, 20, 8)])
def test_cost_volume_84_channel_padded_output_off_grid(shape, dt, off):
    """ops.cost_volume_into(prv, nxt, buf, 0) with buf an off-grid (B, H, W, 84) view full of NaN: no kernel writes the
    pads itself then (the workgroup-shared kernels report pads_written = false, the per-wave and tiled ones never do),
    so zero_pads_kernel runs beside the scalar epilogue.  fp16 at 8 mod 16 is the other side of that rule: 8-byte rows
    are enough for the fp16 kernels' dense epilogue, which then writes the pads itself.  Channels 0..80 equal the dense result
    (test_cost_volume_84_channel_padded_layout), 81..83 are exactly 0, the guards are intact (on an MI355X: all exact)."""
    dtype = DTYPES[dt]
    prv, nxt, _ = _cv_case(shape, dtype)
    buf = off_grid_out(shape[:3] + (84,), dtype, off)
    ops.cost_volume_into(prv, nxt, buf, 0)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    assert torch.equal(buf[..., :81], ops.cost_volume(prv, nxt))
    assert float(buf[..., 81:].abs().max()) == 0.0


def test_cost_volume_negative_control():
    """c_ref.cost_volume of prv read one float early against the kernel's result for the off-grid prv: more than 1000 x
    TOL apart.  Measured: 3.1."""
    prv, nxt, ref = _cv_case((2, 9, 11, 4), torch.float32)
    p = off_grid(prv, 4)
    got = _np(ops.cost_volume(p, nxt))
    d = _nanmax(got - c_ref.cost_volume(_np(one_early(p)), _np(nxt)))
    print("cost volume negative control: {:.3e}".format(d))
    assert d > 1000 * TOL


# ---- fused warp + cost volume ----------------------------------------------------------------------------------------
def test_fused_front_end_flow_off_grid():
    """qpwc_warp_cost_volume_fwd at (4, 64, 64, 32) fp32 with flo 4 bytes off (4 mod 8): the matrix-core launcher returns
    1 for it and cost_volume_tiled_kernel<fused> runs instead of cost_volume_mfma_lds_kernel<true>.  Within TOL of the
    aligned call and of c_ref on images 0 and B - 1 (test_fused_front_end_on_the_matrix_cores...).  Measured on an
    MI355X: 1.8e-7 against the aligned call, 1.8e-7 against c_ref."""
    shape = (4, 64, 64, 32)
    assert ops.cost_volume_kernel(*shape, fused=True) == "cost_volume_mfma_lds_kernel<true>"
    prv, nxt, _ = _cv_case(shape, torch.float32)
    g = torch.Generator(device=DEV).manual_seed(5)
    flo = torch.randn(4, 64, 64, 2, device=DEV, generator=g) * 3
    aligned = ops.warp_cost_volume(prv, nxt, flo)
    got = ops.warp_cost_volume(prv, nxt, off_grid(flo, 4))
    d = float((got - aligned).abs().max())
    sub = [0, 3]
    ref = c_ref.cost_volume(_np(prv[sub]), c_ref.warp(_np(nxt[sub]), _np(flo[sub])))
    e = float(np.abs(_np(got[sub]) - ref).max())
    print("fused, flo +4: {:.3e} against the aligned call, {:.3e} against c_ref".format(d, e))
    assert d <= TOL and e <= TOL


@pytest.mark.parametrize("which", ["prv", "nxt"])
def test_fused_front_end_refuses_off_grid_images(which):
    """No fused kernel has an element-wise form for prv / nxt: both wrappers raise with the validator's text."""
    prv, nxt, _ = _cv_case((2, 8, 16, 32), torch.float32)
    flo = torch.zeros(2, 8, 16, 2, device=DEV)
    p, n = (off_grid(prv, 4), nxt) if which == "prv" else (prv, off_grid(nxt, 4))
    with pytest.raises(ValueError, match="{} must be 16-byte aligned for the fused".format(which)):
        ops.warp_cost_volume(p, n, flo)
    out = torch.zeros(2, 8, 16, 84, device=DEV)
    with pytest.raises(ValueError, match="{} must be 16-byte aligned for the fused".format(which)):
        ops.cost_volume_into(p, n, out, 0, flo=flo)
    assert float(out.abs().max()) == 0.0


# ---- flow_to_image ---------------------------------------------------------------------------------------------------
VIS_B = 2
VIS_SHAPES = [(15, 25), (5, 7)]
VIS_FLOWS = [random_flow(70 + i, (VIS_B,) + s) for i, s in enumerate(VIS_SHAPES)]


def _vis_c(flows, outs, sizes, out_layout):
    """qpwc_flow_to_image_fwd on channels-last flows into the caller's outputs."""
    L, n = _hip.lib(), len(flows)
    arr = lambda v: (ctypes.c_int * n)(*v)
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    h, w = arr([f.shape[1] for f in flows]), arr([f.shape[2] for f in flows])
    nws = int(L.qpwc_flow_to_image_workspace_floats(n, VIS_B, h, w))
    _hip.check(min(nws, 0))
    ws = torch.empty(nws, dtype=torch.float32, device=DEV)
    u8 = outs[0].dtype == torch.uint8
    _hip.check(L.qpwc_flow_to_image_fwd(ptrs(flows), arr([ops._DTYPES[f.dtype] for f in flows]), h, w, n, VIS_B, _hip.NHWC,
                                        ptrs(outs), arr([s[0] for s in sizes]), arr([s[1] for s in sizes]),
                                        _hip.U8 if u8 else _hip.F32,
                                        _hip.NHWC if out_layout == "channels_last" else _hip.NCHW, ws.data_ptr(),
                                        ops._stream(flows[0])))
    torch.cuda.synchronize()


@pytest.mark.parametrize("size", [None, (20, 25)], ids=["native", "20x25"])
@pytest.mark.parametrize("dt,off", [("f32", 4), ("f16", 2)])
def test_flow_to_image_flows_off_grid(dt, off, size):
    """Channels-last flows (2, 15, 25, 2) and (2, 5, 7, 2) with fp32 at 4 mod 8 / fp16 at 2 mod 4: `pair == 0`, the two
    element loads of vis_load in both launches (maximum and colour) instead of one 8- / 4-byte load.  The bits of the
    aligned call, and ref_flow_to_image (ref_nearest) within BOUND.  Measured on an MI355X: max |err| 4.8e-7 (fp32), 3.4e-7 (fp16)."""
    ts = [torch.from_numpy(f).to(DEV, DTYPES[dt]) for f in VIS_FLOWS]
    sizes = None if size is None else [size] * len(ts)
    aligned = ops.flow_to_image(ts, sizes)
    got = ops.flow_to_image([off_grid(t, off) for t in ts], sizes)
    for a, g, t in zip(aligned, got, ts):
        assert torch.equal(g, a)
        ref = ref_flow_to_image(_np(t))
        ref = ref if size is None else ref_nearest(ref, size)
        e = float(np.abs(_np(g) - ref).max())
        print("flow_to_image flows {} +{} {}: max |err| {:.3e}".format(dt, off, size, e))
        assert e <= BOUND


@pytest.mark.parametrize("which", ["all", "level 1"])
@pytest.mark.parametrize("out_layout", ["channels_last", "channels_first"])
@pytest.mark.parametrize("dtype,off", [(torch.float32, 4), (torch.uint8, 1)], ids=["f32", "u8"])
def test_flow_to_image_outputs_off_grid(dtype, off, out_layout, which):
    """qpwc_flow_to_image_fwd with 20 x 25 pictures (a multiple of 4 pixels) whose outputs -- all of them, or level 1's
    alone -- are off the grid: one such output forces flow_to_image_kernel<scalar> on the whole call, the form query
    says so, and the pictures have the bits of the <vec4> call (test_two_calls_are_bitwise_equal); guards intact (on an MI355X: bit-equal in all 8 cases)."""
    ts = [torch.from_numpy(f).to(DEV) for f in VIS_FLOWS]
    sizes = [(20, 25)] * 2
    shape = (VIS_B, 20, 25, 3) if out_layout == "channels_last" else (VIS_B, 3, 20, 25)
    vec = ops.flow_to_image(ts, sizes, "channels_last", dtype, out_layout)
    assert ops.flow_to_image_kernel(VIS_B, sizes, dtype, out_layout, vec) == "flow_to_image_kernel<vec4>"
    blank = lambda: torch.full(shape, 0 if dtype == torch.uint8 else float("nan"), dtype=dtype, device=DEV)
    outs = [blank() if which == "level 1" else off_grid_out(shape, dtype, off), off_grid_out(shape, dtype, off)]
    assert ops.flow_to_image_kernel(VIS_B, sizes, dtype, out_layout, outs) == "flow_to_image_kernel<scalar>"
    _vis_c(ts, outs, sizes, out_layout)
    assert all(guards_intact(o) for o in outs if hasattr(o, "_guard"))
    assert all(torch.equal(o, v) for o, v in zip(outs, vec))


def test_flow_to_image_wide_and_narrow_pictures():
    """Picture widths 1, 255, 256, 257 and 515 (no existing picture is wider than 128) with 2 to 4 rows: the
    step_y / step_x row walk of the colour kernel with one pixel per row, with a lane's next pixel in the same row
    (widths above 256), exactly one row on (256) and just short of it (255, 257).  Against ref_nearest at BOUND.
    Measured on an MI355X: max |err| 3.8e-7."""
    sizes = [(2, 1), (3, 255), (4, 256), (2, 257), (3, 515)]
    flow = VIS_FLOWS[0]
    ref = ref_flow_to_image(flow)
    t = torch.from_numpy(flow).to(DEV)
    for out_layout in ("channels_last", "channels_first"):
        outs = ops.flow_to_image([t] * len(sizes), sizes, "channels_last", torch.float32, out_layout)
        for o, s in zip(outs, sizes):
            g = to_layout(_np(o), out_layout, "channels_last")
            assert g.shape == (VIS_B,) + s + (3,)
            e = float(np.abs(g - ref_nearest(ref, s)).max())
            print("flow_to_image picture {} {}: max |err| {:.3e}".format(s, out_layout, e))
            assert e <= BOUND


def test_flow_to_image_negative_control():
    """ref_flow_to_image of the flow read one float early (x and y swapped and shifted) against the kernel's picture of
    the off-grid flow: more than 1000 x BOUND apart.  Measured: 1.0."""
    t = off_grid(torch.from_numpy(VIS_FLOWS[0]).to(DEV), 4)
    got = _np(ops.flow_to_image([t])[0])
    early = np.nan_to_num(_np(one_early(t)))
    d = float(np.abs(got - ref_flow_to_image(early)).max())
    print("flow_to_image negative control: {:.3e}".format(d))
    assert d > 1000 * BOUND


# ---- the optimizer step ----------------------------------------------------------------------------------------------
def _carved_optimizer(p0, clip):
    """The `small` parameters carved out of one flat buffer without padding, 16 bytes of sentinel at both ends."""
    names = [n for n, _ in OPT_CASES["small"]]
    total = sum(p0[n].size for n in names)
    flat = torch.full((4 + total + 4,), SENTINEL[torch.float32], device=DEV)
    assert flat.data_ptr() % 16 == 0
    named, o = [], 4
    for n in names:
        v = flat[o:o + p0[n].size].view(p0[n].shape)
        v.copy_(torch.from_numpy(p0[n]))
        named.append((n, torch.nn.Parameter(v)))
        assert named[-1][1].data_ptr() == v.data_ptr()
        o += p0[n].size
    from qpwcnet_amd import optim
    return optim.KerasAdamAGC(named, clip_factor=clip), named, flat


def _optimizer_run(variant, clip):
    p0, grads, after = trajectory("small", clip)
    flat, views = None, []
    if variant == "carved":
        opt, named, flat = _carved_optimizer(p0, clip)
    else:
        opt, named = make_optimizer("small", p0, DEV, clip)
    for k in range(STEPS):
        set_grads(named, grads[k])
        if variant == "grads":
            views = [off_grid(p.grad, 4 * (1 + i % 3)) for i, (_, p) in enumerate(named)]
            for (_, p), v in zip(named, views):
                p.grad = v
        opt.step()
    torch.cuda.synchronize()
    return opt, named, after[STEPS - 1], flat, views


@pytest.mark.parametrize("clip", [None, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("variant", ["carved", "grads"])
def test_optimizer_step_mismatched_phases(variant, clip):
    """agc_adam_kernel's `vec == false` branch (head = len: every element as a scalar) for units whose p, g, m, v do not
    share a phase.  'carved': the parameters of test_optim_cpu's `small` case are views of one flat buffer without
    padding, so f.pointwise.weight starts at float 18443 (phase 12) while its gradient, m and v are on phase 0; 'grads':
    dense parameters, every gradient a view 1, 2 or 3 floats off the grid.  Without clipping there are no sums: p, m and
    v have the bits of the aligned run.  With clipping they stay within P_BOUND / M_BOUND / V_BOUND of the float64 oracle
    after STEPS steps.  Measured on an MI355X: p abs 3.8e-8, m rel 2.3e-7, v rel 3.3e-7."""
    opt, named, ref, flat, views = _optimizer_run(variant, clip)
    if variant == "carved":
        p = dict(named)["f.pointwise.weight"]
        assert (p.data_ptr() - flat.data_ptr()) // 4 - 4 == 18443 and p.data_ptr() % 16 == 12
        assert opt.state[p]["m"].data_ptr() % 16 == 0 and opt.state[p]["v"].data_ptr() % 16 == 0
        assert bool((flat[:4] == SENTINEL[torch.float32]).all()) and bool((flat[-4:] == SENTINEL[torch.float32]).all())
    else:
        assert all(p.grad.data_ptr() == v.data_ptr() and v.data_ptr() % 16 == 4 * (1 + i % 3) and guards_intact(v)
                   for i, ((_, p), v) in enumerate(zip(named, views)))
    assert_within_bounds(errors("small", named, opt, ref), "HIP step, {} clip={}".format(variant, clip))
    if clip is None:
        base, base_named, _, _, _ = _optimizer_run("aligned", clip)
        for (n, a), (_, b) in zip(named, base_named):
            assert torch.equal(a.detach(), b.detach()), n
            assert torch.equal(opt.state[a]["m"], base.state[b]["m"]) and torch.equal(opt.state[a]["v"], base.state[b]["v"]), n


# ---- SeparableConv2D (fp16 storage), depthwise, fp32 SeparableConv2D ------------------------------------------------
def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def _sepconv_f16_ref(srcs, dw, pw, bias):
    """The rounding points of test_sepconv3x3_fused_fp16_storage restated on the oracle's ops."""
    y = torch_ref.depthwise3x3([x.float() for x in srcs], dw, False).half().float()
    return torch.nn.functional.conv2d(y.permute(0, 3, 1, 2), pw.float(), bias).permute(0, 2, 3, 1)


@pytest.mark.parametrize("case", ["tail 2 mod 4", "dw +4", "narrow +8"])
def test_sepconv3x3_fp16_tail_taps_and_narrow_form(case):
    """sepconv3x3_fused_f16_kernel, (2, 19, 37) pixels, F = 16, bound rtol 2e-3 / atol 4e-3 of
    test_sepconv3x3_fused_fp16_storage:
      'tail 2 mod 4': sources (8, 2) with the 2-channel one = wide[..., 1:3] of a (B,H,W,4) tensor, pixel stride 4 and
          pointer 2 mod 4: three element loads per pixel instead of one 4-byte load; channels 0 and 3 of `wide` hold NaN;
      'dw +4': C = 12 (cpad <= 128: all taps staged at once) with dw 4 bytes off: stage_all_taps' scalar staging;
      'narrow +8': one source of 16 channels 8 bytes off: 8-byte loads (`wide` false) where 16-byte ones would run.
    Measured on an MI355X: max |err| 3.9e-3, 7.0e-3 and 3.9e-3, inside 4e-3 + 2e-3 |ref| at every element."""
    rng = np.random.default_rng(len(case))
    B, H, W, F = 2, 19, 37, 16
    if case == "tail 2 mod 4":
        a, wide = _rand(rng, B, H, W, 8).half(), _rand(rng, B, H, W, 4).half()
        srcs = [a, wide[..., 1:3]]
        poisoned = wide.clone()
        poisoned[..., 0] = poisoned[..., 3] = float("nan")
        tail = poisoned.to(DEV)[..., 1:3]
        assert tail.data_ptr() % 4 == 2 and tail.stride(2) == 4
        dsrcs = [a.to(DEV), tail]
    elif case == "dw +4":
        srcs = [_rand(rng, B, H, W, 12).half()]
        dsrcs = [srcs[0].to(DEV)]
    else:
        srcs = [_rand(rng, B, H, W, 16).half()]
        dsrcs = [off_grid(srcs[0].to(DEV), 8)]
    C = sum(s.shape[3] for s in srcs)
    dw = _rand(rng, C, 1, 3, 3)
    pw = (_rand(rng, F, C, 1, 1) / np.sqrt(C)).half()
    bias = _rand(rng, F)
    ref = _sepconv_f16_ref(srcs, dw, pw, bias)
    d_dw = off_grid(dw.reshape(C, 9).to(DEV), 4) if case == "dw +4" else dw.to(DEV)
    out = ops.sepconv3x3(dsrcs, d_dw, ops.pad_pointwise(pw.to(DEV), torch.float16), bias.to(DEV))
    assert out.dtype == torch.float16
    print("sepconv f16 {}: max |err| {:.3e}".format(case, float((out.float().cpu() - ref).abs().max())))
    torch.testing.assert_close(out.float().cpu(), ref, rtol=2e-3, atol=4e-3)


@pytest.mark.parametrize("place", ["source", "out"])
def test_dwconv3x3_fp16_off_grid(place):
    """qpwc_dwconv3x3_fwd in fp16, (2, 12, 20, 32), with the source or the output 4 bytes off (4 mod 8): `vec_ok` false,
    dwconv3x3_kernel<__half> (one channel per lane) instead of dwconv3x3_vec_kernel.  Bound rtol = atol = 2e-3 of
    test_optflow_pieces_fp16_storage.  Measured on an MI355X: max |err| 3.9e-3, inside 2e-3 + 2e-3 |ref| at every element."""
    rng = np.random.default_rng(12)
    B, H, W, C = 2, 12, 20, 32
    x, w = _rand(rng, B, H, W, C).half(), _rand(rng, C, 1, 3, 3)
    ref = torch_ref.depthwise3x3([x.float()], w, False)
    src = off_grid(x.to(DEV), 4) if place == "source" else x.to(DEV)
    out = off_grid_out((B, H, W, C), torch.float16, 4) if place == "out" else _nan_like(src)
    wd = w.reshape(C, 9).to(DEV).contiguous()
    _hip.check(_hip.lib().qpwc_dwconv3x3_fwd((ctypes.c_void_p * 1)(src.data_ptr()), (ctypes.c_int * 1)(C),
                                             (ctypes.c_int64 * 1)(C), 1, 0, wd.data_ptr(), out.data_ptr(), B, H, W,
                                             _hip.F16, ops._stream(src)))
    torch.cuda.synchronize()
    assert place == "source" or guards_intact(out)
    print("dwconv f16 {} +4: max |err| {:.3e}".format(place, float((out.float().cpu() - ref).abs().max())))
    torch.testing.assert_close(out.float().cpu(), ref, rtol=2e-3, atol=2e-3)


def test_sepconv3x3_fp32_first_source_off_grid():
    """ops.sepconv3x3 in fp32 with sources (8, 8), the first one 4 bytes off: `vec` false at C % 4 == 0, the
    element-wise staging of sepconv3x3_fused_kernel.  Bound atol 5e-5 of test_sepconv3x3_fused_short_tail_source.
    Measured on an MI355X: max |err| 1.9e-6."""
    rng = np.random.default_rng(13)
    B, H, W, F = 2, 9, 13, 16
    a, b = _rand(rng, B, H, W, 8), _rand(rng, B, H, W, 8)
    dw, pw, bias = _rand(rng, 16, 1, 3, 3), _rand(rng, F, 16, 1, 1) / 4, _rand(rng, F)
    y = torch_ref.depthwise3x3([a, b], dw, False)
    ref = torch.nn.functional.conv2d(y.permute(0, 3, 1, 2), pw, bias).permute(0, 2, 3, 1)
    out = ops.sepconv3x3([off_grid(a.to(DEV), 4), b.to(DEV)], dw.to(DEV), ops.pad_pointwise(pw.to(DEV)),
                         bias.to(DEV)).cpu()
    print("sepconv f32, first source +4: max |err| {:.3e}".format(float((out - ref).abs().max())))
    torch.testing.assert_close(out, ref, rtol=0, atol=5e-5)


# ---- upsample2x_flow -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (9, 13)])
@pytest.mark.parametrize("dt,off", [("f32", 4), ("f16", 2)])
def test_upsample2x_flow_channels_last_off_grid(dt, off, hw):
    """Channels-last flows (3, h, w, 2) with fp32 at 4 mod 8 / fp16 at 2 mod 4: upsample2x_flow_kernel (one output pixel
    per thread, element loads) on channels-last data instead of the pair kernel; same expressions, so the bits of the
    aligned call (test_upsample2x_flow_pair_kernel_equals_the_pixel_kernel), and the oracle's F.interpolate restatement
    within test_upsample2x_flow's 2e-6 (fp16: test_optflow_pieces_fp16_storage's 2e-3).  Measured on an MI355X: bit-equal;
    against the oracle fp32 max |err| 4.8e-7, fp16 1.9e-3 (inside 2e-3 + 2e-3 |ref| at every element)."""
    rng = np.random.default_rng(hw[0] * 31 + hw[1])
    f = torch.from_numpy(rng.standard_normal((3,) + hw + (2,)).astype(np.float32)).to(DEV, DTYPES[dt])
    aligned = ops.upsample2x_flow(f, 2.0)
    got = ops.upsample2x_flow(off_grid(f, off), 2.0)
    assert torch.equal(got, aligned)
    ref = net_ref.RefNet.upsample(f.float().cpu(), 2.0)
    print("upsample2x_flow {} +{} {}: max |err| {:.3e}".format(dt, off, hw, float((got.float().cpu() - ref).abs().max())))
    if dt == "f32":
        torch.testing.assert_close(got.cpu(), ref, rtol=0, atol=2e-6)
    else:
        torch.testing.assert_close(got.float().cpu(), ref, rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("dt,off", [("f32", 4), ("f32", 8), ("f16", 2), ("f16", 4)])
def test_upsample2x_flow_output_off_grid(dt, off):
    """qpwc_upsample2x_flow_fwd with the (3, 18, 26, 2) output off the 16- (fp32) / 8-byte (fp16) grid of the pair kernel's
    stores: upsample2x_flow_kernel again, element stores.  The bits of the aligned call, guards intact (on an MI355X:
    bit-equal)."""
    rng = np.random.default_rng(off)
    f = torch.from_numpy(rng.standard_normal((3, 9, 13, 2)).astype(np.float32)).to(DEV, DTYPES[dt])
    out = off_grid_out((3, 18, 26, 2), DTYPES[dt], off)
    _hip.check(_hip.lib().qpwc_upsample2x_flow_fwd(f.data_ptr(), out.data_ptr(), 3, 9, 13, 2.0, ops._DTYPES[f.dtype],
                                                   _hip.NHWC, _hip.NHWC, ops._stream(f)))
    torch.cuda.synchronize()
    assert guards_intact(out)
    assert torch.equal(out, ops.upsample2x_flow(f, 2.0))


# ---- loss backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["dpred", "grad_pred"])
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_loss_backward_off_grid_dpred(dt, place):
    """qpwc_loss_bwd with two levels of n_elems % 4 == 0 (192 and 48); level 0's dpred is 4 bytes off, or its grad_pred is
    (fp32 4 bytes, fp16 2: off the 16- / 8-byte grid of its vector stores): loss_bwd_kernel's scalar loop for that level
    beside the float4 loop for the other.  One fp32 product per element, rounded once: the bits of the aligned call and
    of the torch product; guards intact (on an MI355X: bit-equal)."""
    dtype = DTYPES[dt]
    g = torch.Generator(device=DEV).manual_seed(3)
    dpreds = [torch.randn(2, 6, 8, 2, device=DEV, generator=g), torch.randn(2, 3, 4, 2, device=DEV, generator=g)]
    grad_losses = torch.tensor([0.75, -1.5], device=DEV)
    aligned = ops.loss_bwd(dpreds, grad_losses, [dtype] * 2)
    if place == "dpred":
        got = ops.loss_bwd([off_grid(dpreds[0], 4), dpreds[1]], grad_losses, [dtype] * 2)
    else:
        got = [off_grid_out(dpreds[0].shape, dtype, 4 if dt == "f32" else 2), torch.full_like(dpreds[1], float("nan"), dtype=dtype)]
        ptrs = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])
        _hip.check(_hip.lib().qpwc_loss_bwd(ptrs(dpreds), grad_losses.data_ptr(), ptrs(got),
                                            (ctypes.c_int64 * 2)(*[d.numel() for d in dpreds]),
                                            (ctypes.c_int * 2)(*[ops._DTYPES[dtype]] * 2), 2, ops._stream(grad_losses)))
        torch.cuda.synchronize()
        assert guards_intact(got[0])
    for l, (a, b, d) in enumerate(zip(aligned, got, dpreds)):
        assert torch.equal(a, b), l
        assert torch.equal(b, (grad_losses[l] * d).to(dtype)), l

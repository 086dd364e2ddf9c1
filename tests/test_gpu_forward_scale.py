"""GPU suite of the forward kernels in the launch forms that only large launches reach.

Several forward kernels change form when a launch is large, and the large form holds the state that can go wrong: the
fused SeparableConv2D walks its tiles with resident workgroups (next tile requested early, accumulators re-zeroed in
the loop), the fp16 transposed convolution walks several output blocks per workgroup (weights reloaded, skip copy
indexed per block), and the generic cost volume, the pad zeroing and the pixel copy run capped grids whose threads
loop.  The other kernel-level tests launch shapes below every one of these thresholds.  Each case below is the
smallest that reaches its form; tests/test_forward_scale_cpu.py reads the thresholds from the sources and checks that
the shapes in CASES still do.  Data are seeded random values, so no tile, block or stride repeats another.

Oracles: the rounding points of the fp16 kernels restated on the oracle's ops, with the bounds of the small-shape
tests in tests/test_gpu_optflow.py; the C oracle for the cost volume; and, because a tile's arithmetic is the same
template body in both forms, the same images launched one at a time (the small form) bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import torch_ref
from qpwcnet_amd import _hip, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4            # the fp32 cost volume against the C oracle (tests/test_gpu_optflow.py, tests/test_gpu_parity.py)

CASES = {
    # sepconv3x3_fused_f16_kernel<.., RES = true>: (B, H, W, chans, F).  13 x 13 x 5 = 845 ragged tiles on 768
    # resident workgroups: 77 of them take a second tile, the right and bottom tiles are partial.  1, 1, 4 and 2
    # steps on the 16-byte form, then the 8-byte form over a virtual concat with a 2-channel tail (5 steps).
    "sepconv_f16_resident": [(5, 100, 200, (64,), 32), (5, 100, 200, (32,), 16), (5, 100, 200, (128,), 32),
                             (5, 100, 200, (40,), 16), (5, 100, 200, (84, 64, 2), 32)],
    # sepconv3x3_fused_kernel<.., RES = true> over three sources: 676 tiles on 512 resident workgroups
    "sepconv_f32_resident_concat": [(4, 100, 200, (84, 64, 2), 32), (4, 100, 200, (84, 32, 2), 16)],
    # upconv4x4s2_mish_f16_kernel with nfb output blocks per workgroup: (C, F, B, H, W, nfb).  Config 5's dec0,
    # dec1's form, a ragged one (partial tiles, 35 tiles per image), and every block of F = 128 in one workgroup.
    "upconv_f16_nfb": [(256, 128, 64, 8, 16, 2), (256, 64, 16, 32, 64, 4), (128, 32, 15, 50, 70, 2),
                       (256, 128, 16, 32, 64, 8)],
    # cost_volume_generic_kernel past 65536 workgroups: (B, H, W, C, data_format).  17.01 M outputs on 16.78 M
    # threads, an uneven second trip; both index branches of the kernel.
    "cost_volume_generic": [(2, 300, 350, 3, "channels_last"), (2, 300, 350, 3, "channels_first")],
    # zero_pads_kernel past 4096 workgroups: (B, H, W, C, kernel family).  1,071,648 pad values on 1,048,576 threads.
    # C = 8 is the tiled kernel (pads always zeroed by the extra launch), C = 32 the matrix-core kernel, whose dense
    # epilogue does not write the pads at W % 4 = 2.
    "zero_pads": [(24, 122, 122, 8, "cost_volume_tiled_kernel"), (24, 122, 122, 32, "cost_volume_mfma")],
    # copy_pixels_kernel: (B, H, W, C) fp32.  30.4 M 16-byte chunks on 4.19 M threads: the first 1,048,576 threads
    # take the x4-unrolled loop twice, the others once and then the tail loop three times.
    "copy_pixels": [(29, 512, 512, 16)],
}


def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def _ids(rows):
    return ["-".join(str(v) if not isinstance(v, tuple) else "x".join(map(str, v)) for v in r) for r in rows]


# ---- fused SeparableConv2D, resident forms ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sepconv_inputs(row, f16):
    """CPU operands of a SeparableConv2D case: sources, depthwise (C,1,3,3), pointwise (F,C,1,1), bias.  fp16
    storage: sources and pointwise weights rounded to fp16 (kept as fp16), depthwise and bias fp32."""
    B, H, W, chans, F = row
    C = sum(chans)
    rng = np.random.default_rng(C + F + (1 if f16 else 0))
    srcs = [_rand(rng, B, H, W, c) for c in chans]
    dw = _rand(rng, C, 1, 3, 3)
    pw = _rand(rng, F, C, 1, 1) / np.sqrt(C)
    bias = _rand(rng, F)
    if f16:
        srcs, pw = [s.half() for s in srcs], pw.half()
    return srcs, dw, pw, bias


@functools.lru_cache(maxsize=None)
def _sepconv_ref(row, f16, act):
    """The pre-activation oracle output.  fp16: the rounding points of tests/test_gpu_optflow.py's
    test_sepconv3x3_fused_fp16_storage (fp16 inputs and pointwise weights, the depthwise result rounded to fp16 once,
    an fp32 pointwise convolution)."""
    srcs, dw, pw, bias = _sepconv_inputs(row, f16)
    y = torch_ref.depthwise3x3([s.float() for s in srcs], dw, act)
    if f16:
        y = y.half().float()
    return torch.nn.functional.conv2d(y.permute(0, 3, 1, 2), pw.float(), bias).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def _sepconv_device(row, f16):
    srcs, dw, pw, bias = _sepconv_inputs(row, f16)
    return ([s.to(DEV) for s in srcs], dw.to(DEV), ops.pad_pointwise(pw.to(DEV), torch.float16 if f16 else torch.float32),
            bias.to(DEV))


def _report(what, err, bound):
    print("{}: largest error {:.3g} against a bound of {:.3g}".format(what, err, bound))


@pytest.mark.parametrize("store_act", [False, True], ids=["plain-store", "mish-on-store"])
@pytest.mark.parametrize("act", [False, True], ids=["plain-load", "mish-on-load"])
@pytest.mark.parametrize("row", CASES["sepconv_f16_resident"], ids=_ids(CASES["sepconv_f16_resident"]))
def test_sepconv3x3_fp16_resident_workgroups(row, act, store_act):
    """qpwc_sepconv3x3_f16_fwd as 768 resident workgroups over 845 tiles: against the oracle with the fp16 rounding
    points restated (rtol 2e-3, atol 4e-3: a depthwise sum on an fp16 rounding boundary may round the other way), and
    every image BIT-IDENTICAL to the same image launched alone (169 tiles: one workgroup per tile)."""
    B, H, W, chans, F = row
    d_srcs, d_dw, d_pw, d_b = _sepconv_device(row, True)
    ref = _sepconv_ref(row, True, act)
    if store_act:
        ref = torch_ref.mish(ref)
    out = ops.sepconv3x3(d_srcs, d_dw, d_pw, d_b, mish_on_load=act, mish_on_store=store_act)
    assert out.dtype == torch.float16 and out.shape == ref.shape
    got = out.float().cpu()
    excess = float(((got - ref).abs() - 2e-3 * ref.abs()).max())
    _report("fp16 resident sepconv {} -> {}".format(chans, F), excess, 4e-3)
    torch.testing.assert_close(got, ref, rtol=2e-3, atol=4e-3)
    for b in range(B):
        one = ops.sepconv3x3([s[b:b + 1] for s in d_srcs], d_dw, d_pw, d_b, mish_on_load=act, mish_on_store=store_act)
        assert torch.equal(out[b:b + 1], one), "image %d differs between the resident and the one-shot launch" % b


@pytest.mark.parametrize("act", [False, True], ids=["plain-load", "mish-on-load"])
@pytest.mark.parametrize("row", CASES["sepconv_f32_resident_concat"], ids=_ids(CASES["sepconv_f32_resident_concat"]))
def test_sepconv3x3_fp32_resident_workgroups_over_three_sources(row, act):
    """The fp32 resident form over a virtual concat [84 | 64 or 32 | 2]: the per-lane source selection is redone for
    the tile a workgroup requests early.  Against the oracle (atol 5e-5, the fp32 bound of the small-shape tests), and
    bit-identical to the same channels passed as ONE dense source (torch.cat), both stores.  The dense source has
    150 / 118 channels, so it takes the element-wise staging and the three sources the 16-byte one: two instantiations
    of one kernel.  With Mish on load they differed in the last bit until mishf stopped contracting `t + 2` into an
    FMA in one of them and not in the other (csrc/optflow_common.h)."""
    B, H, W, chans, F = row
    d_srcs, d_dw, d_pw, d_b = _sepconv_device(row, False)
    ref = _sepconv_ref(row, False, act)
    dense = torch.cat(d_srcs, dim=3)
    for store_act in (False, True):
        out = ops.sepconv3x3(d_srcs, d_dw, d_pw, d_b, mish_on_load=act, mish_on_store=store_act)
        want = torch_ref.mish(ref) if store_act else ref
        got = out.cpu()
        _report("fp32 resident sepconv {} -> {}".format(chans, F), float((got - want).abs().max()), 5e-5)
        torch.testing.assert_close(got, want, rtol=0, atol=5e-5)
        one = ops.sepconv3x3([dense], d_dw, d_pw, d_b, mish_on_load=act, mish_on_store=store_act)
        assert torch.equal(out, one), "three sources and their dense concat differ"


# ---- fp16 transposed convolution, several output blocks per workgroup ------------------------------------------------
@pytest.mark.parametrize("row", CASES["upconv_f16_nfb"], ids=_ids(CASES["upconv_f16_nfb"]))
def test_upconv4x4s2_fp16_several_output_blocks_per_workgroup(row):
    """qpwc_upconv4x4s2_mish_f16_fwd / _cat_f16_fwd with nfb = 2, 4, 2, 8: the channels past F stay untouched, the
    one-launch concat equals the transposed convolution plus the skip assignment bit for bit (strided skip: the
    interior of a zero-bordered tensor), every image equals its own one-image launch (nfb = 1) bit for bit, and
    images 0 and B - 1 meet fp32 torch on the fp16-rounded operands within the stored value's rounding:
    err - 2^-11 |ref| <= 2e-5 (tests/test_gpu_optflow.py's test_upconv4x4s2_mish_fp16_storage)."""
    C, F, B, H, W, nfb = row
    g = torch.Generator(device=DEV).manual_seed(C + F + B + H)
    x = torch.randn(B, H, W, C, device=DEV, generator=g).half()
    w = (torch.randn(C, F, 4, 4, device=DEV, generator=g) / (4 * C) ** 0.5).half()
    bias = torch.randn(F, device=DEV, generator=g)
    taps = ops.upconv_taps(w, torch.float16)
    dst = torch.full((B, 2 * H, 2 * W, F + 24), 7.0, device=DEV, dtype=torch.float16)
    ops.upconv4x4s2_mish_into(x, taps, bias, dst)
    assert bool((dst[..., F:] == 7.0).all())
    # the concat form
    padded = torch.zeros(B, 2 * H + 1, 2 * W + 1, F, device=DEV, dtype=torch.float16)
    padded[:, :2 * H, :2 * W] = torch.randn(B, 2 * H, 2 * W, F, device=DEV, generator=g).half()
    skip = padded[:, :2 * H, :2 * W, :]
    want = torch.full((B, 2 * H, 2 * W, 2 * F + 8), 7.0, device=DEV, dtype=torch.float16)
    ops.upconv4x4s2_mish_into(x, taps, bias, want)
    assert torch.equal(want[..., :F], dst[..., :F])
    want[..., F:2 * F] = skip
    got = torch.full_like(want, 7.0)
    assert ops.upconv_cat_ok(x, taps, skip, got)
    ops.upconv4x4s2_mish_cat_into(x, taps, bias, skip, got)
    assert torch.equal(got, want)
    # one image per launch: one output block per workgroup
    one = torch.empty((1, 2 * H, 2 * W, F + 24), device=DEV, dtype=torch.float16)
    for b in range(B):
        one.fill_(7.0)
        ops.upconv4x4s2_mish_into(x[b:b + 1], taps, bias, one)
        assert torch.equal(dst[b:b + 1], one), "image %d differs between nfb = %d and the one-image launch" % (b, nfb)
    # the oracle on the first and the last image
    sel = [0, B - 1]
    xs = x[sel].float().cpu().permute(0, 3, 1, 2)
    ref = torch_ref.mish(torch.nn.functional.conv_transpose2d(xs, w.float().cpu(), bias.cpu(), stride=2, padding=1))
    ref = ref.permute(0, 2, 3, 1)
    err = (dst[sel][..., :F].float().cpu() - ref).abs()
    excess = float((err - (2.0 ** -11) * ref.abs()).max())
    _report("fp16 upconv C={} F={} nfb={}".format(C, F, nfb), excess, 2e-5)
    assert excess <= 2e-5


# ---- grid-stride loops -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("row", CASES["cost_volume_generic"], ids=_ids(CASES["cost_volume_generic"]))
def test_generic_cost_volume_past_its_grid_cap(row, dtype, c_oracle):
    """cost_volume_generic_kernel (any C: here the 3-channel image cost volume) on 17.01 M outputs for 65536 x 256
    threads, channels-last and channels-first: against the C oracle, fp32 within TOL, fp16 within the bound of
    test_cost_volume_fp16_matrix_core_kernel (rtol = atol = 1e-3: the stored value's rounding)."""
    B, H, W, C, fmt = row
    assert ops.cost_volume_kernel(B, H, W, C, dtype, layout=_hip.NHWC if fmt == "channels_last" else _hip.NCHW) \
        == "cost_volume_generic_kernel"
    assert fmt == "channels_last" or not ops._nchw_fast_path(C)
    rng = np.random.default_rng(H + C)
    shape = (B, H, W, C) if fmt == "channels_last" else (B, C, H, W)
    np_dtype = np.float32 if dtype == torch.float32 else np.float16
    prv = rng.standard_normal(shape).astype(np_dtype)
    nxt = rng.standard_normal(shape).astype(np_dtype)
    out = ops.cost_volume(torch.from_numpy(prv).to(DEV), torch.from_numpy(nxt).to(DEV), data_format=fmt)
    assert out.dtype == dtype
    out = out.float().cpu().numpy()
    ref = c_oracle.cost_volume(prv.astype(np.float32), nxt.astype(np.float32), data_format=fmt)
    assert out.shape == ref.shape
    rtol, atol = (0.0, TOL) if dtype == torch.float32 else (1e-3, 1e-3)
    _report("generic cost volume {} {}".format(fmt, dtype), float((np.abs(out - ref) - rtol * np.abs(ref)).max()), atol)
    np.testing.assert_allclose(out, ref, rtol=rtol, atol=atol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("row", CASES["zero_pads"], ids=_ids(CASES["zero_pads"]))
def test_cost_volume_pad_channels_are_zeroed_past_the_grid_cap(row, dtype):
    """The 84-channel cost volume (81 + 3 zero pads, what the fp16 / vector loads downstream read) at 357,216 pixels:
    zero_pads_kernel's 4096 workgroups take a second, uneven trip.  The buffer starts as NaN; the 81 channels must be
    the dense cost volume's bits and the pads exactly 0."""
    B, H, W, C, family = row
    assert ops.cost_volume_kernel(B, H, W, C, dtype, out_pixel_stride=84).startswith(family)
    g = torch.Generator(device=DEV).manual_seed(C)
    prv = torch.randn(B, H, W, C, device=DEV, generator=g).to(dtype)
    nxt = torch.randn(B, H, W, C, device=DEV, generator=g).to(dtype)
    buf = torch.full((B, H, W, 84), float("nan"), device=DEV, dtype=dtype)
    ops.cost_volume_into(prv, nxt, buf, 0)
    assert torch.equal(buf[..., :81], ops.cost_volume(prv, nxt))
    assert bool((buf[..., 81:] == 0).all())


@pytest.mark.parametrize("row", CASES["copy_pixels"], ids=_ids(CASES["copy_pixels"]))
def test_copy_pixels_takes_a_second_unrolled_trip(row):
    """copy_pixels_kernel on 30.4 M chunks: the un-padded view of a zero-bordered tensor into the upper channels of a
    wider buffer; the lower channels stay untouched."""
    B, H, W, C = row
    g = torch.Generator(device=DEV).manual_seed(61)
    padded = torch.zeros(B, H + 1, W + 1, C, device=DEV)
    src = padded[:, :H, :W]
    src.normal_(generator=g)
    buf = torch.full((B, H, W, 2 * C), 7.0, device=DEV)
    dst = buf[..., C:]
    assert ops.copy_pixels_ok(src, dst)
    ops.copy_pixels(src, dst)
    try:
        assert torch.equal(dst, src)
        assert bool((buf[..., :C] == 7.0).all())
        assert float(padded[:, H].abs().max()) == 0.0 and float(padded[:, :, W].abs().max()) == 0.0
    finally:
        del padded, src, buf, dst
        torch.cuda.empty_cache()

"""GPU suite of the training-side reductions at the sizes where their loops run more than one trip.

The loss kernels (csrc/loss.hip), the EPE reductions (csrc/epe.hip) and the backward passes (csrc/backward.hip) run a
fixed or capped grid, and each workgroup or thread loops until the work runs out.  Their other tests use shapes where
every thread makes one trip, so a stale tile prefetch, a wrong stride or a dropped unrolled term passes there.  Every
case below makes at least two trips, and most have an uneven last trip.  tests/test_training_scale_cpu.py reads the
grid constants from the sources and checks that the shapes in CASES still do.  Data are seeded random values, so no
tile or stride repeats another.

Oracles: the float64 loss restatement of tests/test_loss_cpu.py with the tolerances of tests/test_gpu_loss.py; a
float64 EPE of the same tensors; for the backward passes the same op called one image at a time (one trip each,
checked against float64 autograd in tests/test_gpu_autograd.py)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_loss import F16_EPS, _make, _oracle  # noqa: E402
from test_loss_cpu import area_mean, make_case  # noqa: E402

from qpwcnet_amd import _hip, loss, metrics, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# The case shapes, one entry per loop path.  Loss rows are (B, H, W, [(h, w) per level]), EPE rows (B, h, w), the
# backward row (B, H, W, C).
PYR_512 = [(256, 512), (128, 256), (64, 128), (32, 64), (16, 32)]
PYR_1024 = [(512, 1024), (256, 512), (128, 256), (64, 128), (32, 64)]
CASES = {
    # loss_area_tile_kernel: 2,560 tiles on 2,048 workgroups (512 of them take a second tile), and 6,144 tiles (three
    # per workgroup).  The finest level of both also loops loss_bwd_kernel's float4 path.
    "tile": [(5, 512, 1024, PYR_512), (3, 1024, 2048, PYR_1024)],
    # area factors (sh, sw) = (2, 16) (32, 32) (1, 4) (8, 32) (2, 8): nested, different per axis, not in area order
    "tile_plan": [(5, 512, 1024, [(256, 64), (16, 32), (512, 256), (64, 32), (256, 128)])],
    # FlowMseLossV2 on loss_pixel_kernel (misaligned ground truth) against the tile kernel
    "tile_vs_pixel": [(5, 512, 1024, PYR_512)],
    # the bilinear kinds on loss_pixel_kernel, every level past one trip; ratios 2, 2.5 and 1.875 (exact in fp32, so
    # the sample points are the float64 oracle's)
    "bilinear": [(5, 480, 960, [(240, 480), (192, 384), (256, 512)])],
    # loss_bwd_kernel's scalar path: B * h * w odd, so neither flows (C = 2) nor images (C = 3) are whole float4;
    # one trip, then several
    "bwd_scalar": [(1, 42, 70, [(21, 35)]), (3, 402, 666, [(201, 333)])],
    # epe_multi_partial_kernel, fp32 channels-last and 16-byte aligned: the x4 loop over float4 (2 pixels each), the
    # remainder loop and the odd-pixel tail; then a config-4 level
    "epe_f32_x4": [(3, 257, 511), (16, 512, 1024)],
    # ... fp16 predictions, channels-last: the x4 loop over pixels
    "epe_f16_x4": [(3, 257, 511)],
    # ... channels-first (fp32 and fp16) and misaligned fp32: plain grid-stride loops
    "epe_plain": [(2, 257, 511)],
    # epe_partial_kernel (ops.epe), both layouts
    "epe": [(2, 257, 511)],
    # cost_volume_bwd_kernel, warp_bwd_kernel, fill_zero_kernel, f32_to_f16_kernel: 64 lanes per pixel at C = 64
    "backward": [(4, 1024, 1040, 64)],
}
KIND_CODES = {"v2": _hip.LOSS_FLOW_MSE_V2, "mse": _hip.LOSS_FLOW_MSE, "finetune": _hip.LOSS_FLOW_FINETUNE,
              "autoresize": _hip.LOSS_AUTORESIZE_MSE}


# ---- losses ----------------------------------------------------------------------------------------------------------
def _layout(t, data_format):
    return t.permute(0, 3, 1, 2).contiguous() if data_format == "channels_first" else t


def _nhwc(t, data_format):
    return t.permute(0, 2, 3, 1) if data_format == "channels_first" else t


def _kernel(kind, gt, levels, data_format):
    """The forward kernel qpwc_loss_fwd takes for this device ground truth (its own selection rule, run on the host)."""
    B, H, W, C = gt.shape if data_format == "channels_last" else (gt.shape[0], gt.shape[2], gt.shape[3], gt.shape[1])
    I, n = ctypes.c_int, len(levels)
    h, w = zip(*levels)
    return _hip.lib().qpwc_loss_fwd_kernel(KIND_CODES[kind], gt.data_ptr(), B, H, W, C, (I * n)(*h), (I * n)(*w),
                                           n).decode()


def _misaligned(t, floats=1):
    """A dense copy of fp32 device tensor t that starts `floats` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + floats, dtype=t.dtype, device=t.device)
    out = buf[floats:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 * floats
    return out


def _gpu_losses(kind, data_format, gt_dev, preds, scale):
    """Per-level losses and the gradients of scale * their sum (channels-last views) from loss.multiscale; preds are
    channels-last CPU tensors of the prediction dtype."""
    xs = [_layout(p, data_format).to(DEV).requires_grad_() for p in preds]
    _, per = loss.multiscale(_make(kind, data_format), gt_dev, xs)
    (scale * per).sum().backward()
    return per.tolist(), [_nhwc(x.grad, data_format) for x in xs]


def _check_losses(per, grads, ref_v, ref_g, dtype, what):
    """tests/test_gpu_loss.py's bounds: values within 1e-5 relative; fp32 gradients within 1e-5 of their maximum; fp16
    gradients within half an fp16 ulp (plus 1e-5 of the maximum), and a 1/16 larger gradient must fail that bound."""
    assert len(per) == len(ref_v)
    for l, (v, g, rv, rg) in enumerate(zip(per, grads, ref_v, ref_g)):
        assert abs(v - rv) <= 1e-5 * abs(rv), (what, l, v, rv)
        assert g.dtype == dtype and g.shape == rg.shape, (what, l, g.dtype, tuple(g.shape))
        got = g.double().cpu()
        d = (got - rg).abs()
        m = float(rg.abs().max())
        if dtype == torch.float32:
            assert float(d.max()) <= 1e-5 * m, (what, l, float(d.max()), m)
        else:
            bound = F16_EPS * rg.abs() + 1e-5 * m + 2.0 ** -24
            assert bool((d <= bound).all()), (what, l, float((d - bound).max()))
            bad = rg * (1 + 1 / 16)
            bound = F16_EPS * bad.abs() + 1e-5 * m + 2.0 ** -24
            assert not bool(((got - bad).abs() <= bound).all()), (what, l)


def _case(kind, row, seed, dtype=torch.float32, f16_scale=2.0 ** 16):
    """make_case in channels-last, the predictions in dtype, and the float64 oracle -> (gt, preds, ref_v, ref_g, scale).
    fp16: the loss scale that keeps the gradients normal in fp16."""
    B, H, W, lv = row
    gt, preds = make_case(kind, B, H, W, lv, "channels_last", seed, torch.float32)
    preds = [p.to(dtype) for p in preds]
    scale = 1.0 if dtype == torch.float32 else f16_scale
    ref_v, ref_g = _oracle(kind, gt, preds, "channels_last", scale)
    return gt, preds, ref_v, ref_g, scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("row", CASES["tile"], ids=["2560_tiles", "6144_tiles"])
def test_area_tile_kernel_walks_several_tiles_per_workgroup(row, dtype):
    # FlowMseLossV2's gradient is (2 / (w + h))^2 * residual / n: ~1e-12 per unit of loss scale at these finest levels,
    # so 2^16 leaves it a few fp16 subnormal steps (where the negative control cannot fail); 2^32 keeps every level
    # between 1e-3 and 1e3
    gt, preds, ref_v, ref_g, scale = _case("v2", row, 31, dtype, f16_scale=2.0 ** 32)
    for fmt in ("channels_last", "channels_first"):
        g = _layout(gt, fmt).to(DEV)
        assert _kernel("v2", g, row[3], fmt) == "loss_area_tile_kernel"
        per, grads = _gpu_losses("v2", fmt, g, preds, scale)
        _check_losses(per, grads, ref_v, ref_g, dtype, fmt)


def test_area_tile_plan_with_per_axis_factors_keeps_the_callers_level_order():
    row = CASES["tile_plan"][0]
    B, H, W, lv = row
    areas = [(H // h) * (W // w) for h, w in lv]
    assert areas != sorted(areas) and len({H // h for h, _ in lv}) > 1 and any(H // h != W // w for h, w in lv)
    gt, preds, ref_v, ref_g, scale = _case("v2", row, 32)
    for fmt in ("channels_last", "channels_first"):
        g = _layout(gt, fmt).to(DEV)
        assert _kernel("v2", g, lv, fmt) == "loss_area_tile_kernel"
        per, grads = _gpu_losses("v2", fmt, g, preds, scale)
        _check_losses(per, grads, ref_v, ref_g, torch.float32, fmt)


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
def test_area_tile_and_pixel_kernels_agree_past_one_trip(data_format):
    """The same FlowMseLossV2 inputs with a 16-byte aligned ground truth (tile kernel) and one a float further on
    (pixel kernel): both against float64, and against each other.  Then the area ground truth alone."""
    row = CASES["tile_vs_pixel"][0]
    B, H, W, lv = row
    gt, preds, ref_v, ref_g, scale = _case("v2", row, 33)
    aligned = _layout(gt, data_format).to(DEV)
    shifted = _misaligned(aligned)
    inputs = (("loss_area_tile_kernel", aligned), ("loss_pixel_kernel", shifted))
    per = {}
    for name, g in inputs:
        assert _kernel("v2", g, lv, data_format) == name
        per[name], grads = _gpu_losses("v2", data_format, g, preds, scale)
        _check_losses(per[name], grads, ref_v, ref_g, torch.float32, name)
    for l, (a, b) in enumerate(zip(per["loss_area_tile_kernel"], per["loss_pixel_kernel"])):
        assert abs(a - b) <= 1e-6 * abs(b), (l, a, b)
    refs = [area_mean(gt.double(), h, w) * (h / H) for h, w in lv]
    outs = {name: metrics.multiscale_ground_truth(g, lv, data_format, mode="area") for name, g in inputs}
    for name, ts in outs.items():
        for (h, w), t, r in zip(lv, ts, refs):
            t = _nhwc(t, data_format).double().cpu()
            assert t.shape == r.shape
            d = float((t - r).abs().max())
            assert d <= 1e-6 * float(r.abs().max()), (name, (h, w), d)
    for (h, w), a, b in zip(lv, outs["loss_area_tile_kernel"], outs["loss_pixel_kernel"]):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), (h, w)


@pytest.mark.parametrize("kind", ["mse", "finetune", "autoresize"])
def test_bilinear_losses_on_the_pixel_kernel_past_one_trip(kind):
    row = CASES["bilinear"][0]
    gt, preds, ref_v, ref_g, scale = _case(kind, row, 34)
    assert any(row[1] % h or row[2] % w for h, w in row[3])          # a ratio that is not an integer
    for fmt in ("channels_last", "channels_first"):
        g = _layout(gt, fmt).to(DEV)
        assert _kernel(kind, g, row[3], fmt) == "loss_pixel_kernel"
        per, grads = _gpu_losses(kind, fmt, g, preds, scale)
        _check_losses(per, grads, ref_v, ref_g, torch.float32, fmt)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("row", CASES["bwd_scalar"], ids=["one_trip", "looped"])
@pytest.mark.parametrize("kind", ["mse", "autoresize"])
def test_loss_backward_scalar_path(kind, row, dtype):
    gt, preds, ref_v, ref_g, scale = _case(kind, row, 35, dtype)
    assert all(p.numel() % 4 for p in preds)
    per, grads = _gpu_losses(kind, "channels_last", gt.to(DEV), preds, scale)
    _check_losses(per, grads, ref_v, ref_g, dtype, kind)


# ---- EPE -------------------------------------------------------------------------------------------------------------
def _flow_pair(gen, shape):
    a = torch.randn(shape, generator=gen) * 4
    return a, a + torch.randn(shape, generator=gen)


def _epe64(a, b, axis):
    return float(torch.linalg.vector_norm(a.double() - b.double(), dim=axis).mean())


def _check_epe(got, refs, what):
    got = got.tolist() if isinstance(got, torch.Tensor) else got
    assert len(got) == len(refs)
    for l, (g, r) in enumerate(zip(got, refs)):
        assert abs(g - r) <= 1e-5 * r, (what, l, g, r)


def test_epe_multi_fp32_unrolled_loop():
    gen = torch.Generator().manual_seed(41)
    pairs = [_flow_pair(gen, (B, h, w, 2)) for B, h, w in CASES["epe_f32_x4"]]
    refs = [_epe64(a, b, -1) for a, b in pairs]
    ta, tb = [a.to(DEV) for a, _ in pairs], [b.to(DEV) for _, b in pairs]
    assert all(t.data_ptr() % 16 == 0 for t in ta + tb)
    _check_epe(metrics.per_level_epe(ta, tb), refs, "levels together")
    for a, b, r in zip(ta, tb, refs):
        _check_epe(ops.epe_multi([a], [b]), [r], tuple(a.shape))


def test_epe_multi_fp16_predictions_past_one_trip():
    gen = torch.Generator().manual_seed(42)
    for B, h, w in CASES["epe_f16_x4"] + CASES["epe_plain"]:
        a, b = _flow_pair(gen, (B, h, w, 2))
        b = b.half()
        _check_epe(ops.epe_multi([a.to(DEV)], [b.to(DEV)]), [_epe64(a, b, -1)], ("channels_last", B, h, w))
        a, b = a.permute(0, 3, 1, 2).contiguous(), b.permute(0, 3, 1, 2).contiguous()
        got = ops.epe_multi([a.to(DEV)], [b.to(DEV)], data_format="channels_first")
        _check_epe(got, [_epe64(a, b, 1)], ("channels_first", B, h, w))


def test_epe_multi_plain_fp32_loops():
    gen = torch.Generator().manual_seed(43)
    for B, h, w in CASES["epe_plain"]:
        a, b = _flow_pair(gen, (B, h, w, 2))
        ref = _epe64(a, b, -1)
        ac, bc = a.permute(0, 3, 1, 2).contiguous(), b.permute(0, 3, 1, 2).contiguous()
        _check_epe(ops.epe_multi([ac.to(DEV)], [bc.to(DEV)], data_format="channels_first"), [ref], "channels_first")
        # one pixel (8 bytes) past a 16-byte boundary: the float2 loop instead of the float4 one
        ma, mb = _misaligned(a.to(DEV), 2), _misaligned(b.to(DEV), 2)
        _check_epe(ops.epe_multi([ma], [mb]), [ref], "misaligned")


def test_epe_grid_stride_loop_both_layouts():
    gen = torch.Generator().manual_seed(44)
    for B, h, w in CASES["epe"]:
        a, b = _flow_pair(gen, (B, h, w, 2))
        ref = _epe64(a, b, -1)
        _check_epe([float(ops.epe(a.to(DEV), b.to(DEV)))], [ref], "channels_last")
        ac, bc = (t.permute(0, 3, 1, 2).contiguous().to(DEV) for t in (a, b))
        _check_epe([float(ops.epe(ac, bc, "channels_first"))], [ref], "channels_first")


# ---- backward passes -------------------------------------------------------------------------------------------------
def _grid(gen, shape, dtype):
    """Multiples of 1/16 in [-1, 1] on the device: exact in fp16.  With flows in steps of 2^-6, most of the sums that
    grad_img's atomics form are then exact in fp32, whatever order the atomics land in."""
    t = torch.rand(shape, device=DEV, generator=gen)
    return t.mul_(33).floor_().sub_(16).div_(16).to(dtype)


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_cost_volume_backward_grid_stride_is_the_per_image_op_bit_for_bit(dtype):
    """4,259,840 pixels for 2^22 pixel groups: a second trip.  grad_prv / grad_nxt are gathers summed in a fixed order,
    so the batched call must give the bits of four one-trip calls.  The outputs start as NaN: a pixel that no trip
    writes fails.  `out` only supplies the LeakyReLU mask (out > 0), so random values serve."""
    B, H, W, C = CASES["backward"][0]
    r, d = 4, 9
    gen = torch.Generator(device=DEV).manual_seed(51)
    prv, nxt = _grid(gen, (B, H, W, C), dtype), _grid(gen, (B, H, W, C), dtype)
    out, gout = _grid(gen, (B, H, W, d * d), dtype), _grid(gen, (B, H, W, d * d), dtype)
    gp, gn = _nan(prv.shape, dtype), _nan(nxt.shape, dtype)
    rc = _hip.lib().qpwc_cost_volume_bwd(prv.data_ptr(), nxt.data_ptr(), out.data_ptr(), gout.data_ptr(),
                                         gp.data_ptr(), gn.data_ptr(), B, H, W, C, r, ops._DTYPES[dtype], 0.1,
                                         ops._stream(prv))
    _hip.check(rc)
    for b in range(B):
        s = slice(b, b + 1)
        rp, rn = ops.cost_volume_bwd(prv[s], nxt[s], out[s], gout[s], r, 0.1)
        assert torch.equal(gp[s], rp), b
        assert torch.equal(gn[s], rn), b


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("mode", ["clamp", "tfwarp"])
def test_warp_backward_grid_stride_matches_the_per_image_op(mode, dtype):
    """As the cost-volume case: grad_flo is a fixed-order reduction per pixel, so bit-identical; grad_img is scattered
    by float atomics, so within 1e-6 of its maximum (fp16: plus one fp16 ulp of the element, for a sum that rounds to
    the other side).  fill_zero_kernel and f32_to_f16_kernel walk 272.6 M elements here: their targets start as NaN."""
    B, H, W, C = CASES["backward"][0]
    gen = torch.Generator(device=DEV).manual_seed(52)
    img, gout = _grid(gen, (B, H, W, C), dtype), _grid(gen, (B, H, W, C), dtype)
    flo = torch.randint(-6 * 64, 6 * 64 + 1, (B, H, W, 2), device=DEV, generator=gen).float() / 64
    L = _hip.lib()
    dt = ops._DTYPES[dtype]
    gi, gf = _nan(img.shape, dtype), _nan((B, H, W, 2), torch.float32)
    nws = int(L.qpwc_warp_bwd_workspace_floats(B, H, W, C, dt))
    _hip.check(min(nws, 0))
    ws = _nan((max(nws, 1),), torch.float32)
    code = _hip.WARP_CLAMP if mode == "clamp" else _hip.WARP_TFWARP
    _hip.check(L.qpwc_warp_bwd(img.data_ptr(), flo.data_ptr(), gout.data_ptr(), gi.data_ptr(), gf.data_ptr(),
                               ws.data_ptr() if nws > 0 else None, B, H, W, C, dt, code, ops._stream(img)))
    for b in range(B):
        s = slice(b, b + 1)
        ri, rf = ops.warp_bwd(img[s], flo[s], gout[s], mode)
        assert torch.equal(gf[s], rf), b
        ref = ri.float()
        m = float(ref.abs().max())
        d = (gi[s].float() - ref).abs()
        bound = 1e-6 * m + (2.0 ** -10 * ref.abs() if dtype == torch.float16 else 0.0)
        assert bool((d <= bound).all()), (b, float((d - bound).max()))

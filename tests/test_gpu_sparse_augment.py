"""GPU suite of the sparse-ground-truth input pipeline (qpwcnet_amd.augment ``*_sparse`` on qpwc_augment_sparse_fwd).

Oracle: ``ref_augment_sparse`` (tests/test_sparse_augment_cpu.py), a float64 restatement whose coordinates and weights are
the contract's fp32 values.  The output mask must equal the restatement's in every pixel; the flow is held to BOUND =
1e-4 px where the mask is 1 and to exactly 0 where it is 0; the frames to BOUND against the dense restatement, and to
``augment.preprocess`` on the device bit for bit.
Inputs: make_case (384 output pixels = one full and one half workgroup, every flip combination, the <vec4> form) and
tiny_case (35 pixels, the <scalar> form) under half-density masks with NaN, +Inf and 1e10 planted; the CPU suite proves
that both hold output pixels with 0, 1, 2, 3 and 4 valid corners.
Measured on an MI355X: frames 4.5e-6 with the colour stage and 2.2e-6 without, flow 4.3e-6 px (make_case); frames 3.4e-7,
flow 2.3e-6 px (tiny_case)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import as_params, make_case, smooth_flow, tiny_case  # noqa: E402
from test_sparse_augment_cpu import (FORMATS, check_against, garbage_pair, ref_augment_sparse, reference,  # noqa: E402
                                     sparse_case, torch_case)

from qpwcnet_amd import augment, loss, metrics, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("data_format", FORMATS)
@pytest.mark.parametrize("name,dtype", [("make", np.uint8), ("make", np.float32), ("tiny", np.uint8)],
                         ids=["make-u8", "make-f32", "tiny-u8"])
def test_kernels_match_restatement(name, dtype, data_format, colour, with_mask):
    ims, flo, mask, params, hw = torch_case(sparse_case(name, dtype), DEV)
    form = "<vec4>" if name == "make" else "<scalar>"
    assert ops.augment_sparse_kernel(ims.shape[0], *hw) == "augment_sparse_pixel_kernel" + form
    got = ops.augment_sparse(ims, flo, mask.view(torch.uint8) if with_mask else None, params.iparams, params.fparams, hw,
                             colour=colour, data_format=data_format)
    assert all(t.is_contiguous() and t.device == ims.device for t in got)
    check_against(got, reference(name, dtype, colour, True, with_mask), data_format,
                  "kernel {} {} colour={} mask={}".format(name, np.dtype(dtype).name, colour, with_mask))


@pytest.mark.parametrize("data_format", FORMATS)
def test_entry_points_run_the_kernels(data_format):
    ims, flo, mask, params, hw = torch_case(sparse_case("make", np.uint8), DEV)
    got = augment.preprocess_sparse(ims, flo, mask, data_format, out_shape=hw, params=params)
    check_against(got, reference("make"), data_format, "preprocess_sparse")
    f_ims = torch_case(sparse_case("make", np.float32), DEV)[0]
    if data_format == "channels_last":
        got = augment.image_augment_sparse(f_ims, flo, hw, valid=mask.float(), params=params)
        check_against(got, reference("make", np.float32, True, False), what="image_augment_sparse")
    case = sparse_case("make", np.uint8)
    rp = augment.resize_params(4, (30, 52), hw)
    want = ref_augment_sparse(case[0], case[1], case[2], rp.iparams.numpy(), rp.fparams.numpy(), hw, colour=False)
    check_against(augment.preprocess_no_op_sparse(ims, flo, mask, data_format, out_shape=hw), want, data_format,
                  "preprocess_no_op_sparse")
    if data_format == "channels_last":
        want = ref_augment_sparse(sparse_case("make", np.float32)[0], case[1], case[2], rp.iparams.numpy(),
                                  rp.fparams.numpy(), hw, colour=False, finish=False)
        check_against(augment.image_resize_sparse(f_ims, flo, hw, valid=mask), want, what="image_resize_sparse")


@pytest.mark.parametrize("data_format", FORMATS)
def test_all_valid_is_the_dense_pipeline_bit_for_bit(data_format):
    for case in (make_case(np.uint8), make_case(np.float32), tiny_case()):          # both forms
        ims, flo, ip, fp, hw = case
        t_ims, t_flo, p = torch.from_numpy(ims).to(DEV), torch.from_numpy(flo).to(DEV), as_params(ip, fp, DEV)
        want = augment.preprocess(t_ims, t_flo, data_format, out_shape=hw, params=p)
        for valid in (None, torch.ones(flo.shape[:3], dtype=torch.uint8, device=DEV)):
            got = augment.preprocess_sparse(t_ims, t_flo, valid, data_format, out_shape=hw, params=p)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool((got[2] == 1).all())
        # the frames keep the dense bits under a mask too
        mask = torch.from_numpy(sparse_case("make")[2] if len(ims) == 4 else sparse_case("tiny")[2]).to(DEV)
        assert torch.equal(augment.preprocess_sparse(t_ims, t_flo, mask, data_format, out_shape=hw, params=p)[0], want[0])


@pytest.mark.parametrize("name", ["make", "tiny"])
def test_layouts_and_a_repeated_call_agree_bit_for_bit(name):
    ims, flo, mask, params, hw = torch_case(sparse_case(name), DEV)
    last = augment.preprocess_sparse(ims, flo, mask, "channels_last", out_shape=hw, params=params)
    first = augment.preprocess_sparse(ims, flo, mask, "channels_first", out_shape=hw, params=params)
    again = augment.preprocess_sparse(ims, flo, mask, "channels_first", out_shape=hw, params=params)
    assert _same(first, again)
    assert torch.equal(first[0], last[0].permute(0, 3, 1, 2)) and torch.equal(first[1], last[1].permute(0, 3, 1, 2))
    assert torch.equal(first[2], last[2])


@pytest.mark.parametrize("data_format", FORMATS)
@pytest.mark.parametrize("name", ["make", "tiny"])
def test_selected_out_pixels_change_no_bit(name, data_format):
    plain, dirty = garbage_pair(name)
    outs = []
    for case in (plain, dirty):
        ims, flo, mask, params, hw = torch_case(case, DEV)
        outs.append([t.cpu().numpy() for t in augment.preprocess_sparse(ims, flo, mask, data_format, out_shape=hw,
                                                                         params=params)])
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    check_against(outs[1], reference(name), data_format, "garbage " + name)


def test_one_sample_without_a_valid_pixel():
    ims, flo, mask, params, hw = torch_case(sparse_case("make"), DEV)
    want = augment.preprocess_sparse(ims, flo, mask, "channels_first", out_shape=hw, params=params)
    empty = mask.clone()
    empty[2] = False
    got = augment.preprocess_sparse(ims, flo, empty, "channels_first", out_shape=hw, params=params)
    assert not got[1][2].any() and not got[2][2].any() and got[1][2].cpu().numpy().tobytes() == bytes(2 * 16 * 24 * 4)
    keep = [0, 1, 3]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1][keep], want[1][keep]) and torch.equal(got[2][keep], want[2][keep])
    assert bool(want[2][2].any())


def test_the_sampler_with_a_device_generator_is_reproducible():
    ims, flo, mask, _, hw = torch_case(sparse_case("make"), DEV)
    g = lambda seed: torch.Generator(device=DEV).manual_seed(seed)
    a = augment.preprocess_sparse(ims, flo, mask, out_shape=hw, base_scale=1.0, generator=g(5))
    b = augment.preprocess_sparse(ims, flo, mask, out_shape=hw, base_scale=1.0, generator=g(5))
    c = augment.preprocess_sparse(ims, flo, mask, out_shape=hw, base_scale=1.0, generator=g(6))
    assert _same(a, b) and not torch.equal(a[1], c[1])
    p = augment.sample_params(4, (30, 52), hw, 1.0, generator=g(5), device=DEV)
    assert _same(a, augment.preprocess_sparse(ims, flo, mask, out_shape=hw, params=p))


def test_hand_off_to_the_masked_loss_and_the_flow_scores():
    """preprocess_sparse -> loss.multiscale_masked (forward and backward) and metrics.flow_quality at 64 x 64, against the
    same calls on CPU tensors, at tests/test_gpu_masked_loss.py's bounds: losses 1e-5 relative, gradients 1e-5 of the
    level's largest; the scores 1e-5 relative; counts and masks exact."""
    rng = np.random.default_rng(8)
    B, H, W, hw = 2, 80, 96, (64, 64)
    ims = torch.from_numpy(rng.integers(0, 256, (B, H, W, 6), dtype=np.uint8))
    flo = torch.from_numpy(smooth_flow(B, H, W, seed=3))
    mask = torch.from_numpy(rng.random((B, H, W)) < 0.3)
    flo[0, 5, 7, 0], flo[1, 40, 41, 1] = float("nan"), 1e10
    mask[0, 5, 7] = mask[1, 40, 41] = True
    params = augment.sample_params(B, (H, W), hw, 0.9, generator=torch.Generator().manual_seed(9))
    preds = [torch.from_numpy(rng.standard_normal((B, 2, 64 >> k, 64 >> k)).astype(np.float32)) for k in (1, 2)]
    # end-point errors of 0.5, 2, 4 and 7 px: well away from the scores' thresholds (1, 3, 5 px; 5 % of a speed below 30 px)
    ang, mag = rng.random((B, 64, 64)) * 2 * np.pi, rng.choice([0.5, 2.0, 4.0, 7.0], size=(B, 64, 64))
    pred0 = torch.from_numpy(np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1).astype(np.float32))
    obj = loss.FlowMseLoss("channels_first")
    res = {}
    for dev in ("cpu", DEV):
        o_ims, o_flo, o_valid = augment.preprocess_sparse(ims.to(dev), flo.to(dev), mask.to(dev), "channels_first",
                                                          out_shape=hw, params=as_params(params.iparams.numpy(),
                                                                                         params.fparams.numpy(), dev))
        xs = [p.clone().to(dev).requires_grad_() for p in preds]
        total, per, counts = loss.multiscale_masked(obj, o_flo, xs, o_valid)
        total.backward()
        scores = metrics.flow_quality(o_flo, o_flo + pred0.to(dev), valid=o_valid, data_format="channels_first")
        res[dev] = (o_valid.cpu(), per.detach().cpu().double(), counts.cpu(), [x.grad.cpu().double() for x in xs],
                    [s.cpu().double() for s in scores])
    (v0, per0, n0, g0, s0), (v1, per1, n1, g1, s1) = res["cpu"], res[DEV]
    assert torch.equal(v0, v1) and torch.equal(n0, n1) and 0.2 < float(v0.float().mean()) < 0.95
    assert bool(((per1 - per0).abs() <= 1e-5 * per0.abs()).all()), (per0, per1)
    for a, b in zip(g0, g1):
        assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
    for field, a, b in zip(metrics.FlowScores._fields, s0, s1):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), field
        ok = ~torch.isnan(a)
        assert bool(((a - b).abs()[ok] <= 1e-5 * a.abs()[ok]).all()), (field, a, b)


def test_refusals_on_the_device():
    ims, flo, mask, params, hw = torch_case(sparse_case("tiny"), DEV)
    m8 = mask.view(torch.uint8)
    with pytest.raises(ValueError, match="valid"):
        ops.augment_sparse(ims, flo, mask, params.iparams, params.fparams, hw)              # bool: the wrapper converts
    with pytest.raises(ValueError, match="valid"):
        ops.augment_sparse(ims, flo, m8.cpu(), params.iparams, params.fparams, hw)
    with pytest.raises(ValueError, match="valid"):
        ops.augment_sparse(ims, flo, m8[:, :, :-1], params.iparams, params.fparams, hw)
    with pytest.raises(ValueError, match="Unsupported data format"):
        ops.augment_sparse(ims, flo, m8, params.iparams, params.fparams, hw, data_format="channels_middle")
    with pytest.raises(ValueError, match="non-positive"):
        ops.augment_sparse(ims, flo, m8, params.iparams, params.fparams, (0, 5))

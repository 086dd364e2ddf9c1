"""GPU suite of the flow evaluation metrics (qpwcnet_amd.metrics.flow_quality on qpwc_flow_quality_fwd).

Oracle: ``ref_flow_quality``, the float64 restatement in tests/test_flow_quality_cpu.py (the fp32 torch composition meets
the same bounds there).  Bounds: the count ratios (fl, acc1, acc3, acc5, valid) to the fp32 rounding of the quotient
(1 ulp; no valid pixel of a case lies within 1e-3 of a threshold), the EPE-type means 1e-4 px absolute, aae 1e-3 degrees.
B = 2 throughout; the two images of a batch differ in content and in error level (sigma 0.3 px and 4 px), so a batch-index
mix-up shows.  The cases (CASES, sized by _hip.FLOW_QUALITY_CHUNK = CHUNK pixels per workgroup) and what each is chosen
for:
  1x1                    one pixel per image;
  3x5                    less than a wave;
  chunks                 H * W = 2 CHUNK + 3 with an odd width: two whole chunks and a last one of 3 pixels; a 50 px error at
                         pixel 0 and at the last pixel; the only s40+ pixels of image 1 lie in the last chunk
                         (test_flow_quality_cpu.py::test_the_comparison_sees_the_planted_defects);
  chunks_channels_first, chunks_f16_pred     the other layout; an fp16 prediction;
  valid, occluded, both_masks                independent random masks (48 % / 7 % masked out, 30 % occluded in image 0;
                         the only occluded pixels of image 1 are the last chunk);
  unknown_gt             NaN, +-inf and +-1e10 planted in the ground truth: excluded;
  all_invalid            image 0 fully masked out: NaN ratios and valid = 0, image 1 normal;
  near_equal             prediction = truth + N(0, 0.01): acosf of the normalised dot product would miss aae.
Beside the values: operands the wrapper has to copy (a flow 4 bytes off the 8-byte grid, an fp16 prediction 2 bytes off the
4-byte grid, masks that are strided views) and uint8 masks holding 2, 128 or 255 for 1 give the same bits.  Larger batches
and longer images, where the fold kernel's loops iterate: tests/test_gpu_eval_scale.py; past 2^31 elements:
tests/test_gpu_large_offsets.py.
Measured on an MI355X: see the docstrings of the tests and DESIGN.md section 4.25."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_quality_cpu import (B, BOUNDS, CASES, CHUNK, CHUNKS, FIELDS, LAST, check, check_state,  # noqa: E402
                                   closed_form, make_flows, reference, run_case, state_scenario, tensor, violations)

from qpwcnet_amd import metrics, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_the_float64_restatement(name):
    """Every case against ref_flow_quality.  Measured on an MI355X, the largest error over the eleven cases: 1.8e-6 px in
    the EPE-type means (the cases on the chunks flows; 3.8e-7 on 3x5), 5.2e-7 degrees in aae (unknown_gt), every count
    ratio the rounded float64 quotient (at most 0.5 ulp); the torch composition on the CPU is at 1.8e-6 px and 5.8e-7
    degrees."""
    c = CASES[name]
    shape = c["truth"].shape
    H, W = (shape[1], shape[2]) if c["data_format"] == "channels_last" else (shape[2], shape[3])
    if name not in ("1x1", "3x5", "near_equal"):
        assert (H, W) == CHUNKS and -(-(H * W) // CHUNK) == 3 and 0 < LAST < 64
    res, got = run_case(name, DEV)
    assert isinstance(res, metrics.FlowScores) and all(v.is_cuda and v.dtype == torch.float32 for v in res)
    assert all(tuple(v.shape) == (B,) for v in res)
    check("hip " + name, got, reference(name))
    # the launcher gives twelve views of one tensor
    assert all(v.data_ptr() == res.epe.data_ptr() + 4 * B * i for i, v in enumerate(res))


def test_closed_form_and_truth_is_pred():
    """truth (3, 4) against 0: e = m = 5 on every strict comparison's threshold; one buffer for both flows: e = 0,
    aae = 0, fl = 0, acc = 1.  Measured on an MI355X: the closed form is exact but for aae, 3.6e-6 degrees from
    atan2(5, 1); truth is pred gives 0 and 1 exactly."""
    err = closed_form(DEV)
    print("hip closed form: aae {:.2e} deg".format(err))
    t = tensor(CASES["chunks"]["truth"]).to(DEV)
    res = metrics.flow_quality(t, t, data_format="channels_last")
    for k in ("epe", "aae", "fl", "epe_noc"):
        assert bool((getattr(res, k) == 0).all()), k
    for k in ("acc1", "acc3", "acc5", "valid"):
        assert bool((getattr(res, k) == 1).all()), k
    assert bool(torch.isnan(res.epe_occ).all()) and bool((res.epe_s0_10 == 0).all())


def test_state_accumulates_in_image_order():
    """Two calls on different batches through one FlowQuality: the float64 running sums, images = 2 B, the pixels and
    the pixel-weighted result, as on the CPU; with and without a state, out is the same bit for bit."""
    m, per, sums, pixels = state_scenario(DEV)
    assert m.state.is_cuda
    for got, name in zip(per, ("chunks", "both_masks")):
        assert violations(got, reference(name))[0] == []
        assert same_bits(got, run_case(name, DEV)[0])
    check_state(m, per, sums, pixels)


def test_two_runs_and_both_layouts_are_bitwise_equal():
    a, _ = run_case("chunks", DEV)
    b, _ = run_case("chunks", DEV)
    assert same_bits(a, b)
    # which lane sums which pixel does not depend on the layout
    cf, _ = run_case("chunks_channels_first", DEV)
    assert same_bits(a, cf)


def test_flows_off_the_8_byte_grid_take_the_wrappers_copy():
    """An fp32 flow sliced so that its first byte is 4 off the 8-byte grid of the (B,H,W,2) pixel loads: the wrapper
    copies it, and the scores are those of the aligned clone, bit for bit."""
    c = CASES["both_masks"]
    valid, occluded = tensor(c["valid"]).to(DEV), tensor(c["occluded"]).to(DEV)
    want, _ = run_case("both_masks", DEV)
    for which in ("truth", "pred", "both"):
        ops_in = {}
        for k in ("truth", "pred"):
            x = tensor(c[k]).to(DEV)
            if which in (k, "both"):
                room = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)
                room[1:] = x.reshape(-1)
                x = room[1:].view(x.shape)
                assert x.data_ptr() % 8 == 4 and x.is_contiguous()
            ops_in[k] = x
        got = metrics.flow_quality(ops_in["truth"], ops_in["pred"], valid=valid, occluded=occluded,
                                   data_format="channels_last")
        assert same_bits(got, want), which


def test_fp16_prediction_off_the_4_byte_grid_takes_the_wrappers_copy():
    """An fp16 channels-last prediction whose first byte is 2 off the 4-byte grid of the __half2 pixel load: the wrapper
    copies it, and the scores are those of the aligned clone, bit for bit."""
    c = CASES["chunks_f16_pred"]
    want, _ = run_case("chunks_f16_pred", DEV)
    pred = tensor(c["pred"]).to(DEV)
    room = torch.empty(pred.numel() + 1, dtype=torch.float16, device=DEV)
    room[1:] = pred.reshape(-1)
    off = room[1:].view(pred.shape)
    assert off.dtype == torch.float16 and off.data_ptr() % 4 == 2 and off.is_contiguous()
    got = metrics.flow_quality(tensor(c["truth"]).to(DEV), off, data_format="channels_last")
    assert same_bits(got, want)
    assert violations(got, reference("chunks_f16_pred"))[0] == []


def test_a_strided_mask_is_copied():
    """Masks that are strided views (every second column of a wider tensor, a transposed tensor): same bits."""
    c = CASES["both_masks"]
    want, _ = run_case("both_masks", DEV)
    t, p = tensor(c["truth"]).to(DEV), tensor(c["pred"]).to(DEV)
    H, W = CHUNKS
    views = {}
    for k in ("valid", "occluded"):
        m = tensor(c[k]).to(DEV)
        wide = torch.ones(B, H, 2 * W, dtype=torch.bool, device=DEV)
        wide[:, :, ::2] = m
        views[k] = wide[:, :, ::2]
        assert not views[k].is_contiguous() and torch.equal(views[k], m)
    got = metrics.flow_quality(t, p, valid=views["valid"], occluded=views["occluded"], data_format="channels_last")
    assert same_bits(got, want)
    turned = {k: tensor(c[k]).to(DEV).transpose(1, 2).contiguous().transpose(1, 2) for k in ("valid", "occluded")}
    assert not turned["valid"].is_contiguous()
    got = metrics.flow_quality(t, p, valid=turned["valid"].view(torch.uint8), occluded=turned["occluded"],
                               data_format="channels_last")
    assert same_bits(got, want)


@pytest.mark.parametrize("byte", [2, 128, 255])
def test_any_nonzero_mask_byte_is_set(byte):
    """include/qpwc_flow_quality.h: a mask byte counts where it is nonzero.  uint8 masks holding 2, 128 or 255 where the
    case's masks hold 1 give the same bits, in both layouts."""
    for name in ("both_masks", "chunks_channels_first"):
        c = CASES[name]
        v, o = (tensor(CASES["both_masks"][k]).to(DEV).to(torch.uint8) * byte for k in ("valid", "occluded"))
        assert int(v.max()) == byte and int(o.max()) == byte and int(v.min()) == 0
        t, p = tensor(c["truth"]).to(DEV), tensor(c["pred"]).to(DEV)
        ones = tuple(tensor(CASES["both_masks"][k]).to(DEV) for k in ("valid", "occluded"))
        want = metrics.flow_quality(t, p, valid=ones[0], occluded=ones[1], data_format=c["data_format"])
        got = metrics.flow_quality(t, p, valid=v, occluded=o, data_format=c["data_format"])
        assert same_bits(got, want), name
    assert violations(want, reference("both_masks"))[0] == []          # the same flows in the other layout


def test_occluded_estimate_is_the_map_passed_explicitly():
    from qpwcnet_amd import occlusion
    t, p = (tensor(a * np.float32(0.05)).to(DEV) for a in make_flows(8, (9, 14)))     # up to about 3 px: some pixels stay
    the_map = occlusion.estimate_occlusion_map(t, "channels_last")
    assert tuple(the_map.shape) == (B, 9, 14) and 0 < int(the_map.sum()) < the_map.numel()
    got = metrics.flow_quality(t, p, occluded="estimate", data_format="channels_last")
    want = metrics.flow_quality(t, p, occluded=the_map, data_format="channels_last")
    assert same_bits(got, want) and bool(torch.isfinite(got.epe_occ).any())


def test_kernel_query_and_refusals():
    """Python refusals raise before anything is launched."""
    H, W = CHUNKS
    assert ops.flow_quality_kernel(B, H, W) == "flow_quality_tile_kernel"
    ok = torch.zeros(B, 4, 5, 2, device=DEV)
    with pytest.raises(ValueError, match="one shape"):
        metrics.flow_quality(ok, torch.zeros(B, 4, 6, 2, device=DEV))
    with pytest.raises(ValueError, match="valid must have shape"):
        metrics.flow_quality(ok, ok, valid=torch.ones(B, 5, 4, device=DEV))
    with pytest.raises(ValueError, match="occluded is on"):
        metrics.flow_quality(ok, ok, occluded=torch.ones(B, 4, 5))
    with pytest.raises(ValueError, match="accuracy"):
        metrics.flow_quality(ok, ok, accuracy=(3.0, 1.0, 5.0))
    with pytest.raises(ValueError, match="speed"):
        metrics.flow_quality(ok, ok, speed=(40.0, 10.0))
    with pytest.raises(ValueError, match="outlier"):
        metrics.flow_quality(ok, ok, outlier=(0.0, 0.05))
    with pytest.raises(ValueError, match="one device"):
        metrics.flow_quality(ok, ok.cpu())
    with pytest.raises(ValueError, match="state"):
        metrics.flow_quality(ok, ok, state=torch.zeros(17, dtype=torch.float64))
    with pytest.raises(ValueError, match="uint8"):
        ops.flow_quality(ok, ok, valid=torch.ones(B, 4, 5, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        ops.flow_quality(ok.half(), ok.half())
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.flow_quality(ok.cpu(), ok.cpu())
    assert all(f in metrics.FlowScores._fields for f in FIELDS) and BOUNDS["epe"] == 1e-4

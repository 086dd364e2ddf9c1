"""GPU suite of the evaluation-side kernels at the shapes where their loops iterate and their rarely taken forms run:
the flow metrics (csrc/flow_quality.hip) where flow_quality_fold_kernel walks more than one round of 16 images and more
than one trip of 64 chunks, and the masked flow losses (csrc/masked_loss.hip on the bodies of csrc/loss_common.h) in the
scalar backward, in sum plans with 1x2 / 2x1 steps, a 32x32 factor and ten steps, and on second trips of the pixel walk.
tests/test_gpu_flow_quality.py and tests/test_gpu_masked_loss.py hold the values at B = 2; every case there makes one
round, one trip and 2x2 steps.  The shapes and inputs live in tests/test_eval_scale_cpu.py, which proves from the
constants in the kernel sources that each still reaches the code it claims and runs the float64 oracles over them.

Flow metrics.  Oracle: ``ref_flow_quality`` / ``ref_sums`` in float64; bounds test_flow_quality_cpu.BOUNDS (count ratios
1 ulp of the float64 quotient, EPE-type means 1e-4 px, aae 1e-3 degrees; no valid pixel within 1e-3 of a threshold).
Beyond the bounds: which lane sums which pixel depends on the position inside the image only, and the fold adds the
images' doubles in image order, so row n of a batched launch is the image run alone bit for bit, and the 17 state values
are those of B one-image calls in image order on one state.
  fold_rounds   B = 35: two whole rounds of 16 waves and a third of 3 (the guard `n0 + w < B` keeps 13 stale rows out);
                3 chunks, odd width; every image its own content and error level; both masks; run twice into one state;
  fold_chunks   B = 3, 131 chunks: lanes 0..63 take three trips, the last one of 3 lanes; the last chunk under a wave;
                image 1's only s40+ and only occluded pixels lie in chunks >= 128;
  fold_both     B = 17, 65 chunks, channels-first, fp16 prediction.

Masked losses.  Oracle: ``loss.multiscale_masked_torch`` / ``masked_ground_truth_torch`` in float64 through
test_gpu_masked_loss._compare with its bounds (losses 1e-5 relative; fp32 gradients 1e-5 of the level's largest; fp16
gradients F16_EPS |g| + 1e-5 max + 2^-24; ground truth 1e-6 of the level's largest; masks and counts exact; gradients
exactly 0 at invalid level pixels).
  bwd_scalar           n % 4 == 2: masked_loss_bwd_kernel's scalar form, one trip and two; three kinds, fp32 and fp16;
  tile_plan            factors (2,16) (32,32) (1,4) (8,32) (2,8) -- eight steps -- and two ten-step plans on
                       masked_loss_tile_kernel; validity by tile: empty, one pixel in a corner or on an edge, full, 30 %;
                       all valid: the ground truth is ops.area_ground_truth's bit for bit;
  pixel_loop_area      3 x 3 blocks on masked_loss_pixel_kernel, 270,000 level pixels for 262,144 threads;
  pixel_loop_bilinear  renormalised corners at ratios 2, 2.5 and 1.875, two or three trips a level.
Measured on an MI355X: see the docstrings of the tests; test_zz_report_the_observed_errors prints the module's worst
case per quantity as a share of its bound (pytest -s).

What the module notices, tried once on an MI355X with three in-bounds defects built into the library: the fold kernel's
guard `n0 + w < B` removed (the state tests of all three flow cases and the layout test of fold_chunks fail), the count
plane's `n += qn` skipped on 2x1 steps (all twelve tile-plan tests fail), the scalar gradient loop ended after its first
trip (the twelve bwd_scalar cases of 401,598 elements fail, the twelve of 1,470 pass): 29 failed, 22 passed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_eval_scale_cpu import (FLOW_NAMES, MASKED, MASKED_KERNEL, MASKED_PARAMS,  # noqa: E402
                                 PLAN_FACTORS, ROUNDS_B, flow_case, flow_geometry, flow_reference, masked_inputs, masked_oracle,
                                 run_flow_case)
from test_flow_quality_cpu import check, check_state  # noqa: E402
from test_gpu_flow_quality import same_bits  # noqa: E402
from test_gpu_masked_loss import F16_EPS, WORST, _compare  # noqa: E402
from test_masked_loss_cpu import CODES, make_loss, to_layout  # noqa: E402

from qpwcnet_amd import loss, metrics, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_BATCHED = {}
SCALE_WORST = {}        # the largest observed error of this module per quantity, in units of its bound


def _batched(name):
    """The batched launch of a flow case (with a state of its own), run once -> (FlowScores, state)."""
    if name not in _BATCHED:
        state = torch.zeros(17, dtype=torch.float64, device=DEV)
        _BATCHED[name] = (run_flow_case(name, DEV, state=state), state)
    return _BATCHED[name]


# ---- flow metrics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FLOW_NAMES))
def test_flow_metrics_match_float64_where_the_fold_loops_iterate(name):
    """Every field of every image against ref_flow_quality.  Measured on an MI355X: the EPE-type means at most
    1.0e-6 px (0.010 of the bound; fold_rounds), aae 2.1e-6 degrees (0.002; fold_rounds), every count ratio the rounded
    float64 quotient (at most 0.5 ulp)."""
    Bn, H, W, chunks = flow_geometry(name)
    assert ops.flow_quality_kernel(Bn, H, W) == "flow_quality_tile_kernel"
    res, _ = _batched(name)
    assert all(v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (Bn,) for v in res)
    check("hip " + name, res, flow_reference(name)[0])


@pytest.mark.parametrize("name", list(FLOW_NAMES))
def test_batched_rows_and_state_are_the_one_image_calls_bit_for_bit(name):
    """out[:, n] of the batched launch against image n run alone, and the 17 state values against those of the B
    one-image calls made in image order on one state: the same doubles added in the same order."""
    Bn = flow_geometry(name)[0]
    res, state = _batched(name)
    one_state = torch.zeros(17, dtype=torch.float64, device=DEV)
    for n in range(Bn):
        one = run_flow_case(name, DEV, images=slice(n, n + 1), state=one_state)
        assert same_bits([v[n:n + 1] for v in res], one), (name, n)
    assert torch.equal(state, one_state), (name, (state - one_state).tolist())
    assert float(state[15]) == Bn and float(state[0]) == float(flow_reference(name)[1][:, 0].sum())
    # with and without a state, out is the same
    assert same_bits(res, run_flow_case(name, DEV))


def test_fold_rounds_twice_into_one_state():
    """Two calls of B = 35 through one FlowQuality: 70 images in image order against the float64 sums, the
    pixel-weighted result, and bit for bit the state of the 70 one-image calls."""
    Bn, H, W, _ = flow_geometry("fold_rounds")
    c = flow_case("fold_rounds")
    args = [torch.from_numpy(np.array(c[k])).to(DEV) for k in ("truth", "pred", "valid", "occluded")]
    m = metrics.FlowQuality(data_format="channels_last")
    per = [m.update_state(args[0], args[1], valid=args[2], occluded=args[3]) for _ in range(2)]
    assert m.state.is_cuda and same_bits(per[0], per[1]) and same_bits(per[0], _batched("fold_rounds")[0])
    singles = metrics.FlowQuality(data_format="channels_last")
    for _ in range(2):
        for n in range(Bn):
            singles.update_state(args[0][n:n + 1], args[1][n:n + 1], valid=args[2][n:n + 1], occluded=args[3][n:n + 1])
    assert torch.equal(m.state, singles.state)
    sums = flow_reference("fold_rounds")[1]
    check_state(m, per, np.concatenate([sums, sums]), H * W, images=2 * ROUNDS_B)


@pytest.mark.parametrize("name", list(FLOW_NAMES))
def test_both_layouts_give_the_same_bits(name):
    c = flow_case(name)
    other = "channels_first" if c["data_format"] == "channels_last" else "channels_last"
    perm = (0, 3, 1, 2) if other == "channels_first" else (0, 2, 3, 1)
    t, p = (torch.from_numpy(np.array(c[k])).permute(*perm).contiguous().to(DEV) for k in ("truth", "pred"))
    v, o = (torch.from_numpy(np.array(c[k])).to(DEV) for k in ("valid", "occluded"))
    state = torch.zeros(17, dtype=torch.float64, device=DEV)
    got = metrics.flow_quality(t, p, valid=v, occluded=o, data_format=other, state=state)
    res, want_state = _batched(name)
    assert same_bits(got, res) and torch.equal(state, want_state)


# ---- masked losses ----------------------------------------------------------------------------------------------------
def _measured(tag, *args):
    """_compare, with the case's own worst error per quantity as a share of its bound printed (pytest -s) and kept in
    SCALE_WORST; test_gpu_masked_loss.WORST, that module's own record, is left as it was."""
    before = dict(WORST)
    WORST.clear()
    try:
        out = _compare(*args, tag)
        print("masked {}: ".format(tag) + ", ".join("{} {:.3f}".format(k, v) for k, v in sorted(WORST.items())))
        for k, v in WORST.items():
            SCALE_WORST[k] = max(SCALE_WORST.get(k, 0.0), v)
    finally:
        WORST.clear()
        WORST.update(before)
    return out


def _tensors(name, index, kind, data_format, dtype):
    gt, valid, preds = masked_inputs(name, index, kind)
    return to_layout(gt.numpy(), data_format, torch.float32), [to_layout(p.numpy(), data_format, dtype) for p in preds], valid


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("name,index,kind", [p for p in MASKED_PARAMS if p[0] == "bwd_scalar"])
def test_masked_backward_scalar_form(name, index, kind, data_format, dtype):
    """n = B * h * w * 2 with n % 4 == 2, 1,470 elements (one trip) and 401,598 (past one trip of 1024 x 256): every
    bound of _compare, and a gradient 1/16 too large must miss the fp16 bound.  Measured on an MI355X, worst of the 24
    cases as a share of the bound: losses 0.007, fp32 gradients 0.064, fp16 gradients 0.974 (the half ulp of fp16
    itself), ground truth 0.059."""
    B, H, W, shapes = MASKED[name][index]
    assert ops.masked_loss_kernel(CODES[kind], B, H, W, shapes) == MASKED_KERNEL[name] == "masked_loss_pixel_kernel"
    gt, preds, valid = _tensors(name, index, kind, data_format, dtype)
    assert all(p.numel() % 4 == 2 for p in preds)
    per, counts, grads = _measured((name, index, kind, data_format), make_loss(kind, data_format), gt, preds, valid, dtype)
    assert all(g.numel() % 4 != 0 and g.dtype == dtype for g in grads)
    if dtype == torch.float16:
        _, _, ref_g, _ = masked_oracle(name, index, kind, 2.0 ** 16)
        for g, rg in zip(grads, ref_g):
            got = (g.permute(0, 2, 3, 1) if data_format == "channels_first" else g).double().cpu()
            bad = rg * (1 + 1 / 16)
            bound = F16_EPS * bad.abs() + 1e-5 * float(rg.abs().max()) + 2.0 ** -24
            assert not bool(((got - bad).abs() <= bound).all())


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("plan", list(PLAN_FACTORS))
def test_masked_tile_plans_with_unequal_steps(plan, data_format):
    """The count plane through 1x2 and 2x1 steps, a 32x32 factor (one level pixel a tile, n up to 1024), levels not in
    area order, and ten steps; validity by tile (tests/test_eval_scale_cpu.py holds what each tile is).  Counts exact.
    Measured on an MI355X, worst share of the bound: losses 0.009, fp32 gradients 0.018, ground truth 0.084."""
    index = list(PLAN_FACTORS).index(plan)
    B, H, W, shapes = MASKED["tile_plan"][index]
    assert ops.masked_loss_kernel(CODES["v2"], B, H, W, shapes) == "masked_loss_tile_kernel"
    gt, preds, valid = _tensors("tile_plan", index, "v2", data_format, torch.float32)
    per, counts, _ = _measured((plan, data_format), make_loss("v2", data_format), gt, preds, valid, torch.float32)
    assert torch.equal(counts.cpu(), masked_oracle("tile_plan", index, "v2")[1])
    assert all(0 < c < B * h * w for c, (h, w) in zip(counts.tolist(), shapes) if (H // h) * (W // w) < 1024)


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("plan", list(PLAN_FACTORS))
def test_all_valid_tile_ground_truth_is_the_dense_kernels_bit_for_bit(plan, data_format):
    """loss_common.h: "for a full block (n a power of two) h / H / n is exact and the product is the dense branch's, bit
    for bit" -- with no mask and with a mask of ones, on the plans with unequal steps."""
    index = list(PLAN_FACTORS).index(plan)
    B, H, W, shapes = MASKED["tile_plan"][index]
    gen = torch.Generator().manual_seed(77 + index)
    gt = to_layout((torch.randn(B, H, W, 2, generator=gen) * 4.0).numpy(), data_format, torch.float32).to(DEV)
    obj = make_loss("v2", data_format)
    dense = ops.area_ground_truth(gt, shapes, data_format)
    for valid in (None, torch.ones(B, H, W, dtype=torch.bool, device=DEV)):
        gts, masks = loss.masked_ground_truth(obj, gt, shapes, valid)
        for l, (g, d, m) in enumerate(zip(gts, dense, masks)):
            assert g.shape == d.shape and torch.equal(g, d.contiguous()), (plan, l)
            assert bool((m == 1).all())
    assert float(dense[0].abs().max()) > 0


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("name", ["pixel_loop_area", "pixel_loop_bilinear"])
def test_masked_pixel_walks_take_a_second_trip(name, data_format):
    """The area walk (the sh x sw loop with the per-pixel validity and the integer count) and the down-sampling bilinear
    walk with renormalised corners, past one trip of the grid.  Measured on an MI355X, worst share of the bound: losses
    0.003, fp32 gradients 0.152, ground truth 0.121 (both on the bilinear row)."""
    kind = "v2" if name == "pixel_loop_area" else "mse"
    B, H, W, shapes = MASKED[name][0]
    assert ops.masked_loss_kernel(CODES[kind], B, H, W, shapes) == "masked_loss_pixel_kernel"
    gt, preds, valid = _tensors(name, 0, kind, data_format, torch.float32)
    _, counts, _ = _measured((name, data_format), make_loss(kind, data_format), gt, preds, valid, torch.float32)
    assert all(0 < c < B * h * w for c, (h, w) in zip(counts.tolist(), shapes))


def test_zz_report_the_observed_errors():
    """The largest error of this module's masked-loss cases per quantity, as a share of its bound (pytest -s shows it).
    Measured on an MI355X: losses 0.009, fp32 gradients 0.152, fp16 gradients 0.974, ground truth 0.121."""
    print("\nmasked loss at scale, worst observed / bound: " + ", ".join("{} {:.3f}".format(k, v) for k, v in sorted(SCALE_WORST.items())))
    assert all(v <= 1.0 for v in SCALE_WORST.values())

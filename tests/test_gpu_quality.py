"""GPU suite of the interpolator's image quality (qpwcnet_amd.metrics.image_quality on qpwc_image_quality_fwd).

Oracle: ``ref_quality``, the float64 restatement in tests/test_quality_cpu.py (the fp32 torch composition meets the same
bounds there).  Bounds (BOUNDS): ssim 1e-4 absolute, mse 1e-5 relative, psnr 1e-4 dB absolute.  B = 2 throughout; the two
images of a batch differ in content and in error level, so a batch-index mix-up shows.  The cases (CASES, sized by
_hip.QUALITY_TILE = TH x TW SSIM positions per workgroup) and what each is chosen for:
  11x11                  one SSIM position per channel and image;
  12x27                  less than one tile, odd in both extents;
  tiles                  (TH + 11) x (2 TW + 13): two tile rows and three tile columns, the last ones partial (one row and
                         three columns of positions); a bright patch centred on the last position, a single large error
                         at pixel (0, 0) and at (H - 1, W - 1): a dropped last tile shows in ssim, a rim pixel that is
                         dropped or counted twice in mse (test_quality_cpu.py::test_the_comparison_sees_the_planted_defects);
  c1, c4                 one and four channels at 12 x 27;
  tiles_channels_first, tiles_f16_truth, tiles_f16_pred      the other layout; fp16 against fp32, either way round;
  clip, quantize         offsets (0.5, 0.5) on images in [-0.5, 0.5]; for quantize no element lies within 1e-3 of an
                         8-bit step, so no element is left out of the comparison.
Measured on an MI355X: see the docstrings of the tests and DESIGN.md section 4.23."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_quality_cpu import (B, BOUNDS, CASES, CONSTANTS, TH, TILES, TW, check, near_a_step, reference,  # noqa: E402
                              run_case, tensor)

from qpwcnet_amd import metrics, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def assert_property(name):
    """What the case is chosen for, before it runs."""
    c = CASES[name]
    shape = c["truth"].shape
    H, W, C = (shape[1], shape[2], shape[3]) if c["data_format"] == "channels_last" else (shape[2], shape[3], shape[1])
    tiles = (-(-(H - 10) // TH), -(-(W - 10) // TW))
    assert shape[0] == B
    if name == "11x11":
        assert (H - 10) * (W - 10) == 1 and C == 3
    elif name in ("12x27", "c1", "c4"):
        assert tiles == (1, 1) and H % 2 == 0 and W % 2 == 1 and (H - 10) < TH and (W - 10) < TW
        assert C == {"12x27": 3, "c1": 1, "c4": 4}[name]
    else:
        assert (H, W) == TILES and tiles == (2, 3) and (H - 10) % TH == 1 and (W - 10) % TW == 3 and C == 3
    if name == "tiles_channels_first":
        assert c["data_format"] == "channels_first"
    if name.startswith("tiles_f16"):
        assert {c["truth"].dtype, c["pred"].dtype} == {np.dtype(np.float16), np.dtype(np.float32)}
    if name == "clip":
        t = c["truth"].astype(np.float64) + 0.5
        assert c["kw"] == dict(offset=(0.5, 0.5), clip=True) and 0.02 < float(((t < 0) | (t > 1)).mean()) < 0.5
    if name == "quantize":
        assert c["kw"] == dict(offset=(0.5, 0.5), quantize=True)
        assert not near_a_step(c["truth"], 0.5).any() and not near_a_step(c["pred"], 0.5).any()


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_the_float64_restatement(name):
    """Every case against ref_quality.  Measured on an MI355X, the largest error over the ten cases: ssim 3.8e-7 (11x11),
    mse 6.7e-8 relative (tiles), psnr 1.1e-6 dB (c4) -- the rounding of the fp32 results; the torch composition on the
    CPU is at 3.8e-7, 4.5e-8 and 8.8e-7."""
    assert_property(name)
    res, got = run_case(name, DEV)
    assert isinstance(res, metrics.ImageQuality) and all(v.is_cuda and v.dtype == torch.float32 for v in res)
    assert all(tuple(v.shape) == (B,) for v in res) and all(np.isfinite(g).all() for g in got)
    check("hip " + name, got, reference(name))
    # the launcher gives three views of one tensor
    assert res.psnr.data_ptr() == res.mse.data_ptr() + 4 * B and res.ssim.data_ptr() == res.mse.data_ptr() + 8 * B


@pytest.mark.parametrize("a,b,max_val", CONSTANTS)
def test_constant_images(a, b, max_val):
    """The closed form, independent of the restatement: ssim = (2ab + c1) / (a^2 + b^2 + c1), mse = (a - b)^2.  Measured
    on an MI355X: ssim 1.6e-5 for 0.3 against 0.4 (den1 - den0 cancels against c2: the worst kind of input), 1.7e-8 for
    0.1 against 0.2, 1.5e-8 for 90 against 120; mse at most 4.1e-8 relative, psnr at most 5.2e-7 dB."""
    t, p = (torch.full((B, TILES[0], TILES[1], 3), v, device=DEV) for v in (a, b))
    a, b = float(np.float32(a)), float(np.float32(b))
    c1 = (0.01 * max_val) ** 2
    want = (np.full(B, (a - b) ** 2), np.full(B, 20 * np.log10(max_val) - 20 * np.log10(abs(a - b))),
            np.full(B, (2 * a * b + c1) / (a * a + b * b + c1)))
    got = metrics.image_quality(t, p, max_val=max_val, data_format="channels_last")
    check("hip constant {:g} {:g}".format(a, b), [v.cpu().numpy() for v in got], want)


def test_truth_is_pred():
    """One buffer for both images: mse 0, psnr +inf, ssim 1 to the bound.  Measured on an MI355X: |ssim - 1| = 0."""
    t = tensor(CASES["tiles"]["truth"]).to(DEV)
    res = metrics.image_quality(t, t, data_format="channels_last")
    assert bool((res.mse == 0).all()) and bool(torch.isinf(res.psnr).all()) and bool((res.psnr > 0).all())
    err = float((res.ssim - 1).abs().max())
    print("hip truth is pred: |ssim - 1| {:.2e}".format(err))
    assert err <= BOUNDS["ssim"]


def test_state_accumulates_in_image_order():
    """Two calls on different batches with one state: the count is 2 B and each sum is the float64 running sum of the
    two outs, in order; without a state, out is the same bit for bit."""
    state = torch.zeros(4, dtype=torch.float64, device=DEV)
    outs = []
    for name in ("tiles", "quantize"):
        c = CASES[name]
        t, p = tensor(c["truth"]).to(DEV), tensor(c["pred"]).to(DEV)
        with_state = metrics.image_quality(t, p, data_format=c["data_format"], state=state, **c["kw"])
        without = metrics.image_quality(t, p, data_format=c["data_format"], **c["kw"])
        assert all(torch.equal(a, b) for a, b in zip(with_state, without))
        outs.append(with_state)
    got = state.cpu()
    assert float(got[3]) == 2 * B
    for i in range(3):
        want = torch.cumsum(torch.cat([outs[0][i], outs[1][i]]).double().cpu(), 0)[-1]
        assert abs(float(got[i]) - float(want)) <= 1e-12 * abs(float(want)), (i, float(got[i]), float(want))
    m = metrics.InterpolationQuality(data_format="channels_last")
    c = CASES["quantize"]
    per = m.update_state(tensor(c["truth"]).to(DEV), tensor(c["pred"]).to(DEV))
    assert m.state.is_cuda and all(torch.equal(a, b) for a, b in zip(per, outs[1]))
    res = m.result()
    assert all(abs(res[k] - float(v.double().mean())) <= 1e-12 * abs(res[k]) for k, v in zip(("mse", "psnr", "ssim"), per))
    m.reset_state()
    assert m.result() == {"mse": 0.0, "psnr": 0.0, "ssim": 0.0}


def test_two_runs_are_bitwise_equal():
    a, _ = run_case("tiles", DEV)
    b, _ = run_case("tiles", DEV)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the layout decides which lane sums which squared error, not what reaches LDS: ssim is the same bit for bit
    cf, _ = run_case("tiles_channels_first", DEV)
    assert torch.equal(a.ssim, cf.ssim)


def test_kernel_query_and_refusals():
    H, W = TILES
    run_case("tiles", DEV)
    assert ops.image_quality_kernel(B, H, W, 3) == "quality_tile_kernel"
    small = torch.zeros(B, 10, 64, 3, device=DEV)
    with pytest.raises(ValueError, match="at least 11"):
        ops.image_quality(small, small)
    with pytest.raises(ValueError, match="filter size"):
        metrics.image_quality(small, small, data_format="channels_last")
    ok = torch.zeros(B, 11, 11, 3, device=DEV)
    with pytest.raises(ValueError, match="one device"):
        metrics.image_quality(ok, ok.cpu())
    with pytest.raises(ValueError, match="state"):
        metrics.image_quality(ok, ok, state=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.image_quality(ok.cpu(), ok.cpu())

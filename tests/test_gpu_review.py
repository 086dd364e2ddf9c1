"""GPU suite of the inference review panels (qpwcnet_amd.vis inference_panels / interpolation_panels on
qpwc_inference_panels_fwd / qpwc_interpolation_panels_fwd, include/qpwc_review.h).

Oracle, fixtures and comparison helpers: tests/test_review_cpu.py -- the float64 restatement of both scripts, flows that
keep every sample coordinate 1e-3 away from tf_warp's two discontinuities, and ``float_error`` / ``uint8_share``; the fp32
torch composition meets the same assertions there.  Bound: 1e-4, the project's kernel bound.

B = 2.  Set 1 at 33 x 70 (2310 pixels: more than one max-tile of _hip.VIS_MAX_TILE, no multiple of it and none of 4:
<scalar>; ten panel tiles of _hip.REVIEW_TILE per image, the last partial; grid lines at rows 0, 32 and columns 0, 32,
64) and at 32 x 68 (<vec4>, the last tile partial); image 0's largest flow vector sits in the last, partial max-tile and
image 1's in the first.  Set 2 at 34 x 70 with a 17 x 35 flow (s = 2, an odd-sized flow picture: <scalar>), at 36 x 72
with 18 x 36 (<vec4>) and at 20 x 36 with s = 1.  Measured on an MI355X: see the docstrings of the tests."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_review_cpu import (B, BOUND, FORMATS, KERNELS, SET1, SET2, as_half, float_error, ref_flow_to_image,  # noqa: E402
                             ref_inference_panels, ref_interpolation_panels, ref_tf_warp, ref_upflow, reference,
                             run_panels, set1_case, set2_case, uint8_share)

from qpwcnet_amd import _hip, layers, ops, synth, vis, warp  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dev = lambda a: torch.from_numpy(np.array(a, order="C")).to(DEV)
CASES = [(1, f) for f in SET1] + [(2, f) for f in SET2]
case_of = lambda set_no, form: (set1_case if set_no == 1 else set2_case)(form)


def kernel_of(set_no, form, dtype=torch.float32, out_format="channels_last"):
    if set_no == 1:
        return ops.review_panels_kernel(2, B, *SET1[form], out_dtype=dtype, out_layout=out_format)
    (H, W), s = SET2[form]
    return ops.review_panels_kernel(1, B, H, W, H // s, W // s, dtype, out_format)


@pytest.mark.parametrize("grid", [0, 32])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("out_format", FORMATS)
@pytest.mark.parametrize("in_format", FORMATS)
@pytest.mark.parametrize("set_no,form", CASES)
def test_kernels_match_the_float64_restatement(set_no, form, in_format, out_format, half, grid):
    """Every element of every picture.  Measured on an MI355X: max |err| 4.4e-6 over the 80 cases (6-warp at s = 2); the torch
    composition on the CPU is at 4.4e-6."""
    case = case_of(set_no, form)
    outs, got = run_panels(set_no, as_half(case) if half else case, in_format, out_format, torch.float32, grid, DEV)
    assert kernel_of(set_no, form, torch.float32, out_format) == KERNELS[form]
    err = float_error(got, reference(set_no, form, half, grid))
    print("review set {} {} {}->{} {} grid {}: max |err| {:.3e}".format(set_no, form, in_format, out_format,
                                                                        "f16" if half else "f32", grid, err))
    assert err <= BOUND
    assert all(o.is_contiguous() and o.dtype == torch.float32 for o in outs.values())
    if set_no == 1 and grid == 0:
        # flo is normalised by the planted maxima (image 0's sits in the partial max-tile): fully saturated there
        assert got["flo_rgb"][0, -1, -1].min() < 1e-6 and got["flo_rgb"][1, 0, 3].min() < 1e-6


@pytest.mark.parametrize("grid", [0, 32])
@pytest.mark.parametrize("out_format", FORMATS)
@pytest.mark.parametrize("in_format", FORMATS)
@pytest.mark.parametrize("set_no,form", CASES)
def test_uint8_pictures(set_no, form, in_format, out_format, grid):
    """uint8 against the exported float64 pictures: at most one level off, and only at eligible elements (uint8_share);
    those are at most 1 % of a set (0.15-0.72 %: a property of the restatement).  Measured on an MI355X: at most 3 elements of a set one level off, all eligible."""
    outs, got = run_panels(set_no, case_of(set_no, form), in_format, out_format, torch.uint8, grid, DEV)
    assert kernel_of(set_no, form, torch.uint8, out_format) == KERNELS[form]
    share = uint8_share(got, reference(set_no, form, False, grid), grid)
    off = sum(int((got[k] != np.trunc(255 * np.clip(r, 0, 1))).sum()) for k, r in reference(set_no, form, False, grid).items())
    print("review uint8 set {} {} {}->{} grid {}: {:.3f} % eligible, {} elements one level off".format(
        set_no, form, in_format, out_format, grid, 100.0 * share, off))
    assert share <= 0.01
    assert all(o.is_contiguous() and o.dtype == torch.uint8 for o in outs.values())


def test_negative_controls():
    """The comparison tells apart: flo and flo_pred swapped (nxt_w moves by far more than BOUND), the factor s dropped
    from 6-warp, and image 0's planted maximum zeroed (the rest of image 0's flow picture changes, image 1's does not)."""
    c = set1_case("scalar")
    want = reference(1, "scalar", False, 0)
    _, got = run_panels(1, c, device=DEV)
    _, swapped = run_panels(1, dict(c, flo=c["flo_pred"], flo_pred=c["flo"]), device=DEV)
    assert float(np.abs(swapped["nxt_w"] - want["nxt_w"]).max()) > 1000 * BOUND
    assert float(np.abs(swapped["nxt_w"] - ref_inference_panels(c["ims"], c["flo_pred"], c["flo"])["nxt_w"]).max()) <= BOUND
    c2 = set2_case("scalar")
    _, got2 = run_panels(2, c2, device=DEV)
    unscaled = ref_tf_warp(c2["img1"], ref_upflow(c2["flow"], 2) / 2.0)
    assert float(np.abs(got2["6-warp"] - unscaled).max()) > 1000 * BOUND
    cut = c["flo"].copy()
    cut[0, -1, -1] = 0.0
    other = ref_flow_to_image(cut)
    assert float(np.abs(got["flo_rgb"][0, :-1] - other[0, :-1]).max()) > 1000 * BOUND
    assert float(np.abs(got["flo_rgb"][1] - other[1]).max()) <= BOUND                 # image 1 keeps its own
    _, got_cut = run_panels(1, dict(c, flo=cut), device=DEV)
    assert float(np.abs(got_cut["flo_rgb"] - other).max()) <= BOUND


def test_two_calls_are_bitwise_equal():
    """Two runs are bit-identical; the pictures do not depend on the input or output layout or on the store form."""
    for set_no, form in CASES:
        case = case_of(set_no, form)
        for dtype in (torch.float32, torch.uint8):
            a, _ = run_panels(set_no, case, dtype=dtype, grid=32, device=DEV)
            b, _ = run_panels(set_no, case, dtype=dtype, grid=32, device=DEV)
            assert all(torch.equal(a[k], b[k]) for k in a)
            c, _ = run_panels(set_no, case, "channels_first", "channels_first", dtype, 32, DEV)
            assert all(torch.equal(a[k], c[k].permute(0, 2, 3, 1)) for k in a)
            d, _ = run_panels(set_no, case, "channels_last", "channels_first", dtype, 32, DEV)
            assert all(torch.equal(c[k], d[k]) for k in c)
    # <vec4> and <scalar> write the same bits: the pictures without a gather, on a window of the same images
    c = set1_case("vec4")
    full, _ = run_panels(1, c, device=DEV)                                              # 32 x 68: <vec4>
    odd = {k: np.ascontiguousarray(v[:, :31, :67]) for k, v in c.items()}              # 31 x 67 = 2077: <scalar>
    assert ops.review_panels_kernel(2, B, 31, 67) == KERNELS["scalar"]
    part, _ = run_panels(1, odd, device=DEV)
    for k in ("prv", "nxt", "overlay"):
        assert torch.equal(full[k][:, :31, :67], part[k])


def test_graph_replay_follows_the_inputs():
    """Captured once on a side stream, replayed after the inputs changed in place: the pictures follow the new flows and
    their maxima, so no value went through the host and the workspace carries nothing from one run to the next.  The
    graph is linear: two launches, one after the other."""
    first, second = set1_case("vec4"), set1_case("vec4", seed=1)
    ts = {k: dev(v) for k, v in first.items()}
    call = lambda: vis.inference_panels(ts["ims"], ts["flo"], ts["flo_pred"], "channels_last", torch.float32, 32,
                                        "channels_first")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = call()
    for values in (first, second, second, first):
        for k, t in ts.items():
            t.copy_(dev(values[k]))
        graph.replay()
        torch.cuda.synchronize()
        want = ref_inference_panels(grid=32, **values)
        got = {k: o.permute(0, 2, 3, 1).cpu().numpy() for k, o in outs.items()}
        assert float_error(got, want) <= BOUND
    eager = call()
    assert all(torch.equal(outs[k], eager[k]) for k in outs)                            # bit for bit what eager gives


def test_inference_panels_of_the_model():
    """test_infer.py's pictures for layers.FlowerModel at 64 x 64: shapes, dtypes and contiguity, equality with the
    per-piece path (warp.tf_warp, vis.flow_to_image, torch arithmetic) within BOUND, and pictures, not flat fields."""
    hw = (64, 64)
    net = layers.FlowerModel(data_format="channels_last")
    net.load_state_dict({k: torch.as_tensor(v) for k, v in synth.make_weights(42, hw).items()})
    net = net.to(DEV).eval()
    pairs, label = synth.make_frames(B, hw[0], hw[1], seed=5)
    ims, flo = dev(pairs), dev(label)
    with torch.no_grad():
        flo_pred = net(ims)[-1]
    assert tuple(flo_pred.shape) == (B,) + hw + (2,)
    panels = vis.inference_panels(ims, flo, flo_pred)
    assert list(panels) == list(vis.INFERENCE_PANELS)
    prv, nxt = 0.5 + ims[..., 0:3], 0.5 + ims[..., 3:6]
    nxt_w = 0.5 + warp.tf_warp(ims[..., 3:6].contiguous(), flo_pred, "channels_last")
    nxt_w_gt = 0.5 + warp.tf_warp(ims[..., 3:6].contiguous(), flo, "channels_last")
    pieces = [prv, nxt, nxt_w, 0.5 * prv + 0.5 * nxt, 0.5 * prv + 0.5 * nxt_w, 0.5 * prv + 0.5 * nxt_w_gt,
              (0.5 * prv - 0.5 * nxt_w).abs(), (0.5 * prv - 0.5 * nxt_w_gt).abs(), vis.flow_to_image(flo),
              vis.flow_to_image(flo_pred)]
    for (name, p), want in zip(panels.items(), pieces):
        assert p.dtype == torch.float32 and tuple(p.shape) == (B,) + hw + (3,) and p.is_contiguous(), name
        assert float((p - want).abs().max()) <= BOUND, name
        assert float(p.std()) > 1e-3, name                                              # a picture, not a flat field
    u8 = vis.inference_panels(ims, flo, flo_pred, dtype=torch.uint8, grid=32)
    for name, p in u8.items():
        assert p.dtype == torch.uint8 and tuple(p.shape) == (B,) + hw + (3,) and p.is_contiguous()
        assert bool((p[:, ::32] == 255).all()) and bool((p[:, :, ::32] == 255).all())
        want = vis.export_uint8(panels[name])
        inner = torch.ones_like(p, dtype=torch.bool)
        inner[:, ::32] = False
        inner[:, :, ::32] = False
        assert torch.equal(p[inner], want[inner]), name
    half = vis.inference_panels(ims.half(), flo.half(), flo_pred)                        # fp16 flows are widened
    assert float((half["nxt"] - (0.5 + ims.half().float()[..., 3:6])).abs().max()) == 0.0


def test_interpolation_panels_of_the_model():
    """pre_train_test.py's pictures for layers.InterpolatorModel at 64 x 64 with its flow one level below full
    resolution (s = 2): against the per-piece path within BOUND."""
    hw = (64, 64)
    net = layers.InterpolatorModel(data_format="channels_last", output_multiscale=False)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in synth.make_interpolator_weights(42, hw).items()})
    net = net.to(DEV).eval()
    pairs, _ = synth.make_frames(B, hw[0], hw[1], seed=7)
    img_pair = dev(pairs)
    img1 = (0.5 + 0.5 * (img_pair[..., 0:3] + img_pair[..., 3:6])).contiguous()
    with torch.no_grad():
        pred = net(img_pair)
        # the script's flow_model: the forward flow of the finest estimated level, as the model's own stack computes it
        n, _, feats, decs = net._pyramids(img_pair)
        flow = net._flow_stack(feats[-1][n:], feats[-1][:n], [d[n:] for d in decs], [d[:n] for d in decs])[-1]
        flow = flow.float().contiguous()
    assert tuple(pred.shape) == (B,) + hw + (3,) and tuple(flow.shape) == (B, 32, 32, 2)
    panels = vis.interpolation_panels(img_pair, img1, pred, flow, grid=0)
    assert list(panels) == list(vis.INTERPOLATION_PANELS)
    prv, nxt = 0.5 + img_pair[..., 0:3], 0.5 + img_pair[..., 3:6]
    upflow = 2.0 * flow.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    pieces = [prv, nxt, img1, 0.5 + pred, 0.5 * prv + 0.5 * nxt, vis.flow_to_image(flow),
              warp.tf_warp(img1, upflow.contiguous(), "channels_last")]
    for (name, p), want in zip(panels.items(), pieces):
        size = (32, 32) if name == "5-flow" else hw
        assert p.dtype == torch.float32 and tuple(p.shape) == (B,) + size + (3,) and p.is_contiguous(), name
        assert float((p - want).abs().max()) <= BOUND, name
        assert float(p.std()) > 1e-3, name
    shown = vis.interpolation_panels(img_pair, img1, pred, flow, dtype=torch.uint8)      # the script: grid 32, 8-bit
    for name, p in shown.items():
        assert p.dtype == torch.uint8 and bool((p[:, ::32] == 255).all()) and bool((p[:, :, ::32] == 255).all())


def test_form_query():
    for set_no, form in CASES:
        for dtype in (torch.float32, torch.uint8):
            for out_format in FORMATS:
                assert kernel_of(set_no, form, dtype, out_format) == KERNELS[form]
    assert ops.review_panels_kernel(2, 8, 256, 512) == "review_panels_kernel<vec4>"
    assert ops.review_panels_kernel(1, B, 34, 70, 17, 36) == "" and _hip.REVIEW_TILE == 256

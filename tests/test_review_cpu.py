"""The inference review panels (qpwcnet_amd/vis.py inference_panels / interpolation_panels, include/qpwc_review.h)
without a GPU:
  * ``ref_inference_panels`` / ``ref_interpolation_panels``: a float64 numpy restatement written from
    qpwcnet/app/optical_flow/test_infer.py:104-154, qpwcnet/app/frame_interpolation/pre_train_test.py:45-79, 121-163 and
    qpwcnet/core/warp.py:100-151 -- the contract the kernels are held to (tests/test_gpu_review.py imports it, with the
    fixtures and the two comparison helpers below);
  * the fp32 torch compositions, the path CPU tensors take, against every assertion the GPU suite makes, on the same
    fixtures, and against known answers.
Bound: 1e-4, the project's kernel bound (BOUND of test_augment_cpu.py).  Every image value is in [-0.5, 1] and a flow in
N(0, 3^2) with planted vectors of whole numbers; tf_warp's raw weights grow with the distance a sample leaves the image by
(up to 15 x 15 for these flows), so its fp32 sum carries up to about 2^-24 * 4 * 225 * 0.5 = 2.7e-5.

Fixture condition (``checked_flow``).  tf_warp is discontinuous where a sample coordinate crosses -1 or W-1 (H-1) and
continuous at every other whole number, so a coordinate that fp32 rounds to the other side of one of those would show a
difference that is no error.  No sample coordinate of a fixture, in float64 from the fp32 flow, lies within 1e-3 of -1,
W-1 or H-1 unless it IS that value (then the fp32 sum of two small whole numbers is as exact); the generator re-seeds
until that holds, and asserts that more than 5 % of the samples leave the image, so the rim is exercised.  With this no
element is left out of a comparison."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import BOUND  # noqa: E402
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402
from test_vis_cpu import FORMATS, ref_flow_to_image, to_layout  # noqa: E402

from oracle import np_ref  # noqa: E402
from qpwcnet_amd import _hip, vis  # noqa: E402

REVIEW_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qpwc_review.h")
B = 2
MARGIN = 1e-3


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_tf_warp(img, flow, dtype=np.float64):
    """warp.py:100-151 on channels-last arrays, in `dtype`: x = X + fx, y = Y + fy; corners by truncation toward zero,
    then clipped; raw weights from the clipped corners; wa Ia + wb Ib + wc Ic + wd Id in that order."""
    img, flow = np.asarray(img, dtype), np.asarray(flow, dtype)
    n, H, W, _ = img.shape
    gx, gy = np.meshgrid(np.arange(W), np.arange(H))
    x, y = gx[None].astype(dtype) + flow[..., 0], gy[None].astype(dtype) + flow[..., 1]
    x0, y0 = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1, y0, y1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1), np.clip(y0, 0, H - 1), np.clip(y1, 0, H - 1)
    b = np.arange(n).reshape(-1, 1, 1)
    Ia, Ib, Ic, Id = img[b, y0, x0], img[b, y1, x0], img[b, y0, x1], img[b, y1, x1]
    x0f, x1f, y0f, y1f = (v.astype(dtype) for v in (x0, x1, y0, y1))
    wa, wb = ((x1f - x) * (y1f - y))[..., None], ((x1f - x) * (y - y0f))[..., None]
    wc, wd = ((x - x0f) * (y1f - y))[..., None], ((x - x0f) * (y - y0f))[..., None]
    return wa * Ia + wb * Ib + wc * Ic + wd * Id


def ref_grid(img, g):
    """_show, pre_train_test.py:54-59, on a channels-last batch."""
    img = img.copy()
    if g:
        img[:, :, ::g, :] = 1.0
        img[:, ::g, :, :] = 1.0
    return img


def ref_export_uint8(img):
    """_show's export, pre_train_test.py:65-70."""
    return (255 * np.clip(np.asarray(img, np.float64), 0.0, 1.0)).astype(np.uint8)


def ref_inference_panels(ims, flo, flo_pred, grid=0):
    """test_infer.py:104-154: channels-last numbers -> {name: float64 (B,H,W,3)}, in the script's order."""
    ims = np.asarray(ims, np.float64)
    prv, nxt = ims[..., 0:3], ims[..., 3:6]
    nxt_w, nxt_w_gt = ref_tf_warp(nxt, flo_pred), ref_tf_warp(nxt, flo)
    prv, nxt, nxt_w, nxt_w_gt = 0.5 + prv, 0.5 + nxt, 0.5 + nxt_w, 0.5 + nxt_w_gt
    flo_rgb, flo_pred_rgb = ref_flow_to_image(flo), ref_flow_to_image(flo_pred)
    overlay = 0.5 * prv + 0.5 * nxt
    overlay_warped = 0.5 * prv + 0.5 * nxt_w
    delta_warped = np.abs(0.5 * prv - 0.5 * nxt_w)
    overlay_warped_gt = 0.5 * prv + 0.5 * nxt_w_gt
    delta_warped_gt = np.abs(0.5 * prv - 0.5 * nxt_w_gt)
    env = locals()
    return {name: ref_grid(env[name], grid) for name in
            ['prv', 'nxt', 'nxt_w', 'overlay', 'overlay_warped', 'overlay_warped_gt', 'delta_warped', 'delta_warped_gt',
             'flo_rgb', 'flo_pred_rgb']}


def ref_upflow(flow, s):
    """s * einops.repeat(flow, 'n h w c -> n (h h2) (w w2) c', h2=s, w2=s)."""
    return float(s) * np.repeat(np.repeat(np.asarray(flow, np.float64), s, axis=1), s, axis=2)


def ref_interpolation_panels(img_pair, img1, pred, flow, grid=32):
    """pre_train_test.py:121-163 with _show's grid: {name: float64}; '5-flow' has the flow's own size."""
    pair, img1, pred = (np.asarray(v, np.float64) for v in (img_pair, img1, pred))
    s = pair.shape[1] // flow.shape[1]
    assert s >= 1 and pair.shape[1:3] == (s * flow.shape[1], s * flow.shape[2])
    img0, img2 = 0.5 + pair[..., 0:3], 0.5 + pair[..., 3:6]
    out = {'0-prv': img0, '1-nxt': img2, '2-ground-truth': img1, '3-pred': 0.5 + pred,
           '4-overlay': 0.5 * img0 + 0.5 * img2, '5-flow': ref_flow_to_image(flow),
           '6-warp': ref_tf_warp(img1, ref_upflow(flow, s))}
    return {k: ref_grid(v, grid) for k, v in out.items()}


# ---- fixtures, shared with the GPU suite ----------------------------------------------------------------------------
def sample_coordinates(flow, s=1):
    """float64 (x, y) of every tf_warp sample of a channels-last fp32 flow repeated and scaled by s."""
    up = ref_upflow(flow, s)
    gx, gy = np.meshgrid(np.arange(up.shape[2]), np.arange(up.shape[1]))
    return gx[None] + up[..., 0], gy[None] + up[..., 1]


def margin_ok(flow, s=1):
    x, y = sample_coordinates(flow, s)
    H, W = x.shape[1:3]
    for c, edges in ((x, (-1.0, W - 1.0)), (y, (-1.0, H - 1.0))):
        for e in edges:
            d = np.abs(c - e)
            if ((d < MARGIN) & (d != 0.0)).any():
                return False
    return True


def outside_share(flow, s=1):
    x, y = sample_coordinates(flow, s)
    H, W = x.shape[1:3]
    sides = [x < 0, x > W - 1, y < 0, y > H - 1]
    assert all(m.any() for m in sides), "a side of the image no sample leaves by"
    return float(np.mean(sides[0] | sides[1] | sides[2] | sides[3]))


def nudge_to_margin(flow, s=1):
    """The flow with 4e-3 added to every component whose sample coordinate (any of the s x s it is repeated to) lies
    within 1.5e-3 of -1, W-1 or H-1 without being that value, again until margin_ok holds: as
    test_quality_cpu.away_from_steps moves elements off the 8-bit steps.  For fixtures too large to re-seed: among half
    a million samples some always lie that close.  The condition itself is margin_ok's, unchanged."""
    flow = flow.copy()
    n, h, w, _ = flow.shape
    for _ in range(50):
        if margin_ok(flow, s):
            return flow
        x, y = sample_coordinates(flow, s)
        H, W = x.shape[1:3]
        for c, (coord, edges) in enumerate(((x, (-1.0, W - 1.0)), (y, (-1.0, H - 1.0)))):
            near = np.zeros(coord.shape, bool)
            for e in edges:
                d = np.abs(coord - e)
                near |= (d < 1.5 * MARGIN) & (d != 0.0)
            flow[..., c][near.reshape(n, h, s, w, s).any(axis=(2, 4))] += np.float32(4e-3)
    raise AssertionError("could not move every sample away from tf_warp's steps")


def checked_flow(seed, shape, s=1, plant=True, scale=3.0, min_outside=0.05, nudge=False):
    """(B,h,w,2) float32 N(0, scale^2) meeting the fixture condition (module docstring).  plant: image 0's largest
    vector at its last pixel (the last, partial max-tile where h * w > _hip.VIS_MAX_TILE) and image 1's at pixel 3
    (the first), whole numbers far above the rest, as test_gpu_vis.make_levels does; or a sequence of
    (image, pixel, (fx, fy)) to plant other vectors, pixel counted row-major.  min_outside: the share of the samples
    that must leave the image (None: only that every side is left by some sample, which outside_share asserts).
    nudge: meet the condition by nudge_to_margin, not by re-seeding."""
    for k in range(1000):
        flow = (np.random.default_rng(seed + 1000 * k).standard_normal(shape + (2,)) * scale).astype(np.float32)
        if plant:
            assert float(np.abs(flow).max()) < 20.0
            spots = ((0, -1, (30.0, -40.0)), (1, 3, (-21.0, 20.0))) if plant is True else plant
            for n, pixel, vector in spots:
                flow[n].reshape(-1, 2)[pixel] = vector
        if nudge:
            flow = nudge_to_margin(flow, s)
        if margin_ok(flow, s):
            share = outside_share(flow, s)
            assert min_outside is None or share > min_outside, share
            flow.setflags(write=False)
            return flow
    raise AssertionError("no seed meets the margin")


SET1 = {"scalar": (33, 70), "vec4": (32, 68)}                     # 2310 = 2048 + 262 pixels: no multiple of 4; 2176
SET2 = {"scalar": ((34, 70), 2), "vec4": ((36, 72), 2), "s1": ((20, 36), 1)}   # flows 17 x 35 (odd), 18 x 36, 20 x 36
KERNELS = {"scalar": "review_panels_kernel<scalar>", "vec4": "review_panels_kernel<vec4>",
           "s1": "review_panels_kernel<vec4>"}


@functools.lru_cache(maxsize=None)
def set1_case(form, seed=0):
    """Channels-last float32 inputs of inference_panels: uniform images, read-only."""
    H, W = SET1[form]
    assert H * W > _hip.VIS_MAX_TILE and H * W % _hip.VIS_MAX_TILE, "the flow no longer straddles a max-tile"
    rng = np.random.default_rng(100 + seed)
    ims = (rng.random((B, H, W, 6), dtype=np.float32) - np.float32(0.5))
    ims.setflags(write=False)
    return {"ims": ims, "flo": checked_flow(200 + seed, (B, H, W)), "flo_pred": checked_flow(300 + seed, (B, H, W), plant=False)}


@functools.lru_cache(maxsize=None)
def set2_case(form, seed=0):
    """Channels-last float32 inputs of interpolation_panels; pred leaves [-0.5, 0.5] so that 3-pred is clipped."""
    (H, W), s = SET2[form]
    rng = np.random.default_rng(400 + seed)
    pair = rng.random((B, H, W, 6), dtype=np.float32) - np.float32(0.5)
    img1 = rng.random((B, H, W, 3), dtype=np.float32)
    pred = (rng.random((B, H, W, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.2)
    for a in (pair, img1, pred):
        a.setflags(write=False)
    return {"img_pair": pair, "img1": img1, "pred": pred, "flow": checked_flow(500 + seed, (B, H // s, W // s), s)}


def as_half(case):
    """The case with its images rounded to fp16 (the flows stay fp32)."""
    return {k: (v if k.startswith("flo") else v.astype(np.float16)) for k, v in case.items()}


_REF = {}


def reference(set_no, form, half, grid):
    """The float64 pictures of a fixture, computed once per key and left unchanged."""
    key = (set_no, form, half, grid)
    if key not in _REF:
        case = (set1_case if set_no == 1 else set2_case)(form)
        case = {k: v.astype(np.float32) for k, v in (as_half(case) if half else case).items()}
        _REF[key] = (ref_inference_panels if set_no == 1 else ref_interpolation_panels)(grid=grid, **case)
        for r in _REF[key].values():
            r.setflags(write=False)
    return _REF[key]


def run_panels(set_no, case, in_format="channels_last", out_format="channels_last", dtype=torch.float32, grid=0,
               device="cpu"):
    """vis.inference_panels / interpolation_panels of a channels-last numpy case on `device` -> ({name: tensor},
    {name: channels-last numpy})."""
    ts = {k: torch.from_numpy(np.array(to_layout(v, "channels_last", in_format), order="C")).to(device)
          for k, v in case.items()}
    fn = vis.inference_panels if set_no == 1 else vis.interpolation_panels
    outs = fn(data_format=in_format, dtype=dtype, grid=grid, out_format=out_format, **ts)
    return outs, {k: to_layout(o.cpu().numpy(), out_format, "channels_last") for k, o in outs.items()}


def float_error(got, want):
    """Largest |got - want| over EVERY element of every picture, after the checks on names, shapes and types."""
    assert list(got) == list(want)
    worst = 0.0
    for name in want:
        g, r = got[name], want[name]
        assert g.shape == r.shape and g.dtype == np.float32 and np.isfinite(g).all(), name
        worst = max(worst, float(np.abs(g - r).max()))
    return worst


def uint8_share(got, want, grid):
    """The uint8 rule: a picture may differ from the exported float64 one by one level, and only at eligible elements:
    255 x the clipped float64 value within 1e-3 of a whole number, and not on a grid line, not beyond the clip by more
    than 1e-5 and not exactly 0 or 1.  -> the share of eligible elements of the set, which the caller caps at 1 %."""
    assert list(got) == list(want)
    eligible = total = 0
    for name in want:
        g, r = got[name], want[name]
        assert g.shape == r.shape and g.dtype == np.uint8, name
        x = 255 * np.clip(r, 0.0, 1.0)
        near = np.abs(x - np.rint(x)) < 1e-3
        line = np.zeros(r.shape, bool)
        if grid:
            line[:, ::grid, :, :] = True
            line[:, :, ::grid, :] = True
            assert (g[line] == 255).all(), name
        ok = near & ~line & ~((r < -1e-5) | (r > 1.0 + 1e-5)) & ~((r == 0.0) | (r == 1.0))
        diff = np.abs(g.astype(np.int64) - ref_export_uint8(r).astype(np.int64))
        assert diff.max() <= 1 and not diff[~ok].any(), name
        eligible, total = eligible + int(ok.sum()), total + ok.size
    return eligible / total


# ---- the restatement against the oracle package and the flow pictures -----------------------------------------------
def test_restated_warp_equals_the_oracle_in_both_precisions():
    case = set1_case("scalar")
    img = case["ims"][..., 3:6]
    for dtype in (np.float64, np.float32):
        want = np_ref.tf_warp(img.astype(dtype), case["flo"].astype(dtype))
        got = ref_tf_warp(img, case["flo"], dtype)
        assert got.dtype == want.dtype == dtype and np.array_equal(got, want)


def test_restated_flow_pictures_are_flow_to_image():
    c1, c2 = set1_case("scalar"), set2_case("scalar")
    p1, p2 = reference(1, "scalar", False, 0), reference(2, "scalar", False, 0)
    assert np.array_equal(p1["flo_rgb"], ref_flow_to_image(c1["flo"]))
    assert np.array_equal(p1["flo_pred_rgb"], ref_flow_to_image(c1["flo_pred"]))
    assert np.array_equal(p2["5-flow"], ref_flow_to_image(c2["flow"])) and p2["5-flow"].shape == (B, 17, 35, 3)
    assert list(p1) == list(vis.INFERENCE_PANELS) and list(p2) == list(vis.INTERPOLATION_PANELS)


def test_fixtures_meet_their_condition():
    for form in SET1:
        c = set1_case(form)
        for k in ("flo", "flo_pred"):
            assert margin_ok(c[k]) and outside_share(c[k]) > 0.05
        assert float(np.abs(c["flo"][0, :-1]).max()) < 20.0 and tuple(c["flo"][0, -1, -1]) == (30.0, -40.0)
    for form, (_, s) in SET2.items():
        f = set2_case(form)["flow"]
        assert margin_ok(f, s) and outside_share(f, s) > 0.05
    bad = np.zeros((1, 4, 6, 2), np.float32)
    assert margin_ok(bad)                                   # exactly W-1 / H-1 at the rim: exact in both precisions
    bad[0, 1, 2, 0] = np.float32(-3.0005)                   # x = -1.0005
    assert not margin_ok(bad)
    bad[0, 1, 2, 0] = np.float32(-3.0)                      # x = -1 exactly
    assert margin_ok(bad)


# ---- the torch compositions against every assertion of the GPU suite ------------------------------------------------
@pytest.mark.parametrize("grid", [0, 32])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("out_format", FORMATS)
@pytest.mark.parametrize("in_format", FORMATS)
@pytest.mark.parametrize("set_no,form", [(1, f) for f in SET1] + [(2, f) for f in SET2])
def test_torch_path_against_the_restatement(set_no, form, in_format, out_format, half, grid):
    """fp32 torch composition on the CPU: max |err| 4.4e-6 over the 80 cases."""
    case = (set1_case if set_no == 1 else set2_case)(form)
    _, got = run_panels(set_no, as_half(case) if half else case, in_format, out_format, torch.float32, grid)
    err = float_error(got, reference(set_no, form, half, grid))
    print("review torch set {} {} {}->{} {} grid {}: max |err| {:.3e}".format(set_no, form, in_format, out_format,
                                                                              "f16" if half else "f32", grid, err))
    assert err <= BOUND


@pytest.mark.parametrize("grid", [0, 32])
@pytest.mark.parametrize("set_no,form", [(1, f) for f in SET1] + [(2, f) for f in SET2])
def test_torch_path_uint8(set_no, form, grid):
    """Eligible elements (near a step of the export), capped at 1 % of a set: 0.15-0.20 % of set 1, what uniform values
    give, and 0.50-0.72 % of set 2 -- a property of the restatement: 6-warp has no offset, and where a sample leaves
    the image its four terms cancel to about 1e-17 in float64, not to 0, which is near the step at 0 and not on it."""
    case = (set1_case if set_no == 1 else set2_case)(form)
    for out_format in FORMATS:
        _, got = run_panels(set_no, case, "channels_last", out_format, torch.uint8, grid)
        share = uint8_share(got, reference(set_no, form, False, grid), grid)
        print("review torch uint8 set {} {} grid {}: {:.3f} % eligible".format(set_no, form, grid, 100 * share))
        assert share <= 0.01


def test_negative_controls():
    """The comparison tells apart: the two flows swapped, the factor s dropped, image 0's planted maximum zeroed."""
    c = set1_case("scalar")
    want = reference(1, "scalar", False, 0)
    _, got = run_panels(1, dict(c, flo=c["flo_pred"], flo_pred=c["flo"]))
    assert float(np.abs(got["nxt_w"] - want["nxt_w"]).max()) > 1000 * BOUND
    assert float(np.abs(got["nxt_w"] - want["overlay_warped_gt"] * 2 + want["prv"]).max()) <= BOUND   # nxt_w_gt
    c2, w2 = set2_case("scalar"), reference(2, "scalar", False, 0)
    unscaled = ref_tf_warp(c2["img1"], ref_upflow(c2["flow"], 2) / 2.0)
    assert float(np.abs(unscaled - w2["6-warp"]).max()) > 1000 * BOUND
    cut = c["flo"].copy()
    cut[0, -1, -1] = 0.0
    _, got = run_panels(1, c)
    other = ref_flow_to_image(cut)
    assert float(np.abs(got["flo_rgb"][0, :-1] - other[0, :-1]).max()) > 1000 * BOUND
    assert float(np.abs(got["flo_rgb"][1] - other[1]).max()) <= BOUND


# ---- known answers --------------------------------------------------------------------------------------------------
def test_zero_flows_leave_nxt_but_for_the_last_row_and_column():
    """tf_warp returns 0 at a coordinate of exactly W-1 / H-1: both weights of that axis vanish."""
    ims = set1_case("vec4")["ims"][:, :9, :14]
    zero = np.zeros((B, 9, 14, 2), np.float32)
    for fn in (lambda: ref_inference_panels(ims, zero, zero),
               lambda: run_panels(1, {"ims": ims, "flo": zero, "flo_pred": zero})[1]):
        p = fn()
        assert np.abs(p["nxt_w"][:, :-1, :-1] - p["nxt"][:, :-1, :-1]).max() <= 1e-6
        assert (p["nxt_w"][:, -1] == 0.5).all() and (p["nxt_w"][:, :, -1] == 0.5).all()
        inner = np.abs(0.5 * p["prv"] - 0.5 * p["nxt"])[:, :-1, :-1]
        assert np.abs(p["delta_warped"][:, :-1, :-1] - inner).max() <= 1e-6
        assert np.abs(p["delta_warped_gt"][:, :-1, :-1] - inner).max() <= 1e-6
        assert np.abs(p["overlay_warped"][:, :-1, :-1] - p["overlay"][:, :-1, :-1]).max() <= 1e-6
        assert (p["flo_rgb"] == 1.0).all() and (p["flo_pred_rgb"] == 1.0).all()           # an all-zero flow is white
        assert np.abs(p["prv"] - (0.5 + ims[..., 0:3].astype(np.float64))).max() <= 1e-6


def test_impulse_moves_one_column():
    """tests/test_warp.py's 3 x 3 impulse with flow (1, 0): out[y, x] = img[y, x + 1]."""
    ims = np.full((1, 3, 3, 6), -0.5, np.float32)           # nxt = 0 after the offset is undone
    ims[0, 1, 1, 3:6] = 0.5                                 # nxt[1, 1] = 1
    flow = np.zeros((1, 3, 3, 2), np.float32)
    flow[..., 0] = 1.0
    for p in (ref_inference_panels(ims, flow, flow), run_panels(1, {"ims": ims, "flo": flow, "flo_pred": flow})[1]):
        # the warp acts on the offset image: 0.5 + tf_warp(nxt - 0.5); x + 1 = W - 1 in column 1 gives weight 0 -> 0.5
        assert np.abs(p["nxt_w"][0, 1, 0] - 1.0).max() <= 1e-6
        assert np.abs(p["nxt_w"][0, 0, 0] - 0.0).max() <= 1e-6
        assert (p["nxt_w"][0, :, 1:] == 0.5).all()


def test_constant_flow_shifts_the_middle_frame_by_two_columns():
    """6-warp with flow (1, 0) at s = 2: upflow is (2, 0), so 6-warp[y, x] = img1[y, x + 2] inside the image."""
    c = set2_case("s1")
    img1 = c["img1"][:, :8, :12]
    pair, pred = c["img_pair"][:, :8, :12], c["pred"][:, :8, :12]
    flow = np.zeros((B, 4, 6, 2), np.float32)
    flow[..., 0] = 1.0
    case = {"img_pair": pair, "img1": img1, "pred": pred, "flow": flow}
    for p in (ref_interpolation_panels(grid=0, **case), run_panels(2, case, grid=0)[1]):
        assert np.abs(p["6-warp"][:, :-1, :-3] - img1[:, :-1, 2:-1]).max() <= 1e-6
        assert np.abs(p["2-ground-truth"] - img1).max() == 0.0
        assert np.abs(p["3-pred"] - (0.5 + pred.astype(np.float64))).max() <= 1e-6
        assert p["5-flow"].shape == (B, 4, 6, 3)


def test_grid_and_export_rule():
    c = set2_case("s1")
    _, f = run_panels(2, c, grid=8)
    _, u = run_panels(2, c, dtype=torch.uint8, grid=8)
    for name in vis.INTERPOLATION_PANELS:
        assert (f[name][:, ::8] == 1.0).all() and (f[name][:, :, ::8] == 1.0).all()
        assert np.array_equal(u[name], vis.export_uint8(torch.from_numpy(f[name])).numpy())
    assert f["3-pred"].max() > 1.0 and f["3-pred"].min() < 0.0                      # float32: unclipped
    x = torch.tensor([0.0, 1.0, 0.5, -0.25, 1.5, 0.999, 254.5 / 255.0, 1.5 / 255.0])
    want = [0, 255, 127, 0, 255, 254, 254, 1]                                       # not to_uint8's 255.5 rule
    assert vis.export_uint8(x).tolist() == want and ref_export_uint8(x.double().numpy()).tolist() == want
    assert vis.to_uint8(x).tolist()[5] == 255
    no_grid = run_panels(2, c, grid=0)[1]
    assert not (no_grid["0-prv"][:, ::8] == 1.0).all()
    assert not (run_panels(1, set1_case("vec4"))[1]["prv"][:, 0] == 1.0).all()      # inference_panels: grid off by default


def test_refusals():
    c = {k: torch.from_numpy(v.copy()) for k, v in set2_case("s1").items()}
    with pytest.raises(ValueError, match="whole multiple"):
        vis.interpolation_panels(c["img_pair"], c["img1"], c["pred"], c["flow"][:, :5])
    with pytest.raises(ValueError, match="dtype"):
        vis.interpolation_panels(c["img_pair"], c["img1"].half(), c["pred"], c["flow"])
    with pytest.raises(ValueError, match="grid"):
        vis.interpolation_panels(c["img_pair"], c["img1"], c["pred"], c["flow"], grid=-1)
    with pytest.raises(ValueError, match="Unsupported data format"):
        vis.interpolation_panels(c["img_pair"], c["img1"], c["pred"], c["flow"], out_format="nhwc")
    with pytest.raises(ValueError, match="dtype"):
        vis.interpolation_panels(c["img_pair"], c["img1"], c["pred"], c["flow"], dtype=torch.float16)
    s = {k: torch.from_numpy(v.copy()) for k, v in set1_case("vec4").items()}
    with pytest.raises(ValueError, match="must be"):
        vis.inference_panels(s["ims"][..., :5], s["flo"], s["flo_pred"])
    with pytest.raises(ValueError, match="size"):
        vis.inference_panels(s["ims"], s["flo"][:, :8], s["flo_pred"])
    half = vis.inference_panels(s["ims"], s["flo"].half(), s["flo_pred"])           # fp16 flows are widened
    assert half["nxt_w"].dtype == torch.float32


# ---- the C boundary's table ------------------------------------------------------------------------------------------
def test_review_prototypes_match_their_header():
    protos = parse_header(REVIEW_HEADER)
    assert [name for name, _, _ in protos] == ["qpwc_review_workspace_floats", "qpwc_inference_panels_fwd",
                                               "qpwc_interpolation_panels_fwd", "qpwc_review_panels_fwd_kernel"]
    assert mismatches(_hip.REVIEW_PROTOTYPES, protos) == []
    others = (set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES) | set(_hip.TRIPLET_PROTOTYPES) | set(_hip.VIS_PROTOTYPES)
              | set(_hip.QUALITY_PROTOTYPES))
    assert len(_hip.SYMBOLS) == 77 and not set(_hip.REVIEW_PROTOTYPES) & others
    table = dict(_hip.REVIEW_PROTOTYPES)
    restype, argtypes = table["qpwc_inference_panels_fwd"]
    table["qpwc_inference_panels_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_inference_panels_fwd: 14 parameters, table has 13"]


def test_the_library_exports_the_table(hip_lib):
    for name, (restype, argtypes) in _hip.REVIEW_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)

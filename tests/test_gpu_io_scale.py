"""GPU suite of the input pipeline, the flow panels, the review panels and the image quality at the sizes where their
fold loops take a second, uneven trip.

Each of these families ends in a fold that a fixed number of lanes walks: the contrast mean of csrc/augment.hip from the
256-pixel partials of pass 1, the per-image maximum of csrc/vis.hip and csrc/review.hip from the 2048-pixel max-tile
partials, and csrc/quality.hip's fold over sixteen images per trip and 64 tiles per trip.  Their own suites use shapes at
which every one of those loops runs once, so a fold that stopped after its first trip would pass there.  Every case
below needs the second trip, which is uneven (lane 0 alone, or three waves of sixteen), and plants what the answer
depends on behind the first trip.  tests/test_io_scale_cpu.py reads the loop constants from the sources and checks that
the shapes in CASES still do; it also holds the fp32 torch compositions to the same bounds on the same fixtures, and
computes from the restatements the answer a one-trip fold would give, to show that it lies 10 to 1000 bounds away.

Oracles and bounds are the families' own: ref_augment, ref_flow_to_image / ref_nearest, ref_inference_panels /
ref_interpolation_panels at BOUND = 1e-4 over every element, ref_quality at BOUNDS.  No new tolerance.

The review fixtures differ from the small ones of tests/test_review_cpu.py in two ways.  Fixture condition: among half
a million samples some always lie within 1e-3 of one of tf_warp's steps, so re-seeding cannot work; the offending
vectors are moved instead (nudge_to_margin) until the same condition, margin_ok, holds.  Outside share: 0.8 % of the
samples leave a 725 x 725 image, not more than 5 %; these cases need only that every side is left by some sample.
Their images are smooth sinusoids (neighbouring pixels differ by less than 0.01) and both extents stay below 1024: the
fp32 sample coordinate is good to 3e-5 px there, which uniform-random images would turn into 5e-5 to 7e-5 of picture
error, too close to BOUND for a test that is about the fold.

Measured on an MI355X: see the docstrings of the tests."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import BOUND, as_params, max_err, ref_augment, smooth_flow  # noqa: E402
from test_quality_cpu import check, make_images, ref_quality, tensor  # noqa: E402
from test_review_cpu import (checked_flow, float_error, ref_inference_panels, ref_interpolation_panels,  # noqa: E402
                             run_panels)
from test_vis_cpu import FORMATS, random_flow, ref_flow_to_image, ref_nearest, ref_uint8, to_layout  # noqa: E402

from qpwcnet_amd import _hip, metrics, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dev = lambda a: torch.from_numpy(np.array(a, order="C")).to(DEV)
B = 2

# The case shapes, one entry per family.  Planted vectors are (image, pixel counted row-major, (fx, fy)).
CASES = {
    # augment_contrast_kernel: 76,728 / 76,729 output pixels = 300 partials per sample and channel, folded by 256 lanes
    # (44 of them twice); 19 pass-2 workgroups per sample, the last partial.  uint8 sources of 30 x 52, upsampled.
    "augment": {"source": (30, 52), "vec4": (276, 278), "scalar": (277, 277)},
    # flow_to_image_kernel: level 0 has 525,825 pixels = 257 max-tiles, the last of 1537 pixels, folded by 256 lanes
    # (lane 0 twice); level 1's partials start at workgroup 2 * 257.  Pictures: the flows' own sizes (ow = 1025 > 256:
    # step_y == 0; odd pixel counts: <scalar>) and 64 x 256 (ow == 256: step_x == 0; <vec4>).
    "vis": {"levels": [(513, 1025), (5, 7)],
            "pictures": {"native": None, "w256": (64, 256)},
            "plant": [((0, 513 * 1025 - 1, (30.0, -40.0)), (1, 3, (-21.0, 20.0))),
                      ((0, 17, (12.0, -16.0)), (1, 34, (-15.0, 8.0)))]},
    # review_panels_kernel: set 1 at 725 x 725 (525,625 pixels, odd: <scalar>), set 2 at 724 x 726 with s = 1 (525,624:
    # <vec4>), 257 max-tiles each.  flo and set 2's flow: image 0's maximum at its last pixel, image 1's at pixel 3;
    # flo_pred: image 1's inside the last max-tile, image 0's in the first -- each vis_fold_max call needs its second trip.
    "review": {1: {"size": (725, 725), "grid": 0,
                   "plant": {"flo": ((0, 725 * 725 - 1, (30.0, -40.0)), (1, 3, (-21.0, 20.0))),
                             "flo_pred": ((0, 7, (-28.0, 45.0)), (1, 256 * 2048 + 1000, (36.0, 27.0)))}},
               2: {"size": (724, 726), "s": 1, "grid": 32,
                   "plant": {"flow": ((0, 724 * 726 - 1, (30.0, -40.0)), (1, 3, (-21.0, 20.0)))}}},
    # quality_fold_kernel: 19 images = a trip of sixteen and a trip of three; 79 x 413 SSIM positions = 5 x 13 = 65
    # tiles, tile 64 (15 x 29 positions, 1.3 % of them) being lane 0's second trip.
    "quality": {"B": 19, "size": (89, 423), "C": 3},
}


# ---- fixtures: numpy inputs, built on demand (tests/test_io_scale_cpu.py builds the same) ---------------------------
def augment_case(form):
    """(ims, flo, iparams, fparams, (h, w)): B = 2 uint8 frames of 30 x 52 that carry a vertical brightness ramp plus
    noise -- the output pixels past 65,536 (15 % of the image) then have another mean than the rest --, each sample
    with its own window, flip pair and colour parameters; contrast 0.7 and 1.3."""
    h, w = CASES["augment"][form]
    H, W = CASES["augment"]["source"]
    rng = np.random.default_rng(11)
    ramp = np.linspace(60.0, 200.0, H).reshape(1, H, 1, 1)
    ims = np.clip(np.rint(ramp + rng.integers(-30, 31, (B, H, W, 6))), 0, 255).astype(np.uint8)
    flo = smooth_flow(B, H, W, seed=3)
    ip = np.array([[h + 13, w + 22, 5, 9, 1, 0], [h + 4, w + 7, 2, 6, 0, 1]], np.int32)
    fp = np.array([[0.9, -0.9, -0.08, 0.6, -0.15, 0.7], [-1.1, 1.1, 0.06, 1.4, 0.1, 1.3]], np.float32)
    assert np.abs(flo).max() <= 32.0
    return ims, flo, ip, fp, (h, w)


def plant(flow, spots):
    for n, pixel, vector in spots:
        flow[n].reshape(-1, 2)[pixel] = vector
    return flow


def vis_levels(half=False):
    """Channels-last flows of CASES['vis']['levels'], N(0, 3^2), with the planted maxima far above the rest."""
    flows = []
    for l, (shape, spots) in enumerate(zip(CASES["vis"]["levels"], CASES["vis"]["plant"])):
        f = random_flow(70 + l, (B,) + shape)
        assert float(np.abs(f).max()) < 20.0 / (1 + l)
        plant(f, spots)
        for n, pixel, vector in spots:                              # each image's planted vector is its largest
            mag = np.hypot(f[n, ..., 0], f[n, ..., 1]).reshape(-1)
            assert int(mag.argmax()) == pixel and mag[pixel] > 1.25 * np.delete(mag, pixel).max()
        f = f.astype(np.float16) if half else f
        f.setflags(write=False)
        flows.append(f)
    return flows


def smooth_images(n_images, hw, C, lo, hi):
    """(n,H,W,C) float32 sinusoids between lo and hi, test_quality_cpu.make_images without its texture: every image and
    channel its own, neighbouring pixels less than 0.01 apart."""
    H, W = hw
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    out = np.empty((n_images, H, W, C))
    for n in range(n_images):
        for c in range(C):
            out[n, :, :, c] = np.sin(2 * math.pi * ((1.0 + n) * y + (1.5 - 0.5 * n) * x) + 0.7 * c + n)
    out = (lo + (hi - lo) * (0.5 + 0.5 * out)).astype(np.float32)
    assert max(float(np.abs(np.diff(out, axis=a)).max()) for a in (1, 2)) < 0.01
    out.setflags(write=False)
    return out


def review_case(set_no):
    """Channels-last float32 inputs of inference_panels (set 1) / interpolation_panels (set 2), read-only."""
    spec = CASES["review"][set_no]
    hw = spec["size"]
    flow = lambda seed, name: checked_flow(seed, (B,) + hw, spec.get("s", 1), plant=spec["plant"][name],
                                           min_outside=None, nudge=True)
    if set_no == 1:
        return {"ims": smooth_images(B, hw, 6, -0.45, 0.45), "flo": flow(600, "flo"), "flo_pred": flow(601, "flo_pred")}
    # pred leaves [-0.5, 0.5], so that 3-pred is clipped by the export rule
    return {"img_pair": smooth_images(B, hw, 6, -0.45, 0.45), "img1": smooth_images(B, hw, 3, 0.05, 0.95),
            "pred": smooth_images(B, hw, 3, -0.55, 0.55), "flow": flow(602, "flow")}


def review_reference(set_no, case):
    fn = ref_inference_panels if set_no == 1 else ref_interpolation_panels
    return fn(grid=CASES["review"][set_no]["grid"], **case)


def quality_case():
    """(truth, pred): 19 images, each with its own content and its own error level, sigma = 0.02 + 0.02 n.  (The
    content gets finer with n, which raises ssim; with steps of 0.01 images 4 to 6 come within 9e-4 of each other in
    ssim, with steps of 0.02 no two neighbours are closer than 1e-2.)"""
    q = CASES["quality"]
    truth, pred = make_images(8, q["size"], q["C"], batch=q["B"], sigmas=[0.02 + 0.02 * n for n in range(q["B"])])
    truth.setflags(write=False)
    pred.setflags(write=False)
    return truth, pred


# ---- 1. augmentation: the contrast fold -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def augment_refs():
    """{form: (case, float64 answer, the answer with the contrast mean over the first 256 * 256 pixels only)}."""
    out = {}
    for form in ("vec4", "scalar"):
        case = augment_case(form)
        out[form] = (case, ref_augment(*case), ref_augment(*case, mean_over_first=256 * 256))
    return out


def _augment(case, data_format="channels_last"):
    ims, flo, ip, fp, hw = case
    p = as_params(ip, fp, DEV)
    return ops.augment(dev(ims), dev(flo), p.iparams, p.fparams, hw, data_format=data_format)


def _augment_errors(got, ref, data_format):
    g_ims, g_flo = (t.cpu().numpy() for t in got)
    r_ims, r_flo = (to_layout(r, "channels_last", data_format) for r in ref)
    assert g_ims.shape == r_ims.shape and g_flo.shape == r_flo.shape and g_ims.dtype == np.float32
    assert np.isfinite(g_ims).all() and np.isfinite(g_flo).all()
    return max_err(g_ims, r_ims), max_err(g_flo, r_flo)


@pytest.mark.parametrize("data_format", FORMATS)
@pytest.mark.parametrize("form", ["vec4", "scalar"])
def test_augment_contrast_mean_folds_300_partials(augment_refs, form, data_format):
    """Every element against ref_augment, and against the answer of a fold that stops after 256 partials.  Measured on
    an MI355X: images 2.3e-6 (vec4) and 2.5e-6 (scalar), flow 6.5e-6 and 7.0e-6 px, in either layout; 1.2e-2 from the
    one-trip answer.  The torch composition on the CPU is at 2.3e-6 / 2.5e-6 and 6.5e-6 / 7.4e-6 px."""
    case, ref, wrong = augment_refs[form]
    h, w = case[4]
    got = _augment(case, data_format)
    assert ops.augment_kernel(B, h, w, got[0], got[1]) == "augment_pixel_kernel<{}>".format(form)
    e_ims, e_flo = _augment_errors(got, ref, data_format)
    w_ims, w_flo = _augment_errors(got, wrong, data_format)
    print("io-scale augment {} {}: max |ims err| {:.3e}, max |flow err| {:.3e} px; from the one-trip mean {:.3e}".format(
        form, data_format, e_ims, e_flo, w_ims))
    assert e_ims <= BOUND and e_flo <= BOUND
    assert w_ims > 10 * BOUND and w_flo == e_flo


@pytest.mark.parametrize("form", ["vec4", "scalar"])
def test_augment_layouts_and_repeats_agree_bit_for_bit(augment_refs, form):
    case = augment_refs[form][0]
    last, first = _augment(case, "channels_last"), _augment(case, "channels_first")
    assert torch.equal(first[0].permute(0, 2, 3, 1), last[0]) and torch.equal(first[1].permute(0, 2, 3, 1), last[1])
    again = _augment(case, "channels_last")
    assert torch.equal(again[0], last[0]) and torch.equal(again[1], last[1])          # the fixed-order contrast sums


@pytest.mark.parametrize("layout", [_hip.NHWC, _hip.NCHW], ids=["nhwc", "nchw"])
def test_augment_scalar_form_equals_vec4_form(augment_refs, layout):
    """The 276 x 278 batch through the 4-byte-store form (outputs 4 bytes off the 16-byte grid) gives the same bits."""
    ims, flo, ip, fp, (h, w) = augment_refs["vec4"][0]
    _, H, W, _ = ims.shape
    d_ims, d_flo, p = dev(ims), dev(flo), as_params(ip, fp, DEV)
    L = _hip.lib()
    ws = torch.empty(int(L.qpwc_augment_workspace_floats(B, h, w)), dtype=torch.float32, device=DEV)
    outs = {}
    for off, form in ((0, "augment_pixel_kernel<vec4>"), (1, "augment_pixel_kernel<scalar>")):
        o_ims = torch.zeros(B * h * w * 6 + 4, dtype=torch.float32, device=DEV)[off:off + B * h * w * 6]
        o_flo = torch.zeros(B * h * w * 2 + 4, dtype=torch.float32, device=DEV)[off:off + B * h * w * 2]
        assert L.qpwc_augment_fwd_kernel(B, h, w, o_ims.data_ptr(), o_flo.data_ptr()).decode() == form
        rc = L.qpwc_augment_fwd(d_ims.data_ptr(), _hip.U8, d_flo.data_ptr(), B, H, W, p.iparams.data_ptr(),
                                p.fparams.data_ptr(), h, w, _hip.AUGMENT_COLOR, layout, o_ims.data_ptr(),
                                o_flo.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _hip.check(rc)
        outs[off] = (o_ims.clone(), o_flo.clone())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want = _augment(augment_refs["vec4"][0], "channels_last" if layout == _hip.NHWC else "channels_first")
    assert torch.equal(outs[0][0], want[0].reshape(-1)) and torch.equal(outs[0][1], want[1].reshape(-1))


# ---- 2. flow panels: the maximum fold, wide rows, workspace offsets -------------------------------------------------
@pytest.fixture(scope="module")
def vis_refs():
    """{(half, picture): float64 channels-last pictures of both levels}, and the flows: {half: [level 0, level 1]}."""
    flows = {half: vis_levels(half) for half in (False, True)}
    refs = {}
    for half, fs in flows.items():
        imgs = [ref_flow_to_image(f.astype(np.float32)) for f in fs]
        for name, size in CASES["vis"]["pictures"].items():
            refs[half, name] = [i if size is None else ref_nearest(i, size) for i in imgs]
    return flows, refs


def _flow_pictures(flows, size, in_format, out_format, dtype):
    ts = [dev(to_layout(f, "channels_last", in_format)) for f in flows]
    outs = ops.flow_to_image(ts, None if size is None else [size] * len(ts), in_format, dtype, out_format)
    return outs, [to_layout(o.cpu().numpy(), out_format, "channels_last") for o in outs]


def _picture_sizes(size):
    return CASES["vis"]["levels"] if size is None else [size] * len(CASES["vis"]["levels"])


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("picture", list(CASES["vis"]["pictures"]))
@pytest.mark.parametrize("out_format", FORMATS)
@pytest.mark.parametrize("in_format", FORMATS)
def test_flow_pictures_fold_257_max_tiles(vis_refs, in_format, out_format, picture, half):
    """Every element of both pictures.  Measured on an MI355X: max |err| 4.8e-7 for fp32 and for fp16 flows over the 16
    cases (level 0 at its own size; 2.5e-7 at most in the other pictures); the torch composition on the CPU is at
    4.8e-7."""
    flows, refs = vis_refs
    size = CASES["vis"]["pictures"][picture]
    outs, got = _flow_pictures(flows[half], size, in_format, out_format, torch.float32)
    name = ops.flow_to_image_kernel(B, _picture_sizes(size), torch.float32, out_format, outs)
    assert name == "flow_to_image_kernel<{}>".format("scalar" if size is None else "vec4")
    for l, (g, r) in enumerate(zip(got, refs[half, picture])):
        assert g.shape == r.shape and g.dtype == np.float32 and np.isfinite(g).all()
        e = float(np.abs(g - r).max())                          # over EVERY element
        print("io-scale vis {}->{} {} {} level {}: max |err| {:.3e}".format(in_format, out_format, picture,
                                                                            "f16" if half else "f32", l, e))
        assert e <= BOUND
    if size is None:
        # every level is normalised by its planted maxima: fully saturated there
        for g, spots in zip(got, CASES["vis"]["plant"]):
            for n, pixel, _ in spots:
                assert g[n].reshape(-1, 3)[pixel].min() < 1e-6


def test_flow_pictures_negative_control(vis_refs):
    """Without image 0's last pixel, which only lane 0's second trip of the fold sees, its maximum is several times
    smaller and every other pixel of the image several times more saturated; image 1 keeps its own maximum.  Measured
    on an MI355X: 0.69 from the cut restatement."""
    flows, _ = vis_refs
    cut = flows[False][0].copy()
    cut[0, -1, -1] = 0.0
    other = ref_flow_to_image(cut)
    _, got = _flow_pictures(flows[False], None, "channels_last", "channels_last", torch.float32)
    d = float(np.abs(got[0][0].reshape(-1, 3)[:-1] - other[0].reshape(-1, 3)[:-1]).max())
    print("io-scale vis: from the restatement without the last pixel {:.3e}".format(d))
    assert d > 1000 * BOUND
    assert float(np.abs(got[0][1] - other[1]).max()) <= BOUND


@pytest.mark.parametrize("picture", list(CASES["vis"]["pictures"]))
def test_flow_pictures_uint8(vis_refs, picture):
    """uint8 against float64: at most one level off, and only where the float64 value times 255.5 lies within 1e-3 of a
    whole number; those elements may be at most 1 % (0.13 % of these pictures at the flows' own sizes, 0.53 % at
    64 x 256: a property of the restatement).  Measured on an MI355X: no element is off anywhere else."""
    flows, refs = vis_refs
    size = CASES["vis"]["pictures"][picture]
    outs, got = _flow_pictures(flows[False], size, "channels_last", "channels_last", torch.uint8)
    name = ops.flow_to_image_kernel(B, _picture_sizes(size), torch.uint8, "channels_last", outs)
    assert name == "flow_to_image_kernel<{}>".format("scalar" if size is None else "vec4")
    near = total = 0
    for g, r in zip(got, refs[False, picture]):
        assert g.dtype == np.uint8 and g.shape == r.shape
        x = r * 255.5
        close = np.abs(x - np.rint(x)) < 1e-3
        diff = np.abs(g.astype(np.int64) - ref_uint8(r).astype(np.int64))
        assert diff.max() <= 1 and not diff[~close].any()
        near, total = near + int(close.sum()), total + close.size
    print("io-scale vis uint8 {}: {:.3f} % of the elements near a step".format(picture, 100.0 * near / total))
    assert near <= 0.01 * total


# ---- 3. review panels: both folds of set 1, the fold of set 2 -------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 2], ids=["set1", "set2"])
def review_refs(request):
    case = review_case(request.param)
    return request.param, case, review_reference(request.param, case)


@pytest.mark.parametrize("data_format", FORMATS)
def test_review_panels_fold_257_max_tiles(review_refs, data_format):
    """All ten pictures of set 1 (725 x 725, <scalar>) and all seven of set 2 (724 x 726, s = 1, grid 32, <vec4>), every
    element, with the inputs and the pictures in `data_format`.  Measured on an MI355X: max |err| 4.8e-7 for both
    sets; the torch composition on the CPU is at 4.8e-7."""
    set_no, case, want = review_refs
    spec = CASES["review"][set_no]
    H, W = spec["size"]
    outs, got = run_panels(set_no, case, data_format, data_format, torch.float32, spec["grid"], DEV)
    form = ops.review_panels_kernel(2, B, H, W) if set_no == 1 else ops.review_panels_kernel(1, B, H, W, H, W)
    assert form == "review_panels_kernel<{}>".format("scalar" if set_no == 1 else "vec4")
    err = float_error(got, want)
    print("io-scale review set {} {}: max |err| {:.3e}".format(set_no, data_format, err))
    assert err <= BOUND
    assert all(o.is_contiguous() and o.dtype == torch.float32 for o in outs.values())
    if set_no == 1:
        # each flow picture is normalised by its planted maxima: fully saturated there
        for name, pic in (("flo", "flo_rgb"), ("flo_pred", "flo_pred_rgb")):
            for n, pixel, _ in spec["plant"][name]:
                assert got[pic][n].reshape(-1, 3)[pixel].min() < 1e-6, (name, n)


# ---- 4. PSNR / SSIM: the image loop and the tile loop of the fold ---------------------------------------------------
@pytest.fixture(scope="module")
def quality_refs():
    truth, pred = quality_case()
    return truth, pred, ref_quality(truth, pred)


def _running_sum(values):
    """The float64 running sum of fp32 values, in order."""
    return float(torch.cumsum(values.double().cpu(), 0)[-1])


def test_quality_fold_walks_19_images_and_65_tiles(quality_refs):
    """All 19 values of mse, psnr and ssim against ref_quality; the state across the trip boundary, and across two
    calls.  Measured on an MI355X: mse 5.2e-8 relative, psnr 8.5e-7 dB, ssim 2.5e-8 -- the rounding of the fp32 results;
    the torch composition on the CPU is at the same three figures."""
    truth, pred, want = quality_refs
    n = CASES["quality"]["B"]
    t, p = tensor(truth).to(DEV), tensor(pred).to(DEV)
    state = torch.zeros(4, dtype=torch.float64, device=DEV)
    res = metrics.image_quality(t, p, data_format="channels_last", state=state)
    assert all(v.dtype == torch.float32 and tuple(v.shape) == (n,) for v in res)
    got = [v.cpu().numpy() for v in res]
    assert all(np.isfinite(g).all() for g in got)
    check("hip io-scale", got, want)
    plain = metrics.image_quality(t, p, data_format="channels_last")
    assert all(torch.equal(a, b) for a, b in zip(res, plain))                          # the state changes no value
    once = state.cpu()
    assert float(once[3]) == n
    for i in range(3):
        s = _running_sum(res[i])
        assert abs(float(once[i]) - s) <= 1e-12 * abs(s), (i, float(once[i]), s)
    again = metrics.image_quality(t, p, data_format="channels_last", state=state)
    assert all(torch.equal(a, b) for a, b in zip(res, again))
    twice = state.cpu()
    assert float(twice[3]) == 2 * n
    for i in range(3):
        s = _running_sum(torch.cat([res[i], res[i]]))
        assert abs(float(twice[i]) - s) <= 1e-12 * abs(s), (i, float(twice[i]), s)


def test_quality_fold_in_the_other_layout(quality_refs):
    """channels_first.  Measured on an MI355X: mse 5.2e-8 relative, psnr 8.5e-7 dB, ssim 2.5e-8."""
    truth, pred, want = quality_refs
    t, p = (tensor(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))).to(DEV) for a in (truth, pred))
    res = metrics.image_quality(t, p, data_format="channels_first")
    check("hip io-scale channels_first", [v.cpu().numpy() for v in res], want)
    # the layout decides which lane sums which squared error, not what reaches LDS: ssim is the same bit for bit
    last = metrics.image_quality(tensor(truth).to(DEV), tensor(pred).to(DEV), data_format="channels_last")
    assert torch.equal(res.ssim, last.ssim)

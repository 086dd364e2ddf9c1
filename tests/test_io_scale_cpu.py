"""The shapes of tests/test_gpu_io_scale.py still make their fold loops take a second, uneven trip.

The loop constants are read from the kernel sources, and each loop header must occur exactly once in its file, so that a
raised constant or a rewritten loop fails here and does not quietly turn those tests back into one-trip tests.  The launch
form of every case is asked of the library on the host.

The same fixtures then go through the fp32 torch compositions, which must meet the families' own bounds against the
float64 restatements (the review cases BOUND / 4: the fixtures are built so that the comparison has room for the fold),
and through the wrong-answer controls: the restatement of what a fold cut to one trip would give lies 10 to 1000 bounds
away, so the GPU cases fail against such a kernel."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import BOUND, as_params, max_err, ref_augment  # noqa: E402
from test_gpu_io_scale import (B, CASES, augment_case, quality_case, review_case, review_reference,  # noqa: E402
                               vis_levels)
from test_quality_cpu import BOUNDS, check, ref_quality, ref_ssim_map, tensor  # noqa: E402
from test_review_cpu import float_error, margin_ok, outside_share, run_panels  # noqa: E402
from test_vis_cpu import FORMATS, ref_flow_to_image, ref_nearest, ref_nearest_index, ref_uint8, to_layout  # noqa: E402

from qpwcnet_amd import augment, metrics, vis  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constants(name, *keys):
    text = _text(name)
    out = {}
    for k in keys:
        m = re.findall(r"constexpr\s+int\s+{}\s*=\s*(\d+)\s*;".format(k), text)
        assert len(m) == 1, (name, k, m)
        out[k] = int(m[0])
    return out


def _tile_constants():
    m = re.findall(r"constexpr\s+int\s+kQualTH\s*=\s*(\d+)\s*,\s*kQualTW\s*=\s*(\d+)\s*;", _text("quality.hip"))
    assert len(m) == 1, m
    return {"kQualTH": int(m[0][0]), "kQualTW": int(m[0][1])}


AUG = dict(_constants("augment_common.h", "kAugThreads"), **_constants("augment.hip", "kAugPass2Pixels"))
VIS = _constants("vis_common.h", "kVisThreads", "kVisMaxPix")
QUAL = dict(_constants("quality.hip", "kQualFoldThreads"), **_tile_constants())
VIS_MAX_TILE = VIS["kVisThreads"] * VIS["kVisMaxPix"]
WAVE = 64

# the loops the cases are built for, as their files spell them
LOOPS = [("augment.hip", "for (int i = tid; i < nblk; i += kAugThreads) s += p[i];"),
         ("vis_common.h", "for (int i = threadIdx.x; i < mt; i += kVisThreads) m = fmaxf(m, part[i]);"),
         ("quality.hip", "for (int n0 = 0; n0 < B; n0 += kQualFoldThreads / 64) {"),
         ("quality.hip", "for (int t = lane; t < tiles; t += 64) {")]


def _ceil(a, b):
    return -(-a // b)


# ---- the loops and the shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,header", LOOPS)
def test_each_loop_header_occurs_once(name, header):
    assert _text(name).count(header) == 1, (name, header)


def test_review_folds_both_flows_of_set_1_and_the_flow_of_set_2():
    text = _text("review.hip")
    assert text.count("vis_fold_max(ws, 0, n, a.mtiles, red[0])") == 2          # set 1's flo and set 2's flow
    assert text.count("vis_fold_max(ws, a.B * a.mtiles, n, a.mtiles, red[1])") == 1   # set 1's flo_pred, behind flo's
    assert len(re.findall(r"\bvis_fold_max\(", text)) == 3                      # the definition is vis_common.h's
    assert text.count("m.mblk0[k] = k * a.B * a.mtiles;") == 1                  # where the max launch leaves flow k's
    common = _text("vis_common.h")
    assert len(re.findall(r"\bvis_fold_max\(", common)) == 1
    assert "const float* part = ws + blk0 + (int64_t)n * mt;" in common
    assert len(re.findall(r"\bvis_fold_max\(", _text("vis.hip"))) == 1
    assert "inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }" in _text("pixel_io.h")
    assert text.count("a.mtiles = (int)ceil_div((int64_t)a.h * a.w, kVisMaxTile);") == 1
    assert _text("vis.hip").count("lv.m.mtiles[l] = (int)ceil_div((int64_t)h[l] * w[l], kVisMaxTile);") == 1
    assert common.count("constexpr int kVisMaxTile = kVisThreads * kVisMaxPix;") == 1


def test_augment_cases_fold_more_partials_than_lanes():
    threads, chunk = AUG["kAugThreads"], AUG["kAugPass2Pixels"]
    text = _text("augment.hip")
    assert "inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }" in _text("pixel_io.h")
    assert "return ceil_div((int64_t)h * w, kAugThreads); }" in text                              # nblk
    assert "const int nblk2 = (int)ceil_div((int64_t)h * w, kAugPass2Pixels);" in text
    forms = CASES["augment"]
    for form in ("vec4", "scalar"):
        h, w = forms[form]
        nblk = _ceil(h * w, threads)
        assert nblk > threads and nblk % threads, (form, nblk)                  # a second trip, for some lanes only
        assert _ceil(h * w, chunk) > 1 and (h * w) % chunk, form                # several pass-2 workgroups, the last partial
        assert h * w > threads * threads                                        # pixels past the control's 256 * 256
    assert (forms["vec4"][0] * forms["vec4"][1]) % 4 == 0 and (forms["scalar"][0] * forms["scalar"][1]) % 4


def test_vis_and_review_cases_fold_more_max_tiles_than_lanes():
    threads = VIS["kVisThreads"]
    h, w = CASES["vis"]["levels"][0]
    sizes = {"vis": (h, w, CASES["vis"]["plant"][0])}
    for set_no, spec in CASES["review"].items():
        H, W = spec["size"]
        assert spec.get("s", 1) == 1                                            # the flow has the images' size
        assert max(H, W) < 1024                                                 # fp32 sample coordinates good to 3e-5 px
        for name, spots in spec["plant"].items():
            sizes["review {} {}".format(set_no, name)] = (H, W, spots)
    for key, (h, w, spots) in sizes.items():
        mt = _ceil(h * w, VIS_MAX_TILE)
        assert mt > threads and mt % threads, (key, mt)
        tiles = {n: pixel // VIS_MAX_TILE for n, pixel, _ in spots}
        assert sorted(tiles) == [0, 1] and all(0 <= pixel < h * w for _, pixel, _ in spots), key
        # one image's maximum behind the first trip of the fold, the other's in the first max-tile
        assert max(tiles.values()) >= threads and min(tiles.values()) == 0, (key, tiles)
    flo, flo_pred = (CASES["review"][1]["plant"][k] for k in ("flo", "flo_pred"))
    late = lambda spots: [n for n, pixel, _ in spots if pixel // VIS_MAX_TILE >= threads]
    assert late(flo) == [0] and late(flo_pred) == [1]                          # each vis_fold_max call needs its own
    # level 1 reads its partials behind level 0's: ws + mblk0[1] = B * mtiles[0]
    fh, fw = CASES["vis"]["levels"][0]
    assert len(CASES["vis"]["levels"]) == 2 and B * _ceil(fh * fw, VIS_MAX_TILE) >= 2 * threads
    widths = [(CASES["vis"]["levels"][0] if s is None else s)[1] for s in CASES["vis"]["pictures"].values()]
    assert any(ow > threads for ow in widths) and any(ow == threads for ow in widths)
    # no picture is resized across a tie of the nearest rule (ref_nearest_index asserts it)
    for size in CASES["vis"]["pictures"].values():
        for fh, fw in CASES["vis"]["levels"]:
            if size is not None:
                ref_nearest_index(size[0], fh), ref_nearest_index(size[1], fw)


def test_quality_case_folds_two_trips_of_images_and_of_tiles():
    q = CASES["quality"]
    per_trip = QUAL["kQualFoldThreads"] // WAVE
    assert q["B"] > per_trip and q["B"] % per_trip
    H, W = q["size"]
    oh, ow = H - 10, W - 10
    th, tw = QUAL["kQualTH"], QUAL["kQualTW"]
    tiles = _ceil(oh, th) * _ceil(ow, tw)
    assert WAVE < tiles < 2 * WAVE and tiles % WAVE
    last = (oh - (_ceil(oh, th) - 1) * th) * (ow - (_ceil(ow, tw) - 1) * tw)
    assert last > 0.01 * oh * ow, (last, oh * ow)


def test_cases_take_the_launch_form_they_test(hip_lib):
    from qpwcnet_amd import ops
    aligned = 1 << 20
    aug = CASES["augment"]
    assert ops.augment_kernel(B, *aug["vec4"]) == "augment_pixel_kernel<vec4>"
    assert ops.augment_kernel(B, *aug["scalar"]) == "augment_pixel_kernel<scalar>"
    assert ops.augment_kernel(B, aug["vec4"][0], aug["vec4"][1], aligned + 4, aligned + 4) == "augment_pixel_kernel<scalar>"
    forms = {"native": "flow_to_image_kernel<scalar>", "w256": "flow_to_image_kernel<vec4>"}
    for name, size in CASES["vis"]["pictures"].items():
        sizes = CASES["vis"]["levels"] if size is None else [size] * len(CASES["vis"]["levels"])
        for dtype in (torch.float32, torch.uint8):
            for layout in FORMATS:
                assert ops.flow_to_image_kernel(B, sizes, dtype, layout) == forms[name], (name, dtype, layout)
    H, W = CASES["review"][1]["size"]
    assert ops.review_panels_kernel(2, B, H, W) == "review_panels_kernel<scalar>"
    H, W = CASES["review"][2]["size"]
    assert ops.review_panels_kernel(1, B, H, W, H, W) == "review_panels_kernel<vec4>"
    q = CASES["quality"]
    assert ops.image_quality_kernel(q["B"], q["size"][0], q["size"][1], q["C"]) == "quality_tile_kernel"


# ---- 1. augmentation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["vec4", "scalar"])
def test_augment_torch_path_and_the_one_trip_mean(form):
    """augment_torch against ref_augment: images 2.3e-6 (vec4) and 2.5e-6 (scalar), flow 6.5e-6 and 7.4e-6 px.  The
    contrast mean over the first 256 * 256 output pixels alone -- what the fold gives after one trip -- moves the images
    of either sample by 1.2e-2 and the flow not at all."""
    case = augment_case(form)
    ims, flo, ip, fp, hw = case
    want = ref_augment(*case)
    for data_format in FORMATS:
        got = augment.augment_torch(torch.from_numpy(ims), torch.from_numpy(flo), as_params(ip, fp), hw,
                                    data_format=data_format)
        e_ims = max_err(got[0].numpy(), to_layout(want[0], "channels_last", data_format))
        e_flo = max_err(got[1].numpy(), to_layout(want[1], "channels_last", data_format))
        print("io-scale augment torch {} {}: max |ims err| {:.3e}, max |flow err| {:.3e} px".format(form, data_format,
                                                                                                   e_ims, e_flo))
        assert e_ims <= BOUND and e_flo <= BOUND
    threads = AUG["kAugThreads"]
    wrong = ref_augment(*case, mean_over_first=threads * threads)
    d = np.abs(wrong[0] - want[0]).reshape(B, -1).max(axis=1)
    print("io-scale augment {}: the one-trip mean moves the images by {}".format(form, d))
    assert d.min() > 10 * BOUND                                                 # in both samples
    assert np.array_equal(wrong[1], want[1])
    assert np.array_equal(ref_augment(*case, mean_over_first=hw[0] * hw[1])[0], want[0])      # the control's own check
    # the contrast factors are well away from 1, and the pixels behind the first trip differ in their mean
    assert (np.abs(fp[:, 5] - 1.0) > 0.25).all()
    plain = ref_augment(*case, colour=False)[0].reshape(B, -1, 6)
    head, tail = plain[:, :threads * threads].mean(axis=(1, 2)), plain[:, threads * threads:].mean(axis=(1, 2))
    assert np.abs(head - tail).min() > 0.1, (head, tail)


# ---- 2. flow panels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_flow_pictures_torch_path_and_the_cut_maximum(half):
    """flow_to_image_torch against the restatement at both picture sizes: 4.8e-7.  Without image 0's last pixel the rest
    of its picture moves by 0.69; image 1's does not move."""
    flows = vis_levels(half)
    imgs = [ref_flow_to_image(f.astype(np.float32)) for f in flows]
    for name, size in CASES["vis"]["pictures"].items():
        near = total = 0
        for data_format in FORMATS:
            for l, (f, img) in enumerate(zip(flows, imgs)):
                want = img if size is None else ref_nearest(img, size)
                t = tensor(to_layout(f, "channels_last", data_format))
                got = vis.flow_to_image_torch(t, data_format, size, torch.float32, "channels_last").numpy()
                assert got.shape == want.shape
                e = float(np.abs(got - want).max())
                print("io-scale vis torch {} {} {} level {}: max |err| {:.3e}".format(
                    "f16" if half else "f32", name, data_format, l, e))
                assert e <= BOUND
                if data_format == "channels_last":
                    # the uint8 rule of the GPU case: elements near a step of the conversion, at most 1 %
                    x = want * 255.5
                    close = np.abs(x - np.rint(x)) < 1e-3
                    u8 = vis.flow_to_image_torch(t, data_format, size, torch.uint8, "channels_last").numpy()
                    diff = np.abs(u8.astype(np.int64) - ref_uint8(want).astype(np.int64))
                    assert diff.max() <= 1 and not diff[~close].any()
                    near, total = near + int(close.sum()), total + close.size
        print("io-scale vis uint8 {}: {:.3f} % of the elements near a step".format(name, 100.0 * near / total))
        assert near <= 0.01 * total
    cut = flows[0].astype(np.float32)
    cut[0, -1, -1] = 0.0
    other = ref_flow_to_image(cut)
    d = float(np.abs(imgs[0][0].reshape(-1, 3)[:-1] - other[0].reshape(-1, 3)[:-1]).max())
    print("io-scale vis: the restatement without the last pixel differs by {:.3e}".format(d))
    assert d > 1000 * BOUND and np.array_equal(imgs[0][1], other[1])


# ---- 3. review panels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_no", [1, 2])
def test_review_torch_path_and_the_cut_maxima(set_no):
    """The fixtures meet the fixture condition; the fp32 torch composition is within BOUND / 4 of the restatement
    (4.8e-7 for both sets); each flow picture without the vector planted behind the fold's first trip moves by 0.64 to
    0.68."""
    spec = CASES["review"][set_no]
    case = review_case(set_no)
    for name in spec["plant"]:
        assert margin_ok(case[name], 1)
        share = outside_share(case[name], 1)                                    # asserts that every side is left
        print("io-scale review set {} {}: {:.2f} % of the samples leave the image".format(set_no, name, 100 * share))
        assert 0.002 < share < 0.05
    want = review_reference(set_no, case)
    for data_format in FORMATS:
        _, got = run_panels(set_no, case, data_format, data_format, torch.float32, spec["grid"])
        err = float_error(got, want)
        print("io-scale review torch set {} {}: max |err| {:.3e}".format(set_no, data_format, err))
        assert err <= BOUND / 4
    pictures = {"flo": "flo_rgb", "flo_pred": "flo_pred_rgb", "flow": "5-flow"}
    for name, spots in spec["plant"].items():
        (n, pixel, _), = [s for s in spots if s[1] // VIS_MAX_TILE >= VIS["kVisThreads"]]
        cut = case[name].copy()
        cut[n].reshape(-1, 2)[pixel] = 0.0
        other = ref_flow_to_image(cut)
        full = ref_flow_to_image(case[name])                                    # the picture before the grid
        if not spec["grid"]:
            assert np.array_equal(full, want[pictures[name]])
        rest = np.arange(full[n].shape[0] * full[n].shape[1]) != pixel
        d = float(np.abs(full[n].reshape(-1, 3)[rest] - other[n].reshape(-1, 3)[rest]).max())
        print("io-scale review set {}: {} without its planted vector differs by {:.3e}".format(set_no, name, d))
        assert d > 1000 * BOUND and np.array_equal(full[1 - n], other[1 - n])


# ---- 4. PSNR / SSIM -------------------------------------------------------------------------------------------------
def test_quality_torch_path_and_the_dropped_trips():
    """image_quality_torch against ref_quality at B = 19: mse 5.2e-8 relative, psnr 8.5e-7 dB, ssim 2.5e-8.  The images
    differ from their neighbours and from the image sixteen places on; a fold without tile 64, lane 0's second trip,
    misses ssim by 6.3e-3 to 1.3e-2 and mse by 2.4 to 2.7 %; a state without the second trip of images misses every sum
    by more than 1 %."""
    truth, pred = quality_case()
    n = CASES["quality"]["B"]
    want = ref_quality(truth, pred)
    res = metrics.image_quality(tensor(truth), tensor(pred), data_format="channels_last")
    assert all(v.dtype == torch.float32 and tuple(v.shape) == (n,) for v in res)
    check("torch io-scale", [v.numpy() for v in res], want)
    mse, _, ssim = want
    per_trip = QUAL["kQualFoldThreads"] // WAVE
    for step in (1, per_trip):                              # a batch-index mix-up shows, across the trip boundary too
        assert (np.abs(mse[step:] / mse[:-step] - 1.0) > 0.05).all(), step
        assert (np.abs(ssim[step:] - ssim[:-step]) > 1e-3).all(), step
    vt, vp = truth.astype(np.float64), pred.astype(np.float64)
    s = ref_ssim_map(vt, vp, 1.0)
    th, tw = QUAL["kQualTH"], QUAL["kQualTW"]
    y0, x0 = (_ceil(s.shape[1], th) - 1) * th, (_ceil(s.shape[2], tw) - 1) * tw
    cut = s.copy()
    cut[:, y0:, x0:] = 0.0
    positions = s.shape[1] * s.shape[2]
    d_ssim = np.abs(cut.sum(axis=(1, 2)).mean(axis=1) / positions - ssim)
    # the last tile also owns the squared errors of the rim behind it
    sq = (vt - vp) ** 2
    d_mse = sq[:, y0:, x0:].sum(axis=(1, 2, 3)) / sq[0].size / mse
    print("io-scale quality: without tile 64 ssim moves by {:.2e}..{:.2e}, mse by {:.2e}..{:.2e} (relative)".format(
        d_ssim.min(), d_ssim.max(), d_mse.min(), d_mse.max()))
    assert d_ssim.min() > 10 * BOUNDS["ssim"] and d_mse.min() > 1000 * BOUNDS["mse"]
    for v in res:
        total, first = float(v.double().sum()), float(v[:per_trip].double().sum())
        assert abs(first / total - 1.0) > 0.01                  # the state's check is 1e-12 relative

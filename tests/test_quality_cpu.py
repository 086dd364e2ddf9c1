"""PSNR and SSIM of the frame interpolator (qpwcnet_amd/metrics.py, qpwc_image_quality_fwd) without a GPU:
  * ``ref_quality``: a float64 numpy restatement of include/qpwc_quality.h -- the value transform, the mean squared
    error, tf.image.psnr, tf.image.ssim with its default 11-tap Gaussian -- the contract the kernels are held to
    (tests/test_gpu_quality.py imports it and the CASES below).  The 8-bit transform alone is evaluated in float32,
    because the contract defines it there;
  * closed forms that do not depend on the restatement (constant images, identical images);
  * ``metrics.image_quality_torch``, the path CPU tensors take, on every case of the GPU suite;
  * the public surface, the ctypes table against its header, and the workspace query.
Bounds (BOUNDS): ssim 1e-4 absolute, the project's kernel bound; mse 1e-5 relative; psnr 1e-4 dB absolute, which follows
from the mse bound (10 / ln 10 * 1e-5 = 4.3e-5 dB).  An fp32 chain stays about a factor of ten inside them on inputs of
the kind used here (smooth images with a little texture); the worst case is a pair of constant images, where
den1 - den0 cancels against c2 (3.2e-5 in ssim for 0.3 against 0.4)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

from qpwcnet_amd import _hip, metrics  # noqa: E402

QUALITY_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qpwc_quality.h")
BOUNDS = {"ssim": 1e-4, "mse": 1e-5, "psnr": 1e-4}
TH, TW = _hip.QUALITY_TILE
B = 2
SMALL, ODD, TILES = (11, 11), (12, 27), (TH + 11, 2 * TW + 13)
LIMIT = (1 << 31) - 1


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_window():
    k = np.arange(11, dtype=np.float64)
    e = np.exp(-(k - 5.0) ** 2 / 4.5)
    return (e / e.sum()).astype(np.float32).astype(np.float64)


def ref_value(x, offset, max_val, clip, quantize):
    if quantize:       # in float32, as the contract states it: the sum, the product and the truncation each rounded
        v = np.asarray(x, np.float32) + np.float32(offset)
        return np.trunc(np.float32(255.0) * np.clip(v, np.float32(0.0), np.float32(1.0))).astype(np.float64)
    v = np.asarray(x, np.float32).astype(np.float64) + float(np.float32(offset))
    return np.clip(v, 0.0, float(np.float32(max_val))) if clip else v


def ref_conv(x):
    """VALID correlation of (B,H,W,C) with g (x) g: along W, then along H."""
    g = ref_window()
    ow, oh = x.shape[2] - 10, x.shape[1] - 10
    rows = sum(g[k] * x[:, :, k:k + ow] for k in range(11))
    return sum(g[k] * rows[:, k:k + oh] for k in range(11))


def ref_ssim_map(vt, vp, max_val):
    """s at every position: (B,H-10,W-10,C) from the float64 values (B,H,W,C)."""
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mt, mp = ref_conv(vt), ref_conv(vp)
    num0, den0 = 2.0 * mt * mp, mt * mt + mp * mp
    num1, den1 = 2.0 * ref_conv(vt * vp), ref_conv(vt * vt + vp * vp)
    return (num0 + c1) / (den0 + c1) * ((num1 - num0 + c2) / (den1 - den0 + c2))


def ref_quality(truth, pred, max_val=1.0, offset=(0.0, 0.0), clip=False, quantize=False, data_format="channels_last"):
    """-> (mse, psnr, ssim), float64 [B] each, of numpy images (B,H,W,C) / (B,C,H,W), float32 or float16."""
    if data_format == "channels_first":
        truth, pred = np.transpose(truth, (0, 2, 3, 1)), np.transpose(pred, (0, 2, 3, 1))
    max_val = 255.0 if quantize else float(np.float32(max_val))
    vt = ref_value(truth, offset[0], max_val, clip, quantize)
    vp = ref_value(pred, offset[1], max_val, clip, quantize)
    mse = ((vt - vp) ** 2).mean(axis=(1, 2, 3))
    with np.errstate(divide="ignore"):
        psnr = 20.0 * math.log10(max_val) - 10.0 * np.log10(mse)
    return mse, psnr, ref_ssim_map(vt, vp, max_val).mean(axis=(1, 2)).mean(axis=1)


# ---- the inputs -----------------------------------------------------------------------------------------------------
def make_images(seed, hw, C, amplitude=0.35, batch=B, sigmas=(0.04, 0.08)):
    """(truth, pred), float32 (batch,H,W,C) in about [0, 1]: a smooth sinusoid plus N(0, 0.05^2) texture; the prediction
    is the truth plus N(0, sigmas[n]^2) in image n (0.04 in image 0 and 0.08 in image 1), and the images differ in
    content."""
    assert len(sigmas) == batch
    rng = np.random.default_rng(seed)
    H, W = hw
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    truth = np.empty((batch, H, W, C))
    for n in range(batch):
        for c in range(C):
            truth[n, :, :, c] = 0.5 + amplitude * np.sin(2 * math.pi * ((1.0 + n) * y + (1.5 - 0.5 * n) * x) + 0.7 * c + n)
    truth += 0.05 * rng.standard_normal(truth.shape)
    pred = truth + rng.standard_normal(truth.shape) * np.asarray(sigmas).reshape(batch, 1, 1, 1)
    return truth.astype(np.float32), pred.astype(np.float32)


def tiled_images(seed=3):
    """The TILES case: two tile rows and three tile columns of positions, the last ones partial (one row, three columns);
    a bright patch centred on the last SSIM position, a single large error at pixel (0, 0) and at (H - 1, W - 1) -- so
    a dropped last tile shows in ssim, and a rim pixel that is dropped or counted twice shows in mse."""
    H, W = TILES
    assert (H - 10) == TH + 1 and (W - 10) == 2 * TW + 3, "TILES no longer ends in one row and three columns of positions"
    truth, pred = make_images(seed, TILES, 3)
    cy, cx = H - 11 + 5, W - 11 + 5                  # the centre of the last position's window
    truth[:, cy - 2:cy + 3, cx - 2:cx + 3] += 0.4
    pred[:, cy - 2:cy + 3, cx - 2:cx + 3] += 0.25
    pred[0, 0, 0] += 3.0
    pred[1, 0, 0] -= 2.0
    pred[0, H - 1, W - 1] -= 2.5
    pred[1, H - 1, W - 1] += 3.5
    return truth, pred


def away_from_steps(x, offset):
    """x nudged upwards until no element has 255 * clamp(x + offset) within 1e-3 of a whole number (float32 inputs)."""
    x = x.copy()
    for _ in range(50):
        v = np.clip(x + np.float32(offset), np.float32(0), np.float32(1)).astype(np.float64) * 255.0
        near = np.abs(v - np.rint(v)) < 1.5e-3
        if not near.any():
            return x
        x[near] += np.float32(4e-3 / 255.0)
    raise AssertionError("could not move every element away from the 8-bit steps")


def near_a_step(x, offset):
    v = np.clip(np.asarray(x, np.float32) + np.float32(offset), np.float32(0), np.float32(1)).astype(np.float64) * 255.0
    return np.abs(v - np.rint(v)) < 1e-3


def tensor(a):
    """A torch tensor holding a copy of a (possibly read-only) numpy array."""
    return torch.from_numpy(np.array(a))


def _case(truth, pred, data_format="channels_last", half=(False, False), **kw):
    if data_format == "channels_first":
        truth, pred = (np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))) for a in (truth, pred))
    truth, pred = (a.astype(np.float16) if h else a for a, h in zip((truth, pred), half))
    return dict(truth=truth, pred=pred, data_format=data_format, kw=kw)


def _build_cases():
    cases = {"11x11": _case(*make_images(0, SMALL, 3)),
             "12x27": _case(*make_images(1, ODD, 3)),
             "tiles": _case(*tiled_images()),
             "c1": _case(*make_images(4, ODD, 1)),
             "c4": _case(*make_images(5, ODD, 4)),
             "tiles_channels_first": _case(*tiled_images(), data_format="channels_first"),
             "tiles_f16_truth": _case(*tiled_images(), half=(True, False)),
             "tiles_f16_pred": _case(*tiled_images(), half=(False, True))}
    # the interpolator's range, [-0.5, 0.5]; with an amplitude of 0.55 about a tenth of the elements leave [0, 1]
    t, p = make_images(6, TILES, 3, amplitude=0.55)
    assert 0.02 < float(((t < 0) | (t > 1)).mean()) < 0.5
    cases["clip"] = _case(t - np.float32(0.5), p - np.float32(0.5), offset=(0.5, 0.5), clip=True)
    # quantize: every element strictly inside (0, 1) and away from the 8-bit steps, so nothing is left out
    t, p = make_images(7, TILES, 3, amplitude=0.2)
    t, p = (away_from_steps(np.clip(a, 0.02, 0.98) - np.float32(0.5), 0.5) for a in (t, p))
    cases["quantize"] = _case(t, p, offset=(0.5, 0.5), quantize=True)
    for c in cases.values():
        c["truth"].setflags(write=False)
        c["pred"].setflags(write=False)
    return cases


CASES = _build_cases()
_REF = {}


def reference(name):
    """ref_quality of a case, computed once and left unchanged."""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = ref_quality(c["truth"], c["pred"], data_format=c["data_format"], **c["kw"])
        for a in _REF[name]:
            a.setflags(write=False)
    return _REF[name]


def errors(got, want):
    """{'mse' (relative), 'psnr' (dB), 'ssim'}: the largest error over the batch of (mse, psnr, ssim) against float64."""
    mse, psnr, ssim = (np.asarray(g, np.float64) for g in got)
    return {"mse": float(np.max(np.abs(mse - want[0]) / want[0])), "psnr": float(np.max(np.abs(psnr - want[1]))),
            "ssim": float(np.max(np.abs(ssim - want[2])))}


def check(label, got, want):
    err = errors(got, want)
    print("quality {}: mse {:.2e} (rel)  psnr {:.2e} dB  ssim {:.2e}".format(label, err["mse"], err["psnr"], err["ssim"]))
    for k, bound in BOUNDS.items():
        assert err[k] <= bound, (label, k, err[k])
    return err


def run_case(name, device="cpu", fn=None):
    c = CASES[name]
    fn = metrics.image_quality if fn is None else fn
    res = fn(tensor(c["truth"]).to(device), tensor(c["pred"]).to(device),
             data_format=c["data_format"], **c["kw"])
    return res, [v.cpu().numpy() for v in res]


# ---- the cases are what they are chosen for -------------------------------------------------------------------------
def test_the_cases_have_their_properties():
    assert CASES["11x11"]["truth"].shape == (B, 11, 11, 3) and CASES["12x27"]["truth"].shape == (B, 12, 27, 3)
    H, W = TILES
    assert -(-(H - 10) // TH) == 2 and -(-(W - 10) // TW) == 3 and (H - 10) % TH == 1 and (W - 10) % TW == 3
    assert CASES["tiles_channels_first"]["truth"].shape == (B, 3, H, W)
    assert CASES["tiles_f16_truth"]["truth"].dtype == np.float16 and CASES["tiles_f16_truth"]["pred"].dtype == np.float32
    assert CASES["tiles_f16_pred"]["truth"].dtype == np.float32 and CASES["tiles_f16_pred"]["pred"].dtype == np.float16
    assert CASES["c1"]["truth"].shape[3] == 1 and CASES["c4"]["truth"].shape[3] == 4
    q = CASES["quantize"]
    assert not near_a_step(q["truth"], 0.5).any() and not near_a_step(q["pred"], 0.5).any()      # share left out: zero
    for name in CASES:                      # the two images of a batch differ in content and in error level
        mse, _, ssim = reference(name)
        assert abs(mse[1] / mse[0] - 1.0) > 0.2, name
        assert abs(ssim[0] - ssim[1]) > 1e-3, name


def test_the_comparison_sees_the_planted_defects():
    """A kernel that dropped the sums of the last tile row, of the last tile column or of the corner tile alone (1 x 3
    positions), or that dropped or doubled a corner pixel of the rim, would miss the TILES case by far more than the
    bounds."""
    c = CASES["tiles"]
    mse, _, ssim = reference("tiles")
    vt, vp = c["truth"].astype(np.float64), c["pred"].astype(np.float64)
    s = ref_ssim_map(vt, vp, 1.0)
    positions = s.shape[1] * s.shape[2]
    assert np.allclose(s.mean(axis=(1, 2)).mean(axis=1), ssim, rtol=1e-12)
    for rows, cols in ((slice(TH, None), slice(None)), (slice(None), slice(2 * TW, None)),
                       (slice(TH, None), slice(2 * TW, None))):
        cut = s.copy()
        cut[:, rows, cols] = 0.0
        assert cut[0, rows, cols].size in (3 * (2 * TW + 3), 3 * 3 * (TH + 1), 9)
        assert np.abs(cut.sum(axis=(1, 2)).mean(axis=1) / positions - ssim).min() > 10 * BOUNDS["ssim"]
    for y, x in ((0, 0), (-1, -1)):
        share = ((vt[:, y, x] - vp[:, y, x]) ** 2).sum(axis=1) / vt[0].size / mse
        assert share.min() > 1000 * BOUNDS["mse"], share


# ---- closed forms ---------------------------------------------------------------------------------------------------
CONSTANTS = [(0.3, 0.4, 1.0), (0.1, 0.2, 1.0), (90.0, 120.0, 255.0)]


@pytest.mark.parametrize("a,b,max_val", CONSTANTS)
def test_constant_images(a, b, max_val):
    """The variance terms cancel: ssim = (2ab + c1) / (a^2 + b^2 + c1), mse = (a - b)^2.  In fp32 den1 and den0 are
    each a^2 + b^2 to a few units of 2^-24, and their difference stands beside c2 alone: the error in s is about
    (a^2 + b^2) / c2 * 1.2e-7.  The levels are chosen with that ratio below 400 (278, 56, 385), which leaves half of the
    1e-4 bound; for 0.25 against 0.75 (ratio 694) no fp32 chain of this form meets it."""
    assert (a * a + b * b) / (0.03 * max_val) ** 2 < 400
    t, p = np.full((B, 13, 17, 3), a, np.float32), np.full((B, 13, 17, 3), b, np.float32)
    a, b = float(np.float32(a)), float(np.float32(b))
    c1 = (0.01 * max_val) ** 2
    want = (np.full(B, (a - b) ** 2), np.full(B, 20 * math.log10(max_val) - 20 * math.log10(abs(a - b))),
            np.full(B, (2 * a * b + c1) / (a * a + b * b + c1)))
    ref = ref_quality(t, p, max_val)
    # the rounded taps sum to 1 - 1.4e-9, which the cancelling terms magnify: the restatement is within 1e-6 of the form
    assert all(np.allclose(r, w, rtol=1e-5, atol=0) for r, w in zip(ref, want))
    got = metrics.image_quality(tensor(t), tensor(p), max_val=max_val, data_format="channels_last")
    check("constant {} {}".format(a, b), [v.numpy() for v in got], want)


def test_identical_images():
    t = tensor(CASES["12x27"]["truth"])
    res = metrics.image_quality(t, t, data_format="channels_last")
    assert bool((res.mse == 0).all()) and bool(torch.isinf(res.psnr).all()) and bool((res.psnr > 0).all())
    assert float((res.ssim - 1).abs().max()) <= BOUNDS["ssim"]
    mse, psnr, ssim = ref_quality(t.numpy(), t.numpy())
    assert (mse == 0).all() and np.isposinf(psnr).all() and np.abs(ssim - 1).max() < 1e-12


# ---- the torch path on every case of the GPU suite ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_torch_path_against_the_restatement(name):
    res, got = run_case(name)
    assert isinstance(res, metrics.ImageQuality) and res._fields == ("mse", "psnr", "ssim")
    assert all(v.dtype == torch.float32 and tuple(v.shape) == (B,) for v in res)
    check("torch " + name, got, reference(name))


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_psnr_and_ssim_wrappers():
    c = CASES["12x27"]
    t, p = tensor(c["truth"]), tensor(c["pred"])
    res = metrics.image_quality(t, p, data_format="channels_last")
    assert torch.equal(metrics.psnr(t, p, 1.0), res.psnr) and torch.equal(metrics.ssim(t, p, 1.0), res.ssim)
    assert torch.equal(metrics.ssim(t, p, 1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03), res.ssim)
    two = metrics.image_quality(t, p, max_val=2.0, data_format="channels_last")
    assert float((two.psnr - res.psnr - 20 * math.log10(2.0)).abs().max()) < 1e-4 and bool((two.ssim > res.ssim).all())
    one = metrics.image_quality(t[1], p[1], data_format="channels_last")                     # rank 3: one image
    assert all(v.dim() == 0 for v in one) and all(torch.equal(a, b[1]) for a, b in zip(one, res))
    from qpwcnet_amd import backend
    assert backend.image_data_format() == "channels_last" and torch.equal(metrics.image_quality(t, p).ssim, res.ssim)
    pair = metrics.image_quality(t - 0.25, p, offset=(0.25, 0.0))
    assert float((pair.mse - res.mse).abs().max()) < 1e-7
    for kw in (dict(filter_size=7), dict(filter_sigma=1.0), dict(k1=0.02), dict(k2=0.05)):
        with pytest.raises(ValueError, match="filter_size.*11"):
            metrics.ssim(t, p, 1.0, **kw)


def test_refusals():
    ok = torch.zeros(1, 11, 11, 3)
    for shape in ((1, 10, 64, 3), (1, 64, 10, 3)):
        with pytest.raises(ValueError, match="filter size"):
            metrics.image_quality(torch.zeros(shape), torch.zeros(shape), data_format="channels_last")
    with pytest.raises(ValueError, match="filter size"):
        metrics.image_quality(torch.zeros(1, 3, 64, 10), torch.zeros(1, 3, 64, 10), data_format="channels_first")
    with pytest.raises(ValueError, match="one shape"):
        metrics.image_quality(ok, torch.zeros(1, 11, 12, 3))
    with pytest.raises(ValueError, match="channels"):
        metrics.image_quality(torch.zeros(1, 11, 11, 5), torch.zeros(1, 11, 11, 5))
    with pytest.raises(ValueError, match="dtype"):
        metrics.image_quality(ok.double(), ok.double())
    with pytest.raises(ValueError, match="Unsupported data format"):
        metrics.image_quality(ok, ok, data_format="nhwc")
    with pytest.raises(ValueError, match="max_val"):
        metrics.image_quality(ok, ok, max_val=0.0)
    with pytest.raises(ValueError, match="state"):
        metrics.image_quality(ok, ok, state=torch.zeros(4))
    with pytest.raises(ValueError, match="one device"):
        metrics.image_quality(ok, ok.to("meta"))


def test_no_gradient_flows():
    c = CASES["11x11"]
    t, p = tensor(c["truth"]), tensor(c["pred"]).requires_grad_(True)
    res = metrics.image_quality(t, p * 1.0, data_format="channels_last")
    assert not any(v.requires_grad for v in res)


def test_interpolation_quality_is_the_mean_over_all_images():
    """Two batches through one state equal the concatenated batch; the defaults score the 8-bit pictures of images in
    [-0.5, 0.5]."""
    q = CASES["quantize"]
    t, p = tensor(q["truth"]), tensor(q["pred"])
    t2, p2 = t.flip(0) * 0.9, p.flip(0) * 0.8
    m = metrics.InterpolationQuality(data_format="channels_last")
    assert m.result() == {"mse": 0.0, "psnr": 0.0, "ssim": 0.0}
    per = m.update_state(t, p)
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(per, run_case("quantize")[0]))
    m.update_state(t2, p2)
    assert m.state.dtype == torch.float64 and float(m.state[3]) == 2 * B
    both = metrics.image_quality(torch.cat([t, t2]), torch.cat([p, p2]), offset=0.5, quantize=True,
                                 data_format="channels_last")
    res = m.result()
    assert sorted(res) == ["mse", "psnr", "ssim"]
    for k, v in zip(("mse", "psnr", "ssim"), both):
        assert abs(res[k] - float(v.double().mean())) <= 1e-12 * abs(res[k]), k
    assert abs(res["psnr"] - float(np.mean(np.concatenate([reference("quantize")[1], both.psnr[B:].numpy()])))) < 1e-3
    m.reset_state()
    assert m.result() == {"mse": 0.0, "psnr": 0.0, "ssim": 0.0} and float(m.state[3]) == 0.0
    m.update_state(t2, p2)
    assert abs(m.result()["ssim"] - float(both.ssim[B:].double().mean())) < 1e-12


# ---- header and table -----------------------------------------------------------------------------------------------
NAMES = ["qpwc_image_quality_workspace_floats", "qpwc_image_quality_fwd", "qpwc_image_quality_fwd_kernel"]


def test_quality_prototypes_match_their_header():
    protos = parse_header(QUALITY_HEADER)
    assert [name for name, _, _ in protos] == NAMES
    assert mismatches(_hip.QUALITY_PROTOTYPES, protos) == []
    others = (set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES) | set(_hip.TRIPLET_PROTOTYPES) | set(_hip.VIS_PROTOTYPES))
    assert len(_hip.SYMBOLS) == 77 and not set(_hip.QUALITY_PROTOTYPES) & others
    table = dict(_hip.QUALITY_PROTOTYPES)
    restype, argtypes = table["qpwc_image_quality_fwd"]
    table["qpwc_image_quality_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_image_quality_fwd: 17 parameters, table has 16"]
    assert (_hip.QUALITY_CLIP, _hip.QUALITY_U8) == (1, 2)
    with open(QUALITY_HEADER) as f:
        text = f.read()
    assert "#define QPWC_QUALITY_CLIP 1" in text and "#define QPWC_QUALITY_U8 2" in text


def test_the_library_exports_the_table(hip_lib):
    for name, (restype, argtypes) in _hip.QUALITY_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


# ---- the queries (host only) ----------------------------------------------------------------------------------------
def test_workspace_query(hip_lib):
    """C + 1 floats per image and tile of QUALITY_TILE positions: it grows by one tile's floats exactly when H - 10 or
    W - 10 passes a multiple of the tile, and scales with B."""
    q = hip_lib.qpwc_image_quality_workspace_floats
    assert (TH, TW) == (16, 32)
    for C in (1, 3, 4):
        per = C + 1
        assert q(1, 11, 11, C) == per and q(1, 10 + TH, 10 + TW, C) == per
        assert q(1, 10 + TH + 1, 10 + TW, C) == 2 * per and q(1, 10 + TH, 10 + TW + 1, C) == 2 * per
        assert q(1, 10 + 2 * TH, 10 + 2 * TW, C) == 4 * per and q(1, 10 + 2 * TH + 1, 10 + 2 * TW, C) == 6 * per
        assert q(1, 10 + 2 * TH, 10 + 2 * TW + 1, C) == 6 * per
        for b in (2, 16):
            assert q(b, TILES[0], TILES[1], C) == b * 6 * per
    assert q(16, 256, 512, 3) == 16 * 16 * 16 * 4                                  # the trainer's shape
    for bad in ((0, 11, 11, 3), (-1, 11, 11, 3), (1, 10, 11, 3), (1, 11, 10, 3), (1, 11, 11, 0), (1, 11, 11, 5)):
        assert q(*bad) == _hip.E_SHAPE, bad
    assert q(LIMIT // 121, 11, 11, 1) == 2 * (LIMIT // 121) and q(LIMIT // 121 + 1, 11, 11, 1) == _hip.E_SHAPE


def test_kernel_query_is_host_only(hip_lib):
    from qpwcnet_amd import ops
    q = lambda *a: hip_lib.qpwc_image_quality_fwd_kernel(*a).decode()
    assert q(16, 256, 512, 3) == "quality_tile_kernel" and q(B, TILES[0], TILES[1], 3) == "quality_tile_kernel"
    assert q(1, 11, 11, 1) == "quality_tile_kernel" and q(1, 11, 11, 4) == "quality_tile_kernel"
    for bad in ((0, 11, 11, 3), (1, 10, 64, 3), (1, 64, 10, 3), (1, 11, 11, 0), (1, 11, 11, 5),
                (LIMIT // 121 + 1, 11, 11, 1)):
        assert q(*bad) == "", bad
    assert ops.image_quality_kernel(B, 43, 77, 3) == "quality_tile_kernel" and ops.image_quality_kernel(B, 10, 64, 3) == ""

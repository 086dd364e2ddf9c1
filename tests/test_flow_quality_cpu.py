"""The flow evaluation metrics (qpwcnet_amd/metrics.py flow_quality / FlowQuality, qpwc_flow_quality_fwd) without a GPU:
  * ``ref_flow_quality``: a float64 numpy restatement of include/qpwc_flow_quality.h -- end-point error, ground-truth
    speed, the atan2 form of the angular error, validity, the outlier rule, the accuracy counts, the occlusion and speed
    splits -- the contract the kernels are held to (tests/test_gpu_flow_quality.py imports it and the CASES below);
  * a closed form that does not depend on the restatement (truth (3, 4) everywhere, prediction 0);
  * ``metrics.flow_quality_torch``, the path CPU tensors take, on every case of the GPU suite;
  * the running state, its pixel-weighted result and its sum over two gloo ranks;
  * the public surface, the ctypes table against its header, and the two queries.
Bounds: the counts and their ratios (fl, acc1, acc3, acc5, valid) to the fp32 rounding of the quotient (1 ulp) -- no
valid pixel of any case lies within 1e-3 of a threshold, so no count may differ; the EPE-type means 1e-4 px absolute, the
project's kernel bound; aae 1e-3 degrees (an fp32 ulp at 180 degrees is 1.5e-5: room for a few-ulp atan2f and the
conversion, none for acosf of the normalised dot product, which is 0.03 degrees off per pixel on nearly equal flows and
3.4e-3 in the mean of the near_equal case).
Measured, the torch fp32 composition on the CPU, the largest error over the eleven cases: 1.8e-6 px (unknown_gt) in the
EPE-type means and 5.8e-7 degrees in aae (3x5); every count ratio the rounded float64 quotient (at most 0.5 ulp).  The
kernels on an MI355X: 1.8e-6 px and 5.2e-7 degrees (tests/test_gpu_flow_quality.py)."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

from qpwcnet_amd import _hip, metrics  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qpwc_flow_quality.h")
CHUNK = _hip.FLOW_QUALITY_CHUNK
B = 2
LIMIT = (1 << 31) - 1
FIELDS = ("epe", "aae", "fl", "acc1", "acc3", "acc5", "epe_noc", "epe_occ", "epe_s0_10", "epe_s10_40", "epe_s40", "valid")
COUNT_FIELDS = ("fl", "acc1", "acc3", "acc5", "valid")
EPE_FIELDS = ("epe", "epe_noc", "epe_occ", "epe_s0_10", "epe_s10_40", "epe_s40")
BOUNDS = {"epe": 1e-4, "aae": 1e-3}
OUTLIER, ACCURACY, SPEED = (3.0, 0.05), (1.0, 3.0, 5.0), (10.0, 40.0)
MARGIN = 1e-3                       # no valid pixel of a case is nearer to a threshold


def chunks_shape():
    """(H, W) with H * W = 2 CHUNK + 3 and an odd width; were that number prime, the nearest larger one that factors."""
    n = 2 * CHUNK + 3
    while True:
        for w in range(int(math.isqrt(n)) | 1, 2, -2):
            if n % w == 0:
                return n // w, w
        n += 1


SMALL, WAVE, CHUNKS, NEAR = (1, 1), (3, 5), chunks_shape(), (5, 7)
LAST = CHUNKS[0] * CHUNKS[1] - 2 * CHUNK        # the pixels of the last chunk


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_sums(truth, pred, valid=None, occluded=None, outlier=OUTLIER, accuracy=ACCURACY, speed=SPEED):
    """float64 [B, 15]: the sums of include/qpwc_flow_quality.h of channels-last numpy flows (B,H,W,2), in float64."""
    t, p = np.asarray(truth).astype(np.float64), np.asarray(pred).astype(np.float64)
    u, v, up, vp = t[..., 0], t[..., 1], p[..., 0], p[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        du, dv = u - up, v - vp
        e, m, c = np.sqrt(du * du + dv * dv), np.sqrt(u * u + v * v), u * vp - v * up
        ang = np.degrees(np.arctan2(np.sqrt(du * du + dv * dv + c * c), u * up + v * vp + 1.0))
        ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) <= 1e9) & (np.abs(v) <= 1e9)
    if valid is not None:
        ok &= np.asarray(valid) != 0
    occ = ok & (np.asarray(occluded) != 0) if occluded is not None else np.zeros_like(ok)
    e, ang, m = (np.where(ok, a, 0.0) for a in (e, ang, m))
    bins = (ok & (m < speed[0]), ok & (m >= speed[0]) & (m < speed[1]), ok & (m >= speed[1]))
    count = lambda mask: mask.sum(axis=(1, 2)).astype(np.float64)
    total = lambda x, mask: np.where(mask, x, 0.0).sum(axis=(1, 2))
    cols = [count(ok), total(e, ok), total(ang, ok), count(ok & (e > outlier[0]) & (e > outlier[1] * m))]
    cols += [count(ok & (e < a)) for a in accuracy]
    cols += [count(occ), total(e, occ)]
    for b in bins:
        cols += [count(b), total(e, b)]
    return np.stack(cols, axis=1)


def ref_scores(sums, pixels):
    """{field: float64 [...]} from sums [..., 15]; 0 / 0 is NaN."""
    s = [sums[..., i] for i in range(15)]
    with np.errstate(invalid="ignore", divide="ignore"):
        vals = (s[1] / s[0], s[2] / s[0], s[3] / s[0], s[4] / s[0], s[5] / s[0], s[6] / s[0], (s[1] - s[8]) / (s[0] - s[7]),
                s[8] / s[7], s[10] / s[9], s[12] / s[11], s[14] / s[13], s[0] / pixels)
    return dict(zip(FIELDS, (np.asarray(x, np.float64) for x in vals)))


def ref_flow_quality(truth, pred, valid=None, occluded=None, outlier=OUTLIER, accuracy=ACCURACY, speed=SPEED,
                     data_format="channels_last"):
    """-> {field: float64 [B]} of numpy flows (B,H,W,2) / (B,2,H,W); truth float32, pred float32 or float16."""
    if data_format == "channels_first":
        truth, pred = np.transpose(truth, (0, 2, 3, 1)), np.transpose(pred, (0, 2, 3, 1))
    return ref_scores(ref_sums(truth, pred, valid, occluded, outlier, accuracy, speed), truth.shape[1] * truth.shape[2])


# ---- the inputs -----------------------------------------------------------------------------------------------------
def near_a_threshold(truth, pred, valid=None, outlier=OUTLIER, accuracy=ACCURACY, speed=SPEED, which="any"):
    """bool (B,H,W): the valid pixels within MARGIN of a threshold, in float64 (channels-last arrays); which = "speed":
    of a threshold of the ground-truth speed alone."""
    t, p = np.asarray(truth).astype(np.float64), np.asarray(pred).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.hypot(t[..., 0] - p[..., 0], t[..., 1] - p[..., 1])
        m = np.hypot(t[..., 0], t[..., 1])
        ok = np.isfinite(t).all(axis=-1) & (np.abs(t) <= 1e9).all(axis=-1)
        near = np.zeros_like(ok)
        for x in speed:
            near |= np.abs(m - x) < MARGIN
        if which != "speed":
            for x in tuple(accuracy) + (outlier[0],):
                near |= np.abs(e - x) < MARGIN
            near |= np.abs(e - outlier[1] * m) < MARGIN
    if valid is not None:
        ok &= np.asarray(valid) != 0
    return near & ok


def away_from_thresholds(truth, pred, dtype=np.float32):
    """(truth, pred cast to dtype) with every offending pixel moved by 0.01 px at a time until no pixel lies within MARGIN
    of a threshold: the prediction alone where the error is the offender, the truth and the prediction together (the
    error stays) where the ground-truth speed is.  Nothing is left out of any comparison."""
    truth, shadow = truth.copy(), pred.astype(np.float32).copy()
    for _ in range(400):
        out = shadow.astype(dtype)
        near = near_a_threshold(truth, out)
        if not near.any():
            return truth, out
        speed = near_a_threshold(truth, out, which="speed")
        truth[speed, 0] += np.float32(0.01)
        shadow[near, 0] += np.float32(0.01)
    raise AssertionError("could not move every pixel away from the thresholds")


def make_flows(seed, hw, sigmas=(0.3, 4.0), amplitude=(45.0, 25.0), batch=B):
    """(truth, pred), float32 (batch,H,W,2): a smooth field plus N(0, 1) texture, up to about 64 px in image 0 and below
    40 px in image 1 (amplitude = the images' peak of u); the prediction is the truth plus N(0, sigmas[n]^2)."""
    rng = np.random.default_rng(seed)
    H, W = hw
    y, x = np.meshgrid(np.arange(H) / max(H, 2), np.arange(W) / max(W, 2), indexing="ij")
    truth = np.empty((batch, H, W, 2))
    for n in range(batch):
        a = amplitude[n % 2]
        truth[n, :, :, 0] = a * np.sin(2 * math.pi * ((1.0 + n) * y + (1.5 - 0.5 * n) * x) + n)
        truth[n, :, :, 1] = 0.7 * a * np.cos(2 * math.pi * ((0.5 + n) * y - x) + 0.3)
    truth += rng.standard_normal(truth.shape)
    pred = truth + rng.standard_normal(truth.shape) * np.asarray(sigmas).reshape(batch, 1, 1, 1)
    return truth.astype(np.float32), pred.astype(np.float32)


def chunk_flows(seed=3):
    """The CHUNKS case: two whole chunks and a last one of LAST pixels.  A 50 px error at pixel 0 and at the last pixel of
    both images; image 1 is slower than 40 px everywhere but in the last chunk."""
    truth, pred = make_flows(seed, CHUNKS)
    H, W = CHUNKS
    flat_t, flat_p = truth.reshape(B, H * W, 2), pred.reshape(B, H * W, 2)
    assert np.hypot(flat_t[1, :, 0], flat_t[1, :, 1]).max() < 39.0
    flat_p[1, -LAST:] += np.float32([50.0, 30.0]) - flat_t[1, -LAST:]       # the error stays, the speed becomes 58
    flat_t[1, -LAST:] = np.float32([50.0, 30.0])
    flat_p[:, 0, 0] += np.float32(50.0)
    flat_p[:, -1, 1] -= np.float32(50.0)
    return truth, pred


def masks(seed, hw, valid_share=(0.52, 0.93), occluded_share=0.3, batch=B, last=LAST):
    """(valid, occluded), bool (batch,H,W), independent random patterns: valid keeps valid_share[n % 2] of image n (pixel
    0 and the last `last` pixels -- by default the last chunk -- always); occluded marks occluded_share of every image
    but image 1, where it marks the last `last` pixels only."""
    rng = np.random.default_rng(seed)
    H, W = hw
    share = np.asarray([valid_share[n % len(valid_share)] for n in range(batch)])
    valid = rng.random((batch, H * W)) < share.reshape(batch, 1)
    valid[:, 0] = True
    valid[:, -last:] = True
    occluded = rng.random((batch, H * W)) < occluded_share
    occluded[1] = False
    occluded[1, -last:] = True
    return valid.reshape(batch, H, W), occluded.reshape(batch, H, W)


def tensor(a):
    """A torch tensor holding a copy of a (possibly read-only) numpy array."""
    return torch.from_numpy(np.array(a))


def _case(truth, pred, data_format="channels_last", half=False, valid=None, occluded=None):
    truth, pred = away_from_thresholds(truth, pred, np.float16 if half else np.float32)
    if data_format == "channels_first":
        truth, pred = (np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))) for a in (truth, pred))
    return dict(truth=truth, pred=pred, data_format=data_format, valid=valid, occluded=occluded)


UNKNOWN = ((0, 1, np.nan), (0, 7, np.inf), (1, 2 * CHUNK + 1, 1e10), (1, 5, -np.inf), (0, CHUNK, -1e10))  # image, pixel, value


def _build_cases():
    valid, occluded = masks(11, CHUNKS)
    cases = {"1x1": _case(*make_flows(0, SMALL)),
             "3x5": _case(*make_flows(1, WAVE)),
             "chunks": _case(*chunk_flows()),
             "chunks_channels_first": _case(*chunk_flows(), data_format="channels_first"),
             "chunks_f16_pred": _case(*chunk_flows(), half=True),
             "valid": _case(*chunk_flows(), valid=valid),
             "occluded": _case(*chunk_flows(), occluded=occluded),
             "both_masks": _case(*chunk_flows(), valid=valid, occluded=occluded)}
    t, p = chunk_flows()
    flat = t.reshape(B, -1, 2)
    for n, i, value in UNKNOWN:
        flat[n, i, i % 2] = value
    cases["unknown_gt"] = _case(t, p)
    none = valid.copy()
    none[0] = False
    cases["all_invalid"] = _case(*chunk_flows(), valid=none)
    t, _ = make_flows(5, NEAR)
    p = t + np.random.default_rng(6).standard_normal(t.shape).astype(np.float32) * np.float32(0.01)
    cases["near_equal"] = _case(t, p.astype(np.float32))
    for c in cases.values():
        for k in ("truth", "pred", "valid", "occluded"):
            if c[k] is not None:
                c[k].setflags(write=False)
    return cases


CASES = _build_cases()
_REF = {}


def channels_last(c):
    if c["data_format"] == "channels_first":
        return np.transpose(c["truth"], (0, 2, 3, 1)), np.transpose(c["pred"], (0, 2, 3, 1))
    return c["truth"], c["pred"]


def reference(name):
    """ref_flow_quality of a case, computed once and left unchanged."""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = ref_flow_quality(c["truth"], c["pred"], c["valid"], c["occluded"], data_format=c["data_format"])
        for a in _REF[name].values():
            a.setflags(write=False)
    return _REF[name]


def errors(got, want):
    """{field: the largest error over the batch}: in ulps of the rounded quotient for the count ratios, absolute for the
    rest; inf where one side is NaN and the other is not."""
    got = got._asdict() if hasattr(got, "_asdict") else got
    err = {}
    for k in FIELDS:
        g = got[k].detach().cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        g, w = np.asarray(g, np.float64).reshape(-1), np.asarray(want[k], np.float64).reshape(-1)
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            err[k] = float("inf")
            continue
        keep = ~np.isnan(w)
        d = np.abs(g[keep] - w[keep])
        if k in COUNT_FIELDS:
            d = d / np.spacing(np.maximum(np.abs(w[keep]), 1e-30).astype(np.float32)).astype(np.float64)
        err[k] = float(d.max()) if d.size else 0.0
    return err


def violations(got, want):
    err = errors(got, want)
    bound = lambda k: 1.0 if k in COUNT_FIELDS else BOUNDS["aae" if k == "aae" else "epe"]
    return sorted(k for k in FIELDS if not err[k] <= bound(k)), err


def check(label, got, want):
    bad, err = violations(got, want)
    print("flow quality {}: epe-type {:.2e} px  aae {:.2e} deg  count ratios {:.2f} ulp".format(
        label, max(err[k] for k in EPE_FIELDS), err["aae"], max(err[k] for k in COUNT_FIELDS)))
    assert not bad, (label, {k: err[k] for k in bad})
    return err


def run_case(name, device="cpu", fn=None, **kw):
    c = CASES[name]
    fn = metrics.flow_quality if fn is None else fn
    m = lambda a: None if a is None else tensor(a).to(device)
    res = fn(tensor(c["truth"]).to(device), tensor(c["pred"]).to(device), valid=m(c["valid"]), occluded=m(c["occluded"]),
             data_format=c["data_format"], **kw)
    return res, {k: v.cpu().numpy() for k, v in res._asdict().items()}


# ---- the cases are what they are chosen for -------------------------------------------------------------------------
def test_the_cases_have_their_properties():
    H, W = CHUNKS
    assert CHUNK <= 1 << 24 and W % 2 == 1 and H > 1 and W > 1
    assert -(-(H * W) // CHUNK) == 3 and 0 < LAST == H * W - 2 * CHUNK < 64         # the last chunk: partial, under a wave
    assert CASES["1x1"]["truth"].shape == (B, 1, 1, 2) and CASES["3x5"]["truth"].shape == (B, 3, 5, 2)
    assert CASES["chunks"]["truth"].shape == (B, H, W, 2) and CASES["chunks_channels_first"]["truth"].shape == (B, 2, H, W)
    assert CASES["chunks_f16_pred"]["pred"].dtype == np.float16 and CASES["chunks_f16_pred"]["truth"].dtype == np.float32
    for name, c in CASES.items():
        t, p = channels_last(c)
        assert not near_a_threshold(t, p, c["valid"]).any(), name                  # pixels left out: none
    t, p = channels_last(CASES["chunks"])
    e = np.hypot(*(t.astype(np.float64) - p).reshape(B, -1, 2).transpose(2, 0, 1))
    m = np.hypot(*t.astype(np.float64).reshape(B, -1, 2).transpose(2, 0, 1))
    assert (e[:, 0] > 40).all() and (e[:, -1] > 40).all() and np.median(e[0]) < 0.6 and np.median(e[1]) > 3
    assert (m[1, :-LAST] < 40).all() and (m[1, -LAST:] > 40).all() and m[0].max() > 50 and (m[0] < 10).any()
    valid, occluded = CASES["both_masks"]["valid"], CASES["both_masks"]["occluded"]
    for n in range(B):
        assert 0.05 <= 1.0 - valid[n].mean() <= 0.5, n                             # the share masked out
    assert 0.05 <= occluded[0].mean() <= 0.5
    assert occluded[1].reshape(-1)[-LAST:].all() and occluded[1].sum() == LAST     # image 1: the last chunk only
    assert abs(valid[0].mean() - valid[1].mean()) > 0.3
    assert not CASES["all_invalid"]["valid"][0].any() and CASES["all_invalid"]["valid"][1].mean() > 0.5
    flat = channels_last(CASES["unknown_gt"])[0].reshape(B, -1, 2)
    assert all(not abs(flat[n, i, i % 2]) <= 1e9 for n, i, _ in UNKNOWN)
    ref = np.rint(reference("unknown_gt")["valid"] * H * W)
    assert list(H * W - ref) == [sum(1 for n, _, _ in UNKNOWN if n == k) for k in range(B)]
    ref = reference("all_invalid")
    assert ref["valid"][0] == 0 and all(np.isnan(ref[k][0]) for k in FIELDS if k != "valid") and np.isfinite(ref["epe"][1])
    for name in CASES:                                   # the two images of a batch differ in error level
        if CASES[name]["truth"].size == B * 2 * CHUNKS[0] * CHUNKS[1] and name != "all_invalid":
            ref = reference(name)
            assert ref["epe"][1] > 3 * ref["epe"][0], name
    ne = reference("near_equal")
    assert ne["epe"].max() < 0.05 and ne["aae"].max() < 0.5


def test_the_comparison_sees_the_planted_defects():
    """A kernel that dropped the last pixel, counted pixel 0 twice, swapped the two images, ignored a mask or evaluated
    the angle by acosf of the normalised dot product would miss the bounds."""
    c = CASES["both_masks"]
    t, p = channels_last(c)
    H, W = CHUNKS
    want = reference("both_masks")
    sums = ref_sums(t, p, c["valid"], c["occluded"])
    assert violations(ref_scores(sums, H * W), want)[0] == []
    flat_t, flat_p = t.reshape(B, 1, -1, 2), p.reshape(B, 1, -1, 2)
    fv, fo = c["valid"].reshape(B, 1, -1), c["occluded"].reshape(B, 1, -1)
    last = ref_sums(flat_t[:, :, -1:], flat_p[:, :, -1:], fv[:, :, -1:], fo[:, :, -1:])
    first = ref_sums(flat_t[:, :, :1], flat_p[:, :, :1], fv[:, :, :1], fo[:, :, :1])
    assert (last[:, 0] == 1).all() and (first[:, 0] == 1).all()
    for label, broken in (("last pixel dropped", sums - last), ("pixel 0 twice", sums + first), ("swapped", sums[::-1])):
        bad, err = violations(ref_scores(broken, H * W), want)
        assert "epe" in bad and "valid" in bad or label == "swapped" and "epe" in bad, (label, err)
    for label, kw in (("valid ignored", dict(occluded=c["occluded"])), ("occluded ignored", dict(valid=c["valid"]))):
        bad, _ = violations(ref_flow_quality(t, p, **kw), want)
        assert ("valid" in bad) if label == "valid ignored" else ("epe_occ" in bad and "epe_noc" in bad), (label, bad)
    # acosf of the normalised dot product, in fp32, on nearly equal flows: up to 0.034 degrees off per pixel (its result
    # is 0 or at least acos(1 - 2^-24) = 0.02 degrees), which the mean over the 35 pixels of an image keeps 3.4 x over
    # the aae bound
    c = CASES["near_equal"]
    t, p = (a.astype(np.float32) for a in channels_last(c))
    one = np.float32(1.0)
    dot = t[..., 0] * p[..., 0] + t[..., 1] * p[..., 1] + one
    nt = np.sqrt(t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1] + one)
    npd = np.sqrt(p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1] + one)
    acos = np.degrees(np.arccos(np.clip(dot / (nt * npd), -one, one)).astype(np.float32)).astype(np.float64)
    got = dict(reference("near_equal"), aae=acos.mean(axis=(1, 2)))
    bad, err = violations(got, reference("near_equal"))
    assert bad == ["aae"] and err["aae"] > 3 * BOUNDS["aae"], err["aae"]


# ---- the closed form ------------------------------------------------------------------------------------------------
def closed_form(device="cpu"):
    """truth (3, 4) everywhere, prediction 0: e = m = 5 exactly.  Every strict comparison of the contract sits on its
    threshold once: e < 5 is false (acc5 = 0), e > 5 is false (fl = 0 with outlier = (5, 0.05)), m < 5 is false (bin 0
    empty with speed = (5, 40))."""
    t = torch.tensor([3.0, 4.0]).expand(B, 6, 11, 2).contiguous().to(device)
    p = torch.zeros_like(t)
    ang = math.degrees(math.atan2(5.0, 1.0))
    res = metrics.flow_quality(t, p, data_format="channels_last")
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in res._asdict().items()}
    for k, want in (("epe", 5.0), ("fl", 1.0), ("acc1", 0.0), ("acc3", 0.0), ("acc5", 0.0), ("epe_noc", 5.0),
                    ("epe_s0_10", 5.0), ("valid", 1.0)):
        assert (got[k] == want).all(), (k, got[k])
    assert np.abs(got["aae"] - ang).max() <= BOUNDS["aae"]
    assert all(np.isnan(got[k]).all() for k in ("epe_occ", "epe_s10_40", "epe_s40"))
    edge = metrics.flow_quality(t, p, outlier=(5.0, 0.05), accuracy=(1.0, 5.0, 5.5), speed=(5.0, 40.0),
                                data_format="channels_last")
    assert bool((edge.fl == 0).all()) and bool((edge.acc3 == 0).all()) and bool((edge.acc5 == 1).all())
    assert bool(torch.isnan(edge.epe_s0_10).all()) and bool((edge.epe_s10_40 == 5).all())
    rel = metrics.flow_quality(t, p, outlier=(3.0, 1.0), data_format="channels_last")           # e > 1.0 * m is false
    assert bool((rel.fl == 0).all())
    return float(np.abs(got["aae"] - ang).max())


def test_closed_form():
    closed_form()


# ---- the torch path on every case of the GPU suite ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_torch_path_against_the_restatement(name):
    """Measured (CPU): over the eleven cases at most 1.8e-6 px in the EPE-type means (unknown_gt; 2.0e-7 on chunks),
    5.8e-7 degrees in aae (3x5), and every count ratio the rounded float64 quotient (at most 0.5 ulp)."""
    res, got = run_case(name)
    assert isinstance(res, metrics.FlowScores) and res._fields == FIELDS
    assert all(v.dtype == torch.float32 and tuple(v.shape) == (B,) for v in res)
    check("torch " + name, got, reference(name))
    direct, _ = run_case(name, fn=metrics.flow_quality_torch)
    assert all(torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0)) for a, b in zip(res, direct))


def test_masks_of_every_dtype_and_rank_three():
    c = CASES["both_masks"]
    t, p, v, o = (tensor(c[k]) for k in ("truth", "pred", "valid", "occluded"))
    want, _ = run_case("both_masks")
    same = lambda a, b: all(torch.equal(x.nan_to_num(), y.nan_to_num()) for x, y in zip(a, b))
    for conv in (lambda m: m.to(torch.uint8) * 7, lambda m: m.float() * 0.25, lambda m: m.double(), lambda m: m.half()):
        assert same(metrics.flow_quality(t, p, valid=conv(v), occluded=conv(o), data_format="channels_last"), want)
    one = metrics.flow_quality(t[1], p[1], valid=v[1], occluded=o[1], data_format="channels_last")
    assert all(x.dim() == 0 for x in one) and same([x[None] for x in one], [y[1:] for y in want])
    from qpwcnet_amd import backend
    assert backend.image_data_format() == "channels_last"
    assert same(metrics.flow_quality(t, p, valid=v, occluded=o), want)


def test_refusals():
    ok = torch.zeros(1, 4, 5, 2)
    with pytest.raises(ValueError, match="one shape"):
        metrics.flow_quality(ok, torch.zeros(1, 4, 6, 2))
    with pytest.raises(ValueError, match="2 channels"):
        metrics.flow_quality(torch.zeros(1, 4, 5, 3), torch.zeros(1, 4, 5, 3))
    with pytest.raises(ValueError, match="2 channels"):
        metrics.flow_quality(ok, ok, data_format="channels_first")
    with pytest.raises(ValueError, match="float32"):
        metrics.flow_quality(ok.half(), ok.half())
    with pytest.raises(ValueError, match="dtype"):
        metrics.flow_quality(ok, ok.double())
    with pytest.raises(ValueError, match="Unsupported data format"):
        metrics.flow_quality(ok, ok, data_format="nhwc")
    with pytest.raises(ValueError, match="rank"):
        metrics.flow_quality(ok[0, 0], ok[0, 0])
    with pytest.raises(ValueError, match="valid must have shape"):
        metrics.flow_quality(ok, ok, valid=torch.ones(1, 5, 4))
    with pytest.raises(ValueError, match="occluded must have shape"):
        metrics.flow_quality(ok, ok, occluded=torch.ones(1, 4, 5, 1))
    with pytest.raises(TypeError, match="bool, uint8 or floating"):
        metrics.flow_quality(ok, ok, valid=torch.ones(1, 4, 5, dtype=torch.int32))
    with pytest.raises(TypeError, match="torch.Tensor"):
        metrics.flow_quality(ok, ok, valid=np.ones((1, 4, 5)))
    with pytest.raises(TypeError, match="torch.Tensor"):
        metrics.flow_quality(ok.numpy(), ok)
    with pytest.raises(ValueError, match="'estimate'"):
        metrics.flow_quality(ok, ok, occluded="guess")
    for kw in (dict(outlier=(0.0, 0.05)), dict(outlier=(3.0, -0.1)), dict(outlier=(3.0,)), dict(accuracy=(1.0, 1.0, 5.0)),
               dict(accuracy=(3.0, 1.0, 5.0)), dict(accuracy=(0.0, 1.0, 5.0)), dict(accuracy=(1.0, 3.0)),
               dict(speed=(40.0, 10.0)), dict(speed=(0.0, 10.0)), dict(speed=(10.0, float("inf"))),
               dict(outlier=(float("nan"), 0.05))):
        with pytest.raises(ValueError, match="outlier|accuracy|speed"):
            metrics.flow_quality(ok, ok, **kw)
    with pytest.raises(ValueError, match="state"):
        metrics.flow_quality(ok, ok, state=torch.zeros(17))
    with pytest.raises(ValueError, match="state"):
        metrics.flow_quality(ok, ok, state=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="state"):
        metrics.flow_quality(ok, ok, state=torch.zeros(17, dtype=torch.float64, device="meta"))
    with pytest.raises(ValueError, match="one device"):
        metrics.flow_quality(ok, ok.to("meta"))
    with pytest.raises(ValueError, match="occluded"):
        metrics.FlowQuality(occluded="guess")


def test_no_gradient_flows():
    c = CASES["3x5"]
    t, p = tensor(c["truth"]), tensor(c["pred"]).requires_grad_(True)
    assert not any(v.requires_grad for v in metrics.flow_quality(t, p * 1.0, data_format="channels_last"))


def test_occluded_estimate_is_the_map_passed_explicitly(monkeypatch):
    """occluded="estimate" scores with occlusion.estimate_occlusion_map(y_true, data_format), a float map, exactly as if
    it had been passed (the estimate itself is a HIP kernel: tests/test_gpu_flow_quality.py runs it)."""
    from qpwcnet_amd import occlusion
    c = CASES["occluded"]
    t, p = tensor(c["truth"]), tensor(c["pred"])
    the_map = tensor(c["occluded"]).float()
    seen = []

    def fake(flow, data_format=None):
        seen.append((flow, data_format))
        return the_map
    monkeypatch.setattr(occlusion, "estimate_occlusion_map", fake)
    got = metrics.flow_quality(t, p, occluded="estimate", data_format="channels_last")
    want = metrics.flow_quality(t, p, occluded=the_map, data_format="channels_last")
    assert len(seen) == 1 and torch.equal(seen[0][0], t) and seen[0][1] == "channels_last"
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and float(got.epe_occ[0]) > 0
    m = metrics.FlowQuality(occluded="estimate", data_format="channels_last")
    per = m.update_state(t, p)
    assert len(seen) == 2 and all(torch.equal(a, b) for a, b in zip(per, want))


# ---- the running state ----------------------------------------------------------------------------------------------
def state_scenario(device="cpu"):
    """Two batches with different valid shares through one FlowQuality -> (the metric, per-batch FlowScores, the float64
    reference sums [2 B, 15] in image order, pixels per image)."""
    m = metrics.FlowQuality(data_format="channels_last")
    zero = m.result()
    assert sorted(zero) == sorted(FIELDS + ("images", "pixels")) and set(zero.values()) == {0.0}
    per, sums = [], []
    for name in ("chunks", "both_masks"):
        c = CASES[name]
        f = lambda a: None if a is None else tensor(a).to(device)
        per.append(m.update_state(f(c["truth"]), f(c["pred"]), valid=f(c["valid"]), occluded=f(c["occluded"])))
        sums.append(ref_sums(c["truth"], c["pred"], c["valid"], c["occluded"]))
    return m, per, np.concatenate(sums), CHUNKS[0] * CHUNKS[1]


def check_state(m, per, sums, pixels, images=2 * B):
    """The 17 running sums of m against the float64 sums [images, 15] of every image it has seen, in image order."""
    state = m.state.cpu().numpy()
    assert m.state.dtype == torch.float64 and state.shape == (17,)
    assert len(sums) == images and state[15] == images and state[16] == images * pixels
    total = sums.sum(axis=0)
    for i in range(15):
        if i in (1, 8, 10, 12, 14):                       # sums of e: the bound of a mean times its count
            assert abs(state[i] - total[i]) <= BOUNDS["epe"] * max(total[i - 1 if i > 1 else 0], 1), i
        elif i == 2:
            assert abs(state[i] - total[i]) <= BOUNDS["aae"] * total[0]
        else:
            assert state[i] == total[i], i                # counts
    res = m.result()
    want = ref_scores(total, images * pixels)
    assert res["images"] == images and res["pixels"] == images * pixels
    bad, err = violations({k: np.float32(res[k]) for k in FIELDS}, want)
    assert not bad, err
    # pixel-weighted, not the mean of the per-image means: the batches differ in valid share and error level
    means = np.mean([float(v) for b in per for v in b.epe.cpu()])
    assert abs(means - want["epe"]) > 100 * BOUNDS["epe"] and abs(res["epe"] - means) > 100 * BOUNDS["epe"]
    valid_means = np.mean([float(v) for b in per for v in b.valid.cpu()])
    assert abs(res["valid"] - valid_means) < 1e-6         # equal pixel counts per image: here the two agree
    m.reset_state()
    assert set(m.result().values()) == {0.0} and float(m.state.abs().sum()) == 0.0


def test_state_and_pixel_weighted_result():
    m, per, sums, pixels = state_scenario()
    for got, name in zip(per, ("chunks", "both_masks")):
        assert violations(got, reference(name))[0] == []
    # in image order, in float64: the state is the running sum of the per-image sums the torch path formed
    c = CASES["chunks"]
    first = metrics._flow_sums_torch(tensor(c["truth"]), tensor(c["pred"]), None, None,
                                     *metrics._flow_f32(OUTLIER, ACCURACY, SPEED), 3)
    c = CASES["both_masks"]
    second = metrics._flow_sums_torch(tensor(c["truth"]), tensor(c["pred"]), tensor(c["valid"]), tensor(c["occluded"]),
                                      *metrics._flow_f32(OUTLIER, ACCURACY, SPEED), 3)
    run = torch.zeros(15, dtype=torch.float64)
    for row in torch.cat([first, second]):
        run = run + row
    assert torch.equal(m.state[:15], run)
    check_state(m, per, sums, pixels)


# ---- two gloo ranks -------------------------------------------------------------------------------------------------
def rank_batches():
    """Four batches of 23 x 31 flows with their valid masks, from seeds."""
    out = []
    for k in range(4):
        t, p = make_flows(20 + k, (23, 31), sigmas=(0.3 + k, 4.0 + k))
        valid = np.random.default_rng(30 + k).random((B, 23, 31)) < (0.4 + 0.15 * k)
        out.append((tensor(t), tensor(p), tensor(valid)))
    return out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from qpwcnet_amd import dist as qd
    qd.init("gloo")
    m = metrics.FlowQuality(data_format="channels_last")
    for t, p, valid in rank_batches()[2 * rank:2 * rank + 2]:
        m.update_state(t, p, valid=valid)
    local = m.result()
    q.put((rank, local, m.result(all_reduce=True), m.state.clone().numpy()))
    qd.barrier()
    dist.destroy_process_group()


def test_all_reduce_over_two_gloo_ranks():
    """Each rank scores half of a four-batch set; result(all_reduce=True) on either rank is the single-process result of
    the whole set to 1e-12 relative, its own state is left as it was, and without all_reduce a rank sees its half."""
    import torch.multiprocessing as mp
    single = metrics.FlowQuality(data_format="channels_last")
    for t, p, valid in rank_batches():
        single.update_state(t, p, valid=valid)
    want = single.result()
    assert want["images"] == 4 * B and all(math.isfinite(want[k]) for k in FIELDS if k != "epe_occ")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in procs), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, local, reduced, state in res:
        assert local["images"] == 2 * B and abs(local["epe"] - want["epe"]) > 1e-3
        assert state[15] == 2 * B                                                  # the rank's own sums are untouched
        for k in FIELDS + ("images", "pixels"):
            a, b = reduced[k], want[k]
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b), (rank, k, a, b)


# ---- header and table -----------------------------------------------------------------------------------------------
NAMES = ["qpwc_flow_quality_workspace_floats", "qpwc_flow_quality_fwd", "qpwc_flow_quality_fwd_kernel"]


def test_flow_quality_prototypes_match_their_header():
    protos = parse_header(HEADER)
    assert [name for name, _, _ in protos] == NAMES
    assert mismatches(_hip.FLOW_QUALITY_PROTOTYPES, protos) == []
    others = (set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES) | set(_hip.TRIPLET_PROTOTYPES) | set(_hip.VIS_PROTOTYPES)
              | set(_hip.QUALITY_PROTOTYPES) | set(_hip.REVIEW_PROTOTYPES))
    assert len(_hip.SYMBOLS) == 77 and not set(_hip.FLOW_QUALITY_PROTOTYPES) & others
    table = dict(_hip.FLOW_QUALITY_PROTOTYPES)
    restype, argtypes = table["qpwc_flow_quality_fwd"]
    assert len(argtypes) == 20
    table["qpwc_flow_quality_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_flow_quality_fwd: 20 parameters, table has 19"]
    assert metrics.FlowScores._fields == FIELDS
    with open(os.path.join(os.path.dirname(HEADER), "..", "qpwcnet_amd", "csrc", "flow_quality.hip")) as f:
        assert "kFlowQualChunk = {};".format(CHUNK) in f.read()


def test_the_library_exports_the_table(hip_lib):
    for name, (restype, argtypes) in _hip.FLOW_QUALITY_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


# ---- the queries (host only) ----------------------------------------------------------------------------------------
def test_workspace_query(hip_lib):
    """15 floats per image and chunk of FLOW_QUALITY_CHUNK pixels: it grows by one chunk's floats exactly when H * W
    passes a multiple of the chunk, and scales with B."""
    q = hip_lib.qpwc_flow_quality_workspace_floats
    assert q(1, 1, 1) == 15 and q(1, 1, CHUNK) == 15 and q(1, 1, CHUNK + 1) == 30 and q(1, 2, CHUNK) == 30
    assert q(B, CHUNKS[0], CHUNKS[1]) == B * 3 * 15 and q(7, 1, CHUNK + 1) == 7 * 30
    assert q(16, 1024, 2048) == 16 * (1024 * 2048 // CHUNK) * 15
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, 4)):
        assert q(*bad) == _hip.E_SHAPE, bad
    assert q(1, 1, LIMIT) == -(-LIMIT // CHUNK) * 15 and q(LIMIT, 1, 1) == LIMIT * 15
    assert q(2, 1, 1 << 30) == _hip.E_SHAPE and q(1 << 16, 1 << 15, 1) == _hip.E_SHAPE


def test_kernel_query_is_host_only(hip_lib):
    from qpwcnet_amd import ops
    q = lambda *a: hip_lib.qpwc_flow_quality_fwd_kernel(*a).decode()
    assert q(8, 256, 512) == "flow_quality_tile_kernel" and q(1, 1, 1) == "flow_quality_tile_kernel"
    assert q(1, 1, LIMIT) == "flow_quality_tile_kernel"
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (2, 1 << 15, 1 << 15)):
        assert q(*bad) == "", bad
    assert ops.flow_quality_kernel(B, 43, 77) == "flow_quality_tile_kernel" and ops.flow_quality_kernel(B, 0, 64) == ""

"""The valid-masked flow losses (qpwcnet_amd.loss.multiscale_masked / masked_ground_truth, qpwc_masked_loss_fwd / _bwd)
without a GPU:
  * ``ref_levels`` / ``ref_loss``: a float64 numpy restatement of include/qpwc_masked_loss.h written with loops -- the
    validity rule, the mean over a block's valid pixels, the bilinear corners renormalised over the valid ones, the three
    per-pixel terms with their analytic derivatives, the division by the count.  Only the bilinear weights along each
    axis are float32, as the header says (a corner's weight is their product, in float64 here);
  * ``loss.multiscale_masked_torch`` / ``masked_ground_truth_torch`` on float64 inputs against it, on every case that
    tests/test_gpu_masked_loss.py runs the kernels on (it imports CASES and make_case);
  * the public surface and its refusals, the ctypes table against its header, the two queries, and the relation between
    the shapes of the GPU suite's grid-loop cases and the kernels' grid caps.
Bounds: 1e-12 relative for losses, ground truths (of the level's largest value) and autograd gradients (of the level's
largest gradient); masks and counts exact."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

import qpwcnet_amd as K  # noqa: E402
from qpwcnet_amd import _hip, loss, metrics  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qpwc_masked_loss.h")
KINDS = ("v2", "mse", "finetune")
LAYOUTS = ("channels_last", "channels_first")
CODES = {"v2": _hip.LOSS_FLOW_MSE_V2, "mse": _hip.LOSS_FLOW_MSE, "finetune": _hip.LOSS_FLOW_FINETUNE}
DELTA, Q, EPS = 0.1, 0.4, 0.01
TOL = 1e-12

PYRAMID = (2, 32, 64, [(16, 32), (8, 16), (4, 8)])       # area factors 2 / 4 / 8: the tile kernel for the area kind
THREE = (2, 36, 60, [(12, 20)])                          # a 3 x 3 area factor: the pixel kernel
NONINT = (2, 30, 44, [(7, 9)])                           # bilinear only: 30 / 7 and 44 / 9
NARROW = (2, 32, 48, [(16, 24), (8, 12)])                # W % 32 != 0: the pixel kernel for nested powers of two
# name -> (shape, kinds, how the invalid pixels come about)
CASES = {
    "pyramid_mask30": (PYRAMID, KINDS, "mask30"),
    "three_mask30": (THREE, KINDS, "mask30"),
    "nonint_mask30": (NONINT, ("mse", "finetune"), "mask30"),
    "narrow_mask30": (NARROW, KINDS, "mask30"),
    "empty_blocks": (PYRAMID, KINDS, "empty_blocks"),
    "one_per_block": (PYRAMID, KINDS, "one_per_block"),
    "nan_only": (PYRAMID, KINDS, "nan"),
    "inf_only": (PYRAMID, KINDS, "inf"),
    "unknown_only": (PYRAMID, KINDS, "1e10"),
    "one_component": (PYRAMID, KINDS, "component"),
    "garbage_under_mask": (PYRAMID, KINDS, "garbage"),
    "all_valid": (PYRAMID, KINDS, "all"),
    "three_all_valid": (THREE, KINDS, "all"),
    "nonint_all_valid": (NONINT, ("mse", "finetune"), "all"),
    "none_valid": (PYRAMID, KINDS, "none"),
}
RANDOM = ("mask30", "nan", "inf", "1e10", "component", "garbage")     # every level has valid and invalid level pixels


def make_loss(kind, data_format):
    prev = K.image_data_format()
    K.set_image_data_format(data_format)
    try:
        return {"v2": loss.FlowMseLossV2, "mse": lambda: loss.FlowMseLoss(data_format),
                "finetune": lambda: loss.FlowMseLossFineTune(data_format, Q, EPS)}[kind]()
    finally:
        K.set_image_data_format(prev)


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_valid(gt, valid):
    """(B,H,W) bool: both components finite and at most 1e9 in magnitude, and the mask allows it."""
    assert metrics.FLOW_UNKNOWN == 1e9
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(gt).all(-1) & (np.abs(gt) <= 1e9).all(-1)
    return ok if valid is None else ok & (np.asarray(valid) != 0)


def _axis(n_out, n_in):
    """(i0, i1, l0, l1) per output position: float32 arithmetic, every operation rounded on its own."""
    scale = np.float32(n_in) / np.float32(n_out)
    out = []
    for o in range(n_out):
        f = max(scale * (np.float32(o) + np.float32(0.5)) - np.float32(0.5), np.float32(0.0))
        i0 = int(f)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = np.float32(f - np.float32(i0))
        out.append((i0, i1, np.float32(1.0) - l1, l1))
    return out


def ref_levels(kind, gt, valid, shapes):
    """[(ground truth (B,h,w,2) float64 with 0 where there is none, validity (B,h,w) bool)] of channels-last numpy
    ground truth (B,H,W,2), by loops over the level pixels."""
    gt = np.asarray(gt, dtype=np.float64)
    ok = ref_valid(gt, valid)
    B, H, W, _ = gt.shape
    out = []
    for h, w in shapes:
        g, m = np.zeros((B, h, w, 2)), np.zeros((B, h, w), dtype=bool)
        if kind == "v2":
            assert H % h == 0 and W % w == 0
            sh, sw = H // h, W // w
            for b in range(B):
                for y in range(h):
                    for x in range(w):
                        blk = ok[b, y * sh:(y + 1) * sh, x * sw:(x + 1) * sw]
                        n = int(blk.sum())
                        if n >= 1:
                            vals = gt[b, y * sh:(y + 1) * sh, x * sw:(x + 1) * sw][blk]      # the valid pixels only
                            g[b, y, x] = vals.sum(axis=0) / n * (h / H)
                            m[b, y, x] = True
        else:
            ay, ax = _axis(h, H), _axis(w, W)
            for b in range(B):
                for y in range(h):
                    y0, y1, ly0, ly1 = ay[y]
                    for x in range(w):
                        x0, x1, lx0, lx1 = ax[x]
                        S, acc = 0.0, np.zeros(2)
                        for yy, ly in ((y0, ly0), (y1, ly1)):
                            for xx, lx in ((x0, lx0), (x1, lx1)):
                                if ok[b, yy, xx]:                                           # never used otherwise
                                    wk = float(ly) * float(lx)
                                    S += wk
                                    acc += wk * gt[b, yy, xx]
                        if S > 0:
                            g[b, y, x] = acc / S * (h / H)
                            m[b, y, x] = True
        out.append((g, m))
    return out


def ref_loss(kind, g, m, pred):
    """(loss, count, d loss / d pred) of one level, float64 numpy, channels-last."""
    h, w = m.shape[1:]
    count = int(m.sum())
    den = max(count, 1)
    p = np.where(m[..., None], np.asarray(pred, dtype=np.float64), 0.0)
    grad = np.zeros_like(p)
    if kind == "v2":
        s = 2.0 / (w + h)
        e = s * p - s * g
        a = np.abs(e)
        term = np.where(a <= DELTA, 0.5 * e * e, DELTA * a - 0.5 * DELTA * DELTA).sum(-1)
        grad = s * np.where(a <= DELTA, e, DELTA * np.sign(e)) / (2 * den)
        total = term[m].sum() / (2 * den)
    elif kind == "mse":
        r = g - p
        n = np.sqrt((r * r).sum(-1))
        with np.errstate(invalid="ignore", divide="ignore"):
            grad = np.where(n[..., None] > 0, -r / n[..., None], 0.0) / den
        total = n[m].sum() / den
    else:
        r = g - p
        base = np.abs(r).sum(-1) + EPS
        grad = -(Q * base ** (Q - 1.0))[..., None] * np.sign(r) / den
        total = (base ** Q)[m].sum() / den
    return float(total), count, np.where(m[..., None], grad, 0.0)


def ref_dense_level(kind, gt, h, w):
    """The dense loss's ground truth of an all-valid flow: the plain block mean / the plain four-corner interpolation with
    the same float32 weights, no mask and no renormalisation."""
    gt = np.asarray(gt, dtype=np.float64)
    B, H, W, _ = gt.shape
    if kind == "v2":
        return gt.reshape(B, h, H // h, w, W // w, 2).mean(axis=(2, 4)) * (h / H)
    ay, ax = _axis(h, H), _axis(w, W)
    g = np.zeros((B, h, w, 2))
    for y, (y0, y1, ly0, ly1) in enumerate(ay):
        for x, (x0, x1, lx0, lx1) in enumerate(ax):
            top = float(lx0) * gt[:, y0, x0] + float(lx1) * gt[:, y0, x1]
            bot = float(lx0) * gt[:, y1, x0] + float(lx1) * gt[:, y1, x1]
            g[:, y, x] = float(ly0) * top + float(ly1) * bot
    return g * (h / H)


# ---- the cases ------------------------------------------------------------------------------------------------------
def make_case(name, kind, seed=0):
    """-> dict(gt, valid, shapes, preds, clean): channels-last numpy arrays whose values are float32 (and, the
    predictions, float16) numbers, so that every precision is fed the same values.  gt: (B,H,W,2) with whatever the case
    puts at its invalid pixels; valid: (B,H,W) bool or None; preds: one per level, 0.25..0.75 or 2..6 away from the
    level's ground truth in every channel, random signs (away from a zero residual, where the norms have a kink);
    clean: gt with 0 at every invalid pixel."""
    (B, H, W, shapes), kinds, how = CASES[name]
    assert kind in kinds
    rng = np.random.default_rng(1000 * sorted(CASES).index(name) + KINDS.index(kind) + 7919 * seed)
    gt = (rng.standard_normal((B, H, W, 2)) * 4.0).astype(np.float32)
    # about 30 % of the pixels stay: half of the pixels of 60 % of the coarsest level's blocks -- independent pixels at
    # that density would leave no 8 x 8 block empty (0.7^64), and every level is to have invalid level pixels
    ch, cw = -(-H // shapes[-1][0]), -(-W // shapes[-1][1])
    blocks = rng.random((B, -(-H // ch), -(-W // cw))) < 0.6
    keep = np.repeat(np.repeat(blocks, ch, axis=1), cw, axis=2)[:, :H, :W] & (rng.random((B, H, W)) < 0.5)
    drop = ~keep
    valid = None
    if how == "mask30":
        valid = ~drop
    elif how == "empty_blocks":
        valid = rng.random((B, H, W)) < 0.5
        valid[0, :H // 2, :W // 2] = False                             # whole blocks of every level
        valid[1, H // 4:H // 2, W // 2:] = False
    elif how == "one_per_block":
        sh, sw = H // shapes[-1][0], W // shapes[-1][1]
        valid = np.zeros((B, H, W), dtype=bool)
        for b in range(B):
            for y in range(shapes[-1][0]):
                for x in range(shapes[-1][1]):
                    valid[b, y * sh + rng.integers(sh), x * sw + rng.integers(sw)] = True
    elif how in ("nan", "inf", "1e10"):
        gt[drop] = {"nan": np.nan, "inf": np.inf, "1e10": 1e10}[how]
    elif how == "component":
        c = rng.integers(2, size=(B, H, W))
        gt[..., 0][drop & (c == 0)] = np.nan                           # the other component stays an ordinary number
        gt[..., 1][drop & (c == 1)] = -np.inf
    elif how == "garbage":
        valid = ~drop
        junk = np.array([np.nan, np.inf, -np.inf, 1e30, -1e10, 3e38], dtype=np.float32)
        gt[drop] = junk[rng.integers(len(junk), size=(int(drop.sum()), 2))]
    elif how == "none":
        valid = np.zeros((B, H, W), dtype=bool)
    else:
        assert how == "all"
    clean = np.where(ref_valid(gt, valid)[..., None], gt, np.float32(0.0))
    preds = []
    for (h, w), (g, m) in zip(shapes, ref_levels(kind, gt, valid, shapes)):
        mag = (0.25 + 0.5 * rng.random((B, h, w, 2))) * np.where(rng.random((B, h, w, 2)) < 0.5, 1.0, 8.0)
        sign = np.where(rng.random((B, h, w, 2)) < 0.5, -1.0, 1.0)
        preds.append((g + sign * mag).astype(np.float16).astype(np.float32))
    return dict(gt=gt, valid=valid, shapes=shapes, preds=preds, clean=clean, how=how)


def to_layout(a, data_format, dtype=torch.float64):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return t.permute(0, 3, 1, 2).contiguous() if data_format == "channels_first" else t


def from_layout(t, data_format):
    return (t.permute(0, 2, 3, 1) if data_format == "channels_first" else t).detach().cpu().double().numpy()


PARAMS = [(name, kind) for name in CASES for kind in CASES[name][1]]


def test_the_cases_have_their_properties():
    for name, kind in PARAMS:
        case = make_case(name, kind)
        levels = ref_levels(kind, case["gt"], case["valid"], case["shapes"])
        ok = ref_valid(case["gt"], case["valid"])
        if case["how"] in RANDOM:
            assert 0.2 < ok.mean() < 0.4, (name, ok.mean())
            for g, m in levels:
                assert m.any() and not m.all(), (name, kind, m.shape)
        if case["how"] in ("nan", "inf", "1e10", "component"):
            assert case["valid"] is None and not ok.all()
        if case["how"] == "component":
            bad = ~np.isfinite(case["gt"])
            assert (bad.sum(-1) == 1)[~ok].all()                       # one component only
        if case["how"] == "1e10":
            assert np.isfinite(case["gt"]).all()
        if case["how"] == "empty_blocks":
            assert all(not m.all() and m.any() for g, m in levels)
            assert not levels[-1][1][0, :2, :4].any()
        if case["how"] == "one_per_block":
            assert int(ok.sum()) == levels[-1][1].size and not levels[0][1].all()
            # the area kind finds it in every block; the four bilinear corners of a block's centre mostly miss it
            assert levels[-1][1].all() if kind == "v2" else not levels[-1][1].all()
        if case["how"] == "all":
            assert ok.all() and all(m.all() for g, m in levels)
        if case["how"] == "none":
            assert not ok.any() and not any(m.any() for g, m in levels)
        if case["how"] == "garbage":
            assert not np.isfinite(case["gt"][~ok]).all() and np.isfinite(case["gt"][ok]).all()


def test_bilinear_sample_points_of_the_cases_are_unambiguous():
    """m_p = (S > 0) jumps where a corner's weight passes 0, i.e. where a sample point meets a pixel centre.  The sample
    point of output o is (n_in (2 o + 1) - n_out) / (2 n_out): where that is a whole number (the 3 x 3 case) the float32
    arithmetic gives it exactly, so every precision sees the same zero weight; everywhere else it is at least
    1 / (2 n_out) from a centre, far more than a float32 rounding.  The masks can therefore be compared exactly."""
    from fractions import Fraction
    for (B, H, W, shapes), _, _ in CASES.values():
        for h, w in shapes:
            for n_out, n_in in ((h, H), (w, W)):
                for o, (i0, i1, l0, l1) in enumerate(_axis(n_out, n_in)):
                    exact = max(Fraction(n_in * (2 * o + 1) - n_out, 2 * n_out), Fraction(0))
                    got = Fraction(i0) + Fraction(float(l1))
                    if exact.denominator == 1:
                        assert got == exact and float(l1) == 0.0 and float(l0) == 1.0
                    else:
                        assert abs(got - exact) < Fraction(1, 1000 * n_out) and 0.0 < float(l1) < 1.0
                    assert 0 <= i0 <= i1 <= n_in - 1


# ---- the torch chain against the restatement --------------------------------------------------------------------------
def check_against_ref(case, kind, data_format, per, counts, grads, gts, masks, tol_loss, tol_gt, grad_bound):
    """per / counts: [L]; grads, gts: channels-last float64 numpy per level; masks: (B,h,w) numpy per level."""
    levels = ref_levels(kind, case["gt"], case["valid"], case["shapes"])
    for l, ((g, m), pred) in enumerate(zip(levels, case["preds"])):
        want, count, dgrad = ref_loss(kind, g, m, pred)
        assert int(counts[l]) == count, (l, int(counts[l]), count)
        assert abs(float(per[l]) - want) <= tol_loss * abs(want), (l, float(per[l]), want)
        if masks is not None:
            assert masks[l].dtype == np.uint8 and np.array_equal(masks[l] != 0, m), l
        if gts is not None:
            assert np.abs(gts[l] - g).max() <= tol_gt * max(np.abs(g).max(), 1e-30), (l, np.abs(gts[l] - g).max())
            assert not gts[l][~m].any()
        if grads is not None:
            assert not grads[l][~m].any(), l                             # exactly 0 at invalid level pixels
            grad_bound(l, grads[l], dgrad)


@pytest.mark.parametrize("data_format", LAYOUTS)
@pytest.mark.parametrize("name,kind", PARAMS)
def test_torch_chain_against_the_restatement(name, kind, data_format):
    case = make_case(name, kind)
    obj = make_loss(kind, data_format)
    gt = to_layout(case["gt"], data_format)
    valid = None if case["valid"] is None else torch.from_numpy(case["valid"])
    xs = [to_layout(p, data_format).requires_grad_() for p in case["preds"]]
    total, per, counts = loss.multiscale_masked(obj, gt, xs, valid)        # CPU tensors: the torch chain
    assert per.dtype == torch.float64 and counts.dtype == torch.int64 and total.dim() == 0
    assert abs(float(total.detach()) - float(per.detach().sum())) <= 1e-15 * max(abs(float(total.detach())), 1.0)
    total.backward()
    gts, masks = loss.masked_ground_truth(obj, gt, case["shapes"], valid)
    assert all(g.dtype == torch.float64 and g.shape == x.shape for g, x in zip(gts, xs))

    def grad_bound(l, got, want):
        assert np.abs(got - want).max() <= TOL * max(np.abs(want).max(), 1e-30), (l, np.abs(got - want).max())

    check_against_ref(case, kind, data_format, per.detach(), counts, [from_layout(x.grad, data_format) for x in xs],
                      [from_layout(g, data_format) for g in gts], [m.numpy() for m in masks], TOL, TOL, grad_bound)
    if case["how"] == "none":
        assert not per.detach().any() and not counts.any() and all(not x.grad.any() for x in xs)
    if case["how"] == "all":
        for (h, w), g in zip(case["shapes"], gts):
            dense = ref_dense_level(kind, case["gt"], h, w)
            assert np.abs(from_layout(g, data_format) - dense).max() <= TOL * np.abs(dense).max()
    if case["how"] == "garbage":
        # what lies under the zero mask changes no bit of the result
        again = loss.multiscale_masked_torch(obj, to_layout(case["clean"], data_format), [x.detach() for x in xs], valid)
        assert torch.equal(again[1], per.detach()) and torch.equal(again[2], counts)


@pytest.mark.parametrize("kind", KINDS)
def test_all_valid_is_the_dense_loss(kind):
    """With every pixel valid the masked loss and its gradient are the dense restatement's (tests/test_loss_cpu.py's
    term, on the dense ground truth with the same float32 corner weights)."""
    name = "all_valid"
    case = make_case(name, kind)
    obj = make_loss(kind, "channels_last")
    xs = [torch.from_numpy(p).double().requires_grad_() for p in case["preds"]]
    _, per, counts = loss.multiscale_masked_torch(obj, torch.from_numpy(case["gt"]).double(), xs)
    per.sum().backward()
    for l, ((h, w), x) in enumerate(zip(case["shapes"], xs)):
        g = torch.from_numpy(ref_dense_level(kind, case["gt"], h, w))
        p = x.detach().clone().requires_grad_()
        if kind == "v2":
            s = 2.0 / (w + h)
            dense = torch.nn.functional.huber_loss(s * p, s * g, delta=DELTA)
        elif kind == "mse":
            dense = torch.sqrt(((g - p) ** 2).sum(-1)).mean()
        else:
            dense = ((g - p).abs().sum(-1) + EPS).pow(Q).mean()
        dense.backward()
        assert int(counts[l]) == g.shape[0] * h * w
        assert abs(float(per[l].detach()) - float(dense.detach())) <= TOL * float(dense.detach())
        assert float((x.grad - p.grad).abs().max()) <= TOL * float(p.grad.abs().max())


def test_float32_inputs_stay_float32_and_masks_of_every_dtype_agree():
    case = make_case("pyramid_mask30", "v2")
    obj = make_loss("v2", "channels_last")
    gt = torch.from_numpy(case["gt"])
    xs = [torch.from_numpy(p) for p in case["preds"]]
    v = torch.from_numpy(case["valid"])
    base = loss.multiscale_masked(obj, gt, xs, v)
    assert base[1].dtype == torch.float32
    for mask in (v.to(torch.uint8), v.float(), v.double() * 0.25, v.half()):
        got = loss.multiscale_masked(obj, gt, xs, mask)
        assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2])
    ref = loss.multiscale_masked(obj, gt.double(), [x.double() for x in xs], v)
    assert float((base[1].double() - ref[1]).abs().max()) <= 1e-5 * float(ref[1].abs().max())


def test_nan_prediction_at_an_invalid_level_pixel_changes_nothing():
    for kind in KINDS:
        case = make_case("empty_blocks", kind)
        obj = make_loss(kind, "channels_last")
        gt, v = torch.from_numpy(case["gt"]).double(), torch.from_numpy(case["valid"])
        xs = [torch.from_numpy(p).double().requires_grad_() for p in case["preds"]]
        want = loss.multiscale_masked(obj, gt, xs, v)
        want[0].backward()
        ys = []
        for x, (g, m) in zip(xs, ref_levels(kind, case["gt"], case["valid"], case["shapes"])):
            y = x.detach().clone()
            y[torch.from_numpy(~m)] = float("nan")
            ys.append(y.requires_grad_())
        got = loss.multiscale_masked(obj, gt, ys, v)
        got[0].backward()
        assert torch.equal(got[1], want[1])
        assert all(torch.equal(a.grad, b.grad) for a, b in zip(xs, ys))


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    gt = torch.zeros(2, 8, 16, 2)
    x = [torch.zeros(2, 4, 8, 2)]
    obj = loss.FlowMseLoss("channels_last")
    with pytest.raises(TypeError, match="FlowMseLossV2, FlowMseLoss or FlowMseLossFineTune"):
        loss.multiscale_masked(loss.AutoResizeMseLoss(), gt, x)
    with pytest.raises(TypeError):
        loss.masked_ground_truth(loss.AutoResizeMseLoss(), gt, [(4, 8)])
    with pytest.raises(TypeError):
        loss.multiscale_masked_torch(torch.nn.MSELoss(), gt, x)
    with pytest.raises(TypeError, match="valid must be a torch.Tensor or None"):
        loss.multiscale_masked(obj, gt, x, valid=np.ones((2, 8, 16)))
    with pytest.raises(TypeError, match="bool, uint8 or floating"):
        loss.multiscale_masked(obj, gt, x, valid=torch.ones(2, 8, 16, dtype=torch.int32))
    for bad in ((2, 8, 16, 1), (2, 16, 8), (1, 8, 16), (2, 8, 16, 2)):
        with pytest.raises(ValueError, match="valid must have shape"):
            loss.multiscale_masked(obj, gt, x, valid=torch.ones(bad, dtype=torch.bool))
        with pytest.raises(ValueError, match="valid must have shape"):
            loss.masked_ground_truth(obj, gt, [(4, 8)], valid=torch.ones(bad, dtype=torch.bool))
    with pytest.raises(ValueError, match="valid is on"):
        loss.multiscale_masked(obj, gt, x, valid=torch.ones(2, 8, 16, dtype=torch.bool, device="meta"))
    with pytest.raises(ValueError, match="2-channel flow"):
        loss.multiscale_masked(obj, torch.zeros(2, 8, 16, 3), x)
    with pytest.raises(ValueError, match="2-channel flow"):
        loss.multiscale_masked(loss.FlowMseLoss("channels_first"), gt, x)          # read as (B,2,H,W): 8 channels
    with pytest.raises(ValueError, match="whole-block"):
        loss.multiscale_masked(make_loss("v2", "channels_last"), gt, [torch.zeros(2, 3, 8, 2)])
    with pytest.raises(ValueError, match="1..8"):
        loss.multiscale_masked(obj, gt, [])
    # the mask of a channels_first loss is (B,H,W) as well
    cf = loss.FlowMseLoss("channels_first")
    out = loss.multiscale_masked(cf, torch.zeros(2, 2, 8, 16), [torch.ones(2, 2, 4, 8)], torch.ones(2, 8, 16).bool())
    assert float(out[0]) == pytest.approx(2.0 ** 0.5) and int(out[2][0]) == 64


# ---- header, table, queries -------------------------------------------------------------------------------------------
NAMES = ["qpwc_masked_loss_workspace_floats", "qpwc_masked_loss_fwd", "qpwc_masked_loss_fwd_kernel",
         "qpwc_masked_loss_bwd"]


def test_masked_loss_prototypes_match_their_header():
    protos = parse_header(HEADER)
    assert [name for name, _, _ in protos] == NAMES
    assert mismatches(_hip.MASKED_LOSS_PROTOTYPES, protos) == []
    others = (set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES) | set(_hip.TRIPLET_PROTOTYPES) | set(_hip.VIS_PROTOTYPES)
              | set(_hip.QUALITY_PROTOTYPES) | set(_hip.REVIEW_PROTOTYPES) | set(_hip.FLOW_QUALITY_PROTOTYPES))
    assert not set(_hip.MASKED_LOSS_PROTOTYPES) & others
    table = dict(_hip.MASKED_LOSS_PROTOTYPES)
    restype, argtypes = table["qpwc_masked_loss_fwd"]
    assert len(argtypes) == 22
    table["qpwc_masked_loss_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_masked_loss_fwd: 22 parameters, table has 21"]
    with open(os.path.join(ROOT, "qpwcnet_amd", "csrc", "masked_loss.hip")) as f:   # under the family's names
        src = f.read()
    assert "kLossTileBlocks = {};".format(_hip.MASKED_LOSS_TILE_BLOCKS) in src
    assert "kLossPixBlocks = {};".format(_hip.MASKED_LOSS_PIX_BLOCKS) in src
    assert "kLossThreads = {};".format(_hip.MASKED_LOSS_THREADS) in src
    assert "kLossTile = {};".format(_hip.MASKED_LOSS_TILE) in src
    # both translation units state the family's grid constants before loss_common.h: the two statements are one text
    with open(os.path.join(ROOT, "qpwcnet_amd", "csrc", "loss.hip")) as f:
        dense = f.read()
    grid = lambda text: re.findall(r"^constexpr int (kLoss\w+) = (\d+);", text, re.M)
    assert grid(src) == grid(dense) and len(grid(src)) == 5


def test_the_library_exports_the_table(hip_lib):
    for name, (restype, argtypes) in _hip.MASKED_LOSS_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_workspace_and_kernel_queries(hip_lib):
    from qpwcnet_amd import ops
    ws, kernel = hip_lib.qpwc_masked_loss_workspace_floats, hip_lib.qpwc_masked_loss_fwd_kernel
    hs, wd = _ints(128, 64, 32, 16, 8), _ints(256, 128, 64, 32, 16)
    for kind in CODES.values():
        assert ws(kind, 8, 256, 512, 2, hs, wd, 5) == 5 * 2 * _hip.MASKED_LOSS_TILE_BLOCKS
        assert ws(kind, 8, 256, 512, 2, hs, wd, 1) == 2 * _hip.MASKED_LOSS_TILE_BLOCKS
    assert _hip.MASKED_LOSS_PIX_BLOCKS <= _hip.MASKED_LOSS_TILE_BLOCKS           # one workspace serves both kernels
    for bad_kind in (_hip.LOSS_AUTORESIZE_MSE, -1, 4):
        assert ws(bad_kind, 8, 256, 512, 2, hs, wd, 5) == _hip.E_MODE
        assert kernel(bad_kind, 8, 256, 512, 2, hs, wd, 5) == b""
    assert ws(0, 8, 256, 512, 2, hs, wd, 9) == _hip.E_SHAPE and ws(0, 8, 256, 512, 2, hs, wd, 0) == _hip.E_SHAPE
    assert ws(1, 8, 256, 512, 3, hs, wd, 5) == _hip.E_SHAPE and ws(0, 0, 256, 512, 2, hs, wd, 5) == _hip.E_SHAPE
    assert ws(0, 8, 256, 512, 2, None, wd, 5) == _hip.E_NULL and ws(0, 8, 256, 512, 2, hs, None, 5) == _hip.E_NULL
    assert ws(0, 8, 256, 512, 2, _ints(100), _ints(128), 1) == _hip.E_SHAPE       # the area kind: whole blocks only
    assert ws(1, 8, 256, 512, 2, _ints(100), _ints(128), 1) == 2 * _hip.MASKED_LOSS_TILE_BLOCKS
    pick = lambda kind, B, H, W, shapes: ops.masked_loss_kernel(CODES[kind], B, H, W, shapes)
    assert pick("v2", 8, 256, 512, list(zip(hs, wd))) == "masked_loss_tile_kernel"           # the trainer's pyramid
    assert pick("v2", *PYRAMID[:3], PYRAMID[3]) == "masked_loss_tile_kernel"
    assert pick("v2", *PYRAMID[:3], PYRAMID[3][::-1]) == "masked_loss_tile_kernel"           # in any order
    assert pick("v2", *THREE[:3], THREE[3]) == "masked_loss_pixel_kernel"                    # 3 x 3
    assert pick("v2", *NARROW[:3], NARROW[3]) == "masked_loss_pixel_kernel"                  # W % 32 != 0
    assert pick("v2", 2, 32, 64, [(32, 64)]) == "masked_loss_pixel_kernel"                   # 1 x 1
    assert pick("v2", 2, 64, 64, [(32, 16), (16, 32)]) == "masked_loss_pixel_kernel"         # not nested
    for kind in ("mse", "finetune"):
        assert pick(kind, *PYRAMID[:3], PYRAMID[3]) == "masked_loss_pixel_kernel"
        assert pick(kind, *NONINT[:3], NONINT[3]) == "masked_loss_pixel_kernel"
    assert pick("v2", *NONINT[:3], NONINT[3]) == "" and pick("v2", 0, 32, 64, [(16, 32)]) == ""


# ---- the shapes of the GPU suite's grid-loop cases --------------------------------------------------------------------
TILE_LOOP = (3, 832, 864, [(416, 432), (104, 108)])      # area kind, factors 2 and 8
PIXEL_LOOP = (2, 40, 52, [(365, 363)])                   # bilinear, upsampling: the level is larger than the ground truth


def test_the_grid_loop_cases_pass_the_grid_caps(hip_lib):
    """tests/test_gpu_masked_loss.py runs these two: more 32 x 32 tiles than the tile kernel has workgroups (but fewer
    than twice as many: no third trip is needed to show the loop), and more level pixels than the pixel kernel's grid
    covers in one trip."""
    from qpwcnet_amd import ops
    B, H, W, shapes = TILE_LOOP
    tiles = B * (H // _hip.MASKED_LOSS_TILE) * (W // _hip.MASKED_LOSS_TILE)
    assert H % _hip.MASKED_LOSS_TILE == 0 and W % _hip.MASKED_LOSS_TILE == 0
    assert _hip.MASKED_LOSS_TILE_BLOCKS < tiles < 2 * _hip.MASKED_LOSS_TILE_BLOCKS
    assert ops.masked_loss_kernel(_hip.LOSS_FLOW_MSE_V2, B, H, W, shapes) == "masked_loss_tile_kernel"
    B, H, W, shapes = PIXEL_LOOP
    trip = _hip.MASKED_LOSS_PIX_BLOCKS * _hip.MASKED_LOSS_THREADS
    assert trip < B * shapes[0][0] * shapes[0][1] < 2 * trip
    assert ops.masked_loss_kernel(_hip.LOSS_FLOW_FINETUNE, B, H, W, shapes) == "masked_loss_pixel_kernel"
    for n_out, n_in in ((shapes[0][0], H), (shapes[0][1], W)):                   # no sample point on a pixel centre
        assert all((n_in * (2 * o + 1) - n_out) % (2 * n_out) != 0 for o in range(n_out))

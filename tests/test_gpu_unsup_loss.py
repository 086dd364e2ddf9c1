"""The label-free flow losses on the MI355X: unsup_loss_fwd_kernel / unsup_loss_fold_kernel / unsup_loss_bwd_kernel behind
qpwcnet_amd.loss.multiscale_unsupervised, both kinds, both flow layouts, fp32 and fp16 flows, occluded in None, a random
mask and 'estimate'.

Oracle: ``loss.multiscale_unsupervised_torch`` on float64 CPU tensors, fed the same values (the fp16 flows are exact in
fp16; 'estimate': the mask the device estimated); tests/test_unsup_loss_cpu.py holds that chain to a numpy restatement
within 1e-12.  Inputs: tests/test_unsup_loss_cpu.py::make_case -- B = 2, 32 x 48 and 40 x 72 with four levels each
(tiles that meet inside the image, partial tiles on both axes, a level with census count 0, factor 1), flows on the
1/16-pixel grid, never an integer, up to w / 2, so that fp32 and float64 agree on every mask and no pixel is left out of
any comparison; with occluded=None between a tenth and a half of every level's census candidates leave the image
(asserted on the oracle's counts).

Bounds: counts exact.  Losses, parts and gradients: 4 x the error of the same torch chain run in float32 on the CPU
against float64 on these inputs (the kernel sums in another order), and never below 1e-5 -- relative for losses and parts,
of the level's largest gradient for gradients; fp16 gradients (loss scaled by 2^16) F16_EPS |g| + that bound + 2^-24.
Measured floor, the CPU float32 chain against float64 on these cases: losses 1.3e-7 relative, photometric 1.5e-7,
smoothness 9.2e-8; census gradients 2.5e-6 .. 9.2e-6 of the level's largest at 32 x 48 and 40 x 72 and 1.9e-5 at
136 x 264 (the float32 cancellation in the grey differences D is the chain's own), so the census gradient bound lies
between 1e-5 and 3.7e-5 there and is 7.5e-5 at 136 x 264; Charbonnier gradients below 2.5e-6: the bound is the 1e-5.
Observed on an MI355X, the worst case of the module as a share of its bound: losses 0.011, photometric 0.009, smoothness
0.012, fp32 gradients 0.27 (census: the kernel's error is the float32 chain's, 2e-6 .. 9e-6 of the largest and 1.9e-5 at
136 x 264; Charbonnier 7e-8 .. 1.8e-7), fp16 gradients 0.94 (the half ulp of fp16 itself).  The last test prints both.

The grids are one workgroup per tile, not capped, and no kernel walks a remainder; the one loop is the fold's, over a
level's tiles in steps of its 256 threads: test_the_fold_walks_more_tiles_than_it_has_threads has a level of 306 tiles.

The sample points the contract singles out (test_contract_edges_*): make_case never puts a sample on an integer, so
alpha = 0, q = 0 and q = extent - 1 (floor clamped to extent - 2, alpha = 1, inside) never reached the kernel.
tests/test_unsup_loss_cpu.py::make_edge_case plants them: B = 2, 40 x 72 (partial tiles along x, seams inside the image)
and 17 x 65 (partial tiles on both axes, the column x = w - 1 the first of a tile); per image at least 16 pixels of each
class -- q an interior integer, q = 0, q = extent - 1, q 1/16 beyond either end, q more than a whole image beyond -- on
both axes, so at all four sides, one of each in the 3-pixel border strip and one in every partial last tile; flows on the
1/16 grid, exact in fp16.  The companion proves all that on the float64 restatement, holds the oracle to the numpy loops
on a small instance, and holds its gradient to the header's closed form (the slope towards the second tap where inside,
exactly 0 where not), so a tie the oracle split differently would show there.  Bounds: the module's, unchanged.

Degenerate extents and the plan (test_eight_unrelated_levels_in_one_launch and the four tests after it): every level in
one ops.unsup_loss launch, each with frames of its own, the oracle per level.  TINY_LEVELS: 1 x 1, 17 x 65, 1 x 40,
9 x 1, 2 x 2, 6 x 40, 7 x 7, 8 x 33, not in descending order, fp32 and fp16 flows and None and a mask alternating by
level; along an axis of extent 1 every other pixel has a zero flow component, since q = 0 is the only inside point
there.  A 40 x 72 level with everything occluded beside an ordinary one; (q, eps, edge, smooth_eps) at two other sets;
the eight levels reversed.  Observed on an MI355X, worst error over bound (test_report prints them per group): contract
edges: losses 0.011, photometric 0.007, smoothness 0.010, fp32 gradients 0.26, fp16 gradients 0.93; plan: losses 0.016,
photometric 0.007, smoothness 0.012, fp32 gradients 0.26, fp16 gradients 0.96.  The float32 chain's own gradient error
on these cases: 1e-5 of the level's largest at the contract edges, 4.4e-5 at the 17 x 65 level of TINY_LEVELS (its bound
is 1.8e-4 there).

One-line changes to csrc/unsup_loss.hip that these tests catch and the ones above do not, argued on paper (a broken kernel
is never run):
  * `qx <= (float)(w - 1)` to `<` in unsup_taps (or `qx >= 0.0f` to `>`): with make_case no qx equals w - 1, so both
    forms agree on every pixel of every older test.  In make_edge_case every image has at least 16 pixels with
    qx = w - 1 and qy inside; those among the unoccluded census candidates leave the count, which is compared exactly
    with the oracle's, and test_contract_edges_pass_a_gradient_on_the_border_and_none_beyond finds an all-zero gradient
    where the oracle has one, for that side alone.  A wrong slope at a clamped tap (`t.x1 = min(t.x0 + 1, w - 1)` read as
    the floor's own column when alpha = 1) changes the gradient at the same pixels and nowhere else.
  * `max(h - 2, 0)` to `h - 2` in unsup_taps: the two differ at h = 1 only, where the floor becomes -1 and the first tap
    the row before the image.  The older tests reach h = 1 in test_flower_model_trains_without_a_label alone, which
    asks for finite numbers, and whose samples at h = 1 are never inside.  Here the 1 x 1 and 1 x 40 levels hold pixels
    with qy = 0 that Charbonnier counts (asserted on the oracle): alpha becomes 1 instead of 0, d / d qy becomes
    bot - top with top read from another image (or from before the tensor) where the contract says 0, and the gradient
    in v leaves its bound; `max(w - 2, 0)` the same at 9 x 1 and 1 x 1.
  * the level walk of unsup_tile.  `bid >= lv.tile_start[k]` to `>` sends the first tile of every level k >= 1 to image B
    of level k - 1: on paper the four-level cases above lose a tile of 90 census candidates as well, so they notice it
    too, if only through what an out-of-bounds image happens to hold.  Here it is certain: image 0 of the 7 x 7 level,
    one tile, goes to image B of 6 x 40, where census counts nothing whatever it reads, so the count of 2 becomes 1; and
    the bit-equality with the reversed list, where another level precedes each, and with the level launched alone
    fails by construction.  What only these tests catch: `k < n_levels` to `k < 4` (every older launch has four levels
    or one; levels 4 .. 7 of TINY_LEVELS would fold into level 3), `lv.f16[l]` to `lv.f16[0]` in a flow load or store
    (every older launch has one dtype; here they alternate), and a kernel that took `lv.occ[0] == NULL` for "no level
    has a mask".
The fourth gap, offsets past 2^31, is tests/test_gpu_large_offsets.py::test_unsup_loss."""
import numpy as np
import pytest
import torch

from test_unsup_loss_cpu import (EDGE_SHAPES, OUTSIDE_CLASSES, TINY_LEVELS, KINDS, edge_classes, make_case, make_edge_case,
                                 make_levels, to_layout)

from qpwcnet_amd import _hip, layers, loss, ops, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16_EPS = 2.0 ** -11
SHAPES = {"32x48": (32, 48, 11), "40x72": (40, 72, 12)}       # (H, W, seed): four levels each
FOLD_LOOP = {"136x264": (136, 264, 31)}                         # one level
WORST, FLOOR = {}, {}
_CASES, _ORACLES = {}, {}


def _note(book, key, value, bound=1.0, tag=None):
    """The worst figure of the module under `key`, and of the tag's group of cases under 'group: key'."""
    keys = [key]
    if tag is not None:
        group = "contract edges" if tag[1] in EDGE_SHAPES else "plan" if tag[1] in PLAN_CASES else None
        keys += ["{}: {}".format(group, key)] if group else []
    for k in keys:
        book[k] = max(book.get(k, 0.0), float(value) / bound)


PLAN_CASES = ("tiny", "all-occluded", "parameters")             # the cases launched through ops.unsup_loss directly
PARAMS = (0.4, 0.01, 40.0, 1e-3)                                # (q, eps, edge, smooth_eps) of every test but one
KIND_IDS = {"census": _hip.UNSUP_CENSUS, "charbonnier": _hip.UNSUP_CHARBONNIER}


def _dims(shape):
    for book in (SHAPES, FOLD_LOOP, EDGE_SHAPES):
        if shape in book:
            return book[shape][:2]
    raise KeyError(shape)


def _case(shape):
    if shape not in _CASES:
        if shape in EDGE_SHAPES:
            _CASES[shape] = make_edge_case(*EDGE_SHAPES[shape])
        else:
            _CASES[shape] = make_case(*SHAPES[shape]) if shape in SHAPES else make_case(*FOLD_LOOP[shape], levels=1)
    return _CASES[shape]


def _make_loss(kind, data_format, smooth_weight=1.5, params=PARAMS):
    # edge = 40: the frames' neighbour differences are a few hundredths, so the weights spread over (0, 1)
    q, eps, edge, smooth_eps = params
    return loss.PhotometricLoss(kind, q=q, eps=eps, smooth_weight=smooth_weight, edge=edge, smooth_eps=smooth_eps,
                                data_format=data_format)


def _estimate(shape):
    """The device's own occlusion estimate of every level flow (channels-last), as uint8 on the CPU."""
    key = (shape, "estimate-masks")
    if key not in _ORACLES:
        from qpwcnet_amd import occlusion
        _ORACLES[key] = [(occlusion.estimate_occlusion_map(torch.from_numpy(f).to(DEV), "channels_last") != 0)
                         .to(torch.uint8).cpu() for f in _case(shape)["flows"]]
    return _ORACLES[key]


def _masks(shape, occluded):
    case = _case(shape)
    if occluded == "none":
        return None
    return [torch.from_numpy(m) for m in case["masks"]] if occluded == "mask" else _estimate(shape)


def _chain(obj, pairs, flows, masks, dtype):
    """The channels-last torch chain on the CPU in `dtype` -> (per, parts, grads), everything as float64."""
    xs = [torch.from_numpy(f).to(dtype).requires_grad_() for f in flows]
    total, per, parts = loss.multiscale_unsupervised_torch(obj, torch.from_numpy(pairs).to(dtype), xs, masks)
    total.backward()
    return (per.detach().double(), {k: v.double() if v.is_floating_point() else v for k, v in parts.items()},
            [x.grad.double() for x in xs])


def _oracle(kind, shape, occluded, smooth_weight=1.5):
    """(float64 reference, per-quantity bounds) of one case of the module's shapes, made once."""
    case = _case(shape)
    return _oracle_of((kind, shape, occluded, smooth_weight), _make_loss(kind, "channels_last", smooth_weight),
                      case["pairs"], case["flows"], _masks(shape, occluded))


def _oracle_of(key, obj, pairs, flows, masks):
    """(float64 reference, per-quantity bounds) of the chain on these inputs, made once per key: bounds = max(4 x |float32
    chain - float64 chain|, 1e-5 of the reference's size)."""
    if key not in _ORACLES:
        per, parts, grads = _chain(obj, pairs, flows, masks, torch.float64)
        per32, parts32, grads32 = _chain(obj, pairs, flows, masks, torch.float32)
        assert torch.equal(parts["counts"], parts32["counts"])
        bounds = {"per": [], "photometric": [], "smoothness": [], "grad": []}
        for l in range(len(grads)):
            for name, a, b in (("per", per, per32), ("photometric", parts["photometric"], parts32["photometric"]),
                               ("smoothness", parts["smoothness"], parts32["smoothness"])):
                err, size = abs(float(a[l]) - float(b[l])), abs(float(a[l]))
                bounds[name].append(max(4.0 * err, 1e-5 * size))
                _note(FLOOR, name, err / max(size, 1e-30))
            top = float(grads[l].abs().max())
            err = float((grads[l] - grads32[l]).abs().max())
            bounds["grad"].append(max(4.0 * err, 1e-5 * top))
            _note(FLOOR, "grad", err / max(top, 1e-30))
        _ORACLES[key] = (per, parts, grads, bounds)
    return _ORACLES[key]


def _device_run(kind, shape, occluded, data_format, dtype, smooth_weight=1.5, scale=1.0):
    case = _case(shape)
    obj = _make_loss(kind, data_format, smooth_weight)
    xs = [to_layout(f, data_format, dtype).to(DEV).requires_grad_() for f in case["flows"]]
    occ = "estimate" if occluded == "estimate" else _masks(shape, occluded)
    occ = [m.to(DEV) for m in occ] if isinstance(occ, list) else occ
    total, per, parts = loss.multiscale_unsupervised(obj, to_layout(case["pairs"], data_format, torch.float32).to(DEV), xs, occ)
    (scale * per).sum().backward()
    grads = [x.grad if data_format == "channels_last" else x.grad.permute(0, 2, 3, 1) for x in xs]
    return total, per, parts, xs, grads


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("occluded", ["none", "mask", "estimate"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_match_the_float64_chain(kind, shape, occluded, data_format, dtype):
    _compare(kind, shape, occluded, data_format, dtype)


def _compare(kind, shape, occluded, data_format, dtype):
    """One forward + backward on the device against the oracle, every bound of the module."""
    ref_per, ref_parts, ref_grads, bounds = _oracle(kind, shape, occluded)
    scale = 1.0 if dtype == torch.float32 else 2.0 ** 16          # loss scaling keeps the fp16 gradients normal
    total, per, parts, xs, grads = _device_run(kind, shape, occluded, data_format, dtype, scale=scale)
    tag = (kind, shape, occluded, data_format, dtype)
    H, W = _dims(shape)
    assert per.dtype == torch.float32 and per.device == xs[0].device and parts["counts"].dtype == torch.int64
    print(tag, "counts", parts["counts"].tolist(), "per", per.tolist())
    assert torch.equal(parts["counts"].cpu(), ref_parts["counts"]), (tag, parts["counts"].tolist(), ref_parts["counts"].tolist())
    for l, x in enumerate(xs):
        h, w = H >> l, W >> l
        cand = 2 * max(h - 6, 0) * max(w - 6, 0) if kind == "census" else 2 * h * w
        if occluded == "none" and kind == "census" and cand:         # a case with nothing masked cannot pass unnoticed
            assert 0.1 <= 1.0 - int(ref_parts["counts"][l]) / cand <= 0.5, (tag, l)
        if not cand:
            assert int(parts["counts"][l]) == 0 and float(parts["photometric"][l]) == 0.0
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        _hold(tag, l, dtype, scale, (per[l], parts["photometric"][l], parts["smoothness"][l], grads[l]),
              (ref_per[l], ref_parts["photometric"][l], ref_parts["smoothness"][l], ref_grads[l]),
              {k: v[l] for k, v in bounds.items()})
    assert abs(float(total.detach()) - float(per.detach().sum())) <= 1e-6 * abs(float(per.detach().sum()))


def _hold(tag, l, dtype, scale, got, want, bounds):
    """One level's loss, parts and channels-last gradient (of `scale` times the loss) against the reference and its
    bounds: (per, photometric, smoothness, grad) each."""
    for name, g, w_ in zip(("per", "photometric", "smoothness"), got, want):
        d = abs(float(g.detach()) - float(w_))
        print(tag, l, name, "error", d, "bound", bounds[name])
        assert d <= bounds[name], (tag, l, name, float(g.detach()), float(w_), bounds[name])
        _note(WORST, name, d, max(bounds[name], 1e-30), tag)
    grad, ref = got[3].double().cpu() / scale, want[3]
    d = (grad - ref).abs()
    print(tag, l, "grad error", float(d.max()), "bound", bounds["grad"], "largest", float(ref.abs().max()))
    if dtype == torch.float32:
        assert float(d.max()) <= bounds["grad"], (tag, l, float(d.max()), bounds["grad"])
        _note(WORST, "grad_f32", d.max(), max(bounds["grad"], 1e-30), tag)
    else:
        bound = (F16_EPS * (ref * scale).abs() + bounds["grad"] * scale + 2.0 ** -24) / scale
        assert bool((d <= bound).all()), (tag, l, float((d - bound).max()))
        _note(WORST, "grad_f16", (d / bound).max(), tag=tag)


def _sample_inside(flow):
    """(B,h,w) bool of a channels-last float64 flow: the sample point stays inside the image."""
    h, w = flow.shape[1:3]
    qx = torch.arange(w, dtype=flow.dtype).view(1, 1, w) + flow[..., 0]
    qy = torch.arange(h, dtype=flow.dtype).view(1, h, 1) + flow[..., 1]
    return (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)


@pytest.mark.parametrize("occluded", ["none", "mask"])
@pytest.mark.parametrize("kind", KINDS)
def test_photometric_gradient_is_exactly_zero_where_it_must_be(kind, occluded):
    """smooth_weight = 0: exactly 0 at every pixel whose sample is outside the image, and at every pixel farther than 3
    (census; charbonnier: 0) from all pixels with m_p = 1; and the rest still matches the oracle."""
    shape = "40x72"
    ref_per, ref_parts, ref_grads, bounds = _oracle(kind, shape, occluded, smooth_weight=0.0)
    _, per, parts, xs, grads = _device_run(kind, shape, occluded, "channels_last", torch.float32, smooth_weight=0.0)
    assert torch.equal(parts["counts"].cpu(), ref_parts["counts"]) and torch.equal(per, parts["photometric"])
    masks = _masks(shape, occluded)
    for l, f in enumerate(_case(shape)["flows"]):
        inside = _sample_inside(torch.from_numpy(f).double())
        m = inside if masks is None else inside & (masks[l] == 0)
        h, w = m.shape[1:]
        if kind == "census":
            edge = torch.zeros_like(m)
            edge[:, 3:h - 3, 3:w - 3] = True
            m = m & edge
            near = torch.nn.functional.max_pool2d(m.float()[:, None], 7, stride=1, padding=3)[:, 0] > 0
        else:
            near = m
        assert int(m.sum()) == int(ref_parts["counts"][l])
        got = grads[l].cpu()
        assert not got[~inside].any(), (kind, l)
        assert not got[~near].any(), (kind, l)
        if int(m.sum()):
            assert got[near & inside].any()
        assert float((got.double() - ref_grads[l]).abs().max()) <= bounds["grad"][l]
        assert not ref_grads[l][~inside].any() and not ref_grads[l][~near].any()       # the oracle says the same


@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_the_same_bits(kind):
    a = _device_run(kind, "40x72", "mask", "channels_last", torch.float32)
    b = _device_run(kind, "40x72", "mask", "channels_last", torch.float32)
    assert torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert all(torch.equal(x, y) for x, y in zip(a[4], b[4]))


def test_the_fold_walks_more_tiles_than_it_has_threads():
    """One level of 136 x 264 at B = 2: 2 * 17 * 9 = 306 tiles of 8 x 32, more than the fold's 256 threads, with partial
    tiles on both axes."""
    H, W, _ = FOLD_LOOP["136x264"]
    th, tw = _hip.UNSUP_LOSS_TILE
    assert 256 < 2 * -(-H // th) * -(-W // tw) < 512
    _compare("census", "136x264", "none", "channels_last", torch.float32)


# ---- the sample points the contract singles out --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("occluded", ["none", "mask"])
@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_contract_edges_match_the_float64_chain(kind, shape, occluded, data_format, dtype):
    """make_edge_case: q at interior integers, at 0, at extent - 1, 1/16 outside and a whole image outside, on both axes
    and all four sides -- the counts exact (a `<` for `<=` in inside drops every q = 0 and q = extent - 1 pixel from
    them), everything else within the module's bounds."""
    _compare(kind, shape, occluded, data_format, dtype)


@pytest.mark.parametrize("occluded", ["none", "mask"])
@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_contract_edges_pass_a_gradient_on_the_border_and_none_beyond(kind, shape, occluded):
    """smooth_weight = 0: exactly 0 at every pixel of the outside classes (1/16 beyond either end, and a whole image
    beyond), and nonzero somewhere among the unoccluded pixels of each class with q = 0 and q = extent - 1, per side --
    the oracle says the same, and the rest matches it."""
    ref_per, ref_parts, ref_grads, bounds = _oracle(kind, shape, occluded, smooth_weight=0.0)
    _, per, parts, xs, grads = _device_run(kind, shape, occluded, "channels_last", torch.float32, smooth_weight=0.0)
    assert torch.equal(parts["counts"].cpu(), ref_parts["counts"]) and int(parts["counts"][0]) > 0
    case = _case(shape)
    classes = {k: torch.from_numpy(v) for k, v in edge_classes(case["flows"][0]).items()}
    keep = torch.from_numpy(case["masks"][0] == 0) if occluded == "mask" else torch.ones_like(classes["zero_x"])
    got, want = grads[0].cpu(), ref_grads[0]
    for cls in OUTSIDE_CLASSES:
        assert int(classes[cls].sum()) >= 32
        assert not got[classes[cls]].any() and not want[classes[cls]].any(), (kind, shape, cls)
    for cls in ("zero_x", "zero_y", "last_x", "last_y"):
        sel = classes[cls] & keep
        assert want[sel].any() and got[sel].any(), (kind, shape, cls)
    assert float((got.double() - want).abs().max()) <= bounds["grad"][0]


# ---- degenerate extents and the plan: every level in one ops.unsup_loss launch, the oracle per level -------------------

def _plan_oracle(name, kind, levels, use_mask, params=PARAMS, smooth_weight=1.5):
    """Per level the float64 chain on that level's own frames at factor 1 -> [(per, parts, grads, bounds)]."""
    out = []
    for i, lv in enumerate(levels):
        masks = [torch.from_numpy(lv["mask"])] if use_mask[i] else None
        out.append(_oracle_of((name, i, kind, params, smooth_weight, use_mask[i]),
                              _make_loss(kind, "channels_last", smooth_weight, params), lv["pairs"], [lv["flow"]], masks))
    return out


def _plan_run(kind, levels, use_mask, f16, data_format="channels_last", params=PARAMS, smooth_weight=1.5, scale=1.0):
    """One ops.unsup_loss launch (+ one backward of scale * sum) of these levels -> (losses, photometric, smoothness,
    counts, channels-last gradients)."""
    q, eps, edge, smooth_eps = params
    frame = lambda lv, lo: torch.from_numpy(lv["pairs"][..., lo:lo + 3].copy()).to(DEV)
    xs = [to_layout(lv["flow"], data_format, torch.float16 if half else torch.float32).to(DEV).requires_grad_()
          for lv, half in zip(levels, f16)]
    occ = [torch.from_numpy(lv["mask"]).to(DEV) if m else None for lv, m in zip(levels, use_mask)]
    losses, photo, smooth, counts = ops.unsup_loss(KIND_IDS[kind], [frame(lv, 0) for lv in levels],
                                                   [frame(lv, 3) for lv in levels], xs, occ, data_format, q, eps,
                                                   smooth_weight, edge, smooth_eps)
    (scale * losses).sum().backward()
    for x, half in zip(xs, f16):
        assert x.grad.dtype == (torch.float16 if half else torch.float32) and x.grad.shape == x.shape
    grads = [x.grad if data_format == "channels_last" else x.grad.permute(0, 2, 3, 1) for x in xs]
    return losses.detach(), photo, smooth, counts, grads


def _hold_plan(tag, got, refs, f16, scale):
    losses, photo, smooth, counts, grads = got
    assert losses.dtype == torch.float32 and counts.dtype == torch.int64 and len(refs) == losses.numel()
    want_counts = [int(r[1]["counts"][0]) for r in refs]
    print(tag, "counts", counts.tolist(), "oracle", want_counts)
    assert counts.tolist() == want_counts, (tag, counts.tolist(), want_counts)
    for l, (per, parts, ref_grads, bounds) in enumerate(refs):
        _hold(tag, l, torch.float16 if f16[l] else torch.float32, scale, (losses[l], photo[l], smooth[l], grads[l]),
              (per[0], parts["photometric"][0], parts["smoothness"][0], ref_grads[0]), {k: v[0] for k, v in bounds.items()})


def _tiny():
    if "tiny" not in _CASES:
        _CASES["tiny"] = make_levels(TINY_LEVELS, 50)
    n = len(TINY_LEVELS)
    return _CASES["tiny"], [l % 2 == 1 for l in range(n)], [l % 2 == 1 for l in range(n)]     # levels, masks, fp16


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("kind", KINDS)
def test_eight_unrelated_levels_in_one_launch(kind, data_format):
    """TINY_LEVELS at B = 2 in one launch: 1 x 1, 1 x N, N x 1, 2 x 2, 6 x N, 7 x 7, 8 x 33 and 17 x 65, not in descending
    order, fp32 and fp16 flows and None and a mask alternating by level.  Every expectation is the oracle's."""
    levels, use_mask, f16 = _tiny()
    refs = _plan_oracle("tiny", kind, levels, use_mask)
    scale = 2.0 ** 16
    tag = (kind, "tiny", data_format)
    got = _plan_run(kind, levels, use_mask, f16, data_format, scale=scale)
    _hold_plan(tag, got, refs, f16, scale)
    flat = _plan_run(kind, levels, use_mask, f16, data_format, smooth_weight=0.0, scale=scale)
    flat_refs = _plan_oracle("tiny", kind, levels, use_mask, smooth_weight=0.0)
    _hold_plan(tag + ("smooth_weight 0",), flat, flat_refs, f16, scale)
    losses, photo, smooth, counts, grads = got
    for l, (h, w) in enumerate(TINY_LEVELS):
        per, parts, ref_grads, _ = refs[l]
        if kind == "census" and (h < 7 or w < 7):
            # count 0, photometric 0, and the gradient is the smoothness-only one: none at all at smooth_weight = 0
            assert int(parts["counts"][0]) == 0 and float(parts["photometric"][0]) == 0.0
            assert int(counts[l]) == 0 and float(photo[l]) == 0.0
            assert not flat[4][l].any() and not flat_refs[l][2][0].any() and float(flat[0][l]) == 0.0
        if kind == "charbonnier" and (h == 1 or w == 1):
            # q = 0 along the axis of extent 1 is inside: the floor clamped to max(extent - 2, 0) carries pixels that count
            assert 0 < int(parts["counts"][0]) == int(counts[l])
        if (h, w) == (1, 1):
            assert float(parts["smoothness"][0]) == 0.0 and not ref_grads[0].any()
            assert float(smooth[l]) == 0.0 and not grads[l].any()
        elif h > 1 and w > 1:
            assert float(parts["smoothness"][0]) > 0.0 and grads[l].any()
        if kind == "census" and (h, w) == (7, 7):
            assert not use_mask[l] and int(parts["counts"][0]) == 2 and int(counts[l]) == 2
            assert flat[4][l][:, 3, 3].any() and flat_refs[l][2][0][:, 3, 3].any()


@pytest.mark.parametrize("kind", KINDS)
def test_reversed_levels_give_the_same_bits(kind):
    """Nothing of a level depends on its place in the table: the launch of the eight levels with the list reversed gives,
    level for level, the bits of the first launch."""
    levels, use_mask, f16 = _tiny()
    a = _plan_run(kind, levels, use_mask, f16)
    b = _plan_run(kind, levels[::-1], use_mask[::-1], f16[::-1])
    for k in range(4):
        assert torch.equal(a[k], b[k].flip(0)), (kind, k, a[k].tolist(), b[k].tolist())
    for l, (x, y) in enumerate(zip(a[4], b[4][::-1])):
        assert torch.equal(x, y), (kind, l)


def _occluded_pair():
    if "all-occluded" not in _CASES:
        first, second = make_levels(((40, 72), (32, 48)), 60)
        first["mask"] = np.ones_like(first["mask"])
        _CASES["all-occluded"] = [first, second]
    return _CASES["all-occluded"]


@pytest.mark.parametrize("kind", KINDS)
def test_a_level_with_everything_occluded_beside_an_ordinary_one(kind):
    """40 x 72 with a mask of ones, then 32 x 48 with a random mask, in one launch: the first has count 0 and
    photometric exactly 0, its gradient is the smoothness one (within the bound at smooth_weight = 1.5, exactly 0 at
    smooth_weight = 0) although all 7 planes of it are written and read back; the second is bit-equal to the same level
    launched alone."""
    levels = _occluded_pair()
    both, f16 = [True, True], [False, False]
    refs = _plan_oracle("all-occluded", kind, levels, both)
    got = _plan_run(kind, levels, both, f16)
    _hold_plan((kind, "all-occluded"), got, refs, f16, 1.0)
    assert int(refs[0][1]["counts"][0]) == 0 and float(refs[0][1]["photometric"][0]) == 0.0 and int(refs[1][1]["counts"][0]) > 0
    assert int(got[3][0]) == 0 and float(got[1][0]) == 0.0 and got[4][0].any()
    flat = _plan_run(kind, levels, both, f16, smooth_weight=0.0)
    assert float(flat[0][0]) == 0.0 and not flat[4][0].any() and flat[4][1].any()
    for smooth_weight, pair in ((1.5, got), (0.0, flat)):
        alone = _plan_run(kind, levels[1:], both[1:], f16[1:], smooth_weight=smooth_weight)
        for k in range(4):
            assert torch.equal(pair[k][1:], alone[k]), (kind, smooth_weight, k)
        assert torch.equal(pair[4][1], alone[4][0]), (kind, smooth_weight)


@pytest.mark.parametrize("params", [(0.5, 1e-3, 0.0, 0.02), (1.0, 0.05, 150.0, 1e-3)], ids=["q0.5", "q1.0"])
@pytest.mark.parametrize("kind", KINDS)
def test_other_parameters(kind, params):
    """(q, eps, edge, smooth_eps) away from the module's one set, one 32 x 48 level with a mask: edge = 0 (every weight
    1), edge = 150 (the default; most weights small), q = 1 (the power is the identity), a large smooth_eps.  Bounds as
    everywhere: 4 x the float32 chain on the same case, floor 1e-5."""
    if "parameters" not in _CASES:
        _CASES["parameters"] = make_levels(((32, 48),), 70)
    levels = _CASES["parameters"]
    refs = _plan_oracle("parameters", kind, levels, [True], params)
    got = _plan_run(kind, levels, [True], [False], params=params)
    assert 0 < int(refs[0][1]["counts"][0]) < 2 * 32 * 48
    _hold_plan((kind, "parameters", params), got, refs, [False], 1.0)


def test_flower_model_trains_without_a_label():
    """FlowerModel at B = 1, 64 x 64 through multiscale_unsupervised(occluded='estimate') and backward(): every parameter
    has a finite gradient, the flows' gradients are nonzero, and the loss takes the launches INTEGRATION.md states: one
    pooling launch per distinct factor above 1, one occlusion estimate per level, then one forward (+ its fold) and one
    backward launch for all levels."""
    model = layers.FlowerModel(data_format="channels_last")
    model.load_state_dict({k: torch.as_tensor(v) for k, v in synth.make_weights(42, (64, 64)).items()})
    model = model.to(DEV).train()
    pairs = torch.as_tensor(synth.make_frames(1, 64, 64, seed=5)[0]).to(DEV)
    flows = model(pairs)
    assert [tuple(f.shape[1:3]) for f in flows] == [(2, 2), (4, 4), (8, 8), (16, 16), (32, 32), (64, 64)]
    for f in flows:
        f.retain_grad()
    obj = loss.PhotometricLoss(data_format="channels_last")
    with ops.kernel_timing() as kt:
        total, per, parts = loss.multiscale_unsupervised(obj, pairs, flows, occluded="estimate")
        n_fwd = len(kt.records)
        total.backward()
    ours = [key[0] for key, _, _ in kt.records if key[0] in ("avgpool_pyramid", "occlusion", "unsup_loss", "unsup_loss_bwd")]
    assert ours.count("avgpool_pyramid") == 5 and ours.count("occlusion") == 6
    assert ours.count("unsup_loss") == 1 and ours.count("unsup_loss_bwd") == 1
    assert [key[0] for key, _, _ in kt.records[:n_fwd]].count("unsup_loss_bwd") == 0
    assert bool(torch.isfinite(per).all()) and parts["counts"].tolist()[:2] == [0, 0] and int(parts["counts"][-1]) > 0
    for f in flows:
        assert bool(torch.isfinite(f.grad).all()) and f.grad.any()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert sum(int(p.grad.any()) for p in model.parameters()) > 10


def test_report():
    print("CPU float32 chain against float64 (the floor):", {k: "%.2e" % v for k, v in sorted(FLOOR.items())})
    print("worst observed / bound:", {k: "%.3f" % v for k, v in sorted(WORST.items())})

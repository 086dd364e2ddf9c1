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
level's tiles in steps of its 256 threads: test_the_fold_walks_more_tiles_than_it_has_threads has a level of 306 tiles."""
import pytest
import torch

from test_unsup_loss_cpu import KINDS, make_case, to_layout

from qpwcnet_amd import _hip, layers, loss, ops, synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16_EPS = 2.0 ** -11
SHAPES = {"32x48": (32, 48, 11), "40x72": (40, 72, 12)}       # (H, W, seed): four levels each
FOLD_LOOP = {"136x264": (136, 264, 31)}                         # one level
WORST, FLOOR = {}, {}
_CASES, _ORACLES = {}, {}


def _note(book, key, value, bound=1.0):
    book[key] = max(book.get(key, 0.0), float(value) / bound)


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = make_case(*SHAPES[shape]) if shape in SHAPES else make_case(*FOLD_LOOP[shape], levels=1)
    return _CASES[shape]


def _make_loss(kind, data_format, smooth_weight=1.5):
    # edge = 40: the frames' neighbour differences are a few hundredths, so the weights spread over (0, 1)
    return loss.PhotometricLoss(kind, smooth_weight=smooth_weight, edge=40.0, data_format=data_format)


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


def _chain(kind, shape, occluded, dtype, smooth_weight):
    """The channels-last torch chain on the CPU in `dtype` -> (per, parts, grads), everything as float64."""
    case = _case(shape)
    obj = _make_loss(kind, "channels_last", smooth_weight)
    xs = [torch.from_numpy(f).to(dtype).requires_grad_() for f in case["flows"]]
    total, per, parts = loss.multiscale_unsupervised_torch(obj, torch.from_numpy(case["pairs"]).to(dtype), xs,
                                                           _masks(shape, occluded))
    total.backward()
    return (per.detach().double(), {k: v.double() if v.is_floating_point() else v for k, v in parts.items()},
            [x.grad.double() for x in xs])


def _oracle(kind, shape, occluded, smooth_weight=1.5):
    """(float64 reference, per-quantity bounds) of one case, made once: bounds = max(4 x |float32 chain - float64 chain|,
    1e-5 of the reference's size)."""
    key = (kind, shape, occluded, smooth_weight)
    if key not in _ORACLES:
        per, parts, grads = _chain(kind, shape, occluded, torch.float64, smooth_weight)
        per32, parts32, grads32 = _chain(kind, shape, occluded, torch.float32, smooth_weight)
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
    H, W, _ = SHAPES[shape] if shape in SHAPES else FOLD_LOOP[shape]
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
        for name, got, want in (("per", per, ref_per), ("photometric", parts["photometric"], ref_parts["photometric"]),
                                ("smoothness", parts["smoothness"], ref_parts["smoothness"])):
            d = abs(float(got[l].detach()) - float(want[l]))
            print(tag, l, name, "error", d, "bound", bounds[name][l])
            assert d <= bounds[name][l], (tag, l, name, float(got[l].detach()), float(want[l]), bounds[name][l])
            _note(WORST, name, d, max(bounds[name][l], 1e-30))
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        got, want = grads[l].double().cpu() / scale, ref_grads[l]
        d = (got - want).abs()
        print(tag, l, "grad error", float(d.max()), "bound", bounds["grad"][l], "largest", float(want.abs().max()))
        if dtype == torch.float32:
            assert float(d.max()) <= bounds["grad"][l], (tag, l, float(d.max()), bounds["grad"][l])
            _note(WORST, "grad_f32", d.max(), max(bounds["grad"][l], 1e-30))
        else:
            bound = (F16_EPS * (want * scale).abs() + bounds["grad"][l] * scale + 2.0 ** -24) / scale
            assert bool((d <= bound).all()), (tag, l, float((d - bound).max()))
            _note(WORST, "grad_f16", (d / bound).max())
    assert abs(float(total.detach()) - float(per.detach().sum())) <= 1e-6 * abs(float(per.detach().sum()))


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

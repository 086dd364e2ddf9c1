"""The interpolator's SSIM + Charbonnier loss on the MI355X: image_loss_fwd_kernel / image_loss_fold_kernel /
image_loss_bwd_kernel behind qpwcnet_amd.loss.multiscale_image, both layouts, fp32 and fp16 predictions.

Oracle: ``loss.multiscale_image_torch`` on float64 CPU tensors fed the same values (the predictions lie on the fp16 grid);
tests/test_image_loss_cpu.py holds that chain to a numpy restatement within 1e-12.  Inputs: its make_case -- B = 2,
textured targets (a base level per image and channel plus uniform noise of amplitude 0.25, clamped to +-0.5; 0.02 for the
low-contrast case), predictions = the level's target + uniform noise of amplitude 0.05.

Bounds, per quantity the larger of 4 x |float32 torch chain - float64 torch chain| on the same case (the kernel sums in
another order; measured against the reference chain, never against the kernel) and 1e-5 of the reference's size -- the
value itself for losses and parts, the level's largest gradient for gradients; fp16 predictions add 2^-11 |g| + 2^-25 per
gradient element for the store's rounding.  test_report prints the float32 chain's own error (the floor) and the kernel's
worst error as a share of its bound; DESIGN.md section 4.29 records them.  Observed on an MI355X: the floor, worst case
of the module: total 8.4e-6 relative, dssim 1.2e-5, Charbonnier 1.2e-7, gradients 8.4e-5 of the level's largest (the
low-contrast case); the kernels' worst error over its bound: total 0.29, dssim 0.29, Charbonnier 0.008, fp32 gradients
0.31, fp16 gradients 0.94 (the half ulp of fp16 itself).

Shapes follow _hip.IMAGE_LOSS_TILE = (16, 32): 11 x 11 is one position; 26 x 42 exactly one full tile of positions;
27 x 43 spills one position row and column into second tiles; 17 x 33 has pixel tiles that own no position but receive
gradient from a neighbour's; 10 x 40 and 40 x 10 have one axis below the window; the six levels of 64 x 96 put three
levels below it and levels of different tile counts behind one prefix table."""
import pytest
import torch

from test_image_loss_cpu import make_case, to_layout

from qpwcnet_amd import _hip, loss, metrics, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16_EPS = 2.0 ** -11
TH, TW = _hip.IMAGE_LOSS_TILE
EDGES = {"one position": (11, 11), "one full tile": (TH + 10, TW + 10), "spill": (TH + 11, TW + 11),
         "tiles without positions": (TH + 1, TW + 1), "h below the window": (10, 40), "w below the window": (40, 10)}
WORST, FLOOR = {}, {}
_CASES, _ORACLES = {}, {}


def _note(book, key, value, bound=1.0):
    book[key] = max(book.get(key, 0.0), float(value) / bound)


def _case(key, *args, **kwargs):
    if key not in _CASES:
        _CASES[key] = make_case(*args, **kwargs)
    return _CASES[key]


def _chain(kwargs, y, preds, dtype):
    """The channels-first torch chain on the CPU in `dtype` -> (per, dssim, charbonnier, grads), everything float64."""
    obj = loss.ImageLoss(data_format="channels_first", **kwargs)
    xs = [torch.from_numpy(p).to(dtype).requires_grad_() for p in preds]
    total, per, parts = loss.multiscale_image_torch(obj, torch.from_numpy(y).to(dtype), xs)
    total.backward()
    return per.detach().double(), parts["dssim"].double(), parts["charbonnier"].double(), [x.grad.double() for x in xs]


def _oracle(key, kwargs, y, preds):
    """(float64 reference, per-quantity bounds) of the chain on these inputs, made once per key: bounds = max(4 x |float32
    chain - float64 chain|, 1e-5 of the reference's size)."""
    key = (key, tuple(sorted(kwargs.items())))
    if key not in _ORACLES:
        ref, ref32 = _chain(kwargs, y, preds, torch.float64), _chain(kwargs, y, preds, torch.float32)
        bounds = {"per": [], "dssim": [], "charbonnier": [], "grad": []}
        for l in range(len(preds)):
            for name, a, b in zip(("per", "dssim", "charbonnier"), ref[:3], ref32[:3]):
                err, size = abs(float(a[l]) - float(b[l])), abs(float(a[l]))
                bounds[name].append(max(4.0 * err, 1e-5 * size))
                _note(FLOOR, name, err / max(size, 1e-30))
            top = float(ref[3][l].abs().max())
            err = float((ref[3][l] - ref32[3][l]).abs().max())
            bounds["grad"].append(max(4.0 * err, 1e-5 * top))
            _note(FLOOR, "grad", err / max(top, 1e-30))
        _ORACLES[key] = ref + (bounds,)
    return _ORACLES[key]


def _device(kwargs, y, preds, data_format, f16=(), scale=1.0):
    """One forward + backward of scale * total on the device -> (total, per, parts, xs, channels-first gradients)."""
    obj = loss.ImageLoss(data_format=data_format, **kwargs)
    xs = [to_layout(p, data_format, torch.float16 if l in f16 else torch.float32).to(DEV).requires_grad_()
          for l, p in enumerate(preds)]
    total, per, parts = loss.multiscale_image(obj, to_layout(y, data_format).to(DEV), xs)
    (scale * total).backward()
    grads = [x.grad.permute(0, 3, 1, 2) if data_format == "channels_last" else x.grad for x in xs]
    return total.detach(), per.detach(), parts, xs, grads


def _compare(tag, y, preds, data_format, f16=(), **kwargs):
    """One forward + backward on the device against the oracle, every bound of the module."""
    ref_per, ref_dssim, ref_charb, ref_grads, bounds = _oracle(tag[0], kwargs, y, preds)
    total, per, parts, xs, grads = _device(kwargs, y, preds, data_format, f16)
    assert per.dtype == torch.float32 and per.device == xs[0].device and per.shape == (len(preds),)
    assert parts["dssim"].dtype == torch.float32 and parts["charbonnier"].dtype == torch.float32
    assert not parts["dssim"].requires_grad and not parts["charbonnier"].requires_grad
    for l, x in enumerate(xs):
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape and x.grad.is_contiguous()
        h, w = preds[l].shape[2:]
        if h < 11 or w < 11:
            assert float(parts["dssim"][l]) == 0.0 and float(ref_dssim[l]) == 0.0
        else:
            assert float(parts["dssim"][l]) > 0.0
        for name, got, want in (("per", per[l], ref_per[l]), ("dssim", parts["dssim"][l], ref_dssim[l]),
                                ("charbonnier", parts["charbonnier"][l], ref_charb[l])):
            d, bound = abs(float(got) - float(want)), bounds[name][l]
            print(tag, data_format, l, name, "error", d, "bound", bound, "value", float(want))
            assert d <= bound, (tag, l, name, float(got), float(want), bound)
            if bound > 0.0:
                _note(WORST, name, d, bound)
        ref = ref_grads[l]
        d = (grads[l].double().cpu() - ref).abs()
        print(tag, data_format, l, "grad error", float(d.max()), "bound", bounds["grad"][l], "largest", float(ref.abs().max()))
        if l in f16:
            bound = F16_EPS * ref.abs() + 2.0 ** -25 + bounds["grad"][l]
            assert bool((d <= bound).all()), (tag, l, float((d - bound).max()))
            _note(WORST, "grad_f16", (d / bound).max())
        else:
            assert float(d.max()) <= bounds["grad"][l], (tag, l, float(d.max()), bounds["grad"][l])
            _note(WORST, "grad_f32", d.max(), bounds["grad"][l])
        assert grads[l].any()
    assert abs(float(total) - float(per.sum())) <= 1e-6 * abs(float(per.sum()))
    return per, parts, grads


@pytest.mark.parametrize("f16", [(), (0, 2)], ids=["f32", "f16 at levels 0 and 2"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
def test_six_levels_match_the_float64_chain(data_format, f16):
    """64 x 96, 32 x 48, 16 x 24, 8 x 12, 4 x 6, 2 x 3 at C = 3 in one launch: 24, 8, 2, 2, 2, 2 tiles behind one prefix
    table, three levels with positions and three without."""
    y, preds = _case("six", 2, 3, 64, 96, seed=21, levels=6)
    assert [p.shape[2:] for p in preds] == [(64, 96), (32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]
    _compare(("six",), y, preds, data_format, f16)


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("edge", list(EDGES))
def test_tile_edges_match_the_float64_chain(edge, data_format):
    h, w = EDGES[edge]
    y, preds = _case(edge, 2, 3, h, w, seed=30 + list(EDGES).index(edge))
    _compare((edge,), y, preds, data_format)


@pytest.mark.parametrize("C", [1, 4])
def test_one_and_four_channels(C):
    y, preds = _case("C%d" % C, 2, C, 27, 45, seed=40 + C)
    _compare(("C%d" % C,), y, preds, "channels_first")
    _compare(("C%d" % C,), y, preds, "channels_first", f16=(0,))


def test_low_contrast_images():
    """Amplitude 0.02 at 24 x 40: sigma^2 of the window is of c2's order, D goes down to 1.5e-3 and the float32
    cancellation in conv(vt^2 + vp^2) - (mt^2 + mp^2) is the chain's own: its bound is what the float32 chain loses."""
    y, preds = _case("low contrast", 2, 3, 24, 40, seed=50, amp=0.02)
    _compare(("low contrast",), y, preds, "channels_last")
    _compare(("low contrast",), y, preds, "channels_first")


def test_dssim_is_the_quality_kernel_s_ssim():
    """One level at the truth's own size (the resize is the identity): parts['dssim'] against the merged
    quality_tile_kernel through metrics.image_quality, within 1e-6."""
    y, preds = _case("spill", 2, 3, TH + 11, TW + 11, seed=32)
    for data_format in ("channels_last", "channels_first"):
        t, p = to_layout(y, data_format).to(DEV), to_layout(preds[0], data_format).to(DEV)
        _, per, parts = loss.multiscale_image(loss.ImageLoss(data_format=data_format), t, [p])
        ssim = metrics.image_quality(t, p, offset=0.5, data_format=data_format).ssim
        want = (1.0 - float(ssim.double().mean())) / 2.0
        print(data_format, "dssim", float(parts["dssim"][0]), "from image_quality", want)
        assert abs(float(parts["dssim"][0]) - want) <= 1e-6 and want > 1e-3
        assert not per.requires_grad


@pytest.mark.parametrize("ssim_weight", [0.0, 1.0])
def test_one_part_alone(ssim_weight):
    """ssim_weight 0 and 1 against the one-part reference under the module's bounds; and the other part is exactly
    absent from the gradient: at weight 1 eps (the Charbonnier term's alone) changes no bit of it, at weight 0 max_val
    and offset (SSIM's alone) change none."""
    y, preds = _case("six", 2, 3, 64, 96, seed=21, levels=6)
    preds = preds[:3]                                      # the levels with positions: every gradient is nonzero
    per, parts, grads = _compare(("six[:3]",), y, preds, "channels_last", ssim_weight=ssim_weight)
    other = dict(eps=0.1) if ssim_weight == 1.0 else dict(max_val=3.0, offset=1.5)
    _, per2, parts2, _, grads2 = _device(dict(ssim_weight=ssim_weight, **other), y, preds, "channels_last")
    for l, (a, b) in enumerate(zip(grads, grads2)):
        assert torch.equal(a, b), (ssim_weight, l)
    if ssim_weight == 1.0:
        assert torch.equal(per, parts["dssim"]) and torch.equal(per, per2)
        assert not torch.equal(parts["charbonnier"], parts2["charbonnier"])
        # a level below the window has nothing left to differentiate
        _, per3, _, _, grads3 = _device(dict(ssim_weight=1.0), *_case("h below the window", 2, 3, 10, 40, seed=34),
                                        "channels_last")
        assert float(per3[0]) == 0.0 and not grads3[0].any()
    else:
        assert torch.equal(per, parts["charbonnier"]) and torch.equal(per, per2)
        assert not torch.equal(parts["dssim"], parts2["dssim"])


def test_two_calls_give_the_same_bits():
    y, preds = _case("six", 2, 3, 64, 96, seed=21, levels=6)
    a = _device({}, y, preds, "channels_last", f16=(1,))
    b = _device({}, y, preds, "channels_last", f16=(1,))
    assert torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert all(torch.equal(x, z) for x, z in zip(a[4], b[4]))


def test_the_incoming_gradient_scales_the_result():
    """(3 * total).backward() against 3 x the gradient of total.backward(): within 1 ulp of float32 per element."""
    y, preds = _case("six", 2, 3, 64, 96, seed=21, levels=6)
    one = _device({}, y, preds, "channels_first")[4]
    three = _device({}, y, preds, "channels_first", scale=3.0)[4]
    for l, (a, b) in enumerate(zip(one, three)):
        want = 3.0 * a.double()
        near = want.float().abs()
        ulp = (torch.nextafter(near, torch.full_like(near, float("inf"))) - near).double()
        assert bool(((b.double() - want).abs() <= ulp).all()), l
        assert not torch.equal(a, b)


def test_the_grad_path_refuses_stream_capture():
    y, preds = _case("one position", 2, 3, 11, 11, seed=30)
    obj = loss.ImageLoss(data_format="channels_first")
    t = to_layout(y, "channels_first").to(DEV)
    x = to_layout(preds[0], "channels_first").to(DEV).requires_grad_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.kernel_timing() as kt:
        with pytest.raises(RuntimeError, match="cannot be captured"):
            with torch.cuda.graph(graph):
                loss.multiscale_image(obj, t, [x])
        assert kt.records == []                    # refused before the targets' launch
    torch.cuda.synchronize()
    total, _, _ = loss.multiscale_image(obj, t, [x])     # and the eager path still works afterwards
    total.backward()
    assert bool(torch.isfinite(x.grad).all()) and x.grad.any()


def test_the_loss_takes_the_launches_the_docs_state():
    """One launch for the targets, one forward (+ its fold) and one backward for all six levels."""
    y, preds = _case("six", 2, 3, 64, 96, seed=21, levels=6)
    xs = [to_layout(p, "channels_last").to(DEV).requires_grad_() for p in preds]
    with ops.kernel_timing() as kt:
        total, _, _ = loss.multiscale_image(loss.ImageLoss(data_format="channels_last"), to_layout(y, "channels_last").to(DEV), xs)
        total.backward()
    assert [key[0] for key, _, _ in kt.records] == ["loss", "image_loss", "image_loss_bwd"]


def test_kernel_query():
    assert ops.image_loss_kernel(2, 3, [(64, 96), (2, 3)]) == "image_loss_fwd_kernel"
    assert ops.image_loss_kernel(2, 5, [(64, 96)]) == "" and ops.image_loss_kernel(2, 3, [(64, 0)]) == ""
    assert ops.image_loss_kernel(0, 3, [(64, 96)]) == "" and ops.image_loss_kernel(2, 3, [(8, 8)] * 9) == ""


def test_report():
    """The floor and the worst share of a bound, printed; run alone it makes one case first, so that it never prints
    empty books, and whatever was compared stayed inside its bound."""
    if not WORST:
        y, preds = _case("spill", 2, 3, TH + 11, TW + 11, seed=32)
        _compare(("spill",), y, preds, "channels_last")
    print("CPU float32 chain against float64 (the floor):", {k: "%.2e" % v for k, v in sorted(FLOOR.items())})
    print("worst observed / bound:", {k: "%.3f" % v for k, v in sorted(WORST.items())})
    assert {"per", "dssim", "charbonnier", "grad_f32"} <= set(WORST) and {"per", "dssim", "charbonnier", "grad"} <= set(FLOOR)
    assert all(0.0 <= v <= 1.0 for v in WORST.values()), WORST

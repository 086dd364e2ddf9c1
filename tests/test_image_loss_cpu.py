"""The interpolator's SSIM + Charbonnier loss without a device: ``loss.multiscale_image_torch`` (the chain CPU tensors take
and the oracle of tests/test_gpu_image_loss.py) against a numpy restatement of include/qpwc_image_loss.h, its autograd
gradient against central differences and against the header's closed form, the known answers, and the argument errors
of the Python surface.

The numpy oracle shares no step with the chain: the bilinear target by loops over the four corners, the window as the
direct 121-tap 2-D correlation with outer(g, g) (not the two separable passes), s and the Charbonnier term as written in
the header.  Both are float64, so they agree to rounding: 1e-12 relative.

make_case / make_levels are the inputs of the GPU tests as well: textured targets (a base level per image and channel
plus uniform noise of amplitude `amp`, clamped to +-0.5) and predictions = the level's target + uniform noise of amplitude
0.05, everything on the fp16 grid where asked so that an fp16 prediction holds the same numbers."""
import numpy as np
import pytest
import torch

from qpwcnet_amd import loss, metrics

EPS, Q = 1e-3, 0.5


def window():
    k = np.arange(11, dtype=np.float64) - 5.0
    e = np.exp(-k * k / 4.5)
    return (e / e.sum()).astype(np.float32).astype(np.float64)


def make_case(B, C, H, W, seed, levels=1, amp=0.25, noise=0.05):
    """y_true (B,C,H,W) float32 and `levels` predictions at (H >> k, W >> k), float32 on the fp16 grid, channels-first
    numpy arrays; the predictions are the chain's own float64 target of the level plus noise."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-0.3, 0.3, (B, C, 1, 1))
    y = np.clip(base + amp * rng.uniform(-1.0, 1.0, (B, C, H, W)), -0.5, 0.5).astype(np.float32)
    shapes = [(H >> k, W >> k) for k in range(levels)]
    targets = loss.resized_ground_truth_torch(torch.from_numpy(y).double(), shapes, "channels_first")
    preds = [(t.numpy() + noise * rng.uniform(-1.0, 1.0, t.shape)).astype(np.float16).astype(np.float32) for t in targets]
    return y, preds


def to_layout(x, data_format, dtype=torch.float32):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return t.permute(0, 2, 3, 1).contiguous() if data_format == "channels_last" else t


def np_resize(y, h, w):
    """tf.image.resize bilinear (half-pixel centres, no antialias) of (B,C,H,W) float64, the weights formed in float32
    with every product and sum separately rounded, as the kernel forms them."""
    H, W = y.shape[2:]

    def axis(n_out, n_in):
        scale = np.float32(n_in) / np.float32(n_out)
        out = []
        for o in range(n_out):
            f = max(np.float32(np.float32(scale * np.float32(o + 0.5)) - np.float32(0.5)), np.float32(0.0))
            i0 = int(np.floor(f))
            i1 = i0 + (1 if i0 < n_in - 1 else 0)
            l1 = np.float32(f - np.float32(i0))
            out.append((i0, i1, float(np.float32(1.0) - l1), float(l1)))
        return out

    out = np.zeros(y.shape[:2] + (h, w))
    for oy, (y0, y1, ly0, ly1) in enumerate(axis(h, H)):
        for ox, (x0, x1, lx0, lx1) in enumerate(axis(w, W)):
            out[:, :, oy, ox] = (ly0 * (lx0 * y[:, :, y0, x0] + lx1 * y[:, :, y0, x1])
                                 + ly1 * (lx0 * y[:, :, y1, x0] + lx1 * y[:, :, y1, x1]))
    return out


def np_ssim_parts(t, p, max_val=1.0, offset=0.5):
    """(s, Pa, Pb, Pc) of include/qpwc_image_loss.h for (B,C,h,w) float64 arrays, the window as 121 taps."""
    g = window()
    w2 = np.outer(g, g)
    conv = lambda x: np.einsum("bchwij,ij->bchw", np.lib.stride_tricks.sliding_window_view(x, (11, 11), axis=(2, 3)), w2)
    c1 = float(np.float32((0.01 * max_val) ** 2))
    c2 = float(np.float32((0.03 * max_val) ** 2))
    vt, vp = t + offset, p + offset
    mt, mp = conv(vt), conv(vp)
    A, Bd = 2 * mt * mp + c1, mt * mt + mp * mp + c1
    Cn, D = 2 * conv(vt * vp) - 2 * mt * mp + c2, conv(vt * vt + vp * vp) - (mt * mt + mp * mp) + c2
    lum, cs = A / Bd, Cn / D
    return lum * cs, 2 * (mt - lum * mp) / Bd * cs + lum * 2 * (cs * mp - mt) / D, -lum * cs / D, 2 * lum / D


def np_level(t, p, ssim_weight=0.85, q=Q, eps=EPS, max_val=1.0, offset=0.5):
    """(loss, dssim, charbonnier, gradient) of one level by the header's formulas."""
    h, w = t.shape[2:]
    d = p - t
    charb = ((d * d + eps * eps) ** q).mean()
    grad = (1 - ssim_weight) / d.size * 2 * q * d * (d * d + eps * eps) ** (q - 1)
    dssim = 0.0
    if h >= 11 and w >= 11:
        s, pa, pb, pc = np_ssim_parts(t, p, max_val, offset)
        dssim = (1 - s.mean()) / 2
        g = window()
        full = lambda x: sum(np.pad(x, ((0, 0), (0, 0), (i, 10 - i), (j, 10 - j))) * g[i] * g[j]
                             for i in range(11) for j in range(11))          # T(r) = sum_j g(r - j) P(j)
        grad = grad - ssim_weight / (2 * s.size) * (full(pa) + 2 * (p + offset) * full(pb) + (t + offset) * full(pc))
    return ssim_weight * dssim + (1 - ssim_weight) * charb, dssim, charb, grad


def chain(obj, y, preds, dtype=torch.float64):
    xs = [torch.from_numpy(p).to(dtype).requires_grad_() for p in preds]
    total, per, parts = loss.multiscale_image_torch(obj, torch.from_numpy(y).to(dtype), xs)
    total.backward()
    return total.detach(), per.detach(), parts, [x.grad for x in xs]


@pytest.mark.parametrize("shape,levels", [((2, 3, 24, 40), 2), ((1, 1, 11, 11), 1), ((2, 4, 27, 45), 1), ((1, 2, 22, 30), 2)])
def test_chain_matches_the_numpy_restatement(shape, levels):
    y, preds = make_case(*shape, seed=3, levels=levels)
    obj = loss.ImageLoss(data_format="channels_first")
    total, per, parts, grads = chain(obj, y, preds)
    for l, p in enumerate(preds):
        t = np_resize(y.astype(np.float64), *p.shape[2:])
        want, dssim, charb, grad = np_level(t, p.astype(np.float64))
        for got, ref in ((per[l], want), (parts["dssim"][l], dssim), (parts["charbonnier"][l], charb)):
            assert abs(float(got) - ref) <= 1e-12 * abs(ref), (shape, l, float(got), ref)
        assert np.abs(grads[l].numpy() - grad).max() <= 1e-12 * np.abs(grad).max(), (shape, l)
    assert float(total) == pytest.approx(float(per.sum()), rel=1e-15)
    assert per.dtype == torch.float64 and parts["dssim"].dtype == torch.float64


def test_both_layouts_give_the_same_numbers():
    y, preds = make_case(2, 3, 24, 40, seed=4, levels=2)
    first = chain(loss.ImageLoss(data_format="channels_first"), y, preds)
    last = chain(loss.ImageLoss(data_format="channels_last"), np.ascontiguousarray(y.transpose(0, 2, 3, 1)),
                 [np.ascontiguousarray(p.transpose(0, 2, 3, 1)) for p in preds])
    assert torch.allclose(first[1], last[1], rtol=1e-13, atol=0)
    for a, b in zip(first[3], last[3]):
        assert b.shape == (2,) + a.shape[2:] + (3,) and torch.allclose(a, b.permute(0, 3, 1, 2), rtol=1e-11, atol=1e-18)


def test_autograd_gradient_against_central_differences():
    """1 x 2 x 13 x 14, float64, step 1e-6.  The truncation error of a central difference is step^2 / 6 times the third
    derivative; the Charbonnier term's is at most 3 / eps^2 = 3e6 at q = 0.5, so 5e-7 of its first derivative's scale
    (1), and SSIM's is far smaller; the rounding error is 2^-52 * loss / step = 1e-12 of a gradient of 1e-4.  Bound: 1e-5
    of the largest gradient."""
    y, preds = make_case(1, 2, 13, 14, seed=5)
    obj = loss.ImageLoss(data_format="channels_first")
    _, _, _, grads = chain(obj, y, preds)
    yt, p = torch.from_numpy(y).double(), torch.from_numpy(preds[0]).double()
    f = lambda x: float(loss.multiscale_image_torch(obj, yt, [x])[0])
    step, fd = 1e-6, torch.zeros_like(p)
    flat, out = p.view(-1), fd.view(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + step
        up = f(p)
        flat[i] = keep - step
        down = f(p)
        flat[i] = keep
        out[i] = (up - down) / (2 * step)
    assert float((fd - grads[0]).abs().max()) <= 1e-5 * float(grads[0].abs().max())
    assert float(grads[0].abs().min()) > 0.0


def test_dssim_is_the_metric_s_ssim():
    y, preds = make_case(2, 3, 24, 40, seed=6)
    _, _, parts, _ = chain(loss.ImageLoss(data_format="channels_first"), y, preds, torch.float32)
    ssim = metrics.image_quality_torch(torch.from_numpy(y), torch.from_numpy(preds[0]), offset=(0.5, 0.5),
                                       data_format="channels_first").ssim
    assert abs(float(parts["dssim"][0]) - (1.0 - float(ssim.double().mean())) / 2.0) <= 1e-6
    assert 0.0 < float(parts["dssim"][0]) < 0.5


@pytest.mark.parametrize("q,eps", [(0.5, 1e-3), (0.4, 0.01)])
def test_equal_images_have_the_known_answer(q, eps):
    y, _ = make_case(2, 3, 24, 40, seed=7)
    obj = loss.ImageLoss(q=q, eps=eps, data_format="channels_first")
    _, per, parts, grads = chain(obj, y, [y])
    assert abs(float(parts["dssim"][0])) <= 1e-7
    assert float(parts["charbonnier"][0]) == pytest.approx(eps ** (2 * q), rel=1e-12)
    assert float(per[0]) == pytest.approx(0.15 * eps ** (2 * q), rel=1e-6, abs=1e-7)
    assert float(grads[0].abs().max()) <= 1e-12          # a minimum of both parts


def test_a_level_below_the_window_is_charbonnier_only():
    y, preds = make_case(2, 3, 10, 16, seed=8)
    obj = loss.ImageLoss(data_format="channels_first")
    _, per, parts, grads = chain(obj, y, preds)
    assert float(parts["dssim"][0]) == 0.0
    d = preds[0].astype(np.float64) - y
    want = 0.15 / d.size * 2 * Q * d * (d * d + EPS * EPS) ** (Q - 1)
    assert np.abs(grads[0].numpy() - want).max() <= 1e-14 * np.abs(want).max()
    assert float(per[0]) == pytest.approx(0.15 * float(parts["charbonnier"][0]), rel=1e-14)
    for shape in ((2, 3, 16, 10), (1, 1, 1, 1)):                       # the other axis; a single pixel
        y2, p2 = make_case(*shape, seed=9)
        assert float(chain(obj, y2, p2)[2]["dssim"][0]) == 0.0


def test_the_single_position_spreads_its_gradient_by_the_window():
    """11 x 11, C = 1, ssim_weight = 1: d loss / d p(r) = -1 / (2 N) * g(r_y) g(r_x) * (Pa + 2 vp(r) Pb + vt(r) Pc) with
    the one position's Pa, Pb, Pc and N = B."""
    y, preds = make_case(2, 1, 11, 11, seed=10)
    obj = loss.ImageLoss(ssim_weight=1.0, data_format="channels_first")
    _, per, parts, grads = chain(obj, y, preds)
    t, p = y.astype(np.float64), preds[0].astype(np.float64)
    s, pa, pb, pc = np_ssim_parts(t, p)
    assert s.shape == (2, 1, 1, 1)
    # the taps run backwards from the pixel to the position: g(r - j) with j = 0 is g[r], and g is symmetric
    g2 = np.outer(window(), window())[None, None]
    want = -1.0 / (2 * 2) * g2 * (pa + 2 * (p + 0.5) * pb + (t + 0.5) * pc)
    assert np.abs(grads[0].numpy() - want).max() <= 1e-12 * np.abs(want).max()
    assert float(per[0]) == pytest.approx((1 - s.mean()) / 2, rel=1e-12)
    assert float(parts["charbonnier"][0]) > 0.0                        # reported although its weight is 0


def test_config_round_trip_and_one_level_call():
    obj = loss.ImageLoss(ssim_weight=0.5, q=0.4, eps=0.01, max_val=2.0, offset=1.0, data_format="channels_first", name="x")
    cfg = obj.get_config()
    assert cfg == {"name": "x", "ssim_weight": 0.5, "q": 0.4, "eps": 0.01, "max_val": 2.0, "offset": 1.0,
                   "data_format": "channels_first"}
    assert loss.ImageLoss.from_config(cfg).get_config() == cfg
    from qpwcnet_amd.backend import image_data_format
    assert loss.ImageLoss().data_format == image_data_format() and loss.ImageLoss().ssim_weight == 0.85
    y, preds = make_case(1, 3, 12, 13, seed=11)
    single = loss.ImageLoss(data_format="channels_first")(torch.from_numpy(y), torch.from_numpy(preds[0]))
    assert single.dim() == 0 and single.dtype == torch.float32 and float(single) > 0.0
    assert float(single) == float(loss.ImageLoss(data_format="channels_first").call(torch.from_numpy(y),
                                                                                    torch.from_numpy(preds[0])))


def test_argument_errors():
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ssim_weight"):
            loss.ImageLoss(ssim_weight=bad)
    for bad in (dict(q=0.0), dict(eps=0.0), dict(eps=-1.0), dict(max_val=0.0), dict(max_val=float("inf")),
                dict(offset=float("nan"))):
        with pytest.raises(ValueError):
            loss.ImageLoss(**bad)
    with pytest.raises(ValueError, match="data format"):
        loss.ImageLoss(data_format="nhwc")
    obj = loss.ImageLoss(data_format="channels_first")
    y, p = torch.zeros(2, 3, 12, 16), torch.zeros(2, 3, 12, 16)
    with pytest.raises(ValueError, match="1..4 channels"):
        loss.multiscale_image(obj, torch.zeros(2, 5, 12, 16), [torch.zeros(2, 5, 12, 16)])
    with pytest.raises(ValueError, match="requires grad"):
        loss.multiscale_image(obj, y.clone().requires_grad_(), [p])
    with pytest.raises(ValueError, match="is on"):
        loss.multiscale_image(obj, y, [p.to("meta")])
    with pytest.raises(ValueError, match="channels"):
        loss.multiscale_image(obj, y, [torch.zeros(2, 2, 12, 16)])
    with pytest.raises(ValueError, match="batch"):
        loss.multiscale_image(obj, y, [torch.zeros(1, 3, 12, 16)])
    with pytest.raises(ValueError, match="1..8"):
        loss.multiscale_image(obj, y, [p] * 9)
    with pytest.raises(ValueError, match="1..8"):
        loss.multiscale_image(obj, y, [])
    with pytest.raises(TypeError):
        loss.multiscale_image(loss.AutoResizeMseLoss(), y, [p])
    with pytest.raises(TypeError):
        loss.multiscale_image(obj, y.numpy(), [p])
    with torch.no_grad():                                             # nothing would be differentiated
        assert loss.multiscale_image(obj, y.clone().requires_grad_(), [p])[1].shape == (1,)

"""GPU suite of the trainable frame interpolator: the image head (qpwc_image_head_fwd / _bwd), the x2 upsampling of an
image (qpwc_upsample2x_image_fwd / _bwd) and the frame pyramid (qpwc_avgpool_pyramid_fwd) behind ops.image_head,
ops.upsample2x_image and ops.avgpool_pyramid, and layers.FrameInterpolate / layers.InterpolatorModel on top of them.

Oracle: torch autograd in float64 on the CPU of the composed op, fed the same values.  Inputs and grad_out are multiples
of 1/16 in [-1, 1], weights multiples of 1/64 in [-1/8, 1/8], biases multiples of 1/8.  Tolerance: the project's
1e-4 * max(1, max|ref|) per tensor (tests/test_gpu_autograd.py::_tol)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import net_ref, torch_ref
from qpwcnet_amd import _hip, layers, loss, ops, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_conv_grad import encoder_composite  # noqa: E402
from test_gpu_flow_head_grad import optflow_composite, upsample_composite  # noqa: E402
from test_gpu_upconv_grad import decoder_composite  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (B, H, W) at which the grid-stride loops of the image head kernels, of both upsampling kernels and the lane loop of
# conv_bwd_reduce_kernel make more than one trip with an uneven last one (tests/test_interp_grad_cpu.py checks this
# against the constants of csrc/interp.hip)
MULTI_TRIP = (2, 181, 183)
# the 5-step training case: fp32-vs-float64 drift of the CPU composite and the bound derived from it (see the test)
TRAIN_DRIFT = 1.7e-7
TRAIN_RATES = (0.1, 0.01, 0.02)  # encoder and decoder, flow estimators, interpolation blocks
TRAIN_BOUND = 10 * TRAIN_DRIFT


def _grid(gen, shape, step, lim=1.0):
    n = int(round(lim / step))
    return torch.randint(-n, n + 1, shape, generator=gen).to(torch.float64) * step


def _tol(ref):
    return 1e-4 * max(1.0, float(ref.abs().max()))


def _check(got, ref, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    d = float((got - ref).abs().max())
    print("{}: max|d| = {:.3e}, bound {:.3e}".format(what, d, _tol(ref)))
    assert d <= _tol(ref), "{}: max|d| = {:.3e} > {:.3e}".format(what, d, _tol(ref))


def _dev(t):
    return t.float().to(DEV)


# ---- the composed ops -----------------------------------------------------------------------------------------------------
def head_composite(z, w2, b2):
    """Conv2D(3, 1x1) on channels-last features: z (B,H,W,64), w2 (3,64[,1,1]), b2 (3) -> (B,H,W,3)."""
    return z @ w2.reshape(3, -1).t() + b2


def pyramid_composite(x, levels):
    for _ in range(levels):
        x = net_ref.RefInterpolator.downsample(x)
    return x


def frame_interpolate_composite(P, prefix, prv, nxt, flo_01, flo_10, img_u=None):
    """layers.FrameInterpolate from a {name: tensor} dict as torch ops on the CPU."""
    nxt_w = torch_ref.warp_v2(nxt, 0.5 * flo_01)
    prv_w = torch_ref.warp_v2(prv, 0.5 * flo_10)
    x = torch.cat([prv_w, nxt_w, flo_01, flo_10] + ([] if img_u is None else [img_u]), dim=3).permute(0, 3, 1, 2)
    dw = P[prefix + "conv1.depthwise.weight"]
    x = F.conv2d(x, dw, None, padding=1, groups=dw.shape[0])
    x = torch_ref.mish(F.conv2d(x, P[prefix + "conv1.pointwise.weight"], P[prefix + "conv1.bias"]))
    return head_composite(x.permute(0, 2, 3, 1), P[prefix + "conv2.weight"], P[prefix + "conv2.bias"])


def interpolator_composite(P, pairs, n_enc, n_dec, training=True):
    """layers.InterpolatorModel from a {name: tensor} dict as torch ops on the CPU -> its list of images.  The flow
    stack runs twice, flows_01 first: optflow_composite replaces the moving buffers in P at every call."""
    n = pairs.shape[0]
    img_prv, img_nxt = pairs[..., :3], pairs[..., 3:]
    feats = encoder_composite(P, [img_prv, img_nxt], n_enc)
    decs = decoder_composite(P, feats, n_dec)
    enc_prv, enc_nxt = feats[-1][:n], feats[-1][n:]
    decs_prv, decs_nxt = [d[:n] for d in decs], [d[n:] for d in decs]

    def flow_stack(ep, en, dp, dn):
        flo = optflow_composite(P, "flow.flow.", (torch_ref.cost_volume(ep, en, 4), ep, en), training)
        flows = [flo]
        for i in range(n_dec):
            up = upsample_composite(flo, 2.0)
            cost = torch_ref.cost_volume(dp[i], torch_ref.warp_v2(dn[i], up), 4)
            flo = optflow_composite(P, "upflow.%d.flow." % i, (cost, dp[i], up), training)
            flows.append(flo)
        return flows

    flows_01 = flow_stack(enc_nxt, enc_prv, decs_nxt, decs_prv)
    flows_10 = flow_stack(enc_prv, enc_nxt, decs_prv, decs_nxt)
    img = frame_interpolate_composite(P, "img.0.", pyramid_composite(img_prv, n_enc), pyramid_composite(img_nxt, n_enc),
                                      flows_01[0], flows_10[0])
    imgs = [img]
    for i in range(n_dec):
        img = frame_interpolate_composite(P, "img.%d." % (i + 1), decs_prv[i], decs_nxt[i], flows_01[i + 1],
                                          flows_10[i + 1], upsample_composite(img, 1.0))
        imgs.append(img)
    imgs.append(upsample_composite(img, 1.0))
    return imgs


def autoresize_mse_composite(y_true, pred):
    """AutoResizeMseLoss of one level (tests/test_loss_cpu.py::torch_ops_loss, 'autoresize') in the operands' dtype."""
    g = F.interpolate(y_true.permute(0, 3, 1, 2), size=pred.shape[1:3], mode="bilinear", align_corners=False)
    return F.mse_loss(pred.permute(0, 3, 1, 2), g)


# ---- image head -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_case(B, H, W, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (_grid(gen, (B, H, W, 64), 1 / 16), _grid(gen, (3, 64, 1, 1), 1 / 64, 1 / 8), _grid(gen, (3,), 1 / 8),
            _grid(gen, (B, H, W, 3), 1 / 16))


@functools.lru_cache(maxsize=None)
def _head_oracle(key):
    z, w2, b2, g = _head_case(*key)
    leaves = [t.clone().requires_grad_() for t in (z, w2, b2)]
    out = head_composite(*leaves)
    out.backward(g)
    return (out.detach(),) + tuple(t.grad for t in leaves)


def _head_hip(case):
    z, w2, b2 = [_dev(t).requires_grad_() for t in case[:3]]
    out = ops.image_head(z, w2, b2)
    out.backward(_dev(case[3]))
    return out, z.grad, w2.grad, b2.grad


@pytest.mark.parametrize("key", [(1, 1, 1), (1, 3, 5), (2, 7, 9), MULTI_TRIP], ids=["1x1", "3x5", "2x7x9", "multi_trip"])
def test_image_head_forward_and_gradients(key):
    for a, r, name in zip(_head_hip(_head_case(*key)), _head_oracle(key), ("out", "grad_z", "grad_w2", "grad_b2")):
        _check(a, r, name)


def test_image_head_only_what_is_asked_determinism_and_independence():
    z, w2, b2, g = [_dev(t) for t in _head_case(2, 7, 9)]
    r1 = ops.image_head_bwd(z, w2, g)
    r2 = ops.image_head_bwd(z, w2, g)
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)
    assert torch.equal(ops.image_head(z, w2, b2), ops.image_head(z, w2, b2))
    for bits in range(1, 8):                                             # every need combination
        need = tuple(bool(bits >> i & 1) for i in range(3))
        some = ops.image_head_bwd(z, w2, g, need=need)
        assert [t is None for t in some] == [not n for n in need], need
        for k in range(3):
            assert not need[k] or torch.equal(some[k], r1[k]), (need, k)
    for k in range(3):                                                   # through autograd, asked for alone
        leaves = [t.clone().requires_grad_(i == k) for i, t in enumerate((z, w2, b2))]
        ops.image_head(*leaves).backward(g)
        assert torch.equal(leaves[k].grad, r1[k].reshape(leaves[k].shape)), k
        assert all(t.grad is None for i, t in enumerate(leaves) if i != k)
    # grad_z of image 0 does not change when image 1 does
    z2, g2 = z.clone(), g.clone()
    z2[1], g2[1] = z2[1] * 0.5 + 0.25, -g2[1]
    assert torch.equal(ops.image_head_bwd(z2, w2, g2, need=(True, False, False))[0][0], r1[0][0])
    # the forward with grad is the no-grad forward
    plain = ops.image_head(z, w2, b2)
    out = ops.image_head(z.clone().requires_grad_(), w2, b2)
    assert plain.grad_fn is None and out.grad_fn is not None and torch.equal(out.detach(), plain)
    with torch.no_grad():
        quiet = ops.image_head(z.clone().requires_grad_(), w2, b2)
    assert quiet.grad_fn is None and torch.equal(quiet, plain)


# ---- x2 upsampling of an image --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _up_case(B, h, w, C, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return _grid(gen, (B, h, w, C), 1 / 16), _grid(gen, (B, 2 * h, 2 * w, C), 1 / 16)


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("bhw", [(1, 1, 1), (1, 2, 3), (2, 5, 7), MULTI_TRIP], ids=["1x1", "2x3", "2x5x7", "multi_trip"])
def test_upsample_image_is_exact_on_the_grid(bhw, C, scale):
    """Multiples of 1/16 times 9/16, 3/16 and 1/16 (forward) and times 1/4 and 3/4 twice over (backward) are fp32
    values, and so is every partial sum: the float64 composite is met bit for bit."""
    x, g = _up_case(*bhw, C)
    leaf = x.clone().requires_grad_()
    ref = upsample_composite(leaf, scale)
    ref.backward(g)
    hx = _dev(x).requires_grad_()
    out = ops.upsample2x_image(hx, scale)
    out.backward(_dev(g))
    assert out.shape == ref.shape and torch.equal(out.detach().double().cpu(), ref.detach())
    assert torch.equal(hx.grad.double().cpu(), leaf.grad)
    assert torch.equal(ops.upsample2x_image_bwd(_dev(g), scale), hx.grad)
    plain = ops.upsample2x_image(_dev(x), scale)
    assert plain.grad_fn is None and torch.equal(plain, out.detach())


@pytest.mark.parametrize("bhw", [(1, 1, 1), (2, 5, 7), (1, 33, 18)])
def test_upsample_image_of_two_channels_has_the_bits_of_the_flow_kernel(bhw):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(bhw + (2,), generator=gen).to(DEV) * 5
    for scale in (1.0, 2.0, 0.3):
        assert torch.equal(ops.upsample2x_image(x, scale), ops.upsample2x_flow(x, scale))
    g = torch.randn((bhw[0], 2 * bhw[1], 2 * bhw[2], 2), generator=gen).to(DEV)
    assert torch.equal(ops.upsample2x_image_bwd(g, 2.0), ops.upsample2x_flow_bwd(g, 2.0))
    x4 = torch.randn(bhw + (4,), generator=gen).to(DEV)
    _check(ops.upsample2x_image(x4, 1.0), upsample_composite(x4.double().cpu(), 1.0), "4 channels")


# ---- the frame pyramid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 5])
@pytest.mark.parametrize("shape", [(2, 32, 64, 3), (1, 64, 32, 3)])
def test_pyramid(shape, levels):
    """On the 1/16 grid `levels` levels need 4 + 2 levels fractional bits, 14 at most: every mean is an fp32 value and
    the float64 chain is met bit for bit.  On randn inputs the project tolerance."""
    gen = torch.Generator().manual_seed(levels)
    x = _grid(gen, shape, 1 / 16)
    out = ops.avgpool_pyramid(_dev(x), levels)
    assert out.shape == (shape[0], shape[1] >> levels, shape[2] >> levels, 3)
    assert torch.equal(out.double().cpu(), pyramid_composite(x, levels))
    r = torch.randn(shape, generator=gen, dtype=torch.float64)
    _check(ops.avgpool_pyramid(_dev(r), levels), pyramid_composite(r.float().double(), levels), "randn")


def test_pyramid_other_channel_counts_and_wide_tiles():
    gen = torch.Generator().manual_seed(9)
    for shape, levels in (((1, 8, 8, 1), 3), ((2, 16, 24, 2), 3), ((1, 4, 4100, 4), 2), ((1, 64, 192, 3), 6),
                          ((1, 2, 4098, 3), 1)):
        x = _grid(gen, shape, 1 / 16)
        assert torch.equal(ops.avgpool_pyramid(_dev(x), levels).double().cpu(), pyramid_composite(x, levels)), shape


@pytest.mark.parametrize("shape,levels", [((2, 33, 64, 3), 1), ((1, 20, 40, 3), 3), ((1, 30, 50, 3), 5)])
def test_pyramid_falls_back_where_a_window_is_clipped(shape, levels):
    x = _dev(_grid(torch.Generator().manual_seed(4), shape, 1 / 16))
    B, H, W, C = shape
    out = torch.empty((B, -(-H >> levels), -(-W >> levels), C), device=DEV)
    rc = _hip.lib().qpwc_avgpool_pyramid_fwd(x.data_ptr(), out.data_ptr(), B, H, W, C, levels, None)
    assert rc == _hip.E_SHAPE and b"multiples" in _hip.lib().qpwc_last_error()
    got = ops.avgpool_pyramid(x, levels)
    assert got.shape == out.shape
    _check(got, pyramid_composite(x.double().cpu(), levels), "composed pooling")


# ---- FrameInterpolate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,shape", [(0, (2, 8, 16, 3)), (2, (2, 16, 32, 128))])
def test_frame_interpolate_block(k, shape):
    """One block with the weights of synth.make_interpolator_weights and flows that cross the borders, as
    tests/test_gpu_interpolator.py::test_frame_interpolate_block: forward, the gradient of every parameter and of every
    input, the stacked form and the no-grad forward."""
    weights = synth.make_interpolator_weights(42, (64, 128))
    rng = np.random.default_rng(k)
    B, H, W, C = shape
    arrays = [rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32),
              (rng.standard_normal((B, H, W, 2)) * 6).astype(np.float32),
              (rng.standard_normal((B, H, W, 2)) * 6).astype(np.float32),
              rng.standard_normal((B, H, W, 3)).astype(np.float32)][:5 if k > 0 else 4]
    g = _grid(torch.Generator().manual_seed(k), (B, H, W, 3), 1 / 16)
    prefix = "img.{}.".format(k)
    ref_net = net_ref.RefInterpolator(weights, dtype=torch.float64)
    names = [n for n in ref_net.w if n.startswith(prefix)]
    for n in names:
        ref_net.w[n].requires_grad_()
    leaves = [torch.from_numpy(a).double().requires_grad_() for a in arrays]
    ref = ref_net.frame_interpolate(k, *leaves)
    ref.backward(g)

    blk = layers.FrameInterpolate(C, up=k > 0, data_format="channels_last")
    res = blk.load_state_dict({n[len(prefix):]: torch.as_tensor(weights[n]) for n in names})
    assert not res.missing_keys and not res.unexpected_keys and len(names) == 5
    blk = blk.to(DEV)
    hx = [torch.from_numpy(a).to(DEV).requires_grad_() for a in arrays]
    out = blk(tuple(hx))
    assert out.grad_fn is not None
    out.backward(_dev(g))
    _check(out, ref.detach(), "out")
    for n, p in blk.named_parameters():
        _check(p.grad, ref_net.w[prefix + n].grad, "grad " + n)
    for a, r, name in zip(hx, leaves, ("prv", "nxt", "flo_01", "flo_10", "img_u")):
        _check(a.grad, r.grad, "grad " + name)
    # the stacked form and the no-grad forward: the same bits
    quiet = [t.detach() for t in hx]
    stacked = blk.forward_stacked(torch.cat([quiet[1], quiet[0]]), torch.cat([quiet[2], quiet[3]]), *quiet[4:])
    assert torch.equal(stacked, out.detach())
    with torch.no_grad():
        plain = blk(tuple(hx))
    assert plain.grad_fn is None and torch.equal(plain, out.detach())
    # channels_first at the boundary
    cf = layers.FrameInterpolate(C, up=k > 0, data_format="channels_first").to(DEV)
    cf.load_state_dict(blk.state_dict())
    assert torch.equal(cf(tuple(t.permute(0, 3, 1, 2) for t in quiet)).permute(0, 2, 3, 1), plain)


# ---- the whole interpolator -------------------------------------------------------------------------------------------------
def test_interpolator_model_matches_the_no_grad_network_and_trains():
    from qpwcnet_amd.pwcnet import build_interpolator
    hw = (64, 96)
    weights = synth.make_interpolator_weights(42, hw)
    state = {k: torch.as_tensor(v) for k, v in weights.items()}
    net = layers.InterpolatorModel(data_format="channels_last")
    res = net.load_state_dict(state)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV).eval()
    pairs_np, _ = synth.make_frames(2, hw[0], hw[1], seed=5)
    pairs = torch.as_tensor(pairs_np).to(DEV)
    with torch.no_grad():
        want = build_interpolator(hw, "channels_last", weights=weights, device=DEV, batch_directions=False)(pairs)
    ref = net_ref.RefInterpolator(weights)(pairs_np)
    imgs = net(pairs)
    assert len(imgs) == len(want) == len(ref) == 6 and imgs[-1].shape == (2, 64, 96, 3) and imgs[0].shape == (2, 2, 3, 3)
    assert imgs[0].grad_fn is not None
    for i, (a, w, r) in enumerate(zip(imgs, want, ref)):
        _check(a, w.detach().double().cpu(), "image %d against build_interpolator" % i)
        _check(a, r.double(), "image %d against RefInterpolator" % i)
    with torch.no_grad():
        quiet = net(pairs)
    assert all(q.grad_fn is None and torch.equal(q, a.detach()) for q, a in zip(quiet, imgs))
    last = layers.InterpolatorModel(output_multiscale=False, data_format="channels_last").to(DEV).eval()
    last.load_state_dict(net.state_dict())
    with torch.no_grad():
        assert torch.equal(last(pairs), quiet[-1])
    # channels_first input and output
    cf = layers.InterpolatorModel(data_format="channels_first").to(DEV).eval()
    cf.load_state_dict(net.state_dict())
    with torch.no_grad():
        for a, c in zip(quiet, cf(pairs.permute(0, 3, 1, 2).contiguous())):
            assert torch.equal(c.permute(0, 2, 3, 1), a)
    # train(): every parameter gets a gradient, every OptFlow's moving statistics move twice
    P = {k: v.detach().double().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        interpolator_composite(P, pairs.double().cpu(), 5, 4, training=True)
    net.train()
    middle = torch.rand(2, 64, 96, 3, generator=torch.Generator().manual_seed(2)).to(DEV) - 0.5
    total = loss.multiscale(loss.AutoResizeMseLoss(), middle, net(pairs))[0]
    total.backward()
    assert bool(torch.isfinite(total))
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, n
    for n, b in net.named_buffers():
        assert n.endswith(("norm.mean", "norm.var")), n
        _check(b, P[n], "twice-updated " + n)
        assert not torch.equal(b.cpu(), state[n]), n


# ---- a short training run -------------------------------------------------------------------------------------------------
def train_case():
    """Fixed-seed InterpolatorModel((16, 32, 64), (32,)): Encoder, Decoder, Flow(64), one UpFlow(64), FrameInterpolate(3)
    and FrameInterpolate(64, up); a 32 x 48 pair, a random middle frame and the learning rates (encoder and decoder,
    flow estimators, interpolation blocks).  Kernels and biases as in tests/test_gpu_upconv_grad.py::train_case: the
    kernels that feed a Mish carry synth.KERNEL_GAIN and the biases are small random numbers, which keeps features and
    flows O(1)."""
    torch.manual_seed(0)
    net = layers.InterpolatorModel((16, 32, 64), (32,), data_format="channels_last")
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=gen) - 0.5) * 0.1)
            elif n.endswith("weight") and not n.endswith(("flow.flow.weight", "conv2.weight")):
                p.mul_(synth.KERNEL_GAIN)
    pairs = torch.rand(2, 32, 48, 6, generator=gen) - 0.5
    middle = torch.rand(2, 32, 48, 3, generator=gen) - 0.5
    return net, pairs, middle, TRAIN_RATES


def _rate(name, lr):
    return lr[0] if name.startswith(("enc.", "dec.")) else lr[2] if name.startswith("img.") else lr[1]


def train_composite(dtype, steps=5):
    """The SGD steps of pair -> InterpolatorModel -> AutoResizeMseLoss over all its images on the torch composite in
    `dtype` on the CPU -> ({name: final parameter}, losses)."""
    net, pairs, middle, lr = train_case()
    P = {k: v.detach().to(dtype).clone() for k, v in net.state_dict().items()}
    names = [n for n, _ in net.named_parameters()]
    for n in names:
        P[n].requires_grad_()
    pairs, middle = pairs.to(dtype), middle.to(dtype)
    losses = []
    for _ in range(steps):
        imgs = interpolator_composite(P, pairs, 3, 1)
        total = sum(autoresize_mse_composite(middle, i) for i in imgs)
        losses.append(float(total.detach()))
        grads = torch.autograd.grad(total, [P[n] for n in names])
        with torch.no_grad():
            for n, gr in zip(names, grads):
                P[n] -= _rate(n, lr) * gr
            for n in P:                                  # the moving buffers carry no history into the next step
                if n not in names:
                    P[n] = P[n].detach()
    return {n: P[n].detach() for n in names}, losses


def test_short_training_run():
    """5 SGD steps of a pair -> InterpolatorModel((16, 32, 64), (32,)) -> multiscale AutoResizeMseLoss over all three
    images in training mode on the HIP layers against the same steps of the float64 composite.  Measured on the CPU
    for exactly this case: the fp32 composite ends within TRAIN_DRIFT (max over all parameters) of the float64 one
    (tests/test_interp_grad_cpu.py re-measures it); the bound is 10 x that (TRAIN_BOUND), the margin for fp32 sums in
    another order across 5 compounding steps, as in tests/test_gpu_upconv_grad.py."""
    ref, losses = train_composite(torch.float64)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses            # the case really trains
    net, pairs, middle, lr = train_case()
    start = {n: p.detach().double().clone() for n, p in net.named_parameters()}
    net = net.to(DEV).train()
    pairs, middle = pairs.to(DEV), middle.to(DEV)
    groups = [{"params": [p for n, p in net.named_parameters() if _rate(n, (0, 1, 2)) == k], "lr": lr[k]}
              for k in range(3)]
    opt = torch.optim.SGD(groups)
    seen = []
    for _ in range(5):
        opt.zero_grad()
        total = loss.multiscale(loss.AutoResizeMseLoss(), middle, net(pairs))[0]
        seen.append(float(total.detach()))
        total.backward()
        opt.step()
    print("losses {} (float64 composite {})".format(seen, losses))
    assert all(b < a for a, b in zip(seen, seen[1:])), seen
    got = dict(net.named_parameters())
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0.0 for p in got.values())
    worst = max(float((got[n].detach().double().cpu() - r).abs().max()) for n, r in ref.items())
    moved = min(float((got[n].detach().double().cpu() - start[n]).abs().max()) for n in ref)
    print("final-parameter drift {:.3e}, bound {:.3e}; least-moved parameter {:.3e}".format(worst, TRAIN_BOUND, moved))
    assert moved > 10 * TRAIN_BOUND, moved
    assert worst <= TRAIN_BOUND, worst


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_grad_path_refuses_capture_and_the_no_grad_forwards_replay():
    """Under a real capture only the forward-with-grad refusals are exercised (the backwards' are checked on the host,
    tests/test_interp_grad_cpu.py): nothing of the grad path is enqueued.  The three no-grad forwards capture and
    replay on new inputs."""
    z, w2, b2, _ = [_dev(t) for t in _head_case(2, 7, 9)]
    img = _dev(_up_case(2, 5, 7, 3)[0])
    for call in (lambda: ops.image_head(z.clone().requires_grad_(), w2, b2),
                 lambda: ops.upsample2x_image(img.clone().requires_grad_())):
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="cannot be captured"):
            with torch.cuda.graph(graph):
                call()
        torch.cuda.synchronize()
    frames = _dev(_grid(torch.Generator().manual_seed(5), (2, 32, 64, 3), 1 / 16))
    static = [z.clone(), img.clone(), frames.clone()]
    ops.image_head(static[0], w2, b2), ops.upsample2x_image(static[1]), ops.avgpool_pyramid(static[2], 5)  # warm up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = (ops.image_head(static[0], w2, b2), ops.upsample2x_image(static[1]), ops.avgpool_pyramid(static[2], 5))
    for s, t in zip(static, (z, img, frames)):
        s.copy_(t * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], ops.image_head(z * 0.5, w2, b2))
    assert torch.equal(outs[1], ops.upsample2x_image(img * 0.5))
    assert torch.equal(outs[2], ops.avgpool_pyramid(frames * 0.5, 5))

"""GPU suite of the decoder's Mish(Conv2DTranspose(4x4, stride 2, 'same') + bias) backward (qpwc_upconv4x4s2_bwd behind
torch autograd, ops.upconv4x4s2, layers.UpConv / layers.Decoder / layers.FlowerModel).

Oracle: torch autograd in float64 on the CPU of F.conv_transpose2d(x, w, b, stride=2, padding=1) +
oracle.torch_ref.mish, fed the same values.  Inputs and grad_out are multiples of 1/16 in [-1, 1], bias multiples of
1/8, weights multiples of 1/64 in [-1/8, 1/8] (at 256 input channels z then has std ~1.3 and |z| up to ~5: Mish' is
exercised away from 0 and 1).  Tolerance: the project's 1e-4 * max(1, max|ref|) per tensor
(tests/test_gpu_autograd.py::_tol)."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref
from qpwcnet_amd import layers, loss, ops, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_conv_grad import encoder_composite  # noqa: E402
from test_gpu_flow_head_grad import flow_mse_v2_composite, optflow_composite, upsample_composite  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (B, H, W, C, F) at which the grid-stride loop of upconv_bwd_w_kernel and the lane loop of conv_bwd_reduce_kernel make
# more than one trip with an uneven last one, the last pixel block is partial and the K loops of upconv_bwd_gemm_kernel
# make two steps (tests/test_upconv_grad_cpu.py checks this against the constants of csrc/upconv_bwd.hip)
MULTI_TRIP = (2, 37, 53, 64, 16)
# the 5-step training case: fp32-vs-float64 drift of the CPU composite and the bound derived from it (see the test)
TRAIN_DRIFT = 1.9e-7
TRAIN_RATES = (3.0, 0.1)   # encoder and decoder, flow estimators
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


def composite(x, w, b, mish=True):
    """The layer as torch ops: x (B,H,W,C) channels-last, w (C,F,4,4) in the torch layout, b (F) -> (B,2H,2W,F)."""
    z = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1).permute(0, 2, 3, 1)
    return torch_ref.mish(z) if mish else z


@functools.lru_cache(maxsize=None)
def _case(B, H, W, C, F_, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (_grid(gen, (B, H, W, C), 1 / 16), _grid(gen, (C, F_, 4, 4), 1 / 64, 1 / 8), _grid(gen, (F_,), 1 / 8),
            _grid(gen, (B, 2 * H, 2 * W, F_), 1 / 16))


def _oracle(case, mish):
    x, w, b, g = case
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    out = composite(*leaves, mish)
    out.backward(g)
    return out.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad


@functools.lru_cache(maxsize=None)
def _oracle_of(key, mish=True):
    return _oracle(_case(*key), mish)


def _dev(t):
    return t.float().to(DEV)


def _hip(case):
    """Forward + backward through autograd -> (out, grad_x, grad_w, grad_b)."""
    x, w, b = [_dev(t).requires_grad_() for t in case[:3]]
    out = ops.upconv4x4s2(x, w, b)
    out.backward(_dev(case[3]))
    return out, x.grad, w.grad, b.grad


def _taps_grad(gt):
    """(16, F, C) tap-major -> the torch layout (C, F, 4, 4)."""
    return gt.reshape(4, 4, gt.shape[1], gt.shape[2]).permute(3, 2, 0, 1)


def _compare(key, tag=""):
    ref = _oracle_of(key)
    got = _hip(_case(*key))
    for a, r, name in zip(got, ref, ("out", "grad_x", "grad_w", "grad_b")):
        _check(a, r, tag + name)
    return got


# ---- ragged sizes and borders, every channel pair's kernel instantiations ---------------------------------------------
@pytest.mark.parametrize("key", [(1, 3, 5, 64, 16), (2, 7, 9, 128, 32), (1, 4, 5, 256, 64), (1, 3, 4, 256, 128),
                                 (1, 1, 1, 64, 16)], ids=["64to16", "128to32", "256to64", "256to128", "1x1"])
def test_ragged_and_borders(key):
    _compare(key)


# ---- in the concat ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,S", [((2, 7, 9, 128, 32), 32), ((2, 7, 9, 128, 32), 16), ((1, 3, 5, 64, 16), 48)],
                         ids=["fused", "copy16", "copy48"])
def test_in_the_concat(key, S):
    B, H, W, C, F_ = key
    x, w, b, _ = _case(*key)
    gen = torch.Generator().manual_seed(7)
    skip, gcat = _grid(gen, (B, 2 * H, 2 * W, S), 1 / 16), _grid(gen, (B, 2 * H, 2 * W, F_ + S), 1 / 16)
    leaves = [t.clone().requires_grad_() for t in (x, w, b, skip)]
    ref = torch.cat([composite(*leaves[:3]), leaves[3]], dim=3)
    ref.backward(gcat)
    hx, hw, hb, hs = [_dev(t).requires_grad_() for t in (x, w, b, skip)]
    out = ops.upconv4x4s2(hx, hw, hb, hs)
    assert ops.upconv_cat_ok(hx.detach(), ops.upconv_taps(hw.detach()), hs.detach(), out.detach()) == (S == F_)
    out.backward(_dev(gcat))
    _check(out, ref.detach(), "concat")
    for a, r, name in zip((hx, hw, hb, hs), leaves, ("grad_x", "grad_w", "grad_b", "grad_skip")):
        _check(a.grad, r.grad, name)
    assert torch.equal(hs.grad, _dev(gcat)[..., F_:])
    # the bare call on the strided concat gradient against a contiguous copy of its first F channels
    taps, g = ops.upconv_taps(hw.detach()), _dev(gcat)
    strided = ops.upconv4x4s2_bwd(hx.detach(), taps, hb.detach(), g)
    dense = ops.upconv4x4s2_bwd(hx.detach(), taps, hb.detach(), g[..., :F_].contiguous())
    for a, c in zip(strided, dense):
        assert torch.equal(a, c)
    lin_s = ops.upconv4x4s2_bwd(hx.detach(), taps, hb.detach(), g, mish=False)       # g itself read through the stride
    lin_d = ops.upconv4x4s2_bwd(hx.detach(), taps, hb.detach(), g[..., :F_].contiguous(), mish=False)
    for a, c in zip(lin_s, lin_d):
        assert torch.equal(a, c)


# ---- exact without Mish ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(1, 3, 5, 64, 16), (2, 7, 9, 128, 32)], ids=["64to16", "128to32"])
def test_without_mish_is_exact(key):
    """mish off: inputs and grad_out multiples of 2^-4, weights of 2^-6, so every product and partial sum is a multiple
    of 2^-10; with sum|terms| * 2^10 < 2^24 all of them are fp32 values and any summation order is exact."""
    x, w, b, g = _case(*key)
    terms = _oracle((x.abs(), w.abs(), b.abs(), g.abs()), False)[1:]
    biggest = max(float(t.max()) for t in terms)
    print("max sum|terms| = {}".format(biggest))
    assert biggest * 2 ** 10 < 2 ** 24, biggest
    ref = _oracle_of(key, False)
    gx, gt, gb = ops.upconv4x4s2_bwd(_dev(x), ops.upconv_taps(_dev(w)), _dev(b), _dev(g), mish=False)
    assert torch.equal(gx.double().cpu(), ref[1])
    assert torch.equal(_taps_grad(gt).double().cpu(), ref[2])
    assert torch.equal(gb.double().cpu(), ref[3])


# ---- more than one trip of every loop -----------------------------------------------------------------------------------
def test_more_than_one_trip():
    _compare(MULTI_TRIP)


# ---- determinism, only what is asked, batch independence ---------------------------------------------------------------
@pytest.mark.parametrize("key", [(2, 7, 9, 128, 32), (2, 5, 6, 256, 128)], ids=["128to32", "256to128"])
def test_bitwise_determinism_and_independence(key):
    x, w, b, g = [_dev(t) for t in _case(*key)]
    taps = ops.upconv_taps(w)
    r1 = ops.upconv4x4s2_bwd(x, taps, b, g)
    r2 = ops.upconv4x4s2_bwd(x, taps, b, g)
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)
    for k in range(3):                                                   # each output alone: the other pointers NULL
        need = tuple(i == k for i in range(3))
        one = ops.upconv4x4s2_bwd(x, taps, b, g, need=need)
        assert [t is None for t in one] == [not n for n in need]
        assert torch.equal(one[k], r1[k]), k
    for k in range(3):                                                   # through autograd, asked for alone
        leaves = [t.clone().requires_grad_(i == k) for i, t in enumerate((x, w, b))]
        ops.upconv4x4s2(*leaves).backward(g)
        want = r1[k] if k != 1 else _taps_grad(r1[1])
        assert torch.equal(leaves[k].grad, want.reshape(leaves[k].shape)), k
    # grad_x of image 0 does not depend on the rest of the batch
    one = ops.upconv4x4s2_bwd(x[:1].contiguous(), taps, b, g[:1].contiguous(), need=(True, False, False))
    assert torch.equal(one[0][0], r1[0][0])


# ---- large arguments ---------------------------------------------------------------------------------------------------------
def test_large_arguments_stay_finite():
    key = (2, 7, 9, 128, 32)
    x, w, b, g = _case(*key)
    # every pre-activation near +50: Mish' saturates to 1 and grad_x is that of the linear layer
    up = (x, w, torch.full_like(b, 50.0), g)
    got = _hip(up)
    for a, r, name in zip(got, _oracle(up, True), ("out", "grad_x", "grad_w", "grad_b")):
        _check(a, r, "+50 " + name)
    _check(got[1], _oracle_of(key, False)[1], "+50 grad_x against the linear layer")
    mixed = b.clone()
    mixed[1], mixed[2], mixed[17], mixed[30] = 50.0, -50.0, 50.0, -50.0
    case = (x, w, mixed, g)
    for a, r, name in zip(_hip(case), _oracle(case, True), ("out", "grad_x", "grad_w", "grad_b")):
        _check(a, r, "+-50 " + name)


# ---- the forward with grad is the no-grad forward ---------------------------------------------------------------------
def test_forward_identity():
    key = (2, 7, 9, 128, 32)
    B, H, W, C, F_ = key
    x, w, b, _ = [_dev(t) for t in _case(*key)]
    taps = ops.upconv_taps(w)
    gen = torch.Generator().manual_seed(7)
    for S in (None, 32, 16):
        skip = _dev(_grid(gen, (B, 2 * H, 2 * W, S), 1 / 16)) if S else None
        plain = torch.empty((B, 2 * H, 2 * W, F_ + (S or 0)), device=DEV)
        if S == F_:
            ops.upconv4x4s2_mish_cat_into(x, taps, b, skip, plain)
        else:
            ops.upconv4x4s2_mish_into(x, taps, b, plain)
            if S:
                plain[..., F_:].copy_(skip)
        out = ops.upconv4x4s2(x.clone().requires_grad_(), w, b, skip)
        assert out.grad_fn is not None and torch.equal(out.detach(), plain), S
        assert ops.upconv4x4s2(x, w, b, skip).grad_fn is None
        assert torch.equal(ops.upconv4x4s2(x, w, b, skip), plain), S
        with torch.no_grad():
            quiet = ops.upconv4x4s2(x.clone().requires_grad_(), w, b, skip)
        assert quiet.grad_fn is None and torch.equal(quiet, plain), S
        if S:                                                            # only the skip requires grad
            only = ops.upconv4x4s2(x, w, b, skip.clone().requires_grad_())
            assert only.grad_fn is not None and torch.equal(only.detach(), plain)
    _check(plain[..., :F_], _oracle_of(key)[0], "forward")


# ---- the layers ------------------------------------------------------------------------------------------------------------
def decoder_composite(P, feats, n_levels, prefix="dec."):
    """layers.Decoder from a {name: tensor} dict on the stacked channels-last encoder levels -> the decoder levels."""
    f, decs = feats[-1], []
    for i in range(n_levels):
        up = composite(f, P["%s%d.conv_up.weight" % (prefix, i)], P["%s%d.conv_up.bias" % (prefix, i)])
        f = torch.cat([up, feats[-2 - i]], dim=3)
        decs.append(f)
    return decs


def _random_bias(module, gen):
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)


def test_upconv_layer_surface():
    key = (2, 4, 6, 64, 32)
    torch.manual_seed(0)
    lay = layers.UpConv(64, 32, data_format="channels_first", name="u").to(DEV)
    assert sorted(lay.state_dict()) == ["conv_up.bias", "conv_up.weight"]
    assert lay.get_config() == {"name": "u", "in_channels": 64, "filters": 32}
    x, _, _, g = _case(*key)
    P = {k: v.detach().double().cpu().requires_grad_() for k, v in lay.state_dict().items()}
    xr = x.clone().requires_grad_()
    ref = composite(xr, P["conv_up.weight"], P["conv_up.bias"])
    ref.backward(g)
    xh = _dev(x).permute(0, 3, 1, 2).contiguous().requires_grad_()
    out = lay(xh)
    assert out.shape == (2, 32, 8, 12)
    out.backward(_dev(g).permute(0, 3, 1, 2))
    _check(out.permute(0, 2, 3, 1), ref.detach(), "out")
    _check(xh.grad.permute(0, 2, 3, 1), xr.grad, "grad_x")
    for n, p in lay.named_parameters():
        _check(p.grad, P[n].grad, "grad " + n)
    # cat_skip, and channels_first against channels_last
    cl = layers.UpConv(64, 32, data_format="channels_last").to(DEV)
    cl.load_state_dict(lay.state_dict())
    skip = _dev(_grid(torch.Generator().manual_seed(3), (2, 8, 12, 32), 1 / 16))
    a = cl.cat_skip(_dev(x), skip)
    c = lay.cat_skip(_dev(x).permute(0, 3, 1, 2), skip.permute(0, 3, 1, 2))
    assert a.shape == (2, 8, 12, 64) and c.shape == (2, 64, 8, 12) and torch.equal(c.permute(0, 2, 3, 1), a)
    assert torch.equal(a[..., 32:], skip) and torch.equal(a[..., :32], out.detach().permute(0, 2, 3, 1))
    with pytest.raises(ValueError):
        lay(torch.zeros(1, 128, 4, 4, device=DEV))


def test_decoder_small_against_the_composite():
    """Decoder((32,), 64, (32,)) on leaf features shaped like those of Encoder((16, 32, 64)) at 32 x 48: the decoder
    levels, the gradient of every parameter and of every feature (the deepest one through the transposed convolution,
    the skip through the concat)."""
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    dec = layers.Decoder((32,), in_channels=64, skip_channels=(32,), data_format="channels_last")
    _random_bias(dec, gen)
    shapes = [(2, 32, 48, 3), (2, 16, 24, 16), (2, 8, 12, 32), (2, 4, 6, 64)]
    prv = [torch.randn(s, generator=gen) for s in shapes]
    nxt = [torch.randn(s, generator=gen) for s in shapes]
    P = {k: v.detach().double().clone().requires_grad_() for k, v in dec.state_dict().items()}
    rp, rn = [t.double().requires_grad_() for t in prv], [t.double().requires_grad_() for t in nxt]
    ref = decoder_composite(P, [torch.cat([a, b]) for a, b in zip(rp, rn)], 1)
    g = torch.randn(ref[0].shape, generator=gen, dtype=torch.float64)
    (ref[0] * g).sum().backward()
    dec = dec.to(DEV)
    hp, hn = [t.to(DEV).requires_grad_() for t in prv], [t.to(DEV).requires_grad_() for t in nxt]
    dp, dn = dec((hp, hn))
    assert len(dp) == len(dn) == 1 and dp[0].shape == (2, 8, 12, 64)
    (torch.cat([dp[0], dn[0]]) * g.float().to(DEV)).sum().backward()
    _check(torch.cat([dp[0], dn[0]]), ref[0].detach(), "dec[0]")
    for n, p in dec.named_parameters():
        _check(p.grad, P[n].grad, "grad " + n)
    for i in (2, 3):
        _check(hp[i].grad, rp[i].grad, "grad prv feature %d" % i)
        _check(hn[i].grad, rn[i].grad, "grad nxt feature %d" % i)
    assert hp[0].grad is None and hp[1].grad is None
    # channels_first equals channels_last bitwise, forward and backward
    cf = layers.Decoder((32,), in_channels=64, skip_channels=(32,), data_format="channels_first").to(DEV)
    cf.load_state_dict(dec.state_dict())
    cp, cn = [t.detach().permute(0, 3, 1, 2).requires_grad_() for t in hp], \
        [t.detach().permute(0, 3, 1, 2).requires_grad_() for t in hn]
    ep, en = cf((cp, cn))
    assert ep[0].shape == (2, 64, 8, 12)
    assert torch.equal(ep[0].permute(0, 2, 3, 1), dp[0]) and torch.equal(en[0].permute(0, 2, 3, 1), dn[0])
    (torch.cat([ep[0], en[0]]).permute(0, 2, 3, 1) * g.float().to(DEV)).sum().backward()
    for (n, p), (_, q) in zip(dec.named_parameters(), cf.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for i in (2, 3):
        assert torch.equal(cp[i].grad.permute(0, 2, 3, 1), hp[i].grad), i


def test_decoder_full_has_the_bits_of_the_no_grad_decoder():
    """The four levels at full width on the features of layers.Encoder, with grad: the stacked path and the two-list
    call agree bitwise with each other and with non_layers.UpConv.cat_skip of the no-grad network on the same features."""
    from qpwcnet_amd.pwcnet import build_flower
    hw = (64, 96)
    weights = synth.make_weights(42, hw)
    state = {k: torch.as_tensor(v) for k, v in weights.items()}
    enc, dec = layers.Encoder(data_format="channels_last"), layers.Decoder(data_format="channels_last")
    assert not enc.load_state_dict(state, strict=False).missing_keys
    assert not dec.load_state_dict(state, strict=False).missing_keys
    enc, dec = enc.to(DEV), dec.to(DEV)
    pairs = torch.as_tensor(synth.make_frames(2, hw[0], hw[1], seed=5)[0]).to(DEV)
    prv, nxt = pairs[..., :3], pairs[..., 3:]
    fp, fn = enc((prv, nxt), output_features=True)
    dp, dn = dec((fp, fn))
    assert [tuple(d.shape) for d in dp] == [(2, 4, 6, 256), (2, 8, 12, 128), (2, 16, 24, 64), (2, 32, 48, 32)]
    assert dp[-1].grad_fn is not None
    feats = enc.forward_stacked(torch.cat([prv, nxt]).contiguous())
    decs = dec.forward_stacked(feats)
    model = build_flower(True, hw, "channels_last", weights=weights, device=DEV)
    with torch.no_grad():
        f = feats[-1].detach()
        for i, layer in enumerate(model.dec):
            f = layer.cat_skip(f, feats[-2 - i].detach())
            assert torch.equal(decs[i].detach(), f), i
            assert torch.equal(torch.cat([dp[i], dn[i]]), f), i


# ---- the whole network -----------------------------------------------------------------------------------------------------
def test_whole_network_matches_the_no_grad_network_and_trains():
    from qpwcnet_amd.pwcnet import build_flower
    hw = (64, 96)
    weights = synth.make_weights(42, hw)
    state = {k: torch.as_tensor(v) for k, v in weights.items()}
    net = layers.FlowerModel(data_format="channels_last")
    res = net.load_state_dict(state)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV).eval()
    pairs, flow_gt = synth.make_frames(2, hw[0], hw[1], seed=5)
    pairs, gt = torch.as_tensor(pairs).to(DEV), torch.as_tensor(flow_gt).to(DEV)
    model = build_flower(True, hw, "channels_last", weights=weights, device=DEV)
    with torch.no_grad():
        want = model(pairs)
    flows = net(pairs)
    assert len(flows) == len(want) == 6 and flows[-1].shape == (2, 64, 96, 2) and flows[0].shape == (2, 2, 3, 2)
    assert flows[0].grad_fn is not None
    for i, (a, r) in enumerate(zip(flows, want)):
        _check(a, r.detach().double().cpu(), "flow %d" % i)
    with torch.no_grad():
        quiet = net(pairs)
    assert all(q.grad_fn is None and torch.equal(q, a.detach()) for q, a in zip(quiet, flows))
    # channels_first input and output
    cf = layers.FlowerModel(data_format="channels_first").to(DEV).eval()
    cf.load_state_dict(net.state_dict())
    with torch.no_grad():
        for a, c in zip(quiet, cf(pairs.permute(0, 3, 1, 2).contiguous())):
            assert torch.equal(c.permute(0, 2, 3, 1), a)
    net.train()
    total = loss.multiscale(loss.FlowMseLossV2(), gt, net(pairs))[0]
    total.backward()
    assert bool(torch.isfinite(total))
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, n


# ---- a short training run -------------------------------------------------------------------------------------------------
def train_case():
    """Fixed-seed FlowerModel((16, 32, 64), (32,)): Encoder, Decoder, Flow(64), one UpFlow(64); a 32 x 48 pair, its
    ground truth and the learning rates (encoder and decoder, flow estimators).  With Keras' initialisers as they are
    the activations of this untrained stack decay level by level (flows of 1e-5 pixels, weight gradients of 1e-9: see
    synth.KERNEL_GAIN), and nothing but the BatchNorm offsets moves beyond fp32 rounding; as in synth.make_weights
    the kernels that feed a Mish carry a gain of 1.7 and the biases are small random numbers, which keeps features and
    flows O(1).  The gradients of encoder and decoder are still ~1/30 of the estimators', hence one rate per group."""
    torch.manual_seed(0)
    net = layers.FlowerModel((16, 32, 64), (32,), data_format="channels_last")
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=gen) - 0.5) * 0.1)
            elif n.endswith("weight") and not n.endswith("flow.flow.weight"):
                p.mul_(synth.KERNEL_GAIN)
    pairs = torch.rand(2, 32, 48, 6, generator=gen) - 0.5
    gt = torch.randn(2, 32, 48, 2, generator=gen) * 4.0
    return net, pairs, gt, TRAIN_RATES


def _rate(name, lr):
    return lr[0] if name.startswith(("enc.", "dec.")) else lr[1]


def flower_composite(P, pairs, n_enc, n_dec, training=True):
    """layers.FlowerModel from a {name: tensor} dict as torch ops on the CPU -> its list of flows."""
    n = pairs.shape[0]
    feats = encoder_composite(P, [pairs[..., :3], pairs[..., 3:]], n_enc)
    decs = decoder_composite(P, feats, n_dec)
    prv, nxt = feats[-1][:n], feats[-1][n:]
    flo = optflow_composite(P, "flow.flow.", (torch_ref.cost_volume(prv, nxt, 4), prv, nxt), training)
    flows = [flo]
    for i, d in enumerate(decs):
        up = upsample_composite(flo, 2.0)
        cost = torch_ref.cost_volume(d[:n], torch_ref.warp_v2(d[n:], up), 4)
        flo = optflow_composite(P, "upflow.%d.flow." % i, (cost, d[:n], up), training)
        flows.append(flo)
    flows.append(upsample_composite(flo, 2.0))
    return flows


def train_composite(dtype, steps=5):
    """The SGD steps of pair -> FlowerModel -> FlowMseLossV2 over the estimated levels (the trainer's
    pred_flows[:-1]) on the torch composite in `dtype` on the CPU -> ({name: final parameter}, losses)."""
    net, pairs, gt, lr = train_case()
    P = {k: v.detach().to(dtype).clone() for k, v in net.state_dict().items()}
    names = [n for n, _ in net.named_parameters()]
    for n in names:
        P[n].requires_grad_()
    pairs, gt = pairs.to(dtype), gt.to(dtype)
    losses = []
    for _ in range(steps):
        flows = flower_composite(P, pairs, 3, 1)
        total = sum(flow_mse_v2_composite(gt, f) for f in flows[:-1])
        losses.append(float(total.detach()))
        grads = torch.autograd.grad(total, [P[n] for n in names])
        with torch.no_grad():
            for n, gr in zip(names, grads):
                P[n] -= _rate(n, lr) * gr
    return {n: P[n].detach() for n in names}, losses


def test_short_training_run():
    """5 SGD steps of a pair -> FlowerModel((16, 32, 64), (32,)) -> multiscale FlowMseLossV2 in training mode on the
    HIP layers, encoder, decoder and both estimators trained, against the same steps of the float64 composite.
    Measured on the CPU for exactly this case: the fp32 composite ends within TRAIN_DRIFT (max over all parameters) of
    the float64 one (tests/test_upconv_grad_cpu.py re-measures it); the bound is 10 x that (TRAIN_BOUND), the margin
    for fp32 sums in another order across 5 compounding steps, as TRAIN_DRIFT / TRAIN_BOUND of
    tests/test_gpu_sepconv_grad.py."""
    ref, losses = train_composite(torch.float64)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses            # the case really trains
    net, pairs, gt, lr = train_case()
    start = {n: p.detach().double().clone() for n, p in net.named_parameters()}
    net = net.to(DEV).train()
    pairs, gt = pairs.to(DEV), gt.to(DEV)
    feat = [p for n, p in net.named_parameters() if _rate(n, (0, 1)) == 0]
    est = [p for n, p in net.named_parameters() if _rate(n, (0, 1)) == 1]
    opt = torch.optim.SGD([{"params": feat, "lr": lr[0]}, {"params": est, "lr": lr[1]}])
    seen = []
    for _ in range(5):
        opt.zero_grad()
        total = loss.multiscale(loss.FlowMseLossV2(), gt, net(pairs)[:-1])[0]
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
def test_grad_path_refuses_capture():
    """Under a real capture only the forward-with-grad refusal is exercised (the backward's is checked on the host,
    tests/test_upconv_grad_cpu.py): nothing of the grad path is enqueued."""
    x, w, b, _ = [_dev(t) for t in _case(2, 7, 9, 128, 32)]
    xg = x.clone().requires_grad_()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph):
            ops.upconv4x4s2(xg, w, b)
    torch.cuda.synchronize()

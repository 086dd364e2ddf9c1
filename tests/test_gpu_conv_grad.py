"""GPU suite of the encoder's Conv2D(3x3, stride 1 / 2, 'same') (+ Mish) backward (qpwc_conv3x3_same_bwd behind torch
autograd, ops.conv3x3_same, layers.DownConv / layers.Encoder).

Oracle: torch autograd in float64 on the CPU of F.conv2d(F.pad(x, SAME), w, b, stride) + oracle.torch_ref.mish, fed the
same values.  Inputs and grad_out are multiples of 1/16 in [-1, 1], bias multiples of 1/8, weights multiples of 1/8 in
[-1, 1] for C_in <= 32 and of 1/64 in [-1/8, 1/8] for C_in >= 64 (with [-1, 1] weights at 256 channels |z| reaches 60
and Mish' is only ever 0 or 1).  Tolerance: the project's 1e-4 * max(1, max|ref|) per tensor
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
from test_gpu_flow_head_grad import flow_mse_v2_composite, optflow_composite  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (B, H, W, C_in, C_out, stride) at which the grid-stride loop of conv_bwd_w_kernel and the lane loop of
# conv_bwd_reduce_kernel make more than one trip with an uneven last one and the last pixel block is partial
# (tests/test_conv_grad_cpu.py checks both against the constants of csrc/conv_bwd.hip); the stride-2 twin also gives
# every parity class of the grad_x gather more than one workgroup
MULTI_TRIP = ((2, 101, 167, 16, 16, 1), (2, 101, 167, 16, 32, 2))
# the 5-step training case: fp32-vs-float64 drift of the CPU composite and the bound derived from it (see the test)
TRAIN_DRIFT = 1.5e-7
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


def same_pad(n, stride):
    """TensorFlow 'SAME' for a 3-wide window -> (before, after)."""
    total = max((-(-n // stride) - 1) * stride + 3 - n, 0)
    return total // 2, total - total // 2


def composite(x, w, b, stride, mish):
    """The layer as torch ops: x (B,H,W,C_in) channels-last, w (C_out,C_in,3,3), b (C_out)."""
    pt, pb = same_pad(x.shape[1], stride)
    pl, pr = same_pad(x.shape[2], stride)
    z = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w, b, stride=stride).permute(0, 2, 3, 1)
    return torch_ref.mish(z) if mish else z


@functools.lru_cache(maxsize=None)
def _case(B, H, W, ci, co, stride, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = _grid(gen, (B, H, W, ci), 1 / 16)
    w = _grid(gen, (co, ci, 3, 3), 1 / 8) if ci <= 32 else _grid(gen, (co, ci, 3, 3), 1 / 64, 1 / 8)
    return x, w, _grid(gen, (co,), 1 / 8), _grid(gen, (B, -(-H // stride), -(-W // stride), co), 1 / 16)


def _oracle(case, stride, mish):
    x, w, b, g = case
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    out = composite(*leaves, stride, mish)
    out.backward(g)
    return out.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad


@functools.lru_cache(maxsize=None)
def _oracle_of(key, mish):
    return _oracle(_case(*key), key[5], mish)


def _dev(t):
    return t.float().to(DEV)


def _hip(case, stride, mish):
    """Forward + backward through autograd -> (out, grad_x, grad_w, grad_b)."""
    x, w, b = [_dev(t).requires_grad_() for t in case[:3]]
    out = ops.conv3x3_same(x, w, b, stride=stride, mish=mish)
    out.backward(_dev(case[3]))
    return out, x.grad, w.grad, b.grad


def _compare(key, mish, tag=""):
    ref = _oracle_of(key, mish)
    got = _hip(_case(*key), key[5], mish)
    for a, r, name in zip(got, ref, ("out", "grad_x", "grad_w", "grad_b")):
        _check(a, r, tag + name)
    return got


# ---- ragged stride 1 -----------------------------------------------------------------------------------------------
RAGGED = (1, 7, 11, 16, 16, 1)


@pytest.mark.parametrize("mish", [True, False], ids=["mish", "linear"])
def test_ragged_stride1(mish):
    _compare(RAGGED, mish)


def test_ragged_without_mish_is_exact():
    """mish off: inputs and grad_out multiples of 2^-4, weights and bias of 2^-3, so every product and partial sum is a
    multiple of 2^-8; with sum|terms| * 2^8 < 2^24 all of them are fp32 values and any summation order is exact."""
    x, w, b, g = _case(*RAGGED)
    terms = _oracle((x.abs(), w.abs(), b.abs(), g.abs()), 1, False)
    biggest = max(float(t.max()) for t in terms)
    assert biggest * 2 ** 8 < 2 ** 24, biggest
    ref = _oracle_of(RAGGED, False)
    got = _hip(_case(*RAGGED), 1, False)
    for a, r in zip(got, ref):
        assert torch.equal(a.detach().double().cpu(), r)


# ---- stride 2: every padding case ------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(2, 7, 11, 16, 32, 2), (1, 8, 12, 16, 32, 2), (1, 8, 11, 32, 64, 2),
                                 (1, 1, 1, 16, 32, 2), (1, 2, 3, 16, 32, 2)],
                         ids=["odd", "even", "mixed", "1x1", "2x3"])
def test_stride2_padding(key):
    assert same_pad(7, 2) == (1, 1) and same_pad(8, 2) == (0, 1) and same_pad(1, 2) == (1, 1)
    _compare(key, True)
    _compare(key, False, "linear ")


# ---- the first layer: 12-byte pixels, padded weight slot ----------------------------------------------------------------
@pytest.mark.parametrize("hw", [(8, 12), (7, 9)], ids=["even", "odd"])
def test_first_layer(hw):
    key = (1,) + hw + (3, 16, 2)
    _compare(key, True)
    x, w, b, g = [_dev(t) for t in _case(*key)]
    taps = ops.conv3x3_same_taps(w)
    assert tuple(taps.shape) == (9, 16, 4)
    gx, gt, gb = ops.conv3x3_same_bwd(x, taps, b, g, stride=2, mish=True)
    assert float(gt[..., 3].abs().max()) == 0.0                       # the pad slot is written, as zeros
    ref = _oracle_of(key, True)
    _check(gt[..., :3].reshape(3, 3, 16, 3).permute(2, 3, 0, 1), ref[2], "bare grad_w")
    _check(gx, ref[1], "bare grad_x")


# ---- wide layers at tiny spatial size -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(1, 5, 6, 256, 256, 1), (1, 6, 8, 128, 256, 2), (2, 9, 10, 64, 64, 1),
                                 (2, 9, 10, 64, 128, 2), (1, 9, 10, 128, 128, 1)],
                         ids=["256", "128to256s2", "64", "64to128s2", "128"])
def test_wide_layers(key):
    _compare(key, True)


# ---- more than one trip of every loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MULTI_TRIP, ids=["stride1", "stride2"])
def test_more_than_one_trip(key):
    _compare(key, True)


# ---- determinism, only what is asked, batch independence ---------------------------------------------------------------
@pytest.mark.parametrize("key", [(2, 9, 10, 64, 128, 2), (2, 7, 11, 16, 16, 1)], ids=["s2", "s1"])
def test_bitwise_determinism_and_independence(key):
    x, w, b, g = [_dev(t) for t in _case(*key)]
    s = key[5]
    taps = ops.conv3x3_same_taps(w)
    r1 = ops.conv3x3_same_bwd(x, taps, b, g, s, True)
    r2 = ops.conv3x3_same_bwd(x, taps, b, g, s, True)
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)
    for k in range(3):                                                   # each output alone: the other pointers NULL
        need = tuple(i == k for i in range(3))
        one = ops.conv3x3_same_bwd(x, taps, b, g, s, True, need=need)
        assert [t is None for t in one] == [not n for n in need]
        assert torch.equal(one[k], r1[k]), k
    # through autograd, asked for alone
    for k in range(3):
        leaves = [t.clone().requires_grad_(i == k) for i, t in enumerate((x, w, b))]
        ops.conv3x3_same(*leaves, stride=s).backward(g)
        want = r1[k] if k != 1 else r1[1][..., :key[3]].reshape(3, 3, key[4], key[3]).permute(2, 3, 0, 1)
        assert torch.equal(leaves[k].grad, want.reshape(leaves[k].shape)), k
    # grad_x of image 0 does not depend on the rest of the batch
    one = ops.conv3x3_same_bwd(x[:1].contiguous(), taps, b, g[:1].contiguous(), s, True, need=(True, False, False))
    assert torch.equal(one[0][0], r1[0][0])


# ---- the forward with grad is the no-grad forward ---------------------------------------------------------------------
def test_forward_identity():
    # stride 1, 32 -> 32: qpwc_conv3x3_mish_fwd
    x, w, b, _ = [_dev(t) for t in _case(2, 9, 10, 32, 32, 1)]
    plain = ops.conv3x3_mish(x, ops.conv3x3_taps(w), b)
    out = ops.conv3x3_same(x.clone().requires_grad_(), w, b)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    with torch.no_grad():
        assert torch.equal(ops.conv3x3_same(x, w, b), plain)
    assert ops.conv3x3_same(x, w, b).grad_fn is None
    _check(out, _oracle_of((2, 9, 10, 32, 32, 1), True)[0], "conv3x3_mish out")
    # stride 2, 16 -> 32, even sizes: conv3x3_mish(pad 1, 1) -> conv3x3s2_mish
    key = (2, 8, 12, 16, 32, 2)
    x, w, b, _ = [_dev(t) for t in _case(*key)]
    w0, b0 = [_dev(t) for t in _case(2, 8, 12, 16, 16, 1, seed=3)[1:3]]
    padded = ops.conv3x3_mish(x, ops.conv3x3_taps(w0), b0, 1, 1)
    plain = ops.conv3x3s2_mish(padded, ops.conv3x3_taps(w), b)
    y = padded[:, :8, :12, :].contiguous()
    out = ops.conv3x3_same(y, w, b.clone().requires_grad_(), stride=2)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    with torch.no_grad():
        assert torch.equal(ops.conv3x3_same(y, w, b, stride=2), plain)
    # the new forward kernel's shapes: odd sizes, mish off, C_in = 3, C_out != C_in at stride 1
    for key, mish in (((2, 7, 11, 16, 32, 2), True), ((1, 7, 11, 16, 16, 1), False), ((1, 8, 12, 3, 16, 2), True),
                      ((1, 7, 9, 16, 64, 1), True), ((1, 8, 12, 16, 32, 2), False)):
        x, w, b, _ = [_dev(t) for t in _case(*key)]
        with torch.no_grad():
            plain = ops.conv3x3_same(x, w, b, stride=key[5], mish=mish)
        _check(plain, _oracle_of(key, mish)[0], "conv3x3_same_fwd {} out".format(key))
        out = ops.conv3x3_same(x.clone().requires_grad_(), w, b, stride=key[5], mish=mish)
        assert torch.equal(out.detach(), plain)


# ---- the layers ------------------------------------------------------------------------------------------------------------
def encoder_composite(P, imgs, n_levels, prefix="enc."):
    """layers.Encoder from a {name: tensor} dict -> the stacked-frame features of every level (channels-last)."""
    f = torch.cat(list(imgs), dim=0)
    feats = []
    for i in range(n_levels):
        for name, stride in (("conv_a", 2), ("conv_aa", 1), ("conv_b", 1)):
            f = composite(f, P["%s%d.%s.weight" % (prefix, i, name)], P["%s%d.%s.bias" % (prefix, i, name)], stride, True)
        feats.append(f)
    return feats


def _encoder_case(filters, hw, seed=0):
    torch.manual_seed(seed)
    enc = layers.Encoder(filters, data_format="channels_last")
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
    imgs = [torch.rand((2,) + hw + (3,), generator=gen) for _ in range(2)]
    return enc, imgs, gen


def test_encoder_small_against_the_composite():
    enc, imgs, gen = _encoder_case((16, 32, 64), (32, 48))
    P = {k: v.detach().double().clone().requires_grad_() for k, v in enc.state_dict().items()}
    feats = encoder_composite(P, [t.double() for t in imgs], 3)
    gs = [torch.randn(f.shape, generator=gen, dtype=torch.float64) for f in feats]
    sum((f * g).sum() for f, g in zip(feats, gs)).backward()
    enc = enc.to(DEV)
    fp, fn = enc((imgs[0].to(DEV), imgs[1].to(DEV)), output_features=True)
    assert len(fp) == len(fn) == 4 and fp[0].shape == (2, 32, 48, 3)
    sum((torch.cat([a, b]) * g.float().to(DEV)).sum() for a, b, g in zip(fp[1:], fn[1:], gs)).backward()
    for i in range(3):
        _check(torch.cat([fp[i + 1], fn[i + 1]]), feats[i].detach(), "feature %d" % i)
    for n, p in enc.named_parameters():
        _check(p.grad, P[n].grad, "grad " + n)
    last = enc((imgs[0].to(DEV), imgs[1].to(DEV)))
    assert torch.equal(last[0], fp[-1]) and torch.equal(last[1], fn[-1])


def test_encoder_full_matches_the_no_grad_network():
    from qpwcnet_amd.pwcnet import build_flower
    hw = (64, 96)
    weights = synth.make_weights(42, hw)
    enc = layers.Encoder(data_format="channels_last")
    missing = enc.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()}, strict=False)
    assert not missing.missing_keys
    enc = enc.to(DEV)
    gen = torch.Generator().manual_seed(2)
    pairs = torch.rand((2,) + hw + (6,), generator=gen).to(DEV)
    model = build_flower(True, hw, "channels_last", weights=weights, device=DEV)
    with torch.no_grad():
        want = model._encode_stacked(pairs)
    fp, fn = enc((pairs[..., :3], pairs[..., 3:]), output_features=True)
    assert fp[-1].grad_fn is not None
    for i in range(5):
        _check(torch.cat([fp[i + 1], fn[i + 1]]), want[i + 1].detach().double().cpu(), "enc[%d]" % i)
    # channels_first agrees with channels_last
    cf = layers.Encoder(data_format="channels_first").to(DEV)
    cf.load_state_dict(enc.state_dict())
    gp, gn = cf((pairs[..., :3].permute(0, 3, 1, 2), pairs[..., 3:].permute(0, 3, 1, 2)), output_features=True)
    assert gp[-1].shape == (2, 256, 2, 3)
    for a, b in zip(gp[1:] + gn[1:], fp[1:] + fn[1:]):
        assert torch.equal(a.permute(0, 2, 3, 1), b)
    g = torch.randn(fp[-1].shape, generator=gen).to(DEV)
    ((fp[-1] + fn[-1]) * g).sum().backward()
    ((gp[-1] + gn[-1]).permute(0, 2, 3, 1) * g).sum().backward()
    for (n, p), (_, q) in zip(enc.named_parameters(), cf.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_downconv_layer_surface():
    key = (2, 8, 12, 16, 32, 2)
    torch.manual_seed(0)
    lay = layers.DownConv(16, 32, data_format="channels_first", name="d").to(DEV)
    assert sorted(lay.state_dict()) == ["conv_a.bias", "conv_a.weight", "conv_aa.bias", "conv_aa.weight", "conv_b.bias",
                                        "conv_b.weight"]
    assert lay.get_config() == {"name": "d", "in_channels": 16, "filters": 32}
    x = _dev(_case(*key)[0]).permute(0, 3, 1, 2).contiguous().requires_grad_()
    out = lay(x)
    assert out.shape == (2, 32, 4, 6)
    P = {k: v.detach().double().cpu().requires_grad_() for k, v in lay.state_dict().items()}
    xr = _case(*key)[0].clone().requires_grad_()
    f = xr
    for name, stride in (("conv_a", 2), ("conv_aa", 1), ("conv_b", 1)):
        f = composite(f, P[name + ".weight"], P[name + ".bias"], stride, True)
    g = _grid(torch.Generator().manual_seed(4), tuple(f.shape), 1 / 16)
    f.backward(g)
    out.backward(_dev(g).permute(0, 3, 1, 2))
    _check(out.permute(0, 2, 3, 1), f.detach(), "out")
    _check(x.grad.permute(0, 2, 3, 1), xr.grad, "grad_x")
    for n, p in lay.named_parameters():
        _check(p.grad, P[n].grad, "grad " + n)
    with pytest.raises(ValueError):
        lay(torch.zeros(1, 8, 4, 4, device=DEV))


# ---- a short training run -------------------------------------------------------------------------------------------------
def train_case():
    """Fixed-seed Encoder((16, 32)) + Flow(32) with Keras' initialisers, a 32 x 48 pair, its ground truth and the
    learning rates (encoder, flow block).  The loss scales the flow by 2 / (h + w) and the flow block multiplies by
    sqrt(h^2 + w^2), so the encoder's gradients are ~1e-5 of the flow block's: with one rate for both, either the
    encoder does not move beyond fp32 rounding or the flow block diverges."""
    torch.manual_seed(0)
    enc = layers.Encoder((16, 32), data_format="channels_last")
    flow = layers.Flow(32, data_format="channels_last")
    gen = torch.Generator().manual_seed(1)
    imgs = [torch.rand(2, 32, 48, 3, generator=gen) for _ in range(2)]
    gt = torch.randn(2, 32, 48, 2, generator=gen) * 4.0
    return enc, flow, imgs, gt, (1e5, 1.0)


def train_state(enc, flow, dtype):
    P = {"e." + k: v.detach().to(dtype).clone() for k, v in enc.state_dict().items()}
    P.update({"f." + k: v.detach().to(dtype).clone() for k, v in flow.state_dict().items()})
    names = ["e." + n for n, _ in enc.named_parameters()] + ["f." + n for n, _ in flow.named_parameters()]
    for n in names:
        P[n].requires_grad_()
    return P, names


def train_composite(dtype, steps=5):
    """The SGD steps of images -> encoder -> coarsest Flow -> FlowMseLossV2 on the torch composite in `dtype` on the
    CPU -> ({name: final parameter}, losses)."""
    enc, flow, imgs, gt, lr = train_case()
    P, names = train_state(enc, flow, dtype)
    imgs, gt = [t.to(dtype) for t in imgs], gt.to(dtype)
    losses = []
    for _ in range(steps):
        f = encoder_composite(P, imgs, 2, prefix="e.enc.")[-1]
        prv, nxt = f[:2], f[2:]
        f0 = optflow_composite(P, "f.flow.", (torch_ref.cost_volume(prv, nxt, 4), prv, nxt), True)
        total = flow_mse_v2_composite(gt, f0)
        losses.append(float(total.detach()))
        grads = torch.autograd.grad(total, [P[n] for n in names])
        with torch.no_grad():
            for n, gr in zip(names, grads):
                P[n] -= lr[0 if n.startswith("e.") else 1] * gr
    return {n: P[n].detach() for n in names}, losses


def test_short_training_run():
    """5 SGD steps of images -> Encoder((16, 32)) -> Flow(32) -> multiscale FlowMseLossV2 in training mode on the HIP
    layers, every parameter trained, against the same steps of the float64 composite.  Measured on the CPU for exactly
    this case: the fp32 composite ends within TRAIN_DRIFT (max over all parameters) of the float64 one
    (tests/test_conv_grad_cpu.py re-measures it); the bound is 10 x that (TRAIN_BOUND), the margin for fp32 sums in
    another order across 5 compounding steps, as TRAIN_DRIFT / TRAIN_BOUND of tests/test_gpu_sepconv_grad.py."""
    ref, losses = train_composite(torch.float64)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses            # the case really trains
    enc, flow, imgs, gt, lr = train_case()
    enc, flow = enc.to(DEV).train(), flow.to(DEV).train()
    imgs, gt = [t.to(DEV) for t in imgs], gt.to(DEV)
    opt = torch.optim.SGD([{"params": list(enc.parameters()), "lr": lr[0]},
                           {"params": list(flow.parameters()), "lr": lr[1]}])
    seen = []
    for _ in range(5):
        opt.zero_grad()
        total = loss.multiscale(loss.FlowMseLossV2(), gt, [flow(enc((imgs[0], imgs[1])))])[0]
        seen.append(float(total.detach()))
        total.backward()
        opt.step()
    assert all(b < a for a, b in zip(seen, seen[1:])), seen
    got = dict([("e." + n, p) for n, p in enc.named_parameters()] + [("f." + n, p) for n, p in flow.named_parameters()])
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0.0 for p in got.values())
    worst = max(float((got[n].detach().double().cpu() - r).abs().max()) for n, r in ref.items())
    print("final-parameter drift {:.3e}, bound {:.3e}".format(worst, TRAIN_BOUND))
    assert worst <= TRAIN_BOUND, worst


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_grad_path_refuses_capture():
    """Under a real capture only the forward-with-grad refusal is exercised (the backward's is checked on the host,
    tests/test_conv_grad_cpu.py): nothing of the grad path is enqueued."""
    x, w, b, _ = [_dev(t) for t in _case(2, 9, 10, 32, 32, 1)]
    xg = x.clone().requires_grad_()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph):
            ops.conv3x3_same(xg, w, b)
    torch.cuda.synchronize()

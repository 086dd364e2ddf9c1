"""GPU suite of the SeparableConv2D backward (qpwc_sepconv3x3_bwd behind torch autograd, layers.SeparableConv2D).

Oracle: torch autograd in float64 on the CPU of the composite oracle.torch_ref.depthwise3x3 -> matmul + bias ->
oracle.torch_ref.mish, fed the same values.  Inputs and grad_out are multiples of 1/16 in [-1, 1], weights multiples
of 1/8.  Tolerance: the project's 1e-4 * max(1, max|ref|) per tensor (tests/test_gpu_autograd.py::_tol)."""
import functools

import pytest
import torch

from oracle import torch_ref
from qpwcnet_amd import layers, non_layers, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
# (B, H, W, C, F) at which every grid-stride loop of sepconv_bwd.hip makes two trips with an uneven last one and the
# last pixel block, strip and strip group are partial (tests/test_sepconv_grad_cpu.py checks it against the constants)
MULTI_TRIP = (2, 101, 167, 32, 16)
# the 5-step training case: fp32-vs-float64 drift of the CPU composite and the bound derived from it (see the test)
TRAIN_DRIFT = 7.1e-8
TRAIN_BOUND = 10 * TRAIN_DRIFT


def _grid(gen, shape, step):
    n = int(round(1 / step))
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


def composite(sources, dw, pw, bias, on_load, on_store):
    """The layer as torch ops: dw (C,1,3,3), pw (F,C), bias (F)."""
    d = torch_ref.depthwise3x3(sources, dw, on_load)
    z = d @ pw.t() + bias
    return torch_ref.mish(z) if on_store else z


@functools.lru_cache(maxsize=None)
def _case(B, H, W, chans, F, seed=0):
    gen = torch.Generator().manual_seed(seed)
    C = sum(chans)
    srcs = tuple(_grid(gen, (B, H, W, c), 1 / 16) for c in chans)
    return srcs, _grid(gen, (C, 1, 3, 3), 1 / 8), _grid(gen, (F, C), 1 / 8), _grid(gen, (F,), 1 / 8), \
        _grid(gen, (B, H, W, F), 1 / 16)


def _oracle(case, flags):
    srcs, dw, pw, bias, g = case
    leaves = [t.clone().requires_grad_() for t in srcs + (dw, pw, bias)]
    n = len(srcs)
    out = composite(leaves[:n], leaves[n], leaves[n + 1], leaves[n + 2], *flags)
    out.backward(g)
    return out.detach(), [t.grad for t in leaves[:n]], leaves[n].grad, leaves[n + 1].grad, leaves[n + 2].grad


@functools.lru_cache(maxsize=None)
def _oracle_of(key, flags):
    return _oracle(_case(*key), flags)


def _hip(case, flags, src_views=None):
    """Forward + backward through autograd -> (out, [grad_src], grad_dw, grad_pw (F,C), grad_bias)."""
    srcs, dw, pw, bias, g = case
    xs = src_views if src_views is not None else [t.float().to(DEV).requires_grad_() for t in srcs]
    w = dw.float().to(DEV).requires_grad_()
    p = pw.float().to(DEV).requires_grad_()
    b = bias.float().to(DEV).requires_grad_()
    out = ops.sepconv3x3(xs, w, ops.pad_pointwise(p), b, *flags)
    out.backward(g.float().to(DEV))
    return out, xs, w.grad, p.grad, b.grad


def _compare(key, flags, tag=""):
    case = _case(*key)
    ref = _oracle_of(key, flags)
    out, xs, gdw, gpw, gb = _hip(case, flags)
    _check(out, ref[0], tag + "out")
    for i, x in enumerate(xs):
        _check(x.grad, ref[1][i], tag + "grad_src%d" % i)
    _check(gdw, ref[2], tag + "grad_dw")
    _check(gpw, ref[3], tag + "grad_pw")
    _check(gb, ref[4], tag + "grad_bias")
    return out, xs, gdw, gpw, gb


# ---- ragged, one source --------------------------------------------------------------------------------------------
RAGGED = (1, 7, 11, (5,), 16)


@pytest.mark.parametrize("flags", FLAGS, ids=["00", "10", "01", "11"])
def test_ragged_one_source(flags):
    _compare(RAGGED, flags)


def test_ragged_without_mish_is_exact():
    """Both flags off: inputs and grad_out multiples of 2^-4, weights of 2^-3, so every product and partial sum is a
    multiple of 2^-11; with sum|terms| * 2^11 < 2^24 all of them are fp32 values and any summation order is exact."""
    srcs, dw, pw, bias, g = _case(*RAGGED)
    ab = [t.abs() for t in srcs], dw.abs(), pw.abs(), bias.abs(), g.abs()
    terms = _oracle((tuple(ab[0]),) + ab[1:], (False, False))
    d_abs = torch_ref.depthwise3x3(ab[0], ab[1])
    gd_abs = ab[4] @ ab[2]
    biggest = max(float(t.max()) for t in [terms[0], terms[2], terms[3], terms[4], d_abs, gd_abs] + terms[1])
    assert biggest * 2 ** 11 < 2 ** 24, biggest
    ref = _oracle_of(RAGGED, (False, False))
    out, xs, gdw, gpw, gb = _hip(_case(*RAGGED), (False, False))
    assert torch.equal(out.detach().double().cpu(), ref[0])
    assert torch.equal(xs[0].grad.double().cpu(), ref[1][0])
    assert torch.equal(gdw.double().cpu(), ref[2])
    assert torch.equal(gpw.double().cpu(), ref[3])
    assert torch.equal(gb.double().cpu(), ref[4])


# ---- three sources, the cost volume as an 84-float strided view -----------------------------------------------------
def test_three_sources_strided():
    key = (2, 9, 18, (81, 32, 2), 128)
    case = _case(*key)
    ref = _oracle_of(key, (False, True))
    cost84 = torch.zeros(2, 9, 18, 84, device=DEV)
    cost84[..., :81] = case[0][0].float().to(DEV)
    cost84[..., 81:] = 7.0                                    # the view's pad floats must not be read as channels
    cost84.requires_grad_()
    prv = case[0][1].float().to(DEV).requires_grad_()
    flo = case[0][2].float().to(DEV).requires_grad_()
    out, _, gdw, gpw, gb = _hip(case, (False, True), [cost84[..., :81], prv, flo])
    _check(out, ref[0], "out")
    _check(cost84.grad[..., :81], ref[1][0], "grad_cost")
    assert float(cost84.grad[..., 81:].abs().max()) == 0.0
    _check(prv.grad, ref[1][1], "grad_prv")
    _check(flo.grad, ref[1][2], "grad_flo")
    _check(gdw, ref[2], "grad_dw")
    _check(gpw, ref[3], "grad_pw")
    _check(gb, ref[4], "grad_bias")


def test_three_sources_padded_cost_volume():
    """The 84-channel padded cost volume (OptFlow's layer-1 form): pad channels of value 0 with zero weights."""
    key = (2, 9, 18, (81, 32, 2), 128)
    srcs, dw, pw, bias, g = _case(*key)
    ref = _oracle_of(key, (False, True))
    cost84 = torch.zeros(2, 9, 18, 84, dtype=torch.float64)
    cost84[..., :81] = srcs[0]
    dw84 = torch.cat([dw[:81], torch.zeros(3, 1, 3, 3, dtype=torch.float64), dw[81:]])
    pw84 = torch.cat([pw[:, :81], torch.zeros(128, 3, dtype=torch.float64), pw[:, 81:]], dim=1)
    out, xs, gdw, gpw, gb = _hip(((cost84, srcs[1], srcs[2]), dw84, pw84, bias, g), (False, True))
    _check(out, ref[0], "out")
    _check(xs[0].grad[..., :81], ref[1][0], "grad_cost")
    _check(xs[1].grad, ref[1][1], "grad_prv")
    _check(xs[2].grad, ref[1][2], "grad_flo")
    _check(torch.cat([gdw[:81], gdw[84:]]), ref[2], "grad_dw")
    _check(torch.cat([gpw[:, :81], gpw[:, 84:]], dim=1), ref[3], "grad_pw")
    _check(gb, ref[4], "grad_bias")
    assert float(gpw[:, 81:84].abs().max()) == 0.0 and float(xs[0].grad[..., 81:].abs().max()) == 0.0


# ---- every F and the chain shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,F,flags", [(128, 64, (True, True)), (64, 32, (True, True)), (32, 16, (True, False))],
                         ids=["128to64", "64to32", "32to16"])
def test_chain_shapes(C, F, flags):
    _compare((2, 16, 32, (C,), F), flags)


# ---- only what is asked --------------------------------------------------------------------------------------------
def test_only_what_is_asked():
    key = (2, 9, 18, (7, 12), 32)
    srcs, dw, pw, bias, g = _case(*key)
    flags = (True, True)
    ref = _oracle_of(key, flags)
    dev = lambda t: t.float().to(DEV)
    gd = dev(g)
    # one source without grad: None for it, its neighbour still right
    a, b = dev(srcs[0]), dev(srcs[1]).requires_grad_()
    out = ops.sepconv3x3([a, b], dev(dw), ops.pad_pointwise(dev(pw)), dev(bias), *flags)
    out.backward(gd)
    assert a.grad is None
    _check(b.grad, ref[1][1], "grad_src1 alone")
    # weights only
    w, p, bb = dev(dw).requires_grad_(), dev(pw).requires_grad_(), dev(bias).requires_grad_()
    ops.sepconv3x3([dev(srcs[0]), dev(srcs[1])], w, ops.pad_pointwise(p), bb, *flags).backward(gd)
    _check(w.grad, ref[2], "grad_dw alone")
    _check(p.grad, ref[3], "grad_pw alone")
    _check(bb.grad, ref[4], "grad_bias with weights")
    # bias only
    bb = dev(bias).requires_grad_()
    ops.sepconv3x3([dev(srcs[0]), dev(srcs[1])], dev(dw), ops.pad_pointwise(dev(pw)), bb, *flags).backward(gd)
    _check(bb.grad, ref[4], "grad_bias alone")
    # the thin wrapper: None for whatever is not asked for
    gs, gdw, gpw, gb = ops.sepconv3x3_bwd([dev(srcs[0]), dev(srcs[1])], dev(dw), ops.pad_pointwise(dev(pw)), dev(bias),
                                          gd, *flags, need=((False, True), False, True, False))
    assert gs[0] is None and gdw is None and gb is None
    _check(gs[1], ref[1][1], "wrapper grad_src1")
    _check(gpw[:, :19], ref[3], "wrapper grad_pw")
    assert float(gpw[:, 19:].abs().max()) == 0.0              # pad columns are written, as zeros


# ---- large arguments -----------------------------------------------------------------------------------------------
def test_large_arguments_stay_finite():
    srcs, dw, pw, bias, g = _case(2, 9, 18, (37,), 32, seed=3)
    x, bias = srcs[0].clone(), bias.clone()
    flat = x.view(-1)
    flat[5], flat[77], flat[1201], flat[4003] = 40.0, -40.0, 100.0, -100.0
    bias[1], bias[2], bias[17], bias[30] = 40.0, -40.0, 100.0, -100.0
    case = ((x,), dw, pw, bias, g)
    ref = _oracle(case, (True, True))
    out, xs, gdw, gpw, gb = _hip(case, (True, True))
    _check(out, ref[0], "out")
    _check(xs[0].grad, ref[1][0], "grad_src")
    _check(gdw, ref[2], "grad_dw")
    _check(gpw, ref[3], "grad_pw")
    _check(gb, ref[4], "grad_bias")


# ---- forward bits, determinism, batch independence -------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=["00", "10", "01", "11"])
def test_forward_bits_match_the_no_grad_forward(flags):
    srcs, dw, pw, bias, g = _case(2, 9, 18, (7, 12), 32)
    dev = lambda t: t.float().to(DEV)
    xs, w, p, b = [dev(t) for t in srcs], dev(dw), ops.pad_pointwise(dev(pw)), dev(bias)
    with torch.no_grad():
        plain = ops.sepconv3x3(xs, w, p, b, *flags)
    assert plain.grad_fn is None
    assert ops.sepconv3x3(xs, w, p, b, *flags).grad_fn is None          # nothing requires grad: the same launch
    out = ops.sepconv3x3([t.clone().requires_grad_() for t in xs], w, p, b.clone().requires_grad_(), *flags)
    assert out.grad_fn is not None
    assert torch.equal(out.detach(), plain)


def test_bitwise_determinism_and_batch_independence():
    srcs, dw, pw, bias, g = _case(2, 16, 32, (40, 3), 64, seed=5)
    dev = lambda t: t.float().to(DEV)
    xs, w, p, b, gd = [dev(t) for t in srcs], dev(dw), ops.pad_pointwise(dev(pw)), dev(bias), dev(g)
    r1 = ops.sepconv3x3_bwd(xs, w, p, b, gd, True, True)
    r2 = ops.sepconv3x3_bwd(xs, w, p, b, gd, True, True)
    for a, c in zip(r1[0] + list(r1[1:]), r2[0] + list(r2[1:])):
        assert torch.equal(a, c)
    for i in range(2):
        one = ops.sepconv3x3_bwd([t[i:i + 1].contiguous() for t in xs], w, p, b, gd[i:i + 1].contiguous(), True, True,
                                 need=(True, False, False, False))
        for k in range(2):
            assert torch.equal(one[0][k][0], r1[0][k][i])


# ---- more than one trip of every grid-stride loop ----------------------------------------------------------------------
def test_more_than_one_trip():
    B, H, W, C, F = MULTI_TRIP
    _compare((B, H, W, (C,), F), (True, True))


# ---- the layer -----------------------------------------------------------------------------------------------------
def _load(layer, dw, pw, bias):
    with torch.no_grad():
        layer.depthwise.weight.copy_(dw)
        layer.pointwise.weight.copy_(pw.reshape(pw.shape + (1, 1)))
        layer.bias.copy_(bias)
    return layer.to(DEV)


def _check_layer(layer, ref, tag):
    _check(layer.depthwise.weight.grad, ref[2], tag + "grad_dw")
    _check(layer.pointwise.weight.grad[:, :, 0, 0], ref[3], tag + "grad_pw")
    _check(layer.bias.grad, ref[4], tag + "grad_bias")


def test_layer_surface():
    key = (2, 9, 18, (7, 12), 32)
    srcs, dw, pw, bias, g = _case(*key)
    ref = _oracle_of(key, (False, True))
    one = torch.cat(srcs, dim=3)
    # channels-last, tuple call
    lay = _load(layers.SeparableConv2D(19, 32, data_format="channels_last"), dw, pw, bias)
    xs = [t.float().to(DEV).requires_grad_() for t in srcs]
    out = lay(tuple(xs))
    out.backward(g.float().to(DEV))
    _check(out, ref[0], "nhwc out")
    for i in range(2):
        _check(xs[i].grad, ref[1][i], "nhwc grad_src%d" % i)
    _check_layer(lay, ref, "nhwc ")
    # channels-first, dense NCHW and channels_last memory, one tensor
    for mem in (torch.contiguous_format, torch.channels_last):
        lay = _load(layers.SeparableConv2D(19, 32, data_format="channels_first"), dw, pw, bias)
        x = one.permute(0, 3, 1, 2).float().to(DEV).contiguous(memory_format=mem).requires_grad_()
        out = lay(x)
        assert out.shape == (2, 32, 9, 18)
        out.backward(g.permute(0, 3, 1, 2).float().to(DEV))
        _check(out.permute(0, 2, 3, 1), ref[0], "nchw out")
        _check(x.grad.permute(0, 2, 3, 1), torch.cat(ref[1], dim=3), "nchw grad_x")
        _check_layer(lay, ref, "nchw ")
        with torch.no_grad():
            assert torch.equal(lay(x), out.detach())
    # the functor twin reads the same weights from a params dict
    params = {"h.depthwise.weight": lay.depthwise.weight.detach().clone().requires_grad_(),
              "h.pointwise.weight": lay.pointwise.weight.detach(), "h.bias": lay.bias.detach()}
    fun = non_layers.SeparableConv2D(params, "h.", data_format="channels_first")
    y = fun(x.detach())
    assert torch.equal(y, out.detach())
    y.backward(g.permute(0, 3, 1, 2).float().to(DEV))
    _check(params["h.depthwise.weight"].grad, ref[2], "functor grad_dw")
    # activation=None is flag bit 1 off; config round trip; Keras' fixed arguments
    lay = _load(layers.SeparableConv2D(19, 32, activation=None, data_format="channels_last", name="head"), dw, pw, bias)
    plain = _oracle_of(key, (False, False))                                  # differentiates: outside no_grad
    with torch.no_grad():
        _check(lay(xs), plain[0], "no activation out")
    twin = layers.SeparableConv2D.from_config(lay.get_config())
    assert twin.get_config() == lay.get_config() == {"name": "head", "in_channels": 19, "filters": 32,
                                                     "activation": None}
    assert [tuple(p.shape) for p in twin.parameters()] == [tuple(p.shape) for p in lay.parameters()]
    assert sorted(twin.state_dict()) == ["bias", "depthwise.weight", "pointwise.weight"]
    assert float(twin.bias.abs().max()) == 0.0
    lim = (6.0 / (19 + 32)) ** 0.5
    assert 0.5 * lim < float(twin.pointwise.weight.abs().max()) <= lim      # Glorot uniform
    for bad in (dict(kernel_size=5), dict(strides=2), dict(padding="valid"), dict(use_bias=False),
                dict(depth_multiplier=2), dict(activation="relu")):
        with pytest.raises(ValueError):
            layers.SeparableConv2D(19, 32, **bad)
    with pytest.raises(ValueError):
        lay([xs[0]])                                                          # 7 channels into a 19-channel layer


# ---- chain: cost volume -> two layers -> Huber scalar ------------------------------------------------------------------
def _huber_scalar(out, target):
    """FlowMseLossV2's shape of scalar: Huber(0.1) of the scaled 2-channel flow against a target."""
    return torch.nn.functional.huber_loss(0.25 * out[..., :2], 0.25 * target, delta=0.1)


def test_chain_cost_volume_to_loss():
    gen = torch.Generator().manual_seed(9)
    B, H, W, C = 2, 9, 18, 8
    prv, nxt = _grid(gen, (B, H, W, C), 1 / 16), _grid(gen, (B, H, W, C), 1 / 16)
    flo, target = _grid(gen, (B, H, W, 2), 1 / 16), _grid(gen, (B, H, W, 2), 1 / 16)
    w1 = _grid(gen, (91, 1, 3, 3), 1 / 8), _grid(gen, (32, 91), 1 / 8) / 4, _grid(gen, (32,), 1 / 8)
    w2 = _grid(gen, (32, 1, 3, 3), 1 / 8), _grid(gen, (16, 32), 1 / 8) / 4, _grid(gen, (16,), 1 / 8)
    leaves = [t.clone().requires_grad_() for t in (prv, nxt) + w1 + w2]
    cost = torch_ref.cost_volume(leaves[0], leaves[1], 4)
    h = composite((cost, leaves[0], flo), leaves[2], leaves[3], leaves[4], False, True)
    _huber_scalar(composite((h,), leaves[5], leaves[6], leaves[7], False, True), target).backward()
    p, n = prv.float().to(DEV).requires_grad_(), nxt.float().to(DEV).requires_grad_()
    l1 = _load(layers.SeparableConv2D(91, 32, data_format="channels_last"), *w1)
    l2 = _load(layers.SeparableConv2D(32, 16, data_format="channels_last"), *w2)
    cost = layers.CostVolumeV2(4, data_format="channels_last")((p, n))
    out = l2(l1((cost, p, flo.float().to(DEV))))
    loss = _huber_scalar(out, target.float().to(DEV))
    loss.backward()
    _check(p.grad, leaves[0].grad, "grad_prv")
    _check(n.grad, leaves[1].grad, "grad_nxt")
    for lay, k in ((l1, 2), (l2, 5)):
        _check(lay.depthwise.weight.grad, leaves[k].grad, "layer grad_dw")
        _check(lay.pointwise.weight.grad[:, :, 0, 0], leaves[k + 1].grad, "layer grad_pw")
        _check(lay.bias.grad, leaves[k + 2].grad, "layer grad_bias")


# ---- a short training run ----------------------------------------------------------------------------------------------
def train_case():
    """Fixed-seed two-layer stack (5 -> 16 Mish, 16 -> 16 linear), input, target and learning rate."""
    torch.manual_seed(0)
    l1 = layers.SeparableConv2D(5, 16, data_format="channels_last")
    l2 = layers.SeparableConv2D(16, 16, activation=None, data_format="channels_last")
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 9, 12, 5, generator=gen)
    target = torch.randn(2, 9, 12, 16, generator=gen)
    return l1, l2, x, target, 10.0


def train_composite(dtype, steps=5):
    """The same SGD steps on the torch composite in `dtype` on the CPU -> (final parameters, losses)."""
    l1, l2, x, target, lr = train_case()
    ps = [p.detach().to(dtype).clone().requires_grad_() for p in list(l1.parameters()) + list(l2.parameters())]
    x, target = x.to(dtype), target.to(dtype)
    losses = []
    for _ in range(steps):
        # parameter order of the layer: bias, depthwise.weight, pointwise.weight
        h = composite((x,), ps[1], ps[2][:, :, 0, 0], ps[0], False, True)
        loss = torch.nn.functional.mse_loss(composite((h,), ps[4], ps[5][:, :, 0, 0], ps[3], False, False), target)
        losses.append(float(loss.detach()))
        grads = torch.autograd.grad(loss, ps)
        with torch.no_grad():
            for p, gr in zip(ps, grads):
                p -= lr * gr
    return [p.detach() for p in ps], losses


def test_short_training_run():
    """5 SGD steps of the two-layer stack on the HIP layers against the same steps of the float64 composite.
    Measured on the CPU for exactly this case: the fp32 composite ends within 7.1e-8 (max over all parameters) of the
    float64 one (TRAIN_DRIFT; tests/test_sepconv_grad_cpu.py re-measures it); the bound is 10 x that, 7.1e-7
    (TRAIN_BOUND), the margin for reordered fp32 sums across 5 compounding steps."""
    ref, losses = train_composite(torch.float64)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses            # the case really trains
    l1, l2, x, target, lr = train_case()
    assert [n for n, _ in l1.named_parameters()] == ["bias", "depthwise.weight", "pointwise.weight"]
    l1, l2, x, target = l1.to(DEV), l2.to(DEV), x.to(DEV), target.to(DEV)
    ps = list(l1.parameters()) + list(l2.parameters())
    opt = torch.optim.SGD(ps, lr=lr)
    for _ in range(5):
        opt.zero_grad()
        torch.nn.functional.mse_loss(l2(l1(x)), target).backward()
        opt.step()
    worst = max(float((p.detach().double().cpu() - r).abs().max()) for p, r in zip(ps, ref))
    print("final-parameter drift {:.3e}, bound {:.3e}".format(worst, TRAIN_BOUND))
    assert worst <= TRAIN_BOUND, worst


# ---- capture ---------------------------------------------------------------------------------------------------------
def test_grad_path_refuses_capture_and_no_grad_capture_still_works():
    """Under a real capture only the forward-with-grad refusal is exercised: a backward enqueued into a capture once
    took the process down in capture_end, so the backward's refusal is checked on the host, with the
    capture state monkeypatched (tests/test_sepconv_grad_cpu.py::test_the_grad_path_refuses_graph_capture)."""
    srcs, dw, pw, bias, g = _case(2, 16, 32, (32,), 16)
    dev = lambda t: t.float().to(DEV)
    x, w, p, b = dev(srcs[0]), dev(dw), ops.pad_pointwise(dev(pw)), dev(bias)
    with torch.no_grad():
        eager = ops.sepconv3x3([x], w, p, b, True, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        ops.sepconv3x3([x], w, p, b, True, True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        static = ops.sepconv3x3([x], w, p, b, True, True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    xg = x.clone().requires_grad_()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph2):
            ops.sepconv3x3([xg], w, p * 1.0, b, True, True)
    torch.cuda.synchronize()

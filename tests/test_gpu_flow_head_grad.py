"""GPU suite of the trainable flow estimator: the flow head's training-mode BatchNorm (qpwc_flow_head_stats_fwd), its
backward in both BatchNorm modes (qpwc_flow_head_bwd), the Upsample adjoint (qpwc_upsample2x_flow_bwd), all behind
torch autograd, and layers.OptFlow / Upsample / Flow / UpFlow.

Oracle: torch autograd in float64 on the CPU of oracle.torch_ref.mish + F.conv2d + BatchNorm written out by hand
(mean, var(unbiased=False), moving = moving * momentum + batch * (1 - momentum)); in inference mode that is
oracle.torch_ref.flow_head itself.  Upsample: F.interpolate(scale_factor=2, 'bilinear', align_corners=False) * scale.
Inputs and grad_out are multiples of 1/16 in [-1, 1], weights multiples of 1/8.  Tolerance: the project's
1e-4 * max(1, max|ref|) per tensor."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref
from qpwcnet_amd import layers, loss, non_layers, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS, MOMENTUM = 1e-3, 0.99
SCALE = 2.0
SHAPES = [(2, 1, 1), (3, 16, 16), (2, 19, 37)]   # every halo pixel outside; exactly one tile; partial tiles on both axes
# (B, H, W) at which every grid-stride loop of csrc/flow_head_bwd.hip makes two trips or more with an uneven last one:
# 3 x 14 x 13 = 546 tiles over 512 workgroups, 7794 groups of 16 pixels over 1024 waves, 124701 pixels over 65536
# threads of the Upsample adjoint (tests/test_flow_head_grad_cpu.py checks it against the constants)
MULTI_TRIP = (3, 211, 197)
# the 5-step training case: fp32-vs-float64 drift of the CPU composite and the bound derived from it (see the test)
TRAIN_DRIFT = 1.8e-7
TRAIN_BOUND = 10 * TRAIN_DRIFT
NAMES = ("z", "w1", "b1", "gamma", "beta", "wf")


def _grid(gen, shape, step, lo=-1.0, hi=1.0):
    return torch.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape, generator=gen).to(torch.float64) * step


def _tol(ref):
    return 1e-4 * max(1.0, float(ref.abs().max()))


def _check(got, ref, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    d = float((got - ref).abs().max())
    print("{}: max|d| = {:.3e}, bound {:.3e}".format(what, d, _tol(ref)))
    assert d <= _tol(ref), "{}: max|d| = {:.3e} > {:.3e}".format(what, d, _tol(ref))


# ---- the oracle composite ------------------------------------------------------------------------------------------------
def head_composite(z, w1, b1, gamma, beta, mean, var, wf, scale, training, eps=EPS, momentum=MOMENTUM):
    """The flow head as torch ops in the dtype of its operands -> (flow (B,H,W,2), new moving mean, new moving var).
    z (B,H,W,16), w1 (16,16,1,1), wf (2,16,3,3); training: BatchNorm by hand on the batch statistics."""
    if not training:
        return torch_ref.flow_head(z, w1, b1, gamma, beta, mean, var, eps, wf, scale), mean, var
    u = torch_ref.mish(F.conv2d(torch_ref.mish(z).permute(0, 3, 1, 2), w1, b1))
    bm, bv = u.mean(dim=(0, 2, 3)), u.var(dim=(0, 2, 3), unbiased=False)
    h = (u - bm.view(1, -1, 1, 1)) / torch.sqrt(bv.view(1, -1, 1, 1) + eps) * gamma.view(1, -1, 1, 1) \
        + beta.view(1, -1, 1, 1)
    f = F.conv2d(h, wf, None, padding=1)
    return (scale * f).permute(0, 2, 3, 1), (mean * momentum + bm.detach() * (1 - momentum)), \
        (var * momentum + bv.detach() * (1 - momentum))


def sepconv_composite(sources, dw, pw, bias, on_store):
    z = torch_ref.depthwise3x3(sources, dw) @ pw.reshape(pw.shape[0], -1).t() + bias
    return torch_ref.mish(z) if on_store else z


def upsample_composite(x, scale):
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1) * scale


@functools.lru_cache(maxsize=None)
def _case(B, H, W, seed=0, offset=False):
    """(z, w1, b1, gamma, beta, mean, var, wf, g) on the grids.  offset: b1 = +8 and a small spread of a around it."""
    gen = torch.Generator().manual_seed(seed)
    z = _grid(gen, (B, H, W, 16), 1 / 16)
    w1, b1 = _grid(gen, (16, 16, 1, 1), 1 / 8), _grid(gen, (16,), 1 / 8)
    gamma, beta, mean = _grid(gen, (16,), 1 / 8), _grid(gen, (16,), 1 / 8), _grid(gen, (16,), 1 / 8)
    var = _grid(gen, (16,), 1 / 8, 1 / 8, 2.0)
    wf, g = _grid(gen, (2, 16, 3, 3), 1 / 8), _grid(gen, (B, H, W, 2), 1 / 16)
    if offset:
        w1 = _grid(gen, (16, 16, 1, 1), 1 / 8, -1 / 8, 1 / 8)
        b1 = torch.full((16,), 8.0, dtype=torch.float64)
    return z, w1, b1, gamma, beta, mean, var, wf, g


def _oracle(case, training, scale=SCALE):
    """-> (out, new mean, new var, [grads of z, w1, b1, gamma, beta, wf])."""
    z, w1, b1, gamma, beta, mean, var, wf, g = case
    leaves = [t.clone().requires_grad_() for t in (z, w1, b1, gamma, beta)] + [wf.clone().requires_grad_()]
    out, nm, nv = head_composite(*leaves[:5], mean, var, leaves[5], scale, training)
    out.backward(g)
    return out.detach(), nm.detach(), nv.detach(), [t.grad for t in leaves]


@functools.lru_cache(maxsize=None)
def _oracle_of(key, training):
    return _oracle(_case(*key), training)


def _dev(t):
    return t.float().to(DEV)


def _hip(case, training, scale=SCALE):
    """Forward + backward through autograd -> (out, moving mean, moving var, [grads])."""
    z, w1, b1, gamma, beta, mean, var, wf, g = case
    leaves = [_dev(t).requires_grad_() for t in (z, w1, b1, gamma, beta, wf)]
    mm, mv = _dev(mean), _dev(var)
    out = ops.flow_head_train(*leaves[:5], mm, mv, leaves[5], scale, training=training, momentum=MOMENTUM, eps=EPS)
    out.backward(_dev(g))
    return out, mm, mv, [t.grad for t in leaves]


def _compare(case, ref, training, tag=""):
    out, mm, mv, grads = _hip(case, training)
    _check(out, ref[0], tag + "out")
    _check(mm, ref[1], tag + "moving mean")
    _check(mv, ref[2], tag + "moving var")
    for name, got, want in zip(NAMES, grads, ref[3]):
        _check(got, want, tag + "grad_" + name)
    return out, grads


# ---- the head, both BatchNorm modes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("training", [False, True], ids=["frozen", "batch"])
def test_head_forward_and_six_gradients(shape, training):
    _compare(_case(*shape), _oracle_of(shape, training), training)


def test_head_inference_single_pixel():
    _compare(_case(1, 1, 1), _oracle_of((1, 1, 1), False), False)


def test_inference_mode_leaves_the_moving_statistics_alone():
    case = _case(2, 19, 37)
    _, mm, mv, _ = _hip(case, False)
    assert torch.equal(mm, _dev(case[5])) and torch.equal(mv, _dev(case[6]))


def test_offset_case_large_mean_small_spread():
    """b1 = +8 and W1 in {-1/8, 0, 1/8}: u is about 8 with a standard deviation below 0.25.  A sum u^2 - mean^2 in
    fp32 carries the rounding of sums near 64 M = 9e4 (ulp 0.008) into a variance of a few 1e-2, parts in a thousand of
    rstd^2 and of every gradient through it; the shifted sums do not.  grad_b1 is here a sum of M terms
    of size rstd gamma |gh| (about 15) that cancels to about 1e-4, because Mish'(8) - 1 is 1e-6."""
    key = (2, 19, 37, 7, True)
    ref = _oracle_of(key, True)
    u = torch_ref.mish(F.conv2d(torch_ref.mish(_case(*key)[0]).permute(0, 3, 1, 2), _case(*key)[1], _case(*key)[2]))
    spread = float(u.var(dim=(0, 2, 3), unbiased=False).max())
    assert float(u.mean()) > 7.5 and spread < 0.0625, (float(u.mean()), spread)
    _compare(_case(*key), ref, True, "offset ")
    # the statistics themselves
    z, w1, b1, gamma, beta, mean, var, wf, g = (_dev(t) for t in _case(*key))
    _, stats = ops.flow_head_stats(z, w1, b1, gamma, beta, None, None, wf, MOMENTUM, EPS)
    _check(stats[:16], u.mean(dim=(0, 2, 3)), "batch mean")
    _check(stats[16:32], u.var(dim=(0, 2, 3), unbiased=False), "batch variance")


# ---- only what is asked ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [False, True], ids=["frozen", "batch"])
def test_only_what_is_asked(training):
    z, w1, b1, gamma, beta, mean, var, wf, g = (_dev(t) for t in _case(2, 19, 37))
    if training:
        params, stats = ops.flow_head_stats(z, w1, b1, gamma, beta, None, None, wf, MOMENTUM, EPS)
    else:
        params, stats = ops.pack_flow_head(w1, b1, gamma, beta, mean, var, EPS, wf), ops.frozen_stats(mean, var)
    full = ops.flow_head_bwd(z, params, stats, SCALE, g, training, EPS)
    assert all(t is not None for t in full)
    for i, name in enumerate(NAMES):
        need = tuple(k == i for k in range(6))
        one = ops.flow_head_bwd(z, params, stats, SCALE, g, training, EPS, need)
        assert [t is not None for t in one] == list(need), name
        assert torch.equal(one[i], full[i]), name
    # through autograd: a leaf that does not require grad gets none, its neighbours the same bits
    zz, bb = z.clone().requires_grad_(), beta.clone().requires_grad_()
    ops.flow_head_train(zz, w1, b1, gamma, bb, mean.clone(), var.clone(), wf, SCALE, training=training,
                        momentum=MOMENTUM, eps=EPS).backward(g)
    assert torch.equal(zz.grad, full[0]) and torch.equal(bb.grad, full[4])


# ---- large arguments -------------------------------------------------------------------------------------------------------
def test_large_arguments_stay_finite():
    z, w1, b1, gamma, beta, mean, var, wf, g = _case(2, 9, 18, 3)
    z, b1 = z.clone(), b1.clone()
    flat = z.view(-1)
    flat[5], flat[77], flat[1201], flat[4003] = 40.0, -40.0, 100.0, -100.0
    b1[1], b1[2], b1[7], b1[12] = 40.0, -40.0, 100.0, -100.0
    case = (z, w1, b1, gamma, beta, mean, var, wf, g)
    _compare(case, _oracle(case, False), False, "frozen ")
    _compare(case, _oracle(case, True), True, "batch ")


# ---- determinism, batch independence, forward bits -----------------------------------------------------------------------------
@pytest.mark.parametrize("training", [False, True], ids=["frozen", "batch"])
def test_bitwise_determinism(training):
    case = _case(3, 19, 37, 5)
    a, b = _hip(case, training), _hip(case, training)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)


def test_inference_grad_z_is_batch_independent():
    z, w1, b1, gamma, beta, mean, var, wf, g = (_dev(t) for t in _case(3, 19, 37, 5))
    params, stats = ops.pack_flow_head(w1, b1, gamma, beta, mean, var, EPS, wf), ops.frozen_stats(mean, var)
    need = (True, False, False, False, False, False)
    batch = ops.flow_head_bwd(z, params, stats, SCALE, g, False, EPS, need)[0]
    alone = ops.flow_head_bwd(z[:1].contiguous(), params, stats, SCALE, g[:1].contiguous(), False, EPS, need)[0]
    assert torch.equal(alone[0], batch[0])


def test_forward_bits_and_no_grad_fn_without_grad():
    z, w1, b1, gamma, beta, mean, var, wf, g = (_dev(t) for t in _case(2, 19, 37))
    params = non_layers.pack_flow_head(w1, b1, gamma, beta, mean, var, EPS, wf)
    with torch.no_grad():
        plain = ops.flow_head(z, params, SCALE)
        up = ops.upsample2x_flow(plain, 2.0)
    assert plain.grad_fn is None and up.grad_fn is None
    assert ops.flow_head_train(z, w1, b1, gamma, beta, mean, var, wf, SCALE).grad_fn is None   # nothing requires grad
    out = ops.flow_head_train(z.clone().requires_grad_(), w1, b1, gamma, beta, mean, var, wf, SCALE, training=False)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    with torch.no_grad():
        assert ops.upsample2x_flow(out, 2.0).grad_fn is None
    up_g = ops.upsample2x_flow(out, 2.0)
    assert up_g.grad_fn is not None and torch.equal(up_g.detach(), up)
    assert non_layers.Upsample(2.0, data_format="channels_last")(out).grad_fn is not None


# ---- more than one trip of every grid-stride loop --------------------------------------------------------------------------------
def test_more_than_one_trip():
    case = _case(*MULTI_TRIP, 11)
    _compare(case, _oracle(case, True), True)
    g = _grid(torch.Generator().manual_seed(12), (MULTI_TRIP[0], 2 * MULTI_TRIP[1], 2 * MULTI_TRIP[2], 2), 1 / 16)
    assert torch.equal(ops.upsample2x_flow_bwd(_dev(g), 2.0).double().cpu(), _upsample_oracle(g, MULTI_TRIP, 2.0))


# ---- Upsample ------------------------------------------------------------------------------------------------------------------
def _upsample_oracle(g, shape, scale):
    x = torch.zeros(shape + (2,), dtype=torch.float64, requires_grad=True)
    upsample_composite(x, scale).backward(g)
    return x.grad


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (2, 33, 65)], ids=lambda s: "x".join(map(str, s)))
def test_upsample_backward_is_exact_on_the_grid(shape, scale):
    """Every weight (1/16, 3/16, 9/16, times scale) is a dyadic rational and g a multiple of 2^-4: each term and each
    partial sum is a multiple of 2^-8 below 2^3, an fp32 value, so any summation order gives the float64 result."""
    B, h, w = shape
    gen = torch.Generator().manual_seed(h)
    g = _grid(gen, (B, 2 * h, 2 * w, 2), 1 / 16)
    x = _dev(_grid(gen, (B, h, w, 2), 1 / 16)).requires_grad_()
    out = ops.upsample2x_flow(x, scale)
    assert torch.equal(out.detach().double().cpu(), upsample_composite(x.detach().double().cpu(), scale))
    out.backward(_dev(g))
    assert torch.equal(x.grad.double().cpu(), _upsample_oracle(g, shape, scale))
    # channels_first in and out: the same numbers through the permuted views
    xc = x.detach().permute(0, 3, 1, 2).contiguous().requires_grad_()
    ops.upsample2x_flow(xc, scale, "channels_first", "channels_first").backward(_dev(g).permute(0, 3, 1, 2))
    assert torch.equal(xc.grad.permute(0, 2, 3, 1), x.grad)


# ---- the layers ------------------------------------------------------------------------------------------------------------------
def _optflow_state(gen, c_in):
    """A state dict under the names of weights.py for OptFlow(c_in), on the grids (small pointwise kernels)."""
    sd, chans = {}, (c_in, 128, 64, 32, 16)
    for i in range(4):
        sd["feat.%d.depthwise.weight" % i] = _grid(gen, (chans[i], 1, 3, 3), 1 / 8).float()
        sd["feat.%d.pointwise.weight" % i] = (_grid(gen, (chans[i + 1], chans[i], 1, 1), 1 / 8) / 8).float()
        sd["feat.%d.bias" % i] = _grid(gen, (chans[i + 1],), 1 / 8).float()
    sd["conv.weight"], sd["conv.bias"] = _grid(gen, (16, 16, 1, 1), 1 / 8).float(), _grid(gen, (16,), 1 / 8).float()
    sd["norm.gamma"], sd["norm.beta"] = _grid(gen, (16,), 1 / 8).float(), _grid(gen, (16,), 1 / 8).float()
    sd["norm.mean"], sd["norm.var"] = _grid(gen, (16,), 1 / 8).float(), _grid(gen, (16,), 1 / 8, 1 / 8, 2.0).float()
    sd["flow.weight"] = _grid(gen, (2, 16, 3, 3), 1 / 8).float()
    return sd


def test_layer_surface():
    from qpwcnet_amd import weights
    gen = torch.Generator().manual_seed(21)
    sd = _optflow_state(gen, 19)
    names = sorted(n[len("flow.flow."):] for n in weights.keras_variable_names() if n.startswith("flow.flow."))
    assert sorted(sd) == names
    lay = layers.OptFlow(19, data_format="channels_last")
    lay.load_state_dict(sd)                                              # strict: every name, nothing else
    assert sorted(lay.state_dict()) == names
    assert all(torch.equal(v, sd[k]) for k, v in lay.state_dict().items())
    assert sorted(n for n, _ in lay.named_buffers()) == ["norm.mean", "norm.var"]
    lay = lay.to(DEV).eval()
    srcs = [_dev(_grid(gen, (2, 9, 14, c), 1 / 16)) for c in (7, 10, 2)]
    # eval() against the functor on the same parameters (its own kernels' choice of launches), and the float64 oracle
    fun = non_layers.OptFlow({"p." + k: v.to(DEV) for k, v in sd.items()}, "p.", data_format="channels_last")
    with torch.no_grad():
        want, got = fun.from_sources(srcs), lay(srcs)
    assert got.shape == (2, 9, 14, 2)
    _check(got, want.double().cpu(), "eval vs functor")
    # channels_first agrees with channels_last, forward and gradients, in training mode
    cl = layers.OptFlow(19, scale=3.0, data_format="channels_last")
    cf = layers.OptFlow(19, scale=3.0, data_format="channels_first")
    cl.load_state_dict(sd), cf.load_state_dict(sd)
    cl, cf = cl.to(DEV).train(), cf.to(DEV).train()
    x = torch.cat(srcs, dim=3).requires_grad_()
    xc = x.detach().permute(0, 3, 1, 2).contiguous().requires_grad_()
    g = _dev(_grid(gen, (2, 9, 14, 2), 1 / 16))
    a, b = cl(x), cf(xc)
    assert b.shape == (2, 2, 9, 14)
    a.backward(g), b.backward(g.permute(0, 3, 1, 2))
    _check(b.permute(0, 2, 3, 1), a.detach().double().cpu(), "channels_first out")
    _check(xc.grad.permute(0, 2, 3, 1), x.grad.double().cpu(), "channels_first grad_x")
    for (n, p), (_, q) in zip(cl.named_parameters(), cf.named_parameters()):
        _check(q.grad, p.grad.double().cpu(), "channels_first grad " + n)
    _check(cf.norm.mean, cl.norm.mean.double().cpu(), "channels_first moving mean")
    assert not torch.equal(cl.norm.var.cpu(), sd["norm.var"])            # training mode moved the buffers
    twin = layers.OptFlow.from_config(cl.get_config())
    assert twin.get_config() == cl.get_config() == {"name": None, "in_channels": 19, "filters": (128, 64, 32, 16),
                                                    "scale": 3.0}


# ---- chain: Flow -> Upsample -> UpFlow -> multiscale loss ------------------------------------------------------------------------
def chain_case():
    """Fixed-seed Flow(32) / UpFlow(32) with Keras' initialisers, frozen random features at 8 x 12 and 16 x 24, the
    ground truth at 32 x 48, and the learning rate of the training run."""
    torch.manual_seed(0)
    flow = layers.Flow(32, data_format="channels_last")
    upflow = layers.UpFlow(32, data_format="channels_last")
    gen = torch.Generator().manual_seed(1)
    feats = [torch.randn(2, h, w, 32, generator=gen) for h, w in ((8, 12), (8, 12), (16, 24), (16, 24))]
    gt = torch.randn(2, 32, 48, 2, generator=gen) * 4.0
    return flow, upflow, feats, gt, 1.0


def optflow_composite(P, prefix, sources, training):
    """layers.OptFlow from a {name: tensor} dict P (parameters and buffers) -> flow; moving buffers replaced in P."""
    x = list(sources)
    for i in range(4):
        x = [sepconv_composite(x, P[prefix + "feat.%d.depthwise.weight" % i], P[prefix + "feat.%d.pointwise.weight" % i],
                               P[prefix + "feat.%d.bias" % i], i < 3)]
    z = x[0]
    scale = float(z.shape[1] ** 2 + z.shape[2] ** 2) ** 0.5
    out, nm, nv = head_composite(z, P[prefix + "conv.weight"], P[prefix + "conv.bias"], P[prefix + "norm.gamma"],
                                 P[prefix + "norm.beta"], P[prefix + "norm.mean"], P[prefix + "norm.var"],
                                 P[prefix + "flow.weight"], scale, training)
    P[prefix + "norm.mean"], P[prefix + "norm.var"] = nm, nv
    return out


def flow_mse_v2_composite(gt, pred):
    """FlowMseLossV2 of one level in the dtype of its operands (tests/test_loss_cpu.py::torch_ops_loss, 'v2')."""
    H, W, h, w = gt.shape[1], gt.shape[2], pred.shape[1], pred.shape[2]
    g = F.avg_pool2d(gt.permute(0, 3, 1, 2), (H // h, W // w)) * (h / H)
    s = 2.0 / (w + h)
    return F.huber_loss(s * pred.permute(0, 3, 1, 2), s * g, delta=0.1)


def chain_composite(P, feats, gt, training=True):
    """Flow -> Upsample(2.0) -> UpFlow -> sum of FlowMseLossV2 over both levels, as torch ops on the CPU."""
    f0 = optflow_composite(P, "f.flow.", (torch_ref.cost_volume(feats[0], feats[1], 4), feats[0], feats[1]), training)
    up = upsample_composite(f0, 2.0)
    cost = torch_ref.cost_volume(feats[2], torch_ref.warp_v2(feats[3], up), 4)
    f1 = optflow_composite(P, "u.flow.", (cost, feats[2], up), training)
    return flow_mse_v2_composite(gt, f0) + flow_mse_v2_composite(gt, f1)


def chain_state(flow, upflow, dtype):
    P = {"f." + k: v.detach().to(dtype).clone() for k, v in flow.state_dict().items()}
    P.update({"u." + k: v.detach().to(dtype).clone() for k, v in upflow.state_dict().items()})
    names = ["f." + n for n, _ in flow.named_parameters()] + ["u." + n for n, _ in upflow.named_parameters()]
    for n in names:
        P[n].requires_grad_()
    return P, names


def chain_hip(flow, upflow, feats, gt):
    f0 = flow((feats[0], feats[1]))
    f1 = upflow((feats[2], feats[3], layers.Upsample(2.0, data_format="channels_last")(f0)))
    return loss.multiscale(loss.FlowMseLossV2(), gt, [f0, f1])[0]


def test_chain_flow_upsample_upflow_loss():
    flow, upflow, feats, gt, _ = chain_case()
    P, names = chain_state(flow, upflow, torch.float64)
    fr = [t.double().requires_grad_() for t in feats]
    ref = chain_composite(P, fr, gt.double())
    ref.backward()
    flow, upflow = flow.to(DEV).train(), upflow.to(DEV).train()
    fh = [t.to(DEV).requires_grad_() for t in feats]
    total = chain_hip(flow, upflow, fh, gt.to(DEV))
    total.backward()
    _check(total, ref.detach(), "loss")
    got = dict([("f." + n, p) for n, p in flow.named_parameters()] + [("u." + n, p) for n, p in upflow.named_parameters()])
    for n in names:
        _check(got[n].grad, P[n].grad, "grad " + n)
    for i in range(4):
        _check(fh[i].grad, fr[i].grad, "grad features %d" % i)
    for n, b in list(flow.named_buffers(prefix="f")) + list(upflow.named_buffers(prefix="u")):
        _check(b, P[n].detach(), "moving " + n)


# ---- a short training run ----------------------------------------------------------------------------------------------------
def train_composite(dtype, steps=5):
    """5 SGD steps of the chain on the torch composite in `dtype` on the CPU -> ({name: final parameter}, losses)."""
    flow, upflow, feats, gt, lr = chain_case()
    P, names = chain_state(flow, upflow, dtype)
    feats, gt = [t.to(dtype) for t in feats], gt.to(dtype)
    losses = []
    for _ in range(steps):
        total = chain_composite(P, feats, gt)
        losses.append(float(total.detach()))
        grads = torch.autograd.grad(total, [P[n] for n in names])
        with torch.no_grad():
            for n, gr in zip(names, grads):
                P[n] -= lr * gr
    return {n: P[n].detach() for n in names}, losses


def test_short_training_run():
    """5 SGD steps of Flow -> Upsample -> UpFlow -> multiscale FlowMseLossV2 in training mode on the HIP layers against
    the same steps of the float64 composite.  Measured on the CPU for exactly this case: the fp32 composite ends within
    TRAIN_DRIFT (max over all parameters) of the float64 one (tests/test_flow_head_grad_cpu.py re-measures it); the
    bound is 10 x that (TRAIN_BOUND), the margin for reordered fp32 sums across 5 compounding steps, derived as
    TRAIN_DRIFT / TRAIN_BOUND of tests/test_gpu_sepconv_grad.py."""
    ref, losses = train_composite(torch.float64)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses            # the case really trains
    flow, upflow, feats, gt, lr = chain_case()
    flow, upflow = flow.to(DEV).train(), upflow.to(DEV).train()
    feats, gt = [t.to(DEV) for t in feats], gt.to(DEV)
    opt = torch.optim.SGD(list(flow.parameters()) + list(upflow.parameters()), lr=lr)
    for _ in range(5):
        opt.zero_grad()
        chain_hip(flow, upflow, feats, gt).backward()
        opt.step()
    got = dict([("f." + n, p) for n, p in flow.named_parameters()] + [("u." + n, p) for n, p in upflow.named_parameters()])
    worst = max(float((got[n].detach().double().cpu() - r).abs().max()) for n, r in ref.items())
    print("final-parameter drift {:.3e}, bound {:.3e}".format(worst, TRAIN_BOUND))
    assert worst <= TRAIN_BOUND, worst


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_grad_path_refuses_capture_and_no_grad_capture_still_works():
    """Under a real capture only the forward-with-grad refusals are exercised (a backward enqueued into a capture once
    took the process down); the backward's refusal is checked on the host
    (tests/test_flow_head_grad_cpu.py)."""
    z, w1, b1, gamma, beta, mean, var, wf, g = (_dev(t) for t in _case(2, 19, 37))
    run = lambda: ops.upsample2x_flow(ops.flow_head_train(z, w1, b1, gamma, beta, mean, var, wf, SCALE), 2.0)
    with torch.no_grad():
        eager = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        static = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    zg, fg = z.clone().requires_grad_(), eager.clone().requires_grad_()
    for fn in (lambda: ops.flow_head_train(zg, w1, b1, gamma, beta, mean, var, wf, SCALE),
               lambda: ops.upsample2x_flow(fg, 2.0)):
        graph2 = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="cannot be captured"):
            with torch.cuda.graph(graph2):
                fn()
        torch.cuda.synchronize()

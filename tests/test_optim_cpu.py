"""The trainer's update step (qpwcnet_amd/optim.py) against its definition, on the CPU.

The definition is restated here in float64 numpy (``oracle_*``): the AGC units of core/agc.py on the torch layouts, the
clip of agc.py:39-49 with TF's NaN behaviour, and the dense update of tf.keras.optimizers.Adam.  Keras casts the
hyperparameters to the variable's dtype, so the oracle computes in float64 with the float32 roundings of beta_1,
beta_2, epsilon, clip_factor and eps -- the numbers an fp32 implementation is given.

``optim.step_torch`` (the CPU path) is held to the oracle here; tests/test_gpu_optim.py holds the HIP kernel to the same
oracle, on the same case set, with the same bounds.  The C boundary's validation is in tests/test_optim_capi_cpu.py.
"""
import math
import os

import numpy as np
import pytest
import torch

from qpwcnet_amd import _hip, optim, weights
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

OPTIM_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qpwc_optim.h")

LR, BETA_1, BETA_2, EPSILON, CLIP, AGC_EPS = 1e-4, 0.9, 0.999, 1e-7, 0.01, 1e-3
STEPS = 3

# ---- tolerances ------------------------------------------------------------------------------------------------------
# Measured, not guessed: the largest error of optim.step_torch in fp32 on the CPU against the float64 oracle over the
# 3 steps of both case sets below, with and without clipping (test_step_torch_matches_the_oracle prints the figures):
#     p   absolute                                   3.9e-08   (p is up to ~0.45 here: about half an ulp of it per step)
#     m   relative to the largest |m| of its unit    4.7e-07   (the one-element units of s.weight: per element)
#     v   relative to the largest |v| of its unit    2.9e-07
# (m and v are divided by their unit's largest reference magnitude, not element by element: an element of m that
# cancels to nearly zero over the steps carries the rounding of its terms, not of itself.)
# The bound for BOTH fp32 implementations is 4 x that: the kernel's sums of squares run in another order (per-lane
# partial sums and a butterfly) than torch's.  It is not derived from the kernel's output.
MEASURED_P_ABS, MEASURED_M_REL, MEASURED_V_REL = 3.9e-8, 4.7e-7, 2.9e-7
P_BOUND, M_BOUND, V_BOUND = 4 * MEASURED_P_ABS, 4 * MEASURED_M_REL, 4 * MEASURED_V_REL

# ---- the case set (shared with tests/test_gpu_optim.py) --------------------------------------------------------------
CASE_SMALL = [
    ("a.weight", (4, 256, 3, 3)),               # the longest unit of the models: 2304 floats
    ("dec.0.conv_up.weight", (4, 128, 4, 4)),   # Conv2DTranspose: 4 units of 2048 floats, per INPUT channel
    ("f.depthwise.weight", (115, 1, 3, 3)),     # one unit of 1035 floats: odd length
    ("f.pointwise.weight", (8, 115, 1, 1)),     # 115-float rows: units that do not start on 16 bytes
    ("f.bias", (8,)),                           # zeros: pn = 0, the eps floor
    ("g.bias", (1,)),
    ("h.bias", (5000,)),                        # a unit longer than any in the models
]
# more units than the kernel has waves in its capped grid (1024 workgroups x 4), so that its grid-stride loop iterates
CASE_STRIDED = CASE_SMALL + [("s.weight", (4200, 1, 1, 1))]
CASES = {"small": CASE_SMALL, "strided": CASE_STRIDED}
ZERO = "f.bias"


def _f32(x):
    return float(np.float32(x))


# ---- the float64 oracle ----------------------------------------------------------------------------------------------
def oracle_units(name, shape):
    """The unit table of the definition, written out from the Keras rule (not through optim.agc_units)."""
    n = int(np.prod(shape))
    if len(shape) <= 1 or name.endswith("depthwise.weight"):
        return [(0, n)]
    row = n // shape[0]         # Conv2D / pointwise: per [o]; conv_up (I,O,kh,kw): per [i]
    return [(k * row, row) for k in range(shape[0])]


def oracle_unit_norms(name, p, g, clip=CLIP, eps=AGC_EPS):
    """[(offset, length, gn, mx)] per unit, float64."""
    pf, gf = np.asarray(p, np.float64).ravel(), np.asarray(g, np.float64).ravel()
    out = []
    for off, ln in oracle_units(name, p.shape):
        pn = math.sqrt(float(np.sum(pf[off:off + ln] ** 2)))
        gn = math.sqrt(float(np.sum(gf[off:off + ln] ** 2)))
        mx = float(np.maximum(pn, _f32(eps))) * _f32(clip)      # np.maximum propagates NaN as tf.maximum does
        out.append((off, ln, gn, mx))
    return out


def oracle_clip(name, p, g, clip=CLIP, eps=AGC_EPS):
    out = np.asarray(g, np.float64).copy().ravel()
    for off, ln, gn, mx in oracle_unit_norms(name, p, g, clip, eps):
        if not gn < mx:                                         # a NaN comparison selects the clipped branch
            out[off:off + ln] *= mx / float(np.maximum(gn, 1e-6))
    return out.reshape(np.shape(g))


def oracle_alpha(lr, t, beta_1=BETA_1, beta_2=BETA_2):
    return lr * math.sqrt(1.0 - _f32(beta_2) ** t) / (1.0 - _f32(beta_1) ** t)


def oracle_step(state, grads, clip=CLIP, lr=LR):
    """One update of state = {"p", "m", "v": {name: float64 array}, "t": updates done}, in place.  A None gradient
    leaves its tensor alone."""
    with np.errstate(invalid="ignore"):
        state["t"] += 1
        alpha = oracle_alpha(lr, state["t"])
        for name, g in grads.items():
            if g is None:
                continue
            p, m, v = state["p"][name], state["m"][name], state["v"][name]
            g = oracle_clip(name, p, g, clip) if clip else np.asarray(g, np.float64)
            m += (g - m) * (1.0 - _f32(BETA_1))
            v += (g * g - v) * (1.0 - _f32(BETA_2))
            p -= alpha * m / (np.sqrt(v) + _f32(EPSILON))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def make_params(case, seed=0):
    """{name: float32 array}: N(0, 0.1) parameters, the zero-initialised bias as zeros."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in CASES[case]:
        out[name] = (rng.standard_normal(shape) * 0.1).astype(np.float32)
    out[ZERO][...] = 0.0
    return out


def make_grads(case, p64, seed):
    """{name: float32 array}: random gradients with every unit scaled so that gn / mx is exactly 0.25 or 4, alternating
    over the units (4 for the zero bias, which must come out clipped): no unit sits near the clip threshold, where a
    last-bit difference of a norm would pick the other branch."""
    rng = np.random.default_rng(seed)
    out, k = {}, 0
    for name, shape in CASES[case]:
        g = rng.standard_normal(shape).ravel()
        for off, ln, gn, mx in oracle_unit_norms(name, p64[name], g.reshape(shape)):
            ratio = 4.0 if name == ZERO else (0.25, 4.0)[k % 2]
            g[off:off + ln] *= ratio * mx / gn
            k += 1
        out[name] = g.reshape(shape).astype(np.float32)
    return out


def assert_clear_of_threshold(case, p64, grads):
    """In the float64 oracle no unit lies within 1e-3 relative of its clip threshold; none is left out."""
    n = 0
    for name, shape in CASES[case]:
        for _, _, gn, mx in oracle_unit_norms(name, p64[name], grads[name]):
            assert abs(gn / mx - 1.0) > 1e-3, (name, gn, mx)
            assert min(abs(gn / mx - 0.25), abs(gn / mx - 4.0)) < 1e-5, (name, gn / mx)
            n += 1
    assert n == sum(len(oracle_units(nm, sh)) for nm, sh in CASES[case])


_TRAJECTORIES = {}


def trajectory(case, clip=CLIP):
    """(initial float32 parameters, [float32 gradients of each step], oracle state after each step), computed once
    per (case, clip) and shared; callers must not modify it.  The gradients of a step are scaled against the oracle's
    parameters before that step, and are the same with and without clipping."""
    key = (case, clip)
    if key not in _TRAJECTORIES:
        p0 = make_params(case)
        if clip != CLIP:
            _, grads, _ = trajectory(case, CLIP)
        else:
            ref = {"p": {n: a.astype(np.float64) for n, a in p0.items()}, "t": 0}
            ref["m"] = {n: np.zeros_like(a) for n, a in ref["p"].items()}
            ref["v"] = {n: np.zeros_like(a) for n, a in ref["p"].items()}
            grads = []
            for k in range(STEPS):
                grads.append(make_grads(case, ref["p"], seed=100 + k))
                assert_clear_of_threshold(case, ref["p"], grads[-1])
                oracle_step(ref, grads[-1], CLIP)
        state = {"p": {n: a.astype(np.float64) for n, a in p0.items()}, "t": 0}
        state["m"] = {n: np.zeros_like(a) for n, a in state["p"].items()}
        state["v"] = {n: np.zeros_like(a) for n, a in state["p"].items()}
        after = []
        for k in range(STEPS):
            oracle_step(state, grads[k], clip)
            after.append({key_: ({n: a.copy() for n, a in val.items()} if isinstance(val, dict) else val)
                          for key_, val in state.items()})
        _TRAJECTORIES[key] = (p0, grads, after)
    return _TRAJECTORIES[key]


def make_optimizer(case, p0, device="cpu", clip=CLIP, lr=LR):
    named = [(n, torch.nn.Parameter(torch.from_numpy(p0[n].copy()).to(device))) for n, _ in CASES[case]]
    return optim.KerasAdamAGC(named, lr=lr, clip_factor=clip), named


def set_grads(named, grads):
    for n, p in named:
        g = grads[n]
        p.grad = None if g is None else torch.from_numpy(np.ascontiguousarray(g)).to(p.device)


def errors(case, named, opt, ref, skip=()):
    """(max |p - ref| ; max over units of max |m - ref| / max |ref| ; the same for v) of an optimiser's tensors against
    an oracle state.  NaN must sit exactly where the oracle has it (such elements then count as equal).  Units listed
    in ``skip`` as (name, unit index) are left out."""
    worst = [0.0, 0.0, 0.0]
    shapes = dict(CASES[case])
    for n, p in named:
        have = (p.detach().cpu().numpy().astype(np.float64).ravel(),
                opt.state[p]["m"].cpu().numpy().astype(np.float64).ravel(),
                opt.state[p]["v"].cpu().numpy().astype(np.float64).ravel())
        want = (ref["p"][n].ravel(), ref["m"][n].ravel(), ref["v"][n].ravel())
        for u, (off, ln) in enumerate(oracle_units(n, shapes[n])):
            if (n, u) in skip:
                continue
            for k in range(3):
                h, w = have[k][off:off + ln], want[k][off:off + ln]
                assert np.array_equal(np.isnan(h), np.isnan(w)), (n, u, "pmv"[k])
                d = float(np.nanmax(np.abs(h - w), initial=0.0))
                if k:
                    scale = float(np.nanmax(np.abs(w), initial=0.0))
                    d = (0.0 if d == 0.0 else math.inf) if scale == 0.0 else d / scale
                worst[k] = max(worst[k], d)
    return tuple(worst)


def assert_within_bounds(err, what):
    print("{}: p abs {:.3g} (bound {:.3g}), m rel {:.3g} ({:.3g}), v rel {:.3g} ({:.3g})".format(
        what, err[0], P_BOUND, err[1], M_BOUND, err[2], V_BOUND))
    assert err[0] <= P_BOUND and err[1] <= M_BOUND and err[2] <= V_BOUND, (what, err)


# ---- units -----------------------------------------------------------------------------------------------------------
def test_agc_units_of_each_kind():
    assert optim.agc_units("enc.4.conv_b.weight", (256, 256, 3, 3)) == [(o * 2304, 2304) for o in range(256)]
    # Keras stores Conv2DTranspose as (kh,kw,out,in): one unit per INPUT channel = torch's first axis, O*kh*kw long
    assert optim.agc_units("dec.0.conv_up.weight", (256, 128, 4, 4)) == [(i * 2048, 2048) for i in range(256)]
    assert optim.agc_units("upflow.3.flow.feat.0.depthwise.weight", (115, 1, 3, 3)) == [(0, 1035)]
    assert optim.agc_units("upflow.3.flow.feat.0.pointwise.weight", (128, 115, 1, 1)) == [(o * 115, 115) for o in range(128)]
    assert optim.agc_units("enc.0.conv_a.bias", (16,)) == [(0, 16)]
    assert optim.agc_units("flow.flow.norm.gamma", (2,)) == [(0, 2)]
    assert optim.agc_units("some.norm.weight", (7,)) == [(0, 7)]           # rank 1 is a vector whatever its name
    for name, shape in CASE_STRIDED:
        assert optim.agc_units(name, shape) == oracle_units(name, shape)
    with pytest.raises(ValueError):
        optim.agc_units("conv3d.weight", (2, 2, 2, 2, 2))


def _agc_factors_keras(x_p, x_g):
    """core/agc.py:19-49 on Keras-layout arrays, restated: per-element factor g' / g."""
    if x_p.ndim <= 1:
        axis, keep = None, False
    elif x_p.ndim in (2, 3):
        axis, keep = 0, True
    else:
        axis, keep = (0, 1, 2), True
    pn = np.sqrt(np.sum(x_p ** 2, axis=axis, keepdims=keep))
    gn = np.sqrt(np.sum(x_g ** 2, axis=axis, keepdims=keep))
    mx = np.maximum(pn, AGC_EPS) * CLIP
    return np.broadcast_to(np.where(gn < mx, 1.0, mx / np.maximum(gn, 1e-6)), x_p.shape)


@pytest.mark.parametrize("name,shape", [("c.weight", (6, 5, 3, 3)), ("dec.1.conv_up.weight", (5, 7, 4, 4)),
                                        ("s.depthwise.weight", (9, 1, 3, 3)), ("s.pointwise.weight", (6, 9, 1, 1)),
                                        ("c.bias", (6,))])
def test_units_on_torch_layouts_are_the_keras_units(name, shape):
    """agc.py's axis rule on weights.to_keras_layout of a tensor gives, element for element, the clip factors of the
    torch-layout units: a transposed-convolution or depthwise mix-up would not."""
    rng = np.random.default_rng(3)
    p = rng.standard_normal(shape)
    g = rng.standard_normal(shape)
    gf = g.reshape(-1)
    for k, (off, ln) in enumerate(optim.agc_units(name, shape)):           # half the units clipped, half not
        gf[off:off + ln] *= (1e-4, 1.0)[k % 2]
    fk = _agc_factors_keras(weights.to_keras_layout({name: p})[name], weights.to_keras_layout({name: g})[name])
    want = weights.from_keras_layout({name: fk})[name]
    have = np.empty(p.size)
    pf = p.reshape(-1)
    for off, ln in optim.agc_units(name, shape):
        pn, gn = np.sqrt(np.sum(pf[off:off + ln] ** 2)), np.sqrt(np.sum(gf[off:off + ln] ** 2))
        mx = max(pn, AGC_EPS) * CLIP
        have[off:off + ln] = 1.0 if gn < mx else mx / max(gn, 1e-6)
    assert len(np.unique(want)) > 1 or len(optim.agc_units(name, shape)) == 1
    np.testing.assert_allclose(have.reshape(shape), want, rtol=1e-12, atol=0)
    # and the torch composition clips by the same factors
    out = optim.adaptive_clip_grad([(name, torch.from_numpy(p))], [torch.from_numpy(g)], CLIP, AGC_EPS)[0].numpy()
    np.testing.assert_allclose(out, g * want, rtol=1e-12, atol=0)


# ---- the torch composition against the oracle ------------------------------------------------------------------------
def _run_torch(case, clip, steps=STEPS):
    p0, grads, after = trajectory(case, clip)
    opt, named = make_optimizer(case, p0, "cpu", clip)
    for k in range(steps):
        set_grads(named, grads[k])
        opt.step()
    return opt, named, after[steps - 1]


@pytest.mark.parametrize("clip", [CLIP, None])
@pytest.mark.parametrize("case", list(CASES))
def test_step_torch_matches_the_oracle(case, clip):
    opt, named, ref = _run_torch(case, clip)
    assert opt.iterations == STEPS == ref["t"]
    assert_within_bounds(errors(case, named, opt, ref), "step_torch {} clip={}".format(case, clip))


def test_the_measured_errors_are_what_the_bounds_were_taken_from():
    """The constants above are the fp32 composition's own error against the float64 oracle (not a guess, and not the
    kernel's): it reaches at least a quarter of each on this case set, and stays under each."""
    worst = [0.0, 0.0, 0.0]
    for case in CASES:
        for clip in (CLIP, None):
            opt, named, ref = _run_torch(case, clip)
            worst = [max(a, b) for a, b in zip(worst, errors(case, named, opt, ref))]
    print("step_torch fp32 vs float64 oracle: p abs {:.3g}, m rel {:.3g}, v rel {:.3g}".format(*worst))
    for have, measured in zip(worst, (MEASURED_P_ABS, MEASURED_M_REL, MEASURED_V_REL)):
        assert measured / 4 <= have <= measured * 1.5


def test_zero_bias_is_clipped_to_the_eps_floor():
    p0, grads, _ = trajectory("small")
    g = oracle_clip(ZERO, p0[ZERO].astype(np.float64), grads[0][ZERO])
    assert abs(np.sqrt(np.sum(g ** 2)) / (_f32(AGC_EPS) * _f32(CLIP)) - 1.0) < 1e-6
    out = optim.adaptive_clip_grad([(ZERO, torch.from_numpy(p0[ZERO]))], [torch.from_numpy(grads[0][ZERO])])[0]
    assert abs(float(out.double().norm()) / (AGC_EPS * CLIP) - 1.0) < 1e-5


def test_keras_adam_is_not_torch_adam():
    """One step from the same (zero) state without clipping, on gradients small enough for epsilon to count: equal to
    the oracle, and further from torch.optim.Adam(lr, eps=1e-7) than the bound -- a silent swap to torch's formula
    (sqrt(v_hat) + eps) would be caught."""
    case = "small"
    p0, grads, _ = trajectory(case)
    small = {n: (g * np.float32(1e-3)) for n, g in grads[0].items()}
    ref = {"p": {n: a.astype(np.float64) for n, a in p0.items()}, "t": 0}
    ref["m"] = {n: np.zeros_like(a) for n, a in ref["p"].items()}
    ref["v"] = {n: np.zeros_like(a) for n, a in ref["p"].items()}
    oracle_step(ref, small, None)
    opt, named = make_optimizer(case, p0, "cpu", None)
    set_grads(named, small)
    opt.step()
    assert_within_bounds(errors(case, named, opt, ref), "keras adam, one step")
    theirs = [torch.nn.Parameter(torch.from_numpy(p0[n].copy())) for n, _ in CASES[case]]
    for t, (n, _) in zip(theirs, CASES[case]):
        t.grad = torch.from_numpy(small[n].copy())
    torch.optim.Adam(theirs, lr=LR, betas=(BETA_1, BETA_2), eps=1e-7).step()
    gap = max(float((a.detach() - b.detach()).abs().max()) for a, (_, b) in zip(theirs, named))
    print("largest |p_keras - p_torch| after one step: {:.3g}".format(gap))
    assert gap > 100 * P_BOUND


def nan_case(case="small"):
    """Step 1 of the case with one NaN element in unit 2 of a.weight: (p0, grads, oracle state after, (name, unit))."""
    p0, grads, _ = trajectory(case)
    g = {n: a.copy() for n, a in grads[0].items()}
    g["a.weight"][2, 17, 1, 2] = np.nan
    ref = {"p": {n: a.astype(np.float64) for n, a in p0.items()}, "t": 0}
    ref["m"] = {n: np.zeros_like(a) for n, a in ref["p"].items()}
    ref["v"] = {n: np.zeros_like(a) for n, a in ref["p"].items()}
    oracle_step(ref, g, CLIP)
    return p0, g, ref, ("a.weight", 2)


def assert_nan_unit(named, opt, ref, unit):
    """The whole unit is NaN in p, m and v (in the oracle too), and nothing else is."""
    name, u = unit
    p = dict(named)[name]
    for t, r in ((p.detach(), ref["p"][name]), (opt.state[p]["m"], ref["m"][name]), (opt.state[p]["v"], ref["v"][name])):
        t = t.cpu().numpy()
        assert np.isnan(t[u]).all() and np.isnan(r[u]).all()
        assert not np.isnan(np.delete(t, u, axis=0)).any()
    for n, q in named:
        if n != name:
            assert not torch.isnan(q).any() and not torch.isnan(opt.state[q]["m"]).any()


def test_nan_gradient_poisons_its_unit_only():
    p0, g, ref, unit = nan_case()
    opt, named = make_optimizer("small", p0)
    set_grads(named, g)
    opt.step()
    assert_nan_unit(named, opt, ref, unit)
    assert_within_bounds(errors("small", named, opt, ref), "NaN unit, every other unit")


def test_none_gradient_leaves_its_tensor_alone():
    p0, grads, _ = trajectory("small")
    opt, named = make_optimizer("small", p0)
    g = dict(grads[0])
    g["f.pointwise.weight"] = None
    set_grads(named, g)
    opt.step()
    p = dict(named)["f.pointwise.weight"]
    assert np.array_equal(p.detach().numpy(), p0["f.pointwise.weight"])
    assert not opt.state[p]["m"].any() and not opt.state[p]["v"].any()
    assert not np.array_equal(dict(named)["a.weight"].detach().numpy(), p0["a.weight"])


# ---- the optimiser's surface -----------------------------------------------------------------------------------------
def test_state_dict_round_trip_continues_bit_identically():
    p0, grads, _ = trajectory("small")
    straight, named_s = make_optimizer("small", p0)
    for k in range(3):
        set_grads(named_s, grads[k])
        straight.step()
    first, named_f = make_optimizer("small", p0)
    for k in range(2):
        set_grads(named_f, grads[k])
        first.step()
    saved = first.state_dict()
    assert saved["iterations"] == 2 and list(saved["m"]) == [n for n, _ in CASE_SMALL] == list(saved["v"])
    resumed, named_r = make_optimizer("small", {n: p.detach().numpy() for n, p in named_f})
    resumed.load_state_dict(saved)
    set_grads(named_r, grads[2])
    resumed.step()
    assert resumed.iterations == 3
    for (n, a), (_, b) in zip(named_s, named_r):
        assert torch.equal(a, b), n
        assert torch.equal(straight.state[a]["m"], resumed.state[b]["m"]), n
        assert torch.equal(straight.state[a]["v"], resumed.state[b]["v"]), n
    with pytest.raises(ValueError):
        resumed.load_state_dict({"iterations": 0, "m": {}, "v": {}})


def test_optimizer_surface():
    from qpwcnet_amd import layers
    import qpwcnet_amd
    assert qpwcnet_amd.optim is optim
    model = layers.FlowerModel()
    opt = optim.KerasAdamAGC(model)
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1
    assert opt.param_groups[0]["lr"] == 1e-4 and len(opt.param_groups[0]["params"]) == 123
    assert list(opt.state_dict()["m"]) == [n for n, _ in model.named_parameters()]
    assert set(opt.state_dict()["m"]) <= set(model.state_dict())
    p = next(model.parameters())
    p.grad = torch.ones_like(p)
    opt.zero_grad()
    assert p.grad is None
    # lr: a callable of the step count, or whatever the group holds at the step
    named = [("w.bias", torch.nn.Parameter(torch.ones(3)))]
    seen = []
    opt = optim.KerasAdamAGC(named, lr=lambda step: seen.append(step) or 1e-3, clip_factor=None)
    for _ in range(2):
        named[0][1].grad = torch.ones(3)
        opt.step()
    assert seen == [0, 1]
    with pytest.raises(TypeError):
        optim.KerasAdamAGC([torch.nn.Parameter(torch.ones(3))])            # no names: the units cannot be known
    with pytest.raises(ValueError):
        optim.KerasAdamAGC([("h.bias", torch.nn.Parameter(torch.ones(3, dtype=torch.float16)))]).step()
    with pytest.raises(ValueError):
        optim.KerasAdamAGC(named, beta_2=1.0)
    with pytest.raises(ValueError, match="one parameter group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})


def test_learning_rate_schedule():
    """train.py:29-40 at batch size 8: PiecewiseConstantDecay keeps values[i] up to and including boundaries[i]."""
    lr = optim.learning_rate(8)
    for k, b in enumerate((400000, 600000, 800000, 1000000)):
        assert lr(b) == 1e-4 / 2 ** k and lr(b + 1) == 1e-4 / 2 ** (k + 1)
    assert lr(0) == 1e-4 and lr(10 ** 9) == 1e-4 / 16
    assert optim.learning_rate(16).boundaries == [200000, 300000, 400000, 500000]
    assert optim.learning_rate(3).boundaries == [int(400000 * 8 / 3), 1600000, int(800000 * 8 / 3), int(8e6 / 3)]


# ---- the C boundary: prototypes and link -----------------------------------------------------------------------------
def test_optim_table_matches_its_header():
    protos = parse_header(OPTIM_HEADER)
    assert [n for n, _, _ in protos] == ["qpwc_agc_adam_step", "qpwc_agc_adam_step_kernel"]
    assert mismatches(_hip.OPTIM_PROTOTYPES, protos) == []
    assert len(_hip.SYMBOLS) == 77 and not set(_hip.OPTIM_PROTOTYPES) & set(_hip.SYMBOLS)


def test_library_exports_the_optimiser(hip_lib):
    for name, (restype, argtypes) in _hip.OPTIM_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert hip_lib.qpwc_version() == 200
    # the launch form is a host-side rule: up to 1024 workgroups x 4 waves take one unit per wave
    assert hip_lib.qpwc_agc_adam_step_kernel(4096) == b"agc_adam_kernel<one unit per wave>"
    assert hip_lib.qpwc_agc_adam_step_kernel(4097) == b"agc_adam_kernel<grid-stride>"
    assert hip_lib.qpwc_agc_adam_step_kernel(0) == b""
    units = {c: sum(len(oracle_units(n, s)) for n, s in CASES[c]) for c in CASES}
    assert hip_lib.qpwc_agc_adam_step_kernel(units["small"]) == b"agc_adam_kernel<one unit per wave>"
    assert hip_lib.qpwc_agc_adam_step_kernel(units["strided"]) == b"agc_adam_kernel<grid-stride>"

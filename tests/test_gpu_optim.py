"""The HIP update step (optim.KerasAdamAGC on CUDA tensors: qpwc_agc_adam_step, one launch) against the float64 oracle
of tests/test_optim_cpu.py, on its case set and within its bounds -- which are 4 x the measured error of the fp32 torch
composition on the CPU, not anything the kernel gave."""
import numpy as np
import pytest
import torch

from qpwcnet_amd import _hip, layers, loss, optim, synth
from test_optim_cpu import (CASES, CLIP, M_BOUND, P_BOUND, STEPS, V_BOUND, assert_nan_unit,  # noqa: E402
                            assert_within_bounds, errors, make_optimizer, nan_case, oracle_units, set_grads,
                            trajectory)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _n_units(case):
    return sum(len(oracle_units(n, s)) for n, s in CASES[case])


def _run(case, clip, steps=STEPS, realloc=False):
    p0, grads, after = trajectory(case, clip)
    opt, named = make_optimizer(case, p0, DEV, clip)
    kept, seen = [], set()
    for k in range(steps):
        if realloc:
            kept.append([p.grad for _, p in named])     # the old gradients stay allocated: the new ones cannot land there
            opt.zero_grad(set_to_none=True)
        set_grads(named, grads[k])
        seen.add(named[0][1].grad.data_ptr())
        opt.step()
    assert not realloc or len(seen) == steps
    torch.cuda.synchronize()
    return opt, named, after[steps - 1]


def test_the_case_sets_take_both_launch_forms():
    """'strided' has more units than the capped grid has waves, so its waves take more than one unit."""
    L = _hip.lib()
    assert L.qpwc_agc_adam_step_kernel(_n_units("small")) == b"agc_adam_kernel<one unit per wave>"
    assert L.qpwc_agc_adam_step_kernel(_n_units("strided")) == b"agc_adam_kernel<grid-stride>"


@pytest.mark.parametrize("clip", [CLIP, None])
@pytest.mark.parametrize("case", list(CASES))
def test_three_steps_match_the_oracle(case, clip):
    opt, named, ref = _run(case, clip)
    assert opt.iterations == STEPS
    assert_within_bounds(errors(case, named, opt, ref), "HIP step {} clip={}".format(case, clip))


def test_nan_gradient_poisons_its_unit_only():
    p0, g, ref, unit = nan_case()
    opt, named = make_optimizer("small", p0, DEV)
    set_grads(named, g)
    opt.step()
    torch.cuda.synchronize()
    assert_nan_unit(named, opt, ref, unit)
    assert_within_bounds(errors("small", named, opt, ref), "HIP step, NaN unit, every other unit")


def test_none_gradient_leaves_its_tensor_bit_unchanged():
    """After two real steps (non-zero m and v), a step with grad=None on one tensor: its p, m and v keep their bits
    and the others move."""
    p0, grads, _ = trajectory("small")
    opt, named = make_optimizer("small", p0, DEV)
    for k in range(2):
        set_grads(named, grads[k])
        opt.step()
    skipped = "f.pointwise.weight"
    before = {n: (p.detach().clone(), opt.state[p]["m"].clone(), opt.state[p]["v"].clone()) for n, p in named}
    g = dict(grads[2])
    g[skipped] = None
    set_grads(named, g)
    opt.step()
    torch.cuda.synchronize()
    for n, p in named:
        same = [torch.equal(a, b) for a, b in zip(before[n], (p.detach(), opt.state[p]["m"], opt.state[p]["v"]))]
        assert same == ([True] * 3 if n == skipped else [False] * 3), (n, same)
    assert before[skipped][1].abs().max() > 0


def test_two_runs_give_identical_bits():
    a, named_a, _ = _run("strided", CLIP)
    b, named_b, _ = _run("strided", CLIP)
    for (n, p), (_, q) in zip(named_a, named_b):
        assert torch.equal(p, q) and torch.equal(a.state[p]["m"], b.state[q]["m"]), n
        assert torch.equal(a.state[p]["v"], b.state[q]["v"]), n


def test_reallocated_gradients_still_update():
    """zero_grad(set_to_none=True) and fresh .grad tensors at other addresses between the steps: the pointer table
    follows them."""
    opt, named, ref = _run("small", CLIP, realloc=True)
    assert_within_bounds(errors("small", named, opt, ref), "HIP step, .grad reallocated")


def test_state_dict_round_trip_continues_bit_identically():
    p0, grads, _ = trajectory("small")
    straight, named_s, _ = _run("small", CLIP)
    first, named_f, _ = _run("small", CLIP, steps=2)
    resumed, named_r = make_optimizer("small", {n: p.detach().cpu().numpy() for n, p in named_f}, DEV)
    resumed.load_state_dict(first.state_dict())
    set_grads(named_r, grads[2])
    resumed.step()
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(named_s, named_r):
        assert torch.equal(a, b) and torch.equal(straight.state[a]["m"], resumed.state[b]["m"]), n
        assert torch.equal(straight.state[a]["v"], resumed.state[b]["v"]), n


def test_flower_model_step_matches_the_torch_composition():
    """Real gradients of one loss.multiscale backward through layers.FlowerModel at (1,64,64,6); one HIP step against
    optim.step_torch on a CPU copy of the parameters and gradients."""
    hw = (64, 64)
    model = layers.FlowerModel(data_format="channels_last")
    model.load_state_dict({k: torch.as_tensor(v) for k, v in synth.make_weights(42, hw).items()})   # O(1) features
    model = model.to(DEV).train()
    pairs, flow_gt = synth.make_frames(1, hw[0], hw[1], seed=5)
    pairs, gt = torch.as_tensor(pairs).to(DEV), torch.as_tensor(flow_gt).to(DEV)
    assert tuple(pairs.shape) == (1, 64, 64, 6)
    total = loss.multiscale(loss.FlowMseLossV2(), gt, model(pairs)[:-1])[0]
    total.backward()
    names = [n for n, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    assert all(p.grad is not None for p in params)
    assert _hip.lib().qpwc_agc_adam_step_kernel(sum(len(optim.agc_units(n, p.shape)) for n, p in zip(names, params))) \
        == b"agc_adam_kernel<one unit per wave>"
    cpu = [(n, p.detach().cpu().clone()) for n, p in zip(names, params)]
    grads = [p.grad.detach().cpu().clone() for p in params]
    before = [p.detach().clone() for p in params]
    opt = optim.KerasAdamAGC(model)
    opt.step()
    torch.cuda.synchronize()
    m = [torch.zeros_like(p) for _, p in cpu]
    v = [torch.zeros_like(p) for _, p in cpu]
    optim.step_torch(cpu, grads, m, v, optim.keras_step_size(1e-4, 0.9, 0.999, 1))
    worst = [0.0, 0.0, 0.0]
    for (n, want), p, b, mw, vw in zip(cpu, params, before, m, v):
        assert not torch.equal(p.detach(), b), n + " did not move"
        have = (p.detach().cpu(), opt.state[p]["m"].cpu(), opt.state[p]["v"].cpu())
        for off, ln in optim.agc_units(n, p.shape):
            for k, (h, w) in enumerate(zip(have, (want, mw, vw))):
                h, w = h.reshape(-1)[off:off + ln].double(), w.reshape(-1)[off:off + ln].double()
                assert torch.isfinite(h).all(), n
                d = float((h - w).abs().max())
                if k:
                    scale = float(w.abs().max())
                    d = (0.0 if d == 0.0 else float("inf")) if scale == 0.0 else d / scale
                worst[k] = max(worst[k], d)
    assert_within_bounds(tuple(worst), "HIP step vs step_torch, FlowerModel")


def test_step_refuses_capture_and_changes_nothing():
    p0, grads, _ = trajectory("small")
    opt, named = make_optimizer("small", p0, DEV)
    set_grads(named, grads[0])
    opt.step()                                  # the state and both tables exist before the capture
    set_grads(named, grads[1])
    torch.cuda.synchronize()
    before = [p.detach().clone() for _, p in named]
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured in a torch.cuda graph yet"):
        with torch.cuda.graph(graph):
            opt.step()
    torch.cuda.synchronize()
    assert opt.iterations == 1
    for (n, p), b in zip(named, before):
        assert torch.equal(p.detach(), b), n
    opt.step()                                  # and the optimiser still works afterwards
    torch.cuda.synchronize()
    assert opt.iterations == 2 and not torch.equal(named[0][1].detach(), before[0])


def test_refusals():
    half = [("h.bias", torch.nn.Parameter(torch.ones(4, device=DEV, dtype=torch.float16)))]
    half[0][1].grad = torch.ones_like(half[0][1])
    with pytest.raises(ValueError, match="fp32 only"):
        optim.KerasAdamAGC(half).step()
    mixed = [("a.bias", torch.nn.Parameter(torch.ones(4, device=DEV))), ("b.bias", torch.nn.Parameter(torch.ones(4)))]
    with pytest.raises(ValueError, match="more than one device"):
        optim.KerasAdamAGC(mixed).step()


def test_noncontiguous_gradient_is_made_dense():
    p0, grads, after = trajectory("small")
    opt, named = make_optimizer("small", p0, DEV)
    set_grads(named, grads[0])
    w = dict(named)["a.weight"]
    w.grad = w.grad.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # same values, channels-last strides
    assert not w.grad.is_contiguous()
    opt.step()
    torch.cuda.synchronize()
    assert_within_bounds(errors("small", named, opt, after[0]), "HIP step, non-contiguous gradient")
    assert np.isfinite(P_BOUND + M_BOUND + V_BOUND)

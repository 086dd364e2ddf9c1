"""CPU suite of the trainable flow estimator: qpwc_flow_head_stats_fwd / qpwc_flow_head_bwd / qpwc_upsample2x_flow_bwd
and their workspace queries refuse bad arguments before any HIP call, the float64 oracle composite of
tests/test_gpu_flow_head_grad.py is the true derivative in both BatchNorm modes, the Upsample adjoint of include/qpwc.h
is the adjoint of F.interpolate, the grad paths refuse CPU tensors / capture / fp16, the layers build and name their
state on the host, and the GPU suite's "more than one trip" shape still loops against the constants of
csrc/flow_head_bwd.hip."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_flow_head_grad import (MULTI_TRIP, TRAIN_DRIFT, head_composite, train_composite,  # noqa: E402
                                     upsample_composite)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")
VP = ctypes.c_void_p


def _constants(*keys):
    text = open(os.path.join(CSRC, "flow_head_bwd.hip")).read()
    out = {}
    for k in keys:
        m = re.findall(r"constexpr\s+int\s+{}\s*=\s*([0-9+ ]+);".format(k), text)
        assert len(m) == 1, (k, m)
        out[k] = sum(int(v) for v in m[0].split("+"))
    return out


K = _constants("kFhbTile", "kFhbTileBlocks", "kFhbStatBlocks", "kFhbUpBlocks", "kFhbN1", "kFhbN2")


def _tiles(B, H, W):
    return B * -(-H // K["kFhbTile"]) * -(-W // K["kFhbTile"])


def test_workspace_floats(hip_lib):
    from qpwcnet_amd import _hip
    bwd, stats = hip_lib.qpwc_flow_head_bwd_workspace_floats, hip_lib.qpwc_flow_head_stats_workspace_floats
    assert (K["kFhbN1"], K["kFhbN2"]) == (320, 272)
    for shape in ((1, 1, 1), (2, 19, 37), (8, 128, 256), MULTI_TRIP):
        blocks = min(_tiles(*shape), K["kFhbTileBlocks"])
        assert bwd(*shape) == blocks * K["kFhbN1"] + K["kFhbN1"] + blocks * K["kFhbN2"], shape
        M = shape[0] * shape[1] * shape[2]
        assert stats(*shape) == min(-(-(-(-M // 16)) // 4), K["kFhbStatBlocks"]) * 16 * 4, shape
    for fn in (bwd, stats):
        assert fn(0, 4, 4) == _hip.E_SHAPE and fn(1, -1, 4) == _hip.E_SHAPE
        assert fn(2, 4096, 4096) == _hip.E_SHAPE and b"2^24" in hip_lib.qpwc_last_error()


def _buffers(n):
    keep = (ctypes.c_float * (n << 14))()
    base = ctypes.cast(keep, VP).value
    base += (-base) % 16
    return keep, [base + 65536 * i for i in range(n)]


def test_flow_head_bwd_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, (z, params, stats, gout, gz, gw1, gb1, gg, gb, gwf, ws) = _buffers(11)
    assert L.qpwc_flow_head_bwd_workspace_floats(1, 4, 4) * 4 <= 65536

    def call(z=z, params=params, stats=stats, eps=1e-3, training=1, gout=gout, gz=gz, gw1=gw1, gb1=gb1, gg=gg, gb=gb,
             gwf=gwf, ws=ws, B=1, H=4, W=4):
        return L.qpwc_flow_head_bwd(z, params, stats, eps, training, 2.0, gout, gz, gw1, gb1, gg, gb, gwf, ws, B, H, W,
                                    None)

    err = L.qpwc_last_error
    for kw, name in ((dict(z=None), b"z"), (dict(params=None), b"params"), (dict(stats=None), b"stats"),
                     (dict(gout=None), b"grad_out"), (dict(ws=None), b"workspace")):
        assert call(**kw) == _hip.E_NULL and name in err(), (kw, err())
    assert call(gz=None, gw1=None, gb1=None, gg=None, gb=None, gwf=None) == _hip.E_NULL and b"all null" in err()
    assert call(H=0) == _hip.E_SHAPE
    assert call(eps=0.0) == _hip.E_RANGE and b"eps" in err()
    assert call(z=z + 4) == _hip.E_ALIGN and b"z" in err()
    assert call(params=params + 8) == _hip.E_ALIGN and b"params" in err()
    assert call(gout=gout + 4) == _hip.E_ALIGN and b"grad_out" in err()
    assert call(gz=gz + 8) == _hip.E_ALIGN and b"grad_z" in err()
    assert call(ws=ws + 4) == _hip.E_ALIGN and b"workspace" in err()
    assert call(gb1=gb1 + 2) == _hip.E_ALIGN and b"grad_b1" in err()
    assert call(gz=z) == _hip.E_ALIAS and b"grad_z" in err() and b"z" in err()
    assert call(gw1=params + 16) == _hip.E_ALIAS and b"grad_w1" in err()
    assert call(gg=gb + 32) == _hip.E_ALIAS and b"grad_beta" in err()       # two outputs overlap
    assert call(gwf=gout) == _hip.E_ALIAS and b"grad_out" in err()
    assert call(ws=gz) == _hip.E_ALIAS and b"workspace" in err()
    assert call(ws=gout - 64) == _hip.E_ALIAS                                # the workspace runs into grad_out


def test_flow_head_stats_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, (z, w1, b1, gamma, beta, wf, mm, mv, params, stats, ws) = _buffers(11)
    assert L.qpwc_flow_head_stats_workspace_floats(1, 4, 4) * 4 <= 65536

    def call(z=z, w1=w1, b1=b1, gamma=gamma, beta=beta, wf=wf, mm=mm, mv=mv, momentum=0.99, eps=1e-3, params=params,
             stats=stats, ws=ws, B=1, H=4, W=4):
        return L.qpwc_flow_head_stats_fwd(z, w1, b1, gamma, beta, wf, mm, mv, momentum, eps, params, stats, ws, B, H, W,
                                          None)

    err = L.qpwc_last_error
    for key in ("z", "w1", "b1", "gamma", "beta", "wf", "params"):
        assert call(**{key: None}) == _hip.E_NULL and key.encode() in err(), (key, err())
    assert call(ws=None) == _hip.E_NULL and b"workspace" in err()
    assert call(mv=None) == _hip.E_NULL and b"both or neither" in err()
    assert call(W=0) == _hip.E_SHAPE
    assert call(eps=-1.0) == _hip.E_RANGE and call(momentum=1.5) == _hip.E_RANGE and b"momentum" in err()
    assert call(z=z + 8) == _hip.E_ALIGN and call(params=params + 4) == _hip.E_ALIGN and b"params" in err()
    assert call(params=w1) == _hip.E_ALIAS and b"params" in err()
    assert call(mm=gamma) == _hip.E_ALIAS and b"moving_mean" in err()
    assert call(mv=mm + 32) == _hip.E_ALIAS
    assert call(stats=params + 64) == _hip.E_ALIAS and b"stats" in err()
    assert call(ws=z) == _hip.E_ALIAS and b"workspace" in err()


def test_upsample_bwd_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, (g, out) = _buffers(2)
    call = lambda g=g, out=out, B=1, h=4, w=4: L.qpwc_upsample2x_flow_bwd(g, out, B, h, w, 2.0, None)
    assert call(g=None) == _hip.E_NULL and b"grad_out" in L.qpwc_last_error()
    assert call(out=None) == _hip.E_NULL and b"grad_in" in L.qpwc_last_error()
    assert call(h=0) == _hip.E_SHAPE
    assert call(g=g + 4) == _hip.E_ALIGN and call(out=out + 4) == _hip.E_ALIGN
    assert call(out=g + 64) == _hip.E_ALIAS and b"grad_in" in L.qpwc_last_error()


# ---- the oracle is the derivative ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [False, True], ids=["frozen", "batch"])
def test_gradcheck_composite_oracle(training):
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_()
    z, w1, b1, gamma, beta, wf = r(2, 3, 4, 16), r(16, 16, 1, 1), r(16), r(16), r(16), r(2, 16, 3, 3)
    mean = torch.randn(16, generator=gen, dtype=torch.float64)
    var = torch.rand(16, generator=gen, dtype=torch.float64) + 0.5
    fn = lambda z, w1, b1, gamma, beta, wf: head_composite(z, w1 / 4, b1, gamma, beta, mean, var, wf, 2.0, training)[0]
    assert torch.autograd.gradcheck(fn, (z, w1, b1, gamma, beta, wf), eps=1e-7, atol=1e-6)


def test_training_composite_is_keras_non_fused_batch_norm():
    """Biased variance in the normalisation AND in the moving update (F.batch_norm's running_var is unbiased)."""
    gen = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    z, w1, b1, wf = r(2, 3, 4, 16), r(16, 16, 1, 1) / 4, r(16), r(2, 16, 3, 3)
    gamma, beta, mean, var = r(16), r(16), r(16), torch.rand(16, generator=gen, dtype=torch.float64) + 0.5
    out, nm, nv = head_composite(z, w1, b1, gamma, beta, mean, var, wf, 1.0, True, eps=1e-3, momentum=0.99)
    from oracle import torch_ref
    u = torch_ref.mish(torch.nn.functional.conv2d(torch_ref.mish(z).permute(0, 3, 1, 2), w1, b1))
    flat = u.permute(1, 0, 2, 3).reshape(16, -1)
    bm, bv = flat.mean(1), ((flat - flat.mean(1, keepdim=True)) ** 2).mean(1)
    assert torch.allclose(nm, 0.99 * mean + 0.01 * bm, atol=1e-14) and torch.allclose(nv, 0.99 * var + 0.01 * bv, atol=1e-14)
    # normalising with those statistics by the frozen formula gives the same flow
    same, _, _ = head_composite(z, w1, b1, gamma, beta, bm, bv, wf, 1.0, False, eps=1e-3)
    assert torch.allclose(out, same, atol=1e-12)


def upsample_adjoint(g, scale):
    """The gather of include/qpwc.h (qpwc_upsample2x_flow_bwd) in torch: per axis taps 2i-1 .. 2i+2 with weights
    1/4, 3/4, 3/4, 1/4, a tap past the border clamped onto it."""
    def axis(t, dim):
        n = t.shape[dim] // 2
        i = torch.arange(n)
        taps = [(2 * i - 1).clamp(min=0), 2 * i, 2 * i + 1, (2 * i + 2).clamp(max=2 * n - 1)]
        return sum(wt * t.index_select(dim, k) for wt, k in zip((0.25, 0.75, 0.75, 0.25), taps))
    return scale * axis(axis(g, 1), 2)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 3), (2, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_upsample_adjoint_is_the_gradient_of_interpolate(shape):
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(shape + (2,), generator=gen, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: upsample_composite(t, 2.0), (x,), eps=1e-6, atol=1e-8)
    g = torch.randn(shape[0], 2 * shape[1], 2 * shape[2], 2, generator=gen, dtype=torch.float64)
    upsample_composite(x, 2.0).backward(g)
    assert torch.allclose(x.grad, upsample_adjoint(g, 2.0), atol=1e-13)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _operands(dtype=torch.float32):
    z = torch.zeros(1, 4, 4, 16, dtype=dtype, requires_grad=True)
    return [z, torch.zeros(16, 16, 1, 1), torch.zeros(16), torch.ones(16), torch.zeros(16), torch.zeros(16), torch.ones(16),
            torch.zeros(2, 16, 3, 3), 1.0]


def test_the_grad_paths_need_a_hip_device():
    from qpwcnet_amd import layers, ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.flow_head_train(*_operands())
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.upsample2x_flow(torch.zeros(1, 4, 4, 2, requires_grad=True))
    with pytest.raises(RuntimeError, match="HIP device"):
        layers.OptFlow(5, data_format="channels_last")(torch.zeros(1, 4, 4, 5))
    with pytest.raises(RuntimeError, match="HIP device"):
        layers.Upsample(2.0, data_format="channels_last")(torch.zeros(1, 4, 4, 2, requires_grad=True))


def test_the_grad_paths_refuse_fp16():
    from qpwcnet_amd import ops
    with pytest.raises(ValueError, match="fp16"):
        ops.flow_head_train(*_operands(torch.float16))
    with pytest.raises(ValueError, match="fp16"):
        ops.upsample2x_flow(torch.zeros(1, 4, 4, 2, dtype=torch.float16, requires_grad=True))


def test_the_grad_paths_refuse_graph_capture(monkeypatch):
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.flow_head_train(*_operands())
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.upsample2x_flow(torch.zeros(1, 4, 4, 2, requires_grad=True))
    ctx = types.SimpleNamespace(saved_tensors=(), cfg=None, needs_input_grad=(True,) * 6 + (False,) * 6)
    for fn, g in ((ops._FlowHeadFn, torch.zeros(1, 4, 4, 2)), (ops._UpsampleFn, torch.zeros(1, 8, 8, 2))):
        with pytest.raises(RuntimeError, match="cannot be captured"):
            fn.backward(ctx, g)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._FlowHeadFn.forward(ctx, *_operands()[:5], _operands()[7], *_operands()[5:7], 1.0, True, 0.99, 1e-3)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._UpsampleFn.forward(ctx, torch.zeros(1, 4, 4, 2), 2.0, "channels_last", "channels_last")


# ---- the layers on the host ------------------------------------------------------------------------------------------------
def test_layer_constructors_and_state_dict_names_on_the_host():
    from qpwcnet_amd import layers, weights
    ours = weights.keras_variable_names()
    lay = layers.OptFlow(145, name="of")
    want = sorted(n[len("flow.flow."):] for n in ours if n.startswith("flow.flow."))
    assert sorted(lay.state_dict()) == want and len(want) == 19
    assert sorted(n for n, _ in lay.named_buffers()) == ["norm.mean", "norm.var"]
    assert [tuple(lay.state_dict()[n].shape) for n in ("conv.weight", "conv.bias", "norm.gamma", "flow.weight")] == \
        [(16, 16, 1, 1), (16,), (16,), (2, 16, 3, 3)]
    assert tuple(lay.feat[0].depthwise.weight.shape) == (145, 1, 3, 3) and lay.feat[3].activation is None
    assert [f.activation for f in lay.feat[:3]] == ["Mish"] * 3
    assert float(lay.norm.gamma.min()) == 1.0 and float(lay.norm.var.min()) == 1.0 and float(lay.norm.mean.abs().max()) == 0.0
    assert float(lay.conv.bias.abs().max()) == 0.0 and not hasattr(lay.flow, "bias")
    lim = (6.0 / (16 * 9 + 2 * 9)) ** 0.5
    assert 0.5 * lim < float(lay.flow.weight.abs().max()) <= lim            # Glorot uniform
    assert lay.get_config() == {"name": "of", "in_channels": 145, "filters": (128, 64, 32, 16), "scale": None}
    assert sorted(layers.OptFlow.from_config(lay.get_config()).state_dict()) == want
    with pytest.raises(ValueError):
        layers.OptFlow(145, filters=(64, 32))                                # the head takes 16 channels
    flow, upflow = layers.Flow(32), layers.UpFlow(32)
    assert sorted(flow.state_dict()) == sorted(n[len("flow."):] for n in ours if n.startswith("flow."))
    assert sorted(upflow.state_dict()) == sorted(n[len("upflow.0."):] for n in ours if n.startswith("upflow.0."))
    assert flow.flow.in_channels == 81 + 64 and upflow.flow.in_channels == 81 + 32 + 2
    assert flow.get_config() == {"name": None, "in_channels": 32}
    assert layers.UpFlow.from_config(upflow.get_config()).flow.in_channels == 115
    up = layers.Upsample(2.0, name="up")
    assert up.get_config() == {"name": "up", "scale": 2.0} and layers.Upsample.from_config(up.get_config()).scale == 2.0
    assert not list(up.parameters())
    assert layers.Flow(8, data_format="channels_first").flow.data_format == "channels_first"


# ---- the GPU suite's constants -----------------------------------------------------------------------------------------------
def test_training_case_drift_is_what_the_gpu_bound_was_derived_from():
    """The fp32 CPU composite against the float64 one over the 5 SGD steps of test_short_training_run: the drift the
    GPU test's bound (10 x) was set from; the float64 loss falls at every step.  The figure is an fp32 ulp or two of
    the largest parameters (gamma = 1) and moves a little with the host's BLAS and thread count, hence the factor 2
    either way."""
    ref, losses = train_composite(torch.float64)
    got, _ = train_composite(torch.float32)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    drift = max(float((got[n].double() - ref[n]).abs().max()) for n in ref)
    assert TRAIN_DRIFT / 2 <= drift <= 2 * TRAIN_DRIFT, drift


def test_multi_trip_case_loops_past_every_cap():
    B, H, W = MULTI_TRIP
    M = B * H * W
    # both backward passes: tiles in grid-stride order over min(tiles, kFhbTileBlocks) workgroups
    tiles, cap = _tiles(B, H, W), K["kFhbTileBlocks"]
    assert tiles > cap and tiles % cap, (tiles, cap)
    assert H % K["kFhbTile"] and W % K["kFhbTile"], "no partial last tile"
    # flow_head_stats_kernel: groups of 16 pixels over 4 waves of min(groups / 4, kFhbStatBlocks) workgroups
    groups, cap = -(-M // 16), 4 * K["kFhbStatBlocks"]
    assert groups >= 2 * cap and groups % cap and M % 16, (groups, cap)
    # upsample2x_flow_bwd_kernel: one thread per input pixel over min(blocks, kFhbUpBlocks) workgroups of 256
    cap = 256 * K["kFhbUpBlocks"]
    assert M > cap and M % cap and M % 256, (M, cap)


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernels_use_no_scratch(tmp_path):
    """Every kernel of flow_head_bwd.hip compiles for gfx950 without scratch memory and the 16 x 16 products are on the
    fp32 matrix instruction."""
    s = tmp_path / "flow_head_bwd.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "flow_head_bwd.hip"), "-o", str(s)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    assert len(names) == len(scratch) == 6, names
    assert all("flow_head" in n or "upsample2x_flow_bwd" in n for n in names), names
    assert not any(scratch), dict(zip(names, scratch))
    text = s.read_text()
    assert text.count("v_mfma_f32_16x16x4_f32") >= 20       # W1 m in three kernels, W1^T ga and ga^T m: four each

"""CPU suite of the trainable frame interpolator: the entry points of csrc/interp.hip refuse bad arguments before any
HIP call, the composites of tests/test_gpu_interp_grad.py are what the header states, the grad paths refuse CPU tensors /
fp16 / capture, the layers carry the state-dict names of synth.make_interpolator_weights, and the GPU suite's "more
than one trip" shape still loops against the constants of csrc/interp.hip."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch

from qpwcnet_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_interp_grad import (MULTI_TRIP, TRAIN_BOUND, TRAIN_DRIFT, _rate, head_composite, pyramid_composite,  # noqa: E402
                                  train_case, train_composite)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")
HEADER = os.path.join(os.path.dirname(CSRC), os.pardir, "include", "qpwc.h")
VP = ctypes.c_void_p
NEW = ("qpwc_image_head_fwd", "qpwc_image_head_bwd_workspace_floats", "qpwc_image_head_bwd", "qpwc_upsample2x_image_fwd",
       "qpwc_upsample2x_image_bwd", "qpwc_avgpool_pyramid_fwd")


def _constants(name, *keys):
    text = open(os.path.join(CSRC, name)).read()
    out = {}
    for k in keys:
        m = re.findall(r"constexpr\s+int\s+{}\s*=\s*(\d+)\s*[;,]".format(k), text)
        assert len(m) == 1, (name, k, m)
        out[k] = int(m[0])
    return out


IP = _constants("interp.hip", "kIhPx", "kIhBlocks", "kUiBlocks", "kUiBwdBlocks", "kApTilePx", "kApMaxLevels")
RED_LANES = _constants("conv_bwd_common.h", "kCgRedLanes")["kCgRedLanes"]


def _ws_floats(M):
    """ih_plan() of interp.hip: one partial of grad_w2 (3 x 64) and grad_b2 (3, rounded up to 4) per workgroup."""
    blocks = min(-(-M // IP["kIhPx"]), IP["kIhBlocks"])
    return blocks * 192 + -(-blocks * 3 // 4) * 4


def test_every_symbol_of_the_header_is_exported(hip_lib):
    from qpwcnet_amd import _hip
    declared = set(re.findall(r"\b(qpwc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NEW:
        assert name in declared and name in _hip.SYMBOLS and getattr(hip_lib, name) is not None, name
    assert declared == set(_hip.SYMBOLS)


def test_workspace_floats(hip_lib):
    from qpwcnet_amd import _hip
    ws = hip_lib.qpwc_image_head_bwd_workspace_floats
    sizes = [1, 15, 64, 65, 105, 126, 4096, 63999, 64000, 64001, MULTI_TRIP[0] * MULTI_TRIP[1] * MULTI_TRIP[2], 1 << 20]
    got = [ws(m) for m in sizes]
    assert got == [_ws_floats(m) for m in sizes]
    assert all(g > 0 for g in got) and all(a <= b for a, b in zip(got, got[1:]))
    assert got[0] == 196 and got[-1] == got[-2] == IP["kIhBlocks"] * 195            # capped: the shape alone decides
    assert ws(0) == _hip.E_SHAPE and ws(-5) == _hip.E_SHAPE and b"M=-5" in hip_lib.qpwc_last_error()


def _buffers(n, gap):
    keep = (ctypes.c_float * (n * gap // 4 + 8))()
    base = ctypes.cast(keep, VP).value
    base += (-base) % 16
    return keep, [base + gap * i for i in range(n)]


def test_image_head_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, (z, w2, b2, out, g, gz, gw, gb, ws) = _buffers(9, 4096)                       # M = 4: z holds 1024 bytes
    assert L.qpwc_image_head_bwd_workspace_floats(4) * 4 <= 4096

    def fwd(z=z, w2=w2, b2=b2, out=out, M=4):
        return L.qpwc_image_head_fwd(z, w2, b2, out, M, None)

    def bwd(z=z, w2=w2, g=g, gz=gz, gw=gw, gb=gb, ws=ws, M=4):
        return L.qpwc_image_head_bwd(z, w2, g, gz, gw, gb, ws, M, None)

    def err():
        return L.qpwc_last_error()

    for kw, name in ((dict(z=None), b"z"), (dict(w2=None), b"w2"), (dict(b2=None), b"b2"), (dict(out=None), b"out")):
        assert fwd(**kw) == _hip.E_NULL and name in err(), (kw, err())
    assert fwd(M=0) == _hip.E_SHAPE and b"M=0" in err()
    assert fwd(M=-1) == _hip.E_SHAPE
    assert fwd(z=z + 4) == _hip.E_ALIGN and b"z" in err()
    assert fwd(w2=w2 + 8) == _hip.E_ALIGN and b"w2" in err()
    assert fwd(b2=b2 + 2) == _hip.E_ALIGN and b"b2" in err()
    assert fwd(out=out + 1) == _hip.E_ALIGN and b"out" in err()
    assert fwd(out=z + 16) == _hip.E_ALIAS and b"out" in err() and b"z" in err()
    assert fwd(out=w2 + 4) == _hip.E_ALIAS and b"w2" in err()
    assert fwd(out=b2 + 4) == _hip.E_ALIAS and b"b2" in err()

    for kw, name in ((dict(z=None), b"z"), (dict(w2=None), b"w2"), (dict(g=None), b"grad_out"),
                     (dict(ws=None), b"workspace")):
        assert bwd(**kw) == _hip.E_NULL and name in err(), (kw, err())
    assert bwd(gz=None, gw=None, gb=None) == _hip.E_NULL and b"all null" in err()
    assert bwd(M=0) == _hip.E_SHAPE and b"M=0" in err()
    assert bwd(z=z + 8) == _hip.E_ALIGN and b"z" in err()
    assert bwd(w2=w2 + 4) == _hip.E_ALIGN and b"w2" in err()
    assert bwd(g=g + 2) == _hip.E_ALIGN and b"grad_out" in err()
    assert bwd(gz=gz + 4) == _hip.E_ALIGN and b"grad_z" in err()
    assert bwd(gw=gw + 2) == _hip.E_ALIGN and b"grad_w2" in err()
    assert bwd(gb=gb + 1) == _hip.E_ALIGN and b"grad_b2" in err()
    assert bwd(ws=ws + 4) == _hip.E_ALIGN and b"workspace" in err()
    # every alias pair: an output or the workspace over an input or another output
    assert bwd(gz=z) == _hip.E_ALIAS and b"grad_z" in err() and b"z" in err()
    assert bwd(gz=w2 - 512) == _hip.E_ALIAS and b"grad_z" in err() and b"w2" in err()
    assert bwd(gz=g - 1008) == _hip.E_ALIAS and b"grad_z" in err() and b"grad_out" in err()
    assert bwd(gw=z + 16) == _hip.E_ALIAS and b"grad_w2" in err()
    assert bwd(gw=w2) == _hip.E_ALIAS and b"grad_w2" in err() and b"w2" in err()
    assert bwd(gw=g + 4) == _hip.E_ALIAS and b"grad_w2" in err() and b"grad_out" in err()
    assert bwd(gb=z + 1020) == _hip.E_ALIAS and b"grad_b2" in err()
    assert bwd(gb=w2 + 764) == _hip.E_ALIAS and b"grad_b2" in err() and b"w2" in err()
    assert bwd(gb=g + 44) == _hip.E_ALIAS and b"grad_b2" in err() and b"grad_out" in err()
    assert bwd(gw=gz + 512) == _hip.E_ALIAS and b"grad_w2" in err() and b"grad_z" in err()   # two outputs overlap
    assert bwd(gb=gz + 4) == _hip.E_ALIAS and b"grad_b2" in err() and b"grad_z" in err()
    assert bwd(gb=gw + 4) == _hip.E_ALIAS and b"grad_b2" in err() and b"grad_w2" in err()
    for other in (z, w2, g, gz, gw, gb):
        assert bwd(ws=other) == _hip.E_ALIAS and b"workspace" in err(), other
    assert bwd(ws=z, gz=None) == _hip.E_ALIAS and b"workspace" in err()
    del keep


def test_upsample_and_pyramid_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, (x, out) = _buffers(2, 1 << 16)

    def err():
        return L.qpwc_last_error()

    for fn, a, b in ((L.qpwc_upsample2x_image_fwd, b"in", b"out"), (L.qpwc_upsample2x_image_bwd, b"grad_out", b"grad_in")):
        call = lambda x=x, out=out, B=1, h=4, w=5, C=3: fn(x, out, B, h, w, C, 1.0, None)
        assert call(x=None) == _hip.E_NULL and a in err()
        assert call(out=None) == _hip.E_NULL and b in err()
        assert call(B=0) == _hip.E_SHAPE and call(h=-1) == _hip.E_SHAPE and call(w=0) == _hip.E_SHAPE
        assert call(C=0) == _hip.E_SHAPE and call(C=5) == _hip.E_SHAPE and b"C=5" in err()
        assert call(h=(1 << 29) + 1) == _hip.E_SHAPE and b"doubled" in err()
        assert call(x=x + 2) == _hip.E_ALIGN and a in err()
        assert call(out=out + 1) == _hip.E_ALIGN and b in err()
        assert call(out=x + 64) == _hip.E_ALIAS and a in err() and b in err()
    up = lambda out, C: L.qpwc_upsample2x_image_fwd(x, out, 1, 4, 5, C, 1.0, None)
    assert up(out + 8, 4) == _hip.E_ALIGN and up(out + 4, 2) == _hip.E_ALIGN and b"out" in err()     # vector stores

    pool = lambda x=x, out=out, B=1, H=32, W=64, C=3, levels=5: L.qpwc_avgpool_pyramid_fwd(x, out, B, H, W, C, levels, None)
    assert pool(x=None) == _hip.E_NULL and b"x" in err()
    assert pool(out=None) == _hip.E_NULL and b"out" in err()
    assert pool(B=0) == _hip.E_SHAPE and pool(H=0) == _hip.E_SHAPE and pool(W=-2) == _hip.E_SHAPE
    assert pool(C=5) == _hip.E_SHAPE and b"C=5" in err()
    assert pool(levels=0) == _hip.E_SHAPE and b"levels=0" in err()
    assert pool(levels=IP["kApMaxLevels"] + 1, H=256, W=256) == _hip.E_SHAPE and b"levels=7" in err()
    assert pool(H=48) == _hip.E_SHAPE and b"multiples" in err()
    assert pool(W=72) == _hip.E_SHAPE and b"multiples" in err()
    assert pool(H=33, levels=1) == _hip.E_SHAPE
    assert pool(x=x + 4) == _hip.E_ALIGN and b"x" in err()
    assert pool(out=out + 2) == _hip.E_ALIGN and b"out" in err()
    assert pool(out=x + 1024) == _hip.E_ALIAS and b"out" in err() and b"x" in err()
    del keep


def test_formulas_of_the_header():
    """grad_z / grad_w2 / grad_b2 of include/qpwc.h written out against autograd of the composite, and the pyramid as a
    mean of means in row-major order."""
    gen = torch.Generator().manual_seed(1)
    z, w2, b2 = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((2, 3, 2, 64), (3, 64, 1, 1), (3,)))
    g = torch.randn(2, 3, 2, 3, generator=gen, dtype=torch.float64)
    leaves = [t.clone().requires_grad_() for t in (z, w2, b2)]
    head_composite(*leaves).backward(g)
    G, Z = g.reshape(-1, 3), z.reshape(-1, 64)
    assert torch.allclose(leaves[0].grad.reshape(-1, 64), G @ w2.reshape(3, 64), atol=1e-12)
    assert torch.allclose(leaves[1].grad.reshape(3, 64), G.t() @ Z, atol=1e-12)
    assert torch.allclose(leaves[2].grad, G.sum(0), atol=1e-12)
    assert torch.autograd.gradcheck(head_composite, [t.detach().requires_grad_() for t in leaves], eps=1e-7, atol=1e-6)
    x = torch.randn(1, 8, 4, 2, generator=gen, dtype=torch.float64)
    lvl = x
    for _ in range(2):
        lvl = (((lvl[:, 0::2, 0::2] + lvl[:, 0::2, 1::2]) + lvl[:, 1::2, 0::2]) + lvl[:, 1::2, 1::2]) * 0.25
    assert torch.allclose(pyramid_composite(x, 2), lvl, atol=1e-15) and lvl.shape == (1, 2, 1, 2)


def test_the_ops_refuse_what_they_cannot_take():
    from qpwcnet_amd import ops
    z, w2, b2 = torch.zeros(1, 2, 2, 64), torch.zeros(3, 64, 1, 1), torch.zeros(3)
    for grad in (False, True):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.image_head(z.clone().requires_grad_(grad), w2, b2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.upsample2x_image(torch.zeros(1, 2, 2, 3).requires_grad_(grad))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.avgpool_pyramid(torch.zeros(1, 32, 32, 3), 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.image_head_bwd(z, w2, torch.zeros(1, 2, 2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.upsample2x_image_bwd(torch.zeros(1, 4, 4, 3))


def test_operand_rules(monkeypatch):
    """fp16 storage and bad shapes, with the device check out of the way."""
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    z, w2, b2 = torch.zeros(1, 2, 2, 64), torch.zeros(3, 64, 1, 1), torch.zeros(3)
    for grad in (False, True):
        with pytest.raises(ValueError, match="fp16"):
            ops.image_head(z.half().requires_grad_(grad), w2, b2)
        with pytest.raises(ValueError, match="fp16"):
            ops.image_head(z.clone().requires_grad_(grad), w2.half(), b2)
        with pytest.raises(ValueError, match="fp16"):
            ops.upsample2x_image(torch.zeros(1, 2, 2, 3).half().requires_grad_(grad))
        with pytest.raises(ValueError, match="1..4 channels"):
            ops.upsample2x_image(torch.zeros(1, 2, 2, 5).requires_grad_(grad))
        with pytest.raises(ValueError, match=r"\(B,H,W,64\)"):
            ops.image_head(torch.zeros(1, 2, 2, 32).requires_grad_(grad), w2, b2)
    with pytest.raises(ValueError, match=r"\(B,H,W,64\)"):
        ops.image_head(z, torch.zeros(2, 64), b2)
    with pytest.raises(ValueError, match="fp16"):
        ops.avgpool_pyramid(torch.zeros(1, 32, 32, 3).half(), 5)
    with pytest.raises(ValueError, match="no gradient"):
        ops.avgpool_pyramid(torch.zeros(1, 32, 32, 3, requires_grad=True), 5)
    with pytest.raises(ValueError, match="levels >= 1"):
        ops.avgpool_pyramid(torch.zeros(1, 32, 32, 3), 0)
    with pytest.raises(ValueError, match="grad_out"):
        ops.image_head_bwd(z, w2, torch.zeros(1, 2, 2, 2))
    with pytest.raises(ValueError, match="nothing asked"):
        ops.image_head_bwd(z, w2, torch.zeros(1, 2, 2, 3), need=(False, False, False))
    with pytest.raises(ValueError, match="2h,2w"):
        ops.upsample2x_image_bwd(torch.zeros(1, 3, 4, 3))


def test_the_grad_paths_refuse_graph_capture(monkeypatch):
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    z, w2, b2 = torch.zeros(1, 2, 2, 64, requires_grad=True), torch.zeros(3, 64, 1, 1), torch.zeros(3)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.image_head(z, w2, b2)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.upsample2x_image(torch.zeros(1, 2, 2, 3, requires_grad=True))
    ctx = types.SimpleNamespace(saved_tensors=(z.detach(), w2), needs_input_grad=(True, True, True), scale=1.0,
                                b2_shape=(3,))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._ImageHeadFn.backward(ctx, torch.zeros(1, 2, 2, 3))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._ImageHeadFn.forward(ctx, z.detach(), w2, b2)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._UpsampleImageFn.backward(ctx, torch.zeros(1, 4, 4, 3))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._UpsampleImageFn.forward(ctx, torch.zeros(1, 2, 2, 3), 1.0)


def test_layer_names_are_those_of_the_checkpoint():
    from qpwcnet_amd import layers
    weights = {k: v for k, v in synth.make_interpolator_weights(42, (64, 96)).items() if "#" not in k}
    net = layers.InterpolatorModel()
    assert sorted(net.state_dict()) == sorted(weights)
    res = net.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()})
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(net.img[3].conv1.pointwise.weight.detach(), torch.as_tensor(weights["img.3.conv1.pointwise.weight"]))
    assert torch.equal(net.img[0].conv2.bias.detach(), torch.as_tensor(weights["img.0.conv2.bias"]))
    assert [b.conv1.in_channels for b in net.img] == [10, 519, 263, 135, 71] and [b.up for b in net.img] == [False] + [True] * 4
    assert all(tuple(b.conv2.weight.shape) == (3, 64, 1, 1) and b.conv1.filters == 64 for b in net.img)
    assert sorted(layers.FrameInterpolate(16, up=True).state_dict()) == [
        "conv1.bias", "conv1.depthwise.weight", "conv1.pointwise.weight", "conv2.bias", "conv2.weight"]
    # the flow-to-interpolator weight transfer: a FlowerModel state dict leaves only img.* missing
    flower = layers.FlowerModel()
    res = net.load_state_dict(flower.state_dict(), strict=False)
    assert not res.unexpected_keys and res.missing_keys and all(k.startswith("img.") for k in res.missing_keys)
    assert sorted(res.missing_keys) == sorted(k for k in weights if k.startswith("img."))
    assert torch.equal(net.upflow[2].flow.conv.weight.detach(), flower.upflow[2].flow.conv.weight.detach())
    small = layers.InterpolatorModel((16, 32, 64), (32,))
    assert {k.split(".")[0] for k in small.state_dict()} == {"enc", "dec", "flow", "upflow", "img"}
    assert len(small.img) == 2 and small.img[1].in_channels == 64
    assert net.eval() is net and not net.flow.flow.training and net.train() is net and net.upflow[0].flow.training


def test_config_round_trip_initialisers_and_refusals():
    from qpwcnet_amd import layers
    blk = layers.FrameInterpolate(32, up=True, name="i")
    assert blk.get_config() == {"name": "i", "in_channels": 32, "up": True}
    assert layers.FrameInterpolate.from_config(blk.get_config()).get_config() == blk.get_config()
    assert float(blk.conv2.bias.detach().abs().max()) == 0.0 and float(blk.conv1.bias.detach().abs().max()) == 0.0
    lim = (6.0 / (64 + 3)) ** 0.5
    assert 0.5 * lim < float(blk.conv2.weight.detach().abs().max()) <= lim              # Glorot uniform
    net = layers.InterpolatorModel((16, 32, 64), (32,), output_multiscale=False, data_format="channels_first")
    assert net.get_config() == {"name": None, "enc_filters": (16, 32, 64), "dec_filters": (32,),
                                "output_multiscale": False}
    assert layers.InterpolatorModel.from_config(net.get_config()).get_config() == net.get_config()
    assert layers.InterpolatorModel().get_config()["output_multiscale"] is True
    with pytest.raises(ValueError, match="InterpolatorModel"):
        layers.InterpolatorModel((16, 32), (32, 16))
    with pytest.raises(ValueError):
        layers.InterpolatorModel((16, 32, 64), (64, 32, 16))
    with pytest.raises(ValueError):
        layers.FrameInterpolate(0)
    with pytest.raises(TypeError):
        layers.FrameInterpolate(3, False, 7)
    # CPU tensors: no fallback; wrong shapes are named
    frames, flo = torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layers.FrameInterpolate(3, data_format="channels_last")((frames, frames, flo, flo))
    with pytest.raises(ValueError, match="shapes"):
        layers.FrameInterpolate(3, data_format="channels_last")((frames, frames, flo))
    with pytest.raises(ValueError, match="shapes"):
        layers.FrameInterpolate(3, up=True, data_format="channels_last")((frames, frames, flo, flo, flo))
    with pytest.raises((RuntimeError, ValueError), match="no CPU fallback"):
        net(torch.zeros(1, 6, 32, 48))
    with pytest.raises(ValueError, match="6 channels"):
        net(torch.zeros(1, 3, 32, 48))


def test_training_case_drift_is_what_the_gpu_bound_was_derived_from():
    """The fp32 CPU composite against the float64 one over the 5 SGD steps of test_short_training_run: the drift the
    GPU test's bound (10 x) was set from; the float64 loss falls at every step and every parameter moves by far more
    than the bound.  The figure moves a little with the host's BLAS and thread count, hence the factor 2 either way."""
    ref, losses = train_composite(torch.float64)
    got, _ = train_composite(torch.float32)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    drift = max(float((got[n].double() - ref[n]).abs().max()) for n in ref)
    print("drift {:.3e}".format(drift))
    assert TRAIN_DRIFT / 2 <= drift <= 2 * TRAIN_DRIFT, drift
    net, _, _, lr = train_case()
    start = dict(net.named_parameters())
    assert {_rate(n, lr) for n in start} == set(lr) and sorted(start) == sorted(ref)
    moved = {n: float((ref[n] - start[n].detach().double()).abs().max()) for n in ref}
    print("least moved: {}".format(sorted(moved.items(), key=lambda kv: kv[1])[:3]))
    assert min(moved.values()) > 10 * TRAIN_BOUND, moved


def test_multi_trip_case_loops_past_every_cap():
    B, H, W = MULTI_TRIP
    M = B * H * W
    # image_head_fwd_kernel / image_head_bwd_kernel: kIhPx pixels per workgroup and trip over at most kIhBlocks workgroups
    trips = -(-M // IP["kIhPx"])
    assert M > IP["kIhBlocks"] * IP["kIhPx"] and trips % IP["kIhBlocks"] and M % IP["kIhPx"], (M, trips)
    # conv_bwd_reduce_kernel: kCgRedLanes lanes stride over the kIhBlocks partials of an output
    assert IP["kIhBlocks"] > RED_LANES and IP["kIhBlocks"] % RED_LANES
    # upsample2x_image_kernel: 256 output pixels per trip; upsample2x_image_bwd_kernel: 256 input pixels per trip
    for pixels, cap in ((4 * M, IP["kUiBlocks"]), (M, IP["kUiBwdBlocks"])):
        trips = -(-pixels // 256)
        assert pixels > cap * 256 and trips % cap and pixels % 256, (pixels, cap)
    # a launch of a few hundred thousand pixels makes more than one trip of each
    assert max(IP["kIhBlocks"] * IP["kIhPx"], IP["kUiBlocks"] * 256, IP["kUiBwdBlocks"] * 256) < 300000

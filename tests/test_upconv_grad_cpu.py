"""CPU suite of the decoder transposed convolution's backward: qpwc_upconv4x4s2_bwd and its workspace query refuse bad
arguments before any HIP call, the float64 composite oracle of tests/test_gpu_upconv_grad.py is the true derivative,
the grad path refuses CPU tensors / fp16 / bf16x3 / non-dense inputs / capture, the layers carry the state-dict names of
weights.py, and the GPU suite's "more than one trip" shape still loops against the constants of csrc/upconv_bwd.hip."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import types

import pytest
import torch

from qpwcnet_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_upconv_grad import MULTI_TRIP, TRAIN_BOUND, TRAIN_DRIFT, _rate, composite, train_case, train_composite  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")
VP = ctypes.c_void_p


def _constants(name, *keys):
    text = open(os.path.join(CSRC, name)).read()
    out = {}
    for k in keys:
        m = re.findall(r"constexpr\s+int\s+{}\s*=\s*(\d+)\s*[;,]".format(k), text)
        assert len(m) == 1, (name, k, m)
        out[k] = int(m[0])
    return out


UB = _constants("upconv_bwd.hip", "kUbPx", "kUbKC", "kUbWBlocks", "kUbWTile", "kUbRedLanes")


def _plan(B, H, W, C, F):
    """ub_plan() of upconv_bwd.hip -> (input-pixel blocks, K-splits, workspace floats)."""
    M = B * H * W
    n_pb = -(-M // UB["kUbPx"])
    blocks = (F // min(F, UB["kUbWTile"])) * (C // UB["kUbWTile"])
    nsplit = min(n_pb, max(1, UB["kUbWBlocks"] // (16 * blocks)))
    up4 = lambda n: -(-n // 4) * 4
    return n_pb, nsplit, 4 * M * F + nsplit * 16 * F * C + up4(nsplit * F)


def test_symbols_present(hip_lib):
    from qpwcnet_amd import _hip
    for name in ("qpwc_upconv4x4s2_bwd", "qpwc_upconv4x4s2_bwd_workspace_floats"):
        assert name in _hip.SYMBOLS and getattr(hip_lib, name) is not None


def test_workspace_floats(hip_lib):
    from qpwcnet_amd import _hip
    ws = hip_lib.qpwc_upconv4x4s2_bwd_workspace_floats
    for shape in ((1, 3, 5, 64, 16), (2, 7, 9, 128, 32), (1, 1, 1, 64, 16), (1, 3, 4, 256, 128), MULTI_TRIP,
                  (16, 8, 16, 256, 128), (16, 16, 32, 256, 64), (16, 32, 64, 128, 32), (16, 64, 128, 64, 16)):
        assert ws(*shape) == _plan(*shape)[2], shape
    # the extremes of the split: the K-splits come from the shape alone and bound the workspace
    assert _plan(16, 64, 128, 64, 16)[:2] == (2048, 60) and _plan(16, 8, 16, 256, 128)[:2] == (32, 7)
    assert _plan(1, 1, 1, 64, 16)[:2] == (1, 1)
    assert ws(0, 7, 11, 64, 16) == _hip.E_SHAPE
    assert ws(1, 7, -1, 64, 16) == _hip.E_SHAPE
    assert ws(1, 7, 11, 32, 16) == _hip.E_SHAPE and b"C=32" in hip_lib.qpwc_last_error()
    assert ws(1, 7, 11, 64, 48) == _hip.E_SHAPE and b"F=48" in hip_lib.qpwc_last_error()
    assert ws(1, 7, 11, 64, 256) == _hip.E_SHAPE and b"F=256" in hip_lib.qpwc_last_error()


def test_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep = (ctypes.c_float * (1 << 18))()
    base = ctypes.cast(keep, VP).value
    base += (-base) % 16
    # (1,2,2) pixels, 64 -> 16 channels: each buffer 96 KiB apart
    x, w, b, gout, gx, gw, gb, ws = (base + 98304 * i for i in range(8))
    assert L.qpwc_upconv4x4s2_bwd_workspace_floats(1, 2, 2, 64, 16) * 4 <= 98304 and 16 * 16 * 64 * 4 <= 98304

    def bwd(x=x, w=w, b=b, gout=gout, gs=16, gx=gx, gw=gw, gb=gb, ws=ws, B=1, H=2, W=2, C=64, F=16, mish=1):
        return L.qpwc_upconv4x4s2_bwd(x, w, b, gout, gs, gx, gw, gb, ws, B, H, W, C, F, mish, None)

    def err():
        return L.qpwc_last_error()

    for kw, name in ((dict(x=None), b"x"), (dict(w=None), b"weight"), (dict(b=None), b"bias"),
                     (dict(gout=None), b"grad_out"), (dict(ws=None), b"workspace")):
        assert bwd(**kw) == _hip.E_NULL and name in err(), (kw, err())
    assert bwd(gx=None, gw=None, gb=None) == _hip.E_NULL and b"all null" in err()
    assert bwd(C=32) == _hip.E_SHAPE and b"C=32" in err()
    assert bwd(F=24) == _hip.E_SHAPE and b"F=24" in err()
    assert bwd(mish=2) == _hip.E_SHAPE and b"mish=2" in err()
    assert bwd(H=0) == _hip.E_SHAPE and bwd(B=-1) == _hip.E_SHAPE and bwd(W=0) == _hip.E_SHAPE
    assert bwd(gs=12) == _hip.E_SHAPE and b"grad_out_pixel_stride=12" in err()          # < F
    assert bwd(gs=18) == _hip.E_SHAPE and b"grad_out_pixel_stride=18" in err()          # not a multiple of 4
    assert bwd(gs=-16) == _hip.E_SHAPE
    assert bwd(x=x + 4) == _hip.E_ALIGN and b"x" in err()
    assert bwd(w=w + 4) == _hip.E_ALIGN and b"weight" in err()
    assert bwd(b=b + 2) == _hip.E_ALIGN and b"bias" in err()
    assert bwd(gout=gout + 8) == _hip.E_ALIGN and b"grad_out" in err()
    assert bwd(gx=gx + 4) == _hip.E_ALIGN and b"grad_x" in err()
    assert bwd(gw=gw + 4) == _hip.E_ALIGN and b"grad_w" in err()
    assert bwd(gb=gb + 2) == _hip.E_ALIGN and b"grad_b" in err()
    assert bwd(ws=ws + 4) == _hip.E_ALIGN and b"workspace" in err()
    # every alias pair: an output or the workspace over an input or another output
    assert bwd(gx=x) == _hip.E_ALIAS and b"grad_x" in err() and b"x" in err()
    assert bwd(gx=w + 16) == _hip.E_ALIAS and b"grad_x" in err() and b"weight" in err()
    assert bwd(gx=b - 64) == _hip.E_ALIAS and b"grad_x" in err() and b"bias" in err()
    assert bwd(gx=gout) == _hip.E_ALIAS and b"grad_x" in err() and b"grad_out" in err()
    assert bwd(gw=x) == _hip.E_ALIAS and b"grad_w" in err()
    assert bwd(gw=w) == _hip.E_ALIAS and b"grad_w" in err() and b"weight" in err()
    assert bwd(gw=b - 64) == _hip.E_ALIAS and b"grad_w" in err() and b"bias" in err()
    assert bwd(gw=gout + 16) == _hip.E_ALIAS and b"grad_w" in err() and b"grad_out" in err()
    assert bwd(gb=x + 16) == _hip.E_ALIAS and b"grad_b" in err()
    assert bwd(gb=w + 32) == _hip.E_ALIAS and b"grad_b" in err() and b"weight" in err()
    assert bwd(gb=b) == _hip.E_ALIAS and b"grad_b" in err() and b"bias" in err()
    assert bwd(gb=gout + 16) == _hip.E_ALIAS and b"grad_b" in err() and b"grad_out" in err()
    assert bwd(gw=gx + 16) == _hip.E_ALIAS and b"grad_w" in err() and b"grad_x" in err()     # two outputs overlap
    assert bwd(gb=gx + 32) == _hip.E_ALIAS and b"grad_b" in err() and b"grad_x" in err()
    assert bwd(gb=gw + 32) == _hip.E_ALIAS and b"grad_b" in err() and b"grad_w" in err()
    for other in (x, w, b, gout, gx, gw, gb):
        assert bwd(ws=other) == _hip.E_ALIAS and b"workspace" in err(), other
    assert bwd(ws=x, gx=None) == _hip.E_ALIAS and b"workspace" in err()
    # the pixel stride stretches grad_out: 16 pixels 1536 floats apart reach a grad_x that lies 64 KiB further on
    assert bwd(gs=1536, gx=gout + 65536) == _hip.E_ALIAS and b"grad_x" in err() and b"grad_out" in err()


@pytest.mark.parametrize("hw,mish", [((3, 4), True), ((2, 5), False), ((1, 1), True), ((1, 3), True)])
def test_gradcheck_composite_oracle(hw, mish):
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_()
    x, w, b = r(2, hw[0], hw[1], 3), r(3, 4, 4, 4), r(4)
    assert composite(x, w, b, mish).shape == (2, 2 * hw[0], 2 * hw[1], 4)
    assert torch.autograd.gradcheck(lambda *a: composite(*a, mish), (x, w, b), eps=1e-7, atol=1e-6)


def test_formulas_of_the_header():
    """grad_x / grad_w / grad_b of include/qpwc.h, written out as loops, against autograd of the composite (mish off)."""
    gen = torch.Generator().manual_seed(1)
    B, H, W, C, F_ = 2, 3, 2, 3, 2
    x, w, b = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((B, H, W, C), (C, F_, 4, 4), (F_,)))
    g = torch.randn(B, 2 * H, 2 * W, F_, generator=gen, dtype=torch.float64)
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    composite(*leaves, False).backward(g)
    gx, gw = torch.zeros_like(x), torch.zeros_like(w)
    for ky in range(4):
        for kx in range(4):
            for iy in range(H):
                for ix in range(W):
                    oy, ox = 2 * iy - 1 + ky, 2 * ix - 1 + kx
                    if 0 <= oy < 2 * H and 0 <= ox < 2 * W:
                        gx[:, iy, ix, :] += g[:, oy, ox, :] @ w[:, :, ky, kx].t()
                        gw[:, :, ky, kx] += x[:, iy, ix, :].t() @ g[:, oy, ox, :]
    assert torch.allclose(gx, leaves[0].grad, atol=1e-12) and torch.allclose(gw, leaves[1].grad, atol=1e-12)
    assert torch.allclose(g.sum(dim=(0, 1, 2)), leaves[2].grad, atol=1e-12)


def _operands(dtype=torch.float32, C=64, F_=16):
    return torch.zeros(1, 2, 2, C, dtype=dtype, requires_grad=True), torch.zeros(C, F_, 4, 4, dtype=dtype), \
        torch.zeros(F_, dtype=dtype)


def test_the_grad_path_refuses_what_it_cannot_differentiate():
    from qpwcnet_amd import layers, ops
    with pytest.raises(ValueError, match="HIP device"):
        ops.upconv4x4s2(*_operands())
    with pytest.raises(ValueError, match="HIP device"):
        layers.UpConv(64, 16, data_format="channels_last")(torch.zeros(1, 2, 2, 64))
    with pytest.raises(ValueError, match="bf16x3"):
        ops.upconv4x4s2(*_operands(), matmul="bf16x3")
    with pytest.raises(ValueError, match="does not fit"):
        ops.upconv4x4s2(_operands()[0], torch.zeros(128, 16, 4, 4), torch.zeros(16))


def test_operand_rules_of_the_grad_path(monkeypatch):
    """fp16 storage, a non-dense x, unsupported widths and a bad skip, with the device check out of the way."""
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    x, w, b = _operands()
    taps = torch.zeros(16, 16, 64)
    with pytest.raises(ValueError, match="fp16"):
        ops._upconv_check(x.detach().half(), taps.half(), b, "upconv4x4s2")
    with pytest.raises(ValueError, match="dense"):
        ops._upconv_check(torch.zeros(1, 64, 2, 2).permute(0, 2, 3, 1), taps, b, "upconv4x4s2")
    with pytest.raises(ValueError, match="outside"):
        ops._upconv_check(torch.zeros(1, 2, 2, 32), torch.zeros(16, 16, 32), b, "upconv4x4s2")
    with pytest.raises(ValueError, match="outside"):
        ops._upconv_check(x.detach(), torch.zeros(16, 48, 64), torch.zeros(48), "upconv4x4s2")
    assert ops._upconv_check(torch.zeros(2, 5, 7, 128), torch.zeros(16, 32, 128), torch.zeros(32), "x") == (2, 5, 7, 128, 32)
    assert ops._upconv_check(torch.zeros(2, 5, 7, 128), torch.zeros(128, 32, 4, 4), torch.zeros(32), "x") == (2, 5, 7, 128, 32)
    with pytest.raises(ValueError, match="fp16"):
        ops.upconv4x4s2(x.detach().half().requires_grad_(), w.half(), b)
    with pytest.raises(ValueError, match="dense"):
        ops.upconv4x4s2(torch.zeros(1, 64, 2, 2).permute(0, 2, 3, 1).requires_grad_(), w, b)
    with pytest.raises(ValueError, match="skip"):
        ops.upconv4x4s2(x, w, b, torch.zeros(1, 4, 4, 6))
    with pytest.raises(ValueError, match="skip"):
        ops.upconv4x4s2(x, w, b, torch.zeros(1, 4, 5, 16))
    with pytest.raises(ValueError, match="grad_out"):
        ops.upconv4x4s2_bwd(x.detach(), taps, b, torch.zeros(1, 4, 4, 8))
    with pytest.raises(ValueError, match="nothing asked"):
        ops.upconv4x4s2_bwd(x.detach(), taps, b, torch.zeros(1, 4, 4, 16), need=(False, False, False))


def test_the_grad_path_refuses_graph_capture(monkeypatch):
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.upconv4x4s2(*_operands())
    ctx = types.SimpleNamespace(saved_tensors=(), needs_input_grad=(True, True, True, False))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._UpConvFn.backward(ctx, torch.zeros(1, 4, 4, 16))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._UpConvFn.forward(ctx, *_operands(), None)


def test_layer_names_are_those_of_the_checkpoint():
    from qpwcnet_amd import layers
    weights = {k: v for k, v in synth.make_weights(42, (64, 96)).items() if "#" not in k}
    want = sorted(k for k in weights if k.startswith("dec."))
    dec = layers.Decoder()
    assert sorted(dec.state_dict()) == want and len(want) == 8
    assert sorted(layers.UpConv(256, 128).state_dict()) == ["conv_up.bias", "conv_up.weight"]
    res = dec.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()}, strict=False)
    assert not res.missing_keys
    assert torch.equal(dec.dec[2].conv_up.weight.detach(), torch.as_tensor(weights["dec.2.conv_up.weight"]))
    assert [tuple(l.conv_up.weight.shape) for l in dec.dec] == [(256, 128, 4, 4), (256, 64, 4, 4), (128, 32, 4, 4),
                                                                (64, 16, 4, 4)]
    net = layers.FlowerModel()
    assert sorted(net.state_dict()) == sorted(weights)
    res = net.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()})
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(net.upflow[3].flow.flow.weight.detach(), torch.as_tensor(weights["upflow.3.flow.flow.weight"]))
    assert torch.equal(net.upflow[1].flow.norm.var, torch.as_tensor(weights["upflow.1.flow.norm.var"]))
    small = layers.FlowerModel((16, 32, 64), (32,))
    assert {k.split(".")[0] for k in small.state_dict()} == {"enc", "dec", "flow", "upflow"}
    assert tuple(small.dec[0].conv_up.weight.shape) == (64, 32, 4, 4) and small.upflow[0].in_channels == 64
    # train() / eval() reach the BatchNorm mode of every OptFlow
    assert net.eval() is net and not net.flow.flow.training and not any(u.flow.training for u in net.upflow)
    assert net.train() is net and net.flow.flow.training and all(u.flow.training for u in net.upflow)


def test_config_round_trip_and_initialisers():
    from qpwcnet_amd import layers
    lay = layers.UpConv(128, 32, name="u")
    assert lay.get_config() == {"name": "u", "in_channels": 128, "filters": 32}
    assert layers.UpConv.from_config(lay.get_config()).get_config() == lay.get_config()
    assert float(lay.conv_up.bias.detach().abs().max()) == 0.0 and tuple(lay.conv_up.bias.shape) == (32,)
    lim = (6.0 / (16 * 128 + 16 * 32)) ** 0.5
    assert 0.5 * lim < float(lay.conv_up.weight.detach().abs().max()) <= lim              # Glorot uniform
    dec = layers.Decoder((64, 32), in_channels=128, skip_channels=(64, 32), name="d")
    assert dec.get_config() == {"name": "d", "filters": (64, 32), "in_channels": 128, "skip_channels": (64, 32)}
    assert layers.Decoder.from_config(dec.get_config()).get_config() == dec.get_config()
    assert [l.in_channels for l in dec.dec] == [128, 128]
    plain = layers.Decoder((128, 64), in_channels=256, skip_channels=None)               # use_skip=False
    assert [l.in_channels for l in plain.dec] == [256, 128] and plain.get_config()["skip_channels"] is None
    net = layers.FlowerModel((16, 32, 64), (32,), data_format="channels_first")
    assert net.get_config() == {"name": None, "enc_filters": (16, 32, 64), "dec_filters": (32,)}
    assert layers.FlowerModel.from_config(net.get_config()).get_config() == net.get_config()
    lim = (6.0 / (16 * 64 + 16 * 32)) ** 0.5
    assert 0.5 * lim < float(net.dec[0].conv_up.weight.detach().abs().max()) <= lim
    for bad in ((32, 16), (64, 48), (64, 256)):
        with pytest.raises(ValueError):
            layers.UpConv(*bad)
    with pytest.raises(ValueError):
        layers.Decoder((64, 32), in_channels=128, skip_channels=(64,))
    with pytest.raises(ValueError):
        layers.Decoder(skip_channels=None)             # without skips the fourth level's input holds 32 channels: too narrow
    with pytest.raises(ValueError):
        layers.FlowerModel((16, 32), (32, 16))


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
    B, H, W, C, F_ = MULTI_TRIP
    n_pb, nsplit, _ = _plan(*MULTI_TRIP)
    M = B * H * W
    # upconv_bwd_w_kernel: input-pixel blocks in grid-stride order over nsplit workgroups per (block, tap)
    assert n_pb > nsplit and n_pb % nsplit, (n_pb, nsplit)
    assert M % UB["kUbPx"], "no partial last pixel block"
    # conv_bwd_reduce_kernel (stage R of both files): kUbRedLanes lanes stride over the nsplit partials of an output
    assert nsplit > UB["kUbRedLanes"] and nsplit % UB["kUbRedLanes"], nsplit
    # upconv_bwd_gemm_kernel: more than one workgroup of rows, the last one partial (stages Z and X share the row
    # space), and more than one K step per tap in stage Z (K = C)
    assert M > UB["kUbPx"] and C > UB["kUbKC"]


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernels_use_no_scratch(tmp_path):
    """Every kernel of upconv_bwd.hip compiles for gfx950 without scratch memory and the products are on the fp32
    matrix instruction.  Its stage R is conv_bwd_reduce_kernel, which tests/test_conv_grad_cpu.py covers."""
    s = tmp_path / "upconv_bwd.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "upconv_bwd.hip"), "-o", str(s)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    assert len(names) == len(scratch) == 6 and all("upconv_bwd" in n for n in names), names
    assert not any(scratch), dict(zip(names, scratch))
    assert "v_mfma_f32_16x16x4_f32" in s.read_text()

"""CPU suite of the encoder convolution's backward: qpwc_conv3x3_same_fwd / _bwd and the workspace query refuse bad
arguments before any HIP call, the float64 composite oracle of tests/test_gpu_conv_grad.py is the true derivative, the
grad path refuses CPU tensors / fp16 / bf16x3 / non-dense inputs / capture, the layers carry the state-dict names of
weights.py, and the GPU suite's "more than one trip" shapes still loop against the constants of csrc/conv_bwd.hip."""
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
from test_gpu_conv_grad import MULTI_TRIP, TRAIN_DRIFT, composite, same_pad, train_case, train_composite  # noqa: E402

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


CB = _constants("conv_bwd.hip", "kCbPx", "kCbWBlocks", "kCbWTile", "kCbRedLanes")


def _plan(B, H, W, ci, co, s):
    """cb_plan() of conv_bwd.hip -> (pixel blocks, K-splits, workspace floats)."""
    Ho, Wo = -(-H // s), -(-W // s)
    M, cp, ci16 = B * Ho * Wo, -(-ci // 4) * 4, max(ci, 16)
    n_pb = -(-M // CB["kCbPx"])
    blocks = (co // min(co, CB["kCbWTile"])) * (ci16 // min(ci16, CB["kCbWTile"]))
    nsplit = min(n_pb, max(1, CB["kCbWBlocks"] // (9 * blocks)))
    up4 = lambda n: -(-n // 4) * 4
    return n_pb, nsplit, M * co + nsplit * 9 * co * cp + up4(nsplit * co)


def test_symbols_present(hip_lib):
    from qpwcnet_amd import _hip
    for name in ("qpwc_conv3x3_same_fwd", "qpwc_conv3x3_same_bwd", "qpwc_conv3x3_same_bwd_workspace_floats"):
        assert name in _hip.SYMBOLS and getattr(hip_lib, name) is not None


def test_workspace_floats(hip_lib):
    from qpwcnet_amd import _hip
    ws = hip_lib.qpwc_conv3x3_same_bwd_workspace_floats
    for shape in ((1, 7, 11, 16, 16, 1), (2, 7, 11, 16, 32, 2), (1, 8, 12, 3, 16, 2), (16, 256, 512, 3, 16, 2),
                  (16, 128, 256, 16, 16, 1), (16, 16, 32, 128, 256, 2), (16, 8, 16, 256, 256, 1), (1, 1, 1, 16, 32, 2)):
        assert ws(*shape) == _plan(*shape)[2], shape
    # the extremes of the split: the K-splits come from the shape alone and bound the workspace
    assert _plan(16, 128, 256, 16, 16, 1)[:2] == (8192, 113) and _plan(16, 8, 16, 256, 256, 1)[:2] == (32, 7)
    assert ws(0, 7, 11, 16, 16, 1) == _hip.E_SHAPE
    assert ws(1, 7, -1, 16, 16, 1) == _hip.E_SHAPE
    assert ws(1, 7, 11, 8, 16, 1) == _hip.E_SHAPE and b"C_in=8" in hip_lib.qpwc_last_error()
    assert ws(1, 7, 11, 16, 3, 1) == _hip.E_SHAPE and b"C_out=3" in hip_lib.qpwc_last_error()
    assert ws(1, 7, 11, 16, 16, 3) == _hip.E_SHAPE and b"stride=3" in hip_lib.qpwc_last_error()


def test_conv_same_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep = (ctypes.c_float * (1 << 18))()
    base = ctypes.cast(keep, VP).value
    base += (-base) % 16
    # (1,4,4) pixels, 16 -> 16 channels: each buffer 64 KiB apart
    x, w, b, gout, gx, gw, gb, ws, out = (base + 65536 * i for i in range(9))
    assert L.qpwc_conv3x3_same_bwd_workspace_floats(1, 4, 4, 16, 16, 1) * 4 <= 65536

    def bwd(x=x, w=w, b=b, gout=gout, gx=gx, gw=gw, gb=gb, ws=ws, B=1, H=4, W=4, ci=16, co=16, s=1, mish=1):
        return L.qpwc_conv3x3_same_bwd(x, w, b, gout, gx, gw, gb, ws, B, H, W, ci, co, s, mish, None)

    def fwd(x=x, w=w, b=b, out=out, B=1, H=4, W=4, ci=16, co=16, s=1, mish=1):
        return L.qpwc_conv3x3_same_fwd(x, w, b, out, B, H, W, ci, co, s, mish, None)

    def err():
        return L.qpwc_last_error()

    for kw, name in ((dict(x=None), b"x"), (dict(w=None), b"weight"), (dict(b=None), b"bias"),
                     (dict(gout=None), b"grad_out"), (dict(ws=None), b"workspace")):
        assert bwd(**kw) == _hip.E_NULL and name in err(), (kw, err())
    assert bwd(gx=None, gw=None, gb=None) == _hip.E_NULL and b"all null" in err()
    for kw, name in ((dict(x=None), b"x"), (dict(w=None), b"weight"), (dict(b=None), b"bias"), (dict(out=None), b"out")):
        assert fwd(**kw) == _hip.E_NULL and name in err(), (kw, err())
    for call in (bwd, fwd):
        assert call(ci=24) == _hip.E_SHAPE and b"C_in=24" in err()
        assert call(co=3) == _hip.E_SHAPE and b"C_out=3" in err()
        assert call(s=0) == _hip.E_SHAPE and b"stride=0" in err()
        assert call(mish=2) == _hip.E_SHAPE and b"mish=2" in err()
        assert call(H=0) == _hip.E_SHAPE and call(B=-1) == _hip.E_SHAPE and call(W=0) == _hip.E_SHAPE
        assert call(x=x + 4) == _hip.E_ALIGN and b"x" in err()
        assert call(x=x + 2, ci=3) == _hip.E_ALIGN and b"x" in err()      # 12-byte pixels: 4-byte alignment
        assert call(w=w + 4) == _hip.E_ALIGN and b"weight" in err()
        assert call(b=b + 2) == _hip.E_ALIGN and b"bias" in err()
    assert fwd(out=out + 8) == _hip.E_ALIGN and b"out" in err()
    assert fwd(out=x) == _hip.E_ALIAS and b"out" in err() and b"x" in err()
    assert fwd(out=w + 16) == _hip.E_ALIAS and b"weight" in err()
    assert fwd(out=b - 64) == _hip.E_ALIAS and b"bias" in err()
    assert bwd(gout=gout + 8) == _hip.E_ALIGN and b"grad_out" in err()
    assert bwd(gx=gx + 4) == _hip.E_ALIGN and b"grad_x" in err()
    assert bwd(gw=gw + 4) == _hip.E_ALIGN and b"grad_w" in err()
    assert bwd(gb=gb + 2) == _hip.E_ALIGN and b"grad_b" in err()
    assert bwd(ws=ws + 4) == _hip.E_ALIGN and b"workspace" in err()
    assert bwd(gx=x) == _hip.E_ALIAS and b"grad_x" in err() and b"x" in err()
    assert bwd(gw=w) == _hip.E_ALIAS and b"grad_w" in err() and b"weight" in err()
    assert bwd(gb=gout + 16) == _hip.E_ALIAS and b"grad_b" in err() and b"grad_out" in err()
    assert bwd(gb=b) == _hip.E_ALIAS and b"bias" in err()
    assert bwd(gw=gx + 16) == _hip.E_ALIAS and b"grad_w" in err() and b"grad_x" in err()     # two outputs overlap
    assert bwd(gb=gw + 32) == _hip.E_ALIAS and b"grad_b" in err()
    assert bwd(ws=gx) == _hip.E_ALIAS and b"workspace" in err()
    assert bwd(ws=gout - 64) == _hip.E_ALIAS                                                  # runs into grad_out
    assert bwd(ws=x, gx=None) == _hip.E_ALIAS and b"workspace" in err()


@pytest.mark.parametrize("stride,hw,mish", [(1, (4, 5), True), (1, (3, 4), False), (2, (4, 6), True), (2, (5, 7), True),
                                            (2, (4, 5), False), (2, (1, 2), True)])
def test_gradcheck_composite_oracle(stride, hw, mish):
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_()
    x, w, b = r(2, hw[0], hw[1], 3), r(4, 3, 3, 3), r(4)
    assert composite(x, w, b, stride, mish).shape == (2, -(-hw[0] // stride), -(-hw[1] // stride), 4)
    assert torch.autograd.gradcheck(lambda *a: composite(*a, stride, mish), (x, w, b), eps=1e-7, atol=1e-6)


def test_same_padding_rule():
    assert [same_pad(n, 1) for n in (1, 2, 7)] == [(1, 1)] * 3
    assert same_pad(8, 2) == (0, 1) and same_pad(7, 2) == (1, 1) and same_pad(1, 2) == (1, 1) and same_pad(2, 2) == (0, 1)


def _operands(dtype=torch.float32, ci=16, co=16):
    return torch.zeros(1, 4, 4, ci, dtype=dtype, requires_grad=True), torch.zeros(co, ci, 3, 3, dtype=dtype), \
        torch.zeros(co, dtype=dtype)


def test_the_grad_path_refuses_what_it_cannot_differentiate():
    from qpwcnet_amd import layers, ops
    with pytest.raises(ValueError, match="HIP device"):
        ops.conv3x3_same(*_operands())
    with pytest.raises(ValueError, match="HIP device"):
        layers.DownConv(16, 16, data_format="channels_last")(torch.zeros(1, 4, 4, 16))
    with pytest.raises(ValueError, match="bf16x3"):
        ops.conv3x3_same(*_operands(), matmul="bf16x3")
    with pytest.raises(ValueError, match="does not fit"):
        ops.conv3x3_same(_operands()[0], torch.zeros(16, 32, 3, 3), torch.zeros(16))


def test_operand_rules_of_the_grad_path(monkeypatch):
    """fp16 storage, a non-dense x, a bad stride and unsupported widths, with the device check out of the way."""
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    x, w, b = _operands()
    taps = torch.zeros(9, 16, 16)
    with pytest.raises(ValueError, match="fp16"):
        ops._conv_same_check(x.detach().half(), taps.half(), b, 1, "conv3x3_same")
    with pytest.raises(ValueError, match="dense"):
        ops._conv_same_check(torch.zeros(1, 16, 4, 4).permute(0, 2, 3, 1), taps, b, 1, "conv3x3_same")
    with pytest.raises(ValueError, match="stride"):
        ops._conv_same_check(x.detach(), taps, b, 3, "conv3x3_same")
    with pytest.raises(ValueError, match="outside"):
        ops._conv_same_check(torch.zeros(1, 4, 4, 8), torch.zeros(9, 16, 8), b, 1, "conv3x3_same")
    assert ops._conv_same_check(torch.zeros(2, 5, 7, 3), torch.zeros(9, 16, 4), b, 2, "x") == (2, 5, 7, 3, 16, 3, 4)
    with pytest.raises(ValueError, match="fp16"):
        ops.conv3x3_same(x.detach().half().requires_grad_(), w.half(), b)
    with pytest.raises(ValueError, match="dense"):
        ops.conv3x3_same(torch.zeros(1, 16, 4, 4).permute(0, 2, 3, 1).requires_grad_(), w, b)


def test_the_grad_path_refuses_graph_capture(monkeypatch):
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.conv3x3_same(*_operands())
    ctx = types.SimpleNamespace(saved_tensors=(), cfg=None, needs_input_grad=(True, True, True, False, False))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._ConvSameFn.backward(ctx, torch.zeros(1, 4, 4, 16))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._ConvSameFn.forward(ctx, *_operands(), 1, True)


def test_taps_layout():
    from qpwcnet_amd import ops
    w = torch.arange(16 * 3 * 9, dtype=torch.float32).reshape(16, 3, 3, 3)
    t = ops.conv3x3_same_taps(w)
    assert torch.equal(t, ops.first_conv_taps(w)) and float(t[..., 3].abs().max()) == 0.0
    w = torch.arange(32 * 16 * 9, dtype=torch.float32).reshape(32, 16, 3, 3)
    assert torch.equal(ops.conv3x3_same_taps(w), ops.conv3x3_taps(w))
    assert float(ops.conv3x3_same_taps(w)[5, 7, 3]) == float(w[7, 3, 1, 2])


def test_layer_names_are_those_of_the_checkpoint():
    from qpwcnet_amd import layers
    want = sorted(k for k in synth.make_weights(42, (64, 96)) if k.startswith("enc.") and "#" not in k)
    enc = layers.Encoder()
    assert sorted(enc.state_dict()) == want and len(want) == 30
    assert sorted(layers.DownConv(3, 16).state_dict()) == sorted(k[len("enc.0."):] for k in want if k.startswith("enc.0."))
    weights = synth.make_weights(42, (64, 96))
    res = enc.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()}, strict=False)
    assert not res.missing_keys
    assert torch.equal(enc.enc[3].conv_b.weight.detach(), torch.as_tensor(weights["enc.3.conv_b.weight"]))
    assert enc.get_config() == {"name": None, "filters": (16, 32, 64, 128, 256), "in_channels": 3}
    lay = layers.DownConv(16, 32, name="d")
    assert layers.DownConv.from_config(lay.get_config()).get_config() == lay.get_config()
    assert float(lay.conv_a.bias.detach().abs().max()) == 0.0
    lim = (6.0 / (9 * 16 + 9 * 32)) ** 0.5
    assert 0.5 * lim < float(lay.conv_a.weight.detach().abs().max()) <= lim              # Glorot uniform
    for bad in ((8, 16), (16, 24)):
        with pytest.raises(ValueError):
            layers.DownConv(*bad)


def test_training_case_drift_is_what_the_gpu_bound_was_derived_from():
    """The fp32 CPU composite against the float64 one over the 5 SGD steps of test_short_training_run: the drift the
    GPU test's bound (10 x) was set from; the float64 loss falls at every step and every encoder parameter moves by
    far more than the bound.  The figure is about one fp32 ulp of the parameters and moves a little with the host's BLAS and
    thread count, hence the factor 2 either way."""
    ref, losses = train_composite(torch.float64)
    got, _ = train_composite(torch.float32)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    drift = max(float((got[n].double() - ref[n]).abs().max()) for n in ref)
    assert TRAIN_DRIFT / 2 <= drift <= 2 * TRAIN_DRIFT, drift
    enc, flow = train_case()[:2]
    start = dict([("e." + n, p) for n, p in enc.named_parameters()] + [("f." + n, p) for n, p in flow.named_parameters()])
    moved = {n: float((ref[n] - start[n].detach().double()).abs().max()) for n in ref}
    assert min(v for n, v in moved.items() if n.startswith("e.")) > 1000 * TRAIN_DRIFT, moved


def test_multi_trip_cases_loop_past_every_cap():
    for B, H, W, ci, co, s in MULTI_TRIP:
        n_pb, nsplit, _ = _plan(B, H, W, ci, co, s)
        M = B * -(-H // s) * -(-W // s)
        # conv_bwd_w_kernel: pixel blocks in grid-stride order over nsplit workgroups per (block, tap)
        assert n_pb > nsplit and n_pb % nsplit, (n_pb, nsplit)
        assert M % CB["kCbPx"], "no partial last pixel block"
        # conv_bwd_reduce_kernel: kCbRedLanes lanes stride over the nsplit partials of an output
        assert nsplit > CB["kCbRedLanes"] and nsplit % CB["kCbRedLanes"], nsplit
        # the gather of grad_x: more than one workgroup in its smallest parity class, the last one partial
        rows = B * (H // s) * (W // s)
        assert rows > CB["kCbPx"] and rows % CB["kCbPx"], rows


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernels_use_no_scratch(tmp_path):
    """Every kernel of conv_bwd.hip compiles for gfx950 without scratch memory and the products are on the fp32 matrix
    instruction."""
    s = tmp_path / "conv_bwd.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "conv_bwd.hip"), "-o", str(s)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    assert len(names) == len(scratch) >= 13 and all("conv_bwd" in n for n in names), names
    assert not any(scratch), dict(zip(names, scratch))
    assert "v_mfma_f32_16x16x4_f32" in s.read_text()

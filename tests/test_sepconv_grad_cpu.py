"""CPU suite of the SeparableConv2D backward: qpwc_sepconv3x3_bwd and its workspace query refuse bad arguments before
any HIP call, the float64 composite oracle of tests/test_gpu_sepconv_grad.py is the true derivative, its Mish' is the
closed form of include/qpwc.h, the grad path refuses CPU tensors / capture / fp16 / bf16x3, and the GPU suite's
"more than one trip" shape still loops against the constants of csrc/sepconv_bwd.hip."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys
import types

import pytest
import torch

from oracle import torch_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_sepconv_grad import MULTI_TRIP, TRAIN_DRIFT, composite, train_composite  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")
I, I64, VP = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p


def _constants(name, *keys):
    text = open(os.path.join(CSRC, name)).read()
    out = {}
    for k in keys:
        m = re.findall(r"constexpr\s+int\s+{}\s*=\s*(\d+)\s*[;,]".format(k), text)
        assert len(m) == 1, (name, k, m)
        out[k] = int(m[0])
    return out


SCB = _constants("sepconv_bwd.hip", "kScbPx", "kScbPwBlocks", "kScbStrip", "kScbDwSlots", "kScbDwBlocks")
KC = _constants("optflow_common.h", "kScKC")["kScKC"]


def _workspace(B, H, W, C, F):
    """The layout of scb_plan() in sepconv_bwd.hip."""
    M, cpad = B * H * W, -(-C // KC) * KC
    chunks = cpad // KC
    up4 = lambda n: -(-n // 4) * 4
    pw_x = min(-(-M // SCB["kScbPx"]), max(1, SCB["kScbPwBlocks"] // chunks))
    groups = -(-(B * H * -(-W // SCB["kScbStrip"])) // SCB["kScbDwSlots"])
    dw_x = min(groups, max(1, SCB["kScbDwBlocks"] // chunks))
    return 2 * M * cpad + up4(M * F) + pw_x * F * cpad + up4(pw_x * F) + up4(dw_x * C * 9)


def test_workspace_floats(hip_lib):
    from qpwcnet_amd import _hip
    ws = hip_lib.qpwc_sepconv3x3_bwd_workspace_floats
    assert ws(1, 7, 11, 5, 16) == _workspace(1, 7, 11, 5, 16)
    assert ws(8, 128, 256, 115, 128) == _workspace(8, 128, 256, 115, 128)
    assert ws(1, 7, 11, 5, 16) >= 77 * (2 * 32 + 16)
    assert ws(0, 7, 11, 5, 16) == _hip.E_SHAPE
    assert ws(1, 7, -1, 5, 16) == _hip.E_SHAPE
    assert ws(1, 7, 11, 0, 16) == _hip.E_SHAPE
    assert ws(1, 7, 11, 5, 48) == _hip.E_SHAPE
    assert b"F=48" in hip_lib.qpwc_last_error()


def test_sepconv_bwd_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep = (ctypes.c_float * (1 << 18))()
    base = ctypes.cast(keep, VP).value
    base += (-base) % 16
    # (1,4,4) pixels, sources of 3 and 2 channels (the first in 4-float pixels), F = 16: each buffer 64 KiB apart
    s0, s1, dw, pw, bias, gout, g0, g1, gdw, gpw, gb, ws = (base + 65536 * i for i in range(12))
    assert L.qpwc_sepconv3x3_bwd_workspace_floats(1, 4, 4, 5, 16) * 4 <= 65536

    def call(src=(s0, s1), ch=(3, 2), st=(4, 2), flags=3, dw=dw, pw=pw, bias=bias, gout=gout, gsrc=(g0, g1), gdw=gdw,
             gpw=gpw, gb=gb, ws=ws, B=1, H=4, W=4, F=16, null_src=False, null_gsrc=False):
        n = len(ch)
        return L.qpwc_sepconv3x3_bwd(None if null_src else (VP * n)(*src[:n]), (I * n)(*ch), (I64 * n)(*st), n, flags,
                                     dw, pw, bias, gout, None if null_gsrc else (VP * n)(*gsrc[:n]), gdw, gpw, gb, ws,
                                     B, H, W, F, None)

    def err():
        return L.qpwc_last_error()

    for kw, name in ((dict(null_src=True), b"src"), (dict(src=(s0, None)), b"src[1]"), (dict(dw=None), b"dw"),
                     (dict(pw=None), b"pw"), (dict(bias=None), b"bias"), (dict(gout=None), b"grad_out"),
                     (dict(ws=None), b"workspace")):
        assert call(**kw) == _hip.E_NULL and name in err(), (kw, err())
    assert call(null_gsrc=True, gdw=None, gpw=None, gb=None) == _hip.E_NULL
    assert call(gsrc=(None, None), gdw=None, gpw=None, gb=None) == _hip.E_NULL and b"all null" in err()
    assert call(F=24) == _hip.E_SHAPE and b"F=24" in err()
    assert call(ch=(), st=(), src=(), gsrc=()) == _hip.E_SHAPE and b"n_src" in err()
    assert call(ch=(3, 0)) == _hip.E_SHAPE and b"src[1]" in err()
    assert call(st=(2, 2)) == _hip.E_SHAPE and b"src[0]" in err()       # pixel stride below the channel count
    assert call(H=0) == _hip.E_SHAPE
    assert call(flags=4) == _hip.E_SHAPE and b"mish_flags" in err()
    assert call(src=(s0 + 2, s1)) == _hip.E_ALIGN and b"src[0]" in err()
    assert call(pw=pw + 4) == _hip.E_ALIGN and b"pw" in err()           # 16-byte: read as float4
    assert call(gout=gout + 8) == _hip.E_ALIGN and b"grad_out" in err()
    assert call(gpw=gpw + 4) == _hip.E_ALIGN and b"grad_pw" in err()
    assert call(ws=ws + 4) == _hip.E_ALIGN and b"workspace" in err()
    assert call(gb=gb + 2) == _hip.E_ALIGN and b"grad_bias" in err()
    assert call(gsrc=(s0, g1)) == _hip.E_ALIAS and b"grad_src[0]" in err() and b"src[0]" in err()
    assert call(gsrc=(g0, g0 + 16)) == _hip.E_ALIAS                        # two gradients overlap
    assert call(gdw=dw) == _hip.E_ALIAS and b"grad_dw" in err()
    assert call(gpw=pw) == _hip.E_ALIAS
    assert call(gb=gout + 16) == _hip.E_ALIAS and b"grad_out" in err()
    assert call(ws=g1) == _hip.E_ALIAS and b"workspace" in err()
    assert call(ws=gout - 64) == _hip.E_ALIAS                               # the workspace runs into grad_out
    assert call(gdw=gpw + 16) == _hip.E_ALIAS and b"grad_pw" in err()


def _leaves(gen, chans, F):
    C = sum(chans)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_()
    return [r(1, 4, 5, c) for c in chans], r(C, 1, 3, 3), r(F, C), r(F)


@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["00", "10", "01", "11"])
def test_gradcheck_composite_oracle(flags):
    gen = torch.Generator().manual_seed(0)
    srcs, dw, pw, bias = _leaves(gen, (3,), 4)
    assert torch.autograd.gradcheck(lambda x, a, b, c: composite((x,), a, b, c, *flags), (srcs[0], dw, pw, bias),
                                    eps=1e-7, atol=1e-6)


def test_gradcheck_composite_oracle_three_sources():
    gen = torch.Generator().manual_seed(1)
    srcs, dw, pw, bias = _leaves(gen, (3, 2, 1), 4)
    assert torch.autograd.gradcheck(lambda x, y, z, a, b, c: composite((x, y, z), a, b, c, True, True),
                                    tuple(srcs) + (dw, pw, bias), eps=1e-7, atol=1e-6)


def test_oracle_mish_derivative_is_the_closed_form():
    t = torch.tensor([-100.0, -40.0, -1.19, 0.0, 1.0, 40.0, 100.0], dtype=torch.float64, requires_grad=True)
    torch_ref.mish(t).sum().backward()
    for v, got in zip(t.detach().tolist(), t.grad.tolist()):
        sp = math.log1p(math.exp(v)) if v < 30 else v
        th = math.tanh(sp)
        want = th + v * (1.0 - th * th) / (1.0 + math.exp(-v))
        assert math.isfinite(got) and abs(got - want) <= 1e-12 * max(1.0, abs(want)), (v, got, want)
    assert t.grad[0] == pytest.approx(0.0, abs=1e-40) and t.grad[-1] == pytest.approx(1.0, abs=1e-12)


def _operands(dtype=torch.float32, pw_dtype=torch.float32):
    x = torch.zeros(1, 4, 4, 5, dtype=dtype, requires_grad=True)
    return [x], torch.zeros(5, 1, 3, 3), torch.zeros(16, 32, dtype=pw_dtype), torch.zeros(16)


def test_the_grad_path_needs_a_hip_device():
    from qpwcnet_amd import layers, ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sepconv3x3(*_operands())
    lay = layers.SeparableConv2D(5, 16, data_format="channels_last")
    with pytest.raises(RuntimeError, match="HIP device"):
        lay(torch.zeros(1, 4, 4, 5))


def test_the_grad_path_refuses_fp16_and_bf16x3():
    from qpwcnet_amd import ops
    with pytest.raises(ValueError, match="fp16"):
        ops.sepconv3x3(*_operands(torch.float16, torch.float16))
    srcs, dw, pw3, bias = _operands(pw_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bf16x3"):
        ops.sepconv3x3(srcs, dw, pw3.reshape(1, 16, 32).expand(3, 16, 32), bias)


def test_the_grad_path_refuses_graph_capture(monkeypatch):
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.sepconv3x3(*_operands())
    ctx = types.SimpleNamespace(saved_tensors=(), cfg=None, needs_input_grad=(False,) * 5 + (True,))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._SepConvFn.backward(ctx, torch.zeros(1, 4, 4, 16))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops._SepConvFn.forward(ctx, False, True, *_operands()[1:], *_operands()[0])


def test_layer_constructor_on_the_host():
    from qpwcnet_amd import layers
    lay = layers.SeparableConv2D(19, 32, activation=None, name="head")
    assert lay.get_config() == {"name": "head", "in_channels": 19, "filters": 32, "activation": None}
    assert sorted(layers.SeparableConv2D.from_config(lay.get_config()).state_dict()) == \
        ["bias", "depthwise.weight", "pointwise.weight"]
    assert tuple(lay.depthwise.weight.shape) == (19, 1, 3, 3) and tuple(lay.pointwise.weight.shape) == (32, 19, 1, 1)
    for bad in (dict(kernel_size=5), dict(strides=2), dict(padding="valid"), dict(use_bias=False),
                dict(depth_multiplier=2), dict(activation="relu"), dict(filters=24)):
        with pytest.raises(ValueError):
            layers.SeparableConv2D(**dict(dict(in_channels=19, filters=32), **bad))


def test_training_case_drift_is_what_the_gpu_bound_was_derived_from():
    """The fp32 CPU composite against the float64 one over the 5 SGD steps of test_short_training_run: the drift the
    GPU test's bound (10 x) was set from; the float64 loss falls at every step.  The figure is about one fp32 ulp of
    the parameters and moves a little with the host's BLAS and thread count, hence the factor 2 either way."""
    ref, losses = train_composite(torch.float64)
    got, _ = train_composite(torch.float32)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    drift = max(float((a.double() - b).abs().max()) for a, b in zip(got, ref))
    assert TRAIN_DRIFT / 2 <= drift <= 2 * TRAIN_DRIFT, drift


def test_multi_trip_case_loops_past_every_cap():
    B, H, W, C, F = MULTI_TRIP
    M, chunks = B * H * W, -(-C // KC)
    # sepconv_bwd_pw_kernel: pixel blocks in grid-stride order over min(blocks, kScbPwBlocks / chunks) workgroups
    blocks, cap = -(-M // SCB["kScbPx"]), max(1, SCB["kScbPwBlocks"] // chunks)
    assert blocks > cap and blocks % cap, (blocks, cap)
    assert M % SCB["kScbPx"], "no partial last pixel block"
    # sepconv_bwd_dw_kernel: groups of kScbDwSlots strips over min(groups, kScbDwBlocks / chunks) workgroups
    strips = B * H * -(-W // SCB["kScbStrip"])
    groups, cap = -(-strips // SCB["kScbDwSlots"]), max(1, SCB["kScbDwBlocks"] // chunks)
    assert groups > cap and groups % cap, (groups, cap)
    assert W % SCB["kScbStrip"] and strips % SCB["kScbDwSlots"], "no partial last strip / strip group"
    # stage D walks one partial per workgroup of the stages above
    assert min(SCB["kScbPwBlocks"], SCB["kScbDwBlocks"]) // chunks >= 2


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernels_use_no_scratch(tmp_path):
    """Every kernel of sepconv_bwd.hip compiles for gfx950 without scratch memory and the matrix products are on the
    fp32 matrix instruction."""
    s = tmp_path / "sepconv_bwd.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "sepconv_bwd.hip"), "-o", str(s)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, check=True)
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    assert len(names) == len(scratch) >= 15 and all("sepconv_bwd" in n for n in names), names
    assert not any(scratch), dict(zip(names, scratch))
    text = s.read_text()
    assert "v_mfma_f32_16x16x4_f32" in text

"""CPU suite of the backward passes: the new C-ABI entry points refuse bad arguments before any HIP call, the
gradient oracle (torch autograd of oracle.torch_ref) is the true derivative, the tie rules the kernels follow hold
for that oracle, and the scatter of grad_img compiles to no-return float atomics (no compare-and-swap loop)."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

from oracle import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qpwcnet_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _aligned_buffers(n_floats=1 << 16):
    buf = (ctypes.c_float * n_floats)()
    base = ctypes.cast(buf, ctypes.c_void_p).value
    base += (-base) % 16
    return buf, base


def test_cost_volume_bwd_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, base = _aligned_buffers()
    # (1,2,2,4) operands, r = 1: 9-channel volume; each buffer 4 KiB apart
    prv, nxt, out, gout, gp, gn = (base + 4096 * i for i in range(6))

    def call(prv=prv, nxt=nxt, out=out, gout=gout, gp=gp, gn=gn, B=1, H=2, W=2, C=4, r=1, dtype=0):
        return L.qpwc_cost_volume_bwd(prv, nxt, out, gout, gp, gn, B, H, W, C, r, dtype, 0.1, None)

    assert call(prv=None) == _hip.E_NULL
    assert call(gout=None) == _hip.E_NULL
    assert call(gp=None, gn=None) == _hip.E_NULL
    assert call(dtype=9) == _hip.E_DTYPE
    assert call(H=0) == _hip.E_SHAPE
    assert call(C=-1) == _hip.E_SHAPE
    assert call(r=-1) == _hip.E_RANGE
    assert call(r=17) == _hip.E_RANGE
    assert call(gp=prv) == _hip.E_ALIAS
    assert call(gn=out + 8) == _hip.E_ALIAS                   # overlaps the saved output
    assert call(gp=gout) == _hip.E_ALIAS
    assert call(gn=gp + 16) == _hip.E_ALIAS                   # the two gradients overlap
    assert call(gp=gp + 2) == _hip.E_ALIGN
    assert call(dtype=1, gout=gout + 1) == _hip.E_ALIGN
    assert b"search_range" in (call(r=20) and L.qpwc_last_error())
    # the mask is read from the saved output as out > 0: only the sign of the pre-activation for slope >= 0
    assert L.qpwc_cost_volume_bwd(prv, nxt, out, gout, gp, gn, 1, 2, 2, 4, 1, 0, -0.1, None) == _hip.E_RANGE
    assert b"slope" in L.qpwc_last_error()
    assert L.qpwc_cost_volume_bwd(prv, nxt, out, gout, gp, gn, 1, 2, 2, 4, 1, 0, float("nan"), None) == _hip.E_RANGE


def test_warp_bwd_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, base = _aligned_buffers()
    img, flo, gout, gi, gf, ws = (base + 4096 * i for i in range(6))

    def call(img=img, flo=flo, gout=gout, gi=gi, gf=gf, ws=ws, B=1, H=2, W=2, C=4, dtype=0, mode=0):
        return L.qpwc_warp_bwd(img, flo, gout, gi, gf, ws, B, H, W, C, dtype, mode, None)

    assert call(img=None) == _hip.E_NULL
    assert call(flo=None) == _hip.E_NULL
    assert call(gi=None, gf=None) == _hip.E_NULL
    assert call(dtype=1, ws=None) == _hip.E_NULL              # fp16 grad_img needs the fp32 workspace
    assert call(dtype=7) == _hip.E_DTYPE
    assert call(mode=3) == _hip.E_MODE
    assert call(W=0) == _hip.E_SHAPE
    assert call(H=1, mode=_hip.WARP_CLAMP) == _hip.E_SHAPE     # the reference refuses the grid (warp.py:182-184)
    assert b"at least 2x2" in L.qpwc_last_error()
    assert call(W=1, mode=_hip.WARP_CLAMP) == _hip.E_SHAPE
    assert call(gi=img) == _hip.E_ALIAS
    assert call(gf=gout + 4) == _hip.E_ALIAS
    assert call(gf=gi + 16) == _hip.E_ALIAS                   # the two gradients overlap
    assert call(dtype=1, ws=gi) == _hip.E_ALIAS               # workspace overlaps grad_img
    assert call(gf=gf + 2) == _hip.E_ALIGN
    assert call(dtype=1, gi=gi + 1) == _hip.E_ALIGN
    assert L.qpwc_warp_bwd_workspace_floats(2, 3, 5, 7, 0) == 0
    assert L.qpwc_warp_bwd_workspace_floats(2, 3, 5, 7, 1) == 2 * 3 * 5 * 7
    assert L.qpwc_warp_bwd_workspace_floats(2, 3, 5, 7, 4) == _hip.E_DTYPE
    assert L.qpwc_warp_bwd_workspace_floats(2, 0, 5, 7, 1) == _hip.E_SHAPE


def test_the_layers_need_a_hip_device_with_grad_too():
    """With an input that requires grad the layers still run on the HIP kernels only: a CPU tensor is refused."""
    from qpwcnet_amd import ops
    x = torch.zeros(1, 4, 4, 2, requires_grad=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.cost_volume(x, x.detach(), 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.warp(x, torch.zeros(1, 4, 4, 2), "clamp")


def test_negative_slope_is_refused_on_the_grad_path():
    from qpwcnet_amd import ops
    x = torch.zeros(1, 4, 4, 2, requires_grad=True)
    with pytest.raises(ValueError, match="lrelu_slope >= 0"):
        ops.cost_volume(x, x.detach(), 1, lrelu_slope=-0.1)


def test_the_grad_path_refuses_graph_capture(monkeypatch):
    """Forward and backward of the differentiable path raise a clear error under stream capture instead of being
    recorded (a captured forward + backward is not supported yet)."""
    from qpwcnet_amd import ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    x = torch.zeros(1, 4, 4, 2, requires_grad=True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.cost_volume(x, x.detach(), 1)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        ops.warp(x, torch.zeros(1, 4, 4, 2), "clamp")
    ctx = types.SimpleNamespace(saved_tensors=(), cfg=None, needs_input_grad=(True, True))
    for fn in (ops._CostVolumeFn, ops._WarpFn):
        with pytest.raises(RuntimeError, match="cannot be captured"):
            fn.backward(ctx, torch.zeros(1, 4, 4, 2))


def _grid(gen, shape, step):
    """Values on a grid of `step` in [-1, 1] (exact in fp32)."""
    return torch.randint(-int(1 / step), int(1 / step) + 1, shape, generator=gen).to(torch.float64) * step


def test_gradcheck_cost_volume_oracle():
    gen = torch.Generator().manual_seed(0)
    prv = (_grid(gen, (1, 4, 5, 3), 1 / 16) + 1 / 64).requires_grad_()    # + 1/64: no product sum sits at 0
    nxt = (_grid(gen, (1, 4, 5, 3), 1 / 16) + 1 / 128).requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: torch_ref.cost_volume(a, b, 1), (prv, nxt), eps=1e-7, atol=1e-6)


def test_gradcheck_warp_oracles_away_from_kinks():
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(2, 4, 5, 3, generator=gen, dtype=torch.float64).requires_grad_()
    # sample points strictly between pixels and inside the image: no floor / clamp / truncation kink within eps
    y, x = torch.meshgrid(torch.arange(4.0), torch.arange(5.0), indexing="ij")
    frac = lambda: 0.1 + 0.8 * torch.rand(2, 4, 5, generator=gen, dtype=torch.float64)
    ty = torch.randint(0, 4, (2, 4, 5), generator=gen) + frac()
    tx = torch.randint(0, 5, (2, 4, 5), generator=gen) + frac()
    flo = torch.stack([tx - x, ty - y], dim=-1).requires_grad_()
    assert torch.autograd.gradcheck(torch_ref.warp_v2, (img, flo), eps=1e-7, atol=1e-6)
    assert torch.autograd.gradcheck(torch_ref.tf_warp, (img, flo), eps=1e-7, atol=1e-6)


def test_lrelu_tie_takes_the_slope():
    """A cost-volume entry of exactly 0 back-propagates slope * grad (TF's and torch's leaky_relu gradient): the
    kernels read the mask from the saved output as out > 0."""
    prv = torch.tensor([[[[1.0, -1.0]]]], dtype=torch.float64, requires_grad=True)   # (1,1,1,2)
    nxt = torch.tensor([[[[1.0, 1.0]]]], dtype=torch.float64, requires_grad=True)
    out = torch_ref.cost_volume(prv, nxt, 0)
    assert float(out.detach()) == 0.0
    out.sum().backward()
    assert torch.allclose(prv.grad, 0.1 * 0.5 * nxt.detach())


def _flow_grad_x(fn, img, fx):
    flo = torch.zeros(img.shape[:3] + (2,), dtype=torch.float64)
    flo[..., 0] = fx
    flo.requires_grad_()
    fn(img, flo).sum().backward()
    return flo.grad[..., 0]


def test_warp_flow_gradient_tie_rules():
    gen = torch.Generator().manual_seed(2)
    img = torch.randn(1, 3, 6, 1, generator=gen, dtype=torch.float64)
    v = img[0, :, :, 0]
    fwd = torch.zeros_like(v)
    fwd[:, :-1] = v[:, 1:] - v[:, :-1]
    # zero flow, WarpV2: the forward difference; at the last column (q = W-1, alpha = 1 on the closed interval)
    # the backward difference
    g = _flow_grad_x(torch_ref.warp_v2, img, 0.0)[0]
    assert torch.allclose(g[:, :-1], fwd[:, :-1])
    assert torch.allclose(g[:, -1], v[:, -1] - v[:, -2])
    # zero flow, tf_warp: the forward difference, zero at the last column (both corners clipped to W-1) and on the
    # last row (y1 clipped to y0 = H-1: every raw weight is 0 there)
    g = _flow_grad_x(torch_ref.tf_warp, img, 0.0)[0]
    assert torch.allclose(g[:-1], fwd[:-1])
    assert torch.all(g[-1] == 0)
    # samples beyond the image: no flow gradient under the clamp rules
    assert torch.all(_flow_grad_x(torch_ref.warp_v2, img, 7.5) == 0)
    assert torch.all(_flow_grad_x(torch_ref.warp_v2, img, -6.25) == 0)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_grad_img_scatter_is_no_return_float_atomics(tmp_path):
    s = tmp_path / "backward.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "backward.hip"), "-o", str(s)],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = s.read_text()
    assert text.count("cmpswap") == 0
    adds = [ln.strip() for ln in text.splitlines() if "global_atomic_add_f32" in ln]
    # no-return form: `global_atomic_add_f32 v[a:b], vdata, off[ offset:n]` -- a 64-bit address pair, one data
    # register, no saddr, no sc0 (the returning variant has a destination register first and sets sc0)
    no_return = re.compile(r"^global_atomic_add_f32\s+v\[\d+:\d+\],\s*v\d+,\s*off(\s+offset:-?\d+)?$")
    assert adds and all(no_return.match(ln) for ln in adds), [ln for ln in adds if not no_return.match(ln)][:4]

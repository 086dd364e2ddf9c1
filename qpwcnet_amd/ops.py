"""Functional entry points of the hot path: torch tensors in, HIP kernels underneath.

Each function validates shapes/dtypes/devices the way the reference's graph
construction would, then calls the C ABI (``include/qpwc.h``) on the caller's
current HIP stream.  There is no CPU path: a non-GPU tensor is an error.
"""
import ctypes

import torch

from . import _hip
from .backend import CHANNELS_FIRST, CHANNELS_LAST, get_axis

_DTYPES = {torch.float32: _hip.F32, torch.float16: _hip.F16}


class KernelTimer:
    """HIP-event timing of the hot-path launches, on the stream they are launched
    on (the caller's current stream).  Used by bench.py for the live roofline:

        with ops.kernel_timing() as kt:
            model(x)
        kt.summary()  # {(op, B, H, W, C): (launches, mean_ms)}
    """

    def __init__(self):
        self.records = []

    def __enter__(self):
        global _TIMER
        self._prev, _TIMER = _TIMER, self
        return self

    def __exit__(self, *exc):
        global _TIMER
        _TIMER = self._prev
        return False

    def summary(self):
        torch.cuda.synchronize()
        acc = {}
        for key, e0, e1 in self.records:
            n, t = acc.get(key, (0, 0.0))
            acc[key] = (n + 1, t + e0.elapsed_time(e1))
        return {k: (n, t / n) for k, (n, t) in acc.items()}


_TIMER = None


def kernel_timing():
    return KernelTimer()


class _timed:
    __slots__ = ("key", "e0")

    def __init__(self, op, dims):
        self.key = (op,) + tuple(dims)

    def __enter__(self):
        if _TIMER is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _TIMER is not None and exc[0] is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _TIMER.records.append((self.key, self.e0, e1))
        return False


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def cost_volume_kernel(B, H, W, C, dtype=torch.float32, fused=False, search_range=4, layout=None,
                       out_pixel_stride=0):
    """Name of the kernel ``qpwc_cost_volume_fwd`` (``fused=False``) / ``qpwc_warp_cost_volume_fwd`` (``fused=True``)
    launches for this shape: the C side's own selection rules, run without launching (``qpwc_cost_volume_kernel``;
    host only).  '' for arguments the entry point refuses."""
    dt = {"f32": _hip.F32, "f16": _hip.F16}.get(dtype) if isinstance(dtype, str) else _DTYPES.get(dtype)
    if dt is None:
        return ""
    name = _hip.lib().qpwc_cost_volume_kernel(int(B), int(H), int(W), int(C), int(search_range),
                                              _hip.NHWC if layout is None else layout, dt, int(out_pixel_stride),
                                              1 if fused else 0)
    return name.decode() if name else ""


def _check_tensor(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError("{} must be a torch.Tensor".format(name))
    if not t.is_cuda:
        raise RuntimeError(
            "qpwcnet_amd: {} is on '{}'; the hot path runs on a HIP device only "
            "(no CPU fallback)".format(name, t.device))
    if t.dtype not in _DTYPES:
        raise ValueError("{}: unsupported dtype {}".format(name, t.dtype))
    if t.dim() != 4:
        # the reference's tf_warp breaks on unbatched input too (warp.py:75-79)
        raise ValueError("{} must be rank 4 (batched), got shape {}".format(name, tuple(t.shape)))


def _physical(t, data_format):
    """-> (dense tensor, layout code, (B,H,W,C), nhwc_view_of_nchw).

    A ``channels_first`` tensor stored in torch's channels_last memory format is
    physically NHWC: hand it to the NHWC kernels through a permuted view."""
    get_axis(data_format)  # raises ValueError('Unsupported data format')
    if data_format == CHANNELS_LAST:
        t = t.contiguous()
        B, H, W, C = t.shape
        return t, _hip.NHWC, (B, H, W, C), False
    B, C, H, W = t.shape
    if C > 1 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous():
        return t.permute(0, 2, 3, 1), _hip.NHWC, (B, H, W, C), True
    return t.contiguous(), _hip.NCHW, (B, H, W, C), False


def _empty_like_layout(ref, dims, channels, layout, as_nchw_view):
    B, H, W, _ = dims
    if layout == _hip.NHWC:
        buf = torch.empty((B, H, W, channels), dtype=ref.dtype, device=ref.device)
        return buf, (buf.permute(0, 3, 1, 2) if as_nchw_view else buf)
    buf = torch.empty((B, channels, H, W), dtype=ref.dtype, device=ref.device)
    return buf, buf


def layout_transpose(x, to_format):
    """Dense (B,C,H,W) -> dense (B,H,W,C) for to_format 'channels_last', the reverse for
    'channels_first' (qpwc_layout_transpose_fwd): how a 'channels_first' tensor crosses the boundary
    of the channels-last kernels (the reference transposes in and out the same way, layers.py:179-183)."""
    _check_tensor("x", x)
    get_axis(to_format)
    x = x.contiguous()
    if to_format == CHANNELS_LAST:
        B, C, H, W = x.shape
        out = torch.empty((B, H, W, C), dtype=x.dtype, device=x.device)
        code = _hip.NHWC
    else:
        B, H, W, C = x.shape
        out = torch.empty((B, C, H, W), dtype=x.dtype, device=x.device)
        code = _hip.NCHW
    with torch.cuda.device(x.device), _timed("layout_transpose", (B, H, W, C)):
        rc = _hip.lib().qpwc_layout_transpose_fwd(x.data_ptr(), out.data_ptr(), B, H, W, C, code,
                                                   _DTYPES[x.dtype], _stream(x))
    _hip.check(rc)
    return out


def copy_pixels_ok(src, dst):
    """Whether copy_pixels() can take this pair of (B,H,W,C) views: same shape and dtype, channels contiguous, whole
    16-byte units everywhere (qpwc_copy_pixels_fwd's contract)."""
    if src.dim() != 4 or src.shape != dst.shape or src.dtype != dst.dtype or src.dtype not in _DTYPES or \
            not (src.is_cuda and dst.is_cuda) or src.stride(3) != 1 or dst.stride(3) != 1:
        return False
    es = src.element_size()
    if (src.shape[3] * es) % 16 or src.data_ptr() % 16 or dst.data_ptr() % 16:
        return False
    return all((t.stride(i) * es) % 16 == 0 and t.stride(i) >= 0 for t in (src, dst) for i in range(3))


def copy_pixels(src, dst):
    """dst[...] = src for two channels-last (B,H,W,C) views with their own batch / row / pixel strides
    (qpwc_copy_pixels_fwd): the skip half of the decoder's concat([UpConv(x), skip]) (pwcnet.py:186-195)."""
    _check_tensor("src", src)
    _check_tensor("dst", dst)
    if not copy_pixels_ok(src, dst):
        raise ValueError("copy_pixels needs two (B,H,W,C) views of one shape and dtype with contiguous channels in "
                         "whole 16-byte units")
    B, H, W, C = src.shape
    ss = (ctypes.c_int64 * 3)(src.stride(0), src.stride(1), src.stride(2))
    ds = (ctypes.c_int64 * 3)(dst.stride(0), dst.stride(1), dst.stride(2))
    with torch.cuda.device(src.device), _timed("copy_pixels", (B, H, W, C)):
        rc = _hip.lib().qpwc_copy_pixels_fwd(src.data_ptr(), dst.data_ptr(), B, H, W, C, ss, ds, _DTYPES[src.dtype],
                                             _stream(src))
    _hip.check(rc)
    return dst


def _nchw_fast_path(C, search_range=4):
    """Dense NCHW operands of the hot-path layers go through a transposition to the channels-last
    kernels when those have a vector path for the shape (else: the generic any-layout kernels)."""
    return C % 4 == 0 and search_range == 4


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _refuse_capture(what):
    """The differentiable path is not capturable yet: a torch.cuda.graph holding this forward and its backward
    crashed in the graph instantiation on MI355X / ROCm, with the cause not isolated.  Refuse with
    a clear error, before anything of ours is enqueued, instead of taking the process down.  The no-grad path (the
    network's inference graphs) is not affected."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(
            "qpwcnet_amd: {} with autograd cannot be captured in a torch.cuda graph yet; capture the no-grad "
            "forward (torch.no_grad()) or run the training step eagerly".format(what))


def _grad_operands_check(x, weight, bias, what):
    """What the differentiable convolutions ask of their operands: a dense rank-4 channels-last x; x, weight and bias
    fp32 on a HIP device."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("{}: x must be a rank-4 (B,H,W,C) tensor".format(what))
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if not t.is_cuda:
            raise ValueError("{}: {} is on '{}'; the kernels run on a HIP device only (no CPU fallback)".format(
                what, name, t.device))
        if t.dtype == torch.float16:
            raise ValueError("{}: no fp16 storage path, {} is fp16: train in fp32".format(what, name))
        if t.dtype != torch.float32:
            raise ValueError("{}: {} must be fp32, got {}".format(what, name, t.dtype))
    if not x.is_contiguous():
        raise ValueError("{}: x must be a dense channels-last tensor".format(what))


def _bwd_buffers(nws, shapes, need, dev):
    """The buffers of a backward launch: the fp32 workspace of nws floats (a negative nws is the library's error code)
    and one fp32 output per shape that is asked for -> (workspace, outputs with None for the rest, their pointers with
    None = NULL for the rest)."""
    _hip.check(min(int(nws), 0))
    new = lambda shape: torch.empty(shape, dtype=torch.float32, device=dev)
    outs = [new(tuple(sh)) if n else None for sh, n in zip(shapes, need)]
    return new(int(nws)), outs, [t.data_ptr() if t is not None else None for t in outs]


def _to_nhwc(t, data_format):
    """Dense (B,H,W,C) form of a layer operand or gradient for the channels-last backward kernels: a channels_first
    tensor that is physically NHWC (torch channels_last memory) through its permuted view, else transposed."""
    if data_format == CHANNELS_LAST:
        return t.contiguous()
    v = t.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else layout_transpose(t, CHANNELS_LAST)


def _from_nhwc(t, data_format):
    return t if data_format == CHANNELS_LAST else t.permute(0, 3, 1, 2)


class _CostVolumeFn(torch.autograd.Function):
    """cost_volume() with qpwc_cost_volume_bwd as its gradient: the forward is the no-grad forward itself."""

    @staticmethod
    def forward(ctx, prv, nxt, search_range, data_format, lrelu_slope):
        out = cost_volume(prv, nxt, search_range, data_format, lrelu_slope)
        ctx.save_for_backward(prv, nxt, out)
        ctx.cfg = (int(search_range), data_format, float(lrelu_slope))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the cost-volume backward")
        prv, nxt, out = ctx.saved_tensors
        r, fmt, slope = ctx.cfg
        need_p, need_n = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gp, gn = cost_volume_bwd(_to_nhwc(prv, fmt), _to_nhwc(nxt, fmt), _to_nhwc(out, fmt),
                                 _to_nhwc(grad_out.to(out.dtype), fmt), r, slope, need_p, need_n)
        return (_from_nhwc(gp, fmt) if need_p else None, _from_nhwc(gn, fmt) if need_n else None, None, None, None)


def cost_volume_bwd(prv, nxt, out, grad_out, search_range=4, lrelu_slope=0.1, need_prv=True, need_nxt=True):
    """(grad_prv, grad_nxt) of cost_volume() for dense NHWC operands (qpwc_cost_volume_bwd); out = the saved forward
    output.  A gradient that is not asked for comes back as None."""
    for name, t in (("prv", prv), ("nxt", nxt), ("out", out), ("grad_out", grad_out)):
        _check_tensor(name, t)
        if t.dtype != prv.dtype or not t.is_contiguous():
            raise ValueError("cost_volume_bwd takes dense NHWC tensors of one dtype")
    B, H, W, C = prv.shape
    d = 2 * int(search_range) + 1
    if nxt.shape != prv.shape or tuple(out.shape) != (B, H, W, d * d) or out.shape != grad_out.shape:
        raise ValueError("cost_volume_bwd: shapes {} {} {} {}".format(
            tuple(prv.shape), tuple(nxt.shape), tuple(out.shape), tuple(grad_out.shape)))
    gp = torch.empty_like(prv) if need_prv else None
    gn = torch.empty_like(nxt) if need_nxt else None
    with torch.cuda.device(prv.device), _timed("cost_volume_bwd", (B, H, W, C)):
        rc = _hip.lib().qpwc_cost_volume_bwd(
            prv.data_ptr(), nxt.data_ptr(), out.data_ptr(), grad_out.data_ptr(),
            gp.data_ptr() if need_prv else None, gn.data_ptr() if need_nxt else None, B, H, W, C, int(search_range),
            _DTYPES[prv.dtype], float(lrelu_slope), _stream(prv))
    _hip.check(rc)
    return gp, gn


def cost_volume(prv, nxt, search_range=4, data_format=CHANNELS_LAST, lrelu_slope=0.1):
    """CostVolume / CostVolumeV2 forward (reference: qpwcnet/core/layers.py:72-100,128-132).
    Differentiable in prv and nxt: with grad enabled and an input requiring grad the same forward runs inside an
    autograd Function whose backward is qpwc_cost_volume_bwd (lrelu_slope >= 0 there: the backward reads the
    LeakyReLU mask from the saved output as out > 0)."""
    if _wants_grad(prv, nxt):
        if not float(lrelu_slope) >= 0.0:
            raise ValueError("the cost-volume gradient needs lrelu_slope >= 0 (got {})".format(lrelu_slope))
        _refuse_capture("the cost volume")
        return _CostVolumeFn.apply(prv, nxt, search_range, data_format, lrelu_slope)
    _check_tensor("prv", prv)
    _check_tensor("nxt", nxt)
    if prv.shape != nxt.shape:
        raise ValueError("prv and nxt must have the same shape, got {} and {}".format(
            tuple(prv.shape), tuple(nxt.shape)))
    if prv.dtype != nxt.dtype or prv.device != nxt.device:
        raise ValueError("prv and nxt must share dtype and device")
    p, layout, dims, as_view = _physical(prv, data_format)
    n, layout_n, _, _ = _physical(nxt, data_format)
    if layout_n != layout:  # mixed memory formats: fall back to the declared layout
        p, n = prv.contiguous(), nxt.contiguous()
        layout, as_view = (_hip.NCHW if data_format == CHANNELS_FIRST else _hip.NHWC), False
    B, H, W, C = dims
    d = 2 * int(search_range) + 1
    if layout == _hip.NCHW and _nchw_fast_path(C, int(search_range)):
        # dense (B,C,H,W): transpose in, matrix-core / LDS-tiled channels-last kernel, transpose out
        out_l = cost_volume(layout_transpose(p, CHANNELS_LAST), layout_transpose(n, CHANNELS_LAST), search_range,
                            CHANNELS_LAST, lrelu_slope)
        return layout_transpose(out_l, CHANNELS_FIRST)
    buf, out = _empty_like_layout(p, dims, d * d, layout, as_view)
    with torch.cuda.device(p.device), _timed("cost_volume", dims):
        rc = _hip.lib().qpwc_cost_volume_fwd(
            p.data_ptr(), n.data_ptr(), buf.data_ptr(), B, H, W, C, int(search_range), layout,
            _DTYPES[p.dtype], float(lrelu_slope), _stream(p))
    _hip.check(rc)
    return out


def cost_volume_to_flow(cvol, data_format=CHANNELS_LAST):
    """Displacement of the strongest correlation per pixel, (di, dj) = (row, column)
    (qpwcnet/core/vis.py:9-34): fp32 (..., H, W, 2) / (..., 2, H, W).  Rank 4 or unbatched rank 3 (the
    reference's channels_first branch only parses rank 3, vis.py:19-20; both ranks work here for both
    layouts).  A channels-last view with a wider pixel stride (the 84-channel padded volume's [..., :81])
    is read in place."""
    if not isinstance(cvol, torch.Tensor) or cvol.dim() not in (3, 4):
        raise ValueError("cvol must be a rank 3 or 4 tensor, got {}".format(
            tuple(cvol.shape) if isinstance(cvol, torch.Tensor) else type(cvol)))
    x = cvol if cvol.dim() == 4 else cvol.unsqueeze(0)
    _check_tensor("cvol", x)
    if data_format == CHANNELS_LAST:
        B, H, W, D = x.shape
        if x.stride(3) != 1 or x.stride(1) != W * x.stride(2) or x.stride(0) != H * x.stride(1) or x.stride(2) < D:
            x = x.contiguous()
        layout, stride = _hip.NHWC, x.stride(2)
        out = torch.empty((B, H, W, 2), dtype=torch.float32, device=x.device)
    elif data_format == CHANNELS_FIRST:
        B, D, H, W = x.shape
        x = x.contiguous()
        layout, stride = _hip.NCHW, D
        out = torch.empty((B, 2, H, W), dtype=torch.float32, device=x.device)
    else:
        raise ValueError("Unsupported data format : {}".format(data_format))
    with torch.cuda.device(x.device), _timed("cost_volume_to_flow", (B, H, W, D)):
        rc = _hip.lib().qpwc_cost_volume_to_flow_fwd(x.data_ptr(), out.data_ptr(), B, H, W, D, stride, layout,
                                                      _DTYPES[x.dtype], _stream(x))
    _hip.check(rc)
    return out if cvol.dim() == 4 else out[0]


def _flow_physical(flo, dims, data_format, layout, flo32=None):
    """fp32 flow (flo32 where warp() was given it, else cast), dense over its non-broadcast dims, in the image's layout."""
    B, H, W, _ = dims
    if flo.dim() != 4:
        raise ValueError("flo must be rank 4, got shape {}".format(tuple(flo.shape)))
    if data_format == CHANNELS_LAST:
        fb, fh, fw, fc = flo.shape
    else:
        fb, fc, fh, fw = flo.shape
    if fc != 2:
        raise ValueError("flo must have 2 channels (x, y), got {}".format(fc))
    mask = 0
    for ext, full, bit in ((fb, B, _hip.BCAST_B), (fh, H, _hip.BCAST_H), (fw, W, _hip.BCAST_W)):
        if ext == full:
            continue
        if ext != 1:
            raise ValueError("flo shape {} is not broadcastable to the image".format(
                tuple(flo.shape)))
        mask |= bit
    f = flo.to(torch.float32) if flo32 is None else flo32
    if data_format == CHANNELS_FIRST and layout == _hip.NHWC:
        f = f.permute(0, 2, 3, 1)  # image is physically NHWC: give the flow the same layout
    return f.contiguous(), mask


class _WarpFn(torch.autograd.Function):
    """warp() with qpwc_warp_bwd as its gradient.  flo arrives fp32 and expanded to the image's (B,H,W) by torch ops
    outside (autograd reduces and casts the flow gradient back); the forward is the no-grad forward itself."""

    @staticmethod
    def forward(ctx, img, flo, mode, data_format):
        out = warp(img, flo, mode, data_format)
        ctx.save_for_backward(img, flo)
        ctx.cfg = (mode, data_format)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the warp backward")
        img, flo = ctx.saved_tensors
        mode, fmt = ctx.cfg
        need_i, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gi, gf = warp_bwd(_to_nhwc(img, fmt), _to_nhwc(flo, fmt), _to_nhwc(grad_out.to(img.dtype), fmt), mode,
                          need_i, need_f)
        return (_from_nhwc(gi, fmt) if need_i else None, _from_nhwc(gf, fmt) if need_f else None, None, None)


def warp_bwd(img, flo, grad_out, mode="clamp", need_img=True, need_flo=True):
    """(grad_img, grad_flo) of warp() for a dense NHWC image / grad_out and a dense fp32 (B,H,W,2) flow
    (qpwc_warp_bwd); grad_flo is fp32.  A gradient that is not asked for comes back as None."""
    _check_tensor("img", img)
    _check_tensor("grad_out", grad_out)
    if grad_out.dtype != img.dtype or grad_out.shape != img.shape or not (img.is_contiguous() and grad_out.is_contiguous()):
        raise ValueError("warp_bwd takes a dense NHWC image and grad_out of one shape and dtype")
    B, H, W, C = img.shape
    if tuple(flo.shape) != (B, H, W, 2) or flo.dtype != torch.float32 or not flo.is_contiguous() or flo.device != img.device:
        raise ValueError("warp_bwd takes a dense fp32 (B,H,W,2) flow on the image's device")
    if mode not in ("clamp", "tfwarp"):
        raise ValueError("unknown warp mode '{}'".format(mode))
    L = _hip.lib()
    dt = _DTYPES[img.dtype]
    gi = torch.empty_like(img) if need_img else None
    gf = torch.empty((B, H, W, 2), dtype=torch.float32, device=img.device) if need_flo else None
    nws = L.qpwc_warp_bwd_workspace_floats(B, H, W, C, dt) if need_img else 0
    _hip.check(min(int(nws), 0))
    ws = torch.empty(nws, dtype=torch.float32, device=img.device) if nws > 0 else None
    with torch.cuda.device(img.device), _timed("warp_bwd_" + mode, (B, H, W, C)):
        rc = L.qpwc_warp_bwd(img.data_ptr(), flo.data_ptr(), grad_out.data_ptr(), gi.data_ptr() if need_img else None,
                             gf.data_ptr() if need_flo else None, ws.data_ptr() if ws is not None else None, B, H, W, C,
                             dt, _hip.WARP_CLAMP if mode == "clamp" else _hip.WARP_TFWARP, _stream(img))
    _hip.check(rc)
    return gi, gf


def _grad_flow(flo, img, data_format):
    """The flow as _WarpFn takes it: fp32, expanded to the image's batch and pixels (torch ops, so that autograd
    reduces a broadcast flow's gradient and casts an fp16 flow's back)."""
    if not isinstance(flo, torch.Tensor) or flo.dim() != 4:
        raise ValueError("flo must be a rank 4 tensor")
    if data_format == CHANNELS_LAST:
        B, H, W = img.shape[0], img.shape[1], img.shape[2]
        full = (B, H, W, 2)
    else:
        B, H, W = img.shape[0], img.shape[2], img.shape[3]
        full = (B, 2, H, W)
    # warp()'s flo32 (the fp32 coordinates flow_head_up() returns beside an fp16 flow) is for the no-grad path only: it
    # holds exactly flo.float() (fp16 -> fp32 is exact), so this cast gives the same forward bits, and unlike a
    # separate tensor it stays connected to flo in the autograd graph.
    f = flo.to(torch.float32)
    try:
        return f.expand(full)
    except RuntimeError:
        raise ValueError("flo shape {} is not broadcastable to the image".format(tuple(flo.shape)))


def warp(img, flo, mode="clamp", data_format=CHANNELS_LAST, flo32=None):
    """Warp (mode 'tfwarp', qpwcnet/core/warp.py:63-153) / WarpV2 (mode 'clamp',
    qpwcnet/core/layers.py:177-186): sample img at (y + flo[...,1], x + flo[...,0]).
    flo32: flo's values as a dense fp32 tensor of flo's shape, from a caller that has them (flow_head_up()): the
    coordinates are read from it instead of a cast of flo.  Differentiable in img and flo: with grad enabled and an input
    requiring grad the same forward runs inside an autograd Function whose backward is qpwc_warp_bwd (flo32 is not read)."""
    if flo32 is not None and isinstance(flo, torch.Tensor) and not (
            isinstance(flo32, torch.Tensor) and flo32.dtype == torch.float32 and flo32.shape == flo.shape and
            flo32.device == flo.device and flo32.is_contiguous()):
        raise ValueError("flo32 must be a dense fp32 tensor of flo's shape on flo's device")
    if _wants_grad(img, flo):
        _refuse_capture("the warp")
        _check_tensor("img", img)
        get_axis(data_format)
        if mode not in ("clamp", "tfwarp"):
            raise ValueError("unknown warp mode '{}'".format(mode))
        return _WarpFn.apply(img, _grad_flow(flo, img, data_format), mode, data_format)
    _check_tensor("img", img)
    if not isinstance(flo, torch.Tensor) or not flo.is_cuda or flo.device != img.device:
        raise RuntimeError("flo must be a tensor on the same HIP device as img")
    if mode not in ("clamp", "tfwarp"):
        raise ValueError("unknown warp mode '{}'".format(mode))
    i, layout, dims, as_view = _physical(img, data_format)
    B, H, W, C = dims
    if layout == _hip.NCHW and C % 4 == 0 and (H >= 2 and W >= 2 or mode == "tfwarp"):
        # dense (B,C,H,W): the 16-byte gather kernel on a channels-last copy (flow: 2 channels, permuted)
        out_l = warp(layout_transpose(i, CHANNELS_LAST), (flo if flo32 is None else flo32).permute(0, 2, 3, 1), mode, CHANNELS_LAST)
        return layout_transpose(out_l, CHANNELS_FIRST)
    f, mask = _flow_physical(flo, dims, data_format, layout, flo32)
    buf, out = _empty_like_layout(i, dims, C, layout, as_view)
    with torch.cuda.device(i.device), _timed("warp_" + mode, dims):
        rc = _hip.lib().qpwc_warp_fwd(
            i.data_ptr(), f.data_ptr(), buf.data_ptr(), B, H, W, C, mask, layout,
            _DTYPES[i.dtype], _hip.WARP_CLAMP if mode == "clamp" else _hip.WARP_TFWARP,
            _stream(i))
    _hip.check(rc)
    return out


def cost_volume_into(prv, nxt, out, channel_offset=0, search_range=4, lrelu_slope=0.1, flo=None):
    """NHWC cost volume written into channels [offset, offset+d*d) of the wider
    channels-last buffer ``out`` (B,H,W,Ctot) -- Flow/UpFlow's concat target
    (qpwcnet/core/non_layers.py:332-338, 381-385).  With ``flo`` the WarpV2 of
    ``nxt`` is fused in (non_layers.py:377-380) and ``nxt_w`` never exists."""
    _check_tensor("prv", prv)
    _check_tensor("nxt", nxt)
    _check_tensor("out", out)
    if prv.shape != nxt.shape or prv.dtype != nxt.dtype or out.dtype != prv.dtype:
        raise ValueError("prv, nxt (and out's dtype) must match")
    if not (prv.is_contiguous() and nxt.is_contiguous() and out.is_contiguous()):
        raise ValueError("cost_volume_into needs dense NHWC tensors")
    B, H, W, C = prv.shape
    if out.shape[:3] != prv.shape[:3]:
        raise ValueError("out must be (B,H,W,Ctot) with the image's B,H,W")
    L = _hip.lib()
    with torch.cuda.device(prv.device), \
            _timed("cost_volume" if flo is None else "warp_cost_volume", (B, H, W, C)):
        if flo is None:
            rc = L.qpwc_cost_volume_fwd_strided(
                prv.data_ptr(), nxt.data_ptr(), out.data_ptr(), B, H, W, C, int(search_range),
                _DTYPES[prv.dtype], float(lrelu_slope), out.shape[3], int(channel_offset),
                _stream(prv))
        else:
            if tuple(flo.shape) != (B, H, W, 2) or flo.dtype != torch.float32 or \
                    not flo.is_contiguous() or flo.device != prv.device:
                raise ValueError("flo must be a dense fp32 (B,H,W,2) tensor on the same device")
            rc = L.qpwc_warp_cost_volume_fwd(
                prv.data_ptr(), nxt.data_ptr(), flo.data_ptr(), out.data_ptr(), B, H, W, C,
                int(search_range), _DTYPES[prv.dtype], float(lrelu_slope), out.shape[3],
                int(channel_offset), _stream(prv))
    _hip.check(rc)
    return out


def warp_cost_volume(prv, nxt, flo, search_range=4, lrelu_slope=0.1):
    """cost_volume(prv, WarpV2(nxt, flo)) in one launch; NHWC, dense result."""
    d = 2 * int(search_range) + 1
    out = torch.empty(prv.shape[:3] + (d * d,), dtype=prv.dtype, device=prv.device)
    return cost_volume_into(prv, nxt, out, 0, search_range, lrelu_slope, flo=flo)


def epe(y_true, y_pred, data_format=CHANNELS_LAST):
    """End-point error, qpwcnet/app/optical_flow/train.py:247-253 -> 0-dim tensor."""
    for name, t in (("y_true", y_true), ("y_pred", y_pred)):
        _check_tensor(name, t)
        if t.dtype != torch.float32:
            raise ValueError("{} must be float32".format(name))
    if y_true.shape != y_pred.shape:
        raise ValueError("y_true and y_pred must have the same shape")
    get_axis(data_format)
    a, b = y_true.contiguous(), y_pred.contiguous()
    if data_format == CHANNELS_LAST:
        B, H, W, C = a.shape
        layout = _hip.NHWC
    else:
        B, C, H, W = a.shape
        layout = _hip.NCHW
    if C != 2:
        raise ValueError("flows must have 2 channels")
    L = _hip.lib()
    # per-call scratch: stream-ordered reuse across concurrent streams would race
    ws = torch.empty(L.qpwc_epe_workspace_floats(), dtype=torch.float32, device=a.device)
    out = torch.empty((), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = L.qpwc_epe_fwd(a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), B, H, W,
                            layout, _stream(a))
    _hip.check(rc)
    return out


def dwconv3x3(sources, weight, mish_on_load=False):
    """Depthwise 3x3 'same' convolution over the channel-wise concatenation of 1..3
    channels-last fp32/fp16 sources (each (B,H,W,Ci), last dim contiguous; fp32 weights) -- the
    depthwise half of OptFlow's SeparableConv2D (qpwcnet/core/non_layers.py:223-231) without ever
    building Flow/UpFlow's concat (non_layers.py:336-338, 381-385).
    weight: (C,1,3,3) or (C,3,3) with C = sum(Ci).  -> (B,H,W,C)."""
    keep, c_ptrs, c_ch, c_st, B, H, W, C = _dw_sources(sources)
    w = weight.reshape(-1, 9)
    if w.shape[0] != C or w.dtype != torch.float32 or not w.is_cuda:
        raise ValueError("weight must be fp32 (C,3,3) on the device with C = {}".format(C))
    w = w.contiguous()
    out = torch.empty((B, H, W, C), dtype=keep[0].dtype, device=keep[0].device)
    with torch.cuda.device(out.device), _timed("dwconv3x3", (B, H, W, C)):
        rc = _hip.lib().qpwc_dwconv3x3_fwd(c_ptrs, c_ch, c_st, len(keep), int(bool(mish_on_load)),
                                            w.data_ptr(), out.data_ptr(), B, H, W, _DTYPES[out.dtype],
                                            _stream(out))
    _hip.check(rc)
    return out


def flow_head(z, params, scale, out_format=CHANNELS_LAST):
    """Tail of OptFlow (non_layers.py:238-254, 268-273) on the pre-activation 16-channel
    tensor z (B,H,W,16): scale * conv3x3(BN(Mish(W1 Mish(z) + b1))) -> (B,H,W,2), or (B,2,H,W) for
    out_format 'channels_first' (a channels_first model's output, written by the kernel itself).
    params: packed fp32 vector, see include/qpwc.h / non_layers.pack_flow_head."""
    _check_tensor("z", z)
    if z.shape[3] != 16 or not z.is_contiguous():
        raise ValueError("z must be a dense (B,H,W,16) tensor")
    L = _hip.lib()
    if params.numel() != L.qpwc_flow_head_param_floats() or params.dtype != torch.float32 or \
            not params.is_cuda or not params.is_contiguous():
        raise ValueError("params must be a dense fp32 device vector of {} floats".format(
            L.qpwc_flow_head_param_floats()))
    B, H, W, _ = z.shape
    get_axis(out_format)
    cf = out_format == CHANNELS_FIRST
    out = torch.empty((B, 2, H, W) if cf else (B, H, W, 2), dtype=z.dtype, device=z.device)
    with torch.cuda.device(z.device), _timed("flow_head", (B, H, W, 16)):
        rc = L.qpwc_flow_head_fwd(z.data_ptr(), params.data_ptr(), out.data_ptr(), B, H, W,
                                  float(scale), _DTYPES[z.dtype], _hip.NCHW if cf else _hip.NHWC, _stream(z))
    _hip.check(rc)
    return out


def pack_flow_head(w1, b1, gamma, beta, mean, var, eps, wf):
    """Parameter vector of qpwc_flow_head_fwd (include/qpwc.h): w1[16][16] | b1 | bn_scale |
    bn_shift | wf[ky][kx][in][out]; BatchNorm folded to scale/shift."""
    w1, b1, gamma, beta, mean, var, wf = (t.float() for t in (w1, b1, gamma, beta, mean, var, wf))
    bn_scale = gamma / torch.sqrt(var + eps)
    bn_shift = beta - mean * bn_scale
    return torch.cat([w1.reshape(16, 16).reshape(-1), b1.reshape(-1), bn_scale.reshape(-1),
                      bn_shift.reshape(-1), wf.permute(2, 3, 1, 0).reshape(-1)]).contiguous()


def _head_operands(z, w1, b1, gamma, beta, mean, var, wf):
    """Shape / dtype / device rules of the trainable flow head's operands (the torch layouts of weights.py)."""
    _check_tensor("z", z)
    if z.dtype != torch.float32 or z.shape[3] != 16:
        raise ValueError("z must be an fp32 (B,H,W,16) tensor, got {} {}".format(z.dtype, tuple(z.shape)))
    for name, t, numel in (("w1", w1, 256), ("b1", b1, 16), ("gamma", gamma, 16), ("beta", beta, 16), ("mean", mean, 16),
                           ("var", var, 16), ("wf", wf, 288)):
        if not isinstance(t, torch.Tensor) or t.device != z.device:
            raise RuntimeError("qpwcnet_amd: {} must be a tensor on z's HIP device (no CPU fallback)".format(name))
        if t.dtype != torch.float32 or t.numel() != numel:
            raise ValueError("{} must hold {} fp32 values, got {} {}".format(name, numel, t.dtype, tuple(t.shape)))
    if tuple(wf.shape) != (2, 16, 3, 3):
        raise ValueError("wf must be the (2,16,3,3) kernel of the flow convolution, got {}".format(tuple(wf.shape)))


def flow_head_stats(z, w1, b1, gamma, beta, mean, var, wf, momentum=0.99, eps=1e-3):
    """Training-mode BatchNorm of the flow head (qpwc_flow_head_stats_fwd): the batch mean and biased variance of
    Mish(W1 Mish(z) + b1) over all pixels of z (B,H,W,16) -> (params, stats): the 592-float vector flow_head() takes,
    normalising with the batch statistics, and those statistics as mean | var | mean_lo (48 floats; mean_lo: what the
    fp32 mean dropped, which keeps the backward's normalised activations centred when |mean| >> std).  mean / var (the layer's
    moving buffers) are updated in place on the device, moving * momentum + batch * (1 - momentum); None for both
    leaves out the update.  Two launches, no host synchronisation."""
    moving = mean is not None
    _head_operands(z, w1, b1, gamma, beta, mean if moving else b1, var if moving else b1, wf)
    if moving and not (mean.is_contiguous() and var.is_contiguous()):
        raise ValueError("the moving buffers are updated in place: dense tensors")
    z = z.contiguous()
    B, H, W, _ = z.shape
    L = _hip.lib()
    nws = int(L.qpwc_flow_head_stats_workspace_floats(B, H, W))
    _hip.check(min(nws, 0))
    ws = torch.empty(nws, dtype=torch.float32, device=z.device)
    params = torch.empty(L.qpwc_flow_head_param_floats(), dtype=torch.float32, device=z.device)
    stats = torch.empty(48, dtype=torch.float32, device=z.device)
    w1c, b1c, gc, bc = (t.detach().contiguous() for t in (w1, b1, gamma, beta))
    wfp = wf.detach().permute(2, 3, 1, 0).contiguous()
    with torch.cuda.device(z.device), _timed("flow_head_stats", (B, H, W, 16)):
        rc = L.qpwc_flow_head_stats_fwd(z.data_ptr(), w1c.data_ptr(), b1c.data_ptr(), gc.data_ptr(), bc.data_ptr(),
                                        wfp.data_ptr(), mean.data_ptr() if moving else None,
                                        var.data_ptr() if moving else None, float(momentum), float(eps),
                                        params.data_ptr(), stats.data_ptr(), ws.data_ptr(), B, H, W, _stream(z))
    _hip.check(rc)
    return params, stats


def frozen_stats(mean, var):
    """mean | var | 0 (48 floats): the statistics operand of flow_head_bwd() for frozen (moving) statistics."""
    return torch.cat([mean.reshape(-1).float(), var.reshape(-1).float(), torch.zeros_like(mean.reshape(-1)).float()])


def flow_head_bwd(z, params, stats, scale, grad_out, training=False, eps=1e-3,
                  need=(True, True, True, True, True, True)):
    """Gradients of flow_head() (fp32 channels-last, qpwc_flow_head_bwd) for grad_out = dL/dflow (B,H,W,2).  params:
    the vector the forward ran with, stats: mean | var | mean_lo (48 floats, frozen_stats() / flow_head_stats()) it was made from, training: whether those were the
    batch statistics.  need = (z, w1, b1, gamma, beta, wf) -> (grad_z (B,H,W,16), grad_w1 (16,16), grad_b1 (16),
    grad_gamma (16), grad_beta (16), grad_wf (3,3,16,2) as (ky,kx,in,out)); what is not asked for comes back as None."""
    _check_tensor("z", z)
    _check_tensor("grad_out", grad_out)
    B, H, W, _ = z.shape
    if z.dtype != torch.float32 or z.shape[3] != 16 or not z.is_contiguous():
        raise ValueError("z must be a dense fp32 (B,H,W,16) tensor")
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (B, H, W, 2) or grad_out.device != z.device:
        raise ValueError("grad_out must be fp32 {} on z's device, got {} {}".format(
            (B, H, W, 2), grad_out.dtype, tuple(grad_out.shape)))
    L = _hip.lib()
    for name, t, numel in (("params", params, L.qpwc_flow_head_param_floats()), ("stats", stats, 48)):
        if t.numel() != numel or t.dtype != torch.float32 or t.device != z.device or not t.is_contiguous():
            raise ValueError("{} must be a dense fp32 vector of {} floats on z's device".format(name, numel))
    if len(need) != 6 or not any(need):
        raise ValueError("need holds six flags (z, w1, b1, gamma, beta, wf), at least one set")
    grad_out = grad_out.contiguous()
    ws, outs, ptrs = _bwd_buffers(L.qpwc_flow_head_bwd_workspace_floats(B, H, W),
                                  ((B, H, W, 16), (16, 16), (16,), (16,), (16,), (3, 3, 16, 2)), need, z.device)
    with torch.cuda.device(z.device), _timed("flow_head_bwd", (B, H, W, 16)):
        rc = L.qpwc_flow_head_bwd(z.data_ptr(), params.data_ptr(), stats.data_ptr(), float(eps), int(bool(training)),
                                  float(scale), grad_out.data_ptr(), *ptrs, ws.data_ptr(), B, H, W,
                                  _stream(z))
    _hip.check(rc)
    return tuple(outs)


class _FlowHeadFn(torch.autograd.Function):
    """The flow head with qpwc_flow_head_bwd as its gradient.  The forward is flow_head() itself on a parameter vector
    made from the moving statistics (inference mode) or by flow_head_stats() from the batch (training mode); z, that
    vector and the statistics are saved, nothing else (the backward recomputes the activations)."""

    @staticmethod
    def forward(ctx, z, w1, b1, gamma, beta, wf, mean, var, scale, training, momentum, eps):
        _refuse_capture("the flow head")
        z = z.contiguous()
        if training:
            # mean / var are written in place through their raw pointers: no mark_dirty, no version bump.  They are
            # buffers that never require grad and nothing here saves them for backward (the batch statistics travel
            # in `stats`); a caller that saved them in another autograd node would not be warned of the update.
            params, stats = flow_head_stats(z, w1, b1, gamma, beta, mean, var, wf, momentum, eps)
        else:
            params = pack_flow_head(w1, b1, gamma, beta, mean, var, eps, wf)
            stats = frozen_stats(mean, var)
        out = flow_head(z, params, scale)
        ctx.save_for_backward(z, params, stats)
        ctx.cfg = (float(scale), bool(training), float(eps), w1.shape, wf.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the flow-head backward")
        z, params, stats = ctx.saved_tensors
        scale, training, eps, w1_shape, wf_shape = ctx.cfg
        gz, gw1, gb1, gg, gb, gwf = flow_head_bwd(z, params, stats, scale, grad_out.to(torch.float32), training, eps,
                                                  tuple(ctx.needs_input_grad[:6]))
        return (gz, gw1.reshape(w1_shape) if gw1 is not None else None, gb1, gg, gb,
                gwf.permute(3, 2, 0, 1).reshape(wf_shape) if gwf is not None else None) + (None,) * 6


def flow_head_train(z, w1, b1, gamma, beta, mean, var, wf, scale, training=False, momentum=0.99, eps=1e-3):
    """The flow head on its own parameter tensors, trainable (fp32, channels-last): scale * conv3x3(BN(Mish(W1 Mish(z) +
    b1)), wf) -> (B,H,W,2) for z (B,H,W,16), w1 (16,16,1,1), b1 / gamma / beta (16), wf (2,16,3,3), mean / var the
    BatchNorm's moving buffers (16).  training=False normalises with the moving statistics: the launch, and the bits,
    of flow_head(z, pack_flow_head(...)).  training=True normalises with the batch statistics and updates mean / var
    in place, without grad, as Keras' BatchNormalization(fused=False) does: moving * momentum + batch * (1 - momentum),
    biased variance (flow_head_stats()).  Differentiable in z, w1, b1, gamma, beta and wf: with grad enabled and one of
    them requiring grad the same forward runs inside an autograd Function whose backward is qpwc_flow_head_bwd."""
    if _wants_grad(z, w1, b1, gamma, beta, wf):
        _refuse_capture("the flow head")
        if isinstance(z, torch.Tensor) and z.dtype == torch.float16:
            raise ValueError("the flow head has no gradient for fp16 storage: train in fp32")
        _head_operands(z, w1, b1, gamma, beta, mean, var, wf)
        return _FlowHeadFn.apply(z, w1, b1, gamma, beta, wf, mean, var, float(scale), bool(training), float(momentum),
                                 float(eps))
    if training:
        if isinstance(z, torch.Tensor) and z.dtype == torch.float16:
            raise ValueError("the flow head's batch statistics are fp32 only: train in fp32")
        params, _ = flow_head_stats(z, w1, b1, gamma, beta, mean, var, wf, momentum, eps)
        return flow_head(z.contiguous(), params, scale)
    return flow_head(z, pack_flow_head(w1, b1, gamma, beta, mean, var, eps, wf), scale)


def pointwise_bias(y, pw_padded, bias):
    """Pointwise 1x1 + bias of a split SeparableConv2D on the matrix cores (qpwc_pointwise_bias_fwd): y (..., C) fp32 dense
    -> (..., F) = y . W^T + bias, W = pw_padded (F, ceil(C/32)*32) from pad_pointwise().  The own replacement of the library
    GEMM behind dwconv3x3() on the few-pixel levels."""
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise RuntimeError("qpwcnet_amd: y must be a tensor on a HIP device (no CPU fallback)")
    C = y.shape[-1]
    F_, cpad = pw_padded.shape
    if y.dtype != torch.float32 or not y.is_contiguous() or pw_padded.dtype != torch.float32 or not pw_padded.is_contiguous() \
            or cpad != (C + 31) // 32 * 32 or bias.numel() != F_ or bias.dtype != torch.float32 or not bias.is_contiguous():
        raise ValueError("pointwise_bias takes dense fp32 y (..., C), weights (F, ceil(C/32)*32) from pad_pointwise, bias (F)")
    M = y.numel() // C
    out = torch.empty(y.shape[:-1] + (F_,), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device), _timed("pointwise_bias", (M, C, F_)):
        rc = _hip.lib().qpwc_pointwise_bias_fwd(y.data_ptr(), pw_padded.data_ptr(), bias.data_ptr(), out.data_ptr(), M, C, F_,
                                                _stream(y))
    _hip.check(rc)
    return out


def flow_head_up(z, params, scale, up_scale=2.0):
    """flow_head() (channels-last) and the Upsample(x2, * up_scale) that follows it in the flow chain (pwcnet.py:55,60) in one
    launch (qpwc_flow_head_up_fwd) -> (flow (B,H,W,2), up = up_scale * bilinear x2 of it (B,2H,2W,2), up32); up equals
    upsample2x_flow(flow, up_scale) bit for bit.  up32: fp16 storage: up.float(), written by the same launch (the next
    level's WarpV2 takes fp32 coordinates, warp(flo32=...), and the cast was a launch per level); fp32 storage: None."""
    _check_tensor("z", z)
    if z.shape[3] != 16 or not z.is_contiguous():
        raise ValueError("z must be a dense (B,H,W,16) tensor")
    L = _hip.lib()
    if params.numel() != L.qpwc_flow_head_param_floats() or params.dtype != torch.float32 or \
            not params.is_cuda or not params.is_contiguous():
        raise ValueError("params must be a dense fp32 device vector of {} floats".format(
            L.qpwc_flow_head_param_floats()))
    B, H, W, _ = z.shape
    out = torch.empty((B, H, W, 2), dtype=z.dtype, device=z.device)
    up = torch.empty((B, 2 * H, 2 * W, 2), dtype=z.dtype, device=z.device)
    up32 = torch.empty((B, 2 * H, 2 * W, 2), dtype=torch.float32, device=z.device) if z.dtype == torch.float16 else None
    with torch.cuda.device(z.device), _timed("flow_head", (B, H, W, 16)):
        rc = L.qpwc_flow_head_up_fwd(z.data_ptr(), params.data_ptr(), out.data_ptr(), up.data_ptr(),
                                     up32.data_ptr() if up32 is not None else None, B, H, W,
                                     float(scale), float(up_scale), _DTYPES[z.dtype], _stream(z))
    _hip.check(rc)
    return out, up, up32


def optflow_tail(z2, dw3, pw3, b3, dw4, pw4, b4, head_params, scale, mish_on_load=False, out_format=CHANNELS_LAST):
    """Last two SeparableConv2D (64 -> 32 -> 16) + flow head of OptFlow (non_layers.py:223-231, 238-254,
    268-273) in one launch (qpwc_optflow_tail_fwd): z2 (B,H,W,64) fp32, the second layer's output (activated
    unless mish_on_load) -> flow (B,H,W,2) / (B,2,H,W).  For the coarse pyramid levels."""
    _check_tensor("z2", z2)
    if z2.dtype != torch.float32 or z2.shape[3] != 64 or not z2.is_contiguous():
        raise ValueError("z2 must be a dense fp32 (B,H,W,64) tensor")
    for name, t, shape in (("dw3", dw3, (64, 9)), ("pw3", pw3, (32, 64)), ("b3", b3, (32,)), ("dw4", dw4, (32, 9)),
                           ("pw4", pw4, (16, 32)), ("b4", b4, (16,))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("{} must be a dense fp32 device tensor of shape {}".format(name, shape))
    L = _hip.lib()
    if head_params.numel() != L.qpwc_flow_head_param_floats() or head_params.dtype != torch.float32:
        raise ValueError("head_params must hold {} fp32 values".format(L.qpwc_flow_head_param_floats()))
    get_axis(out_format)
    cf = out_format == CHANNELS_FIRST
    B, H, W, _ = z2.shape
    out = torch.empty((B, 2, H, W) if cf else (B, H, W, 2), dtype=torch.float32, device=z2.device)
    with torch.cuda.device(z2.device), _timed("optflow_tail", (B, H, W, 64)):
        rc = L.qpwc_optflow_tail_fwd(z2.data_ptr(), dw3.data_ptr(), pw3.data_ptr(), b3.data_ptr(), dw4.data_ptr(),
                                     pw4.data_ptr(), b4.data_ptr(), head_params.data_ptr(), out.data_ptr(), B, H, W,
                                     float(scale), int(bool(mish_on_load)), _hip.NCHW if cf else _hip.NHWC,
                                     _stream(z2))
    _hip.check(rc)
    return out


def bias_mish_(x_nhwc, bias=None):
    """In place x = Mish(x + bias) on a dense channels-last fp32 tensor (..., C), C % 4 == 0 --
    the `activation='Mish'` epilogue of the reference's conv blocks (non_layers.py:196-210,
    390-449).  Returns x."""
    _check_tensor("x", x_nhwc)
    if not x_nhwc.is_contiguous():
        raise ValueError("bias_mish_ needs a dense channels-last tensor")
    C = x_nhwc.shape[-1]
    if bias is not None and (bias.numel() != C or bias.dtype != torch.float32 or not bias.is_cuda):
        raise ValueError("bias must be a fp32 device vector of {} elements".format(C))
    n = x_nhwc.numel() // C
    with torch.cuda.device(x_nhwc.device), _timed("bias_mish", tuple(x_nhwc.shape)):
        rc = _hip.lib().qpwc_bias_mish_fwd(x_nhwc.data_ptr(), 0 if bias is None else bias.data_ptr(),
                                            n, C, _DTYPES[x_nhwc.dtype], _stream(x_nhwc))
    _hip.check(rc)
    return x_nhwc


def upsample2x_flow_bwd(grad_out, scale=1.0):
    """Adjoint of upsample2x_flow() (fp32 channels-last, qpwc_upsample2x_flow_bwd): grad_out (B,2h,2w,2) -> (B,h,w,2)."""
    _check_tensor("grad_out", grad_out)
    B, H2, W2, C = grad_out.shape
    if grad_out.dtype != torch.float32 or C != 2 or H2 % 2 or W2 % 2:
        raise ValueError("upsample2x_flow_bwd takes an fp32 (B,2h,2w,2) gradient, got {} {}".format(
            grad_out.dtype, tuple(grad_out.shape)))
    g = grad_out.contiguous()
    out = torch.empty((B, H2 // 2, W2 // 2, 2), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device), _timed("upsample2x_flow_bwd", (B, H2 // 2, W2 // 2, 2)):
        rc = _hip.lib().qpwc_upsample2x_flow_bwd(g.data_ptr(), out.data_ptr(), B, H2 // 2, W2 // 2, float(scale),
                                                  _stream(g))
    _hip.check(rc)
    return out


class _UpsampleFn(torch.autograd.Function):
    """upsample2x_flow() with qpwc_upsample2x_flow_bwd as its gradient: the forward is the no-grad forward itself."""

    @staticmethod
    def forward(ctx, flo, scale, in_format, out_format):
        _refuse_capture("the flow upsampling")
        ctx.cfg = (float(scale), in_format, out_format)
        return upsample2x_flow(flo, scale, in_format, out_format)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the flow-upsampling backward")
        scale, in_format, out_format = ctx.cfg
        g = upsample2x_flow_bwd(_to_nhwc(grad_out.to(torch.float32), out_format), scale)
        return _from_nhwc(g, in_format), None, None, None


def upsample2x_flow(flo, scale=1.0, in_format=CHANNELS_LAST, out_format=CHANNELS_LAST):
    """scale * bilinear x2 upsampling of a flow (B,h,w,2) [(B,2,h,w) for in_format 'channels_first'] --
    the reference's Upsample functor (non_layers.py:183-193) as used on flows (pwcnet.py:55,60);
    out (B,2h,2w,2) or (B,2,2h,2w) by out_format.
    Differentiable (fp32) in flo: with grad enabled and flo requiring grad the same forward runs inside an autograd
    Function whose backward is qpwc_upsample2x_flow_bwd."""
    if _wants_grad(flo):
        _refuse_capture("the flow upsampling")
        if flo.dtype == torch.float16:
            raise ValueError("upsample2x_flow has no gradient for fp16 storage: train in fp32")
        _check_tensor("flo", flo)
        get_axis(in_format)
        get_axis(out_format)
        return _UpsampleFn.apply(flo, scale, in_format, out_format)
    _check_tensor("flo", flo)
    get_axis(in_format)
    get_axis(out_format)
    if flo.shape[1 if in_format == CHANNELS_FIRST else 3] != 2:
        raise ValueError("upsample2x_flow takes a 2-channel flow, got shape {}".format(tuple(flo.shape)))
    f = flo.contiguous()
    if in_format == CHANNELS_FIRST:
        B, _, h, w = f.shape
    else:
        B, h, w, _ = f.shape
    ocf = out_format == CHANNELS_FIRST
    out = torch.empty((B, 2, 2 * h, 2 * w) if ocf else (B, 2 * h, 2 * w, 2), dtype=f.dtype, device=f.device)
    with torch.cuda.device(f.device), _timed("upsample2x_flow", (B, h, w, 2)):
        rc = _hip.lib().qpwc_upsample2x_flow_fwd(f.data_ptr(), out.data_ptr(), B, h, w, float(scale),
                                                  _DTYPES[f.dtype],
                                                  _hip.NCHW if in_format == CHANNELS_FIRST else _hip.NHWC,
                                                  _hip.NCHW if ocf else _hip.NHWC, _stream(f))
    _hip.check(rc)
    return out


def _image_head_check(z, w2, b2, what):
    """What the image head asks of its operands: z (B,H,W,64), w2 (3,64[,1,1]) and b2 (3; None in the backward, which
    does not read it), fp32 on a HIP device."""
    _check_tensor("z", z)
    for name, t in (("z", z), ("w2", w2)) + ((("b2", b2),) if b2 is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if not t.is_cuda:
            raise RuntimeError("qpwcnet_amd: {} is on '{}'; the hot path runs on a HIP device only "
                               "(no CPU fallback)".format(name, t.device))
        if t.dtype == torch.float16:
            raise ValueError("{} has no fp16 storage path ({} is fp16): train in fp32".format(what, name))
        if t.dtype != torch.float32:
            raise ValueError("{}: {} must be fp32, got {}".format(what, name, t.dtype))
    if z.shape[3] != 64 or w2.dim() < 2 or w2.shape[0] != 3 or w2.numel() != 192 or (b2 is not None and b2.numel() != 3):
        raise ValueError("{} takes z (B,H,W,64), w2 (3,64) and b2 (3), got {}, {} and {}".format(
            what, tuple(z.shape), tuple(w2.shape), None if b2 is None else tuple(b2.shape)))


def image_head_bwd(z, w2, grad_out, need=(True, True, True)):
    """Gradients of image_head() (fp32 channels-last, qpwc_image_head_bwd) for grad_out = dL/d(out), (B,H,W,3).
    need = (z, w2, b2) -> (grad_z (B,H,W,64), grad_w2 (3,64), grad_b2 (3)); whatever is not asked for comes back as
    None."""
    _image_head_check(z, w2, None, "image_head_bwd")
    _check_tensor("grad_out", grad_out)
    B, H, W, _ = z.shape
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != (B, H, W, 3):
        raise ValueError("image_head_bwd: grad_out must be fp32 {}, got {} {}".format(
            (B, H, W, 3), grad_out.dtype, tuple(grad_out.shape)))
    if not any(need):
        raise ValueError("image_head_bwd: nothing asked for")
    z, w, g = z.contiguous(), w2.reshape(3, 64).contiguous(), grad_out.contiguous()
    M = B * H * W
    L = _hip.lib()
    ws, outs, ptrs = _bwd_buffers(L.qpwc_image_head_bwd_workspace_floats(M), [(B, H, W, 64), (3, 64), (3,)], need,
                                  z.device)
    with torch.cuda.device(z.device), _timed("image_head_bwd", (B, H, W, 64)):
        rc = L.qpwc_image_head_bwd(z.data_ptr(), w.data_ptr(), g.data_ptr(), *ptrs, ws.data_ptr(), M, _stream(z))
    _hip.check(rc)
    return tuple(outs)


class _ImageHeadFn(torch.autograd.Function):
    """image_head() with qpwc_image_head_bwd as its gradient: the forward is the no-grad forward itself; z and w2 are
    saved."""

    @staticmethod
    def forward(ctx, z, w2, b2):
        _refuse_capture("the image head")
        out = image_head(z, w2, b2)
        ctx.save_for_backward(z, w2)
        ctx.b2_shape = tuple(b2.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the image-head backward")
        z, w2 = ctx.saved_tensors
        gz, gw, gb = image_head_bwd(z, w2, grad_out.to(torch.float32), tuple(ctx.needs_input_grad[:3]))
        return (gz, gw.reshape(w2.shape) if gw is not None else None,
                gb.reshape(ctx.b2_shape) if gb is not None else None)


def image_head(z, w2, b2):
    """The image head of a FrameInterpolate block, Conv2D(3, 1x1) on its 64 features (qpwcnet/core/non_layers.py:293,
    311): z (B,H,W,64) fp32 channels-last, w2 (3,64) or the torch kernel (3,64,1,1), b2 (3) -> (B,H,W,3)
    (qpwc_image_head_fwd).  No activation: z is what the block's SeparableConv2D stored.
    Differentiable in z, w2 and b2: with grad enabled and one of them requiring grad the same forward runs inside an
    autograd Function whose backward is qpwc_image_head_bwd."""
    if _wants_grad(z, w2, b2):
        _refuse_capture("the image head")
        _image_head_check(z, w2, b2, "image_head")
        return _ImageHeadFn.apply(z, w2, b2)
    _image_head_check(z, w2, b2, "image_head")
    zc, w, b = z.contiguous(), w2.reshape(3, 64).contiguous(), b2.contiguous()
    B, H, W, _ = zc.shape
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device=zc.device)
    with torch.cuda.device(zc.device), _timed("image_head", (B, H, W, 64)):
        rc = _hip.lib().qpwc_image_head_fwd(zc.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), B * H * W,
                                             _stream(zc))
    _hip.check(rc)
    return out


def _image_check(name, t, what):
    """An fp32 channels-last image (B,h,w,C) of 1..4 channels on a HIP device."""
    _check_tensor(name, t)
    if t.dtype == torch.float16:
        raise ValueError("{} has no fp16 storage path ({} is fp16): train in fp32".format(what, name))
    if not 1 <= t.shape[3] <= 4:
        raise ValueError("{} takes a channels-last image of 1..4 channels, got shape {}".format(what, tuple(t.shape)))


def upsample2x_image_bwd(grad_out, scale=1.0):
    """Adjoint of upsample2x_image() (fp32 channels-last, qpwc_upsample2x_image_bwd): grad_out (B,2h,2w,C) ->
    (B,h,w,C)."""
    _image_check("grad_out", grad_out, "upsample2x_image_bwd")
    B, H2, W2, C = grad_out.shape
    if H2 % 2 or W2 % 2:
        raise ValueError("upsample2x_image_bwd takes a (B,2h,2w,C) gradient, got {}".format(tuple(grad_out.shape)))
    g = grad_out.contiguous()
    out = torch.empty((B, H2 // 2, W2 // 2, C), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device), _timed("upsample2x_image_bwd", (B, H2 // 2, W2 // 2, C)):
        rc = _hip.lib().qpwc_upsample2x_image_bwd(g.data_ptr(), out.data_ptr(), B, H2 // 2, W2 // 2, C, float(scale),
                                                   _stream(g))
    _hip.check(rc)
    return out


class _UpsampleImageFn(torch.autograd.Function):
    """upsample2x_image() with qpwc_upsample2x_image_bwd as its gradient: the forward is the no-grad forward itself."""

    @staticmethod
    def forward(ctx, img, scale):
        _refuse_capture("the image upsampling")
        ctx.scale = float(scale)
        return upsample2x_image(img, scale)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the image-upsampling backward")
        return upsample2x_image_bwd(grad_out.to(torch.float32), ctx.scale), None


def upsample2x_image(img, scale=1.0):
    """scale * bilinear x2 upsampling of an image (B,h,w,C), C in 1..4, fp32 channels-last -> (B,2h,2w,C): the
    reference's Upsample functor (non_layers.py:183-193) as the interpolator uses it on its 3-channel images
    (pwcnet.py:108,124), one launch (qpwc_upsample2x_image_fwd).  Two channels come out with the bits of
    upsample2x_flow().  Differentiable in img: with grad enabled and img requiring grad the same forward runs inside an
    autograd Function whose backward is qpwc_upsample2x_image_bwd."""
    if _wants_grad(img):
        _refuse_capture("the image upsampling")
        _image_check("img", img, "upsample2x_image")
        return _UpsampleImageFn.apply(img, scale)
    _image_check("img", img, "upsample2x_image")
    x = img.contiguous()
    B, h, w, C = x.shape
    out = torch.empty((B, 2 * h, 2 * w, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("upsample2x_image", (B, h, w, C)):
        rc = _hip.lib().qpwc_upsample2x_image_fwd(x.data_ptr(), out.data_ptr(), B, h, w, C, float(scale), _stream(x))
    _hip.check(rc)
    return out


def avgpool_pyramid(x, levels):
    """`levels` successive AvgPool2D(2, 'same') (non_layers.py:171-180) of x (B,H,W,C) fp32 channels-last, of which
    only the last is returned, (B, ceil(H / 2^levels), ceil(W / 2^levels), C): how the interpolator brings its input
    frames to the coarsest level (pwcnet.py:87-90, 101-102).  One launch (qpwc_avgpool_pyramid_fwd) for 1..4 channels
    and H, W multiples of 2^levels; a shape the entry point refuses (QPWC_E_SHAPE) is pooled level by level by torch
    with the clipped 'same' windows.  No gradient: the frames are data."""
    _check_tensor("x", x)
    if x.dtype != torch.float32:
        raise ValueError("avgpool_pyramid has no fp16 storage path: x is {}".format(x.dtype))
    if _wants_grad(x):
        raise ValueError("avgpool_pyramid has no gradient: the frames it pools are data")
    levels = int(levels)
    if levels < 1 or x.numel() == 0:
        raise ValueError("avgpool_pyramid takes levels >= 1 and a non-empty x, got {} and {}".format(
            levels, tuple(x.shape)))
    x = x.contiguous()
    B, H, W, C = x.shape
    out = torch.empty((B, -(-H >> levels), -(-W >> levels), C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("avgpool_pyramid", (B, H, W, C, levels)):
        rc = _hip.lib().qpwc_avgpool_pyramid_fwd(x.data_ptr(), out.data_ptr(), B, H, W, C, levels, _stream(x))
    if rc == _hip.E_SHAPE:
        y = x.permute(0, 3, 1, 2)
        for _ in range(levels):
            y = torch.nn.functional.avg_pool2d(y, 2, stride=2, ceil_mode=True, count_include_pad=False)
        return y.permute(0, 2, 3, 1).contiguous()
    _hip.check(rc)
    return out


def _flow_dims(flow, data_format):
    get_axis(data_format)
    if flow.dim() != 4:
        raise ValueError("flow must be a batched rank-4 tensor, got rank {}".format(flow.dim()))
    if data_format == CHANNELS_LAST:
        B, H, W, C = flow.shape
        layout = _hip.NHWC
    else:
        B, C, H, W = flow.shape
        layout = _hip.NCHW
    if C != 2:
        raise ValueError("flow must have 2 channels, got {}".format(C))
    return B, H, W, layout


def invert_flow(flow, data_format=CHANNELS_LAST):
    """-tf_warp(flow, flow) (qpwcnet/core/occlusion.py:85; app/test/test_invert_flow.py:47)."""
    _check_tensor("flow", flow)
    B, H, W, layout = _flow_dims(flow, data_format)
    f = flow.contiguous()
    out = torch.empty_like(f)
    with torch.cuda.device(f.device), _timed("invert_flow", (B, H, W, 2)):
        rc = _hip.lib().qpwc_invert_flow_fwd(f.data_ptr(), out.data_ptr(), B, H, W, layout,
                                             _DTYPES[f.dtype], _stream(f))
    _hip.check(rc)
    return out


def occlusion_map(flow, data_format=CHANNELS_LAST):
    """estimate_occlusion_map (qpwcnet/core/occlusion.py:27-118) -> (B,H,W) float32."""
    _check_tensor("flow", flow)
    B, H, W, layout = _flow_dims(flow, data_format)
    f = flow.contiguous()
    out = torch.empty((B, H, W), dtype=torch.float32, device=f.device)
    with torch.cuda.device(f.device), _timed("occlusion", (B, H, W, 2)):
        rc = _hip.lib().qpwc_occlusion_fwd(f.data_ptr(), out.data_ptr(), B, H, W, layout,
                                           _DTYPES[f.dtype], _stream(f))
    _hip.check(rc)
    return out


def epe_multi(flows_true, flows_pred, out=None, data_format=CHANNELS_LAST):
    """Per-level EPE of up to 8 fp32 flow pairs ((B,h,w,2), or (B,2,h,w) for 'channels_first') in two
    launches (FlowMseLoss, qpwcnet/train/loss.py:56-67) -> float32 tensor [n_levels].
    ``out``: dense fp32 device vector [n_levels] to write into (e.g. the all-gather payload of
    qpwcnet_amd.dist.EpeGather, so that no copy stands between the reduction and the collective)."""
    import ctypes
    n = len(flows_true)
    if n != len(flows_pred) or not 1 <= n <= 8:
        raise ValueError("epe_multi takes 1..8 (true, pred) pairs")
    cf = data_format == CHANNELS_FIRST
    get_axis(data_format)
    keep, pa, pb, pdt, npix, plane = [], [], [], [], [], []
    for i, (a, b) in enumerate(zip(flows_true, flows_pred)):
        _check_tensor("y_true[%d]" % i, a)
        _check_tensor("y_pred[%d]" % i, b)
        if a.shape != b.shape or a.shape[1 if cf else 3] != 2:
            raise ValueError("level {}: shapes {} / {}".format(i, tuple(a.shape), tuple(b.shape)))
        a = a.float().contiguous()
        b = b.contiguous() if b.dtype == torch.float16 else b.float().contiguous()   # fp16 predictions as they are
        keep += [a, b]
        pa.append(a.data_ptr())
        pb.append(b.data_ptr())
        pdt.append(_DTYPES[b.dtype])
        npix.append(a.numel() // 2)
        plane.append(a.shape[2] * a.shape[3] if cf else 0)
    dev = keep[0].device
    L = _hip.lib()
    ws = torch.empty(L.qpwc_epe_multi_workspace_floats(), dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.numel() != n or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a dense fp32 vector of {} elements on {}".format(n, dev))
    with torch.cuda.device(dev):
        rc = L.qpwc_epe_multi_mixed_fwd((ctypes.c_void_p * n)(*pa), (ctypes.c_void_p * n)(*pb),
                                        (ctypes.c_int64 * n)(*npix), (ctypes.c_int64 * n)(*plane),
                                        (ctypes.c_int * n)(*pdt), n, out.data_ptr(), ws.data_ptr(), _stream(out))
    _hip.check(rc)
    return out


def augment_kernel(B, h, w, out_ims=None, out_flo=None):
    """Form of the first launch of ``qpwc_augment_fwd`` for a (h, w) output ('augment_pixel_kernel<vec4>' /
    'augment_pixel_kernel<scalar>'; host only).  Tensors or addresses for the outputs; None = 16-byte aligned, as
    torch allocates.  '' for arguments the entry point refuses."""
    ptr = lambda t: 1 << 20 if t is None else (t.data_ptr() if isinstance(t, torch.Tensor) else int(t))
    name = _hip.lib().qpwc_augment_fwd_kernel(int(B), int(h), int(w), ptr(out_ims), ptr(out_flo))
    return name.decode() if name else ""


def _augment_operands(what, ims, flo, iparams, fparams, out_shape):
    """The checks ``augment`` and ``augment_sparse`` share -> (B, H, W, h, w)."""
    for name, t, dt, c in (("ims", ims, (torch.uint8, torch.float32), 6), ("flo", flo, (torch.float32,), 2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if not t.is_cuda:
            raise RuntimeError("qpwcnet_amd: {} is on '{}'; ops.{} runs on a HIP device only (augment.* has the "
                               "CPU path)".format(name, t.device, what))
        if t.dtype not in dt:
            raise ValueError("{}: unsupported dtype {}".format(name, t.dtype))
        if t.dim() != 4 or t.shape[3] != c:
            raise ValueError("{} must be (B,H,W,{}) channels_last, got shape {}".format(name, c, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("{} must be dense (contiguous) channels_last".format(name))
    B, H, W, _ = ims.shape
    if tuple(flo.shape[:3]) != (B, H, W):
        raise ValueError("flo {} does not match ims {}".format(tuple(flo.shape), tuple(ims.shape)))
    for name, t, dt in (("iparams", iparams, torch.int32), ("fparams", fparams, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (B, 6) or not t.is_contiguous():
            raise ValueError("{} must be a dense ({}, 6) {} tensor".format(name, B, dt))
    if not (flo.device == ims.device == iparams.device == fparams.device):
        raise ValueError("ims, flo, iparams and fparams must be on one device")
    h, w = (int(v) for v in out_shape)
    if h <= 0 or w <= 0:
        raise ValueError("non-positive output shape {}".format((h, w)))
    return B, H, W, h, w


def _augment_outputs(L, B, h, w, colour, nhwc, dev):
    """out_ims, out_flo and the colour stage's workspace (None without it), fresh from torch's allocator."""
    out_ims = torch.empty((B, h, w, 6) if nhwc else (B, 6, h, w), dtype=torch.float32, device=dev)
    out_flo = torch.empty((B, h, w, 2) if nhwc else (B, 2, h, w), dtype=torch.float32, device=dev)
    ws = None
    if colour:
        nws = L.qpwc_augment_workspace_floats(B, h, w)
        _hip.check(min(int(nws), 0))
        ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
    return out_ims, out_flo, ws


def augment(ims, flo, iparams, fparams, out_shape, colour=True, finish=True, data_format=CHANNELS_LAST):
    """The training input pipeline of one batch (qpwc_augment_fwd; qpwcnet/data/augment.py:83-173, train.py:54-94):
    ims (B,H,W,6) uint8 (taken times 1/255) or float32, flo (B,H,W,2) float32, both dense channels-last on one HIP
    device; iparams (B,6) int32 = rh, rw, oy, ox, flip_ud, flip_lr and fparams (B,6) float32 = mu, mv, brightness,
    saturation, hue, contrast on the same device (include/qpwc.h) -> (ims, flo) fp32 of spatial size out_shape in
    data_format, written in that layout by the kernels.  colour=False: no colour stage; finish=False: no - 0.5 and no
    NaN scrub.  Enqueues and returns: no host synchronisation."""
    get_axis(data_format)
    B, H, W, h, w = _augment_operands("augment", ims, flo, iparams, fparams, out_shape)
    L = _hip.lib()
    dev = ims.device
    flags = (_hip.AUGMENT_COLOR if colour else 0) | (0 if finish else _hip.AUGMENT_RAW)
    nhwc = data_format == CHANNELS_LAST
    out_ims, out_flo, ws = _augment_outputs(L, B, h, w, colour, nhwc, dev)
    with torch.cuda.device(dev), _timed("augment", (B, H, W, h, w)):
        rc = L.qpwc_augment_fwd(ims.data_ptr(), _hip.U8 if ims.dtype == torch.uint8 else _hip.F32, flo.data_ptr(), B, H, W,
                                iparams.data_ptr(), fparams.data_ptr(), h, w, flags,
                                _hip.NHWC if nhwc else _hip.NCHW, out_ims.data_ptr(), out_flo.data_ptr(),
                                None if ws is None else ws.data_ptr(), _stream(ims))
    _hip.check(rc)
    return out_ims, out_flo


def augment_sparse_kernel(B, h, w):
    """Form of the first launch of ``qpwc_augment_sparse_fwd`` for a (h, w) output
    ('augment_sparse_pixel_kernel<vec4>' / 'augment_sparse_pixel_kernel<scalar>', by the shape alone; host only).  ''
    for shapes the entry point refuses."""
    name = _hip.lib().qpwc_augment_sparse_fwd_kernel(int(B), int(h), int(w))
    return name.decode() if name else ""


def augment_sparse(ims, flo, valid, iparams, fparams, out_shape, colour=True, finish=True, data_format=CHANNELS_LAST):
    """The training input pipeline for sparse ground truth (qpwc_augment_sparse_fwd, include/qpwc_sparse_augment.h;
    beyond the reference, whose pipeline is dense): the operands of ``augment`` and valid, None or a dense uint8
    (B,H,W) tensor on the same device -> (ims, flo, valid): ``augment``'s frames bit for bit, the flow resampled over
    its valid corners only (finite where the mask is 1, exactly 0 where it is 0) and the level-0 mask, uint8 (B,h,w)
    in both layouts.  The outputs are allocated here, on the grid the kernels' stores need.  Enqueues and returns: no
    host synchronisation."""
    get_axis(data_format)
    B, H, W, h, w = _augment_operands("augment_sparse", ims, flo, iparams, fparams, out_shape)
    dev = ims.device
    if valid is not None and not (isinstance(valid, torch.Tensor) and valid.dtype == torch.uint8
                                  and tuple(valid.shape) == (B, H, W) and valid.device == dev and valid.is_contiguous()):
        raise ValueError("valid must be None or a dense uint8 tensor of shape {} on {}".format((B, H, W), dev))
    L = _hip.lib()
    flags = (_hip.AUGMENT_COLOR if colour else 0) | (0 if finish else _hip.AUGMENT_RAW)
    nhwc = data_format == CHANNELS_LAST
    out_ims, out_flo, ws = _augment_outputs(L, B, h, w, colour, nhwc, dev)
    out_valid = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _timed("augment_sparse", (B, H, W, h, w)):
        rc = L.qpwc_augment_sparse_fwd(ims.data_ptr(), _hip.U8 if ims.dtype == torch.uint8 else _hip.F32, flo.data_ptr(),
                                       None if valid is None else valid.data_ptr(), B, H, W, iparams.data_ptr(),
                                       fparams.data_ptr(), h, w, flags, _hip.NHWC if nhwc else _hip.NCHW,
                                       out_ims.data_ptr(), out_flo.data_ptr(), out_valid.data_ptr(),
                                       None if ws is None else ws.data_ptr(), _stream(ims))
    _hip.check(rc)
    return out_ims, out_flo, out_valid


def augment_triplet_kernel(B, h, w, out_pair=None, out_mid=None):
    """Launch form of ``qpwc_augment_triplet_fwd`` for a (h, w) output ('triplet_pixel_kernel<vec4>' /
    'triplet_pixel_kernel<scalar>'; host only).  Tensors or addresses for the outputs; None = 16-byte aligned, as
    torch allocates.  '' for arguments the entry point refuses."""
    ptr = lambda t: 1 << 20 if t is None else (t.data_ptr() if isinstance(t, torch.Tensor) else int(t))
    name = _hip.lib().qpwc_augment_triplet_fwd_kernel(int(B), int(h), int(w), ptr(out_pair), ptr(out_mid))
    return name.decode() if name else ""


def augment_triplet(a, b, c, iparams, fparams, dsize, finish=True, data_format=CHANNELS_LAST):
    """The frame interpolator's input pipeline of one batch in one launch (qpwc_augment_triplet_fwd;
    qpwcnet/data/triplet_dataset_ops.py, app/frame_interpolation/pre_train.py:110-124): a, b, c (B,H,W,3) uint8 (taken
    times 1/255) or float32, the first, middle and last frames, dense channels-last on one HIP device; iparams (B,4)
    int32 = flip_ud, flip_lr, key0, key1 and fparams (B,16) float32 = R, scale, txn, sigma on the same device
    (include/qpwc_triplet.h) -> (img_pair, img1) fp32 of spatial size dsize with 6 and 3 channels in data_format,
    written in that layout by the kernel.  finish=False: no - 0.5.  Enqueues and returns: no host synchronisation."""
    get_axis(data_format)
    for name, t in (("a", a), ("b", b), ("c", c)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if not t.is_cuda:
            raise RuntimeError("qpwcnet_amd: {} is on '{}'; ops.augment_triplet runs on a HIP device only (augment.* "
                               "has the CPU path)".format(name, t.device))
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError("{}: unsupported dtype {}".format(name, t.dtype))
        if t.dim() != 4 or t.shape[3] != 3:
            raise ValueError("{} must be (B,H,W,3) channels_last, got shape {}".format(name, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("{} must be dense (contiguous) channels_last".format(name))
        if t.shape != a.shape or t.dtype != a.dtype:
            raise ValueError("{} {} {} does not match a {} {}".format(name, tuple(t.shape), t.dtype, tuple(a.shape),
                                                                     a.dtype))
    B, H, W, _ = a.shape
    for name, t, dt, n in (("iparams", iparams, torch.int32, 4), ("fparams", fparams, torch.float32, 16)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (B, n) or not t.is_contiguous():
            raise ValueError("{} must be a dense ({}, {}) {} tensor".format(name, B, n, dt))
    if not (a.device == b.device == c.device == iparams.device == fparams.device):
        raise ValueError("a, b, c, iparams and fparams must be on one device")
    h, w = (int(v) for v in dsize)
    if h <= 0 or w <= 0:
        raise ValueError("non-positive output shape {}".format((h, w)))
    dev = a.device
    nhwc = data_format == CHANNELS_LAST
    out_pair = torch.empty((B, h, w, 6) if nhwc else (B, 6, h, w), dtype=torch.float32, device=dev)
    out_mid = torch.empty((B, h, w, 3) if nhwc else (B, 3, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("augment_triplet", (B, H, W, h, w)):
        rc = _hip.lib().qpwc_augment_triplet_fwd(
            a.data_ptr(), b.data_ptr(), c.data_ptr(), _hip.U8 if a.dtype == torch.uint8 else _hip.F32, B, H, W,
            iparams.data_ptr(), fparams.data_ptr(), h, w, 0 if finish else _hip.TRIPLET_RAW,
            _hip.NHWC if nhwc else _hip.NCHW, out_pair.data_ptr(), out_mid.data_ptr(), _stream(a))
    _hip.check(rc)
    return out_pair, out_mid


def flow_to_image_kernel(B, sizes, out_dtype=torch.uint8, out_layout=CHANNELS_LAST, outs=None):
    """Store form of ``qpwc_flow_to_image_fwd`` for pictures of these (oh, ow) sizes ('flow_to_image_kernel<vec4>' /
    'flow_to_image_kernel<scalar>'; host only).  Tensors or addresses for the outputs; None = 16-byte aligned, as
    torch allocates.  '' for arguments the entry point refuses."""
    sizes = [tuple(int(v) for v in s) for s in sizes]
    n = len(sizes)
    ptr = lambda t: t.data_ptr() if isinstance(t, torch.Tensor) else int(t)
    ptrs = (ctypes.c_void_p * max(n, 1))(*([1 << 20] * n if outs is None else [ptr(t) for t in outs]))
    oh, ow = (ctypes.c_int * max(n, 1))(*[s[0] for s in sizes]), (ctypes.c_int * max(n, 1))(*[s[1] for s in sizes])
    name = _hip.lib().qpwc_flow_to_image_fwd_kernel(
        n, int(B), oh, ow, {torch.uint8: _hip.U8, torch.float32: _hip.F32}.get(out_dtype, -1),
        {CHANNELS_LAST: _hip.NHWC, CHANNELS_FIRST: _hip.NCHW}.get(out_layout, -1), ptrs)
    return name.decode() if name else ""


def flow_to_image(flows, sizes=None, in_layout=CHANNELS_LAST, out_dtype=torch.float32, out_layout=CHANNELS_LAST):
    """1..8 flows of one batch size and different spatial sizes -> their pictures, in two launches for all of them
    (qpwc_flow_to_image_fwd, include/qpwc_vis.h; qpwcnet/core/vis.py:37-76 and the nearest resize and uint8 conversion
    of app/train.py's ShowImageCallback).  flows[l] (B,h,w,2) / (B,2,h,w) by in_layout, fp32 or fp16, dense, on one HIP
    device; sizes[l] = (oh, ow) or None for the flow's own size (sizes=None: all of them); -> a list of (B,oh,ow,3) /
    (B,3,oh,ow) tensors by out_layout, float32 or uint8 by out_dtype, each coloured by its own per-image maximum.  The
    workspace comes from torch's allocator on the current stream.  Enqueues and returns: no host synchronisation."""
    get_axis(in_layout)
    get_axis(out_layout)
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError("out_dtype must be torch.float32 or torch.uint8, got {}".format(out_dtype))
    flows = list(flows)
    n = len(flows)
    if not 1 <= n <= 8:
        raise ValueError("flow_to_image takes 1..8 flows, got {}".format(n))
    sizes = [None] * n if sizes is None else list(sizes)
    if len(sizes) != n:
        raise ValueError("{} sizes for {} flows".format(len(sizes), n))
    nhwc_in, nhwc_out = in_layout == CHANNELS_LAST, out_layout == CHANNELS_LAST
    hs, ws_, ohs, ows = [], [], [], []
    for i, f in enumerate(flows):
        name = "flows[%d]" % i
        if not isinstance(f, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if not f.is_cuda:
            raise RuntimeError("qpwcnet_amd: {} is on '{}'; ops.flow_to_image runs on a HIP device only (vis.* has "
                               "the CPU path)".format(name, f.device))
        if f.dtype not in _DTYPES:
            raise ValueError("{}: unsupported dtype {}".format(name, f.dtype))
        if f.dim() != 4 or f.shape[3 if nhwc_in else 1] != 2:
            raise ValueError("{} must be {}, got shape {}".format(name, "(B,h,w,2)" if nhwc_in else "(B,2,h,w)",
                                                                  tuple(f.shape)))
        if f.device != flows[0].device or f.shape[0] != flows[0].shape[0]:
            raise ValueError("{}: every flow must be on one device and of one batch size".format(name))
        flows[i] = f = f.contiguous()
        h, w = (f.shape[1], f.shape[2]) if nhwc_in else (f.shape[2], f.shape[3])
        oh, ow = (h, w) if sizes[i] is None else (int(v) for v in sizes[i])
        if min(h, w, oh, ow) <= 0:
            raise ValueError("{}: non-positive extent {}x{} -> {}x{}".format(name, h, w, oh, ow))
        hs.append(int(h)), ws_.append(int(w)), ohs.append(oh), ows.append(ow)
    B, dev = int(flows[0].shape[0]), flows[0].device
    if B <= 0:
        raise ValueError("empty batch")
    L = _hip.lib()
    arr = lambda v: (ctypes.c_int * n)(*v)
    ha, wa, oha, owa = arr(hs), arr(ws_), arr(ohs), arr(ows)
    nws = L.qpwc_flow_to_image_workspace_floats(n, B, ha, wa)
    _hip.check(min(int(nws), 0))
    with torch.cuda.device(dev):
        ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
        outs = [torch.empty((B, oh, ow, 3) if nhwc_out else (B, 3, oh, ow), dtype=out_dtype, device=dev)
                for oh, ow in zip(ohs, ows)]
        with _timed("flow_to_image", (n, B, ohs[0], ows[0])):
            rc = L.qpwc_flow_to_image_fwd(
                (ctypes.c_void_p * n)(*[f.data_ptr() for f in flows]), arr([_DTYPES[f.dtype] for f in flows]), ha, wa, n,
                B, _hip.NHWC if nhwc_in else _hip.NCHW, (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]), oha, owa,
                _hip.U8 if out_dtype == torch.uint8 else _hip.F32, _hip.NHWC if nhwc_out else _hip.NCHW,
                ws.data_ptr(), _stream(flows[0]))
    _hip.check(rc)
    return outs


def review_panels_kernel(n_flows, B, H, W, h=None, w=None, out_dtype=torch.float32, out_layout=CHANNELS_LAST):
    """Store form of the panel launch of ``qpwc_inference_panels_fwd`` (n_flows = 2) / ``qpwc_interpolation_panels_fwd``
    (n_flows = 1, flow of h x w) for these shapes: 'review_panels_kernel<vec4>' / 'review_panels_kernel<scalar>' (host
    only).  '' for arguments the entry points refuse."""
    h, w = H if h is None else h, W if w is None else w
    name = _hip.lib().qpwc_review_panels_fwd_kernel(
        int(n_flows), int(B), int(H), int(W), int(h), int(w),
        {torch.uint8: _hip.U8, torch.float32: _hip.F32}.get(out_dtype, -1),
        {CHANNELS_LAST: _hip.NHWC, CHANNELS_FIRST: _hip.NCHW}.get(out_layout, -1))
    return name.decode() if name else ""


def _review_image(name, t, C, nhwc, like=None):
    """A dense (B,H,W,C) / (B,C,H,W) image of the review panels -> (tensor, (B, H, W))."""
    _check_tensor(name, t)
    if t.shape[3 if nhwc else 1] != C:
        raise ValueError("{} must be {}, got shape {}".format(name, "(B,H,W,%d)" % C if nhwc else "(B,%d,H,W)" % C,
                                                              tuple(t.shape)))
    if like is not None and (t.device != like.device or t.dtype != like.dtype):
        raise ValueError("{} must have {}'s device and dtype".format(name, "the first image"))
    B, H, W = (t.shape[0], t.shape[1], t.shape[2]) if nhwc else (t.shape[0], t.shape[2], t.shape[3])
    return t.contiguous(), (int(B), int(H), int(W))


def _review_flow(name, t, nhwc, like):
    t, dims = _review_image(name, t, 2, nhwc)
    if t.dtype != torch.float32:
        raise ValueError("{} must be float32 (vis.* widens fp16 flows), got {}".format(name, t.dtype))
    if t.device != like.device:
        raise ValueError("{} must be on the images' device".format(name))
    return t, dims


def _review_call(entry, n_flows, n_out, flow_pic, B, H, W, h, w, out_dtype, nhwc_out, grid, like, call):
    """Allocates the pictures and the workspace of one review-panel call and runs `call(outs_array, ws_ptr)`."""
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError("out_dtype must be torch.float32 or torch.uint8, got {}".format(out_dtype))
    if int(grid) < 0:
        raise ValueError("grid must be 0 (off) or a positive period, got {}".format(grid))
    if min(B, H, W, h, w) <= 0:
        raise ValueError("empty tensor: B={} H={} W={} h={} w={}".format(B, H, W, h, w))
    L = _hip.lib()
    nws = L.qpwc_review_workspace_floats(n_flows, B, h, w)
    _hip.check(min(int(nws), 0))
    dev = like.device
    with torch.cuda.device(dev):
        ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
        size = lambda i: (h, w) if i == flow_pic else (H, W)
        outs = [torch.empty((B,) + size(i) + (3,) if nhwc_out else (B, 3) + size(i), dtype=out_dtype, device=dev)
                for i in range(n_out)]
        with _timed(entry, (B, H, W, n_out)):
            rc = call(L, (ctypes.c_void_p * n_out)(*[o.data_ptr() for o in outs]), ws.data_ptr())
    _hip.check(rc)
    return outs


def inference_panels(ims, flo, flo_pred, in_layout=CHANNELS_LAST, out_dtype=torch.float32, out_layout=CHANNELS_LAST,
                     grid=0):
    """The ten pictures of qpwcnet/app/optical_flow/test_infer.py:104-154 in two launches (qpwc_inference_panels_fwd,
    include/qpwc_review.h).  ims (B,H,W,6) / (B,6,H,W) by in_layout, fp32 or fp16, preprocessed; flo, flo_pred
    (B,H,W,2) / (B,2,H,W) float32; all dense on one HIP device.  -> a list of ten (B,H,W,3) / (B,3,H,W) tensors by
    out_layout, float32 or uint8 by out_dtype, in the header's order.  The workspace comes from torch's allocator on the
    current stream.  Enqueues and returns: no host synchronisation."""
    nhwc, nhwc_out = get_axis(in_layout) == 3, get_axis(out_layout) == 3
    ims, (B, H, W) = _review_image("ims", ims, 6, nhwc)
    flo, d0 = _review_flow("flo", flo, nhwc, ims)
    flo_pred, d1 = _review_flow("flo_pred", flo_pred, nhwc, ims)
    if d0 != (B, H, W) or d1 != (B, H, W):
        raise ValueError("flo {} and flo_pred {} must have ims' batch and size {}".format(d0, d1, (B, H, W)))
    return _review_call(
        "inference_panels", 2, 10, -1, B, H, W, H, W, out_dtype, nhwc_out, grid, ims,
        lambda L, outs, ws: L.qpwc_inference_panels_fwd(
            ims.data_ptr(), _DTYPES[ims.dtype], flo.data_ptr(), flo_pred.data_ptr(), B, H, W,
            _hip.NHWC if nhwc else _hip.NCHW, outs, _hip.U8 if out_dtype == torch.uint8 else _hip.F32,
            _hip.NHWC if nhwc_out else _hip.NCHW, int(grid), ws, _stream(ims)))


def interpolation_panels(img_pair, img1, pred, flow, in_layout=CHANNELS_LAST, out_dtype=torch.float32,
                         out_layout=CHANNELS_LAST, grid=32):
    """The seven pictures of qpwcnet/app/frame_interpolation/pre_train_test.py:45-79, 121-163 in two launches
    (qpwc_interpolation_panels_fwd, include/qpwc_review.h).  img_pair (B,H,W,6) / (B,6,H,W), img1 and pred (B,H,W,3) /
    (B,3,H,W) of one dtype, fp32 or fp16; flow (B,h,w,2) / (B,2,h,w) float32 with H = s * h, W = s * w; all dense on one
    HIP device.  -> a list of seven tensors in the header's order, all (B,H,W,3) / (B,3,H,W) but '5-flow', which has the
    flow's size.  The workspace comes from torch's allocator on the current stream.  Enqueues and returns."""
    nhwc, nhwc_out = get_axis(in_layout) == 3, get_axis(out_layout) == 3
    img_pair, (B, H, W) = _review_image("img_pair", img_pair, 6, nhwc)
    img1, d1 = _review_image("img1", img1, 3, nhwc, img_pair)
    pred, d2 = _review_image("pred", pred, 3, nhwc, img_pair)
    flow, (Bf, h, w) = _review_flow("flow", flow, nhwc, img_pair)
    if d1 != (B, H, W) or d2 != (B, H, W) or Bf != B:
        raise ValueError("img1 {}, pred {} and flow's batch {} must match img_pair's {}".format(d1, d2, Bf, (B, H, W)))
    s = H // h if h > 0 else 0
    if s < 1 or H != s * h or W != s * w:
        raise ValueError("the images' {}x{} must be one whole multiple of the flow's {}x{}".format(H, W, h, w))
    return _review_call(
        "interpolation_panels", 1, 7, 5, B, H, W, h, w, out_dtype, nhwc_out, grid, img_pair,
        lambda L, outs, ws: L.qpwc_interpolation_panels_fwd(
            img_pair.data_ptr(), img1.data_ptr(), pred.data_ptr(), _DTYPES[img_pair.dtype], flow.data_ptr(), B, H, W,
            h, w, _hip.NHWC if nhwc else _hip.NCHW, outs, _hip.U8 if out_dtype == torch.uint8 else _hip.F32,
            _hip.NHWC if nhwc_out else _hip.NCHW, int(grid), ws, _stream(img_pair)))


def image_quality_kernel(B, H, W, C):
    """Form of ``qpwc_image_quality_fwd``'s tile kernel for this shape ('quality_tile_kernel': it has one; host only).
    '' for arguments the entry point refuses."""
    name = _hip.lib().qpwc_image_quality_fwd_kernel(int(B), int(H), int(W), int(C))
    return name.decode() if name else ""


def image_quality(truth, pred, data_format=CHANNELS_LAST, offsets=(0.0, 0.0), flags=0, max_val=1.0, state=None):
    """Per-image MSE, PSNR and SSIM (tf.image.ssim's defaults) of ``pred`` against ``truth`` in two launches
    (qpwc_image_quality_fwd, include/qpwc_quality.h).  truth, pred: (B,H,W,C) / (B,C,H,W) by data_format, one shape, each
    fp32 or fp16, on one HIP device, H, W >= 11, C in 1..4; offsets = (truth, pred), added before ``flags``
    (_hip.QUALITY_CLIP, _hip.QUALITY_U8) apply; state: None or a float64 tensor of 4 elements on the same device, to
    which the call adds its sums of mse, psnr, ssim and its image count.  -> (mse, psnr, ssim), three float32 [B] views
    of one tensor.  The workspace comes from torch's allocator on the current stream.  Enqueues and returns: no host
    synchronisation."""
    get_axis(data_format)
    nhwc = data_format == CHANNELS_LAST
    for name, t in (("truth", truth), ("pred", pred)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if not t.is_cuda:
            raise RuntimeError("qpwcnet_amd: {} is on '{}'; ops.image_quality runs on a HIP device only (metrics.* has "
                               "the CPU path)".format(name, t.device))
        if t.dtype not in _DTYPES:
            raise ValueError("{}: unsupported dtype {}".format(name, t.dtype))
        if t.dim() != 4:
            raise ValueError("{} must be rank 4 (batched), got shape {}".format(name, tuple(t.shape)))
    if truth.shape != pred.shape or truth.device != pred.device:
        raise ValueError("truth {} on {} and pred {} on {} must have one shape and one device".format(
            tuple(truth.shape), truth.device, tuple(pred.shape), pred.device))
    B, H, W, C = (int(v) for v in (truth.shape if nhwc else (truth.shape[0],) + tuple(truth.shape[2:]) + (truth.shape[1],)))
    if H < 11 or W < 11:
        raise ValueError("image_quality: H={} W={} must both be at least 11, the SSIM filter size".format(H, W))
    dev = truth.device
    if state is not None:
        if not (isinstance(state, torch.Tensor) and state.dtype == torch.float64 and state.numel() == 4
                and state.is_contiguous() and state.device == dev):
            raise ValueError("state must be a contiguous float64 tensor of 4 elements on {}".format(dev))
    truth, pred = truth.contiguous(), pred.contiguous()
    off_t, off_p = (float(v) for v in offsets)
    L = _hip.lib()
    nws = L.qpwc_image_quality_workspace_floats(B, H, W, C)
    _hip.check(min(int(nws), 0))
    with torch.cuda.device(dev):
        ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
        out = torch.empty((3, B), dtype=torch.float32, device=dev)
        with _timed("image_quality", (B, H, W, C)):
            rc = L.qpwc_image_quality_fwd(
                truth.data_ptr(), _DTYPES[truth.dtype], pred.data_ptr(), _DTYPES[pred.dtype], B, H, W, C,
                _hip.NHWC if nhwc else _hip.NCHW, off_t, off_p, int(flags), float(max_val), out.data_ptr(),
                None if state is None else state.data_ptr(), ws.data_ptr(), _stream(truth))
    _hip.check(rc)
    return out[0], out[1], out[2]


def flow_quality_kernel(B, H, W):
    """Form of ``qpwc_flow_quality_fwd``'s tile kernel for this shape ('flow_quality_tile_kernel': it has one; host
    only).  '' for arguments the entry point refuses."""
    name = _hip.lib().qpwc_flow_quality_fwd_kernel(int(B), int(H), int(W))
    return name.decode() if name else ""


def _dense_on_grid(t, align):
    """t dense, with its first byte on a multiple of `align`: a fresh copy where it is not (a slice of a larger tensor)."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % align else t


def flow_quality(truth, pred, valid=None, occluded=None, data_format=CHANNELS_LAST, outlier=(3.0, 0.05),
                 accuracy=(1.0, 3.0, 5.0), speed=(10.0, 40.0), state=None):
    """Per-image flow metrics of ``pred`` against ``truth`` over the valid pixels in two launches (qpwc_flow_quality_fwd,
    include/qpwc_flow_quality.h).  truth (float32), pred (float32 or float16): (B,H,W,2) / (B,2,H,W) by data_format, one
    shape, on one HIP device; valid, occluded: None or uint8 (B,H,W) on that device; outlier = (pixels, share of the
    ground-truth speed), accuracy = three rising thresholds, speed = the two bin edges; state: None or a float64 tensor
    of 17 elements on the same device, to which the call adds its 15 sums, its images and its pixels.  -> twelve float32
    [B] views of one tensor, in the header's order.  An operand that is not dense, or whose first byte is off the grid its
    loads need, is copied first.  The workspace comes from torch's allocator on the current stream.  Enqueues and
    returns: no host synchronisation."""
    get_axis(data_format)
    nhwc = data_format == CHANNELS_LAST
    for name, t in (("truth", truth), ("pred", pred)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if not t.is_cuda:
            raise RuntimeError("qpwcnet_amd: {} is on '{}'; ops.flow_quality runs on a HIP device only (metrics.* has "
                               "the CPU path)".format(name, t.device))
        if t.dim() != 4:
            raise ValueError("{} must be rank 4 (batched), got shape {}".format(name, tuple(t.shape)))
    if truth.dtype != torch.float32:
        raise ValueError("truth must be float32, got {}".format(truth.dtype))
    if pred.dtype not in _DTYPES:
        raise ValueError("pred: unsupported dtype {}".format(pred.dtype))
    if truth.shape != pred.shape or truth.device != pred.device:
        raise ValueError("truth {} on {} and pred {} on {} must have one shape and one device".format(
            tuple(truth.shape), truth.device, tuple(pred.shape), pred.device))
    B, H, W, C = (int(v) for v in (truth.shape if nhwc else (truth.shape[0],) + tuple(truth.shape[2:]) + (truth.shape[1],)))
    if C != 2:
        raise ValueError("flows have 2 channels, got {} ({}, shape {})".format(C, data_format, tuple(truth.shape)))
    if min(B, H, W) < 1:
        raise ValueError("empty tensor: B={} H={} W={}".format(B, H, W))
    dev = truth.device
    for name, m in (("valid", valid), ("occluded", occluded)):
        if m is not None and not (isinstance(m, torch.Tensor) and m.dtype == torch.uint8 and tuple(m.shape) == (B, H, W)
                                  and m.device == dev):
            raise ValueError("{} must be a uint8 tensor of shape {} on {}".format(name, (B, H, W), dev))
    if state is not None:
        if not (isinstance(state, torch.Tensor) and state.dtype == torch.float64 and state.numel() == 17
                and state.is_contiguous() and state.device == dev):
            raise ValueError("state must be a contiguous float64 tensor of 17 elements on {}".format(dev))
    if len(outlier) != 2 or len(accuracy) != 3 or len(speed) != 2:
        raise ValueError("outlier takes 2 values, accuracy 3 and speed 2")
    params = [float(v) for v in tuple(outlier) + tuple(accuracy) + tuple(speed)]
    truth = _dense_on_grid(truth, 8 if nhwc else 4)
    pred = _dense_on_grid(pred, (2 if nhwc else 1) * pred.element_size())
    valid = None if valid is None else valid.contiguous()
    occluded = None if occluded is None else occluded.contiguous()
    L = _hip.lib()
    nws = L.qpwc_flow_quality_workspace_floats(B, H, W)
    _hip.check(min(int(nws), 0))
    with torch.cuda.device(dev):
        ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
        out = torch.empty((12, B), dtype=torch.float32, device=dev)
        with _timed("flow_quality", (B, H, W, 2)):
            rc = L.qpwc_flow_quality_fwd(
                truth.data_ptr(), pred.data_ptr(), _DTYPES[pred.dtype],
                None if valid is None else valid.data_ptr(), None if occluded is None else occluded.data_ptr(),
                B, H, W, _hip.NHWC if nhwc else _hip.NCHW, *params, out.data_ptr(),
                None if state is None else state.data_ptr(), ws.data_ptr(), _stream(truth))
    _hip.check(rc)
    return tuple(out[i] for i in range(12))


def _loss_layout(y_true, preds, data_format):
    """-> (y_true, preds, layout code, nhwc_view): 'channels_first' operands that are all physically NHWC (torch
    channels_last memory) are read through their permuted views; everything else dense in its declared layout."""
    get_axis(data_format)
    ts = [y_true] + [p for p in preds if p is not None]
    if data_format == CHANNELS_FIRST and all(
            t.shape[1] > 1 and t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous() for t in ts):
        return (y_true.permute(0, 2, 3, 1), [None if p is None else p.permute(0, 2, 3, 1) for p in preds], _hip.NHWC,
                True)
    return (y_true.contiguous(), [None if p is None else p.contiguous() for p in preds],
            _hip.NHWC if data_format == CHANNELS_LAST else _hip.NCHW, False)


class _LossOperands:
    """What both loss forwards make of their operands: y_true and the predictions checked and in the layout the kernels
    read (gt, preds, layout, nhwc), the extents B, H, W, C, n and hs, ws_, the ctypes arrays ha, wa, pp, pdt, and the
    helpers buffers() (one fp32 tensor per level, shaped like its prediction), ptrs() and back() (the caller's view of
    such buffers).  y_preds=None with shapes=[(h, w), ...]: no predictions.  check(self): the caller's own operand check,
    run once B, H, W, C and dev are known and before the levels' shapes are looked at."""

    def __init__(self, y_true, y_preds, data_format, shapes, check=None):
        if not isinstance(y_true, torch.Tensor):
            raise TypeError("y_true must be a torch.Tensor")
        if _wants_grad(y_true):
            raise ValueError("y_true requires grad: the losses are differentiable in y_pred only, a gradient for y_true "
                             "would be dropped (detach it)")
        _check_tensor("y_true", y_true)
        if y_true.dtype != torch.float32:
            raise ValueError("y_true must be float32, got {}".format(y_true.dtype))
        preds = [None] * len(shapes) if y_preds is None else list(y_preds)
        self.n = n = len(preds)
        if not 1 <= n <= 8:
            raise ValueError("the losses take 1..8 prediction levels, got {}".format(n))
        for i, p in enumerate(preds):
            if p is not None:
                _check_tensor("y_pred[%d]" % i, p)
                if p.device != y_true.device:
                    raise ValueError("y_pred[{}] is on {}, y_true on {}".format(i, p.device, y_true.device))
        self.gt, self.preds, self.layout, self.view = _loss_layout(y_true, preds, data_format)
        self.nhwc = nhwc = self.layout == _hip.NHWC
        unpack = lambda t: t.shape if nhwc else (t.shape[0], t.shape[2], t.shape[3], t.shape[1])
        self.B, self.H, self.W, self.C = B, H, W, C = unpack(self.gt)
        self.dev = self.gt.device
        if check is not None:
            check(self)
        self.hs, self.ws_ = [], []
        for i, p in enumerate(self.preds):
            if p is None:
                pb, pc, (h, w) = B, C, shapes[i]
            else:
                pb, h, w, pc = unpack(p)
            if pb != B or pc != C:
                raise ValueError("level {}: prediction of batch {} / {} channels against a ground truth of {} / {}".format(
                    i, pb, pc, B, C))
            self.hs.append(int(h))
            self.ws_.append(int(w))
        self.ha, self.wa = (ctypes.c_int * n)(*self.hs), (ctypes.c_int * n)(*self.ws_)
        self.pp = (ctypes.c_void_p * n)(*[0 if p is None else p.data_ptr() for p in self.preds])
        self.pdt = (ctypes.c_int * n)(*[_hip.F32 if p is None else _DTYPES[p.dtype] for p in self.preds])

    def buffers(self):
        B, C = self.B, self.C
        return [torch.empty((B, h, w, C) if self.nhwc else (B, C, h, w), dtype=torch.float32, device=self.dev)
                for h, w in zip(self.hs, self.ws_)]

    def ptrs(self, ts):
        return None if ts is None else (ctypes.c_void_p * self.n)(*[t.data_ptr() for t in ts])

    def back(self, ts):
        if not ts:
            return None
        return [t.permute(0, 3, 1, 2) for t in ts] if self.view else ts


def loss_fwd(kind, y_true, y_preds, data_format=CHANNELS_LAST, p0=0.0, p1=0.0, want_dpred=False, want_gt=False,
             shapes=None):
    """Per-level training loss of 1..8 predictions against one full-resolution ground truth (qpwc_loss_fwd; kind
    _hip.LOSS_*; qpwcnet/train/loss.py) -> (losses: fp32 [L] on the device, dpred, gt).
    dpred (want_dpred): fp32 d losses[l] / d y_preds[l], shaped like each prediction; gt (want_gt): each level's
    resampled, flow-scaled ground truth.  y_preds=None with shapes=[(h, w), ...]: the ground truth only (want_gt).
    Enqueues and returns: no host synchronisation."""
    o = _LossOperands(y_true, y_preds, data_format, shapes)
    B, H, W, C, n, dev = o.B, o.H, o.W, o.C, o.n, o.dev
    L = _hip.lib()
    nws = L.qpwc_loss_workspace_floats(int(kind), B, H, W, C, o.ha, o.wa, n)
    _hip.check(min(int(nws), 0))
    ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    dbuf = o.buffers() if want_dpred else None
    gbuf = o.buffers() if want_gt else None
    with torch.cuda.device(dev), _timed("loss", (B, H, W, C)):
        rc = L.qpwc_loss_fwd(int(kind), float(p0), float(p1), o.gt.data_ptr(), B, H, W, C, o.layout, o.pp, o.ha, o.wa,
                             o.pdt, n, out.data_ptr(), o.ptrs(dbuf), o.ptrs(gbuf), ws.data_ptr(), _stream(o.gt))
    _hip.check(rc)
    return out, o.back(dbuf), o.back(gbuf)


def _loss_grads(dpreds, grad_losses, dtypes):
    """-> (g: grad_losses as a dense fp32 device vector, grads: one empty tensor per level in dtypes[l], the ctypes
    arguments of both backward entry points after grad_losses: grad_pred, n_elems, pred_dtype, n)."""
    n = len(dpreds)
    g = grad_losses.to(torch.float32).contiguous()
    if g.numel() != n or not g.is_cuda:
        raise ValueError("grad_losses must be a device vector of {} elements".format(n))
    grads = [torch.empty_like(d, dtype=dt) for d, dt in zip(dpreds, dtypes)]   # same strides: same memory order
    return g, grads, ((ctypes.c_void_p * n)(*[d.data_ptr() for d in dpreds]),
                      (ctypes.c_void_p * n)(*[t.data_ptr() for t in grads]),
                      (ctypes.c_int64 * n)(*[d.numel() for d in dpreds]),
                      (ctypes.c_int * n)(*[_DTYPES[dt] for dt in dtypes]), n)


def loss_bwd(dpreds, grad_losses, dtypes):
    """grad_pred[l] = grad_losses[l] * dpreds[l] in dtypes[l], all levels in one launch (qpwc_loss_bwd); dpreds from
    loss_fwd(want_dpred=True), grad_losses [L] on the device."""
    g, grads, (dp, gp, ne, dt, n) = _loss_grads(dpreds, grad_losses, dtypes)
    with torch.cuda.device(g.device), _timed("loss_bwd", (n,)):
        rc = _hip.lib().qpwc_loss_bwd(dp, g.data_ptr(), gp, ne, dt, n, _stream(g))
    _hip.check(rc)
    return grads


class _LossFn(torch.autograd.Function):
    """loss_fwd() with qpwc_loss_bwd as its gradient: the forward also stores d losses[l] / d y_pred[l] (fp32), the
    backward scales it by the incoming per-level gradient (cheaper than recomputing it, which reads y_true again)."""

    @staticmethod
    def forward(ctx, cfg, y_true, *y_preds):
        kind, data_format, p0, p1 = cfg
        losses, dpred, _ = loss_fwd(kind, y_true, y_preds, data_format, p0, p1, want_dpred=True)
        ctx.dpred = dpred
        ctx.dtypes = [p.dtype for p in y_preds]
        return losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_losses):
        _refuse_capture("the loss backward")
        grads = loss_bwd(ctx.dpred, grad_losses, ctx.dtypes)
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


def loss(kind, y_true, y_preds, data_format=CHANNELS_LAST, p0=0.0, p1=0.0):
    """Per-level losses (fp32 [L]) of loss_fwd(); differentiable in y_preds when grad is enabled and one of them
    requires it."""
    if isinstance(y_true, torch.Tensor) and _wants_grad(y_true):
        raise ValueError("y_true requires grad: the losses are differentiable in y_pred only, a gradient for y_true "
                         "would be dropped (detach it)")
    if _wants_grad(*y_preds):
        _refuse_capture("the loss")
        return _LossFn.apply((int(kind), data_format, float(p0), float(p1)), y_true, *y_preds)
    return loss_fwd(kind, y_true, y_preds, data_format, p0, p1)[0]


def area_ground_truth(flow_gt, shapes, data_format=CHANNELS_LAST):
    """FlowMseLossV2's per-level ground truth (qpwcnet/train/loss.py:160-173): the mean over sh x sw blocks times h / H
    on both channels -> list of fp32 tensors in data_format; up to 8 levels per pass over flow_gt (qpwc_loss_fwd with
    gt_out only)."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    out = []
    for k in range(0, len(shapes), 8):
        out += loss_fwd(_hip.LOSS_FLOW_MSE_V2, flow_gt, None, data_format, 0.1, want_gt=True, shapes=shapes[k:k + 8])[2]
    return out


def masked_loss_kernel(kind, B, H, W, shapes):
    """The forward kernel ``qpwc_masked_loss_fwd`` takes for these levels ('masked_loss_tile_kernel' /
    'masked_loss_pixel_kernel'; host only).  '' for arguments the entry point refuses."""
    n = len(shapes)
    ha, wa = (ctypes.c_int * n)(*[int(h) for h, _ in shapes]), (ctypes.c_int * n)(*[int(w) for _, w in shapes])
    name = _hip.lib().qpwc_masked_loss_fwd_kernel(int(kind), int(B), int(H), int(W), 2, ha, wa, n)
    return name.decode() if name else ""


def masked_loss_fwd(kind, y_true, y_preds, valid=None, data_format=CHANNELS_LAST, p0=0.0, p1=0.0, want_dpred=False,
                    want_gt=False, want_valid=False, shapes=None):
    """Per-level flow loss over the valid pixels of 1..8 predictions against one full-resolution ground truth
    (qpwc_masked_loss_fwd, include/qpwc_masked_loss.h; kind one of the three _hip.LOSS_FLOW_*) -> (losses: fp32 [L],
    counts: int64 [L] valid level pixels, dpred, gt, valid_out), all on the device.  valid: None or uint8 (B,H,W) on
    y_true's device.  dpred (want_dpred): fp32 d term / d y_preds[l], not yet divided by the count (masked_loss_bwd does
    it); gt (want_gt): each level's ground truth, 0 where it has none; valid_out (want_valid): uint8 (B,h,w).
    y_preds=None with shapes=[(h, w), ...]: the ground truth and validity only.  A y_true whose first byte is off the
    16-byte grid, or a mask off the 4-byte grid (a view into a larger tensor), is copied first.  Enqueues and returns: no
    host synchronisation."""
    def check_valid(o):
        if valid is not None and not (isinstance(valid, torch.Tensor) and valid.dtype == torch.uint8
                                      and tuple(valid.shape) == (o.B, o.H, o.W) and valid.device == o.dev):
            raise ValueError("valid must be a uint8 tensor of shape {} on {}".format((o.B, o.H, o.W), o.dev))

    o = _LossOperands(y_true, y_preds, data_format, shapes, check_valid)
    B, H, W, C, n, dev = o.B, o.H, o.W, o.C, o.n, o.dev
    L = _hip.lib()
    nws = L.qpwc_masked_loss_workspace_floats(int(kind), B, H, W, C, o.ha, o.wa, n)
    _hip.check(min(int(nws), 0))
    gt = _dense_on_grid(o.gt, 16)
    valid = None if valid is None else _dense_on_grid(valid, 4)
    with torch.cuda.device(dev):
        ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        dbuf = o.buffers() if want_dpred else None
        gbuf = o.buffers() if want_gt else None
        vbuf = [torch.empty((B, h, w), dtype=torch.uint8, device=dev) for h, w in zip(o.hs, o.ws_)] if want_valid else None
        with _timed("masked_loss", (B, H, W, C)):
            rc = L.qpwc_masked_loss_fwd(int(kind), float(p0), float(p1), gt.data_ptr(),
                                        None if valid is None else valid.data_ptr(), B, H, W, C, o.layout, o.pp, o.ha,
                                        o.wa, o.pdt, n, out.data_ptr(), counts.data_ptr(), o.ptrs(dbuf), o.ptrs(gbuf),
                                        o.ptrs(vbuf), ws.data_ptr(), _stream(gt))
    _hip.check(rc)
    return out, counts, o.back(dbuf), o.back(gbuf), vbuf


def masked_loss_bwd(kind, dpreds, counts, grad_losses, dtypes):
    """grad_pred[l] = grad_losses[l] * dpreds[l] / max(counts[l], 1) (the Huber kind: over twice that) in dtypes[l], all
    levels in one launch (qpwc_masked_loss_bwd); dpreds and counts from masked_loss_fwd(want_dpred=True) with the same
    kind, grad_losses [L] on the device.  The counts stay on the device."""
    g, grads, (dp, gp, ne, dt, n) = _loss_grads(dpreds, grad_losses, dtypes)
    with torch.cuda.device(g.device), _timed("masked_loss_bwd", (n,)):
        rc = _hip.lib().qpwc_masked_loss_bwd(int(kind), dp, counts.data_ptr(), g.data_ptr(), gp, ne, dt, n, _stream(g))
    _hip.check(rc)
    return grads


class _MaskedLossFn(torch.autograd.Function):
    """masked_loss_fwd() with qpwc_masked_loss_bwd as its gradient, as _LossFn: the forward stores d term / d y_pred, the
    backward scales it by the incoming per-level gradient over the level's count, which never leaves the device."""

    @staticmethod
    def forward(ctx, cfg, y_true, valid, *y_preds):
        kind, data_format, p0, p1 = cfg
        losses, counts, dpred, _, _ = masked_loss_fwd(kind, y_true, y_preds, valid, data_format, p0, p1, want_dpred=True)
        ctx.kind, ctx.dpred, ctx.counts = kind, dpred, counts
        ctx.dtypes = [p.dtype for p in y_preds]
        ctx.mark_non_differentiable(counts)
        ctx.set_materialize_grads(False)       # no zeros tensor (a fill launch) for the counts' gradient
        return losses, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_losses, _grad_counts):
        _refuse_capture("the masked loss backward")
        if grad_losses is None:
            return (None,) * (3 + len(ctx.dtypes))
        grads = masked_loss_bwd(ctx.kind, ctx.dpred, ctx.counts, grad_losses, ctx.dtypes)
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))


def masked_loss(kind, y_true, y_preds, valid=None, data_format=CHANNELS_LAST, p0=0.0, p1=0.0):
    """(losses fp32 [L], counts int64 [L]) of masked_loss_fwd(); the losses are differentiable in y_preds when grad is
    enabled and one of them requires it."""
    if isinstance(y_true, torch.Tensor) and _wants_grad(y_true):
        raise ValueError("y_true requires grad: the losses are differentiable in y_pred only, a gradient for y_true "
                         "would be dropped (detach it)")
    if _wants_grad(*y_preds):
        _refuse_capture("the masked loss")
        return _MaskedLossFn.apply((int(kind), data_format, float(p0), float(p1)), y_true, valid, *y_preds)
    return masked_loss_fwd(kind, y_true, y_preds, valid, data_format, p0, p1)[:2]


class _UnsupOperands:
    """What both label-free loss entry points make of their operands: per level the fp32 channels-last frames, the flow
    dense in `data_format` (fp32 or fp16) and the optional uint8 occlusion mask, all checked against one another; B, the
    level shapes and the ctypes arrays."""

    def __init__(self, prvs, nxts, flows, occluded, data_format):
        get_axis(data_format)
        prvs, nxts, flows = list(prvs), list(nxts), list(flows)
        self.n = n = len(flows)
        if not 1 <= n <= 8:
            raise ValueError("the losses take 1..8 levels, got {}".format(n))
        occluded = [None] * n if occluded is None else list(occluded)
        if not len(prvs) == len(nxts) == len(occluded) == n:
            raise ValueError("{} flows against {} / {} frames and {} masks".format(n, len(prvs), len(nxts), len(occluded)))
        self.nhwc = nhwc = data_format == CHANNELS_LAST
        self.layout = _hip.NHWC if nhwc else _hip.NCHW
        self.prvs, self.nxts, self.flows, self.occ, self.hs, self.ws_ = [], [], [], [], [], []
        for i, (p, x, f, m) in enumerate(zip(prvs, nxts, flows, occluded)):
            for name, t in (("prv", p), ("nxt", x), ("flow", f)):
                _check_tensor("{}[{}]".format(name, i), t)
                if t.device != flows[0].device:
                    raise ValueError("{}[{}] is on {}, flow[0] on {}".format(name, i, t.device, flows[0].device))
            B, h, w, c = f.shape if nhwc else (f.shape[0], f.shape[2], f.shape[3], f.shape[1])
            if c != 2 or (i and B != self.B):
                raise ValueError("flow[{}] must be a 2-channel flow ({}) of one batch size, got {}".format(
                    i, data_format, tuple(f.shape)))
            self.B = int(B)
            for name, t in (("prv", p), ("nxt", x)):
                if t.dtype != torch.float32 or tuple(t.shape) != (B, h, w, 3):
                    raise ValueError("{}[{}] must be float32 {}, got {} {}".format(name, i, (B, h, w, 3), t.dtype,
                                                                                  tuple(t.shape)))
                if _wants_grad(t):
                    raise ValueError("{}[{}] requires grad: the frames are constants, only the flow is differentiated "
                                     "(detach it)".format(name, i))
            if m is not None and not (isinstance(m, torch.Tensor) and m.dtype == torch.uint8
                                      and tuple(m.shape) == (B, h, w) and m.device == f.device):
                raise ValueError("occluded[{}] must be None or a uint8 tensor of shape {} on {}".format(i, (B, h, w),
                                                                                                       f.device))
            self.prvs.append(p.contiguous())
            self.nxts.append(x.contiguous())
            self.flows.append(f.contiguous())
            self.occ.append(None if m is None else m.contiguous())
            self.hs.append(int(h))
            self.ws_.append(int(w))
        self.dev = self.flows[0].device
        self.ha, self.wa = (ctypes.c_int * n)(*self.hs), (ctypes.c_int * n)(*self.ws_)
        self.fdt = (ctypes.c_int * n)(*[_DTYPES[f.dtype] for f in self.flows])

    def ptrs(self, ts):
        return (ctypes.c_void_p * self.n)(*[0 if t is None else t.data_ptr() for t in ts])


def unsup_loss_fwd(kind, prvs, nxts, flows, occluded=None, data_format=CHANNELS_LAST, q=0.4, eps=0.01,
                   smooth_weight=0.0, edge=150.0, smooth_eps=1e-3):
    """The label-free flow loss of 1..8 levels (qpwc_unsup_loss_fwd, include/qpwc_unsup_loss.h; kind _hip.UNSUP_CENSUS /
    _hip.UNSUP_CHARBONNIER) -> (losses, photometric, smoothness: fp32 [L], counts: int64 [L], saved), all on the device.
    prvs[l], nxts[l]: fp32 (B,h,w,3) channels-last; flows[l]: fp32 or fp16 in data_format; occluded: None or a list of
    None / uint8 (B,h,w).  saved: what unsup_loss_bwd takes (the operands and the workspace the forward filled).  One
    launch plus the fold; enqueues and returns: no host synchronisation."""
    o = _UnsupOperands(prvs, nxts, flows, occluded, data_format)
    n, dev = o.n, o.dev
    L = _hip.lib()
    nws = L.qpwc_unsup_loss_workspace_floats(int(kind), o.B, o.ha, o.wa, n)
    _hip.check(min(int(nws), 0))
    with torch.cuda.device(dev):
        ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
        out = torch.empty((3, n), dtype=torch.float32, device=dev)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        with _timed("unsup_loss", (o.B, o.hs[0], o.ws_[0], n)):
            rc = L.qpwc_unsup_loss_fwd(int(kind), float(q), float(eps), float(smooth_weight), float(edge),
                                       float(smooth_eps), o.ptrs(o.prvs), o.ptrs(o.nxts), o.ptrs(o.flows),
                                       o.ptrs(o.occ), o.B, o.ha, o.wa, o.fdt, o.layout, n, out[0].data_ptr(),
                                       out[1].data_ptr(), out[2].data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                       _stream(ws))
    _hip.check(rc)
    return out[0], out[1], out[2], counts, (o, ws)


def unsup_loss_bwd(kind, saved, counts, grad_losses, smooth_weight=0.0, smooth_eps=1e-3):
    """d losses / d flows times grad_losses [L] (on the device) in each flow's dtype and layout, all levels in one launch
    (qpwc_unsup_loss_bwd); saved and counts from unsup_loss_fwd with the same kind and parameters.  The counts stay on the
    device."""
    o, ws = saved
    g = grad_losses.to(torch.float32).contiguous()
    if g.numel() != o.n or g.device != o.dev:
        raise ValueError("grad_losses must be a device vector of {} elements".format(o.n))
    with torch.cuda.device(o.dev):
        grads = [torch.empty_like(f) for f in o.flows]
        with _timed("unsup_loss_bwd", (o.n,)):
            rc = _hip.lib().qpwc_unsup_loss_bwd(int(kind), float(smooth_weight), float(smooth_eps), o.ptrs(o.flows),
                                                ws.data_ptr(), counts.data_ptr(), g.data_ptr(), o.ptrs(grads), o.B, o.ha,
                                                o.wa, o.fdt, o.layout, o.n, _stream(g))
    _hip.check(rc)
    return grads


class _UnsupLossFn(torch.autograd.Function):
    """unsup_loss_fwd() with qpwc_unsup_loss_bwd as its gradient: the forward saves per pixel what the backward's gather
    needs; the frames and the masks are constants."""

    @staticmethod
    def forward(ctx, cfg, prvs, nxts, occluded, *flows):
        kind, data_format, q, eps, smooth_weight, edge, smooth_eps = cfg
        losses, photo, smooth, counts, saved = unsup_loss_fwd(kind, prvs, nxts, flows, occluded, data_format, q, eps,
                                                              smooth_weight, edge, smooth_eps)
        ctx.cfg, ctx.saved, ctx.counts, ctx.n = cfg, saved, counts, len(flows)
        ctx.mark_non_differentiable(photo, smooth, counts)
        ctx.set_materialize_grads(False)
        return losses, photo, smooth, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_losses, *_others):
        _refuse_capture("the unsupervised loss backward")
        if grad_losses is None:
            return (None,) * (4 + ctx.n)
        kind, _, _, _, smooth_weight, _, smooth_eps = ctx.cfg
        grads = unsup_loss_bwd(kind, ctx.saved, ctx.counts, grad_losses, smooth_weight, smooth_eps)
        return (None,) * 4 + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:]))


def unsup_loss(kind, prvs, nxts, flows, occluded=None, data_format=CHANNELS_LAST, q=0.4, eps=0.01, smooth_weight=0.0,
               edge=150.0, smooth_eps=1e-3):
    """(losses, photometric, smoothness fp32 [L], counts int64 [L]) of unsup_loss_fwd(); the losses are differentiable in
    the flows when grad is enabled and one of them requires it (the parts are reported, not differentiated)."""
    flows = list(flows)
    if _wants_grad(*flows):
        _refuse_capture("the unsupervised loss")
        cfg = (int(kind), data_format, float(q), float(eps), float(smooth_weight), float(edge), float(smooth_eps))
        return _UnsupLossFn.apply(cfg, list(prvs), list(nxts), None if occluded is None else list(occluded), *flows)
    return unsup_loss_fwd(kind, prvs, nxts, flows, occluded, data_format, q, eps, smooth_weight, edge, smooth_eps)[:4]


def resized_ground_truth(y_true, shapes, data_format=CHANNELS_LAST):
    """AutoResizeMseLoss's per-level target (qpwcnet/train/loss.py:177-197): y_true resized to every (h, w) of shapes as
    tf.image.resize does it (bilinear, half-pixel centres, no antialias), any channel count, no flow scale -> list of
    dense fp32 tensors in data_format; up to 8 levels per pass over y_true (qpwc_loss_fwd with gt_out only)."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    out = []
    for k in range(0, len(shapes), 8):
        out += [t.contiguous() for t in loss_fwd(_hip.LOSS_AUTORESIZE_MSE, y_true, None, data_format, want_gt=True,
                                                 shapes=shapes[k:k + 8])[2]]
    return out


def image_loss_kernel(B, C, shapes):
    """The forward kernel ``qpwc_image_loss_fwd`` takes for these levels ('image_loss_fwd_kernel'; host only).  '' for
    arguments the entry point refuses."""
    n = len(shapes)
    ha, wa = (ctypes.c_int * n)(*[int(h) for h, _ in shapes]), (ctypes.c_int * n)(*[int(w) for _, w in shapes])
    name = _hip.lib().qpwc_image_loss_fwd_kernel(int(B), int(C), ha, wa, n)
    return name.decode() if name else ""


class _ImageLossOperands:
    """What both image loss entry points make of their operands: per level the fp32 target and the prediction (fp32 or
    fp16), dense in `data_format` and of one shape, all levels of one batch and channel count; B, C, the level shapes and
    the ctypes arrays."""

    def __init__(self, truths, preds, data_format):
        get_axis(data_format)
        truths, preds = list(truths), list(preds)
        self.n = n = len(preds)
        if not 1 <= n <= 8:
            raise ValueError("the losses take 1..8 prediction levels, got {}".format(n))
        if len(truths) != n:
            raise ValueError("{} predictions against {} targets".format(n, len(truths)))
        self.nhwc = nhwc = data_format == CHANNELS_LAST
        self.layout = _hip.NHWC if nhwc else _hip.NCHW
        self.truths, self.preds, self.hs, self.ws_ = [], [], [], []
        for i, (t, p) in enumerate(zip(truths, preds)):
            for name, x in (("truth", t), ("pred", p)):
                _check_tensor("{}[{}]".format(name, i), x)
                if x.device != preds[0].device:
                    raise ValueError("{}[{}] is on {}, pred[0] on {}".format(name, i, x.device, preds[0].device))
            B, h, w, C = p.shape if nhwc else (p.shape[0], p.shape[2], p.shape[3], p.shape[1])
            if not 1 <= C <= 4 or (i and (B, C) != (self.B, self.C)):
                raise ValueError("pred[{}] must be an image of 1..4 channels ({}) of one batch size and channel count, "
                                 "got {}".format(i, data_format, tuple(p.shape)))
            self.B, self.C = int(B), int(C)
            if t.dtype != torch.float32 or t.shape != p.shape:
                raise ValueError("truth[{}] must be float32 {}, got {} {}".format(i, tuple(p.shape), t.dtype,
                                                                                  tuple(t.shape)))
            if _wants_grad(t):
                raise ValueError("truth[{}] requires grad: the losses are differentiable in y_pred only, a gradient for "
                                 "y_true would be dropped (detach it)".format(i))
            self.truths.append(t.contiguous())
            self.preds.append(p.contiguous())
            self.hs.append(int(h))
            self.ws_.append(int(w))
        self.dev = self.preds[0].device
        self.ha, self.wa = (ctypes.c_int * n)(*self.hs), (ctypes.c_int * n)(*self.ws_)
        self.pdt = (ctypes.c_int * n)(*[_DTYPES[p.dtype] for p in self.preds])

    def ptrs(self, ts):
        return (ctypes.c_void_p * self.n)(*[t.data_ptr() for t in ts])


def image_loss_fwd(truths, preds, data_format=CHANNELS_LAST, ssim_weight=0.85, q=0.5, eps=1e-3, max_val=1.0, offset=0.5):
    """The SSIM + Charbonnier loss of 1..8 levels (qpwc_image_loss_fwd, include/qpwc_image_loss.h) -> (losses, dssim,
    charbonnier: fp32 [L], saved), all on the device.  truths[l]: the level's fp32 target, preds[l]: fp32 or fp16, both
    dense in data_format and of one shape.  saved: what image_loss_bwd takes (the operands and the workspace the forward
    filled).  One launch plus the fold, the workspace from torch's allocator on the current stream; enqueues and
    returns: no host synchronisation."""
    o = _ImageLossOperands(truths, preds, data_format)
    n, dev = o.n, o.dev
    L = _hip.lib()
    nws = L.qpwc_image_loss_workspace_floats(o.B, o.C, o.ha, o.wa, n)
    _hip.check(min(int(nws), 0))
    with torch.cuda.device(dev):
        ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
        losses, dssim, charb = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))   # no shared base
        with _timed("image_loss", (o.B, o.hs[0], o.ws_[0], o.C, n)):
            rc = L.qpwc_image_loss_fwd(float(ssim_weight), float(q), float(eps), float(max_val), float(offset),
                                       o.ptrs(o.truths), o.ptrs(o.preds), o.B, o.C, o.ha, o.wa, o.pdt, o.layout, n,
                                       losses.data_ptr(), dssim.data_ptr(), charb.data_ptr(), ws.data_ptr(),
                                       _stream(ws))
    _hip.check(rc)
    return losses, dssim, charb, (o, ws)


def image_loss_bwd(saved, grad_losses, ssim_weight=0.85, q=0.5, eps=1e-3, offset=0.5):
    """d losses / d preds times grad_losses [L] (on the device) in each prediction's dtype and layout, all levels in one
    launch (qpwc_image_loss_bwd); saved from image_loss_fwd with the same parameters."""
    o, ws = saved
    g = grad_losses.to(torch.float32).contiguous()
    if g.numel() != o.n or g.device != o.dev:
        raise ValueError("grad_losses must be a device vector of {} elements".format(o.n))
    with torch.cuda.device(o.dev):
        grads = [torch.empty_like(p) for p in o.preds]
        with _timed("image_loss_bwd", (o.n,)):
            rc = _hip.lib().qpwc_image_loss_bwd(float(ssim_weight), float(q), float(eps), float(offset),
                                                o.ptrs(o.truths), o.ptrs(o.preds), ws.data_ptr(), g.data_ptr(),
                                                o.ptrs(grads), o.B, o.C, o.ha, o.wa, o.pdt, o.layout, o.n, _stream(g))
    _hip.check(rc)
    return grads


class _ImageLossFn(torch.autograd.Function):
    """image_loss_fwd() with qpwc_image_loss_bwd as its gradient: the forward saves s's three partial derivatives per
    position, the backward runs the transposed window pass over them; the targets are constants."""

    @staticmethod
    def forward(ctx, cfg, truths, *preds):
        data_format, ssim_weight, q, eps, max_val, offset = cfg
        losses, dssim, charb, saved = image_loss_fwd(truths, preds, data_format, ssim_weight, q, eps, max_val, offset)
        ctx.cfg, ctx.saved, ctx.n = cfg, saved, len(preds)
        ctx.mark_non_differentiable(dssim, charb)
        ctx.set_materialize_grads(False)
        return losses, dssim, charb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_losses, *_others):
        _refuse_capture("the image loss backward")
        if grad_losses is None:
            return (None,) * (2 + ctx.n)
        _, ssim_weight, q, eps, _, offset = ctx.cfg
        grads = image_loss_bwd(ctx.saved, grad_losses, ssim_weight, q, eps, offset)
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


def image_loss(truths, preds, data_format=CHANNELS_LAST, ssim_weight=0.85, q=0.5, eps=1e-3, max_val=1.0, offset=0.5):
    """(losses, dssim, charbonnier: fp32 [L]) of image_loss_fwd(); the losses are differentiable in the predictions when
    grad is enabled and one of them requires it (the parts are reported, not differentiated)."""
    preds = list(preds)
    if _wants_grad(*preds):
        _refuse_capture("the image loss")
        cfg = (data_format, float(ssim_weight), float(q), float(eps), float(max_val), float(offset))
        return _ImageLossFn.apply(cfg, list(truths), *preds)
    return image_loss_fwd(truths, preds, data_format, ssim_weight, q, eps, max_val, offset)[:3]


def _dw_sources(sources):
    """-> (kept tensors, ctypes pointer/channel/stride arrays, B, H, W, C) for 1..3 sources."""
    import ctypes
    if not 1 <= len(sources) <= 3:
        raise ValueError("takes 1..3 sources")
    B, H, W = sources[0].shape[:3]
    chans, strides, ptrs, keep = [], [], [], []
    for i, t in enumerate(sources):
        _check_tensor("source %d" % i, t)
        if t.dtype != sources[0].dtype or tuple(t.shape[:3]) != (B, H, W):
            raise ValueError("sources must share dtype and B,H,W")
        if t.stride(3) != 1 or t.stride(1) != W * t.stride(2) or t.stride(0) != H * t.stride(1):
            t = t.contiguous()
        keep.append(t)
        chans.append(t.shape[3])
        strides.append(t.stride(2))
        ptrs.append(t.data_ptr())
    n = len(keep)
    return keep, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*chans), (ctypes.c_int64 * n)(*strides), \
        B, H, W, sum(chans)


def pad_pointwise(pw, dtype=torch.float32):
    """(F, C[,1,1]) pointwise kernel -> dense (F, ceil(C/32)*32), zero padded: the layout
    qpwc_sepconv3x3_fwd (fp32) / qpwc_sepconv3x3_f16_fwd (fp16) takes."""
    pw = pw.reshape(pw.shape[0], -1).to(dtype)
    F_, C = pw.shape
    cpad = (C + 31) // 32 * 32
    out = torch.zeros((F_, cpad), dtype=dtype, device=pw.device)
    out[:, :C] = pw
    return out


def sepconv3x3_bwd(sources, dw, pw_padded, bias, grad_out, mish_on_load=False, mish_on_store=False,
                   need=(True, True, True, True)):
    """Gradients of sepconv3x3() (fp32, qpwc_sepconv3x3_bwd) for grad_out = dL/d(what the forward stored), dense
    (B,H,W,F).  need = (sources, dw, pw, bias); `sources` one flag for all or one per source.
    -> (list of per-source dense (B,H,W,c_i) gradients, grad_dw (C,3,3), grad_pw (F,Cpad), grad_bias (F)); whatever
    is not asked for comes back as None."""
    import ctypes
    keep, c_ptrs, c_ch, c_st, B, H, W, C = _dw_sources(sources)
    F_ = pw_padded.shape[-2]
    w = dw.reshape(-1, 9)
    cpad = (C + 31) // 32 * 32
    if w.shape[0] != C or pw_padded.shape[-1] != cpad or bias.numel() != F_:
        raise ValueError("weight shapes do not match C = {}".format(C))
    for t in keep + [grad_out]:
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError("sepconv3x3_bwd takes fp32 device tensors")
    for t in (w, pw_padded, bias):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("weights must be dense fp32 device tensors")
    if tuple(grad_out.shape) != (B, H, W, F_):
        raise ValueError("grad_out shape {} is not {}".format(tuple(grad_out.shape), (B, H, W, F_)))
    grad_out = grad_out.contiguous()
    need_src, need_dw, need_pw, need_b = need
    if isinstance(need_src, bool):
        need_src = (need_src,) * len(keep)
    if len(need_src) != len(keep):
        raise ValueError("need[0] must hold one flag per source")
    dev = keep[0].device
    L = _hip.lib()
    ws, outs, ptrs = _bwd_buffers(L.qpwc_sepconv3x3_bwd_workspace_floats(B, H, W, C, F_),
                                  [(B, H, W, t.shape[3]) for t in keep] + [(C, 3, 3), (F_, cpad), (F_,)],
                                  tuple(need_src) + (need_dw, need_pw, need_b), dev)
    gs, (gdw, gpw, gb) = outs[:-3], outs[-3:]
    g_ptrs = (ctypes.c_void_p * len(keep))(*ptrs[:-3])
    flags = int(bool(mish_on_load)) | (2 if mish_on_store else 0)
    with torch.cuda.device(dev), _timed("sepconv3x3_bwd", (B, H, W, C, F_)):
        rc = L.qpwc_sepconv3x3_bwd(c_ptrs, c_ch, c_st, len(keep), flags, w.data_ptr(), pw_padded.data_ptr(),
                                   bias.data_ptr(), grad_out.data_ptr(), g_ptrs, *ptrs[-3:], ws.data_ptr(), B, H, W, F_,
                                   _stream(grad_out))
    _hip.check(rc)
    return gs, gdw, gpw, gb


class _SepConvFn(torch.autograd.Function):
    """sepconv3x3() with qpwc_sepconv3x3_bwd as its gradient: the forward is the no-grad forward itself; the sources
    and weights are saved, never the depthwise result or the pre-activation (the backward recomputes them)."""

    @staticmethod
    def forward(ctx, mish_on_load, mish_on_store, dw, pw_padded, bias, *sources):
        _refuse_capture("the separable convolution")
        out = sepconv3x3(sources, dw, pw_padded, bias, mish_on_load, mish_on_store)
        ctx.save_for_backward(dw, pw_padded, bias, *sources)
        ctx.cfg = (bool(mish_on_load), bool(mish_on_store))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the separable-convolution backward")
        dw, pw_padded, bias = ctx.saved_tensors[:3]
        sources = ctx.saved_tensors[3:]
        on_load, on_store = ctx.cfg
        nig = ctx.needs_input_grad
        gs, gdw, gpw, gb = sepconv3x3_bwd(sources, dw, pw_padded, bias, grad_out.to(torch.float32), on_load, on_store,
                                          (tuple(nig[5:]), nig[2], nig[3], nig[4]))
        # a source handed in as a strided view (the 84-float cost volume) gets a dense gradient of its own shape
        return (None, None, gdw.reshape(dw.shape) if gdw is not None else None, gpw,
                gb.reshape(bias.shape) if gb is not None else None) + tuple(gs)


def sepconv3x3(sources, dw, pw_padded, bias, mish_on_load=False, mish_on_store=False):
    """SeparableConv2D(3x3,'same'), fused (fp32): depthwise 3x3 over the virtual concat of 1..3
    channels-last sources, pointwise 1x1 + bias on the matrix cores
    (qpwcnet/core/non_layers.py:223-231).  pw_padded from pad_pointwise().
    -> (B,H,W,F): the pre-activation output, or Mish of it with mish_on_store (the layer's own
    `activation='Mish'` applied once per element; the consumer then loads without Mish).
    Differentiable (fp32) in the sources, dw, pw_padded and bias: with grad enabled and one of them requiring grad
    the same forward runs inside an autograd Function whose backward is qpwc_sepconv3x3_bwd.  A source that is not
    dense channels-last (the permuted view of a channels_first tensor) is copied dense in the forward and once more
    in the backward: two transposes per step that channels-last training does not pay."""
    if _wants_grad(dw, pw_padded, bias, *sources):
        _refuse_capture("the separable convolution")
        if not 1 <= len(sources) <= 3:
            raise ValueError("takes 1..3 sources")
        if any(isinstance(t, torch.Tensor) and t.dtype == torch.float16 for t in tuple(sources) + (pw_padded,)):
            raise ValueError("sepconv3x3 has no gradient for fp16 storage: train in fp32")
        if pw_padded.dtype == torch.bfloat16:
            raise ValueError("sepconv3x3 has no gradient for a bf16x3 pointwise weight: pass pad_pointwise() itself")
        for i, t in enumerate(sources):
            _check_tensor("source %d" % i, t)
        for name, t in (("dw", dw), ("pw_padded", pw_padded), ("bias", bias)):
            if not t.is_cuda:
                raise RuntimeError("qpwcnet_amd: {} is on '{}'; the hot path runs on a HIP device only "
                                   "(no CPU fallback)".format(name, t.device))
        return _SepConvFn.apply(bool(mish_on_load), bool(mish_on_store), dw, pw_padded, bias, *sources)
    keep, c_ptrs, c_ch, c_st, B, H, W, C = _dw_sources(sources)
    F_ = pw_padded.shape[-2]
    w = dw.reshape(-1, 9)
    if w.shape[0] != C or pw_padded.shape[-1] != (C + 31) // 32 * 32 or bias.numel() != F_:
        raise ValueError("weight shapes do not match C = {}".format(C))
    flags = int(bool(mish_on_load)) | (2 if mish_on_store else 0)
    if keep[0].dtype == torch.float16:
        return _sepconv3x3_f16(keep, c_ptrs, c_ch, c_st, w, pw_padded, bias, flags, B, H, W, C, F_)
    if keep[0].dtype != torch.float32:
        raise ValueError("sepconv3x3 takes fp32 or fp16 sources")
    if pw_padded.dtype == torch.bfloat16:
        return _sepconv3x3_x3(keep, c_ptrs, c_ch, c_st, w, pw_padded, bias, flags, B, H, W, C)
    for t in (w, pw_padded, bias):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("weights must be dense fp32 device tensors")
    out = torch.empty((B, H, W, F_), dtype=torch.float32, device=keep[0].device)
    with torch.cuda.device(out.device), _timed("sepconv3x3", (B, H, W, C, F_)):
        rc = _hip.lib().qpwc_sepconv3x3_fwd(c_ptrs, c_ch, c_st, len(keep), flags,
                                             w.data_ptr(), pw_padded.data_ptr(), bias.data_ptr(),
                                             out.data_ptr(), B, H, W, F_, _stream(out))
    _hip.check(rc)
    return out


def sepconv3x3_x3_applies(sources):
    """True when qpwc_sepconv3x3_x3_fwd takes these fp32 sources: every source but the last a multiple of 4 channels
    in 16-byte aligned pixels (a last source of fewer than 4 channels is allowed), H * W < 2^24."""
    n = len(sources)
    for i, t in enumerate(sources):
        aligned = t.shape[3] % 4 == 0 and t.stride(2) % 4 == 0 and t.data_ptr() % 16 == 0
        if not aligned and (i + 1 < n or t.shape[3] >= 4 or t.shape[0] * t.shape[1] * t.shape[2] * t.stride(2) < 8):
            return False
        if t.shape[1] * t.shape[2] >= 1 << 24 or t.stride(2) >= 1 << 24 or t.shape[1] * t.shape[2] * t.stride(2) >= 1 << 31:
            return False
    return all(t.dtype == torch.float32 for t in sources)


def _sepconv3x3_x3(keep, c_ptrs, c_ch, c_st, w, pw3, bias, flags, B, H, W, C):
    """fp32 with the pointwise products as bf16x3 splits (qpwc_sepconv3x3_x3_fwd): pw3 = split_bf16x3(pad_pointwise(..))
    = (3, F, Cpad) bfloat16, dw / bias fp32."""
    F_ = pw3.shape[1]
    if pw3.dim() != 3 or pw3.shape[0] != 3 or not pw3.is_cuda or not pw3.is_contiguous():
        raise ValueError("pw3 must be a dense (3, F, Cpad) bfloat16 device tensor")
    for t in (w, bias):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("dw / bias must be dense fp32 device tensors")
    out = torch.empty((B, H, W, F_), dtype=torch.float32, device=keep[0].device)
    with torch.cuda.device(out.device), _timed("sepconv3x3_x3", (B, H, W, C, F_)):
        rc = _hip.lib().qpwc_sepconv3x3_x3_fwd(c_ptrs, c_ch, c_st, len(keep), flags, w.data_ptr(), pw3.data_ptr(),
                                                bias.data_ptr(), out.data_ptr(), B, H, W, F_, _stream(out))
    _hip.check(rc)
    return out


def _sepconv3x3_f16(keep, c_ptrs, c_ch, c_st, w, pw_padded, bias, flags, B, H, W, C, F_):
    """fp16-storage form (qpwc_sepconv3x3_f16_fwd): pw_padded fp16, dw / bias fp32."""
    for i, t in enumerate(keep):
        tail = i + 1 == len(keep) and t.shape[3] < 4
        if not tail and (t.shape[3] % 4 or t.stride(2) % 4 or t.data_ptr() % 8):
            raise ValueError("fp16 sepconv3x3: sources must hold multiples of 4 channels in 8-byte aligned pixels")
    for t, dt in ((w, torch.float32), (pw_padded, torch.float16), (bias, torch.float32)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError("fp16 sepconv3x3: dw/bias dense fp32, pw dense fp16 device tensors")
    out = torch.empty((B, H, W, F_), dtype=torch.float16, device=keep[0].device)
    with torch.cuda.device(out.device), _timed("sepconv3x3_f16", (B, H, W, C, F_)):
        rc = _hip.lib().qpwc_sepconv3x3_f16_fwd(c_ptrs, c_ch, c_st, len(keep), flags, w.data_ptr(),
                                                 pw_padded.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                 B, H, W, F_, _stream(out))
    _hip.check(rc)
    return out


def conv3x3_taps(weight, dtype=torch.float32):
    """torch Conv2d weight (C_out, C_in, 3, 3) -> the (9, C_out, C_in) tap-major layout of
    qpwc_conv3x3_mish_fwd (fp32) / qpwc_conv3x3_mish_f16_fwd (dtype=torch.float16)."""
    return weight.to(dtype).permute(2, 3, 0, 1).reshape(9, weight.shape[0], weight.shape[1]).contiguous()


def conv3x3_mish(x_nhwc, taps, bias, pad_h=0, pad_w=0):
    """Mish(conv3x3_same(x) + bias) for C_in = C_out in {16, 32, 64, 128, 256}, channels-last fp32 (the encoder's
    conv_aa / conv_b, non_layers.py:410-449), written into a (B, H+pad_h, W+pad_w, C) tensor whose
    border is zero (the 'SAME' padding of a following stride-2 conv).  taps from conv3x3_taps()."""
    _check_tensor("x", x_nhwc)
    if x_nhwc.dtype not in (torch.float32, torch.float16) or not x_nhwc.is_contiguous():
        raise ValueError("conv3x3_mish needs a dense fp32 / fp16 channels-last tensor")
    B, H, W, C = x_nhwc.shape
    if tuple(taps.shape) != (9, C, C) or taps.dtype != x_nhwc.dtype or not taps.is_cuda or \
            not taps.is_contiguous() or bias.numel() != C or bias.dtype != torch.float32 or not bias.is_cuda:
        raise ValueError("taps must be a dense (9,{0},{0}) device tensor of the input's dtype, bias fp32 ({0})".format(C))
    out = torch.empty((B, H + pad_h, W + pad_w, C), dtype=x_nhwc.dtype, device=x_nhwc.device)
    fn = _hip.lib().qpwc_conv3x3_mish_fwd if x_nhwc.dtype == torch.float32 else _hip.lib().qpwc_conv3x3_mish_f16_fwd
    with torch.cuda.device(out.device), _timed("conv3x3_mish" if x_nhwc.dtype == torch.float32 else "conv3x3_mish_f16",
                                               (B, H, W, C)):
        rc = fn(x_nhwc.data_ptr(), taps.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W, C, int(pad_h), int(pad_w),
                _stream(out))
    _hip.check(rc)
    return out


def conv3x3_same_taps(weight):
    """torch Conv2d weight (C_out, C_in, 3, 3) -> fp32 (9, C_out, Cp) [tap][out][in], Cp = C_in rounded up to 4 with
    zero pad slots: conv3x3_taps() for the encoder's widths, first_conv_taps() for C_in = 3 (qpwc_conv3x3_same_*)."""
    co, ci = weight.shape[0], weight.shape[1]
    w = weight.to(torch.float32).permute(2, 3, 0, 1).reshape(9, co, ci)
    if ci % 4 == 0:
        return w.contiguous()
    out = torch.zeros((9, co, (ci + 3) // 4 * 4), dtype=torch.float32, device=w.device)
    out[..., :ci] = w
    return out


_CONV_SAME_CIN = (3, 16, 32, 64, 128, 256)
_CONV_SAME_COUT = (16, 32, 64, 128, 256)


def _conv_same_check(x, weight, bias, stride, what):
    """The operand rules of qpwc_conv3x3_same_fwd / _bwd -> (B, H, W, C_in, C_out, Ho, Wo); weight in the torch layout
    (C_out, C_in, 3, 3) or as its taps (9, C_out, Cp)."""
    _grad_operands_check(x, weight, bias, what)
    if stride not in (1, 2):
        raise ValueError("{}: stride {} not in (1, 2)".format(what, stride))
    B, H, W, ci = x.shape
    taps = weight.dim() == 3
    co = weight.shape[1] if taps else weight.shape[0]
    if ci not in _CONV_SAME_CIN or co not in _CONV_SAME_COUT:
        raise ValueError("{}: C_in {} -> C_out {} outside {} -> {}".format(what, ci, co, _CONV_SAME_CIN, _CONV_SAME_COUT))
    want = (9, co, (ci + 3) // 4 * 4) if taps else (co, ci, 3, 3)
    if tuple(weight.shape) != want or (taps and not weight.is_contiguous()) or bias.numel() != co or \
            not bias.is_contiguous():
        raise ValueError("{}: weight must hold (C_out, {}, 3, 3), bias (C_out)".format(what, ci))
    if min(B, H, W) < 1:
        raise ValueError("{}: empty input {}".format(what, tuple(x.shape)))
    return B, H, W, ci, co, -(-H // stride), -(-W // stride)


def _conv3x3_same_fwd(x, taps, bias, stride, mish):
    """The forward launch of conv3x3_same(): the encoder's own kernels where their preconditions hold (stride 1 with
    C_in = C_out: qpwc_conv3x3_mish_fwd; stride 2 with even H, W and C_out = 2 C_in: qpwc_conv3x3s2_mish_c_fwd on a
    zero-bordered copy of x), else qpwc_conv3x3_same_fwd."""
    B, H, W, ci, co, Ho, Wo = _conv_same_check(x, taps, bias, stride, "conv3x3_same")
    if mish and stride == 1 and ci == co:
        return conv3x3_mish(x, taps, bias)
    if mish and stride == 2 and H % 2 == 0 and W % 2 == 0 and co == 2 * ci and ci in (16, 32, 64, 128):
        return conv3x3s2_mish(torch.nn.functional.pad(x, (0, 0, 0, 1, 0, 1)), taps, bias)
    out = torch.empty((B, Ho, Wo, co), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("conv3x3_same", (B, H, W, ci, co, stride)):
        rc = _hip.lib().qpwc_conv3x3_same_fwd(x.data_ptr(), taps.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W,
                                               ci, co, int(stride), int(bool(mish)), _stream(x))
    _hip.check(rc)
    return out


def conv3x3_same_bwd(x_nhwc, taps, bias, grad_out, stride=1, mish=True, need=(True, True, True)):
    """Gradients of conv3x3_same() (fp32, qpwc_conv3x3_same_bwd) for grad_out = dL/d(out), dense (B,Ho,Wo,C_out); taps
    from conv3x3_same_taps().  need = (x, weight, bias) -> (grad_x (B,H,W,C_in), grad_taps (9,C_out,Cp) in the layout
    of taps, grad_bias (C_out)); whatever is not asked for comes back as None and its pointer goes in as NULL."""
    B, H, W, ci, co, Ho, Wo = _conv_same_check(x_nhwc, taps, bias, stride, "conv3x3_same_bwd")
    if not isinstance(grad_out, torch.Tensor) or not grad_out.is_cuda or grad_out.dtype != torch.float32 or \
            tuple(grad_out.shape) != (B, Ho, Wo, co):
        raise ValueError("conv3x3_same_bwd: grad_out must be an fp32 device tensor of shape {}".format((B, Ho, Wo, co)))
    if not any(need):
        raise ValueError("conv3x3_same_bwd: nothing asked for")
    grad_out = grad_out.contiguous()
    dev = x_nhwc.device
    L = _hip.lib()
    ws, outs, ptrs = _bwd_buffers(L.qpwc_conv3x3_same_bwd_workspace_floats(B, H, W, ci, co, int(stride)),
                                  ((B, H, W, ci), taps.shape, (co,)), need, dev)
    with torch.cuda.device(dev), _timed("conv3x3_same_bwd", (B, H, W, ci, co, stride)):
        rc = L.qpwc_conv3x3_same_bwd(x_nhwc.data_ptr(), taps.data_ptr(), bias.data_ptr(), grad_out.data_ptr(), *ptrs,
                                     ws.data_ptr(), B, H, W, ci, co, int(stride), int(bool(mish)), _stream(grad_out))
    _hip.check(rc)
    return tuple(outs)


class _ConvSameFn(torch.autograd.Function):
    """conv3x3_same() with qpwc_conv3x3_same_bwd as its gradient: the forward is the no-grad forward itself; x, weight
    and bias are saved, never the pre-activation (the backward recomputes it)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, mish):
        _refuse_capture("the 3x3 convolution")
        out = _conv3x3_same_fwd(x, conv3x3_same_taps(weight), bias, stride, mish)
        ctx.save_for_backward(x, weight, bias)
        ctx.cfg = (int(stride), bool(mish))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the 3x3-convolution backward")
        x, weight, bias = ctx.saved_tensors
        stride, mish = ctx.cfg
        nig = ctx.needs_input_grad
        gx, gt, gb = conv3x3_same_bwd(x, conv3x3_same_taps(weight), bias, grad_out.to(torch.float32), stride, mish,
                                      (nig[0], nig[1], nig[2]))
        co, ci = weight.shape[0], weight.shape[1]
        # the torch layout as a permuted view of the tap-major buffer (its pad slot, C_in = 3, left out)
        gw = gt[..., :ci].reshape(3, 3, co, ci).permute(2, 3, 0, 1) if gt is not None else None
        return gx, gw, gb.reshape(bias.shape) if gb is not None else None, None, None


def conv3x3_same(x_nhwc, weight, bias, stride=1, mish=True, matmul="f32"):
    """Conv2D(C_out, 3x3, strides=stride, padding='same') (+ Mish) of the encoder (qpwcnet/core/non_layers.py:390-449) on
    a dense channels-last fp32 (B,H,W,C_in) tensor of any size, C_in in {3,16,32,64,128,256}, C_out in
    {16,32,64,128,256}; weight in the torch layout (C_out, C_in, 3, 3), bias (C_out) -> (B, ceil(H/stride),
    ceil(W/stride), C_out).  Differentiable in x, weight and bias: with grad enabled and one of them requiring grad the
    same forward launch runs inside an autograd Function whose backward is qpwc_conv3x3_same_bwd (the workspace is
    allocated per call); the result has the bits of the no-grad call."""
    if matmul != "f32":
        raise ValueError("conv3x3_same computes in fp32 only (matmul={!r}): no bf16x3 path, forward or gradient".format(
            matmul))
    for name, t in (("x", x_nhwc), ("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x_nhwc.dim() != 4 or weight.shape[1] != x_nhwc.shape[3]:
        raise ValueError("conv3x3_same: weight {} does not fit x {}".format(tuple(weight.shape), tuple(x_nhwc.shape)))
    if _wants_grad(x_nhwc, weight, bias):
        _refuse_capture("the 3x3 convolution")
        _conv_same_check(x_nhwc, weight, bias, stride, "conv3x3_same")   # the operand rules, before autograd sees the call
        return _ConvSameFn.apply(x_nhwc, weight, bias, int(stride), bool(mish))
    return _conv3x3_same_fwd(x_nhwc, conv3x3_same_taps(weight), bias, stride, mish)


def split_bf16x3(t):
    """fp32 device tensor -> (3, *t.shape) bfloat16: the three-way split of csrc/split_bf16.h (qpwc_split_bf16x3_fwd);
    out[0] + out[1] + out[2] == t exactly (parts below the smallest normal fp32 flush to zero).  The weight operands of the *_x3 kernels."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.numel() == 0:
        raise ValueError("split_bf16x3 takes a non-empty fp32 device tensor")
    t = t.contiguous()
    out = torch.empty((3,) + tuple(t.shape), dtype=torch.bfloat16, device=t.device)
    with torch.cuda.device(t.device):
        rc = _hip.lib().qpwc_split_bf16x3_fwd(t.data_ptr(), out.data_ptr(), t.numel(), _stream(t))
    _hip.check(rc)
    return out


def conv3x3_mish_x3(x_nhwc, taps3, bias, pad_h=0, pad_w=0):
    """conv3x3_mish() for fp32 tensors with the products on the bf16 matrix instructions (bf16x3 split, six partial
    products, fp32 accumulation: qpwc_conv3x3_mish_x3_fwd).  taps3 = split_bf16x3(conv3x3_taps(weight))."""
    _check_tensor("x", x_nhwc)
    if x_nhwc.dtype != torch.float32 or not x_nhwc.is_contiguous():
        raise ValueError("conv3x3_mish_x3 needs a dense fp32 channels-last tensor")
    B, H, W, C = x_nhwc.shape
    if tuple(taps3.shape) != (3, 9, C, C) or taps3.dtype != torch.bfloat16 or not taps3.is_cuda or \
            not taps3.is_contiguous() or bias.numel() != C or bias.dtype != torch.float32 or not bias.is_cuda:
        raise ValueError("taps3 must be a dense (3,9,{0},{0}) bfloat16 device tensor, bias fp32 ({0})".format(C))
    out = torch.empty((B, H + pad_h, W + pad_w, C), dtype=torch.float32, device=x_nhwc.device)
    with torch.cuda.device(out.device), _timed("conv3x3_mish_x3", (B, H, W, C)):
        rc = _hip.lib().qpwc_conv3x3_mish_x3_fwd(x_nhwc.data_ptr(), taps3.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                  B, H, W, C, int(pad_h), int(pad_w), _stream(out))
    _hip.check(rc)
    return out


def first_conv_taps(weight):
    """torch Conv2d weight (16, 3, 3, 3) of enc.0.conv_a -> (9, 16, 4) fp32 [tap][out][in, slot 3 = 0]."""
    w = weight.float().permute(2, 3, 0, 1).reshape(9, 16, 3)
    out = torch.zeros((9, 16, 4), dtype=torch.float32, device=w.device)
    out[..., :3] = w
    return out


def first_conv_mish(pairs, taps, bias, data_format=CHANNELS_LAST):
    """Split(2) + frame stacking + Conv2D(3->16, 3x3, stride 2, 'same') + bias + Mish of the first
    encoder layer (pwcnet.py:229, non_layers.py:402-409) on the raw (B,H,W,6) fp32 input -- or (B,6,H,W)
    for 'channels_first' --, H and W even -> (2B, H/2, W/2, 16) channels-last.  taps from first_conv_taps()."""
    _check_tensor("pairs", pairs)
    cf = data_format == CHANNELS_FIRST
    get_axis(data_format)
    if pairs.shape[1 if cf else 3] != 6 or pairs.dtype not in (torch.float32, torch.float16) or not pairs.is_contiguous():
        raise ValueError("pairs must be a dense fp32 / fp16 (B,H,W,6) / (B,6,H,W) tensor")
    if cf:
        B, _, H, W = pairs.shape
    else:
        B, H, W, _ = pairs.shape
    if tuple(taps.shape) != (9, 16, 4) or taps.dtype != torch.float32 or not taps.is_contiguous() or \
            bias.numel() != 16 or bias.dtype != torch.float32:
        raise ValueError("taps must be fp32 (9,16,4), bias fp32 (16)")
    out = torch.empty((2 * B, H // 2, W // 2, 16), dtype=pairs.dtype, device=pairs.device)
    fn = _hip.lib().qpwc_first_conv_mish_fwd if pairs.dtype == torch.float32 else _hip.lib().qpwc_first_conv_mish_f16_fwd
    with torch.cuda.device(out.device), _timed("first_conv_mish", (B, H, W, 6)):
        rc = fn(pairs.data_ptr(), taps.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W,
                _hip.NCHW if cf else _hip.NHWC, _stream(out))
    _hip.check(rc)
    return out


def conv3x3s2_mish(x_padded, taps, bias):
    """Mish(conv3x3 stride 2 'same' (x) + bias), C_in in {16, 32, 64, 128} -> 2 C_in channels (conv_a of encoder
    levels 2..5, non_layers.py:402-409) on the zero-bordered (B, H+1, W+1, C_in) fp32 tensor
    conv3x3_mish(pad 1, 1) writes, H and W even -> (B, H/2, W/2, 2 C_in).  taps = conv3x3_taps(weight) of
    shape (9, 2 C_in, C_in)."""
    _check_tensor("x", x_padded)
    ci = x_padded.shape[3]
    if x_padded.dtype not in (torch.float32, torch.float16) or not x_padded.is_contiguous() or ci not in (16, 32, 64, 128):
        raise ValueError("conv3x3s2_mish needs a dense fp32 / fp16 (B,H+1,W+1,C) tensor, C in {16,32,64,128}")
    B, Hp, Wp, _ = x_padded.shape
    H, W = Hp - 1, Wp - 1
    if tuple(taps.shape) != (9, 2 * ci, ci) or taps.dtype != x_padded.dtype or not taps.is_contiguous() or \
            bias.numel() != 2 * ci or bias.dtype != torch.float32:
        raise ValueError("taps must be (9,{},{}) of the input's dtype, bias fp32 ({})".format(2 * ci, ci, 2 * ci))
    out = torch.empty((B, H // 2, W // 2, 2 * ci), dtype=x_padded.dtype, device=x_padded.device)
    f16 = x_padded.dtype == torch.float16
    fn = _hip.lib().qpwc_conv3x3s2_mish_f16_fwd if f16 else _hip.lib().qpwc_conv3x3s2_mish_c_fwd
    with torch.cuda.device(out.device), _timed("conv3x3s2_mish_f16" if f16 else "conv3x3s2_mish", (B, H, W, ci)):
        rc = fn(x_padded.data_ptr(), taps.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W, ci, _stream(out))
    _hip.check(rc)
    return out


def conv3x3s2_mish_x3(x_padded, taps3, bias):
    """conv3x3s2_mish() for fp32 tensors, C_in in {32, 64, 128}, with the products on the bf16 matrix instructions
    (qpwc_conv3x3s2_mish_x3_fwd).  taps3 = split_bf16x3(conv3x3_taps(weight)) of shape (3, 9, 2 C_in, C_in)."""
    _check_tensor("x", x_padded)
    ci = x_padded.shape[3]
    if x_padded.dtype != torch.float32 or not x_padded.is_contiguous() or ci not in (32, 64, 128):
        raise ValueError("conv3x3s2_mish_x3 needs a dense fp32 (B,H+1,W+1,C) tensor, C in {32,64,128}")
    B, Hp, Wp, _ = x_padded.shape
    H, W = Hp - 1, Wp - 1
    if tuple(taps3.shape) != (3, 9, 2 * ci, ci) or taps3.dtype != torch.bfloat16 or not taps3.is_contiguous() or \
            not taps3.is_cuda or bias.numel() != 2 * ci or bias.dtype != torch.float32:
        raise ValueError("taps3 must be a dense (3,9,{},{}) bfloat16 device tensor, bias fp32 ({})".format(2 * ci, ci, 2 * ci))
    out = torch.empty((B, H // 2, W // 2, 2 * ci), dtype=torch.float32, device=x_padded.device)
    with torch.cuda.device(out.device), _timed("conv3x3s2_mish_x3", (B, H, W, ci)):
        rc = _hip.lib().qpwc_conv3x3s2_mish_x3_fwd(x_padded.data_ptr(), taps3.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                                    B, H, W, ci, _stream(out))
    _hip.check(rc)
    return out


def upconv_taps(weight, dtype=torch.float32):
    """torch ConvTranspose2d weight (C_in, F, 4, 4) -> the (16, F, C_in) layout of qpwc_upconv4x4s2_mish_fwd (fp32) /
    qpwc_upconv4x4s2_mish_f16_fwd (dtype=torch.float16)."""
    return weight.to(dtype).permute(2, 3, 1, 0).reshape(16, weight.shape[1], weight.shape[0]).contiguous()


def upconv4x4s2_mish_into(x_nhwc, taps, bias, dst):
    """Mish(Conv2DTranspose(4x4, stride 2, 'same')(x) + bias) (the decoder's UpConv, non_layers.py:196-210)
    written into channels [0, F) of the dense channels-last buffer dst (B, 2H, 2W, Ctot >= F): the `up` half of
    concat([up, skip]) (pwcnet.py:186-195).  taps from upconv_taps().  Returns dst."""
    _check_tensor("x", x_nhwc)
    _check_tensor("dst", dst)
    if x_nhwc.dtype not in (torch.float32, torch.float16) or dst.dtype != x_nhwc.dtype or not x_nhwc.is_contiguous() or \
            not dst.is_contiguous():
        raise ValueError("upconv4x4s2_mish_into needs dense fp32 / fp16 channels-last tensors of one dtype")
    B, H, W, C = x_nhwc.shape
    x3 = taps.dtype == torch.bfloat16 and taps.dim() == 4     # split_bf16x3(upconv_taps(w)): the bf16x3 arithmetic
    F_ = taps.shape[-2]
    if x3:
        if tuple(taps.shape) != (3, 16, F_, C) or x_nhwc.dtype != torch.float32 or not taps.is_contiguous() or \
                bias.numel() != F_ or bias.dtype != torch.float32:
            raise ValueError("split taps must be (3,16,F,{}) bfloat16 with fp32 tensors, bias fp32 (F)".format(C))
    elif tuple(taps.shape) != (16, F_, C) or taps.dtype != x_nhwc.dtype or not taps.is_contiguous() or \
            bias.numel() != F_ or bias.dtype != torch.float32:
        raise ValueError("taps must be (16,F,{}) of the input's dtype, bias fp32 (F)".format(C))
    if tuple(dst.shape[:3]) != (B, 2 * H, 2 * W) or dst.shape[3] < F_:
        raise ValueError("dst must be (B,2H,2W,Ctot) with Ctot >= F")
    f16 = x_nhwc.dtype == torch.float16
    fn = _hip.lib().qpwc_upconv4x4s2_mish_x3_fwd if x3 else (
        _hip.lib().qpwc_upconv4x4s2_mish_f16_fwd if f16 else _hip.lib().qpwc_upconv4x4s2_mish_fwd)
    with torch.cuda.device(dst.device), _timed("upconv4x4s2_mish_f16" if f16 else "upconv4x4s2_mish", (B, H, W, C, F_)):
        rc = fn(x_nhwc.data_ptr(), taps.data_ptr(), bias.data_ptr(), dst.data_ptr(), B, H, W, C, F_, dst.shape[3],
                _stream(dst))
    _hip.check(rc)
    return dst


def upconv_cat_ok(x_nhwc, taps, skip, dst):
    """Can upconv4x4s2_mish_cat_into() take these?  (F skip channels, 4-element-aligned strides, plain fp32 / fp16 taps)"""
    if taps.dim() != 3 or skip.dim() != 4 or dst.dim() != 4:
        return False
    F_ = taps.shape[1]
    st = skip.stride()
    esz = 16 // skip.element_size()           # elements per 16 bytes (fp32: 4) -- pointers: 16 B (fp32) / 8 B (fp16)
    return (skip.is_cuda and skip.dtype == x_nhwc.dtype == dst.dtype == taps.dtype and skip.shape[3] == F_ and
            dst.shape[3] >= 2 * F_ and st[3] == 1 and st[2] % 4 == 0 and st[1] % 4 == 0 and st[0] % 4 == 0 and
            st[2] >= F_ and st[1] >= skip.shape[2] * st[2] and st[0] >= skip.shape[1] * st[1] and
            skip.data_ptr() % (4 * skip.element_size()) == 0 and esz in (4, 8))


def upconv4x4s2_mish_cat_into(x_nhwc, taps, bias, skip, dst):
    """upconv4x4s2_mish_into() AND the skip half of the decoder's concat in the same launch: channels [0, F) of dst =
    Mish(Conv2DTranspose(x) + bias), channels [F, 2F) = skip (B, 2H, 2W, F; any 4-element-aligned strides, e.g. the interior
    of a zero-bordered encoder buffer) -- concat([UpConv(x), skip]) of pwcnet.py:186-195 without a separate copy launch."""
    _check_tensor("x", x_nhwc)
    _check_tensor("dst", dst)
    _check_tensor("skip", skip)
    B, H, W, C = x_nhwc.shape
    F_ = taps.shape[-2]
    if x_nhwc.dtype not in (torch.float32, torch.float16) or not x_nhwc.is_contiguous() or not dst.is_contiguous():
        raise ValueError("upconv4x4s2_mish_cat_into needs dense fp32 / fp16 channels-last x and dst")
    if tuple(taps.shape) != (16, F_, C) or not taps.is_contiguous() or bias.numel() != F_ or bias.dtype != torch.float32:
        raise ValueError("taps must be (16,F,{}) of the input's dtype, bias fp32 (F)".format(C))
    if tuple(dst.shape[:3]) != (B, 2 * H, 2 * W) or tuple(skip.shape) != (B, 2 * H, 2 * W, F_) or not upconv_cat_ok(x_nhwc, taps, skip, dst):
        raise ValueError("dst must be (B,2H,2W,>=2F), skip (B,2H,2W,F) of the same dtype with 4-element-aligned strides")
    f16 = x_nhwc.dtype == torch.float16
    fn = _hip.lib().qpwc_upconv4x4s2_mish_cat_f16_fwd if f16 else _hip.lib().qpwc_upconv4x4s2_mish_cat_fwd
    st = skip.stride()
    with torch.cuda.device(dst.device), _timed("upconv4x4s2_mish_f16" if f16 else "upconv4x4s2_mish", (B, H, W, C, F_)):
        rc = fn(x_nhwc.data_ptr(), taps.data_ptr(), bias.data_ptr(), skip.data_ptr(), st[0], st[1], st[2], dst.data_ptr(),
                B, H, W, C, F_, dst.shape[3], _stream(dst))
    _hip.check(rc)
    return dst


_UPCONV_C = (64, 128, 256)
_UPCONV_F = (16, 32, 64, 128)


def _upconv_check(x, weight, bias, what):
    """The operand rules of the differentiable transposed convolution / qpwc_upconv4x4s2_bwd -> (B, H, W, C, F); weight
    in the torch layout (C, F, 4, 4) or as its taps (16, F, C)."""
    _grad_operands_check(x, weight, bias, what)
    B, H, W, C = x.shape
    taps = weight.dim() == 3
    F_ = weight.shape[1]
    if C not in _UPCONV_C or F_ not in _UPCONV_F:
        raise ValueError("{}: C {} -> F {} outside {} -> {}".format(what, C, F_, _UPCONV_C, _UPCONV_F))
    want = (16, F_, C) if taps else (C, F_, 4, 4)
    if tuple(weight.shape) != want or (taps and not weight.is_contiguous()) or bias.numel() != F_ or \
            not bias.is_contiguous():
        raise ValueError("{}: weight must hold ({}, F, 4, 4), bias (F)".format(what, C))
    if min(B, H, W) < 1:
        raise ValueError("{}: empty input {}".format(what, tuple(x.shape)))
    return B, H, W, C, F_


def _upconv4x4s2_fwd(x, taps, bias, skip):
    """The forward launches of upconv4x4s2(): exactly those of the no-grad decoder (non_layers.UpConv.cat_skip)."""
    B, H, W, C, F_ = _upconv_check(x, taps, bias, "upconv4x4s2")
    if skip is None:
        return upconv4x4s2_mish_into(x, taps, bias, torch.empty((B, 2 * H, 2 * W, F_), dtype=x.dtype, device=x.device))
    buf = torch.empty((B, 2 * H, 2 * W, F_ + skip.shape[3]), dtype=x.dtype, device=x.device)
    if upconv_cat_ok(x, taps, skip, buf):
        return upconv4x4s2_mish_cat_into(x, taps, bias, skip, buf)
    upconv4x4s2_mish_into(x, taps, bias, buf)
    half = buf[..., F_:]
    if copy_pixels_ok(skip, half):
        copy_pixels(skip, half)
    else:
        half.copy_(skip)
    return buf


def upconv4x4s2_bwd(x_nhwc, taps, bias, grad_out, mish=True, need=(True, True, True)):
    """Gradients of Mish(Conv2DTranspose(4x4, stride 2, 'same')(x) + bias) (fp32, qpwc_upconv4x4s2_bwd); taps from
    upconv_taps().  grad_out = dL/d(out) is a dense (B,2H,2W,Ctot >= F) tensor whose first F channels are used, read in
    place through its pixel stride Ctot (the gradient of the decoder's concat([up, skip]) as it is).  need = (x,
    weight, bias) -> (grad_x (B,H,W,C), grad_taps (16,F,C) in the layout of taps, grad_bias (F)); whatever is not asked
    for comes back as None and its pointer goes in as NULL."""
    B, H, W, C, F_ = _upconv_check(x_nhwc, taps, bias, "upconv4x4s2_bwd")
    if not isinstance(grad_out, torch.Tensor) or not grad_out.is_cuda or grad_out.dtype != torch.float32 or \
            grad_out.dim() != 4 or tuple(grad_out.shape[:3]) != (B, 2 * H, 2 * W) or grad_out.shape[3] < F_ or \
            grad_out.shape[3] % 4:
        raise ValueError("upconv4x4s2_bwd: grad_out must be an fp32 device tensor of shape {} + (Ctot >= {}, "
                         "Ctot % 4 == 0)".format((B, 2 * H, 2 * W), F_))
    if not any(need):
        raise ValueError("upconv4x4s2_bwd: nothing asked for")
    grad_out = grad_out.contiguous()
    dev = x_nhwc.device
    L = _hip.lib()
    ws, outs, ptrs = _bwd_buffers(L.qpwc_upconv4x4s2_bwd_workspace_floats(B, H, W, C, F_),
                                  ((B, H, W, C), (16, F_, C), (F_,)), need, dev)
    with torch.cuda.device(dev), _timed("upconv4x4s2_bwd", (B, H, W, C, F_)):
        rc = L.qpwc_upconv4x4s2_bwd(x_nhwc.data_ptr(), taps.data_ptr(), bias.data_ptr(), grad_out.data_ptr(),
                                    grad_out.shape[3], *ptrs, ws.data_ptr(), B, H, W, C, F_, int(bool(mish)),
                                    _stream(grad_out))
    _hip.check(rc)
    return tuple(outs)


class _UpConvFn(torch.autograd.Function):
    """upconv4x4s2() with qpwc_upconv4x4s2_bwd as its gradient: the forward is the no-grad forward itself; x, weight
    and bias are saved, never the pre-activation (the backward recomputes it) nor the skip (its gradient is a view)."""

    @staticmethod
    def forward(ctx, x, weight, bias, skip):
        _refuse_capture("the transposed convolution")
        out = _upconv4x4s2_fwd(x, upconv_taps(weight), bias, skip)
        ctx.save_for_backward(x, weight, bias)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        _refuse_capture("the transposed-convolution backward")
        x, weight, bias = ctx.saved_tensors
        nig = ctx.needs_input_grad
        C, F_ = weight.shape[0], weight.shape[1]
        grad_out = grad_out.to(torch.float32).contiguous()   # the concat's gradient: its `up` half is read in place
        gx = gw = gb = None
        if nig[0] or nig[1] or nig[2]:
            gx, gt, gb = upconv4x4s2_bwd(x, upconv_taps(weight), bias, grad_out, True, (nig[0], nig[1], nig[2]))
            # the torch layout as a permuted view of the tap-major buffer
            gw = gt.reshape(4, 4, F_, C).permute(3, 2, 0, 1) if gt is not None else None
        gs = grad_out[..., F_:] if nig[3] else None
        return gx, gw, gb.reshape(bias.shape) if gb is not None else None, gs


def upconv4x4s2(x_nhwc, weight, bias, skip=None, matmul="f32"):
    """Mish(Conv2DTranspose(F, 4x4, strides 2, 'same')(x) + bias) of the decoder (qpwcnet/core/non_layers.py:196-210) on
    a dense channels-last fp32 (B,H,W,C) tensor, C in {64,128,256}, F in {16,32,64,128}; weight in the torch layout
    (C, F, 4, 4), bias (F) -> (B,2H,2W,F), or with skip (B,2H,2W,S), S % 4 == 0, the concat([up, skip]) buffer
    (B,2H,2W,F+S) of pwcnet.py:186-195.  The forward is the no-grad decoder's launches: upconv4x4s2_mish_cat_into where
    upconv_cat_ok, else upconv4x4s2_mish_into plus the skip copy.  Differentiable in x, weight, bias and skip: with
    grad enabled and one of them requiring grad the same launches run inside an autograd Function whose backward is
    qpwc_upconv4x4s2_bwd on the concat's gradient in place (grad_skip is a view of it); the result has the bits of the
    no-grad call."""
    if matmul != "f32":
        raise ValueError("upconv4x4s2 computes in fp32 only (matmul={!r}): no bf16x3 path with a gradient".format(matmul))
    for name, t in (("x", x_nhwc), ("weight", weight), ("bias", bias)) + ((("skip", skip),) if skip is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4) or x_nhwc.dim() != 4 or weight.shape[0] != x_nhwc.shape[3]:
        raise ValueError("upconv4x4s2: weight {} does not fit x {}".format(tuple(weight.shape), tuple(x_nhwc.shape)))
    grad = _wants_grad(x_nhwc, weight, bias, skip)
    if grad:
        _refuse_capture("the transposed convolution")
    _upconv_check(x_nhwc, weight, bias, "upconv4x4s2")   # the operand rules, before autograd sees the call
    if skip is not None:
        B, H, W, _ = x_nhwc.shape
        if not skip.is_cuda or skip.dtype != torch.float32 or skip.dim() != 4 or \
                tuple(skip.shape[:3]) != (B, 2 * H, 2 * W) or skip.shape[3] % 4 or skip.shape[3] < 4:
            raise ValueError("upconv4x4s2: skip must be an fp32 device tensor of shape {} + (S, S % 4 == 0), got {} "
                             "{}".format((B, 2 * H, 2 * W), tuple(skip.shape), skip.dtype))
    if grad:
        return _UpConvFn.apply(x_nhwc, weight, bias, skip)
    return _upconv4x4s2_fwd(x_nhwc, upconv_taps(weight), bias, skip)


def bias_mish_pad(x_nhwc, bias, pad_h, pad_w):
    """Mish(x + bias) written into a new (B, H+pad_h, W+pad_w, C) tensor whose border is zero:
    the activation epilogue and TensorFlow's 'SAME' padding of the following stride-2 conv
    (non_layers.py:402-409) in one pass.  Returns the padded tensor."""
    _check_tensor("x", x_nhwc)
    if not x_nhwc.is_contiguous():
        raise ValueError("bias_mish_pad needs a dense channels-last tensor")
    B, H, W, C = x_nhwc.shape
    out = torch.empty((B, H + pad_h, W + pad_w, C), dtype=x_nhwc.dtype, device=x_nhwc.device)
    with torch.cuda.device(x_nhwc.device), _timed("bias_mish_pad", (B, H, W, C)):
        rc = _hip.lib().qpwc_bias_mish_pad_fwd(x_nhwc.data_ptr(), 0 if bias is None else bias.data_ptr(),
                                                out.data_ptr(), B, H, W, C, int(pad_h), int(pad_w), C,
                                                _DTYPES[x_nhwc.dtype], _stream(x_nhwc))
    _hip.check(rc)
    return out


def bias_mish_into(x_nhwc, bias, dst, channel_offset=0):
    """Mish(x + bias) written into channels [offset, offset+C) of the wider dense channels-last
    buffer `dst` (B,H,W,Ctot): one half of the decoder's concat([up, skip]) (pwcnet.py:186-195)
    without the concat copy of that half.  Returns dst."""
    _check_tensor("x", x_nhwc)
    _check_tensor("dst", dst)
    if not (x_nhwc.is_contiguous() and dst.is_contiguous()) or dst.dtype != x_nhwc.dtype:
        raise ValueError("bias_mish_into needs dense channels-last tensors of one dtype")
    B, H, W, C = x_nhwc.shape
    if tuple(dst.shape[:3]) != (B, H, W) or channel_offset % 4 or channel_offset + C > dst.shape[3]:
        raise ValueError("dst must be (B,H,W,Ctot) with room for C channels at a 4-aligned offset")
    es = dst.element_size()
    with torch.cuda.device(dst.device), _timed("bias_mish_into", (B, H, W, C)):
        rc = _hip.lib().qpwc_bias_mish_pad_fwd(x_nhwc.data_ptr(), 0 if bias is None else bias.data_ptr(),
                                                dst.data_ptr() + channel_offset * es, B, H, W, C, 0, 0,
                                                dst.shape[3], _DTYPES[dst.dtype], _stream(dst))
    _hip.check(rc)
    return dst


def split_frames_pad(pairs, pad_h=0, pad_w=0):
    """(B,H,W,6) channels-last input pair -> (2B, H+pad_h, W+pad_w, 3): Split(2) (pwcnet.py:229),
    both frames stacked on the batch axis, far edges zero-padded for the first stride-2 conv."""
    _check_tensor("pairs", pairs)
    if pairs.shape[3] != 6:
        raise ValueError("pairs must be (B,H,W,6)")
    x = pairs.contiguous()
    B, H, W, _ = x.shape
    out = torch.empty((2 * B, H + pad_h, W + pad_w, 3), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _timed("split_frames_pad", (B, H, W, 6)):
        rc = _hip.lib().qpwc_split_frames_pad_fwd(x.data_ptr(), out.data_ptr(), B, H, W, int(pad_h),
                                                   int(pad_w), _DTYPES[x.dtype], _stream(x))
    _hip.check(rc)
    return out

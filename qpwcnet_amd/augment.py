"""Training input pipeline of the reference, batched (qpwcnet/data/augment.py:83-173 ``image_flip_ud``,
``image_flip_lr``, ``image_scale_and_crop``, ``image_resize``, ``image_augment_colors``, ``image_augment``;
qpwcnet/app/optical_flow/train.py:54-94 ``preprocess``, ``preprocess_no_op``).

The reference maps these over single samples on host threads; here a batch goes through at once.  Inputs are
``(B,H,W,6)`` uint8 or float32 frames (two RGB frames per sample) and ``(B,H,W,2)`` float32 flow, dense and
``channels_last`` as decoded frames are.  CUDA tensors run the gfx950 kernels behind ``ops.augment`` (one launch, two
with the colour stage); CPU tensors run ``augment_torch``, the same chain composed from torch operators, which is
also what ``tools/augbench.py`` times against the kernels.  Outputs are float32.

The random draw is separate from the arithmetic: ``sample_params`` returns the per-sample parameters as two device
tensors (``AugmentParams``), which the kernels read from device memory -- no host synchronisation anywhere.

Sparse ground truth (KITTI, Sintel's unknown pixels) goes through ``preprocess_sparse`` / ``preprocess_no_op_sparse`` /
``image_augment_sparse`` / ``image_resize_sparse``: the same frames, the flow resampled over its valid pixels only and
a uint8 ``(B,h,w)`` mask of the output pixels that have a label, what ``loss.multiscale_masked`` and
``metrics.flow_quality`` take as ``valid=`` (``ops.augment_sparse``; ``sparse_torch`` on the CPU).  The reference has
no such path: its pipeline is dense.

The frame interpolator's pipeline is the last part of the module: three ``(B,H,W,3)`` frames per sample through
``preprocess_triplet`` / ``augment_triplet`` (one launch behind ``ops.augment_triplet``; ``triplet_torch`` on the
CPU), with ``sample_triplet_params`` / ``identity_triplet_params`` as its draws.
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .backend import CHANNELS_FIRST, CHANNELS_LAST, get_axis

# iparams (B,6) int32: rh, rw, oy, ox, flip_ud, flip_lr; fparams (B,6) float32: mu, mv, brightness, saturation, hue,
# contrast (include/qpwc.h, qpwc_augment_fwd)
AugmentParams = collections.namedtuple("AugmentParams", "iparams fparams")

SCALE_RANGE = (0.955, 1.05)     # augment.py:119-123, times base_scale
HUE_RANGE = (-0.2, 0.2)         # augment.py:64-67
BRIGHTNESS_RANGE = (-0.125, 0.125)
SATURATION_RANGE = (0.5, 1.5)
CONTRAST_RANGE = (0.5, 1.5)
_INV255 = float(np.float32(1.0 / 255.0))


def scaled_shape(H, W, scale):
    """``tf.cast(tf.cast((H, W), tf.float32) * scale, tf.int32)`` (augment.py:130-131) for a float32 tensor of scales:
    the product is rounded to float32 before it is truncated."""
    scale = torch.as_tensor(scale, dtype=torch.float32)
    hw = torch.tensor([float(H), float(W)], dtype=torch.float32, device=scale.device)
    return (scale.reshape(-1, 1) * hw).to(torch.int32)


def _scale_bounds(base_scale):
    return np.float32(SCALE_RANGE[0] * base_scale), np.float32(SCALE_RANGE[1] * base_scale)


def sample_params(batch, in_shape, out_shape, base_scale=1.0, generator=None, device=None):
    """Draws one sample's parameters per batch entry as the reference does: flips Bernoulli(0.5), scale ~
    U(0.955, 1.05) * base_scale, (rh, rw) = ``scaled_shape``, the crop offset uniform over the windows that fit, hue ~
    U(-0.2, 0.2), brightness ~ U(-0.125, 0.125), saturation and contrast ~ U(0.5, 1.5).  The numbers come from
    ``generator`` (on its own device; the default generator of ``device`` without one) and the result lives on
    ``device``.  ValueError when a scale of the range leaves the resized image smaller than the crop (where TF's
    random_crop asserts)."""
    H, W = (int(v) for v in in_shape)
    h, w = (int(v) for v in out_shape)
    if batch <= 0 or min(H, W, h, w) <= 0:
        raise ValueError("non-positive batch or shape: {} {} {}".format(batch, (H, W), (h, w)))
    lo, hi = _scale_bounds(base_scale)
    min_rh, min_rw = int(np.float32(H) * lo), int(np.float32(W) * lo)
    if min_rh < h or min_rw < w:
        raise ValueError("a {}x{} crop does not fit the smallest resized image {}x{} ({}x{} at scale {:.4f})".format(
            h, w, min_rh, min_rw, H, W, float(lo)))
    device = torch.device("cpu" if device is None else device)
    draw = generator.device if generator is not None else device
    u = torch.rand((int(batch), 9), generator=generator, device=draw, dtype=torch.float32)
    scale = (float(lo) + u[:, 2] * float(hi - lo)).clamp(float(lo), float(hi))
    r = scaled_shape(H, W, scale)
    room = r - torch.tensor([h, w], dtype=torch.int32, device=draw)                  # >= 0 by the check above
    off = torch.minimum((u[:, 3:5] * (room + 1).to(torch.float32)).to(torch.int32), room)
    flip = (u[:, 0:2] < 0.5)
    sign = 1.0 - 2.0 * flip.to(torch.float32)
    uni = lambda col, rng: rng[0] + u[:, col] * (rng[1] - rng[0])
    iparams = torch.cat([r, off, flip.to(torch.int32)], dim=1)
    fparams = torch.stack([scale * sign[:, 1], scale * sign[:, 0], uni(6, BRIGHTNESS_RANGE), uni(7, SATURATION_RANGE),
                           uni(5, HUE_RANGE), uni(8, CONTRAST_RANGE)], dim=1)
    return AugmentParams(iparams.contiguous().to(device), fparams.contiguous().to(device))


def resize_params(batch, in_shape, out_shape, device=None):
    """The parameters of ``image_resize`` (augment.py:145-153): the whole image resized to out_shape, no flips, flow
    times (w / W, h / H).  The colour entries are the identity settings (the colour stage is off for this path)."""
    H, W = (int(v) for v in in_shape)
    h, w = (int(v) for v in out_shape)
    ip = torch.tensor([[h, w, 0, 0, 0, 0]], dtype=torch.int32).repeat(int(batch), 1)
    fp = torch.tensor([[w / W, h / H, 0.0, 1.0, 0.0, 1.0]], dtype=torch.float32).repeat(int(batch), 1)
    return AugmentParams(ip.to(device or "cpu"), fp.to(device or "cpu"))


# ---- the chain composed from torch operators: the CPU path, and the baseline the kernels are timed against ---------
def _rgb_to_hsv(x):
    r, g, b = x.unbind(-1)
    mx, mn = x.amax(-1), x.amin(-1)
    rng = mx - mn
    s = torch.where(mx > 0, rng / mx, torch.zeros_like(mx))
    norm = 1.0 / (6.0 * rng)
    hh = torch.where(r == mx, norm * (g - b),
                     torch.where(g == mx, norm * (b - r) + 2.0 / 6.0, norm * (r - g) + 4.0 / 6.0))
    hh = torch.where(rng > 0, hh, torch.zeros_like(hh))
    hh = torch.where(hh < 0, hh + 1.0, hh)
    nan = torch.isnan(x).any(-1)                     # amax / amin propagate NaN; keep the hue and saturation NaN too
    hh = torch.where(nan, torch.full_like(hh, math.nan), hh)
    return hh, s, mx


def _hsv_to_rgb(hh, s, v):
    dr = ((6.0 * hh - 3.0).abs() - 1.0).clamp(0.0, 1.0)
    dg = (2.0 - (6.0 * hh - 2.0).abs()).clamp(0.0, 1.0)
    db = (2.0 - (6.0 * hh - 4.0).abs()).clamp(0.0, 1.0)
    d = torch.stack([dr, dg, db], dim=-1)
    return ((d - 1.0) * s.unsqueeze(-1) + 1.0) * v.unsqueeze(-1)


def _colours_torch(x, fparams):
    """image_augment_colors on (B,h,w,6): both frames of a sample with that sample's four scalars."""
    B, h, w, _ = x.shape
    x = x.reshape(B, h, w, 2, 3)
    col = lambda i: fparams[:, i].to(x.dtype).reshape(B, 1, 1, 1)
    x = x + col(2).unsqueeze(-1)
    hh, s, v = _rgb_to_hsv(x)
    x = _hsv_to_rgb(hh, (s * col(3)).clamp(0.0, 1.0), v)
    hh, s, v = _rgb_to_hsv(x)
    hh = hh + col(4)
    x = _hsv_to_rgb(hh - torch.floor(hh), s, v)
    mean = x.mean(dim=(1, 2, 3), keepdim=True)       # per colour channel, over the pixels of BOTH frames
    x = (x - mean) * col(5).unsqueeze(-1) + mean
    return x.reshape(B, h, w, 6)


def augment_torch(ims, flo, params, out_shape, colour=True, finish=True, data_format=CHANNELS_LAST):
    """What ``ops.augment`` computes, composed from torch operators on the tensors' own device: flips and crop by
    indexing, ``F.interpolate(mode='bilinear', align_corners=False, antialias=False)`` for the resize (one call when
    (rh, rw) is the same for the whole batch, one per sample otherwise), elementwise operators for the colours.  The
    resized (rh, rw) images are materialised and the sizes are read back to the host, as a composition has to."""
    get_axis(data_format)
    h, w = (int(v) for v in out_shape)
    B = ims.shape[0]
    ip = params.iparams.cpu().tolist()
    fp = params.fparams.to(ims.device)
    x = ims.to(torch.float32) * _INV255 if ims.dtype == torch.uint8 else ims
    x = torch.cat([x, flo], dim=3).permute(0, 3, 1, 2)                       # (B,8,H,W) view
    resize = lambda t, size: F.interpolate(t, size=size, mode="bilinear", align_corners=False, antialias=False)
    if all(row[:2] == ip[0][:2] for row in ip):
        for dim, col in ((2, 4), (3, 5)):
            idx = [b for b in range(B) if ip[b][col]]
            if idx:
                x = x.index_copy(0, torch.tensor(idx, device=x.device), torch.flip(x[idx], [dim]))
        out = resize(x, tuple(ip[0][:2]))
        if all(row[2:4] == ip[0][2:4] for row in ip):
            out = out[:, :, ip[0][2]:ip[0][2] + h, ip[0][3]:ip[0][3] + w]
        else:
            out = torch.stack([out[b, :, r[2]:r[2] + h, r[3]:r[3] + w] for b, r in enumerate(ip)], dim=0)
    else:
        rows = []
        for b, (rh, rw, oy, ox, ud, lr) in enumerate(ip):
            xb = x[b:b + 1]
            dims = [d for d, f in ((2, ud), (3, lr)) if f]
            if dims:
                xb = torch.flip(xb, dims)
            rows.append(resize(xb, (rh, rw))[:, :, oy:oy + h, ox:ox + w])
        out = torch.cat(rows, dim=0)
    out = out.permute(0, 2, 3, 1)
    o_ims, o_flo = out[..., :6], out[..., 6:] * fp[:, None, None, 0:2]
    if colour:
        o_ims = _colours_torch(o_ims, fp)
    if finish:
        o_ims = o_ims - 0.5
        o_ims = torch.where(torch.isnan(o_ims), torch.zeros_like(o_ims), o_ims)
        o_flo = torch.where(torch.isnan(o_flo), torch.zeros_like(o_flo), o_flo)
    if data_format == CHANNELS_FIRST:
        return o_ims.permute(0, 3, 1, 2).contiguous(), o_flo.permute(0, 3, 1, 2).contiguous()
    return o_ims.contiguous(), o_flo.contiguous()


# ---- the reference's names ------------------------------------------------------------------------------------------
def _check_inputs(ims, flo, dtypes):
    for name, t, dt, c in (("ims", ims, dtypes, 6), ("flo", flo, (torch.float32,), 2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if t.dtype not in dt:
            raise ValueError("{}: unsupported dtype {}".format(name, t.dtype))
        if t.dim() != 4 or t.shape[3] != c:
            raise ValueError("{} must be (B,H,W,{}) channels_last, got shape {}".format(name, c, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("{} must be dense (contiguous) channels_last".format(name))
    if tuple(flo.shape[:3]) != tuple(ims.shape[:3]):
        raise ValueError("flo {} does not match ims {}".format(tuple(flo.shape), tuple(ims.shape)))
    if flo.device != ims.device:
        raise ValueError("ims is on {}, flo on {}".format(ims.device, flo.device))


def _check_params(params, B, device):
    if not isinstance(params, AugmentParams):
        params = AugmentParams(*params)
    for name, t, dt in (("iparams", params.iparams, torch.int32), ("fparams", params.fparams, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (B, 6):
            raise ValueError("params.{} must be a ({}, 6) {} tensor".format(name, B, dt))
    return AugmentParams(params.iparams.to(device).contiguous(), params.fparams.to(device).contiguous())


def _run(ims, flo, params, out_shape, colour, finish, data_format):
    if ims.is_cuda:
        return ops.augment(ims, flo, params.iparams, params.fparams, out_shape, colour=colour, finish=finish,
                           data_format=data_format)
    return augment_torch(ims, flo, params, out_shape, colour=colour, finish=finish, data_format=data_format)


def _drawn(ims, out_shape, base_scale, params, generator):
    B, H, W, _ = ims.shape
    if params is None:
        return sample_params(B, (H, W), out_shape, base_scale, generator=generator, device=ims.device)
    return _check_params(params, B, ims.device)


def image_augment(ims, flo, out_shape, base_scale=1.0, params=None, generator=None):
    """augment.py:167-173: flips, scale and crop to out_shape, colours.  float32 frames in [0, 1] in, augmented frames
    (not clipped) and flow out, channels_last.  ``params``: an ``AugmentParams`` (``sample_params``); None draws them
    from ``generator``."""
    _check_inputs(ims, flo, (torch.float32,))
    return _run(ims, flo, _drawn(ims, out_shape, base_scale, params, generator), out_shape, True, False, CHANNELS_LAST)


def image_resize(ims, flo, shape):
    """augment.py:145-153: bilinear resize of frames and flow to ``shape``, flow times (w / W, h / H); channels_last."""
    _check_inputs(ims, flo, (torch.float32,))
    B, H, W, _ = ims.shape
    return _run(ims, flo, resize_params(B, (H, W), shape, ims.device), shape, False, False, CHANNELS_LAST)


def preprocess(ims, flo, data_format=CHANNELS_FIRST, base_scale=1.0, out_shape=(256, 512), params=None,
               generator=None):
    """train.py:71-94: uint8 frames times 1/255 (float32 frames as they are), ``image_augment``, - 0.5, the layout,
    NaN -> 0 in frames and flow."""
    get_axis(data_format)
    _check_inputs(ims, flo, (torch.uint8, torch.float32))
    return _run(ims, flo, _drawn(ims, out_shape, base_scale, params, generator), out_shape, True, True, data_format)


def preprocess_no_op(ims, flo, data_format=CHANNELS_FIRST, out_shape=(256, 512)):
    """train.py:54-68 (the validation path): uint8 frames times 1/255, ``image_resize`` to out_shape, - 0.5, the
    layout; NaN -> 0 as in ``preprocess``."""
    get_axis(data_format)
    _check_inputs(ims, flo, (torch.uint8, torch.float32))
    B, H, W, _ = ims.shape
    return _run(ims, flo, resize_params(B, (H, W), out_shape, ims.device), out_shape, False, True, data_format)


# ---- sparse ground truth (include/qpwc_sparse_augment.h): beyond the reference, whose pipeline is dense ---------------
def _axis_f32(first, n_in, n_resized, count, flip):
    """One axis of the kernels' resampling for `count` output indices from first (B,) on: the fp32 source coordinate
    of ``aug_axis`` (csrc/augment_common.h), every operation separately rounded -> the clamped neighbours lo, hi
    (B,count) int64, mirrored where flip (B,) is set, and the weight t (B,count) float32 of hi."""
    i = (first.reshape(-1, 1) + torch.arange(count, device=first.device, dtype=first.dtype)).to(torch.float32)
    scale = torch.full_like(n_resized, float(n_in), dtype=torch.float32) / n_resized.to(torch.float32)
    s = (i + 0.5) * scale.reshape(-1, 1) - 0.5
    f = torch.floor(s)
    lo, hi = (torch.nan_to_num(v, nan=0.0).clamp(0.0, float(n_in - 1)).to(torch.int64) for v in (f, torch.ceil(s)))
    mirror = (flip != 0).reshape(-1, 1)
    return torch.where(mirror, n_in - 1 - lo, lo), torch.where(mirror, n_in - 1 - hi, hi), s - f


def flow_validity(flo, valid=None):
    """(B,H,W) bool: both components of the (B,H,W,2) flow at most ``metrics.FLOW_UNKNOWN`` in magnitude (false for NaN
    and +-inf) and, with a mask, ``valid != 0``: the rule of the masked losses and the flow scores."""
    from .metrics import FLOW_UNKNOWN
    ok = (flo[..., 0].abs() <= FLOW_UNKNOWN) & (flo[..., 1].abs() <= FLOW_UNKNOWN)
    return ok if valid is None else ok & (valid != 0)


def sparse_torch(ims, flo, valid, params, out_shape, colour=True, finish=True, data_format=CHANNELS_LAST):
    """What ``ops.augment_sparse`` computes, composed from torch operators on the tensors' own device: the CPU path, and
    the baseline tools/sparseaugbench.py times the kernel against.  The frames are ``augment_torch``'s.  The flow's
    corners and weights are the kernel's fp32 values (``_axis_f32``); invalid pixels are zeroed by a select before
    anything reads them; an output pixel with four valid corners takes ``augment_torch``'s flow of the zero-filled
    source (the dense value), one with one to three the weighted sum over the sum of the valid weights, one with none
    zero.  -> (ims, flo, valid), valid uint8 (B,h,w)."""
    get_axis(data_format)
    h, w = (int(v) for v in out_shape)
    B, H, W, _ = ims.shape
    ok = flow_validity(flo, valid)
    flo = torch.where(ok.unsqueeze(-1), flo, torch.zeros((), dtype=flo.dtype, device=flo.device))
    o_ims, dense = augment_torch(ims, flo, params, out_shape, colour=colour, finish=finish, data_format=CHANNELS_LAST)
    ip, fp = params.iparams.to(ims.device), params.fparams.to(ims.device)
    y0, y1, ty = _axis_f32(ip[:, 2], H, ip[:, 0], h, ip[:, 4])
    x0, x1, tx = _axis_f32(ip[:, 3], W, ip[:, 1], w, ip[:, 5])
    ty, tx = ty.reshape(B, h, 1), tx.reshape(B, 1, w)
    ly, lx = (1.0 - ty, ty), (1.0 - tx, tx)
    b = torch.arange(B, device=ims.device).reshape(B, 1, 1)
    zero = torch.zeros((), dtype=torch.float32, device=ims.device)
    S, num, n = None, None, None
    for ky, yy in enumerate((y0, y1)):                                         # corners 00, 01, 10, 11, in this order
        for kx, xx in enumerate((x0, x1)):
            at = (b, yy.reshape(B, h, 1), xx.reshape(B, 1, w))
            v = ok[at]
            wk = torch.where(v, ly[ky] * lx[kx], zero)
            term = wk.unsqueeze(-1) * flo[at]
            S, num, n = (wk, term, v.to(torch.int32)) if S is None else (S + wk, num + term, n + v)
    some = n > 0
    part = num / torch.where(some, S, torch.ones_like(S)).unsqueeze(-1) * fp[:, None, None, 0:2]
    o_flo = torch.where((n == 4).unsqueeze(-1), dense, torch.where(some.unsqueeze(-1), part, zero))
    o_valid = some.to(torch.uint8)
    if data_format == CHANNELS_FIRST:
        return o_ims.permute(0, 3, 1, 2).contiguous(), o_flo.permute(0, 3, 1, 2).contiguous(), o_valid
    return o_ims.contiguous(), o_flo.contiguous(), o_valid


def _run_sparse(ims, flo, valid, params, out_shape, colour, finish, data_format):
    from .metrics import _flow_mask
    valid = _flow_mask("valid", valid, flo, tuple(flo.shape[:3]))
    if ims.is_cuda:
        return ops.augment_sparse(ims, flo, None if valid is None else valid.contiguous(), params.iparams, params.fparams,
                                  out_shape, colour=colour, finish=finish, data_format=data_format)
    return sparse_torch(ims, flo, valid, params, out_shape, colour=colour, finish=finish, data_format=data_format)


def image_augment_sparse(ims, flo, out_shape, valid=None, base_scale=1.0, params=None, generator=None):
    """``image_augment`` for sparse ground truth -> (ims, flo, valid), channels_last: the same frames; the flow over its
    valid pixels only (``flow_validity``; valid: None, bool, uint8 or floating (B,H,W)), exactly 0 where no corner is
    valid; valid uint8 (B,h,w), what ``loss.multiscale_masked`` and ``metrics.flow_quality`` take."""
    _check_inputs(ims, flo, (torch.float32,))
    return _run_sparse(ims, flo, valid, _drawn(ims, out_shape, base_scale, params, generator), out_shape, True, False,
                       CHANNELS_LAST)


def image_resize_sparse(ims, flo, shape, valid=None):
    """``image_resize`` for sparse ground truth -> (ims, flo, valid), channels_last (``image_augment_sparse``)."""
    _check_inputs(ims, flo, (torch.float32,))
    B, H, W, _ = ims.shape
    return _run_sparse(ims, flo, valid, resize_params(B, (H, W), shape, ims.device), shape, False, False, CHANNELS_LAST)


def preprocess_sparse(ims, flo, valid=None, data_format=CHANNELS_FIRST, base_scale=1.0, out_shape=(256, 512),
                      params=None, generator=None):
    """``preprocess`` for sparse ground truth (KITTI, Sintel's unknown pixels) -> (ims, flo, valid): the frames of
    ``preprocess`` bit for bit, the flow in data_format resampled over its valid pixels only -- no false zero next to
    a hole, no blend with a 1e10 "unknown" -- and the uint8 (B,h,w) mask of the output pixels that have a label."""
    get_axis(data_format)
    _check_inputs(ims, flo, (torch.uint8, torch.float32))
    return _run_sparse(ims, flo, valid, _drawn(ims, out_shape, base_scale, params, generator), out_shape, True, True,
                       data_format)


def preprocess_no_op_sparse(ims, flo, valid=None, data_format=CHANNELS_FIRST, out_shape=(256, 512)):
    """``preprocess_no_op`` (the validation path) for sparse ground truth -> (ims, flo, valid) (``preprocess_sparse``)."""
    get_axis(data_format)
    _check_inputs(ims, flo, (torch.uint8, torch.float32))
    B, H, W, _ = ims.shape
    return _run_sparse(ims, flo, valid, resize_params(B, (H, W), out_shape, ims.device), out_shape, False, True,
                       data_format)


# ---- the frame interpolator's triplets (qpwcnet/data/triplet_dataset_ops.py, data/augment.py:10-59,
# app/frame_interpolation/pre_train.py:110-124) ------------------------------------------------------------------------
# iparams (B,4) int32: flip_ud, flip_lr, key0, key1; fparams (B,16) float32: R row-major, scale, txn, sigma
# (include/qpwc_triplet.h, qpwc_augment_triplet_fwd)
TripletParams = collections.namedtuple("TripletParams", "iparams fparams")

_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_M32 = 0xFFFFFFFF


def rotation_matrix_from_euler(x):
    """augment.py:10-25: (..., 3) Euler angles (x, y, z) -> (..., 3, 3) = Rz(z) . Ry(y) . Rx(x)."""
    x = torch.as_tensor(x)
    (cx, cy, cz), (sx, sy, sz) = torch.cos(x).unbind(-1), torch.sin(x).unbind(-1)
    R = [cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz,
         cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz,
         -sy, sx * cy, cx * cy]
    return torch.stack(R, dim=-1).reshape(x.shape[:-1] + (3, 3))


def sample_triplet_params(batch, max_txn=0.3, max_rxn=0.3, max_scale=0.3, noise=0.02, generator=None, device=None):
    """One draw per batch entry as ``augment_triplet(batch_size=B)`` makes it: txn ~ U(-max_txn, max_txn)^3, Euler
    angles ~ U(-max_rxn, max_rxn)^3, scale = exp(U(-max_scale, max_scale))^3, flips Bernoulli(0.5), sigma = noise, and
    two random 32-bit words as the key of the sample's noise field.  The numbers come from ``generator`` (on its own
    device; the default generator of ``device`` without one) and the result lives on ``device``."""
    if batch <= 0:
        raise ValueError("non-positive batch: {}".format(batch))
    device = torch.device("cpu" if device is None else device)
    draw = generator.device if generator is not None else device
    B = int(batch)
    u = torch.rand((B, 11), generator=generator, device=draw, dtype=torch.float32) * 2.0 - 1.0     # U[-1, 1)
    keys = torch.randint(-(1 << 31), 1 << 31, (B, 2), generator=generator, device=draw, dtype=torch.int64)
    R = rotation_matrix_from_euler(u[:, 3:6] * max_rxn).reshape(B, 9)
    sigma = torch.full((B, 1), float(noise), dtype=torch.float32, device=draw)
    fparams = torch.cat([R, torch.exp(u[:, 6:9] * max_scale), u[:, 0:3] * max_txn, sigma], dim=1)
    iparams = torch.cat([(u[:, 9:11] < 0.0).to(torch.int32), keys.to(torch.int32)], dim=1)
    return TripletParams(iparams.contiguous().to(device), fparams.contiguous().to(device))


def identity_triplet_params(batch, device=None):
    """The validation path (``read_triplet_dataset(augment=False)``): R = I, scale 1, txn 0, sigma 0, no flips."""
    fp = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]], dtype=torch.float32).repeat(int(batch), 1)
    return TripletParams(torch.zeros((int(batch), 4), dtype=torch.int32).to(device or "cpu"), fp.to(device or "cpu"))


def _mul32(m, c):
    """(hi, lo) words of the 64-bit product of the 32-bit constant m and int64 tensor c in [0, 2^32), without leaving
    int64: c by 16-bit halves."""
    p, q = m * (c & 0xFFFF), m * (c >> 16)                   # < 2^48 each; the product is (q << 16) + p
    s = p + ((q & 0xFFFF) << 16)
    return (q >> 16) + (s >> 32), s & _M32


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85)
    from integer torch operators, on any device: counter (..., 4) and key (..., 2) integer tensors whose entries are
    taken modulo 2^32 (so int32 bit patterns serve) -> (..., 4) int64 words in [0, 2^32)."""
    c = [t & _M32 for t in torch.as_tensor(counter).to(torch.int64).unbind(-1)]
    k = [t & _M32 for t in torch.as_tensor(key).to(torch.int64).unbind(-1)]
    for _ in range(10):
        hi0, lo0 = _mul32(_PHILOX_M[0], c[0])
        hi1, lo1 = _mul32(_PHILOX_M[1], c[2])
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + _PHILOX_W[0]) & _M32, (k[1] + _PHILOX_W[1]) & _M32]
    return torch.stack(torch.broadcast_tensors(*c), dim=-1)


def triplet_noise(keys, h, w):
    """The noise field of qpwc_augment_triplet_fwd before the flips and before sigma: keys (B,2) integer -> (B,h,w,3)
    float32 standard normals, pixel (y, x) from Philox counter (y * w + x, 0, 0, 0) by Box-Muller on uniforms that are
    exact in fp32 (include/qpwc_triplet.h)."""
    keys = torch.as_tensor(keys)
    B, n = keys.shape[0], int(h) * int(w)
    counter = torch.zeros((1, n, 4), dtype=torch.int64, device=keys.device)
    counter[0, :, 0] = torch.arange(n, device=keys.device)
    r = philox4x32(counter, keys.reshape(B, 1, 2))
    k = 2.0 ** -24
    u1, u2 = ((r[..., 0::2] >> 8) + 1).to(torch.float32) * k, (r[..., 1::2] >> 8).to(torch.float32) * k
    rad = torch.sqrt(-2.0 * torch.log(u1))
    ang = float(np.float32(2.0 * math.pi)) * u2
    z = torch.stack([rad[..., 0] * torch.cos(ang[..., 0]), rad[..., 0] * torch.sin(ang[..., 0]),
                     rad[..., 1] * torch.cos(ang[..., 1])], dim=-1)
    return z.reshape(B, int(h), int(w), 3)


def triplet_torch(a, b, c, params, dsize, finish=True, data_format=CHANNELS_LAST, noise=None):
    """What ``ops.augment_triplet`` computes, composed from torch operators on the tensors' own device, step by step as
    the reference does it: times 1/255, ``F.interpolate(mode='bilinear', align_corners=False, antialias=False)``, the
    colour einsum, the noise field (``triplet_noise``: the same numbers as the kernel's), both flips, - 0.5, concat
    and the layout.  The CPU path.  ``noise``: a callable (B, h, w) -> (B,h,w,3) standard normals to draw the field
    with instead (tools/tripletbench.py times the composition with ``torch.randn``, as the reference would run it)."""
    get_axis(data_format)
    h, w = (int(v) for v in dsize)
    B, H, W, _ = a.shape
    ip, fp = params.iparams.to(a.device), params.fparams.to(a.device)
    x = torch.stack([a, b, c], dim=0)                                          # (3,B,H,W,3)
    x = x.to(torch.float32) * _INV255 if x.dtype == torch.uint8 else x
    if (H, W) != (h, w):
        x = F.interpolate(x.reshape(3 * B, H, W, 3).permute(0, 3, 1, 2), size=(h, w), mode="bilinear",
                          align_corners=False, antialias=False).permute(0, 2, 3, 1).reshape(3, B, h, w, 3)
    per = lambda t: t.reshape(1, B, 1, 1, 3)
    y = torch.einsum("nab,fnhwb->fnhwa", fp[:, 0:9].reshape(B, 3, 3), x) * per(fp[:, 9:12]) + per(fp[:, 12:15])
    z = triplet_noise(ip[:, 2:4], h, w) if noise is None else noise(B, h, w)
    y = y + (fp[:, 15].reshape(B, 1, 1, 1) * z).unsqueeze(0)
    for col, axis in ((0, 2), (1, 3)):
        y = torch.where((ip[:, col] != 0).reshape(1, B, 1, 1, 1), torch.flip(y, [axis]), y)
    if finish:
        y = y - 0.5
    pair, mid = torch.cat([y[0], y[2]], dim=-1), y[1]
    if data_format == CHANNELS_FIRST:
        return pair.permute(0, 3, 1, 2).contiguous(), mid.permute(0, 3, 1, 2).contiguous()
    return pair.contiguous(), mid.contiguous()


def _check_triplet(a, b, c):
    for name, t in (("a", a), ("b", b), ("c", c)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError("{}: unsupported dtype {}".format(name, t.dtype))
        if t.dim() != 4 or t.shape[3] != 3:
            raise ValueError("{} must be (B,H,W,3) channels_last, got shape {}".format(name, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("{} must be dense (contiguous) channels_last".format(name))
        if t.shape != a.shape or t.dtype != a.dtype or t.device != a.device:
            raise ValueError("{} ({}, {}, {}) does not match a ({}, {}, {})".format(
                name, tuple(t.shape), t.dtype, t.device, tuple(a.shape), a.dtype, a.device))


def _triplet_params(params, B, device, generator, augment=True):
    if not augment:
        return identity_triplet_params(B, device)
    if params is None:
        return sample_triplet_params(B, generator=generator, device=device)
    if not isinstance(params, TripletParams):
        params = TripletParams(*params)
    for name, t, dt, n in (("iparams", params.iparams, torch.int32, 4), ("fparams", params.fparams, torch.float32, 16)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (B, n):
            raise ValueError("params.{} must be a ({}, {}) {} tensor".format(name, B, n, dt))
    return TripletParams(params.iparams.to(device).contiguous(), params.fparams.to(device).contiguous())


def _run_triplet(a, b, c, params, dsize, finish, data_format):
    if a.is_cuda:
        return ops.augment_triplet(a, b, c, params.iparams, params.fparams, dsize, finish=finish,
                                   data_format=data_format)
    return triplet_torch(a, b, c, params, dsize, finish=finish, data_format=data_format)


def augment_triplet(a, b, c, dsize, params=None, generator=None):
    """triplet_dataset_ops.py:20-54 on a batch, after read_and_resize's resize to ``dsize``: one colour rotation, scale
    and offset, one noise field and one pair of flips per sample for the three frames -> three (B,h,w,3) float32
    images, channels_last, not offset and not clipped (views of the kernel's two outputs).  ``params``: a
    ``TripletParams`` (``sample_triplet_params``); None draws them from ``generator``."""
    _check_triplet(a, b, c)
    pair, mid = _run_triplet(a, b, c, _triplet_params(params, a.shape[0], a.device, generator), dsize, False,
                             CHANNELS_LAST)
    return pair[..., 0:3], mid, pair[..., 3:6]


def preprocess_triplet(a, b, c, dsize=(256, 512), data_format=CHANNELS_FIRST, augment=True, params=None,
                       generator=None):
    """read_and_resize's conversion and resize, ``augment_triplet`` (augment=False: the validation path, the resize
    alone) and pre_train.py:110-124: uint8 frames times 1/255 (float32 frames as they are), - 0.5, img_pair =
    concat([img0, img2]) -> (img_pair, img1) in data_format, what InterpolatorModel and
    ``loss.multiscale(AutoResizeMseLoss())`` take."""
    get_axis(data_format)
    _check_triplet(a, b, c)
    return _run_triplet(a, b, c, _triplet_params(params, a.shape[0], a.device, generator, augment), dsize, True,
                        data_format)

"""Per-level end-point error, the reduction the benchmark all-gathers.

EPE definition: ``epe_error`` (qpwcnet/app/optical_flow/train.py:247-253);
per-level ground truth as in ``FlowMseLoss.call`` (qpwcnet/train/loss.py:56-62):
bilinear resize of the full-resolution flow to (h, w), times h/H.

Image quality of the frame interpolator: ``image_quality`` (per-image MSE, PSNR and SSIM with tf.image.ssim's defaults),
``psnr`` / ``ssim`` under tf.image's names and ``InterpolationQuality``, the running mean of an evaluation loop
(qpwcnet/app/pre_train.py:71 feeds ``compiled_metrics``; pre_train_test.py:61-77 is the 8-bit export the defaults
score).  HIP tensors take two launches (``qpwc_image_quality_fwd``, include/qpwc_quality.h);
CPU tensors take ``image_quality_torch``, the same chain from torch operators.

Scoring the flow model: ``flow_quality`` (per-image EPE with its matched / unmatched and speed splits, Fl-all, accuracy
at 1 / 3 / 5 px and the average angular error, over the valid pixels) and ``FlowQuality``, the pixel-weighted running
scores of an evaluation loop, optionally summed over the ranks.  HIP tensors take two launches
(``qpwc_flow_quality_fwd``, include/qpwc_flow_quality.h); CPU tensors take
``flow_quality_torch``.
"""
import collections
import math

import torch
import torch.nn.functional as F

from . import _hip, ops
from .backend import CHANNELS_LAST, get_axis, image_data_format


def multiscale_ground_truth(flow_gt, shapes, data_format=CHANNELS_LAST, mode="bilinear"):
    """flow_gt (B,H,W,2) -> list of (B,h,w,2), one per (h,w) in shapes.
    mode 'bilinear': FlowMseLoss's ground truth (F.interpolate, align_corners=False); 'area': FlowMseLossV2's
    (loss.py:160-173, the mean over (H/h) x (W/w) blocks, HIP: every level from one pass over flow_gt).  Both times
    h / H on both channels."""
    if mode == "area":
        return [t.contiguous() for t in ops.area_ground_truth(flow_gt, shapes, data_format)]
    if mode != "bilinear":
        raise ValueError("unknown mode '{}' (bilinear, area)".format(mode))
    x = flow_gt.permute(0, 3, 1, 2) if data_format == CHANNELS_LAST else flow_gt
    H = x.shape[2]
    out = []
    for (h, w) in shapes:
        y = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False) * (h / H)
        out.append(y.permute(0, 2, 3, 1).contiguous() if data_format == CHANNELS_LAST
                   else y.contiguous())
    return out


def per_level_epe(flows_true, flows_pred, data_format=CHANNELS_LAST, out=None):
    """-> float32 tensor [n_levels] on the flows' device (HIP reduction kernel); written into ``out``
    when given (the all-gather payload, see qpwcnet_amd.dist.EpeGather.payload_view)."""
    if len(flows_true) <= 8:
        return ops.epe_multi(flows_true, flows_pred, out=out, data_format=data_format)  # two launches
    res = torch.stack([ops.epe(t, p.float(), data_format) for t, p in zip(flows_true, flows_pred)])
    if out is not None:
        out.copy_(res)
        return out
    return res


ImageQuality = collections.namedtuple("ImageQuality", ["mse", "psnr", "ssim"])

# tf.image.ssim's defaults: the only filter the kernels implement
SSIM_FILTER = {"filter_size": 11, "filter_sigma": 1.5, "k1": 0.01, "k2": 0.03}


def ssim_window():
    """The 11 taps of tf.image.ssim's default Gaussian (sigma 1.5), normalised in float64 and rounded to float32:
    the window is their outer product."""
    k = torch.arange(SSIM_FILTER["filter_size"], dtype=torch.float64) - (SSIM_FILTER["filter_size"] - 1) / 2.0
    e = torch.exp(-k * k / (2.0 * SSIM_FILTER["filter_sigma"] ** 2))
    return (e / e.sum()).float()


def _quality_value(x, offset, max_val, clip, quantize):
    v = x.float() + offset
    if clip:
        v = v.clamp(0.0, max_val)
    if quantize:
        v = torch.trunc(255.0 * v.clamp(0.0, 1.0))
    return v


def image_quality_torch(y_true, y_pred, max_val=1.0, offset=(0.0, 0.0), clip=False, quantize=False,
                        data_format=CHANNELS_LAST):
    """``image_quality`` composed from torch operators, on any device: the path CPU tensors take and the baseline the
    kernels are timed against.  The chain of include/qpwc_quality.h in fp32 -- the value transform, the squared error,
    ``F.conv2d(groups=C)`` along the rows and then the columns with ``ssim_window``, s -- with the means taken in
    float64.  Batched (rank 4) inputs, offset = (truth, pred); -> ImageQuality of float32 [B] tensors."""
    axis = get_axis(data_format)
    max_val = 255.0 if quantize else float(max_val)
    with torch.no_grad():
        vt = _quality_value(y_true.detach(), float(offset[0]), max_val, clip, quantize)
        vp = _quality_value(y_pred.detach(), float(offset[1]), max_val, clip, quantize)
        if axis == 3:
            vt, vp = vt.permute(0, 3, 1, 2), vp.permute(0, 3, 1, 2)
        C = vt.shape[1]
        d = vt - vp
        mse = (d * d).double().mean(dim=(1, 2, 3))
        psnr = 20.0 * math.log10(max_val) - 10.0 * torch.log10(mse)          # +inf for mse == 0
        g = ssim_window().to(vt.device)
        rows, cols = g.view(1, 1, 1, -1).repeat(C, 1, 1, 1), g.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
        conv = lambda x: F.conv2d(F.conv2d(x.contiguous(), rows, groups=C), cols, groups=C)
        c1 = float(torch.tensor((SSIM_FILTER["k1"] * max_val) ** 2, dtype=torch.float64).float())
        c2 = float(torch.tensor((SSIM_FILTER["k2"] * max_val) ** 2, dtype=torch.float64).float())
        mt, mp = conv(vt), conv(vp)
        num0, den0 = 2.0 * mt * mp, mt * mt + mp * mp
        num1, den1 = 2.0 * conv(vt * vp), conv(vt * vt + vp * vp)
        s = (num0 + c1) / (den0 + c1) * ((num1 - num0 + c2) / (den1 - den0 + c2))
        ssim_ = s.double().mean(dim=(2, 3)).mean(dim=1)
        return ImageQuality(mse.float(), psnr.float(), ssim_.float())


def _check_images(y_true, y_pred, data_format):
    for name, t in (("y_true", y_true), ("y_pred", y_pred)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
        if t.dtype not in (torch.float32, torch.float16):
            raise ValueError("{}: unsupported dtype {}".format(name, t.dtype))
    if y_true.shape != y_pred.shape or y_true.device != y_pred.device:
        raise ValueError("y_true {} on {} and y_pred {} on {} must have one shape and one device".format(
            tuple(y_true.shape), y_true.device, tuple(y_pred.shape), y_pred.device))
    if y_true.dim() not in (3, 4):
        raise ValueError("images must be of rank 3 or 4, got shape {}".format(tuple(y_true.shape)))
    shape = tuple(y_true.shape[-3:])
    H, W, C = shape if data_format == CHANNELS_LAST else (shape[1], shape[2], shape[0])
    if not 1 <= C <= 4:
        raise ValueError("images must have 1..4 channels, got {} ({}, shape {})".format(C, data_format,
                                                                                        tuple(y_true.shape)))
    if H < SSIM_FILTER["filter_size"] or W < SSIM_FILTER["filter_size"]:
        raise ValueError("images of {}x{} are smaller than the SSIM filter size {}".format(H, W,
                                                                                           SSIM_FILTER["filter_size"]))


def image_quality(y_true, y_pred, max_val=1.0, offset=0.0, clip=False, quantize=False, data_format=None, state=None):
    """Per-image MSE, PSNR (tf.image.psnr) and SSIM (tf.image.ssim with its defaults: filter_size 11, filter_sigma 1.5,
    k1 0.01, k2 0.03) of ``y_pred`` against ``y_true``: (B,H,W,C) / (B,C,H,W) by ``data_format`` (default
    ``backend.image_data_format()``) or one image of rank 3, one shape, each fp32 or fp16, 1..4 channels, H, W >= 11.
    ``offset`` (a number, or a (truth, pred) pair) is added first; ``clip`` then clamps to [0, max_val]; ``quantize``
    scores the 8-bit pictures ``trunc(255 * clip(x + offset, 0, 1))`` of pre_train_test.py's export with max_val = 255.
    -> ImageQuality(mse, psnr, ssim) of float32 [B] tensors on the inputs' device (scalars for one image); psnr is
    +inf where the images are equal.  ``state``: a float64 tensor of 4 elements on the same device, to which the call
    adds its sums of mse, psnr, ssim and its image count (``InterpolationQuality`` holds one).  No gradient flows.
    HIP tensors: two launches, no host synchronisation."""
    if data_format is None:
        data_format = image_data_format()
    get_axis(data_format)
    _check_images(y_true, y_pred, data_format)
    off_t, off_p = (offset if isinstance(offset, (tuple, list)) else (offset, offset))
    off_t, off_p = float(off_t), float(off_p)
    max_val = 255.0 if quantize else float(max_val)
    if not (math.isfinite(max_val) and max_val > 0.0 and math.isfinite(off_t) and math.isfinite(off_p)):
        raise ValueError("max_val must be finite and > 0 and the offsets finite, got {} and {}".format(
            max_val, (off_t, off_p)))
    if state is not None and not (isinstance(state, torch.Tensor) and state.dtype == torch.float64
                                  and state.numel() == 4 and state.device == y_true.device):
        raise ValueError("state must be a float64 tensor of 4 elements on {}".format(y_true.device))
    single = y_true.dim() == 3
    with torch.no_grad():
        t, p = y_true.detach(), y_pred.detach()
        if single:
            t, p = t[None], p[None]
        if t.is_cuda:
            flags = (_hip.QUALITY_CLIP if clip else 0) | (_hip.QUALITY_U8 if quantize else 0)
            res = ImageQuality(*ops.image_quality(t, p, data_format, (off_t, off_p), flags, max_val, state))
        else:
            res = image_quality_torch(t, p, max_val, (off_t, off_p), clip, quantize, data_format)
            if state is not None:
                # image by image, in float64, as the fold kernel adds them
                flat = state.view(-1)
                for i, v in enumerate(res):
                    flat[i] = torch.cumsum(torch.cat([flat[i:i + 1], v.double()]), 0)[-1]
                flat[3] += float(t.shape[0])
    return ImageQuality(*(v[0] for v in res)) if single else res


def psnr(a, b, max_val, data_format=None):
    """tf.image.psnr(a, b, max_val): float32 [B] (a scalar for rank 3), +inf where the images are equal."""
    return image_quality(a, b, max_val=max_val, data_format=data_format).psnr


def ssim(a, b, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, data_format=None):
    """tf.image.ssim(a, b, max_val) with its default filter, the only one implemented: any other filter_size,
    filter_sigma, k1 or k2 raises ValueError."""
    given = {"filter_size": filter_size, "filter_sigma": filter_sigma, "k1": k1, "k2": k2}
    if given != SSIM_FILTER:
        raise ValueError("ssim supports only tf.image.ssim's defaults {}, got {}".format(
            SSIM_FILTER, {k: v for k, v in given.items() if v != SSIM_FILTER[k]}))
    return image_quality(a, b, max_val=max_val, data_format=data_format).ssim


class InterpolationQuality:
    """Running MSE, PSNR and SSIM of an evaluation loop -- the metric ``pre_train.py`` hands to ``compile``.  The
    defaults score ``model(img_pair)[-1]`` against ``img1`` as ``pre_train.preprocess`` leaves them, both in
    [-0.5, 0.5], as the 8-bit pictures of pre_train_test.py's export (offset 0.5, quantize).  The four float64 sums
    live on the inputs' device and ``update_state`` reads nothing back: ``result()`` does the one host read."""

    def __init__(self, offset=0.5, quantize=True, data_format=None):
        self.offset, self.quantize, self.data_format = offset, quantize, data_format
        self.state = None

    def update_state(self, y_true, y_pred):
        if self.state is None or self.state.device != y_true.device:
            if self.state is not None and float(self.state[3]) != 0.0:
                raise ValueError("InterpolationQuality holds sums on {}; got images on {}".format(self.state.device,
                                                                                                  y_true.device))
            self.state = torch.zeros(4, dtype=torch.float64, device=y_true.device)
        return image_quality(y_true, y_pred, offset=self.offset, quantize=self.quantize, data_format=self.data_format,
                             state=self.state)

    def result(self):
        """{'mse', 'psnr', 'ssim'}: the means over every image seen since the last reset (0.0 before the first)."""
        sums = [0.0] * 4 if self.state is None else self.state.cpu().tolist()
        n = sums[3]
        return {k: (v / n if n else 0.0) for k, v in zip(ImageQuality._fields, sums)}

    def reset_state(self):
        if self.state is not None:
            self.state.zero_()


# ---- scoring the flow model -------------------------------------------------------------------------------------------
FlowScores = collections.namedtuple("FlowScores", ["epe", "aae", "fl", "acc1", "acc3", "acc5", "epe_noc", "epe_occ",
                                                   "epe_s0_10", "epe_s10_40", "epe_s40", "valid"])

# (numerator, denominator) of every FlowScores field but `valid`, as indices into the 15 sums of
# include/qpwc_flow_quality.h; epe_noc is (sum e - sum e (occluded)) / (n_valid - n_occ)
_FLOW_RATIOS = ((1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), None, (8, 7), (10, 9), (12, 11), (14, 13))
FLOW_UNKNOWN = 1e9      # a ground-truth component above it in magnitude marks the pixel unknown (the .flo convention)


def _flow_scores(sums, pixels):
    """FlowScores' twelve values from float64 sums [..., 15] and a pixel count, in float64; 0 / 0 is NaN."""
    vals = []
    for r in _FLOW_RATIOS:
        num, den = (sums[..., 1] - sums[..., 8], sums[..., 0] - sums[..., 7]) if r is None else (sums[..., r[0]],
                                                                                                 sums[..., r[1]])
        vals.append(num / den)
    vals.append(sums[..., 0] / pixels)
    return vals


def _flow_f32(*groups):
    """The thresholds as the kernel receives them: rounded to float32."""
    return [[float(torch.tensor(float(x), dtype=torch.float32)) for x in g] for g in groups]


def _flow_sums_torch(t, p, valid, occluded, outlier, accuracy, speed, axis):
    """float64 [B, 15]: the per-image sums of include/qpwc_flow_quality.h from torch operators, fp32 per pixel."""
    t, p = t.float(), p.float()
    u, v, up, vp = t.select(axis, 0), t.select(axis, 1), p.select(axis, 0), p.select(axis, 1)
    du, dv = u - up, v - vp
    sq = du * du + dv * dv
    e, m, c = torch.sqrt(sq), torch.sqrt(u * u + v * v), u * vp - v * up
    ang = torch.atan2(torch.sqrt(sq + c * c), (u * up + v * vp) + 1.0) * float(torch.tensor(180.0 / math.pi).float())
    ok = (u.abs() <= FLOW_UNKNOWN) & (v.abs() <= FLOW_UNKNOWN)           # false for NaN and +-inf
    if valid is not None:
        ok = ok & (valid != 0)
    occ = torch.zeros_like(ok) if occluded is None else ok & (occluded != 0)
    zero = torch.zeros((), dtype=torch.float32, device=t.device)
    e, ang = torch.where(ok, e, zero), torch.where(ok, ang, zero)
    b0, b2 = ok & (m < speed[0]), ok & (m >= speed[1])
    b1 = ok & ~b0 & ~b2
    count = lambda mask: mask.sum(dim=(1, 2)).double()
    total = lambda x, mask=None: (x if mask is None else torch.where(mask, x, zero)).double().sum(dim=(1, 2))
    cols = [count(ok), total(e), total(ang), count(ok & (e > outlier[0]) & (e > outlier[1] * m))]
    cols += [count(ok & (e < a)) for a in accuracy]
    cols += [count(occ), total(e, occ)]
    for b in (b0, b1, b2):
        cols += [count(b), total(e, b)]
    return torch.stack(cols, dim=1)


def flow_quality_torch(y_true, y_pred, valid=None, occluded=None, outlier=(3.0, 0.05), accuracy=(1.0, 3.0, 5.0),
                       speed=(10.0, 40.0), data_format=CHANNELS_LAST):
    """``flow_quality`` composed from torch operators, on any device: the path CPU tensors take and the baseline the
    kernels are timed against.  The chain of include/qpwc_flow_quality.h in fp32 per pixel, with the sums taken in
    float64.  Batched (rank 4) inputs, masks (B,H,W) of any dtype (``!= 0``) or None; -> FlowScores of float32 [B]
    tensors."""
    axis = get_axis(data_format)
    H, W = (y_true.shape[1], y_true.shape[2]) if axis == 3 else (y_true.shape[2], y_true.shape[3])
    with torch.no_grad():
        sums = _flow_sums_torch(y_true.detach(), y_pred.detach(), valid, occluded, *_flow_f32(outlier, accuracy, speed),
                                axis)
        return FlowScores(*(x.float() for x in _flow_scores(sums, float(H * W))))


def _flow_thresholds(outlier, accuracy, speed):
    try:
        outlier, accuracy, speed = (tuple(float(x) for x in g) for g in (outlier, accuracy, speed))
    except TypeError:
        raise TypeError("outlier, accuracy and speed must be sequences of numbers")
    if len(outlier) != 2 or len(accuracy) != 3 or len(speed) != 2:
        raise ValueError("outlier takes 2 values (pixels, share), accuracy 3 thresholds and speed 2 bin edges, got "
                         "{}, {} and {}".format(outlier, accuracy, speed))
    if not all(math.isfinite(x) for x in outlier + accuracy + speed):
        raise ValueError("outlier, accuracy and speed must be finite, got {}, {} and {}".format(outlier, accuracy, speed))
    if not (outlier[0] > 0.0 and outlier[1] >= 0.0):
        raise ValueError("outlier = (pixels > 0, share >= 0), got {}".format(outlier))
    if not 0.0 < accuracy[0] < accuracy[1] < accuracy[2]:
        raise ValueError("accuracy must be three rising thresholds above 0, got {}".format(accuracy))
    if not 0.0 < speed[0] < speed[1]:
        raise ValueError("speed must be two rising bin edges above 0, got {}".format(speed))
    return outlier, accuracy, speed


def _flow_mask(name, m, like, dims):
    """A (B,H,W) mask as uint8 on the flows' device: bool and uint8 are reinterpreted, a floating mask takes the one
    ``!= 0`` launch."""
    if m is None:
        return None
    if not isinstance(m, torch.Tensor):
        raise TypeError("{} must be a torch.Tensor or None".format(name))
    if tuple(m.shape) != dims:
        raise ValueError("{} must have shape {}, got {}".format(name, dims, tuple(m.shape)))
    if m.device != like.device:
        raise ValueError("{} is on {}; the flows are on {}".format(name, m.device, like.device))
    if m.dtype == torch.uint8:
        return m
    if m.dtype == torch.bool:
        return m.view(torch.uint8)
    if m.is_floating_point():
        return (m != 0).view(torch.uint8)
    raise TypeError("{} must be bool, uint8 or floating, got {}".format(name, m.dtype))


def flow_quality(y_true, y_pred, valid=None, occluded=None, outlier=(3.0, 0.05), accuracy=(1.0, 3.0, 5.0),
                 speed=(10.0, 40.0), data_format=None, state=None):
    """The figures a flow model is judged by, per image, over the valid pixels: ``y_true`` (float32) and ``y_pred``
    (float32 or float16) are (B,H,W,2) / (B,2,H,W) by ``data_format`` (default ``backend.image_data_format()``) or one
    flow of rank 3.  A pixel is valid where both ground-truth components are finite and at most 1e9 in magnitude (the
    .flo "unknown" convention) and ``valid`` -- bool, uint8 or floating, (B,H,W), ``!= 0`` -- allows it.
    -> FlowScores of float32 [B] tensors on the inputs' device (scalars for one flow):
      epe, aae       mean end-point error (pixels) and mean angular error (degrees, between (u, v, 1) and (u', v', 1))
      fl             KITTI Fl-all: the share with error > outlier[0] pixels and > outlier[1] of the ground-truth speed
      acc1/3/5       the share with error below accuracy[0..2] pixels
      epe_noc/_occ   Sintel's matched / unmatched split by ``occluded`` (a mask like ``valid``, or "estimate":
                     ``occlusion.estimate_occlusion_map(y_true)``); without one epe_noc == epe and epe_occ is NaN
      epe_s0_10 ...  mean end-point error by ground-truth speed: below speed[0], up to speed[1], from speed[1]
      valid          the share of valid pixels
    A mean over an empty set is NaN.  ``state``: a float64 tensor of 17 elements on the same device, to which the call
    adds its 15 sums, its image count and its pixel count (``FlowQuality`` holds one).  No gradient flows.  HIP
    tensors: two launches (one more to convert a floating mask), no host synchronisation; CPU tensors:
    ``flow_quality_torch``."""
    if data_format is None:
        data_format = image_data_format()
    axis = get_axis(data_format)
    for name, t in (("y_true", y_true), ("y_pred", y_pred)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a torch.Tensor".format(name))
    if y_true.dtype != torch.float32:
        raise ValueError("y_true must be float32, got {}".format(y_true.dtype))
    if y_pred.dtype not in (torch.float32, torch.float16):
        raise ValueError("y_pred: unsupported dtype {}".format(y_pred.dtype))
    if y_true.shape != y_pred.shape or y_true.device != y_pred.device:
        raise ValueError("y_true {} on {} and y_pred {} on {} must have one shape and one device".format(
            tuple(y_true.shape), y_true.device, tuple(y_pred.shape), y_pred.device))
    if y_true.dim() not in (3, 4):
        raise ValueError("flows must be of rank 3 or 4, got shape {}".format(tuple(y_true.shape)))
    single = y_true.dim() == 3
    shape = tuple(y_true.shape[-3:])
    H, W, C = shape if axis == 3 else (shape[1], shape[2], shape[0])
    if C != 2 or H < 1 or W < 1 or (not single and y_true.shape[0] < 1):
        raise ValueError("flows must have 2 channels and no empty extent, got shape {} ({})".format(
            tuple(y_true.shape), data_format))
    outlier, accuracy, speed = _flow_thresholds(outlier, accuracy, speed)
    if state is not None and not (isinstance(state, torch.Tensor) and state.dtype == torch.float64
                                  and state.numel() == 17 and state.device == y_true.device):
        raise ValueError("state must be a float64 tensor of 17 elements on {}".format(y_true.device))
    estimate = isinstance(occluded, str)
    if estimate and occluded != "estimate":
        raise ValueError("occluded must be a mask, None or 'estimate', got '{}'".format(occluded))
    with torch.no_grad():
        t, p = y_true.detach(), y_pred.detach()
        if single:
            t, p = t[None], p[None]
            valid, occluded = (m[None] if isinstance(m, torch.Tensor) and m.dim() == 2 else m for m in (valid, occluded))
        dims = (int(t.shape[0]), int(H), int(W))
        if estimate:
            from . import occlusion
            occluded = occlusion.estimate_occlusion_map(t, data_format)
        valid, occluded = _flow_mask("valid", valid, t, dims), _flow_mask("occluded", occluded, t, dims)
        if t.is_cuda:
            res = FlowScores(*ops.flow_quality(t, p, valid, occluded, data_format, outlier, accuracy, speed, state))
        else:
            sums = _flow_sums_torch(t, p, valid, occluded, *_flow_f32(outlier, accuracy, speed), axis)
            res = FlowScores(*(x.float() for x in _flow_scores(sums, float(H * W))))
            if state is not None:
                # image by image, in float64, as the fold kernel adds them
                flat = state.view(-1)
                flat[:15] = torch.cumsum(torch.cat([flat[None, :15], sums]), 0)[-1]
                flat[15] += float(dims[0])
                flat[16] += float(dims[0] * H * W)
    return FlowScores(*(v[0] for v in res)) if single else res


class FlowQuality:
    """Running flow scores of an evaluation loop -- what stands in for ``epe_error`` as a ``compile`` metric
    (qpwcnet/app/optical_flow/train.py:247-253, 299, 374).  ``update_state`` returns the per-image FlowScores and adds
    the batch's 15 sums, images and pixels to 17 float64 numbers on the inputs' device, reading nothing back;
    ``result()`` does the one host read and gives the pixel-weighted means over everything seen -- totals over totals,
    the Sintel / KITTI convention, not means of per-image means."""

    def __init__(self, outlier=(3.0, 0.05), accuracy=(1.0, 3.0, 5.0), speed=(10.0, 40.0), occluded=None,
                 data_format=None):
        if occluded not in (None, "estimate"):
            raise ValueError("occluded must be None or 'estimate' (a mask goes to update_state), got {!r}".format(occluded))
        self.outlier, self.accuracy, self.speed = _flow_thresholds(outlier, accuracy, speed)
        self.occluded, self.data_format = occluded, data_format
        self.state = None

    def update_state(self, y_true, y_pred, valid=None, occluded=None):
        if self.state is None or self.state.device != y_true.device:
            if self.state is not None and float(self.state[15]) != 0.0:
                raise ValueError("FlowQuality holds sums on {}; got flows on {}".format(self.state.device, y_true.device))
            self.state = torch.zeros(17, dtype=torch.float64, device=y_true.device)
        return flow_quality(y_true, y_pred, valid=valid, occluded=self.occluded if occluded is None else occluded,
                            outlier=self.outlier, accuracy=self.accuracy, speed=self.speed,
                            data_format=self.data_format, state=self.state)

    def result(self, all_reduce=False):
        """{the twelve FlowScores fields, 'images', 'pixels'}: pixel-weighted means over every flow seen since the last
        reset, 0.0 everywhere before the first; afterwards a mean over an empty set is NaN.  all_reduce: with an
        initialised ``torch.distributed`` group, a copy of the 17 sums is first summed over the ranks -- every entry is
        additive, so every rank gets the whole dataset's scores."""
        state = torch.zeros(17, dtype=torch.float64) if self.state is None else self.state
        if all_reduce:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                state = state.clone()
                dist.all_reduce(state)
        sums = state.cpu()
        images, pixels = float(sums[15]), float(sums[16])
        if images == 0.0:
            return dict({k: 0.0 for k in FlowScores._fields}, images=0.0, pixels=0.0)
        vals = [float(x) for x in _flow_scores(sums[:15], pixels)]
        return dict(zip(FlowScores._fields, vals), images=images, pixels=pixels)

    def reset_state(self):
        if self.state is not None:
            self.state.zero_()

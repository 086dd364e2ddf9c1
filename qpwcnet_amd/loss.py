"""Training losses of the reference (qpwcnet/train/loss.py) on the gfx950 HIP kernels behind ``qpwc_loss_fwd`` /
``qpwc_loss_bwd``: ``FlowMseLossV2``, ``FlowMseLoss``, ``FlowMseLossFineTune``, ``AutoResizeMseLoss``.

Same class names, constructor arguments and ``loss(y_true, y_pred)`` call as the reference's Keras losses; each call
returns a 0-dim fp32 tensor, differentiable in ``y_pred``.  ``multiscale(loss, y_true, y_preds)`` is the trainer's
``[l(flo, o) for o in pred_flows[:-1]]`` + ``sum(...)`` (qpwcnet/app/optical_flow/train.py:98-122) with every level
in one forward launch (plus a fixed-order fold) and one backward launch.

``y_true``: the full-resolution fp32 ground truth, never differentiated (a ``y_true`` that requires grad is refused);
``y_pred``: fp32 or fp16 (the fp16-storage network's flows), gradients come back in its dtype.  Both layouts are read
as they are.  No CPU path.  Keras' ``sample_weight`` / ``reduction`` are not supported.

``multiscale_masked`` / ``masked_ground_truth`` are the valid-masked twins of the three flow losses for sparse ground
truth (below; include/qpwc_masked_loss.h); they do have a torch chain, taken for CPU tensors.

``PhotometricLoss`` / ``multiscale_unsupervised`` are the label-free losses (census or Charbonnier photometric term plus
edge-aware smoothness; include/qpwc_unsup_loss.h), which go beyond the reference as well.

``ImageLoss`` / ``multiscale_image`` are the frame interpolator's SSIM + Charbonnier loss against AutoResizeMseLoss's own
per-level target (at the end of this file; include/qpwc_image_loss.h), beyond the reference too.
"""
import torch

from . import _hip, metrics, ops
from .backend import CHANNELS_FIRST, get_axis, image_data_format


class _Loss:
    """Keras ``Loss`` surface: ``loss(y_true, y_pred)``, ``call``, ``get_config`` / ``from_config``."""
    kind = None

    def __init__(self, name=None):
        self.name = name
        self._config = {}

    def _params(self):
        return 0.0, 0.0

    def __call__(self, y_true, y_pred):
        return multiscale(self, y_true, [y_pred])[1].reshape(())

    def call(self, y_true, y_pred):
        return self(y_true, y_pred)

    def get_config(self):
        cfg = {"name": self.name}
        cfg.update(self._config)
        return cfg

    @classmethod
    def from_config(cls, config):
        return cls(**config)


def _no_extra(args, kwargs):
    if args or kwargs:
        # Keras' Loss.__init__ rejects unknown arguments as well; reduction / sample_weight are not supported here
        raise TypeError("unexpected arguments: {} {}".format(args, sorted(kwargs)))


class FlowMseLossV2(_Loss):
    """qpwcnet/train/loss.py:134-174: ground truth = mean over sh x sw blocks (einops.reduce) times h / H, then
    Keras ``Huber(0.1)`` of ``s * y_true`` and ``s * y_pred`` with s = 2 / (w + h).  Layout from
    ``image_data_format()`` at construction.  H % h and W % w must be 0 (ValueError, as einops fails)."""
    kind = _hip.LOSS_FLOW_MSE_V2
    delta = 0.1

    def __init__(self, *args, name=None, **kwargs):
        _no_extra(args, kwargs)
        super().__init__(name)
        self.data_format = image_data_format()
        self.axis = get_axis(self.data_format)

    def _params(self):
        return self.delta, 0.0


class FlowMseLoss(_Loss):
    """qpwcnet/train/loss.py:25-82: ground truth = tf.image.resize (bilinear, half-pixel centres) times h / H; the
    mean over pixels of ||y_true - y_pred||_2 over the channel axis.  The gradient at a zero residual is 0."""
    kind = _hip.LOSS_FLOW_MSE

    def __init__(self, data_format=CHANNELS_FIRST, *args, name=None, **kwargs):
        _no_extra(args, kwargs)
        super().__init__(name)
        self._config = {"data_format": data_format}
        self.data_format = data_format
        self.axis = get_axis(data_format)


class FlowMseLossFineTune(_Loss):
    """qpwcnet/train/loss.py:85-131: bilinear ground truth as FlowMseLoss; the mean over pixels of
    (||y_true - y_pred||_1 + eps)^q (the L1 norm's gradient with sign(0) = 0)."""
    kind = _hip.LOSS_FLOW_FINETUNE

    def __init__(self, data_format=CHANNELS_FIRST, q=0.4, eps=0.01, *args, name=None, **kwargs):
        _no_extra(args, kwargs)
        super().__init__(name)
        self.data_format = data_format
        self.axis = get_axis(data_format)
        self.q = q
        self.eps = eps
        # the reference stores this as `config_` and its get_config reads `_config` (an AttributeError there)
        self._config = {"data_format": data_format, "q": q, "eps": eps}

    def _params(self):
        return float(self.q), float(self.eps)


class AutoResizeMseLoss(_Loss):
    """qpwcnet/train/loss.py:177-197: y_true resized bilinearly to y_pred's (h, w) -- no flow scale, any channel count
    (the interpolator's images) -- then Keras ``MeanSquaredError``.  Layout from ``image_data_format()``."""
    kind = _hip.LOSS_AUTORESIZE_MSE

    def __init__(self, *args, name=None, **kwargs):
        _no_extra(args, kwargs)
        super().__init__(name)
        self.data_format = image_data_format()
        self.axis = get_axis(self.data_format)


def multiscale(loss, y_true, y_preds):
    """``[loss(y_true, o) for o in y_preds]`` and their sum for 1..8 predictions in one fused pass -> (total,
    per_level): per_level an fp32 device vector [L] (what autograd differentiates), total = per_level.sum()."""
    if not isinstance(loss, _Loss):
        raise TypeError("multiscale takes one of the qpwcnet_amd.loss classes, got {}".format(type(loss).__name__))
    p0, p1 = loss._params()
    per_level = ops.loss(loss.kind, y_true, list(y_preds), loss.data_format, p0, p1)
    return per_level.sum(), per_level


# ---- the flow losses over the valid pixels only (include/qpwc_masked_loss.h) ------------------------------------------
# For sparse ground truth (KITTI) and unknown pixels (Sintel); the reference has no such loss.  A pixel is valid iff both
# components of y_true are at most metrics.FLOW_UNKNOWN in magnitude (false for NaN and +-inf) and the optional mask
# allows it; an invalid pixel is selected out, never multiplied by 0.  Per level pixel:
#   FlowMseLossV2 (area):    valid iff its sh x sw block has a valid pixel; ground truth = the mean over the block's valid
#                            pixels, times h / H;
#   FlowMseLoss / FineTune:  the four bilinear corners with their fp32 weights; valid iff the valid corners' weights sum
#                            to S > 0; ground truth = their weighted sum / S, times h / H.
# The per-pixel term is the dense loss's; loss_l = sum of the valid terms / max(count_l, 1) (FlowMseLossV2: over twice
# that, the mean over elements).  HIP tensors take qpwc_masked_loss_fwd / _bwd; CPU tensors take the torch chain below.

def _masked_args(loss, y_true, valid):
    """-> (y_true, uint8 mask or None) after the checks both paths share."""
    if not isinstance(loss, _Loss) or loss.kind == _hip.LOSS_AUTORESIZE_MSE:
        raise TypeError("the masked losses take FlowMseLossV2, FlowMseLoss or FlowMseLossFineTune, got {}".format(
            type(loss).__name__))
    if not isinstance(y_true, torch.Tensor):
        raise TypeError("y_true must be a torch.Tensor")
    if y_true.dim() != 4 or y_true.shape[loss.axis] != 2:
        raise ValueError("y_true must be a batched 2-channel flow ({}), got shape {}".format(loss.data_format,
                                                                                            tuple(y_true.shape)))
    dims = tuple(int(v) for i, v in enumerate(y_true.shape) if i != loss.axis)
    return metrics._flow_mask("valid", valid, y_true, dims)


def _axis_weights(n_out, n_in):
    """The two source indices and fp32 weights of every output position along one axis, as the kernel forms them: every
    product and sum separately rounded in float32."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    f = (scale * (torch.arange(n_out, dtype=torch.float32) + 0.5) - 0.5).clamp(min=0.0)
    i0 = f.floor().long()
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = f - i0.float()
    return i0, i1, 1.0 - l1, l1


def _masked_level_torch(loss, x, ok, h, w):
    """(ground truth (B,h,w,2) with 0 where it has none, validity (B,h,w) bool) of one level from the channels-last flow
    x with its invalid pixels already zeroed and the full-resolution validity ok, in x's dtype."""
    B, H, W, _ = x.shape
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    if loss.kind == _hip.LOSS_FLOW_MSE_V2:
        if H % h or W % w:
            raise ValueError("level {}x{} is not a whole-block area reduction of {}x{}".format(h, w, H, W))
        n = ok.reshape(B, h, H // h, w, W // w).sum(dim=(2, 4))
        s = x.reshape(B, h, H // h, w, W // w, 2).sum(dim=(2, 4))
        m = n >= 1
        den = n.clamp(min=1).to(x.dtype)
    else:
        y0, y1, ly0, ly1 = _axis_weights(h, H)
        x0, x1, lx0, lx1 = _axis_weights(w, W)
        s = torch.zeros((B, h, w, 2), dtype=x.dtype, device=x.device)
        den = torch.zeros((B, h, w), dtype=x.dtype, device=x.device)
        for yi, ly in ((y0, ly0), (y1, ly1)):
            for xi, lx in ((x0, lx0), (x1, lx1)):
                yi_, xi_ = yi.to(x.device), xi.to(x.device)
                wk = (ly.to(x.dtype).view(h, 1) * lx.to(x.dtype).view(1, w)).to(x.device)   # fp32 factors, x's product
                vk = ok[:, yi_][:, :, xi_]
                s = s + torch.where(vk[..., None], wk[..., None] * x[:, yi_][:, :, xi_], zero)
                den = den + torch.where(vk, wk, zero)
        m = den > 0
        den = torch.where(m, den, zero + 1)
    gt = torch.where(m[..., None], s / den[..., None] * (h / H), zero)
    return gt, m


def _masked_levels_torch(loss, y_true, shapes, valid):
    x = y_true.detach()
    x = x if loss.axis == 3 else x.permute(0, 2, 3, 1)
    ok = (x[..., 0].abs() <= metrics.FLOW_UNKNOWN) & (x[..., 1].abs() <= metrics.FLOW_UNKNOWN)
    if valid is not None:
        ok = ok & (valid != 0)
    x = torch.where(ok[..., None], x, torch.zeros((), dtype=x.dtype, device=x.device))
    return [_masked_level_torch(loss, x, ok, int(h), int(w)) for h, w in shapes]


def _level_shapes(loss, y_preds):
    return [tuple(p.shape[1:3]) if loss.axis == 3 else tuple(p.shape[2:4]) for p in y_preds]


def masked_ground_truth_torch(loss, y_true, shapes, valid=None):
    """``masked_ground_truth`` composed from torch operators, on any device and in y_true's dtype (float64 inputs give
    the float64 reference; the bilinear weights along each axis are the kernel's fp32 values in every dtype)."""
    valid = _masked_args(loss, y_true, valid)
    gts, masks = [], []
    for gt, m in _masked_levels_torch(loss, y_true, shapes, valid):
        gts.append(gt if loss.axis == 3 else gt.permute(0, 3, 1, 2).contiguous())
        masks.append(m.to(torch.uint8))
    return gts, masks


def multiscale_masked_torch(loss, y_true, y_preds, valid=None):
    """``multiscale_masked`` composed from torch operators, on any device, in y_true's dtype and differentiable in
    y_preds through torch autograd: the path CPU tensors take and the baseline the kernels are timed against."""
    valid = _masked_args(loss, y_true, valid)
    y_preds = list(y_preds)
    if not 1 <= len(y_preds) <= 8:
        raise ValueError("the losses take 1..8 prediction levels, got {}".format(len(y_preds)))
    p0, p1 = loss._params()
    per_level, counts = [], []
    for p, (gt, m) in zip(y_preds, _masked_levels_torch(loss, y_true, _level_shapes(loss, y_preds), valid)):
        p = (p if loss.axis == 3 else p.permute(0, 2, 3, 1)).to(gt.dtype)
        h, w = p.shape[1:3]
        zero = torch.zeros((), dtype=gt.dtype, device=gt.device)
        p = torch.where(m[..., None], p, zero)                 # whatever an invalid pixel predicts is selected out
        if loss.kind == _hip.LOSS_FLOW_MSE_V2:
            s = 2.0 / (w + h)
            e = s * p - s * gt
            a = e.abs()
            term = torch.where(a <= p0, 0.5 * e * e, p0 * a - 0.5 * p0 * p0).sum(-1)
            per_element = 2
        elif loss.kind == _hip.LOSS_FLOW_MSE:
            term = torch.linalg.vector_norm(gt - p, 2, dim=-1)  # its gradient at a zero residual is 0
            per_element = 1
        else:
            term = ((gt - p).abs().sum(-1) + p1).pow(p0)
            per_element = 1
        count = m.sum()
        per_level.append(torch.where(m, term, zero).sum() / (count.clamp(min=1) * per_element))
        counts.append(count)
    per_level = torch.stack(per_level)
    return per_level.sum(), per_level, torch.stack(counts)


def multiscale_masked(loss, y_true, y_preds, valid=None):
    """The three flow losses over the valid pixels only, for 1..8 predictions against one full-resolution ground truth
    -> (total, per_level, counts): per_level [L] (what autograd differentiates), total = per_level.sum(), counts int64
    [L], the valid level pixels of each level, all on the inputs' device.  ``loss``: a FlowMseLossV2, FlowMseLoss or
    FlowMseLossFineTune (TypeError for AutoResizeMseLoss); ``valid``: None, or a (B,H,W) mask (bool, uint8 or floating).
    A level without a valid pixel has loss 0 and an all-zero gradient.  HIP tensors (y_true float32): one forward launch
    for all levels plus a fold and one backward launch, no host synchronisation; CPU tensors: ``multiscale_masked_torch``."""
    valid = _masked_args(loss, y_true, valid)
    if not y_true.is_cuda:
        return multiscale_masked_torch(loss, y_true, y_preds, valid)
    p0, p1 = loss._params()
    per_level, counts = ops.masked_loss(loss.kind, y_true, list(y_preds), valid, loss.data_format, p0, p1)
    return per_level.sum(), per_level, counts


def masked_ground_truth(loss, y_true, shapes, valid=None):
    """The per-level ground truth and validity the masked losses compare against, with no prediction -> (gts, masks):
    gts[l] in the loss's layout at (h, w) = shapes[l] with 0 where the level pixel has no ground truth, masks[l] uint8
    (B,h,w).  Up to 8 levels per pass over y_true on a HIP device; CPU tensors: ``masked_ground_truth_torch``."""
    valid = _masked_args(loss, y_true, valid)
    if not y_true.is_cuda:
        return masked_ground_truth_torch(loss, y_true, shapes, valid)
    shapes = [(int(h), int(w)) for h, w in shapes]
    p0, p1 = loss._params()
    gts, masks = [], []
    for k in range(0, len(shapes), 8):
        _, _, _, g, m = ops.masked_loss_fwd(loss.kind, y_true, None, valid, loss.data_format, p0, p1, want_gt=True,
                                            want_valid=True, shapes=shapes[k:k + 8])
        gts += [t.contiguous() for t in g]
        masks += m
    return gts, masks


# ---- the label-free flow losses (include/qpwc_unsup_loss.h) ------------------------------------------------------------
# For raw video and for the unlabelled part of sparse frames; the reference has no such loss.  The UnFlow / UFlow recipe:
# a photometric term between prv and nxt warped by the flow (UFlow's soft ternary census on a 7 x 7 patch, or Charbonnier
# on RGB), over the pixels whose sample stays inside the image and is not occluded, plus edge-aware first-order
# smoothness.  Frames are constants, only the flow is differentiated.  HIP tensors take qpwc_unsup_loss_fwd / _bwd; CPU
# tensors take the torch chain below.  Non-finite flows are out of scope.

_UNSUP_KINDS = {"census": _hip.UNSUP_CENSUS, "charbonnier": _hip.UNSUP_CHARBONNIER}


class PhotometricLoss:
    """The label-free loss of one or more flow levels: ``kind`` 'census' (term = (dist + eps)^q of the soft ternary
    census distance) or 'charbonnier' (term = mean_c ((prv_c - warped_c)^2 + eps^2)^q), averaged over the unmasked pixels,
    plus ``smooth_weight`` times the edge-aware smoothness (weights exp(-edge * mean_c |d prv|), penalty
    sqrt(d flow^2 + smooth_eps^2)).  q and eps carry the names and defaults of FlowMseLossFineTune; smooth_weight = 2.0 is
    a starting point, not a tuned value.  ``loss(pairs, flow, occluded=None)`` is one level; ``multiscale_unsupervised``
    takes the network's list.  There is no ground truth: the first argument is the frame pair the network saw."""

    def __init__(self, kind="census", q=0.4, eps=0.01, smooth_weight=2.0, edge=150.0, smooth_eps=1e-3, data_format=None,
                 name=None):
        if kind not in _UNSUP_KINDS:
            raise ValueError("kind must be 'census' or 'charbonnier', got {!r}".format(kind))
        q, eps, smooth_weight, edge, smooth_eps = (float(v) for v in (q, eps, smooth_weight, edge, smooth_eps))
        if not (q > 0.0 and eps > 0.0 and smooth_eps > 0.0):
            raise ValueError("q, eps and smooth_eps must be > 0, got {}, {} and {}".format(q, eps, smooth_eps))
        if not (edge >= 0.0 and smooth_weight >= 0.0):
            raise ValueError("edge and smooth_weight must be >= 0, got {} and {}".format(edge, smooth_weight))
        self.kind, self.q, self.eps, self.smooth_weight, self.edge, self.smooth_eps = kind, q, eps, smooth_weight, edge, smooth_eps
        self.data_format = image_data_format() if data_format is None else data_format
        self.axis = get_axis(self.data_format)
        self.name = name

    def __call__(self, pairs, flow, occluded=None):
        if isinstance(occluded, torch.Tensor):
            occluded = [occluded]
        return multiscale_unsupervised(self, pairs, [flow], occluded)[1].reshape(())

    def call(self, pairs, flow, occluded=None):
        return self(pairs, flow, occluded)

    def get_config(self):
        return {"name": self.name, "kind": self.kind, "q": self.q, "eps": self.eps, "smooth_weight": self.smooth_weight,
                "edge": self.edge, "smooth_eps": self.smooth_eps, "data_format": self.data_format}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


def _unsup_args(obj, pairs, flows, occluded):
    """-> (flows, level shapes, pooling exponents, occluded as a list or 'estimate') after the checks both paths share."""
    if not isinstance(obj, PhotometricLoss):
        raise TypeError("multiscale_unsupervised takes a PhotometricLoss, got {}".format(type(obj).__name__))
    if not isinstance(pairs, torch.Tensor):
        raise TypeError("pairs must be a torch.Tensor")
    if pairs.dim() != 4 or pairs.shape[obj.axis] != 6:
        raise ValueError("pairs must be the frame pair the network saw, 6 channels on axis {} ({}), got shape {}: this "
                         "loss has no ground truth".format(obj.axis, obj.data_format, tuple(pairs.shape)))
    flows = list(flows)
    if not 1 <= len(flows) <= 8:
        raise ValueError("the losses take 1..8 flow levels, got {}".format(len(flows)))
    H, W = (pairs.shape[1], pairs.shape[2]) if obj.axis == 3 else (pairs.shape[2], pairs.shape[3])
    shapes, exps = [], []
    for i, f in enumerate(flows):
        if not isinstance(f, torch.Tensor) or f.dim() != 4 or f.shape[obj.axis] != 2 or f.shape[0] != pairs.shape[0]:
            raise ValueError("flows[{}] must be a batched 2-channel flow ({}) of batch {}".format(i, obj.data_format,
                                                                                                pairs.shape[0]))
        h, w = (f.shape[1], f.shape[2]) if obj.axis == 3 else (f.shape[2], f.shape[3])
        k = max((H // h).bit_length() - 1, 0) if h else 0
        if h < 1 or w < 1 or h << k != H or w << k != W:
            raise ValueError("level {}: {}x{} is not {}x{} over one power of two on both axes".format(i, h, w, H, W))
        shapes.append((int(h), int(w)))
        exps.append(k)
    if isinstance(occluded, str):
        if occluded != "estimate":
            raise ValueError("occluded must be None, a list of masks or 'estimate', got '{}'".format(occluded))
    elif occluded is not None:
        occluded = list(occluded)
        if len(occluded) != len(flows):
            raise ValueError("{} masks for {} flow levels".format(len(occluded), len(flows)))
        occluded = [metrics._flow_mask("occluded[%d]" % i, m, f, (int(f.shape[0]),) + s)
                    for i, (m, f, s) in enumerate(zip(occluded, flows, shapes))]
    return flows, shapes, exps, occluded


def _unsup_sample_torch(img, flow):
    """img (B,h,w,C) sampled bilinearly at (x, y) + flow (B,h,w,2) by the CLAMP rule, written out with gathers ->
    (values (B,h,w,C), inside (B,h,w)).  floor carries no gradient, alpha passes it on [0, 1], and a sample outside the
    image passes none."""
    B, h, w, C = img.shape
    ys = torch.arange(h, dtype=flow.dtype, device=flow.device).view(1, h, 1)
    xs = torch.arange(w, dtype=flow.dtype, device=flow.device).view(1, 1, w)
    qx, qy = xs + flow[..., 0], ys + flow[..., 1]
    inside = (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
    qx, qy = torch.where(inside, qx, qx.detach()), torch.where(inside, qy, qy.detach())
    fx, fy = qx.detach().floor().clamp(0, max(w - 2, 0)), qy.detach().floor().clamp(0, max(h - 2, 0))
    ax, ay = (qx - fx).clamp(0, 1)[..., None], (qy - fy).clamp(0, 1)[..., None]
    x0, y0 = fx.long(), fy.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    flat = img.reshape(B, h * w, C)
    tap = lambda yi, xi: flat.gather(1, (yi * w + xi).reshape(B, h * w, 1).expand(-1, -1, C)).reshape(B, h, w, C)
    tl, tr, bl, br = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    top, bot = ax * (tr - tl) + tl, ax * (br - bl) + bl
    return ay * (bot - top) + top, inside


def _unsup_grey(img):
    return 255.0 * ((0.2989 * img[..., 0] + 0.587 * img[..., 1]) + 0.114 * img[..., 2])


def _unsup_ternary(g):
    """(B,h,w) -> (B,h-6,w-6,48): D / sqrt(0.81 + D^2) of the 48 neighbours of every interior pixel."""
    h, w = g.shape[1:]
    c = g[:, 3:h - 3, 3:w - 3]
    out = []
    for dy in range(7):
        for dx in range(7):
            if (dy, dx) != (3, 3):
                d = g[:, dy:dy + h - 6, dx:dx + w - 6] - c
                out.append(d / torch.sqrt(0.81 + d * d))
    return torch.stack(out, dim=-1)


def _unsup_level_torch(obj, prv, nxt, flow, occ):
    """(photometric, smoothness, count) of one level: prv, nxt (B,h,w,3) and flow (B,h,w,2) in one dtype, occ None or
    (B,h,w) uint8."""
    B, h, w, _ = prv.shape
    zero = torch.zeros((), dtype=prv.dtype, device=prv.device)
    keep = torch.ones((B, h, w), dtype=torch.bool, device=prv.device) if occ is None else occ == 0
    if obj.kind == "census":
        if h < 7 or w < 7:
            photo, count = flow.sum() * 0, torch.zeros((), dtype=torch.int64, device=prv.device)
        else:
            gw, inside = _unsup_sample_torch(_unsup_grey(nxt)[..., None], flow)
            e = (_unsup_ternary(_unsup_grey(prv)) - _unsup_ternary(gw[..., 0])) ** 2
            term = ((e / (0.1 + e)).sum(-1) + obj.eps) ** obj.q
            m = (inside & keep)[:, 3:h - 3, 3:w - 3]
            count = m.sum()
            photo = torch.where(m, term, zero).sum() / count.clamp(min=1)
    else:
        warped, inside = _unsup_sample_torch(nxt, flow)
        term = (((prv - warped) ** 2 + obj.eps ** 2) ** obj.q).sum(-1) / 3.0
        m = inside & keep
        count = m.sum()
        photo = torch.where(m, term, zero).sum() / count.clamp(min=1)
    robust = lambda d: torch.sqrt(d * d + obj.smooth_eps ** 2)
    sx = sy = zero
    if w > 1:
        wx = torch.exp(-obj.edge * (prv[:, :, 1:] - prv[:, :, :-1]).abs().mean(-1))
        sx = (wx[..., None] * robust(flow[:, :, 1:] - flow[:, :, :-1])).mean()
    if h > 1:
        wy = torch.exp(-obj.edge * (prv[:, 1:] - prv[:, :-1]).abs().mean(-1))
        sy = (wy[..., None] * robust(flow[:, 1:] - flow[:, :-1])).mean()
    return photo, (sx + sy) / 2, count


def _unsup_pool_torch(x, k):
    """k successive 2 x 2 means of x (N,H,W,C), each ((a + b) + c + d) / 4 in row-major order, as
    qpwc_avgpool_pyramid_fwd forms them."""
    for _ in range(k):
        N, H, W, C = x.shape
        x = x.reshape(N, H // 2, 2, W // 2, 2, C)
        x = (((x[:, :, 0, :, 0] + x[:, :, 0, :, 1]) + x[:, :, 1, :, 0]) + x[:, :, 1, :, 1]) / 4
    return x


def _unsup_frames(pairs, axis, exps, pool):
    """The frame pair -> per level (prv, nxt) channels-last, pooled by 2^k with pool(stacked frames, k)."""
    prv, nxt = torch.chunk(pairs.detach(), 2, dim=axis)
    stacked = torch.cat([prv, nxt], dim=0)
    stacked = (stacked if axis == 3 else stacked.permute(0, 2, 3, 1)).contiguous()
    B, made, out = pairs.shape[0], {}, []
    for k in exps:
        if k not in made:
            made[k] = stacked if k == 0 else pool(stacked, k)
        out.append((made[k][:B], made[k][B:]))
    return out


def multiscale_unsupervised_torch(obj, pairs, flows, occluded=None):
    """``multiscale_unsupervised`` composed from torch operators, on any device, in pairs' dtype (float64 inputs give the
    float64 reference) and differentiable in the flows through torch autograd: the path CPU tensors take and the baseline
    the kernels are timed against.  occluded='estimate' needs HIP tensors (occlusion.estimate_occlusion_map)."""
    flows, shapes, exps, occluded = _unsup_args(obj, pairs, flows, occluded)
    if isinstance(occluded, str):
        from . import occlusion
        occluded = [metrics._flow_mask("occluded", occlusion.estimate_occlusion_map(f.detach(), obj.data_format), f,
                                       (int(f.shape[0]),) + s) for f, s in zip(flows, shapes)]
    occluded = [None] * len(flows) if occluded is None else occluded
    photo, smooth, counts = [], [], []
    for (prv, nxt), f, occ in zip(_unsup_frames(pairs, obj.axis, exps, _unsup_pool_torch), flows, occluded):
        f = (f if obj.axis == 3 else f.permute(0, 2, 3, 1)).to(pairs.dtype)
        p, s, c = _unsup_level_torch(obj, prv, nxt, f, occ)
        photo.append(p)
        smooth.append(s)
        counts.append(c)
    photo, smooth = torch.stack(photo), torch.stack(smooth)
    per_level = photo + obj.smooth_weight * smooth
    return per_level.sum(), per_level, {"photometric": photo.detach(), "smoothness": smooth.detach(),
                                        "counts": torch.stack(counts)}


def _unsup_pool_hip(x, k):
    while k > 0:                       # qpwc_avgpool_pyramid_fwd pools up to 6 levels a launch
        x, k = ops.avgpool_pyramid(x, min(k, 6)), k - min(k, 6)
    return x


def multiscale_unsupervised(obj, pairs, flows, occluded=None):
    """The label-free loss of 1..8 flow levels against the frame pair the network saw -> (total, per_level, parts):
    per_level [L] (what autograd differentiates, in the flows only), total = per_level.sum(), parts = {'photometric' [L],
    'smoothness' [L], 'counts' int64 [L]}, all on the inputs' device with nothing read back.  ``obj``: a PhotometricLoss;
    ``pairs``: (B,H,W,6) / (B,6,H,W) by obj.data_format; ``flows``: what FlowerModel returns, each (H / 2^k, W / 2^k) in
    level pixels (anything else is a ValueError), fp32 or fp16.  Per level the frames are the block mean of the pair
    (qpwc_avgpool_pyramid_fwd, both frames stacked on the batch axis, one launch per distinct factor; factor 1: the frames
    themselves).  ``occluded``: None, a list of per-level (B,h,w) masks (bool, uint8 or floating; entries may be None),
    or 'estimate': occlusion.estimate_occlusion_map of each detached level flow.  The backward direction is a second call
    with the frames swapped.  HIP tensors (pairs float32): the frames, then one forward launch for all levels plus a
    fold, and one backward launch; CPU tensors: ``multiscale_unsupervised_torch``."""
    if isinstance(pairs, torch.Tensor) and not pairs.is_cuda:
        return multiscale_unsupervised_torch(obj, pairs, flows, occluded)
    flows, shapes, exps, occluded = _unsup_args(obj, pairs, flows, occluded)
    if pairs.dtype != torch.float32:
        raise ValueError("pairs must be float32, got {}".format(pairs.dtype))
    if isinstance(occluded, str):
        from . import occlusion
        occluded = [metrics._flow_mask("occluded", occlusion.estimate_occlusion_map(f.detach(), obj.data_format), f,
                                       (int(f.shape[0]),) + s) for f, s in zip(flows, shapes)]
    frames = _unsup_frames(pairs, obj.axis, exps, _unsup_pool_hip)
    per_level, photo, smooth, counts = ops.unsup_loss(
        _UNSUP_KINDS[obj.kind], [p for p, _ in frames], [n for _, n in frames], flows, occluded, obj.data_format, obj.q,
        obj.eps, obj.smooth_weight, obj.edge, obj.smooth_eps)
    return per_level.sum(), per_level, {"photometric": photo, "smoothness": smooth, "counts": counts}


# ---- the interpolator's SSIM + Charbonnier loss (include/qpwc_image_loss.h) ---------------------------------------------
# MSE on intermediate frames blurs; the model is scored by SSIM (metrics.image_quality).  Per level, against
# AutoResizeMseLoss's own target: ssim_weight * (1 - SSIM) / 2 + (1 - ssim_weight) * mean ((p - t)^2 + eps^2)^q, SSIM with
# tf.image.ssim's default window on p + offset and t + offset, unclipped.  The reference has no such loss.  HIP tensors
# take qpwc_image_loss_fwd / _bwd; CPU tensors take the torch chain below.  Non-finite images are out of scope.

class ImageLoss:
    """The structural loss of one or more image levels: ``ssim_weight`` times the structural dissimilarity
    (1 - mean SSIM) / 2 plus (1 - ``ssim_weight``) times the Charbonnier term mean ((y_pred - target)^2 + eps^2)^q.
    SSIM is ``metrics.image_quality``'s (filter_size 11, sigma 1.5, k1 0.01, k2 0.03) on the images plus ``offset``
    (0.5 takes [-0.5, 0.5] to [0, 1]) with dynamic range ``max_val``, without clipping; a level below 11 x 11 has no
    SSIM position: its dssim is 0.  ssim_weight = 0.85 is the conventional value (Godard et al.), a hyperparameter
    nobody has tuned here.  The per-level target is AutoResizeMseLoss's: y_true resized bilinearly to the level.
    ``loss(y_true, y_pred)`` is one level; ``multiscale_image`` takes the network's list.  Layout from
    ``image_data_format()`` at construction unless given."""

    def __init__(self, ssim_weight=0.85, q=0.5, eps=1e-3, max_val=1.0, offset=0.5, data_format=None, name=None):
        ssim_weight, q, eps, max_val, offset = (float(v) for v in (ssim_weight, q, eps, max_val, offset))
        if not 0.0 <= ssim_weight <= 1.0:
            raise ValueError("ssim_weight must be in [0, 1], got {}".format(ssim_weight))
        if not (q > 0.0 and eps > 0.0):
            raise ValueError("q and eps must be > 0, got {} and {}".format(q, eps))
        if not (max_val > 0.0 and max_val < float("inf") and abs(offset) < float("inf")):
            raise ValueError("max_val must be finite and > 0 and offset finite, got {} and {}".format(max_val, offset))
        self.ssim_weight, self.q, self.eps, self.max_val, self.offset = ssim_weight, q, eps, max_val, offset
        self.data_format = image_data_format() if data_format is None else data_format
        self.axis = get_axis(self.data_format)
        self.name = name

    def __call__(self, y_true, y_pred):
        return multiscale_image(self, y_true, [y_pred])[1].reshape(())

    def call(self, y_true, y_pred):
        return self(y_true, y_pred)

    def get_config(self):
        return {"name": self.name, "ssim_weight": self.ssim_weight, "q": self.q, "eps": self.eps, "max_val": self.max_val,
                "offset": self.offset, "data_format": self.data_format}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


def _image_args(obj, y_true, y_preds):
    """-> (y_preds, level shapes) after the checks both paths share."""
    if not isinstance(obj, ImageLoss):
        raise TypeError("multiscale_image takes an ImageLoss, got {}".format(type(obj).__name__))
    if not isinstance(y_true, torch.Tensor):
        raise TypeError("y_true must be a torch.Tensor")
    if y_true.requires_grad and torch.is_grad_enabled():
        raise ValueError("y_true requires grad: the losses are differentiable in y_pred only, a gradient for y_true "
                         "would be dropped (detach it)")
    if y_true.dim() != 4 or not 1 <= y_true.shape[obj.axis] <= 4:
        raise ValueError("y_true must be a batched image of 1..4 channels on axis {} ({}), got shape {}".format(
            obj.axis, obj.data_format, tuple(y_true.shape)))
    y_preds = list(y_preds)
    if not 1 <= len(y_preds) <= 8:
        raise ValueError("the losses take 1..8 prediction levels, got {}".format(len(y_preds)))
    shapes = []
    for i, p in enumerate(y_preds):
        if not isinstance(p, torch.Tensor):
            raise TypeError("y_preds[{}] must be a torch.Tensor".format(i))
        if p.device != y_true.device:
            raise ValueError("y_preds[{}] is on {}, y_true on {}".format(i, p.device, y_true.device))
        if p.dim() != 4 or p.shape[0] != y_true.shape[0] or p.shape[obj.axis] != y_true.shape[obj.axis]:
            raise ValueError("y_preds[{}] must be a batched image ({}) of batch {} and {} channels, got shape {}".format(
                i, obj.data_format, y_true.shape[0], y_true.shape[obj.axis], tuple(p.shape)))
        h, w = (p.shape[1], p.shape[2]) if obj.axis == 3 else (p.shape[2], p.shape[3])
        if h < 1 or w < 1:
            raise ValueError("y_preds[{}] is empty: shape {}".format(i, tuple(p.shape)))
        shapes.append((int(h), int(w)))
    return y_preds, shapes


def resized_ground_truth_torch(y_true, shapes, data_format):
    """``ops.resized_ground_truth`` composed from torch operators, on any device and in y_true's dtype: the four
    bilinear corners of tf.image.resize (half-pixel centres, no antialias) with the kernel's fp32 weights along each
    axis in every dtype, combined as the kernel combines them."""
    x = y_true.detach()
    x = x if get_axis(data_format) == 3 else x.permute(0, 2, 3, 1)
    H, W = x.shape[1:3]
    out = []
    for h, w in shapes:
        y0, y1, ly0, ly1 = (t.to(x.device) for t in _axis_weights(int(h), H))
        x0, x1, lx0, lx1 = (t.to(x.device) for t in _axis_weights(int(w), W))
        ly0, ly1 = ly0.to(x.dtype).view(1, -1, 1, 1), ly1.to(x.dtype).view(1, -1, 1, 1)
        lx0, lx1 = lx0.to(x.dtype).view(1, 1, -1, 1), lx1.to(x.dtype).view(1, 1, -1, 1)
        top, bot = x[:, y0], x[:, y1]
        g = ly0 * (lx0 * top[:, :, x0] + lx1 * top[:, :, x1]) + ly1 * (lx0 * bot[:, :, x0] + lx1 * bot[:, :, x1])
        out.append(g if get_axis(data_format) == 3 else g.permute(0, 3, 1, 2).contiguous())
    return out


def _image_level_torch(obj, t, p):
    """(dssim, charbonnier) of one level: target t and prediction p, (B,C,h,w) in one dtype."""
    import torch.nn.functional as F
    C, h, w = t.shape[1:]
    d = p - t
    charb = ((d * d + obj.eps ** 2) ** obj.q).mean()
    if h < metrics.SSIM_FILTER["filter_size"] or w < metrics.SSIM_FILTER["filter_size"]:
        return p.sum() * 0, charb
    g = metrics.ssim_window().to(device=t.device, dtype=t.dtype)
    rows, cols = g.view(1, 1, 1, -1).repeat(C, 1, 1, 1), g.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    conv = lambda x: F.conv2d(F.conv2d(x.contiguous(), rows, groups=C), cols, groups=C)
    c1 = float(torch.tensor((metrics.SSIM_FILTER["k1"] * obj.max_val) ** 2, dtype=torch.float64).float())
    c2 = float(torch.tensor((metrics.SSIM_FILTER["k2"] * obj.max_val) ** 2, dtype=torch.float64).float())
    vt, vp = t + obj.offset, p + obj.offset
    mt, mp = conv(vt), conv(vp)
    num0, den0 = 2.0 * mt * mp, mt * mt + mp * mp
    num1, den1 = 2.0 * conv(vt * vp), conv(vt * vt + vp * vp)
    s = (num0 + c1) / (den0 + c1) * ((num1 - num0 + c2) / (den1 - den0 + c2))
    return (1.0 - s.mean()) / 2.0, charb


def multiscale_image_torch(obj, y_true, y_preds):
    """``multiscale_image`` composed from torch operators (``F.conv2d(groups=C)`` along the rows and then the columns
    with ``metrics.ssim_window()``), on any device, in y_true's dtype (float64 inputs give the float64 reference) and
    differentiable in y_preds through torch autograd: the path CPU tensors take and the baseline the kernels are timed
    against."""
    y_preds, shapes = _image_args(obj, y_true, y_preds)
    dssim, charb = [], []
    for t, p in zip(resized_ground_truth_torch(y_true, shapes, obj.data_format), y_preds):
        if obj.axis == 3:
            t, p = t.permute(0, 3, 1, 2), p.permute(0, 3, 1, 2)
        s, c = _image_level_torch(obj, t, p.to(t.dtype))
        dssim.append(s)
        charb.append(c)
    dssim, charb = torch.stack(dssim), torch.stack(charb)
    per_level = obj.ssim_weight * dssim + (1.0 - obj.ssim_weight) * charb
    return per_level.sum(), per_level, {"dssim": dssim.detach(), "charbonnier": charb.detach()}


def multiscale_image(obj, y_true, y_preds):
    """The SSIM + Charbonnier loss of 1..8 predicted images against one full-resolution image -> (total, per_level,
    parts): per_level [L] (what autograd differentiates, in y_preds only), total = per_level.sum(), parts = {'dssim'
    [L], 'charbonnier' [L]}, fp32 on the inputs' device with nothing read back.  ``obj``: an ImageLoss; ``y_true``:
    float32 (B,H,W,C) / (B,C,H,W) by obj.data_format, 1..4 channels, never differentiated; ``y_preds``: what
    InterpolatorModel returns, each fp32 or fp16 at its own (h, w); the gradient comes back in each one's dtype and
    layout.  Per level the target is AutoResizeMseLoss's (ops.resized_ground_truth, one launch for all levels), so the
    loss swaps in for ``multiscale(AutoResizeMseLoss(), ...)`` without changing what a level is compared against.  HIP
    tensors: the targets, then one forward launch for all levels plus a fold, and one backward launch, no host
    synchronisation; CPU tensors: ``multiscale_image_torch``."""
    y_preds, shapes = _image_args(obj, y_true, y_preds)
    if not y_true.is_cuda:
        return multiscale_image_torch(obj, y_true, y_preds)
    if y_true.dtype != torch.float32:
        raise ValueError("y_true must be float32, got {}".format(y_true.dtype))
    if ops._wants_grad(*y_preds):
        ops._refuse_capture("the image loss")       # before the targets' launch
    truths = ops.resized_ground_truth(y_true, shapes, obj.data_format)
    per_level, dssim, charb = ops.image_loss(truths, y_preds, obj.data_format, obj.ssim_weight, obj.q, obj.eps,
                                             obj.max_val, obj.offset)
    return per_level.sum(), per_level, {"dssim": dssim, "charbonnier": charb}

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

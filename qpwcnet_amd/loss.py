"""Training losses of the reference (qpwcnet/train/loss.py) on the gfx950 HIP kernels behind ``qpwc_loss_fwd`` /
``qpwc_loss_bwd``: ``FlowMseLossV2``, ``FlowMseLoss``, ``FlowMseLossFineTune``, ``AutoResizeMseLoss``.

Same class names, constructor arguments and ``loss(y_true, y_pred)`` call as the reference's Keras losses; each call
returns a 0-dim fp32 tensor, differentiable in ``y_pred``.  ``multiscale(loss, y_true, y_preds)`` is the trainer's
``[l(flo, o) for o in pred_flows[:-1]]`` + ``sum(...)`` (qpwcnet/app/optical_flow/train.py:98-122) with every level
in one forward launch (plus a fixed-order fold) and one backward launch.

``y_true``: the full-resolution fp32 ground truth, never differentiated (a ``y_true`` that requires grad is refused);
``y_pred``: fp32 or fp16 (the fp16-storage network's flows), gradients come back in its dtype.  Both layouts are read
as they are.  No CPU path.  Keras' ``sample_weight`` / ``reduction`` are not supported.
"""
from . import _hip, ops
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

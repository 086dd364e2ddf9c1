"""The trainer's update step of the reference (qpwcnet/app/optical_flow/train.py:294-296,
app/frame_interpolation/pre_train.py:67-69):

    agc_grads = adaptive_clip_grad(params, grads, self.clip_factor, self.eps)      # core/agc.py:39-49
    self.optimizer.apply_gradients(zip(agc_grads, params))                          # tf.keras.optimizers.Adam

``KerasAdamAGC`` is both lines as one ``torch.optim.Optimizer``.  CUDA fp32 parameters take one launch of the gfx950
kernel behind ``qpwc_agc_adam_step`` (include/qpwc_optim.h) for the whole model; CPU parameters run ``step_torch``, the
same chain composed from torch operators, which is also what the tests hold the kernel against.

Two things here are not what a torch user would write by hand:

* AGC clips per *unit*, and the reference defines units on the Keras layouts (the norm of a rank-4 kernel runs over
  axes 0, 1, 2).  On the torch layouts this package stores (``weights.py``) that is one unit per output channel of a
  Conv2D or pointwise kernel, one per INPUT channel of a ``conv_up`` (Conv2DTranspose) kernel, and a single unit for a
  whole depthwise kernel and for every bias / gamma / beta.  A shape cannot tell a depthwise kernel from a
  one-input-channel convolution, so the optimiser is built from *named* parameters (``weights._kind``).
* Keras' Adam folds both bias corrections into the step size and adds ``epsilon`` (1e-7) to the uncorrected
  ``sqrt(v)``; torch divides by ``sqrt(v_hat) + 1e-8``.  The trajectories differ from the first step.

Keras casts the hyperparameters to the variable's dtype: the betas and epsilon used are their float32 roundings.
"""
import bisect
import math

import numpy as np
import torch

from . import _hip
from .weights import _kind

_GRAD_NORM_FLOOR = 1e-6         # agc.py:46


def _f32(x):
    return float(np.float32(x))


def _unit_kind(name, shape):
    """'rows' (one unit per slice of the first axis) or 'whole' (one unit)."""
    if len(shape) <= 1:
        return "whole"
    if len(shape) not in (2, 4):
        raise ValueError("{}: adaptive gradient clipping has no unit rule for a rank-{} parameter".format(name, len(shape)))
    return "whole" if _kind(name) == "depthwise" else "rows"


def agc_units(name, shape):
    """[(offset, length), ...]: the runs of the dense torch-layout tensor ``name`` that share one AGC norm.  Rank <= 1:
    the whole tensor.  Rank 4 by ``weights._kind(name)``: 'conv' (O,I,kh,kw) one unit per [o] slice, 'transpose'
    (I,O,kh,kw) one per [i] slice (Keras stores (kh,kw,out,in): per input channel), 'depthwise' (C,1,kh,kw) the whole
    tensor.  Rank 2 (out,in): one unit per row (agc.py's axis 0 of Keras' (in,out))."""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if n == 0:
        return []
    if _unit_kind(name, shape) == "whole":
        return [(0, n)]
    row = n // shape[0]
    return [(i * row, row) for i in range(shape[0])]


def _named(model_or_named_parameters):
    src = model_or_named_parameters
    if isinstance(src, torch.nn.Module):
        src = [(n, p) for n, p in src.named_parameters() if p.requires_grad]
    elif isinstance(src, dict):
        src = list(src.items())
    else:
        src = list(src)
    for item in src:
        if not (isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[0], str)
                and isinstance(item[1], torch.Tensor)):
            raise TypeError("KerasAdamAGC takes a module or (name, parameter) pairs: the AGC units depend on the name")
    names = [n for n, _ in src]
    if not names:
        raise ValueError("no parameters to optimise")
    if len(set(names)) != len(names):
        raise ValueError("duplicate parameter names")
    return [(n, p) for n, p in src]


def adaptive_clip_grad(named_params, grads, clip_factor=0.01, eps=1e-3):
    """core/agc.py:39-49 on torch layouts, composed from torch operators: the clipped gradients, in order, for
    ``named_params`` (a module or (name, tensor) pairs) and their ``grads`` (None passes through).  For users who keep
    their own optimiser."""
    out = []
    for (name, p), g in zip(_named(named_params), grads):
        if g is None:
            out.append(None)
            continue
        rows = p.shape[0] if _unit_kind(name, p.shape) == "rows" else 1
        pv, gv = p.detach().reshape(rows, -1), g.reshape(rows, -1)
        pn = pv.square().sum(1, keepdim=True).sqrt()
        gn = gv.square().sum(1, keepdim=True).sqrt()
        # torch.maximum propagates NaN as tf.maximum does; a NaN comparison selects the clipped branch
        mx = torch.maximum(pn, torch.full_like(pn, eps)) * clip_factor
        clipped = gv * (mx / torch.maximum(gn, torch.full_like(gn, _GRAD_NORM_FLOOR)))
        out.append(torch.where(gn < mx, gv, clipped).reshape(g.shape))
    return out


def keras_step_size(lr, beta_1, beta_2, t):
    """alpha = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t) of Keras' Adam at its t-th update (t = iterations + 1), in
    Python floats, with the betas rounded to float32 as Keras casts them."""
    b1, b2 = _f32(beta_1), _f32(beta_2)
    return float(lr) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def step_torch(named_params, grads, m, v, alpha, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clip_factor=0.01, eps=1e-3):
    """One update, in place on the parameters and on the moment tensors ``m`` and ``v`` (lists in the parameters'
    order), composed from torch operators on the tensors' own device: ``adaptive_clip_grad`` (skipped for a
    ``clip_factor`` of None or <= 0), then Keras' dense Adam update with the step size ``alpha``
    (``keras_step_size``).  A None gradient leaves its tensor alone."""
    named = _named(named_params)
    if clip_factor is not None and clip_factor > 0:
        grads = adaptive_clip_grad(named, grads, clip_factor, eps)
    omb1, omb2 = 1.0 - _f32(beta_1), 1.0 - _f32(beta_2)
    with torch.no_grad():
        for (_, p), g, mi, vi in zip(named, grads, m, v):
            if g is None:
                continue
            mi.add_((g - mi) * omb1)
            vi.add_((g * g - vi) * omb2)
            p.sub_((mi * float(alpha)) / (vi.sqrt() + _f32(epsilon)))


def learning_rate(batch_size):
    """train.py:29-40: base 1e-4, halved after 400k, 600k, 800k and 1000k batches of 8 samples (the boundaries scale
    with 8 / batch_size), as a callable of the step count -- tf's PiecewiseConstantDecay: values[0] up to and including
    boundaries[0], values[i] on (boundaries[i-1], boundaries[i]], values[-1] after the last."""
    base_lr = 0.0001
    boundaries = [int(x / batch_size) for x in (400000 * 8, 600000 * 8, 800000 * 8, 1000000 * 8)]
    values = [base_lr / (2 ** i) for i in range(len(boundaries) + 1)]

    def schedule(step):
        return values[bisect.bisect_left(boundaries, int(step))]
    schedule.boundaries, schedule.values = boundaries, values
    return schedule


class KerasAdamAGC(torch.optim.Optimizer):
    """Unit-wise adaptive gradient clipping + ``tf.keras.optimizers.Adam`` (dense, no amsgrad).

    ``model_or_named_parameters``: a module (its trainable ``named_parameters()``) or (name, parameter) pairs; the
    names are the state-dict names of the model and select the AGC units (``agc_units``).  ``lr``: a float or a
    callable of the step count (``learning_rate``); ``clip_factor=None`` (or <= 0): no clipping, plain Keras Adam.
    One parameter group, so ``zero_grad()`` and ``param_groups[0]["lr"]`` behave as usual; the hyperparameters are read
    from the group at every step.

    ``m`` and ``v`` live in one flat fp32 buffer each (``state[p]["m"]`` / ``["v"]`` are views), allocated on the
    parameters' device at the first step.  ``state_dict()`` holds ``iterations`` and per-name ``m`` and ``v``; a loaded
    optimiser continues bit-identically.
    """

    def __init__(self, model_or_named_parameters, lr=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clip_factor=0.01,
                 eps=1e-3):
        named = _named(model_or_named_parameters)
        if not callable(lr) and not float(lr) >= 0.0:
            raise ValueError("invalid learning rate {}".format(lr))
        for k, b in (("beta_1", beta_1), ("beta_2", beta_2)):
            if not 0.0 <= b < 1.0:
                raise ValueError("{}={} outside [0, 1)".format(k, b))
        if not epsilon > 0.0 or not eps > 0.0:
            raise ValueError("epsilon and eps must be > 0")
        super().__init__([p for _, p in named], dict(lr=lr, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon,
                                                     clip_factor=clip_factor, eps=eps))
        self._names = [n for n, _ in named]
        self.iterations = 0
        # every tensor's run in the flat moment buffers starts on a multiple of 4 floats, so that m and v share the
        # 16-byte phase of a (16-byte aligned) parameter and the kernel's vector path applies
        self._offsets, units, total = [], [], 0
        for i, (n, p) in enumerate(named):
            self._offsets.append(total)
            units += [(i, off, length) for off, length in agc_units(n, p.shape)]
            total += (p.numel() + 3) // 4 * 4
        self._total = max(total, 4)
        self._units = torch.tensor(units, dtype=torch.int64).reshape(-1, 3)
        self._m = self._v = None
        self._units_dev = self._ptrs_dev = self._ptrs = None

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("KerasAdamAGC has one parameter group: its unit table is built once, from the names")
        super().add_param_group(param_group)

    # ---- state -------------------------------------------------------------------------------------------------------
    def _params(self):
        return self.param_groups[0]["params"]

    def _named_params(self):
        return list(zip(self._names, self._params()))

    def _views(self, flat):
        return [flat[o:o + p.numel()].view(p.shape) for o, p in zip(self._offsets, self._params())]

    def _device(self):
        params = self._params()
        if len({p.device for p in params}) != 1:
            raise ValueError("KerasAdamAGC: the parameters are on more than one device: {}".format(
                sorted({str(p.device) for p in params})))
        for n, p in zip(self._names, params):
            if p.dtype != torch.float32:
                raise ValueError("KerasAdamAGC: {} is {}; the update step is fp32 only".format(n, p.dtype))
        return params[0].device

    def _ensure_state(self, dev):
        if self._m is not None and self._m.device == dev:
            return
        if self._m is not None:     # the model moved: the moments follow it
            self._m, self._v = self._m.to(dev), self._v.to(dev)
        else:
            self._m = torch.zeros(self._total, dtype=torch.float32, device=dev)
            self._v = torch.zeros(self._total, dtype=torch.float32, device=dev)
        self._units_dev = self._ptrs_dev = self._ptrs = None
        for p, mi, vi in zip(self._params(), self._views(self._m), self._views(self._v)):
            self.state[p] = {"m": mi, "v": vi}

    def state_dict(self):
        if self._m is None:
            self._ensure_state(self._device())
        m, v = self._views(self._m), self._views(self._v)
        return {"iterations": int(self.iterations),
                "m": {n: t.clone() for n, t in zip(self._names, m)},
                "v": {n: t.clone() for n, t in zip(self._names, v)}}

    def load_state_dict(self, state_dict):
        for key in ("m", "v"):
            if sorted(state_dict[key]) != sorted(self._names):
                raise ValueError("state_dict['{}'] does not hold this optimiser's parameter names".format(key))
        self._ensure_state(self._device())
        with torch.no_grad():
            for key, flat in (("m", self._m), ("v", self._v)):
                for n, dst in zip(self._names, self._views(flat)):
                    src = state_dict[key][n]
                    if tuple(src.shape) != tuple(dst.shape):
                        raise ValueError("state_dict['{}']['{}'] has shape {}, expected {}".format(
                            key, n, tuple(src.shape), tuple(dst.shape)))
                    dst.copy_(src)
        self.iterations = int(state_dict["iterations"])

    # ---- the step ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = self._device()
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(
                "qpwcnet_amd: KerasAdamAGC.step cannot be captured in a torch.cuda graph yet; its step size changes "
                "with the step count, so a replayed capture would repeat one step's -- run the update eagerly")
        g = self.param_groups[0]
        lr = g["lr"](self.iterations) if callable(g["lr"]) else g["lr"]
        alpha = keras_step_size(float(lr), g["beta_1"], g["beta_2"], self.iterations + 1)
        clip = g["clip_factor"]
        clip = 0.0 if clip is None or clip <= 0 else float(clip)
        grads = []
        for n, p in self._named_params():
            gr = p.grad
            if gr is not None:
                if gr.is_sparse or gr.dtype != torch.float32 or gr.device != dev or gr.shape != p.shape:
                    raise ValueError("KerasAdamAGC: the gradient of {} must be a dense fp32 tensor of the parameter's "
                                     "shape on {}".format(n, dev))
                if not gr.is_contiguous():
                    gr = gr.contiguous()
            grads.append(gr)
        self._ensure_state(dev)
        if dev.type == "cuda":
            self._step_hip(dev, grads, alpha, g, clip)
        else:
            step_torch(self._named_params(), grads, self._views(self._m), self._views(self._v), alpha, g["beta_1"],
                       g["beta_2"], g["epsilon"], clip, g["eps"])
        self.iterations += 1
        return loss

    def _step_hip(self, dev, grads, alpha, g, clip):
        params = self._params()
        for n, p in zip(self._names, params):
            if not p.is_contiguous():
                raise ValueError("KerasAdamAGC: {} is not dense; the kernel updates parameters in place".format(n))
        L = _hip.lib()
        if self._units_dev is None:
            self._units_dev = self._units.to(dev)
        base_m, base_v = self._m.data_ptr(), self._v.data_ptr()
        ptrs = []
        for p, gr, o in zip(params, grads, self._offsets):
            ptrs += [p.data_ptr(), 0 if gr is None else gr.data_ptr(), base_m + 4 * o, base_v + 4 * o]
        if ptrs != self._ptrs:
            # .grad tensors come back at new addresses after zero_grad(set_to_none=True): an ordinary blocking copy
            # of a few KB from a fresh pageable tensor (a reused staging buffer could be overwritten in flight)
            host = torch.tensor(ptrs, dtype=torch.int64)
            if self._ptrs_dev is None:
                self._ptrs_dev = host.to(dev)
            else:
                self._ptrs_dev.copy_(host)
            self._ptrs = ptrs
        with torch.cuda.device(dev):
            rc = L.qpwc_agc_adam_step(self._ptrs_dev.data_ptr(), len(params), self._units_dev.data_ptr(),
                                      int(self._units_dev.shape[0]), alpha, g["beta_1"], g["beta_2"], g["epsilon"], clip,
                                      g["eps"], torch.cuda.current_stream(dev).cuda_stream)
        _hip.check(rc)

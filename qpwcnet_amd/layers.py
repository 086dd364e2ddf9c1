"""``torch.nn.Module`` twins of the reference's Keras hot-path layers
(qpwcnet/core/layers.py:32-186): ``CostVolume``, ``CostVolumeV2``, ``Warp``,
``WarpV2``, and trainable twins of the flow-estimator functors
(qpwcnet/core/non_layers.py:183-193, 213-273, 315-387): ``SeparableConv2D``,
``OptFlow``, ``Upsample``, ``Flow``, ``UpFlow``, and of the encoder (non_layers.py:390-449, pwcnet.py:134-168):
``DownConv``, ``Encoder``, of the decoder (non_layers.py:196-210, pwcnet.py:171-207): ``UpConv``, ``Decoder``, of
the whole ``build_flower`` network: ``FlowerModel``, and of the frame interpolator (layers.py:356-402,
pwcnet.py:70-131, 247-287): ``FrameInterpolate``, ``InterpolatorModel``.  Same names, same constructor
arguments, same ``layer((a, b))`` call convention, same config round trip; the
arithmetic, forward and backward, runs in the gfx950 HIP kernels behind
``include/qpwc.h``.

Layout is read from the process-global ``image_data_format()`` at construction
time exactly like the reference (layers.py:41,119,146,173); an explicit
``data_format=`` keyword (what the reference's test scripts try to pass,
test/test_cost_volume.py:10-11, test/test_warp.py:14-15) overrides it.
"""
import torch

from . import ops
from .backend import CHANNELS_FIRST, CHANNELS_LAST, get_axis, image_data_format


def lrelu(x):
    """qpwcnet/core/layers.py:15-16."""
    return torch.nn.functional.leaky_relu(x, 0.1)


def _get_axis(data_format):
    return get_axis(data_format)


class _HotPathLayer(torch.nn.Module):
    def __init__(self, *args, data_format=None, name=None, **kwargs):
        if args or kwargs:
            # Keras' Layer.__init__ rejects unknown arguments as well
            raise TypeError("unexpected arguments: {} {}".format(args, sorted(kwargs)))
        super().__init__()
        self.data_format = image_data_format() if data_format is None else data_format
        self.axis = _get_axis(self.data_format)  # ValueError('Unsupported data format : ...')
        self.layer_name = name
        self.h = None
        self.w = None

    def build(self, input_shapes):
        """Captures H, W from the first input's shape (layers.py:57-70, 153-164)."""
        shape = input_shapes[0]
        if self.data_format == CHANNELS_FIRST:
            self.h, self.w = shape[2], shape[3]
        elif self.data_format == CHANNELS_LAST:
            self.h, self.w = shape[1], shape[2]
        else:
            raise ValueError("Unsupported data format : {}".format(self.data_format))

    def _unpack(self, inputs):
        a, b = inputs
        self.build((tuple(a.shape), tuple(b.shape)))
        return a, b

    def call(self, inputs):  # Keras spelling
        return self.forward(inputs)

    def get_config(self):
        cfg = {"name": self.layer_name}
        cfg.update(getattr(self, "_config", {}))
        return cfg

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class CostVolume(_HotPathLayer):
    """qpwcnet/core/layers.py:32-109 -- pure-TF cost volume; here the HIP kernel."""

    def __init__(self, search_range=4, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._config = {"search_range": search_range}
        self.search_range = search_range

    def forward(self, inputs):
        prv, nxt = self._unpack(inputs)
        return ops.cost_volume(prv, nxt, self.search_range, self.data_format, 0.1)


class CostVolumeV2(CostVolume):
    """qpwcnet/core/layers.py:112-141 -- tfa CorrelationCost(1, r, 1, 1, r) + lrelu.
    Identical function to CostVolume (app/test/test_cvol_equal.py:25): same kernel."""


class Warp(_HotPathLayer):
    """qpwcnet/core/layers.py:144-168 -> tf_warp (qpwcnet/core/warp.py:63-153)."""

    def forward(self, inputs):
        img, flo = self._unpack(inputs)
        return ops.warp(img, flo, "tfwarp", self.data_format)


class WarpV2(_HotPathLayer):
    """qpwcnet/core/layers.py:171-186 -> tfa.image.dense_image_warp(img, -flo[..., ::-1])."""

    def forward(self, inputs):
        img, flo = self._unpack(inputs)
        return ops.warp(img, flo, "clamp", self.data_format)


class _Kernel(torch.nn.Module):
    """Holder of one `weight`, so that the state dict reads depthwise.weight / pointwise.weight like weights.py."""

    def __init__(self, shape):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(shape))
        torch.nn.init.xavier_uniform_(self.weight)   # Keras' glorot_uniform: the same fan_in + fan_out


class SeparableConv2D(_HotPathLayer):
    """tf.keras.layers.SeparableConv2D(filters, 3, padding='same', activation=...) as the reference uses it
    (qpwcnet/core/non_layers.py:223-231, 291-294): depthwise 3x3 + pointwise 1x1 + bias (+ Mish) in the fused HIP
    kernel, trainable through qpwc_sepconv3x3_bwd.  The call takes one tensor or a tuple / list of 1..3 sources that
    are read as their channel concatenation (never materialised): SeparableConv2D(115, 128)((cost, prv, flo)).
    Parameters in the torch layouts of weights.py: depthwise.weight (C,1,3,3), pointwise.weight (F,C,1,1), bias (F);
    Keras' default initialisers (Glorot-uniform kernels, zero bias).  fp32 only."""

    def __init__(self, in_channels, filters, activation="Mish", kernel_size=3, strides=1, padding="same",
                 use_bias=True, depth_multiplier=1, *args, **kwargs):
        super().__init__(*args, **kwargs)
        fixed = (("kernel_size", kernel_size, (3, (3, 3), [3, 3])), ("strides", strides, (1, (1, 1), [1, 1])),
                 ("padding", padding, ("same",)), ("use_bias", use_bias, (True,)),
                 ("depth_multiplier", depth_multiplier, (1,)))
        for key, value, allowed in fixed:
            if not any(type(value) is type(a) and value == a for a in allowed):
                raise ValueError("SeparableConv2D: {}={!r} is not supported (the reference uses {!r})".format(
                    key, value, allowed[0]))
        if activation not in ("Mish", None):
            raise ValueError("SeparableConv2D: activation must be 'Mish' or None, got {!r}".format(activation))
        if int(in_channels) < 1 or int(filters) not in (16, 32, 64, 128):
            raise ValueError("SeparableConv2D: in_channels >= 1 and filters in (16, 32, 64, 128), got {} -> {}".format(
                in_channels, filters))
        self.in_channels, self.filters, self.activation = int(in_channels), int(filters), activation
        self._config = {"in_channels": self.in_channels, "filters": self.filters, "activation": activation}
        self.depthwise = _Kernel((self.in_channels, 1, 3, 3))
        self.pointwise = _Kernel((self.filters, self.in_channels, 1, 1))
        self.bias = torch.nn.Parameter(torch.zeros(self.filters))

    def forward(self, inputs):
        sources = list(inputs) if isinstance(inputs, (tuple, list)) else [inputs]
        if not 1 <= len(sources) <= 3:
            raise ValueError("SeparableConv2D takes 1..3 sources, got {}".format(len(sources)))
        self.build([tuple(t.shape) for t in sources])
        if sum(t.shape[self.axis] for t in sources) != self.in_channels:
            raise ValueError("SeparableConv2D: the sources hold {} channels, the layer {}".format(
                [t.shape[self.axis] for t in sources], self.in_channels))
        if self.data_format == CHANNELS_FIRST:
            # with grad the permuted view keeps the source in the autograd graph (ops makes it dense inside)
            sources = [t.permute(0, 2, 3, 1) if ops._wants_grad(t) else ops._to_nhwc(t, CHANNELS_FIRST) for t in sources]
        out = ops.sepconv3x3(sources, self.depthwise.weight, ops.pad_pointwise(self.pointwise.weight), self.bias,
                             mish_on_load=False, mish_on_store=self.activation == "Mish")
        return ops._from_nhwc(out, self.data_format)


class _Conv(torch.nn.Module):
    """Holder of a convolution's `weight` (and `bias`): conv.weight / conv.bias / flow.weight like weights.py."""

    def __init__(self, shape, bias):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(shape))
        torch.nn.init.xavier_uniform_(self.weight)   # Keras' glorot_uniform
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(shape[0]))


class _BatchNorm(torch.nn.Module):
    """Keras BatchNormalization's variables under the names of weights.py: gamma, beta; moving mean / var as buffers."""

    def __init__(self, channels):
        super().__init__()
        self.gamma = torch.nn.Parameter(torch.ones(channels))
        self.beta = torch.nn.Parameter(torch.zeros(channels))
        self.register_buffer("mean", torch.zeros(channels))
        self.register_buffer("var", torch.ones(channels))


class OptFlow(_HotPathLayer):
    """The flow estimator of one pyramid level (qpwcnet/core/non_layers.py:213-273), trainable: four
    SeparableConv2D(3x3, 'same', Mish) -> Conv2D(1x1, Mish) -> BatchNormalization(fused=False) -> Conv2D(3x3, 2
    filters, no bias) -> * scale, scale=None meaning sqrt(h^2 + w^2).  The last SeparableConv2D stores its
    pre-activation and the head applies that layer's Mish on load, as the kernels expect.  The call takes one tensor
    or a tuple / list of 1..3 sources read as their channel concatenation.  ``self.training`` selects the BatchNorm
    mode: batch statistics and an in-place update of the moving buffers (Keras' momentum 0.99, epsilon 1e-3, biased
    variance), or the moving statistics.  State-dict names are those of weights.py, so a converted checkpoint's
    ``<prefix>flow.*`` entries load with load_state_dict.  fp32 only."""
    MOMENTUM = 0.99
    EPSILON = 1e-3

    def __init__(self, in_channels, filters=(128, 64, 32, 16), scale=None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        filters = tuple(int(f) for f in filters)
        if not filters or filters[-1] != 16:
            raise ValueError("OptFlow: the flow head takes 16 channels, got filters {}".format(filters))
        self.in_channels, self.filters, self.scale = int(in_channels), filters, scale
        self._config = {"in_channels": self.in_channels, "filters": filters, "scale": scale}
        chans = (self.in_channels,) + filters
        # the stack runs channels-last inside; this layer converts at its own boundary
        self.feat = torch.nn.ModuleList(
            SeparableConv2D(chans[i], f, activation="Mish" if i + 1 < len(filters) else None, data_format=CHANNELS_LAST)
            for i, f in enumerate(filters))
        self.conv = _Conv((16, 16, 1, 1), bias=True)
        self.norm = _BatchNorm(16)
        self.flow = _Conv((2, 16, 3, 3), bias=False)

    def forward(self, inputs):
        sources = list(inputs) if isinstance(inputs, (tuple, list)) else [inputs]
        if not 1 <= len(sources) <= 3:
            raise ValueError("OptFlow takes 1..3 sources, got {}".format(len(sources)))
        self.build([tuple(t.shape) for t in sources])
        if self.data_format == CHANNELS_FIRST:
            sources = [t.permute(0, 2, 3, 1) if ops._wants_grad(t) else ops._to_nhwc(t, CHANNELS_FIRST) for t in sources]
        scale = self.scale if self.scale is not None else float(self.h ** 2 + self.w ** 2) ** 0.5
        z = sources
        for layer in self.feat:
            z = layer(z)
        out = ops.flow_head_train(z, self.conv.weight, self.conv.bias, self.norm.gamma, self.norm.beta, self.norm.mean,
                                  self.norm.var, self.flow.weight, scale, training=self.training,
                                  momentum=self.MOMENTUM, eps=self.EPSILON)
        return ops._from_nhwc(out, self.data_format)


class Upsample(_HotPathLayer):
    """qpwcnet/core/non_layers.py:183-193 on a flow: scale * UpSampling2D(2, 'bilinear'), differentiable."""

    def __init__(self, scale=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.scale = float(scale)
        self._config = {"scale": self.scale}

    def forward(self, x):
        return ops.upsample2x_flow(x, self.scale, self.data_format, self.data_format)


class Flow(_HotPathLayer):
    """First flow block (qpwcnet/core/non_layers.py:315-338), trainable: cost = CostVolumeV2(prv, nxt);
    OptFlow(concat[cost, prv, nxt]).  in_channels: the channels of prv / nxt."""

    def __init__(self, in_channels, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.in_channels = int(in_channels)
        self._config = {"in_channels": self.in_channels}
        self.cost_volume = CostVolumeV2(data_format=self.data_format)
        self.flow = OptFlow(81 + 2 * self.in_channels, data_format=self.data_format)

    def forward(self, inputs):
        prv, nxt = inputs
        return self.flow((self.cost_volume((prv, nxt)), prv, nxt))


class UpFlow(_HotPathLayer):
    """Refinement block (qpwcnet/core/non_layers.py:341-387), trainable: nxt_w = WarpV2(nxt, flo); cost =
    CostVolumeV2(prv, nxt_w); OptFlow(concat[cost, prv, flo]).  in_channels: the channels of prv / nxt."""

    def __init__(self, in_channels, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.in_channels = int(in_channels)
        self._config = {"in_channels": self.in_channels}
        self.warp = WarpV2(data_format=self.data_format)
        self.cost_volume = CostVolumeV2(data_format=self.data_format)
        self.flow = OptFlow(81 + self.in_channels + 2, data_format=self.data_format)

    def forward(self, inputs):
        prv, nxt, flo = inputs
        return self.flow((self.cost_volume((prv, self.warp((nxt, flo)))), prv, flo))


class DownConv(_HotPathLayer):
    """One encoder level (qpwcnet/core/non_layers.py:390-449 with use_normalizer=False, pwcnet.py:145-146), trainable:
    Conv2D(filters, 3x3, strides 2, 'same', Mish) -> two Conv2D(filters, 3x3, 'same', Mish), forward and backward in
    the HIP kernels behind ops.conv3x3_same.  State-dict names as weights.py: conv_a / conv_aa / conv_b .weight and
    .bias in the torch layout; Keras' default initialisers (Glorot-uniform kernels, zero bias).  fp32 only."""

    def __init__(self, in_channels, filters, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.in_channels, self.filters = int(in_channels), int(filters)
        if self.in_channels not in ops._CONV_SAME_CIN or self.filters not in ops._CONV_SAME_COUT:
            raise ValueError("DownConv: in_channels in {} and filters in {}, got {} -> {}".format(
                ops._CONV_SAME_CIN, ops._CONV_SAME_COUT, in_channels, filters))
        self._config = {"in_channels": self.in_channels, "filters": self.filters}
        self.conv_a = _Conv((self.filters, self.in_channels, 3, 3), bias=True)
        self.conv_aa = _Conv((self.filters, self.filters, 3, 3), bias=True)
        self.conv_b = _Conv((self.filters, self.filters, 3, 3), bias=True)

    def forward_nhwc(self, x):
        x = ops.conv3x3_same(x, self.conv_a.weight, self.conv_a.bias, stride=2)
        x = ops.conv3x3_same(x, self.conv_aa.weight, self.conv_aa.bias)
        return ops.conv3x3_same(x, self.conv_b.weight, self.conv_b.bias)

    def forward(self, x):
        self.build((tuple(x.shape),))
        if x.shape[self.axis] != self.in_channels:
            raise ValueError("DownConv: the input holds {} channels, the layer {}".format(x.shape[self.axis],
                                                                                         self.in_channels))
        return ops._from_nhwc(self.forward_nhwc(_dense_nhwc(x, self.data_format)), self.data_format)


def _dense_nhwc(t, data_format):
    """Dense channels-last form of a layer input; with grad through torch's own copy, which autograd follows."""
    if ops._wants_grad(t):
        return (t if data_format == CHANNELS_LAST else t.permute(0, 2, 3, 1)).contiguous()
    return ops._to_nhwc(t, data_format)


class Encoder(_HotPathLayer):
    """The feature pyramid (qpwcnet/core/pwcnet.py:134-168), trainable: one DownConv per entry of `filters`, shared by
    both frames, which are stacked on the batch axis for one pass and split afterwards.  The call is
    encoder((img_prv, img_nxt), output_features=False) -> (feature_prv, feature_nxt) of the coarsest level, or with
    output_features the two lists [img, level 1, ..., level n].  State-dict names enc.{i}.conv_a.weight ... are those of
    weights.py / synth.make_weights: a converted checkpoint loads with load_state_dict(strict=False).  The stack runs
    channels-last inside; this layer converts at its own boundary."""

    def __init__(self, filters=(16, 32, 64, 128, 256), in_channels=3, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.filters, self.in_channels = tuple(int(f) for f in filters), int(in_channels)
        if not self.filters:
            raise ValueError("Encoder: no filters")
        self._config = {"filters": self.filters, "in_channels": self.in_channels}
        chans = (self.in_channels,) + self.filters
        self.enc = torch.nn.ModuleList(DownConv(chans[i], f, data_format=CHANNELS_LAST)
                                       for i, f in enumerate(self.filters))

    def forward(self, inputs, output_features=False):
        img_prv, img_nxt = self._unpack(inputs)
        if img_prv.shape != img_nxt.shape or img_prv.shape[self.axis] != self.in_channels:
            raise ValueError("Encoder: two frames of one shape with {} channels, got {} and {}".format(
                self.in_channels, tuple(img_prv.shape), tuple(img_nxt.shape)))
        n = img_prv.shape[0]
        f = _dense_nhwc(torch.cat([img_prv, img_nxt], dim=0), self.data_format)
        feats_prv, feats_nxt = [img_prv], [img_nxt]
        for layer in self.enc:
            f = layer.forward_nhwc(f)
            feats_prv.append(ops._from_nhwc(f[:n], self.data_format))
            feats_nxt.append(ops._from_nhwc(f[n:], self.data_format))
        if output_features:
            return feats_prv, feats_nxt
        return feats_prv[-1], feats_nxt[-1]

    def forward_stacked(self, frames):
        """The pyramid of 2n stacked frames [prv; nxt] (dense channels-last, (2n,H,W,C)) -> [level 1, ..., level n],
        stacked and channels-last as the levels compute them: what layers.Decoder.forward_stacked and FlowerModel
        take, without the split and re-concatenation of forward()."""
        return _encode_stacked(self.enc, frames)


def _encode_stacked(levels, f):
    feats = []
    for layer in levels:
        f = layer.forward_nhwc(f)
        feats.append(f)
    return feats


class _ConvT(torch.nn.Module):
    """Holder of a transposed convolution's `weight` (C_in, F, k, k) and `bias` (F): conv_up.weight / conv_up.bias."""

    def __init__(self, shape):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(shape))
        torch.nn.init.xavier_uniform_(self.weight)   # Keras' glorot_uniform: fan_in + fan_out = (C_in + F) k k either way
        self.bias = torch.nn.Parameter(torch.zeros(shape[1]))


class UpConv(_HotPathLayer):
    """One decoder level (qpwcnet/core/non_layers.py:196-210), trainable: Conv2DTranspose(filters, 4x4, strides 2,
    'same') + Mish, forward and backward in the HIP kernels behind ops.upconv4x4s2.  UpConv(x) -> the upsampled
    features; UpConv.cat_skip(x, skip) -> concat([UpConv(x), skip]) on the channel axis (pwcnet.py:186-195), written by
    the layer's own launch, with the gradient of the concat read in place.  State-dict names as weights.py:
    conv_up.weight (C, F, 4, 4), conv_up.bias (F); Keras' default initialisers.  fp32 only."""

    def __init__(self, in_channels, filters, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.in_channels, self.filters = int(in_channels), int(filters)
        if self.in_channels not in ops._UPCONV_C or self.filters not in ops._UPCONV_F:
            raise ValueError("UpConv: in_channels in {} and filters in {}, got {} -> {}".format(
                ops._UPCONV_C, ops._UPCONV_F, in_channels, filters))
        self._config = {"in_channels": self.in_channels, "filters": self.filters}
        self.conv_up = _ConvT((self.in_channels, self.filters, 4, 4))

    def forward_nhwc(self, x, skip=None):
        return ops.upconv4x4s2(x, self.conv_up.weight, self.conv_up.bias, skip)

    def _check(self, x):
        self.build((tuple(x.shape),))
        if x.shape[self.axis] != self.in_channels:
            raise ValueError("UpConv: the input holds {} channels, the layer {}".format(x.shape[self.axis],
                                                                                       self.in_channels))

    def forward(self, x):
        self._check(x)
        return ops._from_nhwc(self.forward_nhwc(_dense_nhwc(x, self.data_format)), self.data_format)

    def cat_skip(self, x, skip):
        self._check(x)
        if self.data_format == CHANNELS_FIRST:
            skip = skip.permute(0, 2, 3, 1) if ops._wants_grad(skip) else ops._to_nhwc(skip, CHANNELS_FIRST)
        return ops._from_nhwc(self.forward_nhwc(_dense_nhwc(x, self.data_format), skip), self.data_format)


def _decode_stacked(levels, feats, use_skip):
    f, decs = feats[-1], []
    for i, layer in enumerate(levels):
        f = layer.forward_nhwc(f, feats[-2 - i] if use_skip else None)
        decs.append(f)
    return decs


class Decoder(_HotPathLayer):
    """The feature decoder (qpwcnet/core/pwcnet.py:171-207), trainable: one UpConv per entry of `filters`, each
    concatenated with the encoder feature of its resolution (`skip_channels`: that feature's channels per level; None
    is the reference's use_skip=False).  The call is decoder((encs_prv, encs_nxt)) on the two feature lists of
    Encoder(..., output_features=True) -> (decs_prv, decs_nxt); both frames go through one launch per level, stacked
    on the batch axis.  A level's input width, in_channels or the concat of the level before, must be one the
    transposed convolution takes (64, 128, 256).  State-dict names dec.{i}.conv_up.* are those of weights.py."""

    def __init__(self, filters=(128, 64, 32, 16), in_channels=256, skip_channels=(128, 64, 32, 16), *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.filters, self.in_channels = tuple(int(f) for f in filters), int(in_channels)
        self.skip_channels = None if skip_channels is None else tuple(int(c) for c in skip_channels)
        if not self.filters or (self.skip_channels is not None and len(self.skip_channels) != len(self.filters)):
            raise ValueError("Decoder: one skip width per filter, got {} and {}".format(filters, skip_channels))
        self._config = {"filters": self.filters, "in_channels": self.in_channels, "skip_channels": self.skip_channels}
        levels, c = [], self.in_channels
        for i, f in enumerate(self.filters):
            levels.append(UpConv(c, f, data_format=CHANNELS_LAST))
            c = f + (self.skip_channels[i] if self.skip_channels is not None else 0)
        self.dec = torch.nn.ModuleList(levels)

    def forward_stacked(self, feats):
        """Stacked channels-last encoder levels [..., level n] (Encoder.forward_stacked) -> the stacked decoder levels."""
        return _decode_stacked(self.dec, feats, self.skip_channels is not None)

    def forward(self, inputs):
        encs_prv, encs_nxt = inputs
        need = len(self.dec) + 1 if self.skip_channels is not None else 1
        if len(encs_prv) != len(encs_nxt) or len(encs_prv) < need:
            raise ValueError("Decoder: two feature lists of at least {} levels, got {} and {}".format(
                need, len(encs_prv), len(encs_nxt)))
        self.build((tuple(encs_prv[-1].shape),))
        n = encs_prv[-1].shape[0]
        feats = [_dense_nhwc(torch.cat([a, b], dim=0), self.data_format)
                 for a, b in zip(encs_prv[-need:], encs_nxt[-need:])]
        decs = self.forward_stacked(feats)
        return ([ops._from_nhwc(d[:n], self.data_format) for d in decs],
                [ops._from_nhwc(d[n:], self.data_format) for d in decs])


class FlowerModel(_HotPathLayer):
    """The whole flow network of build_flower (qpwcnet/core/pwcnet.py:210-244 with train=True), trainable: Encoder,
    Decoder, the coarsest Flow and one UpFlow per decoder level with Upsample(2.0) between the levels and at the end.
    The input is the frame pair (B,H,W,6), or (B,6,H,W) for channels_first; the result is the list of multi-scale flows,
    coarse to fine, plus the final upsample-only one -- what loss.multiscale takes.  Every parameter receives a
    gradient from HIP kernels.  State-dict names enc.*, dec.*, flow.flow.*, upflow.{i}.flow.* are those of weights.py /
    synth.make_weights, so a converted checkpoint loads with load_state_dict.  train() / eval() select the BatchNorm
    mode of every OptFlow.  The stack runs channels-last inside; this layer converts at its own boundary."""

    def __init__(self, enc_filters=(16, 32, 64, 128, 256), dec_filters=(128, 64, 32, 16), *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.enc_filters = tuple(int(f) for f in enc_filters)
        self.dec_filters = tuple(int(f) for f in dec_filters)
        if not self.enc_filters or len(self.dec_filters) >= len(self.enc_filters):
            raise ValueError("{}: fewer decoder levels than encoder levels, got {} and {}".format(
                type(self).__name__, enc_filters, dec_filters))
        self._config = {"enc_filters": self.enc_filters, "dec_filters": self.dec_filters}
        skips = tuple(self.enc_filters[-2 - i] for i in range(len(self.dec_filters)))
        self.enc = Encoder(self.enc_filters, data_format=CHANNELS_LAST).enc
        self.dec = Decoder(self.dec_filters, self.enc_filters[-1], skips, data_format=CHANNELS_LAST).dec
        self.flow = Flow(self.enc_filters[-1], data_format=CHANNELS_LAST)
        self.upflow = torch.nn.ModuleList(UpFlow(f + c, data_format=CHANNELS_LAST)
                                          for f, c in zip(self.dec_filters, skips))
        self.up = Upsample(2.0, data_format=CHANNELS_LAST)

    def _pyramids(self, pairs):
        """The frame pair -> (n, the 2n stacked channels-last frames [prv; nxt], their encoder levels, their decoder
        levels)."""
        if pairs.dim() != 4 or pairs.shape[self.axis] != 6:
            raise ValueError("{}: a frame pair with 6 channels on axis {}, got {}".format(
                type(self).__name__, self.axis, tuple(pairs.shape)))
        self.build((tuple(pairs.shape),))
        prv, nxt = torch.chunk(pairs, 2, dim=self.axis)
        frames = _dense_nhwc(torch.cat([prv, nxt], dim=0), self.data_format)
        feats = _encode_stacked(self.enc, frames)
        return pairs.shape[0], frames, feats, _decode_stacked(self.dec, feats, True)

    def _flow_stack(self, enc_prv, enc_nxt, decs_prv, decs_nxt):
        """The estimated flows of one direction, coarse to fine (pwcnet.py:28-64): Flow, then Upsample(2.0) + UpFlow per
        decoder level."""
        flo = self.flow((enc_prv, enc_nxt))
        flows = [flo]
        for d_prv, d_nxt, upflow in zip(decs_prv, decs_nxt, self.upflow):
            flo = upflow((d_prv, d_nxt, self.up(flo)))
            flows.append(flo)
        return flows

    def forward(self, pairs):
        n, _, feats, decs = self._pyramids(pairs)
        flows = self._flow_stack(feats[-1][:n], feats[-1][n:], [d[:n] for d in decs], [d[n:] for d in decs])
        flows.append(self.up(flows[-1]))
        return [ops._from_nhwc(f, self.data_format) for f in flows]


class FrameInterpolate(_HotPathLayer):
    """One block of the interpolation stack (qpwcnet/core/layers.py:356-402, non_layers.py:276-312), trainable: both
    inputs warped half way along their flows, nxt_w = WarpV2(nxt, 0.5 flo_01) and prv_w = WarpV2(prv, 0.5 flo_10), then
    concat [prv_w, nxt_w, flo_01, flo_10 (, img_u)] -> SeparableConv2D(64, 3x3, 'same', Mish) -> Conv2D(3, 1x1).  The
    call takes (prv, nxt, flo_01, flo_10) or, with up=True, (prv, nxt, flo_01, flo_10, img_u), img_u being the
    upsampled image of the level before.  The two warped members are read by the separable convolution as a virtual
    concat; where in_channels is no multiple of 4 (the coarsest block, on the 3-channel frames) the concat is one dense
    tensor.  State-dict names as weights.py: conv1.depthwise.weight, conv1.pointwise.weight, conv1.bias, conv2.weight
    (3,64,1,1), conv2.bias; Keras' default initialisers.  in_channels: the channels of prv / nxt.  fp32 only."""
    FILTERS = 64

    def __init__(self, in_channels, up=False, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.in_channels, self.up = int(in_channels), bool(up)
        if self.in_channels < 1:
            raise ValueError("FrameInterpolate: in_channels >= 1, got {}".format(in_channels))
        self._config = {"in_channels": self.in_channels, "up": self.up}
        # the block runs channels-last inside; this layer converts at its own boundary
        self.conv1 = SeparableConv2D(2 * self.in_channels + 4 + (3 if self.up else 0), self.FILTERS, "Mish",
                                     data_format=CHANNELS_LAST)
        self.conv2 = _Conv((3, self.FILTERS, 1, 1), bias=True)

    def _head(self, prv_w, nxt_w, rest):
        small = torch.cat(rest, dim=3)
        if self.in_channels % 4:
            sources = [torch.cat([prv_w, nxt_w, small], dim=3)]
        else:
            sources = [prv_w, nxt_w, small]
        return ops.image_head(self.conv1(sources), self.conv2.weight, self.conv2.bias)

    def _check(self, tensors, shape):
        B, H, W = shape[0], shape[1], shape[2]
        want = [(B, H, W, c) for c in (self.in_channels, self.in_channels, 2, 2, 3)][:len(tensors)]
        if len(tensors) != (5 if self.up else 4) or [tuple(t.shape) for t in tensors] != want:
            raise ValueError("FrameInterpolate(in_channels={}, up={}): got the shapes {}".format(
                self.in_channels, self.up, [tuple(t.shape) for t in tensors]))

    def forward_nhwc(self, prv, nxt, flo_01, flo_10, img_u=None):
        nxt_w = ops.warp(nxt, 0.5 * flo_01, "clamp")
        prv_w = ops.warp(prv, 0.5 * flo_10, "clamp")
        return self._head(prv_w, nxt_w, [flo_01, flo_10] + ([img_u] if self.up else []))

    def forward(self, inputs):
        tensors = [_dense_nhwc(t, self.data_format) for t in inputs]
        self.build((tuple(inputs[0].shape),))
        self._check(tensors, tensors[0].shape)
        return ops._from_nhwc(self.forward_nhwc(*tensors), self.data_format)

    def forward_stacked(self, swapped, flows, img_u=None):
        """The same block with both warps in one launch (non_layers.FrameInterpolate.call_stacked of the no-grad
        network): `swapped` = [nxt; prv] and `flows` = [flo_01; flo_10] stacked on the batch axis (2n), dense
        channels-last, img_u (n,H,W,3) with up=True.  The bits of the plain call."""
        n = swapped.shape[0] // 2
        rest = [flows[:n], flows[n:]] + ([img_u] if self.up else [])
        self._check([swapped[n:], swapped[:n]] + rest, swapped[:n].shape)
        w = ops.warp(swapped, 0.5 * flows, "clamp")     # [nxt_w; prv_w]
        return self._head(w[n:], w[:n], rest)


class InterpolatorModel(FlowerModel):
    """The whole frame interpolator of build_interpolator (qpwcnet/core/pwcnet.py:247-287, 70-131), trainable: the
    encoder, decoder and flow stack of FlowerModel, the flow stack run in both directions with the same modules --
    flows_01 = flower(enc_nxt, enc_prv, decs_nxt, decs_prv), then flows_10 with the roles swapped, two passes in that
    order in train() and eval() alike, so that every BatchNormalization takes its batch statistics per call and moves
    its moving buffers twice per step as the reference's does -- and one FrameInterpolate block per level.  The coarsest
    block reads the input frames pooled len(enc_filters) times (ops.avgpool_pyramid: the reference's n+1 poolings for
    its own configuration, the coarsest feature size for any other), every finer one the decoder features of its level
    and the upsampled image of the level before (ops.upsample2x_image); the last image is upsample-only.  The final
    upsample-only flow of each direction is not needed and not computed.  The input is the frame pair (B,H,W,6), or
    (B,6,H,W) for channels_first; the result is the list of len(dec_filters) + 2 images, coarse to fine -- what
    loss.multiscale(loss.AutoResizeMseLoss(), ...) takes -- or with output_multiscale=False the last one.  State-dict
    names enc.*, dec.*, flow.flow.*, upflow.{i}.flow.*, img.{k}.conv1.*, img.{k}.conv2.* are those of
    synth.make_interpolator_weights; a FlowerModel state dict loads with strict=False and leaves img.* missing (the
    reference's flow-to-interpolator weight transfer, pwcnet.py:276-279)."""

    def __init__(self, enc_filters=(16, 32, 64, 128, 256), dec_filters=(128, 64, 32, 16), output_multiscale=True,
                 *args, **kwargs):
        super().__init__(enc_filters, dec_filters, *args, **kwargs)
        self.output_multiscale = bool(output_multiscale)
        self._config["output_multiscale"] = self.output_multiscale
        self.img = torch.nn.ModuleList(
            [FrameInterpolate(3, up=False, data_format=CHANNELS_LAST)] +
            [FrameInterpolate(u.in_channels, up=True, data_format=CHANNELS_LAST) for u in self.upflow])

    def forward(self, pairs):
        n, frames, feats, decs = self._pyramids(pairs)
        enc_prv, enc_nxt = feats[-1][:n], feats[-1][n:]
        decs_prv, decs_nxt = [d[:n] for d in decs], [d[n:] for d in decs]
        flows_01 = self._flow_stack(enc_nxt, enc_prv, decs_nxt, decs_prv)
        flows_10 = self._flow_stack(enc_prv, enc_nxt, decs_prv, decs_nxt)
        # the pooling is per image: the stacked [prv; nxt] frames give the reference's two pyramids in one launch
        small = ops.avgpool_pyramid(frames.detach(), len(self.enc_filters))
        img = self.img[0].forward_nhwc(small[:n], small[n:], flows_01[0], flows_10[0])
        imgs = [img]
        for i, block in enumerate(self.img[1:]):
            img = block.forward_nhwc(decs_prv[i], decs_nxt[i], flows_01[i + 1], flows_10[i + 1],
                                     ops.upsample2x_image(img))
            imgs.append(img)
        imgs.append(ops.upsample2x_image(img))
        if not self.output_multiscale:
            return ops._from_nhwc(imgs[-1], self.data_format)
        return [ops._from_nhwc(t, self.data_format) for t in imgs]

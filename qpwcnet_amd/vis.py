"""The functions of the reference's ``qpwcnet/core/vis.py`` that touch the network's data.

``cost_volume_to_flow`` (vis.py:9-34) decodes a cost volume into the displacement of its strongest correlation -- the
in-tree statement of the channel order ``i0 * 9 + j0``.

``flow_to_image`` (vis.py:37-76) colours a flow by direction (hue) and by magnitude relative to the image's own maximum
(saturation); ``flow_panels`` is what the trainer's ``ShowImageCallback.on_batch_end`` builds from it at every logging
step: the label and every predicted flow coloured, nearest-resized to one size and converted to uint8, channels-last.
HIP tensors take two launches for all flows together (``qpwc_flow_to_image_fwd``, include/qpwc_vis.h, DESIGN.md section
4.22); CPU tensors take ``flow_to_image_torch``, the same chain from torch operators.  The drawing helpers around them
(cv2 windows, TensorBoard writing, the overlay panels of test_infer.py) stay out of scope, DESIGN.md section 8."""
import math

import torch

from . import ops
from .backend import CHANNELS_FIRST, CHANNELS_LAST, get_axis, image_data_format


def cost_volume_to_flow(cvol, data_format=None):
    if data_format is None:
        data_format = image_data_format()
    return ops.cost_volume_to_flow(cvol, data_format)


def nearest_index(n_out, n_in, device=None):
    """Source index of every output index of tf.image.resize(..., NEAREST_NEIGHBOR) along one axis (TF2's half-pixel
    rule): min(floor((i + 0.5) * (float32(n_in) / n_out)), n_in - 1), in fp32 as the kernel computes it."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    i = torch.arange(n_out, dtype=torch.float32, device=device)
    return torch.floor((i + 0.5) * scale.to(i.device)).long().clamp_(max=n_in - 1)


def to_uint8(img):
    """tf.image.convert_image_dtype(img, uint8, saturate=True) of a float image in [0, 1]: trunc(x * 255.5), clamped."""
    return torch.trunc(img.float() * 255.5).clamp_(0.0, 255.0).to(torch.uint8)


def flow_to_image_torch(flow, data_format=CHANNELS_LAST, size=None, dtype=torch.float32, out_format=None):
    """``flow_to_image`` composed from torch operators, on any device: the path CPU tensors take and the baseline the
    kernels are timed against.  size = (oh, ow): nearest-resized; dtype torch.uint8: converted by ``to_uint8``;
    out_format: the picture's data format (default: the flow's)."""
    axis = get_axis(data_format)
    out_format = data_format if out_format is None else out_format
    get_axis(out_format)
    single = flow.dim() == 3
    f = (flow[None] if single else flow).float()
    fx, fy = f.select(axis, 0), f.select(axis, 1)                      # (B, h, w)
    hue = (torch.atan2(fy, fx) + math.pi) / (2.0 * math.pi)
    mag = torch.sqrt(fx * fx + fy * fy)
    smax = mag.amax(dim=(-2, -1), keepdim=True)
    s = mag / (smax + 1e-6)
    dh = 6.0 * hue
    d = torch.stack([((dh - 3.0).abs() - 1.0).clamp(0.0, 1.0), (2.0 - (dh - 2.0).abs()).clamp(0.0, 1.0),
                     (2.0 - (dh - 4.0).abs()).clamp(0.0, 1.0)], dim=-1 if out_format == CHANNELS_LAST else 1)
    s = s.unsqueeze(-1 if out_format == CHANNELS_LAST else 1)
    img = (1.0 - s) + s * d
    if size is not None:
        ya, xa = (1, 2) if out_format == CHANNELS_LAST else (2, 3)
        oh, ow = (int(v) for v in size)
        if (oh, ow) != (img.shape[ya], img.shape[xa]):
            img = img.index_select(ya, nearest_index(oh, img.shape[ya], img.device))
            img = img.index_select(xa, nearest_index(ow, img.shape[xa], img.device))
    if dtype == torch.uint8:
        img = to_uint8(img)
    elif dtype != torch.float32:
        raise ValueError("dtype must be torch.float32 or torch.uint8, got {}".format(dtype))
    return img[0] if single else img


def _check_flow(flow, data_format, name="flow"):
    if not isinstance(flow, torch.Tensor):
        raise TypeError("{} must be a torch.Tensor".format(name))
    if flow.dtype not in (torch.float32, torch.float16):
        raise ValueError("{}: unsupported dtype {}".format(name, flow.dtype))
    if flow.dim() not in (3, 4) or flow.shape[-1 if data_format == CHANNELS_LAST else -3] != 2:
        raise ValueError("{} must be (...,h,w,2) channels_last or (...,2,h,w) channels_first of rank 3 or 4, got "
                         "shape {}".format(name, tuple(flow.shape)))


def flow_to_image(flow, data_format='channels_last'):
    """qpwcnet/core/vis.py:37-76: a flow (h,w,2) / (B,h,w,2) or, channels_first, (2,h,w) / (B,2,h,w), fp32 or fp16 ->
    its fp32 RGB picture in the same data format; hue from the direction, saturation from the magnitude over the
    image's own maximum (+ 1e-6), value 1.  An all-zero image is white."""
    get_axis(data_format)
    _check_flow(flow, data_format)
    if not flow.is_cuda:
        return flow_to_image_torch(flow, data_format)
    single = flow.dim() == 3
    img = ops.flow_to_image([flow[None] if single else flow], None, data_format, torch.float32, data_format)[0]
    return img[0] if single else img


def flow_panels(flows, size=None, data_format=None, dtype=torch.uint8):
    """The pictures ShowImageCallback.on_batch_end hands to tf.summary.image (qpwcnet/app/optical_flow/train.py:212-244):
    1..8 batched flows of different sizes, e.g. ``[label] + list(model(ims))``, in ``data_format`` (default
    ``backend.image_data_format()``) -> a list of (B,H,W,3) channels-last images of ``size`` (default: the first flow's
    (H, W)), each coloured by its own per-image maximum at its own size and then nearest-resized, uint8 (what the
    summary writer converts to) or float32 by ``dtype``.  HIP tensors: all of them in one call of the C entry point."""
    if data_format is None:
        data_format = image_data_format()
    get_axis(data_format)
    flows = list(flows)
    if not flows:
        raise ValueError("flow_panels needs at least one flow")
    for i, f in enumerate(flows):
        _check_flow(f, data_format, "flows[%d]" % i)
        if f.dim() != 4:
            raise ValueError("flows[{}] must be batched (rank 4), got shape {}".format(i, tuple(f.shape)))
    if size is None:
        size = flows[0].shape[1:3] if data_format == CHANNELS_LAST else flows[0].shape[2:4]
    size = tuple(int(v) for v in size)
    if not flows[0].is_cuda:
        return [flow_to_image_torch(f, data_format, size, dtype, CHANNELS_LAST) for f in flows]
    return ops.flow_to_image(flows, [size] * len(flows), data_format, dtype, CHANNELS_LAST)

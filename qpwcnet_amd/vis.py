"""The functions of the reference's ``qpwcnet/core/vis.py`` that touch the network's data.

``cost_volume_to_flow`` (vis.py:9-34) decodes a cost volume into the displacement of its strongest correlation -- the
in-tree statement of the channel order ``i0 * 9 + j0``.

``flow_to_image`` (vis.py:37-76) colours a flow by direction (hue) and by magnitude relative to the image's own maximum
(saturation); ``flow_panels`` is what the trainer's ``ShowImageCallback.on_batch_end`` builds from it at every logging
step: the label and every predicted flow coloured, nearest-resized to one size and converted to uint8, channels-last.
HIP tensors take two launches for all flows together (``qpwc_flow_to_image_fwd``, include/qpwc_vis.h, DESIGN.md section
4.22); CPU tensors take ``flow_to_image_torch``, the same chain from torch operators.

``inference_panels`` and ``interpolation_panels`` are the pictures the two test scripts show after training
(app/optical_flow/test_infer.py:104-154: frames, warps, overlays, differences and both flows in colour;
app/frame_interpolation/pre_train_test.py:45-79, 121-163: frames, ground truth, prediction, overlay, flow, the warped
middle frame, ``_show``'s alignment grid and its 8-bit export).  HIP tensors take two launches per call
(include/qpwc_review.h); CPU tensors take ``inference_panels_torch`` /
``interpolation_panels_torch``.  What stays out of scope is the drawing itself (cv2 windows, cv2.imwrite, TensorBoard
writing), DESIGN.md section 8."""
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


# ---- the review panels of the two test scripts -----------------------------------------------------------------------
INFERENCE_PANELS = ("prv", "nxt", "nxt_w", "overlay", "overlay_warped", "overlay_warped_gt", "delta_warped",
                    "delta_warped_gt", "flo_rgb", "flo_pred_rgb")
INTERPOLATION_PANELS = ("0-prv", "1-nxt", "2-ground-truth", "3-pred", "4-overlay", "5-flow", "6-warp")


def export_uint8(img):
    """``_show``'s 8-bit export (pre_train_test.py:61-77): (255 * np.clip(img, 0, 1)).astype(np.uint8), i.e.
    trunc(255 * clip(x)) -- not ``to_uint8``'s 255.5 rule."""
    return torch.trunc(255.0 * img.float().clamp(0.0, 1.0)).to(torch.uint8)


def tf_warp_torch(img, flow, data_format=CHANNELS_LAST):
    """``tf_warp`` (qpwcnet/core/warp.py:100-151) composed from torch operators in fp32, on any device: corner indices
    by truncation, then clipped; the raw weights from the clipped corners; the sum in the order a, b, c, d."""
    cf = get_axis(data_format) == 1
    im, f = img.float(), flow.float()
    if cf:
        im, f = im.permute(0, 2, 3, 1), f.permute(0, 2, 3, 1)
    B, H, W, _ = im.shape
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=im.device),
                            torch.arange(W, dtype=torch.float32, device=im.device), indexing="ij")
    x, y = gx + f[..., 0], gy + f[..., 1]
    x0, y0 = x.to(torch.int32), y.to(torch.int32)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = x0.clamp(0, W - 1).long(), x1.clamp(0, W - 1).long()
    y0, y1 = y0.clamp(0, H - 1).long(), y1.clamp(0, H - 1).long()
    b = torch.arange(B, device=im.device).view(-1, 1, 1)
    Ia, Ib, Ic, Id = im[b, y0, x0], im[b, y1, x0], im[b, y0, x1], im[b, y1, x1]
    x0f, x1f, y0f, y1f = x0.float(), x1.float(), y0.float(), y1.float()
    wa, wb = ((x1f - x) * (y1f - y)).unsqueeze(-1), ((x1f - x) * (y - y0f)).unsqueeze(-1)
    wc, wd = ((x - x0f) * (y1f - y)).unsqueeze(-1), ((x - x0f) * (y - y0f)).unsqueeze(-1)
    out = ((wa * Ia + wb * Ib) + wc * Ic) + wd * Id
    return out.permute(0, 3, 1, 2) if cf else out


def _finish_panels(names, pics, grid, dtype, out_format):
    """Channels-last fp32 pictures -> the dict the panel functions return: the grid, then the conversion, then the
    layout."""
    get_axis(out_format)
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError("dtype must be torch.float32 or torch.uint8, got {}".format(dtype))
    out = {}
    for name, img in zip(names, pics):
        img = img.clone()
        if grid:
            img[:, ::grid, :, :] = 1.0
            img[:, :, ::grid, :] = 1.0
        if dtype == torch.uint8:
            img = export_uint8(img)
        out[name] = (img if out_format == CHANNELS_LAST else img.permute(0, 3, 1, 2)).contiguous()
    return out


def _nhwc(t, data_format):
    return t.float() if data_format == CHANNELS_LAST else t.float().permute(0, 2, 3, 1)


def inference_panels_torch(ims, flo, flo_pred, data_format=CHANNELS_LAST, dtype=torch.float32, grid=0,
                           out_format=CHANNELS_LAST):
    """``inference_panels`` composed from torch operators, on any device: the path CPU tensors take and the baseline
    the kernels are timed against."""
    get_axis(data_format)
    x, f_gt, f_pred = _nhwc(ims, data_format), _nhwc(flo, data_format), _nhwc(flo_pred, data_format)
    prv, nxt = 0.5 + x[..., 0:3], 0.5 + x[..., 3:6]
    nxt_w = 0.5 + tf_warp_torch(x[..., 3:6], f_pred)
    nxt_w_gt = 0.5 + tf_warp_torch(x[..., 3:6], f_gt)
    pics = [prv, nxt, nxt_w, 0.5 * prv + 0.5 * nxt, 0.5 * prv + 0.5 * nxt_w, 0.5 * prv + 0.5 * nxt_w_gt,
            (0.5 * prv - 0.5 * nxt_w).abs(), (0.5 * prv - 0.5 * nxt_w_gt).abs(),
            flow_to_image_torch(f_gt), flow_to_image_torch(f_pred)]
    return _finish_panels(INFERENCE_PANELS, pics, grid, dtype, out_format)


def _flow_scale(H, W, h, w):
    s = H // h if h > 0 else 0
    if s < 1 or H != s * h or W != s * w:
        raise ValueError("the images' {}x{} must be one whole multiple of the flow's {}x{}".format(H, W, h, w))
    return s


def interpolation_panels_torch(img_pair, img1, pred, flow, grid=32, data_format=CHANNELS_LAST, dtype=torch.float32,
                               out_format=CHANNELS_LAST):
    """``interpolation_panels`` composed from torch operators, on any device."""
    get_axis(data_format)
    pair, mid, out, f = (_nhwc(t, data_format) for t in (img_pair, img1, pred, flow))
    s = _flow_scale(pair.shape[1], pair.shape[2], f.shape[1], f.shape[2])
    prv, nxt = 0.5 + pair[..., 0:3], 0.5 + pair[..., 3:6]
    upflow = float(s) * f.repeat_interleave(s, dim=1).repeat_interleave(s, dim=2)
    pics = [prv, nxt, mid, 0.5 + out, 0.5 * prv + 0.5 * nxt, flow_to_image_torch(f), tf_warp_torch(mid, upflow)]
    return _finish_panels(INTERPOLATION_PANELS, pics, grid, dtype, out_format)


def _check_panel_input(t, C, data_format, name, dtypes=(torch.float32, torch.float16)):
    if not isinstance(t, torch.Tensor):
        raise TypeError("{} must be a torch.Tensor".format(name))
    if t.dtype not in dtypes:
        raise ValueError("{}: unsupported dtype {}".format(name, t.dtype))
    if t.dim() != 4 or t.shape[get_axis(data_format)] != C:
        raise ValueError("{} must be (B,H,W,{c}) channels_last or (B,{c},H,W) channels_first, got shape {}".format(
            name, tuple(t.shape), c=C))
    return tuple(t.shape[1:3] if data_format == CHANNELS_LAST else t.shape[2:4])


def _check_panel_args(dtype, grid, out_format):
    get_axis(out_format)
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError("dtype must be torch.float32 or torch.uint8, got {}".format(dtype))
    if int(grid) != grid or grid < 0:
        raise ValueError("grid must be 0 (off) or a positive period, got {}".format(grid))
    return int(grid)


def inference_panels(ims, flo, flo_pred, data_format=None, dtype=torch.float32, grid=0, out_format=CHANNELS_LAST):
    """The pictures of app/optical_flow/test_infer.py:104-154 for a batch: ``ims`` (B,H,W,6) / (B,6,H,W), fp32 or fp16,
    preprocessed (- 0.5; channels 0-2 prv, 3-5 nxt), the ground-truth ``flo`` and the predicted ``flo_pred`` (B,H,W,2) /
    (B,2,H,W) (fp16 flows are widened), in ``data_format`` (default ``backend.image_data_format()``) -> an ordered dict
    of ten (B,H,W,3) pictures under the script's names (INFERENCE_PANELS): prv, nxt, nxt_w = 0.5 + tf_warp(nxt,
    flo_pred) on the offset image, overlay, overlay_warped, overlay_warped_gt, delta_warped, delta_warped_gt, flo_rgb,
    flo_pred_rgb.  dtype float32: the values, unclipped; uint8: ``export_uint8``.  grid: 0, or the period of ``_show``'s
    alignment grid (rows and columns 0, g, 2g, ... set to 1 before the conversion).  out_format: the pictures' layout.
    HIP tensors: two launches (include/qpwc_review.h); CPU tensors: ``inference_panels_torch``."""
    if data_format is None:
        data_format = image_data_format()
    get_axis(data_format)
    grid = _check_panel_args(dtype, grid, out_format)
    size = _check_panel_input(ims, 6, data_format, "ims")
    for name, f in (("flo", flo), ("flo_pred", flo_pred)):
        if _check_panel_input(f, 2, data_format, name) != size or f.shape[0] != ims.shape[0]:
            raise ValueError("{} {} must have ims' batch and size {}".format(name, tuple(f.shape), tuple(ims.shape)))
    if not ims.is_cuda:
        return inference_panels_torch(ims, flo, flo_pred, data_format, dtype, grid, out_format)
    outs = ops.inference_panels(ims, flo.float(), flo_pred.float(), data_format, dtype, out_format, grid)
    return dict(zip(INFERENCE_PANELS, outs))


def interpolation_panels(img_pair, img1, pred, flow, grid=32, data_format=None, dtype=torch.float32,
                         out_format=CHANNELS_LAST):
    """The pictures of app/frame_interpolation/pre_train_test.py:45-79, 121-163 for a batch: ``img_pair`` (B,H,W,6) /
    (B,6,H,W) preprocessed (- 0.5), the ground-truth middle frame ``img1`` in [0, 1] and the model's output ``pred``
    (- 0.5), both (B,H,W,3) / (B,3,H,W), all of one dtype (fp32 or fp16), and the model's ``flow`` (B,h,w,2) / (B,2,h,w)
    with H = s * h, W = s * w for one integer s >= 1 (the script: s = 2) -> an ordered dict of seven pictures
    (INTERPOLATION_PANELS): 0-prv, 1-nxt, 2-ground-truth, 3-pred = 0.5 + pred, 4-overlay, 5-flow (at the flow's own
    size, (B,h,w,3)) and 6-warp = tf_warp(img1, s * repeat(flow, s)) without an offset -- the script's key for the last
    is '6-warp(==0-prv)'.  grid: the period of ``_show``'s alignment grid, counted in each picture's own pixels (the
    script: 32; 0: off).  dtype, out_format: as ``inference_panels``.  HIP tensors: two launches; CPU tensors:
    ``interpolation_panels_torch``."""
    if data_format is None:
        data_format = image_data_format()
    get_axis(data_format)
    grid = _check_panel_args(dtype, grid, out_format)
    size = _check_panel_input(img_pair, 6, data_format, "img_pair")
    for name, t in (("img1", img1), ("pred", pred)):
        if _check_panel_input(t, 3, data_format, name) != size or t.shape[0] != img_pair.shape[0]:
            raise ValueError("{} {} must have img_pair's batch and size".format(name, tuple(t.shape)))
        if t.dtype != img_pair.dtype:
            raise ValueError("{} must have img_pair's dtype {}, got {}".format(name, img_pair.dtype, t.dtype))
    fsize = _check_panel_input(flow, 2, data_format, "flow")
    if flow.shape[0] != img_pair.shape[0]:
        raise ValueError("flow must have img_pair's batch size")
    _flow_scale(size[0], size[1], fsize[0], fsize[1])
    if not img_pair.is_cuda:
        return interpolation_panels_torch(img_pair, img1, pred, flow, grid, data_format, dtype, out_format)
    outs = ops.interpolation_panels(img_pair, img1, pred, flow.float(), data_format, dtype, out_format, grid)
    return dict(zip(INTERPOLATION_PANELS, outs))

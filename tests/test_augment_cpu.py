"""The training input pipeline (qpwcnet_amd/augment.py, qpwc_augment_fwd) without a GPU:
  * ``ref_augment``: a float64 numpy restatement of qpwcnet/data/augment.py:83-173 and app/optical_flow/train.py:54-94,
    one sample at a time with the four bilinear neighbours spelled out -- the contract the kernels are held to
    (tests/test_gpu_augment.py imports it), itself checked against a second restatement and against known answers;
  * the torch-composed CPU path of every entry point against it;
  * ``sample_params``; the C ABI's refusals; the launch-form selection at the shapes the GPU suite uses.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from qpwcnet_amd import augment

BOUND = 1e-4          # images: the project's kernel bound; flow: px, with |flow| <= 32 px in the inputs
INV255 = np.float32(1.0 / 255.0)


# ---- the restatement ------------------------------------------------------------------------------------------------
def _axis(i, n_in, n_out):
    """tf.image.resize(BILINEAR), half-pixel centres, no antialias, one axis: (lo, hi, t) of output indices i."""
    src = (np.asarray(i, np.float64) + 0.5) * (n_in / float(n_out)) - 0.5
    fl = np.floor(src)
    lo = np.maximum(fl, 0).astype(np.int64)
    hi = np.minimum(np.ceil(src), n_in - 1).astype(np.int64)
    return lo, hi, src - fl


def ref_rgb_to_hsv(x):
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    mx, mn = np.max(x, -1), np.min(x, -1)
    rng = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(mx > 0, rng / mx, 0.0)
        norm = 1.0 / (6.0 * rng)
        hh = np.where(r == mx, norm * (g - b), np.where(g == mx, norm * (b - r) + 2.0 / 6.0, norm * (r - g) + 4.0 / 6.0))
    hh = np.where(rng > 0, hh, 0.0)
    hh = np.where(hh < 0, hh + 1.0, hh)
    hh = np.where(np.isnan(x).any(-1), np.nan, hh)
    return hh, s, mx


def ref_hsv_to_rgb(hh, s, v):
    d = np.stack([np.clip(np.abs(6 * hh - 3) - 1, 0, 1), np.clip(2 - np.abs(6 * hh - 2), 0, 1),
                  np.clip(2 - np.abs(6 * hh - 4), 0, 1)], -1)
    return ((d - 1) * s[..., None] + 1) * v[..., None]


def ref_colours(x, brightness, saturation, hue, contrast, per_frame_means=False, mean_over_first=None):
    """image_augment_colors on one sample (h,w,6): brightness, saturation, hue, contrast on both frames.
    mean_over_first = N (WRONG on purpose): the contrast mean over the first N pixels, row-major, of both frames."""
    h, w, _ = x.shape
    x = x.reshape(h, w, 2, 3) + brightness
    hh, s, v = ref_rgb_to_hsv(x)
    x = ref_hsv_to_rgb(hh, np.clip(s * saturation, 0, 1), v)
    hh, s, v = ref_rgb_to_hsv(x)
    x = ref_hsv_to_rgb(np.mod(hh + hue, 1.0), s, v)
    # 'h w (k c) -> h (w k) c': adjust_contrast's mean runs over the pixels of both frames
    mean = x.mean(axis=(0, 1), keepdims=True) if per_frame_means else x.mean(axis=(0, 1, 2), keepdims=True)
    if mean_over_first is not None:
        mean = x.reshape(h * w, 2, 3)[:mean_over_first].mean(axis=(0, 1)).reshape(1, 1, 1, 3)
    x = (x - mean) * contrast + mean
    return x.reshape(h, w, 6)


def ref_augment(ims, flo, iparams, fparams, out_shape, colour=True, finish=True, data_format="channels_last",
                per_frame_means=False, flow_by_shape_ratio=False, mean_over_first=None):
    """float64 outputs for numpy inputs ims (B,H,W,6) uint8 / float, flo (B,H,W,2), iparams (B,6), fparams (B,6).
    per_frame_means / flow_by_shape_ratio build the two WRONG outputs the GPU suite's negative controls need;
    mean_over_first = N a third: the contrast mean of a fold that stops after the first N output pixels."""
    ims, flo = np.asarray(ims), np.asarray(flo)
    iparams, fparams = np.asarray(iparams), np.asarray(fparams, np.float32)
    B, H, W, _ = ims.shape
    h, w = out_shape
    if ims.dtype == np.uint8:
        x = (ims.astype(np.float32) * INV255).astype(np.float64)       # the multiply is an fp32 one
    else:
        x = ims.astype(np.float64)
    x = np.concatenate([x, flo.astype(np.float64)], -1)
    o_ims, o_flo = np.zeros((B, h, w, 6)), np.zeros((B, h, w, 2))
    for b in range(B):
        rh, rw, oy, ox, ud, lr = (int(v) for v in iparams[b])
        mu, mv, bri, sat, hue, con = (float(v) for v in fparams[b])
        assert 0 <= oy <= rh - h and 0 <= ox <= rw - w
        s = x[b]
        if ud:
            s = s[::-1]
        if lr:
            s = s[:, ::-1]
        ylo, yhi, ty = _axis(oy + np.arange(h), H, rh)
        xlo, xhi, tx = _axis(ox + np.arange(w), W, rw)
        nb = {}
        for ky, yy in (("t", ylo), ("b", yhi)):
            for kx, xx in (("l", xlo), ("r", xhi)):
                nb[ky + kx] = s[yy[:, None], xx[None, :]]
        tx_, ty_ = tx[None, :, None], ty[:, None, None]
        top = nb["tl"] + (nb["tr"] - nb["tl"]) * tx_
        bot = nb["bl"] + (nb["br"] - nb["bl"]) * tx_
        val = top + (bot - top) * ty_
        if flow_by_shape_ratio:
            mu, mv = np.sign(mu) * rw / W, np.sign(mv) * rh / H
        o_flo[b] = val[..., 6:] * np.array([mu, mv])
        o_ims[b] = val[..., :6]
        if colour:
            o_ims[b] = ref_colours(val[..., :6], bri, sat, hue, con, per_frame_means, mean_over_first)
    if finish:
        o_ims = o_ims - 0.5
        o_ims = np.where(np.isnan(o_ims), 0.0, o_ims)
        o_flo = np.where(np.isnan(o_flo), 0.0, o_flo)
    if data_format == "channels_first":
        return o_ims.transpose(0, 3, 1, 2), o_flo.transpose(0, 3, 1, 2)
    return o_ims, o_flo


# ---- fixtures shared with the GPU suite -----------------------------------------------------------------------------------
def smooth_flow(B, H, W, amp=30.0, seed=0):
    """|flow| <= 32 px, at most ~2 px of change per pixel: the fp32 source coordinate is good to ~4e-6 at these sizes,
    so the resampled flow is good to ~1e-5 px."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((B, H, W, 2), np.float32)
    for b in range(B):
        out[b, ..., 0] = amp * np.sin(0.05 * x + 0.03 * y + b + seed)
        out[b, ..., 1] = amp * np.cos(0.04 * x - 0.06 * y + 0.5 * b + seed)
    return out


def make_case(dtype, seed=0):
    """The GPU suite's batch: B = 4, one sample per flip combination, source 30 x 52 (6 * 52 bytes per row is no
    multiple of 16), output 16 x 24.  Every sample has its own scale in [0.9, 1.1] (the flow multiplier), window and
    colour parameters; the last one resizes straight to the output size (rh = h, rw = w, offsets 0)."""
    rng = np.random.default_rng(seed)
    B, H, W, h, w = 4, 30, 52, 16, 24
    if dtype == np.uint8:
        ims = rng.integers(0, 256, (B, H, W, 6), dtype=np.uint8)
    else:
        ims = rng.random((B, H, W, 6), dtype=np.float32)
    flo = smooth_flow(B, H, W, seed=seed)
    scales = np.array([0.9, 0.97, 1.1, 1.03], np.float32)
    ip = np.zeros((B, 6), np.int32)
    fp = np.zeros((B, 6), np.float32)
    for b, (ud, lr) in enumerate(itertools.product((0, 1), (0, 1))):
        rh, rw = (int(np.float32(H) * scales[b]), int(np.float32(W) * scales[b])) if b < 3 else (h, w)
        ip[b] = (rh, rw, (3 * b + 1) % (rh - h + 1), (5 * b + 2) % (rw - w + 1), ud, lr)
        fp[b, :2] = (scales[b] * (1 - 2 * lr), scales[b] * (1 - 2 * ud))
    fp[:, 2] = (-0.1, 0.05, 0.12, -0.03)      # brightness
    fp[:, 3] = (0.6, 1.4, 1.0, 0.8)           # saturation
    fp[:, 4] = (-0.15, 0.1, 0.19, -0.05)      # hue
    fp[:, 5] = (1.3, 0.7, 0.55, 1.45)         # contrast
    assert tuple(ip[3, :4]) == (h, w, 0, 0)
    return ims, flo, ip, fp, (h, w)


def tiny_case(seed=1):
    """B = 1, output 7 x 5: rows shorter than any tile, 35 pixels (no multiple of 4)."""
    rng = np.random.default_rng(seed)
    ims = rng.integers(0, 256, (1, 11, 9, 6), dtype=np.uint8)
    ip = np.array([[9, 8, 1, 2, 1, 0]], np.int32)
    fp = np.array([[0.95, -0.95, 0.07, 1.2, -0.11, 0.8]], np.float32)
    return ims, smooth_flow(1, 11, 9, seed=seed), ip, fp, (7, 5)


def as_params(ip, fp, device="cpu"):
    return augment.AugmentParams(torch.from_numpy(np.ascontiguousarray(ip)).to(device),
                                 torch.from_numpy(np.ascontiguousarray(fp)).to(device))


def max_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


# ---- the restatement against a second one -------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(13, 21), (40, 70), (30, 52)])
def test_resampling_matches_half_pixel_interpolate(size):
    rng = np.random.default_rng(2)
    H, W = 30, 52
    ims = rng.random((1, H, W, 6))
    flo = rng.standard_normal((1, H, W, 2))
    ip = np.array([[size[0], size[1], 0, 0, 0, 0]])
    fp = np.array([[1.0, 1.0, 0, 1, 0, 1]], np.float32)
    o_ims, o_flo = ref_augment(ims, flo, ip, fp, size, colour=False, finish=False)
    x = torch.from_numpy(np.concatenate([ims, flo], -1)).permute(0, 3, 1, 2)
    want = F.interpolate(x, size=size, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    assert max_err(o_ims, want[..., :6]) < 1e-12 and max_err(o_flo, want[..., 6:]) < 1e-12


def test_colour_chain_matches_the_torch_restatement():
    rng = np.random.default_rng(3)
    x = rng.random((2, 9, 11, 6))
    x[0, :2, :2] = 0.4                                # grey pixels: range == 0
    x[1, 3, 3, :3] = (0.9, 0.9, 0.1)                  # a tie for the maximum
    fp = np.array([[1, 1, -0.1, 0.6, -0.15, 1.3], [1, 1, 0.12, 1.4, 0.19, 0.55]], np.float32)
    want = augment._colours_torch(torch.from_numpy(x), torch.from_numpy(fp)).numpy()
    for b in range(2):
        got = ref_colours(x[b], *(float(v) for v in fp[b, 2:]))
        assert max_err(got, want[b]) < 1e-12


# ---- known answers ------------------------------------------------------------------------------------------------------
def _identity_params(B, H, W, flips=((0, 0),)):
    ip = np.array([[H, W, 0, 0, ud, lr] for ud, lr in flips], np.int32)
    fp = np.array([[1 - 2 * lr, 1 - 2 * ud, 0, 1, 0, 1] for ud, lr in flips], np.float32)
    return ip, fp


def identity_case():
    """All four flip combinations of one uint8 sample at identity geometry, and the exact answers."""
    rng = np.random.default_rng(4)
    H, W = 10, 14
    flips = list(itertools.product((0, 1), (0, 1)))
    ims = np.repeat(rng.integers(0, 256, (1, H, W, 6), dtype=np.uint8), 4, 0)
    flo = np.repeat(rng.standard_normal((1, H, W, 2)).astype(np.float32), 4, 0)
    ip, fp = _identity_params(4, H, W, flips)
    want_ims = ims.astype(np.float32) * INV255 - np.float32(0.5)
    want_flo = flo.copy()
    for b, (ud, lr) in enumerate(flips):
        if ud:
            want_ims[b], want_flo[b] = want_ims[b, ::-1], want_flo[b, ::-1] * np.float32([1, -1])
        if lr:
            want_ims[b], want_flo[b] = want_ims[b, :, ::-1], want_flo[b, :, ::-1] * np.float32([-1, 1])
    return ims, flo, ip, fp, (H, W), want_ims, want_flo


def test_identity_and_flips_are_exact():
    ims, flo, ip, fp, hw, want_ims, want_flo = identity_case()
    o_ims, o_flo = ref_augment(ims, flo, ip, fp, hw, colour=False)
    # the restatement is float64: the fp32 answer is (u8 * float32(1/255)) - 0.5 rounded once more
    assert np.array_equal(o_ims.astype(np.float32), want_ims) and np.array_equal(o_flo, want_flo.astype(np.float64))
    t_ims, t_flo = augment.augment_torch(torch.from_numpy(ims), torch.from_numpy(flo), as_params(ip, fp), hw,
                                         colour=False)
    assert np.array_equal(t_ims.numpy(), want_ims) and np.array_equal(t_flo.numpy(), want_flo)


def test_constant_image_stays_constant_and_linear_flow_stays_linear():
    H, W, h, w = 30, 52, 16, 24
    ims = np.full((1, H, W, 6), 0.3)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    flo = np.stack([0.5 * x - 0.25 * y + 1.0, -0.125 * x + 0.75 * y - 2.0], -1)[None]
    for rh, rw, oy, ox in ((27, 46, 5, 9), (33, 57, 11, 20), (16, 24, 0, 0)):
        ip = np.array([[rh, rw, oy, ox, 0, 0]])
        fp = np.array([[1, 1, 0, 1, 0, 1]], np.float32)
        o_ims, o_flo = ref_augment(ims, flo, ip, fp, (h, w), colour=False, finish=False)
        assert max_err(o_ims, 0.3) < 1e-12
        # interior: source coordinates inside [0, n - 1], where no edge clamp bends the line
        sy = (oy + np.arange(h) + 0.5) * H / rh - 0.5
        sx = (ox + np.arange(w) + 0.5) * W / rw - 0.5
        iy, ix = (sy >= 0) & (sy <= H - 1), (sx >= 0) & (sx <= W - 1)
        want = np.stack([0.5 * sx[None, :] - 0.25 * sy[:, None] + 1.0, -0.125 * sx[None, :] + 0.75 * sy[:, None] - 2.0], -1)
        assert iy.sum() >= h - 2 and ix.sum() >= w - 2
        assert max_err(o_flo[0][iy][:, ix], want[iy][:, ix]) < 1e-12


def test_hue_third_turns_red_into_green_and_grey_is_a_fixed_point():
    red = np.zeros((2, 2, 6))
    red[..., 0] = red[..., 3] = 1.0
    got = ref_colours(red, 0.0, 1.0, 1.0 / 3.0, 1.0)
    want = np.zeros((2, 2, 6))
    want[..., 1] = want[..., 4] = 1.0
    assert max_err(got, want) < 1e-12
    grey = np.full((3, 3, 6), 0.37)
    for sat, hue in ((0.5, -0.2), (1.5, 0.2), (0.0, 0.5), (1.0, 0.0)):
        assert max_err(ref_colours(grey, 0.0, sat, hue, 1.0), grey) < 1e-12


def test_contrast_zero_gives_the_mean_over_both_frames():
    rng = np.random.default_rng(5)
    x = rng.random((4, 5, 6)) * 0.5
    x[..., 3:] += 0.4                                   # frame 1 brighter: joint and per-frame means differ
    got = ref_colours(x, 0.0, 1.0, 0.0, 0.0)
    joint = (x[..., :3].mean((0, 1)) + x[..., 3:].mean((0, 1))) / 2
    assert max_err(got[..., :3], joint) < 1e-12 and max_err(got[..., 3:], joint) < 1e-12
    per_frame = ref_colours(x, 0.0, 1.0, 0.0, 0.0, per_frame_means=True)
    assert np.abs(per_frame - got).max() > 0.1


# ---- the torch-composed CPU path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
def test_cpu_preprocess_matches_restatement(dtype, data_format):
    """Also the check the GPU suite's bounds rest on: the fp32 composition meets them on the GPU suite's own inputs."""
    for case in (make_case(dtype), tiny_case()):
        ims, flo, ip, fp, hw = case
        for colour in (True, False):
            want = ref_augment(ims, flo, ip, fp, hw, colour=colour, data_format=data_format)
            got = augment.augment_torch(torch.from_numpy(ims), torch.from_numpy(flo), as_params(ip, fp), hw,
                                        colour=colour, data_format=data_format)
            assert tuple(got[0].shape) == want[0].shape and got[0].dtype == torch.float32 and got[0].is_contiguous()
            assert max_err(got[0].numpy(), want[0]) <= BOUND and max_err(got[1].numpy(), want[1]) <= BOUND
        got = augment.preprocess(torch.from_numpy(ims), torch.from_numpy(flo), data_format, out_shape=hw,
                                 params=as_params(ip, fp))
        want = ref_augment(ims, flo, ip, fp, hw, data_format=data_format)
        assert max_err(got[0].numpy(), want[0]) <= BOUND and max_err(got[1].numpy(), want[1]) <= BOUND


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
def test_cpu_preprocess_no_op_and_image_resize_match_restatement(data_format):
    ims, flo, _, _, _ = make_case(np.uint8)
    B, H, W, _ = ims.shape
    for hw in ((16, 24), (40, 61)):
        rp = augment.resize_params(B, (H, W), hw)
        assert rp.iparams.tolist() == [[hw[0], hw[1], 0, 0, 0, 0]] * B
        assert np.allclose(rp.fparams[:, :2].numpy(), [hw[1] / W, hw[0] / H], rtol=1e-7)
        want = ref_augment(ims, flo, rp.iparams.numpy(), rp.fparams.numpy(), hw, colour=False, data_format=data_format)
        got = augment.preprocess_no_op(torch.from_numpy(ims), torch.from_numpy(flo), data_format, out_shape=hw)
        assert max_err(got[0].numpy(), want[0]) <= BOUND and max_err(got[1].numpy(), want[1]) <= BOUND
    f_ims = ims.astype(np.float32) / 255
    want = ref_augment(f_ims, flo, rp.iparams.numpy(), rp.fparams.numpy(), hw, colour=False, finish=False)
    got = augment.image_resize(torch.from_numpy(f_ims), torch.from_numpy(flo), hw)
    assert max_err(got[0].numpy(), want[0]) <= BOUND and max_err(got[1].numpy(), want[1]) <= BOUND


def test_cpu_image_augment_matches_restatement_and_draws_when_asked():
    ims, flo, ip, fp, hw = make_case(np.float32)
    want = ref_augment(ims, flo, ip, fp, hw, finish=False)
    got = augment.image_augment(torch.from_numpy(ims), torch.from_numpy(flo), hw, params=as_params(ip, fp))
    assert max_err(got[0].numpy(), want[0]) <= BOUND and max_err(got[1].numpy(), want[1]) <= BOUND
    t_ims, t_flo = torch.from_numpy(ims), torch.from_numpy(flo)
    g = lambda: torch.Generator().manual_seed(11)
    a = augment.image_augment(t_ims, t_flo, hw, base_scale=1.0, generator=g())
    p = augment.sample_params(4, (30, 52), hw, 1.0, generator=g())
    b = augment.image_augment(t_ims, t_flo, hw, params=p)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want = ref_augment(ims, flo, p.iparams.numpy(), p.fparams.numpy(), hw, finish=False)
    assert max_err(a[0].numpy(), want[0]) <= BOUND and max_err(a[1].numpy(), want[1]) <= BOUND


def test_inputs_are_checked():
    ims, flo, ip, fp, hw = make_case(np.uint8)
    t_ims, t_flo, p = torch.from_numpy(ims), torch.from_numpy(flo), as_params(ip, fp)
    with pytest.raises(ValueError, match="Unsupported data format"):
        augment.preprocess(t_ims, t_flo, "channels_middle", out_shape=hw, params=p)
    with pytest.raises(ValueError, match="dtype"):
        augment.image_augment(t_ims, t_flo, hw, params=p)                   # uint8: float frames only
    with pytest.raises(ValueError, match="dtype"):
        augment.preprocess(t_ims, t_flo.double(), out_shape=hw, params=p)
    with pytest.raises(ValueError, match="channels_last"):
        augment.preprocess(t_ims.permute(0, 3, 1, 2), t_flo, out_shape=hw, params=p)
    with pytest.raises(ValueError, match="dense"):
        augment.preprocess(t_ims[:, ::2], t_flo[:, ::2], out_shape=hw, params=p)
    with pytest.raises(ValueError, match="does not match"):
        augment.preprocess(t_ims, t_flo[:, :-1].contiguous(), out_shape=hw, params=p)
    with pytest.raises(ValueError, match="iparams"):
        augment.preprocess(t_ims, t_flo, out_shape=hw, params=as_params(ip[:2], fp))


# ---- sample_params ------------------------------------------------------------------------------------------------------
def test_scaled_shape_truncates_the_fp32_product():
    s = np.float32(0.7)                                  # 0.699999988...: 10 * s is 7.0 in fp32, 6.99999988 in fp64
    assert int(np.float64(10) * np.float64(s)) == 6
    assert augment.scaled_shape(10, 20, torch.tensor([s])).tolist() == [[7, 14]]
    assert augment.scaled_shape(540, 960, torch.tensor([0.56, 0.5348], dtype=torch.float32)).tolist() == [
        [int(np.float32(540) * np.float32(0.56)), int(np.float32(960) * np.float32(0.56))],
        [int(np.float32(540) * np.float32(0.5348)), int(np.float32(960) * np.float32(0.5348))]]


def test_sample_params_ranges_reproducibility_and_refusal():
    H, W, h, w, B, base = 540, 960, 256, 512, 512, 0.56
    g = lambda seed: torch.Generator().manual_seed(seed)
    p = augment.sample_params(B, (H, W), (h, w), base, generator=g(7))
    ip, fp = p.iparams.numpy(), p.fparams.numpy()
    assert ip.dtype == np.int32 and fp.dtype == np.float32 and ip.shape == fp.shape == (B, 6)
    scale = np.abs(fp[:, 0])
    assert np.array_equal(scale, np.abs(fp[:, 1]))
    assert scale.min() >= np.float32(0.955 * base) and scale.max() <= np.float32(1.05 * base)
    assert scale.max() - scale.min() > 0.04 * base
    # (rh, rw): the fp32 product, truncated
    assert np.array_equal(ip[:, 0], (np.float32(H) * scale).astype(np.int32))
    assert np.array_equal(ip[:, 1], (np.float32(W) * scale).astype(np.int32))
    assert (ip[:, 2] >= 0).all() and (ip[:, 2] <= ip[:, 0] - h).all()
    assert (ip[:, 3] >= 0).all() and (ip[:, 3] <= ip[:, 1] - w).all()
    assert ip[:, 2].max() > 0 and ip[:, 3].max() > 0 and (ip[:, 2] == ip[:, 0] - h).any()   # the last window is drawn too
    assert set(np.unique(ip[:, 4:])) == {0, 1}
    assert 0.35 < ip[:, 4].mean() < 0.65 and 0.35 < ip[:, 5].mean() < 0.65
    # the flip signs are folded into the flow multipliers: u with left-right, v with up-down
    assert np.array_equal(np.sign(fp[:, 0]), 1 - 2 * ip[:, 5]) and np.array_equal(np.sign(fp[:, 1]), 1 - 2 * ip[:, 4])
    for col, (lo, hi) in ((2, (-0.125, 0.125)), (3, (0.5, 1.5)), (4, (-0.2, 0.2)), (5, (0.5, 1.5))):
        assert fp[:, col].min() >= lo and fp[:, col].max() <= hi
        assert fp[:, col].max() - fp[:, col].min() > 0.9 * (hi - lo)
        assert len(np.unique(fp[:, col])) > B // 2                                    # per sample, not per batch
    q = augment.sample_params(B, (H, W), (h, w), base, generator=g(7))
    assert torch.equal(p.iparams, q.iparams) and torch.equal(p.fparams, q.fparams)
    r = augment.sample_params(B, (H, W), (h, w), base, generator=g(8))
    assert not torch.equal(p.fparams, r.fparams)
    # 960 * 0.4775 = 458 < 512: TF's random_crop would assert
    with pytest.raises(ValueError, match="does not fit"):
        augment.sample_params(4, (H, W), (h, w), 0.5)
    with pytest.raises(ValueError, match="does not fit"):
        augment.sample_params(4, (30, 52), (30, 52), 1.0)
    augment.sample_params(4, (30, 52), (28, 49), 1.0)                                 # 30 * 0.955 = 28.65, 52 * 0.955 = 49.66


# ---- the C ABI refuses bad arguments before any HIP call ----------------------------------------------------------------
def test_augment_fwd_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep = (ctypes.c_float * (1 << 16))()
    base = ctypes.cast(keep, ctypes.c_void_p).value
    base += (-base) % 256
    # 1 x 8 x 8 source -> 4 x 4: every buffer 16 KiB apart
    ims, flo, ipar, fpar, o_ims, o_flo, ws = (base + (16 << 10) * i for i in range(7))

    def call(ims=ims, dtype=_hip.U8, flo=flo, B=1, H=8, W=8, ip=ipar, fp=fpar, h=4, w=4, flags=1, layout=0, o_ims=o_ims,
             o_flo=o_flo, ws=ws):
        return L.qpwc_augment_fwd(ims, dtype, flo, B, H, W, ip, fp, h, w, flags, layout, o_ims, o_flo, ws, None)

    for name in ("ims", "flo", "ip", "fp", "o_ims", "o_flo", "ws"):
        assert call(**{name: None}) == _hip.E_NULL, name
    for name in ("B", "H", "W", "h", "w"):
        assert call(**{name: 0}) == _hip.E_SHAPE and call(**{name: -3}) == _hip.E_SHAPE, name
    assert b"non-positive" in L.qpwc_last_error()
    assert call(dtype=_hip.F16) == _hip.E_DTYPE and call(dtype=3) == _hip.E_DTYPE and call(dtype=-1) == _hip.E_DTYPE
    assert call(layout=2) == _hip.E_LAYOUT and call(layout=-1) == _hip.E_LAYOUT
    assert b"Unsupported data format" in L.qpwc_last_error()
    assert call(flags=4) == _hip.E_MODE and call(flags=-1) == _hip.E_MODE and call(flags=8 | 1) == _hip.E_MODE
    # counts that overflow the 32-bit pixel indices and grids (the source offsets themselves are 64-bit)
    assert call(H=1 << 16, W=1 << 15) == _hip.E_SHAPE                       # H * W = 2^31
    assert b"overflows" in L.qpwc_last_error()
    assert call(h=1 << 15, w=1 << 14) == _hip.E_SHAPE                       # 6 * h * w > 2^31 - 1
    assert call(B=1 << 20, h=1 << 10, w=1 << 10) == _hip.E_SHAPE            # 2^32 workgroups
    assert call(ims=ims + 1) == _hip.E_ALIGN                                # uint8 pixels are read as 2-byte pieces
    assert call(dtype=_hip.F32, ims=ims + 4) == _hip.E_ALIGN                # fp32 pixels as 8-byte pieces
    assert call(flo=flo + 4) == _hip.E_ALIGN
    for name, p in (("ip", ipar), ("fp", fpar), ("o_ims", o_ims), ("o_flo", o_flo), ("ws", ws)):
        assert call(**{name: p + 2}) == _hip.E_ALIGN, name
    assert call(o_ims=ims) == _hip.E_ALIAS and call(o_flo=flo + 64) == _hip.E_ALIAS
    assert call(o_ims=fpar) == _hip.E_ALIAS and call(o_flo=o_ims + 128) == _hip.E_ALIAS
    assert call(ws=o_flo) == _hip.E_ALIAS and call(ws=ipar) == _hip.E_ALIAS
    with pytest.raises(ValueError, match="flags"):
        _hip.check(call(flags=4))


def test_augment_workspace_and_launch_form_need_no_gpu(hip_lib):
    from qpwcnet_amd import _hip, ops
    L = hip_lib
    ws = L.qpwc_augment_workspace_floats
    assert ws(16, 256, 512) == 3 * 16 * 512                                 # three sums per 256-pixel workgroup
    assert ws(1, 7, 5) == 3
    prev = 0
    for B, h, w in ((1, 1, 1), (1, 16, 16), (1, 16, 17), (1, 17, 17), (2, 17, 17), (2, 64, 128), (16, 256, 512)):
        assert ws(B, h, w) >= prev > -1
        prev = ws(B, h, w)
    assert ws(0, 4, 4) == _hip.E_SHAPE and ws(1, -1, 4) == _hip.E_SHAPE and ws(1, 4, 0) == _hip.E_SHAPE
    assert ws(1 << 20, 1 << 10, 1 << 10) == _hip.E_SHAPE
    # the launch forms at the shapes tests/test_gpu_augment.py relies on: a moved rule fails here
    aligned = 1 << 20
    pick = lambda B, h, w, a=aligned, b=aligned: L.qpwc_augment_fwd_kernel(B, h, w, a, b).decode()
    assert pick(4, 16, 24) == "augment_pixel_kernel<vec4>"                  # the main batch
    assert pick(1, 7, 5) == "augment_pixel_kernel<scalar>"                  # 35 pixels: no multiple of 4
    assert pick(1, 16, 16) == "augment_pixel_kernel<vec4>"                  # the NaN scrub case
    assert pick(2, 64, 128) == "augment_pixel_kernel<vec4>"                 # end to end
    assert pick(16, 256, 512) == "augment_pixel_kernel<vec4>"               # the trainer's shape
    assert pick(4, 16, 24, aligned + 4) == "augment_pixel_kernel<scalar>"   # an output off the 16-byte grid
    assert pick(4, 16, 24, aligned, aligned + 8) == "augment_pixel_kernel<scalar>"
    assert pick(1, 2, 3) == "augment_pixel_kernel<scalar>" and pick(1, 2, 2) == "augment_pixel_kernel<vec4>"
    assert pick(0, 16, 24) == "" and pick(1, 16, 0) == "" and pick(1, 16, 24, None) == ""
    assert ops.augment_kernel(4, 16, 24) == "augment_pixel_kernel<vec4>" and ops.augment_kernel(1, 7, 5).endswith("<scalar>")
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.augment(torch.zeros(1, 8, 8, 6, dtype=torch.uint8), torch.zeros(1, 8, 8, 2), torch.zeros(1, 6, dtype=torch.int32),
                    torch.zeros(1, 6), (4, 4))

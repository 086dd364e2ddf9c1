"""flow_to_image and the trainer's flow panels (qpwcnet_amd/vis.py, qpwc_flow_to_image_fwd) without a GPU:
  * ``ref_flow_to_image``: a float64 numpy restatement of qpwcnet/core/vis.py:37-76 with tf.image.hsv_to_rgb's functor
    written out, ``ref_nearest`` (tf.image.resize(NEAREST_NEIGHBOR), TF2's half-pixel rule, in exact rational
    arithmetic) and ``ref_uint8`` (convert_image_dtype(saturate=True)) -- the contract the kernels are held to
    (tests/test_gpu_vis.py imports them);
  * ``vis.flow_to_image_torch``, the path CPU tensors take, against the restatement and against known answers.
Bound: 1e-4, the project's kernel bound (BOUND of test_augment_cpu.py).  Every quantity is in [0, 1] or an angle below
pi, so the fp32 chain's own error is a few 1e-7 (numpy fp32 against float64: 4.8e-7)."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import BOUND  # noqa: E402

from qpwcnet_amd import vis  # noqa: E402


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_flow_to_image(flow, data_format="channels_last"):
    """(B,h,w,2) / (B,2,h,w) numbers -> float64 (B,h,w,3) / (B,3,h,w) in the same data format."""
    f = np.asarray(flow, np.float64)
    fx, fy = (f[..., 0], f[..., 1]) if data_format == "channels_last" else (f[:, 0], f[:, 1])
    hue = (np.arctan2(fy, fx) + math.pi) / (2.0 * math.pi)
    mag = np.sqrt(fx * fx + fy * fy)
    smax = mag.max(axis=(-2, -1), keepdims=True)
    s = mag / (smax + 1e-6)
    dh = 6.0 * hue
    dr = np.clip(np.abs(dh - 3.0) - 1.0, 0.0, 1.0)
    dg = np.clip(2.0 - np.abs(dh - 2.0), 0.0, 1.0)
    db = np.clip(2.0 - np.abs(dh - 4.0), 0.0, 1.0)
    return np.stack([(1.0 - s) + s * d for d in (dr, dg, db)], axis=-1 if data_format == "channels_last" else 1)


def ref_nearest_index(n_out, n_in):
    """min(floor((i + 1/2) * n_in / n_out), n_in - 1), exactly.  (2 i + 1) * n_in / (2 n_out) is never within
    1 / (2 n_out) of an integer unless it is one, so the fp32 product of the kernel cannot land on the other side; where
    it is one, the scale must be a whole number, which fp32 holds and multiplies exactly."""
    idx = [min(math.floor(Fraction(2 * i + 1, 2) * Fraction(n_in, n_out)), n_in - 1) for i in range(n_out)]
    for i in range(n_out):
        tie = (Fraction(2 * i + 1, 2) * Fraction(n_in, n_out)).denominator == 1
        assert not tie or n_in % n_out == 0, "a tie under an inexact scale: choose another size"
    return np.asarray(idx)


def ref_nearest(img, size, data_format="channels_last"):
    ya, xa = (1, 2) if data_format == "channels_last" else (2, 3)
    img = np.take(img, ref_nearest_index(size[0], img.shape[ya]), axis=ya)
    return np.take(img, ref_nearest_index(size[1], img.shape[xa]), axis=xa)


def ref_uint8(img):
    return np.clip(np.trunc(np.asarray(img, np.float64) * 255.5), 0, 255).astype(np.uint8)


def to_layout(x, src, dst):
    """numpy image or flow between the two data formats."""
    if src == dst:
        return x
    return np.transpose(x, (0, 3, 1, 2) if dst == "channels_first" else (0, 2, 3, 1))


def random_flow(seed, shape, scale=3.0):
    """(B,h,w,2) float32 N(0, scale^2), channels-last."""
    return (np.random.default_rng(seed).standard_normal(shape + (2,)) * scale).astype(np.float32)


FORMATS = ("channels_last", "channels_first")


# ---- the torch path against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("data_format", FORMATS)
def test_torch_path_against_the_restatement(data_format):
    flow = to_layout(random_flow(0, (3, 13, 21)), "channels_last", data_format)
    got = vis.flow_to_image(torch.from_numpy(flow), data_format).numpy()
    want = ref_flow_to_image(flow, data_format)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.abs(got - want).max())
    print("flow_to_image_torch vs float64, {}: {:.2e}".format(data_format, err))
    assert err < BOUND
    half = torch.from_numpy(flow).half()
    got = vis.flow_to_image(half, data_format)
    assert got.dtype == torch.float32
    assert float(np.abs(got.numpy() - ref_flow_to_image(half.float().numpy(), data_format)).max()) < BOUND
    one = vis.flow_to_image(torch.from_numpy(flow[1]), data_format)          # rank 3: one image
    assert torch.equal(one, vis.flow_to_image(torch.from_numpy(flow[1:2]), data_format)[0])


def test_signature_matches_the_reference():
    import inspect
    sig = inspect.signature(vis.flow_to_image)
    assert list(sig.parameters) == ["flow", "data_format"] and sig.parameters["data_format"].default == "channels_last"
    with pytest.raises(ValueError, match="Unsupported data format"):
        vis.flow_to_image(torch.zeros(1, 2, 2, 2), "nhwc")
    with pytest.raises(ValueError, match="must be"):
        vis.flow_to_image(torch.zeros(1, 2, 2, 3))
    with pytest.raises(ValueError, match="dtype"):
        vis.flow_to_image(torch.zeros(1, 2, 2, 2, dtype=torch.float64))


# ---- known answers --------------------------------------------------------------------------------------------------
KNOWN = [((1.0, 0.0), (0.5, 1.0, 1.0)),
         ((-1.0, 0.0), (1.0, 0.5, 0.5)),
         ((-1.0, -0.0), (1.0, 0.5, 0.5)),      # hue 0 and hue 1 are the same red
         ((0.0, 1.0), (0.75, 0.5, 1.0)),
         ((0.0, -1.0), (0.75, 1.0, 0.5))]


@pytest.mark.parametrize("probe,rgb", KNOWN)
@pytest.mark.parametrize("data_format", FORMATS)
def test_known_answers(probe, rgb, data_format):
    """The image also holds a pixel (2, 0): s = 1 / (2 + 1e-6) = 0.5 (1 - 5e-7) at the probed pixel."""
    flow = np.zeros((1, 2, 3, 2), np.float32)
    flow[0, 0, 1] = (2.0, 0.0)
    flow[0, 1, 2] = probe
    assert bool(np.signbit(flow[0, 1, 2, 1])) == (math.copysign(1.0, probe[1]) < 0)      # -0.0 survives the store
    for f in (ref_flow_to_image, lambda x, d: vis.flow_to_image(torch.from_numpy(x), d).numpy()):
        img = to_layout(f(to_layout(flow, "channels_last", data_format), data_format), data_format, "channels_last")
        assert np.abs(img[0, 1, 2] - np.asarray(rgb)).max() <= 1e-6, img[0, 1, 2]
        assert np.abs(img[0, 0, 1] - (0.0, 1.0, 1.0)).max() <= 1e-6                 # the maximum itself: full cyan
        assert np.abs(img[0, 0, 0] - 1.0).max() == 0.0                              # a zero pixel is white


def test_all_zero_image_is_white():
    for data_format in FORMATS:
        img = vis.flow_to_image(torch.zeros(2, 2, 5, 5) if data_format == "channels_first" else torch.zeros(2, 5, 5, 2),
                                data_format)
        assert torch.isfinite(img).all() and bool((img == 1.0).all())
    assert (ref_flow_to_image(np.zeros((1, 4, 4, 2))) == 1.0).all()


def test_each_image_has_its_own_maximum():
    flow = np.zeros((2, 4, 4, 2), np.float32)
    flow[0, 0, 0] = (4.0, 0.0)
    flow[1, 0, 0] = (1.0, 0.0)
    flow[:, 2, 2] = (0.5, 0.0)                     # the same vector in both: s = 1/8 and 1/2
    img = vis.flow_to_image(torch.from_numpy(flow)).numpy()
    assert abs(img[0, 2, 2, 0] - (1 - 0.125)) < 1e-6 and abs(img[1, 2, 2, 0] - 0.5) < 1e-6
    assert np.abs(img - ref_flow_to_image(flow)).max() < BOUND


# ---- nearest, uint8 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(3, 8), (5, 7), (4, 8), (8, 4), (7, 7), (1, 5), (33, 37), (70, 128), (2, 256)])
def test_nearest_rule(n_in, n_out):
    """tf.image.resize(NEAREST_NEIGHBOR) in TF2: the pixel whose cell holds the output pixel's centre."""
    table = [min(int(math.floor((i + 0.5) * n_in / n_out)), n_in - 1) for i in range(n_out)]
    assert ref_nearest_index(n_out, n_in).tolist() == table
    assert vis.nearest_index(n_out, n_in).tolist() == table
    if n_in == n_out:
        assert table == list(range(n_in))
    if (n_in, n_out) == (3, 8):
        assert table == [0, 0, 0, 1, 1, 2, 2, 2]
    if (n_in, n_out) == (4, 8):
        assert table == [0, 0, 1, 1, 2, 2, 3, 3]
    if (n_in, n_out) == (5, 7):
        assert table == [0, 1, 1, 2, 3, 3, 4]


def test_uint8_rule():
    x = torch.tensor([0.0, 1.0, 0.5, -0.25, 1.5, 1.5 / 255.5, 0.999])
    want = [0, 255, 127, 0, 255, 1, 255]
    assert vis.to_uint8(x).tolist() == want and ref_uint8(x.numpy()).tolist() == want


# ---- the panels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data_format", FORMATS)
def test_flow_panels_equal_the_per_level_path(data_format):
    sizes = [(4, 8), (8, 16), (16, 32)]
    flows = [to_layout(random_flow(10 + i, (2,) + s), "channels_last", data_format) for i, s in enumerate(sizes)]
    ts = [torch.from_numpy(f) for f in flows]
    for size in (None, (16, 32), (32, 96), (2, 4)):            # whole ratios: a power of two ties at any other
        out = (flows[0].shape[1:3] if data_format == "channels_last" else flows[0].shape[2:4]) if size is None else size
        panels = vis.flow_panels(ts, size=size, data_format=data_format)
        assert len(panels) == 3
        for p, f, t in zip(panels, flows, ts):
            assert p.dtype == torch.uint8 and tuple(p.shape) == (2,) + tuple(out) + (3,)
            img = to_layout(vis.flow_to_image(t, data_format).numpy(), data_format, "channels_last")
            assert np.array_equal(p.numpy(), vis.to_uint8(torch.from_numpy(ref_nearest(img, out))).numpy())
            exact = ref_nearest(to_layout(ref_flow_to_image(f, data_format), data_format, "channels_last"), out)
            assert np.abs(p.numpy().astype(np.int64) - ref_uint8(exact).astype(np.int64)).max() <= 1
        floats = vis.flow_panels(ts, size=size, data_format=data_format, dtype=torch.float32)
        assert all(p.dtype == torch.float32 for p in floats)
        assert all(torch.equal(vis.to_uint8(a), b) for a, b in zip(floats, panels))


def test_flow_panels_defaults_and_refusals():
    from qpwcnet_amd import backend
    t = torch.from_numpy(random_flow(3, (1, 4, 6)))
    assert backend.image_data_format() == "channels_last"
    assert tuple(vis.flow_panels([t, t[:, :2, :3]])[1].shape) == (1, 4, 6, 3)
    with pytest.raises(ValueError):
        vis.flow_panels([])
    with pytest.raises(ValueError, match="batched"):
        vis.flow_panels([t[0]])

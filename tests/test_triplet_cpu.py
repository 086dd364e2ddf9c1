"""The frame interpolator's input pipeline (qpwcnet_amd/augment.py, qpwc_augment_triplet_fwd) without a GPU:
  * ``ref_triplet``: a float64 numpy restatement of qpwcnet/data/triplet_dataset_ops.py (read_and_resize's resize,
    augment_triplet), data/augment.py:10-59 and app/frame_interpolation/pre_train.py:110-124, in the reference's own
    order (resize, colours, noise, flips, - 0.5, concat) with its own Philox4x32-10 in uint64, its own resize and its
    own flips -- the contract the kernel is held to (tests/test_gpu_triplet.py imports it and the cases);
  * ``augment.philox4x32`` against known answers from an independent pure-Python Philox4x32-10;
  * the torch-composed CPU path against the restatement; the noise field's statistics; the sampler; the ctypes table
    against include/qpwc_triplet.h.
Bound: 1e-4, the project's kernel bound (BOUND of test_augment_cpu.py).  |values| < 3 here, so the fp32 chain's own
error is a few 1e-7; the noise adds 0.02 times a few fp32 ulps of a number < 6.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import BOUND  # noqa: E402
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

from qpwcnet_amd import _hip, augment  # noqa: E402

TRIPLET_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qpwc_triplet.h")
INV255 = np.float32(1.0 / 255.0)


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_philox(counter, key):
    """Philox4x32-10 on uint64 numpy arrays holding 32-bit words: counter (..., 4), key (..., 2) -> (..., 4)."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(counter, np.uint64)[..., i] & m32 for i in range(4)]
    k = [np.asarray(key, np.uint64)[..., i] & m32 for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]      # < 2^64: no wrap
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return np.stack(np.broadcast_arrays(*c), axis=-1)


def ref_noise_at(keys, counters):
    """(B,N,3) float64 standard normals of sample b from the counters (c, 0, 0, 0), c = counters (N,) for every sample or
    (B,N), under key keys[b]: what a pixel whose pre-flip index in the whole output is c receives."""
    keys = np.asarray(keys).astype(np.int64) & 0xFFFFFFFF
    c0 = np.broadcast_to(np.asarray(counters, np.int64), (len(keys),) + np.shape(counters)[-1:])
    assert c0.min() >= 0 and c0.max() <= 0xFFFFFFFF
    counter = np.zeros(c0.shape + (4,), np.uint64)
    counter[..., 0] = c0
    r = ref_philox(counter, keys.astype(np.uint64)[:, None, :]).astype(np.float64)
    u = np.floor(r / 256.0)                                                     # r >> 8
    u1, u2, v1, v2 = (u[..., 0] + 1) / 2 ** 24, u[..., 1] / 2 ** 24, (u[..., 2] + 1) / 2 ** 24, u[..., 3] / 2 ** 24
    rad, rad2 = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(v1))
    return np.stack([rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2), rad2 * np.cos(2 * np.pi * v2)], axis=-1)


def ref_noise(keys, h, w):
    """(B,h,w,3) float64 standard normals: pixel (y, x) of sample b from counter (y * w + x, 0, 0, 0), key keys[b]."""
    return ref_noise_at(keys, np.arange(h * w)).reshape(len(keys), h, w, 3)


def ref_resize(x, h, w):
    """tf.image.resize(BILINEAR) of (..., H, W, 3) float64: half-pixel centres, no antialias, rows after columns."""
    def axis(n_out, n_in):
        src = (np.arange(n_out) + 0.5) * (n_in / float(n_out)) - 0.5
        lo = np.clip(np.floor(src), 0, n_in - 1).astype(int)
        hi = np.clip(np.ceil(src), 0, n_in - 1).astype(int)
        return lo, hi, src - np.floor(src)
    H, W = x.shape[-3:-1]
    (y0, y1, ty), (x0, x1, tx) = axis(h, H), axis(w, W)
    tx, ty = tx[:, None], ty[:, None, None]
    top = x[..., y0, :, :][..., :, x0, :] + (x[..., y0, :, :][..., :, x1, :] - x[..., y0, :, :][..., :, x0, :]) * tx
    bot = x[..., y1, :, :][..., :, x0, :] + (x[..., y1, :, :][..., :, x1, :] - x[..., y1, :, :][..., :, x0, :]) * tx
    return top + (bot - top) * ty


def ref_triplet(a, b, c, iparams, fparams, dsize, finish=True, noise_before_flips=True, noise=None):
    """-> (img_pair (B,h,w,6), img1 (B,h,w,3)) float64, channels_last.  noise_before_flips=False is the nearest wrong
    reading (the noise indexed by the output pixel), for the negative control.  noise: the (B,h,w,3) standard normals of
    the pre-flip pixels, for a window of a larger output whose counters are not its own (ref_noise_at)."""
    h, w = dsize
    fp = np.asarray(fparams, np.float64)
    x = np.stack([a, b, c], axis=0)
    x = x.astype(np.float64) * np.float64(INV255) if x.dtype == np.uint8 else x.astype(np.float64)
    x = ref_resize(x, h, w)                                                     # (3,B,h,w,3)
    if noise is None:
        noise = ref_noise(np.asarray(iparams)[:, 2:4], h, w)
    assert noise.shape == (x.shape[1], h, w, 3)
    out = np.empty_like(x)
    for n in range(x.shape[1]):
        R, scale, txn, sigma = fp[n, 0:9].reshape(3, 3), fp[n, 9:12], fp[n, 12:15], fp[n, 15]
        y = x[:, n] @ R.T * scale + txn
        if noise_before_flips:
            y = y + sigma * noise[n]
        if iparams[n][0]:
            y = y[:, ::-1]
        if iparams[n][1]:
            y = y[:, :, ::-1]
        if not noise_before_flips:
            y = y + sigma * noise[n]
        out[:, n] = y
    if finish:
        out = out - 0.5
    return np.concatenate([out[0], out[2]], axis=-1), out[1]


# ---- the cases, built once (tests/test_gpu_triplet.py imports CASES) -------------------------------------------------
def _params(B, seed, sigma=0.02):
    """Distinct R / scale / txn / key per sample, inside the sampler's ranges; flips cycle through the combinations."""
    rng = np.random.default_rng(seed)
    ip = np.zeros((B, 4), np.int32)
    ip[:, 0], ip[:, 1] = (np.arange(B) >> 1) & 1, np.arange(B) & 1
    ip[:, 2:4] = rng.integers(-2 ** 31, 2 ** 31, (B, 2)).astype(np.int32)
    fp = np.zeros((B, 16), np.float32)
    fp[:, 0:9] = augment.rotation_matrix_from_euler(torch.from_numpy(rng.uniform(-0.3, 0.3, (B, 3)))).reshape(B, 9).numpy()
    fp[:, 9:12] = np.exp(rng.uniform(-0.3, 0.3, (B, 3)))
    fp[:, 12:15] = rng.uniform(-0.3, 0.3, (B, 3))
    fp[:, 15] = sigma
    return ip, fp


def _case(dtype, B, H, W, h, w, seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) for _ in range(3)]
    if dtype == np.float32:
        frames = [f.astype(np.float32) * INV255 for f in frames]
    return tuple(frames) + _params(B, seed + 100) + ((h, w),)


def _build_cases():
    cases = {
        "u8": _case(np.uint8, 4, 37, 53, 24, 40, 0),        # 960 pixels: <vec4>, three whole workgroups and 192 pixels
        "f32": _case(np.float32, 4, 37, 53, 24, 40, 0),
        "tiny": _case(np.uint8, 2, 9, 11, 5, 7, 1),         # 35 pixels: <scalar>
        "same": _case(np.uint8, 4, 12, 20, 12, 20, 2),      # H == h, W == w: no resampling
    }
    return {k: (v, ref_triplet(*v), ref_triplet(*v, finish=False)) for k, v in cases.items()}


CASES = _build_cases()       # name -> (case, (pair, mid) finished, (pair, mid) raw), the answers float64 channels_last
FORMS = {"u8": "vec4", "f32": "vec4", "tiny": "scalar", "same": "vec4"}


def as_tparams(ip, fp, device="cpu"):
    return augment.TripletParams(torch.from_numpy(np.ascontiguousarray(ip)).to(device),
                                 torch.from_numpy(np.ascontiguousarray(fp)).to(device))


def max_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max())


# ---- Philox and the noise field -------------------------------------------------------------------------------------
KNOWN = (
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        want = [int(v, 16) for v in want.split()]
        assert augment.philox4x32(torch.tensor(counter), torch.tensor(key)).tolist() == want
        assert ref_philox(np.array(counter, np.uint64), np.array(key, np.uint64)).tolist() == want
    # int32 bit patterns are the same words, and a batch is its rows
    got = augment.philox4x32(torch.tensor([[-1, -1, -1, -1], [0, 0, 0, 0]], dtype=torch.int32),
                             torch.tensor([[-1, -1], [0, 0]], dtype=torch.int32))
    assert got.dtype == torch.int64 and got[0].tolist() == [int(v, 16) for v in KNOWN[1][2].split()]
    assert got[1].tolist() == [int(v, 16) for v in KNOWN[0][2].split()]


def test_noise_matches_the_restatement_and_is_standard_normal():
    ip = CASES["u8"][0][3]
    z = augment.triplet_noise(torch.from_numpy(ip[:, 2:4]), 24, 40)
    want = ref_noise(ip[:, 2:4], 24, 40)
    assert z.dtype == torch.float32 and tuple(z.shape) == (4, 24, 40, 3)
    assert max_err(z.numpy(), want) <= 1e-5                 # a few fp32 ulps of a number < 6
    n = z.numel()
    assert n == 11520
    for field in (want, z.numpy().astype(np.float64)):      # 5 standard errors of the mean and of the deviation
        print("noise: mean {:+.4f} (bound {:.4f}), std - 1 {:+.4f} (bound {:.4f})".format(
            field.mean(), 5 / math.sqrt(n), field.std() - 1, 5 / math.sqrt(2 * n)))
        assert abs(field.mean()) <= 5 / math.sqrt(n)
        assert abs(field.std() - 1.0) <= 5 / math.sqrt(2 * n)
        assert np.abs(field).max() <= math.sqrt(48 * math.log(2)) + 1e-5


def test_same_key_same_field_different_key_different_field():
    keys = torch.tensor([[7, -9], [7, -9], [7, -8], [8, -9]], dtype=torch.int32)
    z = augment.triplet_noise(keys, 6, 10)
    assert torch.equal(z[0], z[1]) and not torch.equal(z[0], z[2]) and not torch.equal(z[0], z[3])
    assert torch.equal(augment.triplet_noise(keys, 6, 10), z)
    # a field is a function of the pixel's index y * w + x alone
    assert torch.equal(augment.triplet_noise(keys, 3, 20).reshape(4, 60, 3), z.reshape(4, 60, 3))


# ---- the colour rotation --------------------------------------------------------------------------------------------
def test_rotation_matrix_from_euler():
    rng = np.random.default_rng(4)
    ang = rng.uniform(-math.pi, math.pi, (16, 3))
    got = augment.rotation_matrix_from_euler(torch.from_numpy(ang.astype(np.float32)))
    assert tuple(got.shape) == (16, 3, 3) and got.dtype == torch.float32
    ang = ang.astype(np.float32).astype(np.float64)
    for i, (x, y, z) in enumerate(ang):
        Rx = np.array([[1, 0, 0], [0, math.cos(x), -math.sin(x)], [0, math.sin(x), math.cos(x)]])
        Ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
        Rz = np.array([[math.cos(z), -math.sin(z), 0], [math.sin(z), math.cos(z), 0], [0, 0, 1]])
        assert max_err(got[i].numpy(), Rz @ Ry @ Rx) <= 1e-6
        g = got[i].numpy().astype(np.float64)
        assert np.abs(g @ g.T - np.eye(3)).max() <= 1e-6
    assert tuple(augment.rotation_matrix_from_euler(torch.zeros(2, 5, 3)).shape) == (2, 5, 3, 3)
    assert torch.equal(augment.rotation_matrix_from_euler(torch.zeros(3)), torch.eye(3))


# ---- the CPU path against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("finish", [True, False], ids=["finish", "raw"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("name", ["u8", "f32", "tiny", "same"])
def test_triplet_torch_matches_the_restatement(name, data_format, finish):
    (a, b, c, ip, fp, hw), fin, raw = CASES[name]
    want = fin if finish else raw
    got = augment.triplet_torch(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c), as_tparams(ip, fp), hw,
                                finish=finish, data_format=data_format)
    for g, r in zip(got, want):
        r = r.transpose(0, 3, 1, 2) if data_format == "channels_first" else r
        assert g.dtype == torch.float32 and tuple(g.shape) == r.shape and g.is_contiguous()
        assert np.abs(r).max() < 3.0
        e = max_err(g.numpy(), r)
        print("triplet_torch {} {} finish={}: max |err| {:.3e}".format(name, data_format, finish, e))
        assert e <= BOUND


def test_the_restatement_tells_the_nearest_wrong_reading():
    (a, b, c, ip, fp, hw), fin, _ = CASES["u8"]
    wrong = ref_triplet(a, b, c, ip, fp, hw, noise_before_flips=False)
    assert np.array_equal(wrong[0][0], fin[0][0])                      # sample 0 has no flip
    assert np.abs(wrong[0][3] - fin[0][3]).max() > 100 * BOUND


def test_entry_points_on_the_cpu():
    (a, b, c, ip, fp, hw), fin, raw = CASES["u8"]
    ta, tb, tc = (torch.from_numpy(v) for v in (a, b, c))
    pair, mid = augment.preprocess_triplet(ta, tb, tc, hw, "channels_first", params=as_tparams(ip, fp))
    assert max_err(pair.numpy(), fin[0].transpose(0, 3, 1, 2)) <= BOUND
    assert max_err(mid.numpy(), fin[1].transpose(0, 3, 1, 2)) <= BOUND
    i0, i1, i2 = augment.augment_triplet(ta, tb, tc, hw, params=(torch.from_numpy(ip), torch.from_numpy(fp)))
    assert max_err(i0.numpy(), raw[0][..., 0:3]) <= BOUND and max_err(i2.numpy(), raw[0][..., 3:6]) <= BOUND
    assert max_err(i1.numpy(), raw[1]) <= BOUND
    # the validation path: the resize and the offset alone
    pair, mid = augment.preprocess_triplet(ta, tb, tc, hw, "channels_last", augment=False)
    idp = augment.identity_triplet_params(4)
    want = ref_triplet(a, b, c, idp.iparams.numpy(), idp.fparams.numpy(), hw)
    assert max_err(pair.numpy(), want[0]) <= BOUND and max_err(mid.numpy(), want[1]) <= BOUND
    # a draw of its own, repeatable under a seeded generator
    g = lambda: torch.Generator().manual_seed(11)
    one, two = (augment.preprocess_triplet(ta, tb, tc, hw, generator=g()) for _ in range(2))
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and tuple(one[0].shape) == (4, 6, 24, 40)
    other = augment.preprocess_triplet(ta, tb, tc, hw, generator=torch.Generator().manual_seed(12))
    assert not torch.equal(one[0], other[0])


def test_identity_is_exact_on_the_cpu():
    a, b, c = (CASES["same"][0][i] for i in range(3))
    pair, mid = augment.preprocess_triplet(*(torch.from_numpy(v) for v in (a, b, c)), (12, 20), "channels_last",
                                           augment=False)
    plain = lambda v: v.astype(np.float32) * INV255 - np.float32(0.5)
    assert np.array_equal(pair.numpy(), np.concatenate([plain(a), plain(c)], -1)) and np.array_equal(mid.numpy(), plain(b))


def test_inputs_are_checked():
    a = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for bad in (a.float().half(), a[:, :, :, :2], a.permute(0, 2, 1, 3)[:, :, ::2], a[0]):
        with pytest.raises(ValueError):
            augment.preprocess_triplet(a, bad, a, (4, 4))
    with pytest.raises(ValueError, match="does not match"):
        augment.preprocess_triplet(a, a.float(), a, (4, 4))
    with pytest.raises(ValueError, match="does not match"):
        augment.preprocess_triplet(a, a, torch.zeros(2, 8, 9, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(TypeError):
        augment.preprocess_triplet(a, a.numpy(), a, (4, 4))
    with pytest.raises(ValueError, match="params.iparams"):
        augment.preprocess_triplet(a, a, a, (4, 4), params=augment.identity_triplet_params(3))
    with pytest.raises(ValueError):
        augment.preprocess_triplet(a, a, a, (4, 4), data_format="nhwc")
    from qpwcnet_amd import ops
    p = augment.identity_triplet_params(2)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.augment_triplet(a, a, a, p.iparams, p.fparams, (4, 4))


# ---- the sampler ----------------------------------------------------------------------------------------------------
def test_sample_triplet_params_ranges_and_reproducibility():
    g = lambda seed=3: torch.Generator().manual_seed(seed)
    p = augment.sample_triplet_params(512, generator=g())
    q = augment.sample_triplet_params(512, generator=g())
    assert isinstance(p, augment.TripletParams) and torch.equal(p.iparams, q.iparams) and torch.equal(p.fparams, q.fparams)
    assert not torch.equal(p.fparams, augment.sample_triplet_params(512, generator=g(4)).fparams)
    assert p.iparams.dtype == torch.int32 and tuple(p.iparams.shape) == (512, 4) and p.iparams.is_contiguous()
    assert p.fparams.dtype == torch.float32 and tuple(p.fparams.shape) == (512, 16) and p.fparams.is_contiguous()
    ip, fp = p.iparams.numpy(), p.fparams.numpy().astype(np.float64)
    assert set(np.unique(ip[:, 0:2])) == {0, 1}
    assert 0.35 < ip[:, 0].mean() < 0.65 and 0.35 < ip[:, 1].mean() < 0.65
    assert len(np.unique(ip[:, 2:4])) > 1000 and (ip[:, 2:4] < 0).any() and (ip[:, 2:4] > 0).any()    # 32-bit words
    tol = 1e-6
    assert (fp[:, 9:12] >= math.exp(-0.3) - tol).all() and (fp[:, 9:12] <= math.exp(0.3) + tol).all()
    assert fp[:, 9:12].min() < 0.8 and fp[:, 9:12].max() > 1.25
    assert (np.abs(fp[:, 12:15]) <= 0.3 + tol).all() and np.abs(fp[:, 12:15]).max() > 0.25
    assert (fp[:, 15] == np.float32(0.02)).all()
    R = fp[:, 0:9].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    # the angles stay inside max_rxn: -sin(y) = R[2, 0]
    assert np.abs(R[:, 2, 0]).max() <= math.sin(0.3) + tol and np.abs(R[:, 2, 0]).max() > math.sin(0.25)
    zero = augment.sample_triplet_params(8, max_txn=0.0, max_rxn=0.0, max_scale=0.0, noise=0.0, generator=g())
    assert torch.equal(zero.fparams, augment.identity_triplet_params(8).fparams)
    with pytest.raises(ValueError):
        augment.sample_triplet_params(0)


def test_identity_triplet_params():
    p = augment.identity_triplet_params(3)
    assert p.iparams.dtype == torch.int32 and not p.iparams.any() and tuple(p.iparams.shape) == (3, 4)
    assert p.fparams.dtype == torch.float32 and tuple(p.fparams.shape) == (3, 16)
    assert torch.equal(p.fparams[:, 0:9].reshape(3, 3, 3), torch.eye(3).expand(3, 3, 3))
    assert torch.equal(p.fparams[:, 9:12], torch.ones(3, 3)) and not p.fparams[:, 12:16].any()


# ---- the ctypes table against the header ----------------------------------------------------------------------------
def test_triplet_prototypes_match_their_header():
    protos = parse_header(TRIPLET_HEADER)
    assert [name for name, _, _ in protos] == ["qpwc_augment_triplet_fwd", "qpwc_augment_triplet_fwd_kernel"]
    assert mismatches(_hip.TRIPLET_PROTOTYPES, protos) == []
    assert len(_hip.SYMBOLS) == 77 and not set(_hip.TRIPLET_PROTOTYPES) & (set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES))
    table = dict(_hip.TRIPLET_PROTOTYPES)
    restype, argtypes = table["qpwc_augment_triplet_fwd"]
    table["qpwc_augment_triplet_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_augment_triplet_fwd: 16 parameters, table has 15"]
    assert _hip.TRIPLET_RAW == 1


def test_the_library_exports_the_table(hip_lib):
    for name, (restype, argtypes) in _hip.TRIPLET_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)

"""The input pipeline for sparse ground truth (qpwcnet_amd/augment.py ``*_sparse``, qpwc_augment_sparse_fwd) without a GPU:
  * ``ref_augment_sparse``: a float64 numpy restatement of include/qpwc_sparse_augment.h, one sample at a time.  The source
    coordinates, the weights t and the factors w_k are formed in numpy float32 exactly as the contract states them; the
    sums and the division are float64.  The mask depends on those fp32 values only, so an output mask must equal the
    restatement's in every pixel; the flow is held to the project's bound where the mask is 1 and to exactly 0 where not
    (tests/test_gpu_sparse_augment.py imports all of it);
  * the inputs: the two cases of tests/test_augment_cpu.py under a half-density mask with NaN, +Inf and 1e10 planted, and
    the proof that both hold output pixels with 0, 1, 2, 3 and 4 valid corners;
  * ``sparse_torch`` and the four entry points against the restatement; known answers; negative controls.
"""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import BOUND, as_params, make_case, max_err, ref_augment, tiny_case  # noqa: E402

from qpwcnet_amd import augment, metrics  # noqa: E402

FORMATS = ("channels_last", "channels_first")
F32 = np.float32


# ---- the restatement ------------------------------------------------------------------------------------------------
def axis_f32(i, n_in, n_out, dtype=np.float32):
    """aug_axis (csrc/augment_common.h) for output indices i, every operation rounded to `dtype`: (lo, hi, t)."""
    s = (np.asarray(i).astype(dtype) + dtype(0.5)) * (dtype(n_in) / dtype(n_out)) - dtype(0.5)
    f = np.floor(s)
    lo = np.clip(f, 0, n_in - 1).astype(np.int64)
    hi = np.clip(np.ceil(s), 0, n_in - 1).astype(np.int64)
    t = s - f
    assert t.dtype == dtype
    return lo, hi, t


def source_validity(flo, valid=None):
    with np.errstate(invalid="ignore"):
        ok = (np.abs(flo[..., 0]) <= metrics.FLOW_UNKNOWN) & (np.abs(flo[..., 1]) <= metrics.FLOW_UNKNOWN)
    return ok if valid is None else ok & (np.asarray(valid) != 0)


def corner_geometry(ip_row, H, W, out_shape, dtype=np.float32):
    """The four corners of every output pixel of one sample, in the order 00, 01, 10, 11: [(ys (h,1), xs (1,w))] and the
    weights ty (h,), tx (w,) in `dtype`."""
    rh, rw, oy, ox, ud, lr = (int(v) for v in ip_row)
    h, w = out_shape
    y0, y1, ty = axis_f32(oy + np.arange(h), H, rh, dtype)
    x0, x1, tx = axis_f32(ox + np.arange(w), W, rw, dtype)
    if ud:
        y0, y1 = H - 1 - y0, H - 1 - y1
    if lr:
        x0, x1 = W - 1 - x0, W - 1 - x1
    return [(yy[:, None], xx[None, :]) for yy in (y0, y1) for xx in (x0, x1)], ty, tx


def corner_counts(flo, valid, ip, out_shape, dtype=np.float32):
    """(B,h,w) int: the number of valid corners of every output pixel."""
    B, H, W, _ = flo.shape
    ok = source_validity(flo, valid)
    return np.stack([sum(ok[b][c].astype(np.int64) for c in corner_geometry(ip[b], H, W, out_shape, dtype)[0])
                     for b in range(B)])


def ref_augment_sparse(ims, flo, valid, iparams, fparams, out_shape, colour=True, finish=True,
                       data_format="channels_last", no_division=False, dense_over_zero_fill=False):
    """float64 (ims, flo), uint8 valid (B,h,w).  The frames are ref_augment's.  no_division / dense_over_zero_fill build
    the two WRONG flows of the negative controls: the weighted sum without / S, and the dense bilinear value of the flow
    with zeros at its invalid pixels."""
    ims, flo = np.asarray(ims), np.asarray(flo, np.float32)
    fparams = np.asarray(fparams, np.float32)
    B, H, W, _ = ims.shape
    h, w = out_shape
    o_ims, _ = ref_augment(ims, np.zeros_like(flo), iparams, fparams, out_shape, colour=colour, finish=finish)
    ok = source_validity(flo, valid)
    clean = np.where(ok[..., None], flo, 0.0).astype(np.float64)
    o_flo, o_valid = np.zeros((B, h, w, 2)), np.zeros((B, h, w), np.uint8)
    for b in range(B):
        corners, ty, tx = corner_geometry(iparams[b], H, W, out_shape)
        one = F32(1.0)
        ly, lx = ((one - ty)[:, None], ty[:, None]), ((one - tx)[None, :], tx[None, :])
        wk = [ly[k // 2] * lx[k % 2] for k in range(4)]                     # fp32 products
        assert all(x.dtype == np.float32 for x in wk)
        v = [ok[b][c] for c in corners]
        f = [clean[b][c] for c in corners]
        n = sum(x.astype(np.int64) for x in v)
        S = sum(np.where(v[k], wk[k].astype(np.float64), 0.0) for k in range(4))
        num = sum(np.where(v[k], wk[k].astype(np.float64), 0.0)[..., None] * f[k] for k in range(4))
        assert (S[n > 0] > 0).all()
        tx_, ty_ = tx.astype(np.float64)[None, :, None], ty.astype(np.float64)[:, None, None]
        top, bot = f[0] + (f[1] - f[0]) * tx_, f[2] + (f[3] - f[2]) * tx_
        lerp = top + (bot - top) * ty_
        part = num if no_division else num / np.where(n > 0, S, 1.0)[..., None]
        val = np.where((n == 4)[..., None], lerp, np.where((n > 0)[..., None], part, 0.0))
        if dense_over_zero_fill:
            val = np.where((n > 0)[..., None], lerp, 0.0)
        o_flo[b] = val * fparams[b, :2].astype(np.float64)
        o_valid[b] = n > 0
    if data_format == "channels_first":
        return o_ims.transpose(0, 3, 1, 2), o_flo.transpose(0, 3, 1, 2), o_valid
    return o_ims, o_flo, o_valid


# ---- fixtures shared with the GPU suite -----------------------------------------------------------------------------
MASK_SEEDS = {"make": 100, "tiny": 101}
PLANTED = (np.nan, np.inf, 1e10)


def base_mask(name, shape):
    return np.random.default_rng(MASK_SEEDS[name]).random(shape) < 0.5


def sparse_case(name, dtype=np.uint8):
    """'make' / 'tiny': make_case / tiny_case with the half-density mask of MASK_SEEDS, and, on top of it, in every sample
    three pixels whose mask is 1 made invalid through their flow: NaN in u, +Inf in v, 1e10 in u.
    -> ims, flo, mask (bool), ip, fp, hw."""
    ims, flo, ip, fp, hw = make_case(dtype) if name == "make" else tiny_case()
    flo = flo.copy()
    mask = base_mask(name, flo.shape[:3])
    for b in range(flo.shape[0]):
        ys, xs = np.nonzero(mask[b])
        pick = np.linspace(0, len(ys) - 1, 5).astype(int)[1:4]                # three, spread over the image
        for (y, x), bad, c in zip(zip(ys[pick], xs[pick]), PLANTED, (0, 1, 0)):
            flo[b, y, x, c] = bad
    return ims, flo, mask, ip, fp, hw


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.uint8, colour=True, finish=True, with_mask=True):
    """The restatement of a case, computed once, channels_last; treat as read-only."""
    ims, flo, mask, ip, fp, hw = sparse_case(name, dtype)
    return ref_augment_sparse(ims, flo, mask if with_mask else None, ip, fp, hw, colour=colour, finish=finish)


def to_format(x, data_format):
    return x if data_format == "channels_last" else np.ascontiguousarray(np.moveaxis(x, -1, 1))


def check_against(got, want, data_format="channels_last", what=""):
    """The contract's three assertions for outputs in data_format against a channels_last restatement -> the measured
    maxima (frames, flow where the mask is 1)."""
    g_ims, g_flo, g_valid = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in got)
    w_ims, w_flo, w_valid = want
    assert g_valid.dtype == np.uint8 and g_valid.shape == w_valid.shape
    assert np.array_equal(g_valid, w_valid), "{}: {} mask pixels differ".format(what, int((g_valid != w_valid).sum()))
    w_ims, w_flo = to_format(w_ims, data_format), to_format(w_flo, data_format)
    assert g_ims.shape == w_ims.shape and g_flo.shape == w_flo.shape and g_flo.dtype == np.float32
    m = np.broadcast_to(np.expand_dims(w_valid != 0, -1 if data_format == "channels_last" else 1), g_flo.shape)
    assert np.isfinite(g_flo).all() and (g_flo[~m] == 0).all(), what
    e_ims, e_flo = max_err(g_ims, w_ims), max_err(g_flo[m], w_flo[m])
    print("sparse augment {} {}: max |ims err| {:.3e}, max |flow err| {:.3e} px".format(what, data_format, e_ims, e_flo))
    assert e_ims <= BOUND and e_flo <= BOUND, (what, e_ims, e_flo)
    return e_ims, e_flo


def torch_case(case, device="cpu"):
    ims, flo, mask, ip, fp, hw = case
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    return t(ims), t(flo), t(mask), as_params(ip, fp, device), hw


# ---- the inputs reach every branch ----------------------------------------------------------------------------------
def _classes(n):
    return [int((n == k).sum()) for k in range(5)]


def test_cases_hold_every_number_of_valid_corners():
    """make_case under mask seed 100: every sample has at least 18 pixels in every class (0..4 valid corners), sample 0
    31 / 98 / 139 / 88 / 28; tiny_case under seed 101: 4 / 9 / 17 / 4 / 1.  float32 and float64 coordinates give the same
    classes, and every class stays populated after NaN, +Inf and 1e10 are planted."""
    for name, floor in (("make", 18), ("tiny", 1)):
        ims, flo, mask, ip, fp, hw = sparse_case(name)
        clean = np.zeros_like(flo)
        n32, n64 = (corner_counts(clean, mask, ip, hw, dt) for dt in (np.float32, np.float64))
        assert np.array_equal(n32, n64)
        for b in range(len(n32)):
            print("sparse augment classes {} sample {} mask alone: {}".format(name, b, _classes(n32[b])))
            assert min(_classes(n32[b])) >= floor, (name, b, _classes(n32[b]))
        planted = corner_counts(flo, mask, ip, hw)
        assert np.array_equal(planted, corner_counts(flo, mask, ip, hw, np.float64))
        assert (planted <= n32).all() and (planted < n32).any()
        for b in range(len(planted)):
            print("sparse augment classes {} sample {} planted: {}".format(name, b, _classes(planted[b])))
            assert min(_classes(planted[b])) >= 1, (name, b, _classes(planted[b]))
        assert source_validity(flo, mask).sum() == mask.sum() - 3 * len(flo)         # the planted pixels had mask 1
    assert _classes(corner_counts(np.zeros((4, 30, 52, 2), F32), base_mask("make", (4, 30, 52)), make_case(np.uint8)[2],
                                  (16, 24))[0]) == [31, 98, 139, 88, 28]
    assert _classes(corner_counts(np.zeros((1, 11, 9, 2), F32), base_mask("tiny", (1, 11, 9)), tiny_case()[2],
                                  (7, 5))) == [4, 9, 17, 4, 1]
    # the forms the two cases take are checked where the library is loaded (test_sparse_augment_capi_cpu.py)
    assert (16 * 24) % 4 == 0 and (7 * 5) % 4 != 0 and 16 * 24 == 256 + 128


def test_the_restatement_with_everything_valid_is_the_dense_one():
    ims, flo, ip, fp, hw = make_case(np.uint8)
    want = ref_augment(ims, flo, ip, fp, hw)
    got = ref_augment_sparse(ims, flo, None, ip, fp, hw)
    assert np.array_equal(got[0], want[0]) and max_err(got[1], want[1]) < 1e-5 and got[2].all()
    # and the fp32 coordinates move the dense flow by far less than the bound (smooth_flow: ~2 px per pixel)
    ones = ref_augment_sparse(ims, flo, np.ones(flo.shape[:3], np.uint8), ip, fp, hw)
    assert np.array_equal(ones[1], got[1])


# ---- the torch-composed CPU path and the entry points ---------------------------------------------------------------
@pytest.mark.parametrize("data_format", FORMATS)
@pytest.mark.parametrize("name,dtype", [("make", np.uint8), ("make", np.float32), ("tiny", np.uint8)])
def test_sparse_torch_matches_restatement(name, dtype, data_format):
    """Measured on the CPU path: frames 4.5e-6 with the colour stage and 2.2e-6 without (make_case, uint8), 3.7e-7 and
    1.9e-7 (tiny_case); flow 4.3e-6 px (make_case) and 2.3e-6 px (tiny_case) where the mask is 1; the masks equal the
    restatement's in every pixel."""
    ims, flo, mask, params, hw = torch_case(sparse_case(name, dtype))
    for colour, with_mask in itertools.product((True, False), (True, False)):
        got = augment.sparse_torch(ims, flo, mask if with_mask else None, params, hw, colour=colour,
                                   data_format=data_format)
        assert all(t.is_contiguous() for t in got)
        check_against(got, reference(name, dtype, colour, True, with_mask), data_format,
                      "torch {} colour={} mask={}".format(name, colour, with_mask))


@pytest.mark.parametrize("data_format", FORMATS)
def test_entry_points_match_restatement(data_format):
    case = sparse_case("make", np.uint8)
    ims, flo, mask, params, hw = torch_case(case)
    got = augment.preprocess_sparse(ims, flo, mask, data_format, out_shape=hw, params=params)
    check_against(got, reference("make"), data_format, "preprocess_sparse")
    B, H, W, _ = ims.shape
    rp = augment.resize_params(B, (H, W), hw)
    want = ref_augment_sparse(case[0], case[1], case[2], rp.iparams.numpy(), rp.fparams.numpy(), hw, colour=False)
    got = augment.preprocess_no_op_sparse(ims, flo, mask, data_format, out_shape=hw)
    check_against(got, want, data_format, "preprocess_no_op_sparse")
    if data_format == "channels_last":
        f_case = sparse_case("make", np.float32)
        f_ims = torch.from_numpy(f_case[0])
        got = augment.image_augment_sparse(f_ims, flo, hw, valid=mask, params=params)
        check_against(got, reference("make", np.float32, True, False), what="image_augment_sparse")
        want = ref_augment_sparse(f_case[0], case[1], case[2], rp.iparams.numpy(), rp.fparams.numpy(), hw, colour=False,
                                  finish=False)
        check_against(augment.image_resize_sparse(f_ims, flo, hw, valid=mask), want, what="image_resize_sparse")
        # the sampler: the same generator state gives the dense pipeline's draw
        g = lambda: torch.Generator().manual_seed(11)
        a = augment.image_augment_sparse(f_ims, flo, hw, valid=mask, generator=g())
        p = augment.sample_params(B, (H, W), hw, 1.0, generator=g())
        b = augment.image_augment_sparse(f_ims, flo, hw, valid=mask, params=p)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_masks_of_every_dtype_mean_the_same():
    ims, flo, mask, params, hw = torch_case(sparse_case("tiny"))
    want = augment.preprocess_sparse(ims, flo, mask, out_shape=hw, params=params)
    for m in (mask.to(torch.uint8), mask.to(torch.uint8) * 255, mask.to(torch.uint8) * 2, mask.float() * 0.25,
              mask.double()):
        got = augment.preprocess_sparse(ims, flo, m, out_shape=hw, params=params)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), m.dtype


@pytest.mark.parametrize("data_format", FORMATS)
def test_all_valid_is_the_dense_pipeline_bit_for_bit(data_format):
    for ims, flo, ip, fp, hw in (make_case(np.uint8), make_case(np.float32), tiny_case()):
        t_ims, t_flo, p = torch.from_numpy(ims), torch.from_numpy(flo), as_params(ip, fp)
        want = augment.preprocess(t_ims, t_flo, data_format, out_shape=hw, params=p)
        for valid in (None, torch.ones(flo.shape[:3], dtype=torch.bool)):
            got = augment.preprocess_sparse(t_ims, t_flo, valid, data_format, out_shape=hw, params=p)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert got[2].dtype == torch.uint8 and tuple(got[2].shape) == (len(ims),) + hw and bool((got[2] == 1).all())


def identity_sparse_case():
    """All four flip combinations of one sample at identity geometry under a mask -> inputs and the exact answers."""
    rng = np.random.default_rng(6)
    H, W = 10, 14
    flips = list(itertools.product((0, 1), (0, 1)))
    ims = np.repeat(rng.integers(0, 256, (1, H, W, 6), dtype=np.uint8), 4, 0)
    flo = np.repeat(rng.standard_normal((1, H, W, 2)).astype(np.float32), 4, 0)
    mask = np.repeat(rng.random((1, H, W)) < 0.5, 4, 0)
    flo[:, 2, 3, 0], flo[:, 7, 1, 1] = np.nan, 1e10
    mask[:, 2, 3] = mask[:, 7, 1] = True
    ip = np.array([[H, W, 0, 0, ud, lr] for ud, lr in flips], np.int32)
    fp = np.array([[1 - 2 * lr, 1 - 2 * ud, 0, 1, 0, 1] for ud, lr in flips], np.float32)
    ok = source_validity(flo, mask)
    want_flo, want_valid = np.where(ok[..., None], flo, F32(0)), ok.astype(np.uint8)
    for b, (ud, lr) in enumerate(flips):
        if ud:
            want_flo[b], want_valid[b] = want_flo[b, ::-1] * F32([1, -1]), want_valid[b, ::-1]
        if lr:
            want_flo[b], want_valid[b] = want_flo[b, :, ::-1] * F32([-1, 1]), want_valid[b, :, ::-1]
    return (ims, flo, mask, ip, fp, (H, W)), want_flo, want_valid


def test_identity_scale_with_each_flip_is_exact():
    case, want_flo, want_valid = identity_sparse_case()
    assert 0.3 < want_valid.mean() < 0.7
    r_ims, r_flo, r_valid = ref_augment_sparse(*case, colour=False)
    assert np.array_equal(r_valid, want_valid) and np.array_equal(r_flo, want_flo.astype(np.float64))
    ims, flo, mask, params, hw = torch_case(case)
    got = augment.sparse_torch(ims, flo, mask, params, hw, colour=False)
    assert np.array_equal(got[2].numpy(), want_valid) and np.array_equal(got[1].numpy(), want_flo)


def garbage_pair(name="make", dtype=np.uint8):
    """Two inputs with one meaning: zeros at the invalid pixels, mask bytes 0 / 1; and NaN, Inf, 1e30 there with mask
    bytes 0, 2 and 255 -- wherever the mask byte is non-zero the flow itself is what makes the pixel invalid."""
    ims, flo, mask, ip, fp, hw = sparse_case(name, dtype)
    ok = source_validity(flo, mask)
    rng = np.random.default_rng(7)
    plain_flo, plain_mask = np.where(ok[..., None], flo, F32(0)), ok.astype(np.uint8)
    junk = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32), size=flo.shape)
    keep_one = rng.integers(0, 3, ok.shape)                      # 0: u is junk, 1: v is junk, 2: both
    dirty_flo = flo.copy()
    dirty_flo[..., 0] = np.where(~ok & (keep_one != 1), junk[..., 0], np.where(ok, flo[..., 0], F32(3.0)))
    dirty_flo[..., 1] = np.where(~ok & (keep_one != 0), junk[..., 1], np.where(ok, flo[..., 1], F32(-2.0)))
    dirty_mask = np.where(ok, rng.choice(np.array([1, 2, 255], np.uint8), size=ok.shape),
                          rng.choice(np.array([0, 2, 255], np.uint8), size=ok.shape)).astype(np.uint8)
    # a finite flow at an invalid pixel needs the mask byte 0
    finite = ~ok & (np.abs(np.nan_to_num(dirty_flo, nan=np.inf)) <= 1e9).all(-1)
    dirty_mask[finite] = 0
    assert np.array_equal(source_validity(dirty_flo, dirty_mask), ok) and (dirty_mask[~ok] != 0).any()
    assert {2, 255} <= set(np.unique(dirty_mask[ok]))
    return (ims, plain_flo, plain_mask, ip, fp, hw), (ims, dirty_flo, dirty_mask, ip, fp, hw)


@pytest.mark.parametrize("name", ["make", "tiny"])
def test_selected_out_pixels_change_no_bit(name):
    plain, dirty = garbage_pair(name)
    for data_format in FORMATS:
        outs = []
        for case in (plain, dirty):
            ims, flo, mask, params, hw = torch_case(case)
            outs.append(augment.preprocess_sparse(ims, flo, mask, data_format, out_shape=hw, params=params))
        for a, b in zip(*outs):
            assert torch.equal(a, b) and a.numpy().tobytes() == b.numpy().tobytes()
    check_against(outs[1], reference(name), FORMATS[-1], "garbage " + name)


def test_constant_flow_over_the_valid_pixels_stays_constant():
    ims, flo, mask, ip, fp, hw = sparse_case("make")
    ok = source_validity(flo, mask)
    const = np.where(ok[..., None], F32([12.5, -7.25]), flo)               # the planted NaN / Inf / 1e10 stay
    want = ref_augment_sparse(ims, const, mask, ip, fp, hw)
    t_ims, t_flo, t_mask, params, _ = torch_case((ims, const, mask, ip, fp, hw))
    got = augment.preprocess_sparse(t_ims, t_flo, t_mask, "channels_last", out_shape=hw, params=params)
    for out in (want[1], got[1].numpy().astype(np.float64)):
        for b in range(len(ims)):
            m = want[2][b] != 0
            err = np.abs(out[b][m] - np.float64(F32([12.5, -7.25])) * fp[b, :2].astype(np.float64)).max()
            assert err <= 1e-5, (b, err)
    assert np.array_equal(got[2].numpy(), want[2])


def test_negative_controls_miss_the_bound():
    """The weighted sum without the division by S misses by 31.5 px (make_case) and 21.9 px (tiny_case), the dense
    bilinear over a zero-filled flow by the same amounts: 3e5 and 2e5 times the bound."""
    for name in ("make", "tiny"):
        ims, flo, mask, ip, fp, hw = sparse_case(name)
        want = reference(name)
        m = want[2] != 0
        for control in ("no_division", "dense_over_zero_fill"):
            wrong = ref_augment_sparse(ims, flo, mask, ip, fp, hw, **{control: True})
            assert np.array_equal(wrong[2], want[2])
            miss = np.abs(wrong[1] - want[1])[m].max()
            print("sparse augment control {} {}: misses by {:.3e} px = {:.1e} x BOUND".format(name, control, miss,
                                                                                            miss / BOUND))
            assert miss > 1e4 * BOUND
            with pytest.raises(AssertionError):
                check_against(wrong, want, what="control")


def test_inputs_are_checked():
    ims, flo, mask, params, hw = torch_case(sparse_case("tiny"))
    call = lambda **kw: augment.preprocess_sparse(**dict(dict(ims=ims, flo=flo, valid=mask, out_shape=hw, params=params),
                                                         **kw))
    with pytest.raises(TypeError, match="valid"):
        call(valid=mask.numpy())
    with pytest.raises(TypeError, match="valid"):
        call(valid=mask.to(torch.int32))
    with pytest.raises(ValueError, match="valid"):
        call(valid=mask[:, :-1])
    with pytest.raises(ValueError, match="Unsupported data format"):
        call(data_format="channels_middle")
    with pytest.raises(ValueError, match="dtype"):
        call(flo=flo.double())
    with pytest.raises(ValueError, match="dtype"):
        augment.image_augment_sparse(ims, flo, hw, valid=mask, params=params)       # uint8: float frames only
    with pytest.raises(ValueError, match="dtype"):
        augment.image_resize_sparse(ims, flo, hw, valid=mask)
    with pytest.raises(TypeError, match="torch.Tensor"):
        call(ims=ims.numpy())
    with pytest.raises(ValueError, match="iparams"):
        call(params=as_params(np.zeros((2, 6), np.int32), np.zeros((2, 6), np.float32)))
    with pytest.raises(ValueError, match="does not match"):
        augment.preprocess_no_op_sparse(ims, flo[:, :-1].contiguous(), None, out_shape=hw)

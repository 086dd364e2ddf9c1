"""GPU suite of the training input pipeline (qpwcnet_amd.augment on qpwc_augment_fwd).

Oracle: ``ref_augment``, the float64 restatement in tests/test_augment_cpu.py (checked there against a second
restatement and known answers; the fp32 torch composition meets the same bounds on these exact inputs there).
Bounds: images 1e-4 (the project's kernel bound), flow 1e-4 px with |flow| <= 32 px in the inputs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_augment_cpu import (BOUND, _axis, as_params, identity_case, make_case, max_err, ref_augment,  # noqa: E402
                              smooth_flow, tiny_case)

from qpwcnet_amd import _hip, augment, layers, loss, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(case, data_format="channels_last", colour=True, finish=True):
    ims, flo, ip, fp, hw = case
    p = as_params(ip, fp, DEV)
    return ops.augment(dev(ims), dev(flo), p.iparams, p.fparams, hw, colour=colour, finish=finish,
                       data_format=data_format)


@pytest.fixture(scope="module")
def cases():
    """The inputs and their float64 answers, computed once: {(name, colour): (case, ref_ims, ref_flo)} channels_last."""
    out = {}
    for name, case in (("u8", make_case(np.uint8)), ("f32", make_case(np.float32)), ("tiny", tiny_case())):
        assert np.abs(case[1]).max() <= 32.0
        for colour in (True, False):
            out[name, colour] = (case,) + ref_augment(*case, colour=colour)
    return out


def _errors(got, ref_ims, ref_flo, data_format):
    """max |hip - ref| over EVERY element of both outputs."""
    g_ims, g_flo = (t.cpu().numpy() for t in got)
    if data_format == "channels_first":
        ref_ims, ref_flo = ref_ims.transpose(0, 3, 1, 2), ref_flo.transpose(0, 3, 1, 2)
    assert g_ims.shape == ref_ims.shape and g_flo.shape == ref_flo.shape and g_ims.dtype == np.float32
    assert np.isfinite(g_ims).all() and np.isfinite(g_flo).all()
    return max_err(g_ims, ref_ims), max_err(g_flo, ref_flo)


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("name", ["u8", "f32", "tiny"])
def test_kernels_match_the_float64_restatement(cases, name, data_format, colour):
    case, ref_ims, ref_flo = cases[name, colour]
    B, (h, w) = case[0].shape[0], case[4]
    form = "augment_pixel_kernel<scalar>" if name == "tiny" else "augment_pixel_kernel<vec4>"
    got = _run(case, data_format, colour)
    assert ops.augment_kernel(B, h, w, got[0], got[1]) == form          # both launch forms are reached
    e_ims, e_flo = _errors(got, ref_ims, ref_flo, data_format)
    print("augment {} {} colour={}: max |ims err| {:.3e}, max |flow err| {:.3e} px".format(name, data_format, colour,
                                                                                          e_ims, e_flo))
    assert e_ims <= BOUND and e_flo <= BOUND


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
def test_entry_points_match_the_restatement(cases, data_format):
    case, ref_ims, ref_flo = cases["u8", True]
    ims, flo, ip, fp, hw = case
    got = augment.preprocess(dev(ims), dev(flo), data_format, out_shape=hw, params=as_params(ip, fp))   # CPU params
    assert max(_errors(got, ref_ims, ref_flo, data_format)) <= BOUND
    B, H, W, _ = ims.shape
    for shape in (hw, (33, 47)):
        rp = augment.resize_params(B, (H, W), shape)
        want = ref_augment(ims, flo, rp.iparams.numpy(), rp.fparams.numpy(), shape, colour=False)
        got = augment.preprocess_no_op(dev(ims), dev(flo), data_format, out_shape=shape)
        assert max(_errors(got, want[0], want[1], data_format)) <= BOUND
    case, _, _ = cases["f32", True]
    ims, flo, ip, fp, hw = case
    want = ref_augment(ims, flo, ip, fp, hw, finish=False)
    got = augment.image_augment(dev(ims), dev(flo), hw, params=as_params(ip, fp, DEV))
    assert max(_errors(got, want[0], want[1], "channels_last")) <= BOUND
    rp = augment.resize_params(B, (H, W), (20, 31))
    want = ref_augment(ims, flo, rp.iparams.numpy(), rp.fparams.numpy(), (20, 31), colour=False, finish=False)
    got = augment.image_resize(dev(ims), dev(flo), (20, 31))
    assert max(_errors(got, want[0], want[1], "channels_last")) <= BOUND


def test_negative_controls(cases):
    """The comparison tells the right semantics from the two nearest wrong ones."""
    case, _, _ = cases["u8", True]
    got = _run(case)
    wrong = ref_augment(*case, per_frame_means=True)
    e_ims, e_flo = _errors(got, wrong[0], wrong[1], "channels_last")
    assert e_ims > 10 * BOUND and e_flo <= BOUND
    wrong = ref_augment(*case, flow_by_shape_ratio=True)
    e_ims, e_flo = _errors(got, wrong[0], wrong[1], "channels_last")
    assert e_ims <= BOUND and e_flo > 10 * BOUND


def test_identity_and_flips_are_exact():
    ims, flo, ip, fp, hw, want_ims, want_flo = identity_case()
    got = _run((ims, flo, ip, fp, hw), colour=False)
    assert np.array_equal(got[0].cpu().numpy(), want_ims) and np.array_equal(got[1].cpu().numpy(), want_flo)
    got = _run((ims.astype(np.float32), flo, ip, fp, hw), colour=False, finish=False)      # fp32 frames: as they are
    plain = ims.astype(np.float32)
    for b in range(4):
        ud, lr = int(ip[b, 4]), int(ip[b, 5])
        plain[b] = plain[b, ::-1] if ud else plain[b]
        plain[b] = plain[b, :, ::-1] if lr else plain[b]
    assert np.array_equal(got[0].cpu().numpy(), plain) and np.array_equal(got[1].cpu().numpy(), want_flo)


@pytest.mark.parametrize("name", ["u8", "tiny"])
def test_layouts_forms_and_repeats_agree_bit_for_bit(cases, name):
    case = cases[name, True][0]
    for colour in (True, False):
        last, first = _run(case, "channels_last", colour), _run(case, "channels_first", colour)
        assert torch.equal(first[0].permute(0, 2, 3, 1), last[0]) and torch.equal(first[1].permute(0, 2, 3, 1), last[1])
        again = _run(case, "channels_last", colour)
        assert torch.equal(again[0], last[0]) and torch.equal(again[1], last[1])      # the fixed-order contrast sums


@pytest.mark.parametrize("layout", [_hip.NHWC, _hip.NCHW], ids=["nhwc", "nchw"])
def test_scalar_form_equals_vec4_form(cases, layout):
    """The same batch through the 4-byte-store form (outputs 4 bytes off the 16-byte grid) gives the same bits."""
    ims, flo, ip, fp, (h, w) = cases["u8", True][0]
    B, H, W, _ = ims.shape
    d_ims, d_flo, p = dev(ims), dev(flo), as_params(ip, fp, DEV)
    L = _hip.lib()
    ws = torch.empty(int(L.qpwc_augment_workspace_floats(B, h, w)), dtype=torch.float32, device=DEV)
    outs = {}
    for off, form in ((0, "augment_pixel_kernel<vec4>"), (1, "augment_pixel_kernel<scalar>")):
        o_ims = torch.zeros(B * h * w * 6 + 4, dtype=torch.float32, device=DEV)[off:off + B * h * w * 6]
        o_flo = torch.zeros(B * h * w * 2 + 4, dtype=torch.float32, device=DEV)[off:off + B * h * w * 2]
        assert L.qpwc_augment_fwd_kernel(B, h, w, o_ims.data_ptr(), o_flo.data_ptr()).decode() == form
        rc = L.qpwc_augment_fwd(d_ims.data_ptr(), _hip.U8, d_flo.data_ptr(), B, H, W, p.iparams.data_ptr(),
                                p.fparams.data_ptr(), h, w, _hip.AUGMENT_COLOR, layout, o_ims.data_ptr(),
                                o_flo.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _hip.check(rc)
        outs[off] = (o_ims.clone(), o_flo.clone())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want = ops.augment(d_ims, d_flo, p.iparams, p.fparams, (h, w),
                       data_format="channels_last" if layout == _hip.NHWC else "channels_first")
    assert torch.equal(outs[0][0], want[0].reshape(-1)) and torch.equal(outs[0][1], want[1].reshape(-1))


def test_nan_scrub():
    """preprocess_no_op 8 x 8 -> 16 x 16: source coordinates i / 2 - 1 / 4, exact in fp32 and 1 / 4 away from every
    integer.  One NaN in the flow at (3, 4), one in channel 2 of the image at (5, 1)."""
    rng = np.random.default_rng(9)
    ims = rng.random((1, 8, 8, 6), dtype=np.float32) * 0.4 + 0.05          # never 0.5: no clean output is exactly 0
    flo = smooth_flow(1, 8, 8) + 40.0                                       # nor any clean flow
    lo, hi, t = _axis(np.arange(16), 8, 16)
    assert (np.minimum(t, 1 - t) > 1e-3).all()
    bad_ims, bad_flo = ims.copy(), flo.copy()
    bad_flo[0, 3, 4, 0] = np.nan
    bad_ims[0, 5, 1, 2] = np.nan
    clean = augment.preprocess_no_op(dev(ims), dev(flo), "channels_last", out_shape=(16, 16))
    got = augment.preprocess_no_op(dev(bad_ims), dev(bad_flo), "channels_last", out_shape=(16, 16))
    assert bool((clean[0] != 0).all()) and bool((clean[1] != 0).all())
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    foot = lambda y, x: ((lo == y) | (hi == y))[:, None] & ((lo == x) | (hi == x))[None, :]
    hit_flo = np.zeros((1, 16, 16, 2), bool)
    hit_flo[0, ..., 0] = foot(3, 4)
    hit_ims = np.zeros((1, 16, 16, 6), bool)
    hit_ims[0, ..., 2] = foot(5, 1)
    assert hit_flo.sum() == 16 and hit_ims.sum() == 16                      # an interior source pixel is a neighbour of 4 x 4 outputs
    for g, c, hit in ((got[0], clean[0], hit_ims), (got[1], clean[1], hit_flo)):
        g, c = g.cpu().numpy(), c.cpu().numpy()
        assert np.array_equal(g == 0, hit)
        assert np.array_equal(g[~hit], c[~hit])


def test_sampler_on_the_device():
    ims, flo, _, _, _ = make_case(np.uint8)
    ims, flo = np.repeat(ims, 2, 0), np.repeat(flo, 2, 0)
    d_ims, d_flo = dev(ims), dev(flo)
    hw, base = (16, 24), 0.75                                               # 30 * 0.716 = 21, 52 * 0.716 = 37
    g = lambda: torch.Generator(device=DEV).manual_seed(5)
    a = augment.preprocess(d_ims, d_flo, "channels_first", base, hw, generator=g())
    b = augment.preprocess(d_ims, d_flo, "channels_first", base, hw, generator=g())
    p = augment.sample_params(8, (30, 52), hw, base, generator=g(), device=DEV)
    c = augment.preprocess(d_ims, d_flo, "channels_first", base, hw, params=p)
    assert p.iparams.is_cuda and p.fparams.is_cuda
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1])
    assert not torch.equal(a[0][0], a[0][4])                                # the same source, another draw
    want = ref_augment(ims, flo, p.iparams.cpu().numpy(), p.fparams.cpu().numpy(), hw)
    assert max(_errors(a, want[0], want[1], "channels_first")) <= BOUND
    other = augment.preprocess(d_ims, d_flo, "channels_first", base, hw, generator=torch.Generator(device=DEV).manual_seed(6))
    assert not torch.equal(a[0], other[0])


def test_preprocess_feeds_the_trainable_network():
    """uint8 frames -> augment.preprocess -> FlowerModel -> loss.multiscale -> backward: the pieces connect."""
    rng = np.random.default_rng(3)
    ims = dev(rng.integers(0, 256, (2, 80, 150, 6), dtype=np.uint8))
    flo = dev(smooth_flow(2, 80, 150, amp=4.0))
    x, y = augment.preprocess(ims, flo, "channels_last", base_scale=0.9, out_shape=(64, 128),
                              generator=torch.Generator(device=DEV).manual_seed(1))
    assert tuple(x.shape) == (2, 64, 128, 6) and tuple(y.shape) == (2, 64, 128, 2)
    assert float(x.min()) >= -1.5 and float(x.max()) <= 1.5
    torch.manual_seed(0)
    net = layers.FlowerModel(data_format="channels_last").to(DEV).train()
    total = loss.multiscale(loss.FlowMseLossV2(), y, net(x)[:-1])[0]
    total.backward()
    assert bool(torch.isfinite(total))
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n

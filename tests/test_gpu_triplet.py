"""GPU suite of the frame interpolator's input pipeline (qpwcnet_amd.augment on qpwc_augment_triplet_fwd).

Oracle: ``ref_triplet``, the float64 restatement in tests/test_triplet_cpu.py (its Philox holds the known answers
there, and the fp32 torch composition meets the same bound on these exact inputs there).  Bound: 1e-4, the project's
kernel bound; |values| < 3, and the noise adds 0.02 times a few fp32 ulps of a number < 6."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_triplet_cpu import BOUND, CASES, FORMS, INV255, as_tparams, max_err, ref_triplet  # noqa: E402

from qpwcnet_amd import _hip, augment, layers, loss, ops, optim  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(case, data_format="channels_last", finish=True, ip=None, fp=None):
    a, b, c, ip0, fp0, hw = case
    p = as_tparams(ip0 if ip is None else ip, fp0 if fp is None else fp, DEV)
    return ops.augment_triplet(dev(a), dev(b), dev(c), p.iparams, p.fparams, hw, finish=finish, data_format=data_format)


@pytest.mark.parametrize("finish", [True, False], ids=["finish", "raw"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("name", ["u8", "f32", "tiny", "same"])
def test_kernel_matches_the_float64_restatement(name, data_format, finish):
    case, fin, raw = CASES[name]
    B, (h, w) = case[0].shape[0], case[5]
    got = _run(case, data_format, finish)
    assert ops.augment_triplet_kernel(B, h, w, got[0], got[1]) == "triplet_pixel_kernel<{}>".format(FORMS[name])
    for g, r, ch in zip(got, fin if finish else raw, (6, 3)):
        r = r.transpose(0, 3, 1, 2) if data_format == "channels_first" else r
        g = g.cpu().numpy()
        assert g.shape == r.shape and g.dtype == np.float32 and r.shape[1 if data_format == "channels_first" else 3] == ch
        assert np.isfinite(g).all()
        e = max_err(g, r)                                    # over EVERY element
        print("triplet {} {} finish={} ({} channels): max |err| {:.3e}".format(name, data_format, finish, ch, e))
        assert e <= BOUND


def test_negative_control():
    """The comparison tells the noise that flips with the image from the noise indexed by the output pixel."""
    case, _, _ = CASES["u8"]
    wrong = ref_triplet(*case, noise_before_flips=False)
    got = _run(case)
    assert max_err(got[0][0].cpu().numpy(), wrong[0][0]) <= BOUND          # sample 0: no flip
    assert max_err(got[0][3].cpu().numpy(), wrong[0][3]) > 100 * BOUND


def test_identity_and_flips_are_exact():
    a, b, c, _, _, hw = CASES["same"][0]
    B = a.shape[0]
    idp = augment.identity_triplet_params(B)
    plain = lambda v: v.astype(np.float32) * INV255 - np.float32(0.5)
    want_pair, want_mid = np.concatenate([plain(a), plain(c)], -1), plain(b)
    pair, mid = augment.preprocess_triplet(dev(a), dev(b), dev(c), hw, "channels_last", augment=False)
    assert np.array_equal(pair.cpu().numpy(), want_pair) and np.array_equal(mid.cpu().numpy(), want_mid)
    ip = idp.iparams.numpy().copy()
    ip[:, 0], ip[:, 1] = (np.arange(B) >> 1) & 1, np.arange(B) & 1          # one sample per flip combination
    pair, mid = _run(CASES["same"][0], ip=ip, fp=idp.fparams.numpy())
    for n in range(B):
        axes = tuple(ax for ax, f in ((0, ip[n, 0]), (1, ip[n, 1])) if f)
        assert np.array_equal(pair[n].cpu().numpy(), np.flip(want_pair[n], axes) if axes else want_pair[n]), n
        assert np.array_equal(mid[n].cpu().numpy(), np.flip(want_mid[n], axes) if axes else want_mid[n]), n
    # fp32 frames are taken as they are (RAW: no offset either)
    f = a.astype(np.float32) * np.float32(1.7) - np.float32(20.0)
    pair, mid = ops.augment_triplet(dev(f), dev(f), dev(f), idp.iparams.to(DEV), idp.fparams.to(DEV), hw, finish=False)
    assert np.array_equal(mid.cpu().numpy(), f) and np.array_equal(pair.cpu().numpy(), np.concatenate([f, f], -1))


@pytest.mark.parametrize("name", ["u8", "tiny"])
def test_one_draw_serves_the_three_frames(name):
    a, _, _, ip, fp, hw = CASES[name][0]
    pair, mid = _run((a, a, a, ip, fp, hw))
    assert torch.equal(pair[..., 0:3], mid) and torch.equal(pair[..., 3:6], mid)
    assert float(mid.std()) > 0.1


@pytest.mark.parametrize("name", ["u8", "tiny"])
def test_layouts_and_repeats_agree_bit_for_bit(name):
    case = CASES[name][0]
    for finish in (True, False):
        last, first = _run(case, "channels_last", finish), _run(case, "channels_first", finish)
        assert torch.equal(first[0].permute(0, 2, 3, 1), last[0]) and torch.equal(first[1].permute(0, 2, 3, 1), last[1])
        again = _run(case, "channels_last", finish)
        assert torch.equal(again[0], last[0]) and torch.equal(again[1], last[1])


@pytest.mark.parametrize("layout", [_hip.NHWC, _hip.NCHW], ids=["nhwc", "nchw"])
def test_scalar_form_equals_vec4_form(layout):
    """The same batch through the 4-byte-store form (outputs 4 bytes off the 16-byte grid) gives the same bits."""
    a, b, c, ip, fp, (h, w) = CASES["u8"][0]
    B, H, W, _ = a.shape
    d_a, d_b, d_c, p = dev(a), dev(b), dev(c), as_tparams(ip, fp, DEV)
    L = _hip.lib()
    outs = {}
    for off, form in ((0, "triplet_pixel_kernel<vec4>"), (1, "triplet_pixel_kernel<scalar>")):
        o_pair = torch.zeros(B * h * w * 6 + 4, dtype=torch.float32, device=DEV)[off:off + B * h * w * 6]
        o_mid = torch.zeros(B * h * w * 3 + 4, dtype=torch.float32, device=DEV)[off:off + B * h * w * 3]
        assert L.qpwc_augment_triplet_fwd_kernel(B, h, w, o_pair.data_ptr(), o_mid.data_ptr()).decode() == form
        rc = L.qpwc_augment_triplet_fwd(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), _hip.U8, B, H, W,
                                        p.iparams.data_ptr(), p.fparams.data_ptr(), h, w, 0, layout, o_pair.data_ptr(),
                                        o_mid.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _hip.check(rc)
        outs[off] = (o_pair.clone(), o_mid.clone())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want = ops.augment_triplet(d_a, d_b, d_c, p.iparams, p.fparams, (h, w),
                               data_format="channels_last" if layout == _hip.NHWC else "channels_first")
    assert torch.equal(outs[0][0], want[0].reshape(-1)) and torch.equal(outs[0][1], want[1].reshape(-1))


def test_noise_on_the_device():
    a, b, c, ip, _, hw = CASES["u8"][0]
    B = a.shape[0]
    fp = augment.identity_triplet_params(B).fparams.numpy().copy()
    noflip = ip.copy()
    noflip[:, 0:2] = 0
    quiet = _run(CASES["u8"][0], ip=noflip, fp=fp)
    fp[:, 15] = 0.02
    loud = _run(CASES["u8"][0], ip=noflip, fp=fp)
    z = augment.triplet_noise(torch.from_numpy(ip[:, 2:4]), *hw).numpy()
    want = np.float32(0.02) * z
    for k, (lo, q) in enumerate(zip(loud, quiet)):
        d = (lo - q).cpu().numpy()
        for f in range(d.shape[-1] // 3):                                   # the same field in every frame
            e = float(np.abs(d[..., 3 * f:3 * f + 3] - want).max())
            print("device noise, output {} frame {}: max |sigma z - (loud - quiet)| {:.3e}".format(k, f, e))
            assert e <= 1e-6
    # the device's own words: augment.triplet_noise run there gives the field the CPU gives, to fp32 rounding of log/cos
    z_dev = augment.triplet_noise(dev(ip[:, 2:4]), *hw)
    assert z_dev.is_cuda and float((z_dev.cpu() - torch.from_numpy(z)).abs().max()) <= 1e-5
    # different keys differ
    other = noflip.copy()
    other[:, 2] += 1
    assert not torch.equal(_run(CASES["u8"][0], ip=other, fp=fp)[1], loud[1])
    same = noflip.copy()
    same[:, 2:4] = noflip[0, 2:4]
    one = _run(CASES["u8"][0], ip=same, fp=fp)[1] - _run(CASES["u8"][0], ip=same, fp=fp * (np.arange(16) != 15))[1]
    assert float((one[0] - one[1]).abs().max()) <= 1e-6 and float(one[0].abs().max()) > 0.02
    # the noise flips with the image: with the flips on, the difference is the flipped field
    flipped = _run(CASES["u8"][0], ip=ip, fp=fp)[1] - _run(CASES["u8"][0], ip=ip, fp=fp * (np.arange(16) != 15))[1]
    for n in range(B):
        axes = tuple(ax for ax, f in ((0, ip[n, 0]), (1, ip[n, 1])) if f)
        w_n = np.flip(want[n], axes) if axes else want[n]
        assert float(np.abs(flipped[n].cpu().numpy() - w_n).max()) <= 1e-6, n
        if axes:
            assert float(np.abs(flipped[n].cpu().numpy() - want[n]).max()) > 1e-2, n


def test_sampler_on_the_device():
    a, b, c, _, _, hw = CASES["u8"][0]
    d = [dev(np.repeat(v, 2, 0)) for v in (a, b, c)]
    g = lambda seed=5: torch.Generator(device=DEV).manual_seed(seed)
    one = augment.preprocess_triplet(*d, hw, "channels_first", generator=g())
    two = augment.preprocess_triplet(*d, hw, "channels_first", generator=g())
    p = augment.sample_triplet_params(8, generator=g(), device=DEV)
    three = augment.preprocess_triplet(*d, hw, "channels_first", params=p)
    assert p.iparams.is_cuda and p.fparams.is_cuda                          # drawn and read on the device: no host copy
    for x in (two, three):
        assert torch.equal(one[0], x[0]) and torch.equal(one[1], x[1])
    assert not torch.equal(one[0][0], one[0][4])                            # the same source, another draw
    want = ref_triplet(*(v.cpu().numpy() for v in d), p.iparams.cpu().numpy(), p.fparams.cpu().numpy(), hw)
    assert max_err(one[0].cpu().numpy(), want[0].transpose(0, 3, 1, 2)) <= BOUND
    assert max_err(one[1].cpu().numpy(), want[1].transpose(0, 3, 1, 2)) <= BOUND
    assert not torch.equal(one[0], augment.preprocess_triplet(*d, hw, "channels_first", generator=g(6))[0])
    i0, i1, i2 = augment.augment_triplet(*d, hw, params=p)
    raw = ref_triplet(*(v.cpu().numpy() for v in d), p.iparams.cpu().numpy(), p.fparams.cpu().numpy(), hw, finish=False)
    assert max_err(i0.cpu().numpy(), raw[0][..., 0:3]) <= BOUND and max_err(i2.cpu().numpy(), raw[0][..., 3:6]) <= BOUND
    assert max_err(i1.cpu().numpy(), raw[1]) <= BOUND


def test_preprocess_triplet_feeds_one_training_step():
    """uint8 triplets -> augment.preprocess_triplet -> InterpolatorModel -> loss.multiscale(AutoResizeMseLoss()) ->
    optim.KerasAdamAGC.step(), at the smallest input the default InterpolatorModel takes (five halvings, and the
    coarsest warp needs 2 x 2): 64 x 64.  Frames with structure at every scale (synth.make_frames) and the synthetic
    weights of tests/test_gpu_interp_grad.py: white-noise frames pool to a constant at the coarsest level, where no
    gradient worth an Adam step reaches the flow estimator."""
    from qpwcnet_amd import synth
    pairs, _ = synth.make_frames(2, 70, 90, seed=5)
    u8 = lambda x: dev(np.clip(np.rint((x + 0.5) * 255.0), 0, 255).astype(np.uint8))
    a, b, c = u8(pairs[..., 0:3]), u8(0.5 * (pairs[..., 0:3] + pairs[..., 3:6])), u8(pairs[..., 3:6])
    pair, mid = augment.preprocess_triplet(a, b, c, (64, 64), "channels_last",
                                           generator=torch.Generator(device=DEV).manual_seed(1))
    assert tuple(pair.shape) == (2, 64, 64, 6) and tuple(mid.shape) == (2, 64, 64, 3)
    assert float(pair.min()) >= -3.0 and float(pair.max()) <= 3.0
    net = layers.InterpolatorModel(data_format="channels_last")
    net.load_state_dict({k: torch.as_tensor(v) for k, v in synth.make_interpolator_weights(42, (64, 64)).items()})
    net = net.to(DEV).train()
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    total = loss.multiscale(loss.AutoResizeMseLoss(), mid, net(pair))[0]
    total.backward()
    assert bool(torch.isfinite(total))
    optim.KerasAdamAGC(net).step()
    still = [n for n, p in net.named_parameters() if not bool(torch.isfinite(p).all()) or torch.equal(p.detach(), before[n])]
    assert not still, still

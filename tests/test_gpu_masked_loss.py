"""GPU suite of the valid-masked flow losses (qpwcnet_amd.loss.multiscale_masked / masked_ground_truth on
qpwc_masked_loss_fwd / qpwc_masked_loss_bwd).

Oracle: ``loss.multiscale_masked_torch`` / ``masked_ground_truth_torch`` on float64 CPU tensors, fed the same values
(fp16 predictions: the fp16 values themselves); tests/test_masked_loss_cpu.py holds that chain to a numpy restatement
within 1e-12.  Bounds, those of tests/test_gpu_loss.py: losses 1e-5 relative; fp32 gradients 1e-5 of the level's largest
gradient; fp16 gradients F16_EPS |g| + 1e-5 max + 2^-24; ground truth 1e-6 of the level's largest value; masks and counts
exact; gradients at invalid level pixels exactly 0.
Measured on an MI355X, the worst case of the module as a share of its bound: losses 0.015, fp32 gradients 0.038, fp16
gradients 0.97 (the half ulp of fp16 itself), ground truth 0.16; all valid against loss.multiscale: losses 6e-8 relative,
gradients 2.2e-7 of the level's largest (bound 2e-5).  test_zz_report_the_observed_errors prints them (pytest -s).
B = 2 and factors 2 / 4 / 8 throughout: the scalar backward, sum plans with unequal steps and the pixel walks' further trips
run in tests/test_gpu_eval_scale.py, a mask past 2^31 bytes in tests/test_gpu_large_offsets.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_masked_loss_cpu import (CASES, CODES, KINDS, PARAMS, PIXEL_LOOP, TILE_LOOP, make_case, make_loss,  # noqa: E402
                                  to_layout)

from oracle import torch_ref  # noqa: E402
from qpwcnet_amd import layers, loss, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16_EPS = 2.0 ** -11
WORST = {}          # the largest observed error per quantity, in units of its bound (printed by the last test)


def _note(key, value, bound):
    WORST[key] = max(WORST.get(key, 0.0), float(value) / bound)


def _oracle(obj, gt, preds, valid, scale):
    """float64 chain on the CPU: (per-level losses, counts, d (scale * sum) / d preds, ground truths, masks)."""
    xs = [p.detach().double().cpu().requires_grad_() for p in preds]
    v = None if valid is None else valid.cpu()
    _, per, counts = loss.multiscale_masked_torch(obj, gt.double().cpu(), xs, v)
    (scale * per).sum().backward()
    shapes = [tuple(x.shape[1:3]) if obj.axis == 3 else tuple(x.shape[2:4]) for x in xs]
    gts, masks = loss.masked_ground_truth_torch(obj, gt.double().cpu(), shapes, v)
    return per.detach(), counts, [x.grad for x in xs], gts, masks


def _expand(m, like, axis):
    return (m != 0).unsqueeze(axis).expand_as(like)


def _compare(obj, gt, preds, valid, dtype, tag):
    """One forward + backward + ground-truth pass on the device against the oracle, every bound of the module."""
    scale = 1.0 if dtype == torch.float32 else 2.0 ** 16        # loss scaling keeps the fp16 gradients normal
    ref_per, ref_counts, ref_g, ref_gt, ref_m = _oracle(obj, gt, preds, valid, scale)
    xs = [p.to(DEV).requires_grad_() for p in preds]
    v = None if valid is None else valid.to(DEV)
    total, per, counts = loss.multiscale_masked(obj, gt.to(DEV), xs, v)
    assert per.dtype == torch.float32 and counts.dtype == torch.int64 and counts.device == per.device
    (scale * per).sum().backward()
    shapes = [tuple(m.shape[1:]) for m in ref_m]
    gts, masks = loss.masked_ground_truth(obj, gt.to(DEV), shapes, v)
    assert torch.equal(counts.cpu(), ref_counts), (tag, counts.tolist(), ref_counts.tolist())
    for l, x in enumerate(xs):
        rv = float(ref_per[l])
        assert abs(float(per[l].detach()) - rv) <= 1e-5 * abs(rv), (tag, l, float(per[l].detach()), rv)
        _note("loss", abs(float(per[l].detach()) - rv), 1e-5 * max(abs(rv), 1e-30))
        assert masks[l].dtype == torch.uint8 and torch.equal(masks[l].cpu(), ref_m[l]), (tag, l)
        g, rg = gts[l].double().cpu(), ref_gt[l]
        assert g.shape == rg.shape and gts[l].is_contiguous()
        top = float(rg.abs().max())
        assert float((g - rg).abs().max()) <= 1e-6 * top, (tag, l, float((g - rg).abs().max()), top)
        _note("gt", (g - rg).abs().max(), 1e-6 * max(top, 1e-30))
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        got, want = x.grad.double().cpu(), ref_g[l]
        assert not got[~_expand(ref_m[l], got, obj.axis)].any(), (tag, l)          # exactly 0 where invalid
        d, m = (got - want).abs(), float(want.abs().max())
        if dtype == torch.float32:
            assert float(d.max()) <= 1e-5 * m, (tag, l, float(d.max()), m)
            _note("grad_f32", d.max(), 1e-5 * max(m, 1e-30))
        else:
            bound = F16_EPS * want.abs() + 1e-5 * m + 2.0 ** -24
            assert bool((d <= bound).all()), (tag, l, float((d - bound).max()))
            _note("grad_f16", (d / bound).max(), 1.0)
    assert abs(float(total.detach()) - float(per.detach().sum())) <= 1e-6 * abs(float(per.detach().sum())) + 1e-30
    return per.detach(), counts, [x.grad for x in xs]


@pytest.fixture(scope="module")
def cases():
    """Every case of the CPU suite, made once."""
    return {(name, kind): make_case(name, kind) for name, kind in PARAMS}


def _tensors(case, data_format, dtype):
    gt = to_layout(case["gt"], data_format, torch.float32)
    preds = [to_layout(p, data_format, dtype) for p in case["preds"]]
    valid = None if case["valid"] is None else torch.from_numpy(case["valid"])
    return gt, preds, valid


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("name,kind", PARAMS)
def test_kernels_match_the_float64_chain(cases, name, kind, data_format, dtype):
    case = cases[(name, kind)]
    obj = make_loss(kind, data_format)
    gt, preds, valid = _tensors(case, data_format, dtype)
    per, counts, grads = _compare(obj, gt, preds, valid, dtype, (name, kind, data_format))
    (B, H, W, shapes), _, how = CASES[name]
    want = "masked_loss_tile_kernel" if kind == "v2" and name not in ("three_mask30", "three_all_valid",
                                                                      "narrow_mask30") else "masked_loss_pixel_kernel"
    assert ops.masked_loss_kernel(CODES[kind], B, H, W, shapes) == want
    if how == "none":
        assert not per.any() and not counts.any() and all(not g.any() for g in grads)
    if how == "garbage":
        clean = to_layout(case["clean"], data_format, torch.float32)
        again = loss.multiscale_masked(obj, clean.to(DEV), [p.to(DEV) for p in preds], valid.to(DEV))
        assert torch.equal(again[1], per) and torch.equal(again[2], counts)      # what lies under the mask: no bit


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("kind", KINDS)
def test_nan_prediction_at_an_invalid_level_pixel(cases, kind, data_format):
    """NaN and Inf predictions where the level has no ground truth: the loss and every other gradient stay within the
    bounds, the gradient there is exactly 0."""
    case = cases[("empty_blocks", kind)]
    obj = make_loss(kind, data_format)
    gt, preds, valid = _tensors(case, data_format, torch.float32)
    shapes = [tuple(p.shape[1:3]) for p in case["preds"]]
    _, masks = loss.masked_ground_truth_torch(obj, gt.double(), shapes, valid)
    poisoned = []
    for p, m in zip(preds, masks):
        bad = ~_expand(m, p, obj.axis)
        assert bool(bad.any())
        q = p.clone()
        q[bad] = float("nan")
        q.view(-1)[bad.reshape(-1).nonzero()[0]] = float("inf")
        poisoned.append(q)
    per, counts, grads = _compare(obj, gt, poisoned, valid, torch.float32, ("poisoned", kind, data_format))
    assert bool(torch.isfinite(per).all()) and all(bool(torch.isfinite(g).all()) for g in grads)
    clean = loss.multiscale_masked(obj, gt.to(DEV), [p.to(DEV) for p in preds], valid.to(DEV))
    assert torch.equal(clean[1], per)


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("name,kind", [(n, k) for n, k in PARAMS if CASES[n][2] == "all"])
def test_all_valid_is_the_dense_loss(cases, name, kind, data_format):
    """Against the existing loss.multiscale, within 2e-5 relative: each side carries 1e-5 against float64."""
    case = cases[(name, kind)]
    obj = make_loss(kind, data_format)
    gt, preds, _ = _tensors(case, data_format, torch.float32)
    xs = [p.to(DEV).requires_grad_() for p in preds]
    ys = [p.to(DEV).requires_grad_() for p in preds]
    _, per, counts = loss.multiscale_masked(obj, gt.to(DEV), xs)
    _, dense = loss.multiscale(obj, gt.to(DEV), ys)
    per.sum().backward()
    dense.sum().backward()
    assert counts.tolist() == [p[..., 0].size for p in case["preds"]]
    for l, (x, y) in enumerate(zip(xs, ys)):
        a, b = float(per[l].detach()), float(dense[l].detach())
        assert abs(a - b) <= 2e-5 * abs(b), (l, a, b)
        _note("all_valid_loss_vs_dense", abs(a - b), 2e-5 * abs(b))
        m = float(y.grad.abs().max())
        assert float((x.grad - y.grad).abs().max()) <= 2e-5 * m, (l, float((x.grad - y.grad).abs().max()), m)
        _note("all_valid_grad_vs_dense", (x.grad - y.grad).abs().max(), 2e-5 * m)


def test_a_level_without_a_valid_pixel_beside_levels_with_some():
    """One valid ground-truth pixel: the bilinear corners of the coarse levels miss it (count 0: loss 0, gradient 0, all
    finite) while the finest level has it; nothing is read back to get there."""
    obj = loss.FlowMseLoss("channels_last")
    B, H, W, shapes = 2, 32, 64, [(16, 32), (8, 16), (4, 8)]
    gt = torch.full((B, H, W, 2), float("nan"))
    gt[1, 4, 6] = torch.tensor([3.0, -4.0])                  # a corner of level-0 pixel (2, 3) and of no coarser pixel
    xs = [torch.randn(B, h, w, 2, generator=torch.Generator().manual_seed(h)).to(DEV).requires_grad_() for h, w in shapes]
    total, per, counts = loss.multiscale_masked(obj, gt.to(DEV), xs)
    total.backward()
    assert counts.tolist()[1:] == [0, 0] and counts.tolist()[0] >= 1
    assert per.tolist()[1:] == [0.0, 0.0] and float(per[0].detach()) > 0.0 and bool(torch.isfinite(per).all())
    assert not xs[1].grad.any() and not xs[2].grad.any()
    assert int((xs[0].grad != 0).any(dim=-1).sum()) == int(counts[0]) and bool(torch.isfinite(xs[0].grad).all())
    _compare(obj, gt, [x.detach().cpu() for x in xs], None, torch.float32, "one_pixel")


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
def test_tile_loop_iterates(data_format):
    """More 32 x 32 tiles than the tile kernel has workgroups (tests/test_masked_loss_cpu.py holds the relation)."""
    B, H, W, shapes = TILE_LOOP
    assert ops.masked_loss_kernel(CODES["v2"], B, H, W, shapes) == "masked_loss_tile_kernel"
    gen = torch.Generator().manual_seed(11)
    gt = torch.randn(B, H, W, 2, generator=gen) * 4.0
    valid = (torch.rand(B, H // 16, W // 16, generator=gen) < 0.6).repeat_interleave(16, 1).repeat_interleave(16, 2)
    valid &= torch.rand(B, H, W, generator=gen) < 0.5
    gt[torch.rand(B, H, W, generator=gen) < 0.05] = float("nan")
    preds = [torch.randn(B, h, w, 2, generator=gen) for h, w in shapes]
    tr = (lambda t: t.permute(0, 3, 1, 2).contiguous()) if data_format == "channels_first" else (lambda t: t)
    _, counts, _ = _compare(make_loss("v2", data_format), tr(gt), [tr(p) for p in preds], valid, torch.float32,
                            ("tile_loop", data_format))
    assert all(0 < c < B * h * w for c, (h, w) in zip(counts.tolist(), shapes))


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
def test_pixel_loop_iterates(data_format):
    """More level pixels than the pixel kernel's grid covers in one trip."""
    B, H, W, shapes = PIXEL_LOOP
    assert ops.masked_loss_kernel(CODES["finetune"], B, H, W, shapes) == "masked_loss_pixel_kernel"
    gen = torch.Generator().manual_seed(12)
    # a small flow: the level is 9 times larger than the ground truth and h / H scales the values with it; at 0.1 px they
    # stay near 1, where the fp32 rounding of the residual (an ulp of the value over a residual >= 0.25) is far below 1e-5
    gt = torch.randn(B, H, W, 2, generator=gen) * 0.1
    valid = torch.rand(B, H // 4, W // 4, generator=gen) < 0.5
    valid = valid.repeat_interleave(4, 1).repeat_interleave(4, 2)
    # 0.25..0.75 off the level's ground truth in every channel: no residual near 0, where sign() would amplify a rounding
    base = loss.masked_ground_truth_torch(make_loss("finetune", "channels_last"), gt.double(), shapes, valid)[0]
    preds = [(g + torch.where(torch.rand(g.shape, generator=gen) < 0.5, -1.0, 1.0)
              * (0.25 + 0.5 * torch.rand(g.shape, generator=gen))).float() for g in base]
    tr = (lambda t: t.permute(0, 3, 1, 2).contiguous()) if data_format == "channels_first" else (lambda t: t)
    _, counts, _ = _compare(make_loss("finetune", data_format), tr(gt), [tr(p) for p in preds], valid, torch.float32,
                            ("pixel_loop", data_format))
    assert 0 < counts.tolist()[0] < B * shapes[0][0] * shapes[0][1]


def test_views_off_the_grid_are_copied():
    """A y_true 8 bytes and a mask 1 byte off the grid the kernels load on (slices of larger tensors): same bits."""
    case = make_case("pyramid_mask30", "v2")
    obj = make_loss("v2", "channels_last")
    gt, preds, valid = _tensors(case, "channels_last", torch.float32)
    xs = [p.to(DEV) for p in preds]
    want = loss.multiscale_masked(obj, gt.to(DEV), xs, valid.to(DEV))
    flat = torch.zeros(gt.numel() + 2, device=DEV)
    flat[2:] = gt.to(DEV).view(-1)
    mflat = torch.zeros(valid.numel() + 1, dtype=torch.uint8, device=DEV)
    mflat[1:] = valid.to(DEV).view(-1)
    off_gt, off_mask = flat[2:].view(gt.shape), mflat[1:].view(valid.shape)
    assert off_gt.data_ptr() % 16 == 8 and off_mask.data_ptr() % 4 == 1
    got = loss.multiscale_masked(obj, off_gt, xs, off_mask)
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("byte", [2, 128, 255])
def test_any_nonzero_mask_byte_is_valid(cases, byte, data_format):
    """include/qpwc_masked_loss.h: a mask byte allows its pixel where it is nonzero.  The tile kernel unpacks the bytes
    out of a 16-bit load (channels-last) or a 32-bit load (channels-first) with shifts and & 0xff, the pixel kernel
    compares the byte: uint8 masks holding 2, 128 or 255 where the case's mask holds 1 give the bits of the mask of
    ones -- losses, counts, gradients, ground truths and level masks (which stay 0 / 1)."""
    for kind in ("v2", "mse"):                                   # the tile kernel, the pixel kernel
        case = cases[("pyramid_mask30", kind)]
        obj = make_loss(kind, data_format)
        gt, preds, valid = _tensors(case, data_format, torch.float32)
        shapes = [tuple(p.shape[1:3]) for p in case["preds"]]
        runs = []
        for mask in (valid.to(DEV), valid.to(DEV).to(torch.uint8) * byte):
            xs = [p.to(DEV).requires_grad_() for p in preds]
            total, per, counts = loss.multiscale_masked(obj, gt.to(DEV), xs, mask)
            total.backward()
            gts, masks = loss.masked_ground_truth(obj, gt.to(DEV), shapes, mask)
            runs.append((per.detach(), counts, [x.grad for x in xs], gts, masks))
        assert int(mask.max()) == byte and 0 < int(runs[0][1].min())
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        for k in (2, 3, 4):
            assert all(torch.equal(a, b) for a, b in zip(runs[0][k], runs[1][k])), (kind, k)
        assert all(int(m.max()) == 1 for m in runs[1][4])


def test_two_runs_and_another_level_order_give_the_same_bits(cases):
    for kind in KINDS:
        case = cases[("pyramid_mask30", kind)]
        obj = make_loss(kind, "channels_last")
        gt, preds, valid = _tensors(case, "channels_last", torch.float32)
        runs = []
        for order in ((0, 1, 2), (0, 1, 2), (2, 0, 1)):
            xs = [preds[i].to(DEV).requires_grad_() for i in order]
            total, per, counts = loss.multiscale_masked(obj, gt.to(DEV), xs, valid.to(DEV))
            total.backward()
            back = [order.index(i) for i in range(3)]
            runs.append((per.detach()[back].clone(), counts[back].clone(), [xs[j].grad.clone() for j in back]))
        for other in runs[1:]:
            assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1])
            assert all(torch.equal(a, b) for a, b in zip(runs[0][2], other[2]))


def test_refusals_on_the_device():
    gt = torch.zeros(2, 32, 64, 2, device=DEV)
    x = [torch.zeros(2, 16, 32, 2, device=DEV)]
    obj = loss.FlowMseLossV2()
    with pytest.raises(ValueError, match="valid is on"):
        loss.multiscale_masked(obj, gt, x, valid=torch.ones(2, 32, 64, dtype=torch.bool))
    with pytest.raises(ValueError, match="float32"):
        loss.multiscale_masked(obj, gt.half(), x)
    with pytest.raises(ValueError, match="y_true requires grad"):
        loss.multiscale_masked(obj, gt.clone().requires_grad_(), x)
    with pytest.raises(ValueError, match="whole-block"):
        loss.multiscale_masked(obj, gt, [torch.zeros(2, 5, 32, 2, device=DEV)])
    with pytest.raises(TypeError):
        loss.multiscale_masked(loss.AutoResizeMseLoss(), gt, x)


class _Tiny(torch.nn.Module):
    """tests/test_gpu_loss.py's model: torch convs around WarpV2 and CostVolumeV2 (search range 2): a 16x16 flow and its
    2x / 4x area means -- three prediction levels against a 32x32 ground truth."""

    def __init__(self, warp_fn, cv_fn):
        super().__init__()
        self.warp_fn, self.cv_fn = warp_fn, cv_fn
        self.enc = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.flo = torch.nn.Conv2d(6, 2, 3, padding=1)
        self.head = torch.nn.Conv2d(25, 2, 3, padding=1)

    def forward(self, a, b):
        fa = self.enc(a).permute(0, 2, 3, 1)
        fb = self.enc(b).permute(0, 2, 3, 1)
        flo = 2.0 * self.flo(torch.cat([a, b], 1)).permute(0, 2, 3, 1)
        out = self.head(self.cv_fn(fa, self.warp_fn(fb, flo)).permute(0, 3, 1, 2))
        pyr = [out, torch.nn.functional.avg_pool2d(out, 2), torch.nn.functional.avg_pool2d(out, 4)]
        return [p.permute(0, 2, 3, 1) for p in pyr]


def test_small_model_trains_on_sparse_ground_truth_like_the_float64_chain():
    torch.manual_seed(1)
    wp, cv = layers.WarpV2(data_format="channels_last"), layers.CostVolumeV2(2, data_format="channels_last")
    m = _Tiny(lambda i, f: wp((i, f)), lambda p, n: cv((p, n))).to(DEV)
    ref = _Tiny(torch_ref.warp_v2, lambda p, n: torch_ref.cost_volume(p, n, 2)).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()})
    gen = torch.Generator().manual_seed(3)
    a, b = torch.randn(2, 3, 16, 16, generator=gen), torch.randn(2, 3, 16, 16, generator=gen)
    gt = 3.0 * torch.randn(2, 32, 32, 2, generator=gen)
    keep = (torch.rand(2, 4, 4, generator=gen) < 0.6).repeat_interleave(8, 1).repeat_interleave(8, 2)
    keep &= torch.rand(2, 32, 32, generator=gen) < 0.5
    assert 0.2 < float(keep.float().mean()) < 0.4
    gt[~keep] = float("nan")                                # 30 %-dense ground truth, NaN elsewhere, no mask
    obj = loss.FlowMseLossV2()
    assert obj.data_format == "channels_last"
    opt = torch.optim.SGD(m.parameters(), lr=5.0)
    opt_ref = torch.optim.SGD(ref.parameters(), lr=5.0)
    ga, gb, gg = a.to(DEV), b.to(DEV), gt.to(DEV)
    mine, theirs = [], []
    for it in range(6):
        opt.zero_grad()
        total, per, counts = loss.multiscale_masked(obj, gg, m(ga, gb))
        total.backward()
        opt.step()
        opt_ref.zero_grad()
        t_ref = loss.multiscale_masked_torch(obj, gt.double(), ref(a.double(), b.double()))[0]
        t_ref.backward()
        opt_ref.step()
        mine.append(float(total.detach()))
        theirs.append(float(t_ref.detach()))
    for x, y in zip(mine, theirs):
        assert abs(x - y) <= 1e-3 * abs(y), (mine, theirs)
    assert mine[-1] < mine[0], mine
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert 0 < min(counts.tolist()) and counts.tolist()[2] < 2 * 4 * 4


def test_zz_report_the_observed_errors():
    """The largest error of the module per quantity, as a share of its bound (pytest -s shows it)."""
    print("\nmasked loss, worst observed / bound: " + ", ".join("{} {:.3f}".format(k, v) for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())

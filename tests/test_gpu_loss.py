"""GPU suite of the training losses (qpwcnet_amd.loss on qpwc_loss_fwd / qpwc_loss_bwd).

Oracle: the float64 restatement of qpwcnet/train/loss.py in tests/test_loss_cpu.py (checked there against a second,
torch-op restatement and by gradcheck), its gradient by torch autograd on the CPU, fed the same values (fp16
predictions: the fp16 values themselves)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_loss_cpu import make_case, ref_loss  # noqa: E402

from oracle import torch_ref  # noqa: E402
from qpwcnet_amd import layers, loss, metrics  # noqa: E402
import qpwcnet_amd as K  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16_EPS = 2.0 ** -11
PYRAMID = (2, 256, 512, [(128, 256), (64, 128), (32, 64), (16, 32), (8, 16)])   # config 2's five levels, B = 2
RAGGED = (2, 96, 160, [(32, 32), (24, 40)])          # area factors 3 x 5 (generic path) and 4 x 4
KINDS = {"v2": loss.FlowMseLossV2, "mse": loss.FlowMseLoss, "finetune": loss.FlowMseLossFineTune,
         "autoresize": loss.AutoResizeMseLoss}


def _make(kind, data_format):
    prev = K.image_data_format()
    K.set_image_data_format(data_format)
    try:
        return KINDS[kind](data_format) if kind in ("mse", "finetune") else KINDS[kind]()
    finally:
        K.set_image_data_format(prev)


def _oracle(kind, gt, preds, data_format, scale):
    """float64 per-level losses and d(scale * loss_l) / d pred_l."""
    vals, grads = [], []
    for p in preds:
        x = p.detach().double().cpu().requires_grad_()
        v = ref_loss(kind, gt.double().cpu(), x, data_format)
        (scale * v).backward()
        vals.append(float(v.detach()))
        grads.append(x.grad)
    return vals, grads


@pytest.mark.parametrize("shapes", [PYRAMID, RAGGED], ids=["pyramid", "ragged"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_losses_and_gradients_match_the_float64_restatement(kind, data_format, dtype, shapes):
    B, H, W, lv = shapes
    gt, preds = make_case(kind, B, H, W, lv, data_format, 1, torch.float32)
    preds = [p.to(dtype) for p in preds]
    scale = 1.0 if dtype == torch.float32 else 2.0 ** 16    # loss scaling keeps the fp16 gradients normal
    ref_v, ref_g = _oracle(kind, gt, preds, data_format, scale)
    obj = _make(kind, data_format)
    xs = [p.to(DEV).requires_grad_() for p in preds]
    total, per = loss.multiscale(obj, gt.to(DEV), xs)
    (scale * per).sum().backward()
    for l, (x, rv, rg) in enumerate(zip(xs, ref_v, ref_g)):
        assert abs(float(per[l].detach()) - rv) <= 1e-5 * abs(rv), (l, float(per[l].detach()), rv)
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        d = (x.grad.double().cpu() - rg).abs()
        m = float(rg.abs().max())
        if dtype == torch.float32:
            assert float(d.max()) <= 1e-5 * m, (l, float(d.max()), m)
        else:
            bound = F16_EPS * rg.abs() + 1e-5 * m + 2.0 ** -24
            assert bool((d <= bound).all()), (l, float((d - bound).max()))
            bad = rg * (1 + 1 / 16)                             # negative control: a 1/16 larger gradient fails it
            bound = F16_EPS * bad.abs() + 1e-5 * m + 2.0 ** -24
            assert not bool(((x.grad.double().cpu() - bad).abs() <= bound).all())
    # one loss object on one level is the same path with L = 1
    single = obj(gt.to(DEV), xs[-1].detach())
    assert single.dim() == 0 and abs(float(single) - ref_v[-1]) <= 1e-5 * abs(ref_v[-1])


@pytest.mark.parametrize("kind", list(KINDS))
def test_multiscale_equals_the_sum_of_the_per_level_calls(kind):
    B, H, W, lv = PYRAMID
    gt, preds = make_case(kind, B, H, W, lv, "channels_last", 2, torch.float32)
    obj = _make(kind, "channels_last")
    g = gt.to(DEV)
    xs = [p.to(DEV) for p in preds]
    total, per = loss.multiscale(obj, g, xs)
    singles = [float(obj(g, x)) for x in xs]
    assert per.shape == (5,) and per.dtype == torch.float32 and total.dim() == 0
    for a, b in zip(per.tolist(), singles):
        assert abs(a - b) <= 1e-6 * abs(b)
    assert abs(float(total) - sum(singles)) <= 1e-6 * abs(sum(singles))


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
def test_flow_mse_is_the_epe_of_the_bilinear_ground_truth_and_area_mode(data_format):
    B, H, W, lv = PYRAMID
    gt, preds = make_case("mse", B, H, W, lv, data_format, 3, torch.float32)
    g, xs = gt.to(DEV), [p.to(DEV) for p in preds]
    _, per = loss.multiscale(loss.FlowMseLoss(data_format), g, xs)
    epe = metrics.per_level_epe(metrics.multiscale_ground_truth(g, lv, data_format), xs, data_format)
    for a, b in zip(per.tolist(), epe.tolist()):
        assert abs(a - b) <= 1e-6 * abs(b), (a, b)
    # the bilinear default is unchanged; 'area' is FlowMseLossV2's ground truth
    area = metrics.multiscale_ground_truth(g, lv, data_format, mode="area")
    nhwc = gt.double().permute(0, 2, 3, 1) if data_format == "channels_first" else gt.double()
    for (h, w), t in zip(lv, area):
        ref = nhwc.reshape(B, h, H // h, w, W // w, 2).mean(dim=(2, 4)) * (h / H)
        if data_format == "channels_first":
            ref = ref.permute(0, 3, 1, 2)
        assert t.shape == ref.shape and t.is_contiguous()
        assert float((t.double().cpu() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    with pytest.raises(ValueError):
        metrics.multiscale_ground_truth(g, [(100, 100)], data_format, mode="area")


def test_two_calls_are_bit_identical():
    B, H, W, lv = PYRAMID
    for kind in ("v2", "finetune"):
        gt, preds = make_case(kind, B, H, W, lv, "channels_last", 4, torch.float32)
        obj = _make(kind, "channels_last")
        runs = []
        for _ in range(2):
            xs = [p.to(DEV).requires_grad_() for p in preds]
            total, per = loss.multiscale(obj, gt.to(DEV), xs)
            total.backward()
            runs.append((per.detach().clone(), [x.grad.clone() for x in xs]))
        assert torch.equal(runs[0][0], runs[1][0])
        assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_huber_both_branches():
    B, H, W = 2, 64, 128
    gen = torch.Generator().manual_seed(5)
    gt = torch.randn(B, H, W, 2, generator=gen, dtype=torch.float64) * 3
    h, w = 16, 32
    s = 2.0 / (w + h)
    base = gt.reshape(B, h, H // h, w, W // w, 2).mean(dim=(2, 4)) * (h / H)
    # residuals e = s * (pred - gt_l): 0.02 (quadratic) or 0.5 (linear) against delta = 0.1, random signs
    mag = torch.where(torch.rand(B, h, w, 2, generator=gen) < 0.5, 0.02, 0.5).double()
    sign = torch.where(torch.rand(B, h, w, 2, generator=gen) < 0.5, -1.0, 1.0).double()
    pred = (base + sign * mag / s).float()
    e = s * pred.double() - s * base
    assert bool((e.abs() < 0.05).any()) and bool((e.abs() > 0.2).any())
    rv, rg = _oracle("v2", gt.float(), [pred], "channels_last", 1.0)
    x = pred.to(DEV).requires_grad_()
    v = loss.FlowMseLossV2()(gt.float().to(DEV), x)
    v.backward()
    assert abs(float(v.detach()) - rv[0]) <= 1e-5 * rv[0]
    assert float((x.grad.double().cpu() - rg[0]).abs().max()) <= 1e-5 * float(rg[0].abs().max())


def test_grad_path_refuses_capture():
    gt = torch.randn(2, 64, 64, 2, device=DEV)
    x = torch.randn(2, 32, 32, 2, device=DEV, requires_grad=True)
    obj = loss.FlowMseLossV2()
    with torch.no_grad():
        obj(gt, x)                                     # warm up outside the capture
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph):
            obj(gt, x)
    torch.cuda.synchronize()


class _Tiny(torch.nn.Module):
    """Torch convs around WarpV2 and CostVolumeV2 (search range 2): a 16x16 flow (B,16,16,2) and its 2x / 4x area means
    -- three prediction levels against a 32x32 ground truth."""

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


def test_small_model_trains_with_multiscale_flow_mse_v2_like_the_float64_oracle():
    torch.manual_seed(1)
    wp, cv = layers.WarpV2(data_format="channels_last"), layers.CostVolumeV2(2, data_format="channels_last")
    m = _Tiny(lambda i, f: wp((i, f)), lambda p, n: cv((p, n))).to(DEV)
    ref = _Tiny(torch_ref.warp_v2, lambda p, n: torch_ref.cost_volume(p, n, 2)).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()})
    gen = torch.Generator().manual_seed(3)
    a, b = torch.randn(2, 3, 16, 16, generator=gen), torch.randn(2, 3, 16, 16, generator=gen)
    gt = 3.0 * torch.randn(2, 32, 32, 2, generator=gen)
    obj = loss.FlowMseLossV2()
    assert obj.data_format == "channels_last"
    opt = torch.optim.SGD(m.parameters(), lr=5.0)
    opt_ref = torch.optim.SGD(ref.parameters(), lr=5.0)
    ga, gb, gg = a.to(DEV), b.to(DEV), gt.to(DEV)
    mine, theirs = [], []
    for it in range(6):
        opt.zero_grad()
        total, per = loss.multiscale(obj, gg, m(ga, gb))
        total.backward()
        opt.step()
        opt_ref.zero_grad()
        t_ref = sum(ref_loss("v2", gt.double(), p) for p in ref(a.double(), b.double()))
        t_ref.backward()
        opt_ref.step()
        mine.append(float(total))
        theirs.append(float(t_ref))
    for x, y in zip(mine, theirs):
        assert abs(x - y) <= 1e-3 * abs(y), (mine, theirs)
    assert mine[-1] < mine[0], mine

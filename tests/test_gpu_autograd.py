"""GPU suite of the backward passes (qpwc_cost_volume_bwd / qpwc_warp_bwd behind torch autograd).

Oracle: torch.autograd of oracle.torch_ref.cost_volume / warp_v2 / tf_warp on the CPU in float64, fed the same values.
Inputs avoid fp32-vs-fp64 kink disagreements: prv / nxt / grad_out are multiples of 1/16 in [-1, 1] (every sum of
products is exact in fp32, so the LeakyReLU sign -- ties at 0 included -- is the same on both sides), flows are
multiples of 2^-6 (exact sample coordinates) with exact-integer and zero flows among them."""
import pytest
import torch

from oracle import torch_ref
from qpwcnet_amd import layers, non_layers, ops, warp as qwarp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEVELS = [(8, 16, 256), (16, 32, 256), (32, 64, 128), (64, 128, 64), (128, 256, 32)]
F16_EPS = 2.0 ** -11


def _grid(gen, shape, step=1 / 16):
    n = int(round(1 / step))
    return torch.randint(-n, n + 1, shape, generator=gen).to(torch.float64) * step


def _flow(gen, B, H, W, reach=6):
    """Multiples of 2^-6 within +-reach pixels; every 5th pixel an exact integer, every 7th zero."""
    f = torch.randint(-reach * 64, reach * 64 + 1, (B, H, W, 2), generator=gen).to(torch.float64) / 64
    flat = f.view(-1, 2)
    flat[::5] = flat[::5].round()
    flat[::7] = 0
    return f


def _tol(ref):
    return 1e-4 * max(1.0, float(ref.abs().max()))


def _check(got, ref, what):
    d = float((got.detach().double().cpu() - ref).abs().max())
    assert d <= _tol(ref), "{}: max|d| = {:.3e} > {:.3e}".format(what, d, _tol(ref))


def _oracle_cv(prv, nxt, g, r):
    a, b = prv.clone().requires_grad_(), nxt.clone().requires_grad_()
    out = torch_ref.cost_volume(a, b, r)
    out.backward(g)
    return out.detach(), a.grad, b.grad


def _oracle_warp(img, flo, g, mode):
    a, f = img.clone().requires_grad_(), flo.clone().requires_grad_()
    out = (torch_ref.warp_v2 if mode == "clamp" else torch_ref.tf_warp)(a, f)
    out.backward(g)
    return out.detach(), a.grad, f.grad


def _cv_case(shape, r, seed):
    gen = torch.Generator().manual_seed(seed)
    B, H, W, C = shape
    d = 2 * r + 1
    return _grid(gen, shape), _grid(gen, shape), _grid(gen, (B, H, W, d * d))


# ---- cost volume -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwc", LEVELS, ids=["L0", "L1", "L2", "L3", "L4"])
def test_cost_volume_grad_level_shapes(hwc):
    prv, nxt, g = _cv_case((2,) + hwc, 4, 0)
    out_ref, gp_ref, gn_ref = _oracle_cv(prv, nxt, g, 4)
    assert (out_ref > 0).any() and (out_ref < 0).any()                # both LeakyReLU branches occur
    a = prv.float().to(DEV).requires_grad_()
    b = nxt.float().to(DEV).requires_grad_()
    out = layers.CostVolumeV2(4, data_format="channels_last")((a, b))
    out.backward(g.float().to(DEV))
    _check(out, out_ref, "out")
    _check(a.grad, gp_ref, "grad_prv")
    _check(b.grad, gn_ref, "grad_nxt")


@pytest.mark.parametrize("C", [1, 3, 17, 32, 64])
@pytest.mark.parametrize("r", [0, 2, 4])
def test_cost_volume_grad_ragged(C, r):
    prv, nxt, g = _cv_case((2, 7, 11, C), r, 10 + C + r)
    out_ref, gp_ref, gn_ref = _oracle_cv(prv, nxt, g, r)
    a = prv.float().to(DEV).requires_grad_()
    b = nxt.float().to(DEV).requires_grad_()
    out = ops.cost_volume(a, b, r)
    out.backward(g.float().to(DEV))
    _check(a.grad, gp_ref, "grad_prv")
    _check(b.grad, gn_ref, "grad_nxt")


@pytest.mark.parametrize("memory", ["dense", "channels_last"])
@pytest.mark.parametrize("C", [3, 32])
def test_cost_volume_grad_channels_first(memory, C):
    prv, nxt, g = _cv_case((2, 9, 12, C), 4, 3)
    _, gp_ref, gn_ref = _oracle_cv(prv, nxt, g, 4)
    mf = torch.channels_last if memory == "channels_last" else torch.contiguous_format
    a = prv.float().permute(0, 3, 1, 2).to(DEV).contiguous(memory_format=mf).requires_grad_()
    b = nxt.float().permute(0, 3, 1, 2).to(DEV).contiguous(memory_format=mf).requires_grad_()
    out = non_layers.CostVolumeV2(4, data_format="channels_first")((a, b))
    out.backward(g.float().permute(0, 3, 1, 2).to(DEV))
    _check(a.grad.permute(0, 2, 3, 1), gp_ref, "grad_prv")
    _check(b.grad.permute(0, 2, 3, 1), gn_ref, "grad_nxt")


def test_cost_volume_only_the_asked_gradient_and_slope_tie():
    prv, nxt, g = _cv_case((1, 6, 6, 4), 2, 5)
    prv[0, 2, 2] = 0                                                    # a pixel whose 25 entries are all exactly 0
    out_ref, gp_ref, gn_ref = _oracle_cv(prv, nxt, g, 2)
    assert (out_ref == 0).any()
    a = prv.float().to(DEV).requires_grad_()
    b = nxt.float().to(DEV)
    ops.cost_volume(a, b, 2).backward(g.float().to(DEV))
    _check(a.grad, gp_ref, "grad_prv")
    assert b.grad is None


def test_cost_volume_fp16_bound_and_negative_control():
    prv, nxt, g = _cv_case((2, 32, 64, 32), 4, 7)                       # 1/16 grid: exact in fp16 too
    _, gp_ref, gn_ref = _oracle_cv(prv, nxt, g, 4)
    a = prv.half().to(DEV).requires_grad_()
    b = nxt.half().to(DEV).requires_grad_()
    ops.cost_volume(a, b, 4).backward(g.half().to(DEV))
    assert a.grad.dtype == torch.float16
    # inputs and grad_out are exact in fp16, sums accumulate in fp32: what remains is the one rounding of the result
    for got, ref in ((a.grad, gp_ref), (b.grad, gn_ref)):
        bound = F16_EPS * ref.abs() + 1e-6 * float(ref.abs().max()) + 2.0 ** -24
        assert bool(((got.double().cpu() - ref).abs() <= bound).all())
    # negative control: the gradient of a 1/16 larger grad_out must violate the same bound
    _, gp_bad, _ = _oracle_cv(prv, nxt, g * (1 + 1 / 16), 4)
    bound = F16_EPS * gp_bad.abs() + 1e-6 * float(gp_bad.abs().max()) + 2.0 ** -24
    assert not bool(((a.grad.double().cpu() - gp_bad).abs() <= bound).all())


# ---- warp ------------------------------------------------------------------------------------------------------------
def _warp_case(shape, seed, reach=6):
    gen = torch.Generator().manual_seed(seed)
    B, H, W, C = shape
    return _grid(gen, shape), _flow(gen, B, H, W, reach), _grid(gen, shape)


def _assert_all_sides_leave(flo):
    B, H, W, _ = flo.shape
    y, x = torch.meshgrid(torch.arange(H, dtype=flo.dtype), torch.arange(W, dtype=flo.dtype), indexing="ij")
    qx, qy = x + flo[..., 0], y + flo[..., 1]
    assert (qx < 0).any() and (qx > W - 1).any() and (qy < 0).any() and (qy > H - 1).any()


@pytest.mark.parametrize("mode", ["clamp", "tfwarp"])
@pytest.mark.parametrize("hwc", LEVELS, ids=["L0", "L1", "L2", "L3", "L4"])
def test_warp_grad_level_shapes(hwc, mode):
    img, flo, g = _warp_case((2,) + hwc, 1)
    _assert_all_sides_leave(flo)
    out_ref, gi_ref, gf_ref = _oracle_warp(img, flo, g, mode)
    a = img.float().to(DEV).requires_grad_()
    f = flo.float().to(DEV).requires_grad_()
    layer = layers.WarpV2 if mode == "clamp" else layers.Warp
    out = layer(data_format="channels_last")((a, f))
    out.backward(g.float().to(DEV))
    _check(out, out_ref, "out")
    _check(a.grad, gi_ref, "grad_img")
    _check(f.grad, gf_ref, "grad_flo")


@pytest.mark.parametrize("mode", ["clamp", "tfwarp"])
@pytest.mark.parametrize("C", [1, 3, 17, 32, 64])
def test_warp_grad_ragged(C, mode):
    img, flo, g = _warp_case((2, 7, 11, C), 20 + C, reach=4)
    _, gi_ref, gf_ref = _oracle_warp(img, flo, g, mode)
    a = img.float().to(DEV).requires_grad_()
    f = flo.float().to(DEV).requires_grad_()
    ops.warp(a, f, mode).backward(g.float().to(DEV))
    _check(a.grad, gi_ref, "grad_img")
    _check(f.grad, gf_ref, "grad_flo")


@pytest.mark.parametrize("memory", ["dense", "channels_last"])
@pytest.mark.parametrize("C", [3, 32])
def test_warp_grad_channels_first(memory, C):
    img, flo, g = _warp_case((2, 9, 12, C), 4)
    _, gi_ref, gf_ref = _oracle_warp(img, flo, g, "tfwarp")
    mf = torch.channels_last if memory == "channels_last" else torch.contiguous_format
    a = img.float().permute(0, 3, 1, 2).to(DEV).contiguous(memory_format=mf).requires_grad_()
    f = flo.float().permute(0, 3, 1, 2).to(DEV).contiguous().requires_grad_()
    out = qwarp.tf_warp(a, f, data_format="channels_first")
    out.backward(g.float().permute(0, 3, 1, 2).to(DEV))
    _check(a.grad.permute(0, 2, 3, 1), gi_ref, "grad_img")
    _check(f.grad.permute(0, 2, 3, 1), gf_ref, "grad_flo")


def test_warp_grad_broadcast_and_fp16_flow():
    img, flo, g = _warp_case((2, 8, 10, 4), 6)
    f1 = torch.tensor([[[[1.25, -0.5]]]], dtype=torch.float64)          # (1,1,1,2)
    _, gi_ref, gf_ref = _oracle_warp(img, f1.expand(2, 8, 10, 2), g, "clamp")
    a = img.float().to(DEV).requires_grad_()
    f = f1.half().to(DEV).requires_grad_()
    layers.WarpV2(data_format="channels_last")((a, f)).backward(g.float().to(DEV))
    assert f.grad.shape == (1, 1, 1, 2) and f.grad.dtype == torch.float16
    _check(a.grad, gi_ref, "grad_img")
    ref = gf_ref.sum(dim=(0, 1, 2), keepdim=True)
    assert float((f.grad.double().cpu() - ref).abs().max()) <= F16_EPS * float(ref.abs().max()) + 1e-3


def test_dense_image_warp_entry_points():
    img, flo, g = _warp_case((2, 8, 10, 4), 8)
    # dense_image_warp: query = grid + flow with flow[..., 0] rows; the oracle's warp_v2 takes (x, y)
    _, gi_ref, gf_ref = _oracle_warp(img, flo, g, "clamp")
    a = img.float().to(DEV).requires_grad_()
    f = flo.flip(-1).float().to(DEV).requires_grad_()
    qwarp.dense_image_warp(a, f).backward(g.float().to(DEV))
    _check(a.grad, gi_ref, "grad_img")
    _check(f.grad.flip(-1), gf_ref, "grad_flo")
    f2 = (-flo.flip(-1)).float().to(DEV).requires_grad_()
    qwarp.tfa_dense_image_warp(img.float().to(DEV), f2).backward(g.float().to(DEV))
    _check(-f2.grad.flip(-1), gf_ref, "grad_flo (tfa sign)")


def test_warp_fp16_bound_and_negative_control():
    img, flo, g = _warp_case((2, 16, 32, 32), 9)
    _, gi_ref, gf_ref = _oracle_warp(img, flo, g, "clamp")
    a = img.half().to(DEV).requires_grad_()
    f = flo.float().to(DEV).requires_grad_()
    ops.warp(a, f, "clamp").backward(g.half().to(DEV))
    assert a.grad.dtype == torch.float16
    bound = F16_EPS * gi_ref.abs() + 1e-6 * float(gi_ref.abs().max()) + 2.0 ** -24
    assert bool(((a.grad.double().cpu() - gi_ref).abs() <= bound).all())
    _check(f.grad, gf_ref, "grad_flo")                                  # fp32 sums of exact fp16 products
    _, gi_bad, _ = _oracle_warp(img, flo, g * (1 + 1 / 16), "clamp")
    bound = F16_EPS * gi_bad.abs() + 1e-6 * float(gi_bad.abs().max()) + 2.0 ** -24
    assert not bool(((a.grad.double().cpu() - gi_bad).abs() <= bound).all())


# ---- the no-grad path, capture, determinism, a small model ---------------------------------------------------------------------------
def test_forward_bits_and_no_grad_fn():
    prv, nxt, _ = _cv_case((2, 16, 32, 32), 4, 11)
    img, flo, _ = _warp_case((2, 16, 32, 32), 11)
    p, n = prv.float().to(DEV), nxt.float().to(DEV)
    i, f = img.float().to(DEV), flo.float().to(DEV)
    for fmt in ("channels_last", "channels_first"):
        tr = (lambda t: t) if fmt == "channels_last" else (lambda t: t.permute(0, 3, 1, 2).contiguous())
        plain = ops.cost_volume(tr(p), tr(n), 4, fmt)
        assert plain.grad_fn is None
        graded = ops.cost_volume(tr(p).clone().requires_grad_(), tr(n), 4, fmt)
        assert graded.grad_fn is not None and torch.equal(plain, graded.detach())
        for mode in ("clamp", "tfwarp"):
            plain = ops.warp(tr(i), tr(f), mode, fmt)
            assert plain.grad_fn is None
            graded = ops.warp(tr(i), tr(f).clone().requires_grad_(), mode, fmt)
            assert graded.grad_fn is not None and torch.equal(plain, graded.detach())
    with torch.no_grad():
        assert ops.cost_volume(p.requires_grad_(), n).grad_fn is None


def test_backward_is_deterministic():
    prv, nxt, g = _cv_case((4, 64, 128, 32), 4, 12)
    p, n, gd = prv.float().to(DEV), nxt.float().to(DEV), g.float().to(DEV)
    out = ops.cost_volume(p, n)
    r1 = ops.cost_volume_bwd(p, n, out, gd)
    r2 = ops.cost_volume_bwd(p, n, out, gd)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    img, flo, gw = _warp_case((4, 64, 128, 32), 12)
    i, f, gwd = img.float().to(DEV), flo.float().to(DEV), gw.float().to(DEV)
    for mode in ("clamp", "tfwarp"):
        a = ops.warp_bwd(i, f, gwd, mode)
        b = ops.warp_bwd(i, f, gwd, mode)
        assert torch.equal(a[1], b[1])
        assert float((a[0] - b[0]).abs().max()) <= 1e-5 * max(1.0, float(a[0].abs().max()))


def test_grad_path_refuses_capture_and_no_grad_capture_still_works():
    """Under stream capture the differentiable path raises a clear error before it enqueues anything (a captured
    forward + backward is not supported yet); the no-grad forward captures and replays as before."""
    a = torch.randn(2, 16, 32, 32, device=DEV)
    b = torch.randn(2, 16, 32, 32, device=DEV)
    with torch.no_grad():
        eager = ops.cost_volume(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        ops.cost_volume(a, b)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        static = ops.cost_volume(a, b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    ag = a.clone().requires_grad_()
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph2):
            y = b * 2.0
            ops.cost_volume(ag, y)
    torch.cuda.synchronize()


class _Tiny(torch.nn.Module):
    """Torch convs around WarpV2 and CostVolumeV2 (search range 2), channels-last hot-path operands."""

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
        cv = self.cv_fn(fa, self.warp_fn(fb, flo))
        return self.head(cv.permute(0, 3, 1, 2))


def _hip_model():
    wp, cv = layers.WarpV2(data_format="channels_last"), layers.CostVolumeV2(2, data_format="channels_last")
    return _Tiny(lambda i, f: wp((i, f)), lambda p, n: cv((p, n)))


def _data(seed=0, B=2, H=16, W=16):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 3, H, W, generator=gen), torch.randn(B, 3, H, W, generator=gen),
            0.1 * torch.randn(B, 2, H, W, generator=gen))


def test_small_model_trains_and_matches_the_float64_oracle():
    torch.manual_seed(1)
    m = _hip_model().to(DEV)
    ref = _Tiny(torch_ref.warp_v2, lambda p, n: torch_ref.cost_volume(p, n, 2)).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()})
    a, b, t = _data(3)
    ((ref(a.double(), b.double()) - t.double()) ** 2).mean().backward()
    a, b, t = a.to(DEV), b.to(DEV), t.to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    losses = []
    for it in range(6):
        opt.zero_grad()
        loss = ((m(a, b) - t) ** 2).mean()
        loss.backward()
        if it == 0:
            for (name, p), q in zip(m.named_parameters(), ref.parameters()):
                d = float((p.grad.double().cpu() - q.grad).abs().max())
                assert d <= 1e-3 * max(1e-3, float(q.grad.abs().max())), (name, d)
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses

"""The label-free flow losses (qpwcnet_amd.loss.PhotometricLoss / multiscale_unsupervised, include/qpwc_unsup_loss.h) without
a GPU: the float64 torch chain that tests/test_gpu_unsup_loss.py holds the kernels to.
  * against an independent numpy restatement written with explicit loops over pixels and offsets (B = 2, 12 x 20, both
    kinds, with and without a mask): 1e-12 relative on the values, masks and counts exact -- the bound
    tests/test_masked_loss_cpu.py holds its chain to;
  * torch.autograd.gradcheck with its default tolerances (B = 1, 8 x 9, both kinds, smooth_weight > 0);
  * known answers: identical frames and zero flow, a constant image under a constant flow, an integer shift;
  * a 4 x 6 level: count 0, photometric loss 0, only the smoothness gradient;
  * the config round trip and the refusals;
  * the sample points the contract singles out (make_edge_case: q on an integer, at 0, at extent - 1, 1/16 and a whole
    image beyond either end): every class is hit where the GPU suite needs it, the chain agrees with the numpy loops
    there, and its gradient is the header's closed-form bilinear derivative, ties included;
  * the eight unrelated levels of the GPU suite's one-launch plan (TINY_LEVELS, make_levels): the tiles they have.
It also makes the cases of the GPU suite (make_case, make_edge_case, make_levels), so that both suites see the same
inputs."""
import math

import numpy as np
import pytest
import torch

from qpwcnet_amd import loss

KINDS = ("census", "charbonnier")


# ---- the inputs of the GPU suite ---------------------------------------------------------------------------------------

def make_case(H, W, seed, B=2, levels=4):
    """pairs (B,H,W,6) float32 on the 1/256 grid (every block mean up to 8 x 8 is exact in float32, so that every
    precision sees the same frames), and per level k a flow (B, H >> k, W >> k, 2) float32 on the 1/16-pixel grid, never
    an integer (a fractional part of 0 is moved to 8/16), with magnitudes up to w / 2 (exact in fp16), and a random
    occlusion mask (about 20 % set).  Channels-last; to_layout() makes the other layout."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = []
    for shift in (0.0, 1.5):
        chans = [0.25 * np.sin((xx + shift) * (0.35 + 0.1 * c) + 0.2 * c) * np.cos(yy * (0.3 + 0.05 * c))
                 + 0.04 * rng.standard_normal((B, H, W)) for c in range(3)]
        frames.append(np.stack(chans, axis=-1))
    pairs = np.concatenate(frames, axis=-1)
    pairs = (np.clip(np.round((pairs + 0.5) * 256.0), 0, 256) / 256.0 - 0.5).astype(np.float32)
    flows, masks = [], []
    for k in range(levels):
        h, w = H >> k, W >> k
        r = rng.uniform(-1.0, 1.0, (B, h, w, 2))
        f = np.round(r * np.abs(r) * np.array([w / 2.0, h / 2.0]) * 1.25 * 16.0)      # the square: most flows are small ...
        f = np.clip(f, -w * 8.0, w * 8.0)                                              # ... and the largest reach w / 2
        f = np.where(f % 16 == 0, f + 8, f) / 16.0
        flows.append(f.astype(np.float32))
        masks.append((rng.random((B, h, w)) < 0.2).astype(np.uint8))
    return {"pairs": pairs, "flows": flows, "masks": masks}


EDGE_CLASSES = ("int_x", "int_y", "zero_x", "zero_y", "last_x", "last_y", "below_x", "below_y", "above_x", "above_y",
                "far_neg_x", "far_pos_x", "far_neg_y", "far_pos_y")
EDGE_SHAPES = {"edge40x72": (40, 72, 1), "edge17x65": (17, 65, 2)}       # (H, W, seed): the first seeds whose case
                                                                         # passes the companion test below
OUTSIDE_CLASSES = tuple(c for c in EDGE_CLASSES if c[:3] in ("bel", "abo", "far"))


def make_edge_case(H, W, seed, B=2, per_class=20):
    """The sample points the contract singles out, one level: make_case's frames, flows and mask, with per_class pixels
    of every image given, per entry of EDGE_CLASSES, a flow that puts q = (x + u, y + v) on that axis at an interior
    integer (alpha = 0), at 0, at extent - 1 (floor clamped to extent - 2, alpha = 1, inside), 1/16 outside either end,
    or more than a whole image outside; the other axis gets an in-image point on the 1/16 grid off the integers.  Every
    flow is a multiple of 1/16 below 128 or of 1/2 below 256: exact in fp16, and x + u is exact in every precision.  Of
    each class the first pixels lie in the 3-pixel border strip of the image (which census leaves out of the sum but
    whose warped grey its neighbours read) and in the partial last tile of each axis that has one.
    -> make_case's dictionary plus "planted": (B,H,W) int8, the class index or -1."""
    th, tw = 8, 32                                               # _hip.UNSUP_LOSS_TILE, asserted by the companion test
    case = make_case(H, W, seed, B=B, levels=1)
    flow = case["flows"][0].astype(np.float64)
    rng = np.random.default_rng(seed + 1000)
    yy, xx = np.mgrid[0:H, 0:W]
    strip = (xx < 3) | (xx >= W - 3) | (yy < 3) | (yy >= H - 3)
    regions = [strip]
    if W % tw and W > tw:
        regions.append(xx >= (W - 1) // tw * tw)
    if H % th and H > th:
        regions.append(yy >= (H - 1) // th * th)
    planted = np.full((B, H, W), -1, dtype=np.int8)

    def inside_point(n):                                         # in the image, 1/16 or more from an integer
        return float(rng.integers(0, n - 1)) + float(rng.integers(1, 16)) / 16.0

    def target(name, n):
        return {"int": lambda: float(rng.integers(1, n - 1)), "zero": lambda: 0.0, "last": lambda: n - 1.0,
                "below": lambda: -1.0 / 16.0, "above": lambda: n - 1.0 + 1.0 / 16.0,
                "far_neg": lambda: -(n + float(rng.integers(0, 4)) + 0.5),
                "far_pos": lambda: 2.0 * n - 1.0 + float(rng.integers(0, 4)) + 0.5}[name]()

    for b in range(B):
        for ci, cls in enumerate(EDGE_CLASSES):
            name, axis = cls.rsplit("_", 1)
            for k in range(per_class):
                free = planted[b] < 0
                pool = np.argwhere(free & regions[k]) if k < len(regions) else np.empty((0, 2), dtype=np.int64)
                pool = pool if len(pool) else np.argwhere(free)
                y, x = pool[rng.integers(0, len(pool))]
                qx, qy = (target(name, W), inside_point(H)) if axis == "x" else (inside_point(W), target(name, H))
                flow[b, y, x] = (qx - x, qy - y)
                planted[b, y, x] = ci
    case["flows"] = [flow.astype(np.float32)]
    case["planted"] = planted
    return case


def edge_classes(flow):
    """{class: (B,h,w) bool} of a channels-last flow by the float64 restatement of q = (x + u, y + v): the classes are
    read off the sample points, not off what make_edge_case meant to plant."""
    flow = np.asarray(flow, dtype=np.float64)
    h, w = flow.shape[1:3]
    yy, xx = np.mgrid[0:h, 0:w]
    q = {"x": (xx + flow[..., 0], w), "y": (yy + flow[..., 1], h)}
    out = {}
    for axis, other in (("x", "y"), ("y", "x")):
        (a, n), (o, m) = q[axis], q[other]
        ok = (o >= 0) & (o <= m - 1)                              # the other axis stays inside
        out["int_" + axis] = ok & (a == np.floor(a)) & (a > 0) & (a < n - 1)
        out["zero_" + axis] = ok & (a == 0)
        out["last_" + axis] = ok & (a == n - 1)
        out["below_" + axis] = ok & (a == -1.0 / 16.0)
        out["above_" + axis] = ok & (a == n - 1 + 1.0 / 16.0)
        out["far_neg_" + axis] = ok & (a < -n)
        out["far_pos_" + axis] = ok & (a > 2 * n - 1)
    return out


# The plan of tests/test_gpu_unsup_loss.py: eight levels of unrelated sizes in one launch, not in descending order.
TINY_LEVELS = ((1, 1), (17, 65), (1, 40), (9, 1), (2, 2), (6, 40), (7, 7), (8, 33))


def make_levels(sizes, seed, B=2):
    """Per size a level of its own, frames included (factor 1): [{"pairs" (B,h,w,6), "flow" (B,h,w,2), "mask" (B,h,w)}]
    as make_case draws them.  A 7 x 7 level has one census candidate per image, (3, 3): its flow is set to keep the
    sample inside and its mask to 0 there.  Along an axis of extent 1 the only inside point is q = 0, which make_case's
    flows (never an integer) cannot reach: there every other pixel gets a zero component, so that the clamped floor
    max(extent - 2, 0) = 0 and the second tap min(floor + 1, extent - 1) = 0 carry pixels that count."""
    levels = []
    for i, (h, w) in enumerate(sizes):
        case = make_case(h, w, seed + i, B=B, levels=1)
        flow, mask = case["flows"][0], case["masks"][0]
        if h == 1:
            flow[:, :, ::2, 1] = 0.0
        if w == 1:
            flow[:, ::2, :, 0] = 0.0
        if (h, w) == (7, 7):
            flow[:, 3, 3] = (1.5, -2.25)
            mask[:, 3, 3] = 0
        levels.append({"pairs": case["pairs"], "flow": flow, "mask": mask})
    return levels


def to_layout(x, data_format, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x))
    t = t if data_format == "channels_last" else t.permute(0, 3, 1, 2).contiguous()
    return t.to(dtype)


# ---- the numpy restatement ---------------------------------------------------------------------------------------------

def _np_sample(img, b, y, x, u, v):
    """(value per channel, inside) of img[b] at (x + u, y + v) by the CLAMP rule."""
    h, w = img.shape[1:3]
    qx, qy = x + u, y + v
    fx = min(max(math.floor(qx), 0), max(w - 2, 0))
    fy = min(max(math.floor(qy), 0), max(h - 2, 0))
    ax, ay = min(max(qx - fx, 0.0), 1.0), min(max(qy - fy, 0.0), 1.0)
    x1, y1 = min(fx + 1, w - 1), min(fy + 1, h - 1)
    tl, tr, bl, br = img[b, fy, fx], img[b, fy, x1], img[b, y1, fx], img[b, y1, x1]
    top, bot = ax * (tr - tl) + tl, ax * (br - bl) + bl
    return ay * (bot - top) + top, (0 <= qx <= w - 1) and (0 <= qy <= h - 1)


def _np_grey(rgb):
    return 255.0 * (0.2989 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2])


def np_level(kind, prv, nxt, flow, occ, q, eps, edge, eps_s):
    """(photometric, smoothness, count, mask) of one level with loops: prv, nxt (B,h,w,3), flow (B,h,w,2) float64."""
    B, h, w, _ = prv.shape
    mask = np.zeros((B, h, w), dtype=bool)
    inside = np.zeros((B, h, w), dtype=bool)
    gp, gw = _np_grey(prv), np.zeros((B, h, w))
    warped = np.zeros((B, h, w, 3))
    for b in range(B):
        for y in range(h):
            for x in range(w):
                if kind == "census":
                    val, ins = _np_sample(_np_grey(nxt)[..., None], b, y, x, flow[b, y, x, 0], flow[b, y, x, 1])
                    gw[b, y, x] = val[0]
                else:
                    warped[b, y, x], ins = _np_sample(nxt, b, y, x, flow[b, y, x, 0], flow[b, y, x, 1])
                inside[b, y, x] = ins
    total, count = 0.0, 0
    for b in range(B):
        for y in range(h):
            for x in range(w):
                m = inside[b, y, x] and not (occ is not None and occ[b, y, x] != 0)
                if kind == "census":
                    m = m and 3 <= x < w - 3 and 3 <= y < h - 3
                mask[b, y, x] = m
                if not m:
                    continue
                count += 1
                if kind == "census":
                    dist = 0.0
                    for dy in range(-3, 4):
                        for dx in range(-3, 4):
                            if dy == 0 and dx == 0:
                                continue
                            dp = gp[b, y + dy, x + dx] - gp[b, y, x]
                            dw = gw[b, y + dy, x + dx] - gw[b, y, x]
                            e = (dp / math.sqrt(0.81 + dp * dp) - dw / math.sqrt(0.81 + dw * dw)) ** 2
                            dist += e / (0.1 + e)
                    total += (dist + eps) ** q
                else:
                    total += sum(((prv[b, y, x, c] - warped[b, y, x, c]) ** 2 + eps * eps) ** q for c in range(3)) / 3.0
    photo = total / max(count, 1)
    sx = sy = 0.0
    for b in range(B):
        for y in range(h):
            for x in range(w):
                for (yn, xn, axis) in ((y, x + 1, 0), (y + 1, x, 1)):
                    if yn >= h or xn >= w:
                        continue
                    wgt = math.exp(-edge * sum(abs(prv[b, yn, xn, c] - prv[b, y, x, c]) for c in range(3)) / 3.0)
                    s = sum(wgt * math.sqrt((flow[b, yn, xn, c] - flow[b, y, x, c]) ** 2 + eps_s * eps_s) for c in range(2))
                    if axis == 0:
                        sx += s
                    else:
                        sy += s
    sx = sx / (B * h * (w - 1) * 2) if w > 1 else 0.0
    sy = sy / (B * (h - 1) * w * 2) if h > 1 else 0.0
    return photo, (sx + sy) / 2.0, count, mask


def np_pool(x, k):
    for _ in range(k):
        N, H, W, C = x.shape
        x = x.reshape(N, H // 2, 2, W // 2, 2, C).mean(axis=(2, 4))
    return x


@pytest.fixture(scope="module")
def small():
    """B = 2, 12 x 20 with a second level of 6 x 10 (census count 0 there), float64."""
    rng = np.random.default_rng(7)
    pairs = rng.random((2, 12, 20, 6)) * 0.3 - 0.15
    flows = [rng.standard_normal((2, 12, 20, 2)) * 2.5, rng.standard_normal((2, 6, 10, 2)) * 1.5]
    masks = [(rng.random((2, 12, 20)) < 0.25).astype(np.uint8), (rng.random((2, 6, 10)) < 0.25).astype(np.uint8)]
    return pairs, flows, masks


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("kind", KINDS)
def test_chain_matches_the_numpy_restatement(small, kind, data_format, masked):
    pairs, flows, masks = small
    obj = loss.PhotometricLoss(kind, q=0.4, eps=0.01, smooth_weight=1.5, edge=20.0, smooth_eps=1e-3, data_format=data_format)
    occ = [torch.from_numpy(m) for m in masks] if masked else None
    total, per, parts = loss.multiscale_unsupervised(obj, to_layout(pairs, data_format, torch.float64),
                                                     [to_layout(f, data_format, torch.float64) for f in flows], occ)
    assert per.dtype == torch.float64 and parts["counts"].dtype == torch.int64
    some = 0
    for l, f in enumerate(flows):
        prv, nxt = np_pool(pairs[..., :3], l), np_pool(pairs[..., 3:], l)
        photo, smooth, count, mask = np_level(kind, prv, nxt, f, masks[l] if masked else None, 0.4, 0.01, 20.0, 1e-3)
        assert int(parts["counts"][l]) == count
        assert abs(float(parts["photometric"][l]) - photo) <= 1e-12 * abs(photo)
        assert abs(float(parts["smoothness"][l]) - smooth) <= 1e-12 * abs(smooth) and smooth > 1e-3
        want = photo + 1.5 * smooth
        assert abs(float(per[l]) - want) <= 1e-12 * abs(want)
        some += count
        if kind == "census" and l == 1:
            assert count == 0 and photo == 0.0
        else:
            assert 0 < count < mask.size         # something is masked, something is not
    assert abs(float(total) - float(per.sum())) <= 1e-12 * abs(float(total))


def _gradcheck_inputs(seed, keep_inside):
    """B = 1, 8 x 9: frames, a flow whose sample points are 0.2 or more from every integer (the kink of the CLAMP rule)
    and a mask.  keep_inside: every sample point is moved into the image."""
    torch.manual_seed(seed)
    h, w = 8, 9
    pairs = torch.rand(1, h, w, 6, dtype=torch.float64) * 0.4 - 0.2
    flow = (torch.rand(1, h, w, 2, dtype=torch.float64) * 0.6 + 0.2) * torch.where(torch.rand(1, h, w, 2) < 0.5, -1.0, 1.0)
    flow = flow + torch.randint(-2, 3, (1, h, w, 2))
    if keep_inside:
        xs, ys = torch.arange(w, dtype=torch.float64).view(1, 1, w), torch.arange(h, dtype=torch.float64).view(1, h, 1)
        flow = torch.stack([(xs + flow[..., 0]).clamp(0.2, w - 1.2) - xs, (ys + flow[..., 1]).clamp(0.2, h - 1.2) - ys], dim=-1)
    return pairs, flow, [torch.rand(1, h, w) < 0.2]


def _inside(flow):
    h, w = flow.shape[1:3]
    qx = torch.arange(w, dtype=flow.dtype).view(1, 1, w) + flow[..., 0]
    qy = torch.arange(h, dtype=flow.dtype).view(1, h, 1) + flow[..., 1]
    return (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)


@pytest.mark.parametrize("kind", KINDS)
def test_gradcheck(kind):
    """torch.autograd.gradcheck with its default tolerances, smooth_weight > 0, a mask.  Charbonnier: samples leave the
    image.  Census: every sample inside -- a pixel whose sample is outside passes no photometric gradient by the rule,
    though its warped grey still enters its neighbours' patches, so there the rule is not the derivative (next test)."""
    obj = loss.PhotometricLoss(kind, smooth_weight=0.7, edge=10.0, data_format="channels_last")
    pairs, flow, occ = _gradcheck_inputs(3, keep_inside=kind == "census")
    inside = _inside(flow)
    assert bool(inside.all()) == (kind == "census") and 0.1 < float(inside.float().mean())
    flow.requires_grad_()
    counts = loss.multiscale_unsupervised(obj, pairs, [flow], occ)[2]["counts"]
    assert 0 < int(counts[0]) < (6 if kind == "census" else 72)
    assert torch.autograd.gradcheck(lambda f: loss.multiscale_unsupervised(obj, pairs, [f], occ)[0], (flow,))


def test_gradcheck_census_with_samples_outside():
    """The census gradient with samples that leave the image: exactly zero (smooth_weight = 0) at the pixels whose sample
    is outside, and the derivative everywhere else -- gradcheck with those pixels' flows held fixed."""
    pairs, flow, occ = _gradcheck_inputs(4, keep_inside=False)
    inside = _inside(flow)
    assert 0.2 < float(inside.float().mean()) < 0.9
    photo = loss.PhotometricLoss("census", smooth_weight=0.0, data_format="channels_last")
    x = flow.clone().requires_grad_()
    total, _, parts = loss.multiscale_unsupervised(photo, pairs, [x], occ)
    assert int(parts["counts"][0]) > 0
    g = torch.autograd.grad(total, x)[0]
    assert not g[~inside].any() and g[inside].any()
    obj = loss.PhotometricLoss("census", smooth_weight=0.7, edge=10.0, data_format="channels_last")
    held = lambda f: torch.where(inside[..., None], f, flow)
    assert torch.autograd.gradcheck(lambda f: loss.multiscale_unsupervised(obj, pairs, [held(f)], occ)[0],
                                    (flow.clone().requires_grad_(),))


def test_known_answers_identical_frames_and_constants():
    B, h, w = 2, 9, 11
    frame = torch.rand(B, h, w, 3, dtype=torch.float64) - 0.5
    pairs = torch.cat([frame, frame], dim=3)
    zero = torch.zeros(B, h, w, 2, dtype=torch.float64)
    obj = loss.PhotometricLoss("census", q=0.4, eps=0.01, smooth_weight=1.0, data_format="channels_last")
    _, per, parts = loss.multiscale_unsupervised(obj, pairs, [zero])
    assert int(parts["counts"][0]) == B * (h - 6) * (w - 6)
    assert abs(float(parts["photometric"][0]) - 0.01 ** 0.4) <= 1e-12
    ch = loss.PhotometricLoss("charbonnier", q=0.4, eps=0.01, data_format="channels_last")
    _, _, parts = loss.multiscale_unsupervised(ch, pairs, [zero])
    assert int(parts["counts"][0]) == B * h * w and abs(float(parts["photometric"][0]) - (0.01 ** 2) ** 0.4) <= 1e-12
    # a constant image (every edge weight 1) under a constant flow: sqrt(0 + eps_s^2)
    const = torch.full((B, h, w, 6), 0.25, dtype=torch.float64)
    flow = torch.full((B, h, w, 2), 0.5, dtype=torch.float64)
    for eps_s in (1e-3, 0.02):
        obj = loss.PhotometricLoss("census", smooth_eps=eps_s, data_format="channels_last")
        assert abs(float(loss.multiscale_unsupervised(obj, const, [flow])[2]["smoothness"][0]) - eps_s) <= 1e-15


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shift", [(2, 0), (-3, 1), (0, -4), (5, 5)])
def test_known_answer_integer_shift(kind, shift):
    """Under the flow (sx, sy) everywhere the sample of (x, y) stays inside iff 0 <= x + sx <= w - 1 and the same along
    y: the count is the number of (interior) pixels in that window."""
    B, h, w = 2, 13, 17
    sx, sy = shift
    pairs = torch.rand(B, h, w, 6, dtype=torch.float64) - 0.5
    flow = torch.zeros(B, h, w, 2, dtype=torch.float64)
    flow[..., 0], flow[..., 1] = sx, sy
    obj = loss.PhotometricLoss(kind, data_format="channels_last")
    lo = 3 if kind == "census" else 0
    nx = sum(1 for x in range(lo, w - lo) if 0 <= x + sx <= w - 1)
    ny = sum(1 for y in range(lo, h - lo) if 0 <= y + sy <= h - 1)
    assert int(loss.multiscale_unsupervised(obj, pairs, [flow])[2]["counts"][0]) == B * nx * ny


def test_a_coarse_level_has_only_the_smoothness_gradient():
    torch.manual_seed(5)
    pairs = torch.rand(1, 4, 6, 6, dtype=torch.float64) * 0.1
    flow = (torch.randn(1, 4, 6, 2, dtype=torch.float64) * 0.4).requires_grad_()
    obj = loss.PhotometricLoss("census", smooth_weight=2.0, edge=5.0, data_format="channels_last")
    total, per, parts = loss.multiscale_unsupervised(obj, pairs, [flow])
    assert int(parts["counts"][0]) == 0 and float(parts["photometric"][0]) == 0.0
    total.backward()
    only = flow.grad.clone()
    assert float(only.abs().max()) > 0
    plain = flow.detach().clone().requires_grad_()
    f = plain
    sx = (torch.exp(-5.0 * (pairs[:, :, 1:, :3] - pairs[:, :, :-1, :3]).abs().mean(-1))[..., None]
          * torch.sqrt((f[:, :, 1:] - f[:, :, :-1]) ** 2 + 1e-6)).mean()
    sy = (torch.exp(-5.0 * (pairs[:, 1:, :, :3] - pairs[:, :-1, :, :3]).abs().mean(-1))[..., None]
          * torch.sqrt((f[:, 1:] - f[:, :-1]) ** 2 + 1e-6)).mean()
    (2.0 * (sx + sy) / 2).backward()
    assert float((only - plain.grad).abs().max()) <= 1e-15
    flat = loss.PhotometricLoss("census", smooth_weight=0.0, data_format="channels_last")
    g = torch.autograd.grad(loss.multiscale_unsupervised(flat, pairs, [flow])[0], flow)[0]
    assert not g.any()


def test_an_axis_of_extent_one():
    pairs = torch.rand(2, 8, 8, 6, dtype=torch.float64)
    flows = [torch.randn(2, 1, 1, 2, dtype=torch.float64).requires_grad_()]
    obj = loss.PhotometricLoss("charbonnier", data_format="channels_last")
    total, per, parts = loss.multiscale_unsupervised(obj, pairs, flows)
    assert float(parts["smoothness"][0]) == 0.0 and bool(torch.isfinite(per).all())
    total.backward()
    assert not flows[0].grad.any()          # one tap on both axes: nothing to differentiate


def test_config_round_trip_and_defaults():
    obj = loss.PhotometricLoss()
    cfg = obj.get_config()
    assert (cfg["kind"], cfg["q"], cfg["eps"], cfg["edge"], cfg["smooth_eps"]) == ("census", 0.4, 0.01, 150.0, 1e-3)
    fine = loss.FlowMseLossFineTune()
    assert (obj.q, obj.eps) == (fine.q, fine.eps)
    other = loss.PhotometricLoss("charbonnier", q=0.5, eps=0.02, smooth_weight=3.0, edge=10.0, smooth_eps=0.01,
                                 data_format="channels_first", name="photo")
    again = loss.PhotometricLoss.from_config(other.get_config())
    assert again.get_config() == other.get_config() and again.axis == 1 and again.name == "photo"


def test_refusals():
    obj = loss.PhotometricLoss(data_format="channels_last")
    pairs = torch.zeros(1, 16, 16, 6)
    flow = lambda h, w: torch.zeros(1, h, w, 2)
    for bad in ((5, 8), (8, 4), (16, 8), (3, 3), (32, 32), (12, 12)):
        with pytest.raises(ValueError, match="power of two"):
            loss.multiscale_unsupervised(obj, pairs, [flow(*bad)])
    for ok in ((16, 16), (8, 8), (1, 1)):
        loss.multiscale_unsupervised(obj, pairs, [flow(*ok)])
    with pytest.raises(ValueError, match="'estimate'"):
        loss.multiscale_unsupervised(obj, pairs, [flow(8, 8)], occluded="guess")
    with pytest.raises(ValueError, match="masks for"):
        loss.multiscale_unsupervised(obj, pairs, [flow(8, 8)], occluded=[None, None])
    with pytest.raises(ValueError, match="shape"):
        loss.multiscale_unsupervised(obj, pairs, [flow(8, 8)], occluded=[torch.zeros(1, 4, 4)])
    # the call of the supervised losses, loss(y_true, y_pred): a ground truth is not a frame pair
    with pytest.raises(ValueError, match="no ground truth"):
        obj(torch.zeros(1, 16, 16, 2), torch.zeros(1, 16, 16, 2))
    with pytest.raises(ValueError, match="no ground truth"):
        loss.multiscale_unsupervised(obj, torch.zeros(1, 6, 16, 16), [flow(16, 16)])      # the other layout's pair
    with pytest.raises(TypeError, match="PhotometricLoss"):
        loss.multiscale_unsupervised(loss.FlowMseLossV2(), pairs, [flow(16, 16)])
    with pytest.raises(TypeError):
        loss.multiscale(obj, pairs, [flow(16, 16)])
    with pytest.raises(ValueError, match="1..8"):
        loss.multiscale_unsupervised(obj, pairs, [])
    with pytest.raises(ValueError, match="batch"):
        loss.multiscale_unsupervised(obj, pairs, [torch.zeros(2, 16, 16, 2)])
    for bad in (dict(kind="ssim"), dict(q=0.0), dict(eps=0.0), dict(eps=float("nan")), dict(smooth_eps=-1.0),
                dict(edge=-1.0), dict(smooth_weight=-0.5), dict(data_format="nhwc")):
        with pytest.raises(ValueError):
            loss.PhotometricLoss(**bad)
    assert float(obj(pairs, flow(16, 16))) >= 0.0        # one level, as a call


def test_the_gpu_cases_mask_a_tenth_to_a_half():
    """What tests/test_gpu_unsup_loss.py asserts on the oracle's counts, here in float64 and float32: the flows of
    make_case send between a tenth and a half of every level's census candidates out of the image, and both precisions
    agree on every count (every sample point is 1/16 pixel or more from a floor boundary and from the border)."""
    for H, W, seed in ((32, 48, 11), (40, 72, 12)):
        case = make_case(H, W, seed)
        obj = loss.PhotometricLoss("census", data_format="channels_last")
        counts = {}
        for dt in (torch.float64, torch.float32):
            counts[dt] = loss.multiscale_unsupervised(obj, torch.from_numpy(case["pairs"]).to(dt),
                                                      [torch.from_numpy(f).to(dt) for f in case["flows"]])[2]["counts"]
        assert torch.equal(counts[torch.float64], counts[torch.float32])
        for k, f in enumerate(case["flows"]):
            h, w = H >> k, W >> k
            assert not (f * 16 % 16 == 0).any() and (f * 16 == np.round(f * 16)).all()
            assert np.abs(f[..., 0]).max() >= w / 2 - 1 and np.array_equal(f, f.astype(np.float16).astype(np.float32))
            cand = 2 * max(h - 6, 0) * max(w - 6, 0)
            if cand:
                assert 0.1 <= 1.0 - int(counts[torch.float64][k]) / cand <= 0.5, (H, W, k, int(counts[torch.float64][k]), cand)
            else:
                assert int(counts[torch.float64][k]) == 0


# ---- the contract edges and the plan of the GPU suite -------------------------------------------------------------------

def np_bilinear(img, flow):
    """The header's warp in closed form, vectorised: img (B,h,w,C) sampled at (x, y) + flow -> (value, d / d qx, d / d qy
    (B,h,w,C), inside (B,h,w)).  The derivative is that of the bilinear form on the clamped taps: the slope towards the
    second tap, at alpha = 0 and at alpha = 1 alike."""
    B, h, w, _ = img.shape
    yy, xx = np.mgrid[0:h, 0:w]
    qx, qy = xx + flow[..., 0], yy + flow[..., 1]
    fx, fy = np.clip(np.floor(qx), 0, max(w - 2, 0)), np.clip(np.floor(qy), 0, max(h - 2, 0))
    ax, ay = np.clip(qx - fx, 0.0, 1.0)[..., None], np.clip(qy - fy, 0.0, 1.0)[..., None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    bi = np.arange(B)[:, None, None]
    tl, tr, bl, br = img[bi, y0, x0], img[bi, y0, x1], img[bi, y1, x0], img[bi, y1, x1]
    top, bot = ax * (tr - tl) + tl, ax * (br - bl) + bl
    inside = (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
    return ay * (bot - top) + top, (1.0 - ay) * (tr - tl) + ay * (br - bl), bot - top, inside


def closed_form_gradient(kind, pairs, flow, occ, q=0.4, eps=0.01):
    """d photo / d flow of one level (smooth_weight = 0) by the header: "the bilinear derivative where inside_p and
    exactly 0 where not", times d photo / d (warped value), which no tie touches.  Float64 numpy (B,h,w,2)."""
    prv, nxt = pairs[..., :3].astype(np.float64), pairs[..., 3:].astype(np.float64)
    flow = flow.astype(np.float64)
    B, h, w, _ = prv.shape
    keep = np.ones((B, h, w), dtype=bool) if occ is None else occ == 0
    if kind == "charbonnier":
        val, dx, dy, inside = np_bilinear(nxt, flow)
        m = inside & keep
        d = prv - val
        k = -(q * (d * d + eps * eps) ** (q - 1.0)) * 2.0 * d / 3.0             # d term / d warped_c
        g = np.stack([(k * dx).sum(-1), (k * dy).sum(-1)], axis=-1) * m[..., None]
        return g / max(int(m.sum()), 1)
    val, dx, dy, inside = np_bilinear(_np_grey(nxt)[..., None], flow)
    if h < 7 or w < 7:
        return np.zeros((B, h, w, 2))
    gw = torch.from_numpy(val[..., 0]).requires_grad_()                          # d photo / d gw by autograd: gw is a leaf
    e = (loss._unsup_ternary(torch.from_numpy(_np_grey(prv))) - loss._unsup_ternary(gw)) ** 2
    term = ((e / (0.1 + e)).sum(-1) + eps) ** q
    m = torch.from_numpy((inside & keep)[:, 3:h - 3, 3:w - 3])
    (torch.where(m, term, torch.zeros(())).sum() / max(int(m.sum()), 1)).backward()
    c = gw.grad.numpy()[..., None]
    return np.concatenate([c * dx, c * dy], axis=-1) * inside[..., None]


def _edge_chain(kind, case, masked, dtype, smooth_weight=0.0):
    obj = loss.PhotometricLoss(kind, smooth_weight=smooth_weight, edge=40.0, data_format="channels_last")
    x = torch.from_numpy(case["flows"][0]).to(dtype).requires_grad_()
    occ = [torch.from_numpy(case["masks"][0])] if masked else None
    total, per, parts = loss.multiscale_unsupervised_torch(obj, torch.from_numpy(case["pairs"]).to(dtype), [x], occ)
    total.backward()
    return per.detach(), parts, x.grad


def test_the_edge_cases_hit_every_class_of_the_contract():
    """What tests/test_gpu_unsup_loss.py relies on, on the float64 restatement, per class and per image: at least 16
    pixels, one of them in the image's 3-pixel border strip and one in the partial last tile of every axis that has one;
    flows exact in fp16 on the 1/16 grid; float32 and float64 agree on every count; with occluded=None between a tenth
    and a half of the census candidates are masked; and the two sizes have the tiles the suite names."""
    from qpwcnet_amd import _hip
    th, tw = _hip.UNSUP_LOSS_TILE
    assert (th, tw) == (8, 32)
    sizes = [v[:2] for v in EDGE_SHAPES.values()]
    assert any(W % tw and W > tw for _, W in sizes) and any(H % th and H > th for H, _ in sizes)     # partial tiles
    assert any(H > th and W > tw for H, W in sizes)                                                  # a seam inside
    assert any((W - 1) % tw == 0 and W > 1 for _, W in sizes)               # x = w - 1 is the first column of a tile
    for name, (H, W, seed) in EDGE_SHAPES.items():
        case = make_edge_case(H, W, seed)
        f = case["flows"][0]
        assert (f * 16 == np.round(f * 16)).all() and np.array_equal(f, f.astype(np.float16).astype(np.float32))
        yy, xx = np.mgrid[0:H, 0:W]
        strip = (xx < 3) | (xx >= W - 3) | (yy < 3) | (yy >= H - 3)
        classes = edge_classes(f)
        assert set(classes) == set(EDGE_CLASSES)
        for cls, sel in classes.items():
            for b in range(f.shape[0]):
                assert int(sel[b].sum()) >= 16, (name, cls, b, int(sel[b].sum()))
                assert (sel[b] & strip).any(), (name, cls, b)
                if W % tw and W > tw:
                    assert (sel[b] & (xx >= (W - 1) // tw * tw)).any(), (name, cls, b)
                if H % th and H > th:
                    assert (sel[b] & (yy >= (H - 1) // th * th)).any(), (name, cls, b)
        for kind in KINDS:
            for masked in (False, True):
                c64 = _edge_chain(kind, case, masked, torch.float64)[1]["counts"]
                c32 = _edge_chain(kind, case, masked, torch.float32)[1]["counts"]
                assert torch.equal(c64, c32), (name, kind, masked)
                if kind == "census" and not masked:
                    share = 1.0 - int(c64[0]) / (2 * (H - 6) * (W - 6))
                    assert 0.1 <= share <= 0.5, (name, share)


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("kind", KINDS)
def test_edge_oracle_matches_the_numpy_restatement(kind, masked):
    """The float64 chain against np_level on a small instance of make_edge_case (B = 2, 10 x 14, two pixels per class):
    values within 1e-12, the count exact."""
    case = make_edge_case(10, 14, 21, per_class=2)
    classes = edge_classes(case["flows"][0])
    assert all(sel.any() for sel in classes.values())
    per, parts, _ = _edge_chain(kind, case, masked, torch.float64, smooth_weight=1.5)
    pairs = case["pairs"].astype(np.float64)
    photo, smooth, count, _ = np_level(kind, pairs[..., :3], pairs[..., 3:], case["flows"][0].astype(np.float64),
                                       case["masks"][0] if masked else None, 0.4, 0.01, 40.0, 1e-3)
    assert int(parts["counts"][0]) == count and count > 0
    assert abs(float(parts["photometric"][0]) - photo) <= 1e-12 * abs(photo)
    assert abs(float(parts["smoothness"][0]) - smooth) <= 1e-12 * abs(smooth)
    assert abs(float(per[0]) - (photo + 1.5 * smooth)) <= 1e-12 * abs(photo + 1.5 * smooth)


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_edge_oracle_gradient_is_the_closed_form_derivative(kind, shape, masked):
    """The oracle's photometric gradient (smooth_weight = 0) against the header's closed form at every pixel, the
    planted ones among them: the slope towards the second tap where the sample is inside (q = 0, q = extent - 1 and
    alpha = 0 included), exactly 0 where it is not.  An oracle that split a tie differently fails here."""
    case = make_edge_case(*EDGE_SHAPES[shape])
    _, _, got = _edge_chain(kind, case, masked, torch.float64)
    want = closed_form_gradient(kind, case["pairs"], case["flows"][0], case["masks"][0] if masked else None)
    got = got.numpy()
    top = np.abs(want).max()
    assert top > 0 and np.abs(got - want).max() <= 1e-12 * top
    classes = edge_classes(case["flows"][0])
    for cls in OUTSIDE_CLASSES:
        assert not got[classes[cls]].any() and not want[classes[cls]].any(), cls
    keep = case["masks"][0] == 0 if masked else np.ones(classes["zero_x"].shape, dtype=bool)
    for cls in ("int_x", "int_y", "zero_x", "zero_y", "last_x", "last_y"):
        assert got[classes[cls] & keep].any(), cls
        assert np.abs(got - want)[classes[cls]].max() <= 1e-12 * top


def test_the_tiny_plan_has_the_tiles_the_gpu_suite_names():
    """TINY_LEVELS against _hip.UNSUP_LOSS_TILE: a level of one tile; levels whose only split axis is x, whose only
    split axis is y, and one split on both, each with a partial last tile; a level three tiles wide whose last tile has
    one column; sizes not in descending order; and the oracle's count of the 7 x 7 level is one per image."""
    from qpwcnet_amd import _hip
    th, tw = _hip.UNSUP_LOSS_TILE
    tiles = [(-(-h // th), -(-w // tw)) for h, w in TINY_LEVELS]
    part = [(h % th != 0 and h > th, w % tw != 0 and w > tw) for h, w in TINY_LEVELS]
    assert len(TINY_LEVELS) == 8 and (1, 1) in tiles
    assert (False, True) in part and (True, False) in part and (True, True) in part
    assert any(t[1] == 3 and w % tw == 1 for t, (h, w) in zip(tiles, TINY_LEVELS))
    area = [h * w for h, w in TINY_LEVELS]
    assert area != sorted(area, reverse=True) and area != sorted(area)
    assert TINY_LEVELS[0] == (1, 1) and sum(1 for h, w in TINY_LEVELS if h < 7 or w < 7) == 5
    levels = make_levels(TINY_LEVELS, 50)
    lv = levels[TINY_LEVELS.index((7, 7))]
    obj = loss.PhotometricLoss("census", data_format="channels_last")
    parts = loss.multiscale_unsupervised_torch(obj, torch.from_numpy(lv["pairs"]).double(),
                                               [torch.from_numpy(lv["flow"]).double()])[2]
    assert int(parts["counts"][0]) == 2
    # an axis of extent 1: some samples are inside (Charbonnier counts them), and not all
    obj = loss.PhotometricLoss("charbonnier", data_format="channels_last")
    for (h, w), lv in zip(TINY_LEVELS, levels):
        if h == 1 or w == 1:
            count = int(loss.multiscale_unsupervised_torch(obj, torch.from_numpy(lv["pairs"]).double(),
                                                           [torch.from_numpy(lv["flow"]).double()])[2]["counts"][0])
            assert 0 < count <= 2 * h * w and (count < 2 * h * w or h * w == 1), (h, w, count)

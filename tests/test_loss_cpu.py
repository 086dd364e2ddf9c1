"""CPU suite of the training losses (qpwcnet_amd.loss, qpwc_loss_fwd / qpwc_loss_bwd):
  * every argument check of the C ABI returns its QPWC_E_* code before any HIP call, and the Python layer maps it to
    ValueError;
  * the float64 restatement of the four losses of qpwcnet/train/loss.py that the GPU suite checks against (einops'
    reduce as reshape-mean, tf.image.resize as explicit half-pixel index math) agrees with a second restatement from
    torch ops, and its gradients pass gradcheck away from kinks;
  * the Keras surface: data_format captured at construction, the config round trip, CPU tensors and a y_true that
    requires grad refused;
  * the loss kernels use no scratch and no float atomics (determinism holds by construction)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qpwcnet_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KINDS = ("v2", "mse", "finetune", "autoresize")


# ---- float64 restatement of qpwcnet/train/loss.py (channels_last arrays; channels_first is permuted in) ----------------
def _nhwc(t, data_format):
    return t.permute(0, 2, 3, 1) if data_format == "channels_first" else t


def area_mean(gt, h, w):
    """einops.reduce(y_true, 'n (h sh) (w sw) c -> n h w c', 'mean') (loss.py:160-173) as reshape-mean."""
    B, H, W, C = gt.shape
    if H % h or W % w:
        raise ValueError("not a whole-block reduction")
    return gt.reshape(B, h, H // h, w, W // w, C).mean(dim=(2, 4))


def _axis(n_out, n_in):
    """tf.image.resize bilinear, half_pixel_centers: in = (out + 0.5) * n_in / n_out - 0.5, lower = max(floor(in), 0),
    upper = min(ceil(in), n_in - 1), lerp = in - floor(in)."""
    src = (torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5
    fl = torch.floor(src)
    lo = fl.clamp(min=0).long()
    hi = torch.ceil(src).clamp(max=n_in - 1).long()
    return lo, hi, src - fl


def resize_bilinear(gt, h, w):
    B, H, W, C = gt.shape
    ylo, yhi, ly = _axis(h, H)
    xlo, xhi, lx = _axis(w, W)
    ly, lx = ly.view(1, h, 1, 1), lx.view(1, 1, w, 1)
    top = gt[:, ylo][:, :, xlo] + (gt[:, ylo][:, :, xhi] - gt[:, ylo][:, :, xlo]) * lx
    bot = gt[:, yhi][:, :, xlo] + (gt[:, yhi][:, :, xhi] - gt[:, yhi][:, :, xlo]) * lx
    return top + (bot - top) * ly


def ref_loss(kind, y_true, y_pred, data_format="channels_last", q=0.4, eps=0.01, delta=0.1):
    """One level of the four losses, float64: y_true (B,H,W,C) / (B,C,H,W), y_pred at the level's (h, w)."""
    gt, p = _nhwc(y_true, data_format).double(), _nhwc(y_pred, data_format).double()
    H = gt.shape[1]
    h, w = p.shape[1], p.shape[2]
    if kind == "v2":
        s = 2.0 / (w + h)
        e = s * p - s * (area_mean(gt, h, w) * (h / H))
        a = e.abs()
        # Keras Huber: mean over the last axis, then SUM_OVER_BATCH_SIZE = the mean over every element
        return torch.where(a <= delta, 0.5 * e * e, delta * a - 0.5 * delta * delta).mean()
    if kind == "autoresize":
        return ((p - resize_bilinear(gt, h, w)) ** 2).mean()
    r = resize_bilinear(gt, h, w) * (h / H) - p
    if kind == "mse":
        return torch.sqrt((r * r).sum(-1)).mean()
    return (r.abs().sum(-1) + eps).pow(q).mean()


def torch_ops_loss(kind, y_true, y_pred, data_format="channels_last", q=0.4, eps=0.01, delta=0.1):
    """The same losses composed from torch ops (F.avg_pool2d, F.interpolate, F.huber_loss)."""
    cf = lambda t: t.double() if data_format == "channels_first" else t.double().permute(0, 3, 1, 2)
    gt, p = cf(y_true), cf(y_pred)
    H, W = gt.shape[2:]
    h, w = p.shape[2:]
    if kind == "v2":
        g = F.avg_pool2d(gt, (H // h, W // w)) * (h / H)
        s = 2.0 / (w + h)
        return F.huber_loss(s * p, s * g, delta=delta)
    g = F.interpolate(gt, size=(h, w), mode="bilinear", align_corners=False)
    if kind == "autoresize":
        return F.mse_loss(p, g)
    r = g * (h / H) - p
    if kind == "mse":
        return torch.linalg.vector_norm(r, 2, dim=1).mean()
    return (torch.linalg.vector_norm(r, 1, dim=1) + eps).pow(q).mean()


def make_case(kind, B, H, W, shapes, data_format, seed, dtype=torch.float64):
    """(y_true, [y_pred per level]) in data_format: flows of a few pixels (images for autoresize) and predictions
    0.25..0.75 away from their level's bilinear ground truth in every channel, random signs: away from the kinks of
    the norms (a zero residual, sign(0)), where the direction of a tiny fp32 residual is ill-conditioned."""
    gen = torch.Generator().manual_seed(seed)
    C = 3 if kind == "autoresize" else 2
    gt = torch.randn(B, H, W, C, generator=gen, dtype=torch.float64) * (1.0 if kind == "autoresize" else 4.0)
    preds = []
    for h, w in shapes:
        base = resize_bilinear(gt, h, w) * (1.0 if kind == "autoresize" else h / H)
        mag = 0.25 + 0.5 * torch.rand(B, h, w, C, generator=gen, dtype=torch.float64)
        sign = torch.where(torch.rand(B, h, w, C, generator=gen) < 0.5, -1.0, 1.0).double()
        preds.append(base + sign * mag)
    tr = (lambda t: t.permute(0, 3, 1, 2).contiguous()) if data_format == "channels_first" else (lambda t: t)
    return tr(gt).to(dtype), [tr(p).to(dtype) for p in preds]


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("kind", KINDS)
def test_restatements_agree(kind, data_format):
    cases = [(2, 32, 64, [(16, 32), (8, 16), (4, 8)]),
             (2, 12, 20, [(4, 4), (3, 5), (6, 10)]),          # sh != sw
             (1, 9, 15, [(3, 5), (9, 15), (1, 1)])]
    for i, (B, H, W, shapes) in enumerate(cases):
        gt, preds = make_case(kind, B, H, W, shapes, data_format, 10 + i)
        for p in preds:
            a, b = ref_loss(kind, gt, p, data_format), torch_ops_loss(kind, gt, p, data_format)
            assert abs(float(a) - float(b)) <= 1e-12 * max(1.0, abs(float(b))), (kind, (H, W), tuple(p.shape))


def test_restatement_resize_matches_half_pixel_interpolate_when_upsampling():
    gen = torch.Generator().manual_seed(3)
    gt = torch.randn(2, 5, 7, 3, generator=gen, dtype=torch.float64)
    ref = F.interpolate(gt.permute(0, 3, 1, 2), size=(11, 13), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert torch.allclose(resize_bilinear(gt, 11, 13), ref, atol=1e-12)


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_gradcheck_away_from_kinks(kind):
    gt, preds = make_case(kind, 1, 8, 12, [(4, 6), (2, 3)], "channels_last", 5)
    for p in preds:
        p = p.clone().requires_grad_()
        if kind == "v2":   # no residual within 1e-3 of +-delta (the Huber kink) at the level's loss scale
            s = 2.0 / (p.shape[1] + p.shape[2])
            e = s * p.detach() - s * area_mean(gt, p.shape[1], p.shape[2]) * (p.shape[1] / gt.shape[1])
            assert float(((e.abs() - 0.1).abs()).min()) > 1e-4
        assert torch.autograd.gradcheck(lambda x: ref_loss(kind, gt, x), (p,), eps=1e-7, atol=1e-7)


def test_area_reduction_refuses_a_factor_that_does_not_divide():
    with pytest.raises(ValueError):
        area_mean(torch.zeros(1, 10, 10, 2, dtype=torch.float64), 3, 5)


# ---- the C ABI refuses bad arguments before any HIP call ----------------------------------------------------------------
def _host(n_floats=1 << 15):
    buf = (ctypes.c_float * n_floats)()
    base = ctypes.cast(buf, ctypes.c_void_p).value
    return buf, base + (-base) % 256


def test_loss_fwd_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, base = _host()
    # y_true (1,4,8,2) at base; two levels (2,4), (1,2); every buffer 4 KiB apart
    yt, p0, p1, d0, d1, g0, g1, out, ws = (base + 4096 * i for i in range(9))
    ws_big = base + 4096 * 9                                  # the workspace: 2 x 2048 floats = 16 KiB
    VP, I = ctypes.c_void_p, ctypes.c_int

    def arr(t, *v):
        return (t * len(v))(*v)

    def call(kind=0, delta=0.1, y_true=yt, B=1, H=4, W=8, C=2, layout=0, preds=(p0, p1), h=(2, 1), w=(4, 2),
             dt=(0, 0), n=2, out=out, dpred=None, gt_out=None, ws=ws_big):
        return L.qpwc_loss_fwd(kind, delta, 0.0, y_true, B, H, W, C, layout, arr(VP, *preds), arr(I, *h), arr(I, *w),
                               arr(I, *dt), n, out, None if dpred is None else arr(VP, *dpred),
                               None if gt_out is None else arr(VP, *gt_out), ws, None)

    assert call(kind=4) == _hip.E_MODE
    assert call(kind=-1) == _hip.E_MODE
    assert call(n=0) == _hip.E_SHAPE
    assert call(n=9, preds=(p0,) * 9, h=(2,) * 9, w=(4,) * 9, dt=(0,) * 9) == _hip.E_SHAPE
    assert b"n_levels" in L.qpwc_last_error()
    assert call(h=(3, 1)) == _hip.E_SHAPE                     # 4 % 3: not a whole-block area reduction
    assert b"whole-block" in L.qpwc_last_error()
    assert call(w=(4, 3)) == _hip.E_SHAPE
    for kind in (0, 1, 2):
        assert call(kind=kind, C=3) == _hip.E_SHAPE           # flow losses take 2 channels
    assert call(B=0) == _hip.E_SHAPE
    assert call(h=(0, 1)) == _hip.E_SHAPE
    assert call(layout=2) == _hip.E_LAYOUT
    assert call(dt=(0, 2)) == _hip.E_DTYPE
    assert call(delta=-0.1) == _hip.E_RANGE
    assert call(y_true=None) == _hip.E_NULL
    assert call(out=None) == _hip.E_NULL
    assert call(ws=None) == _hip.E_NULL
    assert call(preds=(p0, None)) == _hip.E_NULL              # a missing prediction without gt_out
    assert call(dpred=(d0, None)) == _hip.E_NULL
    assert L.qpwc_loss_fwd(0, 0.1, 0.0, yt, 1, 4, 8, 2, 0, None, arr(I, 2), arr(I, 4), arr(I, 0), 1, out, None, None,
                           ws_big, None) == _hip.E_NULL
    assert call(y_true=yt + 2) == _hip.E_ALIGN
    assert call(preds=(p0 + 2, p1)) == _hip.E_ALIGN
    assert call(dt=(1, 0), preds=(p0 + 1, p1)) == _hip.E_ALIGN
    assert call(dpred=(d0 + 2, d1)) == _hip.E_ALIGN
    assert call(dpred=(yt, d1)) == _hip.E_ALIAS               # an output over the ground truth
    assert call(dpred=(d0, p0 + 8)) == _hip.E_ALIAS           # ... over a prediction
    assert call(gt_out=(g0, p1)) == _hip.E_ALIAS
    assert call(dpred=(d0, d1), gt_out=(d1 + 4, g1)) == _hip.E_ALIAS   # two outputs overlap
    assert call(out=ws_big + 64) == _hip.E_ALIAS              # out_losses inside the workspace
    assert call(ws=yt) == _hip.E_ALIAS
    # the Python layer's mapping: argument errors are ValueError
    with pytest.raises(ValueError, match="whole-block"):
        _hip.check(call(h=(3, 1)))
    with pytest.raises(ValueError):
        _hip.check(call(kind=7))


def test_loss_workspace_and_kernel_choice_need_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    I = ctypes.c_int
    hs, ws = (I * 5)(128, 64, 32, 16, 8), (I * 5)(256, 128, 64, 32, 16)
    assert L.qpwc_loss_workspace_floats(0, 8, 256, 512, 2, hs, ws, 5) == 5 * 2048
    assert L.qpwc_loss_workspace_floats(3, 8, 256, 512, 3, hs, ws, 5) == 5 * 2048
    assert L.qpwc_loss_workspace_floats(5, 8, 256, 512, 2, hs, ws, 5) == _hip.E_MODE
    assert L.qpwc_loss_workspace_floats(0, 8, 256, 512, 2, hs, ws, 9) == _hip.E_SHAPE
    assert L.qpwc_loss_workspace_floats(1, 8, 256, 512, 4, hs, ws, 5) == _hip.E_SHAPE
    aligned, odd = 1 << 20, (1 << 20) + 8
    pick = lambda kind, p, H, W, h, w: L.qpwc_loss_fwd_kernel(kind, p, 8, H, W, 2, (I * len(h))(*h), (I * len(w))(*w),
                                                              len(h)).decode()
    assert pick(0, aligned, 256, 512, hs[:5], ws[:5]) == "loss_area_tile_kernel"     # config 2's pyramid
    assert pick(0, odd, 256, 512, hs[:5], ws[:5]) == "loss_pixel_kernel"             # no 16-byte loads
    assert pick(0, aligned, 96, 160, (32, 24), (32, 40)) == "loss_pixel_kernel"      # factors 3 x 5: not nested
    assert pick(0, aligned, 256, 512, (128, 32), (128, 64)) == "loss_area_tile_kernel"   # sh != sw, nested
    assert pick(0, aligned, 256, 512, (128, 64), (128, 256)) == "loss_pixel_kernel"  # 2x4 then 4x2: not nested
    assert pick(0, aligned, 256, 512, (256,), (512,)) == "loss_pixel_kernel"         # 1x1 (more than one per thread)
    assert pick(1, aligned, 256, 512, hs[:5], ws[:5]) == "loss_pixel_kernel"         # bilinear
    assert pick(0, aligned, 256, 512, (100,), (128,)) == ""                          # refused


def test_loss_bwd_argument_validation_needs_no_gpu(hip_lib):
    from qpwcnet_amd import _hip
    L = hip_lib
    keep, base = _host()
    d0, d1, g0, g1, gl = (base + 4096 * i for i in range(5))
    VP = ctypes.c_void_p

    def call(d=(d0, d1), gl=gl, g=(g0, g1), n_el=(16, 8), dt=(0, 0), n=2):
        return L.qpwc_loss_bwd((VP * len(d))(*d), gl, (VP * len(g))(*g), (ctypes.c_int64 * len(n_el))(*n_el),
                               (ctypes.c_int * len(dt))(*dt), n, None)

    assert call(gl=None) == _hip.E_NULL
    assert call(d=(d0, None)) == _hip.E_NULL
    assert call(g=(None, g1)) == _hip.E_NULL
    assert call(n=0) == _hip.E_SHAPE
    assert call(n=9) == _hip.E_SHAPE
    assert call(n_el=(16, 0)) == _hip.E_SHAPE
    assert call(dt=(0, 3)) == _hip.E_DTYPE
    assert call(g=(g0 + 2, g1)) == _hip.E_ALIGN
    assert call(gl=gl + 1) == _hip.E_ALIGN
    assert call(g=(d1, g1)) == _hip.E_ALIAS
    assert call(g=(g0, g0 + 32)) == _hip.E_ALIAS
    assert call(g=(g0, gl)) == _hip.E_ALIAS


# ---- the Keras surface ----------------------------------------------------------------------------------------------------
def test_data_format_is_captured_at_construction_and_configs_round_trip():
    import qpwcnet_amd as K
    from qpwcnet_amd import loss
    prev = K.image_data_format()
    try:
        K.set_image_data_format("channels_first")
        v2, ar = loss.FlowMseLossV2(), loss.AutoResizeMseLoss()
        K.set_image_data_format("channels_last")
        assert v2.data_format == "channels_first" and v2.axis == 1
        assert ar.data_format == "channels_first"
        assert loss.FlowMseLossV2().data_format == "channels_last"
    finally:
        K.set_image_data_format(prev)
    # the two with an explicit argument default to 'channels_first' as in the reference
    assert loss.FlowMseLoss().data_format == "channels_first"
    assert loss.FlowMseLossFineTune().data_format == "channels_first"
    for obj in (loss.FlowMseLoss("channels_last", name="l1"), loss.FlowMseLossFineTune("channels_last", 0.5, 0.02),
                loss.FlowMseLossV2(name="v2"), loss.AutoResizeMseLoss()):
        cfg = obj.get_config()
        again = type(obj).from_config(cfg)
        assert again.get_config() == cfg and again.data_format == obj.data_format
    assert loss.FlowMseLossFineTune("channels_last", 0.5, 0.02).get_config() == {
        "name": None, "data_format": "channels_last", "q": 0.5, "eps": 0.02}
    with pytest.raises(ValueError, match="Unsupported data format"):
        loss.FlowMseLoss("nhwc")
    with pytest.raises(TypeError):
        loss.FlowMseLossV2(reduction="sum")


def test_cpu_tensors_and_a_y_true_that_requires_grad_are_refused():
    from qpwcnet_amd import loss
    gt = torch.zeros(1, 8, 8, 2)
    pred = torch.zeros(1, 4, 4, 2, requires_grad=True)
    for obj in (loss.FlowMseLossV2(), loss.FlowMseLoss("channels_last"), loss.FlowMseLossFineTune("channels_last"),
                loss.AutoResizeMseLoss()):
        with pytest.raises(RuntimeError, match="HIP device"):
            obj(gt, pred)
        with pytest.raises(RuntimeError, match="HIP device"):
            obj(gt, pred.detach())
        with pytest.raises(ValueError, match="y_true requires grad"):
            obj(gt.clone().requires_grad_(), pred)
    with pytest.raises(ValueError, match="y_true requires grad"):
        loss.multiscale(loss.FlowMseLossV2(), gt.clone().requires_grad_(), [pred.detach()])
    with pytest.raises(TypeError):
        loss.multiscale(torch.nn.MSELoss(), gt, [pred])


# ---- ISA: no scratch, no float atomics ------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_loss_kernels_use_no_scratch_and_no_atomics(tmp_path):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--save-temps", "-c",
                    os.path.join(CSRC, "loss.hip"), "-o", str(tmp_path / "loss.o")],
                   cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    isa = [p for p in os.listdir(str(tmp_path)) if p.endswith(".s") and "gfx950" in p]
    assert isa, os.listdir(str(tmp_path))
    text = (tmp_path / isa[0]).read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)$", text, re.M)
    assert len([k for k in kernels if "loss" in k]) == 12, kernels   # 2 tile + 8 pixel + final fold + backward
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", m.group(2)), m.group(1)
    assert not re.search(r"^\s*(global|buffer|flat|ds)_(atomic_)?(add|pk_add)_f(32|16)|atomic", text, re.M | re.I)

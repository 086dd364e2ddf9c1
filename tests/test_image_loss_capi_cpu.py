"""The C boundary of the interpolator's SSIM + Charbonnier loss (include/qpwc_image_loss.h): the ctypes table against the
header, the workspace formula and the form query, and the argument validation of qpwc_image_loss_fwd / qpwc_image_loss_bwd
code by code, with HOST pointers: validation only looks at the values of the pointers and comes before any HIP call.
Without a device a call that passes it fails at the launch (QPWC_E_LAUNCH); with a device it would launch on host memory,
so those tests skip themselves there, as tests/test_unsup_loss_capi_cpu.py does."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

from qpwcnet_amd import _hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qpwc_image_loss.h")
NAMES = ["qpwc_image_loss_workspace_floats", "qpwc_image_loss_fwd", "qpwc_image_loss_fwd_kernel", "qpwc_image_loss_bwd"]
host_only = pytest.mark.skipif(torch.cuda.is_available(),
                               reason="host pointers: a wrongly accepted case would launch on host memory")

B, C, HS, WS = 2, 3, (20, 10), (40, 20)


def ws_floats(b, c, hs, wd):
    """The header's formula: 2 per tile, then 3 planes of the SSIM positions per level."""
    th, tw = _hip.IMAGE_LOSS_TILE
    tiles = sum(b * -(-y // th) * -(-x // tw) for y, x in zip(hs, wd))
    return 2 * tiles + _hip.IMAGE_LOSS_PLANES * sum(b * c * max(y - 10, 0) * max(x - 10, 0) for y, x in zip(hs, wd))


WS_FLOATS = ws_floats(B, C, HS, WS)     # 2 * 2 * (2 * 2 + 1) + 3 * 2 * 3 * 10 * 30 = 5420 floats, 21.7 KB
STEP = 32 << 10                         # every buffer 32 KiB after the one before (the largest is 19.2 KB) ...
BIG = 64 << 10                          # ... and the workspace in a slot of its own
VP, I = ctypes.c_void_p, ctypes.c_int


def arr(t, v):
    return None if v is None else (t * len(v))(*v)


def test_prototypes_match_their_header():
    protos = parse_header(HEADER)
    assert [name for name, _, _ in protos] == NAMES
    assert mismatches(_hip.IMAGE_LOSS_PROTOTYPES, protos) == []
    others = (set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES) | set(_hip.TRIPLET_PROTOTYPES) | set(_hip.VIS_PROTOTYPES)
              | set(_hip.QUALITY_PROTOTYPES) | set(_hip.REVIEW_PROTOTYPES) | set(_hip.FLOW_QUALITY_PROTOTYPES)
              | set(_hip.MASKED_LOSS_PROTOTYPES) | set(_hip.SPARSE_AUGMENT_PROTOTYPES) | set(_hip.UNSUP_LOSS_PROTOTYPES))
    assert not set(_hip.IMAGE_LOSS_PROTOTYPES) & others
    table = dict(_hip.IMAGE_LOSS_PROTOTYPES)
    restype, argtypes = table["qpwc_image_loss_fwd"]
    assert len(argtypes) == 19 and len(table["qpwc_image_loss_bwd"][1]) == 17
    table["qpwc_image_loss_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_image_loss_fwd: 19 parameters, table has 18"]


def test_the_library_exports_the_table(hip_lib):
    for name, (restype, argtypes) in _hip.IMAGE_LOSS_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def test_the_constants_are_the_kernel_file_s():
    with open(os.path.join(ROOT, "qpwcnet_amd", "csrc", "image_loss.hip")) as f:
        src = f.read()
    assert "kImgTileH = %d, kImgTileW = %d;" % _hip.IMAGE_LOSS_TILE in src
    assert "kImgPlanes = %d;" % _hip.IMAGE_LOSS_PLANES in src


def test_workspace_formula_and_form_query(hip_lib):
    ws, kernel = hip_lib.qpwc_image_loss_workspace_floats, hip_lib.qpwc_image_loss_fwd_kernel
    h, w = arr(I, HS), arr(I, WS)
    assert ws(B, C, h, w, 2) == WS_FLOATS == 5420
    for b, c, hs, wd in ((1, 1, (1,), (1,)), (3, 4, (16, 17, 11), (32, 33, 11)), (2, 2, (10, 40), (40, 10)),
                         (8, 3, (256, 128, 64, 32, 16, 8), (512, 256, 128, 64, 32, 16))):
        assert ws(b, c, arr(I, hs), arr(I, wd), len(hs)) == ws_floats(b, c, hs, wd), (b, c, hs, wd)
    assert ws(B, C, None, w, 2) == _hip.E_NULL and ws(B, C, h, None, 2) == _hip.E_NULL
    for bad in ((0, C, h, w, 2), (B, 0, h, w, 2), (B, 5, h, w, 2), (B, C, h, w, 0), (B, C, h, w, 9),
                (B, C, arr(I, (20, 0)), w, 2), (B, C, h, arr(I, (-1, 20)), 2),
                (1 << 9, 4, arr(I, (1 << 10,)), arr(I, (1 << 10,)), 1)):               # 2^31 elements in the level
        assert ws(*bad) == _hip.E_SHAPE, bad
    assert ws((1 << 9) - 1, 4, arr(I, (1 << 10,)), arr(I, (1 << 10,)), 1) > 0
    # extents next to INT_MAX: the tile count is formed without a sum that could wrap, no product leaves 64 bits
    top = (1 << 31) - 1
    assert ws(1, 1, arr(I, (top,)), arr(I, (1,)), 1) == ws_floats(1, 1, (top,), (1,)) == 2 << 27
    assert ws(1, 1, arr(I, (1,)), arr(I, (top,)), 1) == ws_floats(1, 1, (1,), (top,)) == 2 << 26
    assert ws(1, 1, arr(I, (11,)), arr(I, (top // 11,)), 1) == ws_floats(1, 1, (11,), (top // 11,))
    for bad in ((1, 2, arr(I, (top,)), arr(I, (1,)), 1), (1, 1, arr(I, (top,)), arr(I, (2,)), 1),
                (1, 1, arr(I, (top,)), arr(I, (top,)), 1), (top, 4, arr(I, (1 << 15,)), arr(I, (1 << 15,)), 1),
                (top, 4, arr(I, (top,)), arr(I, (top,)), 1)):
        assert ws(*bad) == _hip.E_SHAPE, bad
        assert kernel(*bad) == b""
    assert kernel(1, 1, arr(I, (top,)), arr(I, (1,)), 1) == b"image_loss_fwd_kernel"
    assert kernel(B, C, h, w, 2) == b"image_loss_fwd_kernel"
    assert kernel(B, C, h, w, 9) == b"" and kernel(0, C, h, w, 2) == b"" and kernel(B, 5, h, w, 2) == b""
    assert kernel(B, C, None, w, 2) == b"" and kernel(B, C, h, None, 2) == b""
    assert kernel(B, C, arr(I, (20, 0)), w, 2) == b""


@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(12 * STEP + 2 * BIG + 256)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    return buf, base


@pytest.fixture(scope="module")
def fwd(hip_lib, mem):
    _, base = mem
    at = lambda k: base + k * STEP
    good = dict(ssim_weight=0.85, q=0.5, eps=1e-3, max_val=1.0, offset=0.5, truth=(at(0), at(1)), pred=(at(2), at(3)),
                B=B, C=C, h=HS, w=WS, pred_dtype=(_hip.F32, _hip.F32), layout=_hip.NHWC, n_levels=2, out_losses=at(4),
                out_dssim=at(5), out_charb=at(6), workspace=at(12), stream=None)
    kinds = dict(truth=VP, pred=VP, h=I, w=I, pred_dtype=I)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
        rc = hip_lib.qpwc_image_loss_fwd(*[arr(kinds[k], a[k]) if k in kinds else a[k] for k in good])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good = good
    return run


@pytest.fixture(scope="module")
def bwd(hip_lib, mem):
    _, base = mem
    at = lambda k: base + k * STEP
    good = dict(ssim_weight=0.85, q=0.5, eps=1e-3, offset=0.5, truth=(at(0), at(1)), pred=(at(2), at(3)),
                workspace=at(12), grad_losses=at(4), grad_pred=(at(7), at(8)), B=B, C=C, h=HS, w=WS,
                pred_dtype=(_hip.F32, _hip.F32), layout=_hip.NHWC, n_levels=2, stream=None)
    kinds = dict(truth=VP, pred=VP, grad_pred=VP, h=I, w=I, pred_dtype=I)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL
        rc = hip_lib.qpwc_image_loss_bwd(*[arr(kinds[k], a[k]) if k in kinds else a[k] for k in good])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good = good
    return run


@host_only
def test_a_valid_call_reaches_the_launch(fwd):
    g = fwd.good
    rc, text = fwd()
    assert rc == _hip.E_LAUNCH and text.startswith("image_loss_fwd_kernel: "), (rc, text)
    for ok in (dict(layout=_hip.NCHW), dict(pred_dtype=(_hip.F16, _hip.F32)), dict(n_levels=1), dict(ssim_weight=0.0),
               dict(ssim_weight=1.0), dict(C=1), dict(C=4, h=(16, 8), w=(32, 16)), dict(h=(1, 11), w=(1, 11)),
               dict(offset=0.0), dict(offset=-3.0), dict(max_val=255.0), dict(q=1.0),
               dict(truth=g["pred"], pred=g["truth"]), dict(truth=g["pred"])):              # inputs may overlap
        assert fwd(**ok)[0] == _hip.E_LAUNCH, ok


@host_only
def test_forward_null(fwd):
    for name in ("truth", "pred", "h", "w", "pred_dtype", "out_losses", "out_dssim", "out_charb", "workspace"):
        assert fwd(**{name: None}) == (_hip.E_NULL, name + " is null")
    g = fwd.good
    for name in ("truth", "pred"):
        assert fwd(**{name: (g[name][0], None)}) == (_hip.E_NULL, "null target or prediction at level 1")


@host_only
def test_forward_shape_layout_range_dtype(fwd):
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(B=0), dict(B=-2), dict(C=0), dict(C=5), dict(h=(0, 10)),
                dict(w=(40, -4))):
        assert fwd(**bad)[0] == _hip.E_SHAPE, bad
    assert "n_levels" in fwd(n_levels=9)[1] and "channels" in fwd(C=5)[1]
    for bad in (2, -1):
        assert fwd(layout=bad)[0] == _hip.E_LAYOUT
    nan, inf = float("nan"), float("inf")
    for bad in (dict(ssim_weight=-0.01), dict(ssim_weight=1.01), dict(ssim_weight=nan), dict(q=0.0), dict(q=-0.5),
                dict(q=nan), dict(eps=0.0), dict(eps=-1e-3), dict(eps=nan), dict(max_val=0.0), dict(max_val=-1.0),
                dict(max_val=inf), dict(max_val=nan), dict(offset=inf), dict(offset=-inf), dict(offset=nan)):
        assert fwd(**bad)[0] == _hip.E_RANGE, bad
    for bad in (_hip.U8, 3, -1):
        assert fwd(pred_dtype=(_hip.F32, bad))[0] == _hip.E_DTYPE


@host_only
def test_forward_align(fwd):
    g = fwd.good
    for name in ("truth", "pred"):
        for off in (1, 2, 3):
            assert fwd(**{name: (g[name][0], g[name][1] + off)}) == (_hip.E_ALIGN, name + "[1] must be 4-byte aligned")
        for off in (4, 8, 12):                                  # no access is wider than an element
            assert fwd(**{name: (g[name][0] + off, g[name][1])})[0] == _hip.E_LAUNCH
    assert fwd(pred=(g["pred"][0] + 2, g["pred"][1]), pred_dtype=(_hip.F16, _hip.F32))[0] == _hip.E_LAUNCH
    assert fwd(pred=(g["pred"][0] + 1, g["pred"][1]), pred_dtype=(_hip.F16, _hip.F32)) == (
        _hip.E_ALIGN, "pred[0] must be 2-byte aligned")
    assert fwd(truth=(g["truth"][0] + 2, g["truth"][1]), pred_dtype=(_hip.F16, _hip.F32))[0] == _hip.E_ALIGN   # fp32 always
    for name in ("out_losses", "out_dssim", "out_charb", "workspace"):
        assert fwd(**{name: g[name] + 2}) == (_hip.E_ALIGN, "{} must be 4-byte aligned".format(name))
        assert fwd(**{name: g[name] + 4})[0] == _hip.E_LAUNCH


@host_only
def test_forward_alias(fwd):
    g = fwd.good
    n0, n1 = B * C * 20 * 40 * 4, B * C * 10 * 20 * 4
    assert fwd(out_losses=g["truth"][0] + n0 - 4) == (_hip.E_ALIAS, "out_losses overlaps truth[0]")
    assert fwd(out_losses=g["truth"][0] + n0)[0] == _hip.E_LAUNCH                                    # adjacent is fine
    assert fwd(out_dssim=g["pred"][1]) == (_hip.E_ALIAS, "out_dssim overlaps pred[1]")
    assert fwd(out_charb=g["pred"][1] + n1 - 4) == (_hip.E_ALIAS, "out_charb overlaps pred[1]")
    assert fwd(out_charb=g["pred"][1] + n1)[0] == _hip.E_LAUNCH
    assert fwd(pred_dtype=(_hip.F32, _hip.F16), out_charb=g["pred"][1] + n1 // 2)[0] == _hip.E_LAUNCH
    assert fwd(workspace=g["pred"][0]) == (_hip.E_ALIAS, "workspace overlaps pred[0]")
    # the outputs among themselves
    assert fwd(out_dssim=g["out_losses"]) == (_hip.E_ALIAS, "out_dssim overlaps out_losses")
    assert fwd(out_charb=g["out_dssim"] + 4) == (_hip.E_ALIAS, "out_charb overlaps out_dssim")
    assert fwd(out_charb=g["out_dssim"] + 8)[0] == _hip.E_LAUNCH
    assert fwd(out_losses=g["workspace"] + WS_FLOATS * 4 - 4) == (_hip.E_ALIAS, "workspace overlaps out_losses")
    assert fwd(out_losses=g["workspace"] + WS_FLOATS * 4)[0] == _hip.E_LAUNCH
    with pytest.raises(ValueError, match="overlaps"):
        _hip.check(fwd(out_dssim=g["out_losses"])[0])


@host_only
def test_forward_order_of_the_checks(fwd):
    """null, shape, layout, range, dtype, the per-level nulls, alignment, overlap: the first defect answers."""
    g = fwd.good
    assert fwd(workspace=None, n_levels=0)[0] == _hip.E_NULL
    assert fwd(n_levels=0, layout=7)[0] == _hip.E_SHAPE
    assert fwd(C=5, ssim_weight=2.0)[0] == _hip.E_SHAPE
    assert fwd(layout=7, q=-1.0)[0] == _hip.E_LAYOUT
    assert fwd(q=-1.0, pred_dtype=(7, 0))[0] == _hip.E_RANGE
    assert fwd(pred_dtype=(7, 0), truth=(None, g["truth"][1]))[0] == _hip.E_DTYPE
    assert fwd(truth=(None, g["truth"][1]), pred=(g["pred"][0] + 2, g["pred"][1]))[0] == _hip.E_NULL
    assert fwd(pred=(g["pred"][0] + 2, g["pred"][1]), out_dssim=g["out_losses"])[0] == _hip.E_ALIGN


@host_only
def test_backward(bwd):
    g = bwd.good
    rc, text = bwd()
    assert rc == _hip.E_LAUNCH and text.startswith("image_loss_bwd_kernel: "), (rc, text)
    for ok in (dict(n_levels=1), dict(pred_dtype=(_hip.F16, _hip.F16)), dict(layout=_hip.NCHW), dict(ssim_weight=0.0),
               dict(ssim_weight=1.0), dict(C=1), dict(h=(1, 11), w=(1, 11))):
        assert bwd(**ok)[0] == _hip.E_LAUNCH, ok
    for name in ("truth", "pred", "workspace", "grad_losses", "grad_pred", "h", "w", "pred_dtype"):
        assert bwd(**{name: None}) == (_hip.E_NULL, name + " is null")
    for name in ("truth", "pred", "grad_pred"):
        assert bwd(**{name: (g[name][0], None)}) == (_hip.E_NULL, "null buffer at level 1")
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(B=0), dict(C=5), dict(h=(20, 0))):
        assert bwd(**bad)[0] == _hip.E_SHAPE, bad
    assert bwd(layout=3)[0] == _hip.E_LAYOUT
    nan = float("nan")
    for bad in (dict(ssim_weight=1.5), dict(ssim_weight=nan), dict(q=0.0), dict(eps=0.0), dict(eps=nan),
                dict(offset=float("inf")), dict(offset=nan)):
        assert bwd(**bad)[0] == _hip.E_RANGE, bad
    assert bwd(pred_dtype=(_hip.F32, _hip.U8))[0] == _hip.E_DTYPE
    assert bwd(grad_losses=g["grad_losses"] + 2) == (_hip.E_ALIGN, "grad_losses must be 4-byte aligned")
    assert bwd(workspace=g["workspace"] + 2) == (_hip.E_ALIGN, "workspace must be 4-byte aligned")
    assert bwd(truth=(g["truth"][0] + 2, g["truth"][1])) == (_hip.E_ALIGN, "truth[0] must be 4-byte aligned")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][1] + 2)) == (_hip.E_ALIGN, "grad_pred[1] must be 4-byte aligned")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][1] + 2), pred_dtype=(_hip.F32, _hip.F16))[0] == _hip.E_LAUNCH
    assert bwd(grad_pred=(g["grad_pred"][0] + 4, g["grad_pred"][1]))[0] == _hip.E_LAUNCH
    assert bwd(grad_pred=(g["pred"][1], g["grad_pred"][1])) == (_hip.E_ALIAS, "grad_pred[0] overlaps pred[1]")
    assert bwd(grad_pred=(g["truth"][0], g["grad_pred"][1])) == (_hip.E_ALIAS, "grad_pred[0] overlaps truth[0]")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_losses"])) == (_hip.E_ALIAS, "grad_pred[1] overlaps grad_losses")
    assert bwd(grad_pred=(g["workspace"] + 64, g["grad_pred"][1])) == (_hip.E_ALIAS, "grad_pred[0] overlaps workspace")
    n0 = B * C * 20 * 40 * 4
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][0] + n0 - 4)) == (_hip.E_ALIAS, "grad_pred[1] overlaps grad_pred[0]")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][0] + n0))[0] == _hip.E_LAUNCH
    # the order: null, shape, layout, range, dtype, the per-level nulls, alignment, overlap
    assert bwd(grad_losses=None, n_levels=0)[0] == _hip.E_NULL and bwd(n_levels=0, layout=7)[0] == _hip.E_SHAPE
    assert bwd(layout=7, eps=0.0)[0] == _hip.E_LAYOUT and bwd(eps=0.0, pred_dtype=(7, 0))[0] == _hip.E_RANGE
    assert bwd(pred_dtype=(7, 0), pred=(None, g["pred"][1]))[0] == _hip.E_DTYPE
    assert bwd(pred=(None, g["pred"][1]), grad_losses=g["grad_losses"] + 2)[0] == _hip.E_NULL
    assert bwd(grad_losses=g["grad_losses"] + 2, grad_pred=(g["truth"][0], g["grad_pred"][1]))[0] == _hip.E_ALIGN

"""The argument validation of qpwc_masked_loss_fwd / qpwc_masked_loss_bwd (include/qpwc_masked_loss.h), code by code, with
HOST pointers: validation only looks at the values of the pointers and comes before any HIP call.  Without a device a call
that passes it fails at the launch (QPWC_E_LAUNCH); with a device it would launch on host memory, so the module skips
itself there, as tests/test_flow_quality_capi_cpu.py does.  The header and the table are held in
tests/test_masked_loss_cpu.py."""
import ctypes
import itertools

import pytest
import torch

from qpwcnet_amd import _hip

if torch.cuda.is_available():
    pytest.skip("host pointers: a wrongly accepted case would launch on host memory", allow_module_level=True)

B, H, W = 1, 32, 32
HS, WS = (16, 8), (16, 8)       # two levels: area factors 2 and 4 of one 32 x 32 tile
STEP = 16 << 10                 # every buffer 16 KiB after the one before ...
WS_FLOATS = 2 * 2 * _hip.MASKED_LOSS_TILE_BLOCKS
BIG = 64 << 10                  # ... and the workspace (32 KiB) in a slot of its own
VP, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
KINDS = (_hip.LOSS_FLOW_MSE_V2, _hip.LOSS_FLOW_MSE, _hip.LOSS_FLOW_FINETUNE)


def arr(t, v):
    return None if v is None else (t * len(v))(*v)


@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(14 * STEP + BIG + 256)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    return buf, base


@pytest.fixture(scope="module")
def fwd(hip_lib, mem):
    _, base = mem
    at = lambda k: base + k * STEP
    good = dict(kind=0, p0=0.1, p1=0.0, y_true=at(0), valid=at(1), B=B, H=H, W=W, C=2, layout=_hip.NHWC,
                y_pred=(at(2), at(3)), h=HS, w=WS, pred_dtype=(_hip.F32, _hip.F32), n_levels=2, out_losses=at(4),
                out_counts=at(5), dpred=(at(6), at(7)), gt_out=(at(8), at(9)), valid_out=(at(10), at(11)),
                workspace=at(14), stream=None)
    kinds = dict(y_pred=VP, h=I, w=I, pred_dtype=I, dpred=VP, gt_out=VP, valid_out=VP)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
        rc = hip_lib.qpwc_masked_loss_fwd(*[arr(kinds[k], a[k]) if k in kinds else a[k] for k in good])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good = good
    return run


@pytest.fixture(scope="module")
def bwd(hip_lib, mem):
    _, base = mem
    at = lambda k: base + k * STEP
    good = dict(kind=0, dpred=(at(0), at(1)), counts=at(2), grad_losses=at(3), grad_pred=(at(4), at(5)), n_elems=(64, 16),
                pred_dtype=(_hip.F32, _hip.F32), n_levels=2, stream=None)
    kinds = dict(dpred=VP, grad_pred=VP, n_elems=I64, pred_dtype=I)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL
        rc = hip_lib.qpwc_masked_loss_bwd(*[arr(kinds[k], a[k]) if k in kinds else a[k] for k in good])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good = good
    return run


def test_a_valid_call_reaches_the_launch_in_every_optional_pointer_combination(fwd):
    g = fwd.good
    rc, text = fwd()
    assert rc == _hip.E_LAUNCH and text.startswith("masked_loss_tile_kernel: "), (rc, text)
    for kind in KINDS:
        for valid, dpred, gt_out, valid_out in itertools.product((g["valid"], None), (g["dpred"], None),
                                                                 (g["gt_out"], None), (g["valid_out"], None)):
            rc, text = fwd(kind=kind, valid=valid, dpred=dpred, gt_out=gt_out, valid_out=valid_out)
            name = "masked_loss_tile_kernel" if kind == _hip.LOSS_FLOW_MSE_V2 else "masked_loss_pixel_kernel"
            assert rc == _hip.E_LAUNCH and text.startswith(name + ": "), (kind, rc, text)
    for ok in (dict(layout=_hip.NCHW), dict(pred_dtype=(_hip.F16, _hip.F32)), dict(p0=0.0),
               dict(gt_out=(None, g["gt_out"][1])), dict(valid_out=(g["valid_out"][0], None)),      # entries are optional
               dict(y_pred=(None, g["y_pred"][1]), dpred=None),                                       # gt_out stands in
               dict(y_pred=(None, None), dpred=None, gt_out=None),                                    # valid_out does too
               dict(n_levels=1), dict(kind=1, h=(3, 5), w=(7, 1)), dict(kind=1, p0=-1.0)):
        assert fwd(**ok)[0] == _hip.E_LAUNCH, ok
    # a shape the tile kernel does not take
    rc, text = fwd(h=(16, 32), w=(16, 32))
    assert rc == _hip.E_LAUNCH and text.startswith("masked_loss_pixel_kernel: ")


def test_forward_null(fwd):
    for name in ("y_true", "y_pred", "pred_dtype", "out_losses", "out_counts", "workspace", "h", "w"):
        assert fwd(**{name: None}) == (_hip.E_NULL, name + " is null")
    g = fwd.good
    rc, text = fwd(y_pred=(g["y_pred"][0], None), gt_out=None, valid_out=None)
    assert rc == _hip.E_NULL and text == "null prediction at level 1"
    rc, text = fwd(dpred=(None, g["dpred"][1]))
    assert rc == _hip.E_NULL and text == "null dpred buffer at level 0"


def test_forward_mode_shape_layout_range_dtype(fwd):
    for bad in (_hip.LOSS_AUTORESIZE_MSE, -1, 4):
        rc, text = fwd(kind=bad)
        assert rc == _hip.E_MODE and "three flow losses" in text
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(B=0), dict(H=-1), dict(W=0), dict(C=3), dict(C=1),
                dict(h=(0, 8)), dict(w=(16, -4)), dict(h=(3, 8)), dict(w=(16, 5))):
        assert fwd(**bad)[0] == _hip.E_SHAPE, bad
    assert "whole-block" in fwd(h=(3, 8))[1] and "n_levels" in fwd(n_levels=9)[1]
    assert fwd(kind=1, h=(3, 8))[0] == _hip.E_LAUNCH                 # the bilinear kinds resize to any extent
    for bad in (2, -1):
        assert fwd(layout=bad)[0] == _hip.E_LAYOUT
    for bad in (-0.1, float("nan")):
        rc, text = fwd(p0=bad)
        assert rc == _hip.E_RANGE and "delta" in text
    for bad in (_hip.U8, 3, -1):
        assert fwd(pred_dtype=(_hip.F32, bad))[0] == _hip.E_DTYPE


def test_forward_align(fwd):
    g = fwd.good
    for off in (1, 2, 4, 8, 12):
        assert fwd(y_true=g["y_true"] + off) == (_hip.E_ALIGN, "y_true must be 16-byte aligned")
    assert fwd(y_true=g["y_true"] + 16)[0] == _hip.E_LAUNCH
    for kind in KINDS:                                              # whichever kernel the call would take
        assert fwd(kind=kind, y_true=g["y_true"] + 8)[0] == _hip.E_ALIGN
    for off in (1, 2, 3):
        assert fwd(valid=g["valid"] + off) == (_hip.E_ALIGN, "valid must be 4-byte aligned")
    assert fwd(valid=g["valid"] + 4)[0] == _hip.E_LAUNCH
    assert fwd(y_pred=(g["y_pred"][0] + 2, g["y_pred"][1])) == (_hip.E_ALIGN, "y_pred[0] must be 4-byte aligned")
    assert fwd(y_pred=(g["y_pred"][0] + 2, g["y_pred"][1]), pred_dtype=(_hip.F16, _hip.F32))[0] == _hip.E_LAUNCH
    assert fwd(y_pred=(g["y_pred"][0] + 1, g["y_pred"][1]), pred_dtype=(_hip.F16, _hip.F32))[0] == _hip.E_ALIGN
    for name, grid in (("out_losses", 4), ("out_counts", 8), ("workspace", 4)):
        assert fwd(**{name: g[name] + grid // 2}) == (_hip.E_ALIGN, "{} must be {}-byte aligned".format(name, grid))
        assert fwd(**{name: g[name] + grid})[0] == _hip.E_LAUNCH
    assert fwd(dpred=(g["dpred"][0], g["dpred"][1] + 2)) == (_hip.E_ALIGN, "dpred[1] must be 4-byte aligned")
    assert fwd(gt_out=(g["gt_out"][0] + 1, g["gt_out"][1])) == (_hip.E_ALIGN, "gt_out[0] must be 4-byte aligned")
    assert fwd(valid_out=(g["valid_out"][0] + 1, g["valid_out"][1] + 3))[0] == _hip.E_LAUNCH         # bytes


def test_forward_alias(fwd):
    g = fwd.good
    n_gt, n_mask, n_p0, n_p1 = B * H * W * 8, B * H * W, B * HS[0] * WS[0] * 8, B * HS[1] * WS[1] * 8
    assert fwd(out_losses=g["y_true"] + n_gt - 4) == (_hip.E_ALIAS, "out_losses overlaps y_true")
    assert fwd(out_losses=g["y_true"] + n_gt)[0] == _hip.E_LAUNCH                                    # adjacent is fine
    assert fwd(out_counts=g["valid"] + n_mask - 8) == (_hip.E_ALIAS, "out_counts overlaps valid")
    assert fwd(out_counts=g["valid"] + n_mask)[0] == _hip.E_LAUNCH
    assert fwd(valid=None, out_counts=g["valid"])[0] == _hip.E_LAUNCH                                # no mask: no compare
    assert fwd(workspace=g["y_pred"][1]) == (_hip.E_ALIAS, "workspace overlaps y_pred[1]")
    assert fwd(dpred=(g["y_pred"][0] + n_p0 - 4, g["dpred"][1])) == (_hip.E_ALIAS, "dpred[0] overlaps y_pred[0]")
    assert fwd(dpred=(g["y_pred"][0] + n_p0, g["dpred"][1]))[0] == _hip.E_LAUNCH
    assert fwd(pred_dtype=(_hip.F16, _hip.F32), dpred=(g["y_pred"][0] + n_p0 // 2, g["dpred"][1]))[0] == _hip.E_LAUNCH
    assert fwd(gt_out=(g["gt_out"][0], g["y_true"])) == (_hip.E_ALIAS, "gt_out[1] overlaps y_true")
    assert fwd(valid_out=(g["valid"] + n_mask - 1, g["valid_out"][1])) == (_hip.E_ALIAS, "valid_out[0] overlaps valid")
    assert fwd(valid_out=(g["valid"] + n_mask, g["valid_out"][1]))[0] == _hip.E_LAUNCH
    # the outputs among themselves
    assert fwd(out_counts=g["out_losses"]) == (_hip.E_ALIAS, "out_counts overlaps out_losses")
    assert fwd(out_losses=g["workspace"] + WS_FLOATS * 4 - 4) == (_hip.E_ALIAS, "workspace overlaps out_losses")
    assert fwd(out_losses=g["workspace"] + WS_FLOATS * 4)[0] == _hip.E_LAUNCH
    assert fwd(gt_out=(g["dpred"][0] + 4, g["gt_out"][1])) == (_hip.E_ALIAS, "gt_out[0] overlaps dpred[0]")
    assert fwd(valid_out=(g["valid_out"][0], g["gt_out"][1] + n_p1 - 1)) == (_hip.E_ALIAS, "valid_out[1] overlaps gt_out[1]")
    assert fwd(dpred=(g["dpred"][0], g["dpred"][0] + n_p0 - 4)) == (_hip.E_ALIAS, "dpred[1] overlaps dpred[0]")
    assert fwd(y_pred=(g["y_true"], g["valid"]))[0] == _hip.E_LAUNCH                                 # inputs may overlap
    with pytest.raises(ValueError, match="overlaps"):
        _hip.check(fwd(out_counts=g["out_losses"])[0])


def test_forward_order_of_the_checks(fwd):
    """null, mode, shape, layout, range, dtype, the per-level nulls, alignment, overlap: the first defect answers."""
    g = fwd.good
    assert fwd(workspace=None, kind=3)[0] == _hip.E_NULL
    assert fwd(kind=3, n_levels=0)[0] == _hip.E_MODE
    assert fwd(n_levels=0, layout=7)[0] == _hip.E_SHAPE
    assert fwd(layout=7, p0=-1.0)[0] == _hip.E_LAYOUT
    assert fwd(p0=-1.0, pred_dtype=(7, 0))[0] == _hip.E_RANGE
    assert fwd(pred_dtype=(7, 0), dpred=(None, g["dpred"][1]))[0] == _hip.E_DTYPE
    assert fwd(dpred=(None, g["dpred"][1]), y_true=g["y_true"] + 4)[0] == _hip.E_NULL
    assert fwd(y_true=g["y_true"] + 4, out_counts=g["out_losses"])[0] == _hip.E_ALIGN


def test_backward(bwd):
    g = bwd.good
    rc, text = bwd()
    assert rc == _hip.E_LAUNCH and text.startswith("masked_loss_bwd_kernel: "), (rc, text)
    for ok in (dict(kind=1), dict(kind=2), dict(n_levels=1), dict(pred_dtype=(_hip.F16, _hip.F16)), dict(n_elems=(63, 1))):
        assert bwd(**ok)[0] == _hip.E_LAUNCH, ok
    for name in ("dpred", "counts", "grad_losses", "grad_pred", "n_elems", "pred_dtype"):
        assert bwd(**{name: None}) == (_hip.E_NULL, name + " is null")
    assert bwd(dpred=(g["dpred"][0], None))[0] == _hip.E_NULL and bwd(grad_pred=(None, g["grad_pred"][1]))[0] == _hip.E_NULL
    for bad in (_hip.LOSS_AUTORESIZE_MSE, -1):
        assert bwd(kind=bad)[0] == _hip.E_MODE
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(n_elems=(64, 0))):
        assert bwd(**bad)[0] == _hip.E_SHAPE, bad
    assert bwd(pred_dtype=(_hip.F32, _hip.U8))[0] == _hip.E_DTYPE
    assert bwd(counts=g["counts"] + 4) == (_hip.E_ALIGN, "counts must be 8-byte aligned")
    assert bwd(grad_losses=g["grad_losses"] + 2) == (_hip.E_ALIGN, "grad_losses must be 4-byte aligned")
    assert bwd(dpred=(g["dpred"][0] + 8, g["dpred"][1])) == (_hip.E_ALIGN, "dpred[0] must be 16-byte aligned")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][1] + 8)) == (_hip.E_ALIGN, "grad_pred[1] must be 16-byte aligned")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][1] + 8), pred_dtype=(_hip.F32, _hip.F16))[0] == _hip.E_LAUNCH
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][1] + 4), pred_dtype=(_hip.F32, _hip.F16)) == (
        _hip.E_ALIGN, "grad_pred[1] must be 8-byte aligned")
    assert bwd(grad_pred=(g["dpred"][1], g["grad_pred"][1])) == (_hip.E_ALIAS, "grad_pred[0] overlaps dpred[1]")
    assert bwd(grad_pred=(g["counts"], g["grad_pred"][1])) == (_hip.E_ALIAS, "grad_pred[0] overlaps counts")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_losses"])) == (_hip.E_ALIAS, "grad_pred[1] overlaps grad_losses")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][0] + 64 * 4 - 16)) == (
        _hip.E_ALIAS, "grad_pred[1] overlaps grad_pred[0]")
    assert bwd(grad_pred=(g["grad_pred"][0], g["grad_pred"][0] + 64 * 4))[0] == _hip.E_LAUNCH
    assert bwd(dpred=(g["dpred"][0], g["dpred"][0]))[0] == _hip.E_LAUNCH                             # inputs may overlap


def test_queries(hip_lib):
    ws, kernel = hip_lib.qpwc_masked_loss_workspace_floats, hip_lib.qpwc_masked_loss_fwd_kernel
    h, w = arr(I, HS), arr(I, WS)
    assert ws(0, B, H, W, 2, h, w, 2) == WS_FLOATS
    assert ws(_hip.LOSS_AUTORESIZE_MSE, B, H, W, 2, h, w, 2) == _hip.E_MODE
    assert ws(0, B, H, W, 2, h, w, 0) == _hip.E_SHAPE and ws(0, B, H, W, 2, None, w, 2) == _hip.E_NULL
    assert kernel(0, B, H, W, 2, h, w, 2) == b"masked_loss_tile_kernel"
    assert kernel(0, 1, 8, 16, 2, arr(I, (4, 2)), arr(I, (8, 4)), 2) == b"masked_loss_pixel_kernel"   # no 32 x 32 tile
    assert kernel(0, 1, 32, 32, 2, arr(I, (16, 8)), arr(I, (16, 8)), 2) == b"masked_loss_tile_kernel"
    assert kernel(1, 1, 32, 32, 2, arr(I, (16, 8)), arr(I, (16, 8)), 2) == b"masked_loss_pixel_kernel"
    assert kernel(3, 1, 32, 32, 2, arr(I, (16, 8)), arr(I, (16, 8)), 2) == b""
    assert kernel(0, 1, 32, 32, 3, arr(I, (16, 8)), arr(I, (16, 8)), 2) == b""

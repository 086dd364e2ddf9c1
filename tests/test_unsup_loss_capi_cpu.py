"""The C boundary of the label-free losses (include/qpwc_unsup_loss.h): the ctypes table against the header, the workspace
formula and the form query, and the argument validation of qpwc_unsup_loss_fwd / qpwc_unsup_loss_bwd code by code, with HOST
pointers: validation only looks at the values of the pointers and comes before any HIP call.  Without a device a call that
passes it fails at the launch (QPWC_E_LAUNCH); with a device it would launch on host memory, so those tests skip
themselves there, as tests/test_masked_loss_capi_cpu.py does."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

from qpwcnet_amd import _hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qpwc_unsup_loss.h")
NAMES = ["qpwc_unsup_loss_workspace_floats", "qpwc_unsup_loss_fwd", "qpwc_unsup_loss_fwd_kernel", "qpwc_unsup_loss_bwd"]
host_only = pytest.mark.skipif(torch.cuda.is_available(),
                               reason="host pointers: a wrongly accepted case would launch on host memory")

B, HS, WS = 2, (12, 6), (40, 20)
TILES = B * (2 * 2 + 1 * 1)     # tiles of 8 x 32: 12 x 40 -> 2 x 2, 6 x 20 -> 1 x 1
WS_FLOATS = 4 * TILES + _hip.UNSUP_LOSS_PLANES * B * (12 * 40 + 6 * 20)
STEP = 16 << 10                 # every buffer 16 KiB after the one before ...
BIG = 64 << 10                  # ... and the workspace (33.8 KB) in a slot of its own
VP, I = ctypes.c_void_p, ctypes.c_int


def arr(t, v):
    return None if v is None else (t * len(v))(*v)


def test_prototypes_match_their_header():
    protos = parse_header(HEADER)
    assert [name for name, _, _ in protos] == NAMES
    assert mismatches(_hip.UNSUP_LOSS_PROTOTYPES, protos) == []
    others = (set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES) | set(_hip.TRIPLET_PROTOTYPES) | set(_hip.VIS_PROTOTYPES)
              | set(_hip.QUALITY_PROTOTYPES) | set(_hip.REVIEW_PROTOTYPES) | set(_hip.FLOW_QUALITY_PROTOTYPES)
              | set(_hip.MASKED_LOSS_PROTOTYPES) | set(_hip.SPARSE_AUGMENT_PROTOTYPES))
    assert not set(_hip.UNSUP_LOSS_PROTOTYPES) & others
    table = dict(_hip.UNSUP_LOSS_PROTOTYPES)
    restype, argtypes = table["qpwc_unsup_loss_fwd"]
    assert len(argtypes) == 22
    table["qpwc_unsup_loss_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_unsup_loss_fwd: 22 parameters, table has 21"]
    with open(HEADER) as f:
        text = f.read()
    assert "#define QPWC_UNSUP_CENSUS %d" % _hip.UNSUP_CENSUS in text
    assert "#define QPWC_UNSUP_CHARBONNIER %d" % _hip.UNSUP_CHARBONNIER in text


def test_the_library_exports_the_table(hip_lib):
    for name, (restype, argtypes) in _hip.UNSUP_LOSS_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def test_the_constants_are_the_kernel_file_s():
    with open(os.path.join(ROOT, "qpwcnet_amd", "csrc", "unsup_loss.hip")) as f:
        src = f.read()
    assert "kUnsupTileH = %d, kUnsupTileW = %d;" % _hip.UNSUP_LOSS_TILE in src
    assert "kUnsupPlanes = %d;" % _hip.UNSUP_LOSS_PLANES in src


def test_workspace_formula_and_form_query(hip_lib):
    ws, kernel = hip_lib.qpwc_unsup_loss_workspace_floats, hip_lib.qpwc_unsup_loss_fwd_kernel
    h, w = arr(I, HS), arr(I, WS)
    th, tw = _hip.UNSUP_LOSS_TILE
    assert ws(0, B, h, w, 2) == WS_FLOATS == ws(1, B, h, w, 2)
    for b, hs, wd in ((1, (1,), (1,)), (3, (8, 9), (32, 33)), (8, (256, 128, 64, 32, 16, 8), (512, 256, 128, 64, 32, 16))):
        tiles = sum(b * -(-y // th) * -(-x // tw) for y, x in zip(hs, wd))
        want = 4 * tiles + _hip.UNSUP_LOSS_PLANES * sum(b * y * x for y, x in zip(hs, wd))
        assert ws(0, b, arr(I, hs), arr(I, wd), len(hs)) == want
    assert ws(2, B, h, w, 2) == _hip.E_MODE and ws(-1, B, h, w, 2) == _hip.E_MODE
    assert ws(0, B, None, w, 2) == _hip.E_NULL and ws(0, B, h, None, 2) == _hip.E_NULL
    for bad in ((0, h, w, 2), (B, h, w, 0), (B, h, w, 9), (B, arr(I, (12, 0)), w, 2), (B, h, arr(I, (-1, 20)), 2),
                (1 << 20, arr(I, (1 << 10,)), arr(I, (1 << 10,)), 1)):
        assert ws(0, *bad) == _hip.E_SHAPE, bad
    assert kernel(0, B, h, w, 2) == b"unsup_loss_fwd_kernel<census>"
    assert kernel(1, B, h, w, 2) == b"unsup_loss_fwd_kernel<charbonnier>"
    assert kernel(2, B, h, w, 2) == b"" and kernel(0, B, h, w, 9) == b"" and kernel(0, 0, h, w, 2) == b""
    assert kernel(0, B, None, w, 2) == b""


@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(16 * STEP + 2 * BIG + 256)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    return buf, base


@pytest.fixture(scope="module")
def fwd(hip_lib, mem):
    _, base = mem
    at = lambda k: base + k * STEP
    good = dict(kind=0, q=0.4, eps=0.01, smooth_weight=2.0, edge=150.0, smooth_eps=1e-3, prv=(at(0), at(1)),
                nxt=(at(2), at(3)), flow=(at(4), at(5)), occluded=(at(6), at(7)), B=B, h=HS, w=WS,
                flow_dtype=(_hip.F32, _hip.F32), layout=_hip.NHWC, n_levels=2, out_losses=at(8), out_photo=at(9),
                out_smooth=at(10), out_counts=at(11), workspace=at(16), stream=None)
    kinds = dict(prv=VP, nxt=VP, flow=VP, occluded=VP, h=I, w=I, flow_dtype=I)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
        rc = hip_lib.qpwc_unsup_loss_fwd(*[arr(kinds[k], a[k]) if k in kinds else a[k] for k in good])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good = good
    return run


@pytest.fixture(scope="module")
def bwd(hip_lib, mem):
    _, base = mem
    at = lambda k: base + k * STEP
    good = dict(kind=0, smooth_weight=2.0, smooth_eps=1e-3, flow=(at(4), at(5)), workspace=at(16), counts=at(11),
                grad_losses=at(8), grad_flow=(at(12), at(13)), B=B, h=HS, w=WS, flow_dtype=(_hip.F32, _hip.F32),
                layout=_hip.NHWC, n_levels=2, stream=None)
    kinds = dict(flow=VP, grad_flow=VP, h=I, w=I, flow_dtype=I)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL
        rc = hip_lib.qpwc_unsup_loss_bwd(*[arr(kinds[k], a[k]) if k in kinds else a[k] for k in good])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good = good
    return run


@host_only
def test_a_valid_call_reaches_the_launch(fwd):
    g = fwd.good
    rc, text = fwd()
    assert rc == _hip.E_LAUNCH and text.startswith("unsup_loss_fwd_kernel<census>: "), (rc, text)
    rc, text = fwd(kind=1)
    assert rc == _hip.E_LAUNCH and text.startswith("unsup_loss_fwd_kernel<charbonnier>: "), (rc, text)
    for ok in (dict(occluded=None), dict(occluded=(None, g["occluded"][1])), dict(layout=_hip.NCHW),
               dict(flow_dtype=(_hip.F16, _hip.F32)), dict(n_levels=1), dict(smooth_weight=0.0), dict(edge=0.0),
               dict(h=(1, 7), w=(1, 3)), dict(prv=g["nxt"], nxt=g["prv"]), dict(prv=g["nxt"])):     # inputs may overlap
        assert fwd(**ok)[0] == _hip.E_LAUNCH, ok


@host_only
def test_forward_null(fwd):
    for name in ("prv", "nxt", "flow", "h", "w", "flow_dtype", "out_losses", "out_photo", "out_smooth", "out_counts",
                 "workspace"):
        assert fwd(**{name: None}) == (_hip.E_NULL, name + " is null")
    g = fwd.good
    for name in ("prv", "nxt", "flow"):
        assert fwd(**{name: (g[name][0], None)}) == (_hip.E_NULL, "null frame or flow at level 1")


@host_only
def test_forward_mode_shape_layout_range_dtype(fwd):
    for bad in (2, -1):
        rc, text = fwd(kind=bad)
        assert rc == _hip.E_MODE and "photometric kind" in text
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(B=0), dict(B=-2), dict(h=(0, 6)), dict(w=(40, -4))):
        assert fwd(**bad)[0] == _hip.E_SHAPE, bad
    assert "n_levels" in fwd(n_levels=9)[1]
    for bad in (2, -1):
        assert fwd(layout=bad)[0] == _hip.E_LAYOUT
    nan = float("nan")
    for bad in (dict(q=0.0), dict(q=-0.4), dict(q=nan), dict(eps=0.0), dict(eps=nan), dict(smooth_eps=0.0),
                dict(smooth_eps=-1e-3), dict(smooth_eps=nan), dict(edge=-1.0), dict(edge=nan), dict(smooth_weight=-0.1),
                dict(smooth_weight=nan)):
        assert fwd(**bad)[0] == _hip.E_RANGE, bad
    for bad in (_hip.U8, 3, -1):
        assert fwd(flow_dtype=(_hip.F32, bad))[0] == _hip.E_DTYPE


@host_only
def test_forward_align(fwd):
    g = fwd.good
    for name in ("prv", "nxt", "flow"):
        for off in (1, 2, 3):
            assert fwd(**{name: (g[name][0], g[name][1] + off)}) == (_hip.E_ALIGN, name + "[1] must be 4-byte aligned")
        for off in (4, 8, 12):                                  # no access is wider than an element
            assert fwd(**{name: (g[name][0] + off, g[name][1])})[0] == _hip.E_LAUNCH
    assert fwd(flow=(g["flow"][0] + 2, g["flow"][1]), flow_dtype=(_hip.F16, _hip.F32))[0] == _hip.E_LAUNCH
    assert fwd(flow=(g["flow"][0] + 1, g["flow"][1]), flow_dtype=(_hip.F16, _hip.F32)) == (
        _hip.E_ALIGN, "flow[0] must be 2-byte aligned")
    assert fwd(occluded=(g["occluded"][0] + 1, g["occluded"][1] + 3))[0] == _hip.E_LAUNCH            # bytes
    for name, grid in (("out_losses", 4), ("out_photo", 4), ("out_smooth", 4), ("out_counts", 8), ("workspace", 4)):
        assert fwd(**{name: g[name] + grid // 2}) == (_hip.E_ALIGN, "{} must be {}-byte aligned".format(name, grid))
        assert fwd(**{name: g[name] + grid})[0] == _hip.E_LAUNCH


@host_only
def test_forward_alias(fwd):
    g = fwd.good
    n_img, n_flow, n_occ = B * 12 * 40 * 12, B * 6 * 20 * 8, B * 12 * 40
    assert fwd(out_losses=g["prv"][0] + n_img - 4) == (_hip.E_ALIAS, "out_losses overlaps prv[0]")
    assert fwd(out_losses=g["prv"][0] + n_img)[0] == _hip.E_LAUNCH                                   # adjacent is fine
    assert fwd(out_photo=g["nxt"][1]) == (_hip.E_ALIAS, "out_photo overlaps nxt[1]")
    assert fwd(out_smooth=g["flow"][1] + n_flow - 4) == (_hip.E_ALIAS, "out_smooth overlaps flow[1]")
    assert fwd(out_smooth=g["flow"][1] + n_flow)[0] == _hip.E_LAUNCH
    assert fwd(flow_dtype=(_hip.F32, _hip.F16), out_smooth=g["flow"][1] + n_flow // 2)[0] == _hip.E_LAUNCH
    assert fwd(out_counts=g["occluded"][0] + n_occ - 8) == (_hip.E_ALIAS, "out_counts overlaps occluded[0]")
    assert fwd(occluded=None, out_counts=g["occluded"][0])[0] == _hip.E_LAUNCH                       # no mask: no compare
    assert fwd(workspace=g["flow"][0]) == (_hip.E_ALIAS, "workspace overlaps flow[0]")
    # the outputs among themselves
    assert fwd(out_photo=g["out_losses"]) == (_hip.E_ALIAS, "out_photo overlaps out_losses")
    assert fwd(out_counts=g["out_smooth"]) == (_hip.E_ALIAS, "out_counts overlaps out_smooth")
    assert fwd(out_losses=g["workspace"] + WS_FLOATS * 4 - 4) == (_hip.E_ALIAS, "workspace overlaps out_losses")
    assert fwd(out_losses=g["workspace"] + WS_FLOATS * 4)[0] == _hip.E_LAUNCH
    with pytest.raises(ValueError, match="overlaps"):
        _hip.check(fwd(out_photo=g["out_losses"])[0])


@host_only
def test_forward_order_of_the_checks(fwd):
    """null, mode, shape, layout, range, dtype, the per-level nulls, alignment, overlap: the first defect answers."""
    g = fwd.good
    assert fwd(workspace=None, kind=3)[0] == _hip.E_NULL
    assert fwd(kind=3, n_levels=0)[0] == _hip.E_MODE
    assert fwd(n_levels=0, layout=7)[0] == _hip.E_SHAPE
    assert fwd(layout=7, q=-1.0)[0] == _hip.E_LAYOUT
    assert fwd(q=-1.0, flow_dtype=(7, 0))[0] == _hip.E_RANGE
    assert fwd(flow_dtype=(7, 0), prv=(None, g["prv"][1]))[0] == _hip.E_DTYPE
    assert fwd(prv=(None, g["prv"][1]), nxt=(g["nxt"][0] + 2, g["nxt"][1]))[0] == _hip.E_NULL
    assert fwd(nxt=(g["nxt"][0] + 2, g["nxt"][1]), out_photo=g["out_losses"])[0] == _hip.E_ALIGN


@host_only
def test_backward(bwd):
    g = bwd.good
    rc, text = bwd()
    assert rc == _hip.E_LAUNCH and text.startswith("unsup_loss_bwd_kernel: "), (rc, text)
    for ok in (dict(kind=1), dict(n_levels=1), dict(flow_dtype=(_hip.F16, _hip.F16)), dict(layout=_hip.NCHW),
               dict(smooth_weight=0.0)):
        assert bwd(**ok)[0] == _hip.E_LAUNCH, ok
    for name in ("flow", "workspace", "counts", "grad_losses", "grad_flow", "h", "w", "flow_dtype"):
        assert bwd(**{name: None}) == (_hip.E_NULL, name + " is null")
    assert bwd(flow=(g["flow"][0], None))[0] == _hip.E_NULL and bwd(grad_flow=(None, g["grad_flow"][1]))[0] == _hip.E_NULL
    assert bwd(kind=2)[0] == _hip.E_MODE
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(B=0), dict(h=(12, 0))):
        assert bwd(**bad)[0] == _hip.E_SHAPE, bad
    assert bwd(layout=3)[0] == _hip.E_LAYOUT
    for bad in (dict(smooth_eps=0.0), dict(smooth_eps=float("nan")), dict(smooth_weight=-1.0)):
        assert bwd(**bad)[0] == _hip.E_RANGE, bad
    assert bwd(flow_dtype=(_hip.F32, _hip.U8))[0] == _hip.E_DTYPE
    assert bwd(counts=g["counts"] + 4) == (_hip.E_ALIGN, "counts must be 8-byte aligned")
    assert bwd(grad_losses=g["grad_losses"] + 2) == (_hip.E_ALIGN, "grad_losses must be 4-byte aligned")
    assert bwd(workspace=g["workspace"] + 2) == (_hip.E_ALIGN, "workspace must be 4-byte aligned")
    assert bwd(grad_flow=(g["grad_flow"][0], g["grad_flow"][1] + 2)) == (_hip.E_ALIGN, "grad_flow[1] must be 4-byte aligned")
    assert bwd(grad_flow=(g["grad_flow"][0], g["grad_flow"][1] + 2), flow_dtype=(_hip.F32, _hip.F16))[0] == _hip.E_LAUNCH
    assert bwd(grad_flow=(g["grad_flow"][0] + 4, g["grad_flow"][1]))[0] == _hip.E_LAUNCH
    assert bwd(grad_flow=(g["flow"][1], g["grad_flow"][1])) == (_hip.E_ALIAS, "grad_flow[0] overlaps flow[1]")
    assert bwd(grad_flow=(g["counts"], g["grad_flow"][1])) == (_hip.E_ALIAS, "grad_flow[0] overlaps counts")
    assert bwd(grad_flow=(g["grad_flow"][0], g["grad_losses"])) == (_hip.E_ALIAS, "grad_flow[1] overlaps grad_losses")
    assert bwd(grad_flow=(g["workspace"] + 64, g["grad_flow"][1])) == (_hip.E_ALIAS, "grad_flow[0] overlaps workspace")
    n0 = B * 12 * 40 * 8
    assert bwd(grad_flow=(g["grad_flow"][0], g["grad_flow"][0] + n0 - 4)) == (_hip.E_ALIAS, "grad_flow[1] overlaps grad_flow[0]")
    assert bwd(grad_flow=(g["grad_flow"][0], g["grad_flow"][0] + n0))[0] == _hip.E_LAUNCH
    # the order: null, mode, shape, layout, range, dtype, the per-level nulls, alignment, overlap
    assert bwd(counts=None, kind=5)[0] == _hip.E_NULL and bwd(kind=5, n_levels=0)[0] == _hip.E_MODE
    assert bwd(n_levels=0, layout=7)[0] == _hip.E_SHAPE and bwd(layout=7, smooth_eps=0.0)[0] == _hip.E_LAYOUT
    assert bwd(smooth_eps=0.0, flow_dtype=(7, 0))[0] == _hip.E_RANGE
    assert bwd(flow_dtype=(7, 0), flow=(None, g["flow"][1]))[0] == _hip.E_DTYPE
    assert bwd(flow=(None, g["flow"][1]), counts=g["counts"] + 4)[0] == _hip.E_NULL
    assert bwd(counts=g["counts"] + 4, grad_flow=(g["counts"], g["grad_flow"][1]))[0] == _hip.E_ALIGN

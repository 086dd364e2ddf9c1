"""The C boundary of the sparse-ground-truth input pipeline (include/qpwc_sparse_augment.h) without a GPU: the header
against ``_hip.SPARSE_AUGMENT_PROTOTYPES``, the validator's codes in the order the header documents, the grids the
outputs must be on, and the launch-form query at the shapes tests/test_gpu_sparse_augment.py relies on.
The validator is called with HOST pointers: it only looks at their values and comes before any HIP call.  Without a device
a call that passes it fails at the launch (QPWC_E_LAUNCH); with one it would launch on host memory, so those tests skip
themselves there, as tests/test_flow_quality_capi_cpu.py does."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

from qpwcnet_amd import _hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qpwc_sparse_augment.h")
NAMES = ["qpwc_augment_sparse_fwd", "qpwc_augment_sparse_fwd_kernel"]
VEC, SCALAR = "augment_sparse_pixel_kernel<vec4>", "augment_sparse_pixel_kernel<scalar>"
host_pointers = pytest.mark.skipif(torch.cuda.is_available(),
                                   reason="host pointers: a wrongly accepted case would launch on host memory")


def test_prototypes_match_their_header():
    protos = parse_header(HEADER)
    assert [name for name, _, _ in protos] == NAMES
    assert mismatches(_hip.SPARSE_AUGMENT_PROTOTYPES, protos) == []
    others = (set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES) | set(_hip.TRIPLET_PROTOTYPES) | set(_hip.VIS_PROTOTYPES)
              | set(_hip.QUALITY_PROTOTYPES) | set(_hip.REVIEW_PROTOTYPES) | set(_hip.FLOW_QUALITY_PROTOTYPES)
              | set(_hip.MASKED_LOSS_PROTOTYPES))
    assert not set(_hip.SPARSE_AUGMENT_PROTOTYPES) & others
    with open(os.path.join(ROOT, "include", "qpwc.h")) as f:
        assert "augment_sparse" not in f.read()
    table = dict(_hip.SPARSE_AUGMENT_PROTOTYPES)
    restype, argtypes = table["qpwc_augment_sparse_fwd"]
    assert len(argtypes) == 18
    table["qpwc_augment_sparse_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_augment_sparse_fwd: 18 parameters, table has 17"]


def test_the_loaded_library_carries_the_prototypes(hip_lib):
    for name, (restype, argtypes) in _hip.SPARSE_AUGMENT_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)


def _buffers():
    keep = (ctypes.c_float * (1 << 16))()
    base = ctypes.cast(keep, ctypes.c_void_p).value
    base += (-base) % 256
    return keep, [base + (16 << 10) * i for i in range(9)]           # every buffer 16 KiB apart


def _caller(L, bufs, **shape):
    ims, flo, valid, ipar, fpar, o_ims, o_flo, o_valid, ws = bufs
    d = dict(ims=ims, dtype=_hip.U8, flo=flo, valid=valid, B=1, H=8, W=8, ip=ipar, fp=fpar, h=4, w=4, flags=1, layout=0,
             o_ims=o_ims, o_flo=o_flo, o_valid=o_valid, ws=ws)
    d.update(shape)

    def call(**kw):
        a = dict(d, **kw)
        return L.qpwc_augment_sparse_fwd(a["ims"], a["dtype"], a["flo"], a["valid"], a["B"], a["H"], a["W"], a["ip"],
                                         a["fp"], a["h"], a["w"], a["flags"], a["layout"], a["o_ims"], a["o_flo"],
                                         a["o_valid"], a["ws"], None)
    return call


@host_pointers
def test_argument_validation_needs_no_gpu_and_keeps_its_order(hip_lib):
    L = hip_lib
    keep, bufs = _buffers()
    ims, flo, valid, ipar, fpar, o_ims, o_flo, o_valid, ws = bufs
    call = _caller(L, bufs)                                          # 1 x 8 x 8 -> 4 x 4: the <vec4> form
    for name in ("ims", "flo", "ip", "fp", "o_ims", "o_flo", "o_valid", "ws"):
        assert call(**{name: None}) == _hip.E_NULL, name
    assert call(flags=0, ws=None) != _hip.E_NULL                     # the workspace belongs to the colour stage
    for name in ("B", "H", "W", "h", "w"):
        assert call(**{name: 0}) == _hip.E_SHAPE and call(**{name: -3}) == _hip.E_SHAPE, name
    assert b"non-positive" in L.qpwc_last_error()
    assert call(dtype=_hip.F16) == _hip.E_DTYPE and call(dtype=3) == _hip.E_DTYPE and call(dtype=-1) == _hip.E_DTYPE
    assert call(layout=2) == _hip.E_LAYOUT and call(layout=-1) == _hip.E_LAYOUT
    assert call(flags=4) == _hip.E_MODE and call(flags=-1) == _hip.E_MODE and call(flags=8 | 1) == _hip.E_MODE
    assert call(H=1 << 16, W=1 << 15) == _hip.E_SHAPE and b"overflows" in L.qpwc_last_error()
    assert call(h=1 << 15, w=1 << 14) == _hip.E_SHAPE and call(B=1 << 20, h=1 << 10, w=1 << 10) == _hip.E_SHAPE
    # the documented order: MODE, NULL, DTYPE, LAYOUT, SHAPE, ALIGN, ALIAS -- each defect hides the ones after it
    order = [("flags", 4, _hip.E_MODE), ("flo", None, _hip.E_NULL), ("dtype", 7, _hip.E_DTYPE),
             ("layout", 5, _hip.E_LAYOUT), ("W", 0, _hip.E_SHAPE), ("o_flo", o_flo + 4, _hip.E_ALIGN),
             ("o_valid", ims, _hip.E_ALIAS)]
    for i, (_, _, code) in enumerate(order):
        assert call(**{k: v for k, v, _ in order[i:]}) == code, code
    # the sources' grids are the dense entry point's; the mask is read byte by byte
    assert call(ims=ims + 1) == _hip.E_ALIGN and call(dtype=_hip.F32, ims=ims + 4) == _hip.E_ALIGN
    assert call(flo=flo + 4) == _hip.E_ALIGN and call(ip=ipar + 2) == _hip.E_ALIGN and call(fp=fpar + 2) == _hip.E_ALIGN
    assert call(ws=ws + 2) == _hip.E_ALIGN
    assert call(valid=valid + 1) == _hip.E_LAUNCH and call(valid=None) == _hip.E_LAUNCH
    # out_valid against every input, every other output and the workspace; the other outputs likewise
    for other in (ims, flo + 64, valid + 32, ipar, fpar, o_ims + 128, o_flo, ws):
        assert call(o_valid=other) == _hip.E_ALIAS, other
    assert b"out_valid" in L.qpwc_last_error() or b"workspace" in L.qpwc_last_error()
    assert call(o_ims=ims) == _hip.E_ALIAS and call(o_flo=valid) == _hip.E_ALIAS and call(o_flo=o_ims + 128) == _hip.E_ALIAS
    assert call(ws=o_valid) == _hip.E_ALIAS and call(ws=ipar) == _hip.E_ALIAS and call(ws=valid) == _hip.E_ALIAS
    assert call(flags=0, ws=o_valid) == _hip.E_LAUNCH                # without the colour stage nobody looks at it
    # a valid call gets as far as the launch
    for kw in ({}, {"flags": 0}, {"flags": 3}, {"layout": 1}, {"dtype": _hip.F32}, {"valid": None}):
        assert call(**kw) == _hip.E_LAUNCH, kw
    with pytest.raises(RuntimeError):
        _hip.check(call())
    with pytest.raises(ValueError, match="flags"):
        _hip.check(call(flags=4))
    del keep


@host_pointers
def test_outputs_off_their_grid_are_refused(hip_lib):
    keep, bufs = _buffers()
    o_ims, o_flo, o_valid = bufs[5:8]
    vec = _caller(hip_lib, bufs, h=12, w=20)                         # 240 pixels: <vec4>, 16 / 16 / 4 bytes
    for off in (4, 8, 12):
        assert vec(o_ims=o_ims + off) == _hip.E_ALIGN and vec(o_flo=o_flo + off) == _hip.E_ALIGN, off
    for off in (1, 2, 3):
        assert vec(o_valid=o_valid + off) == _hip.E_ALIGN, off
    assert b"out_valid must be 4-byte aligned" in hip_lib.qpwc_last_error()
    assert vec(o_ims=o_ims + 16, o_flo=o_flo + 32, o_valid=o_valid + 4) == _hip.E_LAUNCH
    scalar = _caller(hip_lib, bufs, h=7, w=5)                        # 35 pixels: <scalar>, element by element
    assert scalar(o_ims=o_ims + 4, o_flo=o_flo + 8, o_valid=o_valid + 3) == _hip.E_LAUNCH
    assert scalar(o_ims=o_ims + 2) == _hip.E_ALIGN and scalar(o_flo=o_flo + 1) == _hip.E_ALIGN
    del keep


def test_launch_form_follows_the_shape_alone(hip_lib):
    from qpwcnet_amd import ops
    pick = lambda B, h, w: hip_lib.qpwc_augment_sparse_fwd_kernel(B, h, w).decode()
    assert pick(1, 12, 20) == VEC and pick(1, 7, 5) == SCALAR
    assert pick(4, 16, 24) == VEC and pick(2, 64, 64) == VEC and pick(16, 256, 512) == VEC      # the GPU suite's, the trainer's
    assert pick(1, 2, 3) == SCALAR and pick(1, 2, 2) == VEC
    assert pick(0, 12, 20) == "" and pick(1, 12, 0) == "" and pick(1 << 20, 1 << 10, 1 << 10) == ""
    assert ops.augment_sparse_kernel(4, 16, 24) == VEC and ops.augment_sparse_kernel(1, 7, 5) == SCALAR
    assert ops.augment_sparse_kernel(1, -1, 5) == ""
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.augment_sparse(torch.zeros(1, 8, 8, 6, dtype=torch.uint8), torch.zeros(1, 8, 8, 2), None,
                           torch.zeros(1, 6, dtype=torch.int32), torch.zeros(1, 6), (4, 4))

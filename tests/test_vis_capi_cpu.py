"""The argument validation of qpwc_flow_to_image_fwd and its two queries (include/qpwc_vis.h), code by code, with HOST
pointers: validation only looks at the values of the pointers and comes before any HIP call.  Without a device a call
that passes it fails at the launch (QPWC_E_LAUNCH); with a device it would launch on host memory, so the module skips
itself there, as tests/test_triplet_capi_cpu.py does."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_capi_prototypes_cpu import mismatches, parse_header  # noqa: E402

from qpwcnet_amd import _hip, ops  # noqa: E402

if torch.cuda.is_available():
    pytest.skip("host pointers: a wrongly accepted case would launch on host memory", allow_module_level=True)

VIS_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qpwc_vis.h")
B = 2
H, W = (4, 8), (6, 12)          # two levels
OH, OW = (8, 8), (12, 12)
STEP = 16 << 10                 # every buffer 16 KiB after the one before
LIMIT = (1 << 31) - 1
ints = lambda v: (ctypes.c_int * max(len(v), 1))(*v)
ptrs = lambda v: (ctypes.c_void_p * max(len(v), 1))(*v)


@pytest.fixture(scope="module")
def call(hip_lib):
    buf = ctypes.create_string_buffer(6 * STEP + 256)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    good = dict(flows=[base, base + STEP], flow_dtype=[_hip.F32, _hip.F32], h=list(H), w=list(W), n=2, B=B,
                in_layout=_hip.NHWC, outs=[base + 2 * STEP, base + 3 * STEP], oh=list(OH), ow=list(OW),
                out_dtype=_hip.F32, out_layout=_hip.NHWC, ws=base + 4 * STEP, stream=None)

    def run(**changed):
        a = dict(good, **changed)
        arr = lambda key, make: None if a[key] is None else make(a[key])
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
        rc = hip_lib.qpwc_flow_to_image_fwd(arr("flows", ptrs), arr("flow_dtype", ints), arr("h", ints), arr("w", ints),
                                            a["n"], a["B"], a["in_layout"], arr("outs", ptrs), arr("oh", ints),
                                            arr("ow", ints), a["out_dtype"], a["out_layout"], a["ws"], a["stream"])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good, run.keep = good, buf
    return run


def test_a_valid_call_reaches_the_launch(call):
    rc, text = call()
    assert rc == _hip.E_LAUNCH and text.startswith("flow_mag_max_kernel: "), (rc, text)
    g = call.good
    for ok in (dict(flow_dtype=[_hip.F16, _hip.F32]), dict(out_dtype=_hip.U8), dict(in_layout=_hip.NCHW),
               dict(out_layout=_hip.NCHW), dict(oh=[5, 7], ow=[3, 9]), dict(n=1),
               dict(flows=[g["flows"][0], g["flows"][0]], h=[4, 4], w=[8, 8])):    # two flows may be one buffer
        assert call(**ok)[0] == _hip.E_LAUNCH, ok
    eight = dict(n=8, flows=[g["flows"][0]] * 8, flow_dtype=[_hip.F32] * 8, h=[2] * 8, w=[2] * 8, oh=[2] * 8, ow=[2] * 8,
                 outs=[g["outs"][0] + 256 * i for i in range(8)])
    assert call(**eight)[0] == _hip.E_LAUNCH


def test_null(call):
    for name in ("flows", "flow_dtype", "h", "w", "outs", "oh", "ow", "ws"):
        assert call(**{name: None}) == (_hip.E_NULL, name + " is null")
    g = call.good
    assert call(flows=[g["flows"][0], None]) == (_hip.E_NULL, "flows[1] is null")
    assert call(outs=[None, g["outs"][1]]) == (_hip.E_NULL, "outs[0] is null")


def test_dtype_and_layout(call):
    for bad in (_hip.U8, 3, -1):
        rc, text = call(flow_dtype=[_hip.F32, bad])
        assert rc == _hip.E_DTYPE and text.startswith("flows[1]"), text
    for bad in (_hip.F16, 3, -1):
        assert call(out_dtype=bad)[0] == _hip.E_DTYPE
    for name in ("in_layout", "out_layout"):
        for bad in (2, -1):
            rc, text = call(**{name: bad})
            assert rc == _hip.E_LAYOUT and text.startswith("Unsupported data format")


def test_shape(call):
    for bad in (0, 9, -1):
        rc, text = call(n=bad)
        assert rc == _hip.E_SHAPE and "outside [1,8]" in text, (bad, text)
    for bad in (0, -3):
        assert call(B=bad)[0] == _hip.E_SHAPE
        for name in ("h", "w", "oh", "ow"):
            rc, text = call(**{name: [call.good[name][0], bad]})
            assert rc == _hip.E_SHAPE and text.startswith("level 1: non-positive"), (name, bad, text)


def test_shape_limits(call):
    """2 * B * h * w, 3 * B * oh * ow and the workgroups of both launches: 2^31 - 1 passes, the next count that can be
    reached does not.  The buffers of these calls are never touched: validation does not launch, and without a device
    the launch fails."""
    big = 1 << 44                                       # room for the extents below between any two buffers
    base = call.good["flows"][0]
    far = dict(n=1, flows=[base], outs=[base + big], ws=base + 2 * big, flow_dtype=[_hip.F32])
    one = lambda B, h, w, oh, ow: call(B=B, h=[h], w=[w], oh=[oh], ow=[ow], **far)
    assert one(1, 1, LIMIT // 2, 1, 1)[0] == _hip.E_LAUNCH                       # 2 * h * w = 2^31 - 2
    rc, text = one(1, 1, LIMIT // 2 + 1, 1, 1)                                  # 2^31
    assert rc == _hip.E_SHAPE and "overflows" in text
    assert one(1, 1 << 15, 1 << 15, 1, 1)[0] == _hip.E_SHAPE
    assert one(1, 1, 1, 1, LIMIT // 3)[0] == _hip.E_LAUNCH                       # 3 * oh * ow = 2^31 - 1
    assert one(1, 1, 1, 1, LIMIT // 3 + 1)[0] == _hip.E_SHAPE
    assert one(1 << 20, 1, 1, 1, 682)[0] == _hip.E_LAUNCH and one(1 << 20, 1, 1, 1, 683)[0] == _hip.E_SHAPE
    # the workgroups, summed over the levels: B per level and launch here (one level's stay below its element count)
    eight = lambda B: call(B=B, n=8, flows=[base] * 8, flow_dtype=[_hip.F32] * 8, h=[1] * 8, w=[1] * 8, oh=[1] * 8,
                           ow=[1] * 8, outs=[base + (i + 1) * big for i in range(8)], ws=base + 9 * big)
    assert eight(LIMIT // 8)[0] == _hip.E_LAUNCH and eight(LIMIT // 8 + 1)[0] == _hip.E_SHAPE


def test_align(call):
    g = call.good
    for i, name in ((0, "flows[0]"), (1, "flows[1]")):
        shifted = lambda off: [p + (off if k == i else 0) for k, p in enumerate(g["flows"])]
        for off in (1, 2, 3):
            assert call(flows=shifted(off)) == (_hip.E_ALIGN, name + " must be 4-byte aligned")
        assert call(flows=shifted(4))[0] == _hip.E_LAUNCH
        assert call(flows=shifted(1), flow_dtype=[_hip.F16] * 2) == (_hip.E_ALIGN, name + " must be 2-byte aligned")
        assert call(flows=shifted(2), flow_dtype=[_hip.F16] * 2)[0] == _hip.E_LAUNCH
    for off in (1, 2, 3):
        assert call(outs=[g["outs"][0], g["outs"][1] + off]) == (_hip.E_ALIGN, "outs[1] must be 4-byte aligned")
        assert call(outs=[g["outs"][0], g["outs"][1] + off], out_dtype=_hip.U8)[0] == _hip.E_LAUNCH   # any byte
        assert call(ws=g["ws"] + off) == (_hip.E_ALIGN, "ws must be 4-byte aligned")
    assert call(ws=g["ws"] + 4)[0] == _hip.E_LAUNCH


def test_alias(call):
    g = call.good
    n_flow = [B * h * w * 2 * 4 for h, w in zip(H, W)]
    n_out = [B * oh * ow * 3 * 4 for oh, ow in zip(OH, OW)]
    n_ws = B * 2 * 4                                                            # one tile per image and level
    assert call(outs=[g["flows"][1], g["outs"][1]]) == (_hip.E_ALIAS, "outs[0] overlaps flows[1]")
    assert call(outs=[g["outs"][0], g["flows"][0]]) == (_hip.E_ALIAS, "outs[1] overlaps flows[0]")
    assert call(outs=[g["outs"][0], g["outs"][0]]) == (_hip.E_ALIAS, "outs[1] overlaps outs[0]")
    assert call(outs=[g["ws"], g["outs"][1]]) == (_hip.E_ALIAS, "outs[0] overlaps ws")
    assert call(ws=g["flows"][0]) == (_hip.E_ALIAS, "ws overlaps flows[0]")
    assert call(outs=[g["flows"][0] + n_flow[0] - 4, g["outs"][1]])[0] == _hip.E_ALIAS      # the flow's last float
    assert call(outs=[g["flows"][0] + n_flow[0], g["outs"][1]])[0] == _hip.E_LAUNCH         # adjacent is fine
    assert call(outs=[g["outs"][0], g["outs"][0] + n_out[0] - 4])[0] == _hip.E_ALIAS
    assert call(outs=[g["outs"][0], g["outs"][0] + n_out[0]])[0] == _hip.E_LAUNCH
    assert call(outs=[g["ws"] + n_ws - 4, g["outs"][1]])[0] == _hip.E_ALIAS
    assert call(outs=[g["ws"] + n_ws, g["outs"][1]])[0] == _hip.E_LAUNCH
    # a uint8 picture is a quarter as long
    assert call(out_dtype=_hip.U8, outs=[g["outs"][0], g["outs"][0] + n_out[0] // 4 - 1])[0] == _hip.E_ALIAS
    assert call(out_dtype=_hip.U8, outs=[g["outs"][0], g["outs"][0] + n_out[0] // 4])[0] == _hip.E_LAUNCH


def test_order_of_the_checks(call):
    """null, dtype, layout, shape, alignment, overlap: the first defect answers."""
    g = call.good
    assert call(ws=None, out_dtype=7)[0] == _hip.E_NULL
    assert call(flows=[None, None], flow_dtype=[7, 7])[0] == _hip.E_NULL
    assert call(flow_dtype=[7, 7], in_layout=7)[0] == _hip.E_DTYPE
    assert call(out_dtype=7, out_layout=7)[0] == _hip.E_DTYPE
    assert call(in_layout=7, B=0)[0] == _hip.E_LAYOUT
    assert call(out_layout=7, n=0)[0] == _hip.E_LAYOUT
    assert call(B=0, ws=g["ws"] + 1)[0] == _hip.E_SHAPE
    assert call(ws=g["ws"] + 1, outs=[g["outs"][0], g["outs"][0]])[0] == _hip.E_ALIGN
    with pytest.raises(ValueError, match="overlaps"):
        _hip.check(call(outs=[g["outs"][0], g["outs"][0]])[0])


def test_workspace_query(hip_lib):
    q = lambda n, B, h, w: hip_lib.qpwc_flow_to_image_workspace_floats(n, B, ints(h), ints(w))
    assert q(1, 1, [4], [8]) == 1 and q(1, 2, [4], [8]) == 2 and q(1, 16, [4], [8]) == 16      # grows with B
    assert q(3, 2, [4, 8, 33], [8, 16, 70]) == 2 * (1 + 1 + 2)
    # one partial per image and tile of _hip.VIS_MAX_TILE source pixels: the constant the GPU tests size their cases by
    assert _hip.VIS_MAX_TILE == 2048
    assert q(1, 1, [1], [_hip.VIS_MAX_TILE]) == 1 and q(1, 1, [1], [_hip.VIS_MAX_TILE + 1]) == 2
    assert q(8, 16, [256] * 8, [512] * 8) == 8 * 16 * 64
    assert q(0, 1, [4], [8]) == _hip.E_SHAPE and q(9, 1, [4] * 9, [8] * 9) == _hip.E_SHAPE
    assert q(1, 0, [4], [8]) == _hip.E_SHAPE and q(1, 1, [0], [8]) == _hip.E_SHAPE and q(1, 1, [4], [-1]) == _hip.E_SHAPE
    assert hip_lib.qpwc_flow_to_image_workspace_floats(1, 1, None, ints([8])) == _hip.E_NULL
    assert hip_lib.qpwc_flow_to_image_workspace_floats(1, 1, ints([8]), None) == _hip.E_NULL
    assert q(1, 1, [1], [LIMIT // 2]) > 0 and q(1, 1, [1], [LIMIT // 2 + 1]) == _hip.E_SHAPE


def test_kernel_query_is_host_only(hip_lib):
    aligned = 1 << 20

    def pick(B, sizes, dtype=_hip.U8, layout=_hip.NHWC, outs=None, n=None):
        n = len(sizes) if n is None else n
        outs = [aligned + (i << 16) for i in range(len(sizes))] if outs is None else outs
        return hip_lib.qpwc_flow_to_image_fwd_kernel(n, B, ints([s[0] for s in sizes]), ints([s[1] for s in sizes]),
                                                     dtype, layout, ptrs(outs)).decode()
    vec, scalar = "flow_to_image_kernel<vec4>", "flow_to_image_kernel<scalar>"
    assert pick(16, [(256, 512)] * 8) == vec                                    # the trainer's panels
    assert pick(2, [(64, 128)] * 3) == vec and pick(2, [(37, 70)] * 3) == scalar  # the GPU suite's cases: 2590 = 4 * 647 + 2
    assert pick(2, [(33, 70)]) == scalar and pick(2, [(2, 2)]) == vec
    assert pick(2, [(64, 128), (37, 70)]) == scalar                             # one level decides for the launch
    for dtype in (_hip.U8, _hip.F32):
        for layout in (_hip.NHWC, _hip.NCHW):
            assert pick(2, [(8, 8)], dtype, layout) == vec
            for off in (1, 4, 8, 12):                                           # an output off the 16-byte grid
                assert pick(2, [(8, 8)], dtype, layout, [aligned + off]) == scalar
            assert pick(2, [(8, 8)], dtype, layout, [aligned + 16]) == vec
    assert pick(2, [(8, 8)], _hip.F16) == "" and pick(2, [(8, 8)], layout=2) == ""
    assert pick(0, [(8, 8)]) == "" and pick(2, [(0, 8)]) == "" and pick(2, [(8, -1)]) == ""
    assert pick(2, [(8, 8)], outs=[None]) == "" and pick(2, [(8, 8)] * 9) == "" and pick(2, [(8, 8)], n=0) == ""
    assert hip_lib.qpwc_flow_to_image_fwd_kernel(1, 2, None, ints([8]), _hip.U8, _hip.NHWC, ptrs([aligned])) == b""
    assert hip_lib.qpwc_flow_to_image_fwd_kernel(1, 2, ints([8]), ints([8]), _hip.U8, _hip.NHWC, None) == b""
    # one workgroup per image and tile of _hip.VIS_TILE output pixels
    assert _hip.VIS_TILE == 1024
    assert pick(LIMIT, [(1, 4)]) == "" and pick(LIMIT // 3, [(1, 1)]) == scalar   # 3 * B * oh * ow
    assert pick(1 << 19, [(1, _hip.VIS_TILE)], outs=[aligned]) == vec             # 2^19 workgroups, 3 * 2^29 elements
    assert ops.flow_to_image_kernel(16, [(256, 512)] * 8) == vec
    assert ops.flow_to_image_kernel(2, [(37, 70)], torch.float32, "channels_first") == scalar
    assert ops.flow_to_image_kernel(0, [(8, 8)]) == "" and ops.flow_to_image_kernel(2, [(8, 8)], torch.float16) == ""


def test_vis_prototypes_match_their_header():
    protos = parse_header(VIS_HEADER)
    assert [name for name, _, _ in protos] == ["qpwc_flow_to_image_workspace_floats", "qpwc_flow_to_image_fwd",
                                               "qpwc_flow_to_image_fwd_kernel"]
    assert mismatches(_hip.VIS_PROTOTYPES, protos) == []
    others = set(_hip.SYMBOLS) | set(_hip.OPTIM_PROTOTYPES) | set(_hip.TRIPLET_PROTOTYPES)
    assert len(_hip.SYMBOLS) == 77 and not set(_hip.VIS_PROTOTYPES) & others
    table = dict(_hip.VIS_PROTOTYPES)
    restype, argtypes = table["qpwc_flow_to_image_fwd"]
    table["qpwc_flow_to_image_fwd"] = (restype, argtypes[:-1])
    assert mismatches(table, protos) == ["qpwc_flow_to_image_fwd: 14 parameters, table has 13"]


def test_the_library_exports_the_table(hip_lib):
    for name, (restype, argtypes) in _hip.VIS_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)

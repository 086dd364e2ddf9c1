"""The argument validation of qpwc_inference_panels_fwd, qpwc_interpolation_panels_fwd and their two queries
(include/qpwc_review.h), code by code, with HOST pointers: validation only looks at the values of the pointers and comes
before any HIP call.  Without a device a call that passes it fails at the launch (QPWC_E_LAUNCH); with a device it would
launch on host memory, so the module skips itself there, as tests/test_vis_capi_cpu.py does."""
import ctypes

import pytest
import torch

from qpwcnet_amd import _hip, ops

if torch.cuda.is_available():
    pytest.skip("host pointers: a wrongly accepted case would launch on host memory", allow_module_level=True)

B, H, W = 2, 8, 12              # 96 pixels: <vec4>
STEP = 16 << 10                 # every buffer 16 KiB after the one before
LIMIT = (1 << 31) - 1
ptrs = lambda v: (ctypes.c_void_p * max(len(v), 1))(*v)
VEC, SCALAR = "review_panels_kernel<vec4>", "review_panels_kernel<scalar>"


@pytest.fixture(scope="module")
def calls(hip_lib):
    buf = ctypes.create_string_buffer(16 * STEP + 256)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    at = lambda i: base + i * STEP
    good1 = dict(ims=at(0), ims_dtype=_hip.F32, flo=at(1), flo_pred=at(2), B=B, H=H, W=W, in_layout=_hip.NHWC,
                 outs=[at(4 + i) for i in range(10)], out_dtype=_hip.F32, out_layout=_hip.NHWC, grid=0, ws=at(3),
                 stream=None)
    good2 = dict(img_pair=at(0), img1=at(1), pred=at(2), img_dtype=_hip.F32, flow=at(14), B=B, H=H, W=W, h=H // 2,
                 w=W // 2, in_layout=_hip.NHWC, outs=[at(4 + i) for i in range(7)], out_dtype=_hip.F32,
                 out_layout=_hip.NHWC, grid=32, ws=at(3), stream=None)

    def make(fn, good):
        def run(**changed):
            a = dict(good, **changed)
            a["outs"] = None if a["outs"] is None else ptrs(a["outs"])
            assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
            rc = fn(*[a[k] for k in good])
            return rc, hip_lib.qpwc_last_error().decode()
        run.good = good
        return run
    one, two = make(hip_lib.qpwc_inference_panels_fwd, good1), make(hip_lib.qpwc_interpolation_panels_fwd, good2)
    one.keep = buf
    return one, two


def test_a_valid_call_reaches_the_launch(calls):
    for call in calls:
        rc, text = call()
        assert rc == _hip.E_LAUNCH and text.startswith("flow_mag_max_kernel: "), (rc, text)
        for ok in (dict(out_dtype=_hip.U8), dict(in_layout=_hip.NCHW), dict(out_layout=_hip.NCHW), dict(grid=1),
                   dict(grid=0), dict(H=7, W=5) if call is calls[0] else dict(H=9, W=15, h=3, w=5)):
            assert call(**ok)[0] == _hip.E_LAUNCH, ok
    one, two = calls
    assert one(ims_dtype=_hip.F16)[0] == _hip.E_LAUNCH and two(img_dtype=_hip.F16)[0] == _hip.E_LAUNCH
    assert two(h=H, w=W)[0] == _hip.E_LAUNCH                                       # s = 1
    g = one.good
    assert one(flo_pred=g["flo"])[0] == _hip.E_LAUNCH                              # the inputs may be one buffer
    assert two(pred=two.good["img1"])[0] == _hip.E_LAUNCH


def test_null(calls):
    one, two = calls
    for name in ("ims", "flo", "flo_pred", "outs", "ws"):
        assert one(**{name: None}) == (_hip.E_NULL, name + " is null")
    for name in ("img_pair", "img1", "pred", "flow", "outs", "ws"):
        assert two(**{name: None}) == (_hip.E_NULL, name + " is null")
    assert one(outs=one.good["outs"][:9] + [None]) == (_hip.E_NULL, "outs[9] is null")
    assert two(outs=[None] + two.good["outs"][1:]) == (_hip.E_NULL, "outs[0] is null")


def test_dtype_and_layout(calls):
    for call, key in zip(calls, ("ims_dtype", "img_dtype")):
        for bad in (_hip.U8, 3, -1):
            rc, text = call(**{key: bad})
            assert rc == _hip.E_DTYPE and text.startswith("images"), text
        for bad in (_hip.F16, 3, -1):
            assert call(out_dtype=bad)[0] == _hip.E_DTYPE
        for name in ("in_layout", "out_layout"):
            for bad in (2, -1):
                rc, text = call(**{name: bad})
                assert rc == _hip.E_LAYOUT and text.startswith("Unsupported data format")


def test_shape(calls):
    one, two = calls
    for bad in (0, -3):
        for name in ("B", "H", "W"):
            rc, text = one(**{name: bad})
            assert rc == _hip.E_SHAPE and text.startswith("non-positive"), (name, text)
        for name in ("B", "H", "W", "h", "w"):
            rc, text = two(**{name: bad})
            assert rc == _hip.E_SHAPE and text.startswith("non-positive"), (name, text)
    for call in calls:
        rc, text = call(grid=-1)
        assert rc == _hip.E_SHAPE and "grid" in text
    for bad in (dict(h=3), dict(w=5), dict(h=H, w=W // 2), dict(h=2 * H, w=2 * W), dict(H=9, h=4)):
        rc, text = two(**bad)
        assert rc == _hip.E_SHAPE and "whole multiple" in text, (bad, text)


def test_shape_limits(calls):
    """6 * B * H * W: 2^31 - 1 passes, the next count that can be reached does not.  The buffers of these calls are never
    touched: validation does not launch, and without a device the launch fails."""
    one, two = calls
    big = 1 << 44
    base = one.good["ims"]
    far1 = dict(ims=base, flo=base + big, flo_pred=base + 2 * big, ws=base + 3 * big,
                outs=[base + (4 + i) * big for i in range(10)])
    n = LIMIT // 6                                          # 357913941 = 3 * 119304647
    assert one(B=1, H=1, W=n, out_dtype=_hip.U8, **far1)[0] == _hip.E_LAUNCH         # 6 * H * W = 2^31 - 2; scalar
    rc, text = one(B=1, H=1, W=n + 1, **far1)
    assert rc == _hip.E_SHAPE and "overflows" in text
    assert one(B=1 << 20, H=1, W=341, out_dtype=_hip.U8, **far1)[0] == _hip.E_LAUNCH
    assert one(B=1 << 20, H=1, W=342, **far1)[0] == _hip.E_SHAPE
    far2 = dict(img_pair=base, img1=base + big, pred=base + 2 * big, ws=base + 3 * big, flow=base + 12 * big,
                outs=[base + (4 + i) * big for i in range(7)])
    assert two(B=1, H=1, W=n, h=1, w=n, out_dtype=_hip.U8, **far2)[0] == _hip.E_LAUNCH
    assert two(B=1, H=1, W=n + 1, h=1, w=n + 1, **far2)[0] == _hip.E_SHAPE
    assert two(B=1, H=1 << 15, W=1 << 15, h=1 << 14, w=1 << 14, **far2)[0] == _hip.E_SHAPE


def test_align(calls):
    """Inputs: their element size.  Outputs: what the store form needs, which follows from the shape alone: <vec4> 16
    bytes (fp32) / 4 (uint8), <scalar> 4 / 1.  Nothing off that grid is accepted, so the kernel need not look."""
    one, two = calls
    for call, names, key in ((one, ("ims",), "ims_dtype"), (two, ("img_pair", "img1", "pred"), "img_dtype")):
        g = call.good
        for name in names:
            for off in (1, 2, 3):
                assert call(**{name: g[name] + off}) == (_hip.E_ALIGN, name + " must be 4-byte aligned")
            assert call(**{name: g[name] + 4})[0] == _hip.E_LAUNCH
            assert call(**{name: g[name] + 1, key: _hip.F16}) == (_hip.E_ALIGN, name + " must be 2-byte aligned")
            assert call(**{name: g[name] + 2, key: _hip.F16})[0] == _hip.E_LAUNCH
        for name in ("flo", "flo_pred") if call is one else ("flow",):
            for off in (1, 2, 3):
                assert call(**{name: g[name] + off}) == (_hip.E_ALIGN, name + " must be 4-byte aligned")
            assert call(**{name: g[name] + 4})[0] == _hip.E_LAUNCH
        for off in (1, 2, 3):
            assert call(ws=g["ws"] + off) == (_hip.E_ALIGN, "ws must be 4-byte aligned")
        assert call(ws=g["ws"] + 4)[0] == _hip.E_LAUNCH
        last = len(g["outs"]) - 1
        shifted = lambda off: g["outs"][:last] + [g["outs"][last] + off]
        # 8 x 12: <vec4>
        for off in (1, 4, 8, 12):
            assert call(outs=shifted(off)) == (_hip.E_ALIGN, "outs[%d] must be 16-byte aligned" % last)
        assert call(outs=shifted(16))[0] == _hip.E_LAUNCH
        for off in (1, 2, 3):
            assert call(outs=shifted(off), out_dtype=_hip.U8) == (_hip.E_ALIGN, "outs[%d] must be 4-byte aligned" % last)
        assert call(outs=shifted(4), out_dtype=_hip.U8)[0] == _hip.E_LAUNCH
        # <scalar>: 7 x 5 pixels (set 1), 9 x 15 with a 3 x 5 flow (set 2)
        odd = dict(H=7, W=5) if call is one else dict(H=9, W=15, h=3, w=5)
        for off in (1, 2, 3):
            assert call(outs=shifted(off), **odd) == (_hip.E_ALIGN, "outs[%d] must be 4-byte aligned" % last)
            assert call(outs=shifted(off), out_dtype=_hip.U8, **odd)[0] == _hip.E_LAUNCH       # any byte
        assert call(outs=shifted(4), **odd)[0] == _hip.E_LAUNCH
    # set 2: an odd-sized flow picture alone makes the launch <scalar>
    assert two(H=6, W=10, h=3, w=5, outs=[p + 4 for p in two.good["outs"]])[0] == _hip.E_LAUNCH


def test_alias(calls):
    one, two = calls
    g = one.good
    n_img, n_flow, n_out, n_ws = B * H * W * 6 * 4, B * H * W * 2 * 4, B * H * W * 3 * 4, 2 * B * 4
    swap = lambda i, p, outs=None: (outs or g["outs"])[:i] + [p] + (outs or g["outs"])[i + 1:]
    assert one(outs=swap(0, g["ims"])) == (_hip.E_ALIAS, "outs[0] overlaps ims")
    assert one(outs=swap(3, g["flo"])) == (_hip.E_ALIAS, "outs[3] overlaps flo")
    assert one(outs=swap(9, g["flo_pred"])) == (_hip.E_ALIAS, "outs[9] overlaps flo_pred")
    assert one(outs=swap(2, g["ws"])) == (_hip.E_ALIAS, "outs[2] overlaps ws")
    assert one(outs=swap(5, g["outs"][1])) == (_hip.E_ALIAS, "outs[5] overlaps outs[1]")
    assert one(ws=g["ims"]) == (_hip.E_ALIAS, "ws overlaps ims")
    assert one(outs=swap(0, g["ims"] + n_img - 16))[0] == _hip.E_ALIAS             # the image's last 16 bytes
    assert one(outs=swap(0, g["ims"] + n_img))[0] == _hip.E_LAUNCH                 # adjacent is fine
    assert one(outs=swap(0, g["flo"] + n_flow - 16))[0] == _hip.E_ALIAS
    assert one(outs=swap(0, g["flo"] + n_flow))[0] == _hip.E_LAUNCH
    assert one(outs=swap(1, g["outs"][0] + n_out - 16))[0] == _hip.E_ALIAS
    assert one(outs=swap(1, g["outs"][0] + n_out))[0] == _hip.E_LAUNCH
    assert one(outs=swap(0, g["ws"] + n_ws - 16))[0] == _hip.E_ALIAS
    assert one(outs=swap(0, g["ws"] + n_ws))[0] == _hip.E_LAUNCH
    # a uint8 picture is a quarter as long
    assert one(out_dtype=_hip.U8, outs=swap(1, g["outs"][0] + n_out // 4 - 4))[0] == _hip.E_ALIAS
    assert one(out_dtype=_hip.U8, outs=swap(1, g["outs"][0] + n_out // 4))[0] == _hip.E_LAUNCH
    t = two.good
    swap2 = lambda i, p: t["outs"][:i] + [p] + t["outs"][i + 1:]
    for name in ("img_pair", "img1", "pred", "flow"):
        assert two(outs=swap2(6, t[name])) == (_hip.E_ALIAS, "outs[6] overlaps " + name)
    assert two(outs=swap2(4, t["ws"])) == (_hip.E_ALIAS, "outs[4] overlaps ws")
    assert two(ws=t["flow"]) == (_hip.E_ALIAS, "ws overlaps flow")
    # 5-flow has the flow's size: a quarter of the other pictures here
    assert two(outs=swap2(6, t["outs"][5] + n_out // 4 - 16))[0] == _hip.E_ALIAS
    assert two(outs=swap2(6, t["outs"][5] + n_out // 4))[0] == _hip.E_LAUNCH
    assert two(outs=swap2(6, t["outs"][4] + n_out // 4))[0] == _hip.E_ALIAS


def test_order_of_the_checks(calls):
    """null, dtype, layout, shape, alignment, overlap: the first defect answers."""
    for call, key in zip(calls, ("ims_dtype", "img_dtype")):
        g = call.good
        assert call(ws=None, **{key: 7})[0] == _hip.E_NULL
        assert call(outs=[None] * len(g["outs"]), out_dtype=7)[0] == _hip.E_NULL
        assert call(in_layout=7, **{key: 7})[0] == _hip.E_DTYPE
        assert call(out_dtype=7, out_layout=7)[0] == _hip.E_DTYPE
        assert call(in_layout=7, B=0)[0] == _hip.E_LAYOUT
        assert call(out_layout=7, grid=-1)[0] == _hip.E_LAYOUT
        assert call(B=0, ws=g["ws"] + 1)[0] == _hip.E_SHAPE
        assert call(grid=-1, ws=g["ws"] + 1)[0] == _hip.E_SHAPE
        twice = g["outs"][:-1] + [g["outs"][0]]
        assert call(ws=g["ws"] + 1, outs=twice)[0] == _hip.E_ALIGN
        assert call(outs=twice)[0] == _hip.E_ALIAS
        with pytest.raises(ValueError, match="overlaps"):
            _hip.check(call(outs=twice)[0])


def test_workspace_query(hip_lib):
    q = hip_lib.qpwc_review_workspace_floats
    assert q(2, 1, 4, 8) == 2 and q(1, 1, 4, 8) == 1 and q(2, 16, 4, 8) == 32
    # one partial per flow, image and tile of _hip.VIS_MAX_TILE flow pixels: the constant the GPU tests size their cases by
    assert _hip.VIS_MAX_TILE == 2048
    assert q(1, 1, 1, _hip.VIS_MAX_TILE) == 1 and q(1, 1, 1, _hip.VIS_MAX_TILE + 1) == 2
    assert q(2, 2, 33, 70) == 8 and q(2, 8, 256, 512) == 2 * 8 * 64 and q(1, 8, 128, 256) == 8 * 16
    for bad in ((0, 1, 4, 8), (3, 1, 4, 8), (1, 0, 4, 8), (1, 1, 0, 8), (1, 1, 4, -1)):
        assert q(*bad) == _hip.E_SHAPE, bad
    assert q(1, 1, 1, LIMIT // 6) > 0 and q(1, 1, 1, LIMIT // 6 + 1) == _hip.E_SHAPE


def test_kernel_query_is_host_only(hip_lib):
    def pick(n_flows, B, H, W, h=None, w=None, dtype=_hip.F32, layout=_hip.NHWC):
        h, w = H if h is None else h, W if w is None else w
        return hip_lib.qpwc_review_panels_fwd_kernel(n_flows, B, H, W, h, w, dtype, layout).decode()
    assert pick(2, 8, 256, 512) == VEC and pick(1, 8, 256, 512, 128, 256) == VEC          # the scripts' sizes
    assert pick(2, 2, 33, 70) == SCALAR and pick(2, 2, 32, 68) == VEC                     # the GPU suite's cases
    assert pick(1, 2, 34, 70, 17, 35) == SCALAR and pick(1, 2, 36, 72, 18, 36) == VEC and pick(1, 2, 20, 36) == VEC
    assert pick(1, 2, 6, 10, 3, 5) == SCALAR                    # 60 pictures' pixels, but an odd-sized flow picture
    for dtype in (_hip.F32, _hip.U8):
        for layout in (_hip.NHWC, _hip.NCHW):
            assert pick(2, 2, 8, 8, dtype=dtype, layout=layout) == VEC
            assert pick(2, 2, 7, 9, dtype=dtype, layout=layout) == SCALAR
    assert pick(2, 2, 8, 8, dtype=_hip.F16) == "" and pick(2, 2, 8, 8, layout=2) == ""
    assert pick(0, 2, 8, 8) == "" and pick(3, 2, 8, 8) == "" and pick(2, 0, 8, 8) == "" and pick(2, 2, 0, 8) == ""
    assert pick(2, 2, 8, 8, 4, 4) == ""                         # test_infer.py's flows have the images' size
    assert pick(1, 2, 8, 8, 3, 4) == "" and pick(1, 2, 8, 8, 4, 8) == "" and pick(1, 2, 8, 8, 16, 16) == ""
    assert pick(2, 1, 1, LIMIT // 6) == SCALAR and pick(2, 1, 1, LIMIT // 6 + 1) == ""
    assert _hip.REVIEW_TILE == 256
    assert ops.review_panels_kernel(2, 8, 256, 512) == VEC
    assert ops.review_panels_kernel(1, 2, 34, 70, 17, 35, torch.uint8, "channels_first") == SCALAR
    assert ops.review_panels_kernel(2, 0, 8, 8) == "" and ops.review_panels_kernel(2, 2, 8, 8, out_dtype=torch.float16) == ""

"""The argument validation of qpwc_image_quality_fwd (include/qpwc_quality.h), code by code, with HOST pointers:
validation only looks at the values of the pointers and comes before any HIP call.  Without a device a call that passes
it fails at the launch (QPWC_E_LAUNCH); with a device it would launch on host memory, so the module skips itself there,
as tests/test_vis_capi_cpu.py does.  The header, the table and the two queries are held in tests/test_quality_cpu.py."""
import ctypes

import pytest
import torch

from qpwcnet_amd import _hip

if torch.cuda.is_available():
    pytest.skip("host pointers: a wrongly accepted case would launch on host memory", allow_module_level=True)

B, H, W, C = 2, 12, 27, 3
STEP = 16 << 10                 # every buffer 16 KiB after the one before
LIMIT = (1 << 31) - 1
N_IMG = B * H * W * C * 4       # bytes of an fp32 input
N_OUT = 3 * B * 4
N_WS = B * (C + 1) * 4          # one tile per image
N_STATE = 4 * 8


@pytest.fixture(scope="module")
def call(hip_lib):
    buf = ctypes.create_string_buffer(6 * STEP + 256)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    good = dict(truth=base, truth_dtype=_hip.F32, pred=base + STEP, pred_dtype=_hip.F32, B=B, H=H, W=W, C=C,
                layout=_hip.NHWC, offset_truth=0.0, offset_pred=0.0, flags=0, max_val=1.0, out=base + 2 * STEP,
                state=base + 3 * STEP, ws=base + 4 * STEP, stream=None)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
        rc = hip_lib.qpwc_image_quality_fwd(*[a[k] for k in good])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good, run.keep = good, buf
    return run


def test_a_valid_call_reaches_the_launch(call):
    rc, text = call()
    assert rc == _hip.E_LAUNCH and text.startswith("quality_tile_kernel: "), (rc, text)
    g = call.good
    for ok in (dict(truth_dtype=_hip.F16), dict(pred_dtype=_hip.F16), dict(truth_dtype=_hip.F16, pred_dtype=_hip.F16),
               dict(layout=_hip.NCHW), dict(state=None), dict(pred=g["truth"]),            # the images may be one buffer
               dict(flags=_hip.QUALITY_CLIP), dict(flags=_hip.QUALITY_U8, max_val=255.0),
               dict(flags=_hip.QUALITY_U8 | _hip.QUALITY_CLIP, max_val=255.0), dict(offset_truth=0.5, offset_pred=-0.5),
               dict(C=1), dict(C=4), dict(H=11, W=11), dict(max_val=255.0)):
        assert call(**ok)[0] == _hip.E_LAUNCH, ok


def test_null(call):
    for name in ("truth", "pred", "out", "ws"):
        assert call(**{name: None}) == (_hip.E_NULL, name + " is null")
    assert call(state=None)[0] == _hip.E_LAUNCH                                  # no running sums: fine


def test_dtype_and_layout(call):
    for name in ("truth", "pred"):
        for bad in (_hip.U8, 3, -1):
            rc, text = call(**{name + "_dtype": bad})
            assert rc == _hip.E_DTYPE and text.startswith(name + ": unsupported dtype"), text
    for bad in (2, -1):
        rc, text = call(layout=bad)
        assert rc == _hip.E_LAYOUT and text.startswith("Unsupported data format")


def test_shape(call):
    for bad in (0, -3):
        assert call(B=bad)[0] == _hip.E_SHAPE
    for bad in (0, 5, -1):
        rc, text = call(C=bad)
        assert rc == _hip.E_SHAPE and "outside 1..4" in text
    for name in ("H", "W"):
        rc, text = call(**{name: 10})
        assert rc == _hip.E_SHAPE and "at least 11" in text, text
        assert call(**{name: 11})[0] == _hip.E_LAUNCH
        assert call(**{name: 0})[0] == _hip.E_SHAPE and call(**{name: -11})[0] == _hip.E_SHAPE


def test_shape_limits(call):
    """B * H * W * C and the workgroups of the tile launch (never more than the elements: a workgroup has at least 121):
    the largest count that can be reached below 2^31 passes, the next one does not (2^31 - 1 is prime).  The buffers of
    these calls are never touched: validation does not launch, and without a device the launch fails."""
    big = 1 << 44                                       # room for the extents below between any two buffers
    base = call.good["truth"]
    far = dict(truth=base, pred=base + big, out=base + 2 * big, ws=base + 3 * big, state=base + 4 * big)
    one = lambda b, h, w, c: call(B=b, H=h, W=w, C=c, **far)
    assert one(LIMIT // 121, 11, 11, 1)[0] == _hip.E_LAUNCH                       # 2^31 - 90 elements
    rc, text = one(LIMIT // 121 + 1, 11, 11, 1)                                   # 2^31 + 31
    assert rc == _hip.E_SHAPE and "overflows" in text
    assert one(1, 11, LIMIT // 11, 1)[0] == _hip.E_LAUNCH and one(1, 11, LIMIT // 11 + 1, 1)[0] == _hip.E_SHAPE
    assert one(1, 11, LIMIT // 44, 4)[0] == _hip.E_LAUNCH and one(1, 11, LIMIT // 44 + 1, 4)[0] == _hip.E_SHAPE
    assert one(1, 1 << 15, 1 << 15, 1)[0] == _hip.E_LAUNCH and one(1, 1 << 15, 1 << 15, 2)[0] == _hip.E_SHAPE
    assert one(1 << 20, 32, 64, 1)[0] == _hip.E_SHAPE and one((1 << 20) - 1, 32, 64, 1)[0] == _hip.E_LAUNCH


def test_range(call):
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        rc, text = call(max_val=bad)
        assert rc == _hip.E_RANGE and text.startswith("max_val"), (bad, text)
    for name in ("offset_truth", "offset_pred"):
        for bad in (float("inf"), float("-inf"), float("nan")):
            rc, text = call(**{name: bad})
            assert rc == _hip.E_RANGE and text.startswith(name), (bad, text)
    for flags in (_hip.QUALITY_U8, _hip.QUALITY_U8 | _hip.QUALITY_CLIP):
        rc, text = call(flags=flags, max_val=1.0)
        assert rc == _hip.E_RANGE and "255" in text
        assert call(flags=flags, max_val=254.0)[0] == _hip.E_RANGE and call(flags=flags, max_val=255.0)[0] == _hip.E_LAUNCH


def test_mode(call):
    for bad in (4, 8, -1, 6):
        rc, text = call(flags=bad, max_val=255.0)
        assert rc == _hip.E_MODE and "flags" in text, (bad, text)
    for ok in (0, 1, 2, 3):
        assert call(flags=ok, max_val=255.0)[0] == _hip.E_LAUNCH


def test_align(call):
    g = call.good
    for name in ("truth", "pred"):
        for off in (1, 2, 3):
            assert call(**{name: g[name] + off}) == (_hip.E_ALIGN, name + " must be 4-byte aligned")
        assert call(**{name: g[name] + 4})[0] == _hip.E_LAUNCH
        assert call(**{name: g[name] + 1, name + "_dtype": _hip.F16}) == (_hip.E_ALIGN, name + " must be 2-byte aligned")
        assert call(**{name: g[name] + 2, name + "_dtype": _hip.F16})[0] == _hip.E_LAUNCH
    for name in ("out", "ws"):
        for off in (1, 2, 3):
            assert call(**{name: g[name] + off}) == (_hip.E_ALIGN, name + " must be 4-byte aligned")
        assert call(**{name: g[name] + 4})[0] == _hip.E_LAUNCH
    for off in (1, 2, 4, 7, 12):                                                  # the state off the 8-byte grid
        assert call(state=g["state"] + off) == (_hip.E_ALIGN, "state must be 8-byte aligned")
    assert call(state=g["state"] + 8)[0] == _hip.E_LAUNCH


def test_alias(call):
    """out, ws or state overlapping an input or each other; every overlap with its adjacent-is-fine twin."""
    g = call.good
    sizes = {"truth": N_IMG, "pred": N_IMG, "out": N_OUT, "ws": N_WS, "state": N_STATE}
    grid = {"out": 4, "ws": 4, "state": 8}
    for moved, fixed in (("out", "truth"), ("out", "pred"), ("ws", "truth"), ("ws", "pred"), ("ws", "out"),
                         ("state", "truth"), ("state", "pred"), ("state", "out"), ("state", "ws")):
        text = "{} overlaps {}".format(moved, fixed)
        assert call(**{moved: g[fixed]}) == (_hip.E_ALIAS, text)
        last = g[fixed] + sizes[fixed] - 4                                        # the last float of the other buffer
        assert call(**{moved: last - last % grid[moved]}) == (_hip.E_ALIAS, text)
        assert call(**{moved: g[fixed] + sizes[fixed]})[0] == _hip.E_LAUNCH       # adjacent is fine
        assert call(**{moved: g[fixed] - sizes[moved]})[0] == _hip.E_LAUNCH       # on the other side too
        assert call(**{moved: g[fixed] - sizes[moved] + grid[moved]}) == (_hip.E_ALIAS, text)
    # fp16 inputs are half as long
    assert call(out=g["truth"] + N_IMG // 2 - 4, truth_dtype=_hip.F16)[0] == _hip.E_ALIAS
    assert call(out=g["truth"] + N_IMG // 2, truth_dtype=_hip.F16)[0] == _hip.E_LAUNCH
    # the workspace grows with the tiles: 12 x 43 has two of them
    assert call(W=43, state=g["ws"] + 2 * N_WS - 8)[0] == _hip.E_ALIAS
    assert call(W=43, state=g["ws"] + 2 * N_WS)[0] == _hip.E_LAUNCH
    assert call(pred=g["truth"] + 4)[0] == _hip.E_LAUNCH                          # the inputs may overlap


def test_order_of_the_checks(call):
    """null, dtype, layout, shape, range, mode, alignment, overlap: the first defect answers."""
    g = call.good
    assert call(ws=None, truth_dtype=7)[0] == _hip.E_NULL
    assert call(truth_dtype=7, layout=7)[0] == _hip.E_DTYPE
    assert call(pred_dtype=7, layout=7)[0] == _hip.E_DTYPE
    assert call(layout=7, H=10)[0] == _hip.E_LAYOUT
    assert call(H=10, max_val=0.0)[0] == _hip.E_SHAPE
    assert call(C=5, flags=_hip.QUALITY_U8)[0] == _hip.E_SHAPE
    assert call(max_val=0.0, flags=9)[0] == _hip.E_RANGE
    assert call(flags=_hip.QUALITY_U8, out=g["out"] + 1)[0] == _hip.E_RANGE      # U8 with max_val 1
    assert call(flags=9, out=g["out"] + 1)[0] == _hip.E_MODE
    assert call(out=g["out"] + 1, ws=g["truth"])[0] == _hip.E_ALIGN
    assert call(state=g["state"] + 4, ws=g["out"])[0] == _hip.E_ALIGN
    with pytest.raises(ValueError, match="overlaps"):
        _hip.check(call(ws=g["out"])[0])

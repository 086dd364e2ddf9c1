"""The argument validation of qpwc_flow_quality_fwd (include/qpwc_flow_quality.h), code by code, with HOST pointers:
validation only looks at the values of the pointers and comes before any HIP call.  Without a device a call that passes
it fails at the launch (QPWC_E_LAUNCH); with a device it would launch on host memory, so the module skips itself there,
as tests/test_quality_capi_cpu.py does.  The header and the table are held in tests/test_flow_quality_cpu.py."""
import ctypes

import pytest
import torch

from qpwcnet_amd import _hip

if torch.cuda.is_available():
    pytest.skip("host pointers: a wrongly accepted case would launch on host memory", allow_module_level=True)

B, H, W = 2, 12, 27
STEP = 16 << 10                 # every buffer 16 KiB after the one before
LIMIT = (1 << 31) - 1
CHUNK = _hip.FLOW_QUALITY_CHUNK
N_FLOW = B * H * W * 2 * 4      # bytes of an fp32 flow
N_MASK = B * H * W
N_OUT = 12 * B * 4
N_WS = B * 15 * 4               # one chunk per image
N_STATE = 17 * 8
PARAMS = ("out_abs", "out_rel", "t0", "t1", "t2", "s0", "s1")


@pytest.fixture(scope="module")
def call(hip_lib):
    buf = ctypes.create_string_buffer(8 * STEP + 256)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    good = dict(truth=base, pred=base + STEP, pred_dtype=_hip.F32, valid=base + 2 * STEP, occluded=base + 3 * STEP,
                B=B, H=H, W=W, layout=_hip.NHWC, out_abs=3.0, out_rel=0.05, t0=1.0, t1=3.0, t2=5.0, s0=10.0, s1=40.0,
                out=base + 4 * STEP, state=base + 5 * STEP, ws=base + 6 * STEP, stream=None)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
        rc = hip_lib.qpwc_flow_quality_fwd(*[a[k] for k in good])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good, run.keep = good, buf
    return run


def test_a_valid_call_reaches_the_launch(call):
    rc, text = call()
    assert rc == _hip.E_LAUNCH and text.startswith("flow_quality_tile_kernel: "), (rc, text)
    g = call.good
    for ok in (dict(pred_dtype=_hip.F16), dict(layout=_hip.NCHW), dict(layout=_hip.NCHW, pred_dtype=_hip.F16),
               dict(state=None), dict(valid=None), dict(occluded=None), dict(valid=None, occluded=None, state=None),
               dict(pred=g["truth"]),                                            # the flows may be one buffer
               dict(occluded=g["valid"]),                                        # and so may the masks
               dict(out_rel=0.0), dict(H=1, W=1), dict(B=1), dict(t0=0.5, t1=1.0, t2=2.0, s0=1.0, s1=2.0)):
        assert call(**ok)[0] == _hip.E_LAUNCH, ok


def test_queries(hip_lib):
    ws, kernel = hip_lib.qpwc_flow_quality_workspace_floats, hip_lib.qpwc_flow_quality_fwd_kernel
    assert ws(B, H, W) == N_WS // 4 and ws(B, 1, CHUNK + 1) == 2 * N_WS // 4
    assert kernel(B, H, W) == b"flow_quality_tile_kernel"
    for bad in ((0, H, W), (B, 0, W), (B, H, -1), (2, 1 << 15, 1 << 15)):
        assert ws(*bad) == _hip.E_SHAPE and kernel(*bad) == b"", bad


def test_null(call):
    for name in ("truth", "pred", "out", "ws"):
        assert call(**{name: None}) == (_hip.E_NULL, name + " is null")
    for name in ("valid", "occluded", "state"):
        assert call(**{name: None})[0] == _hip.E_LAUNCH                           # optional


def test_dtype_and_layout(call):
    for bad in (_hip.U8, 3, -1):
        rc, text = call(pred_dtype=bad)
        assert rc == _hip.E_DTYPE and text.startswith("pred: unsupported dtype"), text
    for bad in (2, -1):
        rc, text = call(layout=bad)
        assert rc == _hip.E_LAYOUT and text.startswith("Unsupported data format")


def test_shape(call):
    for name in ("B", "H", "W"):
        for bad in (0, -3):
            rc, text = call(**{name: bad})
            assert rc == _hip.E_SHAPE and "non-positive" in text, text
        assert call(**{name: 1})[0] == _hip.E_LAUNCH


def test_shape_limits(call):
    """B * H * W and the workgroups of the tile launch (never more than the pixels): the largest count passes, the next
    one does not.  The buffers of these calls are never touched: validation does not launch, and without a device the
    launch fails."""
    big = 1 << 44                                       # room for the extents below between any two buffers
    base = call.good["truth"]
    far = dict(truth=base, pred=base + big, valid=base + 2 * big, occluded=base + 3 * big, out=base + 4 * big,
               ws=base + 5 * big, state=base + 6 * big)
    one = lambda b, h, w: call(B=b, H=h, W=w, **far)
    assert one(1, 1, LIMIT)[0] == _hip.E_LAUNCH and one(LIMIT, 1, 1)[0] == _hip.E_LAUNCH     # 2^31 - 1 pixels
    assert one(1, LIMIT, 1)[0] == _hip.E_LAUNCH
    rc, text = one(2, 1, 1 << 30)                                                              # 2^31
    assert rc == _hip.E_SHAPE and "overflows" in text
    assert one(1, 1 << 15, 1 << 16)[0] == _hip.E_SHAPE and one(1, 1 << 15, (1 << 16) - 1)[0] == _hip.E_LAUNCH
    assert one(1 << 20, 32, 64)[0] == _hip.E_SHAPE and one((1 << 20) - 1, 32, 64)[0] == _hip.E_LAUNCH
    assert one(LIMIT // 121, 11, 11)[0] == _hip.E_LAUNCH and one(LIMIT // 121 + 1, 11, 11)[0] == _hip.E_SHAPE


def test_range(call):
    for name in PARAMS:
        for bad in (float("inf"), float("-inf"), float("nan")):
            rc, text = call(**{name: bad})
            assert rc == _hip.E_RANGE and text.startswith(name + "=") and "finite" in text, (name, bad, text)
    for name in ("out_abs", "t0", "s0"):
        for bad in (0.0, -1.0):
            rc, text = call(**{name: bad})
            assert rc == _hip.E_RANGE and name in text, (name, bad, text)
        assert call(**{name: 0.25})[0] == _hip.E_LAUNCH
    rc, text = call(out_rel=-0.01)
    assert rc == _hip.E_RANGE and text.startswith("out_rel")
    assert call(out_rel=0.0)[0] == _hip.E_LAUNCH and call(out_rel=2.0)[0] == _hip.E_LAUNCH
    # the orderings: equal is refused, the next float is not
    up = lambda x: float(torch.nextafter(torch.tensor(x), torch.tensor(float("inf"))))
    for bad in (dict(t1=1.0), dict(t1=0.5), dict(t2=3.0), dict(t2=2.0), dict(t0=3.0), dict(t0=6.0)):
        rc, text = call(**bad)
        assert rc == _hip.E_RANGE and "t0 < t1 < t2" in text, (bad, text)
    assert call(t1=up(1.0))[0] == _hip.E_LAUNCH and call(t2=up(3.0))[0] == _hip.E_LAUNCH
    for bad in (dict(s1=10.0), dict(s1=5.0), dict(s0=40.0), dict(s0=50.0)):
        rc, text = call(**bad)
        assert rc == _hip.E_RANGE and "s0 < s1" in text, (bad, text)
    assert call(s1=up(10.0))[0] == _hip.E_LAUNCH


def test_align(call):
    """A (B,H,W,2) pixel is one load: 8 bytes in fp32, 4 in fp16; a (B,2,H,W) plane is read by element: 4 and 2."""
    g = call.good
    grid = {(_hip.NHWC, _hip.F32): 8, (_hip.NHWC, _hip.F16): 4, (_hip.NCHW, _hip.F32): 4, (_hip.NCHW, _hip.F16): 2}
    for (layout, dtype), step in grid.items():
        truth_step = 8 if layout == _hip.NHWC else 4                               # the truth is always fp32
        kw = dict(layout=layout, pred_dtype=dtype)
        for off in range(1, truth_step):
            assert call(truth=g["truth"] + off, **kw) == (_hip.E_ALIGN, "truth must be {}-byte aligned".format(truth_step))
        assert call(truth=g["truth"] + truth_step, **kw)[0] == _hip.E_LAUNCH
        for off in range(1, step):
            assert call(pred=g["pred"] + off, **kw) == (_hip.E_ALIGN, "pred must be {}-byte aligned".format(step))
        assert call(pred=g["pred"] + step, **kw)[0] == _hip.E_LAUNCH
    for name in ("valid", "occluded"):
        for off in (1, 2, 3):
            assert call(**{name: g[name] + off})[0] == _hip.E_LAUNCH               # bytes
    for name in ("out", "ws"):
        for off in (1, 2, 3):
            assert call(**{name: g[name] + off}) == (_hip.E_ALIGN, name + " must be 4-byte aligned")
        assert call(**{name: g[name] + 4})[0] == _hip.E_LAUNCH
    for off in (1, 2, 4, 7, 12):                                                  # the state off the 8-byte grid
        assert call(state=g["state"] + off) == (_hip.E_ALIGN, "state must be 8-byte aligned")
    assert call(state=g["state"] + 8)[0] == _hip.E_LAUNCH


def test_alias(call):
    """out, ws or state overlapping an input, a mask or each other; every overlap with its adjacent-is-fine twin."""
    g = call.good
    sizes = {"truth": N_FLOW, "pred": N_FLOW, "valid": N_MASK, "occluded": N_MASK, "out": N_OUT, "ws": N_WS,
             "state": N_STATE}
    grid = {"out": 4, "ws": 4, "state": 8}
    pairs = [(moved, fixed) for moved in ("out", "ws", "state") for fixed in ("truth", "pred", "valid", "occluded")]
    pairs += [("ws", "out"), ("state", "out"), ("state", "ws")]
    for moved, fixed in pairs:
        text = "{} overlaps {}".format(moved, fixed)
        assert call(**{moved: g[fixed]}) == (_hip.E_ALIAS, text)
        last = g[fixed] + sizes[fixed] - 1                                        # the last byte of the other buffer
        assert call(**{moved: last - last % grid[moved]}) == (_hip.E_ALIAS, text)
        end = g[fixed] + sizes[fixed]
        assert call(**{moved: end + (-end) % grid[moved]})[0] == _hip.E_LAUNCH    # adjacent is fine
        assert call(**{moved: g[fixed] - sizes[moved]})[0] == _hip.E_LAUNCH       # on the other side too
        assert call(**{moved: g[fixed] - sizes[moved] + grid[moved]}) == (_hip.E_ALIAS, text)
    # a mask that is not given is not compared
    assert call(valid=None, out=g["valid"])[0] == _hip.E_LAUNCH and call(occluded=None, ws=g["occluded"])[0] == _hip.E_LAUNCH
    assert call(state=None, out=g["state"])[0] == _hip.E_LAUNCH
    # an fp16 prediction is half as long
    assert call(out=g["pred"] + N_FLOW // 2 - 4, pred_dtype=_hip.F16)[0] == _hip.E_ALIAS
    assert call(out=g["pred"] + N_FLOW // 2, pred_dtype=_hip.F16)[0] == _hip.E_LAUNCH
    # the workspace grows with the chunks: 2 x (CHUNK / 2 + 1) has two of them; the buffers are far apart here
    big = 1 << 30
    far = dict(truth=g["truth"], pred=g["truth"] + big, valid=g["truth"] + 2 * big, occluded=g["truth"] + 3 * big,
               out=g["truth"] + 4 * big, ws=g["truth"] + 5 * big, H=2, W=CHUNK // 2 + 1)
    assert call(state=far["ws"] + 2 * N_WS - 8, **far)[0] == _hip.E_ALIAS
    assert call(state=far["ws"] + 2 * N_WS, **far)[0] == _hip.E_LAUNCH
    assert call(pred=g["truth"] + 8)[0] == _hip.E_LAUNCH                          # the inputs may overlap


def test_order_of_the_checks(call):
    """null, dtype, layout, shape, range, alignment, overlap: the first defect answers."""
    g = call.good
    assert call(ws=None, pred_dtype=7)[0] == _hip.E_NULL
    assert call(pred_dtype=7, layout=7)[0] == _hip.E_DTYPE
    assert call(layout=7, H=0)[0] == _hip.E_LAYOUT
    assert call(H=0, out_abs=0.0)[0] == _hip.E_SHAPE
    assert call(B=2, H=1 << 15, W=1 << 15, t0=float("nan"))[0] == _hip.E_SHAPE
    assert call(out_abs=0.0, out=g["out"] + 1)[0] == _hip.E_RANGE
    assert call(s1=5.0, truth=g["truth"] + 4)[0] == _hip.E_RANGE
    assert call(truth=g["truth"] + 4, ws=g["truth"])[0] == _hip.E_ALIGN
    assert call(state=g["state"] + 4, ws=g["out"])[0] == _hip.E_ALIGN
    with pytest.raises(ValueError, match="overlaps"):
        _hip.check(call(ws=g["out"])[0])

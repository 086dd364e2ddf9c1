"""The argument validation of qpwc_augment_triplet_fwd (include/qpwc_triplet.h), code by code, with HOST pointers:
validation only looks at the values of the pointers and comes before any HIP call.  Without a device a call that
passes it fails at the launch (QPWC_E_LAUNCH); with a device it would launch on host memory, so the module skips itself
there, as tests/test_optim_capi_cpu.py does (which is why these tests are not part of tests/test_triplet_cpu.py: the
GPU suite imports that module)."""
import ctypes

import pytest
import torch

from qpwcnet_amd import _hip, ops

if torch.cuda.is_available():
    pytest.skip("host pointers: a wrongly accepted case would launch on host memory", allow_module_level=True)

B, H, W, h, w = 2, 8, 8, 4, 4
STEP = 16 << 10         # every buffer 16 KiB after the one before
LIMIT = (1 << 31) - 1


@pytest.fixture(scope="module")
def call(hip_lib):
    buf = ctypes.create_string_buffer(8 * STEP + 256)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    names = ("a", "b", "c", "iparams", "fparams", "out_pair", "out_mid")
    good = dict({n: base + i * STEP for i, n in enumerate(names)}, dtype=_hip.U8, B=B, H=H, W=W, h=h, w=w, flags=0,
                layout=_hip.NHWC, stream=None)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
        rc = hip_lib.qpwc_augment_triplet_fwd(a["a"], a["b"], a["c"], a["dtype"], a["B"], a["H"], a["W"], a["iparams"],
                                              a["fparams"], a["h"], a["w"], a["flags"], a["layout"], a["out_pair"],
                                              a["out_mid"], a["stream"])
        return rc, hip_lib.qpwc_last_error().decode()
    run.good, run.keep, run.pointers = good, buf, names
    return run


def test_a_valid_call_reaches_the_launch(call):
    rc, text = call()
    assert rc == _hip.E_LAUNCH and text.startswith("triplet_pixel_kernel: "), (rc, text)
    for ok in (dict(dtype=_hip.F32), dict(flags=_hip.TRIPLET_RAW), dict(layout=_hip.NCHW), dict(h=5, w=7),
               dict(b=call.good["a"], c=call.good["a"])):                       # the frames may be one buffer
        assert call(**ok)[0] == _hip.E_LAUNCH, ok


def test_mode(call):
    for bad in (2, 4, 3, -1, 1 << 30):
        rc, text = call(flags=bad)
        assert rc == _hip.E_MODE and "flags" in text, (bad, text)


def test_null(call):
    for name in call.pointers:
        assert call(**{name: None}) == (_hip.E_NULL, name + " is null")


def test_dtype_and_layout(call):
    for bad in (_hip.F16, 3, -1):
        assert call(dtype=bad)[0] == _hip.E_DTYPE
    for bad in (2, -1):
        rc, text = call(layout=bad)
        assert rc == _hip.E_LAYOUT and text.startswith("Unsupported data format")


def test_shape(call):
    for name in ("B", "H", "W", "h", "w"):
        for bad in (0, -3):
            rc, text = call(**{name: bad})
            assert rc == _hip.E_SHAPE and text.startswith("non-positive extent"), (name, bad, text)


def test_shape_limits(call):
    """H * W, 6 * h * w and the workgroup count B * ceil(h * w / 256): 2^31 - 1 passes, 2^31 (or the next count that can
    be reached) does not.  The buffers of these calls are never touched: validation does not launch, and without a
    device the launch fails."""
    big = 1 << 44                                       # room for the extents below between any two buffers
    far = {n: call.good["a"] + i * big for i, n in enumerate(call.pointers)}
    assert call(H=1, W=LIMIT, **far)[0] == _hip.E_LAUNCH                        # H * W = 2^31 - 1
    assert call(H=2, W=1 << 30, **far)[0] == _hip.E_SHAPE                       # 2^31
    assert call(H=1 << 16, W=1 << 15, **far)[0] == _hip.E_SHAPE
    assert LIMIT // 6 == 357913941
    assert call(B=1, h=1, w=LIMIT // 6, **far)[0] == _hip.E_LAUNCH              # 6 * h * w = 2^31 - 2
    rc, text = call(B=1, h=1, w=LIMIT // 6 + 1, **far)                          # 2^31 + 4
    assert rc == _hip.E_SHAPE and "overflows" in text
    assert call(B=1, h=1 << 15, w=1 << 14, **far)[0] == _hip.E_SHAPE
    assert call(B=LIMIT, h=16, w=16, **far)[0] == _hip.E_LAUNCH                 # 2^31 - 1 workgroups
    assert call(B=LIMIT, h=16, w=17, **far)[0] == _hip.E_SHAPE                  # two per sample
    assert call(B=1 << 23, h=256, w=256, **far)[0] == _hip.E_SHAPE              # 2^23 * 256 = 2^31
    assert call(B=(1 << 23) - 1, h=256, w=256, **far)[0] == _hip.E_LAUNCH


def test_align(call):
    g = call.good
    for name in ("a", "b", "c"):
        for off in (1, 2, 3):                                                   # a uint8 pixel starts on any byte
            assert call(**{name: g[name] + off})[0] == _hip.E_LAUNCH
            assert call(dtype=_hip.F32, **{name: g[name] + off}) == (_hip.E_ALIGN, name + " must be 4-byte aligned")
        assert call(dtype=_hip.F32, **{name: g[name] + 4})[0] == _hip.E_LAUNCH
    for name in ("iparams", "fparams", "out_pair", "out_mid"):
        for off in (1, 2):
            assert call(**{name: g[name] + off}) == (_hip.E_ALIGN, name + " must be 4-byte aligned")
        assert call(**{name: g[name] + 4})[0] == _hip.E_LAUNCH


def test_alias(call):
    g = call.good
    src, n_pair, n_mid = B * H * W * 3, B * h * w * 6 * 4, B * h * w * 3 * 4
    for out in ("out_pair", "out_mid"):
        for name in ("a", "b", "c", "iparams", "fparams"):
            assert call(**{out: g[name]}) == (_hip.E_ALIAS, "{} overlaps {}".format(out, name))
    assert call(out_mid=g["out_pair"]) == (_hip.E_ALIAS, "out_mid overlaps out_pair")
    assert call(out_mid=g["out_pair"] + n_pair - 4)[0] == _hip.E_ALIAS          # the last float of the pair
    assert call(out_mid=g["out_pair"] + n_pair)[0] == _hip.E_LAUNCH             # adjacent is fine
    assert call(out_pair=g["out_mid"] + n_mid - 4)[0] == _hip.E_ALIAS
    assert call(out_pair=g["a"] + src - 4)[0] == _hip.E_ALIAS                   # the last bytes of a uint8 frame
    assert call(out_pair=g["a"] + src)[0] == _hip.E_LAUNCH
    assert call(dtype=_hip.F32, out_pair=g["a"] + 4 * src - 4)[0] == _hip.E_ALIAS
    for name, n in (("iparams", B * 16), ("fparams", B * 64)):
        assert call(out_mid=g[name] + n - 4)[0] == _hip.E_ALIAS and call(out_mid=g[name] + n)[0] == _hip.E_LAUNCH


def test_order_of_the_checks(call):
    """flags, null, dtype, layout, shape, alignment, overlap: the first defect answers."""
    g = call.good
    assert call(flags=2, a=None)[0] == _hip.E_MODE
    assert call(a=None, dtype=7)[0] == _hip.E_NULL
    assert call(dtype=7, layout=7)[0] == _hip.E_DTYPE
    assert call(layout=7, B=0)[0] == _hip.E_LAYOUT
    assert call(B=0, iparams=g["iparams"] + 1)[0] == _hip.E_SHAPE
    assert call(iparams=g["iparams"] + 1, out_mid=g["out_pair"])[0] == _hip.E_ALIGN
    with pytest.raises(ValueError, match="flags"):
        _hip.check(call(flags=2)[0])


def test_kernel_query_is_host_only(hip_lib):
    aligned = 1 << 20
    pick = lambda B, h, w, a=aligned, b=aligned: hip_lib.qpwc_augment_triplet_fwd_kernel(B, h, w, a, b).decode()
    assert pick(4, 24, 40) == "triplet_pixel_kernel<vec4>"                      # the GPU suite's main case
    assert pick(2, 5, 7) == "triplet_pixel_kernel<scalar>"                      # 35 pixels: no multiple of 4
    assert pick(4, 12, 20) == "triplet_pixel_kernel<vec4>"
    assert pick(8, 256, 512) == "triplet_pixel_kernel<vec4>"                    # the trainer's shape
    assert pick(1, 2, 3) == "triplet_pixel_kernel<scalar>" and pick(1, 2, 2) == "triplet_pixel_kernel<vec4>"
    for off in (4, 8, 12):                                                      # an output off the 16-byte grid
        assert pick(4, 24, 40, aligned + off) == "triplet_pixel_kernel<scalar>"
        assert pick(4, 24, 40, aligned, aligned + off) == "triplet_pixel_kernel<scalar>"
    assert pick(4, 24, 40, aligned + 16, aligned + 32) == "triplet_pixel_kernel<vec4>"
    assert pick(0, 24, 40) == "" and pick(1, 24, 0) == "" and pick(1, -1, 4) == ""
    assert pick(1, 24, 40, None) == "" and pick(1, 24, 40, aligned, None) == ""
    assert pick(1, 1, LIMIT // 6) != "" and pick(1, 1, LIMIT // 6 + 1) == ""
    assert pick(LIMIT, 16, 16) == "triplet_pixel_kernel<vec4>" and pick(LIMIT, 16, 17) == ""
    assert ops.augment_triplet_kernel(4, 24, 40) == "triplet_pixel_kernel<vec4>"
    assert ops.augment_triplet_kernel(2, 5, 7) == "triplet_pixel_kernel<scalar>"
    assert ops.augment_triplet_kernel(0, 5, 7) == ""

"""The argument validation of qpwc_agc_adam_step (include/qpwc_optim.h), code by code, with HOST pointers: validation
only looks at the values of the two table pointers and comes before any HIP call.  Without a device a call that passes
it fails at the launch (QPWC_E_LAUNCH); with a device it would launch on host memory, so the module skips itself there,
as tests/test_capi_contract_cpu.py does (which is why these tests are not part of tests/test_optim_cpu.py: the GPU
suite imports that module)."""
import ctypes
import math

import pytest
import torch

from qpwcnet_amd import _hip

if torch.cuda.is_available():
    pytest.skip("host pointers: a wrongly accepted case would launch on host memory", allow_module_level=True)

N_TENSORS, N_UNITS = 3, 5


@pytest.fixture(scope="module")
def call(hip_lib):
    buf = ctypes.create_string_buffer(4096 + 16)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    good = dict(tensors=base, n_tensors=N_TENSORS, units=base + 1024, n_units=N_UNITS, alpha=1e-4, beta1=0.9,
                beta2=0.999, epsilon=1e-7, clip_factor=0.01, agc_eps=1e-3, stream=None)

    def run(**changed):
        a = dict(good, **changed)
        assert hip_lib.qpwc_device_copy(None, None, 0, None) == _hip.E_NULL    # the error text is sticky: reset it
        rc = hip_lib.qpwc_agc_adam_step(a["tensors"], a["n_tensors"], a["units"], a["n_units"], a["alpha"], a["beta1"],
                                        a["beta2"], a["epsilon"], a["clip_factor"], a["agc_eps"], a["stream"])
        return rc, hip_lib.qpwc_last_error().decode()
    run.base, run.keep = base, buf
    return run


def test_a_valid_call_reaches_the_launch(call):
    rc, text = call()
    assert rc == _hip.E_LAUNCH and text.startswith("agc_adam_kernel: "), (rc, text)
    # clip_factor <= 0 (no clipping) and the largest table are valid too
    assert call(clip_factor=0.0)[0] == _hip.E_LAUNCH and call(clip_factor=-1.0)[0] == _hip.E_LAUNCH
    assert call(beta1=0.0, beta2=0.0)[0] == _hip.E_LAUNCH


def test_null(call):
    assert call(tensors=None) == (_hip.E_NULL, "tensors is null")
    assert call(units=None) == (_hip.E_NULL, "units is null")


def test_shape(call):
    for bad in (0, -1):
        assert call(n_tensors=bad)[0] == _hip.E_SHAPE
        assert call(n_units=bad)[0] == _hip.E_SHAPE
    assert call(n_units=1 << 31) == (_hip.E_SHAPE, "n_units=2147483648 outside [1, 2147483647]")
    assert call(n_units=1 << 40)[0] == _hip.E_SHAPE


def test_range(call):
    for key in ("beta1", "beta2"):
        for bad in (1.0, -0.1, 1.5, math.nan):
            rc, text = call(**{key: bad})
            assert rc == _hip.E_RANGE and text.startswith(key + "="), (key, bad, text)
    for key in ("epsilon", "agc_eps"):
        for bad in (0.0, -1e-7, math.nan):
            rc, text = call(**{key: bad})
            assert rc == _hip.E_RANGE and text.startswith(key + "="), (key, bad, text)
    for bad in (math.inf, -math.inf, math.nan):
        rc, text = call(alpha=bad)
        assert rc == _hip.E_RANGE and "not finite" in text
    assert call(alpha=0.0)[0] == _hip.E_LAUNCH and call(alpha=-1.0)[0] == _hip.E_LAUNCH


def test_align(call):
    assert call(tensors=call.base + 4) == (_hip.E_ALIGN, "tensors must be 8-byte aligned")
    assert call(units=call.base + 1024 + 4) == (_hip.E_ALIGN, "units must be 8-byte aligned")


def test_alias(call):
    assert call(units=call.base) == (_hip.E_ALIAS, "units overlaps tensors")
    assert call(units=call.base + 32 * N_TENSORS - 8)[0] == _hip.E_ALIAS      # the last 8 bytes of the tensor table
    assert call(units=call.base + 32 * N_TENSORS)[0] == _hip.E_LAUNCH          # adjacent is fine
    assert call(tensors=call.base + 1024 + 24 * N_UNITS - 8)[0] == _hip.E_ALIAS


def test_order_of_the_checks(call):
    """null, shape, range, alignment, overlap: the first defect answers."""
    assert call(tensors=None, n_tensors=0)[0] == _hip.E_NULL
    assert call(n_units=0, beta1=2.0)[0] == _hip.E_SHAPE
    assert call(beta2=2.0, units=call.base + 4)[0] == _hip.E_RANGE
    assert call(tensors=call.base + 4, units=call.base + 4)[0] == _hip.E_ALIGN


def test_kernel_query_is_host_only(hip_lib):
    assert hip_lib.qpwc_agc_adam_step_kernel(1) == b"agc_adam_kernel<one unit per wave>"
    assert hip_lib.qpwc_agc_adam_step_kernel((1 << 31) - 1) == b"agc_adam_kernel<grid-stride>"
    assert hip_lib.qpwc_agc_adam_step_kernel(1 << 31) == b"" and hip_lib.qpwc_agc_adam_step_kernel(-3) == b""

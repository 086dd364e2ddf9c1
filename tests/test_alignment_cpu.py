"""The off-grid dispatch of the launchers, as far as the host alone can tell.

About twenty launchers in qpwcnet_amd/csrc look at the low bits of a pointer and pick a vector or an element-wise form;
tests/test_gpu_alignment.py runs every one of them with an operand off the 16-byte grid.  Here, without a GPU:
  * the host-only form queries name the fallback for such a pointer;
  * SITES lists, per source file, how many lines test a pointer's low bits.  It is compared with the sources, so that a
    new dispatch on alignment cannot arrive without a case on the GPU;
  * qpwc_warp_cost_volume_fwd refuses a prv / nxt off the grid with QPWC_E_ALIGN, by name, before anything is launched
    (its kernels have no element-wise form)."""
import ctypes
import glob
import json
import os

import pytest
import torch

from qpwcnet_amd import _hip

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")
GRID, OFF = 1 << 20, (1 << 20) + 4          # addresses the queries only look at

# source file -> lines that cast a pointer to uintptr_t to test its low bits (csrc/*.hip and csrc/*.inc; capi.hip, the
# boundary, validates and does not dispatch).  The case of tests/test_gpu_alignment.py that reaches each:
SITES = {
    "warp.hip": 2,               # test_warp_forward_off_grid, test_warp_channels_first_off_grid_image
    "cost_volume.hip": 2,        # test_cost_volume_inputs_off_grid (C = 4: the tiled kernels' `fast`)
    "cost_volume_mfma.hip": 5,   # ..._inputs_off_grid (C = 16, 32), ..._output_off_grid, ..._84_channel_..., test_fused_..
    "optflow.hip": 4,            # test_dwconv3x3_fp16_off_grid (2), test_sepconv3x3_fp32_..., test_upsample2x_flow_* (2)
    "sepconv_x3.inc": 1,         # none: see test_sites_without_a_case
    "sepconv_f16.hip": 3,        # test_sepconv3x3_fp16_tail_taps_and_narrow_form
    "vis.hip": 2,                # test_flow_to_image_flows_off_grid, test_flow_to_image_outputs_off_grid
    "optim.hip": 3,              # test_optimizer_step_mismatched_phases
    "loss.hip": 4,               # test_loss_backward_off_grid_dpred (2); ground truth (2): test_gpu_training_scale.py
    "epe.hip": 1,                # test_gpu_training_scale.py::test_epe_multi_plain_fp32_loops
    "augment.hip": 1,            # test_gpu_augment.py (outputs); the query below
    "triplet.hip": 1,            # test_gpu_triplet.py (outputs); the query below
}
# sepconv_x3.inc's line is sepconv_x3_sources_ok: no form is chosen there, qpwc_sepconv3x3_x3_fwd refuses an off-grid
# source that is not a short tail with QPWC_E_ALIGN, and the contract golden pins that answer (checked below)
NO_CASE = ("sepconv_x3.inc",)


def _pointer_tests(path):
    n = 0
    for line in open(path):
        code = line.split("//")[0]
        if "uintptr_t" in code:
            n += 1
    return n


def test_every_alignment_dispatch_site_is_listed():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.inc"))):
        name = os.path.basename(path)
        if name == "capi.hip":
            continue
        n = _pointer_tests(path)
        if n:
            found[name] = n
    assert found == SITES, ("the lines that test a pointer's low bits changed in {}: give the new dispatch a case with an "
                            "off-grid operand in tests/test_gpu_alignment.py, then update SITES".format(
                                sorted(k for k in set(found) | set(SITES) if found.get(k) != SITES.get(k))))


def test_sites_without_a_case():
    assert set(NO_CASE) <= set(SITES)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_contract.json")) as f:
        rec = json.load(f)["functions"]["qpwc_sepconv3x3_x3_fwd"]
    base = rec["base"][0]
    moved = [ret for diff, ret, _ in rec["cases"]
             if len(diff) == 2 and diff[0] == 0 and diff[1] is not None and diff[1][1:] == base[1:]
             and diff[1][0] is not None and diff[1][0] - base[0] in (4, 8)]
    assert moved == [_hip.E_ALIGN, _hip.E_ALIGN], moved


def _ptrs(*values):
    return (ctypes.c_void_p * len(values))(*values)


def _ints(*values):
    return (ctypes.c_int * len(values))(*values)


def test_form_queries_name_the_fallback_for_off_grid_pointers(hip_lib):
    L = hip_lib
    # flow_to_image: 20 x 25 pictures (a multiple of 4 pixels); any one output off the grid forces <scalar> for all
    for dt, off in ((_hip.F32, 4), (_hip.U8, 1)):
        for layout in (_hip.NHWC, _hip.NCHW):
            q = lambda a, b: L.qpwc_flow_to_image_fwd_kernel(2, 2, _ints(20, 20), _ints(25, 25), dt, layout,
                                                             _ptrs(a, b)).decode()
            assert q(GRID, 2 * GRID) == "flow_to_image_kernel<vec4>"
            assert q(GRID + off, 2 * GRID) == "flow_to_image_kernel<scalar>"
            assert q(GRID, 2 * GRID + off) == "flow_to_image_kernel<scalar>"
    # the input pipelines: h * w = 240
    assert L.qpwc_augment_fwd_kernel(2, 12, 20, GRID, 2 * GRID) == b"augment_pixel_kernel<vec4>"
    assert L.qpwc_augment_fwd_kernel(2, 12, 20, OFF, 2 * GRID) == b"augment_pixel_kernel<scalar>"
    assert L.qpwc_augment_fwd_kernel(2, 12, 20, GRID, 2 * GRID + 8) == b"augment_pixel_kernel<scalar>"
    assert L.qpwc_augment_triplet_fwd_kernel(2, 12, 20, GRID, 2 * GRID) == b"triplet_pixel_kernel<vec4>"
    assert L.qpwc_augment_triplet_fwd_kernel(2, 12, 20, OFF, 2 * GRID) == b"triplet_pixel_kernel<scalar>"
    assert L.qpwc_augment_triplet_fwd_kernel(2, 12, 20, GRID, 2 * GRID + 8) == b"triplet_pixel_kernel<scalar>"
    # the area loss: nested powers of two on 32 x 32 tiles
    q = lambda p: L.qpwc_loss_fwd_kernel(_hip.LOSS_FLOW_MSE_V2, p, 1, 64, 64, 2, _ints(32, 16), _ints(32, 16), 2).decode()
    assert q(GRID) == "loss_area_tile_kernel"
    assert q(OFF) == "loss_pixel_kernel" and q(GRID + 8) == "loss_pixel_kernel"


@pytest.mark.parametrize("which", ["prv", "nxt"])
@pytest.mark.parametrize("off", [4, 8])
def test_fused_front_end_refuses_off_grid_images_by_name(hip_lib, which, off):
    """QPWC_E_ALIGN with the operand and the 16 bytes in the text, from the validator: without a device the aligned call
    gets as far as its launch (QPWC_E_LAUNCH), the off-grid one does not.  With a device the operands are real device
    memory, so that a call that is wrongly let through computes on it."""
    B, H, W, C = 1, 8, 8, 4
    if torch.cuda.is_available():
        mem = torch.zeros(4 * (1 << 16), device="cuda:0")
        base, stream = mem.data_ptr(), torch.cuda.current_stream().cuda_stream
    else:
        mem, base, stream = None, GRID, None
    slot = 1 << 16                         # bytes: far more than any operand here
    prv, nxt, flo, out = (base + k * slot for k in range(4))
    args = {"prv": prv, "nxt": nxt}
    args[which] += off
    call = lambda p, n: hip_lib.qpwc_warp_cost_volume_fwd(p, n, flo, out, B, H, W, C, 4, _hip.F32, 0.1, 81, 0, stream)
    rc = call(args["prv"], args["nxt"])
    text = hip_lib.qpwc_last_error().decode()
    assert rc == _hip.E_ALIGN, (rc, text)
    assert text == "{} must be 16-byte aligned for the fused warp+cost volume".format(which)
    with pytest.raises(ValueError, match="{} must be 16-byte aligned".format(which)):
        _hip.check(rc)
    # what cost_volume_impl's own message describes still gets it: a channel count the fused kernels do not take
    rc = hip_lib.qpwc_warp_cost_volume_fwd(args["prv"], args["nxt"], flo, out, B, H, W, 3, 4, _hip.F32, 0.1, 81, 0, stream)
    assert rc == _hip.E_SHAPE and "C % 4 == 0 (got C=3 r=4)" in hip_lib.qpwc_last_error().decode()
    rc = call(prv, nxt)
    assert rc == (0 if mem is not None else _hip.E_LAUNCH), hip_lib.qpwc_last_error().decode()
    if mem is not None:
        torch.cuda.synchronize()

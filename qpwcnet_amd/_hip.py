"""ctypes binding of ``libqpwc_hip.so`` (C ABI declared in ``include/qpwc.h``).

There is deliberately no fallback: if the library is missing or a call fails
the error propagates.  PyTorch is used only for device memory and streams; the
ABI itself sees raw device pointers.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# QPWC_HIP_LIB: another build of the same library (kernel A/B experiments); default = in-tree build
LIB_PATH = os.environ.get("QPWC_HIP_LIB") or os.path.join(_HERE, "csrc", "libqpwc_hip.so")

NHWC, NCHW = 0, 1
F32, F16, U8 = 0, 1, 2
AUGMENT_COLOR, AUGMENT_RAW = 1, 2
TRIPLET_RAW = 1
VIS_MAX_TILE, VIS_TILE = 2048, 1024     # csrc/vis.hip: source pixels per partial maximum, output pixels per workgroup
REVIEW_TILE = 256                       # csrc/review.hip: pixels per workgroup of the panel launch
QUALITY_TILE = (16, 32)                 # csrc/quality.hip: SSIM positions (rows, columns) per workgroup
QUALITY_CLIP, QUALITY_U8 = 1, 2
FLOW_QUALITY_CHUNK = 4096               # csrc/flow_quality.hip: consecutive pixels per workgroup of the tile launch
WARP_CLAMP, WARP_TFWARP = 0, 1
BCAST_B, BCAST_H, BCAST_W = 1, 2, 4
LOSS_FLOW_MSE_V2, LOSS_FLOW_MSE, LOSS_FLOW_FINETUNE, LOSS_AUTORESIZE_MSE = 0, 1, 2, 3

E_NULL, E_LAYOUT, E_DTYPE, E_SHAPE, E_RANGE, E_MODE, E_ALIAS, E_LAUNCH, E_ALIGN, E_STRIDE, \
    E_NODEVICE = range(-1, -12, -1)
_ARGUMENT_ERRORS = {E_NULL, E_LAYOUT, E_DTYPE, E_SHAPE, E_RANGE, E_MODE, E_ALIAS, E_ALIGN, E_STRIDE}

_vp, _ci, _cf, _i64, _str = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64, ctypes.c_char_p
_pvp, _pi, _pi64 = ctypes.POINTER(_vp), ctypes.POINTER(_ci), ctypes.POINTER(_i64)
_sepconv_fwd = [_pvp, _pi, _pi64, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]
_upconv_fwd = [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _i64, _vp]
_upconv_cat_fwd = [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _ci, _ci, _ci, _ci, _ci, _i64, _vp]

# The C ABI, once: name -> (restype, argtypes) for every symbol include/qpwc.h declares, in the header's order.
# lib() applies it; tests/test_capi_prototypes_cpu.py holds it to the header (an `int` where the header says
# `int64_t` would corrupt an argument silently).
PROTOTYPES = {
    "qpwc_version": (_ci, []),
    "qpwc_last_error": (_str, []),
    "qpwc_strerror": (_str, [_ci]),
    "qpwc_build_info": (_str, []),
    "qpwc_layout_transpose_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_copy_pixels_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _pi64, _pi64, _ci, _vp]),
    "qpwc_device_copy": (_ci, [_vp, _vp, _i64, _vp]),
    "qpwc_clock_probe": (_ci, [_vp, _ci, _ci, _vp]),
    "qpwc_cost_volume_fwd": (_ci, [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cf, _vp]),
    "qpwc_cost_volume_fwd_strided": (_ci, [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cf, _i64, _i64, _vp]),
    "qpwc_warp_fwd": (_ci, [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_cost_volume_bwd": (_ci, [_vp] * 6 + [_ci, _ci, _ci, _ci, _ci, _ci, _cf, _vp]),
    "qpwc_warp_bwd_workspace_floats": (_i64, [_ci, _ci, _ci, _ci, _ci]),
    "qpwc_warp_bwd": (_ci, [_vp] * 6 + [_ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_loss_workspace_floats": (_i64, [_ci, _ci, _ci, _ci, _ci, _pi, _pi, _ci]),
    "qpwc_loss_fwd": (_ci, [_ci, _cf, _cf, _vp, _ci, _ci, _ci, _ci, _ci, _pvp, _pi, _pi, _pi, _ci, _vp, _pvp, _pvp,
                            _vp, _vp]),
    "qpwc_loss_fwd_kernel": (_str, [_ci, _vp, _ci, _ci, _ci, _ci, _pi, _pi, _ci]),
    "qpwc_loss_bwd": (_ci, [_pvp, _vp, _pvp, _pi64, _pi, _ci, _vp]),
    "qpwc_augment_workspace_floats": (_i64, [_ci, _ci, _ci]),
    "qpwc_augment_fwd": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp]),
    "qpwc_augment_fwd_kernel": (_str, [_ci, _ci, _ci, _vp, _vp]),
    "qpwc_warp_cost_volume_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cf, _i64, _i64, _vp]),
    "qpwc_cost_volume_kernel": (_str, [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _i64, _ci]),
    "qpwc_epe_workspace_floats": (_ci, []),
    "qpwc_epe_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_epe_multi_workspace_floats": (_ci, []),
    "qpwc_epe_multi_fwd": (_ci, [_pvp, _pvp, _pi64, _pi64, _ci, _vp, _vp, _vp]),
    "qpwc_epe_multi_mixed_fwd": (_ci, [_pvp, _pvp, _pi64, _pi64, _pi, _ci, _vp, _vp, _vp]),
    "qpwc_cost_volume_to_flow_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _i64, _ci, _ci, _vp]),
    "qpwc_dwconv3x3_fwd": (_ci, [_pvp, _pi, _pi64, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_sepconv3x3_fwd": (_ci, _sepconv_fwd),
    "qpwc_sepconv3x3_bwd_workspace_floats": (_i64, [_ci, _ci, _ci, _ci, _ci]),
    "qpwc_sepconv3x3_bwd": (_ci, [_pvp, _pi, _pi64, _ci, _ci, _vp, _vp, _vp, _vp, _pvp, _vp, _vp, _vp, _vp,
                                  _ci, _ci, _ci, _ci, _vp]),
    "qpwc_sepconv3x3_x3_fwd": (_ci, _sepconv_fwd),
    "qpwc_sepconv3x3_f16_fwd": (_ci, _sepconv_fwd),
    "qpwc_flow_head_param_floats": (_ci, []),
    "qpwc_flow_head_fwd": (_ci, [_vp, _vp, _vp, _ci, _ci, _ci, _cf, _ci, _ci, _vp]),
    "qpwc_flow_head_stats_workspace_floats": (_i64, [_ci, _ci, _ci]),
    "qpwc_flow_head_stats_fwd": (_ci, [_vp] * 8 + [_cf, _cf, _vp, _vp, _vp, _ci, _ci, _ci, _vp]),
    "qpwc_flow_head_bwd_workspace_floats": (_i64, [_ci, _ci, _ci]),
    "qpwc_flow_head_bwd": (_ci, [_vp, _vp, _vp, _cf, _ci, _cf] + [_vp] * 8 + [_ci, _ci, _ci, _vp]),
    "qpwc_pointwise_bias_fwd": (_ci, [_vp, _vp, _vp, _vp, _i64, _ci, _ci, _vp]),
    "qpwc_flow_head_up_fwd": (_ci, [_vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cf, _cf, _ci, _vp]),
    "qpwc_optflow_tail_fwd": (_ci, [_vp] * 9 + [_ci, _ci, _ci, _cf, _ci, _ci, _vp]),
    "qpwc_bias_mish_fwd": (_ci, [_vp, _vp, _i64, _ci, _ci, _vp]),
    "qpwc_bias_mish_pad_fwd": (_ci, [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _i64, _ci, _vp]),
    "qpwc_split_frames_pad_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_upsample2x_flow_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _cf, _ci, _ci, _ci, _vp]),
    "qpwc_upsample2x_flow_bwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _cf, _vp]),
    "qpwc_invert_flow_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_occlusion_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_conv3x3_mish_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_conv3x3_mish_x3_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_split_bf16x3_fwd": (_ci, [_vp, _vp, ctypes.c_longlong, _vp]),
    "qpwc_conv3x3_mish_f16_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_first_conv_mish_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_first_conv_mish_f16_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_conv3x3s2_mish_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _vp]),
    "qpwc_conv3x3s2_mish_c_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_conv3x3s2_mish_x3_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_conv3x3s2_mish_f16_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_conv3x3_same_fwd": (_ci, [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_conv3x3_same_bwd_workspace_floats": (_i64, [_ci, _ci, _ci, _ci, _ci, _ci]),
    "qpwc_conv3x3_same_bwd": (_ci, [_vp] * 8 + [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_upconv4x4s2_mish_fwd": (_ci, _upconv_fwd),
    "qpwc_upconv4x4s2_mish_x3_fwd": (_ci, _upconv_fwd),
    "qpwc_upconv4x4s2_mish_f16_fwd": (_ci, _upconv_fwd),
    "qpwc_upconv4x4s2_mish_cat_fwd": (_ci, _upconv_cat_fwd),
    "qpwc_upconv4x4s2_mish_cat_f16_fwd": (_ci, _upconv_cat_fwd),
    "qpwc_upconv4x4s2_bwd_workspace_floats": (_i64, [_ci, _ci, _ci, _ci, _ci]),
    "qpwc_upconv4x4s2_bwd": (_ci, [_vp] * 4 + [_i64] + [_vp] * 4 + [_ci, _ci, _ci, _ci, _ci, _ci, _vp]),
    "qpwc_image_head_fwd": (_ci, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "qpwc_image_head_bwd_workspace_floats": (_i64, [_i64]),
    "qpwc_image_head_bwd": (_ci, [_vp] * 7 + [_i64, _vp]),
    "qpwc_upsample2x_image_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _cf, _vp]),
    "qpwc_upsample2x_image_bwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _cf, _vp]),
    "qpwc_avgpool_pyramid_fwd": (_ci, [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp]),
}
SYMBOLS = tuple(PROTOTYPES)

# The trainer's update step, declared in include/qpwc_optim.h: a table of its own, applied after PROTOTYPES and held
# to its header by tests/test_optim_cpu.py.
OPTIM_PROTOTYPES = {
    "qpwc_agc_adam_step": (_ci, [_vp, _ci, _vp, _i64, _cf, _cf, _cf, _cf, _cf, _cf, _vp]),
    "qpwc_agc_adam_step_kernel": (_str, [_i64]),
}

# The frame interpolator's input pipeline, declared in include/qpwc_triplet.h: a table of its own under the same rules,
# held to its header by tests/test_triplet_cpu.py.
TRIPLET_PROTOTYPES = {
    "qpwc_augment_triplet_fwd": (_ci, [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp]),
    "qpwc_augment_triplet_fwd_kernel": (_str, [_ci, _ci, _ci, _vp, _vp]),
}

# The trainer's flow panels, declared in include/qpwc_vis.h: a table of its own under the same rules, held to its header
# by tests/test_vis_capi_cpu.py.
VIS_PROTOTYPES = {
    "qpwc_flow_to_image_workspace_floats": (_i64, [_ci, _ci, _pi, _pi]),
    "qpwc_flow_to_image_fwd": (_ci, [_pvp, _pi, _pi, _pi, _ci, _ci, _ci, _pvp, _pi, _pi, _ci, _ci, _vp, _vp]),
    "qpwc_flow_to_image_fwd_kernel": (_str, [_ci, _ci, _pi, _pi, _ci, _ci, _pvp]),
}

# The interpolator's image quality (MSE, PSNR, SSIM), declared in include/qpwc_quality.h: a table of its own under the
# same rules, held to its header by tests/test_quality_cpu.py.
QUALITY_PROTOTYPES = {
    "qpwc_image_quality_workspace_floats": (_i64, [_ci, _ci, _ci, _ci]),
    "qpwc_image_quality_fwd": (_ci, [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cf, _cf, _ci, _cf, _vp, _vp, _vp, _vp]),
    "qpwc_image_quality_fwd_kernel": (_str, [_ci, _ci, _ci, _ci]),
}

# The inference review panels of both test scripts, declared in include/qpwc_review.h: a table of its own under the same
# rules, held to its header by tests/test_review_cpu.py.
REVIEW_PROTOTYPES = {
    "qpwc_review_workspace_floats": (_i64, [_ci, _ci, _ci, _ci]),
    "qpwc_inference_panels_fwd": (_ci, [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _pvp, _ci, _ci, _ci, _vp, _vp]),
    "qpwc_interpolation_panels_fwd": (_ci, [_vp, _vp, _vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _pvp, _ci, _ci, _ci,
                                            _vp, _vp]),
    "qpwc_review_panels_fwd_kernel": (_str, [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci]),
}

# The flow evaluation metrics (EPE splits, Fl-all, accuracy, AAE), declared in include/qpwc_flow_quality.h: a table of
# its own under the same rules, held to its header by tests/test_flow_quality_cpu.py.
FLOW_QUALITY_PROTOTYPES = {
    "qpwc_flow_quality_workspace_floats": (_i64, [_ci, _ci, _ci]),
    "qpwc_flow_quality_fwd": (_ci, [_vp, _vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci] + [_cf] * 7 + [_vp, _vp, _vp, _vp]),
    "qpwc_flow_quality_fwd_kernel": (_str, [_ci, _ci, _ci]),
}

# The valid-masked flow losses, declared in include/qpwc_masked_loss.h: a table of its own under the same rules, held to
# its header by tests/test_masked_loss_cpu.py.
MASKED_LOSS_PROTOTYPES = {
    "qpwc_masked_loss_workspace_floats": (_i64, [_ci, _ci, _ci, _ci, _ci, _pi, _pi, _ci]),
    "qpwc_masked_loss_fwd": (_ci, [_ci, _cf, _cf, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _pvp, _pi, _pi, _pi, _ci, _vp, _vp,
                                   _pvp, _pvp, _pvp, _vp, _vp]),
    "qpwc_masked_loss_fwd_kernel": (_str, [_ci, _ci, _ci, _ci, _ci, _pi, _pi, _ci]),
    "qpwc_masked_loss_bwd": (_ci, [_ci, _pvp, _vp, _vp, _pvp, _pi64, _pi, _ci, _vp]),
}
MASKED_LOSS_TILE_BLOCKS, MASKED_LOSS_PIX_BLOCKS = 2048, 1024   # csrc/masked_loss.hip: the grid caps of its two forward kernels
MASKED_LOSS_THREADS, MASKED_LOSS_TILE = 256, 32                # threads per workgroup, tile edge

# The sparse-ground-truth input pipeline, declared in include/qpwc_sparse_augment.h: a table of its own under the same
# rules, held to its header by tests/test_sparse_augment_capi_cpu.py.
SPARSE_AUGMENT_PROTOTYPES = {
    "qpwc_augment_sparse_fwd": (_ci, [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp,
                                      _vp]),
    "qpwc_augment_sparse_fwd_kernel": (_str, [_ci, _ci, _ci]),
}

# The label-free flow losses (census / Charbonnier photometric term + edge-aware smoothness), declared in
# include/qpwc_unsup_loss.h: a table of its own under the same rules, held to its header by
# tests/test_unsup_loss_capi_cpu.py.
UNSUP_LOSS_PROTOTYPES = {
    "qpwc_unsup_loss_workspace_floats": (_i64, [_ci, _ci, _pi, _pi, _ci]),
    "qpwc_unsup_loss_fwd": (_ci, [_ci, _cf, _cf, _cf, _cf, _cf, _pvp, _pvp, _pvp, _pvp, _ci, _pi, _pi, _pi, _ci, _ci,
                                  _vp, _vp, _vp, _vp, _vp, _vp]),
    "qpwc_unsup_loss_fwd_kernel": (_str, [_ci, _ci, _pi, _pi, _ci]),
    "qpwc_unsup_loss_bwd": (_ci, [_ci, _cf, _cf, _pvp, _vp, _vp, _vp, _pvp, _ci, _pi, _pi, _pi, _ci, _ci, _vp]),
}
UNSUP_CENSUS, UNSUP_CHARBONNIER = 0, 1
UNSUP_LOSS_TILE = (8, 32)               # csrc/unsup_loss.hip: pixels (rows, columns) per workgroup
UNSUP_LOSS_PLANES = 7                   # floats it saves per pixel for the backward

# The interpolator's SSIM + Charbonnier training loss, declared in include/qpwc_image_loss.h: a table of its own under the
# same rules, held to its header by tests/test_image_loss_capi_cpu.py.
IMAGE_LOSS_PROTOTYPES = {
    "qpwc_image_loss_workspace_floats": (_i64, [_ci, _ci, _pi, _pi, _ci]),
    "qpwc_image_loss_fwd": (_ci, [_cf, _cf, _cf, _cf, _cf, _pvp, _pvp, _ci, _ci, _pi, _pi, _pi, _ci, _ci, _vp, _vp, _vp,
                                  _vp, _vp]),
    "qpwc_image_loss_fwd_kernel": (_str, [_ci, _ci, _pi, _pi, _ci]),
    "qpwc_image_loss_bwd": (_ci, [_cf, _cf, _cf, _cf, _pvp, _pvp, _vp, _vp, _pvp, _ci, _ci, _pi, _pi, _pi, _ci, _ci, _vp]),
}
IMAGE_LOSS_TILE = (16, 32)              # csrc/image_loss.hip: pixels (rows, columns) per workgroup
IMAGE_LOSS_PLANES = 3                   # floats it saves per SSIM position and channel for the backward

_lib = None


def build(verbose=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles on CPU)."""
    import subprocess
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    if not verbose:
        cmd.append("-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "qpwcnet_amd: {} is missing -- build it with `make -C qpwcnet_amd/csrc` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU "
            "fallback.".format(LIB_PATH))
    # PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Load it
    # FIRST so that our NEEDED entry binds to that same runtime instance: a second
    # HIP runtime in the process cannot see torch's streams or allocations
    # ("no ROCm-capable device is detected" at the first launch).
    import torch
    hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip_rt):
        ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
    L = ctypes.CDLL(LIB_PATH)
    later = dict(OPTIM_PROTOTYPES, **TRIPLET_PROTOTYPES, **VIS_PROTOTYPES, **QUALITY_PROTOTYPES,
                 **REVIEW_PROTOTYPES, **FLOW_QUALITY_PROTOTYPES, **MASKED_LOSS_PROTOTYPES,
                 **SPARSE_AUGMENT_PROTOTYPES, **UNSUP_LOSS_PROTOTYPES, **IMAGE_LOSS_PROTOTYPES)
    for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(later.items()):
        if name in later and not hasattr(L, name):
            continue        # QPWC_HIP_LIB naming an older build: the call itself fails, by name (AttributeError)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = L
    return L


def build_info():
    """{'path', 'version', 'build', 'product'} of the loaded library: bench.py prints it, so that a number
    from another build (QPWC_HIP_LIB -> e.g. `make ab`) can never pass for the product's."""
    L = lib()
    info = L.qpwc_build_info().decode()
    return {"path": LIB_PATH, "version": int(L.qpwc_version()), "build": info,
            "product": not os.environ.get("QPWC_HIP_LIB")}


def source_sha256(names=("cost_volume_mfma.hip", "cost_volume.hip", "warp.hip", "common.h")):
    """sha256 over the named kernel sources (qpwcnet_amd/csrc): stamps profiles/traffic.json, and
    bench.py drops `roofline.traffic` when the kernels have changed since the counters were read."""
    import hashlib
    h = hashlib.sha256()
    for n in names:
        with open(os.path.join(_HERE, "csrc", n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def check(rc):
    """Map a QPWC_E_* code to the exception the reference would raise."""
    if rc == 0:
        return
    L = lib()
    msg = "{} ({})".format(L.qpwc_last_error().decode(), L.qpwc_strerror(rc).decode())
    if rc in _ARGUMENT_ERRORS:
        raise ValueError(msg)
    raise RuntimeError(msg)

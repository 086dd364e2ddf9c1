"""The shapes of tests/test_gpu_training_scale.py still make their loops take more than one trip.

The grid constants are read from the kernel sources.  Raising one of them would otherwise turn those tests back into
one-trip tests, and nothing would notice.  The kernel choice of the loss cases is checked on the host through the C
ABI's own selection rule."""
import ctypes
import math
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_training_scale import CASES  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")


def _constants(name, *keys):
    text = open(os.path.join(CSRC, name)).read()
    out = {}
    for k in keys:
        m = re.findall(r"constexpr\s+int\s+{}\s*=\s*(\d+)\s*;".format(k), text)
        assert len(m) == 1, (name, k, m)
        out[k] = int(m[0])
    return out


LOSS = _constants("loss.hip", "kLossTileBlocks", "kLossPixBlocks", "kLossBwdBlocks", "kLossThreads", "kLossTile")
EPE = _constants("epe.hip", "kEpeBlocks", "kEpeMultiBlocks", "kEpeThreads")


def _backward_cap():
    """The workgroup cap of backward.hip's grid_for: want < CAP ? want : CAP."""
    text = open(os.path.join(CSRC, "backward.hip")).read()
    m = re.search(r"static unsigned grid_for\(int64_t threads\)\s*\{(.*?)\n\}", text, re.S)
    assert m, "grid_for not found"
    body = m.group(1)
    assert re.search(r"\(threads \+ 255\) / 256", body), body
    caps = re.findall(r"\(1 << (\d+)\)", body)
    assert len(caps) == 2 and caps[0] == caps[1], body
    return 1 << int(caps[0])


def _trips(work, threads):
    return -(-work // threads)


def test_loss_tile_cases_walk_several_tiles():
    blocks = LOSS["kLossTileBlocks"]
    uneven = False
    for key in ("tile", "tile_plan", "tile_vs_pixel"):
        for B, H, W, lv in CASES[key]:
            tiles = B * (H // LOSS["kLossTile"]) * (W // LOSS["kLossTile"])
            assert _trips(tiles, min(tiles, blocks)) >= 2, (key, tiles, blocks)
            uneven |= tiles % blocks != 0
    assert uneven, "no tile case has an uneven last trip"
    # the finest level of the first tile case also loops loss_bwd_kernel's float4 path (n / 4 float4 per level)
    B, H, W, lv = CASES["tile"][0]
    vec = B * lv[0][0] * lv[0][1] * 2 // 4
    assert vec > LOSS["kLossBwdBlocks"] * LOSS["kLossThreads"], vec


def test_loss_pixel_cases_loop():
    threads = LOSS["kLossPixBlocks"] * LOSS["kLossThreads"]
    B, H, W, lv = CASES["tile_vs_pixel"][0]
    assert max(B * h * w for h, w in lv) > threads
    for B, H, W, lv in CASES["bilinear"]:
        assert all(B * h * w > threads for h, w in lv), (lv, threads)
        assert any(B * h * w % threads for h, w in lv)
        assert any(H % h or W % w for h, w in lv)                   # a ratio that is not an integer


def test_loss_backward_scalar_cases():
    threads = LOSS["kLossBwdBlocks"] * LOSS["kLossThreads"]
    for C in (2, 3):
        sizes = [B * h * w * C for B, H, W, lv in CASES["bwd_scalar"] for h, w in lv]
        assert all(n % 4 for n in sizes), (C, sizes)                 # never whole float4: the scalar loop
        assert min(sizes) <= threads and max(sizes) > threads, (C, sizes, threads)


def test_epe_cases_reach_the_unrolled_loops():
    nthr = EPE["kEpeMultiBlocks"] * EPE["kEpeThreads"]
    f32 = [B * h * w for B, h, w in CASES["epe_f32_x4"]]
    # fp32 aligned: float4 (2 pixels) per load; thread 0 enters `for (; i + 3 * nthr < n2; ...)` once at least
    assert all(n // 2 > 3 * nthr for n in f32), (f32, nthr)
    assert any(n % 2 for n in f32), "no odd-pixel tail"
    assert any((n // 2) % nthr for n in f32), "no uneven remainder trip"
    assert all(B * h * w > 3 * nthr for B, h, w in CASES["epe_f16_x4"])
    assert all(B * h * w > nthr for B, h, w in CASES["epe_plain"])
    assert all(B * h * w > EPE["kEpeBlocks"] * EPE["kEpeThreads"] for B, h, w in CASES["epe"])


def test_backward_cases_loop_past_the_grid_cap():
    threads = _backward_cap() * 256
    for B, H, W, C in CASES["backward"]:
        G = min(64, 1 << math.ceil(math.log2(C)))
        assert B * H * W * G > threads, (B, H, W, C, threads)        # cost_volume_bwd / warp_bwd: pixel groups
        assert B * H * W * C > threads                               # fill_zero / f32_to_f16: elements
        assert (B * H * W * G) % threads                             # uneven last trip


def test_loss_cases_take_the_kernel_they_test(hip_lib):
    from qpwcnet_amd import _hip
    I = ctypes.c_int
    aligned, shifted = 1 << 20, (1 << 20) + 4

    def pick(kind, ptr, B, H, W, C, lv):
        h, w = zip(*lv)
        return hip_lib.qpwc_loss_fwd_kernel(kind, ptr, B, H, W, C, (I * len(lv))(*h), (I * len(lv))(*w),
                                            len(lv)).decode()

    for key in ("tile", "tile_plan", "tile_vs_pixel"):
        for B, H, W, lv in CASES[key]:
            assert pick(_hip.LOSS_FLOW_MSE_V2, aligned, B, H, W, 2, lv) == "loss_area_tile_kernel", key
    for B, H, W, lv in CASES["tile_vs_pixel"]:
        assert pick(_hip.LOSS_FLOW_MSE_V2, shifted, B, H, W, 2, lv) == "loss_pixel_kernel"
    for kind, C in ((_hip.LOSS_FLOW_MSE, 2), (_hip.LOSS_FLOW_FINETUNE, 2), (_hip.LOSS_AUTORESIZE_MSE, 3)):
        for B, H, W, lv in CASES["bilinear"] + CASES["bwd_scalar"]:
            assert pick(kind, aligned, B, H, W, C, lv) == "loss_pixel_kernel"

"""The shapes of tests/test_gpu_forward_scale.py still reach the launch forms they are there for.

The thresholds and grid caps are read from the kernel sources, and the host rules that pick a form are restated here.
Raising a threshold would otherwise turn those tests back into small-form tests, and nothing would notice.  The
kernel choice of the cost-volume cases is asked of the library itself (qpwc_cost_volume_kernel: the launchers' own
selection rules, run on the host)."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_forward_scale import CASES  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qpwcnet_amd", "csrc")


def _once(name, pattern, flags=0):
    """The groups of the only match of pattern in csrc/name."""
    m = re.findall(pattern, open(os.path.join(CSRC, name)).read(), flags)
    assert len(m) == 1, (name, pattern, m)
    return m[0]


def _define(name, key):
    return int(_once(name, r"#define\s+{}\s+(\d+)\b".format(key)))


SC16_RESIDENT = _define("sepconv_f16.hip", "QPWC_SC16_RESIDENT")
SC16_RES_MAXF = _define("sepconv_f16.hip", "QPWC_SC16_RES_MAXF")
SC_RESIDENT = _define("optflow.hip", "QPWC_SC_RESIDENT")
SC_SLICE_TARGET = _define("optflow.hip", "QPWC_SC_SLICE_TARGET")
UPCONV16_NFB_MIN_WGS = _define("encoder.hip", "QPWC_UPCONV16_NFB_MIN_WGS")
SC_TH, SC_TW = map(int, _once("optflow_common.h", r"constexpr\s+int\s+kScTH\s*=\s*(\d+)\s*,\s*kScTW\s*=\s*(\d+)\s*;"))
EC_TW = int(_once("encoder.hip", r"constexpr\s+int\s+kEcTH\s*=\s*\d+\s*,\s*kEcTW\s*=\s*(\d+)\s*;"))
THREADS = 256     # every kernel below is launched with dim3(256): checked beside each cap


def _upconv16_th():
    """{C: TH} of upconv4x4s2_mish_f16_launch's cases."""
    text = open(os.path.join(CSRC, "encoder.hip")).read()
    m = re.findall(r"case\s+(\d+):\s*return\s+upconv_f16_launch_t<(\d+),\s*(\d+)>", text)
    assert len(m) == 3 and all(a == b for a, b, _ in m), m
    return {int(c): int(th) for c, _, th in m}


def _sc_tiles(B, H, W):
    return B * (-(-H // SC_TH)) * (-(-W // SC_TW))


def test_fp16_sepconv_cases_run_as_resident_workgroups():
    # n_res = (F <= 32 ? 3 : 2) * (QPWC_SC16_RESIDENT / 2); resident = F <= QPWC_SC16_RES_MAXF && n_work > n_res
    narrow, per_narrow, per_wide = map(int, _once(
        "sepconv_f16.hip", r"const int n_res = \(F <= (\d+) \? (\d+) : (\d+)\) \* \(QPWC_SC16_RESIDENT / 2\);"))
    _once("sepconv_f16.hip", r"const bool resident = QPWC_SC16_RESIDENT > 0 && F <= QPWC_SC16_RES_MAXF && n_work > n_res;")
    assert SC16_RESIDENT > 0
    two_tiles = one_tile = False
    for B, H, W, chans, F in CASES["sepconv_f16_resident"]:
        n_res = (per_narrow if F <= narrow else per_wide) * (SC16_RESIDENT // 2)
        tiles = _sc_tiles(B, H, W)
        assert F <= SC16_RES_MAXF and tiles > n_res, (chans, F, tiles, n_res)
        # the one-image launch of the bit-identity half is the one-shot form
        assert _sc_tiles(1, H, W) <= n_res
        assert H % SC_TH and W % SC_TW                               # partial tiles at the bottom and right edges
        two_tiles |= tiles > n_res
        one_tile |= tiles < 2 * n_res
    assert two_tiles and one_tile, "workgroups should own one or two tiles"
    # the forms: 16-byte loads (one dense source, C % 8 == 0) with 1, 2 and 4 steps; 8-byte loads over three sources
    steps = {-(-sum(c) // 32) for _, _, _, c, _ in CASES["sepconv_f16_resident"] if len(c) == 1 and sum(c) % 8 == 0}
    assert {1, 2, 4} <= steps, steps
    assert any(len(c) == 3 and c[-1] < 4 for _, _, _, c, _ in CASES["sepconv_f16_resident"])


def test_fp32_sepconv_cases_run_as_resident_workgroups_over_three_sources():
    maxf = int(_once("optflow.hip", r"const bool resident = F <= (\d+) && QPWC_SC_RESIDENT > 0 && slices == 1 && "
                                    r"n_work > QPWC_SC_RESIDENT;"))
    # (the fp16 twin's copy of this loop is not counted: it lives in sepconv_f16.hip)
    _once("optflow.hip", r"while \(nblk \* slices < QPWC_SC_SLICE_TARGET && F / \(slices \* 2\) >= 16\) slices \*= 2;")
    assert SC_RESIDENT > 0
    for B, H, W, chans, F in CASES["sepconv_f32_resident_concat"]:
        tiles = _sc_tiles(B, H, W)
        slices = 1
        while tiles * slices < SC_SLICE_TARGET and F // (slices * 2) >= 16:
            slices *= 2
        assert F <= maxf and slices == 1 and tiles > SC_RESIDENT, (chans, F, tiles, slices)
        assert len(chans) == 3 and chans[-1] < 4 and all(c % 4 == 0 for c in chans[:-1])
        assert H % SC_TH and W % SC_TW


def _nfb(C, F, B, H, W, th):
    tiles = B * (-(-H // th[C])) * (-(-W // EC_TW))
    nfb = 1
    while nfb * 2 <= F // 16 and (F // 16) % (nfb * 2) == 0 and tiles * (F // 16) // (nfb * 2) >= UPCONV16_NFB_MIN_WGS:
        nfb *= 2
    return nfb


def test_fp16_upconv_cases_walk_several_output_blocks():
    _once("encoder.hip", r"while \(nfb \* 2 <= F / 16 && \(F / 16\) % \(nfb \* 2\) == 0 && "
                         r"n_tiles \* \(F / 16\) / \(nfb \* 2\) >= QPWC_UPCONV16_NFB_MIN_WGS\) nfb \*= 2;")
    th = _upconv16_th()
    seen = set()
    for C, F, B, H, W, nfb in CASES["upconv_f16_nfb"]:
        assert _nfb(C, F, B, H, W, th) == nfb and nfb > 1, (C, F, B, H, W, _nfb(C, F, B, H, W, th), nfb)
        assert _nfb(C, F, 1, H, W, th) == 1, (C, F, H, W)            # the one-image launch of the bit-identity half
        seen.add(nfb)
    assert {2, 4, 8} <= seen
    assert any(H % th[C] and W % EC_TW and (B * (-(-H // th[C])) * (-(-W // EC_TW))) % 2
               for C, F, B, H, W, _ in CASES["upconv_f16_nfb"]), "no ragged case with an odd tile count"


def _uneven_second_trip(work, cap):
    threads = cap * THREADS
    return -(-work // THREADS) > cap and work > threads and work % threads != 0


def test_generic_cost_volume_cases_loop(hip_lib):
    from qpwcnet_amd import _hip
    cap = int(_once("cost_volume.hip", r"const unsigned grid = \(unsigned\)\(want < (\d+) \? want : \1\);").strip())
    assert cap == 65536
    _once("cost_volume.hip", r"const int64_t want = \(total \+ 255\) / 256;")
    layouts = set()
    for B, H, W, C, fmt in CASES["cost_volume_generic"]:
        assert _uneven_second_trip(B * H * W * 81, cap), (B, H, W)
        layout = _hip.NHWC if fmt == "channels_last" else _hip.NCHW
        layouts.add(layout)
        for dt in (_hip.F32, _hip.F16):
            assert hip_lib.qpwc_cost_volume_kernel(B, H, W, C, 4, layout, dt, 0, 0).decode() == \
                "cost_volume_generic_kernel", (fmt, dt)
    assert layouts == {_hip.NHWC, _hip.NCHW}


def test_pad_zeroing_cases_loop(hip_lib):
    from qpwcnet_amd import _hip
    caps = _once("cost_volume.hip", r"\(npx \* 3 \+ 255\) / 256 < (\d+) \? \(npx \* 3 \+ 255\) / 256 : (\d+)\);")
    assert caps[0] == caps[1]
    cap = int(caps[0])
    assert cap == 4096
    # the matrix-core launch leaves the pads to zero_pads_kernel unless every 4 x 4 tile is dense
    assert len(re.findall(r"\*pads_written = pad84 && W % 4 == 0 && H % 4 == 0 &&",
                          open(os.path.join(CSRC, "cost_volume_mfma.hip")).read())) == 2     # fp32 and fp16
    families = set()
    for B, H, W, C, family in CASES["zero_pads"]:
        assert _uneven_second_trip(B * H * W * 3, cap), (B, H, W)
        assert not (W % 4 == 0 and H % 4 == 0)                        # pads_written is false
        for dt in (_hip.F32, _hip.F16):
            name = hip_lib.qpwc_cost_volume_kernel(B, H, W, C, 4, _hip.NHWC, dt, 84, 0).decode()
            assert name.startswith(family), (C, dt, name)
        families.add(family)
    assert families == {"cost_volume_tiled_kernel", "cost_volume_mfma"}


def test_copy_pixels_case_takes_the_unrolled_loop_twice():
    caps = _once("layout.hip", r"want < 1 \? 1 : \(want > (\d+) \? (\d+) : want\)")
    assert caps[0] == caps[1]
    cap = int(caps[0])
    assert cap == 16384
    unroll = int(_once("layout.hip", r"const int64_t want = \(total \+ (\d+) \* 256 - 1\) / \(\1 \* 256\);"))
    _once("layout.hip", r"for \(; i \+ 3 \* nthr < total; i \+= 4 \* nthr\)")
    assert unroll == 4
    for B, H, W, C in CASES["copy_pixels"]:
        total = B * H * W * (C * 4 // 16)
        assert -(-total // (unroll * THREADS)) > cap                  # the grid is capped
        nthr = cap * THREADS
        trips, i = 0, 0                                               # thread 0
        while i + 3 * nthr < total:
            trips, i = trips + 1, i + 4 * nthr
        assert trips >= 2, (total, nthr, trips)
        last = nthr - 1                                               # the last thread: fewer trips, then the tail loop
        while last + 3 * nthr < total:
            trips, last = trips - 1, last + 4 * nthr
        assert trips > 0 and last < total and total % nthr, (total, nthr, trips)

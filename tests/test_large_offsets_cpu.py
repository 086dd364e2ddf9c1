"""CPU companion of tests/test_gpu_large_offsets.py: every shape of its CASES crosses the boundaries it claims (2^29,
2^30 and 2^31 fp32 elements: byte offsets 2^31 and 2^32, the `int` index limit), with each boundary in the image the
GPU test relies on, and is still admitted by the validators; the workspace regions cross what DESIGN.md 4.17 says
they cross; the planned device memory stays under 48 GiB; the float64 restatement on crops and windows agrees with
the fp32 torch composition within the bounds the GPU test uses; the negative controls move the window sums by at
least 100 bounds; and the ctypes table carries every size that can pass 2^31 as a 64-bit integer.  For the masked
losses and the flow metrics, whose masks are indexed by byte, also: the windows lie behind the masks' byte boundaries
and the ground truth's 2^32nd element, a mask read at a wrapped byte offset meets no window, and the windows' flows
keep the metrics' thresholds at a distance.  For the label-free losses and the input pipelines, whose oracles are crops
of a trivial background: the shapes cross what they claim, the crops are disjoint, and the crop oracles equal the whole
float64 restatement on a level and a source small enough to have one.  For the occlusion map, the interpolator's input
pipeline and the update step: the shapes cross what they claim (and, for the occlusion kernels, make the grid-stride
loops iterate at least four times with a partial last trip, from the cap and the workgroup size read out of the
source), the windowed restatements equal oracle.np_ref / ref_triplet where those can run, with the margins the GPU test
uses, both unit tables address the same elements, and the fp32 torch composition keeps the update step's bounds on
rows drawn as the GPU test draws them.

The plans are restated from the constants read out of the kernel sources (tests/test_conv_grad_cpu.py::_plan) and
compared with the library's own host functions, so a changed plan constant that pulls a region back under a boundary
fails here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_large_offsets as lo  # noqa: E402
from test_capi_prototypes_cpu import parse_header  # noqa: E402
from test_conv_grad_cpu import CB, CSRC, _plan  # noqa: E402
from test_gpu_autograd import _flow, _oracle_warp  # noqa: E402
from test_gpu_conv_grad import _grid, composite  # noqa: E402
from test_gpu_flow_head_grad import upsample_composite  # noqa: E402
from test_gpu_interp_grad import head_composite, pyramid_composite  # noqa: E402
from test_training_scale_cpu import _backward_cap  # noqa: E402
from test_gpu_upconv_grad import composite as up_composite  # noqa: E402
from test_gpu_sepconv_grad import composite as sep_composite  # noqa: E402
from test_sepconv_grad_cpu import KC, SCB, _workspace as _sep_workspace  # noqa: E402
from test_upconv_grad_cpu import UB, _plan as _up_plan  # noqa: E402

P29, P30, P31 = lo.BOUNDARIES
CONV = ("conv3x3_same_s1", "conv3x3_same_s2")
UP = "upconv4x4s2"
SEP = "sepconv3x3"


def test_boundaries_are_the_byte_and_index_limits():
    assert (P29 * 4, P30 * 4, P31) == (1 << 31, 1 << 32, 1 << 31)
    assert lo.crossed(P31 + 2) == [P29, P30, P31] and lo.crossed(P31 + 1) == [P29, P30] and lo.crossed(P29) == []


# ---- Conv2D 3x3 'same' -----------------------------------------------------------------------------------------------
def conv_plan(key):
    """cb_plan() + cg_split() restated: the workspace regions gz | part_w | part_b as (first, end) in floats."""
    B, H, W, ci, co, s = key
    n_pb, nsplit, total = _plan(*key)
    M, cp = B * -(-H // s) * -(-W // s), -(-ci // 4) * 4
    off_pw = M * co
    off_pb = off_pw + nsplit * 9 * co * cp
    assert total == off_pb + -(-nsplit * co // 4) * 4
    return {"gz": (0, off_pw), "part_w": (off_pw, off_pb), "part_b": (off_pb, total)}, n_pb, nsplit


def test_conv_cases_cross_what_they_claim():
    claims = {"conv3x3_same_s1": {"x": [P29, P30, P31], "out": [P29, P30, P31]},
              "conv3x3_same_s2": {"x": [P29, P30, P31], "out": [P29, P30]}}
    images = {"conv3x3_same_s1": {"x": [0, 1, 2], "out": [0, 1, 2]}, "conv3x3_same_s2": {"x": [0, 1, 2], "out": [1, 2]}}
    for name in CONV:
        key = lo.CASES[name]
        B, H, W, ci, co, s = key
        g = lo.conv_geo(key)
        n = lo.conv_operands(key)
        assert B == 3 and H % 2 and W % 2 and H != W                                    # ragged
        assert n["x"] == n["grad_x"] == B * H * W * ci > P31
        assert n["out"] == n["grad_out"] == n["gz"] == B * g["Ho"] * g["Wo"] * co
        assert lo.crossed(n["x"]) == claims[name]["x"] and lo.crossed(n["out"]) == claims[name]["out"]
        # each boundary in another image, none in a first or last row or column: both terms of the offset count
        at = [lo.locate(b, H, W, ci) for b in lo.crossed(n["x"])]
        assert [a[0] for a in at] == images[name]["x"]
        at_o = [lo.locate(b, g["Ho"], g["Wo"], co) for b in lo.crossed(n["out"])]
        assert [a[0] for a in at_o] == images[name]["out"]
        for rows, cols, where in ((H, W, at), (g["Ho"], g["Wo"], at_o)):
            assert all(0 < y < rows - 2 - lo.WIN and 0 < x < cols - 1 for _, y, x in where), where
        # the last pixel block is partial, so the crop on the last pixels holds it
        assert (B * g["Ho"] * g["Wo"]) % CB["kCbPx"]


def test_conv_workspace_regions(hip_lib):
    """Stage Z's gz in the workspace crosses what grad_out crosses; the partials lie behind all of it, so their
    offsets (off_pw, off_pb of cg_split) are beyond 2^31 elements at stride 1 and beyond 2^30 at stride 2."""
    want = {"conv3x3_same_s1": [P29, P30, P31], "conv3x3_same_s2": [P29, P30]}
    for name in CONV:
        key = lo.CASES[name]
        regions, n_pb, nsplit = conv_plan(key)
        assert hip_lib.qpwc_conv3x3_same_bwd_workspace_floats(*key) == regions["part_b"][1]
        assert lo.crossed(regions["gz"][1]) == want[name]
        assert regions["part_w"][0] > want[name][-1] and regions["part_b"][0] > regions["part_w"][0]
        assert n_pb > (1 << 19) and nsplit == CB["kCbWBlocks"] // 9          # stage W walks > 2^12 blocks a workgroup
        # one image alone stays below every boundary but the first: what oracle (a) compares with
        one = (1,) + key[1:]
        assert lo.crossed(lo.conv_operands(one)["x"]) == [P29]
        assert hip_lib.qpwc_conv3x3_same_bwd_workspace_floats(*one) < P30


def test_conv_cases_are_admitted(hip_lib):
    from qpwcnet_amd import _hip
    text = open(os.path.join(CSRC, "conv_bwd.hip")).read()
    m = re.search(r"bool conv3x3_same_shape_ok\(.*?\{(.*?)\n\}", text, re.S)
    body = m.group(1)
    # the rule, each expression exactly once: pixel blocks of the input within INT32_MAX, B within 2^24
    assert body.count("(p.M_in + kCbPx - 1) / kCbPx <= INT32_MAX") == 1 and body.count("B <= (1 << 24)") == 1
    assert body.count("return") == 1
    assert text.count("p.M_in = (int64_t)B * H * W;") == 1 and text.count("p.M_out = (int64_t)B * g.Ho * g.Wo;") == 1
    for name in CONV:
        B, H, W, ci, co, s = lo.CASES[name]
        assert -(-B * H * W // CB["kCbPx"]) <= 2 ** 31 - 1 and B <= 1 << 24
        assert max(B, H, W, ci, co) < 2 ** 31                      # every size argument of the entry points fits an int
        assert hip_lib.qpwc_conv3x3_same_bwd_workspace_floats(B, H, W, ci, co, s) > 0
    # the cap is far off (2^37 pixels): no case sits at it, the refusal is by name all the same
    assert hip_lib.qpwc_conv3x3_same_bwd_workspace_floats(1 << 16, 1 << 15, 1 << 7, 16, 16, 1) == _hip.E_SHAPE
    assert b"too large for the launch grids" in hip_lib.qpwc_last_error()
    assert hip_lib.qpwc_conv3x3_same_bwd_workspace_floats((1 << 16) - 1, 1 << 15, 1 << 6, 16, 16, 1) > P31


def test_conv_planned_memory(hip_lib):
    ws = hip_lib.qpwc_conv3x3_same_bwd_workspace_floats
    for name in CONV:
        key = lo.CASES[name]
        planned = lo.conv_planned_bytes(key, ws(*key), ws(1, *key[1:]))
        n = lo.conv_operands(key)
        assert planned >= 4 * (n["x"] + n["grad_x"] + n["out"] + n["grad_out"] + n["gz"])
        assert planned <= 48 * lo.GIB, planned / lo.GIB
        assert 1.10 * planned <= 64 * lo.GIB


def test_conv_crops_and_windows_lie_where_the_offsets_wrap():
    for name in CONV + (UP, SEP):
        key = lo.CASES[name]
        g = lo.conv_geo(key)
        g.setdefault("s", 1)                    # transposed: the windows' x rows lie within 3 input rows of the boundary
        n_el = lo.conv_operands(key)
        crops, wins = lo.conv_crops(key), lo.conv_windows(key)
        tags = [c[0] for c in crops]
        assert tags[-1] == "last" and len(set(tags)) == len(tags)
        assert {t for t in tags if t.startswith("x>")} | {t for t in tags if t.startswith("out>")} == set(tags[:-1])
        for b in lo.crossed(n_el["out"]):              # the pixel before and the pixel at the boundary are compared
            n, y, x = lo.locate(b, g["Ho"], g["Wo"], g["co"])
            assert any(c[1] == n and c[2] <= y < c[3] and c[4] <= x - 1 and x < c[5] for c in crops), (name, b)
        for b in lo.crossed(n_el["x"]):
            n, y, x = lo.locate(b, g["H"], g["W"], g["ci"])
            hit = False
            for c in crops:
                (cy0, cy1, cx0, cx1), _ = lo.conv_x_region(key, c)
                if c[1] == n and cy0 <= y < cy1 and cx0 <= x - 1 and x < cx1:
                    ok = lo.conv_gx_valid(key, c)
                    hit |= bool(ok[y - cy0, x - cx0]) and bool(ok[y - cy0, x - 1 - cx0])
            assert hit, (name, b)
        last = crops[-1]
        (cy0, cy1, cx0, cx1), pads = lo.conv_x_region(key, last)
        assert (cy1, cx1) == (g["H"], g["W"]) and (g["up"] or pads[1] + pads[3] >= 1)    # the 'SAME' border is in it
        assert bool(lo.conv_gx_valid(key, last)[-1, -1])                            # and the very last x pixel
        # windows: disjoint, the first at offset 0, one wholly behind every boundary, the last in the corner
        assert wins[0][1:] == (0, 0, lo.WIN, 0, lo.WIN) and wins[-1][1] == g["B"] - 1 and wins[-1][3] == g["Ho"]
        for i, a in enumerate(wins):
            for b_ in wins[i + 1:]:
                assert a[1] != b_[1] or a[3] <= b_[2] or b_[3] <= a[2] or a[5] <= b_[4] or b_[5] <= a[4], (a, b_)
        for b in lo.crossed(n_el["out"]):
            assert any(((w[1] * g["Ho"] + w[2]) * g["Wo"] + w[4]) * g["co"] > b and
                       ((w[1] * g["Ho"] + w[2] - 1) * g["Wo"] + w[4]) * g["co"] < b + 5 * g["Wo"] * g["co"]
                       for w in wins[1:-1]), (name, b)
        for b in lo.crossed(n_el["x"]):
            firsts = []
            for w in wins[1:-1]:
                (cy0, _, cx0, _), _ = lo.conv_x_region(key, w)
                firsts.append(((w[1] * g["H"] + cy0) * g["W"] + cx0) * g["ci"])
            assert any(b < f < b + (2 * g["s"] + 2) * g["W"] * g["ci"] for f in firsts), (name, b)
        # a 32-bit byte offset finds every window behind a boundary somewhere else, inside the tensor
        moved = [lo.conv_wrapped_regions(key, w) for w in wins]
        assert moved[0] == [] and all(len(m) >= 1 for m in moved[1:])
        assert {mod for m in moved for mod, _ in m} == {1 << 31, 1 << 32}
        for m, w in zip(moved, wins):
            (cy0, cy1, cx0, cx1), _ = lo.conv_x_region(key, w)
            for _, (n, y0, y1, x0, x1) in m:
                assert 0 <= n < g["B"] and 0 <= y0 < y1 <= g["H"] and 0 <= x0 < x1 <= g["W"]
                assert (y1 - y0, x1 - x0) == (cy1 - cy0, cx1 - cx0) and (n, y0, x0) != (w[1], cy0, cx0)


def _axis_users_brute(i, n_out, s, p):
    return [o for o in range(n_out) if 0 <= i - (o * s - p) <= 2]


def test_gx_valid_mask_against_brute_force():
    for key in ((1, 9, 11, 16, 16, 1), (1, 9, 11, 16, 32, 2), (1, 8, 12, 16, 32, 2)):
        g = lo.conv_geo(key)
        for o0, o1 in ((0, 3), (1, 4), (g["Ho"] - 3, g["Ho"])):
            reg = ("t", 0, o0, o1, 0, g["Wo"])
            (cy0, cy1, _, _), _ = lo.conv_x_region(key, reg)
            want = [all(o0 <= o < o1 for o in _axis_users_brute(i, g["Ho"], g["s"], g["pt"])) for i in range(cy0, cy1)]
            assert lo.conv_gx_valid(key, reg)[:, 0].tolist() == want, (key, o0)


@pytest.mark.parametrize("stride,hw", [(1, (40, 45)), (2, (81, 87)), (2, (80, 86))], ids=["s1", "s2odd", "s2even"])
@pytest.mark.parametrize("mish", [True, False], ids=["mish", "linear"])
def test_crop_restatement_is_the_layer(stride, hw, mish):
    """conv_region_ref on a crop against the float64 composite of the whole (small) tensor, wherever the crop lies:
    the outputs everywhere in the crop, grad_x where conv_gx_valid says so; and the window sums against the composite
    fed a grad_out that is zero outside the windows."""
    key = (2,) + hw + (16, 32 if stride == 2 else 16, stride)
    gen = torch.Generator().manual_seed(5)
    g_ = lo.conv_geo(key)
    x, w, b = _grid(gen, (2,) + hw + (16,), 1 / 16), _grid(gen, (key[4], 16, 3, 3), 1 / 8), _grid(gen, (key[4],), 1 / 8)
    go = _grid(gen, (2, g_["Ho"], g_["Wo"], key[4]), 1 / 16)
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    out = composite(*leaves, stride, mish)
    out.backward(go)
    C = lo.CROP
    regs = [("tl", 0, 0, C, 0, C), ("mid", 1, 5, 5 + C, 7, 7 + C), ("br", 1, g_["Ho"] - C, g_["Ho"], g_["Wo"] - C, g_["Wo"])]
    for reg in regs:
        (cy0, cy1, cx0, cx1), pads = lo.conv_x_region(key, reg)
        n = reg[1]
        ro, rx, _, _ = lo.conv_region_ref(key, x[n:n + 1, cy0:cy1, cx0:cx1], pads, w, b,
                                          go[n:n + 1, reg[2]:reg[3], reg[4]:reg[5]], mish)
        assert float((ro - out.detach()[n:n + 1, reg[2]:reg[3], reg[4]:reg[5]]).abs().max()) < 1e-12
        ok = lo.conv_gx_valid(key, reg)
        assert int(ok.sum()) >= (C - 2) ** 2
        assert float((rx[0][ok] - leaves[0].grad[n, cy0:cy1, cx0:cx1][ok]).abs().max()) < 1e-12
        assert float((rx[0][~ok] - leaves[0].grad[n, cy0:cy1, cx0:cx1][~ok]).abs().max()) > 1e-3      # the mask is needed
    wins = [("a", 0, 0, 16, 0, 16), ("b", 1, 3, 19, 9, 25), ("c", 1, g_["Ho"] - 16, g_["Ho"], g_["Wo"] - 16, g_["Wo"])]
    sparse = torch.zeros_like(go)
    crops = []
    for reg in wins:
        sparse[reg[1], reg[2]:reg[3], reg[4]:reg[5]] = go[reg[1], reg[2]:reg[3], reg[4]:reg[5]]
        (cy0, cy1, cx0, cx1), pads = lo.conv_x_region(key, reg)
        crops.append((x[reg[1]:reg[1] + 1, cy0:cy1, cx0:cx1], pads, go[reg[1]:reg[1] + 1, reg[2]:reg[3], reg[4]:reg[5]]))
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    composite(*leaves, stride, mish).backward(sparse)
    rw, rb = lo.conv_window_sums(key, crops, w, b, mish)
    assert float((rw - leaves[1].grad).abs().max()) < 1e-11 and float((rb - leaves[2].grad).abs().max()) < 1e-11


def _cpu_windows(key, seed):
    """The windows of a case with crops drawn on the CPU from the grids the GPU test draws from on the device."""
    gen = torch.Generator().manual_seed(seed)
    ci, co = key[3], key[4]
    w, b = _grid(gen, (co, ci, 3, 3), 1 / 8), _grid(gen, (co,), 1 / 8)
    crops, moved = [], []
    for k, reg in enumerate(lo.conv_windows(key)):
        (cy0, cy1, cx0, cx1), pads = lo.conv_x_region(key, reg)
        crops.append((_grid(gen, (1, cy1 - cy0, cx1 - cx0, ci), 1 / 16), pads,
                      _grid(gen, (1, reg[3] - reg[2], reg[5] - reg[4], co), 1 / 16)))
        for mod, _ in lo.conv_wrapped_regions(key, reg):        # dense random data read elsewhere: another draw
            moved.append(("window %d mod %d" % (k, mod), k, _grid(gen, (1, cy1 - cy0, cx1 - cx0, ci), 1 / 16)))
    return crops, moved, w, b


@pytest.mark.parametrize("name", CONV)
@pytest.mark.parametrize("mish", [True, False], ids=["mish", "linear"])
def test_conv_window_sums_bounds_and_negative_controls(name, mish):
    """On the CPU: the fp32 composition of the window sums stays within the bound the GPU test uses (1e-4 max(1,
    max|ref|)) of the float64 restatement -- exactly on it without Mish, under the asserted magnitude precondition --
    and every negative control moves grad_w by at least 100 bounds."""
    key = lo.CASES[name]
    crops, moved, w, b = _cpu_windows(key, 11)
    rw, rb = lo.conv_window_sums(key, crops, w, b, mish)
    gw32, gb32 = 0.0, 0.0
    for xc, pads, gc in crops:
        lv = [t.float().clone().requires_grad_() for t in (xc, w, b)]
        z = torch.nn.functional.conv2d(torch.nn.functional.pad(lv[0].permute(0, 3, 1, 2), pads), lv[1], lv[2],
                                       stride=key[5]).permute(0, 2, 3, 1)
        (lo.torch_ref.mish(z) if mish else z).backward(gc.float())
        gw32, gb32 = gw32 + lv[1].grad, gb32 + lv[2].grad
    if mish:
        assert float((gw32.double() - rw).abs().max()) <= 0.1 * lo._tol(rw)
        assert float((gb32.double() - rb).abs().max()) <= 0.1 * lo._tol(rb)
    else:
        assert lo.exactness_precondition(key, crops, w, b) * 2 ** 8 < 2 ** 24
        assert torch.equal(gw32.double(), rw) and torch.equal(gb32.double(), rb)
    controls = lo.conv_controls(key, crops, moved, w, b, mish)
    assert len(controls) == len(crops) + len(moved) and len(moved) >= 2
    assert min(r for _, r in controls) >= 100.0, controls


def test_size_arguments_of_the_entry_points_used():
    """The entry points the GPU test reaches are in the table that tests/test_capi_prototypes_cpu.py compares with
    the header; what can pass 2^31 there -- the workspace size -- is 64-bit on both sides, and every `int` parameter
    carries an extent that the cases keep far below 2^31."""
    from qpwcnet_amd import _hip
    protos = {name: (ret, params) for name, ret, params in parse_header()}
    for name in ("qpwc_conv3x3_same_fwd", "qpwc_conv3x3_same_bwd", "qpwc_conv3x3_mish_fwd"):
        assert name in protos and name in _hip.PROTOTYPES
        assert protos[name][0] == "int" and set(protos[name][1]) <= {"const void*", "void*", "int"}
    ret, params = protos["qpwc_conv3x3_same_bwd_workspace_floats"]
    assert ret == "int64_t" and params == ["int"] * 6
    restype, argtypes = _hip.PROTOTYPES["qpwc_conv3x3_same_bwd_workspace_floats"]
    assert ctypes.sizeof(restype) == 8 and all(t is ctypes.c_int for t in argtypes)


# ---- transposed conv 4x4 stride 2 ------------------------------------------------------------------------------------
def test_upconv_case_crosses_what_it_claims(hip_lib):
    from qpwcnet_amd import _hip
    key = lo.CASES[UP]
    B, H, W, C, F_ = key
    n = lo.conv_operands(key)
    assert B == 3 and H % 2 and W % 2 and H != W
    assert n["x"] == B * H * W * C and n["out"] == n["gz"] == B * 2 * H * 2 * W * F_ == n["x"]
    assert lo.crossed(n["x"]) == lo.crossed(n["out"]) == [P29, P30, P31]
    assert [lo.locate(b, H, W, C)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    assert [lo.locate(b, 2 * H, 2 * W, F_)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    for rows, cols, ch in ((H, W, C), (2 * H, 2 * W, F_)):
        assert all(0 < y < rows - 4 - lo.WIN and 0 < x < cols - 1 for _, y, x in (lo.locate(b, rows, cols, ch) for b in lo.BOUNDARIES))
    assert (B * H * W) % UB["kUbPx"]                                              # a partial last pixel block
    # ub_plan() restated: gz | part_w | part_b; gz crosses all three, the partials lie behind 2^31 elements
    n_pb, nsplit, total = _up_plan(*key)
    off_pw = 4 * B * H * W * F_
    off_pb = off_pw + nsplit * 16 * F_ * C
    assert total == off_pb + -(-nsplit * F_ // 4) * 4 == hip_lib.qpwc_upconv4x4s2_bwd_workspace_floats(*key)
    assert lo.crossed(off_pw) == [P29, P30, P31] and off_pb > off_pw > P31 and nsplit == UB["kUbWBlocks"] // 16
    one = (1,) + key[1:]
    assert lo.crossed(lo.conv_operands(one)["x"]) == [P29] and hip_lib.qpwc_upconv4x4s2_bwd_workspace_floats(*one) < P30
    # admitted: upconv4x4s2_bwd_shape_ok, each expression once
    text = open(os.path.join(CSRC, "upconv_bwd.hip")).read()
    body = re.search(r"bool upconv4x4s2_bwd_shape_ok\(.*?\{(.*?)\n\}", text, re.S).group(1)
    for expr in ("p.n_pb <= INT32_MAX", "B <= (1 << 24)", "H <= (1 << 29)", "W <= (1 << 29)"):
        assert body.count(expr) == 1, expr
    assert body.count("return") == 1 and text.count("p.M_in = (int64_t)B * H * W;") == 1
    assert n_pb <= 2 ** 31 - 1 and B <= 1 << 24 and max(H, W) <= 1 << 29
    ws = hip_lib.qpwc_upconv4x4s2_bwd_workspace_floats
    assert ws(1, (1 << 29) + 1, 1, 64, 16) == _hip.E_SHAPE and b"too large for the launch grids" in hip_lib.qpwc_last_error()
    assert ws(1 << 16, 1 << 15, 1 << 7, 64, 16) == _hip.E_SHAPE
    planned = lo.conv_planned_bytes(key, ws(*key), ws(*one))
    assert 4 * 5 * n["x"] <= planned <= 48 * lo.GIB and 1.10 * planned <= 64 * lo.GIB


@pytest.mark.parametrize("mish", [True, False], ids=["mish", "linear"])
def test_upconv_crop_restatement_is_the_layer(mish):
    key = (2, 20, 23, 64, 16)
    gen = torch.Generator().manual_seed(6)
    x, w, b = _grid(gen, (2, 20, 23, 64), 1 / 16), _grid(gen, (64, 16, 4, 4), 1 / 64, 1 / 8), _grid(gen, (16,), 1 / 8)
    go = _grid(gen, (2, 40, 46, 16), 1 / 16)
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    out = up_composite(*leaves, mish)
    out.backward(go)
    C = lo.CROP
    for reg in (("tl", 0, 0, C, 0, C), ("mid", 1, 5, 5 + C, 7, 7 + C), ("mid2", 1, 6, 6 + C, 8, 8 + C), ("br", 1, 40 - C, 40, 46 - C, 46)):
        (cy0, cy1, cx0, cx1), place = lo.conv_x_region(key, reg)
        n = reg[1]
        ro, rx, _, _ = lo.conv_region_ref(key, x[n:n + 1, cy0:cy1, cx0:cx1], place, w, b,
                                          go[n:n + 1, reg[2]:reg[3], reg[4]:reg[5]], mish)
        assert float((ro - out.detach()[n:n + 1, reg[2]:reg[3], reg[4]:reg[5]]).abs().max()) < 1e-12
        ok = lo.conv_gx_valid(key, reg)
        assert int(ok.sum()) >= (C // 2 - 2) ** 2
        assert float((rx[0][ok] - leaves[0].grad[n, cy0:cy1, cx0:cx1][ok]).abs().max()) < 1e-12
        assert float((rx[0][~ok] - leaves[0].grad[n, cy0:cy1, cx0:cx1][~ok]).abs().max()) > 1e-3
    wins = [("a", 0, 0, 16, 0, 16), ("b", 1, 3, 19, 9, 25), ("c", 1, 24, 40, 30, 46)]
    sparse = torch.zeros_like(go)
    crops = []
    for reg in wins:
        sparse[reg[1], reg[2]:reg[3], reg[4]:reg[5]] = go[reg[1], reg[2]:reg[3], reg[4]:reg[5]]
        (cy0, cy1, cx0, cx1), place = lo.conv_x_region(key, reg)
        crops.append((x[reg[1]:reg[1] + 1, cy0:cy1, cx0:cx1], place, go[reg[1]:reg[1] + 1, reg[2]:reg[3], reg[4]:reg[5]]))
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    up_composite(*leaves, mish).backward(sparse)
    rw, rb = lo.conv_window_sums(key, crops, w, b, mish)
    assert float((rw - leaves[1].grad).abs().max()) < 1e-11 and float((rb - leaves[2].grad).abs().max()) < 1e-11


@pytest.mark.parametrize("mish", [True, False], ids=["mish", "linear"])
def test_upconv_window_sums_bounds_and_negative_controls(mish):
    key = lo.CASES[UP]
    gen = torch.Generator().manual_seed(12)
    C, F_ = key[3], key[4]
    w, b = _grid(gen, (C, F_, 4, 4), 1 / 64, 1 / 8), _grid(gen, (F_,), 1 / 8)
    crops, moved = [], []
    for k, reg in enumerate(lo.conv_windows(key)):
        (cy0, cy1, cx0, cx1), place = lo.conv_x_region(key, reg)
        crops.append((_grid(gen, (1, cy1 - cy0, cx1 - cx0, C), 1 / 16), place,
                      _grid(gen, (1, reg[3] - reg[2], reg[5] - reg[4], F_), 1 / 16)))
        for mod, _ in lo.conv_wrapped_regions(key, reg):
            moved.append(("window %d mod %d" % (k, mod), k, _grid(gen, (1, cy1 - cy0, cx1 - cx0, C), 1 / 16)))
    rw, rb = lo.conv_window_sums(key, crops, w, b, mish)
    gw32, gb32 = 0.0, 0.0
    for xc, place, gc in crops:
        lv = [t.float().clone().requires_grad_() for t in (xc, w, b)]
        z = torch.nn.functional.conv_transpose2d(lv[0].permute(0, 3, 1, 2), lv[1], lv[2], stride=2, padding=1)
        z = z.permute(0, 2, 3, 1)[:, place[2]:place[3], place[0]:place[1]]
        (lo.torch_ref.mish(z) if mish else z).backward(gc.float())
        gw32, gb32 = gw32 + lv[1].grad, gb32 + lv[2].grad
    if mish:
        assert float((gw32.double() - rw).abs().max()) <= 0.1 * lo._tol(rw)
        assert float((gb32.double() - rb).abs().max()) <= 0.1 * lo._tol(rb)
    else:
        assert lo.exactness_precondition(key, crops, w, b, unit=2 ** 10) * 2 ** 10 < 2 ** 24
        assert torch.equal(gw32.double(), rw) and torch.equal(gb32.double(), rb)
    controls = lo.conv_controls(key, crops, moved, w, b, mish)
    assert len(controls) == len(crops) + len(moved) and len(moved) >= 2
    assert min(r for _, r in controls) >= 100.0, controls


def test_size_arguments_of_the_upconv_entry_points():
    from qpwcnet_amd import _hip
    protos = {name: (ret, params) for name, ret, params in parse_header()}
    ret, params = protos["qpwc_upconv4x4s2_bwd"]
    # grad_out's pixel stride is the one size there that is 64-bit; every extent is an int the case keeps small
    assert ret == "int" and params.count("int64_t") == 1 and set(params) <= {"const void*", "void*", "int", "int64_t"}
    assert [ctypes.sizeof(t) for t in _hip.PROTOTYPES["qpwc_upconv4x4s2_bwd"][1]].count(8) >= 1
    ret, params = protos["qpwc_upconv4x4s2_bwd_workspace_floats"]
    assert ret == "int64_t" and params == ["int"] * 5
    assert ctypes.sizeof(_hip.PROTOTYPES["qpwc_upconv4x4s2_bwd_workspace_floats"][0]) == 8
    assert "qpwc_upconv4x4s2_mish_fwd" in protos and "qpwc_upconv4x4s2_mish_fwd" in _hip.PROTOTYPES


# ---- SeparableConv2D backward ---------------------------------------------------------------------------------------
def sep_plan(key):
    """scb_plan() restated: the workspace regions d | gd | gz | part_pw | part_b | part_dw as (first, end) in floats."""
    B, H, W, C, F_ = key[:5]
    M, cpad = B * H * W, -(-C // KC) * KC
    chunks = cpad // KC
    up4 = lambda n: -(-n // 4) * 4
    pw_x = min(-(-M // SCB["kScbPx"]), max(1, SCB["kScbPwBlocks"] // chunks))
    groups = -(-(B * H * -(-W // SCB["kScbStrip"])) // SCB["kScbDwSlots"])
    dw_x = min(groups, max(1, SCB["kScbDwBlocks"] // chunks))
    sizes = (("d", M * cpad), ("gd", M * cpad), ("gz", up4(M * F_)), ("part_pw", pw_x * F_ * cpad),
             ("part_b", up4(pw_x * F_)), ("part_dw", up4(dw_x * C * 9)))
    regions, at = {}, 0
    for name, n in sizes:
        regions[name] = (at, at + n)
        at += n
    assert at == _sep_workspace(B, H, W, C, F_)
    return regions


def test_sepconv_case_crosses_what_it_claims(hip_lib):
    from qpwcnet_amd import _hip
    key = lo.CASES[SEP]
    B, H, W, C, F_, one_ = key
    assert one_ == 1 and B == 3 and H % 2 and W % 2 and H != W and C == KC           # Cpad = C: d and gd are x-sized
    n = lo.sepconv_operands(key)
    assert n["x"] == lo.conv_operands(key)["x"] == B * H * W * C and n["grad_out"] == lo.conv_operands(key)["out"]
    assert lo.crossed(n["x"]) == [P29, P30, P31] and lo.crossed(n["grad_out"]) == [P29, P30]
    assert [lo.locate(b, H, W, C)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    assert [lo.locate(b, H, W, F_)[0] for b in (P29, P30)] == [1, 2]
    assert all(0 < y < H - 2 - lo.WIN and 0 < x < W - 1 for _, y, x in (lo.locate(b, H, W, C) for b in lo.BOUNDARIES))
    assert (B * H * W) % SCB["kScbPx"] and W % SCB["kScbStrip"]                        # partial last block, partial strips
    # the workspace: gd starts behind 2^31 elements, gz and the partials behind 2^32; d itself crosses all three
    r = sep_plan(key)
    ws = hip_lib.qpwc_sepconv3x3_bwd_workspace_floats
    assert ws(B, H, W, C, F_) == r["part_dw"][1]
    assert lo.crossed(r["d"][1]) == [P29, P30, P31]
    assert r["gd"][0] > P31 and r["gz"][0] > 1 << 32 and r["part_pw"][0] > r["gz"][0] and r["part_dw"][0] > r["part_b"][0]
    assert r["gz"][1] * 4 > 1 << 34                                                     # byte offsets past 2^34
    assert lo.crossed(lo.sepconv_operands((1,) + key[1:])["x"]) == [P29] and ws(1, H, W, C, F_) < P31
    # admitted: sepconv3x3_bwd_shape_ok, each expression once; C <= 2^20 in the C boundary
    text = open(os.path.join(CSRC, "sepconv_bwd.hip")).read()
    body = re.search(r"bool sepconv3x3_bwd_shape_ok\(.*?\{(.*?)\n\}", text, re.S).group(1)
    for expr in ("p.chunks <= 65535", "(p.n_strips * p.cpad + 255) / 256 <= INT32_MAX", "p.n_pb <= INT32_MAX",
                 "(int64_t)F * p.cpad <= INT32_MAX / 2", "(int64_t)C * 9 <= INT32_MAX / 2"):
        assert body.count(expr) == 1, expr
    assert body.count("return") == 1
    strips = B * H * -(-W // SCB["kScbStrip"])
    assert -(-strips * C // 256) <= 2 ** 31 - 1 and -(-B * H * W // SCB["kScbPx"]) <= 2 ** 31 - 1
    # the rule bounds grids, not bytes: one step past the stage-A grid is refused by name
    assert ws(1 << 14, 1 << 14, 1 << 13, 32, 16) == _hip.E_SHAPE
    assert b"too large for the backward's launch grids" in hip_lib.qpwc_last_error()
    planned = lo.sepconv_planned_bytes(key, ws(B, H, W, C, F_), ws(1, H, W, C, F_))
    assert 4 * (n["x"] + n["grad_x"] + n["grad_out"] + n["d"] + n["gd"] + n["gz"]) <= planned <= 48 * lo.GIB
    assert 1.10 * planned <= 64 * lo.GIB


@pytest.mark.parametrize("flags", [(True, True), (False, False)], ids=["11", "00"])
def test_sepconv_crop_restatement_is_the_layer(flags):
    key = (2, 40, 45, 32, 16, 1)
    gen = torch.Generator().manual_seed(7)
    x, dw, pw, b = (_grid(gen, (2, 40, 45, 32), 1 / 16), _grid(gen, (32, 1, 3, 3), 1 / 8), _grid(gen, (16, 32), 1 / 8),
                    _grid(gen, (16,), 1 / 8))
    go = _grid(gen, (2, 40, 45, 16), 1 / 16)
    leaves = [t.clone().requires_grad_() for t in (x, dw, pw, b)]
    out = sep_composite([leaves[0]], leaves[1], leaves[2], leaves[3], *flags)
    out.backward(go)
    C = lo.CROP
    for reg in (("tl", 0, 0, C, 0, C), ("mid", 1, 5, 5 + C, 7, 7 + C), ("br", 1, 40 - C, 40, 45 - C, 45)):
        (cy0, cy1, cx0, cx1), pads = lo.conv_x_region(key, reg)
        n = reg[1]
        ro, rx, _, _ = lo.conv_region_ref(key, x[n:n + 1, cy0:cy1, cx0:cx1], pads, (dw, pw), b,
                                          go[n:n + 1, reg[2]:reg[3], reg[4]:reg[5]], flags)
        assert float((ro - out.detach()[n:n + 1, reg[2]:reg[3], reg[4]:reg[5]]).abs().max()) < 1e-12
        ok = lo.conv_gx_valid(key, reg)
        assert int(ok.sum()) >= (C - 2) ** 2
        assert float((rx[0][ok] - leaves[0].grad[n, cy0:cy1, cx0:cx1][ok]).abs().max()) < 1e-12
        assert float((rx[0][~ok] - leaves[0].grad[n, cy0:cy1, cx0:cx1][~ok]).abs().max()) > 1e-3
    wins = [("a", 0, 0, 16, 0, 16), ("b", 1, 3, 19, 9, 25), ("c", 1, 24, 40, 29, 45)]
    sparse = torch.zeros_like(go)
    crops = []
    for reg in wins:
        sparse[reg[1], reg[2]:reg[3], reg[4]:reg[5]] = go[reg[1], reg[2]:reg[3], reg[4]:reg[5]]
        (cy0, cy1, cx0, cx1), pads = lo.conv_x_region(key, reg)
        crops.append((x[reg[1]:reg[1] + 1, cy0:cy1, cx0:cx1], pads, go[reg[1]:reg[1] + 1, reg[2]:reg[3], reg[4]:reg[5]]))
    leaves = [t.clone().requires_grad_() for t in (x, dw, pw, b)]
    sep_composite([leaves[0]], leaves[1], leaves[2], leaves[3], *flags).backward(sparse)
    rw, rb = lo.conv_window_sums(key, crops, (dw, pw), b, flags)
    want = torch.cat([leaves[1].grad.flatten(), leaves[2].grad.flatten()])
    assert float((rw - want).abs().max()) < 1e-11 and float((rb - leaves[3].grad).abs().max()) < 1e-11


@pytest.mark.parametrize("flags", [(True, True), (False, False)], ids=["11", "00"])
def test_sepconv_window_sums_bounds_and_negative_controls(flags):
    key = lo.CASES[SEP]
    gen = torch.Generator().manual_seed(13)
    C, F_ = key[3], key[4]
    dw, pw, b = _grid(gen, (C, 1, 3, 3), 1 / 8), _grid(gen, (F_, C), 1 / 8), _grid(gen, (F_,), 1 / 8)
    crops, moved = [], []
    for k, reg in enumerate(lo.conv_windows(key)):
        (cy0, cy1, cx0, cx1), pads = lo.conv_x_region(key, reg)
        crops.append((_grid(gen, (1, cy1 - cy0, cx1 - cx0, C), 1 / 16), pads,
                      _grid(gen, (1, reg[3] - reg[2], reg[5] - reg[4], F_), 1 / 16)))
        for mod, _ in lo.conv_wrapped_regions(key, reg):
            moved.append(("window %d mod %d" % (k, mod), k, _grid(gen, (1, cy1 - cy0, cx1 - cx0, C), 1 / 16)))
    rw, rb = lo.conv_window_sums(key, crops, (dw, pw), b, flags)
    gw32, gb32 = 0.0, 0.0
    for xc, pads, gc in crops:
        lv = [t.float().clone().requires_grad_() for t in (xc, dw, pw, b)]
        xp = torch.nn.functional.pad(lv[0], (0, 0) + tuple(pads))
        d = lo.torch_ref.depthwise3x3([xp], lv[1], flags[0])[:, 1:-1, 1:-1]
        z = d @ lv[2].t() + lv[3]
        (lo.torch_ref.mish(z) if flags[1] else z).backward(gc.float())
        gw32, gb32 = gw32 + torch.cat([lv[1].grad.flatten(), lv[2].grad.flatten()]), gb32 + lv[3].grad
    rdw, rpw = rw[:C * 9], rw[C * 9:]
    if flags == (False, False):
        assert lo.exactness_precondition(key, crops, (dw, pw), b, unit=2 ** 11) * 2 ** 11 < 2 ** 24
        assert torch.equal(gw32.double(), rw) and torch.equal(gb32.double(), rb)
    else:
        assert float((gw32.double()[:C * 9] - rdw).abs().max()) <= 0.1 * lo._tol(rdw)
        assert float((gw32.double()[C * 9:] - rpw).abs().max()) <= 0.1 * lo._tol(rpw)
        assert float((gb32.double() - rb).abs().max()) <= 0.1 * lo._tol(rb)
    controls = lo.conv_controls(key, crops, moved, (dw, pw), b, flags)
    assert len(controls) == len(crops) + len(moved) and len(moved) >= 2
    assert min(r for _, r in controls) >= 100.0, controls


def test_size_arguments_of_the_sepconv_entry_points():
    from qpwcnet_amd import _hip
    protos = {name: (ret, params) for name, ret, params in parse_header()}
    ret, params = protos["qpwc_sepconv3x3_bwd"]
    # the pixel strides are the sizes there that can be large: an int64_t array on both sides
    assert ret == "int" and params.count("const int64_t*") == 1
    assert _hip.PROTOTYPES["qpwc_sepconv3x3_bwd"][1][2]._type_ is ctypes.c_int64
    ret, params = protos["qpwc_sepconv3x3_bwd_workspace_floats"]
    assert ret == "int64_t" and params == ["int"] * 5
    assert ctypes.sizeof(_hip.PROTOTYPES["qpwc_sepconv3x3_bwd_workspace_floats"][0]) == 8


# ---- cost volume and warp backward ------------------------------------------------------------------------------------
def test_backward_case_crosses_what_it_claims(hip_lib):
    B, H, W, C = lo.CASES["backward"]
    D = (2 * lo.SEARCH + 1) ** 2
    assert B == 3 and H % 2 and W % 2 and H != W
    assert lo.crossed(B * H * W * C) == lo.crossed(B * H * W * D) == [P29, P30, P31]
    assert [lo.locate(b, H, W, C)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    assert [lo.locate(b, H, W, D)[0] for b in lo.BOUNDARIES] == [0, 1, 2]        # 81 floats a pixel
    assert lo.crossed(B * H * W * 2) == []                                            # the flow stays small
    assert lo.crossed(H * W * C) == [P29] and lo.crossed(H * W * D) == [P29]          # one image alone
    # the kernels walk pixel groups in grid-stride order past the grid cap; the last trip is uneven
    threads = _backward_cap() * 256
    assert B * H * W * 64 > 4 * threads and (B * H * W * 64) % threads
    # admitted: check_common asks for positive extents only; the fp16 workspace of the warp is the image's size
    from qpwcnet_amd import _hip
    assert hip_lib.qpwc_warp_bwd_workspace_floats(B, H, W, C, _hip.F16) == B * H * W * C > P31
    assert hip_lib.qpwc_warp_bwd_workspace_floats(B, H, W, C, _hip.F32) == 0
    # planned memory of the two tests, as they state it
    n_in, n_cv = B * H * W * C, B * H * W * D
    assert 4 * (2 * n_in + 2 * n_cv + n_in) <= lo.cost_volume_planned_bytes(lo.CASES["backward"]) <= 48 * lo.GIB
    assert 4 * 3 * n_in <= lo.warp_planned_bytes(lo.CASES["backward"]) <= 48 * lo.GIB
    # the crops hold the pixel before and the pixel at every boundary, `margin` inside the region of the reference
    for ch, margin in ((C, lo.SEARCH), (D, lo.SEARCH), (C, lo.REACH + 2)):
        crops = lo.pixel_crops(B, H, W, ch, margin)
        assert [c[0] for c in crops] == [">2^29", ">2^30", ">2^31", "last"]
        for b, c in zip(lo.BOUNDARIES, crops):
            n, y, x = lo.locate(b, H, W, ch)
            assert c[1] == n and c[2] <= y < c[3] and c[4] <= x - 1 and x < c[5]
            assert c[6] == (c[2] - margin, c[3] + margin, c[4] - margin, c[5] + margin)
        assert crops[-1][1:6] == (B - 1, H - lo.CROP, H, W - lo.CROP, W) and crops[-1][6][1::2] == (H, W)


def test_cost_volume_bwd_restatement_is_the_derivative():
    """cost_volume_bwd_ref against float64 autograd of oracle.torch_ref.cost_volume fed its own output, whole and on a
    region with the reference's margin; a random saved output changes the result (the mask is really read)."""
    from oracle import torch_ref
    gen = torch.Generator().manual_seed(8)
    prv, nxt, g = _grid(gen, (1, 20, 23, 8), 1 / 16), _grid(gen, (1, 20, 23, 8), 1 / 16), _grid(gen, (1, 20, 23, 81), 1 / 16)
    a, b = prv.clone().requires_grad_(), nxt.clone().requires_grad_()
    out = torch_ref.cost_volume(a, b, 4)
    out.backward(g)
    out = out.detach()
    gp, gn = lo.cost_volume_bwd_ref(prv, nxt, out, g)
    assert float((gp - a.grad).abs().max()) < 1e-14 and float((gn - b.grad).abs().max()) < 1e-14
    m = lo.SEARCH
    cut = lambda t: t[:, 2:18, 3:20]
    gp2, gn2 = lo.cost_volume_bwd_ref(cut(prv), cut(nxt), cut(out), cut(g))
    assert float((gp2[:, m:-m, m:-m] - cut(a.grad)[:, m:-m, m:-m]).abs().max()) < 1e-14
    assert float((gn2[:, m:-m, m:-m] - cut(b.grad)[:, m:-m, m:-m]).abs().max()) < 1e-14
    assert float((gn2 - cut(b.grad)).abs().max()) > 1e-3                               # the margin is needed
    other = lo.cost_volume_bwd_ref(prv, nxt, _grid(gen, (1, 20, 23, 81), 1 / 16), g)[0]
    assert float((other - gp).abs().max()) > 100 * lo._tol(gp)


@pytest.mark.parametrize("mode", ["clamp", "tfwarp"])
def test_warp_bwd_reference_on_a_region(mode):
    """warp_bwd_ref on a region REACH + 2 wider than what is compared equals the gradient of the whole image there,
    also where the region ends at the image's last row and column; and the fp32 composition stays within the bound."""
    gen = torch.Generator().manual_seed(9)
    img, flo, g = _grid(gen, (1, 60, 64, 4), 1 / 16), _flow(gen, 1, 60, 64, lo.REACH), _grid(gen, (1, 60, 64, 4), 1 / 16)
    _, gi, gf = _oracle_warp(img, flo, g, mode)
    m = lo.REACH + 2
    for y0, y1, x0, x1 in ((10, 10 + lo.CROP + 2 * m, 12, 12 + lo.CROP + 2 * m), (60 - lo.CROP - m, 60, 64 - lo.CROP - m, 64)):
        cut = lambda t: t[:, y0:y1, x0:x1]
        ri, rf = lo.warp_bwd_ref(cut(img), cut(flo), cut(g), mode)
        ys = slice(m, m + lo.CROP)
        assert float((ri[:, ys, ys] - cut(gi)[:, ys, ys]).abs().max()) < 1e-13
        assert float((rf[:, ys, ys] - cut(gf)[:, ys, ys]).abs().max()) < 1e-13
        r32 = lo.warp_bwd_ref(cut(img).float(), cut(flo).float(), cut(g).float(), mode)
        a32, f32 = cut(img).float().requires_grad_(), cut(flo).float().requires_grad_()
        (lo.torch_ref.warp_v2 if mode == "clamp" else lo.torch_ref.tf_warp)(a32, f32).backward(cut(g).float())
        assert float((a32.grad.double() - r32[0]).abs().max()) <= 0.1 * lo._tol(r32[0])
        assert float((f32.grad.double() - r32[1]).abs().max()) <= 0.1 * lo._tol(r32[1])


def test_size_arguments_of_the_backward_entry_points():
    from qpwcnet_amd import _hip
    protos = {name: (ret, params) for name, ret, params in parse_header()}
    for name in ("qpwc_cost_volume_bwd", "qpwc_warp_bwd"):
        assert name in _hip.PROTOTYPES and protos[name][0] == "int"
        assert set(protos[name][1]) <= {"const void*", "void*", "int", "float"}          # extents only, each small
    ret, params = protos["qpwc_warp_bwd_workspace_floats"]
    assert ret == "int64_t" and ctypes.sizeof(_hip.PROTOTYPES["qpwc_warp_bwd_workspace_floats"][0]) == 8


# ---- losses: what Step 0 of the audit found ---------------------------------------------------------------------------
def test_loss_validator_refuses_what_the_kernels_decode_in_32_bits(hip_lib):
    """loss_pixel_kernel decodes a pixel inside its image as `(int)(i - b * plane)` and loss_area_tile_kernel counts the
    ground truth's tiles in an `int`: an image, or a level, of 2^31 pixels and a ground truth of 2^31 tiles are refused
    by name, one step below they are admitted."""
    from qpwcnet_amd import _hip
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("loss_common.h", "loss.hip", "masked_loss.hip"))
    assert text.count("const int r = (int)(i - b * plane);") == 1 and text.count("const int ntiles = B * tiles_y * tiles_x;") == 1
    I = ctypes.c_int

    def ws(kind, B, H, W, h, w):
        return hip_lib.qpwc_loss_workspace_floats(kind, B, H, W, 2, (I * 1)(h), (I * 1)(w), 1)

    v2, mse = _hip.LOSS_FLOW_MSE_V2, _hip.LOSS_FLOW_MSE
    assert ws(v2, 3, 1 << 15, 1 << 15, 1 << 14, 1 << 14) > 0                        # 2^30 pixels an image, 3 images
    assert ws(v2, 1, 1 << 16, (1 << 15) - 1, 1 << 15, (1 << 15) - 1) > 0             # 2^31 - 2^16 pixels
    assert ws(v2, 1, 1 << 16, 1 << 15, 1 << 15, 1 << 14) == _hip.E_SHAPE
    assert b"pixels per image" in hip_lib.qpwc_last_error()
    assert ws(v2, 2047, 1 << 15, 1 << 15, 1 << 14, 1 << 14) > 0                      # 2047 * 2^20 tiles
    assert ws(v2, 2048, 1 << 15, 1 << 15, 1 << 14, 1 << 14) == _hip.E_SHAPE
    assert b"tiles of 32 x 32" in hip_lib.qpwc_last_error()
    assert ws(mse, 2048, 1 << 15, 1 << 15, 1 << 14, 1 << 14) > 0                     # no tile path, no tile count
    assert ws(mse, 1, 8, 8, 1 << 16, (1 << 15) - 1) > 0                              # a bilinear level may be larger
    assert ws(mse, 1, 8, 8, 1 << 16, 1 << 15) == _hip.E_SHAPE
    assert b"level 0" in hip_lib.qpwc_last_error()


# ---- the interpolator's pieces ----------------------------------------------------------------------------------------
IH = {k: int(re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % k, open(os.path.join(CSRC, "interp.hip")).read())[0])
      for k in ("kIhC", "kIhK", "kIhPx", "kIhBlocks", "kUiBlocks", "kUiBwdBlocks", "kApTilePx", "kApMaxLevels")}


def test_interp_cases_cross_what_they_claim(hip_lib):
    from qpwcnet_amd import _hip
    # image head: M > 2^25 pixels of 64 features; ih_plan() restated; M is 64-bit on both sides, the cap 2^40
    B, H, W = lo.CASES["image_head"]
    M = B * H * W
    assert B == 3 and H % 2 and W % 2 and M > 1 << 25 and M % IH["kIhPx"]
    assert lo.crossed(M * IH["kIhC"]) == [P29, P30, P31] and lo.crossed(M * IH["kIhK"]) == []
    assert [lo.locate(b, H, W, 64)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    blocks = min(-(-M // IH["kIhPx"]), IH["kIhBlocks"])
    ws = hip_lib.qpwc_image_head_bwd_workspace_floats
    assert ws(M) == blocks * IH["kIhK"] * IH["kIhC"] + -(-blocks * IH["kIhK"] // 4) * 4 and blocks == IH["kIhBlocks"]
    assert ws(1 << 40) > 0 and ws((1 << 40) + 1) == _hip.E_SHAPE and b"2^40" in hip_lib.qpwc_last_error()
    protos = {name: (ret, params) for name, ret, params in parse_header()}
    for name in ("qpwc_image_head_fwd", "qpwc_image_head_bwd", "qpwc_image_head_bwd_workspace_floats"):
        assert protos[name][1][-2 if name != "qpwc_image_head_bwd_workspace_floats" else -1] == "int64_t", name
        args = _hip.PROTOTYPES[name][1]
        assert ctypes.sizeof(args[-2] if name != "qpwc_image_head_bwd_workspace_floats" else args[-1]) == 8
    assert 4 * 2 * M * 64 <= lo.image_head_planned_bytes(lo.CASES["image_head"], ws(M)) <= 48 * lo.GIB
    wins = lo.pixel_windows(B, H, W, 64)
    assert [w[0] for w in wins] == ["first", ">2^29", ">2^30", ">2^31", "last"]
    moved = [lo.wrapped_pixel_regions(B, H, W, 64, w) for w in wins]
    assert moved[0] == [] and all(m for m in moved[1:]) and {mod for m in moved for mod, _ in m} == {1 << 31, 1 << 32}
    for b, w in zip(lo.BOUNDARIES, wins[1:4]):
        assert b < ((w[1] * H + w[2]) * W + w[4]) * 64 < b + 2 * W * 64
    # image upsampling: C = 3, more than 2^31 output elements, the input itself past 2^29
    B, h, w, C = lo.CASES["upsample2x_image"]
    assert B == 3 and h % 2 and w % 2 and C == 3
    assert lo.crossed(4 * B * h * w * C) == [P29, P30, P31] and lo.crossed(B * h * w * C) == [P29]
    assert [lo.locate(b, 2 * h, 2 * w, C)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    assert max(h, w) <= 1 << 29 and 4 * B * h * w > 4 * IH["kUiBlocks"] * 256 and B * h * w > 4 * IH["kUiBwdBlocks"] * 256
    assert 4 * 10 * B * h * w * C <= lo.upsample_planned_bytes(lo.CASES["upsample2x_image"]) <= 48 * lo.GIB
    # the pyramid: levels = 5, more than 2^31 input elements, H and W multiples of 32
    B, H, W, C, levels = lo.CASES["avgpool_pyramid"]
    S = 1 << levels
    assert B == 3 and levels == 5 <= IH["kApMaxLevels"] and H % S == 0 and W % S == 0 and H != W
    assert lo.crossed(B * H * W * C) == [P29, P30, P31] and [lo.locate(b, H, W, C)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    assert 4 * B * H * W * C <= lo.pyramid_planned_bytes(lo.CASES["avgpool_pyramid"]) <= 48 * lo.GIB
    TW = min(max(IH["kApTilePx"] // S, S), W)
    assert B * (H // S) * -(-W // TW) <= 2 ** 31 - 1 and (H * W * C) % 2 == 0        # tiles fit; an image alone is 8-byte aligned


def test_interp_references_are_the_layers():
    gen = torch.Generator().manual_seed(14)
    x, g = _grid(gen, (1, 20, 23, 3), 1 / 16), _grid(gen, (1, 40, 46, 3), 1 / 16)
    leaf = x.clone().requires_grad_()
    up = upsample_composite(leaf, 2.0)
    up.backward(g)
    C = lo.CROP
    for reg in (("a", 0, 0, C, 0, C), ("b", 0, 7, 7 + C, 9, 9 + C), ("c", 0, 8, 8 + C, 10, 10 + C), ("d", 0, 40 - C, 40, 46 - C, 46)):
        (iy0, iy1, ix0, ix1), place = lo.upsample_regions(reg, 20, 23)
        ro, rx = lo.upsample_region_ref(x[:, iy0:iy1, ix0:ix1], place, g[:, reg[2]:reg[3], reg[4]:reg[5]], 2.0)
        ok = lo.upsample_valid(reg, 20, 23)
        assert torch.equal(ro, up.detach()[:, reg[2]:reg[3], reg[4]:reg[5]]) and int(ok.sum()) >= (C // 2 - 2) ** 2
        assert torch.equal(rx[0][ok], leaf.grad[0, iy0:iy1, ix0:ix1][ok])
        assert float((rx[0][~ok] - leaf.grad[0, iy0:iy1, ix0:ix1][~ok]).abs().max()) > 1e-3
    xx = _grid(gen, (1, 64, 96, 3), 1 / 16)
    assert torch.equal(lo.pyramid_ref(xx, 5), pyramid_composite(xx, 5))
    # the image head's window sums are those of the composite fed a grad_out that is zero outside the windows
    z, w2, b2, go = _grid(gen, (1, 20, 23, 64), 1 / 16), _grid(gen, (3, 64), 1 / 64, 1 / 8), _grid(gen, (3,), 1 / 8), _grid(gen, (1, 20, 23, 3), 1 / 16)
    sparse = torch.zeros_like(go)
    crops = []
    for y0, x0 in ((0, 0), (12, 15)):
        sparse[:, y0:y0 + 8, x0:x0 + 8] = go[:, y0:y0 + 8, x0:x0 + 8]
        crops.append((z[:, y0:y0 + 8, x0:x0 + 8], go[:, y0:y0 + 8, x0:x0 + 8]))
    leaves = [t.clone().requires_grad_() for t in (z, w2, b2)]
    head_composite(*leaves).backward(sparse)
    gw, gb = lo.head_window_sums(crops, None)
    assert torch.equal(gw, leaves[1].grad) and torch.equal(gb, leaves[2].grad)


def test_image_head_window_controls():
    B, H, W = lo.CASES["image_head"]
    gen = torch.Generator().manual_seed(15)
    crops, moved = [], []
    for k, reg in enumerate(lo.pixel_windows(B, H, W, 64)):
        crops.append((_grid(gen, (1, 16, 16, 64), 1 / 16), _grid(gen, (1, 16, 16, 3), 1 / 16)))
        for mod, _ in lo.wrapped_pixel_regions(B, H, W, 64, reg):
            moved.append(("window %d mod %d" % (k, mod), k, _grid(gen, (1, 16, 16, 64), 1 / 16)))
    assert float(lo.head_window_sums([(z.abs(), g.abs()) for z, g in crops], None)[0].max()) * 2 ** 8 < 2 ** 24
    gw32 = sum(g.float().reshape(-1, 3).t() @ z.float().reshape(-1, 64) for z, g in crops)
    assert torch.equal(gw32.double(), lo.head_window_sums(crops, None)[0])              # exact in fp32 on the grids
    controls = lo.head_controls(crops, moved)
    assert len(controls) == len(crops) + len(moved) and len(moved) >= 2 and min(r for _, r in controls) >= 100.0, controls


def test_flow_head_cap_keeps_its_operands_under_every_boundary(hip_lib):
    """flow_head_train_check_shape caps the training flow head at 2^24 pixels (its pixel counts are fp32): there z has
    2^28 elements and the upsampled gradient 2^27, below 2^29, so no GPU case exists for it; one pixel more is refused
    by name."""
    from qpwcnet_amd import _hip
    text = open(os.path.join(CSRC, "capi.hip")).read()
    body = re.search(r"static int flow_head_train_check_shape\(.*?\{(.*?)\n\}", text, re.S).group(1)
    assert body.count("(int64_t)B * H * W > (1 << 24)") == 1
    cap = 1 << 24
    assert lo.crossed(cap * 16) == [] and lo.crossed(4 * cap * 2) == []
    for fn in (hip_lib.qpwc_flow_head_bwd_workspace_floats, hip_lib.qpwc_flow_head_stats_workspace_floats):
        assert fn(1, 4096, 4096) > 0
        assert fn(1, 4097, 4096) == _hip.E_SHAPE and b"2^24" in hip_lib.qpwc_last_error()
        assert fn(1, cap + 1, 1) == _hip.E_SHAPE and b"more than 2^24 pixels" in hip_lib.qpwc_last_error()


# ---- losses and EPE: the GPU cases --------------------------------------------------------------------------------------
def test_loss_and_epe_cases_cross_what_they_claim(hip_lib):
    from qpwcnet_amd import _hip
    from test_training_scale_cpu import EPE, LOSS
    I = ctypes.c_int
    aligned = 1 << 20

    def pick(kind, B, H, W, h, w):
        return hip_lib.qpwc_loss_fwd_kernel(kind, aligned, B, H, W, 2, (I * 1)(h), (I * 1)(w), 1).decode()

    def ws(kind, B, H, W, h, w):
        return hip_lib.qpwc_loss_workspace_floats(kind, B, H, W, 2, (I * 1)(h), (I * 1)(w), 1)

    for name in ("loss", "epe"):
        B, H, W, C = lo.CASES[name]
        assert B == 3 and C == 2 and H != W and B * H * W > 1 << 30                  # more than 2^30 ground-truth pixels
        assert lo.crossed(B * H * W * C) == [P29, P30, P31]
        at = [lo.locate(b, H, W, C) for b in lo.BOUNDARIES]
        assert [a[0] for a in at] == [0, 1, 2] and all(0 < y < H - 2 - lo.WIN and 0 < x < W - 1 for _, y, x in at)
        assert H * W <= 2 ** 31 - 1 and B * -(-H // 32) * -(-W // 32) <= 2 ** 31 - 1  # what loss_check_shapes asks
    # the tile case: H, W multiples of the tile, one half-resolution level -> loss_area_tile_kernel, float4 backward
    key = lo.CASES["loss"]
    B, H, W, C = key
    h, w = H // 2, W // 2
    assert H % LOSS["kLossTile"] == 0 and W % LOSS["kLossTile"] == 0
    assert pick(_hip.LOSS_FLOW_MSE_V2, B, H, W, h, w) == "loss_area_tile_kernel"
    assert ws(_hip.LOSS_FLOW_MSE_V2, B, H, W, h, w) == LOSS["kLossTileBlocks"]
    tiles = B * (H // LOSS["kLossTile"]) * (W // LOSS["kLossTile"])
    assert tiles > 256 * LOSS["kLossTileBlocks"] and tiles % LOSS["kLossTileBlocks"]   # every workgroup walks > 256 tiles
    assert lo.crossed(B * h * w * C) == [P29] and (B * h * w * C) % 4 == 0
    assert B * h * w * C // 4 > LOSS["kLossBwdBlocks"] * LOSS["kLossThreads"]
    assert 4 * (B * H * W * C + 4 * B * h * w * C) == lo.loss_planned_bytes(key, (h, w), True) <= 48 * lo.GIB
    wins = lo.loss_tile_windows(key)
    assert [x[0] for x in wins] == ["first", ">2^29", "gt>2^29", "gt>2^30", "gt>2^31", "last"]
    for i, a in enumerate(wins):
        for b_ in wins[i + 1:]:
            assert a[1] != b_[1] or a[3] <= b_[2] or b_[3] <= a[2] or a[5] <= b_[4] or b_[5] <= a[4], (a, b_)
    for b, x in zip(lo.BOUNDARIES, wins[2:5]):                       # the ground truth under a window lies behind its boundary
        assert b < ((x[1] * H + 2 * x[2]) * W + 2 * x[4]) * C < b + 6 * W * C
    assert P29 < ((wins[1][1] * h + wins[1][2]) * w + wins[1][4]) * C < P29 + 2 * w * C
    moved = [lo.wrapped_pixel_regions(B, H, W, C, (x[0], x[1], 2 * x[2], 2 * x[3], 2 * x[4], 2 * x[5])) for x in wins]
    assert moved[0] == [] and all(m for m in moved[1:]) and {mod for m in moved for mod, _ in m} == {1 << 31, 1 << 32}
    # the odd case: a full-resolution level -> loss_pixel_kernel for the area loss (1 x 1) and the bilinear one, the
    # scalar backward (no multiple of 4), the EPE kernels' float4 loop with the odd last pixel
    key = lo.CASES["epe"]
    B, H, W, C = key
    assert H % 2 and W % 2 and (B * H * W) % 2 and (B * H * W * C) % 4
    for kind in (_hip.LOSS_FLOW_MSE_V2, _hip.LOSS_FLOW_MSE):
        assert pick(kind, B, H, W, H, W) == "loss_pixel_kernel" and ws(kind, B, H, W, H, W) > 0
    assert B * H * W > LOSS["kLossPixBlocks"] * LOSS["kLossThreads"] and B * H * W * C > LOSS["kLossBwdBlocks"] * LOSS["kLossThreads"]
    assert B * H * W // 2 > 3 * EPE["kEpeMultiBlocks"] * EPE["kEpeThreads"] and B * H * W > EPE["kEpeBlocks"] * EPE["kEpeThreads"]
    assert 4 * 4 * B * H * W * C == lo.loss_planned_bytes(key, (H, W), False) <= 48 * lo.GIB
    wins = lo.pixel_windows(B, H, W, C)
    assert [x[0] for x in wins] == ["first", ">2^29", ">2^30", ">2^31", "last"]
    for b, x in zip(lo.BOUNDARIES, wins[1:4]):
        assert b < ((x[1] * H + x[2]) * W + x[4]) * C < b + 2 * W * C
    moved = [lo.wrapped_pixel_regions(B, H, W, C, x) for x in wins]
    assert moved[0] == [] and all(m for m in moved[1:]) and {mod for m in moved for mod, _ in m} == {1 << 31, 1 << 32}
    # the ctypes widths: element and pixel counts are 64-bit arrays on both sides; the extents are ints the cases keep small
    protos = {name: (ret, params) for name, ret, params in parse_header()}
    assert protos["qpwc_loss_bwd"][1].count("const int64_t*") == 1
    assert _hip.PROTOTYPES["qpwc_loss_bwd"][1][3]._type_ is ctypes.c_int64
    for name in ("qpwc_epe_multi_fwd", "qpwc_epe_multi_mixed_fwd"):
        assert protos[name][1].count("const int64_t*") == 2
        assert [t._type_ for t in _hip.PROTOTYPES[name][1][2:4]] == [ctypes.c_int64, ctypes.c_int64]
    for name in ("qpwc_loss_fwd", "qpwc_epe_fwd", "qpwc_loss_workspace_floats"):
        assert "int64_t" not in protos[name][1] and max(B, H, W) < 2 ** 31
    assert protos["qpwc_loss_workspace_floats"][0] == "int64_t"


@pytest.mark.parametrize("kind", ["v2", "norm"])
def test_loss_window_reference_is_the_loss(kind):
    """loss_window_ref on the windows alone is the loss of the whole tensors when the prediction equals the level's
    ground truth elsewhere, and that loss is Keras' Huber mean / the mean end-point error; area_level_ref is the area
    mean times the flow scale; the fp32 composition stays within a tenth of the GPU test's bound."""
    from oracle import torch_ref
    gen = torch.Generator().manual_seed(16)
    gt = _grid(gen, (2, 40, 48, 2), 1 / 16)
    gl = lo.area_level_ref(gt[:1], 2, 2, 0.5)
    want = torch.nn.functional.avg_pool2d(gt[:1].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * 0.5
    assert torch.equal(gl, want)
    gl = torch.cat([gl, lo.area_level_ref(gt[1:], 2, 2, 0.5)])
    pred = gl.clone()
    wins = [(0, 0, 8, 0, 8), (1, 5, 13, 9, 17), (1, 12, 20, 0, 8)]
    crops = []
    for n, y0, y1, x0, x1 in wins:
        pred[n, y0:y1, x0:x1] += _grid(gen, (y1 - y0, x1 - x0, 2), 1 / 16)
        crops.append((gl[n:n + 1, y0:y1, x0:x1], pred[n:n + 1, y0:y1, x0:x1]))
    hw, n_pix = (20, 24), 2 * 20 * 24
    value, grads = lo.loss_window_ref(kind, crops, n_pix, hw, 7.0)
    whole, gw = lo.loss_window_ref(kind, [(gl, pred)], n_pix, hw, 7.0)
    assert abs(float(value - whole)) <= 1e-15 * abs(float(whole)) + 1e-300
    for (n, y0, y1, x0, x1), g in zip(wins, grads):
        assert torch.equal(g[0], gw[0][n, y0:y1, x0:x1])
    if kind == "v2":
        s = 2.0 / (hw[0] + hw[1])
        other = 7.0 * torch.nn.functional.huber_loss(s * pred, s * gl, delta=lo.LOSS_DELTA)
    else:
        other = 7.0 * torch_ref.epe_error(gl, pred)
    assert abs(float(other - whole)) <= 1e-12 * abs(float(whole))
    v32 = lo.loss_window_ref(kind, [(a.float(), b.float().double()) for a, b in crops], n_pix, hw, 7.0)[0]
    assert abs(float(v32 - value)) <= 0.1 * lo.LOSS_REL * abs(float(value))


@pytest.mark.parametrize("name,kind", [("loss", "v2"), ("epe", "v2"), ("epe", "norm")])
def test_loss_negative_controls(name, kind):
    key = lo.CASES[name]
    B, H, W, C = key
    tile = name == "loss"
    h, w = (H // 2, W // 2) if tile else (H, W)
    gen = torch.Generator().manual_seed(17)
    crops, moved = [], []
    for k, reg in enumerate(lo.loss_tile_windows(key) if tile else lo.pixel_windows(B, H, W, C)):
        level = (lambda: lo.area_level_ref(_grid(gen, (1, 32, 32, 2), 1 / 16), 2, 2, 0.5)) if tile else \
            (lambda: _grid(gen, (1, 16, 16, 2), 1 / 16))
        gl = level()
        crops.append((gl, gl + _grid(gen, (1, 16, 16, 2), 1 / 16)))
        gt_reg = (reg[0], reg[1], 2 * reg[2], 2 * reg[3], 2 * reg[4], 2 * reg[5]) if tile else reg
        for mod, _ in lo.wrapped_pixel_regions(B, H, W, C, gt_reg):
            moved.append(("window %d mod %d" % (k, mod), k, level()))
    controls = lo.loss_controls(kind, crops, moved, B * h * w, (h, w))
    assert len(controls) == len(crops) + len(moved) and len(moved) >= 2
    assert min(r for _, r in controls) >= 100.0, controls


# ---- masked losses and flow metrics: byte-indexed masks, 2^32 elements -------------------------------------------------
P32 = 1 << 32


def _disjoint(a, b):
    return a[1] != b[1] or a[3] <= b[2] or b[3] <= a[2] or a[5] <= b[4] or b[5] <= a[4]


def test_masked_loss_cases_cross_what_they_claim(hip_lib):
    from qpwcnet_amd import _hip, ops
    from test_eval_scale_cpu import ML
    I = ctypes.c_int
    assert lo.BOUNDARIES_32 == (P29, P30, P31, P32)
    # the tile case: the smallest 32-multiple square at B = 3 whose pixel count passes 2^31
    key = lo.CASES["masked_loss"]
    B, H, W, C = key
    assert B == 3 and C == 2 and H % ML["kLossTile"] == 0 and W % ML["kLossTile"] == 0
    assert B * H * W > P31 > B * (H - 32) * (W - 32)                             # the mask's byte index passes 2^31
    assert lo.crossed(B * H * W * C, lo.BOUNDARIES_32) == [P29, P30, P31, P32]   # the ground truth's element index
    assert [lo.locate(b, H, W, C)[0] for b in lo.BOUNDARIES_32] == [0, 0, 1, 2]
    assert [lo.locate(b, H, W, 1)[0] for b in (P29, P30, P31)] == [0, 1, 2]
    factors = [(2, 2), (32, 32)]
    levels = [(H // sh, W // sw) for sh, sw in factors]
    assert lo.crossed(B * levels[0][0] * levels[0][1] * C, lo.BOUNDARIES_32) == [P29, P30]
    assert H * W <= 2 ** 31 - 1 and B * (H // 32) * (W // 32) <= 2 ** 31 - 1    # what loss_check_shapes caps: not B * H * W
    hs, ws_ = (I * 2)(*[h for h, _ in levels]), (I * 2)(*[w for _, w in levels])
    assert hip_lib.qpwc_masked_loss_workspace_floats(_hip.LOSS_FLOW_MSE_V2, B, H, W, C, hs, ws_, 2) == 2 * 2 * ML["kLossTileBlocks"]
    assert ops.masked_loss_kernel(_hip.LOSS_FLOW_MSE_V2, B, H, W, levels) == "masked_loss_tile_kernel"
    tiles = B * (H // 32) * (W // 32)
    assert tiles > 1000 * ML["kLossTileBlocks"] and tiles % ML["kLossTileBlocks"]
    assert (B * levels[0][0] * levels[0][1] * C) % 4 == 0                        # the float4 backward at level 0
    wins = lo.masked_loss_windows(key, levels[0])
    assert [x[0] for x in wins] == ["first", ">2^29", ">2^30", ">2^31", ">2^32", "pred>2^29", "pred>2^30", "last"]
    regs = [lo.aligned_region(x, 32, H, W) for x in wins]
    assert all(_disjoint(a, b) for i, a in enumerate(regs) for b in regs[i + 1:])
    for x, r in zip(wins, regs):
        assert r[2] % 32 == 0 and r[4] % 32 == 0 and (r[3] - r[2]) % 32 == 0 and (r[5] - r[4]) % 32 == 0
        assert r[2] <= x[2] and x[3] <= r[3] and r[4] <= x[4] and x[5] <= r[5] and r[3] <= H and r[5] <= W
    first = lambda x, rows, cols, ch, f=1: ((x[1] * rows + x[2] // f) * cols + x[4] // f) * ch
    for b, x in zip(lo.BOUNDARIES_32, wins[1:5]):                    # behind each boundary of the ground truth ...
        assert b < first(x, H, W, C) < b + 2 * W * C
    for b, x in zip((P29, P30, P31), wins[2:5]):                     # ... which is where the mask's byte boundaries lie
        assert b < first(x, H, W, 1) < b + 2 * W
    for b, x in zip((P29, P30), wins[5:7]):                          # and of the level's prediction, dpred and grad_pred
        assert b < first(x, levels[0][0], levels[0][1], C, 2) < b + 2 * levels[0][1] * C
    # a wrapped read: of the ground truth, other values inside the tensor; of the mask, no window
    moved = [lo.wrapped_pixel_regions(B, H, W, C, x) for x in wins]
    assert {mod for m in moved for mod, _ in m} == {1 << 31, 1 << 32} and all(m for m in moved[2:])
    mask_moved = [lo.wrapped_pixel_regions(B, H, W, 1, x, 1) for x in wins]
    assert any(m for m in mask_moved) and mask_moved[0] == []
    for m in mask_moved:
        for _, at in m:
            assert all(_disjoint(("at",) + at, x) for x in wins), at
    planned = lo.masked_loss_planned_bytes(key, levels, 4)
    assert 4 * B * H * W * C + B * H * W + 4 * 4 * B * levels[0][0] * levels[0][1] * C <= planned <= 48 * lo.GIB
    assert 36e9 < planned < 38e9 and 1.10 * planned <= 64 * lo.GIB
    # the pixel case: the odd "epe" shape with one full-resolution level
    key = lo.CASES["masked_loss_pixel"]
    assert key == lo.CASES["epe"]
    B, H, W, C = key
    assert lo.crossed(B * H * W * C, lo.BOUNDARIES_32) == [P29, P30, P31] and lo.crossed(B * H * W, lo.BOUNDARIES_32) == [P29, P30]
    assert (B * H * W * C) % 4 == 2 and B * H * W * C > ML["kLossBwdBlocks"] * ML["kLossThreads"]
    for kind in (_hip.LOSS_FLOW_MSE_V2, _hip.LOSS_FLOW_MSE):
        assert ops.masked_loss_kernel(kind, B, H, W, [(H, W)]) == "masked_loss_pixel_kernel"
    assert B * H * W > 4096 * ML["kLossPixBlocks"] * ML["kLossThreads"]          # thousands of trips of the pixel walk
    wins = lo.masked_loss_windows(key)
    assert [x[0] for x in wins] == ["first", ">2^29", ">2^30", ">2^31", "last"]
    assert all(_disjoint(a, b) for i, a in enumerate(wins) for b in wins[i + 1:])
    for b, x in zip((P29, P30), wins[2:4]):
        assert b < first(x, H, W, 1) < b + 2 * W
    for x in wins:
        for _, at in lo.wrapped_pixel_regions(B, H, W, 1, x, 1):
            assert all(_disjoint(("at",) + at, y) for y in wins), at
    assert lo.masked_loss_planned_bytes(key, [(H, W)], 3) <= 48 * lo.GIB
    # the sizes that pass 2^31 travel as 64-bit integers
    protos = {name: (ret, params) for name, ret, params in parse_header(os.path.join(os.path.dirname(CSRC), "..", "include",
                                                                                     "qpwc_masked_loss.h"))}
    assert protos["qpwc_masked_loss_bwd"][1].count("const int64_t*") == 1
    assert any(getattr(t, "_type_", None) is ctypes.c_int64 for t in _hip.MASKED_LOSS_PROTOTYPES["qpwc_masked_loss_bwd"][1])


@pytest.mark.parametrize("kind", ["v2", "norm"])
def test_masked_window_reference_is_the_masked_loss(kind):
    """masked_area_level_ref / masked_window_ref on the windows' regions alone against loss.multiscale_masked_torch and
    masked_ground_truth_torch in float64 on whole (small) tensors whose validity is zero outside the windows, with
    random predictions everywhere."""
    from qpwcnet_amd import loss
    gen = torch.Generator().manual_seed(21)
    B, H, W = 2, 96, 128
    gt = _grid(gen, (B, H, W, 2), 1 / 16)
    valid = torch.zeros(B, H, W, dtype=torch.uint8)
    wins = [("a", 0, 0, 16, 0, 16), ("b", 1, 37, 53, 71, 87), ("c", 1, 80, 96, 112, 128)]
    for _, n, y0, y1, x0, x1 in wins:
        valid[n, y0:y1, x0:x1] = 1
    factors = [(2, 2), (32, 32)] if kind == "v2" else [(1, 1)]
    obj = loss.FlowMseLossV2() if kind == "v2" else loss.FlowMseLoss("channels_last")
    if kind == "v2":
        obj.delta = lo.LOSS_DELTA
    levels = [(H // sh, W // sw) for sh, sw in factors]
    preds = [_grid(gen, (B, h, w, 2), 1 / 16) for h, w in levels]
    xs = [p.clone().requires_grad_() for p in preds]
    _, per, counts = loss.multiscale_masked_torch(obj, gt, xs, valid)
    (7.0 * per).sum().backward()
    gts, masks_ = loss.masked_ground_truth_torch(obj, gt, levels, valid)
    regs = [lo.aligned_region(x, 32 if kind == "v2" else 1, H, W) for x in wins]
    for l, (sh, sw) in enumerate(factors):
        crops = []
        for _, n, y0, y1, x0, x1 in regs:
            gl, m = lo.masked_area_level_ref(gt[n:n + 1, y0:y1, x0:x1], valid[n:n + 1, y0:y1, x0:x1], sh, sw, 1.0 / sh)
            cut = lambda t: t[n:n + 1, y0 // sh:y1 // sh, x0 // sw:x1 // sw]
            assert float((gl - cut(gts[l])).abs().max()) <= 1e-15 and torch.equal(m, cut(masks_[l]) != 0)
            crops.append((gl, m, cut(preds[l])))
        value, grads, count = lo.masked_window_ref(kind, crops, levels[l], 7.0)
        assert count == int(counts[l]) == int(masks_[l].sum()) > 0
        assert abs(float(value) - 7.0 * float(per[l].detach())) <= 1e-12 * abs(float(value))
        inside = torch.zeros_like(xs[l].grad, dtype=torch.bool)
        for (_, n, y0, y1, x0, x1), g in zip(regs, grads):
            got = xs[l].grad[n:n + 1, y0 // sh:y1 // sh, x0 // sw:x1 // sw]
            assert float((got - g).abs().max()) <= 1e-12 * float(g.abs().max())
            inside[n:n + 1, y0 // sh:y1 // sh, x0 // sw:x1 // sw] = True
        assert not xs[l].grad[~inside].any()


@pytest.mark.parametrize("name,kind", [("masked_loss", "v2"), ("masked_loss_pixel", "v2"), ("masked_loss_pixel", "norm")])
def test_masked_loss_negative_controls(name, kind):
    key = lo.CASES[name]
    B, H, W, C = key
    tile = name == "masked_loss"
    factors = [(2, 2), (32, 32)] if tile else [(1, 1)]
    wins = lo.masked_loss_windows(key, (H // 2, W // 2) if tile else None)
    regs = [lo.aligned_region(x, 32 if tile else 1, H, W) for x in wins]
    gen = torch.Generator().manual_seed(22)
    data = []
    for x, r in zip(wins, regs):
        ok = torch.zeros(1, r[3] - r[2], r[5] - r[4], dtype=torch.uint8)
        ok[:, x[2] - r[2]:x[3] - r[2], x[4] - r[4]:x[5] - r[4]] = 1
        data.append((_grid(gen, (1, r[3] - r[2], r[5] - r[4], 2), 1 / 16), ok))
    for sh, sw in factors:
        crops, moved = [], []
        for k, ((g, ok), x, r) in enumerate(zip(data, wins, regs)):
            gl, m = lo.masked_area_level_ref(g, ok, sh, sw, 1.0 / sh)
            crops.append((gl, m, _grid(gen, tuple(gl.shape), 1 / 16)))
            for mod, _ in lo.wrapped_pixel_regions(B, H, W, C, x):            # random data read elsewhere: another draw
                moved.append(("window %d mod %d" % (k, mod), k, lo.masked_area_level_ref(_grid(gen, tuple(g.shape), 1 / 16), ok, sh, sw, 1.0 / sh)[0]))
        controls = lo.masked_loss_controls(kind, crops, moved, (H // sh, W // sw))
        assert len(controls) == len(crops) + len(moved) and len(moved) >= 2
        assert min(r_ for _, r_ in controls) >= 100.0, controls
        # the fp32 composition of the windows' sum stays within a tenth of the bound
        v64 = lo.masked_window_ref(kind, crops, (H // sh, W // sw))[0]
        v32 = lo.masked_window_ref(kind, [(gl.float().double(), m, p) for gl, m, p in crops], (H // sh, W // sw))[0]
        assert abs(float(v32 - v64)) <= 0.1 * lo.LOSS_REL * abs(float(v64))


def test_flow_quality_case_crosses_what_it_claims(hip_lib):
    from qpwcnet_amd import _hip, ops
    from test_eval_scale_cpu import FQ
    key = lo.CASES["flow_quality"]
    B, H, W, C = key
    assert B == 5 and C == 2 and H % 2 and W % 2 and H != W
    assert B * H * W <= 2 ** 31 - 1                                                    # flow_quality_shape_ok's cap
    assert lo.crossed(B * H * W * C) == [P29, P30, P31] and lo.crossed(H * W * C) == []   # one image crosses nothing
    assert [lo.locate(b, H, W, C)[0] for b in lo.BOUNDARIES] == [1, 2, 4]
    assert lo.crossed(B * H * W) == [P29, P30] and [lo.locate(b, H, W, 1)[0] for b in (P29, P30)] == [2, 4]
    # channels-first: `o = 2 * img + p` stays below 2^31 and `o + hw`, the v plane, passes it in the last image, before
    # the pixels of the ">2^31" window and of the last one
    assert 2 * (B - 1) * H * W + H * W < P31 < 2 * B * H * W
    wins = lo.pixel_windows(B, H, W, C)
    assert all(x[1] == B - 1 and 2 * (B - 1) * H * W + x[2] * W + x[4] + H * W > P31 for x in wins[3:])
    chunks = -(-H * W // FQ["kFlowQualChunk"])
    assert chunks > 800 * 64 and hip_lib.qpwc_flow_quality_workspace_floats(B, H, W) == B * chunks * 15
    assert ops.flow_quality_kernel(B, H, W) == "flow_quality_tile_kernel" and ops.flow_quality_kernel(2 * B, H, W) == ""
    wins = lo.pixel_windows(B, H, W, C)
    assert [x[0] for x in wins] == ["first", ">2^29", ">2^30", ">2^31", "last"]
    assert sorted({x[1] for x in wins}) == [0, 1, 2, 4]                                # image 3 holds no window
    assert all(_disjoint(a, b) for i, a in enumerate(wins) for b in wins[i + 1:])
    assert {x[1:] for x in lo.pixel_windows(B, H, W, 1)} <= {x[1:] for x in wins}       # the masks' boundaries: the same places
    for b, x in zip(lo.BOUNDARIES, wins[1:4]):
        assert b < ((x[1] * H + x[2]) * W + x[4]) * C < b + 2 * W * C
    moved = [lo.wrapped_pixel_regions(B, H, W, C, x) for x in wins]
    assert moved[0] == [] and all(m for m in moved[1:]) and {mod for m in moved for mod, _ in m} == {1 << 31, 1 << 32}
    planned = lo.flow_quality_planned_bytes(key)
    assert 4 * 2 * B * H * W * C + 2 * B * H * W <= planned <= 48 * lo.GIB and 19e9 < planned < 25e9


def test_flow_windows_and_their_oracle():
    """The windows' flows keep the bounds' precondition (no pixel within MARGIN of a threshold, in fp32 and in fp16) and
    fill all three speed bins; flow_window_oracle on the crops and the mask counts is ref_flow_quality of whole (small)
    tensors built the way the GPU test builds them; the controls move an image's epe by at least 100 bounds."""
    from test_flow_quality_cpu import FIELDS, near_a_threshold, ref_flow_quality, violations
    n_windows = len(lo.pixel_windows(*lo.CASES["flow_quality"]))
    for half in (False, True):
        for k in range(n_windows):
            t, p = lo.flow_window_data(k, half)
            assert t.shape == (1, lo.WIN, lo.WIN, 2) and p.dtype == (np.float16 if half else np.float32)
            assert not near_a_threshold(t, p).any()
            m = np.hypot(t[..., 0].astype(np.float64), t[..., 1])
            assert (m < 10).any() and ((m >= 10) & (m < 40)).any() and (m >= 40).any()
    rng = np.random.default_rng(23)
    B, H, W = 3, 40, 50
    truth = (rng.integers(-64, 65, (B, H, W, 2)) / 16).astype(np.float32)
    pred = truth.copy()
    valid, occ = rng.random((B, H, W)) < 0.7, rng.random((B, H, W)) < 0.3
    wins = [(0, 0, 0), (0, 20, 30), (2, 24, 34)]
    planted = []
    for k, (n, y, x) in enumerate(wins):
        t, p = lo.flow_window_data(k)
        truth[n, y:y + lo.WIN, x:x + lo.WIN], pred[n, y:y + lo.WIN, x:x + lo.WIN] = t[0], p[0]
        planted.append((n, t, p, valid[n:n + 1, y:y + lo.WIN, x:x + lo.WIN], occ[n:n + 1, y:y + lo.WIN, x:x + lo.WIN]))
    n_valid, n_occ = valid.sum(axis=(1, 2)), (valid & occ).sum(axis=(1, 2))
    got, sums = lo.flow_window_oracle(B, H * W, planted, n_valid, n_occ)
    want = ref_flow_quality(truth, pred, valid, occ)
    assert violations(got, want)[0] == []
    for k in FIELDS:
        keep = ~np.isnan(want[k])
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])) and np.abs(got[k][keep] - want[k][keep]).max() <= 1e-12
    assert got["epe"][1] == 0 and got["acc1"][1] == 1
    moved = [("window 1 elsewhere", 1, truth[1:2, 3:3 + lo.WIN, 5:5 + lo.WIN])]
    big = [150_000_000] * B                                           # the GPU case's counts: the ratios do not depend on them
    controls = lo.flow_controls(B, H * W, planted, moved, big, [45_000_000] * B)
    assert len(controls) == 4 and min(r for _, r in controls) >= 100.0, controls


# ---- the label-free losses ---------------------------------------------------------------------------------------------
def test_unsup_case_crosses_what_it_claims(hip_lib):
    """3 x 15489 x 15497: the frames' element index passes 2^29, 2^30 and 2^31 in images 0, 1 and 2, the flow's 2^29 and
    2^30, the mask's byte index 2^29, the saved planes' 2^29 .. 2^32; the validator admits it and refuses the batch that
    passes 2^31 - 1 pixels; a window lies behind every one of these places, the crops are disjoint, and the plan fits."""
    from qpwcnet_amd import _hip
    key = lo.CASES["unsup_loss"]
    B, H, W = key
    npix = B * H * W
    assert B == 3 and H % 2 and W % 2 and H != W and H % 8 and W % 32                  # ragged: partial tiles on both axes
    assert lo.crossed(3 * npix) == [P29, P30, P31] and [lo.locate(b, H, W, 3)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    assert lo.crossed(2 * npix) == [P29, P30] and lo.crossed(npix) == [P29]
    assert lo.crossed(7 * npix, lo.BOUNDARIES_32) == list(lo.BOUNDARIES_32)
    ha, wa = (ctypes.c_int * 1)(H), (ctypes.c_int * 1)(W)
    tiles = B * -(-H // _hip.UNSUP_LOSS_TILE[0]) * -(-W // _hip.UNSUP_LOSS_TILE[1])
    assert hip_lib.qpwc_unsup_loss_workspace_floats(_hip.UNSUP_CENSUS, B, ha, wa, 1) == 4 * tiles + _hip.UNSUP_LOSS_PLANES * npix
    assert hip_lib.qpwc_unsup_loss_fwd_kernel(_hip.UNSUP_CENSUS, B, ha, wa, 1) == b"unsup_loss_fwd_kernel<census>"
    assert hip_lib.qpwc_unsup_loss_workspace_floats(_hip.UNSUP_CENSUS, 3 * B, ha, wa, 1) == _hip.E_SHAPE   # 2.16 G pixels
    planned = lo.unsup_planned_bytes(key)
    assert planned == 4 * (6 + 2 + 2) * npix + npix + 4 * (4 * tiles + 7 * npix)
    assert planned <= 48 * lo.GIB and 1.10 * planned <= 64 * lo.GIB
    wins = lo.unsup_windows(key)
    tags = [x[0] for x in wins]
    assert len(set(tags)) == len(tags) >= 10 and tags[0] == "first" and tags[-1] == "last"
    # a window in the rows just behind the pixel under every boundary: all of its elements lie beyond it
    under = [lo.locate(b, H, W, ch) for ch in (3, 2, 1) for b in lo.crossed(ch * npix)]
    under += [lo.locate(b % npix, H, W, 1) for b in lo.BOUNDARIES_32]                  # plane b // npix of that pixel
    assert len(under) == 3 + 2 + 1 + 4
    for n, y, x in under:
        assert any(w_[1] == n and w_[2] == y + 1 and w_[4] <= x < w_[5] for w_ in wins), (n, y, x)
    crops = [lo.unsup_grown(x, lo.UNSUP_MARGIN + 1, H, W) for x in wins]
    for i, a in enumerate(crops):
        for c in crops[i + 1:]:
            assert a[1] != c[1] or a[3] <= c[2] or c[3] <= a[2] or a[5] <= c[4] or c[5] <= a[4], (a, c)
    # a control exists: some crop's frames lie beyond each modulus the GPU test wraps at
    for mod_elems in (1 << 29, 1 << 30, 1 << 31):
        assert any(((c[1] * H + c[2]) * W + c[4]) * 3 >= mod_elems for c in crops)
    assert 2.0 ** -20 == lo.UNSUP_PARAMS["smooth_eps"] and np.float32(2.0 ** -40) > 0            # eps_s^2 is a normal fp32


@pytest.mark.parametrize("kind", ["census", "charbonnier"])
def test_unsup_window_oracle_is_the_chain_on_a_small_level(kind):
    """unsup_window_ref against the float64 chain on a whole level that is small enough to have one: 3 x 61 x 67 with a
    window in the first corner, one inside image 1 and one in the last corner -- count exact, values and gradients within
    1e-12, the chain's gradient exactly 0 outside the crops, and a crop with other frames moves the value."""
    from qpwcnet_amd import loss
    key = (3, 61, 67)
    B, H, W = key
    wins = [("first", 0, 0, lo.WIN, 0, lo.WIN), ("inside", 1, 20, 20 + lo.WIN, 25, 25 + lo.WIN),
            ("last", 2, H - lo.WIN, H, W - lo.WIN, W)]
    prv, nxt = (torch.full((B, H, W, 3), lo.UNSUP_COLOUR) for _ in range(2))
    flow, occ = torch.zeros((B, H, W, 2)), torch.ones((B, H, W), dtype=torch.uint8)
    plants = [lo.unsup_plant(k, x, key) for k, x in enumerate(wins)]
    lo.unsup_fill(prv, nxt, flow, occ, wins, plants)
    regs = [p["crop"] for p in plants]
    crops = [lo.unsup_cut(prv, nxt, flow, occ, r) for r in regs]
    photo, smooth, count, grads, share = lo.unsup_window_ref(kind, crops, key, torch.float64)
    p = lo.UNSUP_PARAMS
    obj = loss.PhotometricLoss(kind, data_format="channels_last", **p)
    x = flow.double().requires_grad_()
    total, per, parts = loss.multiscale_unsupervised_torch(obj, torch.cat([prv, nxt], dim=3).double(), [x], [occ])
    total.backward()
    assert int(parts["counts"][0]) == count > 100 and 0.9 < share < 1.0
    assert abs(float(parts["photometric"][0] - photo)) <= 1e-12 * float(photo)
    assert abs(float(parts["smoothness"][0] - smooth)) <= 1e-12 * float(smooth)
    top = float(x.grad.abs().max())
    rest = x.grad.clone()
    for r, g in zip(regs, grads):
        n, y0, y1, x0, x1 = r[1:]
        assert float((x.grad[n:n + 1, y0:y1, x0:x1] - g).abs().max()) <= 1e-12 * top and g.any()
        rest[n, y0:y1, x0:x1] = 0
    assert not rest.any()
    ref32 = lo.unsup_window_ref(kind, crops, key, torch.float32)
    bounds = lo.unsup_bounds((photo, smooth, count, grads, share), ref32)
    assert ref32[2] == count and bounds["photo"] <= 1e-4 * float(photo) and bounds["grad"] <= 1e-3 * top
    alt = crops[:1] + [lo.unsup_cut(prv, nxt, flow, occ, regs[1], frames_at=(1, 0, regs[1][3] - regs[1][2], 0,
                                                                              regs[1][5] - regs[1][4]))] + crops[2:]
    assert abs(float(lo.unsup_window_ref(kind, alt, key, torch.float64)[0] - photo)) >= 100 * bounds["photo"]


# ---- the input pipelines ---------------------------------------------------------------------------------------------------
def test_augment_case_crosses_what_it_claims():
    """3 x 26833 x 26839 source pixels: the pixel index passes 2^29, 2^30 and 2^31 in samples 0, 1 and 2 -- the mask's
    byte index, the flow's float2 index (bytes 2^32 .. 2^34) and the frames' 6-byte pixel index; the validator's rule
    admits it; each sample's window reads source rows on both sides of its boundary pixel, under another flip pair, at
    coordinates that fp32 holds exactly; the plan fits."""
    key = lo.CASES["augment"]
    B, H, W = key
    assert B == 3 and H % 2 and W % 2 and H != W
    assert lo.crossed(B * H * W) == [P29, P30, P31] and [lo.locate(b, H, W, 1)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    text = open(os.path.join(CSRC, "augment.hip")).read()
    body = re.search(r"bool augment_shape_ok\(.*?\{(.*?)\n\}", text, re.S).group(1)
    assert body.count("(int64_t)H * W <= lim") == 1 and "0x7fffffff" in body and H * W <= 0x7fffffff
    assert lo.AUG_OUT[0] * lo.AUG_OUT[1] <= 0x7fffffff // 6
    places = lo.augment_placement(key)
    assert sorted((p["ip"][4], p["ip"][5]) for p in places) == [(0, 1), (1, 0), (1, 1)]
    for n, p in enumerate(places):
        m, y, x = p["pixel"]
        _, r0, r1, c0, c1 = p["src"]
        rh, rw, oy, ox, ud, lr = p["ip"]
        assert m == n and (m * H + y) * W + x == lo.BOUNDARIES[n]
        assert r0 + 8 < y < r1 - 8 and c0 + 8 < x < c1 - 8 and r1 - r0 <= 40 and c1 - c0 <= 40
        assert (rh, rw) == (2 * H, 2 * W) and 0 <= oy <= rh - lo.AUG_OUT[0] and 0 <= ox <= rw - lo.AUG_OUT[1]
        ch, cw, coy, cox = p["crop_ip"][:4]
        assert (ch, cw) == (2 * (r1 - r0), 2 * (c1 - c0)) and 0 <= coy <= ch - lo.AUG_OUT[0] and 0 <= cox <= cw - lo.AUG_OUT[1]
        # the fp32 source coordinates of the window are exact, and the crop's differ from them by an integer
        for o, co, size, csize, extent in ((oy, coy, H, r1 - r0, lo.AUG_OUT[0]), (ox, cox, W, c1 - c0, lo.AUG_OUT[1])):
            i = np.arange(extent)
            s32 = (np.float32(o + i) + np.float32(0.5)) * (np.float32(size) / np.float32(2 * size)) - np.float32(0.5)
            c32 = (np.float32(co + i) + np.float32(0.5)) * (np.float32(csize) / np.float32(2 * csize)) - np.float32(0.5)
            s64 = (o + i + 0.5) * 0.5 - 0.5
            assert np.array_equal(s32.astype(np.float64), s64) and len(set((s64 - c32).tolist())) == 1
            assert (s64 - c32)[0] == int((s64 - c32)[0])
    planned = lo.augment_planned_bytes(key)
    assert planned == 15 * B * H * W and planned <= 48 * lo.GIB and 1.10 * planned <= 64 * lo.GIB


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "plain"])
def test_augment_crop_oracle_is_the_oracle_on_a_small_image(colour):
    """augment_window_ref (the restatements on a window's source crop, offsets shifted) against the same restatements on
    the whole source where that is small: 3 x 301 x 311, the windows across a pixel in the middle of each image."""
    from test_augment_cpu import ref_augment
    from test_sparse_augment_cpu import ref_augment_sparse
    key = (3, 301, 311)
    B, H, W = key
    places = lo.augment_placement(key, [(n * H + 140 + 7 * n) * W + 100 + 30 * n for n in range(B)])
    ims, flo, valid = np.zeros((B, H, W, 6), np.uint8), np.zeros((B, H, W, 2), np.float32), np.zeros((B, H, W), np.uint8)
    for n, p in enumerate(places):
        _, r0, r1, c0, c1 = p["src"]
        for t, crop in zip((ims, flo, valid), lo.augment_source(n, p)):
            t[n, r0:r1, c0:c1] = crop[0]
    ip, fp = np.array([p["ip"] for p in places], np.int32), lo.augment_fparams(places)
    w_ims, w_flo = ref_augment(ims, flo, ip, fp, lo.AUG_OUT, colour=colour)
    s_ims, s_flo, s_valid = ref_augment_sparse(ims, flo, valid, ip, fp, lo.AUG_OUT, colour=colour)
    for n, p in enumerate(places):
        _, r0, r1, c0, c1 = p["src"]
        cut = lambda t: t[n:n + 1, r0:r1, c0:c1]
        (r_ims, r_flo), (q_ims, q_flo, q_valid) = lo.augment_window_ref(p, cut(ims), cut(flo), cut(valid), fp[n], colour)
        assert np.abs(r_ims[0] - w_ims[n]).max() <= 1e-12 and np.abs(r_flo[0] - w_flo[n]).max() <= 1e-12
        assert np.abs(q_flo[0] - s_flo[n]).max() <= 1e-12 and np.array_equal(q_valid[0], s_valid[n])
        assert 0.5 < q_valid.mean() < 1.0 and np.abs(r_flo).max() > 8.0 and np.abs(r_ims).max() > 0.25


# ---- occlusion map and inverse flow ------------------------------------------------------------------------------------
def _occlusion_trip():
    """(workgroup cap, workgroup size) of occlusion.hip: grid_for's `want < CAP ? want : CAP` and the launches' dim3(256)."""
    text = open(os.path.join(CSRC, "occlusion.hip")).read()
    body = re.search(r"static unsigned grid_for\(int64_t total\)\s*\{(.*?)\n\}", text, re.S).group(1)
    assert "(total + 255) / 256" in body, body
    caps = re.findall(r"\(1 << (\d+)\)", body)
    assert len(caps) == 2 and caps[0] == caps[1], body
    assert text.count("dim3(grid), dim3(256)") == text.count("hipLaunchKernelGGL") == 5
    assert text.count("__launch_bounds__(256)") == 3
    return 1 << int(caps[0]), 256


def test_occlusion_case_crosses_what_it_claims():
    """3 x 18917 x 18923: `idx * 2` passes 2^29, 2^30 and 2^31 in images 0, 1 and 2, the channels-first plane index too,
    the map's pixel index 2^29 and 2^30; every launch makes at least four grid-stride trips with a partial last one;
    check_flow_args admits it; the windows hold what they are named after inside what is compared; the plan fits."""
    key = lo.CASES["occlusion"]
    B, H, W = key
    P = B * H * W
    assert B == 3 and H % 2 and W % 2 and H != W and P > P30
    assert lo.crossed(2 * P) == [P29, P30, P31] and [lo.locate(b, H, W, 2)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    assert lo.crossed(P) == [P29, P30] and [lo.locate(b, H, W, 1)[0] for b in (P29, P30)] == [1, 2]
    assert [b // (H * W) // 2 for b in lo.BOUNDARIES] == [0, 1, 2] and 2 * P - H * W < P31 < 2 * P   # in the last y plane
    cap, block = _occlusion_trip()
    assert cap * block == lo.OCC_TRIP == 1 << 28
    assert -(-P // lo.OCC_TRIP) >= 4 and 0 < P % lo.OCC_TRIP < lo.OCC_TRIP and P > 3 * lo.OCC_TRIP
    assert H * W > lo.OCC_TRIP                                         # the launch on one image iterates too
    # coordinates plus flows on the 2^-6 grid are exact in fp32: 15 + 6 bits
    assert max(H, W) < 1 << 15 and lo.OCC_F * 64 == 384
    text = open(os.path.join(CSRC, "capi.hip")).read()
    body = re.search(r"static int check_flow_args\(.*?\{(.*?)\n\}", text, re.S).group(1)
    assert "check_common(B, H, W, 2, layout, dtype)" in body
    assert body.count("(int64_t)B * H * W * 2 >= ((int64_t)1 << 40)") == 1 and body.count("QPWC_E_SHAPE") == 1
    assert 2 * P < 1 << 40
    for name in ("qpwc_invert_flow_fwd", "qpwc_occlusion_fwd"):
        assert re.search(name + r"\(.*?\{\s*const int rc = check_flow_args\(", text, re.S), name
    planned = lo.occlusion_planned_bytes(key)
    assert planned == 20 * P + 16 * H * W and planned <= 48 * lo.GIB and 1.10 * planned <= 64 * lo.GIB
    pixels = lo.occ_pixels(key)
    assert [p[0] for p in pixels] == ["nhwc>2^29", "nhwc>2^30", "nhwc>2^31", "trip 4", "nchw>2^29", "nchw>2^30", "nchw>2^31",
                                      "top left", "top right", "bottom left", "bottom right"]
    # the map's boundaries and trip 2 fall on pixels the channels-last flow already names
    at = {p[0]: p[1:] for p in pixels}
    assert at["nhwc>2^29"] == lo.locate(lo.OCC_TRIP, H, W, 1) and at["nhwc>2^30"] == lo.locate(P29, H, W, 1)
    assert at["nhwc>2^31"] == lo.locate(P30, H, W, 1) and at["trip 4"] == lo.locate(3 * lo.OCC_TRIP, H, W, 1)
    assert [at[t][0] for t in ("nhwc>2^29", "nhwc>2^30", "nhwc>2^31", "trip 4", "nchw>2^29", "nchw>2^30", "nchw>2^31")] == \
        [0, 1, 2, 2, 0, 1, 2]
    wins = lo.occ_windows(key)
    m = lo.OCC_MARGIN
    assert m == 2 * lo.OCC_F + 3 and lo.OCC_EDGE_MARGIN >= 9 * lo.OCC_F + 1 + lo.OCC_F + 1 + 1
    for (tag, n, y, x), win in zip(pixels, wins):
        _, wn, y0, y1, x0, x1, (c0, c1, d0, d1) = win
        assert wn == n and (y1 - y0, x1 - x0) == (lo.OCC_WIN, lo.OCC_WIN) and 0 <= y0 and y1 <= H and 0 <= x0 and x1 <= W
        assert c0 <= y - y0 < c1 and d0 <= x - x0 < d1, tag            # the pixel itself is compared
        edge = lo.OCC_EDGE_MARGIN if y0 == 0 or x0 == 0 else m
        assert (c0, d0) == (0 if y0 == 0 else edge, 0 if x0 == 0 else edge), tag
        assert (lo.OCC_WIN - c1, lo.OCC_WIN - d1) == (0 if y1 == H else edge, 0 if x1 == W else edge), tag
        assert (c1 - c0) * (d1 - d0) >= 96 * 96
        if not tag.startswith(("top", "bottom")):
            assert x0 > 0 and y0 > 0 and c0 < y - y0 - 1 and d0 < x - x0 - 1 and y - y0 + 1 < c1   # both sides of the boundary
    # the controls: the element indices are the kernel's, and every boundary has windows that reach it
    for layout, esize, want in (("channels_last", 4, {P30: "nhwc>2^30", P31: "nhwc>2^31"}),
                                ("channels_first", 4, {P30: "nchw>2^30", P31: "nchw>2^31"}),
                                ("channels_first", 2, {P31: "nchw>2^31"})):
        count = {}
        for (tag, n, y, x), win in zip(pixels, wins):
            idx = lo.occ_element_index(key, win, layout)
            assert idx.shape == (lo.OCC_WIN, lo.OCC_WIN, 2) and idx.dtype == np.int64
            yy, xx = y - win[2], x - win[4]
            if layout == "channels_last":
                assert idx[yy, xx, 0] == ((n * H + y) * W + x) * 2 and idx[yy, xx, 1] == idx[yy, xx, 0] + 1
                if tag.startswith("nhwc"):
                    assert idx[yy, xx, 0] == 1 << int(tag[-2:])
            else:
                assert idx[yy, xx, 0] == n * 2 * H * W + y * W + x and idx[yy, xx, 1] == idx[yy, xx, 0] + H * W
                if tag.startswith("nchw"):
                    assert 1 << int(tag[-2:]) in (idx[yy, xx, 0], idx[yy, xx, 1])
            c0, c1, d0, d1 = win[6]
            for mod, mask, wrapped in lo.occ_wrapped(key, win, layout, esize):
                assert mod in (P30, P31) and mod * esize in (1 << 32, 1 << 33) and wrapped.max() < mod
                assert ((idx[mask] - wrapped) % mod == 0).all() and (idx[mask] - wrapped >= mod).all()
                if mask.any(-1)[c0:c1, d0:d1].sum() >= 500:
                    count.setdefault(mod, set()).add(tag)
        assert sorted(count) == sorted(want), (layout, esize, count)
        for mod, tag in want.items():                                  # the window across the boundary, and the corners behind it
            assert tag in count[mod] and {"bottom left", "bottom right"} <= count[mod] and len(count[mod]) >= 4, (layout, mod, count)


def _grid_flow(rng, shape, reach):
    """Flows as the GPU case draws them: multiples of 2^-6 within +-reach, every 5th an integer, every 7th zero."""
    f = rng.integers(-reach * 64, reach * 64 + 1, size=shape).astype(np.float32) / np.float32(64)
    flat = f.reshape(-1, 2)
    flat[::5] = np.round(flat[::5])
    flat[::7] = 0
    return f


def test_occ_restatement_at_the_origin_is_np_ref_on_the_goldens():
    """occ_restatement on a whole image at origin (0, 0) against oracle.np_ref, bit for bit, on the goldens' flows (which
    leave the image and fold), fp32 and with the inverse flow rounded to fp16."""
    from oracle import np_ref
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import cases
    for name in sorted(cases.OCC_CASES):
        fmt = cases.OCC_CASES[name][0]
        flow = cases.make_flow(name)
        nhwc = flow if fmt == "channels_last" else np.ascontiguousarray(np.moveaxis(flow, 1, 3))
        inv, occ = np_ref.invert_flow(nhwc), np_ref.estimate_occlusion_map(nhwc)
        assert inv.dtype == np.float32
        for n in range(nhwc.shape[0]):
            r_inv, r_map = lo.occ_restatement(nhwc[n], (0, 0), nhwc.shape[1:3])
            assert r_inv.tobytes() == inv[n].tobytes() and np.array_equal(r_map, occ[n]), (name, n)
            h_inv, h_map = lo.occ_restatement(nhwc[n], (0, 0), nhwc.shape[1:3], half=True)
            assert np.array_equal(h_inv, inv[n].astype(np.float16).astype(np.float32)) and np.array_equal(h_map, occ[n])


@pytest.mark.parametrize("full,origin", [((18200, 200), (18000, 20)), ((200, 18200), (20, 18000)), ((400, 400), (0, 0)),
                                         ((400, 400), (0, 240)), ((400, 400), (240, 0)), ((400, 400), (240, 240))],
                         ids=["rows near 18000", "columns near 18000", "top left", "top right", "bottom left", "bottom right"])
def test_occ_restatement_on_a_crop_is_np_ref_where_it_is_compared(full, origin):
    """A window of OCC_WIN x OCC_WIN cut from an image small enough for oracle.np_ref, at coordinates near 18000 in one
    axis (`(float)y + inv.y` rounds to 2^-9 there) and in the four corners: what occ_windows() would compare of it equals
    np_ref on the whole image, so the margins are enough; the whole window does not (the margins are needed)."""
    from oracle import np_ref
    H, W = full
    oy, ox = origin
    flow = _grid_flow(np.random.default_rng(5), (1, H, W, 2), lo.OCC_F)
    inv, occ = np_ref.invert_flow(flow)[0], np_ref.estimate_occlusion_map(flow)[0]
    y0, y1, x0, x1 = oy, oy + lo.OCC_WIN, ox, ox + lo.OCC_WIN
    corner = [w for w in lo.occ_windows((1, H, W)) if w[1] == 0 and w[2:6] == (y0, y1, x0, x1)]
    assert len(corner) == (1 if H == W else 0)
    c0, c1, d0, d1 = corner[0][6] if corner else (lo.OCC_MARGIN, lo.OCC_WIN - lo.OCC_MARGIN) * 2
    r_inv, r_map = lo.occ_restatement(flow[0, y0:y1, x0:x1], (y0, x0), full)
    assert r_inv[c0:c1, d0:d1].tobytes() == np.ascontiguousarray(inv[y0:y1, x0:x1][c0:c1, d0:d1]).tobytes()
    assert np.array_equal(r_map[c0:c1, d0:d1], occ[y0:y1, x0:x1][c0:c1, d0:d1])
    assert set(np.unique(r_map[c0:c1, d0:d1])) == {0.0, 1.0}
    # the reach the margins are derived from: F, and 9 F where the first F rows or columns extrapolate
    assert np.abs(inv[lo.OCC_F:, lo.OCC_F:]).max() <= lo.OCC_F * (1 + 1e-6) and np.abs(inv).max() <= 9 * lo.OCC_F * (1 + 1e-6)
    assert not np.array_equal(r_map, occ[y0:y1, x0:x1])


# ---- the interpolator's input pipeline ---------------------------------------------------------------------------------
def test_triplet_case_crosses_what_it_claims():
    """3 x 28528 x 28534 uint8 frames -> 14264 x 14267: the source pixel index passes 2^29, 2^30 and 2^31 in samples 0, 1
    and 2, its byte index 2^31 and 2^32; out_pair passes 2^31 elements and out_mid 2^30; the ratio is exactly 2 and the
    fp32 source coordinates are exact; the shape rule admits it and gives the <vec4> form; every window holds what it is
    named after and reads source pixels inside its sample; enough windows lie behind the byte boundaries; the plan fits."""
    key = lo.CASES["triplet"]
    B, H, W = key
    h, w = H // 2, W // 2
    assert B == 3 and H % 2 == 0 and W % 2 == 0 and H != W and 2 ** 29.6 < H * W < 1 << 30
    assert lo.crossed(B * H * W) == [P29, P30, P31] and [lo.locate(b, H, W, 1)[0] for b in lo.BOUNDARIES] == [0, 1, 2]
    assert 3 * B * H * W > 1 << 32 and 3 * H * W > 1 << 31                           # bytes of a frame, of a sample
    assert lo.crossed(B * h * w * 6) == [P29, P30, P31] and lo.crossed(B * h * w * 3) == [P29, P30]
    assert lo.crossed(h * w * 6) == [P29, P30] and lo.crossed(h * w * 3) == [P29]     # one sample stays under 2^31
    assert (h * w) % 4 == 0                                                           # tri_vec: the <vec4> form
    text = open(os.path.join(CSRC, "triplet.hip")).read()
    assert "((int64_t)h * w) % 4 == 0 && (uintptr_t)out_pair % 16 == 0 && (uintptr_t)out_mid % 16 == 0" in text
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert "static int triplet_check_shapes(int B, int H, int W, int h, int w) { return augment_check_shapes(B, H, W, h, w); }" in capi
    body = re.search(r"bool augment_shape_ok\(.*?\{(.*?)\n\}", open(os.path.join(CSRC, "augment.hip")).read(), re.S).group(1)
    assert "(int64_t)H * W <= lim && (int64_t)h * w <= lim / 6 && (int64_t)B * aug_nblk(h, w) <= lim" in body and "0x7fffffff" in body
    assert H * W <= 0x7fffffff and h * w <= 0x7fffffff // 6 and B * -(-h * w // 256) <= 0x7fffffff
    for size, out in ((H, h), (W, w)):
        i = np.arange(out)
        s32 = (i.astype(np.float32) + np.float32(0.5)) * (np.float32(size) / np.float32(out)) - np.float32(0.5)
        assert np.array_equal(s32.astype(np.float64), 2.0 * i + 0.5)                 # lo = 2 i, hi = 2 i + 1, t = 1/2
    assert h * w <= 0xFFFFFFFF                                                        # the noise counter
    planned = lo.triplet_planned_bytes(key)
    assert planned == 18 * B * H * W + 9 * H * W and planned <= 48 * lo.GIB and 1.10 * planned <= 64 * lo.GIB
    controls = 0
    for layout in ("channels_last", "channels_first"):
        pixels, wins = lo.triplet_output_pixels(key, layout), lo.triplet_windows(key, layout)
        assert [p[0] for p in pixels] == ["src>2^29", "src>2^30", "src>2^31", "pair>2^29", "pair>2^30", "pair>2^31",
                                          "mid>2^29", "mid>2^30", "last"]
        assert [p[1] for p in pixels[:3]] == [0, 1, 2] and pixels[-1][1:] == (B - 1, h - 1, w - 1)
        for (tag, n, y, x), (_, wn, oy0, ox0, r0, c0) in zip(pixels, wins):
            ud, lr = lo.TRI_FLIPS[n]
            assert wn == n and 0 <= oy0 <= y < oy0 + lo.TRI_WIN <= h and 0 <= ox0 <= x < ox0 + lo.TRI_WIN <= w
            assert 0 <= r0 and r0 + 2 * lo.TRI_WIN <= H and 0 <= c0 and c0 + 2 * lo.TRI_WIN <= W and r0 % 2 == 0 and c0 % 2 == 0
            # the source rows and columns of the output pixel (y, x) lie in the crop
            sy, sx = h - 1 - y if ud else y, w - 1 - x if lr else x
            assert r0 <= 2 * sy and 2 * sy + 1 < r0 + 2 * lo.TRI_WIN and c0 <= 2 * sx and 2 * sx + 1 < c0 + 2 * lo.TRI_WIN
            b = int(tag[-2:]) if tag != "last" else None
            if tag.startswith("src"):                                                  # ... the boundary source pixel among them
                m, Y, X = lo.locate(1 << b, H, W, 1)
                assert m == n and (Y // 2, X // 2) == (sy, sx) and (n * H + Y) * W + X == 1 << b
                assert 8 < y - oy0 < lo.TRI_WIN - 8 or oy0 in (0, h - lo.TRI_WIN)
            elif tag != "last":
                C = 6 if tag.startswith("pair") else 3
                first = ((n * h + y) * w + x) * C if layout == "channels_last" else (n * C * h + y) * w + x
                assert (first <= 1 << b < first + C) if layout == "channels_last" else ((1 << b) - first) % (h * w) == 0
            c = lo.triplet_counters(key, (tag, n, oy0, ox0, r0, c0))
            assert c.shape == (lo.TRI_WIN ** 2,) and c[0] == (r0 // 2) * w + c0 // 2 and c[-1] == (r0 // 2 + lo.TRI_WIN - 1) * w + c0 // 2 + lo.TRI_WIN - 1
            idx = lo.triplet_source_bytes(key, (tag, n, oy0, ox0, r0, c0))
            assert idx[0, 0, 0] == ((n * H + r0) * W + c0) * 3 and idx[1, 2, 1] == ((n * H + r0 + 1) * W + c0 + 2) * 3 + 1
            controls += sum(bool((idx >= mod).any()) for mod in (1 << 31, 1 << 32))
        assert {t[1] for t in wins} == {0, 1, 2}
    assert controls >= 12, controls


def test_triplet_window_oracle_is_the_oracle_on_a_small_image():
    """triplet_window_ref (ref_triplet on a window's source crop with the noise of the whole output's counters) against
    ref_triplet on the whole, where that is small: 3 x 96 x 104 -> 48 x 52 under the case's flips; and the noise of the
    window's own counters is another one."""
    from test_triplet_cpu import _params, ref_noise, ref_noise_at, ref_triplet
    key = (3, 96, 104)
    B, H, W = key
    h, w = H // 2, W // 2
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) for _ in range(3)]
    ip, fp = _params(B, 78)
    ip[:, 0:2] = lo.TRI_FLIPS
    pair, mid = ref_triplet(*frames, ip, fp, (h, w))
    wins = lo.triplet_windows(key, "channels_last", [("w%d" % n, n, 20 + 3 * n, 9 + 14 * n) for n in range(B)] + [("last", 2, h - 1, w - 1)])
    assert [t[2:4] for t in wins] == [(4, 0), (7, 7), (10, 20), (h - lo.TRI_WIN, w - lo.TRI_WIN)]
    for win in wins:
        _, n, oy0, ox0, r0, c0 = win
        crops = [f[n:n + 1, r0:r0 + 2 * lo.TRI_WIN, c0:c0 + 2 * lo.TRI_WIN] for f in frames]
        r_pair, r_mid = lo.triplet_window_ref(key, win, crops, ip[n], fp[n])
        assert np.abs(r_pair - pair[n, oy0:oy0 + lo.TRI_WIN, ox0:ox0 + lo.TRI_WIN]).max() <= 1e-12
        assert np.abs(r_mid - mid[n, oy0:oy0 + lo.TRI_WIN, ox0:ox0 + lo.TRI_WIN]).max() <= 1e-12
        own = ref_triplet(*crops, ip[n:n + 1], fp[n:n + 1], (lo.TRI_WIN, lo.TRI_WIN))[1][0]
        assert np.abs(own - r_mid).max() > 100 * 1e-4
    # ref_noise_at is ref_noise read at its counters, for one row of counters and for one a sample
    z = ref_noise(ip[:, 2:4], h, w).reshape(B, h * w, 3)
    at = rng.integers(0, h * w, (B, 40))
    assert np.array_equal(ref_noise_at(ip[:, 2:4], at[0]), z[:, at[0]])
    assert np.array_equal(ref_noise_at(ip[:, 2:4], at), np.stack([z[b, at[b]] for b in range(B)]))


# ---- the update step --------------------------------------------------------------------------------------------------
def test_optim_case_crosses_what_it_claims(hip_lib):
    """18,683,000 rows of 115 floats: the element offsets pass 2^29, 2^30 and 2^31 inside a row each, by more than 2^20;
    the unit count is admitted and takes the grid-stride form; five slices of whole rows stay under 2^29 elements; the
    sampled rows hold the boundary rows, the first and the last; the plan fits."""
    key = lo.CASES["optim"]
    rows, cols = key
    n = rows * cols
    assert cols == 115 and n > P31 + (1 << 20) and lo.crossed(n) == [P29, P30, P31]
    assert all(b % cols for b in lo.BOUNDARIES)                                       # each boundary lies inside a row
    assert sorted({(4 * cols * r) % 16 for r in range(8)}) == [0, 4, 8, 12]           # the four phases of a row's start
    text = open(os.path.join(CSRC, "optim.hip")).read()
    waves, cap = int(re.search(r"kOptThreads = (\d+)", text).group(1)) // 64, int(re.search(r"kOptMaxBlocks = (\d+)", text).group(1))
    assert "int64_t agc_adam_max_units() { return 0x7fffffff; }" in text and 1 <= rows <= 0x7fffffff
    assert rows > 1000 * waves * cap and rows % (waves * cap)                          # thousands of trips a wave, the last uneven
    assert hip_lib.qpwc_agc_adam_step_kernel(rows) == b"agc_adam_kernel<grid-stride>"
    assert hip_lib.qpwc_agc_adam_step_kernel(waves * cap) == b"agc_adam_kernel<one unit per wave>"
    R = lo.OPT_SLICE_ROWS
    assert R * cols < P29 <= (R + 1) * cols and -(-rows // R) == 5 and 0 < rows - 4 * R < R
    sample = lo.optim_sample_rows(rows, cols)
    assert sample[:5] == [P29 // cols, P30 // cols, P31 // cols, 0, rows - 1] and len(set(sample)) == len(sample) >= 35
    for b, r in zip(lo.BOUNDARIES, sample):
        assert r * cols < b < (r + 1) * cols
    assert sum(r * cols >= P31 for r in sample) >= 1 and (P31 // cols + 1) * cols - P31 >= 0
    planned = lo.optim_planned_bytes(key)
    assert planned == 20 * n + 48 * rows and planned <= 48 * lo.GIB and 1.10 * planned <= 64 * lo.GIB


def test_optim_tables_tile_the_tensor_and_satisfy_the_validator():
    """optim_tables on a small parameter: both unit tables name every row once, the sliced launch's offsets are counted
    from its slice and address the same elements, and the tables are what qpwc_agc_adam_step's validator asks for (dense
    int64: 8-byte aligned, 32 bytes a tensor and 24 a unit, separate allocations)."""
    rows, cols, R = 1003, 115, 250
    base = [1 << 20, 1 << 24, 1 << 28, 1 << 32]
    (tw, uw), (ts, us) = lo.optim_tables(base, rows, cols, R, "cpu")
    for t in (tw, uw, ts, us):
        assert t.dtype == torch.int64 and t.is_contiguous() and t.data_ptr() % 8 == 0
    assert tuple(tw.shape) == (1, 4) and tuple(uw.shape) == tuple(us.shape) == (rows, 3) and tuple(ts.shape) == (5, 4)
    assert tw[0].tolist() == base and uw[:, 0].eq(0).all() and uw[:, 1].tolist() == [r * cols for r in range(rows)]
    assert uw[:, 2].eq(cols).all() and us[:, 2].eq(cols).all() and us[:, 0].max() == 4 and us[:, 1].max() == (R - 1) * cols
    for k in range(4):                                                                 # the same address for every row
        whole = tw[uw[:, 0], k] + 4 * uw[:, 1]
        sliced = ts[us[:, 0], k] + 4 * us[:, 1]
        assert torch.equal(whole, sliced)
    text = open(os.path.join(CSRC, "capi.hip")).read()
    assert "{tensors, (size_t)n_tensors * 32, 8, \"tensors\"}, {units, (size_t)n_units * 24, 8, \"units\"}" in text


def test_optim_rows_stay_within_the_bounds_in_the_fp32_composition():
    """optim.step_torch in fp32 on rows drawn and scaled as the GPU case draws them (optim_draw, optim_scale_rows) against
    the float64 oracle, at t = 1 with clipping on: the bounds of tests/test_optim_cpu.py, 4 x what the composition
    measured on that module's cases, hold on these rows too, so the GPU case uses them unchanged.
    Measured here on 4096 rows: p abs 1.5e-08, m rel 7.1e-08, v rel 5.9e-08 (bounds 1.56e-07, 1.88e-06, 1.16e-06)."""
    from qpwcnet_amd import optim
    from test_optim_cpu import AGC_EPS, BETA_1, BETA_2, CLIP, EPSILON, LR, M_BOUND, P_BOUND, V_BOUND, oracle_alpha
    rows, cols = 4096, 115
    arr = {k: torch.empty(rows * cols) for k in "pgmv"}
    for k in "pgmv":
        lo.optim_draw(arr[k], k)
    ratio = lo.optim_scale_rows(arr["p"], arr["g"], cols, CLIP, AGC_EPS)
    assert float((ratio - 1.0).abs().min()) > 1e-3 and float(torch.minimum((ratio - 0.25).abs(), (ratio - 4.0).abs()).max()) < 1e-4
    assert float(arr["v"].min()) >= 0.0 and 0.09 < float(arr["p"].std()) < 0.11
    before = [arr[k].view(rows, cols).numpy().copy() for k in "pgmv"]
    want = lo.optim_rows_oracle(*before)
    # the oracle clipped every odd row by 16 and left the even rows alone
    g64 = before[1].astype(np.float64)
    m_plain = before[2] + (g64 - before[2]) * (1.0 - float(np.float32(BETA_1)))
    assert np.abs(want[1][0::2] - m_plain[0::2]).max() < 1e-15 and np.abs(want[1][1::2] - m_plain[1::2]).max() > 1e-6
    p = arr["p"].view(rows, cols, 1, 1)
    optim.step_torch([("rows.pointwise.weight", p)], [arr["g"].view(rows, cols, 1, 1)], [arr["m"].view(rows, cols, 1, 1)],
                     [arr["v"].view(rows, cols, 1, 1)], float(np.float32(oracle_alpha(LR, 1))), BETA_1, BETA_2, EPSILON, CLIP, AGC_EPS)
    err = lo.optim_row_errors([arr[k].view(rows, cols).numpy() for k in "pmv"], want)
    print("step_torch on {} rows: p abs {:.3g} (bound {:.3g}), m rel {:.3g} ({:.3g}), v rel {:.3g} ({:.3g})".format(
        rows, err[0], P_BOUND, err[1], M_BOUND, err[2], V_BOUND))
    assert err[0] <= P_BOUND and err[1] <= M_BOUND and err[2] <= V_BOUND, err
    # the control: other rows' data gives another answer, by far more than a bound
    other = lo.optim_rows_oracle(*[np.roll(b, 1, axis=0) for b in before])
    assert float(np.abs(other[0] - want[0]).max(1).min()) / P_BOUND > 100.0

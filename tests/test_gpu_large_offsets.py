"""GPU suite of the training kernels where element offsets pass 2^29, 2^30 and 2^31 (byte offsets 2^31 and 2^32, and the
`int` index limit): one entry of CASES per kernel family, each B = 3 with ragged H x W so that the three boundaries of
its main operand fall into three different images (tests/test_large_offsets_cpu.py proves that for every entry, and
that the validators admit the shape).  The entries added for the byte-indexed masks differ: the masked losses' tile case
is a square of 32-multiples (the smallest whose pixel count passes 2^31), the flow metrics have B = 5 (each image under
2^29 floats).

No whole-array float64 reference exists at 8 GB per operand.  The oracles are

  (a) bit equality on the device, per image: the kernels accumulate a pixel row independently of the rest of the
      batch (csrc/conv_bwd.hip: "grad_x of an image does not depend on the rest of the batch"), so out[n] and
      grad_x[n] of the big launch must be torch.equal to the same op on x[n:n+1] alone, a launch that stays below
      every boundary and that the small-shape suites hold to float64;
  (b) float64 autograd on the CPU over crops of CROP x CROP output pixels: one around each boundary pixel of every
      per-pixel operand, one on the last pixels of the last image ('SAME' border, partial last pixel block).  The crop
      of x is exactly what the crop's outputs read (zeros where that lies outside the image), grad_out is the dense
      one, and grad_x is compared where every output that reads the x pixel lies inside the crop -- the crop's
      artificial border cannot contribute to what is compared.  Bound: the family's 1e-4 * max(1, max|ref|);
  (c) for the sums over the batch (grad_w, grad_b) a second backward with grad_out zero except WIN x WIN windows at
      the start of image 0, just behind each boundary and in the bottom-right corner of the last image, x still dense
      random: the float64 answer needs the windows' crops only.  Without Mish every product and partial sum is exact
      on these grids (tests/test_gpu_conv_grad.py::test_ragged_without_mish_is_exact; the magnitude precondition is
      asserted) and torch.equal is required; with Mish the family bound.  Negative controls on the device's own data:
      leaving out any one window, or reading a window's x crop at its offset wrapped mod 2^31 / 2^32 bytes, moves
      the answer by at least 100 bounds.

The losses and the EPE are sums over the batch only: the prediction equals the level's ground truth outside planted
windows (the area loss takes the kernel's own gt_out, itself held to float64 on crops; a full-resolution level takes a
copy of the ground truth), so value and grad_pred follow from the windows' crops in float64.  Their magnitudes are
1e-6 and below, so their bound is relative (LOSS_REL, derived at its definition), not the 1e-4 of the layers.

The masked losses and the flow metrics ("masked_loss", "masked_loss_pixel", "flow_quality" of CASES) index a uint8 mask by pixel, so a byte offset
is an index: their shapes put 2^31 (masked losses, tile path) and 2^30 (the others) pixels into the batch, and the tile
path's ground truth reaches 2^32 elements (BOUNDARIES_32).  Validity is zero (masked losses) or the prediction is the
truth (flow metrics) except in planted windows, so the float64 answer needs the windows' crops and the masks' counts
only; see the comments at their sections.

The label-free losses and the input pipelines ("unsup_loss", "augment") have a trivial background instead -- one
colour, zero flow, everything occluded; zero sources with a zero mask -- so that their float64 answers need crops only;
see the comments at their sections.  On paper, for these two: the casts in the sources are redundant one by one --
`pix = (b * h + y) * (int64_t)w + x` of unsup_loss_fwd_kernel has an int64_t `b`, and the validator keeps B * h * w
itself below 2^31, so dropping that cast changes no value; `p00 = img + (int64_t)y0 * W + x0` of aug_pixel_pass has an
int64_t `img` and a y0 * W below 2^31 -- and what a 32-bit offset takes is a narrower type.  `int64_t b` to `int b` in
unsup_ld_rgb makes `((b * h + y) * w + x) * 3` wrap at element 2^31, pixel (15213, 5955) of image 2: from there on the
frames are read 2^32 elements lower, before the tensor.  The windows ">2^31" (rows 15214 on) and "last" lie there; the
value and the gradient need their texture, and the control shows that other frames in one window move the value by
185 bounds or more.  `const int64_t np` to `const int np` makes `3 * np` .. `6 * np` wrap: planes 3 .. 6 of every pixel
(d gw / d q, the edge weights) are stored and gathered 2^32 floats lower, plane 6 on top of plane 0 and the others
before the workspace, over whatever lies there; the gradient of every window and the zeros around them go.  `const
int64_t p00` to `const int p00` makes sample 2 read the source rows behind its boundary pixel 2^32 pixels lower; the
control reads them 2^31 lower, finds the zeros that lie there, and every output moves by thousands of bounds.  `int64_t
pix` to `int pix` in aug_load_pixel wraps `pix * 6` from pixel 357,913,942 on: all three windows lie beyond.

The last three entries of CASES -- the occlusion map and inverse flow, the interpolator's input pipeline, the update
step -- are held to equality or to their family's float64 oracle on windows and rows of fully random data (the
occlusion kernels are bit-exact, so their windows need a restatement in the full image's coordinates), and each has the
control that the data a narrow index would read gives another answer; the comments at their sections say what a 32-bit
index, a loop without its stride and a truncated unit offset would break, on paper: those mutants write outside their
tensors and are not run.

Where a family departs from this: grad_img of the warp is a scatter of float atomics, so it is held to (b) only; the
cost-volume backward is fed a random saved output (it reads it for the LeakyReLU mask only) and gives its two
gradients in two launches; the SeparableConv2D case calls the backward op without running the fused forward; the
cost volume, the warp, the image upsampling and the pyramid have no sums over the batch, hence no (c); the pyramid
needs H and W to be multiples of 32, so its sizes are unequal but not odd.  Not here: the flow
head's training path, whose validator caps it at 2^24 pixels where its operands stay under 2^29 elements (DESIGN.md
4.17; a run at exactly the cap was considered: it would cross no boundary, and the cap's reason, fp32 pixel counts, is
the small-shape suite's subject).

What catches a 32-bit offset, on paper: with the `(int64_t)` of the stage-X store of conv_bwd_gemm_kernel
(`dst[(((int64_t)img * g.H + row_y) * g.W + row_x) * g.cin + col]`) changed to `int`, the element index of every pixel
behind 2^31 elements (image 2 from row 6621 on) wraps to a negative offset: grad_x[2] of the big launch keeps whatever
the allocation held there, while the launch of image 2 alone (offsets < 2^30) writes it, so (a) fails for image 2, and
(b) fails on the "x>2^31" crop and on the last-corner crop.  The same change in a load of stage W would read x at a
wrapped place: the "wrapped" control of (c) shows that this moves grad_w by more than 100 bounds.

Everything full-size is drawn on the device from a seeded generator on the grids of the grad suites (multiples of 1/16
for x and grad_out, 1/8 for weights and bias); only crops leave the device.  Device memory: the peak of each test is
asserted within planned bytes + 10 % (a hidden full-size copy in ops.py would show), planned being the larger of the
two phases big launch (operands, outputs, workspace) and one-image repeats (the workspace is released by then), and
the peak being counted over what earlier tests of the session still hold.

Measured on an MI355X (peak of torch.cuda.max_memory_allocated, wall time of the test body):
  case                      peak GiB (planned)   seconds      largest |error| against float64 (bound 1e-4 max(1, max|ref|))
  conv3x3_same_s1 mish      40.16 (40.16)        0.2 - 2.4    out 9.5e-7, grad_x 7.2e-6, grad_w 3.8e-6, grad_b 4.9e-6
  conv3x3_same_s1 linear    40.16 (40.16)        0.2 - 1.5    0 (exact), grad_w / grad_b torch.equal
  conv3x3_same_s2 mish      29.46 (29.45)        0.2 - 1.3    out 1.9e-6, grad_x 5.8e-6, grad_w 5.3e-6, grad_b 3.7e-6
  conv3x3_same_s2 linear    29.46 (29.45)        0.1 - 1.0    0 (exact)
  upconv4x4s2               40.16 (40.16)        0.5 - 1.4    out 3.3e-7, grad_x 1.1e-6, grad_w 3.1e-6, grad_b 4.1e-6; mish = 0 exact
  sepconv3x3 flags 11       40.08 (40.08)        0.2 - 3.0    grad_x 1.7e-6, grad_dw 1.2e-5, grad_pw 1.4e-5, grad_bias 4.0e-6
  sepconv3x3 flags 00       40.08 (40.08)        0.2          0 (exact)
  cost_volume_bwd           47.77 (47.10)        0.7 - 2.9    grad_prv 3.9e-8, grad_nxt 4.3e-8
  warp_bwd clamp + fp16     24.70 (24.68)        0.1 - 0.9    0 (exact on the 2^-6 flow grid)
  warp_bwd tfwarp           24.70 (24.68)        0.1          0
  image_head                20.29 (19.62)        0.03 - 1.3   0 (exact)
  upsample2x_image          24.03 (23.36)        0.03 - 2.9   0 (exact)
  avgpool_pyramid            8.04 (8.04)         0.01         0 (exact)
  loss tile path            14.01 (16.02)        0.4          relative: loss 5.8e-8, grad_pred 9.0e-8 (bound 1e-5)
  loss pixel paths, EPE     32.05 (32.05)        0.1          relative: losses 4.3e-8, grad_pred 1.3e-7, EPE 7.7e-10 (bound 1e-5)
  masked_loss tile path     34.14 (34.64)        0.6          relative: losses 5.0e-9, grad_pred 1.3e-7 (bound 1e-5); gt_out 1.7e-8 of the level's largest (bound 1e-6)
  masked_loss pixel paths   33.06 (34.06)        0.1          relative: losses 1.6e-8, grad_pred 1.2e-7 (bound 1e-5); gt_out exact
  flow_quality              22.01 (22.01)        2.1          relative: means 2.7e-7 (bound 1e-5); 1.7e-7 px, 3.5e-13 degrees, count ratios 0.50 ulp
  unsup_loss (census)       46.32 (46.32)        1.5          relative: photometric 4.7e-9, smoothness 1.3e-8 (bound 1e-5); grad_flow 6.4e-9 of a largest 2.4e-3 (bound 2.6e-8)
  augment, dense + sparse   30.18 (30.18)        1.9          frames 4.5e-7, flow 3.8e-6 px, sparse flow 7.6e-6 px (bound 1e-4); masks equal
  occlusion, inverse flow   26.01 (25.34)        0.4 - 1.3    0 (equality): 33 windows, 3 x 3 one-image launches; 30 controls: the inverse flow differs in 0.86 - 1.00, the map in 0.46 - 0.49 of the pixels behind the boundary
  triplet                   48.90 (47.76)        0.1 - 0.9       pair 2.3e-7, middle frame 2.0e-7 (bound 1e-4); 16 controls 10151 - 12367 bounds
  agc_adam step             42.86 (40.85)        2.1 - 4.0    37 rows: p 1.5e-8 (bound 1.56e-7), m 5.3e-8 (1.88e-6), v 4.9e-8 (1.16e-6); p, m, v torch.equal; control 2.6e6 bounds
unsup_loss: 10 windows, count 1871; the windows' share of the smoothness sum is 0.888 at smooth_eps = 2^-20; the bounds,
4 x the float32 chain on the same crops, came out at their floor of 1e-5 for both values and at 2.6e-8 (4 x 6.5e-9, of
a largest gradient of 2.4e-3) for grad_flow.
The whole module: 23 tests, 3 - 16 s (the seconds are test bodies in different runs).  The peaks above the plan are the boolean of torch.equal on one image (0.67 GiB);
ops.py itself allocates what is planned and nothing else.  The negative controls moved the sums by 1300 - 20500 bounds;
those of the masked losses moved the loss or grad_pred by 190 - 200000 bounds, those of the flow metrics an image's epe by
7100 - 100000; those of the label-free loss moved the photometric value by 185 - 10500 bounds, those of the input pipelines
every output by 6300 - 11500.
"""
import gc
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref
from qpwcnet_amd import metrics, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_quality_cpu import (COUNT_FIELDS, EPE_FIELDS, away_from_thresholds, check, make_flows,  # noqa: E402
                                   ref_scores, ref_sums)
from test_gpu_conv_grad import same_pad  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUNDARIES = (1 << 29, 1 << 30, 1 << 31)      # fp32 elements: byte offsets 2^31 and 2^32, the int index limit
CROP, WIN = 24, 16
GIB = 1 << 30
# family -> (B, H, W, ...) of the kernel family's own key
CASES = {
    "conv3x3_same_s1": (3, 6701, 6703, 16, 16, 1),       # (B, H, W, C_in, C_out, stride)
    "conv3x3_same_s2": (3, 6701, 6703, 16, 32, 2),
    "upconv4x4s2": (3, 3349, 3353, 64, 16),              # (B, H, W, C, F)
    "sepconv3x3": (3, 4733, 4735, 32, 16, 1),            # (B, H, W, C, F, 1): the 3x3 'same' stride-1 geometry
    "backward": (3, 3349, 3353, 64),                     # (B, H, W, C) of cost_volume_bwd and warp_bwd
    "image_head": (3, 3349, 3353),                       # (B, H, W) of 64 features: M > 2^25 pixels
    "upsample2x_image": (3, 7727, 7729, 3),              # (B, h, w, C): 2.150 G output floats
    "avgpool_pyramid": (3, 15456, 15488, 3, 5),          # (B, H, W, C, levels): 2.154 G input floats
    "loss": (3, 18912, 18944, 2),                        # (B, H, W, 2) ground truth, H and W multiples of 32: the tile path
    "epe": (3, 18931, 18937, 2),                         # (B, H, W, 2) odd: pixel and bilinear losses, both EPE kernels
    "masked_loss": (3, 26784, 26784, 2),                 # 2.152 G pixels: the mask's byte index passes 2^31, the ground
                                                         # truth's element index 2^32; multiples of 32: the tile path
    "masked_loss_pixel": (3, 18931, 18937, 2),           # the "epe" shape: the masked pixel walks, the scalar backward
    "flow_quality": (5, 14653, 14661, 2),                # 1.074 G pixels (the cap is 2^31 - 1 elements a flow): truth and
                                                         # an fp32 pred pass 2^31 elements, the masks 2^30 bytes
    "unsup_loss": (3, 15489, 15497),                     # (B, h, w) of one level: 0.720 G pixels, the frames 2.160 G floats,
                                                         # the saved planes 5.04 G, the mask 2^29 bytes and more
    "augment": (3, 26833, 26839),                        # (B, H, W) of the source: 2.161 G pixels of 6 bytes, a float2 and a
                                                         # mask byte each
    "occlusion": (3, 18917, 18923),                      # (B, H, W) of a flow: 1.0739 G pixels, 2^28 a stride trip: five
                                                         # trips, the last of 157,349 pixels; 2.148 G flow elements
    "triplet": (3, 28528, 28534),                        # (B, H, W) of a uint8 frame: 2^29.6 < 0.814 G pixels < 2^30 a sample,
                                                         # 7.33 GB a frame; the outputs (H / 2, W / 2): 3.66 G and 1.83 G floats
    "optim": (18683000, 115),                            # (rows, floats a row) of one parameter: 2.1485 G floats, a unit a row
}
BOUNDARIES_32 = BOUNDARIES + (1 << 32,)                  # ... and the unsigned index limit, for operands that reach it


# ---- where the boundaries lie (pure; shared with the CPU companion) ------------------------------------------------
def crossed(n_elems, boundaries=BOUNDARIES):
    """The boundaries that an operand of n_elems floats crosses: its last element lies beyond them."""
    return [b for b in boundaries if n_elems - 1 > b]


def locate(elem, rows, cols, ch):
    """Element offset into a dense (B, rows, cols, ch) tensor -> (image, row, column) of its pixel."""
    p = elem // ch
    return p // (rows * cols), (p // cols) % rows, p % cols


def _span(c, size, n):
    lo = min(max(c - size // 2, 0), n - size)
    return lo, lo + size


def conv_geo(key):
    """The geometry of a convolution key: (B, H, W, C_in, C_out, stride) of the 3x3 'same' layer, or (B, H, W, C, F) of
    the 4x4 stride-2 transposed one (up = True: output pixel o = 2 i - 1 + k, k = 0 .. 3)."""
    if len(key) == 5:
        B, H, W, C, F_ = key
        return dict(B=B, H=H, W=W, ci=C, co=F_, up=True, Ho=2 * H, Wo=2 * W)
    B, H, W, ci, co, s = key
    return dict(B=B, H=H, W=W, ci=ci, co=co, s=s, up=False, Ho=-(-H // s), Wo=-(-W // s), pt=same_pad(H, s)[0],
                pl=same_pad(W, s)[0])


def conv_operands(key):
    """Element counts of the full-size operands of a forward + backward."""
    g = conv_geo(key)
    n_in, n_out = g["B"] * g["H"] * g["W"] * g["ci"], g["B"] * g["Ho"] * g["Wo"] * g["co"]
    return {"x": n_in, "grad_x": n_in, "out": n_out, "grad_out": n_out, "gz": n_out}


def conv_boundary_pixels(key):
    """[(tag, image, output row, output column)]: the output pixel at (or, for x, reading) the pixel that holds each
    boundary of the output-sized operands and of the input-sized ones; one entry per distinct pixel."""
    g = conv_geo(key)
    ops_ = conv_operands(key)
    seen, out = set(), []
    for b in crossed(ops_["out"]):
        n, y, x = locate(b, g["Ho"], g["Wo"], g["co"])
        if (n, y, x) not in seen:
            seen.add((n, y, x))
            out.append(("out>2^%d" % (b.bit_length() - 1), n, y, x))
    for b in crossed(ops_["x"]):
        n, y, x = locate(b, g["H"], g["W"], g["ci"])
        y, x = (2 * y, 2 * x) if g["up"] else (y // g["s"], x // g["s"])
        if (n, y, x) not in seen:
            seen.add((n, y, x))
            out.append(("x>2^%d" % (b.bit_length() - 1), n, y, x))
    return out


def conv_crops(key):
    """[(tag, n, oy0, oy1, ox0, ox1)] in output pixels: a CROP x CROP region around each boundary pixel, one on the
    last pixels of the last image."""
    g = conv_geo(key)
    regs = [(tag, n) + _span(y, CROP, g["Ho"]) + _span(x, CROP, g["Wo"]) for tag, n, y, x in conv_boundary_pixels(key)]
    regs.append(("last", g["B"] - 1, g["Ho"] - CROP, g["Ho"], g["Wo"] - CROP, g["Wo"]))
    return regs


def conv_windows(key):
    """[(tag, n, oy0, oy1, ox0, ox1)]: WIN x WIN windows of grad_out for the batch sums: the start of image 0, the rows
    just behind each boundary pixel, the bottom-right corner of the last image."""
    g = conv_geo(key)
    wins = [("first", 0, 0, WIN, 0, WIN)]
    for tag, n, y, x in conv_boundary_pixels(key):
        d = 4 if g["up"] else 2                           # far enough down that what the window reads of x lies behind it too
        assert y + d + WIN <= g["Ho"], (tag, y)
        wins.append((tag, n, y + d, y + d + WIN) + _span(x, WIN, g["Wo"]))
    wins.append(("last", g["B"] - 1, g["Ho"] - WIN, g["Ho"], g["Wo"] - WIN, g["Wo"]))
    return wins


def conv_x_region(key, reg):
    """What the outputs of a region read: ((iy0, iy1, ix0, ix1) inside the image, (left, right, top, bottom) zeros of
    the 'SAME' window outside it; transposed: the region's place (left, right, top, bottom) in the output of those
    inputs)."""
    g = conv_geo(key)
    _, _, oy0, oy1, ox0, ox1 = reg
    if g["up"]:      # output o reads inputs ceil((o - 2) / 2) .. floor((o + 1) / 2)
        cy0, cy1, cx0, cx1 = max((oy0 - 1) // 2, 0), min(oy1 // 2 + 1, g["H"]), max((ox0 - 1) // 2, 0), min(ox1 // 2 + 1, g["W"])
        return (cy0, cy1, cx0, cx1), (ox0 - 2 * cx0, ox1 - 2 * cx0, oy0 - 2 * cy0, oy1 - 2 * cy0)
    iy0, iy1 = oy0 * g["s"] - g["pt"], (oy1 - 1) * g["s"] + 3 - g["pt"]
    ix0, ix1 = ox0 * g["s"] - g["pl"], (ox1 - 1) * g["s"] + 3 - g["pl"]
    cy0, cy1, cx0, cx1 = max(iy0, 0), min(iy1, g["H"]), max(ix0, 0), min(ix1, g["W"])
    return (cy0, cy1, cx0, cx1), (cx0 - ix0, ix1 - cx1, cy0 - iy0, iy1 - cy1)


def _axis_valid(i0, i1, o0, o1, n_out, s, p):
    """Per input coordinate of [i0, i1): every output of [0, n_out) whose 3-wide window holds it (s = None: that the
    transposed convolution writes from it) lies in [o0, o1)."""
    ok = []
    for i in range(i0, i1):
        if s is None:
            users = range(max(0, 2 * i - 1), min(n_out - 1, 2 * i + 2) + 1)
        else:
            users = range(max(0, (i + p - 2 + s - 1) // s), min(n_out - 1, (i + p) // s) + 1)
        ok.append(all(o0 <= o < o1 for o in users))
    return torch.tensor(ok)


def conv_gx_valid(key, reg):
    """Mask over the x region of a crop: grad_x there depends on outputs of the crop only."""
    g = conv_geo(key)
    (cy0, cy1, cx0, cx1), _ = conv_x_region(key, reg)
    _, _, oy0, oy1, ox0, ox1 = reg
    return _axis_valid(cy0, cy1, oy0, oy1, g["Ho"], g.get("s"), g.get("pt"))[:, None] & \
        _axis_valid(cx0, cx1, ox0, ox1, g["Wo"], g.get("s"), g.get("pl"))[None, :]


def conv_wrapped_regions(key, reg):
    """The x region of a window as a 32-bit byte offset would find it: its first element's byte offset mod 2^31 and
    mod 2^32, where that differs -> [(modulus, (n, iy0, iy1, ix0, ix1))] of the same extent, inside the tensor."""
    g = conv_geo(key)
    (cy0, cy1, cx0, cx1), _ = conv_x_region(key, reg)
    first = ((reg[1] * g["H"] + cy0) * g["W"] + cx0) * g["ci"]
    out = []
    for mod in (1 << 31, 1 << 32):
        e = (first * 4 % mod) // 4
        if e == first:
            continue
        n, y, x = locate(e, g["H"], g["W"], g["ci"])
        y0, x0 = min(y, g["H"] - (cy1 - cy0)), min(x, g["W"] - (cx1 - cx0))
        out.append((mod, (n, y0, y0 + cy1 - cy0, x0, x0 + cx1 - cx0)))
    return out


def conv_planned_bytes(key, ws_floats, ws_floats_one):
    """Planned device memory of a test: the larger of the big launch (x, grad_out, out, grad_x, workspace) and the
    one-image repeats beside the big launch's tensors (out, grad_x and workspace of one image)."""
    n = conv_operands(key)
    B = key[0]
    held = n["x"] + n["grad_out"] + n["out"] + n["grad_x"]
    return 4 * max(held + ws_floats, held + n["out"] // B + n["grad_x"] // B + ws_floats_one)


# ---- the float64 restatement on crops -----------------------------------------------------------------------------
def _tol(ref):
    return 1e-4 * max(1.0, float(ref.abs().max()))


def conv_region_ref(key, xc, pads, w, b, gc, mish):
    """Float64 autograd of the layer on a crop: xc (1, h, w, C_in) as conv_x_region() cut it, gc the crop's grad_out
    -> (out, grad of xc, grad_w, grad_b)."""
    if isinstance(w, (tuple, list)):
        # SeparableConv2D: w = (dw (C,1,3,3), pw (F,C)), mish = (on load, on store); grad_w = grad_dw | grad_pw, flat
        leaves = [t.double().clone().requires_grad_() for t in (xc, w[0], w[1], b)]
        xp = F.pad(leaves[0], (0, 0, pads[0], pads[1], pads[2], pads[3]))        # Mish(0) = 0: the padding stays zero
        d = torch_ref.depthwise3x3([xp], leaves[1], mish[0])[:, 1:-1, 1:-1]
        z = d @ leaves[2].t() + leaves[3]
        out = torch_ref.mish(z) if mish[1] else z
        assert out.shape == gc.shape, (out.shape, gc.shape)
        out.backward(gc.double())
        return out.detach(), leaves[0].grad, torch.cat([leaves[1].grad.flatten(), leaves[2].grad.flatten()]), leaves[3].grad
    leaves = [t.double().clone().requires_grad_() for t in (xc, w, b)]
    if len(key) == 5:
        z = F.conv_transpose2d(leaves[0].permute(0, 3, 1, 2), leaves[1], leaves[2], stride=2, padding=1)
        z = z.permute(0, 2, 3, 1)[:, pads[2]:pads[3], pads[0]:pads[1]]
    else:
        z = F.conv2d(F.pad(leaves[0].permute(0, 3, 1, 2), pads), leaves[1], leaves[2], stride=key[5]).permute(0, 2, 3, 1)
    out = torch_ref.mish(z) if mish else z
    assert out.shape == gc.shape, (out.shape, gc.shape)
    out.backward(gc.double())
    return out.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad


def conv_window_sums(key, crops, w, b, mish):
    """grad_w, grad_b in float64 of a grad_out that is zero outside the windows: crops = [(xc, pads, gc)]."""
    gw, gb = 0.0, 0.0
    for xc, pads, gc in crops:
        _, _, w_, b_ = conv_region_ref(key, xc, pads, w, b, gc, mish)
        gw, gb = gw + w_, gb + b_
    return gw, gb


def conv_controls(key, crops, moved, w, b, mish):
    """The negative controls of the window sums -> [(what, max|change| of grad_w / its bound)]: every window left out
    in turn, and every moved = [(what, window index, x crop read elsewhere)] put in its window's place."""
    ref = conv_window_sums(key, crops, w, b, mish)[0]
    out = []
    for k in range(len(crops)):
        alt = conv_window_sums(key, crops[:k] + crops[k + 1:], w, b, mish)[0]
        out.append(("without window %d" % k, float((alt - ref).abs().max()) / _tol(ref)))
    for what, k, xc in moved:
        alt = conv_window_sums(key, crops[:k] + [(xc,) + crops[k][1:]] + crops[k + 1:], w, b, mish)[0]
        out.append((what, float((alt - ref).abs().max()) / _tol(ref)))
    return out


def exactness_precondition(key, crops, w, b, unit=2 ** 8):
    """sum|terms| * unit < 2^24 for every sum of the linear layer on these grids, 1 / unit the product of the grids'
    steps (2^-8 with 1/8 weights, 2^-10 with 1/64 weights) -> the largest sum."""
    ab = [(xc.abs(), pads, gc.abs()) for xc, pads, gc in crops]
    biggest = 0.0
    linear = (False, False) if isinstance(w, (tuple, list)) else False
    w = tuple(t.abs() for t in w) if isinstance(w, (tuple, list)) else w.abs()
    for xc, pads, gc in ab:
        biggest = max(biggest, max(float(t.max()) for t in conv_region_ref(key, xc, pads, w, b.abs(), gc, linear)[:2]))
    biggest = max(biggest, max(float(t.max()) for t in conv_window_sums(key, ab, w, b.abs(), linear)))
    assert biggest * unit < 2 ** 24, biggest
    return biggest


# ---- the device side -------------------------------------------------------------------------------------------------
def _dgrid(gen, shape, step, lim=1.0):
    n = int(round(lim / step))
    return torch.randint(-n, n + 1, shape, generator=gen, device=DEV, dtype=torch.float32).mul_(step)


def _check(got, ref, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    d = float((got - ref).abs().max())
    print("{}: max|d| = {:.3e}, bound {:.3e}".format(what, d, _tol(ref)))
    assert d <= _tol(ref), "{}: max|d| = {:.3e} > {:.3e}".format(what, d, _tol(ref))
    return d


@pytest.fixture
def arena():
    """Holds a case's device tensors; frees them and the allocator's cache when the test is over."""
    if torch.cuda.get_device_properties(0).total_memory < 96 * GIB:
        pytest.skip("needs a device with at least 96 GiB")
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = {"_base": torch.cuda.memory_allocated()}      # what earlier tests of the session still hold
    yield held
    held.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _cut(t, n, y0, y1, x0, x1):
    return t.detach()[n:n + 1, y0:y1, x0:x1, :].cpu()


@pytest.mark.parametrize("mish", [True, False], ids=["mish", "linear"])
@pytest.mark.parametrize("name", ["conv3x3_same_s1", "conv3x3_same_s2"])
def test_conv3x3_same(name, mish, arena):
    """Conv2D 3x3 'same' forward and stages Z, X, W, R of its backward at x of 2.156 G floats.  The forward runs
    conv3x3_mish_kernel (stride 1 with Mish) or conv_bwd_gemm_kernel mode 0.  Measured: peak 40.16 GiB (stride 1) / 29.46 GiB (stride 2), 0.1 - 2.4 s a case."""
    key = CASES[name]
    B, H, W, ci, co, s = key
    g_ = conv_geo(key)
    Ho, Wo = g_["Ho"], g_["Wo"]
    L = ops._hip.lib()
    planned = conv_planned_bytes(key, L.qpwc_conv3x3_same_bwd_workspace_floats(B, H, W, ci, co, s),
                                 L.qpwc_conv3x3_same_bwd_workspace_floats(1, H, W, ci, co, s))
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(0)
    a = arena
    a["x"] = _dgrid(gen, (B, H, W, ci), 1 / 16).requires_grad_()
    a["w"] = _dgrid(gen, (co, ci, 3, 3), 1 / 8).requires_grad_()
    a["b"] = _dgrid(gen, (co,), 1 / 8).requires_grad_()
    a["g"] = _dgrid(gen, (B, Ho, Wo, co), 1 / 16)
    x, w, b, g = a["x"], a["w"], a["b"], a["g"]
    assert x.numel() > 1 << 31

    # the big launch, through autograd
    a["out"] = ops.conv3x3_same(x, w, b, stride=s, mish=mish)
    a["out"].backward(g)
    out, gx = a["out"].detach(), x.grad
    assert tuple(out.shape) == (B, Ho, Wo, co) and tuple(gx.shape) == (B, H, W, ci)
    assert w.grad is not None and b.grad is not None and bool(torch.isfinite(w.grad).all())
    wd, bd = w.detach(), b.detach()

    # (a) every image alone
    for n in range(B):
        x1 = x.detach()[n:n + 1].requires_grad_()
        assert x1.is_contiguous() and x1.data_ptr() == x.data_ptr() + 4 * n * H * W * ci
        o1 = ops.conv3x3_same(x1, wd, bd, stride=s, mish=mish)
        o1.backward(g[n:n + 1])
        assert torch.equal(o1.detach(), out[n:n + 1]), "out of image %d" % n
        assert torch.equal(x1.grad, gx[n:n + 1]), "grad_x of image %d" % n
        del x1, o1

    # (b) float64 on crops
    wc, bc = wd.cpu(), bd.cpu()
    worst = {"out": 0.0, "grad_x": 0.0}
    for reg in conv_crops(key):
        (cy0, cy1, cx0, cx1), pads = conv_x_region(key, reg)
        tag, n = reg[0], reg[1]
        ro, rx, _, _ = conv_region_ref(key, _cut(x, n, cy0, cy1, cx0, cx1), pads, wc, bc, _cut(g, *reg[1:]), mish)
        worst["out"] = max(worst["out"], _check(_cut(out, *reg[1:]), ro, "%s %s out" % (name, tag)))
        ok = conv_gx_valid(key, reg)
        assert int(ok.sum()) >= (CROP - 2) ** 2, (tag, int(ok.sum()))
        got = _cut(gx, n, cy0, cy1, cx0, cx1)[0][ok]
        worst["grad_x"] = max(worst["grad_x"], _check(got, rx[0][ok], "%s %s grad_x" % (name, tag)))

    # (c) the sums over the batch: grad_out zero outside the windows
    wins = conv_windows(key)
    g.zero_()
    crops, moved = [], []
    for k, reg in enumerate(wins):
        n, oy0, oy1, ox0, ox1 = reg[1:]
        g[n, oy0:oy1, ox0:ox1, :] = _dgrid(gen, (oy1 - oy0, ox1 - ox0, co), 1 / 16)
        (cy0, cy1, cx0, cx1), pads = conv_x_region(key, reg)
        crops.append((_cut(x, n, cy0, cy1, cx0, cx1), pads, _cut(g, *reg[1:])))
        for mod, at in conv_wrapped_regions(key, reg):
            moved.append(("window %d (%s) x read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k, _cut(x, *at)))
    assert 0 < sum(int(torch.count_nonzero(g[n])) for n in range(B)) <= len(wins) * WIN * WIN * co
    _, gt, gb = ops.conv3x3_same_bwd(x.detach(), ops.conv3x3_same_taps(wd), bd, g, s, mish, need=(False, True, True))
    gw = gt[..., :ci].reshape(3, 3, co, ci).permute(2, 3, 0, 1)
    rw, rb = conv_window_sums(key, crops, wc, bc, mish)
    if mish:
        worst["grad_w"], worst["grad_b"] = _check(gw, rw, name + " grad_w"), _check(gb, rb, name + " grad_b")
    else:
        exactness_precondition(key, crops, wc, bc)
        assert torch.equal(gw.double().cpu(), rw), float((gw.double().cpu() - rw).abs().max())
        assert torch.equal(gb.double().cpu(), rb), float((gb.double().cpu() - rb).abs().max())
    controls = conv_controls(key, crops, moved, wc, bc, mish)
    assert len(controls) >= len(wins) + 2, controls
    for what, ratio in controls:
        assert ratio >= 100.0, (what, ratio)
    print("{}: controls move grad_w by {:.0f} .. {:.0f} bounds".format(name, min(r for _, r in controls),
                                                                         max(r for _, r in controls)))

    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("{} mish={}: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}".format(
        name, mish, peak / GIB, planned / GIB, secs, worst))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


def test_upconv4x4s2(arena):
    """Transposed conv 4x4 stride 2: the layer's forward (upconv4x4s2_mish_kernel) and stages Z, X, W, R of its backward
    at x and out of 2.156 G floats each.  The layer always applies Mish; the batch sums are also taken with mish = 0
    through ops.upconv4x4s2_bwd, where they are exact.  Measured: peak 40.16 GiB, 0.5 - 1.4 s."""
    name = "upconv4x4s2"
    key = CASES[name]
    B, H, W, C, F_ = key
    L = ops._hip.lib()
    planned = conv_planned_bytes(key, L.qpwc_upconv4x4s2_bwd_workspace_floats(B, H, W, C, F_),
                                 L.qpwc_upconv4x4s2_bwd_workspace_floats(1, H, W, C, F_))
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(1)
    a = arena
    a["x"] = _dgrid(gen, (B, H, W, C), 1 / 16).requires_grad_()
    a["w"] = _dgrid(gen, (C, F_, 4, 4), 1 / 64, 1 / 8).requires_grad_()
    a["b"] = _dgrid(gen, (F_,), 1 / 8).requires_grad_()
    a["g"] = _dgrid(gen, (B, 2 * H, 2 * W, F_), 1 / 16)
    x, w, b, g = a["x"], a["w"], a["b"], a["g"]
    assert x.numel() > 1 << 31 and g.numel() > 1 << 31

    a["out"] = ops.upconv4x4s2(x, w, b)
    a["out"].backward(g)
    out, gx = a["out"].detach(), x.grad
    assert tuple(out.shape) == (B, 2 * H, 2 * W, F_) and tuple(gx.shape) == (B, H, W, C)
    assert w.grad is not None and b.grad is not None and bool(torch.isfinite(w.grad).all())
    wd, bd = w.detach(), b.detach()

    # (a) every image alone
    for n in range(B):
        x1 = x.detach()[n:n + 1].requires_grad_()
        o1 = ops.upconv4x4s2(x1, wd, bd)
        o1.backward(g[n:n + 1])
        assert torch.equal(o1.detach(), out[n:n + 1]), "out of image %d" % n
        assert torch.equal(x1.grad, gx[n:n + 1]), "grad_x of image %d" % n
        del x1, o1

    # (b) float64 on crops
    wc, bc = wd.cpu(), bd.cpu()
    worst = {"out": 0.0, "grad_x": 0.0}
    for reg in conv_crops(key):
        (cy0, cy1, cx0, cx1), place = conv_x_region(key, reg)
        tag, n = reg[0], reg[1]
        ro, rx, _, _ = conv_region_ref(key, _cut(x, n, cy0, cy1, cx0, cx1), place, wc, bc, _cut(g, *reg[1:]), True)
        worst["out"] = max(worst["out"], _check(_cut(out, *reg[1:]), ro, "%s %s out" % (name, tag)))
        ok = conv_gx_valid(key, reg)
        assert int(ok.sum()) >= (CROP // 2 - 2) ** 2, (tag, int(ok.sum()))
        got = _cut(gx, n, cy0, cy1, cx0, cx1)[0][ok]
        worst["grad_x"] = max(worst["grad_x"], _check(got, rx[0][ok], "%s %s grad_x" % (name, tag)))

    # (c) the sums over the batch: grad_out zero outside the windows
    wins = conv_windows(key)
    g.zero_()
    crops, moved = [], []
    for k, reg in enumerate(wins):
        n, oy0, oy1, ox0, ox1 = reg[1:]
        g[n, oy0:oy1, ox0:ox1, :] = _dgrid(gen, (oy1 - oy0, ox1 - ox0, F_), 1 / 16)
        (cy0, cy1, cx0, cx1), place = conv_x_region(key, reg)
        crops.append((_cut(x, n, cy0, cy1, cx0, cx1), place, _cut(g, *reg[1:])))
        for mod, at in conv_wrapped_regions(key, reg):
            moved.append(("window %d (%s) x read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k, _cut(x, *at)))
    assert 0 < sum(int(torch.count_nonzero(g[n])) for n in range(B)) <= len(wins) * WIN * WIN * F_
    taps = ops.upconv_taps(wd)
    for mish in (True, False):
        _, gt, gb = ops.upconv4x4s2_bwd(x.detach(), taps, bd, g, mish, need=(False, True, True))
        gw = gt.reshape(4, 4, F_, C).permute(3, 2, 0, 1)
        rw, rb = conv_window_sums(key, crops, wc, bc, mish)
        if mish:
            worst["grad_w"], worst["grad_b"] = _check(gw, rw, name + " grad_w"), _check(gb, rb, name + " grad_b")
        else:
            exactness_precondition(key, crops, wc, bc, unit=2 ** 10)
            assert torch.equal(gw.double().cpu(), rw), float((gw.double().cpu() - rw).abs().max())
            assert torch.equal(gb.double().cpu(), rb), float((gb.double().cpu() - rb).abs().max())
        controls = conv_controls(key, crops, moved, wc, bc, mish)
        assert len(controls) >= len(wins) + 2, controls
        for what, ratio in controls:
            assert ratio >= 100.0, (what, ratio)
        print("{} mish={}: controls move grad_w by {:.0f} .. {:.0f} bounds".format(
            name, mish, min(r for _, r in controls), max(r for _, r in controls)))
        del gt, gb, gw

    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("{}: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}".format(name, peak / GIB, planned / GIB, secs, worst))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


def sepconv_operands(key):
    """Element counts of the SeparableConv2D backward's full-size operands and workspace regions (Cpad = C here)."""
    B, H, W, C, F_ = key[:5]
    assert C % 32 == 0
    M = B * H * W
    return {"x": M * C, "grad_x": M * C, "grad_out": M * F_, "d": M * C, "gd": M * C, "gz": M * F_}


def sepconv_planned_bytes(key, ws_floats, ws_floats_one):
    """x, grad_out, grad_x and the workspace of the big launch, or beside them grad_x and workspace of one image."""
    n = sepconv_operands(key)
    held = n["x"] + n["grad_out"] + n["grad_x"]
    return 4 * max(held + ws_floats, held + n["grad_x"] // key[0] + ws_floats_one)


@pytest.mark.parametrize("flags", [(True, True), (False, False)], ids=["11", "00"])
def test_sepconv3x3_bwd(flags, arena):
    """SeparableConv2D backward, stages A to D, one source of 2.151 G floats, through ops.sepconv3x3_bwd (what the
    autograd Function's backward calls; the forward is not run: the backward recomputes d and z).  The workspace
    regions d | gd | gz start at 0, 2.15 G and 4.30 G floats: gd lies behind 2^31 elements, gz behind 2^32.  grad_x is
    held to oracles (a) and (b); grad_dw, grad_pw and grad_bias to (c), exact with both flags off.  Measured: peak 40.08 GiB, 0.2 - 3.0 s."""
    name = "sepconv3x3"
    key = CASES[name]
    B, H, W, C, F_ = key[:5]
    L = ops._hip.lib()
    planned = sepconv_planned_bytes(key, L.qpwc_sepconv3x3_bwd_workspace_floats(B, H, W, C, F_),
                                    L.qpwc_sepconv3x3_bwd_workspace_floats(1, H, W, C, F_))
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(2)
    a = arena
    a["x"] = _dgrid(gen, (B, H, W, C), 1 / 16)
    dw, pw, b = _dgrid(gen, (C, 1, 3, 3), 1 / 8), _dgrid(gen, (F_, C), 1 / 8), _dgrid(gen, (F_,), 1 / 8)
    a["g"] = _dgrid(gen, (B, H, W, F_), 1 / 16)
    x, g = a["x"], a["g"]
    pwp = ops.pad_pointwise(pw)
    assert x.numel() > 1 << 31 and tuple(pwp.shape) == (F_, C)

    gs, gdw, gpw, gb = ops.sepconv3x3_bwd([x], dw, pwp, b, g, *flags)
    a["gx"] = gx = gs[0]
    assert tuple(gx.shape) == (B, H, W, C) and all(bool(torch.isfinite(t).all()) for t in (gdw, gpw, gb))
    del gs, gdw, gpw, gb

    # (a) every image alone
    for n in range(B):
        one = ops.sepconv3x3_bwd([x[n:n + 1]], dw, pwp, b, g[n:n + 1], *flags, need=(True, False, False, False))[0][0]
        assert torch.equal(one, gx[n:n + 1]), "grad_x of image %d" % n
        del one

    # (b) float64 on crops
    wc, bc = (dw.cpu(), pw.cpu()), b.cpu()
    worst = {"grad_x": 0.0}
    for reg in conv_crops(key):
        (cy0, cy1, cx0, cx1), pads = conv_x_region(key, reg)
        tag, n = reg[0], reg[1]
        _, rx, _, _ = conv_region_ref(key, _cut(x, n, cy0, cy1, cx0, cx1), pads, wc, bc, _cut(g, *reg[1:]), flags)
        ok = conv_gx_valid(key, reg)
        assert int(ok.sum()) >= (CROP - 2) ** 2, (tag, int(ok.sum()))
        got = _cut(gx, n, cy0, cy1, cx0, cx1)[0][ok]
        worst["grad_x"] = max(worst["grad_x"], _check(got, rx[0][ok], "%s %s grad_x" % (name, tag)))

    # (c) the sums over the batch: grad_out zero outside the windows
    wins = conv_windows(key)
    g.zero_()
    crops, moved = [], []
    for k, reg in enumerate(wins):
        n, oy0, oy1, ox0, ox1 = reg[1:]
        g[n, oy0:oy1, ox0:ox1, :] = _dgrid(gen, (oy1 - oy0, ox1 - ox0, F_), 1 / 16)
        (cy0, cy1, cx0, cx1), pads = conv_x_region(key, reg)
        crops.append((_cut(x, n, cy0, cy1, cx0, cx1), pads, _cut(g, *reg[1:])))
        for mod, at in conv_wrapped_regions(key, reg):
            moved.append(("window %d (%s) x read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k, _cut(x, *at)))
    assert 0 < sum(int(torch.count_nonzero(g[n])) for n in range(B)) <= len(wins) * WIN * WIN * F_
    _, gdw, gpw, gb = ops.sepconv3x3_bwd([x], dw, pwp, b, g, *flags, need=(False, True, True, True))
    rw, rb = conv_window_sums(key, crops, wc, bc, flags)
    rdw, rpw = rw[:C * 9].reshape(C, 1, 3, 3), rw[C * 9:].reshape(F_, C)
    if flags == (False, False):
        exactness_precondition(key, crops, wc, bc, unit=2 ** 11)
        for got, ref, what in ((gdw.reshape(C, 1, 3, 3), rdw, "grad_dw"), (gpw, rpw, "grad_pw"), (gb, rb, "grad_bias")):
            assert torch.equal(got.double().cpu(), ref), (what, float((got.double().cpu() - ref).abs().max()))
    else:
        worst["grad_dw"] = _check(gdw.reshape(C, 1, 3, 3), rdw, name + " grad_dw")
        worst["grad_pw"] = _check(gpw, rpw, name + " grad_pw")
        worst["grad_bias"] = _check(gb, rb, name + " grad_bias")
    controls = conv_controls(key, crops, moved, wc, bc, flags)
    assert len(controls) >= len(wins) + 2, controls
    for what, ratio in controls:
        assert ratio >= 100.0, (what, ratio)
    print("{} {}: controls move grad_dw | grad_pw by {:.0f} .. {:.0f} bounds".format(
        name, flags, min(r for _, r in controls), max(r for _, r in controls)))

    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("{} {}: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}".format(name, flags, peak / GIB, planned / GIB,
                                                                                 secs, worst))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- cost volume and warp backward: per-pixel outputs only ---------------------------------------------------------
F16_EPS = 2.0 ** -11
SEARCH = 4           # the cost volume's search range: grad_prv / grad_nxt of a pixel depend on pixels within +-4
REACH = 3            # |flow| <= 3 pixels: a warp sample's corners lie within 4 pixels


def pixel_crops(B, H, W, C, margin):
    """[(tag, n, y0, y1, x0, x1, (ey0, ey1, ex0, ex1))]: CROP x CROP pixels around the pixel that holds each boundary of
    a dense (B,H,W,C) operand and on the last pixels of the last image, each with the region `margin` pixels wider
    (clipped to the image) that the reference is computed on."""
    regs = []
    for b in crossed(B * H * W * C):
        n, y, x = locate(b, H, W, C)
        regs.append((">2^%d" % (b.bit_length() - 1), n) + _span(y, CROP, H) + _span(x, CROP, W))
    regs.append(("last", B - 1, H - CROP, H, W - CROP, W))
    return [r + ((max(r[2] - margin, 0), min(r[3] + margin, H), max(r[4] - margin, 0), min(r[5] + margin, W)),)
            for r in regs]


def cost_volume_bwd_ref(prv, nxt, out, g, r=SEARCH, slope=0.1):
    """The formulas of csrc/backward.hip in float64 on a (1,h,w,C) region whose outside counts as zero: g' = g where the
    saved output is > 0, else slope g; grad_prv = (1/C) sum_ij g'[.., ij] nxt[+(i-r, j-r)]; grad_nxt likewise from the
    pixels whose window holds it."""
    prv, nxt, out, g = [t.double() for t in (prv, nxt, out, g)]
    _, h, w, C = prv.shape
    d = 2 * r + 1
    gq = torch.where(out > 0, g, slope * g)
    pad = lambda t: F.pad(t, (0, 0, r, r, r, r))
    nxt_p = pad(nxt)
    gp, gn_p = torch.zeros_like(prv), torch.zeros_like(nxt_p)
    for i in range(d):
        for j in range(d):
            gij = gq[..., i * d + j].unsqueeze(-1)
            gp += gij * nxt_p[:, i:i + h, j:j + w]
            gn_p[:, i:i + h, j:j + w] += gij * prv
    return gp / C, gn_p[:, r:r + h, r:r + w] / C


def warp_bwd_ref(img, flo, g, mode):
    """Float64 autograd of oracle.torch_ref.warp_v2 / tf_warp on a region -> (grad_img, grad_flo)."""
    a, f = img.double().clone().requires_grad_(), flo.double().clone().requires_grad_()
    (torch_ref.warp_v2 if mode == "clamp" else torch_ref.tf_warp)(a, f).backward(g.double())
    return a.grad, f.grad


def _dflow(gen, B, H, W, reach=REACH):
    """Multiples of 2^-6 within +-reach pixels; every 5th pixel an exact integer, every 7th zero."""
    f = torch.randint(-reach * 64, reach * 64 + 1, (B, H, W, 2), generator=gen, device=DEV, dtype=torch.float32).div_(64)
    flat = f.view(-1, 2)
    flat[::5] = flat[::5].round()
    flat[::7] = 0
    return f


def _inner(t, reg):
    """The CROP x CROP part of a tensor cut on the wider region of a pixel_crops() entry."""
    _, _, y0, y1, x0, x1, (ey0, _, ex0, _) = reg
    return t[:, y0 - ey0:y1 - ey0, x0 - ex0:x1 - ex0]


def cost_volume_planned_bytes(key):
    """prv, nxt, the saved output and grad_out, one gradient at a time, and that gradient of one image."""
    B, H, W, C = key
    n_in, n_cv = B * H * W * C, B * H * W * (2 * SEARCH + 1) ** 2
    return 4 * (2 * n_in + 2 * n_cv + n_in + n_in // B)


def warp_planned_bytes(key):
    """img, grad_out, grad_img; the flow and grad_flo; grad_flo of one image."""
    B, H, W, C = key
    return 4 * (3 * B * H * W * C + 2 * B * H * W * 2 + H * W * 2)


def test_cost_volume_bwd(arena):
    """cost_volume_bwd_kernel at prv / nxt of 2.156 G floats and a saved output / grad_out of 2.729 G (81 per pixel),
    through ops.cost_volume_bwd.  The saved output is drawn at random, zeros included: the backward reads it for the
    LeakyReLU mask only, and the forward cost volume at this size is not part of this suite.  grad_prv and grad_nxt are
    asked for in two launches (one pointer NULL each), which keeps the planned memory under 48 GiB.  Oracles (a) and
    (b); there is no sum over the batch.  Measured: peak 47.77 GiB, 0.7 - 2.9 s."""
    B, H, W, C = CASES["backward"]
    D = (2 * SEARCH + 1) ** 2
    n_in, n_cv = B * H * W * C, B * H * W * D
    planned = cost_volume_planned_bytes(CASES["backward"])
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(3)
    a = arena
    a["prv"], a["nxt"] = _dgrid(gen, (B, H, W, C), 1 / 16), _dgrid(gen, (B, H, W, C), 1 / 16)
    a["out"], a["g"] = _dgrid(gen, (B, H, W, D), 1 / 16), _dgrid(gen, (B, H, W, D), 1 / 16)
    prv, nxt, out, g = a["prv"], a["nxt"], a["out"], a["g"]
    assert prv.numel() > 1 << 31 and out.numel() > 1 << 31
    worst = {}
    for k, what in enumerate(("grad_prv", "grad_nxt")):
        need = (k == 0, k == 1)
        both = ops.cost_volume_bwd(prv, nxt, out, g, SEARCH, 0.1, *need)
        assert both[1 - k] is None
        a["grad"] = big = both[k]
        del both
        for n in range(B):
            one = ops.cost_volume_bwd(prv[n:n + 1], nxt[n:n + 1], out[n:n + 1], g[n:n + 1], SEARCH, 0.1, *need)[k]
            assert torch.equal(one, big[n:n + 1]), "%s of image %d" % (what, n)
            del one
        worst[what] = 0.0
        for reg in pixel_crops(B, H, W, C, SEARCH) + [r for r in pixel_crops(B, H, W, D, SEARCH) if r[0] != "last"]:
            n, e = reg[1], reg[6]
            ref = cost_volume_bwd_ref(*[_cut(t, n, *e) for t in (prv, nxt, out, g)])[k]
            worst[what] = max(worst[what], _check(_inner(_cut(big, n, *e), reg), _inner(ref, reg),
                                                  "cost volume %s %s" % (reg[0], what)))
        del big
        a.pop("grad")
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("cost_volume_bwd: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}".format(peak / GIB, planned / GIB,
                                                                                             secs, worst))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


@pytest.mark.parametrize("mode", ["clamp", "tfwarp"])
def test_warp_bwd(mode, arena):
    """warp_bwd_kernel and fill_zero_kernel at img and grad_out of 2.156 G floats, through ops.warp_bwd.  grad_flo is a
    gather: oracles (a) and (b).  grad_img is a scatter of float atomics whose bits may vary with their order, so no
    bit equality is asked of it: oracle (b) only.  In clamp mode the fp16 path follows, whose grad_img is accumulated
    in the fp32 workspace and cast by f32_to_f16_kernel (bound of tests/test_gpu_autograd.py's fp16 case).
    Measured: peak 24.70 GiB, 0.1 - 0.9 s."""
    B, H, W, C = CASES["backward"]
    n_in = B * H * W * C
    planned = warp_planned_bytes(CASES["backward"])
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(4)
    a = arena
    a["img"], a["flo"], a["g"] = _dgrid(gen, (B, H, W, C), 1 / 16), _dflow(gen, B, H, W), _dgrid(gen, (B, H, W, C), 1 / 16)
    img, flo, g = a["img"], a["flo"], a["g"]
    assert img.numel() > 1 << 31
    a["gi"], a["gf"] = gi, gf = ops.warp_bwd(img, flo, g, mode)
    for n in range(B):
        one = ops.warp_bwd(img[n:n + 1], flo[n:n + 1], g[n:n + 1], mode, need_img=False)[1]
        assert torch.equal(one, gf[n:n + 1]), "grad_flo of image %d" % n
        del one
    worst = {"grad_img": 0.0, "grad_flo": 0.0}
    crops = pixel_crops(B, H, W, C, REACH + 2)
    refs = []
    for reg in crops:
        n, e = reg[1], reg[6]
        ri, rf = warp_bwd_ref(_cut(img, n, *e), _cut(flo, n, *e), _cut(g, n, *e), mode)
        refs.append(_inner(ri, reg))
        worst["grad_img"] = max(worst["grad_img"], _check(_inner(_cut(gi, n, *e), reg), refs[-1], "warp %s grad_img" % reg[0]))
        worst["grad_flo"] = max(worst["grad_flo"], _check(_inner(_cut(gf, n, *e), reg), _inner(rf, reg), "warp %s grad_flo" % reg[0]))
    if mode == "clamp":          # fp16 storage: values on the 1/16 grid are exact in fp16
        del gi, gf
        a.pop("gi"), a.pop("gf")
        a["img"], a["g"] = img, g = img.half(), g.half()
        gi16, gf16 = ops.warp_bwd(img, flo, g, mode)
        assert gi16.dtype == torch.float16
        for reg, ref in zip(crops, refs):
            got = _inner(_cut(gi16, reg[1], *reg[6]), reg).double()
            bound = F16_EPS * ref.abs() + 1e-6 * float(ref.abs().max()) + 2.0 ** -24
            assert bool(((got - ref).abs() <= bound).all()), ("fp16 grad_img", reg[0], float((got - ref).abs().max()))
        del gi16, gf16
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("warp_bwd {}: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}".format(mode, peak / GIB, planned / GIB,
                                                                                         secs, worst))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- the interpolator's pieces ---------------------------------------------------------------------------------------
def pixel_windows(B, H, W, C, boundaries=BOUNDARIES):
    """[(tag, n, y0, y1, x0, x1)]: WIN x WIN pixels at the start of image 0, in the rows just behind the pixel that holds
    each boundary of a dense (B,H,W,C) operand, and in the bottom-right corner of the last image."""
    wins = [("first", 0, 0, WIN, 0, WIN)]
    for b in crossed(B * H * W * C, boundaries):
        n, y, x = locate(b, H, W, C)
        assert y + 1 + WIN <= H, (b, y)
        wins.append((">2^%d" % (b.bit_length() - 1), n, y + 1, y + 1 + WIN) + _span(x, WIN, W))
    wins.append(("last", B - 1, H - WIN, H, W - WIN, W))
    return wins


def wrapped_pixel_regions(B, H, W, C, reg, elem_bytes=4):
    """conv_wrapped_regions for an operand that is read pixel by pixel: the window itself at its first element's byte
    offset mod 2^31 and mod 2^32, where that differs.  elem_bytes: 4 for fp32, 1 for a uint8 mask."""
    _, n, y0, y1, x0, x1 = reg
    first = ((n * H + y0) * W + x0) * C
    out = []
    for mod in (1 << 31, 1 << 32):
        e = (first * elem_bytes % mod) // elem_bytes
        if e != first:
            m, y, x = locate(e, H, W, C)
            y, x = min(y, H - (y1 - y0)), min(x, W - (x1 - x0))
            out.append((mod, (m, y, y + y1 - y0, x, x + x1 - x0)))
    return out


def head_window_sums(crops, w2):
    """grad_w2 (3,64) and grad_b2 (3) in float64 of a grad_out that is zero outside the windows: crops = [(z, g)]."""
    gw = sum(g.double().reshape(-1, 3).t() @ z.double().reshape(-1, 64) for z, g in crops)
    return gw, sum(g.double().reshape(-1, 3).sum(0) for _, g in crops)


def head_controls(crops, moved):
    ref = head_window_sums(crops, None)[0]
    out = [("without window %d" % k, float((head_window_sums(crops[:k] + crops[k + 1:], None)[0] - ref).abs().max()) / _tol(ref))
           for k in range(len(crops))]
    for what, k, z in moved:
        alt = head_window_sums(crops[:k] + [(z, crops[k][1])] + crops[k + 1:], None)[0]
        out.append((what, float((alt - ref).abs().max()) / _tol(ref)))
    return out


def image_head_planned_bytes(key, ws_floats):
    """z and grad_z, out and grad_out, the workspace; out and grad_z of one image."""
    B, H, W = key
    M = B * H * W
    return 4 * (2 * M * 64 + 2 * M * 3 + ws_floats + H * W * 67)


def upsample_planned_bytes(key):
    """in and grad_in, out and grad_out; out and grad_in of one image."""
    B, h, w, C = key
    n_in = B * h * w * C
    return 4 * (2 * n_in + 8 * n_in + (4 * n_in + n_in) // B)


def pyramid_planned_bytes(key):
    """x, the output, the output of the one-image repeats."""
    B, H, W, C, levels = key
    return 4 * (B * H * W * C + 2 * B * H * W * C // (1 << 2 * levels))


def test_image_head(arena):
    """Image head forward and backward at M = 33.7 M pixels (> 2^25) of 64 features, z and grad_z of 2.156 G floats,
    through autograd.  out and grad_z: oracles (a) and (b) (the op is pixel-wise: a crop needs no halo).  grad_w2 and
    grad_b2: oracle (c); the layer is linear, so they are exact on the grids (precondition asserted).
    Measured: peak 20.29 GiB, 0.03 - 1.3 s."""
    B, H, W = CASES["image_head"]
    M = B * H * W
    L = ops._hip.lib()
    planned = image_head_planned_bytes(CASES["image_head"], L.qpwc_image_head_bwd_workspace_floats(M))
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = arena
    a["z"] = _dgrid(gen, (B, H, W, 64), 1 / 16).requires_grad_()
    w2 = _dgrid(gen, (3, 64, 1, 1), 1 / 64, 1 / 8).requires_grad_()
    b2 = _dgrid(gen, (3,), 1 / 8).requires_grad_()
    a["g"] = _dgrid(gen, (B, H, W, 3), 1 / 16)
    z, g = a["z"], a["g"]
    assert z.numel() > 1 << 31 and M > 1 << 25
    a["out"] = ops.image_head(z, w2, b2)
    a["out"].backward(g)
    out, gz = a["out"].detach(), z.grad
    wd, bd = w2.detach(), b2.detach()
    for n in range(B):
        z1 = z.detach()[n:n + 1].requires_grad_()
        o1 = ops.image_head(z1, wd, bd)
        o1.backward(g[n:n + 1])
        assert torch.equal(o1.detach(), out[n:n + 1]) and torch.equal(z1.grad, gz[n:n + 1]), "image %d" % n
        del z1, o1
    wc, bc = wd.double().cpu().reshape(3, 64), bd.double().cpu()
    worst = {"out": 0.0, "grad_z": 0.0}
    for reg in pixel_crops(B, H, W, 64, 0):
        zc, gc = _cut(z, *reg[1:6]).double(), _cut(g, *reg[1:6]).double()
        worst["out"] = max(worst["out"], _check(_cut(out, *reg[1:6]), zc @ wc.t() + bc, "image head %s out" % reg[0]))
        worst["grad_z"] = max(worst["grad_z"], _check(_cut(gz, *reg[1:6]), gc @ wc, "image head %s grad_z" % reg[0]))
    wins = pixel_windows(B, H, W, 64)
    g.zero_()
    crops, moved = [], []
    for k, reg in enumerate(wins):
        n, y0, y1, x0, x1 = reg[1:]
        g[n, y0:y1, x0:x1, :] = _dgrid(gen, (y1 - y0, x1 - x0, 3), 1 / 16)
        crops.append((_cut(z, *reg[1:]), _cut(g, *reg[1:])))
        for mod, at in wrapped_pixel_regions(B, H, W, 64, reg):
            moved.append(("window %d (%s) z read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k, _cut(z, *at)))
    _, gw, gb = ops.image_head_bwd(z.detach(), wd, g, need=(False, True, True))
    rw, rb = head_window_sums(crops, None)
    assert float(head_window_sums([(zc.abs(), gc.abs()) for zc, gc in crops], None)[0].max()) * 2 ** 8 < 2 ** 24
    assert torch.equal(gw.double().cpu(), rw), float((gw.double().cpu() - rw).abs().max())
    assert torch.equal(gb.double().cpu(), rb), float((gb.double().cpu() - rb).abs().max())
    controls = head_controls(crops, moved)
    assert len(controls) >= len(wins) + 2 and min(r for _, r in controls) >= 100.0, controls
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("image_head: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}, controls {:.0f} .. {:.0f} bounds".format(
        peak / GIB, planned / GIB, secs, worst, min(r for _, r in controls), max(r for _, r in controls)))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


def upsample_regions(reg, h, w):
    """An output region (.., oy0, oy1, ox0, ox1) of the x2 upsampling -> (the input region one pixel wider than what it
    reads, clipped to the image; the region's place (y0, y1, x0, x1) in the upsampled input region)."""
    _, _, oy0, oy1, ox0, ox1 = reg[:6]
    iy0, iy1 = max((oy0 - 1) // 2 - 1, 0), min(oy1 // 2 + 2, h)
    ix0, ix1 = max((ox0 - 1) // 2 - 1, 0), min(ox1 // 2 + 2, w)
    return (iy0, iy1, ix0, ix1), (oy0 - 2 * iy0, oy1 - 2 * iy0, ox0 - 2 * ix0, ox1 - 2 * ix0)


def upsample_valid(reg, h, w):
    """Mask over the input region: the four output rows / columns that an input pixel's gradient reads (2i - 1 .. 2i + 2,
    clamped to the image) all lie in the output region."""
    (iy0, iy1, ix0, ix1), _ = upsample_regions(reg, h, w)
    _, _, oy0, oy1, ox0, ox1 = reg[:6]
    ok = lambda i, o0, o1, n: all(o0 <= min(max(t, 0), 2 * n - 1) < o1 for t in (2 * i - 1, 2 * i, 2 * i + 1, 2 * i + 2))
    return torch.tensor([ok(i, oy0, oy1, h) for i in range(iy0, iy1)])[:, None] & \
        torch.tensor([ok(j, ox0, ox1, w) for j in range(ix0, ix1)])[None, :]


def upsample_region_ref(xc, place, gc, scale):
    """Float64 autograd of F.interpolate(x2, bilinear) on an input region -> (the output region, grad of the input)."""
    leaf = xc.double().clone().requires_grad_()
    up = F.interpolate(leaf.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1) * scale
    out = up[:, place[0]:place[1], place[2]:place[3]]
    out.backward(gc.double())
    return out.detach(), leaf.grad


def test_upsample2x_image(arena):
    """upsample2x_image forward and backward at C = 3 with 2.150 G output floats (and 0.537 G input floats, past 2^29),
    through autograd, scale 2.  Per-pixel outputs only: oracles (a) and (b).  Measured: peak 24.03 GiB, 0.03 - 2.9 s."""
    B, h, w, C = CASES["upsample2x_image"]
    n_in = B * h * w * C
    planned = upsample_planned_bytes(CASES["upsample2x_image"])
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(6)
    a = arena
    a["x"] = _dgrid(gen, (B, h, w, C), 1 / 16).requires_grad_()
    a["g"] = _dgrid(gen, (B, 2 * h, 2 * w, C), 1 / 16)
    x, g = a["x"], a["g"]
    assert g.numel() > 1 << 31 and x.numel() > 1 << 29
    a["out"] = ops.upsample2x_image(x, 2.0)
    a["out"].backward(g)
    out, gx = a["out"].detach(), x.grad
    for n in range(B):
        x1 = x.detach()[n:n + 1].requires_grad_()
        o1 = ops.upsample2x_image(x1, 2.0)
        o1.backward(g[n:n + 1])
        assert torch.equal(o1.detach(), out[n:n + 1]) and torch.equal(x1.grad, gx[n:n + 1]), "image %d" % n
        del x1, o1
    worst = {"out": 0.0, "grad_in": 0.0}
    regs = pixel_crops(B, 2 * h, 2 * w, C, 0)
    for b in crossed(n_in):                      # and around the input pixel that holds the input's own boundary
        n, y, x_ = locate(b, h, w, C)
        regs.append(("in>2^%d" % (b.bit_length() - 1), n) + _span(2 * y, CROP, 2 * h) + _span(2 * x_, CROP, 2 * w))
    for reg in regs:
        n = reg[1]
        (iy0, iy1, ix0, ix1), place = upsample_regions(reg, h, w)
        ro, rx = upsample_region_ref(_cut(x, n, iy0, iy1, ix0, ix1), place, _cut(g, *reg[1:6]), 2.0)
        worst["out"] = max(worst["out"], _check(_cut(out, *reg[1:6]), ro, "upsample %s out" % reg[0]))
        ok = upsample_valid(reg, h, w)
        assert int(ok.sum()) >= (CROP // 2 - 2) ** 2, (reg[0], int(ok.sum()))
        worst["grad_in"] = max(worst["grad_in"], _check(_cut(gx, n, iy0, iy1, ix0, ix1)[0][ok], rx[0][ok],
                                                        "upsample %s grad_in" % reg[0]))
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("upsample2x_image: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}".format(peak / GIB, planned / GIB,
                                                                                             secs, worst))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


def pyramid_ref(x, levels):
    """`levels` 2 x 2 means in float64, each (((a + b) + c) + d) / 4 in row-major order like a chain of AvgPool2D."""
    x = x.double()
    for _ in range(levels):
        x = (((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + x[:, 1::2, 0::2]) + x[:, 1::2, 1::2]) * 0.25
    return x


def test_avgpool_pyramid(arena):
    """avgpool_pyramid at levels = 5 on 2.154 G input floats (C = 3).  Oracle (a) per image, and (b) on the 4 x 4 output
    pixels around the one whose 32 x 32 inputs hold each boundary, and on the last ones.  Measured: peak 8.04 GiB, 0.01 s."""
    B, H, W, C, levels = CASES["avgpool_pyramid"]
    S = 1 << levels
    n_in = B * H * W * C
    planned = pyramid_planned_bytes(CASES["avgpool_pyramid"])
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(7)
    arena["x"] = x = _dgrid(gen, (B, H, W, C), 1 / 16)
    assert x.numel() > 1 << 31
    out = ops.avgpool_pyramid(x, levels)
    assert tuple(out.shape) == (B, H // S, W // S, C)
    for n in range(B):
        assert torch.equal(ops.avgpool_pyramid(x[n:n + 1], levels), out[n:n + 1]), "image %d" % n
    worst = 0.0
    regs = [(">2^%d" % (b.bit_length() - 1),) + locate(b, H, W, C) for b in crossed(n_in)]
    regs = [(t, n) + _span(y // S, 4, H // S) + _span(x_ // S, 4, W // S) for t, n, y, x_ in regs]
    regs.append(("last", B - 1, H // S - 4, H // S, W // S - 4, W // S))
    for tag, n, y0, y1, x0, x1 in regs:
        ref = pyramid_ref(_cut(x, n, y0 * S, y1 * S, x0 * S, x1 * S), levels)
        worst = max(worst, _check(_cut(out, n, y0, y1, x0, x1), ref, "pyramid %s" % tag))
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("avgpool_pyramid: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {:.3e}".format(peak / GIB, planned / GIB,
                                                                                              secs, worst))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- losses and EPE: sums over the batch, planted windows ------------------------------------------------------------
LOSS_DELTA = 0.1                 # FlowMseLossV2's Huber delta, the reference's
# a loss value or an EPE is a sum of fp32 terms that are exactly zero outside the windows: a thread adds a few window
# terms, then 6 wave steps, 2 block steps, and the fold of at most 2048 partials in 256 lanes + 8 steps; with the few
# roundings of a term itself fewer than 64 roundings of 2^-24 lie on any path, 3.8e-6 relative.  Asserted: 1e-5.
LOSS_REL = 1e-5


def loss_planned_bytes(key, level, with_gt_out):
    """gt, and per prediction level: the prediction, dpred saved by the forward, grad_pred (and gt_out where the
    prediction is made from it)."""
    B, H, W, C = key
    return 4 * (B * H * W * C + (4 if with_gt_out else 3) * B * level[0] * level[1] * C)


def loss_window_ref(kind, crops, n_pix, hw, scale=1.0):
    """Float64 value and gradients of a loss whose prediction equals the level's ground truth outside the windows:
    crops = [(gl, p)], gl the level's resampled, flow-scaled ground truth on a window, p the prediction there; n_pix the
    pixels of the whole level.  kind "v2": FlowMseLossV2 (Keras Huber of s * pred - s * gt, s = 2 / (w + h), mean over
    elements); "norm": FlowMseLoss and the EPE (mean over pixels of the 2-norm, gradient 0 at a zero residual).
    -> (scale * loss, [d / d p])."""
    leaves = [p.double().clone().requires_grad_() for _, p in crops]
    total = torch.zeros((), dtype=torch.float64)
    for (gl, _), p in zip(crops, leaves):
        if kind == "v2":
            s = 2.0 / (hw[0] + hw[1])
            e = s * p - s * gl.double()
            a = e.abs()
            total = total + torch.where(a <= LOSS_DELTA, 0.5 * e * e, LOSS_DELTA * a - 0.5 * LOSS_DELTA ** 2).sum() / (2 * n_pix)
        else:
            sq = (gl.double() - p).pow(2).sum(-1)
            total = total + (torch.where(sq > 0, sq, torch.ones_like(sq)).sqrt() * (sq > 0)).sum() / n_pix
    total = total * scale
    total.backward()
    return total.detach(), [t.grad for t in leaves]


def loss_controls(kind, crops, moved, n_pix, hw):
    """[(what, |change of the loss| / its bound)]: every window left out in turn; every moved = (what, window index,
    the level's ground truth as a wrapped offset finds it) in its window's place."""
    ref = float(loss_window_ref(kind, crops, n_pix, hw)[0])
    out = []
    for k in range(len(crops)):
        alt = float(loss_window_ref(kind, crops[:k] + crops[k + 1:], n_pix, hw)[0])
        out.append(("without window %d" % k, abs(alt - ref) / (LOSS_REL * abs(ref))))
    for what, k, gl in moved:
        alt = float(loss_window_ref(kind, crops[:k] + [(gl, crops[k][1])] + crops[k + 1:], n_pix, hw)[0])
        out.append((what, abs(alt - ref) / (LOSS_REL * abs(ref))))
    return out


def area_level_ref(gt_crop, sh, sw, fscale):
    """FlowMseLossV2's level ground truth of a crop in float64: the mean over sh x sw blocks times the flow scale."""
    _, hh, ww, c = gt_crop.shape
    return gt_crop.double().reshape(1, hh // sh, sh, ww // sw, sw, c).mean((2, 4)) * fscale


def loss_tile_windows(key):
    """Windows of the half-resolution prediction of the tile case: pixel_windows of the prediction itself, and behind
    the prediction pixel under each boundary pixel of the ground truth; one entry per distinct place."""
    B, H, W, C = key
    h, w = H // 2, W // 2
    wins = pixel_windows(B, h, w, C)
    seen = {x[1:] for x in wins}
    for b in crossed(B * H * W * C):
        n, y, x = locate(b, H, W, C)
        assert y // 2 + 2 + WIN <= h
        reg = (n, y // 2 + 2, y // 2 + 2 + WIN) + _span(x // 2, WIN, w)
        if reg not in seen:
            seen.add(reg)
            wins.insert(-1, ("gt>2^%d" % (b.bit_length() - 1),) + reg)
    return wins


def _rel_check(got, ref, what):
    got = got.detach().double().cpu()
    scale = float(ref.abs().max())
    d = float((got - ref).abs().max())
    print("{}: max|d| = {:.3e} of {:.3e}, bound {:.1e} relative".format(what, d, scale, LOSS_REL))
    assert scale > 0 and bool(torch.isfinite(got).all()) and d <= LOSS_REL * scale, (what, d, scale)
    return d / scale


def _count_above(t, thr, rows=1024):
    """Elements of a (B,H,W,C) tensor with |value| > thr, counted a block of rows at a time (small temporaries)."""
    return sum(int(torch.count_nonzero(t[n, y:y + rows].abs() > thr)) for n in range(t.shape[0])
               for y in range(0, t.shape[1], rows))


def _loss_run(kind_id, gt, pred, scale):
    """ops.loss through autograd -> (loss value on the device, grad of pred)."""
    p = pred.detach().requires_grad_()
    losses = ops.loss(kind_id, gt, [p], p0=LOSS_DELTA)
    (losses * scale).sum().backward()
    return losses.detach()[0], p.grad


def test_loss_tile_path(arena):
    """FlowMseLossV2 on loss_area_tile_kernel and loss_bwd_kernel's float4 path at a ground truth of 1.075 G pixels
    (2.150 G floats) and one half-resolution level.  The prediction is the kernel's own gt_out, held on crops to the
    float64 area mean bit for bit (oracle (b)), plus planted windows; the loss value and grad_pred against float64
    from the windows' crops (oracle (c), LOSS_REL).  Outside the windows the kernel's Huber error s * pred - s * gt is the
    rounding of its own fused multiply-add, not zero: grad_pred there must stay below LOSS_REL of the windows' largest
    gradient, which is asserted over the whole tensor.  Measured: peak 14.01 GiB (planned 16.02), 0.4 s."""
    key = CASES["loss"]
    B, H, W, C = key
    h, w = H // 2, W // 2
    hip = ops._hip
    planned = loss_planned_bytes(key, (h, w), True)
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(8)
    a = arena
    a["gt"] = gt = _dgrid(gen, (B, H, W, C), 1 / 16)
    assert B * H * W > 1 << 30 and gt.numel() > 1 << 31 and gt.data_ptr() % 16 == 0
    I = ops.ctypes.c_int
    assert hip.lib().qpwc_loss_fwd_kernel(hip.LOSS_FLOW_MSE_V2, gt.data_ptr(), B, H, W, C, (I * 1)(h), (I * 1)(w),
                                          1).decode() == "loss_area_tile_kernel"
    a["gl"] = gl = ops.area_ground_truth(gt, [(h, w)])[0]
    regs = [r[:6] for r in pixel_crops(B, h, w, C, 0)]
    regs += [("gt" + t, n, y0 // 2, y0 // 2 + CROP // 2, x0 // 2, x0 // 2 + CROP // 2)     # the level pixels under a boundary
             for t, n, y0, _, x0, _, _ in pixel_crops(B, H, W, C, 0) if t != "last"]       # pixel of the ground truth
    for tag, n, y0, y1, x0, x1 in regs:
        ref = area_level_ref(_cut(gt, n, 2 * y0, 2 * y1, 2 * x0, 2 * x1), 2, 2, h / H)
        assert torch.equal(_cut(gl, n, y0, y1, x0, x1).double(), ref), "gt_out " + tag
    a["pred"] = pred = gl.clone()
    wins = loss_tile_windows(key)
    crops, moved = [], []
    for k, reg in enumerate(wins):
        n, y0, y1, x0, x1 = reg[1:]
        pred[n, y0:y1, x0:x1, :] += _dgrid(gen, (y1 - y0, x1 - x0, C), 1 / 16)
        crops.append((area_level_ref(_cut(gt, n, 2 * y0, 2 * y1, 2 * x0, 2 * x1), 2, 2, h / H), _cut(pred, *reg[1:])))
        for mod, at in wrapped_pixel_regions(B, H, W, C, (reg[0], n, 2 * y0, 2 * y1, 2 * x0, 2 * x1)):
            moved.append(("window %d (%s) gt read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k,
                          area_level_ref(_cut(gt, *at), 2, 2, h / H)))
    del gl
    a.pop("gl")
    value, grad = _loss_run(hip.LOSS_FLOW_MSE_V2, gt, pred, 7.0)
    a["grad"] = grad
    rv, rg = loss_window_ref("v2", crops, B * h * w, (h, w), 7.0)
    worst = {"loss": _rel_check(value * 7.0, rv, "tile loss")}
    worst["grad_pred"] = max(_rel_check(_cut(grad, *reg[1:]), g, "tile grad_pred %s" % reg[0]) for reg, g in zip(wins, rg))
    big = max(float(g.abs().max()) for g in rg)
    assert 0 < _count_above(grad, LOSS_REL * big) <= len(wins) * WIN * WIN * C       # nothing of weight outside the windows
    assert grad.numel() % 4 == 0                                       # loss_bwd_kernel's float4 path
    controls = loss_controls("v2", crops, moved, B * h * w, (h, w))
    assert len(controls) >= len(wins) + 2 and min(r for _, r in controls) >= 100.0, controls
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("loss tile: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}, controls {:.0f} .. {:.0f} bounds".format(
        peak / GIB, planned / GIB, secs, worst, min(r for _, r in controls), max(r for _, r in controls)))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


def test_loss_pixel_paths_and_epe(arena):
    """On an odd-sized ground truth of 1.075 G pixels with one full-resolution level (the resampling is the identity,
    so the prediction is a copy of the ground truth plus planted windows): FlowMseLossV2 on loss_pixel_kernel (area
    1 x 1), FlowMseLoss on its bilinear branch, loss_bwd_kernel's scalar path (the element count is no multiple of 4),
    epe_partial_kernel and epe_multi_partial_kernel (float4 loop with the odd last pixel).  Values and grad_pred
    against float64 from the windows' crops (oracle (c), LOSS_REL), grad_pred below LOSS_REL of the windows' largest
    gradient everywhere else (asserted over the whole tensor); prediction and
    grad_pred cross all three boundaries like the ground truth.  Measured: peak 32.05 GiB (planned 32.05), 0.1 s."""
    key = CASES["epe"]
    B, H, W, C = key
    hip = ops._hip
    planned = loss_planned_bytes(key, (H, W), False)
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(9)
    a = arena
    a["gt"] = gt = _dgrid(gen, (B, H, W, C), 1 / 16)
    assert B * H * W > 1 << 30 and gt.numel() > 1 << 31 and gt.numel() % 4 and (B * H * W) % 2
    I = ops.ctypes.c_int
    for kind in (hip.LOSS_FLOW_MSE_V2, hip.LOSS_FLOW_MSE):
        assert hip.lib().qpwc_loss_fwd_kernel(kind, gt.data_ptr(), B, H, W, C, (I * 1)(H), (I * 1)(W),
                                              1).decode() == "loss_pixel_kernel"
    a["pred"] = pred = gt.clone()
    wins = pixel_windows(B, H, W, C)
    crops, moved = [], []
    for k, reg in enumerate(wins):
        n, y0, y1, x0, x1 = reg[1:]
        pred[n, y0:y1, x0:x1, :] += _dgrid(gen, (y1 - y0, x1 - x0, C), 1 / 16)
        crops.append((_cut(gt, *reg[1:]).double(), _cut(pred, *reg[1:])))
        for mod, at in wrapped_pixel_regions(B, H, W, C, reg):
            moved.append(("window %d (%s) gt read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k,
                          _cut(gt, *at).double()))
    worst = {}
    for name, kind_id, kind in (("v2 pixel", hip.LOSS_FLOW_MSE_V2, "v2"), ("bilinear", hip.LOSS_FLOW_MSE, "norm")):
        value, grad = _loss_run(kind_id, gt, pred, 7.0)
        rv, rg = loss_window_ref(kind, crops, B * H * W, (H, W), 7.0)
        worst[name] = _rel_check(value * 7.0, rv, name + " loss")
        worst[name + " grad"] = max(_rel_check(_cut(grad, *reg[1:]), g, "%s grad_pred %s" % (name, reg[0]))
                                    for reg, g in zip(wins, rg))
        big = max(float(g.abs().max()) for g in rg)
        assert 0 < _count_above(grad, LOSS_REL * big) <= len(wins) * WIN * WIN * C
        del grad
        controls = loss_controls(kind, crops, moved, B * H * W, (H, W))
        assert len(controls) >= len(wins) + 2 and min(r for _, r in controls) >= 100.0, controls
    rv = loss_window_ref("norm", crops, B * H * W, (H, W))[0]
    worst["epe"] = _rel_check(ops.epe(gt, pred), rv, "epe")
    worst["epe_multi"] = _rel_check(ops.epe_multi([gt], [pred])[0], rv, "epe_multi")
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("loss pixel / epe: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}, controls {:.0f} .. {:.0f} bounds".format(
        peak / GIB, planned / GIB, secs, worst, min(r for _, r in controls), max(r for _, r in controls)))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- masked losses: a byte-indexed mask past 2^31, a ground truth past 2^32 elements ---------------------------------
# The masked flow losses are sums over the valid pixels only: validity is zero except planted WIN x WIN windows, so the
# counts, the level masks, the level ground truths, the loss and grad_pred follow in float64 from the windows' crops,
# and whatever lies elsewhere -- random ground truth, random predictions -- must reach nothing.  A mask read at a
# wrapped byte offset finds zeros (the window drops out: the count fails), a ground truth read at a wrapped offset
# finds other values.  Bounds: LOSS_REL for the loss and grad_pred; the project's 1e-6 of the level's largest for the
# level ground truth; counts and masks exact; gradients exactly 0 outside the windows, over the whole tensor.
GT_REL = 1e-6                    # tests/test_gpu_masked_loss.py's bound of the level ground truth


def masked_loss_windows(key, level=None):
    """[(tag, n, y0, y1, x0, x1)] in ground-truth pixels: pixel_windows of the ground truth with the boundary at 2^32
    elements added, of the mask (a byte a pixel) and, with `level` = (h, w), of the level's own tensors (prediction,
    dpred, grad_pred); one entry per distinct place."""
    B, H, W, C = key
    wins = pixel_windows(B, H, W, C, BOUNDARIES_32)
    seen = {x[1:] for x in wins}
    more = [("mask" + x[0],) + x[1:] for x in pixel_windows(B, H, W, 1, BOUNDARIES_32)[1:-1]]
    if level is not None:
        h, w = level
        sh, sw = H // h, W // w
        more += [("pred" + t, n, sh * y0, sh * y0 + WIN) + _span(sw * x0, WIN, W)
                 for t, n, y0, _, x0, _ in pixel_windows(B, h, w, C, BOUNDARIES_32)[1:-1]]
    for x in more:
        if x[1:] not in seen:
            seen.add(x[1:])
            wins.insert(-1, x)
    return wins


def aligned_region(win, tile, H, W):
    """The window's enclosing region of whole tile x tile blocks -> (tag, n, y0, y1, x0, x1)."""
    tag, n, y0, y1, x0, x1 = win
    up = lambda v, lim: min(-(-v // tile) * tile, lim)
    return (tag, n, y0 // tile * tile, up(y1, H), x0 // tile * tile, up(x1, W))


def region_around(win, reg, at, H, W):
    """Where a window's aligned region lies when the window itself is found at `at` = (n, y0, y1, x0, x1)."""
    n, y, _, x, _ = at
    hh, ww = reg[3] - reg[2], reg[5] - reg[4]
    y = min(max(y - (win[2] - reg[2]), 0), H - hh)
    x = min(max(x - (win[4] - reg[4]), 0), W - ww)
    return (n, y, y + hh, x, x + ww)


def masked_area_level_ref(gt_crop, ok_crop, sh, sw, fscale):
    """The masked FlowMseLossV2 level of a crop in float64: the mean over each sh x sw block's valid pixels times the flow
    scale, 0 where the block has none -> (gl (1,hh,ww,2), m (1,hh,ww) bool)."""
    _, hh, ww, c = gt_crop.shape
    ok = ok_crop.reshape(1, hh, ww) != 0
    x = torch.where(ok[..., None], gt_crop.double(), torch.zeros((), dtype=torch.float64))
    s = x.reshape(1, hh // sh, sh, ww // sw, sw, c).sum((2, 4))
    n = ok.reshape(1, hh // sh, sh, ww // sw, sw).sum((2, 4))
    return s / n.clamp(min=1)[..., None] * fscale, n >= 1


def masked_window_ref(kind, crops, hw, scale=1.0):
    """loss_window_ref for a masked loss: crops = [(gl, m, p)] with m the level's validity on the window.  An invalid
    pixel is given a zero residual, whose term and gradient are 0 in both kinds, and the mean runs over the count
    -> (scale * loss, [d / d p], count)."""
    count = sum(int(m.sum()) for _, m, _ in crops)
    fed = [(gl, torch.where(m[..., None], p.double(), gl.double())) for gl, m, p in crops]
    value, grads = loss_window_ref(kind, fed, max(count, 1), hw, scale)
    return value, grads, count


def masked_loss_controls(kind, crops, moved, hw):
    """loss_controls for a masked loss -> [(what, change / bound)], the change being the larger of what the two asserted
    quantities show: the loss (relative, LOSS_REL) and grad_pred on the windows (LOSS_REL of each window's largest).  The
    loss is a mean over the valid pixels, so a window left out takes its pixels out of the count as well and may leave
    the mean nearly where it was; its own gradient then vanishes, and every other window's grows with the count."""
    rv, rg, _ = masked_window_ref(kind, crops, hw)

    def change(alt_crops, at):
        """at: the positions of alt_crops' windows in crops."""
        av, ag, _ = masked_window_ref(kind, alt_crops, hw)
        grads = dict(zip(at, ag))
        moved_by = [float(((grads[k] if k in grads else torch.zeros_like(g)) - g).abs().max()) / (LOSS_REL * float(g.abs().max()))
                    for k, g in enumerate(rg)]
        return max([abs(float(av - rv)) / (LOSS_REL * abs(float(rv)))] + moved_by)

    every = list(range(len(crops)))
    out = [("without window %d" % k, change(crops[:k] + crops[k + 1:], every[:k] + every[k + 1:])) for k in every]
    for what, k, gl in moved:
        out.append((what, change(crops[:k] + [(gl, crops[k][1], crops[k][2])] + crops[k + 1:], every)))
    return out


def masked_loss_planned_bytes(key, levels, held):
    """The ground truth, its mask, and `held` fp32 tensors per level at the fullest moment (prediction, dpred, grad_pred;
    a fourth where a second gradient or the level's ground truth is held beside them) with a byte a level pixel."""
    B, H, W, C = key
    return 4 * B * H * W * C + B * H * W + sum((4 * held * C + 1) * B * h * w for h, w in levels)


def _fill_grid(t, gen, lim=16):
    """Multiples of 1/16 in [-lim/16, lim/16] drawn in place, an image at a time (no temporary of the tensor's size)."""
    for n in range(t.shape[0]):
        t[n].random_(-lim, lim + 1, generator=gen).mul_(1 / 16)
    return t


def _nonzero(t, rows=2048):
    """count_nonzero of a (B,H,...) tensor, a block of rows at a time."""
    return sum(int(torch.count_nonzero(t[n, y:y + rows])) for n in range(t.shape[0]) for y in range(0, t.shape[1], rows))


def _cut3(t, n, y0, y1, x0, x1):
    return t.detach()[n:n + 1, y0:y1, x0:x1].cpu()


def _masked_run(kind_id, gt, preds, valid, scale):
    """ops.masked_loss through autograd -> (per-level losses, counts, [grad of each prediction])."""
    xs = [p.detach().requires_grad_() for p in preds]
    losses, counts = ops.masked_loss(kind_id, gt, xs, valid, p0=LOSS_DELTA)
    (losses * scale).sum().backward()
    return losses.detach(), counts, [x.grad for x in xs]


def _masked_level_crops(gt, valid, pred, regs, factor, fscale):
    """[(gl, m, p)] of one level on the windows' regions, from crops of the device tensors."""
    sh, sw = factor
    out = []
    for _, n, y0, y1, x0, x1 in regs:
        gl, m = masked_area_level_ref(_cut(gt, n, y0, y1, x0, x1), _cut3(valid, n, y0, y1, x0, x1), sh, sw, fscale)
        out.append((gl, m, _cut(pred, n, y0 // sh, y1 // sh, x0 // sw, x1 // sw)))
    return out


def _check_masked_level(what, crops, regs, factor, hw, value, count, grad, gt_out, valid_out, kind, scale):
    """One level of a masked loss against float64 from the windows' crops: the loss and grad_pred within LOSS_REL, the
    count and the level mask exact, the level ground truth within GT_REL, and over the whole tensors nothing but the
    windows: grad_pred and gt_out exactly 0 elsewhere, valid_out 0."""
    sh, sw = factor
    rv, rg, rcount = masked_window_ref(kind, crops, hw, scale)
    assert int(count) == rcount > 0, (what, int(count), rcount)
    worst = {"loss": _rel_check(value * scale, rv, what + " loss")}
    level_reg = lambda r: (r[1], r[2] // sh, r[3] // sh, r[4] // sw, r[5] // sw)
    worst["grad_pred"] = max(_rel_check(_cut(grad, *level_reg(r)), g, "%s grad_pred %s" % (what, r[0])) for r, g in zip(regs, rg))
    inside = sum(int(torch.count_nonzero(_cut(grad, *level_reg(r)))) for r in regs)
    assert 0 < inside == _nonzero(grad), (what, inside)                     # exactly 0 outside the windows
    for r, (gl, m, _) in zip(regs, crops):
        assert not _cut(grad, *level_reg(r))[~m].any(), (what, r[0])         # and at the windows' own invalid pixels
    if gt_out is not None:
        top = max(float(gl.abs().max()) for gl, _, _ in crops)
        d = max(float((_cut(gt_out, *level_reg(r)).double() - gl).abs().max()) for r, (gl, _, _) in zip(regs, crops))
        print("{} gt_out: max|d| = {:.3e}, bound {:.3e}".format(what, d, GT_REL * top))
        assert d <= GT_REL * top, (what, d, top)
        worst["gt_out"] = d / top
        assert sum(int(torch.count_nonzero(_cut(gt_out, *level_reg(r)))) for r in regs) == _nonzero(gt_out)
        for r, (_, m, _) in zip(regs, crops):
            assert torch.equal(_cut3(valid_out, *level_reg(r)) != 0, m), (what, r[0])
        assert _nonzero(valid_out) == rcount and valid_out.dtype == torch.uint8
    return worst


def test_masked_loss_tile_path(arena):
    """FlowMseLossV2 over the valid pixels on masked_loss_tile_kernel at 2.152 G ground-truth pixels with levels at
    factors (2,2) and (32,32): the mask's byte index passes 2^31, the ground truth's element index 2^29 .. 2^32, the
    level tensors' 2^29 and 2^30.  Ground truth and predictions are random on the 1/16 grid everywhere; validity is
    zero except WIN x WIN windows at the start, behind every boundary and in the last corner.  Once with the mask;
    once more on the same buffers with valid=None and NaN outside the windows, which must give the same bits.
    Measured: peak 34.14 GiB (planned 34.64), 0.6 s; of the bounds, losses 0.0005, grad_pred 0.013, gt_out 0.017; the
    controls moved the loss or grad_pred by 190 .. 100000 bounds."""
    key = CASES["masked_loss"]
    B, H, W, C = key
    hip = ops._hip
    factors = [(2, 2), (32, 32)]
    levels = [(H // sh, W // sw) for sh, sw in factors]
    planned = masked_loss_planned_bytes(key, levels, 4)
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(18)
    a = arena
    assert ops.masked_loss_kernel(hip.LOSS_FLOW_MSE_V2, B, H, W, levels) == "masked_loss_tile_kernel"
    a["gt"] = gt = _fill_grid(torch.empty((B, H, W, C), device=DEV), gen)
    assert B * H * W > 1 << 31 and gt.numel() > 1 << 32 and gt.data_ptr() % 16 == 0
    a["valid"] = valid = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    wins = masked_loss_windows(key, levels[0])
    regs = [aligned_region(x, 32, H, W) for x in wins]
    for _, n, y0, y1, x0, x1 in wins:
        valid[n, y0:y1, x0:x1] = 1
    assert _nonzero(valid) == len(wins) * WIN * WIN
    a["preds"] = preds = [_fill_grid(torch.empty((B, h, w, C), device=DEV), gen) for h, w in levels]
    crops = [_masked_level_crops(gt, valid, p, regs, f, 1.0 / f[0]) for p, f in zip(preds, factors)]
    moved = [[], []]
    for k, (win, reg) in enumerate(zip(wins, regs)):
        for mod, at in wrapped_pixel_regions(B, H, W, C, win):
            at = region_around(win, reg, at, H, W)
            for l, f in enumerate(factors):
                gl = masked_area_level_ref(_cut(gt, *at), _cut3(valid, *reg[1:]), f[0], f[1], 1.0 / f[0])[0]
                moved[l].append(("window %d (%s) gt read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k, gl))
        for mod, at in wrapped_pixel_regions(B, H, W, 1, win, 1):               # the mask at a wrapped byte offset: zeros
            assert not _cut3(valid, *at).any(), (win, mod, at)
    losses, counts, grads = _masked_run(hip.LOSS_FLOW_MSE_V2, gt, preds, valid, 7.0)
    a["grads"] = grads
    _, counts2, _, gt_out, valid_out = ops.masked_loss_fwd(hip.LOSS_FLOW_MSE_V2, gt, None, valid, p0=LOSS_DELTA,
                                                           want_gt=True, want_valid=True, shapes=levels)
    assert torch.equal(counts, counts2)
    worst, controls = {}, []
    for l, f in enumerate(factors):
        w_ = _check_masked_level("masked tile level %d" % l, crops[l], regs, f, levels[l], losses[l], counts[l], grads[l],
                                 gt_out[l], valid_out[l], "v2", 7.0)
        worst.update({"%s[%d]" % (k, l): v for k, v in w_.items()})
        controls += masked_loss_controls("v2", crops[l], moved[l], levels[l])
    assert len(controls) >= 2 * (len(wins) + 2) and min(r for _, r in controls) >= 100.0, controls
    assert len(wins) * (WIN // 2) ** 2 <= int(counts[0]) <= len(wins) * (WIN // 2 + 1) ** 2 and len(wins) <= int(counts[1]) <= 4 * len(wins)
    del gt_out, valid_out
    # the same validity by NaN: no mask, NaN outside the windows, on the same buffers
    for n in range(B):
        gt[n].masked_fill_((valid[n] == 0).unsqueeze(-1), float("nan"))
    losses_b, counts_b, grads_b = _masked_run(hip.LOSS_FLOW_MSE_V2, gt, preds, None, 7.0)
    assert torch.equal(losses_b, losses) and torch.equal(counts_b, counts)
    for l in range(len(levels)):
        assert all(torch.equal(grads_b[l][n], grads[l][n]) for n in range(B)), l
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("masked loss tile: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}, controls {:.0f} .. {:.0f} bounds".format(
        peak / GIB, planned / GIB, secs, worst, min(r for _, r in controls), max(r for _, r in controls)))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


def test_masked_loss_pixel_paths(arena):
    """masked_loss_pixel_kernel at 1.075 G pixels with one full-resolution level: the area walk (FlowMseLossV2, 1 x 1
    blocks) and the bilinear walk with renormalised corners (FlowMseLoss; the sample points are the pixel centres), the
    mask read by pixel index past 2^30 bytes, valid_out written there, and masked_loss_bwd_kernel's scalar form at
    2.15 G elements (no multiple of 4).  The window oracle of test_masked_loss_tile_path.
    Measured: peak 33.06 GiB (planned 34.06), 0.1 s; of the bound, losses 0.0016, grad_pred 0.012; gt_out exact."""
    key = CASES["masked_loss_pixel"]
    B, H, W, C = key
    hip = ops._hip
    planned = masked_loss_planned_bytes(key, [(H, W)], 3)
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(19)
    a = arena
    a["gt"] = gt = _fill_grid(torch.empty((B, H, W, C), device=DEV), gen)
    assert B * H * W > 1 << 30 and gt.numel() > 1 << 31 and gt.numel() % 4 == 2
    a["valid"] = valid = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    wins = masked_loss_windows(key)
    for _, n, y0, y1, x0, x1 in wins:
        valid[n, y0:y1, x0:x1] = 1
    a["pred"] = pred = _fill_grid(torch.empty((B, H, W, C), device=DEV), gen)
    crops = _masked_level_crops(gt, valid, pred, wins, (1, 1), 1.0)
    assert all(bool(m.all()) for _, m, _ in crops)
    moved = []
    for k, reg in enumerate(wins):
        for mod, at in wrapped_pixel_regions(B, H, W, C, reg):
            moved.append(("window %d (%s) gt read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k, _cut(gt, *at).double()))
        for mod, at in wrapped_pixel_regions(B, H, W, 1, reg, 1):
            assert not _cut3(valid, *at).any(), (reg, mod, at)
    worst = {}
    for name, kind_id, kind in (("masked v2 pixel", hip.LOSS_FLOW_MSE_V2, "v2"), ("masked bilinear", hip.LOSS_FLOW_MSE, "norm")):
        assert ops.masked_loss_kernel(kind_id, B, H, W, [(H, W)]) == "masked_loss_pixel_kernel"
        losses, counts, grads = _masked_run(kind_id, gt, [pred], valid, 7.0)
        assert grads[0].numel() % 4 != 0                                      # masked_loss_bwd_kernel's scalar form
        w_ = _check_masked_level(name, crops, wins, (1, 1), (H, W), losses[0], counts[0], grads[0], None, None, kind, 7.0)
        del grads
        _, _, _, gt_out, valid_out = ops.masked_loss_fwd(kind_id, gt, None, valid, p0=LOSS_DELTA, want_gt=True,
                                                         want_valid=True, shapes=[(H, W)])
        for r, (gl, m, _) in zip(wins, crops):
            assert torch.equal(_cut(gt_out[0], *r[1:]).double(), gl) and torch.equal(_cut3(valid_out[0], *r[1:]) != 0, m)
        assert _nonzero(valid_out[0]) == int(counts[0]) == len(wins) * WIN * WIN
        assert sum(int(torch.count_nonzero(_cut(gt_out[0], *r[1:]))) for r in wins) == _nonzero(gt_out[0])
        del gt_out, valid_out
        worst.update({"%s %s" % (name, k): v for k, v in w_.items()})
        controls = masked_loss_controls(kind, crops, moved, (H, W))
        assert len(controls) >= len(wins) + 2 and min(r for _, r in controls) >= 100.0, controls
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("masked loss pixel: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}, controls {:.0f} .. {:.0f} bounds".format(
        peak / GIB, planned / GIB, secs, worst, min(r for _, r in controls), max(r for _, r in controls)))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- flow metrics: truth and prediction past 2^31 elements, the masks past 2^30 bytes --------------------------------
# Per-image figures, so both oracles apply.  (a): an image of the batched launch is the image run alone bit for bit (which
# lane sums which pixel depends on the position inside the image only), and the state is that of the B calls in order;
# one image stays under 2^29 floats.  (c): the prediction equals the truth outside planted windows and the truth there is
# slower than 6 px, so a valid pixel outside the windows has e = 0, angle 0, and falls into the first speed bin: the 15
# sums follow in float64 from the windows' crops and from the masks' counts (torch.count_nonzero, an image at a time).
# The windows' flows come from seeds on the CPU (flow_window_data), so that tests/test_large_offsets_cpu.py can hold
# them away from every threshold.  Bounds: tests/test_flow_quality_cpu.py's (count ratios 1 ulp, means 1e-4 px, aae 1e-3
# degrees) and, since a mean over 150 M pixels of a few hundred non-zero terms is far below those, LOSS_REL relative on
# every mean and on the state's sums, which are such sums.
def flow_window_data(k, half=False):
    """(truth, pred) of window k, numpy (1,WIN,WIN,2): a full period of a 45 px wave (all three speed bins) plus texture,
    the prediction 0.3 px (even k) or 4 px (odd k) off, in fp32 or fp16 values; no pixel within MARGIN of a threshold."""
    t, p = make_flows(300 + k, (WIN, WIN), sigmas=((0.3, 4.0)[k % 2],), amplitude=(45.0,), batch=1)
    return away_from_thresholds(t, p, np.float16 if half else np.float32)


def flow_window_oracle(B, pixels, planted, n_valid, n_occ):
    """float64 (scores {field: [B]}, sums [B, 15]) of a batch whose prediction equals its slow (< 10 px) truth outside
    the windows: planted = [(image, truth, pred, valid, occluded)] crops, n_valid / n_occ [B] the images' counts of
    valid and of valid occluded pixels."""
    sums = np.zeros((B, 15))
    for n, t, p, v, o in planted:
        sums[n] += ref_sums(t, p, v, o)[0]
    rest, rest_occ = np.asarray(n_valid, np.float64) - sums[:, 0], np.asarray(n_occ, np.float64) - sums[:, 7]
    assert (rest >= 0).all() and (rest_occ >= 0).all()
    for i in (0, 4, 5, 6, 9):                     # valid; e < each accuracy threshold; the first speed bin
        sums[:, i] += rest
    sums[:, 7] += rest_occ
    return ref_scores(sums, pixels), sums


def flow_controls(B, pixels, planted, moved, n_valid, n_occ):
    """[(what, |change of its image's epe| / LOSS_REL of it)]: every window left out in turn (the prediction is the truth
    there); every moved = (what, window index, the truth as a wrapped offset finds it) in its window's place."""
    ref = flow_window_oracle(B, pixels, planted, n_valid, n_occ)[0]["epe"]
    out = []
    for k, (n, t, p, v, o) in enumerate(planted):
        alt = flow_window_oracle(B, pixels, planted[:k] + [(n, t, t, v, o)] + planted[k + 1:], n_valid, n_occ)[0]["epe"]
        out.append(("without window %d" % k, abs(alt[n] - ref[n]) / (LOSS_REL * ref[n])))
    for what, k, t2 in moved:
        n, t, p, v, o = planted[k]
        alt = flow_window_oracle(B, pixels, planted[:k] + [(n, t2, p, v, o)] + planted[k + 1:], n_valid, n_occ)[0]["epe"]
        out.append((what, abs(alt[n] - ref[n]) / (LOSS_REL * ref[n])))
    return out


def flow_quality_planned_bytes(key):
    """The fuller of the two phases: the channels-last run (truth, fp32 prediction, two masks) and the change of layout
    (truth in both layouts, the fp16 prediction, two masks)."""
    B, H, W, C = key
    flow = 4 * B * H * W * C
    return max(2 * flow, 2 * flow + flow // 2) + 2 * B * H * W


def _check_flow_scores(what, got, want):
    """check()'s bounds, and LOSS_REL relative on every mean (a mean that is 0 in float64 must be 0)."""
    err = check(what, got, want)
    worst = 0.0
    for k in EPE_FIELDS + ("aae",):
        g, w = getattr(got, k).double().cpu().numpy(), want[k]
        keep = ~np.isnan(w)
        assert (np.abs(g[keep] - w[keep]) <= LOSS_REL * np.abs(w[keep])).all(), (what, k, g, w)
        nz = keep & (w != 0)
        worst = max([worst] + list(np.abs(g[nz] - w[nz]) / np.abs(w[nz])))
    return worst, max(err[k] for k in COUNT_FIELDS)


def _flow_run(truth, pred, valid, occluded, data_format):
    """The batched launch with a state, then image by image on another state -> (scores, state); asserts oracle (a)."""
    B = truth.shape[0]
    state, one_state = (torch.zeros(17, dtype=torch.float64, device=DEV) for _ in range(2))
    res = metrics.flow_quality(truth, pred, valid=valid, occluded=occluded, data_format=data_format, state=state)
    for n in range(B):
        s = slice(n, n + 1)
        one = metrics.flow_quality(truth[s], pred[s], valid=valid[s], occluded=occluded[s], data_format=data_format,
                                   state=one_state)
        assert all(torch.equal(a[s].view(torch.int32), b.view(torch.int32)) for a, b in zip(res, one)), n
    assert torch.equal(state, one_state), (state - one_state).tolist()
    return res, state


def test_flow_quality(arena):
    """flow_quality_tile_kernel / flow_quality_fold_kernel at 1.074 G pixels in five images: `img + p` of truth and of an
    fp32 prediction passes 2^29, 2^30 and 2^31 elements (as float2: byte 2^31 and 2^32 of an 8-byte pixel at pixel 2^28
    and 2^29), the masks' 2^29 and 2^30 bytes; then channels-first with an fp16 prediction, where `2 * img + p + hw`,
    the v plane, passes 2^31 in the last image.  Oracles (a) and (c) above, 52,449 chunks an image (820 trips of the fold's lanes).
    Measured: peak 22.01 GiB (planned 22.01), 2.1 s; the means 2.7e-7 relative (0.027 of LOSS_REL), 1.7e-7 px (0.002 of
    the 1e-4 bound), aae 3.5e-13 degrees, count ratios at most 0.50 ulp; the controls moved an image's epe by 7100 .. 100000
    bounds."""
    key = CASES["flow_quality"]
    B, H, W, C = key
    planned = flow_quality_planned_bytes(key)
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(20)
    a = arena
    assert ops.flow_quality_kernel(B, H, W) == "flow_quality_tile_kernel"
    a["truth"] = truth = _fill_grid(torch.empty((B, H, W, C), device=DEV), gen, lim=64)        # |u|, |v| <= 4: m < 6
    assert truth.numel() > 1 << 31 and H * W * C < 1 << 29
    a["valid"] = valid = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    a["occluded"] = occluded = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    for n in range(B):
        valid[n].random_(0, 10, generator=gen).lt_(7)                      # 70 % valid, 30 % occluded, independent
        occluded[n].random_(0, 10, generator=gen).lt_(3)
    wins = pixel_windows(B, H, W, C)
    assert all(x[1:] in {y[1:] for y in wins} for x in pixel_windows(B, H, W, 1))       # the masks' boundaries: the same places
    n_valid = [int(torch.count_nonzero(valid[n])) for n in range(B)]
    n_occ = [int(torch.count_nonzero(valid[n] & occluded[n])) for n in range(B)]
    a["pred"] = pred = truth.clone()
    worst = {}

    def plant(half, channels_first):
        """The windows' flows into truth and the prediction at hand -> (planted, moved)."""
        planted, moved = [], []
        for k, reg in enumerate(wins):
            n, y0, y1, x0, x1 = reg[1:]
            for mod, at in ([] if channels_first else wrapped_pixel_regions(B, H, W, C, reg)):
                moved.append(("window %d (%s) truth read mod 2^%d bytes" % (k, reg[0], mod.bit_length() - 1), k,
                              _cut(a["truth"], *at).numpy()))
            t, p = flow_window_data(k, half)
            for name, crop in (("truth", t), ("pred", p)):
                crop = torch.from_numpy(crop[0]).to(DEV)
                if channels_first:
                    a[name][n, :, y0:y1, x0:x1] = crop.permute(2, 0, 1)
                else:
                    a[name][n, y0:y1, x0:x1, :] = crop
            planted.append((n, t, p, _cut3(valid, *reg[1:]).numpy(), _cut3(occluded, *reg[1:]).numpy()))
        return planted, moved

    for tag, half, fmt in (("f32 channels_last", False, "channels_last"), ("f16 channels_first", True, "channels_first")):
        if half:
            a["pred"] = pred = torch.empty((B, C, H, W), dtype=torch.float16, device=DEV).copy_(truth.permute(0, 3, 1, 2))
            a["truth"] = truth = truth.permute(0, 3, 1, 2).contiguous()        # the old layouts are released here
            assert truth.shape == (B, C, H, W) and truth.numel() > 1 << 31           # `o + hw` of the last image's v plane
        planted, moved = plant(half, half)
        res, state = _flow_run(truth, pred, valid, occluded, fmt)
        want, sums = flow_window_oracle(B, H * W, planted, n_valid, n_occ)
        worst[tag] = _check_flow_scores("hip large " + tag, res, want)
        total, st = sums.sum(axis=0), state.cpu().numpy()
        assert st[15] == B and st[16] == float(B) * H * W
        for i in range(15):
            if i in (1, 2, 8, 10, 12, 14):
                assert abs(st[i] - total[i]) <= LOSS_REL * total[i], (tag, i, st[i], total[i])
            else:
                assert st[i] == total[i], (tag, i, st[i], total[i])               # counts
        assert float(res.epe[3]) == 0.0 and float(res.acc1[3]) == 1.0 and float(res.aae[3]) == 0.0    # no window in image 3
        controls = flow_controls(B, H * W, planted, moved, n_valid, n_occ)
        assert len(controls) >= len(wins) + (0 if half else 2) and min(r for _, r in controls) >= 100.0, controls
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("flow quality: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst (relative mean, count ulp) {}, controls {:.0f} .. "
          "{:.0f} bounds".format(peak / GIB, planned / GIB, secs, worst, min(r for _, r in controls), max(r for _, r in controls)))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- the label-free losses: frames past 2^31 elements, the saved planes past 2^32, the mask past 2^29 bytes ----------
# unsup_loss_fwd_kernel / unsup_loss_bwd_kernel index the frames by ((b*h+y)*w+x)*3, the flow by pixel * 2, the mask by
# pixel and the seven saved planes by k * (B*h*w) + pixel.  The background is trivial -- prv = nxt = one colour, flow 0,
# everything occluded -- so the float64 answer needs crops only: around WIN x WIN windows (textured frames, make_case's
# flows on the 1/16 grid up to UNSUP_REACH pixels, its 20 % mask) the frames are textured UNSUP_MARGIN = 4 + UNSUP_REACH
# pixels further (3 for the census patch, 1 for the second tap, the reach of a sample), and the crop is one pixel wider,
# so that every pair of neighbours outside all crops is a background pair: weight 1, difference 0, term smooth_eps, which
# at 2^-20 the kernel sums exactly.  The crops' own terms are the float64 chain's on each crop -- a window pixel's
# sample, patch and neighbours lie inside its crop, or outside the image where the crop ends at the image's border --
# rescaled from the crop's count and pairs to the whole level's.
UNSUP_REACH = 9                                  # make_case(WIN, WIN): flows up to w / 2, an integer moved by 1/2
UNSUP_MARGIN = 4 + UNSUP_REACH
UNSUP_COLOUR = 0.25
UNSUP_PARAMS = dict(q=0.4, eps=0.01, smooth_weight=1.5, edge=40.0, smooth_eps=2.0 ** -20)


def unsup_windows(key):
    """[(tag, n, y0, y1, x0, x1)]: pixel_windows of the frames (3 floats a pixel), and behind the pixel under every
    boundary of the flow (2 a pixel), of the mask (a byte a pixel) and of the saved planes (plane k at k * B*H*W + pixel,
    boundaries up to 2^32); one entry per distinct place."""
    B, H, W = key
    wins = pixel_windows(B, H, W, 3)
    more = [("flow" + x[0],) + x[1:] for x in pixel_windows(B, H, W, 2)[1:-1]]
    more += [("mask" + x[0],) + x[1:] for x in pixel_windows(B, H, W, 1)[1:-1]]
    npix = B * H * W
    for b in crossed(7 * npix, BOUNDARIES_32):
        plane, pix = divmod(b, npix)
        n, y, x = locate(pix, H, W, 1)
        assert y + 1 + WIN <= H, (b, y)
        more.append(("plane%d>2^%d" % (plane, b.bit_length() - 1), n, y + 1, y + 1 + WIN) + _span(x, WIN, W))
    seen = {x[1:] for x in wins}
    for x in more:
        if x[1:] not in seen:
            seen.add(x[1:])
            wins.insert(-1, x)
    return wins


def unsup_grown(win, by, H, W):
    """The window grown by `by` pixels on every side, cut at the image -> (tag, n, y0, y1, x0, x1)."""
    tag, n, y0, y1, x0, x1 = win
    return (tag, n, max(y0 - by, 0), min(y1 + by, H), max(x0 - by, 0), min(x1 + by, W))


def unsup_plant(k, win, key):
    """What window k holds, on the CPU: textured frames on the window grown by UNSUP_MARGIN, make_case's flow and mask
    on the window -> {"textured": region, "crop": region, "prv", "nxt" (1,ph,pw,3), "flow" (1,WIN,WIN,2), "occ"}."""
    from test_unsup_loss_cpu import make_case
    B, H, W = key
    tex, side = unsup_grown(win, UNSUP_MARGIN, H, W), WIN + 2 * UNSUP_MARGIN
    # every window its own contrast ((k + 2) / 16) and, every other one, its axes swapped: a wrapped offset that finds
    # another window's frames must not find the like of its own
    pairs = torch.from_numpy(make_case(side, side, 200 + k, B=1, levels=1)["pairs"]) * ((k + 2) / 16.0)
    pairs = pairs.transpose(1, 2) if k % 2 else pairs
    oy, ox = tex[2] - (win[2] - UNSUP_MARGIN), tex[4] - (win[4] - UNSUP_MARGIN)
    pairs = pairs[:, oy:oy + tex[3] - tex[2], ox:ox + tex[5] - tex[4]]
    small = make_case(WIN, WIN, 300 + k, B=1, levels=1)
    flow = torch.from_numpy(small["flows"][0])
    assert float(flow.abs().max()) <= UNSUP_REACH
    return {"textured": tex, "crop": unsup_grown(win, UNSUP_MARGIN + 1, H, W), "prv": pairs[..., :3].contiguous(),
            "nxt": pairs[..., 3:].contiguous(), "flow": flow, "occ": torch.from_numpy(small["masks"][0])}


def unsup_fill(prv, nxt, flow, occ, wins, plants):
    """The windows' contents into the full-size tensors (on any device)."""
    for win, p in zip(wins, plants):
        _, n, y0, y1, x0, x1 = p["textured"]
        prv[n, y0:y1, x0:x1] = p["prv"][0].to(prv.device)
        nxt[n, y0:y1, x0:x1] = p["nxt"][0].to(prv.device)
        _, n, y0, y1, x0, x1 = win
        flow[n, y0:y1, x0:x1] = p["flow"][0].to(prv.device)
        occ[n, y0:y1, x0:x1] = p["occ"][0].to(prv.device)


def unsup_cut(prv, nxt, flow, occ, reg, frames_at=None):
    """One crop of the four tensors on the CPU; frames_at = (n, y0, y1, x0, x1): the frames read there instead."""
    at = reg[1:] if frames_at is None else frames_at
    return {"prv": _cut(prv, *at), "nxt": _cut(nxt, *at), "flow": _cut(flow, *reg[1:]), "occ": _cut3(occ, *reg[1:])}


def unsup_window_ref(kind, crops, key, dtype, params=UNSUP_PARAMS):
    """The level's photometric value, smoothness, count and gradient from the crops alone, in `dtype`:
    photo = sum_c photo_c count_c / count, sx = (the crops' pair terms + 2 smooth_eps per background pair) over the
    header's normaliser 2 B h (w - 1), sy alike -> (photo, smooth, count, [d loss / d flow of each crop], the crops'
    share of the smoothness sum)."""
    from qpwcnet_amd import loss
    B, H, W = key
    nx, ny = B * H * (W - 1), B * (H - 1) * W
    eps_s, edge, sw = params["smooth_eps"], params["edge"], params["smooth_weight"]
    obj = loss.PhotometricLoss(kind, q=params["q"], eps=params["eps"], smooth_weight=0.0, edge=edge, smooth_eps=eps_s,
                               data_format="channels_last")
    xs, photo, count, sx, sy, px, py = [], 0.0, 0, 0.0, 0.0, 0, 0
    for c in crops:
        x = c["flow"].detach().to(dtype).clone().requires_grad_()
        prv = c["prv"].to(dtype)
        _, per, parts = loss.multiscale_unsupervised_torch(obj, torch.cat([prv, c["nxt"].to(dtype)], dim=3), [x], [c["occ"]])
        n_c = int(parts["counts"][0])
        photo, count = photo + per[0] * n_c, count + n_c
        robust = lambda d: torch.sqrt(d * d + eps_s ** 2)
        wx = torch.exp(-edge * (prv[:, :, 1:] - prv[:, :, :-1]).abs().mean(-1))
        wy = torch.exp(-edge * (prv[:, 1:] - prv[:, :-1]).abs().mean(-1))
        sx = sx + (wx[..., None] * robust(x[:, :, 1:] - x[:, :, :-1])).sum()
        sy = sy + (wy[..., None] * robust(x[:, 1:] - x[:, :-1])).sum()
        px, py = px + wx.numel(), py + wy.numel()
        xs.append(x)
    photo = photo / max(count, 1)
    back = 0.5 * (2.0 * (nx - px) * eps_s / (2.0 * nx) + 2.0 * (ny - py) * eps_s / (2.0 * ny))
    smooth = 0.5 * (sx / (2.0 * nx) + sy / (2.0 * ny)) + back
    (photo + sw * smooth).backward()
    return (photo.detach().double(), smooth.detach().double(), count, [x.grad.double() for x in xs],
            1.0 - back / float(smooth.detach()))


def unsup_bounds(ref, ref32):
    """The module's rule at its definition: 4 x |float32 chain - float64 chain| on the same crops, never below 1e-5 --
    relative for the values, of the largest gradient for the gradients -> {"photo", "smooth", "grad"}."""
    top = max(float(g.abs().max()) for g in ref[3])
    err = max(float((a - b).abs().max()) for a, b in zip(ref[3], ref32[3]))
    return {"photo": max(4.0 * abs(float(ref[0] - ref32[0])), 1e-5 * abs(float(ref[0]))),
            "smooth": max(4.0 * abs(float(ref[1] - ref32[1])), 1e-5 * abs(float(ref[1]))),
            "grad": max(4.0 * err, 1e-5 * top)}


def unsup_planned_bytes(key):
    """Both frames, the flow, its gradient, the mask, and the workspace: 4 floats a tile and 7 planes."""
    B, H, W = key
    npix, tiles = B * H * W, B * -(-H // 8) * -(-W // 32)
    return 4 * (2 * 3 * npix + 2 * 2 * npix + 7 * npix + 4 * tiles) + npix


def _unsup_run(kind_id, prv, nxt, flow, occ):
    p = UNSUP_PARAMS
    x = flow.detach().requires_grad_()
    losses, photo, smooth, counts = ops.unsup_loss(kind_id, [prv], [nxt], [x], [occ], "channels_last", p["q"], p["eps"],
                                                   p["smooth_weight"], p["edge"], p["smooth_eps"])
    losses.sum().backward()
    return losses.detach(), photo, smooth, counts, x.grad


def test_unsup_loss(arena):
    """The census loss, forward and backward, at 3 x 15489 x 15497 pixels: the frames' element index passes 2^29, 2^30 and
    2^31 in images 0, 1 and 2, the flow's 2^29 and 2^30, the mask's byte index 2^29, the saved planes' 2^29 .. 2^32.
    count, the photometric value, the smoothness and grad_flow against float64 from the windows' crops; grad_flow
    exactly 0 outside the crops over the whole tensor; a second launch gives the same bits; a window's frames read at
    their offset wrapped mod 2^31 / 2^32 bytes and elements must move the photometric value by 100 bounds.
    Measured: peak 46.32 GiB (planned 46.32), 1.5 s; of the bounds, photometric 0.0005, smoothness 0.0013, grad_flow 0.24;
    the controls moved the photometric value by 185 .. 10500 bounds."""
    key = CASES["unsup_loss"]
    B, H, W = key
    hip = ops._hip
    planned = unsup_planned_bytes(key)
    t0 = time.perf_counter()
    a = arena
    a["prv"] = prv = torch.full((B, H, W, 3), UNSUP_COLOUR, device=DEV)
    a["nxt"] = nxt = torch.full((B, H, W, 3), UNSUP_COLOUR, device=DEV)
    a["flow"] = flow = torch.zeros((B, H, W, 2), device=DEV)
    a["occ"] = occ = torch.ones((B, H, W), dtype=torch.uint8, device=DEV)
    assert prv.numel() > 1 << 31 and 7 * B * H * W > 1 << 32 and occ.numel() > 1 << 29
    wins = unsup_windows(key)
    plants = [unsup_plant(k, win, key) for k, win in enumerate(wins)]
    unsup_fill(prv, nxt, flow, occ, wins, plants)
    regs = [p["crop"] for p in plants]
    crops = [unsup_cut(prv, nxt, flow, occ, r) for r in regs]
    ref = unsup_window_ref("census", crops, key, torch.float64)
    bounds = unsup_bounds(ref, unsup_window_ref("census", crops, key, torch.float32))
    photo64, smooth64, count64, grads64, share = ref
    assert count64 > 50 * len(wins) and share > 0.5, (count64, share)

    losses, photo, smooth, counts, grad = _unsup_run(hip.UNSUP_CENSUS, prv, nxt, flow, occ)
    assert int(counts[0]) == count64, (int(counts[0]), count64)
    worst = {}
    for name, got, want in (("photo", photo[0], photo64), ("smooth", smooth[0], smooth64),
                            ("loss", losses[0], photo64 + UNSUP_PARAMS["smooth_weight"] * smooth64)):
        d, bound = abs(float(got) - float(want)), bounds["photo"] + UNSUP_PARAMS["smooth_weight"] * bounds["smooth"] \
            if name == "loss" else bounds[name]
        print("unsup {}: {:.9e} against {:.9e}, |d| = {:.3e}, bound {:.3e}".format(name, float(got), float(want), d, bound))
        assert d <= bound, (name, float(got), float(want), bound)
        worst[name] = d / bound
    kept, inside = [], 0
    for r, g in zip(regs, grads64):
        got = _cut(grad, *r[1:])
        d = float((got.double() - g).abs().max())
        print("unsup grad_flow {}: max|d| = {:.3e}, bound {:.3e}".format(r[0], d, bounds["grad"]))
        assert d <= bounds["grad"], (r[0], d, bounds["grad"])
        worst["grad"] = max(worst.get("grad", 0.0), d / bounds["grad"])
        assert got.any(), r[0]
        inside += int(torch.count_nonzero(got))
        kept.append(got)
    assert 0 < inside == _nonzero(grad), inside                                   # exactly 0 outside the crops
    first = (losses, photo, smooth, counts)
    del grad, losses, photo, smooth, counts

    # the same bits again: zero outside the crops both times, so the crops decide
    again = _unsup_run(hip.UNSUP_CENSUS, prv, nxt, flow, occ)
    assert all(torch.equal(x, y) for x, y in zip(first, again[:4]))
    assert all(torch.equal(_cut(again[4], *r[1:]), g) for r, g in zip(regs, kept)) and _nonzero(again[4]) == inside
    del again

    # the negative control, on the device's own data: a window's frames as a wrapped offset finds them
    controls = []
    for k, r in enumerate(regs):
        for elem_bytes in (4, 1):                          # byte offsets mod 2^31, 2^32; element offsets mod 2^31, 2^32
            for mod, at in wrapped_pixel_regions(B, H, W, 3, r, elem_bytes):
                alt = crops[:k] + [unsup_cut(prv, nxt, flow, occ, r, frames_at=at)] + crops[k + 1:]
                moved = abs(float(unsup_window_ref("census", alt, key, torch.float64)[0] - photo64)) / bounds["photo"]
                controls.append(("window %d (%s) frames read mod 2^%d %s" % (
                    k, r[0], mod.bit_length() - 1, "bytes" if elem_bytes == 4 else "elements"), moved))
    assert len(controls) >= len(wins) and min(m for _, m in controls) >= 100.0, controls
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("unsup_loss: {} windows, count {}, the crops' share of the smoothness {:.3f}, peak {:.2f} GiB, planned {:.2f} "
          "GiB, {:.2f} s, worst/bound {}, bounds {}, controls {:.0f} .. {:.0f} bounds".format(
              len(wins), count64, share, peak / GIB, planned / GIB, secs, worst, bounds, min(m for _, m in controls),
              max(m for _, m in controls)))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- the input pipelines: source pixels past 2^29, 2^30 and 2^31 -------------------------------------------------------
# aug_pixel_pass reads four source pixels p00 .. p11 = b * H * W + y * W + x per output pixel: the frames at 6 bytes a
# pixel, the flow as a float2, the mask as a byte.  Only the 64 x 64 output window of each sample is computed, so the
# oracle needs the source pixels under it: ref_augment / ref_augment_sparse on that crop as an image of its own, the
# window's offsets shifted.  The scale is 2 (rh = 2 H, rw = 2 W): the fp32 source coordinate (i + 0.5) * 0.5 - 0.5 is
# then exact at any i below 2^22, the weights are 0.25 and 0.75, and the crop's coordinates differ from the image's by
# an integer -- at a ratio that fp32 rounds, a coordinate near 26000 would be good to 2e-3 pixels only.
AUG_OUT = (64, 64)
AUG_PAD = 2                                      # source pixels kept around those the window reads


def augment_placement(key, boundaries=BOUNDARIES):
    """Per sample n the window across the pixel that holds boundary n of the pixel index (2^29, 2^30, 2^31), each with
    another flip pair -> [{"pixel": (n, y, x), "ip": the sample's iparams row, "src": (n, r0, r1, c0, c1) the source
    pixels kept, "crop_ip": the iparams of the same window on that crop alone}]."""
    import math
    B, H, W = key
    h, w = AUG_OUT
    out = []
    for n, (b, (ud, lr)) in enumerate(zip(boundaries, ((0, 1), (1, 0), (1, 1)))):
        m, y, x = locate(b, H, W, 1)
        assert m == n, (b, m)
        ax = []
        for size, at, flip, extent in ((H, y, ud, h), (W, x, lr, w)):
            f = size - 1 - at if flip else at                 # the boundary pixel as the flipped image counts it
            o = 2 * f - extent // 2                           # the window's middle lies on it
            lo = math.floor((o + 0.5) * 0.5 - 0.5) - AUG_PAD
            hi = math.ceil((o + extent - 0.5) * 0.5 - 0.5) + AUG_PAD + 1
            assert 0 <= lo and hi <= size and 0 <= o <= 2 * size - extent, (n, o, lo, hi)
            ax.append((o, lo, hi, (size - hi, size - lo) if flip else (lo, hi)))
        (oy, ly, hy, (r0, r1)), (ox, lx, hx, (c0, c1)) = ax
        out.append({"pixel": (n, y, x), "ip": (2 * H, 2 * W, oy, ox, ud, lr), "src": (n, r0, r1, c0, c1),
                    "crop_ip": (2 * (hy - ly), 2 * (hx - lx), oy - 2 * ly, ox - 2 * lx, ud, lr)})
    return out


AUG_FPARAMS = ((0.05, 1.2, 0.1, 0.8), (-0.1, 0.7, -0.1, 1.3), (0.12, 1.0, 0.19, 0.55))   # brightness, saturation, hue, contrast


def augment_fparams(places):
    """(B, 6) float32: the flow multipliers of scale 2 with the flips' signs, and colour parameters of the small suite."""
    return np.array([(2.0 * (1 - 2 * p["ip"][5]), 2.0 * (1 - 2 * p["ip"][4])) + c for p, c in zip(places, AUG_FPARAMS)],
                    np.float32)


def augment_source(n, place):
    """The source pixels of one window: random uint8 frames, a smooth flow of up to 32 px, a half-density mask."""
    from test_augment_cpu import smooth_flow
    _, r0, r1, c0, c1 = place["src"]
    rng = np.random.default_rng(400 + n)
    return (rng.integers(0, 256, (1, r1 - r0, c1 - c0, 6), dtype=np.uint8), smooth_flow(1, r1 - r0, c1 - c0, seed=n),
            (rng.random((1, r1 - r0, c1 - c0)) < 0.5).astype(np.uint8))


def augment_window_ref(place, ims, flo, valid, fp_row, colour):
    """Both restatements of one sample on its crop -> (ims, flo) dense and (ims, flo, valid) sparse, float64."""
    from test_augment_cpu import ref_augment
    from test_sparse_augment_cpu import ref_augment_sparse
    ip = np.array([place["crop_ip"]], np.int32)
    fp = np.asarray(fp_row, np.float32).reshape(1, 6)
    return (ref_augment(ims, flo, ip, fp, AUG_OUT, colour=colour),
            ref_augment_sparse(ims, flo, valid, ip, fp, AUG_OUT, colour=colour))


def augment_planned_bytes(key):
    B, H, W = key
    return (6 + 8 + 1) * B * H * W


def test_augment(arena):
    """qpwc_augment_fwd and qpwc_augment_sparse_fwd on uint8 frames at 3 x 26833 x 26839 source pixels: p00 .. p11 pass
    2^29, 2^30 and 2^31 in samples 0, 1 and 2 (the mask's byte index, the flow's float2 index, the frames' 6-byte pixel
    index), each sample's 64 x 64 window lying across its boundary pixel under another flip pair.  Everything but the
    windows' sources is zero, the mask included.  Both restatements on the crops at BOUND, the mask equal in every
    pixel, with and without the colour stage; the sources read at the pixel index wrapped at the boundary move every
    output by 100 bounds.  Measured: peak 30.18 GiB (planned 30.18), 1.9 s; frames 4.5e-7, flow 3.8e-6 px, sparse flow
    7.6e-6 px against the bound of 1e-4; the controls moved every output by 6300 .. 11500 bounds."""
    from test_augment_cpu import BOUND
    key = CASES["augment"]
    B, H, W = key
    planned = augment_planned_bytes(key)
    t0 = time.perf_counter()
    a = arena
    a["ims"] = ims = torch.zeros((B, H, W, 6), dtype=torch.uint8, device=DEV)
    a["flo"] = flo = torch.zeros((B, H, W, 2), device=DEV)
    a["valid"] = valid = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    assert B * H * W > 1 << 31 and H * W < 1 << 30
    places = augment_placement(key)
    for n, p in enumerate(places):
        _, r0, r1, c0, c1 = p["src"]
        for t, crop in zip((ims, flo, valid), augment_source(n, p)):
            t[n, r0:r1, c0:c1] = torch.from_numpy(crop[0]).to(DEV)
    ip = torch.tensor([p["ip"] for p in places], dtype=torch.int32, device=DEV)
    fparams = augment_fparams(places)
    fp = torch.from_numpy(fparams).to(DEV)
    crops = [(_cut(ims, *p["src"]).numpy(), _cut(flo, *p["src"]).numpy(), _cut3(valid, *p["src"]).numpy()) for p in places]
    assert all(c[0].any() and c[2].any() and not c[2].all() for c in crops)
    worst, controls = {}, []
    for colour in (True, False):
        d_ims, d_flo = ops.augment(ims, flo, ip, fp, AUG_OUT, colour=colour)
        s_ims, s_flo, s_valid = ops.augment_sparse(ims, flo, valid, ip, fp, AUG_OUT, colour=colour)
        assert torch.equal(d_ims, s_ims) and s_valid.dtype == torch.uint8
        got = [t.cpu().numpy() for t in (d_ims, d_flo, s_flo, s_valid)]
        for n, (p, c) in enumerate(zip(places, crops)):
            (r_ims, r_flo), (q_ims, q_flo, q_valid) = augment_window_ref(p, c[0], c[1], c[2], fparams[n], colour)
            assert np.array_equal(got[3][n], q_valid[0]) and 0.5 < q_valid.mean() < 1.0, n
            assert not got[2][n][q_valid[0] == 0].any()
            errs = {"ims": np.abs(got[0][n] - r_ims[0]).max(), "flo": np.abs(got[1][n] - r_flo[0]).max(),
                    "sparse flo": np.abs(got[2][n] - q_flo[0]).max()}
            print("augment sample {} colour={}: {}".format(n, colour, {k: "%.2e" % v for k, v in errs.items()}))
            for k, v in errs.items():
                assert v <= BOUND, (n, colour, k, v)
                worst[k] = max(worst.get(k, 0.0), float(v))
            assert np.abs(r_flo[0]).max() > 8.0 and np.abs(r_ims[0]).max() > 0.25
            # the control: the source rows behind the boundary pixel as an index wrapped at the boundary finds them
            _, y, x = p["pixel"]
            _, r0, r1, c0, c1 = p["src"]
            m, yy, xx = locate((n * H + y + 1) * W + c0 - BOUNDARIES[n], H, W, 1)
            at = (m, yy, yy + r1 - y - 1, min(xx, W - (c1 - c0)), min(xx, W - (c1 - c0)) + c1 - c0)
            alt = [x_.copy() for x_ in c]
            for t, full, cut in zip(alt, (ims, flo, valid), (_cut, _cut, _cut3)):
                t[:, y + 1 - r0:] = cut(full, *at).numpy()
            (w_ims, w_flo), (_, v_flo, v_valid) = augment_window_ref(p, alt[0], alt[1], alt[2], fparams[n], colour)
            controls.append(min(np.abs(w_ims - r_ims).max(), np.abs(w_flo - r_flo).max(), np.abs(v_flo - q_flo).max()) / BOUND)
            assert not np.array_equal(v_valid, q_valid)
        del d_ims, d_flo, s_ims, s_flo, s_valid
    assert len(controls) == 2 * B and min(controls) >= 100.0, controls
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("augment: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}, controls {:.0f} .. {:.0f} bounds".format(
        peak / GIB, planned / GIB, secs, worst, min(controls), max(controls)))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- occlusion map and inverse flow: above 2^28 pixels (the stride loops iterate) and past 2^31 flow elements ------
# csrc/occlusion.hip launches min(ceil(pixels / 256), 2^20) workgroups of 256: one grid-stride trip covers 2^28 pixels.
# At 3 x 18917 x 18923 every launch makes five trips, the last of 157,349 pixels; the channels-last element index
# `idx * 2` passes 2^29, 2^30 and 2^31 in images 0, 1 and 2, the channels-first `b * 2 * plane + y * W + x` likewise
# (2^31 fp16 elements: 2^32 bytes), and the map's pixel index passes 2^29 and 2^30 (2^31 and 2^32 bytes).
#
# Both ops are bit-exact against the fp32 numpy restatement (tests/test_gpu_occlusion.py), so every comparison here is
# equality.  (a) per image against the launch on that image alone, and invert_flow against -tf_warp(flow, flow) of the
# warp kernel; (b) OCC_WIN x OCC_WIN windows against occ_restatement(), the fp32 chain of oracle.np_ref in the FULL
# image's coordinates: `(float)y + inv.y` at y near 18000 rounds to 2^-9 where the same window numbered from 0 would
# not, and the truncated target may differ by a pixel, so a crop handed to np_ref as an image of its own is no oracle;
# (c) the restatement fed the crop that an element index wrapped at 2^31 elements or 2^32 bytes finds differs from the
# right answer in every window behind that boundary.
#
# What is compared of a window: with |flow| <= F = 6 and weights in [0, 1] the inverse flow of a pixel lies within F,
# its truncated target within F + 1, and it reads flows within F + 1 of itself: a map pixel depends on flows within
# 2 F + 2, and pixels 2 F + 3 from a crop edge that is no image edge are compared.  The image's first rows and columns
# are different: a sample at -1 < x + fx < 0 truncates to corner 0 with the second corner 1 and weights 1 - xf and xf,
# an extrapolation of up to 3 F an axis and 9 F = 54 pixels over both, so a window that touches the image's top or left
# edge compares what lies OCC_EDGE_MARGIN = 64 >= 54 + 1 + F + 1 + 1 from its artificial edges.  Past the bottom and
# right edges both corners clip to the last pixel and the weights cancel.
#
# On paper: `int64_t idx` to `int idx` in invert_flow_kernel makes `idx += gridDim.x * blockDim.x` a 32-bit sum; from
# the fourth trip on it is 2^30 and more, and `idx * 2` as an int wraps at pixel 2^30: image 2 from there on is not
# written (or written 2^32 elements lower), so (a) fails for image 2 and (b) in the ">2^30 px" window and the corners
# behind it.  Without the loop's increment a lane runs one trip, pixels from 2^28 on keep what the allocation held: (a)
# fails for every image, (b) in every window.  A 32-bit `b * 2 * plane` in FlowField::at reads image 2's y plane 2^32
# elements lower; control (c) shows that other flows there change both results in every such window.
OCC_F = 6
OCC_WIN = 160
OCC_MARGIN = 2 * OCC_F + 3
OCC_EDGE_MARGIN = 64
OCC_TRIP = (1 << 20) * 256            # pixels of one grid-stride trip; the CPU companion reads both factors from the source


def occ_restatement(crop, origin, full, half=False):
    """oracle.np_ref.invert_flow and estimate_occlusion_map in fp32 on a crop (h, w, 2) of one image whose first pixel
    is `origin` = (y, x) of the `full` = (H, W) image: coordinates, clips and the out-of-bounds test are the full
    image's, gathers that leave the crop read its nearest pixel (what depends on them is not compared: see above).
    half: the inverse flow as fp16 storage holds it; the map is computed from the unrounded one, as the kernel does.
    -> (inverse flow (h, w, 2), map (h, w))."""
    f32 = np.float32
    crop = np.ascontiguousarray(crop, dtype=f32)
    h, w, _ = crop.shape
    (oy, ox), (H, W) = origin, full
    gy = (oy + np.arange(h)).astype(f32)[:, None]
    gx = (ox + np.arange(w)).astype(f32)[None, :]
    x, y = gx + crop[..., 0], gy + crop[..., 1]                       # warp.py:100-111
    x0, y0 = x.astype(np.int32), y.astype(np.int32)                   # :115-117, |x|, |y| < 2^15: no saturation here
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1)             # :121-124
    y0, y1 = np.clip(y0, 0, H - 1), np.clip(y1, 0, H - 1)
    at = lambda yy, xx: crop[np.clip(yy - oy, 0, h - 1), np.clip(xx - ox, 0, w - 1)]
    Ia, Ib, Ic, Id = at(y0, x0), at(y1, x0), at(y0, x1), at(y1, x1)   # :127-130
    x0f, x1f, y0f, y1f = (t.astype(f32) for t in (x0, x1, y0, y1))
    wa, wb = (x1f - x) * (y1f - y), (x1f - x) * (y - y0f)             # :139-142
    wc, wd = (x - x0f) * (y1f - y), (x - x0f) * (y - y0f)
    inv = -(wa[..., None] * Ia + wb[..., None] * Ib + wc[..., None] * Ic + wd[..., None] * Id)   # :151, occlusion.py:85
    assert inv.dtype == f32
    i2, j2 = gy + crop[..., 1], gx + crop[..., 0]                     # occlusion.py:60
    oob = ((i2 < 0) | (i2 >= H) | (j2 < 0) | (j2 >= W)).astype(f32)   # :74
    ti = np.clip((gy + inv[..., 1]).astype(np.int32), 0, H - 1) - oy  # :86-92
    tj = np.clip((gx + inv[..., 0]).astype(np.int32), 0, W - 1) - ox
    inside = (ti >= 0) & (ti < h) & (tj >= 0) & (tj < w)
    map3 = np.ones((h, w), f32)                                       # :94-95
    map3[ti[inside], tj[inside]] = 0.0
    return (inv.astype(np.float16).astype(f32) if half else inv), np.maximum(oob, map3)   # :98


def occ_pixels(key):
    """[(tag, n, y, x)]: the pixels that hold each boundary of the channels-last flow and inverse flow (two elements a
    pixel), of the map, of the channels-first planes (`b * 2 * plane + y * W + x`, the x plane's index), the first
    pixel of stride trips 2 and 4, and the four corners of the last image; one entry a pixel."""
    B, H, W = key
    plane = H * W
    out, seen = [], set()

    def add(tag, n, y, x):
        if (n, y, x) not in seen:
            seen.add((n, y, x))
            out.append((tag, n, y, x))
    for b in crossed(B * plane * 2):
        add("nhwc>2^%d" % (b.bit_length() - 1), *locate(b, H, W, 2))
    for b in crossed(B * plane):
        add("map>2^%d" % (b.bit_length() - 1), *locate(b, H, W, 1))
    for k in (1, 3):
        add("trip %d" % (k + 1), *locate(k * OCC_TRIP, H, W, 1))
    for b in crossed(B * plane * 2):
        add("nchw>2^%d" % (b.bit_length() - 1), b // plane // 2, b % plane // W, b % W)
    for tag, y, x in (("top left", 0, 0), ("top right", 0, W - 1), ("bottom left", H - 1, 0), ("bottom right", H - 1, W - 1)):
        add(tag, B - 1, y, x)
    return out


def occ_windows(key):
    """[(tag, n, y0, y1, x0, x1, (cy0, cy1, cx0, cx1))]: an OCC_WIN x OCC_WIN window around each pixel of occ_pixels()
    and the part of it, in window coordinates, that is compared."""
    B, H, W = key
    wins = []
    for tag, n, y, x in occ_pixels(key):
        (y0, y1), (x0, x1) = _span(y, OCC_WIN, H), _span(x, OCC_WIN, W)
        m = OCC_EDGE_MARGIN if y0 == 0 or x0 == 0 else OCC_MARGIN
        cmp_ = (0 if y0 == 0 else m, OCC_WIN - (0 if y1 == H else m), 0 if x0 == 0 else m, OCC_WIN - (0 if x1 == W else m))
        wins.append((tag, n, y0, y1, x0, x1, cmp_))
    return wins


def occ_element_index(key, win, layout):
    """(h, w, 2) int64: the element index of every flow value of a window, `idx * 2 + c` (channels-last) or
    `b * 2 * plane + y * W + x + c * plane` (channels-first), as FlowField::at forms it."""
    B, H, W = key
    _, n, y0, y1, x0, x1 = win[:6]
    yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.int64)
    if layout == "channels_last":
        base = ((n * H + yy) * W + xx) * 2
        return np.stack([base, base + 1], -1)
    base = n * 2 * H * W + yy * W + xx
    return np.stack([base, base + H * W], -1)


def occ_wrapped(key, win, layout, esize):
    """What a narrow index would read: [(modulus in elements, mask (h, w, 2) of the window's flow values whose element
    index reaches it, their indices wrapped)] for 2^31 elements and 2^32 bytes, where the window reaches them."""
    idx = occ_element_index(key, win, layout)
    out = []
    for mod in sorted({1 << 31, (1 << 32) // esize}):
        mask = idx >= mod
        if mask.any():
            out.append((mod, mask, idx[mask] % mod))
    return out


def occlusion_planned_bytes(key):
    """The fp32 flow, its inverse and the map of the big launches; beside them the inverse flow of one image and the
    warp kernel's, negated in place."""
    B, H, W = key
    return (8 + 8 + 4) * B * H * W + 2 * 8 * H * W


def _occ_cut(t, layout, n, y0, x0):
    """An OCC_WIN x OCC_WIN crop (h, w, 2) of a flow tensor as fp32 on the host (fp16 -> fp32 is exact)."""
    if layout == "channels_last":
        return t[n, y0:y0 + OCC_WIN, x0:x0 + OCC_WIN, :].float().cpu().numpy()
    return t[n, :, y0:y0 + OCC_WIN, x0:x0 + OCC_WIN].permute(1, 2, 0).float().cpu().numpy()


def _occ_check(key, flow, inv, occ, layout, what, stats):
    """Oracles (a), (b) and (c) of one layout and dtype on the big launch's results."""
    from qpwcnet_amd import warp
    B, H, W = key
    half = flow.dtype == torch.float16
    for n in range(B):
        one = ops.invert_flow(flow[n:n + 1], layout)
        assert torch.equal(one, inv[n:n + 1]), "%s: inverse flow of image %d" % (what, n)
        w_ = warp.tf_warp(flow[n:n + 1], flow[n:n + 1], layout).neg_()
        assert torch.equal(one, w_), "%s: -tf_warp of image %d" % (what, n)
        del one, w_
        one = ops.occlusion_map(flow[n:n + 1], layout)
        assert torch.equal(one, occ[n:n + 1]), "%s: map of image %d" % (what, n)
        del one
    for win in occ_windows(key):
        tag, n, y0, y1, x0, x1, (c0, c1, d0, d1) = win
        crop = _occ_cut(flow, layout, n, y0, x0)
        r_inv, r_map = occ_restatement(crop, (y0, x0), (H, W), half)
        g_inv = _occ_cut(inv, layout, n, y0, x0)
        g_map = occ[n, y0:y1, x0:x1].cpu().numpy()
        a, b = r_inv[c0:c1, d0:d1], g_inv[c0:c1, d0:d1]
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b), (what, tag, "inverse flow", int((a != b).sum()))
        a, b = r_map[c0:c1, d0:d1], g_map[c0:c1, d0:d1]
        assert np.array_equal(a, b), (what, tag, "map", int((a != b).sum()))
        assert a.min() == 0.0 and a.max() == 1.0 and r_inv[c0:c1, d0:d1].any(), (what, tag)      # the window says something
        stats["windows"] += 1
        for mod, mask, at in occ_wrapped(key, win, layout, 2 if half else 4):
            behind = mask.any(-1)[c0:c1, d0:d1]                       # compared pixels with a flow value past the modulus
            if behind.sum() < 500:
                continue
            alt = crop.copy()
            alt[mask] = flow.view(-1)[torch.from_numpy(at).to(DEV)].float().cpu().numpy()
            w_inv, w_map = occ_restatement(alt, (y0, x0), (H, W), half)
            moved = (float((w_inv[c0:c1, d0:d1] != r_inv[c0:c1, d0:d1]).any(-1)[behind].mean()),
                     float((w_map[c0:c1, d0:d1] != r_map[c0:c1, d0:d1])[behind].mean()))
            print("{} {}: read at the index mod 2^{}, the inverse flow differs in {:.3f}, the map in {:.3f} of {} pixels".format(
                what, tag, mod.bit_length() - 1, moved[0], moved[1], int(behind.sum())))
            assert moved[0] > 0.5 and moved[1] > 0.1, (what, tag, mod, moved)
            stats["controls"].append(moved)


def test_occlusion_and_inverse_flow(arena):
    """invert_flow_kernel, fill_ones_kernel and occlusion_scatter_kernel at 3 x 18917 x 18923: 1.0739 G pixels (five
    grid-stride trips, the last partial), 2.148 G flow elements, through ops.invert_flow and ops.occlusion_map; fp32
    channels_last, fp32 channels_first and fp16 channels_first.  Equality throughout: oracles (a), (b), (c) of the
    section's comment.  Measured: peak 26.01 GiB (planned 25.34), 0.4 - 1.3 s; 33 windows and 9 one-image launches equal; the 30 controls differ in
    0.86 - 1.00 (inverse flow) and 0.46 - 0.49 (map) of the compared pixels behind their boundary."""
    key = CASES["occlusion"]
    B, H, W = key
    planned = occlusion_planned_bytes(key)
    t0 = time.perf_counter()
    gen = torch.Generator(device=DEV).manual_seed(21)
    a = arena
    a["flow"] = flow = _dflow(gen, B, H, W, reach=OCC_F)
    assert B * H * W > 4 * OCC_TRIP and (B * H * W) % OCC_TRIP and flow.numel() > 1 << 31
    assert float(flow.abs().max()) == OCC_F
    stats = {"windows": 0, "controls": []}
    a["inv"], a["occ"] = ops.invert_flow(flow), ops.occlusion_map(flow)
    _occ_check(key, flow, a["inv"], a["occ"], "channels_last", "fp32 channels_last", stats)
    a.pop("inv")
    occ_last = a.pop("occ")
    # fp32 channels_first: the same values in planes; the map is the same map
    a["cf"] = cf = torch.empty((B, 2, H, W), device=DEV)
    cf.copy_(flow.permute(0, 3, 1, 2))
    del flow
    a.pop("flow")
    a["occ"] = ops.occlusion_map(cf, "channels_first")
    assert torch.equal(a["occ"], occ_last)
    del occ_last
    a["inv"] = ops.invert_flow(cf, "channels_first")
    _occ_check(key, cf, a["inv"], a["occ"], "channels_first", "fp32 channels_first", stats)
    a.pop("inv")
    # fp16 channels_first: the 2^-6 grid within 6 px is exact in fp16, so the map is still the same map
    a["cf16"] = cf16 = torch.empty((B, 2, H, W), device=DEV, dtype=torch.float16)
    cf16.copy_(cf)
    del cf
    a.pop("cf")
    assert cf16.numel() > 1 << 31
    a["inv"], occ16 = ops.invert_flow(cf16, "channels_first"), ops.occlusion_map(cf16, "channels_first")
    assert a["inv"].dtype == torch.float16 and torch.equal(occ16, a["occ"])
    del occ16
    _occ_check(key, cf16, a["inv"], a["occ"], "channels_first", "fp16 channels_first", stats)
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    c = stats["controls"]
    print("occlusion: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, {} windows equal, {} controls: inverse flow differs in "
          "{:.3f} .. {:.3f}, map in {:.3f} .. {:.3f} of a window".format(peak / GIB, planned / GIB, secs, stats["windows"], len(c),
                                                                        min(x[0] for x in c), max(x[0] for x in c),
                                                                        min(x[1] for x in c), max(x[1] for x in c)))
    assert stats["windows"] == 3 * len(occ_windows(key)) and len(c) >= 3 * 4
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- the interpolator's input pipeline: 3-byte source pixels, 6- and 3-channel outputs ------------------------------------
# uint8 frames of 3 x 28528 x 28534: the source pixel index `b * H * W + y * W + x` of triplet_pixel_kernel passes 2^29,
# 2^30 and 2^31 in samples 0, 1 and 2, aug_load_rgb's `pix * 3` 2^31 and 2^32 bytes.  The output is (H / 2, W / 2): the
# fp32 source coordinate (i + 0.5) * 2 - 0.5 = 2 i + 0.5 is exact (at another ratio a coordinate near 26000 is good to
# 2e-3 px, twenty bounds on random uint8 frames), an output pixel reads the 2 x 2 source pixels (2 sy .. 2 sy + 1, 2 sx ..
# 2 sx + 1) of its pre-flip place (sy, sx), and out_pair (3.66 G floats) passes 2^31, out_mid (1.83 G) 2^30: TileStore's
# `obase`.  h * w is a multiple of 4: the <vec4> form.  The frames are zero except the sources of the windows.
#
# (a) out[n] equals the launch on sample n alone with its parameter row; (b) float64 ref_triplet on the 64 x 64 source
# crop of TRI_WIN x TRI_WIN output windows across each source boundary (at the output pixel that reads it, where the flips
# put it), across each element boundary of out_pair and out_mid in both layouts, and on the last pixels of sample 2, the
# noise from the FULL output's pre-flip pixel index (ref_noise_at), bound BOUND = 1e-4; (c) with the source bytes whose
# index reaches 2^31 or 2^32 read at the index modulo that, every such window moves by 100 bounds and more.
#
# On paper: `int64_t pix` to `int pix` in aug_load_rgb makes `pix * 3` wrap from pixel 715,827,883 on, in sample 0: the
# windows "src>2^30", "src>2^31" and every output window of samples 1 and 2 read zeros or nothing of theirs, (a) fails for
# all three samples and (b) there; control (c) is that reading.  `int64_t obase` to `int obase` leaves `(img + base + t) * C`
# (or `img * C`) a 32-bit product: out_pair from element 2^31 on and out_mid's tail are not written; (a) fails for samples 1
# and 2 (the one-sample launch has obase 0), (b) in the windows "pair>2^31" of both layouts and "last".
TRI_WIN = 32
TRI_FLIPS = ((0, 1), (1, 0), (1, 1))                   # (flip_ud, flip_lr) of samples 0, 1, 2


def triplet_output_pixels(key, layout):
    """[(tag, n, y, x)] in output coordinates: the pixel that reads each boundary pixel of the source (through the
    sample's flips), the pixel that holds each element boundary of out_pair and out_mid in this layout, the last pixel."""
    B, H, W = key
    h, w = H // 2, W // 2
    out = []
    for b in crossed(B * H * W):
        n, Y, X = locate(b, H, W, 1)
        ud, lr = TRI_FLIPS[n]
        out.append(("src>2^%d" % (b.bit_length() - 1), n, h - 1 - Y // 2 if ud else Y // 2, w - 1 - X // 2 if lr else X // 2))
    for name, C in (("pair", 6), ("mid", 3)):
        for b in crossed(B * h * w * C):
            if layout == "channels_last":
                n, y, x = locate(b, h, w, C)
            else:
                n, y, x = b // (h * w) // C, b % (h * w) // w, b % w
            out.append(("%s>2^%d" % (name, b.bit_length() - 1), n, y, x))
    out.append(("last", B - 1, h - 1, w - 1))
    return out


def triplet_windows(key, layout, pixels=None):
    """[(tag, n, oy0, ox0, r0, c0)]: TRI_WIN x TRI_WIN output pixels from (oy0, ox0) around each pixel of
    triplet_output_pixels() (or of `pixels`) and the first of the 2 TRI_WIN x 2 TRI_WIN source pixels (r0, c0) they read."""
    B, H, W = key
    h, w = H // 2, W // 2
    wins = []
    for tag, n, y, x in triplet_output_pixels(key, layout) if pixels is None else pixels:
        oy0, ox0 = _span(y, TRI_WIN, h)[0], _span(x, TRI_WIN, w)[0]
        ud, lr = TRI_FLIPS[n]
        sy0, sx0 = h - oy0 - TRI_WIN if ud else oy0, w - ox0 - TRI_WIN if lr else ox0        # the pre-flip place
        wins.append((tag, n, oy0, ox0, 2 * sy0, 2 * sx0))
    return wins


def triplet_counters(key, win):
    """(TRI_WIN * TRI_WIN,) the noise counters of a window's pre-flip pixels: sy * w + sx of the whole output."""
    w = key[2] // 2
    sy, sx = np.mgrid[win[4] // 2:win[4] // 2 + TRI_WIN, win[5] // 2:win[5] // 2 + TRI_WIN]
    return (sy * w + sx).reshape(-1)


def triplet_window_ref(key, win, crops, ip_row, fp_row):
    """Float64 ref_triplet of a window from the three source crops (1, 2 TRI_WIN, 2 TRI_WIN, 3) -> (pair, mid), the window
    as the output holds it (flipped), channels last."""
    from test_triplet_cpu import ref_noise_at, ref_triplet
    noise = ref_noise_at(ip_row[None, 2:4], triplet_counters(key, win)).reshape(1, TRI_WIN, TRI_WIN, 3)
    pair, mid = ref_triplet(crops[0], crops[1], crops[2], ip_row[None], fp_row[None], (TRI_WIN, TRI_WIN), noise=noise)
    return pair[0], mid[0]


def triplet_source_bytes(key, win):
    """(2 TRI_WIN, 2 TRI_WIN, 3) int64: the byte index `pix * 3 + c` of a window's source in a frame."""
    B, H, W = key
    _, n, _, _, r0, c0 = win
    yy, xx = np.mgrid[r0:r0 + 2 * TRI_WIN, c0:c0 + 2 * TRI_WIN].astype(np.int64)
    return (((n * H + yy) * W + xx) * 3)[..., None] + np.arange(3)


def triplet_planned_bytes(key):
    """Three uint8 frames, out_pair and out_mid of the batch and of one sample."""
    B, H, W = key
    return 3 * 3 * B * H * W + 4 * 9 * (B + 1) * (H // 2) * (W // 2)


def test_triplet(arena):
    """triplet_pixel_kernel<vec4> on uint8 frames of 3 x 28528 x 28534 -> 14264 x 14267, both layouts: aug_load_rgb's
    `pix * 3` past 2^31 and 2^32 bytes, TileStore<.., 6, ..> / <.., 3, ..> at an obase past 2^31 / 2^30 elements.  Oracles
    (a), (b), (c) of the section's comment.  Measured: peak 48.90 GiB (planned 47.76; the rest is the boolean of torch.equal), 0.1 - 0.9 s; pair 2.3e-7, middle
    frame 2.0e-7 against the bound of 1e-4; the 16 controls moved their windows by 10151 - 12367 bounds."""
    from test_augment_cpu import BOUND
    from test_triplet_cpu import _params
    key = CASES["triplet"]
    B, H, W = key
    h, w = H // 2, W // 2
    planned = triplet_planned_bytes(key)
    t0 = time.perf_counter()
    a = arena
    frames = [torch.zeros((B, H, W, 3), dtype=torch.uint8, device=DEV) for _ in range(3)]
    a["frames"] = frames
    assert B * H * W > 1 << 31 and 1 << 29 < H * W < 1 << 30 and B * h * w * 6 > 1 << 31 and (h * w) % 4 == 0
    ip_np, fp_np = _params(B, 77)
    ip_np[:, 0:2] = TRI_FLIPS
    assert len({tuple(r) for r in fp_np.tolist()}) == B and (fp_np[:, 15] == np.float32(0.02)).all()
    ip, fp = torch.from_numpy(ip_np).to(DEV), torch.from_numpy(fp_np).to(DEV)
    wins = {lay: triplet_windows(key, lay) for lay in ("channels_last", "channels_first")}
    rng = np.random.default_rng(12)
    for lay in wins:
        for _, n, _, _, r0, c0 in wins[lay]:
            for f in frames:
                f[n, r0:r0 + 2 * TRI_WIN, c0:c0 + 2 * TRI_WIN] = torch.from_numpy(
                    rng.integers(0, 256, (2 * TRI_WIN, 2 * TRI_WIN, 3), dtype=np.uint8)).to(DEV)
    worst, controls = {"pair": 0.0, "mid": 0.0}, []
    for lay in wins:
        assert ops.augment_triplet_kernel(B, h, w) == "triplet_pixel_kernel<vec4>"
        a["pair"], a["mid"] = pair, mid = ops.augment_triplet(*frames, ip, fp, (h, w), data_format=lay)
        assert pair.numel() > 1 << 31 and mid.numel() > 1 << 30
        for n in range(B):
            one = ops.augment_triplet(*[f[n:n + 1] for f in frames], ip[n:n + 1], fp[n:n + 1], (h, w), data_format=lay)
            assert torch.equal(one[0], pair[n:n + 1]) and torch.equal(one[1], mid[n:n + 1]), (lay, n)
            del one
        for win in wins[lay]:
            tag, n, oy0, ox0, r0, c0 = win
            crops = [f[n:n + 1, r0:r0 + 2 * TRI_WIN, c0:c0 + 2 * TRI_WIN].cpu().numpy() for f in frames]
            assert all(c.any() for c in crops) and not np.array_equal(crops[0], crops[1])
            r_pair, r_mid = triplet_window_ref(key, win, crops, ip_np[n], fp_np[n])
            assert np.abs(r_pair).max() > 0.25 and np.abs(r_mid).max() > 0.25
            for name, got, ref in (("pair", pair, r_pair), ("mid", mid, r_mid)):
                g = got[n, oy0:oy0 + TRI_WIN, ox0:ox0 + TRI_WIN] if lay == "channels_last" else \
                    got[n, :, oy0:oy0 + TRI_WIN, ox0:ox0 + TRI_WIN].permute(1, 2, 0)
                e = float(np.abs(g.double().cpu().numpy() - ref).max())
                print("triplet {} {} {}: max|d| = {:.3e}".format(lay, tag, name, e))
                assert e <= BOUND, (lay, tag, name, e)
                worst[name] = max(worst[name], e)
            idx = triplet_source_bytes(key, win)
            for mod in (1 << 31, 1 << 32):
                mask = idx >= mod
                if not mask.any():
                    continue
                at = torch.from_numpy(idx[mask] % mod).to(DEV)
                alt = []
                for f, c in zip(frames, crops):
                    c = c.copy()
                    c[0][mask] = f.view(-1)[at].cpu().numpy()
                    alt.append(c)
                w_pair, w_mid = triplet_window_ref(key, win, alt, ip_np[n], fp_np[n])
                ratio = min(np.abs(w_pair - r_pair).max(), np.abs(w_mid - r_mid).max()) / BOUND
                print("triplet {} {}: sources read at the byte index mod 2^{} move the window by {:.0f} bounds".format(
                    lay, tag, mod.bit_length() - 1, ratio))
                assert ratio >= 100.0, (lay, tag, mod, ratio)
                controls.append(ratio)
        del pair, mid, got, g                             # the last two are views of the outputs
        a.pop("pair"), a.pop("mid")
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("triplet: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s, worst {}, {} controls {:.0f} .. {:.0f} bounds".format(
        peak / GIB, planned / GIB, secs, worst, len(controls), min(controls), max(controls)))
    assert len(controls) >= 2 * 6
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)


# ---- the update step on one parameter of more than 2^31 floats --------------------------------------------------------
# agc_adam_kernel through the C entry point, both tables built by torch on the device: one tensor of 18,683,000 rows of
# 115 floats (the models' pointwise row: no row but every fourth starts on 16 bytes, so the head / float4 / tail split
# cycles through its four phases), a unit a row, `un.offset` up to 2,148,544,885.  18.7 M units on 4096 waves: the
# grid-stride form.
#
# (a) p, m and v are torch.equal to a second launch on the same data whose tensor table lists five slices of the arrays,
# each under 2^29 elements, the units' offsets rebased to their slice: units are independent and the kernel has no
# atomics, every row has the same addresses in both launches.  Both results of an array do not fit beside the operands:
# the data is redrawn from its seeds and both launches repeated for each of p, m, v, one array of the first launch
# kept at a time.  (b) the float64 oracle of tests/test_optim_cpu.py on the rows that straddle elements 2^29, 2^30 and
# 2^31, the first and the last row and 32 seeded rows, at that module's bounds (tests/test_large_offsets_cpu.py shows
# that the fp32 torch composition stays within a tenth of them on rows drawn like these).  (c) the float64 answer
# for the 115 elements that the offset of a row behind 2^31, wrapped there, addresses lies more than 100 bounds away.
#
# On paper: `un.offset` cut to 32 bits is negative from row 18,673,771 on: those rows' p, m, v are not updated (or other
# memory is): (a) fails for all three arrays, (b) on the last row and the seeded rows behind it.
OPT_SLICE_ROWS = ((1 << 29) - 1) // 115               # whole rows under 2^29 elements
OPT_SEEDS = {"p": 31, "g": 32, "m": 33, "v": 34}


def optim_draw(t, which):
    """Redraws one array in place from its seed: p ~ N(0, 0.1) as the models' weights, m ~ N(0, 1e-3), v the square of
    such a number (>= 0), g ~ N(0, 1) before its rows are scaled."""
    gen = torch.Generator(device=t.device).manual_seed(OPT_SEEDS[which])
    t.normal_(0.0, {"p": 0.1, "g": 1.0, "m": 1e-3, "v": 1e-3}[which], generator=gen)
    if which == "v":
        t.mul_(t)


def optim_scale_rows(p, g, cols, clip, eps):
    """Scales g's rows so that gn / mx is 0.25 (even rows) or 4 (odd rows), mx = max(pn, eps) * clip -> the fp32 ratio
    of every row afterwards, (rows,)."""
    pr, gr = p.view(-1, cols), g.view(-1, cols)
    mx = torch.linalg.vector_norm(pr, dim=1).clamp_(min=eps).mul_(clip)
    want = torch.full_like(mx, 0.25)
    want[1::2] = 4.0
    gr.mul_((want * mx / torch.linalg.vector_norm(gr, dim=1))[:, None])
    return torch.linalg.vector_norm(gr, dim=1) / mx


def optim_tables(base, rows, cols, slice_rows, device):
    """The tables of both launches, int64 on the device.  base: the addresses of p, g, m, v.
    -> (tensors (1, 4), units (rows, 3)) of the launch on the whole arrays, (tensors (K, 4), units (rows, 3)) of the
    launch on K slices of slice_rows rows (the last shorter), offsets counted from the slice's start."""
    r = torch.arange(rows, dtype=torch.int64, device=device)
    whole = torch.stack([torch.zeros_like(r), r * cols, torch.full_like(r, cols)], 1).contiguous()
    sliced = torch.stack([r // slice_rows, (r % slice_rows) * cols, torch.full_like(r, cols)], 1).contiguous()
    k = -(-rows // slice_rows)
    starts = torch.arange(k, dtype=torch.int64) * (slice_rows * cols * 4)
    tens_whole = torch.tensor([list(base)], dtype=torch.int64).to(device)
    tens_sliced = (torch.tensor(list(base), dtype=torch.int64)[None, :] + starts[:, None]).contiguous().to(device)
    return (tens_whole, whole), (tens_sliced, sliced)


def optim_sample_rows(rows, cols):
    """The rows held to the oracle: those that straddle elements 2^29, 2^30 and 2^31, the first, the last, 32 seeded."""
    out = [b // cols for b in crossed(rows * cols)] + [0, rows - 1]
    rng = np.random.default_rng(41)
    return out + sorted(int(x) for x in rng.choice(rows, 32, replace=False) if int(x) not in out)


def optim_rows_oracle(p, g, m, v):
    """One update of rows (R, cols) by tests/test_optim_cpu.py's float64 oracle, a unit a row, clipping on, t = 1
    -> (p, m, v) float64."""
    from test_optim_cpu import oracle_step, oracle_units
    name, shape = "rows.pointwise.weight", p.shape + (1, 1)
    assert oracle_units(name, shape) == [(k * p.shape[1], p.shape[1]) for k in range(p.shape[0])]
    state = {k: {name: np.asarray(a, np.float64).reshape(shape).copy()} for k, a in (("p", p), ("m", m), ("v", v))}
    state["t"] = 0
    oracle_step(state, {name: np.asarray(g).reshape(shape)})
    return tuple(state[k][name].reshape(p.shape) for k in "pmv")


def optim_row_errors(have, want):
    """(max |p - ref|, max over rows of max |m - ref| / max |ref|, the same for v), as tests/test_optim_cpu.py::errors."""
    out = []
    for k in range(3):
        d = np.abs(np.asarray(have[k], np.float64) - want[k]).max(1)
        assert np.isfinite(d).all()
        out.append(float((d if k == 0 else d / np.abs(want[k]).max(1)).max()))
    return tuple(out)


def optim_planned_bytes(key):
    """p, g, m, v, one array of the first launch kept for the comparison, and the two unit tables."""
    rows, cols = key
    return 5 * 4 * rows * cols + 2 * 24 * rows


def test_agc_adam_step(arena):
    """agc_adam_kernel<grid-stride> on one parameter of 18,683,000 rows of 115 floats (2.1485 G): oracles (a), (b), (c)
    of the section's comment.  Measured: peak 42.86 GiB (planned 40.85), 2.1 - 4.0 s; 37 rows against float64: p 1.5e-8, m
    5.3e-8, v 4.9e-8 (bounds 1.56e-7, 1.88e-6, 1.16e-6); the control's rows lie 2.6e6 bounds away."""
    from test_optim_cpu import (AGC_EPS, BETA_1, BETA_2, CLIP, EPSILON, LR, M_BOUND, P_BOUND, V_BOUND, oracle_alpha)
    key = CASES["optim"]
    rows, cols = key
    n = rows * cols
    planned = optim_planned_bytes(key)
    t0 = time.perf_counter()
    L = ops._hip.lib()
    assert n > (1 << 31) + (1 << 20) and L.qpwc_agc_adam_step_kernel(rows) == b"agc_adam_kernel<grid-stride>"
    a = arena
    for k in "pgmv":
        a[k] = torch.empty(n, device=DEV)
        optim_draw(a[k], k)
    p, g, m, v = (a[k] for k in "pgmv")
    ratio = optim_scale_rows(p, g, cols, CLIP, AGC_EPS)
    assert float((ratio - 1.0).abs().min()) > 1e-3                                     # no row near the clip threshold
    assert float(torch.minimum((ratio - 0.25).abs(), (ratio - 4.0).abs()).max()) < 1e-4 and float(v.min()) >= 0.0
    del ratio
    sample = optim_sample_rows(rows, cols)
    at = torch.tensor(sample, device=DEV)
    before = [t.view(rows, cols)[at].cpu().numpy() for t in (p, g, m, v)]
    want = optim_rows_oracle(*before)
    # the control's rows: what the offsets of the first row behind 2^31 and of the last row address when wrapped at 2^31
    behind = [r for r in (BOUNDARIES[2] // cols + 1, rows - 1)]
    wrapped = torch.tensor([[r * cols - (1 << 31) + c for c in range(cols)] for r in behind], device=DEV)
    assert int(wrapped.min()) >= 0
    alt = optim_rows_oracle(*[t[wrapped].cpu().numpy() for t in (p, g, m, v)])
    right = optim_rows_oracle(*[t.view(rows, cols)[torch.tensor(behind, device=DEV)].cpu().numpy() for t in (p, g, m, v)])
    control = float(np.abs(alt[0] - right[0]).max(1).min()) / P_BOUND
    print("agc_adam: rows read at their offset mod 2^31 move p by {:.0f} bounds".format(control))
    assert control > 100.0
    (t_whole, u_whole), (t_sliced, u_sliced) = optim_tables([t.data_ptr() for t in (p, g, m, v)], rows, cols, OPT_SLICE_ROWS, DEV)
    a["tables"] = (t_whole, u_whole, t_sliced, u_sliced)
    assert t_sliced.shape == (5, 4) and int(u_sliced[:, 1].max()) + cols <= 1 << 29 and int(u_whole[:, 1].max()) + cols == n
    alpha = float(np.float32(oracle_alpha(LR, 1)))

    def launch(tens, units):
        rc = L.qpwc_agc_adam_step(tens.data_ptr(), int(tens.shape[0]), units.data_ptr(), rows, alpha, BETA_1, BETA_2, EPSILON,
                                  CLIP, AGC_EPS, torch.cuda.current_stream().cuda_stream)
        ops._hip.check(rc)

    err = None
    for k, name in enumerate("pmv"):
        if k:
            for which in "pmv":
                optim_draw(a[which], which)
        launch(t_whole, u_whole)
        if k == 0:
            after = [t.view(rows, cols)[at].cpu().numpy() for t in (p, m, v)]
            err = optim_row_errors(after, want)
            print("agc_adam: {} rows against float64: p abs {:.3g} (bound {:.3g}), m rel {:.3g} ({:.3g}), v rel {:.3g} ({:.3g})".format(
                len(sample), err[0], P_BOUND, err[1], M_BOUND, err[2], V_BOUND))
            assert err[0] <= P_BOUND and err[1] <= M_BOUND and err[2] <= V_BOUND, err
            assert torch.equal(g.view(rows, cols)[at].cpu(), torch.from_numpy(before[1]))
        a["kept"] = kept = a[name].clone()
        for which in "pmv":
            optim_draw(a[which], which)
        launch(t_sliced, u_sliced)
        assert torch.equal(a[name], kept), "%s of the launch on slices" % name
        del kept
        a.pop("kept")
    for t, ref in zip((p, m, v), after):
        assert np.array_equal(t.view(rows, cols)[at].cpu().numpy(), ref)
    torch.cuda.synchronize()
    peak, secs = torch.cuda.max_memory_allocated() - arena["_base"], time.perf_counter() - t0
    print("agc_adam: peak {:.2f} GiB, planned {:.2f} GiB, {:.2f} s".format(peak / GIB, planned / GIB, secs))
    assert planned <= 48 * GIB
    assert peak <= 1.10 * planned, (peak / GIB, planned / GIB)

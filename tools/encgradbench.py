#!/usr/bin/env python3
"""Backward of the encoder's Conv2D(3x3, stride 1 / 2, 'same') + Mish layers (qpwc_conv3x3_same_bwd behind torch
autograd) at the 15 layer shapes of the encoder, against torch autograd of the composed restatement (F.pad 'SAME' +
F.conv2d + F.mish) on the same GPU.

    python tools/encgradbench.py [--iters 20] [--warmup 5] [--json profiles/gradbench_encoder.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/encgradbench.py --trace 1:aa --iters 10

Shapes: config 2 (B = 8 fp32 pairs of 256 x 512 = 16 stacked frames); level outputs 128x256x16, 64x128x32, 32x64x64,
16x32x128, 8x16x256; per level conv_a (stride 2 from the level above; the first one 3 -> 16 from 256 x 512), conv_aa and
conv_b.  Times are medians of HIP-event pairs around eager calls, the HIP backward through autograd, the composed torch
backward and the bare ops.conv3x3_same_bwd (no autograd bookkeeping, all three gradients) alternating in one process.
Per stage the compulsory bytes and matrix FLOPs come from the shapes; floor = max(bytes / 8 TB/s, FLOPs / 157 TFLOP/s),
the fp32 matrix-instruction peak being 64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz; the three matrix stages (z, grad_x,
grad_w) are 2 M_out 9 C_in C_out FLOP each.  --trace LEVEL:LAYER (level 1..5, layer a / aa / b) runs only the bare HIP
backward of one shape, for a kernel trace."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import ops  # noqa: E402

HBM = 8000.0     # GB/s
MFMA32 = 157.0   # TFLOP/s
FILTERS = (16, 32, 64, 128, 256)
FRAMES, IMG = 16, (256, 512)
DEV = "cuda:0"


def shapes():
    """[(level, layer, H, W, C_in, C_out, stride)]: H, W of the layer's input."""
    out, h, w, c = [], IMG[0], IMG[1], 3
    for i, f in enumerate(FILTERS):
        out.append((i + 1, "a", h, w, c, f, 2))
        h, w = h // 2, w // 2
        out += [(i + 1, "aa", h, w, f, f, 1), (i + 1, "b", h, w, f, f, 1)]
        c = f
    return out


def same_pad(n, s):
    total = max((-(-n // s) - 1) * s + 3 - n, 0)
    return total // 2, total - total // 2


def composed(x, w, b, stride):
    pt, pb = same_pad(x.shape[1], stride)
    pl, pr = same_pad(x.shape[2], stride)
    return F.mish(F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w, b, stride=stride)).permute(0, 2, 3, 1)


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def stage_floors(M_in, M_out, ci, co):
    """{stage: bytes, flops, floor_us} of the stages of csrc/conv_bwd.hip with every gradient asked for."""
    cp = (ci + 3) // 4 * 4
    wts = 9 * co * cp
    mm = 2 * M_out * 9 * ci * co
    st = {"Z_gz": (4 * (M_in * ci + wts + 2 * M_out * co), mm),       # x, w, grad_out -> gz
          "X_grad_x": (4 * (M_out * co + wts + M_in * ci), mm),       # gz, w -> grad_x
          "W_grad_w": (4 * (M_out * co + M_in * ci + wts), mm)}       # gz, x -> grad_w, grad_b
    return {k: dict(bytes=b, flops=f, floor_us=max(b / HBM / 1e3, f / MFMA32 / 1e6)) for k, (b, f) in st.items()}


def make_case(shape, gen):
    _, _, H, W, ci, co, s = shape
    x = torch.randn(FRAMES, H, W, ci, device=DEV, generator=gen)
    w = torch.randn(co, ci, 3, 3, device=DEV, generator=gen) / (9 * ci) ** 0.5
    b = torch.randn(co, device=DEV, generator=gen) / 4
    g = torch.randn(FRAMES, -(-H // s), -(-W // s), co, device=DEV, generator=gen)
    return x, w, b, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", default=None, help="LEVEL:LAYER: only the bare HIP backward of that layer")
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    if a.trace:
        lv, name = a.trace.split(":")
        shape = [s for s in shapes() if s[0] == int(lv) and s[1] == name][0]
        x, w, b, g = make_case(shape, gen)
        taps = ops.conv3x3_same_taps(w)
        for _ in range(a.iters):
            ops.conv3x3_same_bwd(x, taps, b, g, shape[6], True)
        torch.cuda.synchronize()
        return
    rows = []
    for shape in shapes():
        level, name, H, W, ci, co, s = shape
        x, w, b, g = make_case(shape, gen)
        leaves = [t.requires_grad_() for t in (x, w, b)]
        out_h = ops.conv3x3_same(*leaves, stride=s)
        out_t = composed(*leaves, s)
        hip = lambda: torch.autograd.grad(out_h, leaves, g, retain_graph=True)
        ref = lambda: torch.autograd.grad(out_t, leaves, g, retain_graph=True)
        det = [t.detach() for t in leaves]
        taps = ops.conv3x3_same_taps(det[1])
        kern = lambda: ops.conv3x3_same_bwd(det[0], taps, det[2], g, s, True)
        for _ in range(a.warmup):
            hip(), ref(), kern()
        th, tr, tk = [], [], []
        for _ in range(a.iters):                      # alternating: all three see the same clocks and cache state
            th.append(event_us(hip))
            tr.append(event_us(ref))
            tk.append(event_us(kern))
        # agreement of the two backwards (the comparison is only worth something if they compute the same)
        gh, gr = hip(), ref()
        err = max(float((p - q).abs().max() / max(1.0, float(q.abs().max()))) for p, q in zip(gh, gr))
        M_in, M_out = FRAMES * H * W, FRAMES * -(-H // s) * -(-W // s)
        floors = stage_floors(M_in, M_out, ci, co)
        floor = sum(v["floor_us"] for v in floors.values())
        row = dict(level=level, layer="conv_" + name, frames=FRAMES, H=H, W=W, C_in=ci, C_out=co, stride=s,
                   hip_bwd_us=statistics.median(th), torch_bwd_us=statistics.median(tr),
                   bwd_kernel_us=statistics.median(tk), speedup=statistics.median(tr) / statistics.median(th),
                   stages=floors, floor_us=floor, frac_of_floor=floor / statistics.median(tk),
                   max_rel_diff_vs_torch=err)
        rows.append(row)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items() if k != "stages"}),
              flush=True)
        del x, w, b, g, leaves, out_h, out_t, det, gh, gr
        torch.cuda.empty_cache()
    total = dict(hip_bwd_us=sum(r["hip_bwd_us"] for r in rows), torch_bwd_us=sum(r["torch_bwd_us"] for r in rows),
                 bwd_kernel_us=sum(r["bwd_kernel_us"] for r in rows), floor_us=sum(r["floor_us"] for r in rows))
    print(json.dumps({"sum_over_15_layers": {k: round(v, 1) for k, v in total.items()}}), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "rows": rows,
                       "sum": total}, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Backward of the decoder's Mish(Conv2DTranspose(4x4, stride 2, 'same') + bias) layers (qpwc_upconv4x4s2_bwd behind torch
autograd) at the four layer shapes of the decoder, against torch autograd of the composed restatement
(F.conv_transpose2d(stride=2, padding=1) + F.mish) on the same GPU.

    python tools/decgradbench.py [--iters 20] [--warmup 5] [--json profiles/gradbench_decoder.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/decgradbench.py --trace 2 --iters 10

Shapes: config 2 (B = 8 fp32 pairs of 256 x 512 = 16 stacked frames); layer inputs 8x16x256 -> 128, 16x32x256 -> 64,
32x64x128 -> 32, 64x128x64 -> 16 filters.  Times are medians of HIP-event pairs around eager calls, the HIP backward
through autograd, the composed torch backward and the bare ops.upconv4x4s2_bwd (no autograd bookkeeping, all three
gradients) in one process, their order reversed from one iteration to the next.  Per stage the compulsory bytes and
matrix FLOPs come from the shapes; floor = max(bytes / 8 TB/s, FLOPs / 157 TFLOP/s), the fp32 matrix-instruction peak
being 64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz.  The three matrix stages (z, grad_x, grad_w) are 2 M_in 16 C F FLOP
each (an output pixel meets 4 taps and there are 4 M_in of them).  --trace LEVEL (0..3) runs only the bare HIP backward
of one shape, for a kernel trace."""
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
FRAMES = 16
SHAPES = ((0, 8, 16, 256, 128), (1, 16, 32, 256, 64), (2, 32, 64, 128, 32), (3, 64, 128, 64, 16))   # level, H, W, C, F
DEV = "cuda:0"


def composed(x, w, b):
    return F.mish(F.conv_transpose2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1)).permute(0, 2, 3, 1)


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def stage_floors(M_in, C, F_):
    """{stage: bytes, flops, floor_us} of the stages of csrc/upconv_bwd.hip with every gradient asked for."""
    M_out, wts, mm = 4 * M_in, 16 * F_ * C, 2 * M_in * 16 * C * F_
    st = {"Z_gz": (4 * (M_in * C + wts + 2 * M_out * F_), mm),       # x, w, grad_out -> gz
          "X_grad_x": (4 * (M_out * F_ + wts + M_in * C), mm),       # gz, w -> grad_x
          "W_grad_w": (4 * (M_out * F_ + M_in * C + wts), mm)}       # gz, x -> grad_w, grad_b
    return {k: dict(bytes=b, flops=f, floor_us=max(b / HBM / 1e3, f / MFMA32 / 1e6)) for k, (b, f) in st.items()}


def make_case(shape, gen):
    _, H, W, C, F_ = shape
    x = torch.randn(FRAMES, H, W, C, device=DEV, generator=gen)
    w = torch.randn(C, F_, 4, 4, device=DEV, generator=gen) / (4 * C) ** 0.5
    b = torch.randn(F_, device=DEV, generator=gen) / 4
    g = torch.randn(FRAMES, 2 * H, 2 * W, F_, device=DEV, generator=gen)
    return x, w, b, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", type=int, default=None, help="LEVEL: only the bare HIP backward of that layer")
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    if a.trace is not None:
        x, w, b, g = make_case(SHAPES[a.trace], gen)
        taps = ops.upconv_taps(w)
        for _ in range(a.iters):
            ops.upconv4x4s2_bwd(x, taps, b, g)
        torch.cuda.synchronize()
        return
    rows = []
    for shape in SHAPES:
        level, H, W, C, F_ = shape
        x, w, b, g = make_case(shape, gen)
        leaves = [t.requires_grad_() for t in (x, w, b)]
        out_h = ops.upconv4x4s2(*leaves)
        out_t = composed(*leaves)
        det = [t.detach() for t in leaves]
        taps = ops.upconv_taps(det[1])
        runs = {"hip": lambda: torch.autograd.grad(out_h, leaves, g, retain_graph=True),
                "torch": lambda: torch.autograd.grad(out_t, leaves, g, retain_graph=True),
                "kernel": lambda: ops.upconv4x4s2_bwd(det[0], taps, det[2], g)}
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        times = {k: [] for k in runs}
        order = list(runs)
        for i in range(a.iters):                      # order reversed every other iteration
            for k in (order if i % 2 == 0 else order[::-1]):
                times[k].append(event_us(runs[k]))
        # agreement of the two backwards (the comparison is only worth something if they compute the same)
        gh, gr = runs["hip"](), runs["torch"]()
        err = max(float((p - q).abs().max() / max(1.0, float(q.abs().max()))) for p, q in zip(gh, gr))
        med = {k: statistics.median(v) for k, v in times.items()}
        floors = stage_floors(FRAMES * H * W, C, F_)
        floor = sum(v["floor_us"] for v in floors.values())
        row = dict(level=level, frames=FRAMES, H=H, W=W, C=C, F=F_, hip_bwd_us=med["hip"], torch_bwd_us=med["torch"],
                   bwd_kernel_us=med["kernel"], speedup=med["torch"] / med["hip"], stages=floors, floor_us=floor,
                   frac_of_floor=floor / med["kernel"], max_rel_diff_vs_torch=err)
        rows.append(row)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items() if k != "stages"}),
              flush=True)
        del x, w, b, g, leaves, out_h, out_t, det, gh, gr, runs
        torch.cuda.empty_cache()
    total = dict(hip_bwd_us=sum(r["hip_bwd_us"] for r in rows), torch_bwd_us=sum(r["torch_bwd_us"] for r in rows),
                 bwd_kernel_us=sum(r["bwd_kernel_us"] for r in rows), floor_us=sum(r["floor_us"] for r in rows))
    print(json.dumps({"sum_over_4_layers": {k: round(v, 1) for k, v in total.items()}}), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "rows": rows,
                       "sum": total}, fh, indent=1)


if __name__ == "__main__":
    main()

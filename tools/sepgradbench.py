#!/usr/bin/env python3
"""Backward of the fused SeparableConv2D (qpwc_sepconv3x3_bwd behind torch autograd) at OptFlow's layer shapes, against
torch autograd of the composed restatement (torch.cat + F.conv2d(groups=C) + addmm + F.mish) on the same GPU.

    python tools/sepgradbench.py [--iters 20] [--warmup 5] [--json profiles/gradbench_sepconv.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/sepgradbench.py --trace L4:115:128 --iters 10

Shapes: config 2 (B = 8, fp32) at L2 / L3 / L4; per level OptFlow's four layers (81 + feat + 2 -> 128 -> 64 -> 32 -> 16)
with one dense source, and layer 1 in its network form: three sources [84-float padded cost volume | features | flow].
Times are medians of HIP-event pairs around eager calls, the HIP backward and the composed backward alternating in one
process; `bwd_kernel_us` is ops.sepconv3x3_bwd alone (no autograd bookkeeping, all gradients).  Per stage the
compulsory bytes and matrix FLOPs are computed from the shapes; floor = max(bytes / 8 TB/s, FLOPs / 157 TFLOP/s), the
fp32 matrix-instruction peak being 64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz.  --trace runs only the HIP backward of one
shape (LEVEL:C:F, or LEVEL:3src) for a kernel trace."""
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
LEVELS = {"L2": (32, 64, 128), "L3": (64, 128, 64), "L4": (128, 256, 32)}   # H, W, feature channels
B = 8
DEV = "cuda:0"


def composed(sources, dw, pw, bias, on_load, on_store):
    x = torch.cat(sources, dim=3) if len(sources) > 1 else sources[0]
    if on_load:
        x = F.mish(x)
    d = F.conv2d(x.permute(0, 3, 1, 2), dw, None, padding=1, groups=x.shape[3]).permute(0, 2, 3, 1)
    z = torch.addmm(bias, d.reshape(-1, d.shape[3]), pw.t()).reshape(d.shape[:3] + (pw.shape[0],))
    return F.mish(z) if on_store else z


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def stage_floors(M, C, cpad, Fo, on_store):
    """{stage: (bytes, flops, floor_us)} of the stages of csrc/sepconv_bwd.hip with every gradient asked for."""
    st = {"A_depthwise": (4 * M * (C + cpad), 0)}
    if on_store:
        st["B1_gz"] = (4 * M * (cpad + 2 * Fo), 2 * M * cpad * Fo)
    st["B2_pointwise"] = (4 * M * (Fo + 2 * cpad), 4 * M * cpad * Fo)
    st["C_depthwise_bwd"] = (4 * M * (cpad + 2 * C), 0)
    return {k: dict(bytes=b, flops=f, floor_us=max(b / HBM / 1e3, f / MFMA32 / 1e6)) for k, (b, f) in st.items()}


def make_case(level, spec, gen):
    H, W, feat = LEVELS[level]
    if spec == "3src":
        cost = torch.randn(B, H, W, 84, device=DEV, generator=gen)
        cost[..., 81:] = 0
        srcs = [cost, torch.randn(B, H, W, feat, device=DEV, generator=gen),
                torch.randn(B, H, W, 2, device=DEV, generator=gen)]
        Fo, flags = 128, (False, True)
    else:
        C, Fo = spec
        srcs = [torch.randn(B, H, W, C, device=DEV, generator=gen)]
        # layer 1 reads the raw concat; the later layers load with Mish, the last stores its pre-activation
        flags = (C != 81 + feat + 2, Fo != 16)
    C = sum(t.shape[3] for t in srcs)
    dw = torch.randn(C, 1, 3, 3, device=DEV, generator=gen) / 3
    pw = torch.randn(Fo, C, device=DEV, generator=gen) / C ** 0.5
    bias = torch.randn(Fo, device=DEV, generator=gen) / 4
    gout = torch.randn(B, H, W, Fo, device=DEV, generator=gen)
    return srcs, dw, pw, bias, gout, flags


def specs(level):
    feat = LEVELS[level][2]
    return [(81 + feat + 2, 128), (128, 64), (64, 32), (32, 16), "3src"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", default=None, help="LEVEL:C:F or LEVEL:3src: only the HIP backward of that shape")
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    if a.trace:
        parts = a.trace.split(":")
        spec = "3src" if parts[1] == "3src" else (int(parts[1]), int(parts[2]))
        srcs, dw, pw, bias, gout, flags = make_case(parts[0], spec, gen)
        pwp = ops.pad_pointwise(pw)
        for _ in range(a.iters):
            ops.sepconv3x3_bwd(srcs, dw, pwp, bias, gout, *flags)
        torch.cuda.synchronize()
        return
    rows = []
    for level in LEVELS:
        for spec in specs(level):
            srcs, dw, pw, bias, gout, flags = make_case(level, spec, gen)
            leaves = [t.requires_grad_() for t in srcs + [dw, pw, bias]]
            n = len(srcs)
            out_h = ops.sepconv3x3(leaves[:n], leaves[n], ops.pad_pointwise(leaves[n + 1]), leaves[n + 2], *flags)
            out_t = composed(leaves[:n], leaves[n], leaves[n + 1], leaves[n + 2], *flags)
            hip = lambda: torch.autograd.grad(out_h, leaves, gout, retain_graph=True)
            ref = lambda: torch.autograd.grad(out_t, leaves, gout, retain_graph=True)
            det = [t.detach() for t in leaves]
            pwp = ops.pad_pointwise(det[n + 1])
            kern = lambda: ops.sepconv3x3_bwd(det[:n], det[n], pwp, det[n + 2], gout, *flags)
            for _ in range(a.warmup):
                hip(), ref(), kern()
            th, tr, tk = [], [], []
            for _ in range(a.iters):                      # alternating: both see the same clocks and cache state
                th.append(event_us(hip))
                tr.append(event_us(ref))
                tk.append(event_us(kern))
            # agreement of the two backwards (the comparison is only worth something if they compute the same)
            gh, gr = hip(), ref()
            err = max(float((x - y).abs().max() / max(1.0, float(y.abs().max()))) for x, y in zip(gh, gr))
            H, W, _ = LEVELS[level]
            M, C, Fo = B * H * W, sum(t.shape[3] for t in srcs), pw.shape[0]
            floors = stage_floors(M, C, (C + 31) // 32 * 32, Fo, flags[1])
            floor = sum(v["floor_us"] for v in floors.values())
            row = dict(level=level, B=B, H=H, W=W, sources=[t.shape[3] for t in srcs], C=C, F=Fo,
                       mish_on_load=flags[0], mish_on_store=flags[1], hip_bwd_us=statistics.median(th),
                       torch_bwd_us=statistics.median(tr), bwd_kernel_us=statistics.median(tk),
                       speedup=statistics.median(tr) / statistics.median(th), stages=floors, floor_us=floor,
                       frac_of_floor=floor / statistics.median(tk), max_rel_diff_vs_torch=err)
            rows.append(row)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items() if k != "stages"}),
                  flush=True)
            del srcs, leaves, out_h, out_t, det, gh, gr
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "rows": rows},
                      fh, indent=1)


if __name__ == "__main__":
    main()

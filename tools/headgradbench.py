#!/usr/bin/env python3
"""Backward of the flow head (qpwc_flow_head_bwd behind torch autograd, both BatchNorm modes) and of Upsample
(qpwc_upsample2x_flow_bwd) at the L2 / L3 / L4 shapes of config 2 (B = 8, fp32), against torch autograd of the composed
restatement (F.mish + F.conv2d + hand-written batch norm, F.interpolate) on the same GPU.

    python tools/headgradbench.py [--iters 20] [--warmup 5] [--json profiles/gradbench_flow_head.json]

Times are medians of HIP-event pairs around eager calls, the HIP backward and the composed backward alternating in one
process; `bwd_call_us` is the eager call ops.flow_head_bwd / ops.upsample2x_flow_bwd alone (no autograd bookkeeping, all
gradients): a call time -- Python, the workspace and output allocations and ctypes included --, not a kernel time.
The composite is the yardstick, not the code under test.  Byte floors from the shapes (M = B H W pixels, fp32):
  head, pass 1      reads z (64 M) and g (8 M)                           72 M bytes
  head, pass 2      reads z and g again, writes grad_z (64 M)            136 M bytes
  Upsample adjoint  reads g (8 bytes x 4 M), writes 8 M                   40 M bytes
floor = bytes / 8 TB/s, `floor_over_call` = floor / bwd_call_us; the two 16 x 16 products (2 x 2 x 256 M FLOP per pass) are far below it at 157 TFLOP/s."""
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
LEVELS = {"L2": (32, 64), "L3": (64, 128), "L4": (128, 256)}
B = 8
DEV = "cuda:0"
EPS, MOMENTUM = 1e-3, 0.99


def composed_head(z, w1, b1, gamma, beta, mean, var, wf, scale, training):
    u = F.mish(F.conv2d(F.mish(z).permute(0, 3, 1, 2), w1, b1))
    if training:
        mean, var = u.mean(dim=(0, 2, 3)), u.var(dim=(0, 2, 3), unbiased=False)
    h = (u - mean.view(1, -1, 1, 1)) * (gamma / torch.sqrt(var + EPS)).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    return (scale * F.conv2d(h, wf, None, padding=1)).permute(0, 2, 3, 1)


def composed_upsample(x, scale):
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1) * scale


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def measure(hip, ref, kern, iters, warmup):
    for _ in range(warmup):
        hip(), ref(), kern()
    th, tr, tk = [], [], []
    for _ in range(iters):                      # alternating: all three see the same clocks and cache state
        th.append(event_us(hip))
        tr.append(event_us(ref))
        tk.append(event_us(kern))
    gh, gr = hip(), ref()
    err = max(float((x - y).abs().max() / max(1.0, float(y.abs().max()))) for x, y in zip(gh, gr))
    med = statistics.median
    return dict(hip_bwd_us=med(th), torch_bwd_us=med(tr), bwd_call_us=med(tk), speedup=med(tr) / med(th),
                max_rel_diff_vs_torch=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    rows = []
    for level, (H, W) in LEVELS.items():
        M = B * H * W
        scale = float(H * H + W * W) ** 0.5
        z, g = r(B, H, W, 16), r(B, H, W, 2)
        w1, b1, wf = r(16, 16, 1, 1) / 4, r(16) / 4, r(2, 16, 3, 3) / 12
        gamma, beta, mean, var = 1 + r(16) / 4, r(16) / 4, r(16) / 4, 0.5 + torch.rand(16, device=DEV, generator=gen)
        leaves = [t.requires_grad_() for t in (z, w1, b1, gamma, beta, wf)]
        for training in (False, True):
            out_h = ops.flow_head_train(*leaves[:5], mean.clone(), var.clone(), leaves[5], scale, training=training,
                                        momentum=MOMENTUM, eps=EPS)
            out_t = composed_head(*leaves[:5], mean, var, leaves[5], scale, training)
            det = [t.detach() for t in leaves]
            if training:
                params, stats = ops.flow_head_stats(*det[:5], None, None, det[5], MOMENTUM, EPS)
            else:
                params, stats = ops.pack_flow_head(*det[1:5], mean, var, EPS, det[5]), ops.frozen_stats(mean, var)
            row = measure(lambda: torch.autograd.grad(out_h, leaves, g, retain_graph=True),
                          lambda: torch.autograd.grad(out_t, leaves, g, retain_graph=True),
                          lambda: ops.flow_head_bwd(det[0], params, stats, scale, g, training, EPS), a.iters, a.warmup)
            nbytes = (72 + 136) * M
            row = dict(op="flow_head", batch_norm="batch" if training else "frozen", level=level, B=B, H=H, W=W,
                       bytes=nbytes, floor_us=nbytes / HBM / 1e3, **row)
            row["floor_over_call"] = row["floor_us"] / row["bwd_call_us"]
            rows.append(row)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
            del out_h, out_t
        x = r(B, H, W, 2).requires_grad_()
        gu = r(B, 2 * H, 2 * W, 2)
        up_h, up_t = ops.upsample2x_flow(x, 2.0), composed_upsample(x, 2.0)
        row = measure(lambda: torch.autograd.grad(up_h, [x], gu, retain_graph=True),
                      lambda: torch.autograd.grad(up_t, [x], gu, retain_graph=True),
                      lambda: ops.upsample2x_flow_bwd(gu, 2.0), a.iters, a.warmup)
        row = dict(op="upsample2x_flow", batch_norm=None, level=level, B=B, H=H, W=W, bytes=40 * M,
                   floor_us=40 * M / HBM / 1e3, **row)
        row["floor_over_call"] = row["floor_us"] / row["bwd_call_us"]
        rows.append(row)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
        del leaves, up_h, up_t
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "rows": rows},
                      fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Forward and backward of the cost volume (r = 4) and WarpV2 through torch autograd at the five config-2 level
shapes, HIP kernels vs torch autograd of a composed torch restatement on the same GPU.

    python tools/gradbench.py [--iters 20] [--warmup 5] [--json out.json]

Configs: B = 8 fp32 and B = 32 fp16.  Composed cost volume: F.pad + 81 x (slice, multiply, mean) + concat +
leaky_relu (oracle/torch_ref.py, layers.py:72-100); composed warp: the index-gather form of tfa's
interpolate_bilinear (warp.py:157-211).  Times are medians of HIP-event pairs around eager launches (the kernel
backward alone is also timed on its own: `bwd_kernel_us`, with its compulsory bytes and the fraction of 8 TB/s).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import torch_ref  # noqa: E402
from qpwcnet_amd import ops  # noqa: E402

PEAK = 8000.0   # GB/s, HBM
LEVELS = [(8, 16, 256), (16, 32, 256), (32, 64, 128), (64, 128, 64), (128, 256, 32)]


def composed_warp_v2(img, flo):
    """tfa dense_image_warp(img, -flo[..., ::-1]) as torch ops on the image's device."""
    B, H, W, C = img.shape
    gy, gx = torch.meshgrid(torch.arange(H, device=img.device), torch.arange(W, device=img.device), indexing="ij")
    qy = (gy.to(flo.dtype) + flo[..., 1]).reshape(B, -1)
    qx = (gx.to(flo.dtype) + flo[..., 0]).reshape(B, -1)
    fy = torch.clamp(torch.floor(qy), 0.0, float(H - 2))
    fx = torch.clamp(torch.floor(qx), 0.0, float(W - 2))
    ay = torch.clamp(qy - fy, 0.0, 1.0).unsqueeze(-1).to(img.dtype)
    ax = torch.clamp(qx - fx, 0.0, 1.0).unsqueeze(-1).to(img.dtype)
    iy, ix = fy.long(), fx.long()
    flat = img.reshape(B * H * W, C)
    boff = (torch.arange(B, device=img.device) * H * W).reshape(B, 1)

    def gather(y, x):
        return flat[(boff + y * W + x).reshape(-1)].reshape(B, -1, C)

    tl, tr, bl, br = gather(iy, ix), gather(iy, ix + 1), gather(iy + 1, ix), gather(iy + 1, ix + 1)
    top = ax * (tr - tl) + tl
    bot = ax * (br - bl) + bl
    return (ay * (bot - top) + top).reshape(B, H, W, C)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    return statistics.median(ts)


def fwd_bwd(f, inputs, gout, iters, warmup):
    fwd = timed(lambda: f(*inputs), iters, warmup)
    out = f(*inputs)
    bwd = timed(lambda: torch.autograd.grad(out, inputs, gout, retain_graph=True), iters, warmup)
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for B, dt in ((8, torch.float32), (32, torch.float16)):
        es = 4 if dt == torch.float32 else 2
        for lvl, (H, W, C) in enumerate(LEVELS):
            n = B * H * W
            prv = torch.randn(B, H, W, C, device=dev, generator=g).to(dt).requires_grad_()
            nxt = torch.randn(B, H, W, C, device=dev, generator=g).to(dt).requires_grad_()
            gcv = torch.randn(B, H, W, 81, device=dev, generator=g).to(dt)
            img = torch.rand(B, H, W, C, device=dev, generator=g).to(dt).requires_grad_()
            flo = (torch.randn(B, H, W, 2, device=dev, generator=g) * 4).requires_grad_()
            gw = torch.randn(B, H, W, C, device=dev, generator=g).to(dt)
            # cost volume
            hip = fwd_bwd(lambda p, q: ops.cost_volume(p, q), (prv, nxt), gcv, a.iters, a.warmup)
            ref = fwd_bwd(lambda p, q: torch_ref.cost_volume(p, q), (prv, nxt), gcv, max(3, a.iters // 4), 2)
            with torch.no_grad():
                out = ops.cost_volume(prv, nxt)
            pd, nd = prv.detach(), nxt.detach()
            kern = timed(lambda: ops.cost_volume_bwd(pd, nd, out, gcv), a.iters, a.warmup)
            floor_b = n * (4 * C + 2 * 81) * es
            rows.append(dict(op="cost_volume", B=B, dtype=str(dt).split(".")[-1], level="L%d" % lvl, H=H, W=W, C=C,
                             fwd_us=hip[0], bwd_us=hip[1], torch_fwd_us=ref[0], torch_bwd_us=ref[1],
                             bwd_kernel_us=kern, bwd_bytes=floor_b, bwd_floor_us=floor_b / PEAK / 1e3,
                             bwd_frac_of_floor=floor_b / PEAK / 1e3 / kern, bwd_speedup=ref[1] / hip[1]))
            # WarpV2
            hip = fwd_bwd(lambda i, f: ops.warp(i, f, "clamp"), (img, flo), gw, a.iters, a.warmup)
            ref = fwd_bwd(composed_warp_v2, (img, flo), gw, max(3, a.iters // 4), 2)
            idt, fd = img.detach(), flo.detach()
            kern = timed(lambda: ops.warp_bwd(idt, fd, gw, "clamp"), a.iters, a.warmup)
            # compulsory: img + grad_out reads, grad_img write (+ its zeroing), flow read + grad_flo write
            floor_b = n * (4 * C * es + 16)
            atomic_b = n * 4 * C * 4   # fp32 atomic payload (4 corners)
            rows.append(dict(op="warp_v2", B=B, dtype=str(dt).split(".")[-1], level="L%d" % lvl, H=H, W=W, C=C,
                             fwd_us=hip[0], bwd_us=hip[1], torch_fwd_us=ref[0], torch_bwd_us=ref[1],
                             bwd_kernel_us=kern, bwd_bytes=floor_b, bwd_floor_us=floor_b / PEAK / 1e3,
                             atomic_bytes=atomic_b, atomic_floor_us=atomic_b / 1300.0 / 1e3,
                             bwd_frac_of_floor=max(floor_b / PEAK, atomic_b / 1300.0) / 1e3 / kern,
                             bwd_speedup=ref[1] / hip[1]))
            for r in rows[-2:]:
                print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
            del prv, nxt, gcv, img, flo, gw, out
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

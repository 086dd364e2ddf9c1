#!/usr/bin/env python3
"""The interpolation stack's own kernels (csrc/interp.hip: image head, x2 upsampling of an image, frame pyramid) at the
interpolator's level shapes, against the torch compositions they replace on the same GPU, and one eager training step
of layers.InterpolatorModel with the new ops and with the three compositions swapped in.

    python tools/interpgradbench.py [--iters 20] [--warmup 5] [--json profiles/gradbench_interp.json] [--no-step]

Shapes: config 2 (B = 8 fp32 pairs of 256 x 512).  The five FrameInterpolate blocks run at 8x16, 16x32, 32x64, 64x128
and 128x256; the image head reads (8, H, W, 64) there, the upsampling doubles the (8, H, W, 3) image of each level, and
the pyramid takes the 16 stacked frames (16, 256, 512, 3) down five levels.  Times are medians of HIP-event pairs
around eager calls, the HIP op and the composition in one process, their order reversed from one iteration to the next.
Compositions: torch.addmm on the (M, 64) view and its autograd backward; F.interpolate(scale_factor=2, 'bilinear')
between the NHWC -> NCHW -> NHWC permutes of non_layers.Upsample and its autograd backward; five
F.avg_pool2d(2, ceil_mode, count_include_pad=False) between the same permutes.  floor_us = compulsory bytes at 8 TB/s;
at these sizes most rows are bound by the launch, not by the bytes."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import layers, loss, ops, synth  # noqa: E402

HBM = 8000.0     # GB/s
B = 8
HW = (256, 512)
LEVELS = tuple((k, HW[0] >> (5 - k), HW[1] >> (5 - k)) for k in range(5))   # block k, H, W
DEV = "cuda:0"


def head_composed(z, w2, b2):
    return torch.addmm(b2, z.reshape(-1, 64), w2.reshape(3, 64).t()).view(z.shape[:3] + (3,))


def upsample_composed(x, scale=1.0):
    y = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    return (y * scale).permute(0, 2, 3, 1).contiguous()


def pyramid_composed(x, levels):
    y = x.permute(0, 3, 1, 2)
    for _ in range(levels):
        y = F.avg_pool2d(y, 2, stride=2, ceil_mode=True, count_include_pad=False)
    return y.permute(0, 2, 3, 1).contiguous()


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def alternate(runs, iters, warmup):
    """{name: median us} of the callables, their order reversed every other iteration."""
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    times = {k: [] for k in runs}
    order = list(runs)
    for i in range(iters):
        for k in (order if i % 2 == 0 else order[::-1]):
            times[k].append(event_us(runs[k]))
    return {k: statistics.median(v) for k, v in times.items()}


def rel_diff(a, b):
    return max(float((p - q).abs().max() / max(1.0, float(q.abs().max()))) for p, q in zip(a, b))


def bench_head(k, H, W, gen, a):
    z = torch.randn(B, H, W, 64, device=DEV, generator=gen).requires_grad_()
    w2 = (torch.randn(3, 64, 1, 1, device=DEV, generator=gen) / 8).requires_grad_()
    b2 = (torch.randn(3, device=DEV, generator=gen) / 4).requires_grad_()
    g = torch.randn(B, H, W, 3, device=DEV, generator=gen)
    leaves = [z, w2, b2]
    det = [t.detach() for t in leaves]
    out_h, out_t = ops.image_head(*leaves), head_composed(*leaves)
    med = alternate({"hip_fwd": lambda: ops.image_head(*det), "torch_fwd": lambda: head_composed(*det),
                     "hip_bwd": lambda: torch.autograd.grad(out_h, leaves, g, retain_graph=True),
                     "torch_bwd": lambda: torch.autograd.grad(out_t, leaves, g, retain_graph=True),
                     "bwd_kernel": lambda: ops.image_head_bwd(det[0], det[1], g)}, a.iters, a.warmup)
    M = B * H * W
    err = rel_diff(torch.autograd.grad(out_h, leaves, g, retain_graph=True) + (out_h.detach(),),
                   torch.autograd.grad(out_t, leaves, g, retain_graph=True) + (out_t.detach(),))
    return dict(op="image_head", block=k, B=B, H=H, W=W, **{n + "_us": v for n, v in med.items()},
                fwd_floor_us=M * 268 / HBM / 1e3, bwd_floor_us=M * 524 / HBM / 1e3,
                fwd_speedup=med["torch_fwd"] / med["hip_fwd"], bwd_speedup=med["torch_bwd"] / med["hip_bwd"],
                max_rel_diff_vs_torch=err)


def bench_upsample(k, H, W, gen, a):
    x = torch.randn(B, H, W, 3, device=DEV, generator=gen).requires_grad_()
    g = torch.randn(B, 2 * H, 2 * W, 3, device=DEV, generator=gen)
    det = x.detach()
    out_h, out_t = ops.upsample2x_image(x), upsample_composed(x)
    med = alternate({"hip_fwd": lambda: ops.upsample2x_image(det), "torch_fwd": lambda: upsample_composed(det),
                     "hip_bwd": lambda: torch.autograd.grad(out_h, [x], g, retain_graph=True),
                     "torch_bwd": lambda: torch.autograd.grad(out_t, [x], g, retain_graph=True),
                     "bwd_kernel": lambda: ops.upsample2x_image_bwd(g)}, a.iters, a.warmup)
    n = B * H * W * 3 * 4
    err = rel_diff(torch.autograd.grad(out_h, [x], g, retain_graph=True) + (out_h.detach(),),
                   torch.autograd.grad(out_t, [x], g, retain_graph=True) + (out_t.detach(),))
    return dict(op="upsample2x_image", block=k, B=B, H=H, W=W, **{n_ + "_us": v for n_, v in med.items()},
                fwd_floor_us=5 * n / HBM / 1e3, bwd_floor_us=5 * n / HBM / 1e3,
                fwd_speedup=med["torch_fwd"] / med["hip_fwd"], bwd_speedup=med["torch_bwd"] / med["hip_bwd"],
                max_rel_diff_vs_torch=err)


def bench_pyramid(gen, a):
    x = torch.rand(2 * B, HW[0], HW[1], 3, device=DEV, generator=gen) - 0.5
    med = alternate({"hip_fwd": lambda: ops.avgpool_pyramid(x, 5), "torch_fwd": lambda: pyramid_composed(x, 5)},
                    a.iters, a.warmup)
    n = x.numel() * 4
    return dict(op="avgpool_pyramid", frames=2 * B, H=HW[0], W=HW[1], levels=5, **{k + "_us": v for k, v in med.items()},
                fwd_floor_us=(n + n / 1024) / HBM / 1e3, fwd_speedup=med["torch_fwd"] / med["hip_fwd"],
                max_rel_diff_vs_torch=rel_diff([ops.avgpool_pyramid(x, 5)], [pyramid_composed(x, 5)]))


def bench_step(a):
    """One eager training step of InterpolatorModel (forward, multiscale AutoResizeMseLoss over the six images,
    backward) with the ops of csrc/interp.hip and with the three compositions in their place."""
    weights = synth.make_interpolator_weights(42, HW)
    net = layers.InterpolatorModel(data_format="channels_last")
    net.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()})
    net = net.to(DEV).train()
    pairs = torch.as_tensor(synth.make_frames(B, HW[0], HW[1], seed=5)[0]).to(DEV)
    middle = 0.5 * (pairs[..., :3] + pairs[..., 3:]).contiguous()
    hip = (ops.image_head, ops.upsample2x_image, ops.avgpool_pyramid)
    composed = (head_composed, upsample_composed, pyramid_composed)

    def step(fns):
        ops.image_head, ops.upsample2x_image, ops.avgpool_pyramid = fns
        try:
            net.zero_grad(set_to_none=True)
            total = loss.multiscale(loss.AutoResizeMseLoss(), middle, net(pairs))[0]
            total.backward()
            return float(total.detach())
        finally:
            ops.image_head, ops.upsample2x_image, ops.avgpool_pyramid = hip

    losses = (step(hip), step(composed))
    med = alternate({"hip": lambda: step(hip), "composed": lambda: step(composed)}, a.iters, a.warmup)
    return dict(op="training_step", B=B, H=HW[0], W=HW[1], hip_step_us=med["hip"], composed_step_us=med["composed"],
                speedup=med["composed"] / med["hip"], loss_hip=losses[0], loss_composed=losses[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-step", action="store_true", help="skip the training step")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interpgradbench needs a HIP device")
    gen = torch.Generator(device=DEV).manual_seed(0)
    rows = []

    def add(row):
        rows.append(row)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)

    for k, H, W in LEVELS:
        add(bench_head(k, H, W, gen, a))
    for k, H, W in LEVELS:
        add(bench_upsample(k, H, W, gen, a))
    add(bench_pyramid(gen, a))
    if not a.no_step:
        add(bench_step(a))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "rows": rows}, fh,
                      indent=1)


if __name__ == "__main__":
    main()

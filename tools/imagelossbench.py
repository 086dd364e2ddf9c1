#!/usr/bin/env python3
"""The interpolator's SSIM + Charbonnier loss over its six levels (B = 8, C = 3, 256 x 512 down to 8 x 16;
qpwcnet_amd.loss.multiscale_image: qpwc_image_loss_fwd / _bwd) against the same loss composed from torch operators on
the same device (loss.multiscale_image_torch), forward + backward, both layouts.

    python tools/imagelossbench.py [--iters 30] [--warmup 5] [--json profiles/imagelossbench.json]
    python tools/imagelossbench.py --kernels-only      # the HIP path only, for rocprofv3 --kernel-trace --stats

Times.  `hip_fwd_bwd_us` / `torch_fwd_bwd_us`: medians of HIP-event pairs around eager calls, the two paths alternating; a
call's time includes its launches, its allocations and its Python, and both paths' include the per-level targets.
`device_us`: HIP events around the entry points alone (ops.kernel_timing), i.e. the device time of the targets' launch
('loss'), of the forward launch with its fold and of the backward launch.  The images are textured (a base level per
image and channel plus uniform noise of amplitude 0.25), the predictions the level's target plus noise of amplitude 0.05;
the torch chain gets the same tensors.  `rel_diff_vs_torch`: of the total; `grad_rel_diff_vs_torch`: the largest gradient
difference over the level's largest gradient, the worst level.
There is no performance gate and no parent to compare with: the numbers are written down as they are."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import loss, ops  # noqa: E402

B, C, H, W, LEVELS = 8, 3, 256, 512, 6


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def make_case(data_format, dev="cuda:0"):
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.rand(B, C, 1, 1, device=dev, generator=g) * 0.6 - 0.3
    y = (base + 0.25 * (2.0 * torch.rand(B, C, H, W, device=dev, generator=g) - 1.0)).clamp(-0.5, 0.5)
    shapes = [(H >> k, W >> k) for k in range(LEVELS - 1, -1, -1)]        # coarse to fine, as the model returns them
    preds = [t + 0.05 * (2.0 * torch.rand(t.shape, device=dev, generator=g) - 1.0)
             for t in ops.resized_ground_truth(y.contiguous(), shapes, "channels_first")]
    if data_format == "channels_last":
        y, preds = y.permute(0, 2, 3, 1), [p.permute(0, 2, 3, 1) for p in preds]
    return y.contiguous(), [p.contiguous().requires_grad_() for p in preds]


def run(data_format, iters, warmup):
    y, preds = make_case(data_format)
    obj = loss.ImageLoss(data_format=data_format)
    paths = {"hip": lambda: loss.multiscale_image(obj, y, preds),
             "torch": lambda: loss.multiscale_image_torch(obj, y, preds)}

    def fwd_bwd(f):
        for p in preds:
            p.grad = None
        f()[0].backward()

    fwd_bwd(paths["hip"])
    a, ga = paths["hip"](), [p.grad.clone() for p in preds]
    fwd_bwd(paths["torch"])
    c, gc = paths["torch"](), [p.grad.clone() for p in preds]
    diff = abs(float(a[0].detach()) - float(c[0].detach())) / abs(float(c[0].detach()))
    grad_diff = max(float((x - z).abs().max()) / float(z.abs().max()) for x, z in zip(ga, gc))
    parts = {k: [round(float(v), 6) for v in a[2][k]] for k in a[2]}
    del a, c, ga, gc
    ts = {k: [] for k in paths}
    for it in range(warmup + iters):
        for k, f in paths.items():                               # alternating: the paths see the same machine state
            t = event_us(lambda: fwd_bwd(f))
            if it >= warmup:
                ts[k].append(t)
    with ops.kernel_timing() as kt:
        for _ in range(iters):
            fwd_bwd(paths["hip"])
    device = {}
    for key, (n, ms) in kt.summary().items():
        if key[0] in ("loss", "image_loss", "image_loss_bwd"):
            calls, us = device.get(key[0], (0, 0.0))
            device[key[0]] = (calls + n, us + n * ms * 1000.0)
    device = {k: {"calls_per_step": n // iters, "us_per_step": us / iters} for k, (n, us) in device.items()}
    r = dict(data_format=data_format, B=B, C=C, H=H, W=W, levels=[list(s) for s in
             ([p.shape[1:3] for p in preds] if data_format == "channels_last" else [p.shape[2:] for p in preds])],
             iters=iters, warmup=warmup, parts=parts, rel_diff_vs_torch=diff, grad_rel_diff_vs_torch=grad_diff,
             device_us=device, hip_fwd_bwd_us=statistics.median(ts["hip"]),
             torch_fwd_bwd_us=statistics.median(ts["torch"]))
    r["torch_over_hip"] = r["torch_fwd_bwd_us"] / r["hip_fwd_bwd_us"]
    print(json.dumps({k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def kernels_only(iters):
    for data_format in ("channels_last", "channels_first"):
        y, preds = make_case(data_format)
        obj = loss.ImageLoss(data_format=data_format)
        for _ in range(iters):
            loss.multiscale_image(obj, y, preds)[0].backward()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("imagelossbench needs a HIP device: a CPU run gives no time")
    if a.kernels_only:
        kernels_only(a.iters)
        return
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [run(f, a.iters, a.warmup) for f in ("channels_last", "channels_first")]}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The label-free flow loss over the six levels of the bench config (B = 8, 256 x 512 down to 8 x 16;
qpwcnet_amd.loss.multiscale_unsupervised: qpwc_unsup_loss_fwd / _bwd) against the same loss composed from torch
operators on the same device (loss.multiscale_unsupervised_torch), forward + backward, both photometric kinds.

    python tools/unsuplossbench.py [--iters 30] [--warmup 5] [--json profiles/unsuplossbench.json]
    python tools/unsuplossbench.py --kernels-only      # the HIP path only, for rocprofv3 --kernel-trace --stats

Times.  `hip_fwd_bwd_us` / `torch_fwd_bwd_us`: medians of HIP-event pairs around eager calls, the two paths alternating; a
call's time includes its launches, its allocations and its Python, and the HIP path's includes the frame pyramid (5
launches).  `device_us`: HIP events around the entry points alone (ops.kernel_timing), i.e. the device time of the
forward launch with its fold, of the backward launch, and of the pooling launches.  The flows are random, a few pixels
large at every level, on smooth frames; the torch chain gets the same tensors.  `rel_diff_vs_torch`: of the total.
There is no performance gate and no parent to compare with: the numbers are written down as they are."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import loss, ops  # noqa: E402

B, H, W, LEVELS = 8, 256, 512, 6


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def make_case(dev="cuda:0"):
    g = torch.Generator(device=dev).manual_seed(0)
    yy = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1, 1)
    xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W, 1)
    phase = torch.rand(B, 1, 1, 6, device=dev, generator=g) * 6.28
    pairs = 0.3 * torch.sin(xx * 0.11 + phase) * torch.cos(yy * 0.07 + phase) + 0.02 * torch.randn(B, H, W, 6, device=dev,
                                                                                                 generator=g)
    flows = [(3.0 * torch.randn(B, H >> k, W >> k, 2, device=dev, generator=g)).requires_grad_()
             for k in range(LEVELS - 1, -1, -1)]
    return pairs.contiguous(), flows


def run(kind, iters, warmup):
    pairs, flows = make_case()
    obj = loss.PhotometricLoss(kind, data_format="channels_last")
    paths = {"hip": lambda: loss.multiscale_unsupervised(obj, pairs, flows, occluded="estimate"),
             "torch": lambda: loss.multiscale_unsupervised_torch(obj, pairs, flows, occluded="estimate")}

    def fwd_bwd(f):
        for p in flows:
            p.grad = None
        f()[0].backward()

    a, c = paths["hip"](), paths["torch"]()
    diff = abs(float(a[0].detach()) - float(c[0].detach())) / abs(float(c[0].detach()))
    counts_equal = bool(torch.equal(a[2]["counts"], c[2]["counts"]))
    counts = a[2]["counts"].tolist()
    del a, c
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
        if key[0] in ("unsup_loss", "unsup_loss_bwd", "avgpool_pyramid", "occlusion"):
            calls, us = device.get(key[0], (0, 0.0))
            device[key[0]] = (calls + n, us + n * ms * 1000.0)
    device = {k: {"calls_per_step": n // iters, "us_per_step": us / iters} for k, (n, us) in device.items()}
    r = dict(kind=kind, B=B, H=H, W=W, levels=[list(p.shape[1:3]) for p in flows], iters=iters, warmup=warmup,
             counts=counts, counts_equal_torch=counts_equal, rel_diff_vs_torch=diff, device_us=device,
             hip_fwd_bwd_us=statistics.median(ts["hip"]), torch_fwd_bwd_us=statistics.median(ts["torch"]))
    r["torch_over_hip"] = r["torch_fwd_bwd_us"] / r["hip_fwd_bwd_us"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def kernels_only(iters):
    pairs, flows = make_case()
    for kind in ("census", "charbonnier"):
        obj = loss.PhotometricLoss(kind, data_format="channels_last")
        for _ in range(iters):
            loss.multiscale_unsupervised(obj, pairs, flows, occluded="estimate")[0].backward()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unsuplossbench needs a HIP device: a CPU run gives no time")
    if a.kernels_only:
        kernels_only(a.iters)
        return
    doc = {"device": torch.cuda.get_device_name(0), "cases": [run(k, a.iters, a.warmup) for k in ("census", "charbonnier")]}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()

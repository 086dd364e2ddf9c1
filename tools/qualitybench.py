#!/usr/bin/env python3
"""The interpolator's image quality on the HIP kernels (qpwcnet_amd.metrics.image_quality on CUDA images:
qpwc_image_quality_fwd, two launches) against the same numbers composed from torch operators on the same device
(metrics.image_quality_torch: the value transform, eight depthwise convolutions of 11 taps and the elementwise chain of
s).  Two cases, both scored as the 8-bit pictures of images in [-0.5, 0.5] (offset 0.5, quantize): the trainer's shape
(pre_train.py: batch 16, 256 x 512 x 3) and one Vimeo-90K frame (1 x 256 x 448 x 3).

    python tools/qualitybench.py [--iters 200] [--warmup 20] [--json profiles/qualitybench.json]
    python tools/qualitybench.py --kernels-only [--case trainer]     # the HIP path only: the target of
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <name> -- \
            python tools/qualitybench.py --kernels-only --case trainer --iters 100

Times: medians of HIP-event pairs around eager calls, the two paths alternating; a call's time includes its launches,
its allocations and its Python.  Algorithmic bytes from the shapes: both images read once (2 * 4 * B * H * W * C); the
fraction is of 8 TB/s.  The kernel is bound by LDS and vector arithmetic, not by HBM: there is no performance gate, the
numbers are written down as they are.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import metrics  # noqa: E402

PEAK = 8000.0   # GB/s, HBM
CASES = {"trainer": (16, 256, 512, 3), "vimeo_frame": (1, 256, 448, 3)}
DATA_FORMAT = "channels_last"
KW = dict(offset=(0.5, 0.5), quantize=True)


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def make_images(shape, dev="cuda:0"):
    """A smooth picture with a little texture in [-0.5, 0.5] and a prediction 0.04 (RMS) away from it."""
    g = torch.Generator(device=dev).manual_seed(0)
    B, H, W, C = shape
    y = torch.arange(H, device=dev).view(1, H, 1, 1) / H
    x = torch.arange(W, device=dev).view(1, 1, W, 1) / W
    c = torch.arange(C, device=dev).view(1, 1, 1, C)
    truth = 0.35 * torch.sin(6.2831853 * (y + 1.5 * x) + 0.7 * c) + 0.05 * torch.randn(shape, device=dev, generator=g)
    pred = truth + 0.04 * torch.randn(shape, device=dev, generator=g)
    return truth.contiguous(), pred.contiguous()


def run(name, iters, warmup, dev="cuda:0"):
    shape = CASES[name]
    truth, pred = make_images(shape, dev)
    fns = {"hip": lambda: metrics.image_quality(truth, pred, data_format=DATA_FORMAT, **KW),
           "torch": lambda: metrics.image_quality_torch(truth, pred, data_format=DATA_FORMAT, **KW)}
    x, y = fns["hip"](), fns["torch"]()
    diff = dict(mse_rel=float(((x.mse - y.mse) / y.mse).abs().max()), psnr_db=float((x.psnr - y.psnr).abs().max()),
                ssim=float((x.ssim - y.ssim).abs().max()))
    mean = dict(psnr_db=float(x.psnr.mean()), ssim=float(x.ssim.mean()))
    del x, y
    for _ in range(warmup):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():           # alternating: the paths see the same machine state
            ts[k].append(event_us(f))
    B, H, W, C = shape
    r = dict(case=name, B=B, H=H, W=W, C=C, data_format=DATA_FORMAT, offset=KW["offset"], quantize=True, iters=iters,
             warmup=warmup, algorithmic_bytes=2 * 4 * B * H * W * C, diff_vs_torch=diff, mean=mean)
    r.update(hip_us=statistics.median(ts["hip"]), hip_min_us=min(ts["hip"]), torch_us=statistics.median(ts["torch"]),
             torch_min_us=min(ts["torch"]))
    r["floor_us"] = r["algorithmic_bytes"] / PEAK / 1e3
    r["hip_frac_of_peak"] = r["floor_us"] / r["hip_us"]
    r["speedup"] = r["torch_us"] / r["hip_us"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def kernels_only(iters, names):
    for name in names:
        truth, pred = make_images(CASES[name])
        for _ in range(iters):
            metrics.image_quality(truth, pred, data_format=DATA_FORMAT, **KW)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="one case (default: both)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qualitybench needs a HIP device: a CPU run gives no time")
    names = list(CASES) if a.case is None else [a.case]
    if a.kernels_only:
        kernels_only(a.iters, names)
        return
    doc = {"device": torch.cuda.get_device_name(0), "peak_gbps": PEAK, "cases": [run(n, a.iters, a.warmup) for n in names]}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()

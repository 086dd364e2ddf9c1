#!/usr/bin/env python3
"""The flow evaluation metrics on the HIP kernels (qpwcnet_amd.metrics.flow_quality on CUDA flows:
qpwc_flow_quality_fwd, two launches) against the same numbers composed from torch operators on the same device
(metrics.flow_quality_torch: the per-pixel chain, seven masks and fifteen float64 reductions).  Two shapes, a
validation batch of the trainer's size (8 x 256 x 512) and a batch of full-resolution frames (16 x 1024 x 2048), each
without masks and with both masks (uint8 valid, 90 % set; uint8 occluded, 20 % set).

    python tools/flowqualitybench.py [--iters 100] [--warmup 10] [--json profiles/flowqualitybench.json]
    python tools/flowqualitybench.py --kernels-only [--case full_masks]     # the HIP path only: the target of
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <name> -- \
            python tools/flowqualitybench.py --kernels-only --case full_masks --iters 100

Times: medians of HIP-event pairs around eager calls, the two paths alternating; a call's time includes its launches,
its allocations and its Python.  `graph_us` is the two launches alone, replayed from a captured graph (the replay's own
fixed cost included).  Algorithmic bytes from the shapes: both flows read once (16 B a pixel in fp32) plus one byte a
pixel per mask; the fraction is of 8 TB/s.  There is no performance gate: the numbers are written down as they are.
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
CASES = {"batch": ((8, 256, 512), False), "batch_masks": ((8, 256, 512), True),
         "full": ((16, 1024, 2048), False), "full_masks": ((16, 1024, 2048), True)}
DATA_FORMAT = "channels_last"


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def make_flows(shape, masks, dev="cuda:0"):
    """A smooth flow of up to about 60 px with a little texture and a prediction 1 px (RMS per component) away from it;
    one pixel in a thousand of the ground truth is marked unknown (1e10)."""
    g = torch.Generator(device=dev).manual_seed(0)
    B, H, W = shape
    y = torch.arange(H, device=dev).view(1, H, 1, 1) / H
    x = torch.arange(W, device=dev).view(1, 1, W, 1) / W
    c = torch.arange(2, device=dev).view(1, 1, 1, 2)
    truth = 45.0 * torch.sin(6.2831853 * (y + 1.5 * x) + 1.3 * c) + torch.randn((B, H, W, 2), device=dev, generator=g)
    pred = truth + torch.randn((B, H, W, 2), device=dev, generator=g)
    truth = torch.where(torch.rand((B, H, W, 1), device=dev, generator=g) < 1e-3, torch.full_like(truth, 1e10), truth)
    valid = occluded = None
    if masks:
        valid = (torch.rand((B, H, W), device=dev, generator=g) < 0.9).to(torch.uint8)
        occluded = (torch.rand((B, H, W), device=dev, generator=g) < 0.2).to(torch.uint8)
    return truth.contiguous(), pred.contiguous(), valid, occluded


def run(name, iters, warmup, dev="cuda:0"):
    shape, masks = CASES[name]
    truth, pred, valid, occluded = make_flows(shape, masks, dev)
    kw = dict(valid=valid, occluded=occluded, data_format=DATA_FORMAT)
    fns = {"hip": lambda: metrics.flow_quality(truth, pred, **kw),
           "torch": lambda: metrics.flow_quality_torch(truth, pred, **kw)}
    x, y = fns["hip"](), fns["torch"]()
    diff = {k: float((a - b).abs().nan_to_num().max()) for k, a, b in zip(x._fields, x, y)}
    # None: a mean over an empty set (no occlusion mask; no ground truth slower than 10 px in these flows)
    mean = {k: (None if bool(torch.isnan(a).any()) else float(a.mean())) for k, a in zip(x._fields, x)}
    del x, y
    for _ in range(warmup):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():           # alternating: the paths see the same machine state
            ts[k].append(event_us(f))
    # the two launches alone: one capture, replayed
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fns["hip"]()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fns["hip"]()
    for _ in range(warmup):
        graph.replay()
    ts["graph"] = [event_us(graph.replay) for _ in range(iters)]
    del keep, graph
    B, H, W = shape
    per_pixel = 16 + (2 if masks else 0)
    r = dict(case=name, B=B, H=H, W=W, masks=masks, data_format=DATA_FORMAT, iters=iters, warmup=warmup,
             bytes_per_pixel=per_pixel, algorithmic_bytes=per_pixel * B * H * W, diff_vs_torch=diff, mean=mean)
    r.update(hip_us=statistics.median(ts["hip"]), hip_min_us=min(ts["hip"]), graph_us=statistics.median(ts["graph"]),
             graph_min_us=min(ts["graph"]), torch_us=statistics.median(ts["torch"]), torch_min_us=min(ts["torch"]))
    r["floor_us"] = r["algorithmic_bytes"] / PEAK / 1e3
    r["hip_frac_of_peak"] = r["floor_us"] / r["hip_us"]
    r["graph_frac_of_peak"] = r["floor_us"] / r["graph_us"]
    r["speedup"] = r["torch_us"] / r["hip_us"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def kernels_only(iters, names):
    for name in names:
        shape, masks = CASES[name]
        truth, pred, valid, occluded = make_flows(shape, masks)
        for _ in range(iters):
            metrics.flow_quality(truth, pred, valid=valid, occluded=occluded, data_format=DATA_FORMAT)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="one case (default: all four)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flowqualitybench needs a HIP device: a CPU run gives no time")
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

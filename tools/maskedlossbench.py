#!/usr/bin/env python3
"""The valid-masked FlowMseLossV2 over five area levels (qpwcnet_amd.loss.multiscale_masked: qpwc_masked_loss_fwd /
_bwd) against
  (b) the dense loss at the same shapes (loss.multiscale: existing, unchanged code), and
  (c) the same masked loss composed from torch operators on the same device (loss.multiscale_masked_torch),
forward (no grad) and forward + backward.  Two shapes: the trainer's batch (8 x 256 x 512, levels 128 x 256 .. 8 x 16)
and a batch of full-resolution frames (16 x 1024 x 2048, levels 512 x 1024 .. 32 x 64).  The ground truth is 30 % dense:
NaN elsewhere for half of the invalid pixels, a zero uint8 mask for the other half.  The dense loss gets the same
tensor with its invalid pixels set to 0 (the input pipeline's scrub).

    python tools/maskedlossbench.py [--iters 50] [--warmup 5] [--json profiles/maskedlossbench.json]
    python tools/maskedlossbench.py --kernels-only [--case full]      # the HIP path only: the target of
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <name> -- \
            python tools/maskedlossbench.py --kernels-only --case full --iters 50
    python tools/maskedlossbench.py --merge-stats full=<..._kernel_stats.csv> --json profiles/maskedlossbench.json

Times: medians of HIP-event pairs around eager calls, the three paths alternating; a call's time includes its launches,
its allocations and its Python.  `*_graph_us` is the no-grad forward's two launches alone, replayed from a captured
graph (the replay's own fixed cost included).  Algorithmic bytes from the shapes: the forward reads the ground truth (8 B
a pixel), the mask (1 B a pixel) and every prediction and, with grad, writes d term / d pred (8 B a level pixel); the
backward reads that and writes the gradients.  The fractions are of 8 TB/s.  Launches: counted from one profiled call.
There is no performance gate: the numbers are written down as they are.
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import loss  # noqa: E402

PEAK = 8000.0   # GB/s, HBM
CASES = {"trainer": (8, 256, 512), "full": (16, 1024, 2048)}


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def make_case(name, dev="cuda:0"):
    """-> (sparse ground truth, uint8 mask, scrubbed ground truth, predictions)."""
    B, H, W = CASES[name]
    g = torch.Generator(device=dev).manual_seed(0)
    gt = 4.0 * torch.randn(B, H, W, 2, device=dev, generator=g)
    keep = torch.rand(B, H, W, device=dev, generator=g) < 0.3
    by_nan = ~keep & (torch.rand(B, H, W, device=dev, generator=g) < 0.5)
    sparse = torch.where(by_nan[..., None], torch.full_like(gt, float("nan")), gt)
    valid = (keep | by_nan).to(torch.uint8)                    # the NaN pixels are marked valid: the values rule them out
    scrubbed = torch.where(keep[..., None], gt, torch.zeros_like(gt))
    preds = [torch.randn(B, H >> k, W >> k, 2, device=dev, generator=g).requires_grad_() for k in range(1, 6)]
    return sparse.contiguous(), valid.contiguous(), scrubbed.contiguous(), preds


def launches(fn):
    """Device kernels of one call, from torch's profiler; None where it records none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:                                            # no tracer in this build: the count is left out
        return None


def run(name, iters, warmup):
    sparse, valid, scrubbed, preds = make_case(name)
    obj = loss.FlowMseLossV2()
    paths = {"masked": lambda: loss.multiscale_masked(obj, sparse, preds, valid)[0],
             "dense": lambda: loss.multiscale(obj, scrubbed, preds)[0],
             "torch": lambda: loss.multiscale_masked_torch(obj, sparse, preds, valid)[0]}

    def fwd(f):
        with torch.no_grad():
            f()

    def fwd_bwd(f):
        for p in preds:
            p.grad = None
        f().backward()

    a, c = paths["masked"](), paths["torch"]()
    diff = abs(float(a.detach()) - float(c.detach())) / abs(float(c.detach()))
    del a, c
    ts = {(k, m): [] for k in paths for m in ("fwd", "fwd_bwd")}
    for it in range(warmup + iters):
        for k, f in paths.items():                               # alternating: the paths see the same machine state
            for m, step in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                t = event_us(lambda: step(f))
                if it >= warmup:
                    ts[(k, m)].append(t)
    graph_us = {}
    for k in ("masked", "dense"):                                # the no-grad forward's two launches alone
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            paths[k]()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph):
            keepalive = paths[k]()
        for _ in range(warmup):
            graph.replay()
        graph_us[k] = statistics.median([event_us(graph.replay) for _ in range(iters)])
        del keepalive, graph
    B, H, W = CASES[name]
    level_px = sum(p.numel() // 2 for p in preds)
    fwd_b = B * H * W * 9 + level_px * 8
    fb_b = fwd_b + level_px * 8 + level_px * 16
    r = dict(case=name, B=B, H=H, W=W, levels=[list(p.shape[1:3]) for p in preds], iters=iters, warmup=warmup,
             valid_share=float(valid.float().mean()), rel_diff_vs_torch=diff,
             fwd_bytes=fwd_b, fwd_train_bytes=fwd_b + level_px * 8, fwd_bwd_bytes=fb_b, dense_fwd_bytes=fwd_b - B * H * W,
             fwd_floor_us=fwd_b / PEAK / 1e3, fwd_bwd_floor_us=fb_b / PEAK / 1e3)
    for (k, m), v in ts.items():
        r["{}_{}_us".format(k, m)] = statistics.median(v)
    for k, v in graph_us.items():
        r["{}_fwd_graph_us".format(k)] = v
    r["masked_over_dense_fwd"] = r["masked_fwd_us"] / r["dense_fwd_us"]
    r["masked_over_dense_fwd_bwd"] = r["masked_fwd_bwd_us"] / r["dense_fwd_bwd_us"]
    r["masked_over_dense_fwd_graph"] = r["masked_fwd_graph_us"] / r["dense_fwd_graph_us"]
    r["masked_over_torch_fwd"] = r["masked_fwd_us"] / r["torch_fwd_us"]
    r["masked_over_torch_fwd_bwd"] = r["masked_fwd_bwd_us"] / r["torch_fwd_bwd_us"]
    r["fwd_graph_frac_of_peak"] = r["fwd_floor_us"] / r["masked_fwd_graph_us"]
    r["fwd_bwd_frac_of_peak"] = r["fwd_bwd_floor_us"] / r["masked_fwd_bwd_us"]
    r["launches"] = {"{}_{}".format(k, m): launches(lambda: step(f)) for k, f in paths.items()
                     for m, step in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def kernels_only(iters, names):
    obj = loss.FlowMseLossV2()
    for name in names:
        sparse, valid, scrubbed, preds = make_case(name)
        for _ in range(iters):
            loss.multiscale_masked(obj, sparse, preds, valid)[0].backward()
            loss.multiscale(obj, scrubbed, preds)[0].backward()
        torch.cuda.synchronize()


def merge_stats(path_json, specs):
    """Kernel times of a rocprofv3 --kernel-trace --stats run of --kernels-only --case NAME, into the case's row."""
    with open(path_json) as fh:
        doc = json.load(fh)
    for spec in specs:
        name, csv_path = spec.split("=", 1)
        stats = {}
        with open(csv_path) as fh:
            for row in csv.DictReader(fh):
                if "loss_" in row["Name"]:
                    stats[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                                        "min_us": float(row["MinNs"]) / 1e3}
        for r in doc["cases"]:
            if r["case"] == name:
                r["kernel_stats"] = stats
                tile = [v for k, v in stats.items() if "masked_loss_tile_kernel" in k]
                if tile:
                    r["fwd_kernel_us"] = tile[0]["avg_us"]
                    r["fwd_kernel_frac_of_peak"] = r["fwd_train_bytes"] / PEAK / 1e3 / tile[0]["avg_us"]
    with open(path_json, "w") as fh:
        json.dump(doc, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="one case (default: both)")
    ap.add_argument("--merge-stats", nargs="*", default=None, metavar="CASE=CSV")
    a = ap.parse_args()
    if a.merge_stats is not None:
        merge_stats(a.json, a.merge_stats)
        return
    if not torch.cuda.is_available():
        raise SystemExit("maskedlossbench needs a HIP device: a CPU run gives no time")
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

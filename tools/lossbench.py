#!/usr/bin/env python3
"""The fused multi-scale training losses (qpwcnet_amd.loss.multiscale: one forward kernel + fold, one backward kernel)
against a composed-torch version of the same losses with torch autograd (reshape-mean, F.interpolate, F.huber_loss,
vector norms, F.mse_loss), at the five prediction levels (area factors 2..32) of three configs:

    config 2: B = 8,  GT 256 x 512,   fp32 predictions
    config 4: B = 16, GT 1024 x 2048, fp32 predictions
    config 5: B = 32, GT 256 x 512,   fp16 predictions

    python tools/lossbench.py [--iters 20] [--warmup 5] [--json profiles/lossbench.json]
    python tools/lossbench.py --kernels-only --config 4          # the fused path only: the target of
        rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/lossbench.py --kernels-only --config 4
    python tools/lossbench.py --merge-stats 4=<..._kernel_stats.csv> [...] --json profiles/lossbench.json

Step times: medians of HIP-event pairs around eager calls, forward under torch.no_grad() and forward + backward
(total.backward()).  Byte floor from the shapes: forward = GT once + predictions once; forward + backward additionally
the fp32 derivative written and read once and the gradient written once; the fraction is of 8 TB/s.  Kernel times
come from the rocprofv3 runs (--merge-stats adds them to the JSON: the forward kernel alone against the forward floor).
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import loss  # noqa: E402

PEAK = 8000.0   # GB/s, HBM
CONFIGS = {2: (8, 256, 512, torch.float32), 4: (16, 1024, 2048, torch.float32), 5: (32, 256, 512, torch.float16)}
KINDS = ("FlowMseLossV2", "FlowMseLoss", "FlowMseLossFineTune", "AutoResizeMseLoss")


def composed(kind, gt, preds):
    """The same per-level losses from torch ops, channels_last operands, summed over the levels."""
    B, H, W, C = gt.shape
    x = gt.permute(0, 3, 1, 2)
    total = 0.0
    for p in preds:
        p = p.float()
        h, w = p.shape[1], p.shape[2]
        if kind == "FlowMseLossV2":
            g = gt.reshape(B, h, H // h, w, W // w, C).mean(dim=(2, 4)) * (h / H)
            s = 2.0 / (w + h)
            total = total + F.huber_loss(s * p, s * g, delta=0.1)
            continue
        g = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        if kind == "AutoResizeMseLoss":
            total = total + F.mse_loss(p, g)
            continue
        r = g * (h / H) - p
        n = torch.linalg.vector_norm(r, 2 if kind == "FlowMseLoss" else 1, dim=-1)
        total = total + (n.mean() if kind == "FlowMseLoss" else (n + 0.01).pow(0.4).mean())
    return total


def fused(kind, gt, preds):
    return loss.multiscale(getattr(loss, kind)(*(["channels_last"] if kind in ("FlowMseLoss", "FlowMseLossFineTune")
                                                  else [])), gt, preds)[0]


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


def case(cfg, kind, dev):
    B, H, W, dt = CONFIGS[cfg]
    C = 3 if kind == "AutoResizeMseLoss" else 2
    g = torch.Generator(device=dev).manual_seed(cfg)
    gt = torch.randn(B, H, W, C, device=dev, generator=g)
    preds = [torch.randn(B, H >> k, W >> k, C, device=dev, generator=g).to(dt).requires_grad_() for k in range(1, 6)]
    return gt, preds


def floors(gt, preds):
    gt_b = gt.numel() * 4
    pred_b = sum(p.numel() * p.element_size() for p in preds)
    d_b = sum(p.numel() * 4 for p in preds)
    return gt_b + pred_b, gt_b + pred_b + 2 * d_b + pred_b


def run(cfgs, iters, warmup):
    dev = "cuda:0"
    rows = []
    for cfg in cfgs:
        for kind in KINDS:
            gt, preds = case(cfg, kind, dev)
            fwd_b, fb_b = floors(gt, preds)

            def fwd(f):
                with torch.no_grad():
                    f(kind, gt, preds)

            def fwd_bwd(f):
                for p in preds:
                    p.grad = None
                f(kind, gt, preds).backward()

            r = dict(config=cfg, loss=kind, B=gt.shape[0], H=gt.shape[1], W=gt.shape[2],
                     pred_dtype=str(preds[0].dtype).split(".")[-1], levels=[list(p.shape[1:3]) for p in preds],
                     fwd_us=timed(lambda: fwd(fused), iters, warmup),
                     fwd_bwd_us=timed(lambda: fwd_bwd(fused), iters, warmup),
                     torch_fwd_us=timed(lambda: fwd(composed), max(3, iters // 2), 2),
                     torch_fwd_bwd_us=timed(lambda: fwd_bwd(composed), max(3, iters // 2), 2),
                     fwd_bytes=fwd_b, fwd_bwd_bytes=fb_b)
            r["fwd_floor_us"] = fwd_b / PEAK / 1e3
            r["fwd_bwd_floor_us"] = fb_b / PEAK / 1e3
            r["fwd_frac_of_floor"] = r["fwd_floor_us"] / r["fwd_us"]
            r["fwd_bwd_frac_of_floor"] = r["fwd_bwd_floor_us"] / r["fwd_bwd_us"]
            r["fwd_speedup"] = r["torch_fwd_us"] / r["fwd_us"]
            r["fwd_bwd_speedup"] = r["torch_fwd_bwd_us"] / r["fwd_bwd_us"]
            rows.append(r)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
            del gt, preds
            torch.cuda.empty_cache()
    return rows


def kernels_only(cfg, iters):
    """The fused path of every loss, forward (no grad) then forward + backward, `iters` times each."""
    for kind in KINDS:
        gt, preds = case(cfg, kind, "cuda:0")
        for _ in range(iters):
            with torch.no_grad():
                fused(kind, gt, preds)
        for _ in range(iters):
            fused(kind, gt, preds).backward()
        torch.cuda.synchronize()


def merge_stats(path_json, specs):
    with open(path_json) as fh:
        doc = json.load(fh)
    doc.setdefault("kernel_stats", {})
    for spec in specs:
        cfg, csv_path = spec.split("=", 1)
        stats = {}
        with open(csv_path) as fh:
            for row in csv.DictReader(fh):
                if "loss_" in row["Name"]:
                    stats[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                          "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
        doc["kernel_stats"]["config%s" % cfg] = stats
        # FlowMseLossV2's forward kernel alone against its floor (GT once + predictions once)
        tile = [v for k, v in stats.items() if "loss_area_tile_kernel" in k]
        for r in doc["rows"]:
            if str(r["config"]) == cfg and r["loss"] == "FlowMseLossV2" and tile:
                r["fwd_kernel_us"] = tile[0]["min_us"]
                r["fwd_kernel_frac_of_floor"] = r["fwd_floor_us"] / tile[0]["min_us"]
    with open(path_json, "w") as fh:
        json.dump(doc, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, action="append", choices=sorted(CONFIGS))
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-stats", nargs="*", default=None, metavar="CONFIG=CSV")
    a = ap.parse_args()
    if a.merge_stats is not None:
        merge_stats(a.json, a.merge_stats)
        return
    cfgs = a.config or sorted(CONFIGS)
    if a.kernels_only:
        for cfg in cfgs:
            kernels_only(cfg, a.iters)
        return
    rows = run(cfgs, a.iters, a.warmup)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "peak_gbps": PEAK, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

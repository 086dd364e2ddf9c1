#!/usr/bin/env python3
"""The training input pipeline on the HIP kernels (qpwcnet_amd.augment.preprocess on a CUDA batch: qpwc_augment_fwd, two
launches) against the same chain composed from torch operators on the same device (augment.augment_torch:
F.interpolate per sample, indexing for flips and crop, elementwise colour stages), at the trainer's shape:

    B = 16, source 540 x 960 uint8 frames + fp32 flow, base scale 0.56, output 256 x 512, channels_first

    python tools/augbench.py [--iters 30] [--warmup 5] [--json profiles/augbench.json]
    python tools/augbench.py --kernels-only          # the HIP path only: the target of
        rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/augbench.py --kernels-only
    python tools/augbench.py --merge-stats <..._kernel_stats.csv> --json profiles/augbench.json

Call times: medians of HIP-event pairs around eager calls with the parameters already drawn (the draw itself is timed
separately), the two paths alternating.  Algorithmic bytes from the shapes: the source frames and flow read once, both
outputs written once; the fraction is of 8 TB/s.  The colour stage's second launch reads and writes the image output
once more (`traffic_bytes`).  Kernel times come from the rocprofv3 run (--merge-stats adds them to the JSON).
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import augment  # noqa: E402

PEAK = 8000.0   # GB/s, HBM
SHAPE = dict(B=16, H=540, W=960, h=256, w=512, base_scale=0.56, data_format="channels_first")


def case(dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    B, H, W = SHAPE["B"], SHAPE["H"], SHAPE["W"]
    ims = torch.randint(0, 256, (B, H, W, 6), device=dev, generator=g, dtype=torch.uint8)
    flo = torch.randn(B, H, W, 2, device=dev, generator=g) * 8.0
    params = augment.sample_params(B, (H, W), (SHAPE["h"], SHAPE["w"]), SHAPE["base_scale"], generator=g, device=dev)
    return ims, flo, params


def hip_path(ims, flo, params):
    return augment.preprocess(ims, flo, SHAPE["data_format"], SHAPE["base_scale"], (SHAPE["h"], SHAPE["w"]), params=params)


def torch_path(ims, flo, params):
    return augment.augment_torch(ims, flo, params, (SHAPE["h"], SHAPE["w"]), data_format=SHAPE["data_format"])


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def run(iters, warmup):
    dev = "cuda:0"
    ims, flo, params = case(dev)
    fns = {"hip": lambda: hip_path(ims, flo, params), "torch": lambda: torch_path(ims, flo, params),
           "draw": lambda: augment.sample_params(SHAPE["B"], (SHAPE["H"], SHAPE["W"]), (SHAPE["h"], SHAPE["w"]),
                                                 SHAPE["base_scale"], device=dev)}
    a, b = fns["hip"](), fns["torch"]()
    diff = [float((x - y).abs().max()) for x, y in zip(a, b)]
    del a, b
    for _ in range(warmup):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():           # alternating: both paths see the same machine state
            ts[k].append(event_us(f))
    B, H, W, h, w = (SHAPE[k] for k in "BHWhw")
    src_b, out_b = B * H * W * (6 + 8), B * h * w * 8 * 4
    r = dict(SHAPE)
    r.update(hip_us=statistics.median(ts["hip"]), hip_min_us=min(ts["hip"]), torch_us=statistics.median(ts["torch"]),
             torch_min_us=min(ts["torch"]), draw_us=statistics.median(ts["draw"]), iters=iters,
             algorithmic_bytes=src_b + out_b, traffic_bytes=src_b + out_b + 2 * B * h * w * 6 * 4,
             max_abs_diff_ims=diff[0], max_abs_diff_flo=diff[1])
    r["floor_us"] = r["algorithmic_bytes"] / PEAK / 1e3
    r["hip_frac_of_peak"] = r["floor_us"] / r["hip_us"]
    r["speedup"] = r["torch_us"] / r["hip_us"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def kernels_only(iters):
    ims, flo, params = case("cuda:0")
    for _ in range(iters):
        hip_path(ims, flo, params)
    torch.cuda.synchronize()


def merge_stats(path_json, csv_path):
    with open(path_json) as fh:
        doc = json.load(fh)
    stats = {}
    with open(csv_path) as fh:
        for row in csv.DictReader(fh):
            if "augment_" in row["Name"]:
                stats[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                      "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    doc["kernel_stats"] = stats
    if stats:
        doc["kernel_us"] = sum(v["avg_us"] for v in stats.values())
        doc["kernel_frac_of_peak"] = doc["floor_us"] / doc["kernel_us"]
    with open(path_json, "w") as fh:
        json.dump(doc, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-stats", default=None, metavar="CSV")
    a = ap.parse_args()
    if a.merge_stats is not None:
        merge_stats(a.json, a.merge_stats)
        return
    if not torch.cuda.is_available():
        raise SystemExit("augbench needs a HIP device: a CPU run gives no time")
    if a.kernels_only:
        kernels_only(a.iters)
        return
    r = run(a.iters, a.warmup)
    if a.json:
        doc = {"device": torch.cuda.get_device_name(0), "peak_gbps": PEAK}
        doc.update(r)
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()

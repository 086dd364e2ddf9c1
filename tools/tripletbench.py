#!/usr/bin/env python3
"""The frame interpolator's input pipeline on the HIP kernel (qpwcnet_amd.augment.preprocess_triplet on a CUDA batch:
qpwc_augment_triplet_fwd, one launch) against the same chain composed op for op from torch operators on the same device
(augment.triplet_torch: F.interpolate, the colour einsum, a noise field, two conditional flips, - 0.5, concat, permute)
with the field drawn by torch.randn -- the reference's noise is any N(0, sigma) draw, so the composition is not charged
for Philox in integer operators.  Two cases, both B = 8, uint8 frames, channels_first:

    resize   256 x 448 -> 256 x 512        same   256 x 512 -> 256 x 512

    python tools/tripletbench.py [--iters 200] [--warmup 20] [--json profiles/tripletbench.json]
    python tools/tripletbench.py --kernels-only --case resize      # the HIP path of one case only: the target of
        rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/tripletbench.py --kernels-only --case resize
    python tools/tripletbench.py --merge-stats <..._kernel_stats.csv> --case resize --json profiles/tripletbench.json

Times: medians of HIP-event pairs around eager calls with the parameters already drawn (the draw itself is timed
separately), the paths alternating.  Algorithmic bytes from the shapes: the three source frames read once
(3 * 3 * B * H * W) and both outputs written once (9 * 4 * B * h * w); the fraction is of 8 TB/s.  A call's time is
mostly the launch and its Python; the kernel's own time comes from the rocprofv3 run (--merge-stats adds it to the JSON).
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
CASES = {"resize": dict(B=8, H=256, W=448, h=256, w=512), "same": dict(B=8, H=256, W=512, h=256, w=512)}
DATA_FORMAT = "channels_first"


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def case(shape, dev="cuda:0"):
    B, H, W = (shape[k] for k in "BHW")
    g = torch.Generator(device=dev).manual_seed(0)
    a, b, c = (torch.randint(0, 256, (B, H, W, 3), device=dev, generator=g, dtype=torch.uint8) for _ in range(3))
    return a, b, c, augment.sample_triplet_params(B, generator=g, device=dev)


def run_case(name, shape, iters, warmup, dev="cuda:0"):
    B, H, W, h, w = (shape[k] for k in "BHWhw")
    a, b, c, params = case(shape, dev)
    randn = lambda n, y, x: torch.randn((n, y, x, 3), device=dev)
    fns = {"hip": lambda: augment.preprocess_triplet(a, b, c, (h, w), DATA_FORMAT, params=params),
           "torch": lambda: augment.triplet_torch(a, b, c, params, (h, w), data_format=DATA_FORMAT, noise=randn),
           "draw": lambda: augment.sample_triplet_params(B, device=dev)}
    # the two paths on the kernel's own noise agree (the timed composition draws another field)
    x, y = fns["hip"](), augment.triplet_torch(a, b, c, params, (h, w), data_format=DATA_FORMAT)
    diff = [float((p - q).abs().max()) for p, q in zip(x, y)]
    del x, y
    for _ in range(warmup):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():           # alternating: the paths see the same machine state
            ts[k].append(event_us(f))
    r = dict(shape, case=name, data_format=DATA_FORMAT, iters=iters, warmup=warmup)
    r.update(hip_us=statistics.median(ts["hip"]), hip_min_us=min(ts["hip"]), torch_us=statistics.median(ts["torch"]),
             torch_min_us=min(ts["torch"]), draw_us=statistics.median(ts["draw"]),
             algorithmic_bytes=3 * 3 * B * H * W + 9 * 4 * B * h * w, max_abs_diff_pair=diff[0], max_abs_diff_mid=diff[1])
    r["floor_us"] = r["algorithmic_bytes"] / PEAK / 1e3
    r["hip_frac_of_peak"] = r["floor_us"] / r["hip_us"]
    r["speedup"] = r["torch_us"] / r["hip_us"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def kernels_only(name, iters):
    shape = CASES[name]
    a, b, c, params = case(shape)
    for _ in range(iters):
        augment.preprocess_triplet(a, b, c, (shape["h"], shape["w"]), DATA_FORMAT, params=params)
    torch.cuda.synchronize()


def merge_stats(path_json, csv_path, name):
    with open(path_json) as fh:
        doc = json.load(fh)
    r = next(c for c in doc["cases"] if c["case"] == name)
    with open(csv_path) as fh:
        for row in csv.DictReader(fh):
            if "triplet_pixel_kernel" in row["Name"]:
                r["kernel"] = row["Name"]
                r["kernel_calls"] = int(row["Calls"])
                r["kernel_us"] = float(row["AverageNs"]) / 1e3
                r["kernel_min_us"], r["kernel_max_us"] = float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3
                r["kernel_frac_of_peak"] = r["floor_us"] / r["kernel_us"]
    with open(path_json, "w") as fh:
        json.dump(doc, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--case", default="resize", choices=sorted(CASES), help="with --kernels-only / --merge-stats")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-stats", default=None, metavar="CSV")
    a = ap.parse_args()
    if a.merge_stats is not None:
        merge_stats(a.json, a.merge_stats, a.case)
        return
    if not torch.cuda.is_available():
        raise SystemExit("tripletbench needs a HIP device: a CPU run gives no time")
    if a.kernels_only:
        kernels_only(a.case, a.iters)
        return
    doc = {"device": torch.cuda.get_device_name(0), "peak_gbps": PEAK,
           "cases": [run_case(n, s, a.iters, a.warmup) for n, s in CASES.items()]}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()

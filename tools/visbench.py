#!/usr/bin/env python3
"""The trainer's flow panels on the HIP kernels (qpwcnet_amd.vis.flow_panels on CUDA flows: qpwc_flow_to_image_fwd, two
launches for all flows) against the same pictures composed from torch operators on the same device, per flow
vis.flow_to_image_torch (atan2, the per-image max, HSV -> RGB) + F.interpolate(mode='nearest') to the label's size +
the uint8 conversion.  One case, the shape of the reference's trainer (train.py: batch 16, 256 x 512): the label, six
predictions at 4 x 8 ... 128 x 256 and the full-resolution output -> eight uint8 (16,256,512,3) panels.

    python tools/visbench.py [--iters 200] [--warmup 20] [--json profiles/visbench.json]
    python tools/visbench.py --kernels-only          # the HIP path only: the target of
        rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/visbench.py --kernels-only --iters 100
    python tools/visbench.py --merge-stats <..._kernel_stats.csv> --json profiles/visbench.json

Times: medians of HIP-event pairs around eager calls, the two paths alternating; a call's time includes its launches,
its allocations and its Python.  The kernels' own times come from the rocprofv3 run (--merge-stats adds them to the
JSON).  Algorithmic bytes from the shapes: every flow read once by each of the two launches (2 * 2 * 4 * B * h * w) and
every panel written once (3 * B * H * W); the fraction is of 8 TB/s.  The colour launch re-reads a small flow once per
output pixel, from cache: those reads are not counted.
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
from qpwcnet_amd import vis  # noqa: E402

PEAK = 8000.0   # GB/s, HBM
B, H, W = 16, 256, 512
LEVELS = [(H, W)] + [(H >> k, W >> k) for k in range(6, 0, -1)] + [(H, W)]     # label, six predictions, the output
DATA_FORMAT = "channels_last"


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def make_flows(dev="cuda:0"):
    g = torch.Generator(device=dev).manual_seed(0)
    return [torch.randn((B, h, w, 2), device=dev, generator=g) * 3.0 for h, w in LEVELS]


def panels_torch(flows):
    """The same panels from torch operators, as a port of ShowImageCallback.on_batch_end would write them."""
    out = []
    for f in flows:
        img = vis.flow_to_image_torch(f, DATA_FORMAT)
        if tuple(img.shape[1:3]) != (H, W):
            img = F.interpolate(img.permute(0, 3, 1, 2), size=(H, W), mode="nearest").permute(0, 2, 3, 1)
        out.append(vis.to_uint8(img))
    return out


def bytes_moved():
    flows = sum(2 * 4 * B * h * w for h, w in LEVELS)
    return dict(flow_bytes=flows, panel_bytes=len(LEVELS) * 3 * B * H * W,
                max_launch_bytes=flows, colour_launch_bytes=flows + len(LEVELS) * 3 * B * H * W)


def run(iters, warmup, dev="cuda:0"):
    flows = make_flows(dev)
    fns = {"hip": lambda: vis.flow_panels(flows, data_format=DATA_FORMAT),
           "torch": lambda: panels_torch(flows)}
    x, y = fns["hip"](), fns["torch"]()
    off = [float((p.int() - q.int()).abs().max()) for p, q in zip(x, y)]
    share = [float((p != q).float().mean()) for p, q in zip(x, y)]
    del x, y
    for _ in range(warmup):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():           # alternating: the paths see the same machine state
            ts[k].append(event_us(f))
    r = dict(B=B, H=H, W=W, levels=LEVELS, data_format=DATA_FORMAT, out_dtype="uint8", iters=iters, warmup=warmup)
    r.update(bytes_moved())
    r.update(hip_us=statistics.median(ts["hip"]), hip_min_us=min(ts["hip"]), torch_us=statistics.median(ts["torch"]),
             torch_min_us=min(ts["torch"]), max_level_diff_vs_torch=max(off), max_share_differing_vs_torch=max(share))
    r["algorithmic_bytes"] = r["max_launch_bytes"] + r["colour_launch_bytes"]
    r["floor_us"] = r["algorithmic_bytes"] / PEAK / 1e3
    r["hip_frac_of_peak"] = r["floor_us"] / r["hip_us"]
    r["speedup"] = r["torch_us"] / r["hip_us"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def kernels_only(iters):
    flows = make_flows()
    for _ in range(iters):
        vis.flow_panels(flows, data_format=DATA_FORMAT)
    torch.cuda.synchronize()


def merge_stats(path_json, csv_path):
    with open(path_json) as fh:
        doc = json.load(fh)
    r = doc["case"]
    total = 0.0
    for key, floor in (("flow_mag_max_kernel", "max_launch_bytes"), ("flow_to_image_kernel", "colour_launch_bytes")):
        with open(csv_path) as fh:
            for row in csv.DictReader(fh):
                if key in row["Name"]:
                    us = float(row["AverageNs"]) / 1e3
                    r[key] = dict(name=row["Name"], calls=int(row["Calls"]), us=us, min_us=float(row["MinNs"]) / 1e3,
                                  max_us=float(row["MaxNs"]) / 1e3, floor_us=r[floor] / PEAK / 1e3,
                                  frac_of_peak=r[floor] / PEAK / 1e3 / us)
                    total += us
    r["kernels_us"] = total
    r["kernels_frac_of_peak"] = r["floor_us"] / total if total else None
    with open(path_json, "w") as fh:
        json.dump(doc, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-stats", default=None, metavar="CSV")
    a = ap.parse_args()
    if a.merge_stats is not None:
        merge_stats(a.json, a.merge_stats)
        return
    if not torch.cuda.is_available():
        raise SystemExit("visbench needs a HIP device: a CPU run gives no time")
    if a.kernels_only:
        kernels_only(a.iters)
        return
    doc = {"device": torch.cuda.get_device_name(0), "peak_gbps": PEAK, "case": run(a.iters, a.warmup)}
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()

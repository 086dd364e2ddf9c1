#!/usr/bin/env python3
"""The input pipeline for sparse ground truth on the HIP kernels (qpwcnet_amd.augment.preprocess_sparse on a CUDA batch:
qpwc_augment_sparse_fwd, two launches) against the same chain composed from torch operators on the same device
(augment.sparse_torch) and against the dense pipeline (augment.preprocess, the yardstick: the sparse kernel is the dense
one with another flow rule), at the trainer's shape (tools/augbench.py):

    B = 16, source 540 x 960 uint8 frames + fp32 flow + a uint8 mask of density 0.2, base scale 0.56, output 256 x 512,
    channels_first

    python tools/sparseaugbench.py [--iters 30] [--warmup 5] [--json profiles/sparseaugbench.json]

Call times: medians of HIP-event pairs around eager calls with the parameters already drawn, the paths alternating in
one process; `nomask` is the sparse path with valid = None (the validity from the flow alone: no mask bytes are read).  Bytes by augbench.py's accounting: the sparse path reads the source mask once and writes the
output mask once on top of the dense path's traffic.  `dense_spread` is (max - min) / median of the dense call's times:
what a ratio has to leave behind before it means anything.  The eager calls are host-bound (allocations, ctypes, two
launches), so `*_graph_us` times the two launches of a pipeline alone, replayed from a captured graph, the replays
alternating, with a spread of its own.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from augbench import PEAK, SHAPE, case, event_us, hip_path  # noqa: E402
from qpwcnet_amd import augment  # noqa: E402

DENSITY = 0.2


def sparse_case(dev, seed=0):
    ims, flo, params = case(dev, seed)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    valid = (torch.rand(flo.shape[:3], device=dev, generator=g) < DENSITY).to(torch.uint8)
    return ims, flo, valid, params


def sparse_path(ims, flo, valid, params):
    return augment.preprocess_sparse(ims, flo, valid, SHAPE["data_format"], SHAPE["base_scale"], (SHAPE["h"], SHAPE["w"]),
                                     params=params)


def torch_path(ims, flo, valid, params):
    return augment.sparse_torch(ims, flo, valid, params, (SHAPE["h"], SHAPE["w"]), data_format=SHAPE["data_format"])


def run(iters, warmup):
    dev = "cuda:0"
    ims, flo, valid, params = sparse_case(dev)
    fns = {"sparse": lambda: sparse_path(ims, flo, valid, params), "torch": lambda: torch_path(ims, flo, valid, params),
           "dense": lambda: hip_path(ims, flo, params), "nomask": lambda: sparse_path(ims, flo, None, params)}
    a, b, d = fns["sparse"](), fns["torch"](), fns["dense"]()
    diff = [float((x.float() - y.float()).abs().max()) for x, y in zip(a, b)]
    same_frames, density_out = bool(torch.equal(a[0], d[0])), float(a[2].float().mean())
    del a, b, d
    for _ in range(warmup):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():           # alternating: the paths see the same machine state
            ts[k].append(event_us(f))
    # the two launches of either pipeline alone: one capture each, the replays alternating
    graphs, keep = {}, []
    for k in ("sparse", "dense", "nomask"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fns[k]()
        torch.cuda.current_stream().wait_stream(side)
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            keep.append(fns[k]())
    for _ in range(warmup):
        for g in graphs.values():
            g.replay()
    for k in graphs:
        ts[k + "_graph"] = []
    for _ in range(iters):
        for k, g in graphs.items():
            ts[k + "_graph"].append(event_us(g.replay))
    del keep, graphs
    B, H, W, h, w = (SHAPE[k] for k in "BHWhw")
    dense_traffic = B * H * W * (6 + 8) + B * h * w * 8 * 4 + 2 * B * h * w * 6 * 4
    extra = B * H * W + B * h * w
    med = {k: statistics.median(v) for k, v in ts.items()}
    r = dict(SHAPE, mask_density=DENSITY, out_mask_density=density_out, iters=iters)
    r.update(sparse_us=med["sparse"], sparse_min_us=min(ts["sparse"]), torch_us=med["torch"], torch_min_us=min(ts["torch"]),
             dense_us=med["dense"], dense_min_us=min(ts["dense"]),
             dense_spread=(max(ts["dense"]) - min(ts["dense"])) / med["dense"],
             sparse_graph_us=med["sparse_graph"], sparse_graph_min_us=min(ts["sparse_graph"]),
             dense_graph_us=med["dense_graph"], dense_graph_min_us=min(ts["dense_graph"]),
             dense_graph_spread=(max(ts["dense_graph"]) - min(ts["dense_graph"])) / med["dense_graph"],
             sparse_over_dense_graph=med["sparse_graph"] / med["dense_graph"],
             nomask_graph_us=med["nomask_graph"], nomask_over_dense_graph=med["nomask_graph"] / med["dense_graph"],
             dense_traffic_bytes=dense_traffic, sparse_traffic_bytes=dense_traffic + extra,
             bytes_ratio=(dense_traffic + extra) / dense_traffic, sparse_over_dense=med["sparse"] / med["dense"],
             speedup_over_torch=med["torch"] / med["sparse"], frames_equal_dense=same_frames,
             max_abs_diff_ims=diff[0], max_abs_diff_flo=diff[1], max_abs_diff_valid=diff[2])
    r["floor_us"] = r["sparse_traffic_bytes"] / PEAK / 1e3
    r["sparse_graph_frac_of_peak"] = r["floor_us"] / r["sparse_graph_us"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparseaugbench needs a HIP device: a CPU run gives no time")
    r = run(a.iters, a.warmup)
    if a.json:
        doc = {"device": torch.cuda.get_device_name(0), "peak_gbps": PEAK}
        doc.update(r)
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()

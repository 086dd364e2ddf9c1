#!/usr/bin/env python3
"""The inference review panels on the HIP kernels (qpwcnet_amd.vis.inference_panels / interpolation_panels on CUDA
tensors: two launches per call) against two baselines on the same device in the same run:
  torch   the same pictures composed from torch operators (vis.inference_panels_torch / interpolation_panels_torch),
          as a port of test_infer.py / pre_train_test.py would write them;
  pieces  the project's per-piece kernels: ops.warp('tfwarp') per warp, vis.flow_to_image per flow picture, and torch
          arithmetic for the offsets, overlays, differences, the grid and the export.
Cases: both sets at B = 8, 256 x 512 (set 2: a 128 x 256 flow, s = 2, grid 32 as the script; set 1: no grid), float32
and uint8 pictures, channels-last.

    python tools/reviewbench.py [--iters 100] [--warmup 10] [--count-launches] [--json profiles/reviewbench.json]

Times: medians of HIP-event pairs around eager calls, the three paths alternating; a call's time includes its launches,
its allocations and its Python.  graph_us: the two launches alone, replayed from a captured graph (median per replay).
Launches per call: 2 by construction for the HIP path; counted with torch.profiler for the baselines.  Algorithmic bytes
from the shapes: every flow read once by each of the two launches, every image read once, every picture written once;
the corner gathers of tf_warp come from cache and are not counted.  The fraction is of 8 TB/s.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import ops, vis  # noqa: E402

PEAK = 8000.0   # GB/s, HBM
B, H, W = 8, 256, 512
FMT = "channels_last"


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def finish(pics, grid, dtype):
    out = []
    for img in pics:
        if grid:
            img = img.clone()
            img[:, ::grid] = 1.0
            img[:, :, ::grid] = 1.0
        out.append(vis.export_uint8(img) if dtype == torch.uint8 else img)
    return out


def set1_inputs(dev):
    g = torch.Generator(device=dev).manual_seed(0)
    ims = torch.rand((B, H, W, 6), device=dev, generator=g) - 0.5
    flo, flo_pred = (torch.randn((B, H, W, 2), device=dev, generator=g) * 3.0 for _ in range(2))
    return ims, flo, flo_pred


def set1_pieces(ims, flo, flo_pred, grid, dtype):
    nxt0 = ims[..., 3:6].contiguous()
    prv, nxt = 0.5 + ims[..., 0:3], 0.5 + nxt0
    nxt_w, nxt_w_gt = 0.5 + ops.warp(nxt0, flo_pred, "tfwarp", FMT), 0.5 + ops.warp(nxt0, flo, "tfwarp", FMT)
    return finish([prv, nxt, nxt_w, 0.5 * prv + 0.5 * nxt, 0.5 * prv + 0.5 * nxt_w, 0.5 * prv + 0.5 * nxt_w_gt,
                   (0.5 * prv - 0.5 * nxt_w).abs(), (0.5 * prv - 0.5 * nxt_w_gt).abs(), vis.flow_to_image(flo, FMT),
                   vis.flow_to_image(flo_pred, FMT)], grid, dtype)


def set2_inputs(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    pair = torch.rand((B, H, W, 6), device=dev, generator=g) - 0.5
    img1 = torch.rand((B, H, W, 3), device=dev, generator=g)
    pred = torch.rand((B, H, W, 3), device=dev, generator=g) - 0.5
    flow = torch.randn((B, H // 2, W // 2, 2), device=dev, generator=g) * 3.0
    return pair, img1, pred, flow


def set2_pieces(pair, img1, pred, flow, grid, dtype):
    prv, nxt = 0.5 + pair[..., 0:3], 0.5 + pair[..., 3:6]
    upflow = 2.0 * flow.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return finish([prv, nxt, img1, 0.5 + pred, 0.5 * prv + 0.5 * nxt, vis.flow_to_image(flow, FMT),
                   ops.warp(img1, upflow, "tfwarp", FMT)], grid, dtype)


def bytes_moved(set_no, osz):
    px, fpx = B * H * W, B * (H // 2) * (W // 2)
    if set_no == 1:
        return dict(max_launch_bytes=2 * 8 * px, panel_launch_bytes=(6 * 4 + 2 * 8 + 30 * osz) * px)
    return dict(max_launch_bytes=8 * fpx, panel_launch_bytes=(12 * 4 + 18 * osz) * px + (8 + 8 + 3 * osz) * fpx)


def count_launches(fn):
    """Device kernels of one call, from torch.profiler; None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as exc:                                   # the count is an extra: the times stand without it
        print("launch count unavailable: {}".format(exc), flush=True)
        return None


def run_case(set_no, dtype, iters, warmup, count, dev="cuda:0"):
    grid = 0 if set_no == 1 else 32
    args = set1_inputs(dev) if set_no == 1 else set2_inputs(dev)
    if set_no == 1:
        fns = {"hip": lambda: vis.inference_panels(*args, data_format=FMT, dtype=dtype, grid=grid),
               "torch": lambda: vis.inference_panels_torch(*args, FMT, dtype, grid),
               "pieces": lambda: set1_pieces(*args, grid, dtype)}
    else:
        fns = {"hip": lambda: vis.interpolation_panels(*args, grid=grid, data_format=FMT, dtype=dtype),
               "torch": lambda: vis.interpolation_panels_torch(*args, grid, FMT, dtype),
               "pieces": lambda: set2_pieces(*args, grid, dtype)}
    x, y, z = list(fns["hip"]().values()), list(fns["torch"]().values()), fns["pieces"]()
    diff = lambda p, q: float((p.float() - q.float()).abs().max())
    off_torch, off_pieces = max(diff(p, q) for p, q in zip(x, y)), max(diff(p, q) for p, q in zip(x, z))
    del x, y, z
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
    graph_ts = [event_us(graph.replay) for _ in range(iters)]
    del keep, graph
    osz = 1 if dtype == torch.uint8 else 4
    r = dict(set=set_no, B=B, H=H, W=W, flow=[H, W] if set_no == 1 else [H // 2, W // 2], grid=grid, data_format=FMT,
             out_dtype="uint8" if dtype == torch.uint8 else "float32", iters=iters, warmup=warmup,
             kernel=ops.review_panels_kernel(3 - set_no, B, H, W, *(() if set_no == 1 else (H // 2, W // 2)),
                                             out_dtype=dtype))
    r.update(bytes_moved(set_no, osz))
    for k in fns:
        r[k + "_us"], r[k + "_min_us"] = statistics.median(ts[k]), min(ts[k])
    r["graph_us"], r["graph_min_us"] = statistics.median(graph_ts), min(graph_ts)
    r["algorithmic_bytes"] = r["max_launch_bytes"] + r["panel_launch_bytes"]
    r["floor_us"] = r["algorithmic_bytes"] / PEAK / 1e3
    r["hip_frac_of_peak"] = r["floor_us"] / r["hip_us"]
    r["graph_frac_of_peak"] = r["floor_us"] / r["graph_us"]
    r["achieved_gbps"] = r["algorithmic_bytes"] / r["graph_us"] / 1e3
    r["speedup_vs_torch"], r["speedup_vs_pieces"] = r["torch_us"] / r["hip_us"], r["pieces_us"] / r["hip_us"]
    r["beats_both"] = r["hip_us"] < min(r["torch_us"], r["pieces_us"])
    r["max_diff_vs_torch"], r["max_diff_vs_pieces"] = off_torch, off_pieces
    r["launches"] = {"hip": 2}
    if count:
        r["launches"].update(torch=count_launches(fns["torch"]), pieces=count_launches(fns["pieces"]),
                             hip_counted=count_launches(fns["hip"]))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--count-launches", action="store_true", help="count the baselines' launches with torch.profiler")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reviewbench needs a HIP device: a CPU run gives no time")
    doc = {"device": torch.cuda.get_device_name(0), "peak_gbps": PEAK, "cases": []}
    for set_no in (1, 2):
        for dtype in (torch.float32, torch.uint8):
            doc["cases"].append(run_case(set_no, dtype, a.iters, a.warmup, a.count_launches))
            if a.json:
                with open(a.json, "w") as fh:
                    json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()

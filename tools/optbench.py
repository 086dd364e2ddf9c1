#!/usr/bin/env python3
"""The trainer's update step on the HIP kernel (optim.KerasAdamAGC.step on CUDA parameters: qpwc_agc_adam_step, one
launch for the whole model) against the composition a user would otherwise write on the same device,

    clipped = optim.adaptive_clip_grad(named_parameters, grads)          # ~10 torch operators per tensor
    torch.optim.Adam(params, 1e-4, eps=1e-7, foreach=True).step()        # on the clipped gradients

for the parameter sets of layers.FlowerModel() (123 tensors) and layers.InterpolatorModel() (148), and one whole eager
training step of FlowerModel from the decoded batch to the update (augment.preprocess, the model, multiscale
FlowMseLossV2, backward, update) with each of the two.

    python tools/optbench.py [--iters 50] [--warmup 10] [--step-iters 10] [--batch 8] [--json profiles/optbench.json]
    python tools/optbench.py --kernels-only       # the HIP update only: the target of
        rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/optbench.py --kernels-only
    python tools/optbench.py --merge-stats <..._kernel_stats.csv> --json profiles/optbench.json

Times: medians of HIP-event pairs around eager calls after a warm-up, the two paths alternating with the order reversed
every other iteration.  `hip_launches` is 1 by construction (plus one copy of the pointer table when a .grad moved);
`composed_ops` counts the aten operators the composition dispatches in one step (each at least one launch, a foreach
operator several) -- a count from the dispatcher, not from a trace.  Bytes from the shapes: p and g read twice (the
second time from cache), m and v read once, p, m and v written: `algorithmic_bytes` counts each array once per
direction (4 reads + 3 writes of 4 bytes per element).
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpwcnet_amd import augment, layers, loss, optim, synth  # noqa: E402

DEV = "cuda:0"
PEAK = 8000.0   # GB/s, HBM
RAW = (540, 960)
OUT = (256, 512)


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def alternate(runs, iters, warmup):
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    times = {k: [] for k in runs}
    order = list(runs)
    for i in range(iters):
        for k in (order if i % 2 == 0 else order[::-1]):
            times[k].append(event_us(runs[k]))
    return {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}


def composed_update(named, adam):
    """The user's composition: AGC from torch operators, then torch's foreach Adam on the clipped gradients."""
    grads = [p.grad for _, p in named]
    clipped = optim.adaptive_clip_grad(named, grads)
    for (_, p), c in zip(named, clipped):
        p.grad = c
    adam.step()
    for (_, p), g in zip(named, grads):
        p.grad = g


def make_model(kind):
    if kind == "FlowerModel":
        net = layers.FlowerModel(data_format="channels_last")
        w = synth.make_weights(42, OUT)
    else:
        net = layers.InterpolatorModel(data_format="channels_last")
        w = synth.make_interpolator_weights(42, OUT)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in w.items()})
    return net.to(DEV).train()


def bench_update(kind, a):
    net = make_model(kind)
    named = list(net.named_parameters())
    gen = torch.Generator(device=DEV).manual_seed(1)
    for _, p in named:
        p.grad = torch.randn(p.shape, device=DEV, generator=gen) * 1e-3
    hip = optim.KerasAdamAGC(net)
    adam = torch.optim.Adam([p for _, p in named], 1e-4, eps=1e-7, foreach=True)
    runs = {"hip": hip.step, "composed": lambda: composed_update(named, adam)}
    for fn in runs.values():
        fn()
    with CountOps() as c:
        composed_update(named, adam)
    med, low = alternate(runs, a.iters, a.warmup)
    n = sum(p.numel() for _, p in named)
    units = sum(len(optim.agc_units(k, p.shape)) for k, p in named)
    r = dict(op="update", model=kind, tensors=len(named), units=units, elements=n, hip_us=med["hip"],
             hip_min_us=low["hip"], composed_us=med["composed"], composed_min_us=low["composed"],
             speedup=med["composed"] / med["hip"], hip_launches=1, composed_ops=c.n, algorithmic_bytes=7 * 4 * n,
             iters=a.iters)
    r["floor_us"] = r["algorithmic_bytes"] / PEAK / 1e3
    return r


def bench_step(a):
    """augment.preprocess -> FlowerModel -> multiscale FlowMseLossV2 -> backward -> update, eager, with each update."""
    net = make_model("FlowerModel")
    named = list(net.named_parameters())
    B = a.batch
    gen = torch.Generator(device=DEV).manual_seed(2)
    raw_ims = torch.randint(0, 256, (B,) + RAW + (6,), device=DEV, generator=gen, dtype=torch.uint8)
    raw_flo = torch.randn((B,) + RAW + (2,), device=DEV, generator=gen) * 8.0
    hip = optim.KerasAdamAGC(net)
    adam = torch.optim.Adam([p for _, p in named], 1e-4, eps=1e-7, foreach=True)
    crit = loss.FlowMseLossV2()

    def step(update):
        ims, flo = augment.preprocess(raw_ims, raw_flo, "channels_last", base_scale=0.56, out_shape=OUT)
        net.zero_grad(set_to_none=True)
        total = loss.multiscale(crit, flo, net(ims)[:-1])[0]
        total.backward()
        update()
        return total

    runs = {"hip": lambda: step(hip.step), "composed": lambda: step(lambda: composed_update(named, adam)),
            "no_update": lambda: step(lambda: None)}
    med, low = alternate(runs, a.step_iters, max(2, a.warmup // 3))
    finite = bool(torch.isfinite(step(hip.step)))
    return dict(op="training_step", model="FlowerModel", B=B, raw=list(RAW), out=list(OUT), hip_step_us=med["hip"],
                composed_step_us=med["composed"], no_update_step_us=med["no_update"], hip_step_min_us=low["hip"],
                composed_step_min_us=low["composed"], speedup=med["composed"] / med["hip"], loss_finite=finite,
                iters=a.step_iters)


def kernels_only(iters):
    net = make_model("FlowerModel")
    for p in net.parameters():
        p.grad = torch.randn_like(p) * 1e-3
    opt = optim.KerasAdamAGC(net)
    for _ in range(iters):
        opt.step()
    torch.cuda.synchronize()


def merge_stats(path_json, csv_path):
    """Adds the kernel's own time (FlowerModel's parameter set, the --kernels-only run) from rocprofv3's stats."""
    with open(path_json) as fh:
        doc = json.load(fh)
    with open(csv_path) as fh:
        for row in csv.DictReader(fh):
            if "agc_adam_kernel" in row["Name"]:
                doc["kernel_stats"] = {"model": "FlowerModel", "calls": int(row["Calls"]),
                                       "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                       "max_us": float(row["MaxNs"]) / 1e3}
                floor = next(r["floor_us"] for r in doc["rows"] if r.get("model") == "FlowerModel" and r["op"] == "update")
                doc["kernel_stats"]["frac_of_peak"] = floor / doc["kernel_stats"]["avg_us"]
    with open(path_json, "w") as fh:
        json.dump(doc, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-step", action="store_true", help="skip the whole training step")
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-stats", default=None, metavar="CSV")
    a = ap.parse_args()
    if a.merge_stats is not None:
        merge_stats(a.json, a.merge_stats)
        return
    if not torch.cuda.is_available():
        raise SystemExit("optbench needs a HIP device: a CPU run gives no time")
    if a.kernels_only:
        kernels_only(a.iters)
        return
    doc = {"device": torch.cuda.get_device_name(0), "peak_gbps": PEAK, "rows": []}

    def add(row):
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
        doc["rows"].append(row)
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(doc, fh, indent=1)

    for kind in ("FlowerModel", "InterpolatorModel"):
        add(bench_update(kind, a))
    if not a.no_step:
        add(bench_step(a))


if __name__ == "__main__":
    main()

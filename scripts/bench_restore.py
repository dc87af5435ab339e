#!/usr/bin/env python3
"""What one iteration of a latent fit costs.  At config B (64x64x3, L 3, K 32, hidden 512), batch 1 and batch 64, IN ONE PROCESS,
alternating between

  (a) `Inferer.fit_latents`: the autograd route -- torch.optim.Adam over Python tensors, the objective as torch element-wise
      launches, one decode + one VJP through `_GlowDecodeFn` per iteration.  The yardstick.
  (b) `LatentFit.step_eager`: decode into a static image, glowhip_restore_objective, decode_vjp into persistent gradients, the fused
      Adam step, the histories on the device -- enqueued launch by launch from Python.
  (c) `LatentFit.step_captured`: the same iteration as ONE hipGraph launch.

The problem is in-painting of the left half (mask = weight), started from the latents of the blanked image.  Per round and route:
`--steps` iterations between two HIP events (device_ms: what the stream was busy or waiting for the host, per iteration), then the
host's wall time to enqueue three iterations onto an idle device (host_ms per iteration: three, because the host of (c) may run no
more than `HyperRing`'s four slots ahead of the device and would otherwise be timed waiting for it; (a) ends with its own history
read, so its host time is its wall time).  Warm-up first,
`--rounds` alternations; min / median / max of the per-round means.  `graph_default_ok`: (c) is not slower than (a) by more than
(a)'s own round-to-round spread -- the rule `Inferer.restore(graph=...)`'s default follows.  Prints ONE JSON line and writes it to
--out (default profiles/restore_bench.json); fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_glow_amd.network import Inferer, LatentFit  # noqa: E402

from bench_decode_grad import CONFIGS, DEV, make  # noqa: E402


HOST_STEPS = 3


def timed(fn, steps):
    """(device ms, host ms) per iteration of ``fn(k)``, which enqueues ``k`` iterations."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn(steps)
    e1.record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(HOST_STEPS)
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, host * 1e3 / HOST_STEPS


def summary(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4), "rounds": len(v)}


def run(glow, inf, x, args):
    n = x.shape[0]
    mask = torch.zeros_like(x)
    mask[..., : x.shape[-1] // 2] = 1.0
    with torch.no_grad():
        init = inf.encode_full(x * (1.0 - mask))
    fit = LatentFit(glow, x, weight=mask, init=init, steps=max(args.steps, 2), lr=args.lr)

    def a(steps):
        inf.fit_latents(x, mask=mask, steps=steps, lr=args.lr, init=init)

    def b(steps):
        for _ in range(steps):
            fit.step_eager()

    def c(steps):
        for _ in range(steps):
            fit.step_captured()

    fit.reset()
    a(args.warmup)
    b(args.warmup)
    captured = fit.capture()
    routes = {"a": a, "b": b}
    if captured:
        routes["c"] = c
        c(args.warmup)
    dev_ms, host_ms = {k: [] for k in routes}, {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            d, h = timed(fn, args.steps)
            dev_ms[k].append(d)
            host_ms[k].append(h)
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(fit.loss_hist).all()) and bool(torch.isfinite(fit.norm_hist).all())
    names = {"a": "fit_latents_autograd", "b": "latent_fit_eager", "c": "latent_fit_captured"}
    out = {"batch": n, "timed_iterations_per_route": args.rounds * args.steps, "captured": captured, "graph_error": fit.graph_error,
           "histories_finite": finite}
    for k in routes:
        out[names[k]] = {"device_ms": summary(dev_ms[k]), "host_ms": summary(host_ms[k])}
    if captured:
        med = statistics.median
        spread = max(dev_ms["a"]) - min(dev_ms["a"])
        out["a_round_to_round_spread_ms"] = round(spread, 4)
        out["c_minus_a_ms"] = round(med(dev_ms["c"]) - med(dev_ms["a"]), 4)
        out["graph_default_ok"] = bool(med(dev_ms["c"]) - med(dev_ms["a"]) <= spread)
        out["a_over_c"] = round(med(dev_ms["a"]) / med(dev_ms["c"]), 3)
        out["b_over_c"] = round(med(dev_ms["b"]) / med(dev_ms["c"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed iterations per route and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_restore.py: no GPU visible", file=sys.stderr)
        return 2
    cfg = CONFIGS[args.config]
    batches = [int(v) for v in args.batches.split(",")]
    cfg = dict(cfg, batch=max(batches))
    im = cfg["image"]
    g = torch.Generator().manual_seed(1)
    x = torch.rand(cfg["batch"], 3, im, im, generator=g).to(DEV)
    noise = (torch.rand(cfg["batch"], 3, im, im, generator=g) / 256).to(DEV)
    glow = make(cfg)
    with torch.no_grad():
        glow.train()
        glow.normal_flow(x, None, noise=noise)      # data-dependent ActNorm init from the largest batch
        glow.eval()
    inf = Inferer(glow.hps, glow, [DEV], DEV)
    out = {"bench": "restore", "device": torch.cuda.get_device_name(0),
           "config": f"{args.config} ({im}x{im}x3 L{cfg['L']} K{cfg['K']} hidden {cfg['hidden']})",
           "results": [run(glow, inf, x[:n].contiguous(), args) for n in batches]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

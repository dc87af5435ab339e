#!/usr/bin/env python3
"""What one iteration of the posterior chain costs, next to one iteration of the MAP fit.  At config B (64x64x3, L 3, K 32, hidden
512), batch 1 and batch 64, IN ONE PROCESS, alternating between

  (r) `LatentFit.step_captured`: the restoration iteration (decode, objective, decode_vjp, fused Adam) as one hipGraph launch --
      scripts/bench_restore.py's route (c), the yardstick;
  (e) `LatentMALA.step_eager`: propose, decode, objective, decode_vjp, energy, select, moments -- enqueued launch by launch;
  (c) `LatentMALA.step_captured`: the same iteration as ONE hipGraph launch.

The problem is in-painting of the left half (mask = weight), started from the latents of the blanked image, noise_std 0.1.  Per
round and route: `--steps` iterations between two HIP events (device_ms per iteration), then the host's wall time to enqueue three
iterations onto an idle device (host_ms per iteration).  Warm-up first, `--rounds` alternations; min / median / max of the
per-round means.  Prints ONE JSON line and writes it to --out (default profiles/posterior_bench.json); fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_glow_amd.network import Inferer, LatentFit, LatentMALA  # noqa: E402

from bench_decode_grad import CONFIGS, DEV, make  # noqa: E402
from bench_restore import summary, timed  # noqa: E402


def run(glow, inf, x, args):
    n = x.shape[0]
    mask = torch.zeros_like(x)
    mask[..., : x.shape[-1] // 2] = 1.0
    with torch.no_grad():
        init = inf.encode_full(x * (1.0 - mask))
    total = args.warmup + args.rounds * (args.steps + 3) + 8      # (the histories hold every iteration enqueued)
    fit = LatentFit(glow, x, weight=mask, init=init, steps=total, lr=args.lr)
    mala = LatentMALA(glow, x, weight=mask, noise_std=args.noise_std, init=init, steps=2 * total, burn_in=total, step_size=args.step_size,
                      seed=1)

    def r(steps):
        for _ in range(steps):
            fit.step_captured()

    def e(steps):
        for _ in range(steps):
            mala.step_eager()

    def c(steps):
        for _ in range(steps):
            mala.step_captured()

    fit.reset()
    fit.step_eager()
    routes = {}
    if fit.capture():
        routes["r"] = r
    routes["e"] = e
    e(args.warmup)
    captured = mala.capture()
    if captured:
        routes["c"] = c
    for fn in routes.values():
        fn(args.warmup)
    dev_ms, host_ms = {k: [] for k in routes}, {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            d, h = timed(fn, args.steps)
            dev_ms[k].append(d)
            host_ms[k].append(h)
    torch.cuda.synchronize()
    names = {"r": "restore_captured", "e": "mala_eager", "c": "mala_captured"}
    done = int(mala.iteration.item())
    hist = mala.hist[:, :done].cpu()
    out = {"batch": n, "timed_iterations_per_route": args.rounds * args.steps, "captured": captured, "graph_error": mala.graph_error,
           "restore_graph_error": fit.graph_error, "mala_iterations": done, "accept_rate": round(float(hist[1].mean()), 3),
           "nonfinite_rejections": int(mala.counts[1].sum().item()), "energies_finite": bool(torch.isfinite(hist[0]).all()),
           "step_size_min_max": [float(mala.step.min()), float(mala.step.max())]}
    for k in routes:
        out[names[k]] = {"device_ms": summary(dev_ms[k]), "host_ms": summary(host_ms[k])}
    med = statistics.median
    if "r" in routes and captured:
        out["mala_captured_over_restore_captured"] = round(med(dev_ms["c"]) / med(dev_ms["r"]), 3)
    if captured:
        out["mala_eager_over_captured"] = round(med(dev_ms["e"]) / med(dev_ms["c"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed iterations per route and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--noise-std", type=float, default=0.1)
    ap.add_argument("--step-size", type=float, default=1e-4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_posterior.py: no GPU visible", file=sys.stderr)
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
    out = {"bench": "posterior", "device": torch.cuda.get_device_name(0),
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

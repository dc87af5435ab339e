#!/usr/bin/env python3
"""What a point-spread function costs the restoration path.  At config B (64x64x3, L 3, K 32, hidden 512), batch 1 and batch 64, IN
ONE PROCESS, alternating between the variants

  none   the existing objective, glowhip_restore_objective -- the yardstick, untouched by the PSF entry point
  1x1, 5x5, 15x15   glowhip_restore_objective_psf with a PSF of that size (a normalised Gaussian; 1x1: the single tap 1.0)

two things are timed per variant:

  objective_us   the objective launch alone: `--reps` back-to-back launches on an idle stream between two HIP events, per launch
                 (the launches queue behind each other, so the host's enqueue time is hidden once the first is running)
  iteration_ms   `LatentFit.step_captured`: the whole iteration -- decode, objective, decode VJP, fused Adam step, histories -- as
                 one hipGraph launch; `--steps` iterations between two HIP events, per iteration

The problem is deblurring with unit weights on the valid band (in-painting of the same band for `none`), started from the latents
of the measurement.  Warm-up first, then `--rounds` alternations; min / median / max of the per-round means.
`objective_share_of_iteration`: the variant's median objective launch over the median iteration WITHOUT a PSF -- the figure
DESIGN.md holds against 5 %.  Prints ONE JSON line and writes it to --out (default profiles/deblur_bench.json); fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_glow_amd.network import Inferer, LatentFit, restore_objective  # noqa: E402
from pytorch_glow_amd.network.restore import psf_valid_weight  # noqa: E402

from bench_decode_grad import CONFIGS, DEV, make  # noqa: E402

SIDES = (1, 5, 15)


def gaussian(side):
    r = torch.arange(side, dtype=torch.float64) - (side - 1) / 2
    g = torch.exp(-r ** 2 / (2 * max(side / 5.0, 1e-3) ** 2))
    k = g[:, None] * g[None, :]
    return (k / k.sum()).float().to(DEV)


def between_events(fn, count):
    """Device ms per call of ``fn`` over ``count`` calls enqueued back to back."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count


def summary(v, scale=1.0, digits=4):
    return {"min": round(min(v) * scale, digits), "median": round(statistics.median(v) * scale, digits),
            "max": round(max(v) * scale, digits), "rounds": len(v)}


def run(glow, inf, x, args):
    n = x.shape[0]
    variants = {"none": None, **{f"{s}x{s}": gaussian(s) for s in SIDES}}
    weight = psf_valid_weight(x.shape, max(SIDES), max(SIDES), 1).to(DEV).expand_as(x).contiguous()
    inv = 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0)
    with torch.no_grad():
        init = inf.encode_full(x)
    image = torch.rand_like(x)
    grad, loss, resid = torch.empty_like(x), torch.empty(n, device=DEV), torch.empty_like(x)
    objective, iteration, fits = {}, {}, {}
    for name, psf in variants.items():
        kw = {} if psf is None else dict(psf=psf, resid_out=resid)
        objective[name] = lambda kw=kw: restore_objective(image, x, weight, inv, 1, grad_out=grad, loss_out=loss, **kw)
        fit = fits[name] = LatentFit(glow, x, weight=weight, init=init, steps=max(args.steps, 2), lr=args.lr, psf=psf)
        fit.reset()
        for _ in range(args.warmup):
            fit.step_eager()
        if not fit.capture():
            raise RuntimeError(f"{name}: capture failed: {fit.graph_error}")
        iteration[name] = fit.step_captured
        for _ in range(args.warmup):
            fit.step_captured()
            objective[name]()
    obj_ms, it_ms = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(args.rounds):
        for name in variants:
            obj_ms[name].append(between_events(objective[name], args.reps))
            it_ms[name].append(between_events(iteration[name], args.steps))
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(f.loss_hist).all()) and bool(torch.isfinite(f.norm_hist).all()) for f in fits.values())
    base_it = statistics.median(it_ms["none"])
    out = {"batch": n, "timed_launches_per_variant": args.rounds * args.reps, "timed_iterations_per_variant": args.rounds * args.steps,
           "histories_finite": finite, "variants": {}}
    for name in variants:
        obj, it = statistics.median(obj_ms[name]), statistics.median(it_ms[name])
        out["variants"][name] = {"objective_us": summary(obj_ms[name], 1e3, 2), "iteration_ms": summary(it_ms[name]),
                                 "iteration_minus_none_ms": round(it - base_it, 4),
                                 "objective_share_of_iteration": round(obj / base_it, 5)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed captured iterations per variant and round")
    ap.add_argument("--reps", type=int, default=200, help="timed objective launches per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deblur_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_deblur.py: no GPU visible", file=sys.stderr)
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
    out = {"bench": "deblur", "device": torch.cuda.get_device_name(0),
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

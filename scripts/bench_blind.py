#!/usr/bin/env python3
"""What estimating the point-spread function costs the restoration path.  At config B (64x64x3, L 3, K 32, hidden 512), batch 1 and
batch 64, with 5x5 and 15x15 PSFs, one for the batch (`shared`) and one per sample (`per_sample`), IN ONE PROCESS, alternating
between the variants, two things are timed:

  launches       on the same inputs, each as `--reps` back-to-back calls on an idle stream between two HIP events, per call (the
                 launches queue behind each other, so the host's enqueue time is hidden once the first is running):
                   objective_us   glowhip_restore_objective_psf -- the yardstick the new launches stand next to
                   psf_grad_us    glowhip_restore_psf_grad: the partial and the finishing launch, grad_logits only, as the loop calls it
                   softmax_us     glowhip_psf_from_logits
  iteration_ms   `LatentFit.step_captured`, the whole iteration as one hipGraph launch, `--steps` iterations between two HIP events,
                 per iteration: `blind` (estimate_psf: the softmax, the gradient call and theta's Adam step on top) against
                 `known` -- the same fit with the PSF given, which is the code path as it was before blind deblurring existed
                 (`LatentFit.blind is None`: no softmax, no gradient call, one optimiser), in the same run on the same box

The problem is deblurring with unit weights on the valid band of the 15x15 PSF, started from the latents of the measurement and,
for `blind`, from the Gaussian PSF itself (the cost does not depend on the taps' values).  Warm-up first, then `--rounds`
alternations; min / median / max of the per-round means.  `blind_over_known`: the ratio of the median iterations -- the figure
DESIGN.md holds against 1.05.  Prints ONE JSON line and writes it to --out (default profiles/blind_bench.json); fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_glow_amd.network import Inferer, LatentFit, psf_from_logits, psf_gradient, restore_objective  # noqa: E402
from pytorch_glow_amd.network.restore import psf_grad_scratch, psf_valid_weight  # noqa: E402

from bench_decode_grad import CONFIGS, DEV, make  # noqa: E402
from bench_deblur import between_events, gaussian, summary  # noqa: E402

SIDES = (5, 15)
MODES = ("shared", "per_sample")


def run(glow, inf, x, args):
    n = x.shape[0]
    weight = psf_valid_weight(x.shape, max(SIDES), max(SIDES), 1).to(DEV).expand_as(x).contiguous()
    inv = 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0)
    with torch.no_grad():
        init = inf.encode_full(x)
    image = torch.rand_like(x)
    grad, loss, resid = torch.empty_like(x), torch.empty(n, device=DEV), torch.empty_like(x)
    names, launches, iteration, fits = [], {}, {}, []
    for side in SIDES:
        for mode in MODES:
            name = f"{side}x{side} {mode}"
            names.append(name)
            psf = gaussian(side) if mode == "shared" else gaussian(side).expand(n, side, side).contiguous()
            logits, gl, soft = torch.log(psf), torch.empty_like(psf), torch.empty_like(psf)
            scratch = psf_grad_scratch(x.shape, side, side, 1, DEV)
            launches[name] = {
                "objective_us": lambda psf=psf: restore_objective(image, x, weight, inv, 1, grad_out=grad, loss_out=loss, psf=psf, resid_out=resid),
                "psf_grad_us": lambda psf=psf, gl=gl, scratch=scratch: psf_gradient(image, resid, inv, psf, 1, grad_logits=gl, scratch=scratch),
                "softmax_us": lambda logits=logits, soft=soft: psf_from_logits(logits, out=soft)}
            iteration[name] = {}
            for kind, kw in (("known", dict(psf=psf)), ("blind", dict(psf=psf.cpu(), estimate_psf=mode, psf_lr=args.psf_lr))):
                fit = LatentFit(glow, x, weight=weight, init=init, steps=max(args.steps, 2), lr=args.lr, **kw)
                assert (fit.blind is None) == (kind == "known")
                fit.reset()
                for _ in range(args.warmup):
                    fit.step_eager()
                if not fit.capture():
                    raise RuntimeError(f"{name} {kind}: capture failed: {fit.graph_error}")
                for _ in range(args.warmup):
                    fit.step_captured()
                iteration[name][kind] = fit.step_captured
                fits.append(fit)
            launches[name]["objective_us"]()      # (resid holds a residual before the gradient call is timed)
            for fn in launches[name].values():
                for _ in range(args.warmup):
                    fn()
    l_ms = {name: {k: [] for k in launches[name]} for name in names}
    it_ms = {name: {"known": [], "blind": []} for name in names}
    for _ in range(args.rounds):
        for name in names:
            for k, fn in launches[name].items():
                l_ms[name][k].append(between_events(fn, args.reps))
            for kind in ("known", "blind"):
                it_ms[name][kind].append(between_events(iteration[name][kind], args.steps))
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(f.loss_hist).all()) and bool(torch.isfinite(f.norm_hist).all())
                 and (f.blind is None or bool(torch.isfinite(f.blind.norm_hist).all())) for f in fits)
    out = {"batch": n, "timed_launches_per_variant": args.rounds * args.reps, "timed_iterations_per_variant": args.rounds * args.steps,
           "histories_finite": finite, "variants": {}}
    for name in names:
        known, blind = statistics.median(it_ms[name]["known"]), statistics.median(it_ms[name]["blind"])
        out["variants"][name] = {**{k: summary(v, 1e3, 2) for k, v in l_ms[name].items()},
                                 "iteration_ms": {kind: summary(it_ms[name][kind]) for kind in ("known", "blind")},
                                 "blind_minus_known_ms": round(blind - known, 4), "blind_over_known": round(blind / known, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed captured iterations per variant and round")
    ap.add_argument("--reps", type=int, default=200, help="timed launches per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--psf-lr", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blind_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_blind.py: no GPU visible", file=sys.stderr)
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
    out = {"bench": "blind", "device": torch.cuda.get_device_name(0),
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

#!/usr/bin/env python3
"""What held-out evaluation costs (csrc/evaluate.hip, network.Evaluator), at config B (celeba profile: 64x64x3, L 3, K 32, hidden
512) and batch 64, over a data set of --batches device-resident batches, alternating IN ONE PROCESS between

  (a) the loop the existing API allows: for x in batches: z, nll, _ = glow(x); total += nll.sum().item()      (the baseline)
  (b) Evaluator(glow, draws=1, levels=False)
  (c) Evaluator(glow, draws=1, levels=True)       + n_levels snapshot launches and one terms launch per forward
  (d) Evaluator(glow, draws=4, levels=True)       four forwards per batch, one fold

Per route and round: wall time of one pass over the data set (host clock, device synchronised at both ends) -> images / s, and the
HOST milliseconds per batch (until the host reaches its first wait: (a) waits in every batch, the evaluator once at the end).
min / median / max over --rounds; the spread (max - min) of (a) is the noise figure of this box and hour, and the acceptance of (b)
is relative to it.  Also, by HIP events: the fold launch alone and the inference forward with and without the level terms bound.
Prints ONE JSON line and writes it to --out (default profiles/evaluate_bench.json); fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from pytorch_glow_amd.network import evaluate as EV  # noqa: E402

DEV = "cuda:0"


def make(batch, seed=0):
    hps = util.load_profile("celeba")
    hps.optim.num_batch_train = batch
    hps.device.graph = [DEV]
    torch.manual_seed(seed)
    np.random.seed(seed)
    glow = G.Glow(hps)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():      # zero-init tails would make the coupling and the priors trivial (as bench.py)
        for name, p in glow.named_parameters():
            if ".f.4." in name or "conv2d_zeros" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.002)
    return glow.to(DEV)


def summary(v, digits=4):
    return {"min": round(min(v), digits), "median": round(statistics.median(v), digits), "max": round(max(v), digits),
            "spread": round(max(v) - min(v), digits), "rounds": len(v)}


def event_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_evaluate.py: no GPU visible", file=sys.stderr)
        return 2
    g = torch.Generator().manual_seed(1)
    batches = [torch.rand(args.batch, 3, 64, 64, generator=g).to(DEV) for _ in range(args.batches)]
    images = args.batch * args.batches
    glow = make(args.batch)
    reached = {}
    read = EV.EvalState.read

    def read_timed(self):      # the moment the host reaches the evaluator's one wait
        reached.setdefault("t", time.perf_counter())
        return read(self)
    EV.EvalState.read = read_timed

    def route_a():
        total = 0.0
        for x in batches:
            z, nll, _ = glow(x)
            total += nll.sum().item()
        reached["t"] = time.perf_counter()      # (the host waited in every batch: its time is the wall time)
        return total / images

    def evaluator(draws, levels):
        ev = EV.Evaluator(glow, draws=draws, levels=levels, seed=0, safe=False)
        return lambda: ev.run(batches)

    routes = {"a_glow_item_loop": route_a, "b_evaluator": evaluator(1, False), "c_levels": evaluator(1, True),
              "d_draws4_levels": evaluator(4, True)}
    with torch.no_grad():
        glow.train()
        glow.normal_flow(batches[0], None, noise=torch.rand_like(batches[0]) / 256)      # data-dependent ActNorm init
        glow.eval()
        results = {}
        for fn in routes.values():      # warm-up: plans, packs, workspaces
            fn(); fn()
        torch.cuda.synchronize()
        wall = {k: [] for k in routes}
        host = {k: [] for k in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                reached.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results[name] = fn()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                wall[name].append((t1 - t0) * 1e3)
                host[name].append((reached["t"] - t0) * 1e3 / args.batches)
        # launch times by HIP events
        plan = glow.flow.plan_for(batches[0])
        x = batches[0]
        n_bits = glow.hps.model.n_bits_x
        out = (torch.empty((args.batch,) + plan.out_chw, device=DEV), torch.empty(args.batch, device=DEV), torch.empty(args.batch, device=DEV))
        terms = plan.level_terms_buffer(args.batch)
        plan.set_dequant_stream(0, 0)
        fwd_plain = lambda: plan.glow_forward(x, None, None, None, 0, n_bits, out=out)
        fwd_terms = lambda: plan.glow_forward(x, None, None, None, 0, n_bits, out=out, level_terms=terms)
        for _ in range(5):
            fwd_plain(); fwd_terms()
        f_plain, f_terms = [], []
        for _ in range(args.rounds):
            f_plain.append(event_ms(fwd_plain, 20)); f_terms.append(event_ms(fwd_terms, 20))
        plan.set_dequant_rng(0, False)
        state = EV.EvalState(DEV, plan.n_levels, EV.Evaluator.DEFAULT_HIST)
        per = torch.empty(args.batch, device=DEV)
        fold_ms = {}
        for K in (1, 4):
            obj = torch.full((K, args.batch), -25000.0, device=DEV) + torch.rand(K, args.batch, device=DEV)
            tk = torch.rand(K, plan.n_levels, args.batch, device=DEV) * -8000.0
            fold = lambda: state.fold(obj, tk, 3 * 64 * 64, per, 0)
            fold()
            fold_ms[f"K{K}"] = summary([event_ms(fold, 50) for _ in range(args.rounds)], 5)
    EV.EvalState.read = read
    med = statistics.median
    per_image_us = {k: [w * 1e3 / images for w in v] for k, v in wall.items()}
    a, b, c, d = (per_image_us[k] for k in routes)
    res_b, res_c, res_d = results["b_evaluator"], results["c_levels"], results["d_draws4_levels"]
    out = {
        "bench": "evaluate", "device": torch.cuda.get_device_name(0), "config": "B (64x64x3 L3 K32 hidden 512)", "batch": args.batch,
        "batches": args.batches, "images": images,
        "images_per_s": {k: summary([images / (w * 1e-3) for w in v], 1) for k, v in wall.items()},
        "wall_us_per_image": {k: summary(v, 3) for k, v in per_image_us.items()},
        "host_ms_per_batch": {k: summary(v) for k, v in host.items()},
        "a_spread_us_per_image": round(max(a) - min(a), 3),
        "b_minus_a_us_per_image": round(med(b) - med(a), 3),
        "b_within_a_spread": bool(med(b) - med(a) <= max(a) - min(a)),
        "c_minus_b_us_per_image": round(med(c) - med(b), 3),
        "d_minus_4b_us_per_image": round(med(d) - 4 * med(b), 3),
        "forward_ms_by_events": {"plain": summary(f_plain), "level_terms_bound": summary(f_terms),
                                 "snapshots_and_terms_ms": round(med(f_terms) - med(f_plain), 4), "n_levels": plan.n_levels},
        "fold_launch_ms_by_events": fold_ms,
        "figures": {"a_mean_nll": results["a_glow_item_loop"], "b_bits_per_dim": res_b.bits_per_dim,
                    "c_level_bits": res_c.level_bits, "d_bits_per_dim": res_d.bits_per_dim,
                    "d_bits_per_dim_single": res_d.bits_per_dim_single, "flagged": [res_b.flagged, res_c.flagged, res_d.flagged]},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

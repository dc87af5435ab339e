#!/usr/bin/env python3
"""What a dense linear operator (compressed sensing) costs the restoration path.  At config B (64x64x3: D = 12 288, L 3, K 32,
hidden 512), M in {1 024, 4 096} rows, batch 1 and batch 64, IN ONE PROCESS, alternating between the variants

  torch    the objective as torch calls: two `torch.matmul` (A x and A^T u) plus the element-wise operations between them -- the
           yardstick
  linear   glowhip_restore_objective_linear alone (preallocated outputs and scratch)
  fit      `LatentFit.step_captured` with the operator, beside the same loop without one (in-painting with unit weights): the whole
           iteration -- decode, objective, decode VJP, fused Adam step, histories -- as one hipGraph launch

`objective_us`: `--reps` back-to-back calls on an idle stream between two HIP events, per call (the launches queue behind each other,
so the host's enqueue time is hidden once the first is running).  `effective_TBps`: 2 M D 4 bytes -- A read once by each product --
over that time, to be read beside the 6.0 - 6.3 TB/s streaming rate of an MI355X.  `iteration_ms`: `--steps` captured iterations
between two HIP events, per iteration.  `objective_share_of_iteration`: the linear call's median over the median iteration with the
operator.  Warm-up first, then `--rounds` alternations; min / median / max of the per-round means; `slower_than_torch` is set where
the linear call's median exceeds the torch variant's by more than the latter's round-to-round spread (max - min).
Prints ONE JSON line and writes it to --out (default profiles/linear_bench.json); fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_glow_amd.network import Inferer, LatentFit, gaussian_operator, restore_objective  # noqa: E402
from pytorch_glow_amd.network.restore import linear_scratch  # noqa: E402

from bench_decode_grad import CONFIGS, DEV, make  # noqa: E402
from bench_deblur import between_events, summary  # noqa: E402


def torch_objective(x, t, a2, inv):
    """(loss, grad_x) of the unit-weight objective as torch calls: a2 is the operator flattened to (M, D)."""
    d = torch.matmul(x.flatten(1), a2.t()) - t
    loss = (d * d).sum(dim=1) * inv
    g = torch.matmul((2.0 * inv)[:, None] * d, a2)
    return loss, g.view_as(x)


def run(glow, inf, x, ops, args):
    n = x.shape[0]
    with torch.no_grad():
        init = inf.encode_full(x)
    image = torch.rand_like(x)
    grad, loss = torch.empty_like(x), torch.empty(n, device=DEV)
    calls, fits = {}, {}
    plain = fits["none"] = LatentFit(glow, x, init=init, steps=max(args.steps, 2), lr=args.lr)
    for m, A in ops.items():
        a2 = A.flatten(1)
        t = torch.matmul(x.flatten(1), a2.t())
        inv = torch.full((n,), 1.0 / m, device=DEV)
        resid, scratch = torch.empty_like(t), linear_scratch(n, m, a2.shape[1], x.device)
        calls[f"torch M{m}"] = lambda t=t, a2=a2, inv=inv: torch_objective(image, t, a2, inv)
        calls[f"linear M{m}"] = lambda t=t, A=A, resid=resid, scratch=scratch: restore_objective(
            image, t, None, None, 1, grad_out=grad, loss_out=loss, resid_out=resid, operator=A, scratch=scratch)
        fits[f"M{m}"] = LatentFit(glow, t, init=init, steps=max(args.steps, 2), lr=args.lr, operator=A)
    for name, fit in fits.items():
        fit.reset()
        for _ in range(args.warmup):
            fit.step_eager()
        if not fit.capture():
            raise RuntimeError(f"{name}: capture failed: {fit.graph_error}")
        for _ in range(args.warmup):
            fit.step_captured()
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    call_ms, it_ms = {k: [] for k in calls}, {k: [] for k in fits}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            call_ms[name].append(between_events(fn, args.reps))
        for name, fit in fits.items():
            it_ms[name].append(between_events(fit.step_captured, args.steps))
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(f.loss_hist).all()) and bool(torch.isfinite(f.norm_hist).all()) for f in fits.values())
    out = {"batch": n, "timed_calls_per_variant": args.rounds * args.reps, "timed_iterations_per_variant": args.rounds * args.steps,
           "histories_finite": finite, "iteration_ms_without_operator": summary(it_ms["none"]), "operators": {}}
    for m, A in ops.items():
        lin, ref = call_ms[f"linear M{m}"], call_ms[f"torch M{m}"]
        lin_med, ref_med, it_med = statistics.median(lin), statistics.median(ref), statistics.median(it_ms[f"M{m}"])
        nbytes = 2.0 * A.numel() * 4
        out["operators"][f"M{m}"] = {
            "torch_objective_us": summary(ref, 1e3, 2), "linear_objective_us": summary(lin, 1e3, 2),
            "linear_effective_TBps": round(nbytes / (lin_med * 1e-3) / 1e12, 3), "torch_effective_TBps": round(nbytes / (ref_med * 1e-3) / 1e12, 3),
            "linear_over_torch": round(lin_med / ref_med, 3), "slower_than_torch": bool(lin_med - ref_med > max(ref) - min(ref)),
            "iteration_ms": summary(it_ms[f"M{m}"]), "iteration_minus_none_ms": round(it_med - statistics.median(it_ms["none"]), 4),
            "objective_share_of_iteration": round(lin_med / it_med, 5)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--rows", default="1024,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed captured iterations per variant and round")
    ap.add_argument("--reps", type=int, default=100, help="timed objective calls per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_linear.py: no GPU visible", file=sys.stderr)
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
    ops = {int(m): gaussian_operator(int(m), (3, im, im), 1, DEV) for m in args.rows.split(",")}
    out = {"bench": "linear", "device": torch.cuda.get_device_name(0),
           "config": f"{args.config} ({im}x{im}x3 L{cfg['L']} K{cfg['K']} hidden {cfg['hidden']})", "D": 3 * im * im,
           "results": [run(glow, inf, x[:n].contiguous(), ops, args) for n in batches]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

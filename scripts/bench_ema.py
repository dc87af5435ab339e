#!/usr/bin/env python3
"""What the Polyak average of the weights costs (csrc/optim.hip: the EMA instance of k_optim_update, k_optim_ema_swap), at config
B's parameter set (celeba profile: 64x64x3, L 3, K 32, hidden 512: ~1 060 tensors, 44 M parameters), alternating IN ONE PROCESS
between

  optim (a) the two optimiser launches, EMA off           glowhip_optim_step
  optim (b) the two optimiser launches, EMA on            glowhip_optim_step_ema
  optim (c) (a) followed by torch._foreach_lerp_          the average as a caller keeps it without the fused one
  train (d) captured training step, EMA off / on          TrainLoop(graph=True), batch 64
  swap  (e) parameters <-> average                        glowhip_optim_ema_swap (timed in pairs: the weights end where they began)

(a), (b), (e) call the C ABI directly on the optimiser's own chunk table (a ctypes call per step: the device time of the launches,
not the Python around them); (c) adds the foreach call as a caller would issue it, host time included.  HIP events around blocks
of steps, warm-up first, min / median / max of the per-round means; the spread of (a) and of (d, off) over the rounds is the
run's own noise figure.  On a tree without the EMA entry points (the parent commit) only (a), (c) and (d, off) run -- the same
code, so the two trees can be compared on one box.  Prints ONE JSON line; fails without a GPU.

`--merge parent=FILE ... new=FILE ... --out profiles/ema_bench.json` (no GPU) combines the lines of several such runs -- repeated
runs of the parent's tree and of this one -- into the committed record: the per-run medians side by side, the parent's
run-to-run spread, this tree's distance from the parent's median, and whether (b) stays below (c) as measured on the parent."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib, training  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402

DEV = "cuda:0"
HAS_EMA = "glowhip_optim_step_ema" in _lib.SIGNATURES
ADAM = dict(lr=1e-4, b1=0.9, b2=0.9999, eps=1e-8, clip=5.0, max_norm=100.0)


def make(batch, ema_decay=0.0, seed=0):
    hps = util.load_profile("celeba")
    hps.optim.num_batch_train = batch
    hps.device.graph = [DEV]
    if ema_decay:
        hps.optim.ema_decay = ema_decay
    torch.manual_seed(seed)
    np.random.seed(seed)
    glow = G.Glow(hps)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():      # zero-init tails would make the coupling trivial (as bench.py)
        for name, p in glow.named_parameters():
            if ".f.4." in name or "conv2d_zeros" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.002)
    return glow.to(DEV), hps


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4), "rounds": len(v)}


def optimiser_on_random_gradients(ema_decay):
    """A HIP optimiser over config B's parameters with random gradients, one step done (state and chunk table built)."""
    glow, _ = make(64)
    params = [p for p in glow.parameters()]
    g = torch.Generator(device=DEV).manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=DEV) * 0.01
    kw = dict(ema_decay=ema_decay) if ema_decay else {}
    opt = training.HipAdam(params, lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"], **kw)
    opt.fused_step(ADAM["clip"], ADAM["max_norm"])
    torch.cuda.synchronize()
    return glow, params, opt


def merge(items, out_path):
    """`items`: "parent=FILE" / "new=FILE" in the order the runs were made; every FILE holds one JSON line of this script."""
    runs, order = {"parent": [], "new": []}, []
    for item in items:
        kind, _, path = item.partition("=")
        if kind not in runs or not path:
            raise SystemExit(f"--merge takes parent=FILE or new=FILE, not {item!r}")
        with open(path) as f:
            runs[kind].append(json.loads(f.read().strip().splitlines()[-1]))
        order.append(kind)
    par, new = runs["parent"], runs["new"]
    if not par or not new:
        raise SystemExit("--merge needs at least one parent= and one new= run")
    meds = lambda rs, sec, k: [r[sec][k]["median_ms"] for r in rs if k in r[sec]]
    med = statistics.median
    a_p, a_n = meds(par, "optim_ms", "a_ema_off"), meds(new, "optim_ms", "a_ema_off")
    b_n = meds(new, "optim_ms", "b_ema_on")
    c_p, c_n = meds(par, "optim_ms", "c_ema_off_plus_foreach_lerp"), meds(new, "optim_ms", "c_ema_off_plus_foreach_lerp")
    d_p, d_n = meds(par, "train_step_ms", "d_graphed_ema_off"), meds(new, "train_step_ms", "d_graphed_ema_off")
    d_on = meds(new, "train_step_ms", "d_graphed_ema_on")
    out = {
        "bench": "ema", "script": "scripts/bench_ema.py, one process per run, then scripts/bench_ema.py --merge",
        "how": "processes on one box in the order " + ", ".join(order) + " (parent = the parent commit's tree with this script); every "
               "figure is the median of the per-round means of its run; `comparisons` is computed by --merge from `runs`",
        "device": new[0]["device"], "config": new[0]["config"], "parameters": new[0]["parameters"], "chunks": new[0]["chunks"],
        "batch": new[0]["batch"],
        "a_optim_ema_off_ms": {"parent_runs": a_p, "this_change_runs": a_n},
        "b_optim_ema_on_ms": {"this_change_runs": b_n},
        "c_optim_ema_off_plus_foreach_lerp_ms": {"parent_runs": c_p, "this_change_runs": c_n,
                                                 "foreach_lerp_alone_parent_runs": meds(par, "optim_ms", "c_foreach_lerp_alone")},
        "d_captured_train_step_ms": {"ema_off_parent_runs": d_p, "ema_off_this_change_runs": d_n, "ema_on_this_change_runs": d_on},
        "e_swap_ms": {"this_change_runs": meds(new, "optim_ms", "e_swap")},
        "comparisons": {
            "a_parent_run_to_run_spread_ms": round(max(a_p) - min(a_p), 4),
            "a_this_change_minus_parent_median_ms": round(med(a_n) - med(a_p), 4),
            "d_off_parent_run_to_run_spread_ms": round(max(d_p) - min(d_p), 4),
            "d_off_this_change_minus_parent_median_ms": round(med(d_n) - med(d_p), 4),
            "b_below_c_on_parent": max(b_n) < min(c_p),
            "b_minus_a_ms": [r["optim_b_minus_a_ms"] for r in new],
            "c_on_parent_minus_b_ms": round(med(c_p) - med(b_n), 4),
            "d_on_minus_off_ms": [r["train_on_minus_off_ms"] for r in new if "train_on_minus_off_ms" in r],
        },
        "runs": {kind: rs for kind, rs in runs.items()},
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["comparisons"]))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", metavar="KIND=FILE", help="combine finished runs (parent=FILE / new=FILE) instead of measuring")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"), help="where --merge writes")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30, help="timed training steps per variant and round")
    ap.add_argument("--optim-steps", type=int, default=100, help="timed optimiser steps per variant and round")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    if not torch.cuda.is_available():
        print("bench_ema.py: no GPU visible", file=sys.stderr)
        return 2
    lib = _lib.lib()
    stream = lambda: _lib.stream_ptr(torch.device(DEV))

    # ---- (a) (b) (c) (e): the optimiser alone
    _, params_off, off = optimiser_on_random_gradients(0.0)
    norm = torch.zeros(1, device=DEV)
    n_off = off._n_chunks

    def step_a(i):
        _lib.check(lib.glowhip_optim_step(_lib.ptr(off._keep), n_off, 0, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], 0.0, 2 + i,
                                          ADAM["clip"], ADAM["max_norm"], _lib.ptr(off._partial), _lib.ptr(norm), 0, stream()))

    averages = [p.detach().clone() for p in params_off]
    live = [p.detach() for p in params_off]

    def lerp(i):
        torch._foreach_lerp_(averages, live, 0.001)

    def step_c(i):
        step_a(i)
        lerp(i)

    variants = {"a_ema_off": step_a, "c_ema_off_plus_foreach_lerp": step_c, "c_foreach_lerp_alone": lerp}
    if HAS_EMA:
        _, _, on = optimiser_on_random_gradients(0.999)
        n_on = on._n_chunks

        def step_b(i):
            _lib.check(lib.glowhip_optim_step_ema(_lib.ptr(on._keep), _lib.ptr(on._keep_ema), n_on, 0, ADAM["lr"], ADAM["b1"], ADAM["b2"],
                                                  ADAM["eps"], 0.0, 2 + i, ADAM["clip"], ADAM["max_norm"], 0.001, _lib.ptr(on._partial),
                                                  _lib.ptr(norm), 0, stream()))

        def swap_pair(i):
            for _ in range(2):
                _lib.check(lib.glowhip_optim_ema_swap(_lib.ptr(on._keep), _lib.ptr(on._keep_ema), n_on, stream()))

        variants.update({"b_ema_on": step_b, "e_swap_pair": swap_pair})
    with torch.no_grad():
        for fn in variants.values():
            for i in range(args.warmup):
                fn(i)
        torch.cuda.synchronize()
        optim = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                optim[k].append(timed(fn, args.optim_steps))
    n_params = sum(p.numel() for p in params_off)
    del off, params_off, averages, live
    if HAS_EMA:
        optim["e_swap"] = [v / 2 for v in optim.pop("e_swap_pair")]
        del on
    torch.cuda.empty_cache()

    # ---- (d): the captured training step
    train, captured = {}, None
    if not args.skip_train:
        g = torch.Generator().manual_seed(1)
        x = torch.rand(args.batch, 3, 64, 64, generator=g).to(DEV)
        loops = {"d_graphed_ema_off": training.TrainLoop(*make(args.batch), graph=True)}
        if HAS_EMA:
            loops["d_graphed_ema_on"] = training.TrainLoop(*make(args.batch, ema_decay=0.999), graph=True)
        for _ in range(max(args.warmup, training.TrainLoop.GRAPH_AFTER + 3)):
            for loop in loops.values():
                loop.step(x)
        torch.cuda.synchronize()
        assert all(loop.graph_error is None for loop in loops.values()), [loop.graph_error for loop in loops.values()]
        train = {k: [] for k in loops}
        for _ in range(args.rounds):
            for k, loop in loops.items():
                train[k].append(timed(lambda i: loop.step(x), args.steps))
        for loop in loops.values():
            loop.flush()
        captured = all(loop._graphed is not None for loop in loops.values())

    med = statistics.median
    out = {
        "bench": "ema", "device": torch.cuda.get_device_name(0), "config": "B (64x64x3 L3 K32 hidden 512)", "parameters": n_params,
        "chunks": n_off, "has_ema_entry_points": HAS_EMA, "batch": args.batch,
        "optim_steps_per_variant": args.rounds * args.optim_steps, "train_steps_per_variant": args.rounds * args.steps,
        "optim_ms": {k: summary(v) for k, v in optim.items()},
        "optim_a_spread_ms": round(max(optim["a_ema_off"]) - min(optim["a_ema_off"]), 4),
        "train_step_ms": {k: summary(v) for k, v in train.items()},
        "captured": captured,
    }
    if HAS_EMA:
        out["optim_b_minus_a_ms"] = round(med(optim["b_ema_on"]) - med(optim["a_ema_off"]), 4)
        out["optim_c_minus_b_ms"] = round(med(optim["c_ema_off_plus_foreach_lerp"]) - med(optim["b_ema_on"]), 4)
    if train:
        out["train_off_spread_ms"] = round(max(train["d_graphed_ema_off"]) - min(train["d_graphed_ema_off"]), 4)
        if HAS_EMA:
            out["train_on_minus_off_ms"] = round(med(train["d_graphed_ema_on"]) - med(train["d_graphed_ema_off"]), 4)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the class-conditional top head (csrc/tophead.hip) costs: step times at config B (celeba profile: 64x64x3, L 3, K 32,
hidden 512, batch 64) with num_classes = 40, weight_y = 0.01, multi_class (BCE), alternating IN ONE PROCESS between

  train (a) unconditional captured step          TrainLoop(graph=True)                    -- the baseline
  train (b) conditional captured step            TrainLoop(graph=True), labels
  train (c) conditional eager step, autograd     normal_flow + torch BCE + loss.backward() + fused optimiser step
  fwd   (a) / (b)                                inference forward (eval, no grad), un- / conditional

HIP events around blocks of steps, warm-up first, >= 200 timed steps per variant in `--rounds` alternations; min / median / max of
the per-round means (the spread of (a) is the noise figure of this box and hour).  Prints ONE JSON line; fails without a GPU.
Kernel times of the head come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--rounds 1 is enough)."""
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
from pytorch_glow_amd import parallel, training  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402

DEV = "cuda:0"


def make(conditional, batch, seed=0):
    hps = util.load_profile("celeba")
    hps.optim.num_batch_train = batch
    hps.device.graph = [DEV]
    hps.ablation.y_condition = conditional
    hps.ablation.y_criterion = "multi_class"
    hps.dataset.num_classes = 40
    hps.model.weight_y = 0.01
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
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4), "rounds": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_ycond.py: no GPU visible", file=sys.stderr)
        return 2
    g = torch.Generator().manual_seed(1)
    x = torch.rand(args.batch, 3, 64, 64, generator=g).to(DEV)
    yo = (torch.rand(args.batch, 40, generator=g) > 0.8).float().to(DEV)

    ga, hps_a = make(False, args.batch)
    gb, hps_b = make(True, args.batch)
    gc, hps_c = make(True, args.batch)
    la = training.TrainLoop(ga, hps_a, graph=True)
    lb = training.TrainLoop(gb, hps_b, graph=True)
    lc = training.TrainLoop(gc, hps_c, graph=False)
    step_a = lambda: la.step(x)
    step_b = lambda: lb.step(x, y_onehot=yo)

    def step_c():      # the reference-shaped call: forward, the user's torch loss, loss.backward(), optimiser step
        lc.lr = lc.scheduler(global_step=lc.global_step)
        for group in lc.optimizer.param_groups:
            group["lr"] = lc.lr
        parallel.train_step(gc, lc.optimizer, x, world=1, max_grad_clip=lc.max_grad_clip, max_grad_norm=lc.max_grad_norm,
                            direct=False, y_onehot=yo, criterion="multi_class")
        lc.global_step += 1

    lc.step(x, y_onehot=yo)      # (data-dependent init through the loop, then the autograd route by hand)
    for _ in range(max(args.warmup, training.TrainLoop.GRAPH_AFTER + 3)):
        step_a(); step_b(); step_c()
    torch.cuda.synchronize()
    assert la.graph_error is None and lb.graph_error is None, (la.graph_error, lb.graph_error)
    train = {"a": [], "b": [], "c": []}
    for _ in range(args.rounds):
        train["a"].append(timed(step_a, args.steps))
        train["b"].append(timed(step_b, args.steps))
        train["c"].append(timed(step_c, args.steps))
    la.flush(); lb.flush()
    captured = la._graphed is not None and lb._graphed is not None

    fa, _ = make(False, args.batch)
    fb, _ = make(True, args.batch)
    for m in (fa, fb):
        m.set_actnorm_inited()
        m.eval()
    fwd_a = lambda: fa.normal_flow(x, None)
    fwd_b = lambda: fb.normal_flow(x, yo)
    fwd = {"a": [], "b": []}
    with torch.no_grad():
        for _ in range(args.warmup):
            fwd_a(); fwd_b()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            fwd["a"].append(timed(fwd_a, args.steps))
            fwd["b"].append(timed(fwd_b, args.steps))
        plan = fb.flow.plan_for(x)
        plan.launch_counts(reset=True)
        fwd_b()
        counts = {k: v for k, v in plan.launch_counts().items() if "top_head" in k or "gaussian" in k}

    med = lambda v: statistics.median(v)
    out = {
        "bench": "ycond", "device": torch.cuda.get_device_name(0), "batch": args.batch, "config": "B (64x64x3 L3 K32 hidden 512)",
        "num_classes": 40, "weight_y": 0.01, "criterion": "multi_class", "timed_steps_per_variant": args.rounds * args.steps,
        "train_step_ms": {"a_unconditional_graphed": summary(train["a"]), "b_conditional_graphed": summary(train["b"]),
                          "c_conditional_eager_autograd": summary(train["c"])},
        "train_b_minus_a_ms": round(med(train["b"]) - med(train["a"]), 4),
        "train_a_spread_ms": round(max(train["a"]) - min(train["a"]), 4),
        "train_c_over_b": round(med(train["c"]) / med(train["b"]), 3),
        "captured": captured,
        "forward_ms": {"a_unconditional": summary(fwd["a"]), "b_conditional": summary(fwd["b"])},
        "forward_b_minus_a_ms": round(med(fwd["b"]) - med(fwd["a"]), 4),
        "forward_a_spread_ms": round(max(fwd["a"]) - min(fwd["a"]), 4),
        "head_launches_per_conditional_forward": counts,
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

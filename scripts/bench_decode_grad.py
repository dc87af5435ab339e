#!/usr/bin/env python3
"""What differentiating the decode costs.  At config B (64x64x3, L 3, K 32, hidden 512, batch 64) and config D (128x128x3, L 4,
K 48, hidden 512, batch 32), IN ONE PROCESS per config, alternating between

  (a) decode_latents(latents)                          the plain decode, no autograd
  (b) decode_latents(latents.requires_grad_()) + autograd.grad with a fixed dL/dx: decode + its VJP -- one taping re-encode of the
      decoded image plus the reverse-flow sweep (glowhip_plan_decode_vjp)
  (c) for scale: the training step's forward with tape + backward of the same model, without the optimiser
      (FlowPlan.glow_forward_train + glow_backward with every parameter gradient)

HIP events around blocks of steps, warm-up first, `--rounds` alternations; min / median / max of the per-round means.  Prints ONE
JSON line and writes it to --out (default profiles/decode_grad_bench.json); fails without a GPU.
`--one-vjp`: warm up, then run exactly one decode + VJP and exit -- the run to put under `rocprofv3 --kernel-trace --stats`."""
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
from pytorch_glow_amd.misc import util  # noqa: E402

DEV = "cuda:0"
CONFIGS = {"B": dict(image=64, L=3, K=32, hidden=512, batch=64), "D": dict(image=128, L=4, K=48, hidden=512, batch=32)}


def make(cfg, seed=0):
    hps = util.load_profile("celeba")
    hps.model.image_shape = [cfg["image"], cfg["image"], 3]
    hps.model.L, hps.model.K, hps.model.hidden_channels = cfg["L"], cfg["K"], cfg["hidden"]
    hps.optim.num_batch_train = cfg["batch"]
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


def run(name, args):
    cfg = CONFIGS[name]
    n, im = cfg["batch"], cfg["image"]
    g = torch.Generator().manual_seed(1)
    x = torch.rand(n, 3, im, im, generator=g).to(DEV)
    noise = (torch.rand(n, 3, im, im, generator=g) / 256).to(DEV)
    gx = torch.randn(n, 3, im, im, generator=g).to(DEV)
    glow = make(cfg)
    with torch.no_grad():
        glow.train()
        glow.normal_flow(x, None, noise=noise)      # data-dependent ActNorm init from this batch
        glow.eval()
        lat = glow.encode_latents(x, noise=noise, safe=False)
    plan = glow.flow.plan_for(x)
    leaf = lat.requires_grad_()
    gn = torch.full((n,), 1.0 / n, dtype=torch.float32, device=DEV)

    def dec():
        with torch.no_grad():
            return glow.decode_latents(lat, safe=False)

    def dec_vjp():
        with torch.enable_grad():
            return torch.autograd.grad(glow.decode_latents(leaf, safe=False), leaf.tensors(), gx)

    def train_fb():
        with torch.no_grad():
            _, _, tape = plan.glow_forward_train(x, noise, None, None, 0, 8)
            plan.glow_backward(x, tape, gn, None, None, None, 0, want_grad_x=False, persistent=True)

    for _ in range(args.warmup):
        dec(); dec_vjp()
    torch.cuda.synchronize()
    if args.one_vjp:
        plan.launch_counts(reset=True)
        dec_vjp()
        torch.cuda.synchronize()
        return {"config": name, "launch_counts_decode_plus_vjp": plan.launch_counts(reset=True)}
    for _ in range(args.warmup):
        train_fb()
    torch.cuda.synchronize()
    t = {"a": [], "b": [], "c": []}
    for _ in range(args.rounds):
        t["a"].append(timed(dec, args.steps))
        t["b"].append(timed(dec_vjp, args.steps))
        t["c"].append(timed(train_fb, args.steps))
    plan.launch_counts(reset=True)
    grads = dec_vjp()
    counts = plan.launch_counts(reset=True)
    med = statistics.median
    return {
        "config": f"{name} ({im}x{im}x3 L{cfg['L']} K{cfg['K']} hidden {cfg['hidden']})", "batch": n,
        "timed_steps_per_variant": args.rounds * args.steps,
        "decode_ms": summary(t["a"]), "decode_plus_vjp_ms": summary(t["b"]), "train_forward_backward_ms": summary(t["c"]),
        "vjp_alone_ms": round(med(t["b"]) - med(t["a"]), 4),
        "vjp_over_train_forward_backward": round((med(t["b"]) - med(t["a"])) / med(t["c"]), 4),
        "tape_bytes": int(G.lib().glowhip_plan_tape_bytes(plan._h, n)),
        "vjp_workspace_bytes": int(G.lib().glowhip_plan_decode_vjp_workspace_bytes(plan._h, n)),
        "launch_counts_decode_plus_vjp": counts,
        "gradients_finite": bool(all(torch.isfinite(t_).all() for t_ in grads)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="B,D")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one-vjp", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_grad_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_decode_grad.py: no GPU visible", file=sys.stderr)
        return 2
    out = {"bench": "decode_grad", "device": torch.cuda.get_device_name(0), "results": [run(c, args) for c in args.configs.split(",")]}
    line = json.dumps(out)
    print(line)
    if args.out and not args.one_vjp:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

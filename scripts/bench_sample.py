#!/usr/bin/env python3
"""What sampling costs, four ways, alternating IN ONE PROCESS at config B (64x64x3, L 3, K 32, hidden 512, batch 64) and
config E (256x256x3, L 6, K 32, hidden 512, batch 16):

  (a) reverse_flow(z=None, eps_std)        the reference's route: torch.randn per Split2d and for the top latent, eager launches
  (b) Glow.sample(eps_std)                 every draw inside the kernel that consumes it, eager launches
  (c) capture_sampler(...)()               (b) as one hipGraph launch, fp32 pixels out
  (d) capture_sampler(..., uint8=True)()   the same with 8-bit pixels stored by the final un-squeeze

Per variant: images/s from HIP events around blocks of steps (warm-up first, `--rounds` alternations; min / median / max of the
per-round means -- the spread of (a) is the noise figure of this box and hour) and the main thread's host time per step (the
wall clock of the enqueue loop alone, before the synchronise).  No range check in any variant.  Prints ONE JSON line and writes it
to --out (default profiles/sample_bench.json); fails without a GPU.  `--profile-only C` runs variant (c) alone at one config, for
a kernel trace."""
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

DEV = "cuda:0"
CONFIGS = {"B": dict(image=64, L=3, K=32, hidden=512, batch=64), "E": dict(image=256, L=6, K=32, hidden=512, batch=16)}


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
    glow = glow.to(DEV)
    x = torch.rand(cfg["batch"], 3, cfg["image"], cfg["image"], generator=g).to(DEV)
    with torch.no_grad():
        glow.train()
        glow.normal_flow(x, None)      # data-dependent ActNorm init from this batch
    return glow.eval()


def timed(fn, steps):
    """(device ms per step, host ms per step of the enqueue loop)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    host = (time.perf_counter() - t0) * 1e3 / steps
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, host


def summary(ms, host, batch):
    med = statistics.median(ms)
    return {"min_ms": round(min(ms), 4), "median_ms": round(med, 4), "max_ms": round(max(ms), 4), "rounds": len(ms),
            "images_per_s": round(batch / med * 1e3, 1), "host_ms_per_step": round(statistics.median(host), 4)}


def variants(glow, batch, eps_std):
    fp32 = glow.capture_sampler(batch, eps_std=eps_std, seed=1, call=0)
    u8 = glow.capture_sampler(batch, eps_std=eps_std, uint8=True, seed=1, call=0)
    return {
        "a_reverse_flow": lambda: glow.reverse_flow(None, None, eps_std=eps_std, safe=False),
        "b_sample_eager": lambda: glow.sample(batch, eps_std=eps_std, safe=False),
        "c_captured_fp32": fp32,
        "d_captured_uint8": u8,
    }


def run_config(name, args):
    cfg = CONFIGS[name]
    glow = make(cfg)
    batch = cfg["batch"]
    with torch.no_grad():
        v = variants(glow, batch, args.eps_std)
        for _ in range(args.warmup):
            for fn in v.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in v}
        host = {k: [] for k in v}
        for _ in range(args.rounds):
            for k, fn in v.items():
                d, h = timed(fn, args.steps)
                ms[k].append(d)
                host[k].append(h)
        plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))
        plan.launch_counts(reset=True)
        v["a_reverse_flow"]()
        launches_a = sum(plan.launch_counts(reset=True).values())
        v["b_sample_eager"]()
        launches_b = sum(plan.launch_counts(reset=True).values())
        same = bool(torch.equal(v["c_captured_fp32"]().clone(), glow.sample(batch, eps_std=args.eps_std, safe=False, seed=1,
                                                                           call=v["c_captured_fp32"].last_position[1])))
    out = {k: summary(ms[k], host[k], batch) for k in v}
    out.update(config=f"{name} ({cfg['image']}x{cfg['image']}x3 L{cfg['L']} K{cfg['K']} hidden {cfg['hidden']})", batch=batch,
               plan_launches_counted={"a_reverse_flow": launches_a, "b_sample_eager": launches_b},
               a_spread_ms=round(max(ms["a_reverse_flow"]) - min(ms["a_reverse_flow"]), 4),
               captured_equals_eager_bitwise=same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="B,E")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--eps-std", type=float, default=0.7)
    ap.add_argument("--profile-only", default=None, help="config name: replay the captured fp32 sampler --steps times and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_sample.py: no GPU visible", file=sys.stderr)
        return 2
    if args.profile_only:
        cfg = CONFIGS[args.profile_only]
        glow = make(cfg)
        with torch.no_grad():
            gs = glow.capture_sampler(cfg["batch"], eps_std=args.eps_std, seed=1, call=0)
            for _ in range(args.steps):
                gs()
        torch.cuda.synchronize()
        return 0
    out = {"bench": "sample", "device": torch.cuda.get_device_name(0), "eps_std": args.eps_std,
           "timed_steps_per_variant": args.rounds * args.steps,
           "configs": {name: run_config(name, args) for name in args.configs.split(",")}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

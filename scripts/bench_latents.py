#!/usr/bin/env python3
"""What keeping the full latents costs: the inference forward at config B (celeba profile: 64x64x3, L 3, K 32, hidden 512,
batch 64) with and without latent buffers bound (glowhip_plan_bind_latents), alternating IN ONE PROCESS between

  (a) normal_flow(x, noise=...)                        nothing bound: every Split2d scores its z2 half and drops it
  (b) normal_flow(x, noise=..., eps_out=buffers)       the same launches; the prior kernels also store eps (9 216 floats per image)
  (c) encode_latents(x, noise=...)                     the public call: (b) + allocating the buffers
  (d) decode_latents(latents)                          the inverse with the latents' own eps

HIP events around blocks of steps, warm-up first, `--rounds` alternations; min / median / max of the per-round means (the spread
of (a) is the noise figure of this box and hour).  Prints ONE JSON line and writes it to --out (default
profiles/latents_bench.json); fails without a GPU."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latents_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_latents.py: no GPU visible", file=sys.stderr)
        return 2
    g = torch.Generator().manual_seed(1)
    x = torch.rand(args.batch, 3, 64, 64, generator=g).to(DEV)
    noise = (torch.rand(args.batch, 3, 64, 64, generator=g) / 256).to(DEV)
    glow = make(args.batch)
    with torch.no_grad():
        glow.train()
        glow.normal_flow(x, None, noise=noise)      # data-dependent ActNorm init from this batch
        glow.eval()
        plan = glow.flow.plan_for(x)
        bufs = plan.latent_buffers(args.batch)
        fwd_a = lambda: glow.normal_flow(x, None, noise=noise)
        fwd_b = lambda: glow.normal_flow(x, None, noise=noise, eps_out=bufs)
        fwd_c = lambda: glow.encode_latents(x, noise=noise, safe=False)
        lat = fwd_c()
        dec_d = lambda: glow.decode_latents(lat, safe=False)
        for _ in range(args.warmup):
            fwd_a(); fwd_b(); fwd_c(); dec_d()
        torch.cuda.synchronize()
        t = {"a": [], "b": [], "c": [], "d": []}
        for _ in range(args.rounds):
            t["a"].append(timed(fwd_a, args.steps))
            t["b"].append(timed(fwd_b, args.steps))
            t["c"].append(timed(fwd_c, args.steps))
            t["d"].append(timed(dec_d, args.steps))
        plan.launch_counts(reset=True)
        za, nlla, _ = fwd_a()
        ca = plan.launch_counts(reset=True)
        zb, nllb, _ = fwd_b()
        cb = plan.launch_counts(reset=True)
        back = dec_d()
        rt = (back - (x + noise)).abs().max().item()
    med = statistics.median
    extra_floats = sum(int(np.prod(s)) for s in plan.split_chw)
    out = {
        "bench": "latents", "device": torch.cuda.get_device_name(0), "batch": args.batch, "config": "B (64x64x3 L3 K32 hidden 512)",
        "timed_steps_per_variant": args.rounds * args.steps,
        "forward_ms": {"a_unbound": summary(t["a"]), "b_latents_bound": summary(t["b"]), "c_encode_latents": summary(t["c"])},
        "decode_latents_ms": summary(t["d"]),
        "forward_b_minus_a_ms": round(med(t["b"]) - med(t["a"]), 4),
        "forward_c_minus_a_ms": round(med(t["c"]) - med(t["a"]), 4),
        "forward_a_spread_ms": round(max(t["a"]) - min(t["a"]), 4),
        "extra_floats_per_image": extra_floats, "extra_bytes_per_batch": 4 * extra_floats * args.batch,
        "z_nll_bitwise_equal_bound_vs_unbound": bool(torch.equal(za, zb) and torch.equal(nlla, nllb)),
        "same_launch_counts": ca == cb, "split_launches": {k: v for k, v in cb.items() if k.startswith("split_prior(")},
        "round_trip_max_abs": rt,
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

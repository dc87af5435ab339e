#!/usr/bin/env python3
"""What the LU parameterisation of the invertible 1x1 convolutions costs and saves: the same weights as a dense model and as an
``lu_decomposition=True`` model (misc.util.lu_state_dict_from_dense), at config B (64x64x3, L 3, K 32, hidden 512, batch 64) and
config E (256x256x3, L 6, K 32, hidden 512, batch 16), IN ONE PROCESS, each of

  pack_forward     glowhip_plan_pack_for(INFERENCE): scale tables, weight images, log|det W| (dense: an LU per matrix; LU form:
                   the assemble kernel, no factorisation)
  pack_inverse     ... with GLOWHIP_PACK_INVERSE: W^-1 as well (dense: Gauss-Jordan; LU form: two substitutions per column)
  forward          one inference forward with its pack (normal_flow, repack=True)
  sample           one decode with its inverting pack
  train            (config B) one training step's forward + backward with its pack (loss_and_grads, force_pack=True)

in its own timed region: HIP events around every repetition, warm-up first, the MEDIAN reported (min and max beside it).  The
yardstick is the dense route in the same run -- its kernels are unchanged in behaviour by the LU form.  Prints ONE JSON line and writes it to
--out (default profiles/invconv_lu_bench.json); fails without a GPU.  ``--case dense|lu`` and ``--only NAME`` restrict the run
(one case per rocprofv3 --kernel-trace --stats table)."""
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
CONFIGS = {"B": dict(image=64, L=3, K=32, hidden=512, batch=64), "E": dict(image=256, L=6, K=32, hidden=512, batch=16)}


def hps_for(c, lu):
    return util.AttrDict(dict(
        model=dict(image_shape=[c["image"], c["image"], 3], hidden_channels=c["hidden"], K=c["K"], L=c["L"], actnorm_scale=1.0,
                   n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=lu, flow_permutation="invconv", flow_coupling="affine"),
        optim=dict(num_batch_train=c["batch"]), dataset=dict(num_classes=1), device=dict(graph=[DEV])))


def build(c, x, noise, seed=0):
    """(dense, lu): the dense model after its data-dependent init on x, and the LU model holding the same state."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    dense = G.Glow(hps_for(c, False))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in dense.named_parameters():
            if ".f.4." in name or "conv2d_zeros" in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.002)
            elif name.endswith("invconv.weight"):      # away from orthogonal, as after some training
                p.add_(0.02 * torch.randn(p.shape, generator=g))
    dense = dense.to(DEV)
    with torch.no_grad():
        dense.train()
        dense.normal_flow(x, None, noise=noise)
    sd = util.lu_state_dict_from_dense({k: v.detach().cpu() for k, v in dense.state_dict().items()})
    lu = G.Glow(hps_for(c, True))
    lu.load_state_dict(sd, strict=True)
    lu.set_actnorm_inited()
    return dense, lu.to(DEV)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4), "reps": reps}


def measure(glow, c, x, noise, reps, warmup, train, only):
    res = {}
    plan = glow.flow.plan_for(x)
    with torch.no_grad():
        glow.eval()
        z, _, _ = glow.normal_flow(x, None, noise=noise)
        eps = glow.flow.draw_eps(x.shape[0], plan, 0.7, x.device)
        cases = dict(
            pack_forward=lambda: plan.pack(plan.PACK_INFERENCE, merge=False),
            pack_inverse=lambda: plan.pack(plan.PACK_INFERENCE | plan.PACK_INVERSE, merge=False),
            forward=lambda: glow.normal_flow(x, None, noise=noise, repack=True),
            sample=lambda: plan.decode(z, eps, None, want_logdet=False, repack=True))
        for name, fn in cases.items():
            if only in (None, name):
                res[name] = timed(fn, reps, warmup)
        res["pack_counters"] = {k: v for k, v in plan.launch_counts(reset=True).items() if k.startswith("pack:")}
    if train and only in (None, "train"):
        glow.train()
        res["train"] = timed(lambda: glow.loss_and_grads(x, noise=noise, force_pack=True), reps, warmup)
        glow.eval()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="B,E")
    ap.add_argument("--case", choices=["dense", "lu"], default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "invconv_lu_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_invconv_lu.py: no GPU visible", file=sys.stderr)
        return 2
    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "configs": {}}
    for name in args.configs.split(","):
        c = CONFIGS[name]
        g = torch.Generator().manual_seed(1)
        x = torch.rand(c["batch"], 3, c["image"], c["image"], generator=g).to(DEV)
        noise = (torch.rand(c["batch"], 3, c["image"], c["image"], generator=g) / 256).to(DEV)
        dense, lu = build(c, x, noise)
        out = dict(c)
        for case, glow in (("dense", dense), ("lu", lu)):
            if args.case in (None, case):
                out[case] = measure(glow, c, x, noise, args.reps, args.warmup, name == "B", args.only)
        if "dense" in out and "lu" in out:
            with torch.no_grad():      # the two forms compute the same model: W differs by the fp32 rounding of the factors
                nd = dense.normal_flow(x, None, noise=noise)[1]
                nl = lu.normal_flow(x, None, noise=noise)[1]
            out["nll_max_abs_diff"] = float((nd - nl).abs().max())
        rec["configs"][name] = out
        del dense, lu
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

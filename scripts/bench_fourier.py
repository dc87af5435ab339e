#!/usr/bin/env python3
"""What Fourier-domain measurements cost the restoration path.  IN ONE PROCESS, alternating between the variants

  fourier  glowhip_restore_objective_fourier alone (preallocated outputs and scratch, a 0/1 k-space mask as the weight)
  plain    glowhip_restore_objective on the same image with a real target and the same mask: the one launch every other objective
           is measured against
  torch    the objective as torch calls: `torch.fft.fft2(norm="ortho")`, the element-wise operations, `torch.fft.ifft2` -- the
           yardstick; where this torch build cannot run it on the device the column is dropped and the reason recorded
  fit      `LatentFit.step_captured` with ``fourier=True``, beside the same loop without it (in-painting under the same mask): the
           whole iteration -- decode, objective, decode VJP, fused Adam step, histories -- as one hipGraph launch (config B)

at 64x64x3 with batch 1 and batch 64, 128x128x3 with batch 32 and 256x256x3 with batch 16.
`objective_us`: `--reps` back-to-back calls on an idle stream between two HIP events, per call (the launches queue behind each other,
so the host's enqueue time is hidden once the first is running).  `fourier_effective_TBps`: the 60 bytes per pixel the three launches
move through HBM (x 4, the row pass's spectrum written 8 and read 8, target 8, weight 4, resid 8, the adjoint's intermediate written
8 and read 8, grad_x 4) over that time, to be read beside the 6.0 - 6.3 TB/s streaming rate of an MI355X.  `iteration_ms`: `--steps`
captured iterations between two HIP events, per iteration.  Warm-up first, then `--rounds` alternations; min / median / max of the
per-round means; `slower_than_torch` is set where the call's median exceeds the torch variant's by more than the latter's
round-to-round spread (max - min).
Prints ONE JSON line and writes it to --out (default profiles/fourier_bench.json); fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_glow_amd.network import Inferer, LatentFit, fourier2d, fourier_mask, fourier_scratch, restore_objective  # noqa: E402

from bench_decode_grad import CONFIGS, DEV, make  # noqa: E402
from bench_deblur import between_events, summary  # noqa: E402

SHAPES = ((64, 1), (64, 64), (128, 32), (256, 16))      # (side, batch)


def torch_objective(x, t, w, inv):
    """(loss, grad_x) as torch calls: t complex64 (N,C,H,W), w real."""
    d = torch.fft.fft2(x, norm="ortho") - t
    r = w * d
    loss = (r.real * d.real + r.imag * d.imag).sum(dim=(1, 2, 3)) * inv
    g = torch.fft.ifft2((2.0 * inv).view(-1, 1, 1, 1) * r, norm="ortho").real
    return loss, g


def objective_case(side, n, args):
    g = torch.Generator().manual_seed(side + n)
    x = torch.rand(n, 3, side, side, generator=g).to(DEV)
    y = torch.rand(n, 3, side, side, generator=g).to(DEV)
    w = fourier_mask((side, side), 0.25, seed=1).to(DEV).expand(n, 3, side, side).contiguous()
    inv = 1.0 / w.sum(dim=(1, 2, 3)).clamp(min=1.0)
    t = fourier2d(y)
    t_real = torch.view_as_real(t).contiguous()
    grad, loss, resid = torch.empty_like(x), torch.empty(n, device=DEV), torch.empty_like(t_real)
    scratch = fourier_scratch(n, 3, side, side, DEV)
    calls = {"fourier": lambda: restore_objective(x, t_real, w, inv, 1, grad_out=grad, loss_out=loss, resid_out=resid, fourier=True,
                                                  scratch=scratch),
             "plain": lambda: restore_objective(x, y, w, inv, 1, grad_out=grad, loss_out=loss)}
    torch_error = None
    try:
        l_ref, g_ref = torch_objective(x, t, w, inv)
        torch.cuda.synchronize()
        calls["torch"] = lambda: torch_objective(x, t, w, inv)
    except Exception as e:       # this torch build has no device FFT: the column is dropped, and the reason kept
        torch_error = f"{type(e).__name__}: {str(e)[:200]}"
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            ms[name].append(between_events(fn, args.reps))
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"shape": f"{side}x{side}x3", "batch": n, "timed_calls_per_variant": args.rounds * args.reps,
           "fourier_objective_us": summary(ms["fourier"], 1e3, 2), "plain_objective_us": summary(ms["plain"], 1e3, 2),
           "fourier_over_plain": round(med["fourier"] / med["plain"], 2),
           "fourier_effective_TBps": round(60.0 * x.numel() / (med["fourier"] * 1e-3) / 1e12, 3)}
    if torch_error is None:
        calls["fourier"]()
        out.update({"torch_objective_us": summary(ms["torch"], 1e3, 2), "fourier_over_torch": round(med["fourier"] / med["torch"], 3),
                    "slower_than_torch": bool(med["fourier"] - med["torch"] > max(ms["torch"]) - min(ms["torch"])),
                    "max_abs_grad_difference_from_torch": float((grad - g_ref).abs().max())})
    else:
        out["torch_fft_unavailable"] = torch_error
    return out


def fit_case(glow, inf, x, args):
    n, side = x.shape[0], x.shape[-1]
    mask = fourier_mask((side, side), 0.25, seed=1).to(DEV)
    with torch.no_grad():
        init = inf.encode_full(x)
    fits = {"none": LatentFit(glow, x, weight=mask, init=init, steps=max(args.steps, 2), lr=args.lr),
            "fourier": LatentFit(glow, fourier2d(x), weight=mask, init=init, steps=max(args.steps, 2), lr=args.lr, fourier=True)}
    for name, fit in fits.items():
        fit.reset()
        for _ in range(args.warmup):
            fit.step_eager()
        if not fit.capture():
            raise RuntimeError(f"{name}: capture failed: {fit.graph_error}")
        for _ in range(args.warmup):
            fit.step_captured()
    it_ms = {k: [] for k in fits}
    for _ in range(args.rounds):
        for name, fit in fits.items():
            it_ms[name].append(between_events(fit.step_captured, args.steps))
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(f.loss_hist).all()) and bool(torch.isfinite(f.norm_hist).all()) for f in fits.values())
    med = {k: statistics.median(v) for k, v in it_ms.items()}
    return {"batch": n, "timed_iterations_per_variant": args.rounds * args.steps, "histories_finite": finite,
            "iteration_ms_without_fourier": summary(it_ms["none"]), "iteration_ms_with_fourier": summary(it_ms["fourier"]),
            "iteration_fourier_minus_none_ms": round(med["fourier"] - med["none"], 4),
            "iteration_fourier_over_none": round(med["fourier"] / med["none"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batches", default="1,64", help="batches of the captured iteration")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed captured iterations per variant and round")
    ap.add_argument("--reps", type=int, default=100, help="timed objective calls per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fourier_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_fourier.py: no GPU visible", file=sys.stderr)
        return 2
    out = {"bench": "fourier", "device": torch.cuda.get_device_name(0),
           "objective": [objective_case(side, n, args) for side, n in SHAPES]}
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
    out["fit_config"] = f"{args.config} ({im}x{im}x3 L{cfg['L']} K{cfg['K']} hidden {cfg['hidden']})"
    out["fit"] = [fit_case(glow, inf, x[:n].contiguous(), args) for n in batches]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

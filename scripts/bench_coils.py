#!/usr/bin/env python3
"""What multi-coil k-space costs the restoration path.  IN ONE PROCESS, alternating between the variants

  coils    (k)    glowhip_restore_objective_coils alone (preallocated outputs and scratch, a 0/1 k-space mask as the weight, maps
                  shared by the batch)
  planes   (f.Q)  glowhip_restore_objective_fourier, the existing single-coil call, on the same number of planes, N C Q: the floor
                  the transform part of the new call cannot beat (it does no coil product and no coil sum, so it is not the same
                  result)
  torch    (a)    the objective as torch calls: the broadcast product with the maps, `torch.fft.fft2(norm="ortho")`, the
                  element-wise work, `torch.fft.ifft2`, the product with the conjugate maps and the sum over the coils -- the
                  yardstick; where this torch build cannot run it on the device the column is dropped and the reason recorded
  fit      (c)    `LatentFit.step_captured` with ``coils=`` (Q = 8 and Q = 32), beside the same loop without it (in-painting under
                  the same mask) and the single-coil ``fourier=True`` loop: the whole iteration -- decode, objective, decode VJP,
                  fused Adam step, histories -- as one hipGraph launch (config B)

at 64x64x3 with batch 1 and batch 64 and 256x256x1 with batch 16, each with Q = 8 and Q = 32 coils.
`objective_us`: `--reps` back-to-back calls on an idle stream between two HIP events, per call.  `coils_effective_TBps`: the bytes
the three launches move, counted as
    N C H W (12 + 48 Q) + 8 Q H W
-- per image pixel x 4, weight 4 and grad_x 4 (x and the weight are re-read per coil, from L2); per coil coefficient the row pass's
spectrum written 8 and read 8, target 8, resid 8, the adjoint's intermediate written 8 and read 8; the shared maps 8 per coil pixel,
once -- over that time, to be read beside the 6.0 - 6.3 TB/s streaming rate of an MI355X.  `iteration_ms`: `--steps` captured
iterations between two HIP events, per iteration; `objective_share_of_iteration` is the new call's median over the coil loop's.
Warm-up first, then `--rounds` alternations; min / median / max of the per-round means.
Prints ONE JSON line and writes it to --out (default profiles/coils_bench.json); fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pytorch_glow_amd.network import (Inferer, LatentFit, coil_maps, coils2d, coils_scratch, fourier2d, fourier_mask,  # noqa: E402
                                      fourier_scratch, restore_objective)

from bench_decode_grad import CONFIGS, DEV, make  # noqa: E402
from bench_deblur import between_events, summary  # noqa: E402

SHAPES = ((64, 3, 1), (64, 3, 64), (256, 1, 16))      # (side, channels, batch)
COILS = (8, 32)


def torch_objective(x, t, s, w, inv):
    """(loss, grad_x) as torch calls: t complex64 (N,C,Q,H,W), s complex64 (Q,H,W), w real (N,C,H,W)."""
    d = torch.fft.fft2(s * x.unsqueeze(2), norm="ortho") - t
    r = w.unsqueeze(2) * d
    loss = (r.real * d.real + r.imag * d.imag).sum(dim=(1, 2, 3, 4)) * inv
    g = (s.conj() * torch.fft.ifft2((2.0 * inv).view(-1, 1, 1, 1, 1) * r, norm="ortho")).real.sum(dim=2)
    return loss, g


def objective_case(side, c, n, q, args):
    g = torch.Generator().manual_seed(side + n + q)
    x = torch.rand(n, c, side, side, generator=g).to(DEV)
    y = torch.rand(n, c, side, side, generator=g).to(DEV)
    s = coil_maps((side, side), q).to(DEV)
    s_real = torch.view_as_real(s).contiguous()
    w = fourier_mask((side, side), 0.25, seed=1).to(DEV).expand(n, c, side, side).contiguous()
    inv = 1.0 / (q * w.sum(dim=(1, 2, 3))).clamp(min=1.0)
    t = coils2d(y, s)
    t_real = torch.view_as_real(t).contiguous()
    grad, loss, resid = torch.empty_like(x), torch.empty(n, device=DEV), torch.empty_like(t_real)
    scratch = coils_scratch(n, c, q, side, side, DEV)
    # the single-coil call on as many planes: N images of C Q channels
    xq = torch.rand(n, c * q, side, side, generator=g).to(DEV)
    tq_real = t_real.view(n, c * q, side, side, 2)
    wq = w.unsqueeze(2).expand(n, c, q, side, side).reshape(n, c * q, side, side).contiguous()
    gradq, residq = torch.empty_like(xq), torch.empty_like(tq_real)
    scratchq = fourier_scratch(n, c * q, side, side, DEV)
    calls = {"coils": lambda: restore_objective(x, t_real, w, inv, 1, grad_out=grad, loss_out=loss, resid_out=resid, fourier=True,
                                                coils=s_real, scratch=scratch),
             "planes": lambda: restore_objective(xq, tq_real, wq, inv, 1, grad_out=gradq, loss_out=loss, resid_out=residq, fourier=True,
                                                 scratch=scratchq)}
    torch_error = None
    try:
        l_ref, g_ref = torch_objective(x, t, s, w, inv)
        torch.cuda.synchronize()
        calls["torch"] = lambda: torch_objective(x, t, s, w, inv)
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
    nbytes = x.numel() * (12 + 48 * q) + 8 * q * side * side
    out = {"shape": f"{side}x{side}x{c}", "batch": n, "coils": q, "timed_calls_per_variant": args.rounds * args.reps,
           "coils_objective_us": summary(ms["coils"], 1e3, 2), "planes_objective_us": summary(ms["planes"], 1e3, 2),
           "coils_over_planes": round(med["coils"] / med["planes"], 3), "bytes_counted": nbytes,
           "coils_effective_TBps": round(nbytes / (med["coils"] * 1e-3) / 1e12, 3)}
    if torch_error is None:
        calls["coils"]()
        out.update({"torch_objective_us": summary(ms["torch"], 1e3, 2), "coils_over_torch": round(med["coils"] / med["torch"], 3),
                    "slower_than_torch": bool(med["coils"] - med["torch"] > max(ms["torch"]) - min(ms["torch"])),
                    "max_abs_grad_difference_from_torch": float((grad - g_ref).abs().max())})
    else:
        out["torch_fft_unavailable"] = torch_error
    return out


def fit_case(glow, inf, x, args):
    n, side = x.shape[0], x.shape[-1]
    mask = fourier_mask((side, side), 0.25, seed=1).to(DEV)
    with torch.no_grad():
        init = inf.encode_full(x)
    kw = dict(weight=mask, init=init, steps=max(args.steps, 2), lr=args.lr)
    fits = {"none": LatentFit(glow, x, **kw), "fourier": LatentFit(glow, fourier2d(x), fourier=True, **kw)}
    objective = {}
    for q in COILS:
        s = coil_maps((side, side), q).to(DEV)
        fit = fits[f"coils{q}"] = LatentFit(glow, coils2d(x, s), fourier=True, coils=s, **kw)
        grad, loss = torch.empty_like(fit.image), torch.empty(n, device=DEV)
        image = x.clone()
        objective[q] = lambda fit=fit, image=image, grad=grad, loss=loss: restore_objective(
            image, fit.target, fit.weight, fit.inv_wsum, 1, grad_out=grad, loss_out=loss, resid_out=fit.resid, fourier=True,
            coils=fit.coils, scratch=fit.op_scratch)
    for name, fit in fits.items():
        fit.reset()
        for _ in range(args.warmup):
            fit.step_eager()
        if not fit.capture():
            raise RuntimeError(f"{name}: capture failed: {fit.graph_error}")
        for _ in range(args.warmup):
            fit.step_captured()
    it_ms = {k: [] for k in fits}
    ob_ms = {q: [] for q in COILS}
    for _ in range(args.rounds):
        for name, fit in fits.items():
            it_ms[name].append(between_events(fit.step_captured, args.steps))
        for q in COILS:
            ob_ms[q].append(between_events(objective[q], args.reps))
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(f.loss_hist).all()) and bool(torch.isfinite(f.norm_hist).all()) for f in fits.values())
    med = {k: statistics.median(v) for k, v in it_ms.items()}
    out = {"batch": n, "timed_iterations_per_variant": args.rounds * args.steps, "histories_finite": finite,
           "iteration_ms_without_fourier": summary(it_ms["none"]), "iteration_ms_with_fourier": summary(it_ms["fourier"])}
    for q in COILS:
        ob = statistics.median(ob_ms[q])
        out[f"coils{q}"] = {"iteration_ms": summary(it_ms[f"coils{q}"]), "objective_us": summary(ob_ms[q], 1e3, 2),
                            "iteration_over_none": round(med[f"coils{q}"] / med["none"], 4),
                            "iteration_over_fourier": round(med[f"coils{q}"] / med["fourier"], 4),
                            "iteration_minus_none_ms": round(med[f"coils{q}"] - med["none"], 4),
                            "objective_share_of_iteration": round(ob / med[f"coils{q}"], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="B")
    ap.add_argument("--batches", default="1,64", help="batches of the captured iteration")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed captured iterations per variant and round")
    ap.add_argument("--reps", type=int, default=100, help="timed objective calls per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coils_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_coils.py: no GPU visible", file=sys.stderr)
        return 2
    out = {"bench": "coils", "device": torch.cuda.get_device_name(0),
           "objective": [objective_case(side, c, n, q, args) for side, c, n in SHAPES for q in COILS]}
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

"""fp64 oracle of the held-out evaluation (csrc/evaluate.hip, network/evaluate.py).

`level_terms` walks the oracle's layers itself (oracle/glow_oracle.py: flow_layout, flowstep, split2d; the top prior as
tests/ycond_oracle.py states it) and closes a level behind every Split2d and behind the top prior: the per-level parts of
Glow.normal_flow's objective (reference network/model.py:409-452).  `fold` restates the fold kernel's definitions in numpy fp64
and Python integers: per-image figures, the fixed-point sums (rint(v * 2^32), summed as integers), min / max, the histogram."""
import numpy as np
import torch

from oracle import glow_oracle as O

import ycond_oracle as Y

LN2 = float(np.log(2.0))
FIX = 2.0 ** 32
RANGE = 2048.0      # include/glowhip.h: an image whose |bits/dim| figures are not below this is flagged


def n_levels(cfg):
    return sum(1 for kind, _, _ in O.flow_layout(cfg) if kind == "split") + 1


def level_terms(x, noise, sd, cfg, y_onehot=None, perm_tables=None):
    """(terms [n_levels, N] in nats, offset, objective [N]) in fp64: terms[l] = the log-determinants of level l's FlowSteps plus the
    log-density its Split2d (the last level: the top prior) scores; objective = offset + sum_l terms[l]."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x, noise = x.double(), noise.double()
    z = x + noise
    n = x.shape[0]
    offset = float(-np.log(2.0 ** cfg["n_bits_x"])) * x[0].numel()
    terms, run = [], torch.zeros(n, dtype=torch.float64)
    for kind, i, _ in O.flow_layout(cfg):
        prefix = f"flow.layers.{i}."
        if kind == "squeeze":
            z = O.squeeze2d(z, 2)
        elif kind == "step":
            z, run = O.flowstep(z, run, sd, prefix, cfg["flow_permutation"], cfg["flow_coupling"], reverse=False,
                                perm_tables=None if perm_tables is None else perm_tables[i])
        else:
            z, run = O.split2d(z, run, sd, prefix, reverse=False)
            terms.append(run)
            run = torch.zeros(n, dtype=torch.float64)
    head_sd = dict(sd)
    head_sd["h_top"] = torch.zeros((n, 2 * z.shape[1]) + tuple(z.shape[2:]), dtype=torch.float64)
    mean, logs = Y.prior(head_sd, cfg, None if y_onehot is None else y_onehot.double())
    terms.append(run + O.gaussian_logp(mean, logs, z))
    terms = torch.stack(terms)
    return terms, offset, offset + terms.sum(dim=0)


def q(v):
    """rint(v * 2^32) as a Python integer (round half to even, as the kernel's conversion)."""
    return int(np.rint(np.float64(v) * FIX))


def fixed_total(values):
    return sum(q(v) for v in values)


def per_image(objective, dims):
    """objective [K, N] (any float dtype; widened to fp64) -> (bpd [N], bpd_single [N]) in fp64, max-subtracted log-sum-exp."""
    o = np.asarray(objective, dtype=np.float64)
    K = o.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):      # (an image with a non-finite draw comes out non-finite: it is flagged)
        m = o.max(axis=0)
        L = m + np.log(np.exp(o - m).sum(axis=0)) - np.log(float(K))
        return -L / (LN2 * dims), -o.mean(axis=0) / (LN2 * dims)


def level_bits(terms, dims):
    """terms [K, n_levels, N] -> [n_levels, N] bits/dim of the draw-averaged figure."""
    return -np.asarray(terms, dtype=np.float64).mean(axis=0) / (LN2 * dims)


def hist_slot(b, bins, lo, hi):
    """Where the header puts a value: 'under', 'over' or the bin index."""
    if b < lo:
        return "under"
    if b >= hi:
        return "over"
    return min(int(np.floor((np.float64(b) - lo) * (np.float64(bins) / (hi - lo)))), bins - 1)


def fold(objective, dims, terms=None, hist=None, bpd32=None):
    """The state a fold of these images must leave.  ``bpd32``: the per-image fp32 values to build the integer sums from (the
    device's own output: 'the integer sums GIVEN the per-image values'); None: the oracle's, rounded to fp32."""
    o = np.asarray(objective, dtype=np.float64)
    bpd, single = per_image(o, dims)
    flagged = ~np.isfinite(o).all(axis=0)
    with np.errstate(invalid="ignore"):
        flagged |= ~(np.abs(bpd) < RANGE) | ~(np.abs(single) < RANGE)
        lev = None
        if terms is not None:
            lev = level_bits(terms, dims)
            flagged |= ~(np.abs(lev) < RANGE).all(axis=0)
    keep = ~flagged
    b32 = np.where(keep, bpd, np.nan).astype(np.float32) if bpd32 is None else np.asarray(bpd32, dtype=np.float32)
    vals = b32[keep].astype(np.float64)
    out = dict(count=int(keep.sum()), flagged=int(flagged.sum()), bpd=bpd, single=single, keep=keep, bpd32=b32,
               sum_bpd=fixed_total(vals), sum_bpd2=fixed_total(vals * vals), sum_single=fixed_total(single[keep]),
               min=min((q(v) for v in vals), default=None), max=max((q(v) for v in vals), default=None))
    if lev is not None:
        out["sum_level"] = [fixed_total(row[keep]) for row in lev]
        out["level_bits"] = lev
    if hist is not None:
        bins, lo, hi = hist
        counts, under, over = [0] * bins, 0, 0
        for v in vals:
            s = hist_slot(v, bins, lo, hi)
            if s == "under":
                under += 1
            elif s == "over":
                over += 1
            else:
                counts[s] += 1
        out.update(hist=counts, under=under, over=over)
    return out

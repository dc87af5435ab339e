"""Held-out evaluation on the device: importance-weighted bits per dimension of a data set and where the bits go, level by level.

The reference quotes bits/dim per training batch (network/trainer.py:123-133) and has no evaluation pass.  `Evaluator` runs the
inference forward K times per batch under K named dequantisation draws (csrc/plan.hip: the draw of a forward is ``(seed, call)``,
made inside the leading squeeze -- K draws cost K forwards and no noise tensor), and folds the K objectives -- and, with
``levels``, the per-level terms the plan's executor writes from snapshots of its integer log-det accumulators -- into a
device-resident state with ONE launch per batch (csrc/evaluate.hip).  No host sync per batch; one when the result is read.

    bits_per_dim         mean over images of  -(logsumexp_k objective_k - ln K) / (ln2 D)     the bound log p(x) >= log 1/K sum_k exp(objective_k)
    bits_per_dim_single  mean over images and draws of  -objective / (ln2 D)                  what `nll.mean()` of one draw estimates
    level_bits[l]        the share of level l in bits_per_dim_single; n_bits + sum(level_bits) = bits_per_dim_single.
                         The importance-weighted bound does not decompose by level; the draw-averaged figure does.
"""
import ctypes
from fractions import Fraction

import torch

from .. import _lib
from .._lib import check, lib, ptr, stream_ptr
from . import module
from .model import dequant_position

_TWO63 = 1 << 63


def _s128(pair):
    """The signed integer held by a {lo, hi} pair of uint64 (two's complement)."""
    v = (int(pair[1]) << 64) | int(pair[0])
    return v - (1 << 128) if v >> 127 else v


class EvalResult:
    """What `Evaluator.run` returns.  Every figure derives from the integer state (``state``: `_lib.EvalState` read back once).

    ``bits_per_dim`` / ``bits_per_dim_single`` / ``std_error`` (of bits_per_dim, over images) / ``count`` (images in the sums) /
    ``flagged`` (images left out: non-finite or out of range) / ``min`` / ``max`` / ``level_bits`` (list, None without levels) /
    ``histogram`` (dict: counts, under, over, lo, hi; None without one) / ``per_image`` (device tensor, NaN where flagged)."""

    def __init__(self, state, per_image, n_bits, levels):
        self.state, self.per_image = state, per_image
        st = state
        self.count, self.flagged = int(st.count), int(st.flagged)
        c = self.count
        nan = float("nan")
        mean = Fraction(_s128(st.sum_bpd), 1 << 32) / c if c else None
        self.bits_per_dim = float(mean) if c else nan
        self.bits_per_dim_single = float(Fraction(_s128(st.sum_single), 1 << 32) / c) if c else nan
        if c > 1:      # exact rational arithmetic on the integer sums: no cancellation in sum(b^2) - c mean^2
            var = (Fraction(_s128(st.sum_bpd2), 1 << 32) - c * mean * mean) / (c - 1)
            self.std_error = float(max(var, 0) / c) ** 0.5
        else:
            self.std_error = nan
        self.min = (int(st.min_key) - _TWO63) / 2.0 ** 32 if c else nan
        self.max = (int(st.max_key) - _TWO63) / 2.0 ** 32 if c else nan
        self.level_bits = None
        if levels:
            self.level_bits = [float(Fraction(_s128(st.sum_level[l]), 1 << 32) / c) if c else nan for l in range(int(st.n_levels))]
        self.n_bits = n_bits
        self.histogram = None
        if st.bins > 0:
            self.histogram = dict(counts=[int(v) for v in st.hist[:st.bins]], under=int(st.under), over=int(st.over),
                                  lo=float(st.lo), hi=float(st.hi))

    def state_bytes(self):
        """The raw state: equal bytes = equal evaluation."""
        return bytes(self.state)

    def quantile(self, q):
        """Bits/dim below which a fraction ``q`` of the counted images lies, read off the histogram (linear inside a bin; lo / hi
        when the quantile falls into the underflow / overflow counter)."""
        assert self.histogram is not None, "quantile needs a histogram (hist=(bins, lo, hi))"
        assert 0.0 <= q <= 1.0
        h = self.histogram
        total = h["under"] + sum(h["counts"]) + h["over"]
        if total == 0:
            return float("nan")
        want = q * total
        seen = h["under"]
        if want <= seen and seen > 0:
            return h["lo"]
        width = (h["hi"] - h["lo"]) / len(h["counts"])
        for i, cnt in enumerate(h["counts"]):
            if cnt and want <= seen + cnt:
                return h["lo"] + (i + (want - seen) / cnt) * width
            seen += cnt
        return h["hi"]

    def __repr__(self):
        return (f"EvalResult(bits_per_dim={self.bits_per_dim:.6f}, single={self.bits_per_dim_single:.6f}, "
                f"std_error={self.std_error:.2e}, count={self.count}, flagged={self.flagged})")


class EvalState:
    """The device-resident ``glowhip_eval_state`` and its two calls (glowhip_eval_reset / glowhip_eval_fold)."""

    def __init__(self, device, n_levels=0, hist=None):
        self.device = torch.device(device)
        self.buf = torch.empty(ctypes.sizeof(_lib.EvalState), dtype=torch.uint8, device=self.device)
        self.reset(n_levels, hist)

    def reset(self, n_levels=0, hist=None):
        bins, lo, hi = (0, 0.0, 1.0) if hist is None else hist
        check(lib().glowhip_eval_reset(ptr(self.buf), int(n_levels), int(bins), float(lo), float(hi), stream_ptr(self.device)))

    def fold(self, objective, terms, dims, per_image, offset=0, only_if_nan=None):
        """objective (K, N), terms (K, n_levels, N) or None -> the state and per_image[offset : offset + N].  One launch."""
        K, N = objective.shape
        assert objective.is_contiguous() and objective.dtype == torch.float32
        n_levels = 0
        if terms is not None:
            assert terms.is_contiguous() and terms.dtype == torch.float32 and terms.shape[0] == K and terms.shape[2] == N
            n_levels = terms.shape[1]
        assert per_image.is_contiguous() and per_image.dtype == torch.float32 and per_image.numel() >= offset + N
        assert only_if_nan is None or (only_if_nan.dtype == torch.float32 and only_if_nan.is_contiguous() and only_if_nan.numel() == N)
        check(lib().glowhip_eval_fold(ptr(self.buf), ptr(objective), ptr(terms), K, N, n_levels, float(dims), ptr(only_if_nan),
                                      ptr(per_image), int(offset), stream_ptr(self.device)))

    def read(self):
        """Host copy of the state (synchronises)."""
        return _lib.EvalState.from_buffer_copy(self.buf.cpu().numpy().tobytes())


def stream_seed(seed):
    """``seed`` with the rank folded in, as `model.dequant_position` keys the process's stream."""
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    return (int(seed) + 0x9E3779B97F4A7C15 * rank) & (2 ** 64 - 1)


def _unpack(batch):
    if isinstance(batch, dict):
        return batch["x"], batch.get("y_onehot")
    return batch, None


class Evaluator:
    """``Evaluator(glow, draws=1, levels=True, seed=0, hist=None, safe=True).run(batches)`` -> `EvalResult`.

    ``batches``: an iterable of tensors, or of dicts with ``x`` and optionally ``y_onehot``; fp32 in [0, 1] or uint8 pixels.
    Draw k of batch b is the dequantisation draw ``(seed', b * draws + k)``, seed' = ``seed`` with the rank folded in: the same
    (seed, data) gives the same bits again, and the process's own dequantisation position (`dequant_position`) is not consumed.
    ``hist``: ``(bins, lo, hi)`` of the histogram of per-image bits/dim (None: 64 bins over [0, 16); False: none).
    ``safe``: when images are flagged at the end, ``batches`` is iterated a second time and the batches that held them run on the
    exact-fp32 kernel family with the same draws; only the flagged images are folded again (each image is counted once)."""

    DEFAULT_HIST = (64, 0.0, 16.0)

    def __init__(self, glow, draws=1, levels=True, seed=0, hist=None, safe=True):
        assert int(draws) >= 1
        self.glow, self.draws, self.levels, self.seed, self.safe = glow, int(draws), bool(levels), int(seed), bool(safe)
        self.hist = None if hist is False else (self.DEFAULT_HIST if hist is None else tuple(hist))

    def _forward_draws(self, x, y_onehot, b, key):
        """K forwards of one batch: objective (K, N), terms (K, n_levels, N) or None, the plan."""
        glow = self.glow
        x = _lib.require_device_tensor(x, "Glow input", allow_uint8=True)
        n_bits = glow.hps.model.n_bits_x
        plan = glow.flow.plan_for(x)
        n = x.shape[0]
        head = plan.head_call(n, y_onehot) if glow._attach_head(plan) else None
        K = self.draws
        obj = torch.empty((K, n), dtype=torch.float32, device=x.device)
        terms = torch.empty((K, plan.n_levels, n), dtype=torch.float32, device=x.device) if self.levels else None
        z = torch.empty((n,) + plan.out_chw, dtype=torch.float32, device=x.device)
        nll = torch.empty(n, dtype=torch.float32, device=x.device)
        for k in range(K):
            plan.set_dequant_stream(key, b * K + k)
            plan.glow_forward(x, None, None, None, 0, n_bits, out=(z, nll, obj[k]), head=head,
                              level_terms=None if terms is None else terms[k])
        plan.set_dequant_rng(0, False)
        return obj, terms, plan

    @staticmethod
    def _grown(per_image, need):
        if per_image.numel() >= need:
            return per_image
        bigger = torch.full((max(need, 2 * per_image.numel()),), float("nan"), dtype=torch.float32, device=per_image.device)
        bigger[:per_image.numel()] = per_image
        return bigger

    def run(self, batches):
        glow = self.glow
        dev = glow.h_top.device
        assert dev.type == "cuda", "the evaluator runs on a HIP device (there is no CPU path)"
        # (the walk over every sub-module costs milliseconds at config B: skipped while the flow's own record of it is current)
        if getattr(glow.flow, "_actnorms_all_inited", None) != module.ActNorm.RESET_EPOCH[0]:
            assert glow.actnorm_inited(), "evaluate: the ActNorm layers hold no statistics yet (train or load a snapshot first)"
            glow.flow._actnorms_all_inited = module.ActNorm.RESET_EPOCH[0]
        was_training = glow.training
        key = stream_seed(self.seed)
        position = dequant_position()
        if was_training:
            glow.eval()
        try:
            with torch.no_grad():
                n_levels = glow.flow.plan_for(glow.flow.in_chw, dev).n_levels if self.levels else 0
                state = EvalState(dev, n_levels, self.hist)
                per_image = torch.full((1024,), float("nan"), dtype=torch.float32, device=dev)
                spans, total, dims = [], 0, None
                for b, batch in enumerate(batches):
                    x, y = _unpack(batch)
                    x = x.to(dev)
                    y = None if y is None else y.to(dev)
                    n = x.shape[0]
                    dims = x[0].numel()
                    obj, terms, _ = self._forward_draws(x, y, b, key)
                    per_image = self._grown(per_image, total + n)
                    state.fold(obj, terms, dims, per_image, total)
                    spans.append((total, n))
                    total += n
                st = state.read()      # the one host sync
                if self.safe and st.flagged > 0:
                    st = self._rerun(batches, spans, state, per_image, key, dims)
        finally:
            if was_training:
                glow.train()
        assert dequant_position() == position
        return EvalResult(st, per_image[:total], glow.hps.model.n_bits_x, self.levels)

    def _rerun(self, batches, spans, state, per_image, key, dims):
        """Second pass over the batches that held flagged images, on the exact-fp32 family, same draws."""
        assert iter(batches) is not batches, ("evaluate(safe=True): images were flagged and need a second pass over `batches`, which "
                                              "is a one-shot iterator -- pass a re-iterable (a list, a DataLoader) or safe=False")
        bad = torch.isnan(per_image).cpu()
        seen = 0
        for b, batch in enumerate(batches):
            assert b < len(spans), "evaluate(safe=True): the second pass over `batches` yielded more batches than the first"
            off, n = spans[b]
            seen += 1
            if not bool(bad[off:off + n].any()):
                continue
            x, y = _unpack(batch)
            dev = per_image.device
            x = x.to(dev)
            assert x.shape[0] == n, "evaluate(safe=True): `batches` must yield the same batches when iterated again"
            plan = self.glow.flow.plan_for(x)
            prev = plan.family
            plan.set_family(plan.FAMILY_EXACT_FP32)
            try:
                type(self.glow)._RANGE_FALLBACKS += 1
                obj, terms, _ = self._forward_draws(x, None if y is None else y.to(dev), b, key)
            finally:
                plan.set_family(prev)
            state.fold(obj, terms, dims, per_image, off, only_if_nan=per_image[off:off + n])
        assert seen == len(spans), "evaluate(safe=True): the second pass over `batches` yielded fewer batches than the first"
        return state.read()

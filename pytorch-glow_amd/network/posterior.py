"""Posterior sampling for inverse problems, on the device: a Metropolis-adjusted Langevin (MALA) chain over the latents.

`restore.LatentFit` gives the maximum-a-posteriori latents of a measurement; this gives draws from the posterior

    p(latents | measurement)  ~  exp(-U),     U = sum w (P decode(latents) - t)^2 / (2 noise_std^2)  +  1/2 ||latents||^2

-- what else is consistent with the measurement, and how sure the model is of each pixel.  One independent chain per sample of the
batch.  The latents are whitened by construction (the prior is N(0, I)), so the Langevin proposal needs no preconditioner.  The
definition of an iteration is in include/glowhip.h ("Posterior sampling") and, in numpy, tests/posterior_oracle.py; the kernels are
csrc/posterior.hip.  The pieces around them are the restoration path's: `FlowPlan.decode(out=)`, `restore_objective` with
``inv_wsum = 1 / (2 noise_std^2)`` and `FlowPlan.decode_vjp(out=)`.

The Metropolis test rejects a proposal whose decode is not finite, so a proposal outside the fp16 pairs' range of the product
kernels is refused on the device and never accepted as a wrong value: no exact-family re-run exists here."""
from dataclasses import dataclass
from typing import Optional

import torch

from .. import _lib
from .latents import Latents
from .restore import LatentLoop, check_prior_weight


@dataclass
class PosteriorInfo:
    """What a chain reports.  ``mean`` / ``std`` (N,C,H,W): the Welford moments of each chain's images over its ``count`` kept
    iterations (every ``thin``-th from ``burn_in`` on; std with the count - 1 divisor, zeros for count < 2); ``pooled_mean`` /
    ``pooled_std`` (C,H,W): the same over all chains together, combined by the parallel-variance formula -- meaningful when the
    chains share one measurement.  ``accept_rate`` (N,): accepted fraction of the iterations from ``burn_in`` on (of all of them
    when there are none); ``step_size`` (N,): the adapted steps; ``nonfinite_rejections`` (N,): proposals refused because their
    decode, loss or gradient was not finite; ``energy`` (steps, N): U after each iteration's decision; ``accepted`` and
    ``log_alpha`` (steps, N): the decisions and the log acceptance ratios.  ``finite``: the start state's own loss was finite --
    when False no iteration ran.  ``captured``: the iterations after the first ran as hipGraph replays; ``graph_error``: why a
    requested capture did not happen."""
    mean: torch.Tensor
    std: torch.Tensor
    count: int
    pooled_mean: torch.Tensor
    pooled_std: torch.Tensor
    accept_rate: torch.Tensor
    step_size: torch.Tensor
    nonfinite_rejections: torch.Tensor
    energy: torch.Tensor
    accepted: torch.Tensor
    log_alpha: torch.Tensor
    finite: bool
    captured: bool
    graph_error: Optional[str] = None


def kept_count(steps, burn_in, thin):
    """How many iterations 0 <= t < steps the moments fold: t >= burn_in and (t - burn_in) % thin == 0."""
    return 0 if steps <= burn_in else (steps - burn_in - 1) // thin + 1


class LatentMALA(LatentLoop):
    """The device-resident chain.  Owns the static buffers (target, weights, inv_wsum), two sets {current, proposal} of latent
    leaves, latent gradients and image, the per-sample loss and step, the device words (the stream position {seed, call} and the
    iteration), the histories and the image moments.

    The constructor evaluates the start state eagerly (decode, objective, decode_vjp: the current image, loss and gradient) and
    reads whether its loss is finite -- ``finite``; when it is not, `run` runs no iteration.  One iteration: glowhip_mala_propose;
    decode, objective and decode_vjp at the proposal; glowhip_mala_energy; glowhip_mala_select; glowhip_posterior_moments.
    `step_eager` enqueues that from Python; `capture` records it once as a hipGraph (after at least one eager iteration) and
    `step_captured` replays it: ONE graph launch and nothing else -- the iteration and the stream position live in device words
    the select launch advances, so nothing per step travels from the host.  Same kernels and same bits either way.  `run` is the
    whole chain with ONE host read at the end.  ``psf``: the measurement is the decode blurred by that point-spread function
    (`restore.LatentLoop`); both evaluations of an iteration share the loop's one residual buffer.  ``operator`` (M,C,H,W): the
    measurement (N, M) is the decode seen through that dense matrix, held by reference (`restore.LatentLoop`).  ``fourier=True``: the
    measurement is the decode's unitary 2-D DFT, complex (N,C,H,W), ``weight`` the k-space mask, and ``noise_std`` the standard
    deviation of each of the real and imaginary parts: the energy is sum w |F x - t|^2 / (2 noise_std^2).  ``coils=maps``: multi-coil
    k-space (`restore.LatentLoop`), the measurement complex (N,C,Q,H,W); ``noise_std`` is the standard deviation of each of the real and
    imaginary parts of each coil's coefficient, the energy sum_{c,q,k} w |F (S_q x) - t|^2 / (2 noise_std^2)."""

    def __init__(self, glow, measurement, weight=None, pool=1, noise_std=0.1, init=None, steps=100, burn_in=None, thin=1,
                 step_size=1e-3, adapt_rate=0.5, seed=0, graph=True, call=0, step_clamp=(1e-10, 1.0), psf=None, operator=None,
                 fourier=False, coils=None):
        check_prior_weight(glow, 1.0)
        burn_in = int(steps) // 2 if burn_in is None else int(burn_in)
        if init is None or steps < 1 or burn_in < 0 or thin < 1:
            raise ValueError("LatentMALA needs start latents (init), steps >= 1, burn_in >= 0 and thin >= 1")
        super().__init__(glow, measurement, weight, pool, init, steps, graph, psf=psf, operator=operator, fourier=fourier, coils=coils)
        self.burn_in, self.thin = burn_in, int(thin)
        self.noise_std, self.step_size, self.adapt_rate = float(noise_std), float(step_size), float(adapt_rate)
        self.step_min, self.step_max = (float(v) for v in step_clamp)
        self.seed, self.call = int(seed) & (2 ** 64 - 1), int(call)
        n, dev, plan = self.n, self.device, self.plan
        f32 = dict(dtype=torch.float32, device=dev)
        self.inv_wsum = torch.empty(n, **f32)      # 1 / (2 noise_std^2), written by glowhip_mala_init (`reset`)
        self.step = torch.empty(n, **f32)
        self.image_prop = torch.empty_like(self.image)
        self.loss = torch.zeros(n, **f32)
        self.loss_prop = torch.zeros(n, **f32)
        self.leaves = [t.clone() for t in self._start]
        self.leaves_prop = [torch.zeros_like(t) for t in self._start]
        self.grads = [torch.zeros_like(t) for t in self._start]
        self.grads_prop = [torch.zeros_like(t) for t in self._start]
        self.pos = plan.sampler_position(self.seed, self.call)
        self.iteration = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.counts = torch.zeros((2, n), dtype=torch.int32, device=dev)
        self.hist = torch.zeros((3, self.steps, n), **f32)
        self.mean = torch.zeros_like(self.image)
        self.m2 = torch.zeros_like(self.image)
        # the segment table: leaves, their gradients, the image (include/glowhip.h)
        pairs = list(zip(self.leaves, self.leaves_prop)) + list(zip(self.grads, self.grads_prop)) + [(self.image, self.image_prop)]
        self._n_leaves, self._n_segs = len(self.leaves), len(pairs)
        if self._n_segs > _lib.MALA_MAX_SEGS:
            raise _lib.GlowHipError(f"LatentMALA: {self._n_leaves} latent leaves need {self._n_segs} segments, the kernels take "
                                    f"{_lib.MALA_MAX_SEGS}")
        self._segs = (_lib.MalaSeg * self._n_segs)()
        for sg, (cur, prop) in zip(self._segs, pairs):
            sg.cur, sg.prop, sg.per = cur.data_ptr(), prop.data_ptr(), cur.numel() // n
        need = int(_lib.lib().glowhip_mala_scratch_bytes(self._segs, self._n_segs, self._n_leaves, n))
        if need == 0:
            _lib.check(-1)
        self.scratch = torch.zeros(need // 8, dtype=torch.float64, device=dev)
        self._reset_at = None        # the iteration count the last reset left: nothing to do again while it stands
        self.reset()
        self.finite = bool(torch.isfinite(self.loss).all())      # the start state's own loss (one read, before any iteration)

    # ------------------------------------------------------------------ the iteration
    def _body(self, captured=False):
        lib, check, ptr = _lib.lib(), _lib.check, _lib.ptr
        stream = _lib.stream_ptr(self.device)
        table = (self._segs, self._n_segs, self._n_leaves, self.n)
        nbytes = self.scratch.numel() * 8
        check(lib.glowhip_mala_propose(*table, ptr(self.step), ptr(self.pos), ptr(self.scratch), nbytes, stream))
        self._evaluate(self.leaves_prop, self.image_prop, self.loss_prop, self.grads_prop)
        check(lib.glowhip_mala_energy(*table, ptr(self.step), ptr(self.scratch), nbytes, stream))
        check(lib.glowhip_mala_select(*table, ptr(self.loss), ptr(self.loss_prop), ptr(self.step), ptr(self.pos), ptr(self.iteration),
                                      ptr(self.counts), ptr(self.hist), self.steps, self.burn_in, self.adapt_rate, self.step_min,
                                      self.step_max, ptr(self.ticket), ptr(self.scratch), nbytes, stream))
        # (the select launch advanced the iteration word: the iteration just decided is the word - 1)
        check(lib.glowhip_posterior_moments(ptr(self.image), ptr(self.mean), ptr(self.m2), ptr(self.iteration), -1, self.burn_in,
                                            self.thin, self.image.numel(), stream))

    # ------------------------------------------------------------------ the chain
    @torch.no_grad()
    def reset(self):
        """Back to the start: the start latents and their image, loss and gradient (evaluated eagerly), the initial step, the
        stream position (seed, call), iteration 0, empty histories, counters and moments.  Addresses stay: a capture stays valid."""
        if self._reset_at == self._iterations:
            return
        for p, s in zip(self.leaves, self._start):
            p.copy_(s)
        _lib.check(_lib.lib().glowhip_mala_init(_lib.ptr(self.step), _lib.ptr(self.inv_wsum), self.n, self.step_size, self.noise_std,
                                                _lib.stream_ptr(self.device)))
        self.pos.copy_(self.plan.sampler_position(self.seed, self.call))
        for t in (self.iteration, self.ticket, self.counts, self.hist, self.mean, self.m2, self.loss_prop):
            t.zero_()
        self._evaluate(self.leaves, self.image, self.loss, self.grads)
        self._reset_at = self._iterations

    def latents(self):
        """The current states (copies)."""
        return Latents(self.leaves[0].clone(), [e.clone() for e in self.leaves[1:]])

    def run(self):
        """The whole chain from the start state: `PosteriorInfo`; the final states are in `latents()`.  Nothing raises; one host
        read, at the end.  A start whose own loss is not finite runs no iteration (``finite=False``)."""
        self.reset()
        replayed = self._iterate() if self.finite else False
        n, steps = self.n, self.steps
        parts = [self.hist.reshape(-1), self.step, self.counts.view(torch.float32).reshape(-1), self.mean.reshape(-1), self.m2.reshape(-1)]
        flat = torch.cat(parts).cpu()      # the chain's one host read
        hist, step, counts, mean, m2 = torch.split(flat, [p.numel() for p in parts])
        hist = hist.view(3, steps, n)
        counts = counts.contiguous().view(torch.int32).view(2, n)
        count = kept_count(steps, self.burn_in, self.thin) if self.finite else 0
        mean, m2 = mean.view(self.image.shape), m2.view(self.image.shape).double()
        std = (m2 / (count - 1)).clamp(min=0.0).sqrt().float() if count > 1 else torch.zeros_like(mean)
        # all chains together: counts add, M2 = sum M2_n + count * sum (mean_n - pooled mean)^2
        pooled_mean = mean.double().mean(dim=0)
        pooled_m2 = m2.sum(dim=0) + count * ((mean.double() - pooled_mean) ** 2).sum(dim=0)
        pooled_std = (pooled_m2 / (n * count - 1)).clamp(min=0.0).sqrt().float() if n * count > 1 else torch.zeros_like(mean[0])
        accepted = hist[1]
        tail = accepted[self.burn_in:] if steps > self.burn_in else accepted
        return PosteriorInfo(mean=mean, std=std, count=count, pooled_mean=pooled_mean.float(), pooled_std=pooled_std,
                             accept_rate=tail.mean(dim=0), step_size=step.clone(), nonfinite_rejections=counts[1].clone(),
                             energy=hist[0], accepted=accepted > 0.5, log_alpha=hist[2], finite=self.finite, captured=replayed,
                             graph_error=self.graph_error)

"""GPU tests of posterior sampling (-m gpu): `network.posterior.LatentMALA` and `Inferer.posterior` -- the chain against the fp64
oracle chain on the CPU oracle's decode with the same draws (tests/posterior_oracle.py), eager against captured bit for bit, the
stationary distribution on an exactly solvable linear-Gaussian model, proposals out of the fp16 pairs' range, and the public call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pytorch_glow_amd.network import Inferer, LatentMALA, Latents, PosteriorInfo  # noqa: E402
from pytorch_glow_amd.network import model as gmodel  # noqa: E402

import decode_grad_oracle as D  # noqa: E402
import posterior_oracle as P  # noqa: E402
from test_gpu_decode_grad import DEV, dev, make_glow  # noqa: E402


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def latents_of(arrays):
    t = [dev(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))) for a in arrays]
    return Latents(t[0], t[1:])


# ------------------------------------------------------------------------------------------------ 1. the trajectory
def test_three_iterations_follow_the_oracle_chain():
    """`P.TRAJECTORY`: three adapting iterations of N = 2 chains on the 16x16 affine model (seeded non-zero Conv2dZeros), an
    in-painting mask, against the oracle chain through `O.flow_decode` in fp64 autograd with the same draws.  The oracle's margins
    |log alpha - log u| all exceed 1e-3 (asserted; seed from a CPU scan, the decisions are [[1, 1], [1, 1], [0, 1]]), so the device's
    decisions must be the oracle's.  The latents after iteration k stay within k times
        h (2e-4 max|g| + 1e-7) + 1e-5 sqrtf(2 h) + 4 ulp
    -- the project's gradient bar on the drift, the sampler's draw bar on the noise -- of the oracle's, per leaf tensor, with h and
    max|g| the oracle's at that iteration."""
    kw, case = P.TRAJECTORY, P.trajectory_case()
    chain, ref = case["chain"], case["ref"]
    margins = np.abs(chain["log_alpha"] - chain["log_u"])
    assert margins.min() > 1e-3 and case["relu_margin"] >= D.MIN_MARGIN
    assert chain["accepted"].any() and not chain["accepted"].all()
    glow = make_glow(ref)
    mala = LatentMALA(glow, dev(case["target"]), weight=dev(case["weight"]), noise_std=kw["sigma"], init=latents_of(case["start"]),
                      steps=kw["steps"], burn_in=kw["burn_in"], step_size=kw["step_size"], adapt_rate=kw["adapt_rate"], seed=kw["seed"],
                      graph=False)
    assert mala.finite
    allowed = [np.zeros(1) for _ in case["start"]]
    for k, tr in enumerate(chain["trace"]):
        mala.step_eager()
        acc = chain["accepted"][k]      # the oracle's state after this iteration: the proposal where accepted
        state = [np.where(acc.reshape((-1,) + (1,) * (p.ndim - 1)), p, t) for p, t in zip(tr["proposal"], tr["theta"])]
        h = tr["h"]
        for l, (got, want) in enumerate(zip(mala.leaves, state)):
            hl = h.reshape((-1,) + (1,) * (want.ndim - 1))
            gmax = np.abs(tr["g"][l]).max()
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            allowed[l] = allowed[l] + hl * (2e-4 * gmax + 1e-7) + 1e-5 * np.sqrt(2.0 * hl) + 4.0 * ulp
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            print(f"iteration {k} leaf {l}: worst multiple of the bound {float((err / allowed[l]).max()):.3f}")
            assert (err <= allowed[l]).all(), (k, l)
    info_hist = mala.hist.cpu().numpy()
    assert ((info_hist[1] > 0.5) == chain["accepted"]).all()


# ------------------------------------------------------------------------------------------------ 2. eager = captured
def tiny_setup(n=2):
    case = P.trajectory_case()
    glow = make_glow(case["ref"])
    return glow, dev(case["target"][:n]), dev(case["weight"][:n]), latents_of([a[:n] for a in case["start"]])


def test_eager_and_captured_chains_agree_bitwise_and_a_replay_uploads_nothing():
    glow, meas, weight, init = tiny_setup()
    args = dict(weight=weight, noise_std=0.2, init=init, steps=5, burn_in=3, thin=1, step_size=1e-3, seed=11)
    out = {}
    for name, graph in (("captured", True), ("eager", False)):
        mala = LatentMALA(glow, meas, graph=graph, **args)
        info = mala.run()
        assert isinstance(info, PosteriorInfo) and info.finite
        assert info.captured == graph, f"{name}: captured = {info.captured} ({info.graph_error})"
        out[name] = (mala.latents().tensors(), mala.hist.clone(), mala.step.clone(), mala.counts.clone(), mala.mean.clone(), mala.m2.clone(),
                     mala.image.clone())
        assert mala.iteration.tolist() == [5] and mala.pos.tolist() == [11, 5] and info.count == 2
    a, b = out["captured"], out["eager"]
    assert not same_bits(a[0][0], init.z), "no proposal was accepted in five iterations: nothing was compared"
    assert all(same_bits(x, y) for x, y in zip(a[0], b[0])), "latents differ"
    for k, what in enumerate(("histories", "steps", "counters", "mean", "M2", "image"), 1):
        assert same_bits(a[k], b[k]), f"{what} differ"
    # a replay: one graph launch, no upload, no sync
    mala = LatentMALA(glow, meas, graph=True, **dict(args, steps=8))
    mala.step_eager()
    assert mala.capture(), mala.graph_error
    mala.step_captured()                # (the first replay: whatever the runtime sets up lazily for a graph)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            mala.step_captured()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert mala.iteration.tolist() == [5] and mala.pos.tolist() == [11, 5]
    hist = mala.hist.cpu()
    assert float(hist[0, :5].abs().min()) > 0.0 and float(hist[:, 5:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 3. stationarity
@pytest.mark.parametrize("coup", ["additive", "affine"])
def test_stationary_distribution_on_the_linear_gaussian_model(coup):
    """`P.linear_case`: with every Conv2dZeros at zero the decode is x = A theta + b, so the posterior under a half-image mask and
    sigma = 0.5 is exactly N(mu, Lam^-1).  N = 256 independent chains of `P.STATIONARY_RUN` (fixed on the CPU by
    tests/test_posterior_host.py, where the unadjusted chain fails (ii)) from theta = 0; on the FINAL states, independent across
    chains: (i) every coordinate's mean within 5 sqrt(cov_ii / N) of mu_i; (ii) sum_n (theta_n - mu)^T Lam (theta_n - mu) within
    N D +- 5 sqrt(2 N D).  The post-burn-in acceptance of every chain lies in [0.3, 0.9] (the adaptation ran), and ``pooled_mean``
    is A mu + b within 5 standard errors of A Lam^-1 A^T / N (one effective draw per chain: loose, never tight)."""
    case, run, n = P.linear_case(coup), P.STATIONARY_RUN, P.STATIONARY["chains"]
    ref = dict(cfg=case["cfg"], sd=case["sd"])
    glow = make_glow(ref)
    as_batch = lambda a: dev(torch.from_numpy(a).float()).expand(n, *a.shape).contiguous()
    init = latents_of([np.zeros((n,) + s) for s in case["shapes"]])
    mala = LatentMALA(glow, as_batch(case["target"]), weight=as_batch(case["weight"]), noise_std=P.STATIONARY["sigma"], init=init,
                      steps=run["steps"], burn_in=run["burn_in"], step_size=run["step_size"], adapt_rate=run["adapt_rate"],
                      seed=run["seed"])
    info = mala.run()
    assert info.finite and info.captured, info.graph_error
    theta = [t.cpu().numpy().astype(np.float64) for t in mala.latents().tensors()]
    worst, q, centre, half = P.stationarity(theta, case)
    rate = info.accept_rate.numpy()
    print(f"{coup}: (i) worst multiple {worst:.3f}; (ii) {q:.0f} vs {centre:.0f} +- {half:.0f}; acceptance {rate.min():.2f} .. {rate.max():.2f}; "
          f"h {float(info.step_size.min()):.4f} .. {float(info.step_size.max()):.4f}; non-finite {int(info.nonfinite_rejections.sum())}")
    assert worst <= 1.0
    assert abs(q - centre) <= half
    assert 0.3 <= rate.min() and rate.max() <= 0.9
    assert info.count == run["steps"] - run["burn_in"] and tuple(info.energy.shape) == (run["steps"], n)
    A = case["A"]
    se = np.sqrt(np.einsum("pi,ij,pj->p", A, case["cov"], A) / n)
    pooled = info.pooled_mean.numpy().astype(np.float64).reshape(-1)
    dev_pooled = np.abs(pooled - (A @ case["mu"] + case["b"])) / (5.0 * se)
    print(f"{coup}: pooled mean, worst multiple of 5 standard errors {dev_pooled.max():.3f}")
    assert dev_pooled.max() <= 1.0
    assert bool((info.pooled_std > 0).all()) and bool((info.std >= 0).all())


# ------------------------------------------------------------------------------------------------ 4. range
def test_proposals_out_of_range_are_rejected_on_the_device_and_counted():
    """sigma = 0.01 and a first step of 1 from the in-painting start: the Langevin drift -h g (g ~ residual / sigma^2) throws the
    proposals to |theta'| ~ 1e4 (measured: 1.4e4), far beyond the fp16 pairs' range of the product kernels -- and beyond what this
    model decodes in any precision: the fp64 oracle's decode is already NaN at twice the start latents.  The chain ends; every
    rejection is counted as non-finite; the step shrinks; every state is finite; ``finite`` is True (the start itself decodes)."""
    glow, meas, weight, init = tiny_setup()
    mala = LatentMALA(glow, meas, weight=weight, noise_std=0.01, init=init, steps=6, burn_in=6, step_size=1.0, seed=5)
    info = mala.run()
    print("non-finite rejections", info.nonfinite_rejections.tolist(), "accepted", info.accepted.int().sum(dim=0).tolist(), "steps",
          info.step_size.tolist(), "log alpha", info.log_alpha[:, 0].tolist())
    assert info.finite is True
    assert all(bool(torch.isfinite(t).all()) for t in mala.latents().tensors())
    assert bool(torch.isfinite(mala.image).all()) and bool(torch.isfinite(mala.loss).all())
    assert bool((info.nonfinite_rejections > 0).all()) and not bool(info.accepted.any())
    assert all(same_bits(a, b) for a, b in zip(mala.latents().tensors(), init.tensors())), "a rejected proposal moved the state"
    assert bool((info.step_size < 1.0).all()), "a non-finite proposal must shrink the step"


def test_a_start_that_does_not_decode_runs_no_iteration():
    glow, meas, weight, init = tiny_setup()
    bad = Latents(init.z.clone(), [e.clone() for e in init.eps])
    bad.z[1, 0, 0, 0] = float("nan")
    mala = LatentMALA(glow, meas, weight=weight, noise_std=0.2, init=bad, steps=4, step_size=1e-3, seed=5)
    info = mala.run()
    assert info.finite is False and info.captured is False and info.count == 0
    assert mala.iteration.tolist() == [0] and mala.pos.tolist() == [5, 0]
    assert float(info.energy.abs().max()) == 0.0 and int(info.nonfinite_rejections.sum()) == 0
    assert all(same_bits(a, b) for a, b in zip(mala.latents().tensors(), bad.tensors()))


# ------------------------------------------------------------------------------------------------ 5. the public call
def test_inferer_posterior_chains_pool_and_seeds():
    case = P.trajectory_case()
    ref = case["ref"]
    glow = make_glow(ref)
    inf = Inferer(D.hps_for(ref["cfg"], ref["cfg"]["batch"]), glow, [DEV], DEV)
    image = dev(case["target"][0])                                # (3, 16, 16)
    low = F.avg_pool2d(image[None], 2)[0]                         # (3, 8, 8): the measurement of a super-resolution problem
    weight = torch.zeros_like(low)
    weight[..., :4] = 1.0
    kw = dict(weight=weight, pool=2, noise_std=0.2, chains=4, steps=6, burn_in=3, step_size=1e-3)
    lat, info = inf.posterior(low, seed=42, **kw)
    assert isinstance(lat, Latents) and isinstance(info, PosteriorInfo) and info.finite and info.captured, info.graph_error
    assert len(lat) == 4 and tuple(lat.z.shape) == (4, 24, 4, 4) and [tuple(e.shape) for e in lat.eps] == [(4, 6, 8, 8)]
    assert tuple(info.mean.shape) == (4, 3, 16, 16) == tuple(info.std.shape) and tuple(info.pooled_mean.shape) == (3, 16, 16)
    assert tuple(info.pooled_std.shape) == (3, 16, 16) and info.count == 3
    for t in (info.accept_rate, info.step_size, info.nonfinite_rejections):
        assert tuple(t.shape) == (4,)
    assert tuple(info.energy.shape) == (6, 4) and bool(torch.isfinite(info.energy).all())
    assert not same_bits(lat.z[0], lat.z[1]), "the chains of one measurement must draw differently"
    lat2, info2 = inf.posterior(low, seed=42, **kw)
    assert all(same_bits(a, b) for a, b in zip(lat.tensors(), lat2.tensors())) and same_bits(info.energy, info2.energy)
    assert same_bits(info.mean, info2.mean)
    torch.manual_seed(777)
    key, c0 = gmodel.sampler_position()
    lat3, _ = inf.posterior(low, **kw)
    assert gmodel.sampler_position() == (key, c0 + 1)
    lat4, _ = inf.posterior(low, **kw)
    assert gmodel.sampler_position() == (key, c0 + 2)
    assert not same_bits(lat3.z, lat4.z), "seed=None must draw afresh on a second call"
    # a batch of measurements runs one chain each; several chains on a batch are refused
    both = torch.stack([low, low.flip(-1)])
    lat5, info5 = inf.posterior(both, pool=2, noise_std=0.2, steps=3, burn_in=1, step_size=1e-3, seed=1)
    assert len(lat5) == 2 and tuple(info5.mean.shape) == (2, 3, 16, 16)
    with pytest.raises(ValueError, match="chains"):
        inf.posterior(both, pool=2, noise_std=0.2, chains=2, steps=3)

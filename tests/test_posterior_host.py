"""Host tests of posterior sampling (no GPU): the oracle chain of tests/posterior_oracle.py on the analytic linear-Gaussian target
-- which fixes the seed, length and step of the GPU stationarity test and shows that its bounds can see a missing Metropolis
correction --, the argument checks of the glowhip_mala_* / glowhip_posterior_moments entries that need no device, and the guard of
`Inferer.posterior` against a learned top prior."""
import ctypes

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network import Inferer, LatentMALA, PosteriorInfo

import decode_grad_oracle as D
import posterior_oracle as P

EINVAL = -1


# ------------------------------------------------------------------------------------------------ 1. the chain and its bounds
@pytest.mark.parametrize("coup", ["additive", "affine"])
def test_oracle_chain_is_stationary_and_the_bounds_see_a_missing_metropolis_correction(coup):
    """N = 256 chains of `P.STATIONARY_RUN` (the GPU test's seed, T, burn-in and start step) from theta = 0 on the exact target
    N(mu, Lam^-1): the final states pass (i) and (ii) and the post-burn-in acceptance lies in [0.3, 0.9].  The same chain with the
    accept test forced to "always", run at the SMALLEST step any adjusted chain adapted to (frozen: the most favourable step for
    it), fails (ii): the discretisation bias of the unadjusted chain, 1 / (1 - h lambda / 2) per direction, is what the Metropolis
    test removes, and the bound sees it."""
    case, run = P.linear_case(coup), P.STATIONARY_RUN
    assert case["dim"] == 192 and case["shapes"] == [(24, 2, 2), (6, 4, 4)]
    energy = P.linear_energy(case)
    start = [np.zeros((P.STATIONARY["chains"],) + s) for s in case["shapes"]]
    good = P.run_chain(energy, start, run["seed"], run["steps"], run["burn_in"], run["step_size"], run["adapt_rate"])
    worst, q, centre, half = P.stationarity(good["theta"], case)
    rate = good["accepted"][run["burn_in"]:].mean(axis=0)
    print(f"{coup}: (i) worst multiple {worst:.3f}; (ii) {q:.0f} vs {centre:.0f} +- {half:.0f}; acceptance {rate.min():.2f} .. {rate.max():.2f}; "
          f"h {good['h'].min():.4f} .. {good['h'].max():.4f}")
    assert worst <= 1.0
    assert abs(q - centre) <= half
    assert 0.3 <= rate.min() and rate.max() <= 0.9
    assert good["nonfinite"].sum() == 0
    h = float(good["h"].min())
    bad = P.run_chain(energy, start, run["seed"], run["steps"], 0, h, 0.0, always=True)
    assert bool(bad["accepted"].all()) and np.allclose(bad["h"], np.float32(h))
    _, q_bad, _, _ = P.stationarity(bad["theta"], case)
    print(f"{coup}: unadjusted at h = {h:.4f}: (ii) {q_bad:.0f} = centre {(q_bad - centre) / half:+.2f} half widths")
    assert abs(q_bad - centre) > half


def test_welford_restatement_is_the_two_pass_mean_and_m2():
    rs = np.random.RandomState(0)
    xs = rs.randn(7, 2, 3, 5)
    mean, m2 = P.welford(list(xs))
    assert np.allclose(mean, xs.mean(axis=0), rtol=0, atol=1e-14) and np.allclose(m2, ((xs - xs.mean(axis=0)) ** 2).sum(axis=0), atol=1e-13)


# ------------------------------------------------------------------------------------------------ 2. argument checks, no device call
def table(pers, n_leaves, base):
    """A segment table over fake addresses (nothing dereferences them: every call below is refused on the host)."""
    segs = (_lib.MalaSeg * max(len(pers), 1))()
    for i, per in enumerate(pers):
        segs[i].cur, segs[i].prop, segs[i].per = base + 4096 * i, base + 4096 * i + 2048, per
    return segs


def test_entries_are_exported_and_refuse_bad_arguments_without_a_device_call():
    lib = G.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    err = lambda: lib.glowhip_last_error()
    pers = [5, 48, 1027, 5, 48, 1027, 105]
    segs = table(pers, 3, base)
    # the scratch size is host arithmetic: 4 sums x N samples x B workgroups x 8 bytes, B = ceil(1080 / 256) = 5
    assert lib.glowhip_mala_scratch_bytes(segs, 7, 3, 3) == 4 * 3 * 5 * 8
    assert lib.glowhip_mala_scratch_bytes(segs, 7, 3, 0) == 0 and b"N = 0" in err()
    ok = dict(segs=segs, n_segs=7, n_leaves=3, N=3)

    def propose(**kw):
        a = dict(ok, **kw)
        return lib.glowhip_mala_propose(a["segs"], a["n_segs"], a["n_leaves"], a["N"], kw.get("step", base), kw.get("pos", base),
                                        kw.get("scratch", base), kw.get("nbytes", 480), None)

    def energy(**kw):
        a = dict(ok, **kw)
        return lib.glowhip_mala_energy(a["segs"], a["n_segs"], a["n_leaves"], a["N"], kw.get("step", base), kw.get("scratch", base),
                                       kw.get("nbytes", 480), None)

    def select(**kw):
        a = dict(ok, **kw)
        g = lambda k, d: kw.get(k, d)
        return lib.glowhip_mala_select(a["segs"], a["n_segs"], a["n_leaves"], a["N"], g("loss", base), base, base, g("pos", base), base, base,
                                       base, g("steps", 4), g("burn_in", 2), g("adapt_rate", 0.5), g("step_min", 1e-6), g("step_max", 1.0),
                                       g("ticket", base), base, g("nbytes", 480), None)

    for call in (propose, energy, select):
        assert call(n_leaves=121) == EINVAL and b"leaves" in err()                       # more than 120 leaves
        assert call(n_leaves=0) == EINVAL
        assert call(n_segs=33) == EINVAL and b"n_segs" in err()
        assert call(n_segs=5) == EINVAL                                                   # cannot hold 3 leaves and their gradients
        assert call(N=0) == EINVAL and b"N = 0" in err()
        assert call(segs=None) == EINVAL
        assert call(nbytes=479) == EINVAL and b"scratch" in err()
        bad = table(pers, 3, base)
        bad[1].prop = None
        assert call(segs=bad) == EINVAL and b"null" in err()
        bad = table(pers, 3, base)
        bad[2].cur = base + 2                                                             # not 4-byte aligned
        assert call(segs=bad) == EINVAL and b"aligned" in err()
        bad = table([5, 48, 1027, 5, 47, 1027, 105], 3, base)                             # a gradient that is not its leaf's size
        assert call(segs=bad) == EINVAL
        empty = table([0] * 7, 3, base)                                                   # per == 0: a NULL pointer is legal there ...
        empty[0].cur = None
        assert call(segs=empty, nbytes=0) == EINVAL and b"scratch" in err()               # ... and the next check is what refuses
    assert propose(step=None) == EINVAL and propose(pos=base + 4) == EINVAL and energy(step=base + 1) == EINVAL
    assert select(loss=None) == EINVAL and select(pos=None) == EINVAL and select(ticket=base + 2) == EINVAL
    assert select(steps=0) == EINVAL and select(burn_in=-1) == EINVAL
    for name in ("step_min", "step_max"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            assert select(**{name: v}) == EINVAL and b"clamp" in err(), (name, v)
    assert select(step_min=2.0, step_max=1.0) == EINVAL
    assert select(adapt_rate=float("nan")) == EINVAL and select(adapt_rate=-0.5) == EINVAL
    # the initial step and the noise level
    init = lambda step=0.01, sigma=0.5, n=3, h=base: lib.glowhip_mala_init(h, base, n, step, sigma, None)
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert init(step=v) == EINVAL and b"step" in err()
        assert init(sigma=v) == EINVAL and b"noise_std" in err()
    assert init(sigma=1e-30) == EINVAL                                                    # 1 / (2 sigma^2) is not an fp32 number
    assert init(n=0) == EINVAL and init(h=None) == EINVAL
    # the moments
    mom = lambda image=base, it=base, burn=0, thin=1, n=16: lib.glowhip_posterior_moments(image, base, base, it, 0, burn, thin, n, None)
    assert mom(thin=0) == EINVAL and mom(burn=-1) == EINVAL and mom(n=-1) == EINVAL
    assert mom(image=None) == EINVAL and mom(image=base + 2) == EINVAL and mom(it=None) == EINVAL and mom(it=base + 4) == EINVAL
    assert mom(n=0) == 0                                                                  # nothing to fold: no launch
    assert lib.glowhip_version() == 102


# ------------------------------------------------------------------------------------------------ 3. the guard
def test_posterior_raises_on_a_learned_top_prior():
    cfg = P.linear_case("affine")["cfg"]
    hps = D.hps_for(cfg, cfg["batch"])
    hps.ablation.learn_top = True
    glow = G.Glow(hps)
    inf = Inferer(hps, glow, ["cpu"], "cpu")
    with pytest.raises(ValueError, match="learn_top"):
        inf.posterior(torch.zeros(3, 8, 8), noise_std=0.5, steps=2)
    with pytest.raises(ValueError, match="learn_top"):
        LatentMALA(glow, torch.zeros(1, 3, 8, 8), init=None)
    assert PosteriorInfo.__dataclass_fields__.keys() >= {"mean", "std", "count", "pooled_mean", "pooled_std", "accept_rate", "step_size",
                                                         "nonfinite_rejections", "energy", "finite", "captured", "graph_error"}

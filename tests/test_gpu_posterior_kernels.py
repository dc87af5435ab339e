"""GPU tests of the posterior kernels (-m gpu), each entry on its own against tests/posterior_oracle.py: glowhip_mala_propose,
glowhip_mala_energy + glowhip_mala_select on crafted states, glowhip_posterior_moments.  Ragged sizes throughout: leaves of 5, 48
and 1027 elements per sample (1080 in all: five workgroups per sample, sample boundaries inside a Philox group of four), one
leaf 4 bytes off a 16-byte boundary."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib  # noqa: E402

import posterior_oracle as P  # noqa: E402

DEV = "cuda:0"
PERS = (5, 48, 1027)
IMAGE_PER = 3 * 5 * 7


def stream():
    return _lib.stream_ptr(torch.device(DEV))


def shifted(t):
    """A device copy of ``t`` that starts one float into a larger buffer: contiguous, 4 bytes past a 16-byte address."""
    n = t.numel()
    view = torch.zeros(n + 4, device=DEV)[1:1 + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


class Buffers:
    """Device pairs {current, proposal} for leaves of PERS elements per sample (leaf 1 off the 16-byte boundary), their gradients
    and -- ``image`` -- one more copied segment; the segment table and the scratch."""

    def __init__(self, n, image=False):
        self.n = n
        put = lambda i, a: (shifted if i == 1 else (lambda t: t.to(DEV)))(f32(a))
        zeros = lambda i, per: put(i, np.zeros((n, per)))
        self.theta = [zeros(i, p) for i, p in enumerate(PERS)]
        self.theta_p = [zeros(i, p) for i, p in enumerate(PERS)]
        self.g = [zeros(i, p) for i, p in enumerate(PERS)]
        self.g_p = [zeros(i, p) for i, p in enumerate(PERS)]
        pairs = list(zip(self.theta, self.theta_p)) + list(zip(self.g, self.g_p))
        if image:
            self.image, self.image_p = zeros(0, IMAGE_PER), zeros(0, IMAGE_PER)
            pairs.append((self.image, self.image_p))
        self.n_segs, self.n_leaves = len(pairs), len(PERS)
        self.segs = (_lib.MalaSeg * self.n_segs)()
        for sg, (cur, prop) in zip(self.segs, pairs):
            sg.cur, sg.prop, sg.per = cur.data_ptr(), prop.data_ptr(), cur.shape[1]
        nbytes = G.lib().glowhip_mala_scratch_bytes(self.segs, self.n_segs, self.n_leaves, n)
        self.blocks = nbytes // (4 * n * 8)
        assert self.blocks == 5 and nbytes == 4 * n * 5 * 8
        self.scratch = torch.zeros((4, n, self.blocks), dtype=torch.float64, device=DEV)
        self.table = (self.segs, self.n_segs, self.n_leaves, n)
        self.nbytes = nbytes

    def load(self, name, arrays):
        for dst, a in zip(getattr(self, name), arrays):
            dst.copy_(f32(a))


# ------------------------------------------------------------------------------------------------ 1. propose
def test_propose_vs_oracle_ragged_sizes_and_per_sample_steps():
    """theta' within 1e-5 sqrtf(2 h) (the sampler's draw bar, tests/test_gpu_sampler.py) + 2 ulp(max(|theta|, |h d|)) of the fp64
    oracle on every element, with steps 2^10 apart between the samples; a within 1e-5 relative; the same bits on a second run."""
    n, seed, call = 3, 77, 5
    rs = np.random.RandomState(0)
    theta = [rs.randn(n, p).astype(np.float32) for p in PERS]
    g = [(3.0 * rs.randn(n, p)).astype(np.float32) for p in PERS]
    h = np.array([2.0 ** -12, 2.0 ** -2, 2.0 ** -22], dtype=np.float32)
    buf = Buffers(n)
    buf.load("theta", theta)
    buf.load("g", g)
    step = f32(h).to(DEV)
    pos = torch.tensor([seed, call], dtype=torch.int64, device=DEV)

    def run():
        for t in buf.theta_p:
            t.fill_(float("nan"))
        buf.scratch.fill_(float("nan"))
        _lib.check(G.lib().glowhip_mala_propose(*buf.table, step.data_ptr(), pos.data_ptr(), buf.scratch.data_ptr(), buf.nbytes, stream()))
        return [t.clone() for t in buf.theta_p], buf.scratch.clone()

    got, scratch = run()
    xi = P.leaf_draws(seed, call, [(n, p) for p in PERS])
    ref = P.propose([t.astype(np.float64) for t in theta], [t.astype(np.float64) for t in g], h.astype(np.float64), xi)
    worst = 0.0
    for l, (a, r, t, gl) in enumerate(zip(got, ref, theta, g)):
        hd = np.abs(h.astype(np.float64)[:, None] * (gl.astype(np.float64) + t))
        ulp = np.spacing(np.maximum(np.abs(t), hd).astype(np.float32)).astype(np.float64)
        bound = 1e-5 * np.sqrt(2.0 * h.astype(np.float64))[:, None] + 2.0 * ulp
        err = np.abs(a.cpu().numpy().astype(np.float64) - r)
        worst = max(worst, float((err / bound).max()))
        assert np.isfinite(err).all()
    print(f"propose: worst multiple of the bound {worst:.3f}")
    assert worst <= 1.0
    a_ref = P.sums([x * x for x in xi])
    a_got = scratch[0].sum(dim=1).cpu().numpy()
    assert np.abs(a_got / a_ref - 1.0).max() <= 1e-5, (a_got, a_ref)
    assert bool(torch.isnan(scratch[1:]).all()), "propose wrote beyond its own partial sums"
    # every current buffer untouched, the pos word not advanced
    assert all(same_bits(d, f32(s).to(DEV)) for d, s in zip(buf.theta + buf.g, theta + g)) and pos.tolist() == [seed, call]
    again, scratch2 = run()
    assert all(same_bits(x, y) for x, y in zip(got, again)) and torch.equal(scratch[0].view(torch.int64), scratch2[0].view(torch.int64))


def test_propose_draws_are_the_samplers_bit_for_bit():
    """theta = g = 0 and h = 1/2 make theta' = (0 - 0) + sqrtf(1) xi = xi itself: every draw equals glowhip_normal_noise of the
    same (seed, call, stream 128 + leaf), element = flat index in the (N, per) leaf -- sample boundaries at 5 and 1027 elements fall
    inside a Philox group."""
    n, seed, call = 3, 123456789, (1 << 33) + 7
    buf = Buffers(n)
    step = torch.full((n,), 0.5, device=DEV)
    pos = torch.tensor([seed, call], dtype=torch.int64, device=DEV)
    _lib.check(G.lib().glowhip_mala_propose(*buf.table, step.data_ptr(), pos.data_ptr(), buf.scratch.data_ptr(), buf.nbytes, stream()))
    for l, per in enumerate(PERS):
        noise = torch.empty((n, per), device=DEV)
        _lib.check(G.lib().glowhip_normal_noise(noise.data_ptr(), noise.numel(), seed, call, 128 + l, 1.0, stream()))
        assert same_bits(buf.theta_p[l], noise), f"leaf {l}"
        assert float(noise.abs().max()) > 1.0


# ------------------------------------------------------------------------------------------------ 2. energy + select
SELECT_SEED = 1      # (CPU scan of `select_case`: smallest |log alpha - log u| 0.067 / 0.062 at the two calls used; 22 / 23 accepted)
BAD_L, BAD_THETA, BAD_G = 5, 17, 40      # the samples with L' = NaN, one inf in theta', one NaN in g'


def select_case(seed, n=64, blocks=5):
    """Crafted fp32 states and the oracle's verdict on them.  theta' is a Langevin proposal from (theta, g) with noise xi, a the
    sum xi^2 spread over the workgroup slots, g' a perturbed g, L and L' uniform -- log alpha is O(1), both decisions occur."""
    rs = np.random.RandomState(seed)
    h = (0.01 * 2.0 ** rs.uniform(-1, 1, n)).astype(np.float32)
    theta = [rs.randn(n, p).astype(np.float32) for p in PERS]
    g = [(0.3 * rs.randn(n, p)).astype(np.float32) for p in PERS]
    xi = [rs.randn(n, p) for p in PERS]
    theta_p = [np.float32(t - h[:, None] * (gl + t) + np.sqrt(2.0 * h)[:, None] * x) for t, gl, x in zip(theta, g, xi)]
    g_p = [np.float32(gl + 0.05 * rs.randn(*gl.shape)) for gl in g]
    share = rs.dirichlet(np.ones(blocks), n)
    a_slots = P.sums([x * x for x in xi])[:, None] * share                      # (n, blocks) fp64
    L = rs.uniform(0.0, 40.0, n).astype(np.float32)
    Lp = np.float32(L + rs.uniform(-3.0, 3.0, n))
    image, image_p = rs.rand(n, IMAGE_PER).astype(np.float32), rs.rand(n, IMAGE_PER).astype(np.float32)
    Lp[BAD_L] = np.nan
    theta_p[2][BAD_THETA, 1000] = np.inf
    g_p[1][BAD_G, 7] = np.nan
    a = np.zeros(n)
    for b in range(blocks):
        a = a + a_slots[:, b]                                                   # the kernel's order
    d64 = lambda arrs: [x.astype(np.float64) for x in arrs]
    with np.errstate(all="ignore"):      # (the three non-finite samples)
        _, bb, p, pp = P.terms(d64(theta), d64(theta_p), d64(g_p), h.astype(np.float64), xi)
    return dict(n=n, h=h, theta=theta, g=g, theta_p=theta_p, g_p=g_p, a_slots=a_slots, L=L, Lp=Lp, image=image, image_p=image_p,
                a=a, b=bb, p=p, pp=pp)


def verdict(case, seed, call):
    u = P.accept_uniforms(seed, call, case["n"])
    log_alpha, accept, nonfinite = P.decide(case["L"].astype(np.float64), case["Lp"].astype(np.float64), case["a"], case["b"], case["p"],
                                            case["pp"], case["h"].astype(np.float64), u)
    return log_alpha, accept, nonfinite, np.log(u)


@pytest.mark.parametrize("iteration,burn_in", [(2, 5), (7, 5)], ids=["adapting", "frozen"])
def test_energy_and_select_vs_oracle(iteration, burn_in):
    """Every decision equals the oracle's (its margins |log alpha - log u| all exceed 1e-3: asserted); accepted samples: current ==
    proposal bit for bit in leaves, gradients and image; rejected samples: current unchanged bit for bit; the three samples with a
    NaN L', an inf in theta' and a NaN in g' are rejected, their non-finite counters read 1 and their step shrinks as for acceptance
    probability 0; the new steps are the oracle's to 1e-6 relative (unchanged bits from burn_in on); the position and iteration
    words move by exactly 1; the history row ``iteration`` is written and no other."""
    seed, steps, rate, h_min, h_max = 99, 10, 0.5, 1e-6, 1.0
    call = 1000 + iteration
    case = select_case(SELECT_SEED)
    n = case["n"]
    log_alpha, accept, nonfinite, log_u = verdict(case, seed, call)
    finite = ~nonfinite
    margin = np.abs(log_alpha - log_u)[finite].min()
    print(f"select: {int(accept.sum())} of {n} accepted, smallest margin {margin:.2e}")
    assert margin > 1e-3 and 10 <= accept.sum() <= n - 10
    assert nonfinite.sum() == 3 and nonfinite[[BAD_L, BAD_THETA, BAD_G]].all() and not accept[nonfinite].any()
    buf = Buffers(n, image=True)
    for name in ("theta", "theta_p", "g", "g_p"):
        buf.load(name, case[name])
    buf.image.copy_(f32(case["image"]))
    buf.image_p.copy_(f32(case["image_p"]))
    buf.scratch.fill_(float("nan"))
    buf.scratch[0].copy_(torch.from_numpy(case["a_slots"]))
    step, loss, loss_p = f32(case["h"]).to(DEV), f32(case["L"]).to(DEV), f32(case["Lp"]).to(DEV)
    pos = torch.tensor([seed, call], dtype=torch.int64, device=DEV)
    it = torch.tensor([iteration], dtype=torch.int64, device=DEV)
    counts = torch.zeros((2, n), dtype=torch.int32, device=DEV)
    hist = torch.full((3, steps, n), -7.0, device=DEV)
    ticket = torch.full((1,), 12345, dtype=torch.int32, device=DEV)      # (the call zeroes it itself)
    lib = G.lib()
    _lib.check(lib.glowhip_mala_energy(*buf.table, step.data_ptr(), buf.scratch.data_ptr(), buf.nbytes, stream()))
    sums = buf.scratch.sum(dim=2).cpu().numpy()      # (the slots hold fp64 sums; any order of five agrees far inside the bars)
    ok = finite
    for q, name in ((1, "b"), (2, "p"), (3, "pp")):
        rel = np.abs(sums[q][ok] / case[name][ok] - 1.0).max()
        print(f"energy: {name} worst relative error {rel:.2e}")
        assert rel <= 1e-12, name
    assert np.isnan(sums[1][BAD_G]) and np.isinf(sums[3][BAD_THETA])
    before = {k: [t.clone() for t in getattr(buf, k)] for k in ("theta", "g")}
    _lib.check(lib.glowhip_mala_select(*buf.table, loss.data_ptr(), loss_p.data_ptr(), step.data_ptr(), pos.data_ptr(), it.data_ptr(),
                                       counts.data_ptr(), hist.data_ptr(), steps, burn_in, rate, h_min, h_max, ticket.data_ptr(),
                                       buf.scratch.data_ptr(), buf.nbytes, stream()))
    hist_h = hist.cpu().numpy()
    got_accept = hist_h[1, iteration] > 0.5
    assert (got_accept == accept).all(), np.nonzero(got_accept != accept)
    acc, rej = torch.from_numpy(accept).to(DEV), torch.from_numpy(~accept).to(DEV)
    for cur, prop, old in zip(buf.theta + buf.g + [buf.image], buf.theta_p + buf.g_p + [buf.image_p],
                              before["theta"] + before["g"] + [f32(case["image"]).to(DEV)]):
        assert same_bits(cur[acc], prop[acc]), "an accepted sample is not its proposal"
        assert same_bits(cur[rej], old[rej]), "a rejected sample was written"
    assert same_bits(loss, torch.where(acc, loss_p, f32(case["L"]).to(DEV)))
    assert counts.cpu().numpy().tolist() == [accept.astype(int).tolist(), nonfinite.astype(int).tolist()]
    assert pos.tolist() == [seed, call + 1] and it.tolist() == [iteration + 1]
    h_got = step.cpu().numpy()
    if iteration < burn_in:
        h_ref = P.adapt(case["h"].astype(np.float64), log_alpha, nonfinite, iteration, rate, h_min, h_max)
        assert np.abs(h_got / h_ref - 1.0).max() <= 1e-6
        shrink = np.exp(rate / np.sqrt(iteration + 1.0) * (0.0 - 0.574))
        assert np.abs(h_got[nonfinite] / (case["h"][nonfinite].astype(np.float64) * shrink) - 1.0).max() <= 1e-6
    else:
        assert same_bits(step, f32(case["h"]).to(DEV)), "the step moved after burn-in"
    # the history: row `iteration` and no other
    other = np.delete(hist_h, iteration, axis=1)
    assert (other == -7.0).all()
    assert np.abs(hist_h[2, iteration][finite] - log_alpha[finite]).max() <= 1e-5 * np.abs(log_alpha[finite]).max()
    energy_ref = np.where(accept, case["Lp"].astype(np.float64), case["L"]) + 0.5 * np.where(accept, case["pp"], case["p"])
    assert np.abs(hist_h[0, iteration] / energy_ref - 1.0).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ 3. moments
def test_moments_five_folds_vs_numpy_welford_and_the_gate():
    """burn_in 3, thin 2, the word one ahead of the iteration (offset -1, as behind a select): iterations 3, 5, 7, 9 and 11 fold --
    mean to 1e-6 and M2 to 1e-5 relative to the largest entry of the oracle's --, iterations 0 .. 2, 4, 6, 8 and 10 leave every byte
    of mean and M2 as it was.  The buffers start as NaN: fold 1 starts the moments whatever they held."""
    rs = np.random.RandomState(3)
    shape, burn_in, thin = (2, 3, 5, 7), 3, 2
    images = [rs.rand(*shape).astype(np.float32) + t for t in range(12)]
    x = torch.empty(shape, device=DEV)
    mean, m2 = torch.full(shape, float("nan"), device=DEV), torch.full(shape, float("nan"), device=DEV)
    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    folded = []
    for t in range(12):
        x.copy_(f32(images[t]))
        word.fill_(t + 1)
        before = (mean.clone(), m2.clone())
        _lib.check(G.lib().glowhip_posterior_moments(x.data_ptr(), mean.data_ptr(), m2.data_ptr(), word.data_ptr(), -1, burn_in, thin,
                                                     x.numel(), stream()))
        if t >= burn_in and (t - burn_in) % thin == 0:
            folded.append(images[t])
            assert not same_bits(mean, before[0])
        else:
            assert same_bits(mean, before[0]) and same_bits(m2, before[1]), f"iteration {t} is gated off"
    assert len(folded) == 5
    mean_ref, m2_ref = P.welford(folded)
    e_mean = np.abs(mean.cpu().numpy() - mean_ref).max() / np.abs(mean_ref).max()
    e_m2 = np.abs(m2.cpu().numpy() - m2_ref).max() / np.abs(m2_ref).max()
    print(f"moments: mean {e_mean:.2e}, M2 {e_m2:.2e}")
    assert e_mean <= 1e-6 and e_m2 <= 1e-5

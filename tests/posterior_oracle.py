"""numpy restatement of the posterior chain (include/glowhip.h "Posterior sampling", csrc/posterior.hip), fp64 throughout.  Written
from the definition, independent of the HIP code; its draws are tests/sampler_oracle.py's.

Per sample n, theta = all latent leaves of that sample (leaf 0 = z, leaf 1 + k = eps[k] in decode order), as a LIST of (N, ...) arrays:
    U(theta) = L(theta) + 1/2 ||theta||^2          grad U = g + theta,   (L, g) = energy_and_grad(theta)   -- pluggable
    proposal   d = g + theta;  theta' = (theta - h d) + sqrt(2 h) xi,  xi = N(0, 1) at (seed, call, stream 128 + leaf, flat element)
    a = sum xi^2;  d' = g' + theta';  b = sum (theta - theta' + h d')^2;  p = sum theta^2;  p' = sum theta'^2
    log alpha = (L - L') + 1/2 (p - p') + 1/2 a - b / (4 h)
    accept iff L', b, p' finite and log(u) < log alpha,  u = ((w0 >> 8) + 0.5) 2^-24, w0 = word 0 of group n of stream 254
    while iteration < burn_in:  h <- clamp(h exp(adapt_rate / sqrt(iteration + 1) (min(1, e^{log alpha}) - 0.574)), h_min, h_max),
                                a non-finite proposal counting as probability 0
    moments    Welford over the CURRENT image at iterations t >= burn_in with (t - burn_in) % thin == 0
The chain runs on anything that supplies ``energy_and_grad``: the analytic linear-Gaussian model below, or the CPU oracle's decode
through fp64 autograd (`decode_energy`)."""
import functools

import numpy as np
import torch

import sampler_oracle as S

LEAF_STREAM, ACCEPT_STREAM, TARGET_ACCEPT = 128, 254, 0.574


def leaf_draws(seed, call, shapes):
    """xi of every leaf: stream 128 + leaf, element = flat index in the contiguous (N, ...) leaf."""
    return [S.normal(int(np.prod(s)), seed, call, LEAF_STREAM + l).reshape(s) for l, s in enumerate(shapes)]


def accept_uniforms(seed, call, n):
    """u of samples 0 .. n - 1: word 0 of group n of stream 254."""
    w0 = S.words(4 * n, seed, call, ACCEPT_STREAM)[:n, 0]
    return ((w0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def per_sample(h, leaf):
    return np.asarray(h, dtype=np.float64).reshape((-1,) + (1,) * (leaf.ndim - 1))


def sums(leaves):
    """Per-sample sum over every leaf."""
    return sum(t.reshape(t.shape[0], -1).sum(axis=1) for t in leaves)


def propose(theta, g, h, xi):
    return [(t - per_sample(h, t) * (gl + t)) + np.sqrt(2.0 * per_sample(h, t)) * x for t, gl, x in zip(theta, g, xi)]


def terms(theta, theta_p, g_p, h, xi):
    """(a, b, p, p') per sample."""
    a = sums([x * x for x in xi])
    b = sums([((t - tp) + per_sample(h, t) * (gp + tp)) ** 2 for t, tp, gp in zip(theta, theta_p, g_p)])
    return a, b, sums([t * t for t in theta]), sums([tp * tp for tp in theta_p])


def decide(L, Lp, a, b, p, pp, h, u, always=False):
    """(log alpha, accept, nonfinite) per sample.  ``always``: the accept test forced to yes for every finite proposal -- the
    unadjusted chain, which the stationarity bounds must be able to tell apart."""
    with np.errstate(all="ignore"):
        log_alpha = (L - Lp) + 0.5 * (p - pp) + 0.5 * a - b / (4.0 * h)
        nonfinite = ~(np.isfinite(Lp) & np.isfinite(b) & np.isfinite(pp))
        accept = ~nonfinite & (np.full_like(log_alpha, True, dtype=bool) if always else (np.log(u) < log_alpha))
    return log_alpha, accept, nonfinite


def adapt(h, log_alpha, nonfinite, iteration, adapt_rate, h_min, h_max):
    with np.errstate(all="ignore"):
        prob = np.where(nonfinite | np.isnan(log_alpha), 0.0, np.minimum(1.0, np.exp(np.minimum(log_alpha, 0.0))))
    return np.clip(h * np.exp(adapt_rate / np.sqrt(iteration + 1.0) * (prob - TARGET_ACCEPT)), h_min, h_max)


def run_chain(energy_and_grad, theta0, seed, steps, burn_in, step_size, adapt_rate=0.5, h_min=1e-10, h_max=1.0, call=0, always=False,
              record=False):
    """The chain.  Returns a dict: ``theta`` (final leaves), ``h``, ``accepted`` / ``log_alpha`` / ``log_u`` / ``energy`` (steps, N),
    ``nonfinite`` (N,), and with ``record`` the leaves, the proposals and the steps of every iteration (``trace``)."""
    theta = [np.array(t, dtype=np.float64) for t in theta0]
    n = theta[0].shape[0]
    shapes = [t.shape for t in theta]
    h = np.full(n, float(np.float32(step_size)), dtype=np.float64)
    L, g = energy_and_grad(theta)
    out = dict(accepted=[], log_alpha=[], log_u=[], energy=[], trace=[], nonfinite=np.zeros(n, dtype=np.int64))
    for it in range(steps):
        xi = leaf_draws(seed, call + it, shapes)
        u = accept_uniforms(seed, call + it, n)
        theta_p = propose(theta, g, h, xi)
        Lp, gp = energy_and_grad(theta_p)
        a, b, p, pp = terms(theta, theta_p, gp, h, xi)
        log_alpha, accept, nonfinite = decide(L, Lp, a, b, p, pp, h, u, always)
        if record:
            out["trace"].append(dict(theta=[t.copy() for t in theta], g=[t.copy() for t in g], proposal=theta_p, h=h.copy()))
        for cur, new in list(zip(theta, theta_p)) + list(zip(g, gp)):
            cur[accept] = new[accept]
        L = np.where(accept, Lp, L)
        out["nonfinite"] += nonfinite
        if it < burn_in:
            h = adapt(h, log_alpha, nonfinite, it, adapt_rate, h_min, h_max)
        out["accepted"].append(accept)
        out["log_alpha"].append(log_alpha)
        out["log_u"].append(np.log(u))
        out["energy"].append(L + 0.5 * np.where(accept, pp, p))
    for k in ("accepted", "log_alpha", "log_u", "energy"):
        out[k] = np.stack(out[k])
    out.update(theta=theta, h=h, L=L)
    return out


def welford(images):
    """(mean, M2) after folding ``images`` (a sequence of arrays) one by one."""
    mean, m2 = np.zeros_like(np.asarray(images[0], dtype=np.float64)), None
    m2 = np.zeros_like(mean)
    for c, x in enumerate(images, 1):
        delta = np.asarray(x, dtype=np.float64) - mean
        mean = mean + delta / c
        m2 = m2 + delta * (x - mean)
    return mean, m2


# --------------------------------------------------------------------------------------------------------------------------
# The CPU oracle's decode as the energy: L = sum w (P decode(theta) - t)^2 / (2 sigma^2) and its latent gradient by fp64 autograd
def decode_energy(sd, cfg, target, weight, noise_std, pool=1, tables=None):
    """energy_and_grad(theta) over `O.flow_decode`; also returns the images of the last call in ``.image``."""
    import restore_oracle as R
    n = target.shape[0]
    inv = torch.full((n,), 1.0 / (2.0 * float(noise_std) ** 2), dtype=torch.float64)

    def energy_and_grad(theta):
        x, loss, gz, geps = R.latent_grads(torch.from_numpy(theta[0]), [torch.from_numpy(e) for e in theta[1:]], sd, cfg, target, weight,
                                           inv, pool, tables)
        energy_and_grad.image = x.numpy()
        return loss.numpy().copy(), [gz.numpy().copy()] + [e.numpy().copy() for e in geps]
    return energy_and_grad


# --------------------------------------------------------------------------------------------------------------------------
# The analytic linear-Gaussian target of the stationarity tests: a fresh 3x8x8 model, L = 2, K = 2, every Conv2dZeros at zero, so
# the decode is affine in the latents, x = A theta + b (additive: the coupling adds 0; affine: it divides by sigmoid(2)), with
# ActNorm bias / logs from a seeded batch and perturbed orthogonal invconv weights.  D = 192: z (24,2,2) and eps[0] (6,4,4).
STATIONARY = dict(image=8, hidden=32, K=2, L=2, zeros_std=0.0, sigma=0.5, chains=256)
# fixed by tests/test_posterior_host.py on the CPU (the oracle chain passes both bounds, the unadjusted chain fails (ii)):
STATIONARY_RUN = dict(seed=2024, steps=400, burn_in=200, step_size=0.05, adapt_rate=0.5)


@functools.lru_cache(maxsize=None)
def linear_case(coup):
    """dict(cfg, sd, shapes, A (192 pixels x 192 latents), b, target, weight, mu, Lam, cov) of the stationarity model under coupling
    ``coup``; the target is the decode of seeded latents, the weight the left half of the image."""
    import decode_grad_oracle as D
    from oracle import glow_oracle as O
    kw = STATIONARY
    cfg, sd, z, eps, _ = D.build_case(kw["image"], kw["hidden"], kw["K"], kw["L"], batch=8, seed={"additive": 301, "affine": 302}[coup],
                                      zeros_std=kw["zeros_std"], coup=coup)
    sd64 = {k: v.double() for k, v in sd.items()}
    shapes = [tuple(z.shape[1:])] + [tuple(e.shape[1:]) for e in eps]
    sizes = [int(np.prod(s)) for s in shapes]
    dim = sum(sizes)
    basis = torch.cat([torch.zeros(1, dim, dtype=torch.float64), torch.eye(dim, dtype=torch.float64)])
    parts = torch.split(basis, sizes, dim=1)
    with torch.no_grad():
        x = O.flow_decode(parts[0].reshape((-1,) + shapes[0]), sd64, cfg, [p.reshape((-1,) + s) for p, s in zip(parts[1:], shapes[1:])])
        x = x.reshape(dim + 1, -1).numpy()
    b = x[0]
    A = (x[1:] - b).T                                   # pixels x latents
    rs = np.random.RandomState(7)
    target = A @ rs.randn(dim) + b
    image_shape = (3, kw["image"], kw["image"])
    weight = np.zeros(image_shape)
    weight[..., : kw["image"] // 2] = 1.0
    w = weight.reshape(-1)
    s2 = kw["sigma"] ** 2
    Lam = np.eye(dim) + A.T @ (w[:, None] * A) / s2
    cov = np.linalg.inv(Lam)
    mu = cov @ (A.T @ (w * (target - b))) / s2
    return dict(cfg=cfg, sd=sd, shapes=shapes, sizes=sizes, A=A, b=b, target=target.reshape(image_shape), weight=weight, mu=mu, Lam=Lam,
                cov=cov, dim=dim)


def linear_energy(case):
    """energy_and_grad of the analytic model: L = sum w (A theta + b - t)^2 / (2 sigma^2), g = A^T w (A theta + b - t) / sigma^2."""
    A, b, t, w = case["A"], case["b"], case["target"].reshape(-1), case["weight"].reshape(-1)
    s2, sizes = STATIONARY["sigma"] ** 2, case["sizes"]

    def energy_and_grad(theta):
        flat = np.concatenate([l.reshape(l.shape[0], -1) for l in theta], axis=1)
        r = flat @ A.T + b - t
        L = (w * r * r).sum(axis=1) / (2.0 * s2)
        g = (w * r) @ A / s2
        return L, [p.reshape(l.shape).copy() for p, l in zip(np.split(g, np.cumsum(sizes)[:-1], axis=1), theta)]
    return energy_and_grad


def flatten(theta):
    return np.concatenate([np.asarray(l, dtype=np.float64).reshape(l.shape[0], -1) for l in theta], axis=1)


def stationarity(theta, case):
    """The two bounds on the final states of N independent chains, both from the target N(mu, Lam^-1) alone:
    (i) every coordinate |mean_n theta_i - mu_i| <= 5 sqrt(cov_ii / N); (ii) sum_n (theta_n - mu)^T Lam (theta_n - mu) within
    N D +- 5 sqrt(2 N D).  Returns (worst multiple of (i)'s bound, the quadratic form, its centre, its half width)."""
    flat = flatten(theta)
    n, dim = flat.shape
    dev = flat - case["mu"]
    worst = float((np.abs(dev.mean(axis=0)) / (5.0 * np.sqrt(np.diag(case["cov"]) / n))).max())
    q = float(np.einsum("ni,ij,nj->", dev, case["Lam"], dev))
    return worst, q, float(n * dim), 5.0 * float(np.sqrt(2.0 * n * dim))


# --------------------------------------------------------------------------------------------------------------------------
# The trajectory case of tests/test_gpu_posterior.py: the 16x16 / hidden 32 affine model of tests/restore_oracle.py (seeded non-zero
# Conv2dZeros), its first two samples, the left half of the image as the in-painting mask, the start the encode of the blanked image.
# Seed 1 (CPU scan): decisions [[1, 1], [1, 1], [0, 1]], smallest |log alpha - log u| 0.29, smallest ReLU margin of any evaluated
# point above decode_grad_oracle.MIN_MARGIN.
TRAJECTORY = dict(n=2, sigma=0.2, seed=1, steps=3, burn_in=3, step_size=1e-3, adapt_rate=0.5)


@functools.lru_cache(maxsize=None)
def trajectory_case():
    """dict(ref, target, weight, start (fp32 leaves), chain (the recorded oracle chain), relu_margin)."""
    import decode_grad_oracle as D
    import restore_oracle as R
    kw = TRAJECTORY
    ref = D.reference(**R.TINY_AFF)
    target = ref["x"][:kw["n"]].float()
    weight = torch.zeros_like(target)
    weight[..., : target.shape[-1] // 2] = 1.0
    blank = 1.0 - weight
    with torch.no_grad():
        z0, eps0 = D.encode_latents(target * blank, ref["sd"], ref["cfg"], ref["tables"])
    start = [z0.numpy()] + [e.numpy() for e in eps0]
    energy = decode_energy(ref["sd"], ref["cfg"], target, weight, kw["sigma"], tables=ref["tables"])
    chain = run_chain(energy, start, kw["seed"], kw["steps"], kw["burn_in"], kw["step_size"], kw["adapt_rate"], record=True)
    sd64 = {k: v.double() for k, v in ref["sd"].items()}
    points = [start] + [tr["proposal"] for tr in chain["trace"]]
    margin = min(D.decode_margin(torch.from_numpy(p[0]).double(), [torch.from_numpy(e).double() for e in p[1:]], sd64, ref["cfg"],
                                 ref["tables"]) for p in points)
    return dict(ref=ref, target=target, weight=weight, start=start, chain=chain, relu_margin=margin)

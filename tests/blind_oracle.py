"""fp64 restatement of blind deblurring (csrc/restore_blind.hip; the definition is in include/glowhip.h) on top of
tests/deblur_oracle.py: the gradient of the data term with respect to the taps of the PSF -- by autograd of `deblur_oracle._terms`
and as the explicit correlation --, the softmax and its backward, the bound the device's results are held to, the case tables of
tests/test_blind_host.py and tests/test_gpu_blind.py, and the two fits (calibration, and the joint blind fit through the CPU
oracle's decode).  Nothing here reads the package's compute path.

Per sample n, with v = resid = w (A x - t), inv = inv_wsum[n] (None: 1 / elements of one measurement):
    u[c,i,j]   = 2 inv v[c, i/pool, j/pool] / pool^2
    g_k[n,a,b] = sum_{c,i,j} u[c,i,j] x[c, i + ah - a, j + aw - b]      (x = 0 outside)       = d loss[n] / d k[a,b]
a PSF shared by the batch receives sum_n g_k[n]; with k = softmax(theta), g_theta[q] = k[q] (g_k[q] - sum_r k[r] g_k[r])."""
import functools

import torch
import torch.nn.functional as F

from oracle import glow_oracle as O

import decode_grad_oracle as D
import deblur_oracle as B
import restore_oracle as R
from restore_oracle import FLOOR, SECOND_ORDER, U, inv_wsum_of, round_up_ratio, worst_multiple  # noqa: F401

CHAIN = 64      # the longest fp32 fmaf chain of k_psf_grad_partial (csrc/restore_blind.hip: BLIND_CHAIN, one tile row)

d64 = lambda t: None if t is None else t.detach().double()


# ---------------------------------------------------------------------------------------------------------------------------
# the gradient with respect to the taps
def psf_grad(x, target, weight=None, inv_wsum=None, pool=1, psf=None):
    """g_k in the shape of ``psf`` ((kh,kw): summed over the batch; (N,kh,kw): per sample), fp64 autograd of
    `deblur_oracle._terms` with respect to the PSF."""
    k = d64(psf).requires_grad_(True)
    with torch.enable_grad():
        loss, _ = B._terms(d64(x), d64(target), d64(weight), d64(inv_wsum), pool, k)
        g, = torch.autograd.grad(loss.sum(), [k])
    return g


def u_of(resid, inv_wsum, pool):
    """u = P^T (2 inv resid / pool^2) at image resolution, fp64."""
    v = d64(resid)
    inv = torch.full((v.shape[0],), 1.0 / v[0].numel(), dtype=torch.float64) if inv_wsum is None else d64(inv_wsum)
    cell = (2.0 * inv / float(pool * pool)).view(-1, 1, 1, 1) * v
    return cell.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1) if pool > 1 else cell


def correlate(u, x, kh, kw):
    """(N, kh, kw): sum_{c,i,j} u[n,c,i,j] x[n,c, i + ah - a, j + aw - b], x zero outside -- the definition, tap by tap."""
    ah, aw = (kh - 1) // 2, (kw - 1) // 2
    H, W = x.shape[-2:]
    xp = F.pad(x, (aw, aw, ah, ah))
    g = torch.zeros((x.shape[0], kh, kw), dtype=x.dtype)
    for a in range(kh):
        for b in range(kw):
            g[:, a, b] = (u * xp[:, :, 2 * ah - a:2 * ah - a + H, 2 * aw - b:2 * aw - b + W]).sum(dim=(1, 2, 3))
    return g


def psf_grad_explicit(x, resid, inv_wsum, pool, kh, kw, shared):
    g = correlate(u_of(resid, inv_wsum, pool), d64(x), kh, kw)
    return g.sum(dim=0) if shared else g


def blur_by(x, delta):
    """B_delta x for a (kh,kw) or (N,kh,kw) tap perturbation: the operator is linear in its taps."""
    return B.blur(x, delta)


# ---------------------------------------------------------------------------------------------------------------------------
# the softmax
def softmax(theta):
    """softmax over the last two dimensions, fp64, the max subtracted."""
    t = d64(theta)
    flat = t.reshape(*t.shape[:-2], -1)
    e = torch.exp(flat - flat.max(dim=-1, keepdim=True).values)
    return (e / e.sum(dim=-1, keepdim=True)).reshape(t.shape)


def softmax_backward(k, g):
    """g_theta[q] = k[q] (g[q] - sum_r k[r] g[r]) over the last two dimensions."""
    k, g = d64(k), d64(g)
    dot = (k * g).sum(dim=(-2, -1), keepdim=True)
    return k * (g - dot)


# ---------------------------------------------------------------------------------------------------------------------------
# the bound
def _inexact_constants(inv_wsum, elements, pool):
    """How many of the kernel's two fp32 constants -- the default inv_wsum 1 / elements, and 1 / pool^2 -- are not the oracle's
    exact values (each is then one more relative u on u)."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).float())
    n = int(inv_wsum is None and f32(1.0 / elements) != 1.0 / elements)
    return n + int(f32(1.0 / (pool * pool)) != 1.0 / (pool * pool))


def bound(x, target, weight=None, inv_wsum=None, pool=1, psf=None, E_k=None):
    """(E_grad_psf, E_grad_logits) in the shape of ``psf``: first-order bounds on |device - oracle|, walked over the roundings of
    csrc/restore_blind.hip; they hold for ANY order of the sums.
      v      = resid: `deblur_oracle.bound`'s E_resid, carried through
      u      = (2 inv v) (1 / pool^2): two roundings (2 inv is exact), and one more u |u| for each of the two constants that is not
               the oracle's exact value (`_inexact_constants`):                  E_u = K E_v + (2 + constants) (u |u| + FLOOR)
      chain  an fp32 fmaf chain of at most L = CHAIN terms: each of its L roundings is of a partial sum no larger than the chain's
               sum |u| |x|, so a chain costs L u sum_chain |u| |x|, and all chains of a tap together L u sum |u| |x| -- however the
               pixels are dealt to chains; the errors of u are carried:          sum E_u |x| + L u sum |u| |x|
      folds  in fp64: nothing at this order (2^-53 against 2^-24); a shared PSF sums the samples' bounds
      g_k    the final rounding, once:                                           + u |g_k| + FLOOR
      g_th   = k (g - sum k g) in fp64 from the UNROUNDED g, one rounding; the errors of g and of k (``E_k``: None = k is the
               kernel's input, exact) carried through the formula:
               |k| (E_g + sum |k| E_g + sum E_k |g|) + E_k |g - sum k g| + u |g_th| + FLOOR
    The whole times SECOND_ORDER, FLOOR added per rounding as in `restore_oracle.bound`."""
    x, t, w, inv, k = d64(x), d64(target), d64(weight), d64(inv_wsum), d64(psf)
    shared = k.dim() == 2
    kh, kw = k.shape[-2:]
    _, _, resid = B.objective(x, t, w, inv, pool, k)
    _, _, E_v = B.bound(x, t, w, inv, pool, k)
    invv = torch.full((x.shape[0],), 1.0 / t[0].numel(), dtype=torch.float64) if inv is None else inv
    K = (2.0 * invv / float(pool * pool)).view(-1, 1, 1, 1)
    up = lambda v: v.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1) if pool > 1 else v
    u = up(K * resid)
    E_u = up(K * E_v) + (2.0 + _inexact_constants(inv_wsum, t[0].numel(), pool)) * (U * u.abs() + FLOOR)
    g = correlate(u, x, kh, kw)
    E_sum = correlate(E_u, x.abs(), kh, kw) + CHAIN * U * correlate(u.abs(), x.abs(), kh, kw) + FLOOR
    if shared:
        g, E_sum = g.sum(dim=0), E_sum.sum(dim=0)
    E_gk = E_sum + U * g.abs() + FLOOR
    Ek = torch.zeros_like(k) if E_k is None else d64(E_k)
    s = lambda v: v.sum(dim=(-2, -1), keepdim=True)
    gl = softmax_backward(k, g)
    E_gl = (k.abs() * (E_sum + s(k.abs() * E_sum) + s(Ek * g.abs())) + Ek * (g - s(k * g)).abs() + U * gl.abs() + FLOOR)
    return E_gk * SECOND_ORDER, E_gl * SECOND_ORDER


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# (shape of x, (kh, kw), pool, per-sample PSFs allowed): `deblur_oracle.OBJECTIVE_CASES`; one image of 70 x 66, which crosses the
# 8-row bands and the 64-column tiles with ragged edges both ways; and a batch of five, for the fold over the samples of a shared PSF
GRAD_CASES = B.OBJECTIVE_CASES + (((1, 1, 70, 66), (5, 5), 1), ((5, 2, 9, 12), (3, 5), 1))
GRAD_IDS = [f"{'x'.join(map(str, s))}-psf{k[0]}x{k[1]}-pool{p}" for s, k, p in GRAD_CASES]


def grad_inputs(shape, ksize, pool, weighted, per_sample, seed=0):
    """`deblur_oracle.objective_inputs`: (x, target, weight, inv_wsum, psf)."""
    return B.objective_inputs(shape, ksize, pool, weighted, per_sample, seed)


@functools.lru_cache(maxsize=None)
def grad_reference(shape, ksize, pool, weighted, per_sample):
    """The inputs of a case, the oracle's residual, both gradients and both bounds.  Computed once per process; callers must not
    modify the result."""
    x, t, w, inv, k = grad_inputs(shape, ksize, pool, weighted, per_sample)
    _, _, resid = B.objective(x, t, w, inv, pool, k)
    g = psf_grad(x, t, w, inv, pool, k)
    E_gk, E_gl = bound(x, t, w, inv, pool, k)
    return dict(x=x, target=t, weight=w, inv=inv, psf=k, resid=resid, grad_psf=g, grad_logits=softmax_backward(k, g), E_psf=E_gk,
                E_logits=E_gl)


# ---------------------------------------------------------------------------------------------------------------------------
# the fits
# Thresholds of the GPU fits (tests/test_gpu_blind.py), fixed by the oracle's own runs in tests/test_blind_host.py and rounded up to
# the next of `restore_oracle.RATIO_STEPS`.  Both on TINY_AFF (3 x 3 x 16 x 16), the true PSF the 5x5 Gaussian of sigma 1, the start
# the uniform 5x5 PSF, the weights the valid band.
#   calibrate: the images are known; ratio = final / start L1 error of the PSF
#   blind:     the latents start at the encode of the blurred image; ratio = the worst sample's final / first data term
FITS = {"calibrate": dict(steps=60, psf_lr=0.2, ratio=0.1),
        "blind": dict(steps=60, lr=0.05, psf_lr=0.2, ratio=0.1)}


def _problem():
    ref = D.reference(**R.TINY_AFF)
    psf = B.gaussian_psf(5, 1.0)
    target = ref["x"].float()
    meas = B.operator(target.double(), psf.double(), 1).float()
    weight = B.valid_weight(meas.shape, 5, 5, 1).expand_as(meas).contiguous()
    return ref, psf, target, meas, weight


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """A fit on the oracle, in fp64 with torch.optim.Adam: ``history`` (steps, N) holds the per-sample data term BEFORE each
    update, ``psf`` the final estimate, ``start`` the uniform start, ``true_psf`` the PSF that made the measurement.  Computed once per
    process; callers must not modify the result."""
    fit = FITS[name]
    ref, psf, target, meas, weight = _problem()
    inv = inv_wsum_of(weight).double()
    t, w = meas.double(), weight.double()
    start = torch.full((5, 5), 1.0 / 25.0, dtype=torch.float64)
    theta = torch.log(start).clone().requires_grad_(True)
    groups = [dict(params=[theta], lr=fit["psf_lr"])]
    if name == "blind":
        with torch.no_grad():
            z0, eps0 = D.encode_latents(meas, ref["sd"], ref["cfg"], ref["tables"])
        sdd = {k: v.double() for k, v in ref["sd"].items()}
        leaves = [z0.double().clone().requires_grad_(True)] + [e.double().clone().requires_grad_(True) for e in eps0]
        groups.append(dict(params=leaves, lr=fit["lr"]))
    opt = torch.optim.Adam(groups)
    hist = []
    for _ in range(fit["steps"]):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            x = target.double() if name == "calibrate" else O.flow_decode(leaves[0], sdd, ref["cfg"], leaves[1:], perm_tables=ref["tables"])
            flat = theta.reshape(-1)
            k = torch.softmax(flat, dim=0).reshape(5, 5)
            loss, _ = B._terms(x, t, w, inv, 1, k)
            loss.sum().backward()
        opt.step()
        hist.append(loss.detach())
    return dict(ref=ref, true_psf=psf, start=start.float(), target=target, measurement=meas, weight=weight, history=torch.stack(hist),
                psf=softmax(theta.detach()), **fit)


def l1(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().sum())

"""fp64 restatement of the restoration objective observed through a point-spread function (csrc/restore.hip,
glowhip_restore_objective_psf; the definition is in include/glowhip.h) in plain torch, the bound the device's fp32 result is held
to, the case tables of tests/test_deblur_host.py and tests/test_gpu_deblur.py, and the two deblurring fits through the CPU oracle's
decode.  Nothing here reads the package's compute path.

Per sample n and channel c, with k the sample's PSF (kh x kw, both odd), ah = (kh-1)/2, aw = (kw-1)/2:
    (B x)[c,i,j] = sum_{a,b} k[a,b] x[c, i + ah - a, j + aw - b]     (zero outside)  = F.conv2d with the FLIPPED k, depthwise
    A = P B,  P = avg_pool2d(., pool)
    loss[n] = inv_wsum[n] * sum w (A x - t)^2      resid = w (A x - t)      grad_x = d (sum_n loss[n]) / d x   (autograd)"""
import functools

import torch
import torch.nn.functional as F

from oracle import glow_oracle as O

import decode_grad_oracle as D
import restore_oracle as R
from restore_oracle import FLOOR, SECOND_ORDER, U, inv_wsum_of, round_up_ratio, worst_multiple  # noqa: F401

PSF_MAX = 15


# ---------------------------------------------------------------------------------------------------------------------------
# the operator
def _per_sample(psf, n):
    """(n, kh, kw) from (kh, kw) or (n, kh, kw)."""
    return psf.expand(n, *psf.shape) if psf.dim() == 2 else psf


def _depthwise(x, taps):
    """out[n,c,i,j] = sum_{a,b} taps[n,a,b] x[n,c, i - ah + a, j - aw + b], zero outside: F.conv2d (a correlation), one group per
    (sample, channel)."""
    n, c, h, w = x.shape
    kh, kw = taps.shape[-2:]
    wgt = taps[:, None].expand(n, c, kh, kw).reshape(n * c, 1, kh, kw)
    return F.conv2d(x.reshape(1, n * c, h, w), wgt, padding=((kh - 1) // 2, (kw - 1) // 2), groups=n * c).reshape(n, c, h, w)


def blur(x, psf):
    """B x: the true convolution -- F.conv2d with the flipped PSF, zero padding."""
    return _depthwise(x, _per_sample(psf, x.shape[0]).flip(-2, -1))


def blur_T(u, psf):
    """B^T u: the correlation with the PSF as given (used by the bound and by the adjoint test; `objective` takes autograd's)."""
    return _depthwise(u, _per_sample(psf, u.shape[0]))


def operator(x, psf, pool=1):
    """A x = P B x."""
    bx = blur(x, psf)
    return F.avg_pool2d(bx, pool) if pool > 1 else bx


def operator_T(v, psf, pool=1):
    """A^T v = B^T P^T v (P^T: every x under a cell receives the cell's value / pool^2)."""
    u = v.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1) / (pool * pool) if pool > 1 else v
    return blur_T(u, psf)


def _terms(x, target, weight, inv_wsum, pool, psf):
    d = operator(x, psf, pool) - target
    w = torch.ones_like(target) if weight is None else weight
    inv = torch.full((x.shape[0],), 1.0 / target[0].numel(), dtype=x.dtype) if inv_wsum is None else inv_wsum
    return inv * (w * d ** 2).sum(dim=(1, 2, 3)), w * d


def objective(x, target, weight=None, inv_wsum=None, pool=1, psf=None):
    """(loss (N,), grad_x, resid) in fp64 from inputs of any float dtype (widened exactly)."""
    d = lambda t: None if t is None else t.detach().double()
    xl = d(x).requires_grad_(True)
    with torch.enable_grad():
        loss, resid = _terms(xl, d(target), d(weight), d(inv_wsum), pool, d(psf))
        g, = torch.autograd.grad(loss.sum(), [xl])
    return loss.detach(), g, resid.detach()


# ---------------------------------------------------------------------------------------------------------------------------
# PSFs and inputs
def gaussian_psf(side=5, sigma=1.0):
    """The side x side Gaussian of standard deviation ``sigma``, normalised to sum 1 in fp64, as fp32."""
    r = torch.arange(side, dtype=torch.float64) - (side - 1) / 2
    g = torch.exp(-r ** 2 / (2 * sigma ** 2))
    k = g[:, None] * g[None, :]
    return (k / k.sum()).float()


def asymmetric_psf(kh, kw, n=None, seed=0):
    """A positive PSF with no symmetry (random taps plus a ramp along both axes), sum 1 up to fp32 rounding; ``n``: one per sample."""
    g = torch.Generator().manual_seed(4100 + seed)
    k = torch.rand((n or 1, kh, kw), generator=g) + 0.25
    k = k * torch.linspace(0.5, 1.5, kh)[None, :, None] * torch.linspace(2.0, 0.5, kw)[None, None, :]
    k = (k / k.sum(dim=(1, 2), keepdim=True)).float()
    return k if n else k[0]


# (shape of x, (kh, kw), pool) of tests/test_gpu_deblur.py: an image smaller than any tile with odd sides; a PSF larger than the image;
# a rectangular PSF under a pool; several tiles with the halo across their borders; a one-dimensional PSF (a motion line); pool 4
OBJECTIVE_CASES = (((2, 1, 5, 7), (3, 3), 1), ((2, 1, 5, 7), (15, 15), 1), ((3, 3, 6, 10), (5, 3), 2), ((2, 3, 64, 64), (15, 15), 1),
                   ((2, 3, 64, 64), (1, 9), 1), ((2, 3, 16, 32), (7, 7), 4))
CASE_IDS = [f"{'x'.join(map(str, s))}-psf{k[0]}x{k[1]}-pool{p}" for s, k, p in OBJECTIVE_CASES]


def objective_inputs(shape, ksize, pool, weighted, per_sample, seed=0):
    """(x, target, weight, inv_wsum, psf): `restore_oracle.objective_inputs` (weights with every seventh an exact zero, or None /
    None) and an asymmetric PSF, one for the batch or one per sample."""
    x, target, weight, inv = R.objective_inputs(shape, pool, weighted, seed)
    return x, target, weight, inv, asymmetric_psf(*ksize, n=shape[0] if per_sample else None, seed=seed)


# ---------------------------------------------------------------------------------------------------------------------------
# the bound
def bound(x, target, weight=None, inv_wsum=None, pool=1, psf=None):
    """(E_loss (N,), E_grad like x, E_resid like target): first-order bounds on |device - objective(...)|, built as
    `restore_oracle.bound` is: each fp32 rounding adds u |result| (+ FLOOR), incoming errors are carried through, the whole times
    1 + 2^-10.  They hold for any order of the tap sums, with or without fused multiply-add.  With n = kh kw taps and S = |k| (*) |x|:
      B x    n products and n - 1 additions, every partial sum no larger than S (fused: n roundings in all):           n u S
      px     pool = 1: B x.  pool > 1: pool^2 - 1 additions of values whose moduli sum to at most pool^2 avg_pool(S), and the
             multiplication by 1 / pool^2:          avg_pool(E_Bx) + pool^2 u avg_pool(S)
      d      = px - t, v = w d: one rounding each; v is `resid`
      cell   = (2 inv v) (1 / pool^2): two roundings and the two constants, u |cell| four times; u = P^T cell copies it
      grad   = B^T u: the same n-term sum over the cells' values, whose errors it carries:    |k| (*)^T E_u + n u |k| (*)^T |u|
      loss   as in `restore_oracle.bound`: fp64 products and sum, the errors of v and d carried, the constant and the final rounding."""
    d64 = lambda t: None if t is None else t.detach().double()
    x, t, w, inv, k = d64(x), d64(target), d64(weight), d64(inv_wsum), d64(psf)
    w = torch.ones_like(t) if w is None else w
    inv = torch.full((x.shape[0],), 1.0 / t[0].numel(), dtype=torch.float64) if inv is None else inv
    n_taps = float(k.shape[-2] * k.shape[-1])
    p2 = float(pool * pool)
    up = lambda v: v.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1) if pool > 1 else v
    loss, g, v = objective(x, t, w, inv, pool, k)
    S = blur(x.abs(), k.abs())
    E_bx = n_taps * U * S + FLOOR
    if pool > 1:
        E_px = F.avg_pool2d(E_bx, pool) + p2 * U * F.avg_pool2d(S, pool) + FLOOR
    else:
        E_px = E_bx
    d = operator(x, k, pool) - t
    E_d = E_px + U * d.abs() + FLOOR
    E_v = w.abs() * E_d + U * v.abs() + FLOOR
    K = (2.0 * inv / p2).view(-1, 1, 1, 1)
    cell = K * v
    E_cell = K * E_v + 4.0 * (U * cell.abs() + FLOOR)
    E_g = blur_T(up(E_cell), k.abs()) + n_taps * U * blur_T(up(cell.abs()), k.abs()) + FLOOR
    E_loss = inv * (d.abs() * E_v + v.abs() * E_d).sum(dim=(1, 2, 3)) + 2.0 * (U * loss.abs() + FLOOR)
    return E_loss * SECOND_ORDER, E_g * SECOND_ORDER, E_v * SECOND_ORDER


# ---------------------------------------------------------------------------------------------------------------------------
# latent gradients and the fits
def latent_grads(z, eps, sd, cfg, target, weight=None, inv_wsum=None, pool=1, psf=None, tables=None):
    """(x, loss (N,), g_z, [g_eps]): fp64 autograd of the objective through `O.flow_decode` and the operator above."""
    d = lambda t: None if t is None else t.detach().double()
    sdd = {k: v.double() for k, v in sd.items()}
    zl = d(z).requires_grad_(True)
    el = [d(e).requires_grad_(True) for e in eps]
    with torch.enable_grad():
        x = O.flow_decode(zl, sdd, cfg, el, perm_tables=tables)
        loss, _ = _terms(x, d(target), d(weight), d(inv_wsum), pool, d(psf))
        grads = torch.autograd.grad(loss.sum(), [zl] + el)
    return x.detach(), loss.detach(), grads[0], list(grads[1:])


def valid_weight(meas_shape, kh, kw, pool):
    """The band of ``border="valid"`` by brute force: a measurement cell keeps weight 1 only if every x its footprint reads -- rows
    i pool - ah .. i pool + pool - 1 + ah, columns alike -- lies inside the image."""
    h, w = meas_shape[-2:]
    ah, aw = (kh - 1) // 2, (kw - 1) // 2
    m = torch.zeros((h, w))
    for i in range(h):
        for j in range(w):
            rows = [i * pool + u + ah - a for u in range(pool) for a in range(kh)]      # every x row (B x)[i pool + u] reads
            cols = [j * pool + v + aw - b for v in range(pool) for b in range(kw)]
            inside = all(0 <= y < h * pool for y in rows) and all(0 <= x < w * pool for x in cols)
            m[i, j] = 1.0 if inside else 0.0
    return m


# Thresholds of the GPU fits (tests/test_gpu_deblur.py), fixed by the oracle's own runs in tests/test_deblur_host.py: the largest
# final / first ratio of any sample's data term, rounded up to the next of `restore_oracle.RATIO_STEPS`
FITS = {"deblur": dict(case="tiny", pool=1, steps=40, lr=0.05, ratio=0.1),       # TINY_AFF (16x16), 5x5 Gaussian of sigma 1
        "deblur_sr": dict(case="T", pool=2, steps=20, lr=0.2, ratio=0.1)}        # case T (64x16, hidden 512), the same PSF, pool 2


def case_kwargs(case):
    if case == "tiny":
        return R.TINY_AFF
    from test_decode_grad_host import SHAPE_CASES
    return SHAPE_CASES[case]


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """A deblurring fit on the oracle, as `Inferer.restore(psf=, border="valid")` sets it up: the target is the decode of the
    case's latents, the measurement the operator applied to it (fp64, rounded to fp32), the weights the valid band, the start the
    fp32 encode of the measurement (pool > 1: of its pixel-repeated upsampling).  Adam in fp64 (torch.optim.Adam), the data term
    summed over the samples; ``history`` (steps, N) holds the per-sample loss BEFORE each update.  Computed once per process;
    callers must not modify the result."""
    fit = FITS[name]
    pool = fit["pool"]
    ref = D.reference(**case_kwargs(fit["case"]))
    psf = gaussian_psf(5, 1.0)
    target = ref["x"].float()
    meas = operator(target.double(), psf.double(), pool).float()
    weight = valid_weight(meas.shape, 5, 5, pool).expand_as(meas).contiguous()
    inv = inv_wsum_of(weight)
    start = meas if pool == 1 else meas.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1)
    with torch.no_grad():
        z0, eps0 = D.encode_latents(start, ref["sd"], ref["cfg"], ref["tables"])
    sdd = {k: v.double() for k, v in ref["sd"].items()}
    leaves = [z0.double().clone().requires_grad_(True)] + [e.double().clone().requires_grad_(True) for e in eps0]
    opt = torch.optim.Adam(leaves, lr=fit["lr"])
    t, w, iv, k = meas.double(), weight.double(), inv.double(), psf.double()
    hist = []
    for _ in range(fit["steps"]):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            x = O.flow_decode(leaves[0], sdd, ref["cfg"], leaves[1:], perm_tables=ref["tables"])
            loss, _ = _terms(x, t, w, iv, pool, k)
            loss.sum().backward()
        opt.step()
        hist.append(loss.detach())
    return dict(ref=ref, psf=psf, target=target, measurement=meas, weight=weight, history=torch.stack(hist), **fit)

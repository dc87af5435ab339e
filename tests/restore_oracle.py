"""fp64 restatement of the restoration objective (csrc/restore.hip, glowhip_restore_objective) in plain torch, and of the
restoration loop of `network.restore.LatentFit` through the CPU oracle's decode (tests/decode_grad_oracle.py) with
torch.optim.Adam(weight_decay = prior weight).  Nothing here reads the package's compute path.

Per sample n, with P = avg_pool2d(., pool) (pool = 1: the identity):
    loss[n] = inv_wsum[n] * sum w (P x - t)^2          grad_x = d (sum_n loss[n]) / d x   (autograd)
``weight=None`` is all ones, ``inv_wsum=None`` is 1 / (elements of one sample's measurement)."""
import functools

import torch
import torch.nn.functional as F

from oracle import glow_oracle as O

import decode_grad_oracle as D

# the 16x16 / hidden 32 model of tests/test_gpu_decode_grad.py (TINY_AFF: fp64 ReLU margin 3.7e-5)
TINY_AFF = dict(image=16, hidden=32, K=2, L=2, batch=3, zeros_std=0.05, seed=1)

# Thresholds of the GPU fits (tests/test_gpu_restore.py), fixed by the oracle's own runs in tests/test_restore_host.py: the largest
# final / first ratio of any sample's loss over 20 Adam steps at lr 0.2, rounded up to the next of RATIO_STEPS
RATIO_STEPS = (0.1, 0.2, 0.5)
FIT_STEPS, FIT_LR = 20, 0.2
INPAINT_RATIO = 0.1      # TINY_AFF, pool 1, left half masked: the oracle's samples 0.082, 0.080, 0.090
SUPERRES_RATIO = 0.1     # case T (64x16, hidden 512), pool 2, left half of the low-resolution image: 0.025, 0.023, 0.027


def round_up_ratio(r):
    """The next of RATIO_STEPS at or above ``r`` (None beyond the last: such a fit proves nothing)."""
    return next((s for s in RATIO_STEPS if r <= s), None)


def inv_wsum_of(weight):
    """`Inferer.restore`'s per-sample normalisation: 1 / max(sum w[n], 1), in the dtype of the weights."""
    return 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0)


def _loss(x, target, weight, inv_wsum, pool):
    px = F.avg_pool2d(x, pool) if pool > 1 else x
    w = torch.ones_like(target) if weight is None else weight
    inv = torch.full((x.shape[0],), 1.0 / target[0].numel(), dtype=x.dtype) if inv_wsum is None else inv_wsum
    return inv * (w * (px - target) ** 2).sum(dim=(1, 2, 3))


def objective(x, target, weight=None, inv_wsum=None, pool=1):
    """(loss (N,), grad_x) in fp64 from inputs of any float dtype (widened exactly)."""
    d = lambda t: None if t is None else t.detach().double()
    xl = d(x).requires_grad_(True)
    with torch.enable_grad():
        loss = _loss(xl, d(target), d(weight), d(inv_wsum), pool)
        g, = torch.autograd.grad(loss.sum(), [xl])
    return loss.detach(), g


# ---------------------------------------------------------------------------------------------------------------------------
# The bound the device's fp32 result is held to, from the kernel's operation count (csrc/restore.hip: restore_cell and its callers).
U = 2.0 ** -24                   # unit roundoff of fp32
SECOND_ORDER = 1.0 + 2.0 ** -10  # products of two first-order terms
FLOOR = 2.0 ** -126              # per rounding, absolute (gradual underflow or flush to zero)

# (shape of x, pool) of tests/test_gpu_restore.py: 35 elements per sample (scalar tail only); a 3x5 measurement of odd width; the
# 16-byte path (aligned, and one float off); pool 4
OBJECTIVE_SHAPES = (((2, 1, 5, 7), 1), ((3, 3, 6, 10), 2), ((2, 3, 64, 64), 1), ((2, 3, 16, 32), 4))


def objective_inputs(shape, pool, weighted, seed=0):
    """(x, target, weight, inv_wsum) as fp32 tensors: an image in [0, 1), a measurement in [0, 1), weights in [0, 1) with every
    seventh an exact zero and `inv_wsum_of` them -- or (None, None): all ones, the kernel's own 1 / elements."""
    g = torch.Generator().manual_seed(4000 + seed)
    n, c, h, w = shape
    x = torch.rand(shape, generator=g)
    target = torch.rand((n, c, h // pool, w // pool), generator=g)
    if not weighted:
        return x, target, None, None
    weight = torch.rand(target.shape, generator=g)
    weight.view(-1)[::7] = 0.0
    return x, target, weight, inv_wsum_of(weight)


def bound(x, target, weight=None, inv_wsum=None, pool=1):
    """(E_loss (N,), E_grad like x): first-order bounds on |device - objective(...)|, walking the kernel's fp32 roundings; each
    adds u |result|, incoming errors are carried through, the whole times 1 + 2^-10 for the second-order terms.
      px   pool = 1: x itself, no rounding.  pool > 1: pool^2 - 1 additions, each rounding a partial sum no larger than the patch's
           S = sum |x|, then the multiplication by 1 / pool^2, which scales that error and rounds once more (|px| <= S / pool^2):
           (pool^2 - 1) u S / pool^2 + u S / pool^2 = pool^2 u avg_pool(|x|)
      d    = px - t: one rounding
      wd   = w * d: one rounding
      g    = (2 inv * wd) * (1 / pool^2): two roundings (2 inv is exact), one more each for the constants float(1 / elements) --
             the default inv_wsum -- and float(1 / pool^2) where they are not the oracle's exact values: u |g| four times
      loss = float(inv * sum (double) wd * (double) d): products and sum in fp64 (2^-53 relative: not counted), the error of wd and d
             carried, the constant inv and the final rounding u |loss| each."""
    d64 = lambda t: None if t is None else t.detach().double()
    x, t, w, inv = d64(x), d64(target), d64(weight), d64(inv_wsum)
    w = torch.ones_like(t) if w is None else w
    inv = torch.full((x.shape[0],), 1.0 / t[0].numel(), dtype=torch.float64) if inv is None else inv
    p2 = float(pool * pool)
    loss, g = objective(x, t, w, inv, pool)
    px = F.avg_pool2d(x, pool) if pool > 1 else x
    E_px = p2 * U * F.avg_pool2d(x.abs(), pool) + FLOOR if pool > 1 else torch.zeros_like(x)
    d = px - t
    E_d = E_px + U * d.abs() + FLOOR
    wd = w * d
    E_wd = w.abs() * E_d + U * wd.abs() + FLOOR
    K = (2.0 * inv / p2).view(-1, 1, 1, 1)
    E_cell = K * E_wd
    E_cell = F.interpolate(E_cell, scale_factor=pool, mode="nearest") if pool > 1 else E_cell      # every x under a cell: the cell's
    E_g = E_cell + 4.0 * (U * g.abs() + FLOOR)
    E_loss = inv * (d.abs() * E_wd + wd.abs() * E_d).sum(dim=(1, 2, 3)) + 2.0 * (U * loss.abs() + FLOOR)
    return E_loss * SECOND_ORDER, E_g * SECOND_ORDER


def worst_multiple(got, ref, E):
    """max |got - ref| / E over the elements (0 where they agree exactly, whatever E)."""
    diff = (got.detach().cpu().double() - ref).abs()
    return float(torch.where(diff == 0, torch.zeros_like(diff), diff / E).max())


def latent_grads(z, eps, sd, cfg, target, weight=None, inv_wsum=None, pool=1, tables=None):
    """(x, loss (N,), g_z, [g_eps]): the objective of the decoded latents and its gradient with respect to them, fp64 autograd
    through `O.flow_decode`."""
    d = lambda t: None if t is None else t.detach().double()
    sdd = {k: v.double() for k, v in sd.items()}
    zl = d(z).requires_grad_(True)
    el = [d(e).requires_grad_(True) for e in eps]
    with torch.enable_grad():
        x = O.flow_decode(zl, sdd, cfg, el, perm_tables=tables)
        loss = _loss(x, d(target), d(weight), d(inv_wsum), pool)
        grads = torch.autograd.grad(loss.sum(), [zl] + el)
    return x.detach(), loss.detach(), grads[0], list(grads[1:])


def restore_loop(z, eps, sd, cfg, target, weight=None, inv_wsum=None, pool=1, steps=FIT_STEPS, lr=FIT_LR, prior_weight=0.0, tables=None):
    """The restoration loop in fp64: Adam (torch.optim.Adam, weight_decay = prior_weight: it adds prior_weight * p to the gradient,
    the gradient of prior_weight / 2 ||p||^2) on the latents, the data term summed over the samples.  Returns
    ``(z, [eps], loss history (steps, N))`` -- the history holds the per-sample loss BEFORE each update, as `RestoreInfo.loss`."""
    d = lambda t: None if t is None else t.detach().double()
    sdd = {k: v.double() for k, v in sd.items()}
    leaves = [d(z).clone().requires_grad_(True)] + [d(e).clone().requires_grad_(True) for e in eps]
    opt = torch.optim.Adam(leaves, lr=lr, weight_decay=prior_weight)
    t, w, inv = d(target), d(weight), d(inv_wsum)
    hist = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            x = O.flow_decode(leaves[0], sdd, cfg, leaves[1:], perm_tables=tables)
            loss = _loss(x, t, w, inv, pool)
            loss.sum().backward()
        opt.step()
        hist.append(loss.detach())
    return leaves[0].detach(), [e.detach() for e in leaves[1:]], torch.stack(hist)


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """The two fits the GPU tests repeat -- "inpaint" (TINY_AFF, pool 1) and "superres" (case T of tests/test_decode_grad_host.py,
    pool 2) -- on the oracle: the target is the decode of the case's latents, the measurement its pool x pool average, the weights
    the left half of the measurement, the start the fp32 encode of the target with that half blanked (a start that already matches
    under the mask would have nothing to fit).  Computed once per process; callers must not modify the result."""
    if name == "inpaint":
        kw, pool = TINY_AFF, 1
    else:
        from test_decode_grad_host import SHAPE_CASES
        kw, pool = SHAPE_CASES["T"], 2
    ref = D.reference(**kw)
    target = ref["x"].float()
    with torch.no_grad():
        meas = F.avg_pool2d(target, pool) if pool > 1 else target
    weight = torch.zeros_like(meas)
    weight[..., : meas.shape[-1] // 2] = 1.0
    blank = torch.ones_like(target)
    blank[..., : target.shape[-1] // 2] = 0.0
    with torch.no_grad():
        z0, eps0 = D.encode_latents(target * blank, ref["sd"], ref["cfg"], ref["tables"])
    inv = inv_wsum_of(weight)
    _, _, hist = restore_loop(z0, eps0, ref["sd"], ref["cfg"], meas, weight, inv, pool, tables=ref["tables"])
    return dict(ref=ref, pool=pool, target=target, measurement=meas, weight=weight, blank=blank, history=hist)

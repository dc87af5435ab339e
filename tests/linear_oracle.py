"""fp64 restatement of the restoration objective observed through a dense linear operator (csrc/restore_linear.hip,
glowhip_restore_objective_linear; the definition is in include/glowhip.h) in plain torch, the bound the device's fp32 result is held
to, the case tables of tests/test_linear_host.py and tests/test_gpu_linear.py, the Gaussian sensing matrix of
`network.restore.gaussian_operator` restated through tests/sampler_oracle.py, and a compressed-sensing fit through the CPU oracle's
decode.  Nothing here reads the package's compute path.

Per sample n, with x[n] flattened to D = C H W values in (C,H,W) order and A (M, C, H, W) flattened to (M, D):
    y = A x      resid = w (y - t)      loss[n] = inv_wsum[n] sum_m w (y - t)^2      grad_x = d (sum_n loss[n]) / d x   (autograd)
``weight=None`` is all ones, ``inv_wsum=None`` is 1 / M."""
import functools

import numpy as np
import torch

from oracle import glow_oracle as O

import decode_grad_oracle as D
import restore_oracle as R
import sampler_oracle as SO
from restore_oracle import FLOOR, SECOND_ORDER, U, round_up_ratio, worst_multiple  # noqa: F401

OPERATOR_STREAM = 248      # the sampler stream that names a Gaussian sensing matrix (include/glowhip.h)


# ---------------------------------------------------------------------------------------------------------------------------
# the operator
def operator(x, A):
    """A x: (N, M) from x (N,C,H,W) and A (M,C,H,W)."""
    return x.flatten(1) @ A.flatten(1).t()


def operator_T(v, A):
    """A^T v: (N,C,H,W) from v (N, M)."""
    return (v @ A.flatten(1)).view(v.shape[0], *A.shape[1:])


def inv_wsum_of(weight):
    """`Inferer.restore`'s per-sample normalisation for an (N, M) weight: 1 / max(sum w[n], 1)."""
    return 1.0 / weight.sum(dim=1).clamp(min=1.0)


def _terms(x, target, weight, inv_wsum, A):
    d = operator(x, A) - target
    w = torch.ones_like(target) if weight is None else weight
    inv = torch.full((x.shape[0],), 1.0 / target.shape[1], dtype=x.dtype) if inv_wsum is None else inv_wsum
    return inv * (w * d ** 2).sum(dim=1), w * d


def objective(x, target, weight=None, inv_wsum=None, A=None):
    """(loss (N,), grad_x, resid (N, M)) in fp64 from inputs of any float dtype (widened exactly)."""
    d = lambda t: None if t is None else t.detach().double()
    xl = d(x).requires_grad_(True)
    with torch.enable_grad():
        loss, resid = _terms(xl, d(target), d(weight), d(inv_wsum), d(A))
        g, = torch.autograd.grad(loss.sum(), [xl])
    return loss.detach(), g, resid.detach()


# ---------------------------------------------------------------------------------------------------------------------------
# cases and inputs of tests/test_gpu_linear.py
# image shapes: D = 35 (the element path, less than one 16-byte vector per lane), D = 192, D = 12 288 (three D slices of 4 096)
IMAGE_SHAPES = ((1, 5, 7), (3, 8, 8), (3, 64, 64))
# rows: below, astride and above the forward product's row tile (8) and the adjoint's M slice (128)
ROWS = (1, 3, 67, 130)
# batches: below, at ... above the forward product's sample tile (4); 67 is above the adjoint's sample block (64)
BATCHES = (1, 3, 5)
BATCH_ABOVE_THE_SAMPLE_BLOCK = 67
CASE_IDS = [f"{'x'.join(map(str, s))}-M{m}" for s in IMAGE_SHAPES for m in ROWS]
CASES = [(s, m) for s in IMAGE_SHAPES for m in ROWS]


def batches_of(shape, m):
    """The batch sizes a (shape, M) case runs: `BATCHES`, and the one above the adjoint's sample block where the operator is small
    (and once at the largest shape)."""
    big = shape == IMAGE_SHAPES[0] or (shape == IMAGE_SHAPES[-1] and m == ROWS[-1])
    return BATCHES + ((BATCH_ABOVE_THE_SAMPLE_BLOCK,) if big else ())


def objective_inputs(n, shape, m, weighted, seed=0):
    """(x, target, weight, inv_wsum, A) as fp32 tensors: an image in [0, 1), an operator of N(0, 1/m) entries, a measurement near
    A x' of another image, weights in [0, 1) with every seventh an exact zero and `inv_wsum_of` them -- or (None, None): all ones,
    the kernel's own 1 / M."""
    g = torch.Generator().manual_seed(5000 + seed)
    x = torch.rand((n,) + tuple(shape), generator=g)
    A = torch.randn((m,) + tuple(shape), generator=g) / float(m) ** 0.5
    target = operator(torch.rand((n,) + tuple(shape), generator=g), A) + 0.1 * torch.randn((n, m), generator=g)
    if not weighted:
        return x, target, None, None, A
    weight = torch.rand((n, m), generator=g)
    weight.view(-1)[::7] = 0.0
    return x, target, weight, inv_wsum_of(weight), A


# ---------------------------------------------------------------------------------------------------------------------------
# the bound
def bound(x, target, weight=None, inv_wsum=None, A=None):
    """(E_loss (N,), E_grad like x, E_resid (N, M)): first-order bounds on |device - objective(...)|, built as
    `restore_oracle.bound` is: each fp32 rounding adds u |result| (+ FLOOR), incoming errors are carried through, the whole times
    1 + 2^-10.  They hold for ANY order of the two sums -- sliced, tree-reduced or element by element -- fused or not:
      y      D products and D - 1 additions, every partial sum no larger than S = |A| |x| (fused: D roundings in all):    D u S
      d      = y - t, v = w d: one rounding each; v is `resid`
      u      = (2 inv) v: one rounding (2 inv is exact), one more for the constant float(1 / M) -- the default inv_wsum -- where it
             is not the oracle's exact value: u |u| twice
      grad   = A^T u: an M-term sum over the cells' values, whose errors it carries:    |A|^T E_u + M u |A|^T |u|
      loss   as in `restore_oracle.bound`: fp64 products and sum, the errors of v and d carried, the constant and the final rounding."""
    d64 = lambda t: None if t is None else t.detach().double()
    x, t, w, inv, A = d64(x), d64(target), d64(weight), d64(inv_wsum), d64(A)
    n, m = t.shape
    dim = float(A[0].numel())
    w = torch.ones_like(t) if w is None else w
    inv = torch.full((n,), 1.0 / m, dtype=torch.float64) if inv is None else inv
    loss, g, v = objective(x, t, w, inv, A)
    S = operator(x.abs(), A.abs())
    E_y = dim * U * S + FLOOR
    d = operator(x, A) - t
    E_d = E_y + U * d.abs() + FLOOR
    E_v = w.abs() * E_d + U * v.abs() + FLOOR
    K = (2.0 * inv).view(-1, 1)
    u = K * v
    E_u = K * E_v + 2.0 * (U * u.abs() + FLOOR)
    E_g = operator_T(E_u, A.abs()) + float(m) * U * operator_T(u.abs(), A.abs()) + FLOOR
    E_loss = inv * (d.abs() * E_v + v.abs() * E_d).sum(dim=1) + 2.0 * (U * loss.abs() + FLOOR)
    return E_loss * SECOND_ORDER, E_g * SECOND_ORDER, E_v * SECOND_ORDER


# ---------------------------------------------------------------------------------------------------------------------------
# the Gaussian sensing matrix
def gaussian_operator(m, image_shape, seed):
    """`network.restore.gaussian_operator` on the CPU, in fp64: stream 248 of the sampler's generator at (seed, call 0), element =
    flat index in the (m, C, H, W) matrix, times float32(1 / sqrt(m))."""
    shape = (int(m),) + tuple(int(v) for v in image_shape)
    e = SO.normal(int(np.prod(shape)), seed, 0, OPERATOR_STREAM, np.float32(1.0 / np.sqrt(float(m))))
    return torch.from_numpy(np.ascontiguousarray(e)).view(shape)


# ---------------------------------------------------------------------------------------------------------------------------
# latent gradients and the fit
def latent_grads(z, eps, sd, cfg, target, weight=None, inv_wsum=None, A=None, tables=None):
    """(x, loss (N,), g_z, [g_eps]): fp64 autograd of the objective through `O.flow_decode` and the operator above."""
    d = lambda t: None if t is None else t.detach().double()
    sdd = {k: v.double() for k, v in sd.items()}
    zl = d(z).requires_grad_(True)
    el = [d(e).requires_grad_(True) for e in eps]
    with torch.enable_grad():
        x = O.flow_decode(zl, sdd, cfg, el, perm_tables=tables)
        loss, _ = _terms(x, d(target), d(weight), d(inv_wsum), d(A))
        grads = torch.autograd.grad(loss.sum(), [zl] + el)
    return x.detach(), loss.detach(), grads[0], list(grads[1:])


# The compressed-sensing fit of tests/test_gpu_linear.py, its threshold fixed by the oracle's own run in tests/test_linear_host.py:
# the smallest of `restore_oracle.RATIO_STEPS` that is at least TWICE the oracle's worst final / first ratio
FIT = dict(case="tiny", m=256, seed=7, steps=40, lr=0.1, ratio=0.1)      # TINY_AFF (16x16x3: D = 768, M = D / 3)


def case_kwargs(case):
    if case == "tiny":
        return R.TINY_AFF
    from test_decode_grad_host import SHAPE_CASES
    return SHAPE_CASES[case]


def threshold_of(ratio):
    """The smallest of 0.1 / 0.2 / 0.5 that is at least twice ``ratio`` (None above 0.25: such a fit proves nothing)."""
    return round_up_ratio(2.0 * ratio)


@functools.lru_cache(maxsize=None)
def fit_case():
    """The compressed-sensing fit on the oracle, as `Inferer.restore(t, operator=gaussian_operator(...))` sets it up: the unknown
    image is the decode of the case's latents, the measurement the Gaussian operator applied to it (fp64, rounded to fp32), unit
    weights, the start the all-zero latents.  Adam in fp64 (torch.optim.Adam), the data term summed over the samples; ``history``
    (steps, N) holds the per-sample loss BEFORE each update.  Computed once per process; callers must not modify the result."""
    fit = FIT
    ref = D.reference(**case_kwargs(fit["case"]))
    target = ref["x"].float()
    A = gaussian_operator(fit["m"], target.shape[1:], fit["seed"]).float()
    meas = operator(target.double(), A.double()).float()
    sdd = {k: v.double() for k, v in ref["sd"].items()}
    leaves = [torch.zeros_like(ref["z"], dtype=torch.float64).requires_grad_(True)]
    leaves += [torch.zeros_like(e, dtype=torch.float64).requires_grad_(True) for e in ref["eps"]]
    opt = torch.optim.Adam(leaves, lr=fit["lr"])
    t, a = meas.double(), A.double()
    hist = []
    for _ in range(fit["steps"]):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            x = O.flow_decode(leaves[0], sdd, ref["cfg"], leaves[1:], perm_tables=ref["tables"])
            loss, _ = _terms(x, t, None, None, a)
            loss.sum().backward()
        opt.step()
        hist.append(loss.detach())
    return dict(ref=ref, A=A, target=target, measurement=meas, history=torch.stack(hist), **fit)

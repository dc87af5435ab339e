"""fp64 restatement of the restoration objective observed in the Fourier domain (csrc/restore_fourier.hip,
glowhip_restore_objective_fourier and glowhip_fourier2d; the definition is in include/glowhip.h) in plain torch, the bound the
device's fp32 result is held to, the case tables of tests/test_fourier_host.py and tests/test_gpu_fourier.py, the undersampling masks
of `network.restore.fourier_mask` restated, and a k-space fit through the CPU oracle's decode.  Nothing here reads the package's
compute path.

Per sample n and channel c, with F the unitary 2-D DFT of the H x W plane (`torch.fft.fft2(norm="ortho")`: unshifted, (0,0) is DC):
    X = F x      resid = w (X - t)      loss[n] = inv_wsum[n] sum_{c,k} w |X - t|^2      grad_x = d (sum_n loss[n]) / d x   (autograd)
                                                                                                = 2 inv_wsum[n] Re(F^H resid)
``target`` is complex (N,C,H,W) (or real with a trailing 2), ``weight`` real (N,C,H,W); ``weight=None`` is all ones, ``inv_wsum=None``
is 1 / (C H W)."""
import functools
import math

import torch

from oracle import glow_oracle as O

import decode_grad_oracle as D
import restore_oracle as R
from restore_oracle import FLOOR, SECOND_ORDER, U, round_up_ratio, worst_multiple  # noqa: F401


# ---------------------------------------------------------------------------------------------------------------------------
# the operator
def as_complex(t):
    """complex128 (..., H, W) from a complex tensor or a real one with a trailing 2 (widened exactly)."""
    t = t.detach()
    if not t.is_complex():
        t = torch.view_as_complex(t.double().contiguous())
    return t.to(torch.complex128)


def forward(x):
    """F x: complex128 (..., H, W) from real x (..., H, W)."""
    return torch.fft.fft2(x.double(), norm="ortho")


def adjoint(k):
    """Re(F^H k): real fp64 (..., H, W) from complex k (..., H, W), the adjoint of `forward` as a map from real images."""
    return torch.fft.ifft2(as_complex(k), norm="ortho").real


def inv_wsum_of(weight):
    """`Inferer.restore`'s per-sample normalisation for an (N,C,H,W) k-space weight: 1 / max(sum w[n], 1)."""
    return 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0)


def _terms(x, target, weight, inv_wsum):
    """(loss (N,), resid complex) from fp64 x, complex128 target, fp64 weight / inv_wsum or None."""
    d = torch.fft.fft2(x, norm="ortho") - target
    w = torch.ones_like(x) if weight is None else weight
    inv = torch.full((x.shape[0],), 1.0 / x[0].numel(), dtype=x.dtype) if inv_wsum is None else inv_wsum
    return inv * (w * (d.real ** 2 + d.imag ** 2)).sum(dim=(1, 2, 3)), w * d


def objective(x, target, weight=None, inv_wsum=None):
    """(loss (N,), grad_x, resid complex128 (N,C,H,W)) in fp64 from inputs of any float dtype (widened exactly)."""
    d = lambda t: None if t is None else t.detach().double()
    xl = d(x).requires_grad_(True)
    with torch.enable_grad():
        loss, resid = _terms(xl, as_complex(target), d(weight), d(inv_wsum))
        g, = torch.autograd.grad(loss.sum(), [xl])
    return loss.detach(), g, resid.detach()


# ---------------------------------------------------------------------------------------------------------------------------
# cases and inputs of tests/test_gpu_fourier.py: (C, H, W) -- one stage; H != W both ways; a column tile of 32 with a row tile of
# several rows; the headline plane; the longest row and column against the shortest; the plane that does not fit in LDS (column
# tiles of 16, row tiles of 8 rows)
SHAPES = ((1, 2, 2), (3, 4, 8), (3, 8, 4), (2, 16, 64), (3, 64, 64), (1, 256, 2), (1, 2, 256), (1, 256, 256))
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
BATCHES = (1, 3, 5)
# the kernels block over nothing but planes (one workgroup works on one plane of one sample; the grid is linear in N), so there is no
# sample block to exceed; a batch of 67 at a small shape still runs a grid of several hundred workgroups
LARGE_BATCH, LARGE_BATCH_SHAPE = 67, (3, 4, 8)
WEIGHTS = ("mask", "real", "ones")


def batches_of(shape):
    return BATCHES + ((LARGE_BATCH,) if tuple(shape) == LARGE_BATCH_SHAPE else ())


def objective_inputs(n, shape, weights, seed=0):
    """(x, target, weight, inv_wsum) as fp32 tensors (target complex64): an image in [0, 1), a measurement F x' of another image
    plus noise, and ``weights`` = "mask" (a 0/1 mask with about a third set and `inv_wsum_of` it), "real" (weights in [0, 1) with
    every seventh an exact zero) or "ones" (None, None: all ones and the kernel's own 1 / (C H W))."""
    g = torch.Generator().manual_seed(6000 + seed)
    full = (n,) + tuple(shape)
    x = torch.rand(full, generator=g)
    t = forward(torch.rand(full, generator=g)) + 0.1 * torch.complex(torch.randn(full, generator=g, dtype=torch.float64),
                                                                      torch.randn(full, generator=g, dtype=torch.float64))
    target = t.to(torch.complex64)
    if weights == "ones":
        return x, target, None, None
    if weights == "mask":
        weight = (torch.rand(full, generator=g) < 1.0 / 3.0).float()
    else:
        weight = torch.rand(full, generator=g)
        weight.view(-1)[::7] = 0.0
    return x, target, weight, inv_wsum_of(weight)


# ---------------------------------------------------------------------------------------------------------------------------
# the bound
ETA = (1.0 + 4.0 * math.sqrt(2.0)) * U      # one radix-2 stage, first order (below)


def transform_bound(x_norm, stages):
    """The bound on |fl(T x)[k] - (T x)[k]| for every output k of an UNNORMALISED radix-2 transform of ``stages`` stages applied in
    fp32 to data of 2-norm ``x_norm``, divided by the transform's own gain sqrt(L) (so: in the unitary scale).

    One stage multiplies by a butterfly factor A_s, ||A_s||_2 = sqrt(2), whose entries are 1 and twiddles.  A stored twiddle is the
    fp64 value rounded once to fp32 in each component: |w^ - w| <= u.  A complex product in fp32 (four products, two sums, no
    fused multiply-add) errs by at most sqrt(2) gamma_2 |w| |b|, a complex sum by u |a + b|; together one stage commits a relative
    error, in the 2-norm of its output, of at most eta = mu + gamma_4 (sqrt(2) + mu) with mu = u (N. J. Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., Theorem 24.2 and its proof), to first order (1 + 4 sqrt(2)) u.  The argument is
    per stage and in norms: it holds for decimation in time and in frequency, for the conjugate twiddles, and for any order of the
    butterflies inside a stage.  After t stages ||y^ - y||_2 <= t eta ||y||_2 = t eta sqrt(L) ||x||_2, and no single element errs
    by more than the norm."""
    return stages * ETA * x_norm


def bound(x, target, weight=None, inv_wsum=None):
    """(E_loss (N,), E_grad like x, E_resid real (N,C,H,W)): first-order bounds on |device - objective(...)| -- for ``resid`` on the
    MODULUS of the complex difference, hence on each of its parts -- built as `restore_oracle.bound` is: every fp32 rounding adds
    u |result| (+ FLOOR), incoming errors are carried through, the whole times 1 + 2^-10.
      X      rows then columns, log2 W + log2 H stages on the plane: the row pass errs by log2 W eta sqrt(W) ||x||_F in the plane's
             Frobenius norm, the column pass carries that (gain sqrt(H)) and adds log2 H eta sqrt(H W) ||x||_F; in the unitary scale
             (log2 H + log2 W) eta ||x||_F per element (`transform_bound`).  The scaling by float(1 / sqrt(H W)): the constant's
             rounding and the product's, 2 u |X|
      d      = X - t, r = w d: one rounding in each part; r is `resid`
      u      = (2 inv) r: one rounding (2 inv is exact), one more for the constant float(1 / (C H W)) -- the default inv_wsum --
             where it is not the oracle's exact value: u |u| twice
      grad   = scale Re(F^H u).  The transform's error in X is bounded as a VECTOR, ||e_T||_F <= T_X = (log2 H + log2 W) eta ||x||_F,
             not independently in every cell: through r = w d, u = 2 inv r and the unitary adjoint it reaches any element of the
             gradient with at most 2 inv max|w| T_X.  The cell-wise roundings (the scaling, d, r, u) are carried by their plane's
             2-norm.  Then the adjoint's own log2 H + log2 W stages on ||u||_F and its scaling, 2 u |F^H u|
      loss   fp64 products and sum.  d loss = inv sum Re(conj(e_r) d + conj(r) e_d) with e_r = w e_d + (r's rounding): the
             transform's part is at most 2 inv ||r||_F T_X per plane (Cauchy-Schwarz), the cell-wise roundings are carried cell by
             cell as in `restore_oracle.bound`; the constant and the final rounding."""
    d64 = lambda t: None if t is None else t.detach().double()
    x, w, inv = d64(x), d64(weight), d64(inv_wsum)
    t = as_complex(target)
    n, c, h, wd = x.shape
    stages = int(math.log2(h)) + int(math.log2(wd))
    w = torch.ones_like(x) if w is None else w
    inv = torch.full((n,), 1.0 / (c * h * wd), dtype=torch.float64) if inv is None else inv
    plane_norm = lambda v: (v.abs() ** 2).sum(dim=(2, 3), keepdim=True).sqrt()
    loss, g, r = objective(x, t, w, inv)
    X = forward(x)
    d = X - t
    T_X = transform_bound(plane_norm(x), stages)                      # (N,C,1,1): the transform's error, as a vector and per cell
    cell = 2.0 * U * X.abs() + U * d.abs() + 2.0 * FLOOR              # the scaling's and the subtraction's roundings, per cell
    E_d = T_X + cell
    r_cell = w.abs() * cell + U * r.abs() + FLOOR                     # r's error without the transform's part
    E_r = w.abs() * T_X + r_cell
    K = (2.0 * inv).view(-1, 1, 1, 1)
    u = K * r
    wmax = w.abs().amax(dim=(2, 3), keepdim=True)
    e_u_norm = K * (wmax * T_X + plane_norm(r_cell)) + 2.0 * (U * plane_norm(u) + FLOOR)
    G = torch.fft.ifft2(u, norm="ortho")
    E_g = e_u_norm + transform_bound(plane_norm(u), stages) + 2.0 * U * G.abs() + FLOOR
    per_plane = 2.0 * plane_norm(r) * T_X
    E_loss = inv * (per_plane.sum(dim=(1, 2, 3)) + (d.abs() * r_cell + r.abs() * cell).sum(dim=(1, 2, 3))) + 2.0 * (U * loss.abs() + FLOOR)
    return E_loss * SECOND_ORDER, E_g.expand_as(x) * SECOND_ORDER, E_r * SECOND_ORDER


def fourier2d_bound(v, h, w):
    """The bound on every element of glowhip_fourier2d's output (forward: the modulus of the complex difference) for an input ``v``
    (real, or complex for the adjoint): the stages on the plane's 2-norm and the scaling, as `bound` has them."""
    stages = int(math.log2(h)) + int(math.log2(w))
    v = v.detach()
    v = v.to(torch.complex128) if v.is_complex() else v.double()
    norm = (v.abs() ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    out = torch.fft.ifft2(v, norm="ortho") if v.is_complex() else torch.fft.fft2(v, norm="ortho")
    return (transform_bound(norm, stages) + 2.0 * U * out.abs() + FLOOR) * SECOND_ORDER


def fourier2d_norm_bound(v, h, w):
    """The same roundings bounded as a VECTOR: (..., 1, 1), the most the 2-norm of a plane's whole error can be -- the stages' term
    is a norm bound to begin with, the scaling's cell-wise roundings add their own norm."""
    stages = int(math.log2(h)) + int(math.log2(w))
    v = v.detach()
    v = v.to(torch.complex128) if v.is_complex() else v.double()
    norm = (v.abs() ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    out = torch.fft.ifft2(v, norm="ortho") if v.is_complex() else torch.fft.fft2(v, norm="ortho")
    cells = ((2.0 * U * out.abs() + FLOOR) ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    return (transform_bound(norm, stages) + cells) * SECOND_ORDER


def complex_multiple(got, ref, E):
    """`worst_multiple` for a complex result: max |got - ref| / E with | | the complex modulus."""
    diff = (as_complex(got.cpu()) - ref).abs()
    return float(torch.where(diff == 0, torch.zeros_like(diff), diff / E).max())


# ---------------------------------------------------------------------------------------------------------------------------
# the undersampling masks
def mask_band(n, center):
    """The indices of the always-sampled low frequencies of an axis of ``n`` in unshifted order: 0..c and n-c..n-1,
    c = int(center n) // 2."""
    c = int(float(center) * n) // 2
    return sorted(set(range(0, c + 1)) | set(range(n - c, n)))


# ---------------------------------------------------------------------------------------------------------------------------
# latent gradients and the fit
def latent_grads(z, eps, sd, cfg, target, weight=None, inv_wsum=None, tables=None):
    """(x, loss (N,), g_z, [g_eps]): fp64 autograd of the objective through `O.flow_decode` and the transform above."""
    d = lambda t: None if t is None else t.detach().double()
    sdd = {k: v.double() for k, v in sd.items()}
    zl = d(z).requires_grad_(True)
    el = [d(e).requires_grad_(True) for e in eps]
    with torch.enable_grad():
        x = O.flow_decode(zl, sdd, cfg, el, perm_tables=tables)
        loss, _ = _terms(x, as_complex(target), d(weight), d(inv_wsum))
        grads = torch.autograd.grad(loss.sum(), [zl] + el)
    return x.detach(), loss.detach(), grads[0], list(grads[1:])


# The k-space fit of tests/test_gpu_fourier.py, its threshold fixed by the oracle's own run in tests/test_fourier_host.py with the
# margin of tests/test_linear_host.py: the smallest of `restore_oracle.RATIO_STEPS` that is at least TWICE the oracle's worst
# final / first ratio
FIT = dict(case="tiny", fraction=0.25, kind="lines", seed=0, steps=40, lr=0.1, ratio=0.1)      # TINY_AFF: 16x16x3, 4 of 16 rows


def threshold_of(ratio):
    """The smallest of 0.1 / 0.2 / 0.5 that is at least twice ``ratio`` (None above 0.25: such a fit proves nothing)."""
    return round_up_ratio(2.0 * ratio)


def zero_filled(measurement, weight):
    """clamp(Re(F^H (w t)), 0, 1) as fp32: the start image of `Inferer.restore(..., fourier=True, init=None)`."""
    return adjoint(as_complex(measurement) * weight.double()).clamp(0.0, 1.0).float()


@functools.lru_cache(maxsize=None)
def fit_case():
    """The k-space fit on the oracle, as `Inferer.restore(kspace, weight=fourier_mask((H, W), 0.25), fourier=True)` sets it up: the
    unknown image is the decode of the case's latents, the measurement its unitary 2-D DFT (fp64, rounded to complex64), the weight
    the Cartesian mask broadcast over the batch and the channels, the start the fp32 encode of the zero-filled reconstruction.  Adam
    in fp64 (torch.optim.Adam), the data term summed over the samples; ``history`` (steps, N) holds the per-sample loss BEFORE each
    update.  Computed once per process; callers must not modify the result."""
    from pytorch_glow_amd.network.restore import fourier_mask      # (host code: a seeded generator, no compute path)
    fit = FIT
    ref = D.reference(**R.TINY_AFF)
    target = ref["x"].float()
    mask = fourier_mask(tuple(target.shape[-2:]), fit["fraction"], kind=fit["kind"], seed=fit["seed"])
    weight = mask.expand_as(target).contiguous()
    meas = forward(target).to(torch.complex64)
    start = zero_filled(meas, weight)
    with torch.no_grad():
        z0, eps0 = D.encode_latents(start, ref["sd"], ref["cfg"], ref["tables"])
    sdd = {k: v.double() for k, v in ref["sd"].items()}
    leaves = [z0.double().clone().requires_grad_(True)] + [e.double().clone().requires_grad_(True) for e in eps0]
    opt = torch.optim.Adam(leaves, lr=fit["lr"])
    t, w, inv = as_complex(meas), weight.double(), inv_wsum_of(weight).double()
    hist = []
    for _ in range(fit["steps"]):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            x = O.flow_decode(leaves[0], sdd, ref["cfg"], leaves[1:], perm_tables=ref["tables"])
            loss, _ = _terms(x, t, w, inv)
            loss.sum().backward()
        opt.step()
        hist.append(loss.detach())
    return dict(ref=ref, mask=mask, weight=weight, target=target, measurement=meas, start=start, history=torch.stack(hist), **fit)

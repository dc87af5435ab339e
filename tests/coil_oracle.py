"""fp64 restatement of the multi-coil k-space objective (csrc/restore_fourier.hip, glowhip_restore_objective_coils and
glowhip_coils2d; the definition is in include/glowhip.h) in plain torch, the bound the device's fp32 result is held to, the case tables
of tests/test_coil_host.py and tests/test_gpu_coils.py, the synthetic sensitivity maps of `network.restore.coil_maps` restated from
its docstring, and a multi-coil fit through the CPU oracle's decode.  Nothing here reads the package's compute path.

Per sample n and image channel c, Q coils with complex sensitivity maps S[q] (H x W), F the unitary 2-D DFT of `fourier_oracle`:
    Y[n,c,q] = F (S[q] x[n,c])      resid = w[n,c] (Y - t)      loss[n] = inv_wsum[n] sum_{c,q,k} w |Y - t|^2
    grad_x = d (sum_n loss[n]) / d x   (autograd)   = 2 inv_wsum[n] sum_q Re(conj(S[q]) F^H resid[n,c,q])
``target`` is complex (N,C,Q,H,W) (or real with a trailing 2), ``maps`` complex (Q,H,W) -- shared by the batch -- or (N,Q,H,W),
``weight`` real (N,C,H,W), shared by the coils; ``weight=None`` is all ones, ``inv_wsum=None`` is 1 / (C Q H W)."""
import functools
import math

import torch

from oracle import glow_oracle as O

import decode_grad_oracle as D
import fourier_oracle as F
import restore_oracle as R
from fourier_oracle import ETA, FLOOR, SECOND_ORDER, U, as_complex, complex_multiple, threshold_of, transform_bound, worst_multiple  # noqa: F401


# ---------------------------------------------------------------------------------------------------------------------------
# the operator
def maps_of(maps):
    """complex128 (1 or N, 1, Q, H, W): the maps broadcast against (N, C, Q, H, W)."""
    s = as_complex(maps)
    return s.unsqueeze(0).unsqueeze(0) if s.dim() == 3 else s.unsqueeze(1)


def forward(x, maps):
    """F (S x): complex128 (N,C,Q,H,W) from real x (N,C,H,W)."""
    return torch.fft.fft2(maps_of(maps) * x.double().unsqueeze(2), norm="ortho")


def adjoint(k, maps):
    """sum_q Re(conj(S_q) F^H k_q): real fp64 (N,C,H,W) from complex k (N,C,Q,H,W), the adjoint of `forward` as a map from real
    images."""
    return (maps_of(maps).conj() * torch.fft.ifft2(as_complex(k), norm="ortho")).real.sum(dim=2)


def inv_wsum_of(weight, q):
    """`Inferer.restore`'s per-sample normalisation with ``q`` coils for an (N,C,H,W) k-space weight: 1 / max(q sum w[n], 1)."""
    return 1.0 / (float(q) * weight.sum(dim=(1, 2, 3))).clamp(min=1.0)


def _terms(x, target, maps, weight, inv_wsum):
    """(loss (N,), resid complex (N,C,Q,H,W)) from fp64 x, complex128 target and maps (`maps_of`), fp64 weight / inv_wsum or None."""
    d = torch.fft.fft2(maps * x.unsqueeze(2), norm="ortho") - target
    w = torch.ones_like(x) if weight is None else weight
    w = w.unsqueeze(2)
    inv = torch.full((x.shape[0],), 1.0 / d[0].numel(), dtype=x.dtype) if inv_wsum is None else inv_wsum
    return inv * (w * (d.real ** 2 + d.imag ** 2)).sum(dim=(1, 2, 3, 4)), w * d


def objective(x, target, maps, weight=None, inv_wsum=None):
    """(loss (N,), grad_x, resid complex128 (N,C,Q,H,W)) in fp64 from inputs of any float dtype (widened exactly)."""
    d = lambda t: None if t is None else t.detach().double()
    xl = d(x).requires_grad_(True)
    with torch.enable_grad():
        loss, resid = _terms(xl, as_complex(target), maps_of(maps), d(weight), d(inv_wsum))
        g, = torch.autograd.grad(loss.sum(), [xl])
    return loss.detach(), g, resid.detach()


# ---------------------------------------------------------------------------------------------------------------------------
# the sensitivity maps of `network.restore.coil_maps`, restated from its docstring with scalar arithmetic
def maps_formula(hw, q, width=0.6, seed=0):
    """complex128 (Q,H,W): pixel (i, j) at y = (i + 0.5) / H - 0.5, x = (j + 0.5) / W - 0.5; coil k at angle 2 pi (k + r) / Q on the
    circle of radius 0.6; a Gaussian magnitude of std ``width`` around that point; the phase 2 pi (f_k y + g_k x) + p_k; the draws
    r, f, g, p in that order from one seeded generator (fp64; f, g in [-0.5, 0.5), p in [0, 2 pi)); normalised so that
    sum_q |S_q|^2 = 1 at every pixel."""
    h, w = hw
    gen = torch.Generator().manual_seed(int(seed))
    r = float(torch.rand(1, generator=gen, dtype=torch.float64))
    f = (torch.rand(q, generator=gen, dtype=torch.float64) - 0.5).tolist()
    g = (torch.rand(q, generator=gen, dtype=torch.float64) - 0.5).tolist()
    p = (2.0 * math.pi * torch.rand(q, generator=gen, dtype=torch.float64)).tolist()
    out = torch.zeros((q, h, w), dtype=torch.complex128)
    for k in range(q):
        a = 2.0 * math.pi * (k + r) / q
        cy, cx = 0.6 * math.sin(a), 0.6 * math.cos(a)
        for i in range(h):
            y = (i + 0.5) / h - 0.5
            for j in range(w):
                x = (j + 0.5) / w - 0.5
                mag = math.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * width ** 2))
                ph = 2.0 * math.pi * (f[k] * y + g[k] * x) + p[k]
                out[k, i, j] = complex(mag * math.cos(ph), mag * math.sin(ph))
    return out / (out.abs() ** 2).sum(dim=0, keepdim=True).sqrt()


# ---------------------------------------------------------------------------------------------------------------------------
# cases and inputs of tests/test_gpu_coils.py: (C, Q, H, W) -- one stage; two coils on it; H != W both ways with odd coil counts; a
# column tile of 32 with a row tile of several rows; the headline plane with 8 coils; the largest Q; the longest column and row
# against the shortest; the plane that does not fit in LDS (column tiles of 16, row tiles of 8 rows)
CASES = ((1, 1, 2, 2), (1, 2, 2, 2), (3, 3, 4, 8), (2, 5, 8, 4), (2, 4, 16, 64), (1, 8, 64, 64), (1, 32, 4, 4), (1, 2, 256, 2),
         (1, 2, 2, 256), (1, 2, 256, 256))
CASE_IDS = ["x".join(map(str, s)) for s in CASES]
BATCHES = (1, 3, 5)
LARGE_BATCH, LARGE_BATCH_CASE = 67, (3, 3, 4, 8)      # (the kernels block over planes only: `fourier_oracle.LARGE_BATCH`)
WEIGHTS = F.WEIGHTS
PROPERTY_CASES = ((3, 3, 4, 8), (1, 8, 64, 64), (1, 2, 256, 256))
PROPERTY_IDS = ["x".join(map(str, s)) for s in PROPERTY_CASES]


def batches_of(case):
    return BATCHES + ((LARGE_BATCH,) if tuple(case) == LARGE_BATCH_CASE else ())


def case_maps(case, n=None, seed=0):
    """complex64 maps of a case: `coil_maps` where the plane is at least 4 x 4, a seeded complex normal otherwise; (Q,H,W), or
    (n,Q,H,W) -- ``n`` different sets -- when ``n`` is given."""
    from pytorch_glow_amd.network.restore import coil_maps      # (host code: a seeded generator, no compute path)
    c, q, h, w = case
    def one(s):
        if h >= 4 and w >= 4:
            return coil_maps((h, w), q, seed=s)
        g = torch.Generator().manual_seed(9000 + s)
        return torch.complex(torch.randn((q, h, w), generator=g), torch.randn((q, h, w), generator=g)).to(torch.complex64)
    return one(seed) if n is None else torch.stack([one(seed + 1 + k) for k in range(n)])


def objective_inputs(n, case, weights, seed=0, per_sample=False):
    """(x, target, maps, weight, inv_wsum) as fp32 / complex64 tensors: an image in [0, 1), `case_maps`, a measurement F (S x') of
    another image plus noise, and ``weights`` as in `fourier_oracle.objective_inputs` on (N,C,H,W), with `inv_wsum_of`."""
    c, q, h, w = case
    g = torch.Generator().manual_seed(7000 + seed)
    full = (n, c, h, w)
    maps = case_maps(case, n if per_sample else None, seed)
    x = torch.rand(full, generator=g)
    kshape = (n, c, q, h, w)
    t = forward(torch.rand(full, generator=g), maps) + 0.1 * torch.complex(torch.randn(kshape, generator=g, dtype=torch.float64),
                                                                            torch.randn(kshape, generator=g, dtype=torch.float64))
    target = t.to(torch.complex64)
    if weights == "ones":
        return x, target, maps, None, None
    if weights == "mask":
        weight = (torch.rand(full, generator=g) < 1.0 / 3.0).float()
    else:
        weight = torch.rand(full, generator=g)
        weight.view(-1)[::7] = 0.0
    return x, target, maps, weight, inv_wsum_of(weight, q)


# ---------------------------------------------------------------------------------------------------------------------------
# the bound
def bound(x, target, maps, weight=None, inv_wsum=None):
    """(E_loss (N,), E_grad like x, E_resid real (N,C,Q,H,W)): first-order bounds on |device - objective(...)| -- for ``resid`` on the
    MODULUS of the complex difference -- derived as `fourier_oracle.bound` is (every fp32 rounding adds u |result| (+ FLOOR),
    incoming errors are carried through, the whole times 1 + 2^-10), coil plane by coil plane, with the roundings that are new:
      z      = S_q x, the row pass's input: (S.re x, S.im x), one rounding in each part, u |S_q x| per cell and, as a vector,
             u ||S_q x||_F, which the unitary transform carries whole into any coefficient
      Y      rows then columns, log2 W + log2 H stages, now on the plane S_q x: (log2 H + log2 W) eta ||S_q x||_F
             (`fourier_oracle.transform_bound`).  Together T_Y = ((log2 H + log2 W) eta + u) ||S_q x||_F, a bound on the 2-norm of
             the coil plane's whole error and so on every cell.  The scaling by float(1 / sqrt(H W)): 2 u |Y|
      d, r, u_q = (2 inv) r as there, with the weight of plane (n, c) on every coil; the default inv_wsum is float(1 / (C Q H W))
      G_q    = F^H u_q: as there, its whole error is a VECTOR of 2-norm at most
             V_q = 2 inv (max|w| T_Y + ||r's cell-wise roundings||_F) + 2 (u ||u_q||_F + FLOOR) + (log2 H + log2 W) eta ||u_q||_F
             (the kernel keeps G unscaled until after the coil sum; the scaling is linear, so relative errors are the same)
      term_q = Re(conj(S_q) G_q) = S.re G.re + S.im G.im: G's error reaches it with at most max|S_q| V_q (each coil's transform
             error is carried as a vector through conj(S) with max|S|); two products and a sum in fp32 add
             gamma_2 (|S.re G.re| + |S.im G.im|), gamma_2 = 2 u to first order
      grad   = scale sum_q term_q, the sum in fp32 registers in coil order from an exact zero: Q - 1 rounded additions, at most
             (Q - 1) u sum_q |term_q| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4); the scaling,
             2 u |grad|
      loss   as there, over the C Q planes of the sample: 2 inv ||r||_F T_Y per plane (Cauchy-Schwarz) and the cell-wise roundings
             cell by cell; the constant and the final rounding.
    No constant comes from a device run."""
    d64 = lambda t: None if t is None else t.detach().double()
    x, w, inv = d64(x), d64(weight), d64(inv_wsum)
    t = as_complex(target)
    S = maps_of(maps)
    n, c, h, wd = x.shape
    q = S.shape[2]
    stages = int(math.log2(h)) + int(math.log2(wd))
    w = torch.ones_like(x) if w is None else w
    inv = torch.full((n,), 1.0 / (c * q * h * wd), dtype=torch.float64) if inv is None else inv
    plane_norm = lambda v: (v.abs() ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    loss, g, r = objective(x, t, maps, w, inv)
    w5 = w.unsqueeze(2)                                                # (N,C,1,H,W)
    z = S * x.unsqueeze(2)                                             # (N,C,Q,H,W)
    Y = torch.fft.fft2(z, norm="ortho")
    d = Y - t
    T_Y = transform_bound(plane_norm(z), stages) + U * plane_norm(z)    # (N,C,Q,1,1)
    cell = 2.0 * U * Y.abs() + U * d.abs() + 2.0 * FLOOR
    r_cell = w5.abs() * cell + U * r.abs() + FLOOR
    E_r = w5.abs() * T_Y + r_cell
    K = (2.0 * inv).view(-1, 1, 1, 1, 1)
    u = K * r
    wmax = w5.abs().amax(dim=(-2, -1), keepdim=True)
    V = K * (wmax * T_Y + plane_norm(r_cell)) + 2.0 * (U * plane_norm(u) + FLOOR) + transform_bound(plane_norm(u), stages)
    G = torch.fft.ifft2(u, norm="ortho")
    smax = S.abs().amax(dim=(-2, -1), keepdim=True).expand(n, 1, q, 1, 1)
    products = (S.real * G.real).abs() + (S.imag * G.imag).abs()
    terms = (S.real * G.real + S.imag * G.imag).abs()
    E_g = (smax * V + 2.0 * U * products).sum(dim=2) + (q - 1) * U * terms.sum(dim=2) + 2.0 * U * g.abs() + FLOOR
    per_plane = 2.0 * plane_norm(r) * T_Y
    E_loss = inv * (per_plane.sum(dim=(1, 2, 3, 4)) + (d.abs() * r_cell + r.abs() * cell).sum(dim=(1, 2, 3, 4))) + 2.0 * (U * loss.abs() + FLOOR)
    return E_loss * SECOND_ORDER, E_g * SECOND_ORDER, E_r * SECOND_ORDER


def coils2d_bound(v, maps, h, w):
    """The bound on every element of glowhip_coils2d's output for an input ``v``: real (N,C,H,W) for the forward direction (the
    modulus of the complex difference, (N,C,Q,H,W)), complex (N,C,Q,H,W) for the adjoint (real, (N,C,H,W)) -- the roundings of
    `bound` that the operator alone has."""
    stages = int(math.log2(h)) + int(math.log2(w))
    S = maps_of(maps)
    plane_norm = lambda t: (t.abs() ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    v = v.detach()
    if not v.is_complex():
        z = S * v.double().unsqueeze(2)
        out = torch.fft.fft2(z, norm="ortho")
        return (transform_bound(plane_norm(z), stages) + U * plane_norm(z) + 2.0 * U * out.abs() + FLOOR) * SECOND_ORDER
    k = as_complex(v)
    q = k.shape[2]
    G = torch.fft.ifft2(k, norm="ortho")
    smax = S.abs().amax(dim=(-2, -1), keepdim=True).expand(k.shape[0], 1, q, 1, 1)
    products = (S.real * G.real).abs() + (S.imag * G.imag).abs()
    terms = (S.real * G.real + S.imag * G.imag).abs()
    out = adjoint(k, maps)
    return ((smax * transform_bound(plane_norm(k), stages) + 2.0 * U * products).sum(dim=2) + (q - 1) * U * terms.sum(dim=2)
            + 2.0 * U * out.abs() + FLOOR) * SECOND_ORDER


def coils2d_norm_bound(v, maps, h, w):
    """`coils2d_bound` as a VECTOR: (N,C,1,1), the most the 2-norm of the whole error of one image channel's output (all its coil
    planes, forward; its one plane, adjoint) can be: the square root of the sum of the squared element bounds."""
    E = coils2d_bound(v, maps, h, w)
    dims = (-3, -2, -1) if E.dim() == 5 else (-2, -1)
    out = (E ** 2).sum(dim=dims).sqrt()
    return out.view(out.shape[0], out.shape[1], 1, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# latent gradients and the fit
def latent_grads(z, eps, sd, cfg, target, maps, weight=None, inv_wsum=None, tables=None):
    """(x, loss (N,), g_z, [g_eps]): fp64 autograd of the objective through `O.flow_decode` and the operator above."""
    d = lambda t: None if t is None else t.detach().double()
    sdd = {k: v.double() for k, v in sd.items()}
    zl = d(z).requires_grad_(True)
    el = [d(e).requires_grad_(True) for e in eps]
    with torch.enable_grad():
        x = O.flow_decode(zl, sdd, cfg, el, perm_tables=tables)
        loss, _ = _terms(x, as_complex(target), maps_of(maps), d(weight), d(inv_wsum))
        grads = torch.autograd.grad(loss.sum(), [zl] + el)
    return x.detach(), loss.detach(), grads[0], list(grads[1:])


# The multi-coil fit of tests/test_gpu_coils.py, its threshold fixed by the oracle's own run in tests/test_coil_host.py with the margin
# of tests/test_linear_host.py: the smallest of `restore_oracle.RATIO_STEPS` that is at least TWICE the oracle's worst final / first
# ratio.  TINY_AFF: 16x16x3, 4 of 16 k-space rows, 4 coils
FIT = dict(case="tiny", fraction=0.25, kind="lines", seed=0, coils=4, coil_seed=0, steps=40, lr=0.1, ratio=0.1)


def zero_filled(measurement, maps, weight):
    """clamp(sum_q Re(conj(S_q) F^H (w t_q)), 0, 1) as fp32: the start image of `Inferer.restore(..., fourier=True, coils=maps,
    init=None)`, with normalised maps the coil-combined zero-filled reconstruction."""
    return adjoint(as_complex(measurement) * weight.double().unsqueeze(2), maps).clamp(0.0, 1.0).float()


@functools.lru_cache(maxsize=None)
def fit_case():
    """The multi-coil fit on the oracle, as `Inferer.restore(kspace, weight=fourier_mask((H, W), 0.25), fourier=True,
    coils=coil_maps((H, W), 4))` sets it up: the unknown image is the decode of the case's latents, the measurement F (S x) of it
    (fp64, rounded to complex64), the weight the Cartesian mask broadcast over the batch and the channels, inv_wsum
    1 / max(Q sum w, 1), the start the fp32 encode of the coil-combined zero-filled image.  Adam in fp64 (torch.optim.Adam), the
    data term summed over the samples; ``history`` (steps, N) holds the per-sample loss BEFORE each update.  Computed once per
    process; callers must not modify the result."""
    from pytorch_glow_amd.network.restore import coil_maps, fourier_mask      # (host code: seeded generators, no compute path)
    fit = FIT
    ref = D.reference(**R.TINY_AFF)
    target = ref["x"].float()
    hw = tuple(target.shape[-2:])
    mask = fourier_mask(hw, fit["fraction"], kind=fit["kind"], seed=fit["seed"])
    maps = coil_maps(hw, fit["coils"], seed=fit["coil_seed"])
    weight = mask.expand_as(target).contiguous()
    meas = forward(target, maps).to(torch.complex64)
    start = zero_filled(meas, maps, weight)
    with torch.no_grad():
        z0, eps0 = D.encode_latents(start, ref["sd"], ref["cfg"], ref["tables"])
    sdd = {k: v.double() for k, v in ref["sd"].items()}
    leaves = [z0.double().clone().requires_grad_(True)] + [e.double().clone().requires_grad_(True) for e in eps0]
    opt = torch.optim.Adam(leaves, lr=fit["lr"])
    t, S, w, inv = as_complex(meas), maps_of(maps), weight.double(), inv_wsum_of(weight, fit["coils"]).double()
    hist = []
    for _ in range(fit["steps"]):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            x = O.flow_decode(leaves[0], sdd, ref["cfg"], leaves[1:], perm_tables=ref["tables"])
            loss, _ = _terms(x, t, S, w, inv)
            loss.sum().backward()
        opt.step()
        hist.append(loss.detach())
    return dict(ref=ref, mask=mask, maps=maps, weight=weight, target=target, measurement=meas, start=start, history=torch.stack(hist),
                **fit)

"""Inverse problems under the flow prior, on the device: in-painting, denoising, super-resolution, projection onto the model.

A trained flow is a prior over images; a maximum-a-posteriori fit of its latents to a measurement minimises

    sum_n  inv_wsum[n] * sum w (P decode(latents)_n - t_n)^2   +   prior_weight * 1/2 ||latents||^2

with P the pool x pool average pool (pool = 1: a mask problem, pool > 1: super-resolution), t the measurement and w its weights.
The pieces: `restore_objective` (glowhip_restore_objective, csrc/restore.hip: the data term's per-sample loss and its gradient with
respect to the image, one launch), `FlowPlan.decode` / `decode_vjp` (the image and J^T of that gradient) and the fused Adam step
(`training.HipAdam`), whose weight decay IS the prior term: the update kernel adds prior_weight * p to the gradient, the gradient of
prior_weight * 1/2 ||p||^2.  `LatentFit` runs them as a device-resident loop -- no autograd, no host sync, the histories on the
device -- and, with ``graph=True``, as one hipGraph launch per iteration.

Deblurring: with a point-spread function ``psf`` the decode is observed through A = P B, B the zero-padded convolution by the PSF
(glowhip_restore_objective_psf; include/glowhip.h has the definition).  Only `LatentLoop._evaluate` knows: decode, `decode_vjp`,
the optimiser, the MALA launches, the capture protocol and the histories are the same with and without one.

Compressed sensing: with a dense ``operator`` A of shape (M, C, H, W) the measurement is (N, M), t = A x + noise with x the flattened
decode (glowhip_restore_objective_linear, csrc/restore_linear.hip; `gaussian_operator` makes the standard i.i.d. N(0, 1/M) matrix on
the device from the sampler's stream 248).  Again only `LatentLoop._evaluate` knows.

Blind deblurring: with ``estimate_psf`` the PSF is one more unknown of the fit, ``psf = softmax(theta)``; the new quantity is the
gradient of the data term with respect to the taps, a cross-correlation of the decoded image with the residual the objective leaves
behind (glowhip_restore_psf_grad, csrc/restore_blind.hip; `psf_gradient`, `psf_from_logits`).  `PsfLogits` holds theta and its own
fused Adam step; `LatentFit` runs it inside the same captured iteration, `PsfFit` without the flow (calibration).

Fourier-domain measurements: with ``fourier=True`` the measurement is the unitary 2-D DFT of each channel's plane, complex
(N,C,H,W), and ``weight`` the k-space mask (glowhip_restore_objective_fourier, csrc/restore_fourier.hip: a separable radix-2 FFT in
LDS; sides are powers of two up to 256).  `fourier2d` / `fourier2d_adjoint` are the transform alone, `fourier_mask` the usual
undersampling masks.  Again only `LatentLoop._evaluate` knows.

Multi-coil k-space: with ``fourier=True, coils=maps`` the measurement is complex (N,C,Q,H,W), the decode seen by Q receive coils
through complex sensitivity maps, Y[c,q] = F (S_q x_c) (glowhip_restore_objective_coils, the same file).  `coils2d` /
`coils2d_adjoint` are the operator alone, `coil_maps` smooth synthetic maps."""
import contextlib
import math
from dataclasses import dataclass
from typing import Optional

import torch

from .. import _lib
from .._capture import Capture
from ..training import HipAdam, HyperRing
from .latents import Latents


PSF_MAX = 15       # the largest side of a point-spread function (csrc/restore.hip)


def check_psf_shape(shape, n, what="psf"):
    """``(kh, kw)`` of a PSF of shape (kh,kw) or (n,kh,kw): both sides odd and at most `PSF_MAX`; ValueError otherwise."""
    shape = tuple(shape)
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[0] != n):
        raise ValueError(f"{what} of shape {shape}: expected (kh, kw) or ({n}, kh, kw)")
    kh, kw = shape[-2:]
    if not all(1 <= k <= PSF_MAX and k % 2 == 1 for k in (kh, kw)):
        raise ValueError(f"{what} of {kh} x {kw} taps: both sides must be odd and at most {PSF_MAX}")
    return kh, kw


def psf_valid_weight(meas_shape, kh, kw, pool=1):
    """The band mask of ``border="valid"`` as a CPU fp32 tensor of the measurement's last two dimensions (h, w): 1 where every x the
    cell's footprint reads -- its pool x pool patch widened by (kh-1)/2 rows and (kw-1)/2 columns on each side -- lies inside the
    image, 0 elsewhere: ceil(ah / pool) rows at the top and at the bottom, ceil(aw / pool) columns at the left and at the right."""
    h, w = (int(v) for v in tuple(meas_shape)[-2:])
    pool = int(pool)
    rh, rw = -(-((kh - 1) // 2) // pool), -(-((kw - 1) // 2) // pool)
    m = torch.zeros((h, w), dtype=torch.float32)
    if h > 2 * rh and w > 2 * rw:
        m[rh:h - rh, rw:w - rw] = 1.0
    return m


OPERATOR_STREAM = 248      # the sampler stream that names a Gaussian sensing matrix (include/glowhip.h: the stream table)


def check_operator_shape(shape, image_shape=None, what="operator"):
    """``(M, D)`` of an operator of shape (M, C, H, W); ``image_shape`` (C, H, W): the image it must observe.  ValueError otherwise."""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f"{what} of shape {shape}: expected (M, C, H, W)")
    if image_shape is not None and shape[1:] != tuple(int(v) for v in image_shape):
        raise ValueError(f"{what} of shape {shape} does not observe images of shape {tuple(image_shape)}")
    return shape[0], shape[1] * shape[2] * shape[3]


def linear_scratch(n, m, d, device):
    """The scratch of glowhip_restore_objective_linear for a batch of ``n``: a uint8 device tensor of
    glowhip_restore_linear_scratch_bytes(n, m, d) bytes."""
    need = int(_lib.lib().glowhip_restore_linear_scratch_bytes(int(n), int(m), int(d)))
    if need == 0:
        _lib.check(-1)
    return torch.empty(need, dtype=torch.uint8, device=device)


def gaussian_operator(m, image_shape, seed, device):
    """The standard compressed-sensing matrix, i.i.d. N(0, 1/m), as an (m, C, H, W) fp32 tensor made ON the device: stream 248 of
    the sampler's generator at ``(seed, call = 0)``, element = flat index, times ``float32(1 / sqrt(m))`` (glowhip_normal_noise).
    The matrix is named by ``(m, image_shape, seed)``: it never crosses PCIe, and tests/linear_oracle.py restates it on the CPU."""
    m = int(m)
    shape = (m,) + tuple(int(v) for v in image_shape)
    check_operator_shape(shape)
    out = torch.empty(shape, dtype=torch.float32, device=device)
    std = float(torch.tensor(1.0 / math.sqrt(m), dtype=torch.float32))
    _lib.check(_lib.lib().glowhip_normal_noise(_lib.ptr(out), out.numel(), int(seed) & (2 ** 64 - 1), 0, OPERATOR_STREAM, std,
                                               _lib.stream_ptr(out.device)))
    return out


FOURIER_MAX = 256      # the largest side of a Fourier-domain problem (csrc/restore_fourier.hip)


def check_fourier_shape(hw, what="fourier"):
    """``(H, W)`` of a plane the transform takes: each side a power of two from 2 to `FOURIER_MAX`; ValueError otherwise."""
    hw = tuple(int(v) for v in tuple(hw)[-2:])
    if len(hw) != 2 or not all(2 <= v <= FOURIER_MAX and v & (v - 1) == 0 for v in hw):
        raise ValueError(f"{what}: a plane of {' x '.join(map(str, hw))}: each side must be a power of two from 2 to {FOURIER_MAX}")
    return hw


def fourier_mask(hw, fraction, kind="lines", center=0.08, seed=0):
    """An (H, W) 0/1 fp32 undersampling mask in UNSHIFTED k-space (index 0 is DC), made on the host from a generator seeded with
    ``seed``.  ``"lines"``: the Cartesian MRI mask -- whole rows; the lowest ``center * H`` row frequencies, rows 0..c and
    H-c..H-1 with c = int(center * H) // 2, are always there, and further rows drawn uniformly without replacement bring the count
    to ``round(fraction * H)`` (the band alone where it is already more).  ``"points"``: the same with single coefficients -- the
    block |u| <= int(center * H) // 2, |v| <= int(center * W) // 2, then uniformly drawn coefficients up to
    ``round(fraction * H * W)``.  ``fraction=1`` is all ones."""
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1 or not 0.0 < float(fraction) <= 1.0 or not 0.0 <= float(center) <= 1.0 or kind not in ("lines", "points"):
        raise ValueError(f"fourier_mask: hw {tuple(hw)}, fraction {fraction!r} in (0, 1], center {center!r} in [0, 1], kind {kind!r} 'lines' or 'points'")
    gen = torch.Generator().manual_seed(int(seed))
    low = lambda n: torch.minimum(torch.arange(n), n - torch.arange(n)) <= int(float(center) * n) // 2      # |frequency| <= c
    if kind == "lines":
        chosen, total = low(h), h
    else:
        chosen, total = (low(h).view(h, 1) & low(w).view(1, w)).reshape(-1), h * w
    want = int(round(float(fraction) * total))
    rest = (~chosen).nonzero().view(-1)
    more = max(0, min(want - int(chosen.sum()), rest.numel()))
    chosen = chosen.clone()
    chosen[rest[torch.randperm(rest.numel(), generator=gen)[:more]]] = True
    mask = chosen.view(h, 1).expand(h, w) if kind == "lines" else chosen.view(h, w)
    return mask.to(torch.float32).contiguous()


def fourier_scratch(n, c, h, w, device):
    """The scratch of glowhip_restore_objective_fourier for a batch of ``n`` images (c, h, w): a uint8 device tensor of
    glowhip_restore_fourier_scratch_bytes(n, c, h, w) bytes."""
    need = int(_lib.lib().glowhip_restore_fourier_scratch_bytes(int(n), int(c), int(h), int(w)))
    if need == 0:
        _lib.check(-1)
    return torch.empty(need, dtype=torch.uint8, device=device)


def as_kspace(k, what="measurement"):
    """``k`` -- complex64 (..., H, W) or fp32 (..., H, W, 2) -- as its fp32 view (..., H, W, 2), the memory of
    `torch.view_as_real`; ValueError for anything else."""
    if not torch.is_tensor(k):
        raise TypeError(f"{what}: a tensor, complex64 (..., H, W) or fp32 (..., H, W, 2)")
    if k.is_complex():
        if k.dtype != torch.complex64:
            raise ValueError(f"{what}: complex64, not {k.dtype}")
        return torch.view_as_real(k.contiguous())
    if k.dtype != torch.float32 or k.dim() < 3 or k.shape[-1] != 2:
        raise ValueError(f"{what} of shape {tuple(k.shape)} and dtype {k.dtype}: complex64 (..., H, W) or fp32 (..., H, W, 2)")
    return k


def fourier2d(x, out=None):
    """The unitary 2-D DFT of the last two dimensions of a real fp32 device tensor ``x`` (..., H, W), as complex64 (..., H, W):
    `torch.fft.fft2(x, norm="ortho")` by glowhip_fourier2d (unshifted, index (0,0) the DC term).  ``out``: an fp32 buffer
    (..., H, W, 2) to write."""
    x = _lib.require_device_tensor(x, "x")
    if x.dim() < 2:
        raise ValueError(f"fourier2d: x of shape {tuple(x.shape)}")
    h, w = check_fourier_shape(x.shape, "fourier2d")
    real = torch.empty(tuple(x.shape) + (2,), dtype=torch.float32, device=x.device) if out is None else out
    if not (real.is_cuda and real.dtype == torch.float32 and real.is_contiguous() and tuple(real.shape) == tuple(x.shape) + (2,)):
        raise _lib.GlowHipError("fourier2d: out must be a contiguous fp32 device tensor of the shape of x with a trailing 2")
    _lib.check(_lib.lib().glowhip_fourier2d(_lib.ptr(x), _lib.ptr(real), x.numel() // (h * w), h, w, 0, _lib.stream_ptr(x.device)))
    return torch.view_as_complex(real)


def fourier2d_adjoint(k, out=None):
    """``Re(F^H k)``, real fp32 (..., H, W), of a device tensor ``k``, complex64 (..., H, W) or fp32 (..., H, W, 2): the adjoint of
    `fourier2d` as a map from real images (glowhip_fourier2d with adjoint = 1) -- the zero-filled reconstruction when ``k`` is a
    masked measurement.  ``out``: the fp32 buffer to write."""
    real = _lib.require_device_tensor(as_kspace(k, "k"), "k")
    if real.dim() < 3:
        raise ValueError(f"fourier2d_adjoint: k of shape {tuple(k.shape)}")
    h, w = check_fourier_shape(real.shape[:-1], "fourier2d_adjoint")
    x = torch.empty(real.shape[:-1], dtype=torch.float32, device=real.device) if out is None else out
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == tuple(real.shape[:-1])):
        raise _lib.GlowHipError("fourier2d_adjoint: out must be a contiguous fp32 device tensor of the shape of k")
    _lib.check(_lib.lib().glowhip_fourier2d(_lib.ptr(real), _lib.ptr(x), x.numel() // (h * w), h, w, 1, _lib.stream_ptr(x.device)))
    return x


COILS_MAX = 32      # the most receive coils of a multi-coil k-space problem (csrc/restore_fourier.hip)


def check_coil_maps(maps, n, hw):
    """The coil sensitivity maps of a multi-coil problem as their fp32 view: ``maps`` is complex64 (Q,H,W) -- shared by the batch --
    or (N,Q,H,W) -- per sample -- or fp32 with a trailing 2; returns ``(fp32 view (..., Q, H, W, 2), Q, per_sample)``.  ValueError for
    another dtype or rank, a plane other than ``hw``, a batch other than ``n``, Q outside 1..`COILS_MAX`.  No device work."""
    real = as_kspace(maps, "coils")
    h, w = (int(v) for v in tuple(hw)[-2:])
    if real.dim() not in (4, 5) or tuple(real.shape[-3:-1]) != (h, w):
        raise ValueError(f"coils of shape {tuple(maps.shape)}: expected complex (Q, {h}, {w}) or (N, Q, {h}, {w}), or fp32 with a trailing 2")
    q, per_sample = int(real.shape[-4]), real.dim() == 5
    if not 1 <= q <= COILS_MAX:
        raise ValueError(f"coils: {q} coils; from 1 to {COILS_MAX}")
    if per_sample and int(real.shape[0]) != int(n):
        raise ValueError(f"coils of shape {tuple(maps.shape)}: per-sample maps for a batch of {n}")
    return real, q, per_sample


def coil_maps(hw, q, width=0.6, seed=0):
    """Smooth synthetic coil sensitivities, complex64 (Q,H,W), made on the host.  Pixel (i, j) has the coordinates
    y = (i + 0.5) / H - 0.5 and x = (j + 0.5) / W - 0.5; coil k sits at angle a_k = 2 pi (k + r) / Q on the circle of radius 0.6
    around the field of view, centre (cy, cx) = 0.6 (sin a_k, cos a_k), with r one uniform draw in [0, 1) from a generator seeded
    with ``seed``.  Its magnitude is the Gaussian exp(-((y - cy)^2 + (x - cx)^2) / (2 width^2)) and its phase the linear
    2 pi (f_k y + g_k x) + p_k with f_k, g_k uniform in [-0.5, 0.5) and p_k uniform in [0, 2 pi), drawn in the order
    r, f (Q values), g (Q values), p (Q values), all in fp64.  The maps are divided by sqrt(sum_q |S_q|^2) at every pixel, so that
    sum_q |S_q|^2 = 1, and rounded to complex64."""
    h, w = (int(v) for v in hw)
    q = int(q)
    if h < 1 or w < 1 or not 1 <= q <= COILS_MAX or not float(width) > 0.0:
        raise ValueError(f"coil_maps: hw {tuple(hw)}, q {q!r} from 1 to {COILS_MAX}, width {width!r} > 0")
    gen = torch.Generator().manual_seed(int(seed))
    draw = lambda k: torch.rand(k, generator=gen, dtype=torch.float64)
    r, f, g, p = draw(1), draw(q) - 0.5, draw(q) - 0.5, 2.0 * math.pi * draw(q)
    a = 2.0 * math.pi * (torch.arange(q, dtype=torch.float64) + r) / q
    cy, cx = (0.6 * torch.sin(a)).view(q, 1, 1), (0.6 * torch.cos(a)).view(q, 1, 1)
    y = ((torch.arange(h, dtype=torch.float64) + 0.5) / h - 0.5).view(1, h, 1)
    x = ((torch.arange(w, dtype=torch.float64) + 0.5) / w - 0.5).view(1, 1, w)
    mag = torch.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * float(width) ** 2))
    s = torch.polar(mag, 2.0 * math.pi * (f.view(q, 1, 1) * y + g.view(q, 1, 1) * x) + p.view(q, 1, 1))
    s = s / (s.abs() ** 2).sum(dim=0, keepdim=True).sqrt()
    return s.to(torch.complex64).contiguous()


def coils_scratch(n, c, q, h, w, device):
    """The scratch of glowhip_restore_objective_coils for a batch of ``n`` images (c, h, w) seen by ``q`` coils: a uint8 device
    tensor of glowhip_restore_coils_scratch_bytes(n, c, q, h, w) bytes."""
    need = int(_lib.lib().glowhip_restore_coils_scratch_bytes(int(n), int(c), int(q), int(h), int(w)))
    if need == 0:
        _lib.check(-1)
    return torch.empty(need, dtype=torch.uint8, device=device)


def _device_maps(maps, n, hw, device):
    """(contiguous fp32 device view of the maps, Q, maps_stride in floats) for the C calls."""
    real, q, per_sample = check_coil_maps(maps, n, hw)
    real = _lib.require_device_tensor(real, "coils")
    if real.device != device:
        raise _lib.GlowHipError("coils must be on the device of the image")
    real = real.contiguous()
    return real, q, (q * int(hw[0]) * int(hw[1]) * 2 if per_sample else 0)


def coils2d(x, maps, out=None):
    """The multi-coil forward operator ``F (S x)``: real fp32 device ``x`` (N,C,H,W) to complex64 (N,C,Q,H,W) by glowhip_coils2d;
    ``maps`` as `check_coil_maps` takes them, on the device of x.  ``out``: an fp32 buffer (N,C,Q,H,W,2) to write."""
    x = _lib.require_device_tensor(x, "x")
    if x.dim() != 4:
        raise ValueError(f"coils2d: x of shape {tuple(x.shape)}: expected (N, C, H, W)")
    n, c, h, w = (int(v) for v in x.shape)
    check_fourier_shape((h, w), "coils2d")
    s, q, stride = _device_maps(maps, n, (h, w), x.device)
    real = torch.empty((n, c, q, h, w, 2), dtype=torch.float32, device=x.device) if out is None else out
    if not (real.is_cuda and real.dtype == torch.float32 and real.is_contiguous() and tuple(real.shape) == (n, c, q, h, w, 2)):
        raise _lib.GlowHipError("coils2d: out must be a contiguous fp32 device tensor (N, C, Q, H, W, 2)")
    _lib.check(_lib.lib().glowhip_coils2d(_lib.ptr(x), _lib.ptr(s), stride, _lib.ptr(real), n, c, q, h, w, 0, _lib.stream_ptr(x.device)))
    return torch.view_as_complex(real)


def coils2d_adjoint(k, maps, out=None):
    """``sum_q Re(conj(S_q) F^H k_q)``, real fp32 (N,C,H,W), of a device tensor ``k``, complex64 (N,C,Q,H,W) or fp32 with a trailing
    2: the adjoint of `coils2d` as a map from real images (glowhip_coils2d with adjoint = 1) -- with normalised maps and a masked
    measurement, the coil-combined zero-filled reconstruction.  ``out``: the fp32 buffer to write."""
    real = _lib.require_device_tensor(as_kspace(k, "k"), "k")
    if real.dim() != 6:
        raise ValueError(f"coils2d_adjoint: k of shape {tuple(k.shape)}: expected complex (N, C, Q, H, W)")
    n, c, q, h, w = (int(v) for v in real.shape[:5])
    check_fourier_shape((h, w), "coils2d_adjoint")
    s, qs, stride = _device_maps(maps, n, (h, w), real.device)
    if qs != q:
        raise ValueError(f"coils2d_adjoint: k holds {q} coils, the maps {qs}")
    x = torch.empty((n, c, h, w), dtype=torch.float32, device=real.device) if out is None else out
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (n, c, h, w)):
        raise _lib.GlowHipError("coils2d_adjoint: out must be a contiguous fp32 device tensor (N, C, H, W)")
    _lib.check(_lib.lib().glowhip_coils2d(_lib.ptr(real), _lib.ptr(s), stride, _lib.ptr(x), n, c, q, h, w, 1, _lib.stream_ptr(x.device)))
    return x


def restore_objective(x, target, weight=None, inv_wsum=None, pool=1, *, grad_out=None, loss_out=None, psf=None, resid_out=None,
                      operator=None, scratch=None, fourier=False, coils=None):
    """``(loss (N,), grad_x)`` of the data term for images ``x`` (N,C,H,W): glowhip_restore_objective.  ``target`` / ``weight``
    (N,C,H/pool,W/pool; weight None = ones), ``inv_wsum`` (N,; None = 1 / elements of one measurement).  Contiguous fp32 device
    tensors, read where they are (a contiguous view at any offset is fine).  ``grad_out`` / ``loss_out``: buffers to write.

    ``psf`` (kh,kw) or (N,kh,kw), sides odd and at most 15: the image is observed through that point-spread function before the
    pool (glowhip_restore_objective_psf; include/glowhip.h has the definition), one for the batch or one per sample, not
    normalised.  ``resid_out`` (N,C,H/pool,W/pool): where that call leaves w (A x - t) -- its scratch, allocated when None.
    ``psf=None`` is the call above, unchanged.

    ``operator`` (M,C,H,W): the image is observed through that dense matrix, y = A x with x flattened in (C,H,W) order
    (glowhip_restore_objective_linear); ``target`` / ``weight`` / ``resid_out`` are then (N, M), ``psf`` must be None and ``pool``
    1.  The operator is read where it is and not normalised.  ``scratch``: a uint8 device tensor of at least
    glowhip_restore_linear_scratch_bytes(N, M, C H W) bytes (`linear_scratch`), allocated when None.  ``operator=None`` is every
    call above, unchanged.

    ``fourier=True``: the image is observed through the unitary 2-D DFT of each channel's plane
    (glowhip_restore_objective_fourier); ``target`` / ``resid_out`` are then fp32 (N,C,H,W,2) -- `torch.view_as_real` of a
    complex64 (N,C,H,W) -- ``weight`` the real (N,C,H,W) k-space mask or weight, ``psf`` and ``operator`` must be None and ``pool``
    1.  ``scratch``: a uint8 device tensor of at least glowhip_restore_fourier_scratch_bytes(N, C, H, W) bytes (`fourier_scratch`),
    allocated when None.  ``fourier=False`` is every call above, unchanged.

    ``coils=maps`` (with ``fourier=True``; ValueError without): multi-coil k-space, glowhip_restore_objective_coils -- the image is
    seen by Q coils through the complex sensitivity ``maps`` (Q,H,W), shared by the batch, or (N,Q,H,W), complex64 or fp32 with a
    trailing 2 (`check_coil_maps`); ``target`` / ``resid_out`` are then fp32 (N,C,Q,H,W,2), ``weight`` stays (N,C,H,W), shared by
    the coils, and ``inv_wsum=None`` is 1 / (C Q H W).  ``scratch``: at least glowhip_restore_coils_scratch_bytes(N, C, Q, H, W) bytes
    (`coils_scratch`).  ``coils=None`` is every call above, unchanged."""
    if coils is not None and not fourier:
        raise ValueError("restore_objective: coils needs fourier=True (the maps multiply the image in front of the transform)")
    for name, t in (("x", x), ("target", target), ("weight", weight), ("inv_wsum", inv_wsum), ("grad_out", grad_out), ("loss_out", loss_out),
                    ("psf", psf), ("resid_out", resid_out), ("operator", operator)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device):
            raise _lib.GlowHipError(f"restore_objective: {name} must be a contiguous fp32 tensor on the device of x")
    n, c, h, w = x.shape
    pool = int(pool)
    if fourier and coils is not None:
        return _restore_objective_coils(x, target, weight, inv_wsum, pool, grad_out, loss_out, psf, resid_out, operator, scratch, coils)
    if fourier:
        return _restore_objective_fourier(x, target, weight, inv_wsum, pool, grad_out, loss_out, psf, resid_out, operator, scratch)
    if operator is not None:
        return _restore_objective_linear(x, target, weight, inv_wsum, pool, grad_out, loss_out, psf, resid_out, operator, scratch)
    if scratch is not None:
        raise _lib.GlowHipError("restore_objective: scratch belongs to the call with an operator")
    mshape = None
    if pool >= 1 and h % pool == 0 and w % pool == 0:      # (anything else is the C call's to refuse)
        mshape = (n, c, h // pool, w // pool)
        if tuple(target.shape) != mshape or (weight is not None and tuple(weight.shape) != mshape):
            raise _lib.GlowHipError(f"restore_objective: target / weight must have shape {mshape}")
    if inv_wsum is not None and inv_wsum.numel() != n:
        raise _lib.GlowHipError(f"restore_objective: inv_wsum holds {inv_wsum.numel()} values for a batch of {n}")
    grad = torch.empty_like(x) if grad_out is None else grad_out
    loss = torch.empty(n, dtype=torch.float32, device=x.device) if loss_out is None else loss_out
    if tuple(grad.shape) != tuple(x.shape) or loss.numel() != n:
        raise _lib.GlowHipError("restore_objective: grad_out must have the shape of x, loss_out one value per sample")
    if psf is None:
        if resid_out is not None:
            raise _lib.GlowHipError("restore_objective: resid_out belongs to the call with a psf")
        _lib.check(_lib.lib().glowhip_restore_objective(_lib.ptr(x), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(inv_wsum), n, c, h, w,
                                                        pool, _lib.ptr(grad), _lib.ptr(loss), _lib.stream_ptr(x.device)))
        return loss, grad
    if psf.dim() not in (2, 3) or (psf.dim() == 3 and psf.shape[0] != n):
        raise _lib.GlowHipError(f"restore_objective: psf of shape {tuple(psf.shape)}: expected (kh, kw) or ({n}, kh, kw)")
    kh, kw = psf.shape[-2:]                                # (their parity and range are the C call's to refuse)
    resid = torch.empty_like(target) if resid_out is None else resid_out
    if mshape is not None and tuple(resid.shape) != mshape:
        raise _lib.GlowHipError(f"restore_objective: resid_out must have shape {mshape}")
    _lib.check(_lib.lib().glowhip_restore_objective_psf(_lib.ptr(x), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(inv_wsum),
                                                        _lib.ptr(psf), kh * kw if psf.dim() == 3 else 0, kh, kw, n, c, h, w, pool,
                                                        _lib.ptr(resid), _lib.ptr(grad), _lib.ptr(loss), _lib.stream_ptr(x.device)))
    return loss, grad


def _restore_objective_linear(x, target, weight, inv_wsum, pool, grad_out, loss_out, psf, resid_out, operator, scratch):
    """`restore_objective` with an operator (its tensors are already known to be contiguous fp32 on the device of x)."""
    n = x.shape[0]
    if psf is not None or pool != 1:
        raise _lib.GlowHipError("restore_objective: an operator excludes psf, and pool must be 1")
    if operator.dim() != 4 or tuple(operator.shape[1:]) != tuple(x.shape[1:]):
        raise _lib.GlowHipError(f"restore_objective: operator of shape {tuple(operator.shape)}: expected (M,) + {tuple(x.shape[1:])}")
    m, d = operator.shape[0], operator[0].numel()
    for name, t in (("target", target), ("weight", weight), ("resid_out", resid_out)):
        if t is not None and tuple(t.shape) != (n, m):
            raise _lib.GlowHipError(f"restore_objective: {name} must have shape {(n, m)} with this operator")
    if inv_wsum is not None and inv_wsum.numel() != n:
        raise _lib.GlowHipError(f"restore_objective: inv_wsum holds {inv_wsum.numel()} values for a batch of {n}")
    grad = torch.empty_like(x) if grad_out is None else grad_out
    loss = torch.empty(n, dtype=torch.float32, device=x.device) if loss_out is None else loss_out
    if tuple(grad.shape) != tuple(x.shape) or loss.numel() != n:
        raise _lib.GlowHipError("restore_objective: grad_out must have the shape of x, loss_out one value per sample")
    resid = torch.empty_like(target) if resid_out is None else resid_out
    if scratch is None:
        scratch = linear_scratch(n, m, d, x.device)
    elif not (scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.device == x.device):
        raise _lib.GlowHipError("restore_objective: scratch must be a contiguous uint8 tensor on the device of x")
    _lib.check(_lib.lib().glowhip_restore_objective_linear(_lib.ptr(x), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(inv_wsum),
                                                           _lib.ptr(operator), m, n, d, _lib.ptr(resid), _lib.ptr(grad), _lib.ptr(loss),
                                                           _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr(x.device)))
    return loss, grad


def _restore_objective_fourier(x, target, weight, inv_wsum, pool, grad_out, loss_out, psf, resid_out, operator, scratch):
    """`restore_objective` with ``fourier=True`` (its tensors are already known to be contiguous fp32 on the device of x)."""
    n, c, h, w = x.shape
    if psf is not None or operator is not None or pool != 1:
        raise _lib.GlowHipError("restore_objective: fourier excludes psf and operator, and pool must be 1")
    for name, t, shape in (("target", target, (n, c, h, w, 2)), ("resid_out", resid_out, (n, c, h, w, 2)), ("weight", weight, (n, c, h, w))):
        if t is not None and tuple(t.shape) != shape:
            raise _lib.GlowHipError(f"restore_objective: {name} must have shape {shape} with fourier")
    if inv_wsum is not None and inv_wsum.numel() != n:
        raise _lib.GlowHipError(f"restore_objective: inv_wsum holds {inv_wsum.numel()} values for a batch of {n}")
    grad = torch.empty_like(x) if grad_out is None else grad_out
    loss = torch.empty(n, dtype=torch.float32, device=x.device) if loss_out is None else loss_out
    if tuple(grad.shape) != tuple(x.shape) or loss.numel() != n:
        raise _lib.GlowHipError("restore_objective: grad_out must have the shape of x, loss_out one value per sample")
    resid = torch.empty_like(target) if resid_out is None else resid_out
    if scratch is None:
        if not (2 <= h <= FOURIER_MAX and 2 <= w <= FOURIER_MAX and h & (h - 1) == 0 and w & (w - 1) == 0):      # (let the C call say why)
            scratch = torch.empty(16, dtype=torch.uint8, device=x.device)
        else:
            scratch = fourier_scratch(n, c, h, w, x.device)
    elif not (scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.device == x.device):
        raise _lib.GlowHipError("restore_objective: scratch must be a contiguous uint8 tensor on the device of x")
    _lib.check(_lib.lib().glowhip_restore_objective_fourier(_lib.ptr(x), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(inv_wsum), n, c, h, w,
                                                            _lib.ptr(resid), _lib.ptr(grad), _lib.ptr(loss), _lib.ptr(scratch),
                                                            scratch.numel(), _lib.stream_ptr(x.device)))
    return loss, grad


def _restore_objective_coils(x, target, weight, inv_wsum, pool, grad_out, loss_out, psf, resid_out, operator, scratch, coils):
    """`restore_objective` with ``fourier=True, coils=maps`` (its fp32 tensors are already known to be contiguous on the device of x)."""
    n, c, h, w = x.shape
    if psf is not None or operator is not None or pool != 1:
        raise _lib.GlowHipError("restore_objective: fourier excludes psf and operator, and pool must be 1")
    maps, q, stride = _device_maps(coils, n, (h, w), x.device)
    for name, t, shape in (("target", target, (n, c, q, h, w, 2)), ("resid_out", resid_out, (n, c, q, h, w, 2)), ("weight", weight, (n, c, h, w))):
        if t is not None and tuple(t.shape) != shape:
            raise _lib.GlowHipError(f"restore_objective: {name} must have shape {shape} with {q} coils")
    if inv_wsum is not None and inv_wsum.numel() != n:
        raise _lib.GlowHipError(f"restore_objective: inv_wsum holds {inv_wsum.numel()} values for a batch of {n}")
    grad = torch.empty_like(x) if grad_out is None else grad_out
    loss = torch.empty(n, dtype=torch.float32, device=x.device) if loss_out is None else loss_out
    if tuple(grad.shape) != tuple(x.shape) or loss.numel() != n:
        raise _lib.GlowHipError("restore_objective: grad_out must have the shape of x, loss_out one value per sample")
    resid = torch.empty_like(target) if resid_out is None else resid_out
    if scratch is None:
        if not (2 <= h <= FOURIER_MAX and 2 <= w <= FOURIER_MAX and h & (h - 1) == 0 and w & (w - 1) == 0):      # (let the C call say why)
            scratch = torch.empty(16, dtype=torch.uint8, device=x.device)
        else:
            scratch = coils_scratch(n, c, q, h, w, x.device)
    elif not (scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.device == x.device):
        raise _lib.GlowHipError("restore_objective: scratch must be a contiguous uint8 tensor on the device of x")
    _lib.check(_lib.lib().glowhip_restore_objective_coils(_lib.ptr(x), _lib.ptr(target), _lib.ptr(weight), _lib.ptr(inv_wsum), _lib.ptr(maps),
                                                          stride, n, c, q, h, w, _lib.ptr(resid), _lib.ptr(grad), _lib.ptr(loss),
                                                          _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr(x.device)))
    return loss, grad


ESTIMATE_PSF = (None, "shared", "per_sample")


def blind_start(psf, estimate_psf, n, operator=None):
    """The start of a blind fit, checked on the host before any device work: ``psf`` -- anything `torch.as_tensor` takes, of shape
    (kh,kw) or (n,kh,kw), or a pair of Python ints (kh, kw) meaning the uniform PSF of that support -- as a CPU fp32 tensor
    normalised to sum 1 per PSF, of shape (kh,kw) for ``"shared"`` and (n,kh,kw) for ``"per_sample"`` (a single start is repeated).
    ValueError: an unknown ``estimate_psf``, an ``operator`` beside it, no start, an even or out-of-range side, (n,kh,kw) with
    ``"shared"``, and a tap that is not a finite value > 0 -- a softmax cannot hold an exact zero."""
    if estimate_psf not in ESTIMATE_PSF or estimate_psf is None:
        raise ValueError(f"estimate_psf = {estimate_psf!r}: None, 'shared' or 'per_sample'")
    if operator is not None:
        raise ValueError("estimate_psf: a dense operator has no point-spread function to estimate")
    if psf is None:
        raise ValueError("estimate_psf needs a start: psf = (kh, kw) for the uniform one, or a tensor of positive taps")
    if isinstance(psf, (tuple, list)) and len(psf) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in psf):
        kh, kw = check_psf_shape(psf, n)
        psf = torch.full((kh, kw), 1.0 / (kh * kw), dtype=torch.float64)
    k = torch.as_tensor(psf).detach().cpu().double()
    kh, kw = check_psf_shape(k.shape, n)
    if k.dim() == 3 and estimate_psf == "shared":
        raise ValueError(f"estimate_psf='shared' starts from ONE psf (kh, kw), not from {tuple(k.shape)}")
    if not bool((torch.isfinite(k) & (k > 0)).all()):
        raise ValueError("estimate_psf: every tap of the start must be > 0 (the estimate is a softmax, which cannot hold an exact zero)")
    k = k / k.sum(dim=(-2, -1), keepdim=True)
    if k.dim() == 2 and estimate_psf == "per_sample":
        k = k.expand(n, kh, kw)
    return k.float().contiguous()


def psf_from_logits(logits, out=None):
    """``softmax(logits)`` over the taps of each PSF: glowhip_psf_from_logits (the max subtracted, exponentials and sum in fp64 in
    tap order, one rounding per tap).  ``logits`` (kh,kw) or (n_psf,kh,kw), a contiguous fp32 device tensor; ``out``: the buffer to
    write, of the same shape."""
    psf = torch.empty_like(logits) if out is None else out
    for name, t in (("logits", logits), ("out", psf)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == logits.device):
            raise _lib.GlowHipError(f"psf_from_logits: {name} must be a contiguous fp32 tensor on the device of the logits")
    if logits.dim() not in (2, 3) or tuple(psf.shape) != tuple(logits.shape):
        raise _lib.GlowHipError(f"psf_from_logits: logits of shape {tuple(logits.shape)} (expected (kh, kw) or (n_psf, kh, kw)) and out of the same shape")
    kh, kw = logits.shape[-2:]
    _lib.check(_lib.lib().glowhip_psf_from_logits(_lib.ptr(logits), _lib.ptr(psf), logits.shape[0] if logits.dim() == 3 else 1, kh, kw,
                                                  _lib.stream_ptr(logits.device)))
    return psf


def psf_grad_scratch(shape, kh, kw, pool, device):
    """The scratch of glowhip_restore_psf_grad for images of ``shape`` (N,C,H,W): a uint8 device tensor."""
    n, c, h, w = (int(v) for v in shape)
    need = int(_lib.lib().glowhip_restore_psf_grad_scratch_bytes(n, c, h, w, int(kh), int(kw), int(pool)))
    if need == 0:
        _lib.check(-1)
    return torch.empty(need, dtype=torch.uint8, device=device)


def psf_gradient(x, resid, inv_wsum, psf, pool, *, grad_psf=None, grad_logits=None, scratch=None):
    """``(grad_psf, grad_logits)`` of the data term with respect to the taps of ``psf`` and to the logits of ``psf = softmax(theta)``:
    glowhip_restore_psf_grad (include/glowhip.h has the definition), after ``restore_objective(x, ..., psf=psf, resid_out=resid)``
    on the same ``x`` (N,C,H,W), ``resid`` (N,C,H/pool,W/pool) and ``inv_wsum`` (N,; None = that call's default).  ``psf`` (kh,kw) --
    shared: the gradient is summed over the batch in sample order -- or (N,kh,kw); both gradients have its shape.  Contiguous fp32
    device tensors.  ``grad_psf`` / ``grad_logits``: buffers to write; with neither, both are allocated and returned; with one, the
    other is not computed (None).  ``scratch``: a uint8 device tensor of glowhip_restore_psf_grad_scratch_bytes (`psf_grad_scratch`),
    allocated when None."""
    for name, t in (("x", x), ("resid", resid), ("inv_wsum", inv_wsum), ("psf", psf), ("grad_psf", grad_psf), ("grad_logits", grad_logits)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device):
            raise _lib.GlowHipError(f"psf_gradient: {name} must be a contiguous fp32 tensor on the device of x")
    n, c, h, w = x.shape
    pool = int(pool)
    if psf is None or psf.dim() not in (2, 3) or (psf.dim() == 3 and psf.shape[0] != n):
        raise _lib.GlowHipError(f"psf_gradient: psf of shape {None if psf is None else tuple(psf.shape)}: expected (kh, kw) or ({n}, kh, kw)")
    kh, kw = psf.shape[-2:]                                # (their parity and range are the C call's to refuse)
    if pool >= 1 and h % pool == 0 and w % pool == 0 and tuple(resid.shape) != (n, c, h // pool, w // pool):
        raise _lib.GlowHipError(f"psf_gradient: resid must have shape {(n, c, h // pool, w // pool)}")
    if inv_wsum is not None and inv_wsum.numel() != n:
        raise _lib.GlowHipError(f"psf_gradient: inv_wsum holds {inv_wsum.numel()} values for a batch of {n}")
    if grad_psf is None and grad_logits is None:
        grad_psf, grad_logits = torch.empty_like(psf), torch.empty_like(psf)
    for name, t in (("grad_psf", grad_psf), ("grad_logits", grad_logits)):
        if t is not None and t.numel() != psf.numel():
            raise _lib.GlowHipError(f"psf_gradient: {name} must have the shape of psf")
    if scratch is None:
        scratch = psf_grad_scratch(x.shape, kh, kw, pool, x.device)
    elif not (scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.device == x.device):
        raise _lib.GlowHipError("psf_gradient: scratch must be a contiguous uint8 tensor on the device of x")
    _lib.check(_lib.lib().glowhip_restore_psf_grad(_lib.ptr(x), _lib.ptr(resid), _lib.ptr(inv_wsum), _lib.ptr(psf),
                                                   kh * kw if psf.dim() == 3 else 0, kh, kw, n, c, h, w, pool, _lib.ptr(grad_psf),
                                                   _lib.ptr(grad_logits), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr(x.device)))
    return grad_psf, grad_logits


@dataclass
class RestoreInfo:
    """What a fit reports.  ``loss`` (steps, N): the per-sample data term BEFORE each iteration's update; ``grad_norm`` (steps,):
    the total norm of the data term's latent gradient (all samples, before clipping; the prior term is not in it).  ``finite``: every
    norm was finite -- when False, the iterations with a non-finite norm were skipped on the device.  ``captured``: the iterations
    after the first ran as hipGraph replays.  ``fallback``: how many times the fit was run again on the exact-fp32 kernel family (0
    or 1).  ``graph_error``: why a requested capture did not happen.  A blind fit (``estimate_psf``) adds ``psf``, the estimate --
    softmax of the final logits, (kh,kw) or (N,kh,kw), on the device -- and ``psf_grad_norm`` (steps,), the norm of the data term's
    gradient with respect to the logits; ``finite`` then covers both norm histories."""
    loss: torch.Tensor
    grad_norm: torch.Tensor
    finite: bool
    captured: bool
    fallback: int = 0
    graph_error: Optional[str] = None
    psf: Optional[torch.Tensor] = None
    psf_grad_norm: Optional[torch.Tensor] = None


def check_prior_weight(glow, prior_weight):
    """The prior term 1/2 ||latents||^2 is the latents' negative log-density only under a standard-normal top prior: a model whose
    top prior is learned or class-conditional raises for ``prior_weight > 0`` (whitening its top latent is not implemented)."""
    ab = glow.hps.ablation
    unusual = [name for name in ("learn_top", "y_condition") if ab.get(name, False)]
    if prior_weight and unusual:
        raise ValueError(f"prior_weight = {prior_weight!r}: the prior term 1/2 ||latents||^2 assumes a standard-normal top prior, and this "
                         f"model's is not ({' / '.join(unusual)}); whitening the top latent is not implemented")


class LatentLoop:
    """What the device-resident loops over the latents of a measurement share -- `LatentFit` here, `posterior.LatentMALA`: the
    problem (``target``, ``weight``, ``pool``, the optional point-spread function ``psf`` or dense ``operator``, the plan of the full-resolution image, the start leaves ``_start``, the static
    ``image`` and its gradient ``grad_x``), one evaluation of it, and an iteration as either Python-enqueued launches
    (`step_eager`) or one hipGraph launch (`capture` once, after at least one eager iteration -- lazy allocations, packed weights
    -- then `step_captured`), by the package's one capture protocol (`_capture.Capture`).  Same kernels and same bits either way.

    A subclass supplies ``inv_wsum`` (the per-sample factor of the data term), ``_body(captured)`` (the iteration), `reset`, and,
    where a replay has a host side, ``_capturing()`` / ``_signature()`` / ``_replay_host()``.

    ``operator`` (M,C,H,W), a contiguous fp32 device tensor: the measurement is (N, M) and the image shape is the operator's.  The
    loop holds the operator BY REFERENCE -- a sensing matrix is hundreds of MB; it is not copied -- so the caller must not write
    to it (or free it) while a fit or a chain that uses it is alive.  ``resid`` and the call's scratch ``op_scratch`` are the loop's own.

    ``fourier=True``: the measurement is the unitary 2-D DFT of the decode, complex64 (N,C,H,W) or fp32 with a trailing 2 (kept as
    the latter); ``weight`` is the real k-space mask or weight, broadcast to (N,C,H,W); sides are powers of two up to 256.  It
    excludes ``psf``, ``operator`` and ``pool != 1`` (ValueError).  ``resid`` and ``op_scratch`` are static buffers as above.

    ``coils=maps`` (with ``fourier=True``; ValueError without): multi-coil k-space -- the measurement is complex64 (N,C,Q,H,W) or
    fp32 with a trailing 2, the image shape (C,H,W) is taken from it, ``maps`` are the Q complex sensitivity maps (Q,H,W) or
    (N,Q,H,W) (`check_coil_maps`) and ``weight`` stays (N,C,H,W), shared by the coils.  The maps are CLONED into a static buffer of
    the loop (they are small, unlike the dense operator); ``resid`` and ``op_scratch`` are sized for the coil call."""

    def __init__(self, glow, measurement, weight, pool, init, steps, graph, psf=None, operator=None, fourier=False, coils=None):
        self.glow, self.pool, self.steps, self.want_graph = glow, int(pool), int(steps), bool(graph)
        self.fourier = bool(fourier)
        self.coils, self.n_coils = None, 0
        if coils is not None and not self.fourier:
            raise ValueError("coils needs fourier=True (the maps multiply the image in front of the transform)")
        if coils is not None:
            if psf is not None or operator is not None or self.pool != 1:
                raise ValueError("coils excludes psf, operator and estimate_psf, and pool must be 1")
            measurement = as_kspace(measurement)
            if measurement.dim() != 6:
                raise ValueError(f"measurement of shape {tuple(measurement.shape)}: expected complex (N, C, Q, H, W) or fp32 (N, C, Q, H, W, 2) with coils")
            check_fourier_shape(measurement.shape[3:5], "measurement")
            maps, self.n_coils, _ = check_coil_maps(coils, measurement.shape[0], measurement.shape[3:5])
            if self.n_coils != int(measurement.shape[2]):
                raise ValueError(f"measurement of shape {tuple(measurement.shape)} holds {int(measurement.shape[2])} coils, the maps {self.n_coils}")
        elif self.fourier:
            if psf is not None or operator is not None or self.pool != 1:
                raise ValueError("fourier excludes psf, operator and estimate_psf, and pool must be 1")
            measurement = as_kspace(measurement)
            if measurement.dim() != 5:
                raise ValueError(f"measurement of shape {tuple(measurement.shape)}: expected complex (N, C, H, W) or fp32 (N, C, H, W, 2) with fourier")
            check_fourier_shape(measurement.shape[2:4], "measurement")
        meas = _lib.require_device_tensor(measurement, "measurement")
        dev = self.device = meas.device
        if self.pool < 1:
            raise ValueError(f"pool = {pool}")
        if operator is not None:
            if psf is not None or self.pool != 1:
                raise ValueError("an operator excludes psf, and pool must be 1")
            op = _lib.require_device_tensor(operator, "operator")
            if op is not operator or op.device != dev:      # (never a copy of a matrix of hundreds of MB behind the caller's back)
                raise ValueError("operator must be a contiguous fp32 tensor on the device of the measurement")
            m, d = check_operator_shape(op.shape)
            if meas.dim() != 2 or meas.shape[1] != m:
                raise ValueError(f"measurement of shape {tuple(meas.shape)}: expected (N, {m}) with this operator")
            n, image_chw = meas.shape[0], tuple(op.shape[1:])
        elif coils is not None:
            n, image_chw = meas.shape[0], (int(meas.shape[1]),) + tuple(meas.shape[3:5])
        elif self.fourier:
            n, image_chw = meas.shape[0], tuple(meas.shape[1:4])
        else:
            n, c, h, w = meas.shape
            image_chw = (c, h * self.pool, w * self.pool)
        self.plan = plan = glow.flow.plan_for(image_chw, dev)
        if tuple(init.z.shape) != (n,) + plan.out_chw or len(init.eps) != plan.n_split:
            raise ValueError(f"init {init!r} does not belong to a batch of {n} images of shape {plan.in_chw}")
        self.n = n
        self.target = meas.clone()
        wshape = meas.shape[:4] if self.fourier else meas.shape      # (the k-space weight is real: one value per coefficient)
        if coils is not None:
            wshape = (n,) + image_chw                                # (and shared by the coils)
        self.weight = None if weight is None else _lib.require_device_tensor(weight, "weight").expand(wshape).contiguous()
        self._start = [t.float().contiguous().clone() for t in init.to(dev).detach().tensors()]
        self.image = torch.empty((n,) + plan.in_chw, dtype=torch.float32, device=dev)
        self.grad_x = torch.empty_like(self.image)
        # the point-spread function (None: the image is observed directly) and the objective's scratch w (A x - t): one buffer,
        # because every evaluation of a loop runs on one stream, one after the other
        self.psf = self.resid = None
        if psf is not None:
            self.psf = _lib.require_device_tensor(psf, "psf").to(dev).clone()
            check_psf_shape(self.psf.shape, n)
            self.resid = torch.empty_like(self.target)
        # the dense operator (by reference), its residual and the scratch of its call: static buffers like the above
        self.operator = self.op_scratch = None
        if operator is not None:
            self.operator = op
            self.resid = torch.empty_like(self.target)
            self.op_scratch = linear_scratch(n, m, d, dev)
        # Fourier-domain measurements: the residual (the forward pass's intermediate too) and the call's scratch, static as above
        if self.fourier:
            self.resid = torch.empty_like(self.target)
            self.op_scratch = fourier_scratch(n, *image_chw, dev) if coils is None else coils_scratch(n, image_chw[0], self.n_coils, *image_chw[1:], dev)
        if coils is not None:      # the maps: the loop's own fp32 copy (..., Q, H, W, 2)
            self.coils = _lib.require_device_tensor(maps, "coils").to(dev).clone()
        self._capture = None
        self.graph_error = None
        self._iterations = 0         # run since construction (a reset does not take the lazy allocations back)

    # ------------------------------------------------------------------ the iteration
    def _evaluate(self, leaves, image, loss, grads):
        """`FlowPlan.decode` of ``leaves`` into ``image``; `restore_objective` (per-sample loss into ``loss``, its image gradient
        into ``grad_x``; through ``psf`` or ``operator`` when the loop has one, with ``resid`` -- and ``op_scratch`` -- as its scratch);
        `FlowPlan.decode_vjp` of that into ``grads``."""
        plan = self.plan
        plan.decode(leaves[0], leaves[1:], out=image)
        restore_objective(image, self.target, self.weight, self.inv_wsum, self.pool, grad_out=self.grad_x, loss_out=loss,
                          psf=self.psf, resid_out=self.resid, operator=self.operator, scratch=self.op_scratch, fourier=self.fourier,
                          coils=self.coils)
        plan.decode_vjp(image, self.grad_x, out=(grads[0], grads[1:]))

    def _capturing(self):            # the context of a recording (the fit: its optimiser's)
        return contextlib.nullcontext()

    def _replay_host(self):          # what a replay does on the host before the graph launch (the fit: the hyper upload)
        pass

    def _signature(self):
        """What a captured iteration reaches through the plan and an eager call in between could have moved or rebuilt: no pack is
        inside, so the parameters' versions and the family count, and the workspaces of the decode and of its VJP.  ``psf``,
        ``resid`` and ``op_scratch`` need no entry: like ``target`` and ``weight`` they are this loop's own static buffers, allocated
        once in the constructor and never rebound, so a recorded launch always reaches them; ``operator`` is the caller's tensor,
        held here for the loop's life, which the caller must leave alone (`LatentLoop`)."""
        sig = self.plan.capture_signature(versions=True, family=True, buffers=("packed", "_ws", "_vjp_tape", "_vjp_ws"))
        if self.coils is not None:
            return {**sig, "fourier": True, "coils": self.n_coils}
        return {**sig, "fourier": True} if self.fourier else sig      # (which objective the recording holds)

    @torch.no_grad()
    def step_eager(self):
        """One iteration enqueued launch by launch."""
        self._body(captured=False)
        self._iterations += 1

    @torch.no_grad()
    def capture(self):
        """Record one iteration as a hipGraph.  True on success; on failure the reason is kept in ``graph_error``, the loop stays
        eager and nothing raises.  Nothing runs during a capture: the device words do not move."""
        if self._iterations < 1:
            raise _lib.GlowHipError(f"{type(self).__name__}.capture: run one eager iteration first (lazy allocations, packed weights)")
        self._capture = None
        try:
            with self._capturing():
                self._capture = Capture(self.plan, lambda: self._body(captured=True), self._signature)
        except Exception as e:       # capture is an optimisation of the host side only
            self.graph_error = f"{type(e).__name__}: {str(e)[:300]}"
            return False
        return True

    @property
    def captured(self):
        return self._capture is not None and not self._capture.moved()

    @torch.no_grad()
    def step_captured(self):
        """One iteration as one graph launch (and whatever the subclass uploads for it)."""
        if not self.captured:
            raise _lib.GlowHipError(f"{type(self).__name__}.step_captured: no valid capture (capture() after an eager iteration; a "
                                    "parameter, a workspace or the kernel family changed since)")
        self._replay_host()
        self._capture.replay()
        self._iterations += 1

    def _iterate(self):
        """``steps`` iterations from where the loop stands: the first eagerly, the others as replays when a graph is wanted and can
        be had (a stale one is recorded again, silently; a failed recording leaves the loop eager).  True when any was a replay."""
        replayed = False
        for it in range(self.steps):
            if self.want_graph and it >= 1 and self.graph_error is None and (self.captured or self.capture()):
                self.step_captured()
                replayed = True
            else:
                self.step_eager()
        return replayed


class PsfLogits:
    """The PSF as an unknown of a fit (`LatentFit(estimate_psf=...)`, `PsfFit`): ``theta`` = the logits of ``psf = softmax(theta)``,
    one row per PSF, started at ``log(start)``; their persistent gradient buffer (bound once as ``theta.grad``); a `training.HipAdam`
    of their OWN at ``psf_lr`` with weight decay 0 -- the HIP optimiser takes one hyper-parameter set per instance, and theta must
    not carry the latents' prior term -- with its own `training.HyperRing` and norm word; and the scratch of
    glowhip_restore_psf_grad.  ``psf`` is the static buffer the objective reads: `forward` fills it from theta, `gradient` takes the
    gradient of the data term from the objective's leftovers (``image``, ``resid``) into ``theta.grad``, and `update` is theta's
    fused step, with a device-side skip of its own when the gradient's norm is not finite, and the norm into row ``row`` of
    ``norm_hist``."""

    def __init__(self, psf, start, image_shape, pool, psf_lr, steps):
        dev = psf.device
        self.psf, self.psf_lr, self.pool = psf, float(psf_lr), int(pool)
        kh, kw = psf.shape[-2:]
        self._theta0 = torch.log(start.double()).float().to(dev).reshape(-1, kh, kw).contiguous()
        self.theta = self._theta0.clone().requires_grad_()
        self.grad = torch.zeros_like(self._theta0)
        self.theta.grad = self.grad
        self.optimizer = HipAdam([self.theta], lr=self.psf_lr, weight_decay=0.0)
        self._token = object()
        self._ring = HyperRing(3, dev)
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.norm_hist = torch.zeros(int(steps), dtype=torch.float32, device=dev)
        self.scratch = psf_grad_scratch(image_shape, kh, kw, self.pool, dev)

    def forward(self):
        psf_from_logits(self.theta.detach().view(self.psf.shape), out=self.psf)

    def gradient(self, image, resid, inv_wsum):
        psf_gradient(image, resid, inv_wsum, self.psf, self.pool, grad_logits=self.grad, scratch=self.scratch)

    def update(self, row, captured):
        self.optimizer.fused_step(0.0, 0.0, skip_nonfinite=True, grads_token=self._token,
                                  hyper_dev=self._ring.words if captured else None, norm_out=self.norm)
        self.norm_hist.index_copy_(0, row, self.norm)

    def replay_host(self):
        self.optimizer.replay_step(self._ring, self.psf_lr)
        torch.autograd.graph.increment_version([self.theta])

    def signature(self):
        return {"psf " + k: v for k, v in self.optimizer.capture_signature().items()}

    @torch.no_grad()
    def reset(self):
        """theta back to its start, the optimiser's state to zero, the history empty; the addresses stay."""
        self.theta.copy_(self._theta0)
        self.optimizer.reset_state()
        self.norm_hist.zero_()

    def estimate(self):
        """softmax of the current logits, in the shape of ``psf`` (a new tensor)."""
        return psf_from_logits(self.theta.detach().view(self.psf.shape).clone())


class LatentFit(LatentLoop):
    """The device-resident fit.  Owns, beyond `LatentLoop`'s buffers, ``inv_wsum`` = 1 / sum w per sample, the latent leaves --
    ``z`` and every ``eps`` of the start `Latents`, copied -- their persistent gradient buffers (bound once as the leaves'
    ``.grad``) and a `training.HipAdam` over the leaves with ``weight_decay = prior_weight``.

    One iteration: decode into the static image, objective, decode VJP into the gradient buffers (`LatentLoop._evaluate`);
    ``fused_step(0, max_grad_norm, skip_nonfinite=True)``; the iteration's losses and norm into row ``row`` of the device histories
    and ``row += 1`` (a device word: the host keeps no count the device could disagree with).  A replay's per-step
    {lr, 1 - beta1^t, 1 - beta2^t} travel through a `training.HyperRing`.  `run` is the whole fit: ``steps`` iterations from the
    start, ONE host read at the end.

    The data term is normalised per sample, so each image of a batch is its own problem; what still couples the batch is the norm
    clip (``max_grad_norm``: one total norm) and the skip of an iteration whose norm is not finite (all samples or none).  A skipped
    iteration still counts in the bias corrections (the host never looks): harmless, because a fit with a skipped iteration is
    either run again on the exact-fp32 family or reported ``finite=False``.

    ``psf`` (kh,kw) or (N,kh,kw), a device tensor: the measurement is the decode blurred by it (`LatentLoop`).  ``operator``
    (M,C,H,W): the measurement (N, M) is the decode seen through that dense matrix, held by reference (`LatentLoop`).

    ``estimate_psf`` = ``"shared"`` / ``"per_sample"``: blind deblurring -- ``psf`` is only the START (`blind_start`: every tap > 0,
    normalised to sum 1; (N,kh,kw) with ``"shared"`` raises, (kh,kw) with ``"per_sample"`` is repeated; an ``operator`` beside it
    raises), and the PSF, as ``softmax(theta)``, is one more unknown of the same loop (`PsfLogits`, ``self.blind``).  An iteration is
    then: `psf_from_logits` into the loop's static ``psf``; the evaluation above, unchanged; `psf_gradient` from the image and the
    residual it left into theta's gradient; the latents' fused step as before; theta's fused step at ``psf_lr``; the histories, with
    theta's gradient norm among them.  The two device-side skips are INDEPENDENT: a non-finite latent norm skips the latents'
    update, a non-finite theta norm theta's, each without the other -- harmless for the same reason as above, since theta's norm
    history enters the test that re-runs a fit on the exact family or reports ``finite=False``.  The softmax fixes the scale
    ambiguity between PSF and image; the translation ambiguity stays, and the centre of the start and the valid-band weights select
    the solution.

    ``fourier=True``: the measurement is the decode's unitary 2-D DFT and ``weight`` the k-space mask (`LatentLoop`).
    ``coils=maps``: multi-coil k-space, the measurement complex (N,C,Q,H,W) (`LatentLoop`)."""

    def __init__(self, glow, measurement, weight=None, pool=1, init=None, steps=100, lr=0.05, prior_weight=0.0, max_grad_norm=0.0,
                 graph=True, psf=None, operator=None, estimate_psf=None, psf_lr=0.2, fourier=False, coils=None):
        check_prior_weight(glow, prior_weight)
        if init is None or steps < 1:
            raise ValueError("LatentFit needs start latents (init) and steps >= 1")
        if fourier and estimate_psf is not None:
            raise ValueError("fourier excludes psf, operator and estimate_psf, and pool must be 1")
        start = None
        if estimate_psf is not None:
            start = blind_start(psf, estimate_psf, len(measurement), operator)
            psf = start.to(measurement.device)
        super().__init__(glow, measurement, weight, pool, init, steps, graph, psf=psf, operator=operator, fourier=fourier, coils=coils)
        self.lr, self.max_grad_norm = float(lr), float(max_grad_norm or 0.0)
        n, dev = self.n, self.device
        # per sample: every image of the batch is its own problem (None: the kernel's 1 / elements, the all-ones weight's)
        self.inv_wsum = None if self.weight is None else 1.0 / self.weight.sum(dim=tuple(range(1, self.weight.dim()))).clamp(min=1.0)
        if self.coils is not None and self.weight is not None:      # every coil's coefficient is a measurement: Q sum w of them
            self.inv_wsum = 1.0 / (float(self.n_coils) * self.weight.sum(dim=(1, 2, 3))).clamp(min=1.0)
        self.loss = torch.zeros(n, dtype=torch.float32, device=dev)
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_hist = torch.zeros((self.steps, n), dtype=torch.float32, device=dev)
        self.norm_hist = torch.zeros(self.steps, dtype=torch.float32, device=dev)
        self.row = torch.zeros(1, dtype=torch.int64, device=dev)
        self.leaves = [t.clone().requires_grad_() for t in self._start]
        self.grads = [torch.zeros_like(t) for t in self._start]
        for p, g in zip(self.leaves, self.grads):
            p.grad = g
        self.optimizer = HipAdam(self.leaves, lr=self.lr, weight_decay=float(prior_weight or 0.0))
        self._token = object()       # "the gradients are this loop's persistent buffers" (HipAdam._chunk_table)
        self._ring = HyperRing(3, dev)
        # blind deblurring: theta, its gradient, its own optimiser, ring and norm word, the gradient call's scratch
        self.blind = None if start is None else PsfLogits(self.psf, start, self.image.shape, self.pool, psf_lr, self.steps)

    # ------------------------------------------------------------------ the iteration
    def _body(self, captured):
        blind = self.blind
        if blind is not None:
            blind.forward()
        self._evaluate(self.leaves, self.image, self.loss, self.grads)
        if blind is not None:        # (before the latents move: the gradient belongs to the image and the residual just evaluated)
            blind.gradient(self.image, self.resid, self.inv_wsum)
        self.optimizer.fused_step(0.0, self.max_grad_norm, skip_nonfinite=True, grads_token=self._token,
                                  hyper_dev=self._ring.words if captured else None, norm_out=self.norm)
        if blind is not None:
            blind.update(self.row, captured)
        self.loss_hist.index_copy_(0, self.row, self.loss.view(1, -1))
        self.norm_hist.index_copy_(0, self.row, self.norm)
        self.row.add_(1).remainder_(self.steps)      # (a loop driven past `steps` iterations wraps around instead of writing outside)

    def _capturing(self):
        if self.blind is None:
            return self.optimizer.capturing()
        stack = contextlib.ExitStack()       # both optimisers counted a step that did not run
        stack.enter_context(self.optimizer.capturing())
        stack.enter_context(self.blind.optimizer.capturing())
        return stack

    def _signature(self):
        """`LatentLoop._signature` and the optimiser's part; a blind fit adds theta's optimiser's.  theta, its gradient, its norm
        word and history, the ring and the gradient call's scratch are this loop's own static buffers, like ``psf`` and ``resid``."""
        sig = {**super()._signature(), **self.optimizer.capture_signature()}
        return sig if self.blind is None else {**sig, **self.blind.signature()}

    def _replay_host(self):          # the step count and the 24-byte upload of the iteration's learning rate and bias corrections
        self.optimizer.replay_step(self._ring, self.lr)
        torch.autograd.graph.increment_version(self.leaves)      # (written behind torch's back, as after fused_step)
        if self.blind is not None:
            self.blind.replay_host()

    # ------------------------------------------------------------------ the fit
    @torch.no_grad()
    def reset(self):
        """Back to the start latents with a fresh optimiser state and empty histories (addresses stay: a capture stays valid)."""
        for p, s in zip(self.leaves, self._start):
            p.copy_(s)
        self.optimizer.reset_state()
        self.row.zero_()
        self.loss_hist.zero_()
        self.norm_hist.zero_()
        if self.blind is not None:
            self.blind.reset()

    def latents(self):
        """The current latents (copies)."""
        return Latents(self.leaves[0].detach().clone(), [e.detach().clone() for e in self.leaves[1:]])

    def _run_once(self):
        self.reset()
        replayed = self._iterate()
        parts = [self.loss_hist.reshape(-1), self.norm_hist] + ([] if self.blind is None else [self.blind.norm_hist])
        hist = torch.cat(parts).cpu()                                             # the loop's one host read
        n, k = self.loss_hist.shape[1], self.steps * self.loss_hist.shape[1]
        self._psf_norm = None if self.blind is None else hist[k + self.steps:]
        return hist[:k].view(self.steps, n), hist[k:k + self.steps], replayed

    def run(self, exact=False):
        """The whole fit from the start latents: `RestoreInfo`; the result is in `latents()`.  ``exact``: on the exact-fp32 kernel
        family (restored afterwards).  A non-finite norm anywhere in the history, with ``exact`` off and ``glow.range_check`` on,
        runs the fit ONCE more from the same start on the exact family (the product kernels carry activations as fp16 pairs: a
        latent the fp32 reference handles can be out of their range), as `Inferer.compute_attribute_delta` re-runs its pass; norms
        that are non-finite there too are the problem's own, and the result says ``finite=False``.  Nothing raises."""
        plan = self.plan
        prev = plan.family
        fallback = 0
        try:
            if exact:
                plan.set_family(plan.FAMILY_EXACT_FP32)
            is_finite = lambda norm: bool(torch.isfinite(norm).all()) and (self.blind is None or bool(torch.isfinite(self._psf_norm).all()))
            loss, norm, replayed = self._run_once()
            finite = is_finite(norm)
            if not finite and not exact and getattr(self.glow, "range_check", True):
                fallback = 1
                plan.set_family(plan.FAMILY_EXACT_FP32)
                loss, norm, replayed = self._run_once()
                finite = is_finite(norm)
        finally:
            plan.set_family(prev)
        info = RestoreInfo(loss=loss, grad_norm=norm, finite=finite, captured=replayed, fallback=fallback, graph_error=self.graph_error)
        if self.blind is not None:
            info.psf, info.psf_grad_norm = self.blind.estimate(), self._psf_norm
        return info


class PsfFit:
    """Calibration: the PSF that turns ``sharp`` (N,C,H,W) into ``blurred`` (N,C,H/pool,W/pool), by the iteration of a blind
    `LatentFit` without the flow -- `psf_from_logits`, `restore_objective` with the PSF, `psf_gradient`, theta's fused Adam step
    (`PsfLogits`) -- on the same kernels, device-resident, one host read at the end.  ``start``: `blind_start`'s result;
    ``per_sample``: one PSF per image instead of one for the batch.  EAGER ONLY: the package's capture protocol (`_capture.Capture`)
    is tied to a flow plan, and this loop has none; its iteration is five launches."""

    def __init__(self, sharp, blurred, start, weight=None, pool=1, steps=100, psf_lr=0.2):
        self.x = _lib.require_device_tensor(sharp, "sharp")
        self.target = _lib.require_device_tensor(blurred, "blurred")
        dev, n = self.x.device, self.x.shape[0]
        self.pool, self.steps = int(pool), int(steps)
        if self.steps < 1 or self.pool < 1:
            raise ValueError(f"steps = {steps}, pool = {pool}")
        if self.x.dim() != 4 or tuple(self.target.shape) != (n, self.x.shape[1], self.x.shape[2] // self.pool, self.x.shape[3] // self.pool):
            raise ValueError(f"blurred of shape {tuple(self.target.shape)} does not belong to sharp images {tuple(self.x.shape)} at pool {self.pool}")
        check_psf_shape(start.shape, n)
        self.weight = None if weight is None else _lib.require_device_tensor(weight, "weight").expand_as(self.target).contiguous()
        self.inv_wsum = None if self.weight is None else 1.0 / self.weight.sum(dim=(1, 2, 3)).clamp(min=1.0)
        self.psf = start.to(dev).float().contiguous().clone()
        self.resid = torch.empty_like(self.target)
        self.grad_x = torch.empty_like(self.x)
        self.loss = torch.zeros(n, dtype=torch.float32, device=dev)
        self.loss_hist = torch.zeros((self.steps, n), dtype=torch.float32, device=dev)
        self.row = torch.zeros(1, dtype=torch.int64, device=dev)
        self.blind = PsfLogits(self.psf, start, self.x.shape, self.pool, psf_lr, self.steps)

    @torch.no_grad()
    def run(self):
        """``steps`` iterations from the start: `RestoreInfo` -- ``loss`` (steps, N) BEFORE each update, ``grad_norm`` and
        ``psf_grad_norm`` both theta's gradient norm, ``psf`` the estimate, ``captured`` False."""
        blind = self.blind
        blind.reset()
        self.row.zero_()
        for _ in range(self.steps):
            blind.forward()
            restore_objective(self.x, self.target, self.weight, self.inv_wsum, self.pool, grad_out=self.grad_x, loss_out=self.loss,
                              psf=self.psf, resid_out=self.resid)
            blind.gradient(self.x, self.resid, self.inv_wsum)
            blind.update(self.row, captured=False)
            self.loss_hist.index_copy_(0, self.row, self.loss.view(1, -1))
            self.row.add_(1)
        n = self.loss_hist.shape[1]
        hist = torch.cat([self.loss_hist.reshape(-1), blind.norm_hist]).cpu()      # the loop's one host read
        norm = hist[self.steps * n:]
        return RestoreInfo(loss=hist[:self.steps * n].view(self.steps, n), grad_norm=norm, finite=bool(torch.isfinite(norm).all()),
                           captured=False, psf=blind.estimate(), psf_grad_norm=norm)



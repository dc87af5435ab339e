"""Host tests of the restoration objective observed through a dense linear operator (no GPU): the exports, the argument checks of
glowhip_restore_objective_linear and glowhip_restore_linear_scratch_bytes that need no device, the fp64 oracle of
tests/linear_oracle.py against closed forms (the adjoint identity, the reduction to tests/restore_oracle.py with the identity), a
float32 restatement of the two sums in two orders inside the bound the GPU test uses, the restated Gaussian sensing matrix, the
guards of `Inferer._problem`, and the oracle's own compressed-sensing fit, which fixes the ratio asked of the HIP path."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network import Inferer
from pytorch_glow_amd.network.restore import OPERATOR_STREAM, check_operator_shape

import linear_oracle as L
import restore_oracle as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glowhip.h")
NAMES = ("glowhip_restore_objective_linear", "glowhip_restore_linear_scratch_bytes")


def test_entry_points_are_exported_declared_and_in_the_signature_table():
    text = open(HEADER).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(so, name) and name + "(" in text, name
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 14 and len(_lib.SIGNATURES[NAMES[1]][1]) == 3
    assert "y[n,m]      = sum_d A[m,d] * x[n,d]" in text and "grad_x[n,d] = sum_m A[m,d] * u[n,m]" in text      # the definition
    assert "248 names the Gaussian sensing matrix" in text and OPERATOR_STREAM == L.OPERATOR_STREAM == 248
    assert "gaussian_operator" in G.network.__all__ and callable(G.network.gaussian_operator)
    assert G.lib().glowhip_version() == 102


def test_bad_arguments_are_einval_without_a_device():
    lib = G.lib()
    none = ctypes.c_void_p(None)
    host = ctypes.create_string_buffer(64)       # never read: every case below returns before any device call
    p = ctypes.c_void_p(ctypes.addressof(host))
    big = 1 << 40

    def call(x=p, t=p, A=p, resid=p, g=p, M=3, N=2, D=5, scratch=p, nbytes=big):
        return lib.glowhip_restore_objective_linear(x, t, none, none, A, M, N, D, resid, g, none, scratch, nbytes, none)

    for name in ("x", "t", "A", "resid", "g"):
        assert call(**{name: none}) == -1 and b"null argument" in lib.glowhip_last_error(), name
    for kw, word in ((dict(M=0), b"M and D"), (dict(M=-4), b"M and D"), (dict(D=0), b"M and D"), (dict(D=-1), b"M and D"),
                     (dict(D=1 << 31), b"2^31"), (dict(M=1 << 20, D=1 << 20), b"2^40"), (dict(M=1 << 40, D=1), b"2^40"),
                     (dict(N=-1), b"N < 0")):
        assert call(**kw) == -1 and word in lib.glowhip_last_error(), (kw, lib.glowhip_last_error())
        assert lib.glowhip_restore_linear_scratch_bytes(kw.get("N", 2), kw.get("M", 3), kw.get("D", 5)) == 0
        assert word in lib.glowhip_last_error()
    need = lib.glowhip_restore_linear_scratch_bytes(2, 3, 5)
    assert need > 0
    assert call(scratch=none) == -1 and b"scratch" in lib.glowhip_last_error()
    assert call(nbytes=need - 1) == -1 and b"scratch" in lib.glowhip_last_error()
    assert call(nbytes=0) == -1 and b"scratch" in lib.glowhip_last_error()
    # an empty batch: nothing to do, whatever the scratch
    assert call(N=0) == 0 and call(N=0, scratch=none, nbytes=0) == 0


def test_scratch_bytes_is_monotone_and_zero_only_on_error():
    f = G.lib().glowhip_restore_linear_scratch_bytes
    ns, ms, ds = (0, 1, 3, 4, 5, 8, 9, 64, 65, 67), (1, 3, 8, 67, 128, 129, 130, 1024, 4096), (1, 35, 192, 4096, 4097, 12288)
    size = {(n, m, d): f(n, m, d) for n in ns for m in ms for d in ds}
    assert all(v > 0 and v % 16 == 0 for v in size.values())
    for (n, m, d), v in size.items():
        for n2, m2, d2 in ((ns[min(ns.index(n) + 1, len(ns) - 1)], m, d), (n, ms[min(ms.index(m) + 1, len(ms) - 1)], d),
                           (n, m, ds[min(ds.index(d) + 1, len(ds) - 1)])):
            assert size[(n2, m2, d2)] >= v, ((n, m, d), (n2, m2, d2))
    # the partial y of every D slice, u, and -- with more than one M slice -- the partial gradients
    assert size[(5, 130, 12288)] >= 4 * (3 * 5 * 130 + 130 * 5 + 2 * 5 * 12288)
    assert size[(5, 67, 192)] >= 4 * (5 * 67 + 67 * 5) and size[(5, 67, 192)] < 4 * 5 * 192 + 4 * (5 * 68 + 67 * 8) + 1024


def test_operator_shape_guard():
    assert check_operator_shape((7, 3, 8, 8)) == (7, 192) and check_operator_shape((1, 1, 5, 7), (1, 5, 7)) == (1, 35)
    for shape, image in (((7, 192), None), ((7, 3, 8, 8, 1), None), ((0, 3, 8, 8), None), ((7, 3, 8, 8), (3, 8, 4)), ((7, 3, 8, 8), (1, 8, 8))):
        with pytest.raises(ValueError):
            check_operator_shape(shape, image)


# ------------------------------------------------------------------------------------------------ the oracle against closed forms
def test_adjoint_identity():
    """<A x, v> = <x, A^T v> to 1e-12 relative, and autograd's gradient of <A x, v> is the same A^T v."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, 2, 6, 10), generator=g, dtype=torch.float64)
    A = torch.randn((17, 2, 6, 10), generator=g, dtype=torch.float64)
    v = torch.randn((3, 17), generator=g, dtype=torch.float64)
    lhs, rhs = (L.operator(x, A) * v).sum(), (x * L.operator_T(v, A)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))
    xl = x.clone().requires_grad_(True)
    with torch.enable_grad():
        ga, = torch.autograd.grad((L.operator(xl, A) * v).sum(), [xl])
    assert torch.allclose(ga, L.operator_T(v, A), rtol=1e-12, atol=1e-15)
    # the definition, written out at one entry: y[n,m] = sum_d A[m,d] x[n,d] with d running over (C,H,W) in that order
    y = L.operator(x, A)
    s = sum(float(A[4, c, i, j]) * float(x[1, c, i, j]) for c in range(2) for i in range(6) for j in range(10))
    assert abs(float(y[1, 4]) - s) <= 1e-13


@pytest.mark.parametrize("shape", [(2, 1, 5, 7), (3, 3, 8, 8)], ids=["5x7", "8x8"])
def test_the_identity_operator_is_the_restoration_oracle(shape):
    x, t, w, inv = R.objective_inputs(shape, 1, True)
    dim = x[0].numel()
    eye = torch.eye(dim).view(dim, *shape[1:])
    loss, g, resid = L.objective(x, t.flatten(1), w.flatten(1), inv, eye)
    loss_ref, g_ref = R.objective(x, t, w, inv, 1)
    assert torch.allclose(loss, loss_ref, rtol=1e-14, atol=0) and torch.allclose(g, g_ref, rtol=1e-13, atol=1e-20)
    assert torch.allclose(resid.view(shape), w.double() * (x.double() - t.double()), rtol=1e-14, atol=1e-20)
    # unit weights and the default normalisation: 1 / M is 1 / elements
    loss, g, _ = L.objective(x, t.flatten(1), None, None, eye)
    loss_ref, g_ref = R.objective(x, t, None, None, 1)
    assert torch.allclose(loss, loss_ref, rtol=1e-14, atol=0) and torch.allclose(g, g_ref, rtol=1e-13, atol=1e-20)


def test_gradient_is_the_written_formula():
    """grad_x = A^T (2 inv resid), with `operator_T` (not autograd) on the right."""
    for (shape, m), weighted in zip(L.CASES, (True, False) * 6):
        x, t, w, inv, A = L.objective_inputs(3, shape, m, weighted)
        _, g, resid = L.objective(x, t, w, inv, A)
        k = 2.0 * (torch.full((3,), 1.0 / m, dtype=torch.float64) if inv is None else inv.double())
        by_hand = L.operator_T(k.view(-1, 1) * resid, A.double())
        assert float((g - by_hand).abs().max()) <= 1e-12 * float(g.abs().max())      # (an M-term sum: relative to the largest entry)


# ------------------------------------------------------------------------------------------------ the kernels' sums in float32
def kernel_f32(x, t, w, inv, A, sliced):
    """The sums of csrc/restore_linear.hip in torch float32, one rounding per operation (no fused multiply-add), in two orders:
    ``sliced`` -- the D sum in slices of 4 096 columns cut into chunks of 4 and summed chunk by chunk then slice by slice, the M sum
    in slices of 128 rows -- or element by element from the first to the last.  d, v = w d, u = 2 inv v; the loss's products and sum
    in float64, as there."""
    f32 = torch.float32
    xf, Af, t = x.to(f32).flatten(1), A.to(f32).flatten(1), t.to(f32)
    n, m = t.shape
    w = torch.ones_like(t) if w is None else w.to(f32)
    inv = torch.full((n,), 1.0, dtype=f32) / torch.tensor(float(m), dtype=f32) if inv is None else inv.to(f32)

    def chain(terms):
        out = terms[0]
        for term in terms[1:]:
            out = out + term
        return out

    def product(a, b, inner):
        """sum over the LAST axis of a[:, None, :] * b[None, :, :] in the chosen order."""
        p = a[:, None, :] * b[None, :, :]
        if not sliced:
            return chain([p[..., k] for k in range(p.shape[-1])])
        parts = []
        for s0 in range(0, p.shape[-1], inner):
            sl = p[..., s0:s0 + inner]
            chunks = [chain([sl[..., k] for k in range(c0, min(c0 + 4, sl.shape[-1]))]) for c0 in range(0, sl.shape[-1], 4)]
            parts.append(chain(chunks))
        return chain(parts)

    y = product(xf, Af, 4096)
    d = y - t
    v = w * d
    u = (2.0 * inv).view(-1, 1) * v
    g = product(u, Af.t().contiguous(), 128).view(x.shape)
    loss = ((v.double() * d.double()).sum(dim=1) * inv.double()).to(f32)
    assert all(r.dtype == f32 for r in (y, d, v, u, g, loss))
    return loss, g, v


@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "ones"])
@pytest.mark.parametrize("shape,m", L.CASES, ids=L.CASE_IDS)
def test_float32_restatement_in_two_orders_stays_inside_the_bound(shape, m, weighted):
    """What the GPU test asks of the kernels, fp32 sums deliver on the very inputs it uses (the batch of 3), sliced or element by
    element: nothing in the bound was tuned on the device."""
    x, t, w, inv, A = L.objective_inputs(3, shape, m, weighted)
    loss, g, resid = L.objective(x, t, w, inv, A)
    E_loss, E_g, E_r = L.bound(x, t, w, inv, A)
    assert bool((E_loss > 0).all()) and bool((E_g > 0).all()) and bool((E_r > 0).all())
    for sliced in (True, False):
        l32, g32, r32 = kernel_f32(x, t, w, inv, A, sliced)
        ml, mg, mr = L.worst_multiple(l32, loss, E_loss), L.worst_multiple(g32, g, E_g), L.worst_multiple(r32, resid, E_r)
        print(f"{shape} M {m} {'weighted' if weighted else 'ones'} sliced={sliced}: worst multiple of the bound  "
              f"loss {ml:.3f}  grad {mg:.3f}  resid {mr:.3f}")
        assert ml <= 1.0 and mg <= 1.0 and mr <= 1.0


# ------------------------------------------------------------------------------------------------ the Gaussian sensing matrix
def test_gaussian_operator_restated_has_the_stated_moments_and_is_a_function_of_its_name():
    m, shape = 64, (3, 16, 16)
    a = L.gaussian_operator(m, shape, 11)
    assert tuple(a.shape) == (m,) + shape and a.dtype == torch.float64
    count = a.numel()
    mean, var = float(a.mean()), float(a.var())
    se_mean, se_var = (1.0 / m / count) ** 0.5, (2.0 / count) ** 0.5 / m
    print(f"mean {mean:+.3e} ({mean / se_mean:+.2f} se)  variance * m - 1 {var * m - 1:+.3e} ({(var - 1.0 / m) / se_var:+.2f} se)")
    assert abs(mean) <= 4.0 * se_mean and abs(var - 1.0 / m) <= 4.0 * se_var
    assert torch.equal(a, L.gaussian_operator(m, shape, 11))
    assert not torch.equal(a, L.gaussian_operator(m, shape, 12))
    # the name is (m, shape, seed): the first rows of a taller matrix of the same seed are the same draws at another scale
    b = L.gaussian_operator(2 * m, shape, 11)
    ratio = float(np.float32(1.0 / np.sqrt(2.0 * m))) / float(np.float32(1.0 / np.sqrt(float(m))))
    assert torch.allclose(b[:m], a * ratio, rtol=1e-15, atol=0)
    # stream 248 at call 0, element = flat index, std = float32(1 / sqrt(m))
    import sampler_oracle as SO
    e = SO.normal(8, 11, 0, 248, 1.0)
    assert np.allclose(a.view(-1)[:8].numpy(), e * float(np.float32(0.125)), rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------ the guards of Inferer._problem
def test_inferer_guards_need_no_device():
    """Every refusal of an operator is a ValueError raised before any device work: the stand-in has no device at all."""
    inf = object.__new__(Inferer)
    inf.graph = types.SimpleNamespace(flow=types.SimpleNamespace(in_chw=(3, 8, 8)))
    inf.device = None
    A = torch.zeros(7, 3, 8, 8)
    t = torch.zeros(2, 7)
    bad = [dict(psf=torch.ones(3, 3)), dict(pool=2), dict(measurement=torch.zeros(2, 8)), dict(measurement=torch.zeros(8)),
           dict(measurement=torch.zeros(2, 3, 7)), dict(weight=torch.ones(2, 6)), dict(weight=torch.ones(3, 7)),
           dict(operator=torch.zeros(7, 192)), dict(operator=torch.zeros(7, 3, 8, 4)), dict(operator=torch.zeros(7, 1, 8, 8)),
           dict(chains=2), dict(chains=0)]
    for kw in bad:
        args = dict(measurement=t, weight=None, pool=1, init=None, chains=1, psf=None, operator=A)
        args.update(kw)
        with pytest.raises(ValueError):
            inf._problem(**args)
    # the last guard before the device: the operator is held by reference, so it must already be a device tensor
    with pytest.raises(ValueError, match="by reference"):
        inf._problem(measurement=t, weight=torch.ones(7), pool=1, init=None, chains=1, psf=None, operator=A)


# ------------------------------------------------------------------------------------------------ the fit that fixes the GPU ratio
def test_oracle_fit_fixes_the_ratio_asked_of_the_hip_path():
    """Adam in fp64 from the all-zero latents on the 16x16x3 model (D = 768) observed through M = 256 Gaussian rows, 40 steps at lr
    0.1: the samples' final / first data terms are 0.0034, 0.0041, 0.0037.  The threshold asked of the GPU fit is the smallest of
    0.1 / 0.2 / 0.5 that is at least twice the worst of them: 0.1.  (A ratio above 0.25 would make the problem too hard for a test.)"""
    case = L.fit_case()
    hist = case["history"]
    assert tuple(hist.shape) == (case["steps"], case["ref"]["cfg"]["batch"])
    ratios = (hist[-1] / hist[0]).tolist()
    print("first", [f"{v:.3e}" for v in hist[0].tolist()], "last", [f"{v:.3e}" for v in hist[-1].tolist()],
          "final / first", [f"{r:.4f}" for r in ratios])
    assert bool((hist[-1] < hist[0]).all()) and bool(torch.isfinite(hist).all())
    assert max(ratios) <= 0.25
    assert L.threshold_of(max(ratios)) == case["ratio"] == 0.1

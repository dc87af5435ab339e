"""Host tests of multi-coil k-space (no GPU): the exports and the ABI trio, the argument checks of glowhip_restore_objective_coils,
glowhip_coils2d and glowhip_restore_coils_scratch_bytes that need no device, the fp64 oracle of tests/coil_oracle.py against the
written formula and fp64 autograd, the adjoint identity, Q = 1 with unit maps against `fourier_oracle`, a float32 restatement of the
three passes in two butterfly orders inside the bound the GPU test uses, `coil_maps`, every ValueError of the Python layers, and the
oracle's own multi-coil fit, which fixes the ratio asked of the HIP path."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network import COILS_MAX, Inferer, LatentFit, LatentMALA, check_coil_maps, coil_maps, restore_objective

import coil_oracle as C
import fourier_oracle as F
import linear_oracle as L
from test_fourier_host import fft_f32

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glowhip.h")
NAMES = ("glowhip_restore_objective_coils", "glowhip_restore_coils_scratch_bytes", "glowhip_coils2d")


def test_entry_points_are_exported_declared_and_in_the_signature_table():
    text = open(HEADER).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(so, name) and name + "(" in text and f" T {name}\n" in exported, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [17, 5, 11]
    for line in ("Y[n,c,q]    = F ( S[q] * x[n,c] )", "grad_x[n,c] = 2 inv_wsum[n] * sum_q Re( conj(S[q]) * F^H resid[n,c,q] )",
                 "VALUE-equal", "the sign of a zero", "Shared maps and the same maps repeated per sample give the same bits"):
        assert line in text, line                                                                  # the definition and the guarantees
    for name in ("COILS_MAX", "check_coil_maps", "coil_maps", "coils2d", "coils2d_adjoint", "coils_scratch"):
        assert name in G.network.__all__ and hasattr(G.network, name), name
    assert COILS_MAX == 32 and G.lib().glowhip_version() == 102


def test_bad_arguments_are_einval_without_a_device():
    lib = G.lib()
    none = ctypes.c_void_p(None)
    host = ctypes.create_string_buffer(64)       # never read: every case below returns before any device call
    p = ctypes.c_void_p(ctypes.addressof(host) + (-ctypes.addressof(host)) % 16)
    big = 1 << 40
    far = lambda k: ctypes.c_void_p(p.value + (k << 20))     # (addresses only: nothing is dereferenced)
    N, Cc, Q, H, W = 2, 3, 4, 8, 4

    def call(x=far(1), t=p, maps=far(8), stride=0, resid=far(2), g=far(4), N=N, C=Cc, Q=Q, H=H, W=W, scratch=p, nbytes=big):
        return lib.glowhip_restore_objective_coils(x, t, none, none, maps, stride, N, C, Q, H, W, resid, g, none, scratch, nbytes, none)

    for name in ("x", "t", "maps", "resid", "g"):
        assert call(**{name: none}) == -1 and b"null argument" in lib.glowhip_last_error(), name
    sides = (dict(H=0), dict(H=1), dict(W=1), dict(H=3), dict(W=12), dict(H=24), dict(W=255), dict(H=512), dict(W=1024), dict(H=-8))
    for kw in sides + (dict(N=-1), dict(C=0), dict(Q=0), dict(Q=33), dict(Q=-1)):
        word = b"power of two" if ("H" in kw or "W" in kw) else b"coils" if "Q" in kw else b"N < 0 or C < 1"
        assert call(**kw) == -1 and word in lib.glowhip_last_error(), (kw, lib.glowhip_last_error())
        args = [kw.get(k, v) for k, v in (("N", N), ("C", Cc), ("Q", Q), ("H", H), ("W", W))]
        assert lib.glowhip_restore_coils_scratch_bytes(*args) == 0 and word in lib.glowhip_last_error()
        assert lib.glowhip_coils2d(far(1), far(8), 0, far(2), *args, 0, none) == -1 and word in lib.glowhip_last_error()
    # the stride of the maps: 0 or Q H W 2, nothing else
    for stride in (1, Q * H * W, Q * H * W * 2 + 2, -Q * H * W * 2, H * W * 2):
        assert call(stride=stride) == -1 and b"maps_stride" in lib.glowhip_last_error(), stride
        assert lib.glowhip_coils2d(far(1), far(8), stride, far(2), N, Cc, Q, H, W, 0, none) == -1 and b"maps_stride" in lib.glowhip_last_error()
    # a grid of more than 2^31 workgroups: N C Q planes of 256 x 256 make 32 row tiles each
    assert call(N=1 << 20, C=4, Q=32, H=256, W=256) == -1 and b"2^31" in lib.glowhip_last_error()
    assert lib.glowhip_restore_coils_scratch_bytes(1 << 20, 4, 32, 256, 256) == 0
    need = lib.glowhip_restore_coils_scratch_bytes(N, Cc, Q, H, W)
    assert need >= N * Cc * Q * H * W * 8 and need % 16 == 0      # at least the complex intermediate of the adjoint
    assert call(scratch=none) == -1 and b"scratch" in lib.glowhip_last_error()
    assert call(nbytes=need - 1) == -1 and b"scratch" in lib.glowhip_last_error()
    assert call(nbytes=0) == -1 and b"scratch" in lib.glowhip_last_error()
    assert call(scratch=ctypes.c_void_p(p.value + 4)) == -1 and b"scratch" in lib.glowhip_last_error()      # misaligned
    # x, grad_x, resid and maps must not overlap: the same address, and ranges that meet by one element
    real_bytes = N * Cc * H * W * 4
    for kw in (dict(g=far(1)), dict(resid=far(1)), dict(g=far(2)), dict(maps=far(4)), dict(maps=far(2)), dict(maps=far(1)),
               dict(g=ctypes.c_void_p(far(1).value + real_bytes - 4)), dict(maps=ctypes.c_void_p(far(2).value + 2 * Q * real_bytes - 8)),
               dict(maps=ctypes.c_void_p(far(4).value - Q * H * W * 8 + 8)),
               dict(maps=ctypes.c_void_p(far(4).value - N * Q * H * W * 8 + 8), stride=Q * H * W * 2)):
        assert call(**kw) == -1 and b"overlap" in lib.glowhip_last_error(), (kw, lib.glowhip_last_error())
    # shared maps end where per-sample maps would not: the same address is fine with stride 0 and overlaps with the full stride
    edge = ctypes.c_void_p(far(4).value - Q * H * W * 8)
    assert call(maps=edge, stride=Q * H * W * 2) == -1 and b"overlap" in lib.glowhip_last_error()
    # the operator alone
    ok = (far(1), far(8), 0, far(2), N, Cc, Q, H, W)
    for k in (0, 1, 3):
        args = list(ok)
        args[k] = none
        assert lib.glowhip_coils2d(*args, 0, none) == -1 and b"null" in lib.glowhip_last_error()
    assert lib.glowhip_coils2d(*ok, 2, none) == -1 and b"adjoint" in lib.glowhip_last_error()
    assert lib.glowhip_coils2d(far(1), far(8), 0, far(1), N, Cc, Q, H, W, 0, none) == -1 and b"overlap" in lib.glowhip_last_error()
    assert lib.glowhip_coils2d(far(1), far(2), 0, far(2), N, Cc, Q, H, W, 1, none) == -1 and b"overlap" in lib.glowhip_last_error()
    # an empty batch: nothing to do, whatever the scratch
    assert call(N=0) == 0 and call(N=0, scratch=none, nbytes=0) == 0
    assert lib.glowhip_coils2d(far(1), far(8), 0, far(2), 0, Cc, Q, H, W, 1, none) == 0


def test_scratch_bytes_is_monotone_in_n_c_and_q_and_zero_only_on_error():
    f = G.lib().glowhip_restore_coils_scratch_bytes
    for h, w in ((2, 2), (8, 4), (64, 64), (256, 2), (2, 256), (256, 256)):
        sizes = [f(n, c, q, h, w) for n in (0, 1, 3, 5, 64, 67) for c in (1, 3) for q in (1, 2, 8, 32)]
        assert all(v > 0 and v % 16 == 0 for v in sizes)
        assert f(0, 1, 1, h, w) <= f(1, 1, 1, h, w) <= f(1, 1, 2, h, w) <= f(1, 3, 2, h, w) <= f(3, 3, 2, h, w) <= f(3, 3, 32, h, w) \
            <= f(64, 3, 32, h, w) <= f(67, 3, 32, h, w)
        assert f(5, 3, 8, h, w) >= 5 * 3 * 8 * h * w * 8
        assert f(5, 3, 1, h, w) == G.lib().glowhip_restore_fourier_scratch_bytes(5, 3, h, w)      # one coil: the plain call's
    assert f(1, 1, 0, 8, 8) == 0 and f(1, 1, 33, 8, 8) == 0 and f(1, 0, 1, 8, 8) == 0 and f(-1, 1, 1, 8, 8) == 0


# ------------------------------------------------------------------------------------------------ the oracle against closed forms
def test_gradient_is_the_written_formula_and_fp64_autograd():
    """grad_x = 2 inv sum_q Re(conj(S_q) F^H resid_q) with `adjoint` (not autograd) on the right; the two agree to fp64 rounding.
    Shared and per-sample maps."""
    for k, (case, weights) in enumerate(zip(C.CASES, C.WEIGHTS * 4)):
        x, t, maps, w, inv = C.objective_inputs(3, case, weights, per_sample=bool(k % 2))
        loss, g, resid = C.objective(x, t, maps, w, inv)
        assert tuple(resid.shape) == (3,) + case and tuple(g.shape) == tuple(x.shape)
        kk = 2.0 * (torch.full((3,), 1.0 / t[0].numel(), dtype=torch.float64) if inv is None else inv.double())
        by_hand = kk.view(-1, 1, 1, 1) * C.adjoint(resid, maps)
        assert float((g - by_hand).abs().max()) <= 1e-13 * max(float(g.abs().max()), 1e-30), case
        ww = torch.ones_like(x, dtype=torch.float64) if w is None else w.double()
        d = C.forward(x, maps) - C.as_complex(t)
        assert torch.allclose(loss, kk / 2.0 * (ww.unsqueeze(2) * d.abs() ** 2).sum(dim=(1, 2, 3, 4)), rtol=1e-13, atol=0)
        assert torch.allclose(resid, ww.unsqueeze(2) * d)


def test_adjoint_identity_and_one_coefficient_written_out():
    """<A x, k> = <x, A^H k> for real x (the real inner product of C^n: Re sum conj(a) b), shared and per-sample maps; and one
    coefficient of A x by its defining sum."""
    g = torch.Generator().manual_seed(5)
    n, c, q, h, w = 2, 3, 5, 8, 16
    x = torch.randn((n, c, h, w), generator=g, dtype=torch.float64)
    cn = lambda s: torch.complex(torch.randn(s, generator=g, dtype=torch.float64), torch.randn(s, generator=g, dtype=torch.float64))
    k = cn((n, c, q, h, w))
    for maps in (cn((q, h, w)), cn((n, q, h, w))):
        lhs, rhs = (C.forward(x, maps).conj() * k).real.sum(), (x * C.adjoint(k, maps)).sum()
        assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))
    maps = cn((n, q, h, w))
    u, v = 3, 5
    s = sum(complex(maps[1, 4, i, j]) * complex(x[1, 2, i, j]) * np.exp(-2j * np.pi * (u * i / h + v * j / w))
            for i in range(h) for j in range(w)) / np.sqrt(h * w)
    assert abs(complex(C.forward(x, maps)[1, 2, 4, u, v]) - s) <= 1e-13


def test_one_coil_with_unit_maps_is_the_fourier_oracle():
    for shape, weights in zip(F.SHAPES[:6], F.WEIGHTS * 2):
        x, t, w, inv = F.objective_inputs(3, shape, weights)
        ones = torch.ones((1,) + shape[1:], dtype=torch.complex64)
        loss, g, r = C.objective(x, t.unsqueeze(2), ones, w, inv)
        loss_f, g_f, r_f = F.objective(x, t, w, inv)
        assert torch.allclose(loss, loss_f, rtol=1e-14, atol=0) and torch.allclose(g, g_f, rtol=1e-13, atol=1e-18)
        assert torch.equal(r.squeeze(2), r_f)
        # and the bound contains the plain call's: every rounding of that call is still there
        E, Ef = C.bound(x, t.unsqueeze(2), ones, w, inv), F.bound(x, t, w, inv)
        assert bool((E[0] >= Ef[0]).all()) and bool((E[1] >= Ef[1]).all()) and bool((E[2].squeeze(2) >= Ef[2]).all())


# ------------------------------------------------------------------------------------------------ the three passes in float32
def kernel_f32(x, t, maps, w, inv, kernel_order):
    """The three launches in numpy float32, one rounding per operation.  ``kernel_order`` True: the kernels' own -- the tile
    (S.re x, S.im x), forward rows then columns by decimation in time, the scaling, d, r = w d, u = 2 inv r, adjoint columns then
    rows by decimation in frequency, S.re G.re + S.im G.im summed in coil order from zero, the scaling.  False: the other butterfly
    order everywhere (columns first and decimation in frequency forward, rows first and decimation in time back); the coil sum stays
    in coil order.  The loss's products and sum in float64, as there."""
    f32 = np.float32
    xn = x.numpy().astype(f32)
    n, c, h, wd = xn.shape
    s = torch.view_as_real(maps if maps.dim() == 4 else maps.unsqueeze(0)).numpy().astype(f32)      # (1 or N, Q, H, W, 2)
    q = s.shape[1]
    sr, si = s[:, None, ..., 0], s[:, None, ..., 1]                                                    # (1 or N, 1, Q, H, W)
    tn = torch.view_as_real(t).numpy().astype(f32)
    wn = (np.ones_like(xn) if w is None else w.numpy().astype(f32))[:, :, None]
    invn = (np.full((n,), 1.0, f32) / f32(c * q * h * wd)) if inv is None else inv.numpy().astype(f32)
    scale = f32(1.0 / np.sqrt(float(h) * float(wd)))
    fwd_axes, fwd_kind, adj_axes, adj_kind = ((4, 3), "dit", (3, 4), "dif") if kernel_order else ((3, 4), "dif", (4, 3), "dit")
    re, im = sr * xn[:, :, None], si * xn[:, :, None]
    for axis in fwd_axes:
        re, im = fft_f32(re, im, axis, False, fwd_kind)
    dr, di = re * scale - tn[..., 0], im * scale - tn[..., 1]
    rr, ri = wn * dr, wn * di
    two_inv = (f32(2.0) * invn).reshape(n, 1, 1, 1, 1)
    ur, ui = two_inv * rr, two_inv * ri
    for axis in adj_axes:
        ur, ui = fft_f32(ur, ui, axis, True, adj_kind)
    acc = np.zeros_like(xn)
    for k in range(q):
        term = sr[:, :, k] * ur[:, :, k] + si[:, :, k] * ui[:, :, k]
        acc = acc + term
    g = acc * scale
    loss = ((rr.astype(np.float64) * dr + ri.astype(np.float64) * di).sum(axis=(1, 2, 3, 4)) * invn.astype(np.float64)).astype(f32)
    assert all(v.dtype == f32 for v in (re, dr, rr, ur, acc, g, loss))
    return torch.from_numpy(loss), torch.from_numpy(g), torch.complex(torch.from_numpy(rr), torch.from_numpy(ri))


@pytest.mark.parametrize("weights", C.WEIGHTS)
@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_float32_restatement_in_two_butterfly_orders_stays_inside_the_bound(case, weights):
    """What the GPU test asks of the kernels, an fp32 restatement of the three passes delivers on the very inputs it uses (the batch
    of 3), in the kernels' butterfly order and in the opposite one: nothing in the bound was tuned on the device."""
    x, t, maps, w, inv = C.objective_inputs(3, case, weights)
    loss, g, resid = C.objective(x, t, maps, w, inv)
    E_loss, E_g, E_r = C.bound(x, t, maps, w, inv)
    assert bool((E_loss > 0).all()) and bool((E_g > 0).all()) and bool((E_r > 0).all())
    assert tuple(E_g.shape) == tuple(x.shape) and tuple(E_r.shape) == tuple(resid.shape)
    for kernel_order in (True, False):
        l32, g32, r32 = kernel_f32(x, t, maps, w, inv, kernel_order)
        ml, mg, mr = C.worst_multiple(l32, loss, E_loss), C.worst_multiple(g32, g, E_g), C.complex_multiple(r32, resid, E_r)
        print(f"{case} {weights} kernel_order={kernel_order}: worst multiple of the bound  loss {ml:.3f}  grad {mg:.3f}  resid {mr:.3f}")
        assert ml <= 1.0 and mg <= 1.0 and mr <= 1.0
        assert mg > 0.0 and mr > 0.0      # (fp32 is not fp64: the comparison is not vacuous)


def test_float32_restatement_with_per_sample_maps_stays_inside_the_bound():
    for case in ((3, 3, 4, 8), (1, 2, 2, 2)):
        x, t, maps, w, inv = C.objective_inputs(3, case, "real", per_sample=True)
        assert maps.dim() == 4 and not torch.equal(maps[0], maps[1])
        loss, g, resid = C.objective(x, t, maps, w, inv)
        E_loss, E_g, E_r = C.bound(x, t, maps, w, inv)
        l32, g32, r32 = kernel_f32(x, t, maps, w, inv, True)
        assert C.worst_multiple(l32, loss, E_loss) <= 1.0 and C.worst_multiple(g32, g, E_g) <= 1.0
        assert C.complex_multiple(r32, resid, E_r) <= 1.0


# ------------------------------------------------------------------------------------------------ the maps
def test_coil_maps_are_normalised_deterministic_and_the_docstring_formula():
    for hw, q in (((16, 16), 4), ((8, 32), 5), ((64, 64), 8), ((4, 4), 32), ((5, 7), 1)):
        s = coil_maps(hw, q)
        assert s.dtype == torch.complex64 and tuple(s.shape) == (q,) + hw and s.is_contiguous()
        energy = (s.to(torch.complex128).abs() ** 2).sum(dim=0)
        assert float((energy - 1.0).abs().max()) <= 4.0 * q * F.U      # each of Q complex64 values carries u, squared: 2 u each
        assert torch.equal(s, coil_maps(hw, q)) and torch.equal(s, coil_maps(hw, q, width=0.6, seed=0))
        assert q == 1 or not torch.equal(s, coil_maps(hw, q, seed=1))
        if hw[0] * hw[1] <= 256:
            ref = C.maps_formula(hw, q)
            assert float((s.to(torch.complex128) - ref).abs().max()) <= 2.0 * F.U + 1e-12, (hw, q)
    s = coil_maps((16, 16), 4)
    mags = s.abs()
    assert float(mags.min()) > 0.0 and len({int(mags[k].argmax()) for k in range(4)}) == 4      # every coil has its own bright spot
    assert not torch.equal(coil_maps((16, 16), 4, width=0.3), s)
    for kw in (dict(q=0), dict(q=33), dict(width=0.0), dict(width=-1.0), dict(hw=(0, 4))):
        with pytest.raises(ValueError):
            coil_maps(**dict(dict(hw=(8, 8), q=4), **kw))


# ------------------------------------------------------------------------------------------------ the guards, without a device
def test_check_coil_maps():
    s = torch.zeros(4, 8, 16, dtype=torch.complex64)
    real, q, per = check_coil_maps(s, 3, (8, 16))
    assert tuple(real.shape) == (4, 8, 16, 2) and real.dtype == torch.float32 and q == 4 and per is False
    real, q, per = check_coil_maps(torch.zeros(3, 4, 8, 16, 2), 3, (8, 16))
    assert tuple(real.shape) == (3, 4, 8, 16, 2) and q == 4 and per is True
    assert check_coil_maps(torch.zeros(32, 8, 16, dtype=torch.complex64), 1, (5, 3, 8, 16))[1] == 32
    for bad in (torch.zeros(4, 8, 16), torch.zeros(4, 8, 16, dtype=torch.complex128), torch.zeros(4, 8, 8, dtype=torch.complex64),
                torch.zeros(2, 4, 8, 16, dtype=torch.complex64), torch.zeros(33, 8, 16, dtype=torch.complex64),
                torch.zeros(0, 8, 16, dtype=torch.complex64), torch.zeros(8, 16, dtype=torch.complex64),
                torch.zeros(1, 3, 4, 8, 16, dtype=torch.complex64), torch.zeros(4, 8, 16, 2, dtype=torch.float64)):
        with pytest.raises(ValueError):
            check_coil_maps(bad, 3, (8, 16))
    with pytest.raises(TypeError):
        check_coil_maps([[1.0]], 3, (8, 16))


def test_restore_objective_refuses_coils_without_fourier_before_anything_else():
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="fourier=True"):
        restore_objective(x, torch.zeros(2, 3, 4, 8, 8, 2), coils=torch.zeros(4, 8, 8, dtype=torch.complex64))


def test_inferer_guards_need_no_device():
    """Every refusal of a multi-coil problem is a ValueError raised before any device work: the stand-in has no device at all."""
    def inferer(chw):
        inf = object.__new__(Inferer)
        inf.graph = types.SimpleNamespace(flow=types.SimpleNamespace(in_chw=chw), hps=types.SimpleNamespace(ablation={}))
        inf.device = None
        return inf

    k = torch.zeros(2, 3, 4, 8, 8, dtype=torch.complex64)
    s = torch.zeros(4, 8, 8, dtype=torch.complex64)
    bad = [dict(psf=torch.ones(3, 3)), dict(operator=torch.zeros(7, 3, 8, 8)), dict(estimate_psf="shared"), dict(pool=2),
           dict(measurement=torch.zeros(2, 3, 4, 8, 8)), dict(measurement=torch.zeros(2, 3, 4, 8, 4, dtype=torch.complex64)),
           dict(measurement=torch.zeros(2, 1, 4, 8, 8, dtype=torch.complex64)), dict(measurement=torch.zeros(4, 8, 8, dtype=torch.complex64)),
           dict(measurement=torch.zeros(2, 3, 5, 8, 8, dtype=torch.complex64)), dict(measurement=torch.zeros(2, 3, 8, 8, dtype=torch.complex64)),
           dict(coils=torch.zeros(4, 8, 4, dtype=torch.complex64)), dict(coils=torch.zeros(3, 4, 8, 8, dtype=torch.complex64)),
           dict(coils=torch.zeros(4, 8, 8)), dict(coils=torch.zeros(33, 8, 8, dtype=torch.complex64)),
           dict(weight=-torch.ones(8, 8)), dict(weight=torch.ones(8, 4)), dict(weight=torch.ones(3, 3, 8, 8)),
           dict(weight=torch.ones(2, 3, 4, 8, 8)), dict(chains=2), dict(chains=0)]
    for kw in bad:
        args = dict(measurement=k, weight=None, pool=1, init=None, chains=1, psf=None, operator=None, estimate_psf=None, coils=s)
        args.update(kw)
        with pytest.raises(ValueError):
            inferer((3, 8, 8))._coils_problem(**args)
    # a side that is not a power of two, and one above 256, whatever the model says
    for chw in ((3, 12, 8), (1, 8, 512)):
        with pytest.raises(ValueError, match="power of two"):
            inferer(chw)._coils_problem(torch.zeros((2, chw[0], 4) + chw[1:], dtype=torch.complex64), None, 1, None, 1, None, None, None,
                                        torch.zeros((4,) + chw[1:], dtype=torch.complex64))
    # the public entry points: coils without fourier, and with what it excludes
    for call in (lambda **kw: inferer((3, 8, 8)).restore(k, **kw), lambda **kw: inferer((3, 8, 8)).posterior(k, **kw)):
        with pytest.raises(ValueError, match="fourier=True"):
            call(coils=s)
        for kw in (dict(psf=torch.ones(3, 3)), dict(operator=torch.zeros(7, 3, 8, 8)), dict(pool=2)):
            with pytest.raises(ValueError, match="exclude"):
                call(coils=s, fourier=True, **kw)
    with pytest.raises(ValueError, match="exclude"):
        inferer((3, 8, 8)).restore(k, coils=s, fourier=True, estimate_psf="shared", psf=(3, 3))


def test_loop_guards_need_no_device():
    """`LatentFit` and `LatentMALA` refuse the exclusions and the sizes before they touch the measurement's device."""
    glow = types.SimpleNamespace(hps=types.SimpleNamespace(ablation={}))
    k = torch.zeros(2, 3, 4, 8, 8, dtype=torch.complex64)
    s = torch.zeros(4, 8, 8, dtype=torch.complex64)
    init = object()
    for kw in (dict(psf=torch.ones(3, 3)), dict(operator=torch.zeros(7, 3, 8, 8)), dict(pool=2), dict(fourier=False),
               dict(measurement=torch.zeros(2, 3, 4, 12, 8, dtype=torch.complex64)), dict(measurement=torch.zeros(2, 3, 4, 8, 8)),
               dict(measurement=torch.zeros(2, 3, 8, 8, dtype=torch.complex64)), dict(measurement=torch.zeros(2, 3, 5, 8, 8, dtype=torch.complex64)),
               dict(coils=torch.zeros(4, 8, 4, dtype=torch.complex64)), dict(coils=torch.zeros(3, 4, 8, 8, dtype=torch.complex64)),
               dict(coils=torch.zeros(33, 8, 8, dtype=torch.complex64)), dict(coils=torch.zeros(4, 8, 8))):
        for cls in (LatentFit, LatentMALA):
            with pytest.raises(ValueError):
                cls(glow, **dict(dict(measurement=k, init=init, steps=2, fourier=True, coils=s), **kw))
    with pytest.raises(ValueError):
        LatentFit(glow, k, init=init, steps=2, fourier=True, coils=s, estimate_psf="shared", psf=(3, 3))


# ------------------------------------------------------------------------------------------------ the fit that fixes the GPU ratio
def test_oracle_fit_fixes_the_ratio_asked_of_the_hip_path():
    """Adam in fp64 on the 16x16x3 model seen by 4 coils (`coil_maps((16, 16), 4)`) through 4 of its 16 k-space rows
    (`fourier_mask((16, 16), 0.25)`), from the encode of the coil-combined zero-filled image, 40 steps at lr 0.1: the samples'
    final / first data terms are 0.0187, 0.0165, 0.0175.  The threshold asked of the GPU fit is the smallest of 0.1 / 0.2 / 0.5 that is at
    least twice the worst of them -- the margin of tests/test_linear_host.py: 0.1.  (A ratio above 0.25 would make the problem too hard
    for a test.)"""
    case = C.fit_case()
    hist = case["history"]
    assert tuple(hist.shape) == (case["steps"], case["ref"]["cfg"]["batch"])
    assert int(case["mask"][:, 0].sum()) == 4 and float(case["mask"][0, 0]) == 1.0 and tuple(case["maps"].shape) == (4, 16, 16)
    ratios = (hist[-1] / hist[0]).tolist()
    print("first", [f"{v:.3e}" for v in hist[0].tolist()], "last", [f"{v:.3e}" for v in hist[-1].tolist()],
          "final / first", [f"{r:.4f}" for r in ratios])
    assert bool((hist[-1] < hist[0]).all()) and bool(torch.isfinite(hist).all())
    assert max(ratios) <= 0.25
    assert C.threshold_of(max(ratios)) == L.threshold_of(max(ratios)) == case["ratio"]

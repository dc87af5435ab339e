"""Host tests of the restoration objective observed in the Fourier domain (no GPU): the exports and the ABI trio, the argument checks
of glowhip_restore_objective_fourier, glowhip_fourier2d and glowhip_restore_fourier_scratch_bytes that need no device, the fp64 oracle
of tests/fourier_oracle.py against fp64 autograd, Parseval and the adjoint identity, a float32 restatement of the radix-2 transform in
two butterfly orders inside the bound the GPU test uses, `fourier_mask`, every ValueError of the Python layers, and the oracle's own
k-space fit, which fixes the ratio asked of the HIP path."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network import Inferer, LatentFit, LatentMALA, check_fourier_shape, fourier_mask
from pytorch_glow_amd.network.restore import FOURIER_MAX, as_kspace

import fourier_oracle as F
import linear_oracle as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glowhip.h")
NAMES = ("glowhip_restore_objective_fourier", "glowhip_restore_fourier_scratch_bytes", "glowhip_fourier2d")


def test_entry_points_are_exported_declared_and_in_the_signature_table():
    text = open(HEADER).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(so, name) and name + "(" in text and f" T {name}\n" in exported, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [14, 4, 7]
    assert "grad_x      = 2 inv_wsum[n] * Re( F^H resid )" in text and 'torch.fft.fft2(norm="ortho")' in text      # the definition
    for name in ("fourier2d", "fourier2d_adjoint", "fourier_mask", "fourier_scratch", "check_fourier_shape"):
        assert name in G.network.__all__ and callable(getattr(G.network, name)), name
    assert G.lib().glowhip_version() == 102


def test_bad_arguments_are_einval_without_a_device():
    lib = G.lib()
    none = ctypes.c_void_p(None)
    host = ctypes.create_string_buffer(64)       # never read: every case below returns before any device call
    p = ctypes.c_void_p(ctypes.addressof(host) + (-ctypes.addressof(host)) % 16)
    big = 1 << 40

    def call(x=p, t=p, resid=p, g=p, N=2, C=3, H=8, W=4, scratch=p, nbytes=big):
        return lib.glowhip_restore_objective_fourier(x, t, none, none, N, C, H, W, resid, g, none, scratch, nbytes, none)

    for name in ("x", "t", "resid", "g"):
        assert call(**{name: none}) == -1 and b"null argument" in lib.glowhip_last_error(), name
    sides = (dict(H=0), dict(H=1), dict(W=1), dict(H=3), dict(W=12), dict(H=24), dict(W=255), dict(H=512), dict(W=1024), dict(H=-8))
    for kw in sides + (dict(N=-1), dict(C=0)):
        word = b"power of two" if ("H" in kw or "W" in kw) else b"N < 0 or C < 1"
        assert call(**kw) == -1 and word in lib.glowhip_last_error(), (kw, lib.glowhip_last_error())
        assert lib.glowhip_restore_fourier_scratch_bytes(kw.get("N", 2), kw.get("C", 3), kw.get("H", 8), kw.get("W", 4)) == 0
        assert word in lib.glowhip_last_error()
    for kw in sides:
        assert lib.glowhip_fourier2d(p, p, 1, kw.get("H", 8), kw.get("W", 4), 0, none) == -1 and b"power of two" in lib.glowhip_last_error()
    need = lib.glowhip_restore_fourier_scratch_bytes(2, 3, 8, 4)
    assert need >= 2 * 3 * 8 * 4 * 8 and need % 16 == 0      # at least the complex intermediate of the adjoint
    far = lambda k: ctypes.c_void_p(p.value + (k << 20))     # (addresses only: nothing is dereferenced)
    ok = dict(x=far(1), resid=far(2), g=far(4))
    assert call(scratch=none, **ok) == -1 and b"scratch" in lib.glowhip_last_error()
    assert call(nbytes=need - 1, **ok) == -1 and b"scratch" in lib.glowhip_last_error()
    assert call(nbytes=0, **ok) == -1 and b"scratch" in lib.glowhip_last_error()
    assert call(scratch=ctypes.c_void_p(p.value + 4), **ok) == -1 and b"scratch" in lib.glowhip_last_error()      # misaligned
    # x, grad_x and resid must not overlap: the same address, and ranges that meet by one element
    for kw in (dict(x=far(1), g=far(1), resid=far(2)), dict(x=far(1), g=far(4), resid=far(1)), dict(x=far(1), g=far(2), resid=far(2)),
               dict(x=far(1), g=ctypes.c_void_p(far(1).value + 2 * 3 * 8 * 4 * 4 - 4), resid=far(2))):
        assert call(**kw) == -1 and b"overlap" in lib.glowhip_last_error(), lib.glowhip_last_error()
    # the transform alone
    assert lib.glowhip_fourier2d(none, p, 1, 8, 4, 0, none) == -1 and lib.glowhip_fourier2d(p, none, 1, 8, 4, 0, none) == -1
    assert lib.glowhip_fourier2d(far(1), far(2), -1, 8, 4, 0, none) == -1 and b"negative" in lib.glowhip_last_error()
    assert lib.glowhip_fourier2d(far(1), far(2), 1, 8, 4, 2, none) == -1 and b"adjoint" in lib.glowhip_last_error()
    assert lib.glowhip_fourier2d(p, p, 1, 8, 4, 0, none) == -1 and b"overlap" in lib.glowhip_last_error()
    # an empty batch: nothing to do, whatever the scratch
    assert call(N=0) == 0 and call(N=0, scratch=none, nbytes=0) == 0 and lib.glowhip_fourier2d(far(1), far(2), 0, 8, 4, 1, none) == 0


def test_scratch_bytes_is_monotone_in_the_batch_and_zero_only_on_error():
    f = G.lib().glowhip_restore_fourier_scratch_bytes
    for h, w in ((2, 2), (8, 4), (64, 64), (256, 2), (2, 256), (256, 256)):
        sizes = [f(n, c, h, w) for n in (0, 1, 3, 5, 64, 67) for c in (1, 3)]
        assert all(v > 0 and v % 16 == 0 for v in sizes)
        assert f(0, 1, h, w) <= f(1, 1, h, w) <= f(1, 3, h, w) <= f(3, 3, h, w) <= f(64, 3, h, w) <= f(67, 3, h, w)
        assert f(5, 3, h, w) >= 5 * 3 * h * w * 8


# ------------------------------------------------------------------------------------------------ the oracle against closed forms
def test_gradient_is_the_written_formula_and_fp64_autograd():
    """grad_x = 2 inv Re(F^H resid) with `adjoint` (not autograd) on the right; the two agree to fp64 rounding."""
    for shape, weights in zip(F.SHAPES, F.WEIGHTS * 3):
        x, t, w, inv = F.objective_inputs(3, shape, weights)
        loss, g, resid = F.objective(x, t, w, inv)
        k = 2.0 * (torch.full((3,), 1.0 / x[0].numel(), dtype=torch.float64) if inv is None else inv.double())
        by_hand = k.view(-1, 1, 1, 1) * F.adjoint(resid)
        assert float((g - by_hand).abs().max()) <= 1e-14 * max(float(g.abs().max()), 1e-30), shape
        ww = torch.ones_like(x, dtype=torch.float64) if w is None else w.double()
        assert torch.allclose(loss, k / 2.0 * (ww * (F.forward(x) - F.as_complex(t)).abs() ** 2).sum(dim=(1, 2, 3)), rtol=1e-13, atol=0)


def test_parseval_with_a_full_mask():
    """sum |F x - F y|^2 = sum (x - y)^2: with unit weights and t = F y the objective is `restore_oracle.objective` of (x, y)."""
    import restore_oracle as R
    g = torch.Generator().manual_seed(3)
    for shape in F.SHAPES[:5]:
        x, y = (torch.rand((2,) + shape, generator=g, dtype=torch.float64) for _ in range(2))
        lhs = ((F.forward(x) - F.forward(y)).abs() ** 2).sum()
        assert abs(float(lhs - ((x - y) ** 2).sum())) <= 1e-12 * float(lhs)
        loss, grad, _ = F.objective(x, F.forward(y))
        loss_ref, grad_ref = R.objective(x, y, None, None, 1)
        assert torch.allclose(loss, loss_ref, rtol=1e-12, atol=0) and torch.allclose(grad, grad_ref, rtol=1e-11, atol=1e-18)


def test_adjoint_identity_and_the_definition_written_out():
    """<F x, k> = <x, Re F^H k> for real x (the real inner product of C^n: Re sum conj(a) b), and one coefficient by its sum."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 8, 16), generator=g, dtype=torch.float64)
    k = torch.complex(torch.randn(x.shape, generator=g, dtype=torch.float64), torch.randn(x.shape, generator=g, dtype=torch.float64))
    lhs, rhs = (F.forward(x).conj() * k).real.sum(), (x * F.adjoint(k)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))
    u, v, h, w = 3, 5, 8, 16
    s = sum(complex(x[1, 2, i, j]) * np.exp(-2j * np.pi * (u * i / h + v * j / w)) for i in range(h) for j in range(w)) / np.sqrt(h * w)
    assert abs(complex(F.forward(x)[1, 2, u, v]) - s) <= 1e-13


# ------------------------------------------------------------------------------------------------ the kernels' transform in float32
def _bitrev(n):
    lg = n.bit_length() - 1
    return np.array([int(format(i, f"0{lg}b")[::-1], 2) if lg else 0 for i in range(n)])


def fft_f32(re, im, axis, conj, kind):
    """The unnormalised radix-2 transform along ``axis`` in numpy float32, one rounding per operation: twiddles exp(-+ i pi k / h)
    from fp64 rounded once.  ``kind`` "dit": bit-reversed input, half-lengths 1 .. L/2, a' = a + w b, b' = a - w b (the kernels'
    forward); "dif": half-lengths L/2 .. 1, a' = a + b, b' = w (a - b), bit-reversed output (the kernels' adjoint)."""
    f32 = np.float32
    re, im = np.moveaxis(re, axis, -1).astype(f32), np.moveaxis(im, axis, -1).astype(f32)
    n = re.shape[-1]
    lead = re.shape[:-1]
    if kind == "dit":
        re, im = re[..., _bitrev(n)], im[..., _bitrev(n)]
    halves = [1 << s for s in range(n.bit_length() - 1)]
    for h in (halves if kind == "dit" else halves[::-1]):
        ang = -np.pi * np.arange(h, dtype=np.float64) / h
        wr, wi = np.cos(ang).astype(f32), (np.sin(ang) * (-1.0 if conj else 1.0)).astype(f32)
        re, im = re.reshape(lead + (n // (2 * h), 2, h)), im.reshape(lead + (n // (2 * h), 2, h))
        ar, ai, br, bi = re[..., 0, :], im[..., 0, :], re[..., 1, :], im[..., 1, :]
        if kind == "dit":
            tr, ti = br * wr - bi * wi, br * wi + bi * wr
            lo, hi = (ar + tr, ai + ti), (ar - tr, ai - ti)
        else:
            dr, di = ar - br, ai - bi
            lo, hi = (ar + br, ai + bi), (dr * wr - di * wi, dr * wi + di * wr)
        re, im = np.stack([lo[0], hi[0]], axis=-2).reshape(lead + (n,)), np.stack([lo[1], hi[1]], axis=-2).reshape(lead + (n,))
        assert re.dtype == f32 and im.dtype == f32
    if kind == "dif":
        re, im = re[..., _bitrev(n)], im[..., _bitrev(n)]
    return np.moveaxis(re, -1, axis), np.moveaxis(im, -1, axis)


def kernel_f32(x, t, w, inv, kernel_order):
    """csrc/restore_fourier.hip in numpy float32.  ``kernel_order`` True: the kernels' own -- forward rows then columns by decimation
    in time, the scaling, d, r = w d, u = 2 inv r, adjoint columns then rows by decimation in frequency, the scaling.  False: the
    other order everywhere -- columns first and decimation in frequency forward, rows first and decimation in time back.  The loss's
    products and sum in float64, as there."""
    f32 = np.float32
    xn = x.numpy().astype(f32)
    n, c, h, wd = xn.shape
    tn = torch.view_as_real(t).numpy().astype(f32)
    wn = np.ones_like(xn) if w is None else w.numpy().astype(f32)
    invn = (np.full((n,), 1.0, f32) / f32(c * h * wd)) if inv is None else inv.numpy().astype(f32)
    scale = f32(1.0 / np.sqrt(float(h) * float(wd)))
    fwd_axes, fwd_kind, adj_axes, adj_kind = ((3, 2), "dit", (2, 3), "dif") if kernel_order else ((2, 3), "dif", (3, 2), "dit")
    re, im = xn, np.zeros_like(xn)
    for axis in fwd_axes:
        re, im = fft_f32(re, im, axis, False, fwd_kind)
    dr, di = re * scale - tn[..., 0], im * scale - tn[..., 1]
    rr, ri = wn * dr, wn * di
    two_inv = (f32(2.0) * invn).reshape(n, 1, 1, 1)
    ur, ui = two_inv * rr, two_inv * ri
    for axis in adj_axes:
        ur, ui = fft_f32(ur, ui, axis, True, adj_kind)
    g = ur * scale
    loss = ((rr.astype(np.float64) * dr + ri.astype(np.float64) * di).sum(axis=(1, 2, 3)) * invn.astype(np.float64)).astype(f32)
    assert all(v.dtype == f32 for v in (dr, rr, ur, g, loss))
    return torch.from_numpy(loss), torch.from_numpy(g), torch.complex(torch.from_numpy(rr), torch.from_numpy(ri))


@pytest.mark.parametrize("weights", F.WEIGHTS)
@pytest.mark.parametrize("shape", F.SHAPES, ids=F.SHAPE_IDS)
def test_float32_restatement_in_two_butterfly_orders_stays_inside_the_bound(shape, weights):
    """What the GPU test asks of the kernels, an fp32 radix-2 transform delivers on the very inputs it uses (the batch of 3), in the
    kernels' butterfly order and in the opposite one: nothing in the bound was tuned on the device."""
    x, t, w, inv = F.objective_inputs(3, shape, weights)
    loss, g, resid = F.objective(x, t, w, inv)
    E_loss, E_g, E_r = F.bound(x, t, w, inv)
    assert bool((E_loss > 0).all()) and bool((E_g > 0).all()) and bool((E_r > 0).all())
    for kernel_order in (True, False):
        l32, g32, r32 = kernel_f32(x, t, w, inv, kernel_order)
        ml, mg, mr = F.worst_multiple(l32, loss, E_loss), F.worst_multiple(g32, g, E_g), F.complex_multiple(r32, resid, E_r)
        print(f"{shape} {weights} kernel_order={kernel_order}: worst multiple of the bound  loss {ml:.3f}  grad {mg:.3f}  resid {mr:.3f}")
        assert ml <= 1.0 and mg <= 1.0 and mr <= 1.0
        assert mg > 0.0 and mr > 0.0 or shape == (1, 2, 2)      # (fp32 is not fp64: the comparison is not vacuous)


def test_bound_for_scale_against_torch_fp32_fft2():
    """For scale: torch's own fp32 fft2 at 256 x 256 on the CPU deviates from fp64 by a fraction of u ||x||_2 per coefficient; the
    16-stage bound allows 16 (1 + 4 sqrt 2) u ||x||_2, about a hundred u ||x||_2 -- a worst case over every rounding."""
    x = torch.rand((1, 1, 256, 256), generator=torch.Generator().manual_seed(1))
    dev = (torch.fft.fft2(x, norm="ortho").to(torch.complex128) - F.forward(x)).abs().max()
    unit = F.U * float(x.double().norm())
    E = F.fourier2d_bound(x, 256, 256)
    print(f"torch fp32 fft2 at 256x256: {float(dev) / unit:.3f} u ||x||_2; the bound: {float(E.min()) / unit:.1f} u ||x||_2")
    assert float(dev) <= float(E.min()) and float(dev) <= 2.0 * unit


# ------------------------------------------------------------------------------------------------ the masks
@pytest.mark.parametrize("hw", [(64, 64), (16, 32), (256, 8)], ids=["64x64", "16x32", "256x8"])
def test_fourier_mask_lines(hw):
    h, w = hw
    for fraction in (0.1, 0.25, 0.5):
        m = fourier_mask(hw, fraction, seed=3)
        assert tuple(m.shape) == hw and m.dtype == torch.float32 and set(m.unique().tolist()) <= {0.0, 1.0}
        rows = m[:, 0]
        assert bool((m == rows.view(h, 1)).all())                                      # whole rows
        band = F.mask_band(h, 0.08)
        assert int(rows.sum()) == max(int(round(fraction * h)), len(band))                 # the row count
        assert bool((rows[band] == 1).all()) and 0 in band                                 # the centre band: DC and its neighbours
        assert torch.equal(m, fourier_mask(hw, fraction, seed=3))                          # deterministic in the seed
        if int(rows.sum()) > len(band) and int(rows.sum()) < h - 1:
            assert any(not torch.equal(m, fourier_mask(hw, fraction, seed=s)) for s in (4, 5, 6))
    assert F.mask_band(64, 0.08) == [0, 1, 2, 62, 63]
    assert bool((fourier_mask(hw, 1.0) == 1).all()) and bool((fourier_mask(hw, 1.0, kind="points") == 1).all())


def test_fourier_mask_points_and_refusals():
    h, w = 32, 64
    m = fourier_mask((h, w), 0.2, kind="points", center=0.1, seed=9)
    assert int(m.sum()) == int(round(0.2 * h * w)) and set(m.unique().tolist()) == {0.0, 1.0}
    bh, bw = F.mask_band(h, 0.1), F.mask_band(w, 0.1)
    assert bool((m[bh][:, bw] == 1).all())
    assert not bool((m == m[:, :1]).all())                                                 # single coefficients, not rows
    assert torch.equal(m, fourier_mask((h, w), 0.2, kind="points", center=0.1, seed=9))
    assert not torch.equal(m, fourier_mask((h, w), 0.2, kind="points", center=0.1, seed=10))
    for kw in (dict(fraction=0.0), dict(fraction=1.5), dict(kind="radial"), dict(center=-0.1), dict(hw=(0, 4))):
        with pytest.raises(ValueError):
            fourier_mask(**dict(dict(hw=(8, 8), fraction=0.5), **kw))


# ------------------------------------------------------------------------------------------------ the guards, without a device
def test_shape_guard():
    assert check_fourier_shape((2, 256)) == (2, 256) and check_fourier_shape((5, 3, 64, 8)) == (64, 8) and FOURIER_MAX == 256
    for hw in ((1, 8), (8, 1), (12, 8), (8, 24), (512, 8), (8, 1024), (0, 8), (255, 256)):
        with pytest.raises(ValueError, match="power of two"):
            check_fourier_shape(hw)
    assert tuple(as_kspace(torch.zeros(2, 3, 8, 8, dtype=torch.complex64)).shape) == (2, 3, 8, 8, 2)
    for bad in (torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.complex128), torch.zeros(2, 3, 8, 8, 2, dtype=torch.float64)):
        with pytest.raises(ValueError):
            as_kspace(bad)


def test_inferer_guards_need_no_device():
    """Every refusal of a Fourier-domain problem is a ValueError raised before any device work: the stand-in has no device at all."""
    def inferer(chw):
        inf = object.__new__(Inferer)
        inf.graph = types.SimpleNamespace(flow=types.SimpleNamespace(in_chw=chw))
        inf.device = None
        return inf

    k = torch.zeros(2, 3, 8, 8, dtype=torch.complex64)
    bad = [dict(psf=torch.ones(3, 3)), dict(operator=torch.zeros(7, 3, 8, 8)), dict(estimate_psf="shared", psf=(3, 3)), dict(pool=2),
           dict(measurement=torch.zeros(2, 3, 8, 8)), dict(measurement=torch.zeros(2, 3, 8, 4, dtype=torch.complex64)),
           dict(measurement=torch.zeros(2, 1, 8, 8, dtype=torch.complex64)), dict(measurement=torch.zeros(8, 8, dtype=torch.complex64)),
           dict(measurement=torch.zeros(2, 3, 8, 8, 2, 2)), dict(weight=-torch.ones(8, 8)), dict(weight=torch.ones(8, 4)),
           dict(weight=torch.ones(3, 3, 8, 8)), dict(chains=2), dict(chains=0)]
    for kw in bad:
        args = dict(measurement=k, weight=None, pool=1, init=None, chains=1, psf=None, operator=None, estimate_psf=None, fourier=True)
        args.update(kw)
        with pytest.raises(ValueError):
            inferer((3, 8, 8))._problem(**args)
    # a side that is not a power of two, and one above 256, whatever the model says
    for chw in ((3, 12, 8), (1, 8, 512)):
        with pytest.raises(ValueError, match="power of two"):
            inferer(chw)._problem(measurement=torch.zeros((2,) + chw, dtype=torch.complex64), weight=None, pool=1, init=None, fourier=True)


def test_loop_guards_need_no_device():
    """`LatentFit` and `LatentMALA` refuse the exclusions and the sizes before they touch the measurement's device."""
    glow = types.SimpleNamespace(hps=types.SimpleNamespace(ablation={}))
    k = torch.zeros(2, 3, 8, 8, dtype=torch.complex64)
    init = object()
    for kw in (dict(psf=torch.ones(3, 3)), dict(operator=torch.zeros(7, 3, 8, 8)), dict(pool=2),
               dict(measurement=torch.zeros(2, 3, 12, 8, dtype=torch.complex64)), dict(measurement=torch.zeros(2, 3, 8, 8)),
               dict(measurement=torch.zeros(3, 8, 8, dtype=torch.complex64))):
        for cls in (LatentFit, LatentMALA):
            with pytest.raises(ValueError):
                cls(glow, **dict(dict(measurement=k, init=init, steps=2, fourier=True), **kw))
    with pytest.raises(ValueError):
        LatentFit(glow, k, init=init, steps=2, fourier=True, estimate_psf="shared", psf=(3, 3))


# ------------------------------------------------------------------------------------------------ the fit that fixes the GPU ratio
def test_oracle_fit_fixes_the_ratio_asked_of_the_hip_path():
    """Adam in fp64 on the 16x16x3 model observed through 4 of its 16 k-space rows (`fourier_mask((16, 16), 0.25)`), from the encode
    of the zero-filled reconstruction, 40 steps at lr 0.1: the samples' final / first data terms are 0.0042, 0.0048, 0.0045.  The
    threshold asked of the GPU fit is the smallest of 0.1 / 0.2 / 0.5 that is at least twice the worst of them -- the margin of
    tests/test_linear_host.py: 0.1.  (A ratio above 0.25 would make the problem too hard for a test.)"""
    case = F.fit_case()
    hist = case["history"]
    assert tuple(hist.shape) == (case["steps"], case["ref"]["cfg"]["batch"])
    assert int(case["mask"][:, 0].sum()) == 4 and float(case["mask"][0, 0]) == 1.0
    ratios = (hist[-1] / hist[0]).tolist()
    print("first", [f"{v:.3e}" for v in hist[0].tolist()], "last", [f"{v:.3e}" for v in hist[-1].tolist()],
          "final / first", [f"{r:.4f}" for r in ratios])
    assert bool((hist[-1] < hist[0]).all()) and bool(torch.isfinite(hist).all())
    assert max(ratios) <= 0.25
    assert F.threshold_of(max(ratios)) == L.threshold_of(max(ratios)) == case["ratio"] == 0.1

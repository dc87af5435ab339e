"""Host tests of the restoration objective observed through a point-spread function (no GPU): the export, the argument checks of
glowhip_restore_objective_psf that need no device, the fp64 oracle of tests/deblur_oracle.py against closed forms (the adjoint
identity, the orientation, the reduction to tests/restore_oracle.py), a float32 restatement of the kernel's sums in two tap orders
inside the bound the GPU test uses, the band mask of ``border="valid"``, and the oracle's own deblurring fits, which fix the ratios
asked of the HIP path."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network.restore import check_psf_shape, psf_valid_weight

import deblur_oracle as B
import restore_oracle as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glowhip.h")
NAME = "glowhip_restore_objective_psf"


def test_entry_point_is_exported_declared_and_in_the_signature_table():
    text = open(HEADER).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert NAME in _lib.SIGNATURES and hasattr(so, NAME) and NAME + "(" in text
    assert len(_lib.SIGNATURES[NAME][1]) == 17
    assert "(B x)[c,i,j] = sum_{a,b} k[a,b] * x[c, i + ah - a, j + aw - b]" in text      # the definition is in the comment
    assert "grad_x      = 2 inv_wsum[n] * B^T P^T (w (A x - t))" in text
    assert G.lib().glowhip_version() == 102


def test_bad_arguments_are_einval_without_a_device():
    lib = G.lib()
    none = ctypes.c_void_p(None)
    host = ctypes.create_string_buffer(64)       # never read: every case below returns before any device call
    p = ctypes.c_void_p(ctypes.addressof(host))

    def call(x=p, t=p, psf=p, resid=p, g=p, stride=0, kh=3, kw=3, N=2, C=1, H=4, W=4, pool=1):
        return lib.glowhip_restore_objective_psf(x, t, none, none, psf, stride, kh, kw, N, C, H, W, pool, resid, g, none, none)

    for name in ("x", "t", "psf", "resid", "g"):
        assert call(**{name: none}) == -1 and b"null argument" in lib.glowhip_last_error(), name
    for kh, kw in ((2, 3), (3, 4), (0, 3), (3, 0), (-1, 3), (17, 3), (3, 17), (16, 16)):
        assert call(kh=kh, kw=kw) == -1 and b"taps" in lib.glowhip_last_error(), (kh, kw)
    for stride in (1, 8, -9):
        assert call(stride=stride) == -1 and b"stride" in lib.glowhip_last_error(), stride
    for pool in (0, -2):
        assert call(pool=pool) == -1 and b"pool" in lib.glowhip_last_error()
    assert call(H=6, W=4, pool=4) == -1 and b"does not divide" in lib.glowhip_last_error()      # H % pool
    assert call(H=4, W=6, pool=4) == -1 and b"does not divide" in lib.glowhip_last_error()      # W % pool
    assert call(N=-1) == -1 and call(C=0) == -1
    assert call(C=1 << 11, H=1 << 10, W=1 << 10) == -1 and b"out of range" in lib.glowhip_last_error()
    assert call(N=0) == 0 and call(N=0, stride=9) == 0 and call(N=0, stride=20, kh=15, kw=1) == 0     # an empty batch: nothing to do


def test_psf_shape_guard():
    assert check_psf_shape((5, 3), 4) == (5, 3) and check_psf_shape((4, 1, 15), 4) == (1, 15)
    for shape in ((4, 3), (3, 17), (5, 3, 3), (3,), (1, 4, 3, 3), (0, 3)):
        with pytest.raises(ValueError):
            check_psf_shape(shape, 4)


# ------------------------------------------------------------------------------------------------ the oracle against closed forms
@pytest.mark.parametrize("pool", [1, 2])
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
def test_adjoint_identity(pool, per_sample):
    """<A x, v> = <x, A^T v> to 1e-12 relative for a rectangular asymmetric PSF: `operator_T` (the correlation with the PSF as
    given, after P^T) is the transpose of `operator` (F.conv2d with the flipped PSF, then the pool), and autograd's gradient of
    <A x, v> is the same A^T v."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, 2, 6, 10), generator=g, dtype=torch.float64)
    v = torch.randn((3, 2, 6 // pool, 10 // pool), generator=g, dtype=torch.float64)
    k = B.asymmetric_psf(5, 3, n=3 if per_sample else None).double()
    lhs, rhs = (B.operator(x, k, pool) * v).sum(), (x * B.operator_T(v, k, pool)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))
    xl = x.clone().requires_grad_(True)
    with torch.enable_grad():
        ga, = torch.autograd.grad((B.operator(xl, k, pool) * v).sum(), [xl])
    assert torch.allclose(ga, B.operator_T(v, k, pool), rtol=1e-12, atol=1e-15)


def test_a_point_source_blurs_to_the_psf_centred_and_not_flipped():
    k = B.asymmetric_psf(5, 3).double()
    assert not torch.equal(k, k.flip(0)) and not torch.equal(k, k.flip(1))
    x = torch.zeros((1, 2, 9, 8), dtype=torch.float64)
    x[0, :, 4, 3] = 1.0
    out = B.operator(x, k)
    ref = torch.zeros_like(x)
    ref[0, :, 2:7, 2:5] = k          # rows 4 - 2 .. 4 + 2, columns 3 - 1 .. 3 + 1
    assert torch.equal(out, ref)
    # the definition, written out at one pixel: (B x)[i,j] = sum k[a,b] x[i + ah - a, j + aw - b]
    g = torch.Generator().manual_seed(6)
    y = torch.rand((1, 1, 9, 8), generator=g, dtype=torch.float64)
    by = B.operator(y, k)
    for i, j in ((0, 0), (4, 3), (8, 7), (1, 6)):
        s = sum(float(k[a, b]) * float(y[0, 0, i + 2 - a, j + 1 - b]) for a in range(5) for b in range(3)
                if 0 <= i + 2 - a < 9 and 0 <= j + 1 - b < 8)
        assert abs(float(by[0, 0, i, j]) - s) <= 1e-15


@pytest.mark.parametrize("shape,pool", R.OBJECTIVE_SHAPES)
def test_a_1x1_psf_of_one_is_the_restoration_oracle(shape, pool):
    x, t, w, inv = R.objective_inputs(shape, pool, True)
    loss, g, resid = B.objective(x, t, w, inv, pool, torch.ones(1, 1))
    loss_ref, g_ref = R.objective(x, t, w, inv, pool)
    assert torch.allclose(loss, loss_ref, rtol=1e-14, atol=0) and torch.allclose(g, g_ref, rtol=1e-13, atol=1e-20)
    px = F.avg_pool2d(x.double(), pool) if pool > 1 else x.double()
    assert torch.allclose(resid, w.double() * (px - t.double()), rtol=1e-14, atol=1e-20)


def test_gradient_is_the_written_formula():
    """grad_x = 2 inv B^T P^T resid, with `operator_T` (not autograd) on the right."""
    for (shape, ksize, pool), per_sample in zip(B.OBJECTIVE_CASES, (False, True) * 3):
        x, t, w, inv, k = B.objective_inputs(shape, ksize, pool, True, per_sample)
        _, g, resid = B.objective(x, t, w, inv, pool, k)
        by_hand = 2.0 * inv.double().view(-1, 1, 1, 1) * B.operator_T(resid, k.double(), pool)
        assert torch.allclose(g, by_hand, rtol=1e-12, atol=1e-18)


# ------------------------------------------------------------------------------------------------ the kernel's sums in float32
def kernel_f32(x, t, w, inv, pool, psf, reverse):
    """The sums of csrc/restore.hip in torch float32, one rounding per operation (no fused multiply-add), the taps in row-major
    order or (``reverse``) in the opposite one: B x, the pool, d, v = w d, the cell's value, B^T P^T; the loss's products and sum in
    float64, as there."""
    f32 = torch.float32
    x, t, psf = x.to(f32), t.to(f32), psf.to(f32)
    n, c, H, W = x.shape
    k = psf.expand(n, *psf.shape) if psf.dim() == 2 else psf
    kh, kw = k.shape[-2:]
    ah, aw = (kh - 1) // 2, (kw - 1) // 2
    w = torch.ones_like(t) if w is None else w.to(f32)
    inv = torch.full((n,), 1.0, dtype=f32) / torch.tensor(float(t[0].numel()), dtype=f32) if inv is None else inv.to(f32)
    taps = [(a, b) for a in range(kh) for b in range(kw)]
    taps = taps[::-1] if reverse else taps

    def gather(src, sign):
        """out[i,j] = sum_{a,b} k[a,b] src[i + sign (ah - a), j + sign (aw - b)]: sign +1 is B, -1 is B^T."""
        pad = F.pad(src, (aw, aw, ah, ah))
        out = None
        for a, b in taps:
            r0, c0 = ah + sign * (ah - a), aw + sign * (aw - b)
            term = k[:, a, b].view(-1, 1, 1, 1) * pad[:, :, r0:r0 + H, c0:c0 + W]
            out = term if out is None else out + term
        return out

    bx = gather(x, +1)
    if pool > 1:
        inv_p2 = torch.tensor(1.0, dtype=f32) / torch.tensor(float(pool * pool), dtype=f32)
        s = torch.zeros_like(t)
        for a in range(pool):
            for b in range(pool):
                s = s + bx[:, :, a::pool, b::pool]
        px = s * inv_p2
    else:
        inv_p2 = torch.tensor(1.0, dtype=f32)
        px = bx
    d = px - t
    v = w * d
    cell = ((2.0 * inv).view(-1, 1, 1, 1) * v) * inv_p2
    u = cell.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1) if pool > 1 else cell
    g = gather(u, -1)
    loss = ((v.double() * d.double()).sum(dim=(1, 2, 3)) * inv.double()).to(f32)
    assert all(r.dtype == f32 for r in (bx, px, d, v, cell, g, loss))
    return loss, g, v


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "ones"])
@pytest.mark.parametrize("shape,ksize,pool", B.OBJECTIVE_CASES, ids=B.CASE_IDS)
def test_float32_restatement_in_two_tap_orders_stays_inside_the_bound(shape, ksize, pool, weighted, per_sample):
    """What the GPU test asks of the kernel, fp32 sums deliver on the very inputs it uses, whichever way the taps are walked -- and
    the bound still notices a result off by a relative 2^-14 (the widest case sums 225 taps: 225 u is about 2^-16.2)."""
    x, t, w, inv, k = B.objective_inputs(shape, ksize, pool, weighted, per_sample)
    loss, g, resid = B.objective(x, t, w, inv, pool, k)
    E_loss, E_g, E_r = B.bound(x, t, w, inv, pool, k)
    assert bool((E_loss > 0).all()) and bool((E_g > 0).all()) and bool((E_r > 0).all())
    for reverse in (False, True):
        l32, g32, r32 = kernel_f32(x, t, w, inv, pool, k, reverse)
        ml, mg, mr = B.worst_multiple(l32, loss, E_loss), B.worst_multiple(g32, g, E_g), B.worst_multiple(r32, resid, E_r)
        print(f"{shape} psf {ksize} pool {pool} {'weighted' if weighted else 'ones'} reverse={reverse}: worst multiple of the bound  "
              f"loss {ml:.3f}  grad {mg:.3f}  resid {mr:.3f}")
        assert ml <= 1.0 and mg <= 1.0 and mr <= 1.0
    off = 1.0 + 2.0 ** -14
    assert B.worst_multiple(g32 * off, g, E_g) > 1.0 and B.worst_multiple(l32 * off, loss, E_loss) > 1.0
    assert B.worst_multiple(r32 * off, resid, E_r) > 1.0


# ------------------------------------------------------------------------------------------------ the band of border="valid"
@pytest.mark.parametrize("meas,ksize,pool", [((5, 7), (3, 3), 1), ((5, 7), (5, 7), 1), ((5, 7), (1, 9), 1), ((5, 7), (15, 15), 1),
                                             ((3, 5), (5, 3), 2), ((3, 5), (3, 1), 2), ((3, 5), (7, 7), 2), ((4, 8), (7, 7), 4),
                                             ((4, 8), (11, 9), 4)])
def test_psf_valid_weight_is_the_brute_force_footprint_test(meas, ksize, pool):
    """On the measurements of the 5x7 (pool 1) and 6x10 (pool 2) cases, and of 16x32 under pool 4: a cell is kept exactly when every
    x its footprint reads is inside the image; the band is ceil(ah / pool) rows and ceil(aw / pool) columns."""
    kh, kw = ksize
    got = psf_valid_weight((2, 3) + meas, kh, kw, pool)
    ref = B.valid_weight(meas, kh, kw, pool)
    assert got.dtype == torch.float32 and tuple(got.shape) == meas and torch.equal(got, ref)
    rh, rw = -(-((kh - 1) // 2) // pool), -(-((kw - 1) // 2) // pool)
    assert int(got.sum()) == max(meas[0] - 2 * rh, 0) * max(meas[1] - 2 * rw, 0)
    if ksize == (15, 15):
        assert not bool(got.any())      # (what `Inferer.restore` refuses)


# ------------------------------------------------------------------------------------------------ the fits that fix the GPU ratios
@pytest.mark.parametrize("name", list(B.FITS))
def test_oracle_fit_fixes_the_ratio_asked_of_the_hip_path(name):
    """Adam in fp64 from the latents of the blurred measurement itself, the weights the valid band: the worst sample's final / first
    data term, rounded up to the next of 0.1 / 0.2 / 0.5, is the constant the GPU test uses (deblur: 0.031, 0.039, 0.027 -> 0.1;
    deblur_sr: 0.043, 0.050, 0.049 -> 0.1).  The descent need not be monotone (deblur_sr's first steps at lr 0.2 are not)."""
    case = B.fit_case(name)
    hist = case["history"]
    assert tuple(hist.shape) == (case["steps"], case["ref"]["cfg"]["batch"])
    ratios = (hist[-1] / hist[0]).tolist()
    print(name, "first", [f"{v:.3e}" for v in hist[0].tolist()], "last", [f"{v:.3e}" for v in hist[-1].tolist()],
          "final / first", [f"{r:.3f}" for r in ratios])
    assert bool((hist[-1] < hist[0]).all()) and bool(torch.isfinite(hist).all())
    assert B.round_up_ratio(max(ratios)) == case["ratio"]

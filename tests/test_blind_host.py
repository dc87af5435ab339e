"""Host tests of blind deblurring (no GPU): the three exports, the argument checks of glowhip_psf_from_logits and
glowhip_restore_psf_grad that need no device, the scratch sizer, the fp64 oracle of tests/blind_oracle.py against closed forms
(autograd = the explicit correlation, the adjoint identity of the map from taps to blurred image, the softmax backward), a float32
restatement of the kernel's sums in two summation orders inside the bound the GPU test uses, the guards of `Inferer._problem` /
`LatentFit` / `blind_start` on objects with no device, and the oracle's own two fits, which fix the thresholds asked of the HIP
path."""
import ctypes
import os
import types

import pytest
import torch
import torch.nn.functional as F

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network import Inferer, LatentFit, RestoreInfo
from pytorch_glow_amd.network.restore import blind_start

import blind_oracle as K
import deblur_oracle as B
import restore_oracle as R
from test_deblur_host import kernel_f32 as objective_f32

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glowhip.h")
NAMES = ("glowhip_psf_from_logits", "glowhip_restore_psf_grad_scratch_bytes", "glowhip_restore_psf_grad")


def test_entry_points_are_exported_declared_and_in_the_signature_table():
    text = open(HEADER).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(so, name) and name + "(" in text, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [6, 7, 17]
    assert "g_k[n,a,b] = sum_{c,i,j} u[c,i,j] * x[c, i + ah - a, j + aw - b]" in text      # the definition is in the comment
    assert "g_theta[q] = k[q] * (g_k[q] - sum_r k[r] g_k[r])" in text
    assert G.lib().glowhip_version() == 102
    info = RestoreInfo(loss=None, grad_norm=None, finite=True, captured=False)
    assert info.psf is None and info.psf_grad_norm is None
    assert list(RestoreInfo.__dataclass_fields__)[-2:] == ["psf", "psf_grad_norm"]


def test_bad_arguments_are_einval_without_a_device():
    lib = G.lib()
    none = ctypes.c_void_p(None)
    host = ctypes.create_string_buffer(1 << 16)       # never read: every case below returns before any device call
    base = (ctypes.addressof(host) + 255) & ~255
    p = ctypes.c_void_p(base)
    need = lambda **kw: lib.glowhip_restore_psf_grad_scratch_bytes(*[{**dict(N=2, C=1, H=4, W=4, kh=3, kw=3, pool=1), **kw}[k]
                                                                   for k in ("N", "C", "H", "W", "kh", "kw", "pool")])

    def call(x=p, resid=p, psf=p, gk=p, gl=p, scratch=p, nbytes=1 << 15, stride=0, kh=3, kw=3, N=2, C=1, H=4, W=4, pool=1):
        return lib.glowhip_restore_psf_grad(x, resid, none, psf, stride, kh, kw, N, C, H, W, pool, gk, gl, scratch, nbytes, none)

    err = lib.glowhip_last_error
    for name in ("x", "resid"):
        assert call(**{name: none}) == -1 and b"null argument" in err(), name
    assert call(gk=none, gl=none) == -1 and b"null argument" in err()
    assert call(psf=none) == -1 and b"null argument" in err()            # grad_logits needs the psf
    for kh, kw in ((2, 3), (3, 4), (0, 3), (3, 0), (-1, 3), (17, 3), (3, 17), (16, 16)):
        assert call(kh=kh, kw=kw) == -1 and b"taps" in err(), (kh, kw)
        assert need(kh=kh, kw=kw) == 0 and b"taps" in err()
    for stride in (1, 8, -9):
        assert call(stride=stride) == -1 and b"stride" in err(), stride
    for pool in (0, -2):
        assert call(pool=pool) == -1 and b"pool" in err() and need(pool=pool) == 0
    assert call(H=6, W=4, pool=4) == -1 and b"does not divide" in err()      # H % pool
    assert call(H=4, W=6, pool=4) == -1 and b"does not divide" in err()      # W % pool
    assert need(H=6, W=4, pool=4) == 0 and need(H=4, W=6, pool=4) == 0
    assert call(N=-1) == -1 and call(C=0) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert need(N=-1) == 0 and need(C=0) == 0
    assert call(C=1 << 11, H=1 << 10, W=1 << 10) == -1 and b"out of range" in err()
    assert need(C=1 << 11, H=1 << 10, W=1 << 10) == 0 and b"out of range" in err()
    assert call(N=1 << 30, C=64, H=64, W=64) == -1 and b"workgroups" in err()
    # the scratch: NULL, misaligned, too small
    want = need()
    assert want > 0 and want <= 1 << 15
    assert call(scratch=none) == -1 and b"scratch" in err()
    assert call(scratch=ctypes.c_void_p(base + 4)) == -1 and b"scratch" in err()
    assert call(nbytes=want - 1) == -1 and b"scratch" in err()
    # an empty batch: nothing to do, whatever the scratch
    assert call(N=0) == 0 and call(N=0, stride=9) == 0 and call(N=0, scratch=none, nbytes=0) == 0
    # the softmax
    sm = lambda a=p, b=p, n=1, kh=3, kw=3: lib.glowhip_psf_from_logits(a, b, n, kh, kw, none)
    assert sm(a=none) == -1 and b"null argument" in err() and sm(b=none) == -1
    for kh, kw in ((2, 3), (3, 4), (0, 3), (17, 3), (3, 17)):
        assert sm(kh=kh, kw=kw) == -1 and b"taps" in err()
    assert sm(n=-1) == -1 and sm(n=0) == 0


def test_scratch_size_is_monotone_in_each_argument_and_zero_only_on_error():
    lib = G.lib()
    base = dict(N=2, C=3, H=24, W=72, kh=5, kw=3, pool=1)
    order = ("N", "C", "H", "W", "kh", "kw", "pool")
    f = lambda **kw: lib.glowhip_restore_psf_grad_scratch_bytes(*[{**base, **kw}[k] for k in order])
    assert f() > 0 and f() % 256 == 0
    assert f(N=0) > 0                                       # zero is the error value
    steps = dict(N=range(0, 70), C=range(1, 9), H=range(24, 24 * 9, 24), W=range(72, 72 * 9, 24), kh=range(1, 16, 2), kw=range(1, 16, 2),
                 pool=(1, 2, 3, 4, 6, 8, 12, 24))
    for name, values in steps.items():
        sizes = [f(**{name: v}) for v in values]
        assert all(s > 0 for s in sizes), (name, sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (name, sizes)
    assert f(N=64) > f(N=1) and f(C=6) > f(C=3) and f(H=240) > f(H=24) and f(W=720) > f(W=72) and f(kh=15) > f(kh=5) and f(kw=15) > f(kw=3)
    # exactly what the launches write: one double per tap, sample and (channel, 8-row band, 64-column tile)
    assert f() >= 2 * 3 * 3 * 2 * 15 * 8
    assert f(kh=4) == 0 and f(pool=5) == 0 and f(W=0) == 0 and f(N=-1) == 0


# ------------------------------------------------------------------------------------------------ the oracle against closed forms
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("shape,ksize,pool", K.GRAD_CASES, ids=K.GRAD_IDS)
def test_autograd_is_the_explicit_correlation(shape, ksize, pool, per_sample):
    """d loss / d k by autograd of `deblur_oracle._terms` = the correlation of u with x written out tap by tap, to 1e-12."""
    x, t, w, inv, k = K.grad_inputs(shape, ksize, pool, True, per_sample)
    _, _, resid = B.objective(x, t, w, inv, pool, k)
    g = K.psf_grad(x, t, w, inv, pool, k)
    e = K.psf_grad_explicit(x, resid, inv, pool, *ksize, shared=not per_sample)
    assert tuple(g.shape) == tuple(k.shape) == tuple(e.shape)
    assert float((g - e).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1.0)
    # unweighted, with the default normalisation
    x, t, _, _, k = K.grad_inputs(shape, ksize, pool, False, per_sample)
    _, _, resid = B.objective(x, t, None, None, pool, k)
    g = K.psf_grad(x, t, None, None, pool, k)
    e = K.psf_grad_explicit(x, resid, None, pool, *ksize, shared=not per_sample)
    assert float((g - e).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1.0)


@pytest.mark.parametrize("pool", [1, 2])
def test_adjoint_identity_of_the_map_from_taps_to_image(pool):
    """<g_k, delta> = <u, B_delta x> for random delta, to 1e-12 relative: the correlation is the transpose of delta -> B_delta x."""
    gen = torch.Generator().manual_seed(8)
    x = torch.randn((3, 2, 6, 10), generator=gen, dtype=torch.float64)
    v = torch.randn((3, 2, 6 // pool, 10 // pool), generator=gen, dtype=torch.float64)
    inv = torch.rand(3, generator=gen, dtype=torch.float64) + 0.5
    u = K.u_of(v, inv, pool)
    g = K.correlate(u, x, 5, 3)
    for _ in range(3):
        delta = torch.randn((3, 5, 3), generator=gen, dtype=torch.float64)
        lhs, rhs = (g * delta).sum(), (u * K.blur_by(x, delta)).sum()
        assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))
    delta = torch.randn((5, 3), generator=gen, dtype=torch.float64)          # a shared perturbation meets the summed gradient
    lhs, rhs = (g.sum(dim=0) * delta).sum(), (u * K.blur_by(x, delta)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))


def test_softmax_and_its_backward():
    gen = torch.Generator().manual_seed(9)
    theta = torch.randn((4, 5, 7), generator=gen, dtype=torch.float64) * 3.0
    g = torch.randn((4, 5, 7), generator=gen, dtype=torch.float64)
    k = K.softmax(theta)
    assert bool((k > 0).all()) and float((k.sum(dim=(1, 2)) - 1.0).abs().max()) <= 1e-15
    assert torch.allclose(k, torch.softmax(theta.reshape(4, -1), dim=1).reshape(4, 5, 7), rtol=1e-14, atol=0)
    gl = K.softmax_backward(k, g)
    assert float(gl.sum(dim=(1, 2)).abs().max()) <= 1e-15 * float(g.abs().max()) * 35      # sum_q g_theta[q] = 0
    tl = theta.clone().requires_grad_(True)
    with torch.enable_grad():
        ga, = torch.autograd.grad((torch.softmax(tl.reshape(4, -1), dim=1).reshape(4, 5, 7) * g).sum(), [tl])
    assert torch.allclose(gl, ga, rtol=1e-12, atol=1e-15)
    # a case's PSF is an fp32 tensor that sums to 1 only up to fp32 rounding: sum_q g_theta[q] = (1 - sum k) sum k g, exactly that
    ref = K.grad_reference(*K.GRAD_CASES[2], True, True)
    kd, gd = ref["psf"].double(), ref["grad_psf"]
    want = (1.0 - kd.sum(dim=(-2, -1))) * (kd * gd).sum(dim=(-2, -1))
    assert float((ref["grad_logits"].sum(dim=(-2, -1)) - want).abs().max()) <= 1e-14 * float(gd.abs().max())


# ------------------------------------------------------------------------------------------------ the kernel's sums in float32
def gradient_f32(x, resid, inv, pool, kh, kw, shared, reverse):
    """The sums of csrc/restore_blind.hip in torch float32, one rounding per operation (no fused multiply-add): u with its two
    roundings from a float32 residual; per tap and image row, chains of at most 64 terms -- the columns left to right in runs of 64,
    or (``reverse``) right to left, dealt to four interleaved chains per run --; everything above a chain in float64, in the chains'
    order or the opposite one; one rounding at the end."""
    f32 = torch.float32
    x, v = x.to(f32), resid.to(f32)
    n, c, H, W = x.shape
    inv = torch.full((n,), 1.0, dtype=f32) / torch.tensor(float(v[0].numel()), dtype=f32) if inv is None else inv.to(f32)
    inv_p2 = torch.tensor(1.0, dtype=f32) / torch.tensor(float(pool * pool), dtype=f32)
    cell = ((2.0 * inv).view(-1, 1, 1, 1) * v) * inv_p2
    u = cell.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1) if pool > 1 else cell
    ah, aw = (kh - 1) // 2, (kw - 1) // 2
    xp = F.pad(x, (aw, aw, ah, ah))
    # X[n,c,i,j,a,b] = x[c, i + ah - a, j + aw - b]
    X = xp.unfold(2, kh, 1).unfold(3, kw, 1).flip(-2, -1)
    assert tuple(X.shape) == (n, c, H, W, kh, kw) and u.dtype == f32 and X.dtype == f32
    chains = []
    for j0 in range(0, W, 64):
        cols = list(range(j0, min(j0 + 64, W)))
        groups = [cols] if not reverse else [cols[::-1][s::4] for s in range(4)]
        for grp in groups:
            acc = torch.zeros((n, c, H, kh, kw), dtype=f32)
            assert len(grp) <= K.CHAIN
            for j in grp:
                acc = acc + u[:, :, :, j, None, None] * X[:, :, :, j]
            chains.append(acc)
    chains = chains[::-1] if reverse else chains
    tot = torch.zeros((n, kh, kw), dtype=torch.float64)
    for ch in chains:
        rows = ch.double().flip(2) if reverse else ch.double()
        tot = tot + rows.sum(dim=(1, 2))
    return (tot.sum(dim=0) if shared else tot).to(f32)


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "ones"])
@pytest.mark.parametrize("shape,ksize,pool", K.GRAD_CASES, ids=K.GRAD_IDS)
def test_float32_restatement_in_two_summation_orders_stays_inside_the_bound(shape, ksize, pool, weighted, per_sample):
    """What the GPU test asks of the kernels, fp32 chains of 64 terms deliver on the very inputs it uses, whichever way the pixels
    are dealt to chains and the chains are folded -- and the bound still notices a result off by 2^-12 of sum |u| |x|."""
    ref = K.grad_reference(shape, ksize, pool, weighted, per_sample)
    x, t, w, inv, k = (ref[n] for n in ("x", "target", "weight", "inv", "psf"))
    assert bool((ref["E_psf"] > 0).all()) and bool((ref["E_logits"] > 0).all())
    for reverse in (False, True):
        _, _, r32 = objective_f32(x, t, w, inv, pool, k, reverse)
        g32 = gradient_f32(x, r32, inv, pool, *ksize, shared=not per_sample, reverse=reverse)
        gl32 = K.softmax_backward(k, g32).float()      # (the kernel's fp64 softmax backward and its one rounding)
        mk, ml = K.worst_multiple(g32, ref["grad_psf"], ref["E_psf"]), K.worst_multiple(gl32, ref["grad_logits"], ref["E_logits"])
        print(f"{shape} psf {ksize} pool {pool} {'weighted' if weighted else 'ones'} reverse={reverse}: worst multiple of the bound  "
              f"grad_psf {mk:.3f}  grad_logits {ml:.3f}")
        assert g32.dtype == torch.float32 and mk <= 1.0 and ml <= 1.0
    S = K.correlate(K.u_of(ref["resid"], inv, pool).abs(), x.double().abs(), *ksize)
    S = S if per_sample else S.sum(dim=0)
    assert K.worst_multiple(g32.double() + 2.0 ** -12 * S, ref["grad_psf"], ref["E_psf"]) > 1.0


# ------------------------------------------------------------------------------------------------ the guards, with no device
def test_blind_start():
    k = blind_start((3, 5), "shared", 4)
    assert tuple(k.shape) == (3, 5) and k.dtype == torch.float32 and torch.equal(k, torch.full((3, 5), 1.0 / 15.0))
    k = blind_start(torch.full((3, 3), 2.0), "per_sample", 4)
    assert tuple(k.shape) == (4, 3, 3) and k.is_contiguous() and float((k.sum(dim=(1, 2)) - 1).abs().max()) <= 1e-6
    k = blind_start(B.asymmetric_psf(5, 3, n=4) * 3.0, "per_sample", 4)
    assert tuple(k.shape) == (4, 5, 3) and float((k.sum(dim=(1, 2)) - 1).abs().max()) <= 1e-6
    zero = torch.ones(3, 3)
    zero[1, 1] = 0.0
    bad = [dict(psf=zero), dict(psf=-torch.ones(3, 3)), dict(psf=torch.full((3, 3), float("nan"))), dict(psf=None),
           dict(psf=torch.ones(4, 3, 3), estimate_psf="shared"), dict(psf=torch.ones(3, 3, 3), estimate_psf="per_sample"),
           dict(psf=(4, 3)), dict(psf=(3, 17)), dict(psf=torch.ones(3, 4)), dict(psf=torch.ones(3)), dict(estimate_psf="both"),
           dict(estimate_psf=True), dict(operator=torch.zeros(7, 3, 8, 8))]
    for kw in bad:
        with pytest.raises(ValueError):
            blind_start(**{**dict(psf=(3, 3), estimate_psf="shared", n=4), **kw})


def test_inferer_and_fit_guards_need_no_device():
    """Every refusal of a blind fit is a ValueError raised before any device work: the stand-ins have no device at all."""
    inf = object.__new__(Inferer)
    inf.graph = types.SimpleNamespace(flow=types.SimpleNamespace(in_chw=(3, 8, 8)), hps=types.SimpleNamespace(ablation={}))
    inf.device = None
    meas = torch.zeros(2, 3, 8, 8)
    zero = torch.ones(3, 3)
    zero[0, 2] = 0.0
    bad = [dict(psf=zero, estimate_psf="shared"), dict(psf=torch.ones(2, 3, 3), estimate_psf="shared"),
           dict(psf=(3, 3), estimate_psf="shared", operator=torch.zeros(7, 3, 8, 8)), dict(psf=(4, 3), estimate_psf="shared"),
           dict(psf=torch.ones(3, 4), estimate_psf="per_sample"), dict(psf=None, estimate_psf="shared"),
           dict(psf=(3, 3), estimate_psf="sample")]
    for kw in bad:
        with pytest.raises(ValueError):
            inf._problem(**{**dict(measurement=meas, weight=None, pool=1, init=None), **kw})
        with pytest.raises(ValueError):
            inf.restore(meas, steps=2, **kw)
        with pytest.raises(ValueError):
            LatentFit(inf.graph, meas, init=object(), steps=2, **kw)
    with pytest.raises(ValueError):
        inf.estimate_psf(meas, meas, psf=zero)
    with pytest.raises(ValueError):
        inf.estimate_psf(meas, meas, psf=(3, 4))
    with pytest.raises(ValueError):
        inf.estimate_psf(meas, meas, psf=torch.ones(2, 3, 3), per_sample=False)
    with pytest.raises(ValueError):
        inf.estimate_psf(meas, meas[:, :, :4], psf=(3, 3))                  # blurred is not sharp's shape at pool 1
    with pytest.raises(ValueError, match="border"):
        inf.estimate_psf(meas, meas, psf=(3, 3), border="reflect")
    with pytest.raises(ValueError, match="no cell"):
        inf.estimate_psf(meas, meas, psf=(15, 15))


# ------------------------------------------------------------------------------------------------ the fits that fix the GPU thresholds
def test_oracle_calibration_fixes_the_ratio_asked_of_the_hip_path():
    """The images known, the PSF from the uniform 5x5 start by 60 Adam steps at 0.2 on the logits, in fp64: the L1 error of the PSF
    falls from 0.868 to 0.021 -- final / start 0.024, rounded up to 0.1, the constant the GPU test uses; the data term falls by more
    than a factor of 1 000."""
    case = K.fit_case("calibrate")
    hist = case["history"]
    e0, e1 = K.l1(case["start"], case["true_psf"]), K.l1(case["psf"], case["true_psf"])
    print("L1 error of the PSF", f"{e0:.4f} -> {e1:.4f}", "ratio", f"{e1 / e0:.4f}", "loss final / first", (hist[-1] / hist[0]).tolist())
    assert tuple(hist.shape) == (case["steps"], 3) and bool(torch.isfinite(hist).all())
    assert abs(float(case["psf"].sum()) - 1.0) <= 1e-12 and bool((case["psf"] > 0).all())
    assert K.round_up_ratio(e1 / e0) == case["ratio"]
    assert e1 / e0 <= 0.5 * case["ratio"], "the oracle alone must sit well inside the rounded threshold"
    assert float((hist[-1] / hist[0]).max()) <= 1e-2


def test_oracle_blind_fit_fixes_the_ratio_asked_of_the_hip_path():
    """Latents and PSF together, from the encode of the blurred image and the uniform 5x5 PSF, 60 Adam steps at 0.05 / 0.2 in fp64:
    the worst sample's final / first data term is 0.012, rounded up to 0.1, the constant the GPU test uses; the PSF moves towards
    the truth (L1 error 0.87 -> 0.19) although the images are unknown."""
    case = K.fit_case("blind")
    hist = case["history"]
    ratios = (hist[-1] / hist[0]).tolist()
    e0, e1 = K.l1(case["start"], case["true_psf"]), K.l1(case["psf"], case["true_psf"])
    print("final / first", [f"{r:.4f}" for r in ratios], "L1 error of the PSF", f"{e0:.4f} -> {e1:.4f}")
    assert tuple(hist.shape) == (case["steps"], 3) and bool(torch.isfinite(hist).all())
    assert K.round_up_ratio(max(ratios)) == case["ratio"]
    assert max(ratios) <= 0.5 * case["ratio"], "the oracle alone must sit well inside the rounded threshold"
    assert e1 < e0

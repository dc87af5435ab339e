"""Host tests of the restoration objective and loop (no GPU): the export, the argument checks of glowhip_restore_objective that need no
device, the fp64 oracle of tests/restore_oracle.py against closed forms, a float32 restatement of the kernel's arithmetic inside the
bound the GPU test uses, and the oracle's own in-painting and super-resolution fits, which fix the ratios asked of the HIP path."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib

import restore_oracle as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glowhip.h")


def test_restore_objective_is_exported_declared_and_in_the_signature_table():
    text = open(HEADER).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    name = "glowhip_restore_objective"
    assert name in _lib.SIGNATURES and hasattr(so, name) and name + "(" in text
    assert len(_lib.SIGNATURES[name][1]) == 12
    assert "inv_wsum[n] * sum w (P x - t)^2" in text and "2 inv_wsum[n] * P^T (w (P x - t))" in text      # the formula is in the comment
    assert G.lib().glowhip_version() == 102


def test_bad_arguments_are_einval_without_a_device():
    lib = G.lib()
    none = ctypes.c_void_p(None)
    host = ctypes.create_string_buffer(64)       # never read: every case below returns before any device call
    p = ctypes.c_void_p(ctypes.addressof(host))
    call = lambda x, t, g, N=2, C=1, H=4, W=4, pool=1: lib.glowhip_restore_objective(x, t, none, none, N, C, H, W, pool, g, none, none)
    for args in ((none, p, p), (p, none, p), (p, p, none)):
        assert call(*args) == -1 and b"null argument" in lib.glowhip_last_error()
    for pool in (0, -2):
        assert call(p, p, p, pool=pool) == -1 and b"pool" in lib.glowhip_last_error()
    assert call(p, p, p, H=6, W=4, pool=4) == -1 and b"does not divide" in lib.glowhip_last_error()      # H % pool
    assert call(p, p, p, H=4, W=6, pool=4) == -1 and b"does not divide" in lib.glowhip_last_error()      # W % pool
    assert call(p, p, p, N=-1) == -1 and call(p, p, p, C=0) == -1
    assert call(p, p, p, C=1 << 11, H=1 << 10, W=1 << 10) == -1 and b"out of range" in lib.glowhip_last_error()
    assert call(p, p, p, N=0) == 0               # an empty batch: nothing to do


# ------------------------------------------------------------------------------------------------ the oracle against closed forms
def test_pool_1_without_weights_is_the_mean_squared_error():
    x, t, _, _ = R.objective_inputs((3, 2, 5, 7), 1, False)
    loss, g = R.objective(x, t)
    ref = ((x.double() - t.double()) ** 2).mean(dim=(1, 2, 3))
    assert torch.allclose(loss, ref, rtol=1e-14, atol=0)
    assert torch.allclose(g, 2.0 * (x.double() - t.double()) / 70.0, rtol=1e-13, atol=1e-18)


@pytest.mark.parametrize("shape,pool", R.OBJECTIVE_SHAPES)
def test_gradient_is_fp64_autograd_of_the_written_formula(shape, pool):
    x, t, w, inv = R.objective_inputs(shape, pool, True)
    loss, g = R.objective(x, t, w, inv, pool)
    xl = x.double().requires_grad_(True)
    with torch.enable_grad():
        px = F.avg_pool2d(xl, pool)
        by_hand = (inv.double().view(-1, 1, 1, 1) * w.double() * (px - t.double()) ** 2).sum(dim=(1, 2, 3))
        ga, = torch.autograd.grad(by_hand.sum(), [xl])
    assert torch.allclose(loss, by_hand.detach(), rtol=1e-14, atol=0) and torch.allclose(g, ga, rtol=1e-13, atol=1e-20)
    # the closed form: every x under a cell receives 2 inv w (P x - t) / pool^2
    cell = 2.0 * inv.double().view(-1, 1, 1, 1) * w.double() * (px.detach() - t.double()) / (pool * pool)
    up = cell.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1)
    assert torch.allclose(g, up, rtol=1e-13, atol=1e-20)


def test_pool_2_is_avg_pool2d():
    x, t, _, _ = R.objective_inputs((2, 3, 6, 10), 2, False)
    loss, _ = R.objective(x, t, pool=2)
    px = x.double().view(2, 3, 3, 2, 5, 2).mean(dim=(3, 5))
    assert torch.allclose(F.avg_pool2d(x.double(), 2), px, rtol=1e-15, atol=0)
    assert torch.allclose(loss, ((px - t.double()) ** 2).mean(dim=(1, 2, 3)), rtol=1e-14, atol=0)


def test_a_zero_weight_sample_gives_zeros_and_leaves_the_others():
    x, t, w, _ = R.objective_inputs((3, 2, 4, 6), 1, True)
    w0 = w.clone()
    w0[1] = 0.0
    loss, g = R.objective(x, t, w0, R.inv_wsum_of(w0))
    ref_loss, ref_g = R.objective(x, t, w, R.inv_wsum_of(w))
    assert float(loss[1]) == 0.0 and float(g[1].abs().max()) == 0.0
    assert torch.equal(loss[[0, 2]], ref_loss[[0, 2]]) and torch.equal(g[[0, 2]], ref_g[[0, 2]])      # per sample: its own problem
    assert float(R.inv_wsum_of(w0)[1]) == 1.0                                                          # 1 / max(0, 1)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in float32
def kernel_f32(x, t, w, inv, pool):
    """csrc/restore.hip operation by operation in numpy float32 (the loss's products and sum in float64, as there)."""
    f = np.float32
    x, t = x.numpy().astype(f), t.numpy().astype(f)
    n, c, H, W = x.shape
    w = np.ones_like(t) if w is None else w.numpy().astype(f)
    inv = np.full(n, f(1.0) / f(t[0].size), f) if inv is None else inv.numpy().astype(f)
    inv_p2 = f(1.0) / f(pool * pool) if pool > 1 else f(1.0)
    s = np.zeros_like(t)
    for a in range(pool):
        for b in range(pool):
            s = (s + x[:, :, a::pool, b::pool]).astype(f)
    px = (s * inv_p2).astype(f) if pool > 1 else x
    d = (px - t).astype(f)
    wd = (w * d).astype(f)
    two_inv = (f(2.0) * inv).reshape(-1, 1, 1, 1)
    g = ((two_inv * wd).astype(f) * inv_p2).astype(f)
    g = g.repeat(pool, axis=-2).repeat(pool, axis=-1)
    loss = ((wd.astype(np.float64) * d.astype(np.float64)).sum(axis=(1, 2, 3)) * inv.astype(np.float64)).astype(f)
    return torch.from_numpy(loss), torch.from_numpy(g)


@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "ones"])
@pytest.mark.parametrize("shape,pool", R.OBJECTIVE_SHAPES)
def test_float32_restatement_of_the_kernel_stays_inside_the_bound(shape, pool, weighted):
    """What the GPU test asks of the kernel, the promised fp32 arithmetic delivers on the very inputs it uses -- and the bound is
    tight enough to notice one dropped operation (a result off by a relative 2^-18 is far outside)."""
    x, t, w, inv = R.objective_inputs(shape, pool, weighted)
    loss, g = R.objective(x, t, w, inv, pool)
    E_loss, E_g = R.bound(x, t, w, inv, pool)
    l32, g32 = kernel_f32(x, t, w, inv, pool)
    ml, mg = R.worst_multiple(l32, loss, E_loss), R.worst_multiple(g32, g, E_g)
    print(f"{shape} pool {pool} {'weighted' if weighted else 'ones'}: worst multiple of the bound  loss {ml:.3f}  grad {mg:.3f}")
    assert ml <= 1.0 and mg <= 1.0
    assert R.worst_multiple(g32 * (1.0 + 2.0 ** -18), g, E_g) > 1.0 and R.worst_multiple(l32 * (1.0 + 2.0 ** -18), loss, E_loss) > 1.0


# ------------------------------------------------------------------------------------------------ the fits that fix the GPU ratios
@pytest.mark.parametrize("name,ratio", [("inpaint", R.INPAINT_RATIO), ("superres", R.SUPERRES_RATIO)])
def test_oracle_fit_fixes_the_ratio_asked_of_the_hip_path(name, ratio):
    """20 Adam steps at lr 0.2 from the latents of the half-blanked image, fp64: every sample's loss falls over the first five
    steps, and the worst sample's final / first, rounded up to the next of 0.1 / 0.2 / 0.5, is the constant the GPU test uses."""
    case = R.fit_case(name)
    hist = case["history"]
    assert tuple(hist.shape) == (R.FIT_STEPS, case["ref"]["cfg"]["batch"])
    ratios = (hist[-1] / hist[0]).tolist()
    print(name, "first", [f"{v:.3e}" for v in hist[0].tolist()], "last", [f"{v:.3e}" for v in hist[-1].tolist()],
          "final / first", [f"{r:.3f}" for r in ratios])
    assert bool((hist[1:6] < hist[:5]).all())
    assert R.round_up_ratio(max(ratios)) == ratio


def test_prior_weight_pulls_the_oracle_fit_towards_the_origin():
    """torch.optim.Adam's weight decay is the prior term: with an all-zero weight the data term has no gradient, and the latents move
    against their own sign."""
    case = R.fit_case("inpaint")
    ref = case["ref"]
    w0 = torch.zeros_like(case["weight"])
    z, eps, hist = R.restore_loop(ref["z"], ref["eps"], ref["sd"], ref["cfg"], case["measurement"], w0, R.inv_wsum_of(w0), 1,
                                  steps=3, lr=0.01, prior_weight=0.5)
    assert float(hist.abs().max()) == 0.0
    for a, b in zip([z] + eps, [ref["z"]] + ref["eps"]):
        moved = a - b.double()
        big = b.double().abs() > 0.1
        assert bool((torch.sign(moved[big]) == -torch.sign(b.double()[big])).all())

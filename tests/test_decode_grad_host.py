"""Host tests of the differentiable decode (no GPU): the two exports, the error paths of glowhip_plan_decode_vjp that need no device,
the workspace query, `Latents.requires_grad_ / detach`, and the CPU oracle helpers the GPU tests rest on."""
import ctypes
import os

import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network import Latents

import decode_grad_oracle as D

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glowhip.h")
EINVAL = 1


def _squeeze_plan(lib):
    d = (_lib.LayerDesc * 2)()
    d[0].kind, d[0].C, d[0].H, d[0].W = _lib.LAYER_SQUEEZE, 3, 8, 8
    d[1].kind, d[1].C, d[1].H, d[1].W = _lib.LAYER_SQUEEZE, 12, 4, 4
    h = lib.glowhip_plan_create(d, 2)
    assert h
    return ctypes.c_void_p(h)


def test_decode_vjp_is_exported_declared_and_in_the_signature_table():
    text = open(HEADER).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("glowhip_plan_decode_vjp", "glowhip_plan_decode_vjp_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(so, name) and name + "(" in text
    assert G.lib().glowhip_version() == 102


def test_wrong_n_eps_and_null_arguments_are_einval_without_a_device():
    lib = G.lib()
    h = _squeeze_plan(lib)
    try:
        none = ctypes.c_void_p(None)
        arr = (ctypes.c_void_p * 1)(None)
        # a squeeze-only plan has no Split2d: one eps gradient is one too many
        rc = lib.glowhip_plan_decode_vjp(h, none, none, none, none, arr, 1, 2, none, 0, none, 0, none)
        assert rc != 0 and b"eps gradients given" in lib.glowhip_last_error()
        rc = lib.glowhip_plan_decode_vjp(h, none, none, none, none, None, 0, 2, none, 0, none, 0, none)
        assert rc != 0 and b"null argument" in lib.glowhip_last_error()
        rc = lib.glowhip_plan_decode_vjp(h, none, none, none, none, None, 0, 70000, none, 0, none, 0, none)
        assert rc != 0 and b"out of range" in lib.glowhip_last_error()
        assert lib.glowhip_plan_decode_vjp(h, none, none, none, none, None, 0, 0, none, 0, none, 0, none) == 0      # empty batch: nothing to do
        assert lib.glowhip_plan_decode_vjp(None, none, none, none, none, None, 0, 1, none, 0, none, 0, none) != 0
    finally:
        lib.glowhip_plan_destroy(h)


def test_workspace_query_is_monotone_in_the_batch():
    lib = G.lib()
    h = _squeeze_plan(lib)
    try:
        sizes = [lib.glowhip_plan_decode_vjp_workspace_bytes(h, n) for n in (0, 1, 2, 7, 64)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[1] > 0
        assert sizes[-1] >= 2 * 64 * 192 * 4                # two gradient buffers of the widest layer
        assert lib.glowhip_plan_decode_vjp_workspace_bytes(None, 4) == 0 and lib.glowhip_plan_decode_vjp_workspace_bytes(h, -1) == 0
    finally:
        lib.glowhip_plan_destroy(h)


def test_latents_requires_grad_and_detach():
    z, eps = torch.randn(2, 4, 2, 2), [torch.randn(2, 2, 4, 4)]
    lat = Latents(z, eps, torch.zeros(2))
    leaf = lat.requires_grad_()
    assert isinstance(leaf, Latents) and all(t.requires_grad and t.is_leaf for t in leaf.tensors()) and leaf.nll is lat.nll
    assert leaf.z.data_ptr() == z.data_ptr()                 # leaves are marked in place, not copied
    derived = Latents(leaf.z * 2, [e * 2 for e in leaf.eps])
    again = derived.requires_grad_()
    assert all(t.is_leaf and t.requires_grad for t in again.tensors())      # results of other operations are cut loose first
    det = derived.detach()
    assert isinstance(det, Latents) and not any(t.requires_grad for t in det.tensors()) and det.z.data_ptr() == derived.z.data_ptr()
    off = leaf.requires_grad_(False)
    assert not any(t.requires_grad for t in off.tensors())


def test_oracle_helpers_agree_with_the_oracle_and_with_finite_algebra():
    """The reference the GPU tests use: its latents decode back to the batch, its gradient is linear in g_x and is the adjoint of a
    directional derivative taken along a direction that flips no ReLU (a small step inside the margin)."""
    ref = D.reference(image=16, hidden=32, K=2, L=2, batch=3, zeros_std=0.05, seed=1)
    assert ref["margin"] >= D.MIN_MARGIN
    assert [tuple(e.shape[1:]) for e in ref["eps"]] == [(6, 8, 8)] and tuple(ref["z"].shape[1:]) == (24, 4, 4)
    x2, gz2, geps2 = D.decode_grads(ref["z"], ref["eps"], 2 * ref["gx"], ref["sd"], ref["cfg"])
    assert torch.allclose(gz2, 2 * ref["gz"], rtol=1e-12, atol=0) and torch.allclose(geps2[0], 2 * ref["geps"][0], rtol=1e-12, atol=0)
    frac, rel = D.beyond(ref["gz"].float(), ref["gz"])
    assert frac == 0.0 and rel < 1e-6
    frac, _ = D.beyond(torch.zeros_like(ref["gz"]), ref["gz"])
    assert frac > 0.9                                         # a wrong answer is outside nearly everywhere
    g = torch.Generator().manual_seed(0)
    dz = torch.randn(ref["z"].shape, generator=g, dtype=torch.float64) * 1e-7
    de = torch.randn(ref["eps"][0].shape, generator=g, dtype=torch.float64) * 1e-7
    sd64 = {k: v.double() for k, v in ref["sd"].items()}
    from oracle import glow_oracle as O
    with torch.no_grad():
        xp = O.flow_decode(ref["z"].double() + dz, sd64, ref["cfg"], [ref["eps"][0].double() + de])
        xm = O.flow_decode(ref["z"].double() - dz, sd64, ref["cfg"], [ref["eps"][0].double() - de])
    lhs = float((ref["gx"].double() * (xp - xm) / 2).sum())
    rhs = float((ref["gz"] * dz).sum() + (ref["geps"][0] * de).sum())
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (lhs, rhs)

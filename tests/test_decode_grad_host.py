"""Host tests of the differentiable decode (no GPU): the two exports, the error paths of glowhip_plan_decode_vjp that need no device,
the workspace query, `Latents.requires_grad_ / detach`, the CPU oracle helpers the GPU tests rest on, and the seeded non-square /
odd / ragged cases of tests/test_gpu_decode_grad_shapes.py (their table lives here, so that the seeds are checked without a GPU)."""
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


# ------------------------------------------------------------------------------------------------ H x W cases
# The cases of tests/test_gpu_decode_grad_shapes.py (L = 2 unless said otherwise), with the fp64 ReLU margin of each seed as a CPU scan
# found it (alternate seeds in brackets) and the floor this file holds it to: MIN_MARGIN where the GPU test compares every entry,
# the recorded margin rounded down for W and T, which go under the capped rule (no seed of 200 / 150 scanned reaches 1e-5 there).
#   R   12x20  hidden 64   seed 20 (30, 54):     9.0e-5      O   20x12  hidden 32   seed 34 (29, 5):    1.8e-4
#   N2  32x48  hidden 128  seed 180 (199, 110):  1.6e-5      D6  64x192 L 6         seed 59 (56, 101):  1.5e-5
#   S   8x64   hidden 128  seed 23 (33, 15):     2.2e-5      F   8x256  hidden 128  seed 26 (82, 115):  2.9e-5
#   W   16x128 hidden 128  seed 197 (134):       9.4e-6      T   64x16  hidden 512  seed 129 (115):     4.6e-6
NP_SEED = 5      # numpy seed of the fixed-permutation tables (test_gpu_decode_grad.NP_SEED)
SHAPE_CASES = {
    "R": dict(image=(12, 20), hidden=64, K=2, L=2, batch=3, zeros_std=0.05, seed=20),
    "O": dict(image=(20, 12), hidden=32, K=2, L=2, batch=3, zeros_std=0.05, seed=34, perm="shuffle", coup="additive", np_seed=NP_SEED),
    "N2": dict(image=(32, 48), hidden=128, K=2, L=2, batch=2, zeros_std=0.05, seed=180),
    "D6": dict(image=(64, 192), hidden=32, K=1, L=6, batch=2, zeros_std=0.02, seed=59, stable=True),
    "S": dict(image=(8, 64), hidden=128, K=2, L=2, batch=3, zeros_std=0.05, seed=23),
    "F": dict(image=(8, 256), hidden=128, K=1, L=2, batch=2, zeros_std=0.01, seed=26, perm="reverse", coup="additive", np_seed=NP_SEED),
    "W": dict(image=(16, 128), hidden=128, K=2, L=2, batch=2, zeros_std=0.01, seed=197),
    "T": dict(image=(64, 16), hidden=512, K=2, L=2, batch=3, zeros_std=0.01, seed=129),
}
SHAPE_MARGIN = {"R": 9.0e-5, "O": 1.8e-4, "N2": 1.6e-5, "D6": 1.5e-5, "S": 2.2e-5, "F": 2.9e-5, "W": 9.4e-6, "T": 4.6e-6}
SHAPE_MARGIN_FLOOR = dict({c: D.MIN_MARGIN for c in SHAPE_CASES}, W=9e-6, T=4e-6)


def test_int_and_pair_forms_of_image_give_the_same_reference_bit_for_bit():
    kw = dict(hidden=32, K=2, L=2, batch=3, zeros_std=0.05, seed=1)      # test_gpu_decode_grad.TINY_AFF
    a, b = D.reference(image=16, **kw), D.reference(image=(16, 16), **kw)
    assert a is not b and tuple(a["cfg"]["image_shape"]) == tuple(b["cfg"]["image_shape"]) == (16, 16, 3)
    assert set(a["sd"]) == set(b["sd"]) and all(torch.equal(a["sd"][k], b["sd"][k]) for k in a["sd"])
    for k in ("z", "gx", "x", "gz"):
        assert torch.equal(a[k], b[k]), k
    for k in ("eps", "geps"):
        assert len(a[k]) == len(b[k]) == 1 and torch.equal(a[k][0], b[k][0]), k
    assert a["margin"] == b["margin"]
    ta, tb = (D.perm_tables(im, 32, 2, 2, 3, "shuffle", "additive", NP_SEED) for im in (16, (16, 16)))
    assert ta.keys() == tb.keys() and all(torch.equal(ta[i][j], tb[i][j]) for i in ta for j in (0, 1))


@pytest.mark.parametrize("cid", list(SHAPE_CASES))
def test_shape_case_seed_keeps_its_margin_and_the_fp32_oracle_stays_inside_the_bound(cid):
    """The seed's fp64 margin is above the case's floor, every reference gradient is finite, and autograd through the same oracle in
    fp32 has no entry beyond 2e-4 max|g| + 1e-7 of the fp64 one: what the GPU test asks of the kernels, the formats themselves can
    deliver.  (The recorded margin is printed, not asserted: the latents are an fp32 encode, whose last bits -- and with them the
    third digit of the margin -- depend on the host's convolution: W 9.4e-6 / 9.2e-6, T 4.6e-6 / 4.5e-6 on two machines.)"""
    from oracle import glow_oracle as O
    kw = SHAPE_CASES[cid]
    ref = D.reference(**kw)
    H, W = kw["image"]
    assert tuple(ref["cfg"]["image_shape"]) == (H, W, 3) and tuple(ref["gx"].shape) == (kw["batch"], 3, H, W)
    L = kw["L"]
    assert tuple(ref["z"].shape[1:]) == (3 * 2 ** (L + 1), H >> L, W >> L)
    assert [tuple(e.shape[1:]) for e in ref["eps"]] == [(3 * 2 ** l, H >> l, W >> l) for l in range(L - 1, 0, -1)]
    print(f"{cid}: margin {ref['margin']:.3e} (recorded {SHAPE_MARGIN[cid]:.1e}, floor {SHAPE_MARGIN_FLOOR[cid]:.0e})")
    assert ref["margin"] >= SHAPE_MARGIN_FLOOR[cid]
    assert all(bool(torch.isfinite(t).all()) for t in [ref["x"], ref["gz"]] + ref["geps"])
    prev = O.STABLE_LOGDET
    O.STABLE_LOGDET = bool(kw.get("stable", False))
    try:
        _, gz32, geps32 = D.decode_grads(ref["z"], ref["eps"], ref["gx"], ref["sd"], ref["cfg"], ref["tables"], dtype=torch.float32)
    finally:
        O.STABLE_LOGDET = prev
    for name, a, r in [("g_z", gz32, ref["gz"])] + [(f"g_eps[{k}]", a, r) for k, (a, r) in enumerate(zip(geps32, ref["geps"]))]:
        frac, rel = D.beyond(a, r)
        print(f"{cid} fp32 oracle {name}: {frac:.3%} beyond the bound, worst err / max|g| {rel:.2e}")
        assert frac == 0.0, f"{cid} {name}: the fp32 oracle itself has {frac:.3%} of its entries beyond the bound ({rel:.2e})"

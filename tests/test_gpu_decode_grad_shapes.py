"""GPU tests of the differentiable decode on non-square, odd and ragged level maps (-m gpu): glowhip_plan_decode_vjp against
autograd through `O.flow_decode` in fp64 (tests/decode_grad_oracle.py), at the shapes where decode_vjp_sweep (csrc/plan_train.hip) and
the kernels of csrc/decode_bwd.hip pick their forms from H, W and H * W separately.  tests/test_gpu_decode_grad.py runs square
power-of-two images only: every level map there has H = W and HW in {4096, ..., 4, 1}, where the scalar kernel forms see p = 0
alone, the partial-sum gather sees R = W rows per tile, no 64-pixel mixer block straddles a sample at an odd offset and no model
mixes fused and per-layer levels.

The cases, their seeds and fp64 ReLU margins are tests/test_decode_grad_host.py's SHAPE_CASES, which holds them on the CPU; the
comparison rules (strict / capped) and their helpers are test_gpu_decode_grad.py's.  Which kernel form ran is asserted from the
plan's launch counters where a counter exists (the fused chain, the gather-only kernel, the two mixer VJPs, the LU pack); the
scalar forms of the elementwise kernels have no counter: their launchers take them whenever HW % 4 != 0, which is a property of the
case (HW = 15 in R and O, 3 in D6)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402

import decode_grad_oracle as D  # noqa: E402
import plu_oracle as PLU  # noqa: E402
from test_decode_grad_host import SHAPE_CASES, SHAPE_MARGIN_FLOOR  # noqa: E402
from test_gpu_decode_grad import DEV, TINY_AFF, assert_margin, check_capped, check_strict, hip_grads, make_glow  # noqa: E402
from test_gpu_shapes import CASES as STEP_CASES  # noqa: E402


def run_case(cid, family=None, what=None):
    """One decode + VJP of a case: (reference, g_z, [g_eps], launch counts of the backward).  The decoded image itself at 1e-4."""
    kw = SHAPE_CASES[cid]
    ref = D.reference(**kw)
    glow = make_glow(ref, kw.get("perm", "invconv"))
    x, gz, geps, counts = hip_grads(glow, ref, family=family)
    ex = float((x.cpu().double() - ref["x"]).abs().max())
    print(f"{what or cid} {kw['image'][0]}x{kw['image'][1]} seed {kw['seed']}: margin {ref['margin']:.2e}, decode err {ex:.2e}, {counts}")
    assert ex <= 1e-4, f"{cid}: decode itself: {ex:.2e}"
    return ref, gz, geps, counts


def mixers(counts):
    return counts.get("k_chanmix_inv_bwd", 0), counts.get("k_chanmix_inv_bwd_wide", 0)


def fused(counts):
    return counts.get("k_cnet(tape)", 0), counts.get("k_cnet(bwd)", 0), counts.get("k_cpart_finish", 0)


# ------------------------------------------------------------------------------------------------ odd and ragged maps, per layer
@pytest.mark.parametrize("cid", ["R", "O", "N2", "D6"])
def test_odd_and_ragged_maps_every_entry_vs_fp64_autograd_oracle(cid):
    """Every entry within 2e-4 max|g| + 1e-7, on the per-layer input-gradient chain (no side of these maps is a power of two, so no
    level has a k_cnet instance: the counters must show none).
      R   6x10 = 60 pixels: the 16-byte elementwise forms, 64-pixel mixer blocks that straddle samples at offsets 60 and 120 and end
          in a ragged block (180 = 2 * 64 + 52); 3x5 = 15 pixels: the scalar k_coupling_inv_bwd and k_relu_bwd1 with p > 0, an odd
          k_split_inv_bwd above it, mixer blocks over three samples (45 pixels in one block).
      O   the gather (shuffle) branch of the mixer VJP and the additive scalar tail on 10x6 and 5x3.
      N2  16x24 and 8x12: wgrad_fast levels (HW % 32 == 0, hidden 128) that k_cnet does not take.
      D6  L = 6 on 64x192: C = 192 on 2x6 still on the pixel-block mixer VJP, C = 384 on 1x3 on k_chanmix_inv_bwd_wide with HW = 3
          (6 pixels of two samples in one 32-pixel block).

    Measured on an MI355X: no entry beyond the bound in any tensor; worst error / max|g| R 5.2e-7, O 3.1e-7, N2 1.2e-6, D6 1.1e-6
    (the fp32 oracle's own: 7.4e-7, 2.5e-7, 1.1e-6, 7.1e-6); the decoded image within 4.3e-6."""
    kw = SHAPE_CASES[cid]
    ref, gz, geps, counts = run_case(cid)
    assert_margin(ref)
    check_strict(ref, gz, geps, cid)
    assert not [k for k in counts if k.startswith("k_cnet")] and "k_cpart_finish" not in counts, counts
    if cid == "D6":
        assert mixers(counts) == (5, 1), counts
    else:
        assert mixers(counts) == (kw["K"] * kw["L"], 0), counts


# ------------------------------------------------------------------------------------------------ fused and per-layer levels in one sweep
# k_cnet launches of one sweep (taping == backward) and gather-only launches.  The VJP gates a FlowStep's fused chain on wgrad_fast
# (HW % 32 == 0 and hidden % 128 == 0: true at every level of these four) and bwd_cnet_chain, which is the training step's gate with
# the same scratch (N * max_hidden floats): the `cnet` column of test_gpu_shapes.CASES, whose derivations of the tile shapes apply
# unchanged (the permutation plays no part in them: S is affine / invconv here).  Within a level the next FlowStep's mixer VJP gathers
# the partial sums; after the level's last FlowStep finish_pending does -- at the Split2d for level 1, at the end of the sweep for
# level 2: one k_cpart_finish per fused level.
FUSED = {"T": (4, 2), "W": (4, 2), "F": (1, 1), "S": (2, 1)}


def check_geometry(cid):
    kw, c = SHAPE_CASES[cid], STEP_CASES[cid]
    assert kw["image"] == (c["H"], c["W"]) and (kw["hidden"], kw["K"], kw["batch"]) == (c["hidden"], c["K"], c["batch"])
    assert FUSED[cid][0] == c["cnet"]


@pytest.mark.parametrize("cid", ["S", "F"])
def test_mixed_levels_on_the_exact_fp32_family_every_entry(cid):
    """S (4x32 fused, 2x16 per layer) and F (4x128 per layer, 2x64 fused) with the f16 pipe out of the sweep: no k_cnet launch, the
    decode-only kernels and the sweep's buffer bookkeeping alone, every entry within the bound.

    Measured on an MI355X: no entry beyond the bound; worst error / max|g| S 6.6e-7, F 2.7e-7."""
    kw = SHAPE_CASES[cid]
    ref, gz, geps, counts = run_case(cid, family=1, what=f"{cid} exact fp32")
    assert_margin(ref)
    assert not [k for k in counts if k.startswith("k_cnet")] and "k_cpart_finish" not in counts, counts
    assert mixers(counts) == (kw["K"] * kw["L"], 0), counts
    check_strict(ref, gz, geps, f"{cid} exact fp32")


@pytest.mark.parametrize("cid", ["S", "F"])
def test_mixed_fused_and_per_layer_levels_every_entry(cid):
    """The pending state machine of decode_vjp_sweep on a model where one level runs fused and the other does not.  S: level 1's two
    backward k_cnet launches leave partial sums that FlowStep 2's mixer VJP and then finish_pending at the Split2d gather, level 2
    runs per layer with nothing pending.  F: level 1 per layer, level 2's one launch is finished at the end of the sweep.

    Measured on an MI355X: the counters as derived above FUSED (S 2 + 2 launches and 1 k_cpart_finish, F 1 + 1 and 1); no entry
    beyond the bound on the fused launches either, worst error / max|g| S 8.6e-7, F 2.4e-7 -- the strict rule holds as it stands."""
    check_geometry(cid)
    kw = SHAPE_CASES[cid]
    ref, gz, geps, counts = run_case(cid)
    assert_margin(ref)
    assert fused(counts) == (FUSED[cid][0], FUSED[cid][0], FUSED[cid][1]), counts
    assert mixers(counts) == (kw["K"] * kw["L"], 0), counts
    check_strict(ref, gz, geps, cid)


@pytest.mark.parametrize("cid", ["W", "T"])
def test_tall_and_wide_fused_levels_under_the_capped_rule(cid):
    """Both levels fused.  W: 8x64 and 4x32 maps, 64-pixel tiles of one and two rows.  T: 32x8 and 16x4 maps, R = 8 rows per tile and
    a tile that is a whole image, hidden 512.  The gather of the partial sums -- by the next FlowStep's mixer VJP inside a level, by
    k_cpart_finish after it -- reads them with fin_src(add_H, add_W): a gather that took H for W puts essentially every entry
    outside.  The margins of these seeds (W 9.4e-6, T 4.6e-6; no seed scanned reaches 1e-5) are below MIN_MARGIN, so the rule is the
    capped one: at most 1 % of a tensor's entries beyond 2e-4 max|g| + 1e-7, none beyond 5e-2 max|g|.  The fp32 oracle has none
    beyond at these seeds (worst 7e-7 max|g|, test_decode_grad_host.py): the cap is there for flipped ReLU masks only.

    Measured on an MI355X: 0.000 % of g_z and of g_eps[0] beyond the bound in both cases -- no mask flipped at these seeds -- worst
    error / max|g| W 2.3e-7, T 4.0e-7; 4 + 4 k_cnet launches and 2 k_cpart_finish each, as derived above FUSED."""
    check_geometry(cid)
    kw = SHAPE_CASES[cid]
    ref, gz, geps, counts = run_case(cid)
    assert ref["margin"] >= SHAPE_MARGIN_FLOOR[cid], ref["margin"]
    assert all(bool(torch.isfinite(t).all()) for t in [ref["gz"]] + ref["geps"])
    assert fused(counts) == (FUSED[cid][0], FUSED[cid][0], FUSED[cid][1]), counts
    assert mixers(counts) == (kw["K"] * kw["L"], 0), counts
    check_capped(ref, gz, geps, 0.01, cid)


# ------------------------------------------------------------------------------------------------ LU-parameterised plan
_LU = {}


def lu_reference(name, kw):
    """The case with every dense 1x1 weight factored into the LU parameters (misc.util.lu_state_dict_from_dense); the reference
    gradients, the decoded image and the margin from the dense-key state dict tests/plu_oracle.py assembles from those fp32
    parameters in fp64 -- not from the matrices that were factored, which differ by the factorisation's rounding."""
    if name not in _LU:
        ref = D.reference(**kw)
        sd_lu = util.lu_state_dict_from_dense({k: v.clone() for k, v in ref["sd"].items()})
        dense = PLU.dense_state_dict(sd_lu)
        assert set(dense) == set(ref["sd"])
        margin = D.decode_margin(ref["z"].double(), [e.double() for e in ref["eps"]], dense, ref["cfg"])
        x, gz, geps = D.decode_grads(ref["z"], ref["eps"], ref["gx"], dense, ref["cfg"])
        _LU[name] = dict(ref, sd=sd_lu, margin=margin, x=x, gz=gz, geps=geps)
    return _LU[name]


@pytest.mark.parametrize("name,kw", [pytest.param("tiny", TINY_AFF, id="tiny-16x16"), pytest.param("R", SHAPE_CASES["R"], id="R-12x20")])
def test_lu_parameterised_plan_every_entry_vs_fp64_autograd_oracle(name, kw):
    """lu_decomposition=True: W^-1 of every FlowStep comes from the triangular solves of csrc/invconv_lu.hip on the pack's side
    stream, and join_lu is on the VJP's path.  The backward's own pack (the training images on top of the decode's) assembles every
    layer's W again -- `pack:invconv_lu` counts one job per layer -- and runs the step that launches k_invconv_lu_inverse whenever
    the pack has the inverse flag (`pack:k_step_prepare_batched`; the solve has no counter of its own); no layer is left to the dense
    factorisations (`pack:lu:*`), so the W^-1 the mixer VJPs read can only be the solves'.

    Measured on an MI355X: no entry beyond the bound; worst error / max|g| 16x16 3.2e-7, R 5.7e-7; margins on the assembled W
    3.7e-5 and 9.0e-5; `pack:invconv_lu` 4, `pack:k_step_prepare_batched` 1, k_chanmix_inv_bwd 4, no `pack:lu:*`."""
    ref = lu_reference(name, kw)
    assert_margin(ref)
    cfg = ref["cfg"]
    hps = D.hps_for(cfg, cfg["batch"])
    hps.ablation.lu_decomposition = True
    glow = G.Glow(hps)
    glow.load_state_dict({k: v.clone() for k, v in ref["sd"].items()}, strict=True)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).eval()
    nsteps = kw["K"] * kw["L"]
    assert sum(isinstance(m, G.Invertible1x1ConvLU) for m in glow.modules()) == nsteps
    x, gz, geps, counts = hip_grads(glow, ref)
    ex = float((x.cpu().double() - ref["x"]).abs().max())
    print(f"LU {name}: margin {ref['margin']:.2e}, decode err {ex:.2e}, {counts}")
    assert ex <= 1e-4, f"decode itself: {ex:.2e}"
    check_strict(ref, gz, geps, f"LU {name}")
    assert counts.get("pack:invconv_lu") == nsteps and counts.get("pack:k_step_prepare_batched") == 1, counts
    assert not [k for k in counts if k.startswith("pack:lu:")], counts
    assert mixers(counts) == (nsteps, 0), counts


# ------------------------------------------------------------------------------------------------ linearity and per-sample normalisation
def test_vjp_on_an_odd_map_is_linear_to_the_bit_over_2_to_the_pm20_and_per_sample():
    """test_vjp_is_linear_to_the_bit_over_2_to_the_pm20_and_per_sample on R: k_grad_norm and k_scale_rows work on per = 3 * 12 * 20 =
    720 elements of each of three samples (no multiple of 1024: one partly filled trip of the 16-byte loop), and the un-normalising
    factor reaches g_eps through the scalar k_split_inv_bwd at HW = 60."""
    ref = D.reference(**SHAPE_CASES["R"])
    assert_margin(ref)
    glow = make_glow(ref)
    _, gz, geps, _ = hip_grads(glow, ref)
    for a in (2.0 ** 20, 2.0 ** -20):
        _, gza, gepsa, _ = hip_grads(glow, ref, gx=ref["gx"] * a)
        assert torch.equal(gza, gz * a), f"alpha {a}: g_z differs"
        assert all(torch.equal(x, y * a) for x, y in zip(gepsa, geps)), f"alpha {a}: g_eps differs"
    # samples 2^24 apart in scale: each meets the strict bound against ITS reference
    scale = torch.tensor([1.0, 2.0 ** 24, 2.0 ** -12]).view(-1, 1, 1, 1)
    _, gzs, gepss, _ = hip_grads(glow, ref, gx=ref["gx"] * scale)
    for n in range(3):
        s = float(scale[n])
        for a, r in zip([gzs] + gepss, [ref["gz"]] + ref["geps"]):
            frac, rel = D.beyond(a[n:n + 1] / s, r[n:n + 1])
            assert frac == 0.0, f"sample {n}: {frac:.3%} beyond the bound ({rel:.2e})"
    # an all-zero g_x[0]: exact zeros for that sample, the others untouched
    gx0 = ref["gx"].clone()
    gx0[0] = 0
    _, gz0, geps0, _ = hip_grads(glow, ref, gx=gx0)
    for a, b in zip([gz0] + geps0, [gz] + geps):
        assert float(a[0].abs().max()) == 0.0 and torch.equal(a[1:], b[1:])

"""Non-square and non-power-of-two images (-m gpu): one training step, the same step on the per-layer kernels, inference and the
data-dependent ActNorm initialisation of whole L = 2 models whose level maps are tall, wide, flat (H = 2), ragged (W % 4 != 0) or
odd -- the shapes at which the backward sweep, the tape and the workspaces pick their kernels and sizes from H, W and H * W
separately (csrc/plan_build.hip, csrc/plan.hip, csrc/plan_train.hip, csrc/backward.hip).  Every other gradient test of the suite runs on a square
power-of-two image, where an index that takes W for H, a halo row from the wrong side or a buffer sized from max(H, W)^2 cannot show.

The yardstick of every gradient is torch autograd through the oracle in fp64 (the reference network/model.py:82-117 and
network/trainer.py:123-150 accept any image_shape = (H, W, C) with H and W divisible by 2^L); z, nll and the decode are held to the
fp32 oracle at the suite's 1e-4.  One reference per case, computed once and shared by the four tests."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402

from test_gpu_grad import hps_for, oracle_grads  # noqa: E402

DEV = "cuda:0"
SEED = 31

# id: H, W, K, hidden, coupling, permutation, batch, fused k_cnet launches of one training step (taping == backward), f16 pipe
#
# The launch counts follow from cnet_geo / cnet_select / cnet_tape_instance (csrc/cnet_sh.hip); a taping launch prefers 64-pixel
# tiles wherever they exist, and the backward launch is the same network transposed (f.4's channels in, C / 2 out):
#   T  level 1 32x8 (6 -> 12 channels) and level 2 16x4 (12 -> 24): 64-pixel tiles of R = 8 rows / of one whole image (R = H = 16),
#      12 and 3 tiles -> the h2 rows split four ways (ms = 4, fewer than 160 workgroups); hidden 512 has a taping instance for every
#      row split, one T unit per wave (NU4 * KS = 8) in both directions: 2 levels x K launches.
#   W  level 1 8x64 and level 2 4x32: 64-pixel tiles of R = 1 / R = 2 rows; hidden 128 allows no row split at 64-pixel tiles
#      (ms_max = 128 / 128 = 1), which is the one taping instance hidden 128 has: 2 levels x K.
#   F  level 1 4x128: W = 128 fits the 128-pixel tile only, where hidden 128 splits its rows in two (8 tiles < 160 workgroups) and has
#      no taping instance: per-layer kernels.  Level 2 2x64: 64-pixel tiles of one row, ms = 1: K launches.
#   S  level 1 4x32 as W's level 2: K launches.  Level 2 2x16 = 32 pixels < 64: none.
#   N1, N2, R, O: a side that is no power of two: none.
CASES = {
    "T": dict(H=64, W=16, K=2, hidden=512, coup="affine", perm="invconv", batch=3, cnet=4, f16=True),
    "W": dict(H=16, W=128, K=2, hidden=128, coup="affine", perm="invconv", batch=2, cnet=4, f16=True),
    "F": dict(H=8, W=256, K=1, hidden=128, coup="additive", perm="reverse", batch=2, cnet=1, f16=True),
    "S": dict(H=8, W=64, K=2, hidden=128, coup="affine", perm="shuffle", batch=3, cnet=2, f16=True),
    "N1": dict(H=48, W=80, K=2, hidden=128, coup="affine", perm="invconv", batch=2, cnet=0, f16=True),
    "N2": dict(H=32, W=48, K=2, hidden=128, coup="additive", perm="invconv", batch=3, cnet=0, f16=True),
    "R": dict(H=12, W=20, K=2, hidden=64, coup="affine", perm="invconv", batch=3, cnet=0, f16=False),
    "O": dict(H=20, W=12, K=2, hidden=32, coup="additive", perm="shuffle", batch=3, cnet=0, f16=False),
}
ALL = list(CASES)


def dev(t):
    return t.to(DEV) if isinstance(t, torch.Tensor) else t


def close(a, b, atol, what=""):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert torch.isfinite(a).all() and err <= atol, f"{what}: max err {err:.3e} (bar {atol:.0e})"
    return err


def build_glow(cid):
    """A fresh host-side Glow of the case, and the tables of its fixed permutations (np.random seeded: the same for every build)."""
    c = CASES[cid]
    cfg = O.default_cfg(image_shape=(c["H"], c["W"], 3), hidden_channels=c["hidden"], K=c["K"], L=2, flow_permutation=c["perm"],
                        flow_coupling=c["coup"], actnorm_scale=1.0, n_bits_x=8, batch=c["batch"])
    np.random.seed(SEED)
    glow = G.Glow(hps_for(cfg, c["batch"]))
    tables = None
    if c["perm"] != "invconv":
        tables = {i: (getattr(l, c["perm"]).indices.copy(), getattr(l, c["perm"]).indices_inverse.copy())
                  for i, l in enumerate(glow.flow.layers) if hasattr(l, c["perm"])}
    return cfg, glow, tables


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Weights, inputs and every reference figure of a case; computed once, read by all tests, never written."""
    c = CASES[cid]
    cfg, glow, tables = build_glow(cid)
    sd0 = O.seeded_state_dict(cfg, seed=SEED, invconv_perturb=0.02, zeros_std=0.01)
    g = torch.Generator().manual_seed(SEED)
    x = torch.rand(c["batch"], 3, c["H"], c["W"], generator=g)
    noise = torch.rand(c["batch"], 3, c["H"], c["W"], generator=g) / 256
    with torch.no_grad():
        sd = O.glow_init_actnorm(x, noise, sd0, cfg, perm_tables=tables)
        z32, nll32, _ = O.glow_forward(x, noise, sd, cfg, perm_tables=tables)
        eps = [torch.randn(c["batch"], *s, generator=torch.Generator().manual_seed(3 + i)) * 0.7
               for i, s in enumerate(glow.flow.split_shapes((3, c["H"], c["W"])))]
        x_rev = O.glow_reverse(z32, sd, cfg, eps, perm_tables=tables)
    grads, gx, loss = oracle_grads(cfg, {k: v.double() for k, v in sd.items()}, x.double(), noise.double(), tables)
    return dict(cfg=cfg, tables=tables, sd0=sd0, sd=sd, x=x, noise=noise, z32=z32, nll32=nll32, eps=eps, x_rev=x_rev,
                grads=grads, gx=gx, loss=loss)


def make_glow(cid, sd, inited=True):
    r = reference(cid)
    cfg, glow, tables = build_glow(cid)
    if tables is not None:
        assert all(np.array_equal(tables[i][0], r["tables"][i][0]) for i in tables)
    sd = {k: v.clone() for k, v in sd.items()}
    sd["h_top"] = torch.zeros_like(glow.h_top)
    glow.load_state_dict(sd)
    glow.set_actnorm_inited(inited)
    return glow.to(DEV)


def train_step_vs_oracle(cid, want_cnet, what):
    """One training step (forward with tape, generative_loss, backward) of a fresh model against the case's references; returns the
    launch counters of the step.  Loss within 1e-4 of the fp64 oracle, z / nll within 1e-4 of the fp32 oracle; per tensor at most 1 %
    of the entries beyond 2e-4 max|g_ref| + 1e-7 -- none where no f16-pipe kernel runs -- and none beyond 5e-2 max|g_ref| + 1e-7."""
    c, r = CASES[cid], reference(cid)
    glow = make_glow(cid, r["sd"]).train()
    plan = glow.flow.plan_for(dev(r["x"]))
    plan.launch_counts(reset=True)
    with torch.enable_grad():
        xd = dev(r["x"]).requires_grad_(True)
        z, nll, _ = glow.normal_flow(xd, None, noise=dev(r["noise"]))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    counts = plan.launch_counts(reset=True)
    got = {n: p.grad for n, p in glow.named_parameters()}
    assert got.pop("h_top") is None
    missing = [n for n, v in got.items() if v is None]
    assert not missing, f"{what}: no gradient for {missing}"
    assert set(got) == set(r["grads"]), set(got) ^ set(r["grads"])
    got["dL/dx"] = xd.grad
    ref = dict(r["grads"])
    ref["dL/dx"] = r["gx"]
    allowed = 0.01 if c["f16"] else 0.0
    worst, fails = ("", 0.0), []
    for name, gr in got.items():
        err = (gr.detach().cpu().double() - ref[name]).abs()
        scale = ref[name].abs().max().item()
        tight = 2e-4 * scale + 1e-7
        outliers = (err > tight).double().mean().item()
        worst = max(worst, (name, err.max().item() / tight), key=lambda t: t[1])
        if not (torch.isfinite(gr).all() and outliers <= allowed and err.max().item() <= 0.05 * scale + 1e-7):
            fails.append(f"{name}: {outliers:.2%} of the entries beyond 2e-4 of max|g| = {scale:.3e} (allowed {allowed:.0%}), "
                         f"max err {err.max().item():.3e} = {err.max().item() / tight:.1f} x the tight bound")
    el = abs(loss.item() - r["loss"])
    ez = (z.detach().cpu() - r["z32"]).abs().max().item()
    en = (nll.detach().cpu() - r["nll32"]).abs().max().item()
    print(f"{what} {cid} {c['H']}x{c['W']} batch {c['batch']}: worst {worst[0]} at {worst[1]:.3f} of the tight bound; "
          f"loss err {el:.2e} z err {ez:.2e} nll err {en:.2e}; {counts}")
    assert (counts.get("k_cnet(tape)", 0), counts.get("k_cnet(bwd)", 0)) == (want_cnet, want_cnet), counts
    assert el < 1e-4 and ez <= 1e-4 and en <= 1e-4, (el, ez, en)
    assert not fails, "\n".join(fails)
    return counts


@pytest.mark.parametrize("cid", ALL)
def test_training_step_vs_fp64_autograd_oracle(cid):
    """Tests 1 and 1b.  The step on the kernels the plan picks, and which those were from the run-time launch counters: the fused
    taping and backward k_cnet launches run on tall maps (T: R != W rows per tile, a tile that is a whole image, W = 4), on wide ones
    (W: a tile that is one image row, H = 4), with H = 2 (F, S) and beside levels they do not take (F level 1, S level 2); N1 / N2
    take the shift-expand + MFMA weight gradient with the one-pixel elementwise kernels, N1's second level and R / O the direct
    kernels throughout, with the scalar squeeze and (odd W) the unfused mixer.

    Measured on an MI355X, worst tensor as a multiple of its tight bound: T 0.86, W 1.04, F 0.81, S 1.27 (f.4 weights behind the f16
    pipe), N1 0.003, N2 0.008, R 0.007, O 0.033 (fp32 kernels with fp64 accumulators)."""
    train_step_vs_oracle(cid, CASES[cid]["cnet"], "step")


@pytest.mark.parametrize("cid", ["T", "W", "S"])
def test_training_step_on_the_per_layer_kernels_vs_fp64_autograd_oracle(cid):
    """Test 2.  The same step with the fused launches switched off in both directions, which puts the halo f.0 kernel (several image
    rows per block, as f.0 and as f.4's input gradient), the MFMA tail kernels (as f.4 and as f.0's input gradient), shift-expand and
    the plain weight-gradient GEMM on power-of-two maps with H != W -- against the oracle, not against the fused step.

    Measured on an MI355X: W and S stay below 0.01 of the tight bound everywhere.  T has ONE f.0 pre-activation of its last FlowStep
    (image 0, channel 235, pixel 30) at 7.2e-7 in the fp64 oracle, inside fp32 rounding of the kink: the per-layer f.0 kernel takes the
    other side of it (the fused launch and the fp32 oracle do not), which moves that one row of flow.layers.6.f.0.weight -- 0.17 % of
    its entries, 0.20 % of f.0.actnorm.bias -- by up to 25 x the tight bound = 0.5 % of max|g|.  That is the case the 1 % / 5 % rule is
    there for; no other tensor of T is beyond 1.3 x."""
    with _lib.debug_flags(_lib.DBG.TRAIN_PER_LAYER_FWD | _lib.DBG.TRAIN_PER_LAYER_BWD):
        train_step_vs_oracle(cid, 0, "per-layer step")


@pytest.mark.parametrize("cid", ALL)
def test_inference_vs_oracle_and_round_trip(cid):
    """Test 3.  eval(): normal_flow and reverse_flow (given z and eps) against the fp32 oracle at 1e-4; encode with the Split2d draws
    returned, then decode with them, gives x + noise back at test_gpu_latents.py's round-trip bar of 1e-4."""
    c, r = CASES[cid], reference(cid)
    glow = make_glow(cid, r["sd"]).eval()
    xd, nd = dev(r["x"]), dev(r["noise"])
    z, nll, _ = glow.normal_flow(xd, None, noise=nd)
    ez, en = close(z, r["z32"], 1e-4, "z"), close(nll, r["nll32"], 1e-4, "nll")
    xr = glow.reverse_flow(dev(r["z32"]), None, eps=[dev(e) for e in r["eps"]])
    ex = close(xr, r["x_rev"], 1e-4, "decode")
    z3, _, eps3 = glow.flow.encode(xd + nd, 0., return_eps=True)
    assert [tuple(e.shape[1:]) for e in eps3] == glow.flow.split_shapes((3, c["H"], c["W"]))
    close(z3, r["z32"], 1e-4, "encode z")
    back = glow.flow.decode(z3, eps=eps3)
    eb = close(back, r["x"] + r["noise"], 1e-4, "decode(encode(x))")
    print(f"inference {cid} {c['H']}x{c['W']}: z {ez:.2e} nll {en:.2e} decode {ex:.2e} round trip {eb:.2e}")


@pytest.mark.parametrize("cid", ["N1", "R"])
def test_data_dependent_actnorm_init_through_the_plan(cid):
    """Test 4.  The first training-mode forward of a model whose ActNorms are still zero: every bias at 1e-5, every log-scale at 1e-4
    (test_g8_glow_celeba64_digests' bars) against glow_init_actnorm, and the nll it returns at 1e-4."""
    r = reference(cid)
    glow = make_glow(cid, r["sd0"], inited=False).train()
    assert not glow.actnorm_inited()
    z, nll, _ = glow.normal_flow(dev(r["x"]), None, noise=dev(r["noise"]))
    assert glow.actnorm_inited()
    post = glow.state_dict()
    names = [k for k in r["sd"] if "actnorm." in k]
    assert len(names) == 2 * CASES[cid]["K"] * 6
    worst = {"bias": 0.0, "logs": 0.0}
    for k in names:
        kind = k.rsplit(".", 1)[1]
        worst[kind] = max(worst[kind], (post[k].cpu() - r["sd"][k]).abs().max().item())
    print(f"init {cid}: worst bias err {worst['bias']:.2e} (bar 1e-5), logs err {worst['logs']:.2e} (bar 1e-4)")
    for k in names:
        close(post[k], r["sd"][k], 1e-5 if k.endswith("bias") else 1e-4, k)
    close(nll, r["nll32"], 1e-4, "init nll")

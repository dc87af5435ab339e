"""GPU tests of the differentiable decode (-m gpu): glowhip_plan_decode_vjp / `_GlowDecodeFn` against autograd through
`O.flow_decode` in fp64 on the CPU (tests/decode_grad_oracle.py).

Two kinds of comparison, because the decode's gradient is piecewise constant in the ReLU masks (see decode_grad_oracle.py):
* strict -- every entry within the project's gradient bound 2e-4 max|g| + 1e-7 (tests/test_gpu_grad.py) -- on seeds whose fp64
  ReLU margin is >= 1e-5; the margin is asserted on the CPU before the GPU is touched.  Seeds and margins found by a CPU scan
  are recorded at each case; for every seed listed the fp32 oracle had no entry beyond the bound either.
* the one-wave kernel shapes (4 M hidden units: the smallest |pre-activation| is ~1e-7 at any seed) under the rule of
  test_one_wave_kernel_taping_and_backward_instances_vs_fp64_autograd_oracle: a capped fraction of entries beyond the bound,
  none beyond 5 % of max|g|.  A wrong kernel puts essentially all entries outside."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib  # noqa: E402
from pytorch_glow_amd.network import Inferer, Latents  # noqa: E402

import decode_grad_oracle as D  # noqa: E402

DEV = "cuda:0"
NP_SEED = 5      # numpy seed under which the fixed-permutation models draw their tables


def dev(t):
    return t.to(DEV)


def make_glow(ref, perm="invconv"):
    cfg = ref["cfg"]
    if perm != "invconv":
        np.random.seed(NP_SEED)
    glow = G.Glow(D.hps_for(cfg, cfg["batch"]))
    glow.load_state_dict({k: v.clone() for k, v in ref["sd"].items()})
    glow.set_actnorm_inited()
    return glow.to(DEV).eval()


def plan_of(glow, ref):
    h, w, c = ref["cfg"]["image_shape"]
    return glow.flow.plan_for((c, h, w), torch.device(DEV))


def hip_grads(glow, ref, gx=None, family=None):
    """(x, g_z, [g_eps], launch counts of the backward) through the public autograd surface."""
    plan = plan_of(glow, ref)
    prev = plan.family
    if family is not None:
        plan.set_family(family)
    try:
        lat = Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]).requires_grad_()
        with torch.enable_grad():
            x = glow.decode_latents(lat, safe=False)
            plan.launch_counts(reset=True)
            grads = torch.autograd.grad(x, lat.tensors(), dev(ref["gx"] if gx is None else gx))
            counts = plan.launch_counts(reset=True)
    finally:
        plan.set_family(prev)
    return x.detach(), grads[0], list(grads[1:]), counts


def check_strict(ref, gz, geps, what):
    worst = 0.0
    for name, a, r in [("g_z", gz, ref["gz"])] + [(f"g_eps[{k}]", a, r) for k, (a, r) in enumerate(zip(geps, ref["geps"]))]:
        assert bool(torch.isfinite(a).all()), f"{what} {name}: non-finite"
        frac, rel = D.beyond(a, r)
        print(f"{what} {name}: {frac:.3%} beyond the bound, worst err / max|g| {rel:.2e} (max|g| {float(r.abs().max()):.2e})")
        worst = max(worst, frac)
    assert worst == 0.0, f"{what}: entries beyond 2e-4 max|g| + 1e-7"


def check_capped(ref, gz, geps, cap, what):
    for name, a, r in [("g_z", gz, ref["gz"])] + [(f"g_eps[{k}]", a, r) for k, (a, r) in enumerate(zip(geps, ref["geps"]))]:
        assert bool(torch.isfinite(a).all()), f"{what} {name}: non-finite"
        frac, rel = D.beyond(a, r)
        print(f"{what} {name}: {frac:.3%} beyond the bound (cap {cap:.0%}), worst err / max|g| {rel:.2e} (cap 5e-2)")
        assert frac <= cap and rel <= 5e-2, f"{what} {name}: {frac:.3%} beyond the bound, worst {rel:.2e}"


def assert_margin(ref):
    assert ref["margin"] >= D.MIN_MARGIN, f"ReLU margin {ref['margin']:.2e} of this seed is below {D.MIN_MARGIN:.0e}: pick another seed"
    assert all(bool(torch.isfinite(t).all()) for t in [ref["gz"]] + ref["geps"])


# ------------------------------------------------------------------------------------------------ strict cases
# (id, reference arguments, what the launch counts must show).  Margins from the CPU scan (fp64):
#   tiny affine+invconv   seed 1: 3.7e-5        tiny additive+reverse  seed 2: 8.0e-5
#   32x32 hidden 128      seed 36: 1.4e-5 (27: 1.4e-5, 47: 1.3e-5)
#   16x16 hidden 512      seed 77: 1.6e-5 (14: 1.4e-5, 74: 1.3e-5); batch 2 is enough for the taping instance
#   32x32 L 5             seed 9: 2.2e-5        64x64 L 6              seed 25: 1.3e-5 (67: 1.2e-5)
TINY = dict(image=16, hidden=32, K=2, L=2, batch=3, zeros_std=0.05)
TINY_AFF = dict(TINY, seed=1)
TINY_ADD = dict(TINY, seed=2, perm="reverse", coup="additive", np_seed=NP_SEED)
MID = dict(image=32, hidden=128, K=2, L=2, batch=2, zeros_std=0.05, seed=36)
WIDE_HIDDEN = dict(image=16, hidden=512, K=2, L=1, batch=2, zeros_std=0.01, seed=77)
DEEP5 = dict(image=32, hidden=32, K=1, L=5, batch=2, zeros_std=0.05, seed=9, stable=True)
DEEP6 = dict(image=64, hidden=32, K=1, L=6, batch=4, zeros_std=0.02, seed=25, stable=True)


@pytest.mark.parametrize("kw", [pytest.param(TINY_AFF, id="tiny-affine-invconv"), pytest.param(TINY_ADD, id="tiny-additive-reverse"),
                                pytest.param(MID, id="32x32-hidden128"), pytest.param(DEEP5, id="32x32-L5"),
                                pytest.param(DEEP6, id="64x64-L6")])
def test_decode_gradients_every_entry_vs_fp64_autograd_oracle(kw):
    ref = D.reference(**kw)
    assert_margin(ref)
    glow = make_glow(ref, kw.get("perm", "invconv"))
    x, gz, geps, counts = hip_grads(glow, ref)
    print(kw, "margin", ref["margin"], counts)
    ex = float((x.cpu().double() - ref["x"]).abs().max())
    assert ex <= 1e-4, f"decode itself: {ex:.2e}"
    check_strict(ref, gz, geps, str(kw["image"]))
    nsteps = kw["K"] * kw["L"]
    assert counts.get("k_chanmix_inv_bwd", 0) + counts.get("k_chanmix_inv_bwd_wide", 0) == nsteps, counts
    if kw["L"] >= 5:      # C = 12 ... 192 on the pixel-block form, C = 384 on the channel-slice form
        assert counts.get("k_chanmix_inv_bwd_wide", 0) == kw["L"] - 5 and counts.get("k_chanmix_inv_bwd", 0) == 5, counts


def test_hidden_512_runs_the_taping_and_backward_k_cnet_and_gathers_their_partial_sums():
    """8x8 level, two steps: step 0's partial sums are gathered by step 1's mixer VJP, step 1's by the gather-only kernel."""
    ref = D.reference(**WIDE_HIDDEN)
    assert_margin(ref)
    glow = make_glow(ref)
    plan = plan_of(glow, ref)
    lat = Latents(dev(ref["z"]), []).requires_grad_()
    with torch.enable_grad():
        x = glow.decode_latents(lat, safe=False)
        plan.launch_counts(reset=True)
        gz, = torch.autograd.grad(x, [lat.z], dev(ref["gx"]))
        counts = plan.launch_counts(reset=True)
    print(counts, "margin", ref["margin"])
    assert counts.get("k_cnet(tape)") == 2 and counts.get("k_cnet(bwd)") == 2, counts
    assert counts.get("k_cpart_finish") == 1 and counts.get("k_chanmix_inv_bwd") == 2, counts
    check_strict(ref, gz, [], "hidden 512")


def test_exact_fp32_family_runs_no_k_cnet_and_meets_the_strict_bound():
    ref = D.reference(**MID)
    assert_margin(ref)
    glow = make_glow(ref)
    _, gz, geps, counts = hip_grads(glow, ref, family=1)
    assert not any(k.startswith("k_cnet") for k in counts), counts
    check_strict(ref, gz, geps, "exact fp32")


# ------------------------------------------------------------------------------------------------ one-wave kernel shapes
@pytest.mark.parametrize("K,hidden,batch,perm,coup,cap", [pytest.param(1, 512, 4, "invconv", "affine", 0.01, id="K1"),
                                                          pytest.param(2, 512, 4, "invconv", "affine", 0.05, id="K2"),
                                                          pytest.param(2, 256, 4, "shuffle", "additive", 0.05, id="K2-additive-shuffle-256"),
                                                          pytest.param(1, 512, 28, "invconv", "affine", 0.01, id="K1-one-wave"),
                                                          pytest.param(2, 512, 28, "invconv", "affine", 0.05, id="K2-one-wave")])
def test_one_wave_kernel_shapes_vs_fp64_autograd_oracle(K, hidden, batch, perm, coup, cap):
    """64x64, L 1.  At batch 4 (32 tiles of 128 pixels) the level runs the two-wave k_cnet instances; the one-wave k_cnet1w takes a
    level from 224 tiles on (tests/test_gpu_grad.py: batch 28), so its taping and backward instances are asserted from the launch
    counters at batch 28, under the same rules."""
    kw = dict(image=64, hidden=hidden, K=K, L=1, batch=batch, zeros_std=0.01, seed=2, perm=perm, coup=coup)
    if perm != "invconv":
        kw["np_seed"] = NP_SEED
    ref = D.reference(**kw)
    glow = make_glow(ref, perm)
    _, gz, geps, counts = hip_grads(glow, ref)
    print(counts, "margin", ref["margin"])
    if hidden == 512:
        assert counts.get("k_cnet(tape)") == K and counts.get("k_cnet(bwd)") == K, counts
        one_wave = K if batch >= 28 else 0
        assert counts.get("k_cnet1w(tape)", 0) == one_wave and counts.get("k_cnet1w(bwd)", 0) == one_wave, counts
    check_capped(ref, gz, geps, cap, f"K{K} hidden {hidden} batch {batch}")


# ------------------------------------------------------------------------------------------------ linearity, range, reproducibility
def test_vjp_is_linear_to_the_bit_over_2_to_the_pm20_and_per_sample():
    ref = D.reference(**MID)
    assert_margin(ref)
    glow = make_glow(ref)
    _, gz, geps, _ = hip_grads(glow, ref)
    for a in (2.0 ** 20, 2.0 ** -20):
        _, gza, gepsa, _ = hip_grads(glow, ref, gx=ref["gx"] * a)
        assert torch.equal(gza, gz * a), f"alpha {a}: g_z differs"
        assert all(torch.equal(x, y * a) for x, y in zip(gepsa, geps)), f"alpha {a}: g_eps differs"
    # samples 2^24 apart in scale: each meets the strict bound against ITS reference
    scale = torch.tensor([1.0, 2.0 ** 24]).view(-1, 1, 1, 1)
    _, gzs, gepss, _ = hip_grads(glow, ref, gx=ref["gx"] * scale)
    for n in range(2):
        s = float(scale[n])
        for a, r in zip([gzs] + gepss, [ref["gz"]] + ref["geps"]):
            frac, rel = D.beyond(a[n:n + 1] / s, r[n:n + 1])
            assert frac == 0.0, f"sample {n}: {frac:.3%} beyond the bound ({rel:.2e})"
    # an all-zero g_x[n]: exact zeros for that sample, the other untouched
    gx0 = ref["gx"].clone()
    gx0[0] = 0
    _, gz0, geps0, _ = hip_grads(glow, ref, gx=gx0)
    for a, b in zip([gz0] + geps0, [gz] + geps):
        assert float(a[0].abs().max()) == 0.0 and torch.equal(a[1], b[1])


def test_vjp_is_bitwise_reproducible():
    ref = D.reference(**MID)
    glow = make_glow(ref)
    _, gz, geps, _ = hip_grads(glow, ref)
    _, gz2, geps2, _ = hip_grads(glow, ref)
    assert torch.equal(gz, gz2) and all(torch.equal(a, b) for a, b in zip(geps, geps2))


# ------------------------------------------------------------------------------------------------ autograd plumbing
def test_autograd_plumbing():
    ref = D.reference(**TINY_AFF)
    glow = make_glow(ref)
    base = Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]])
    with torch.no_grad():
        x_plain = glow.decode_latents(base, safe=False)
    # no input requires grad: no graph, today's bits
    with torch.enable_grad():
        x_nograd = glow.decode_latents(base, safe=False)
    assert x_nograd.grad_fn is None and not x_nograd.requires_grad and torch.equal(x_nograd, x_plain)
    # .backward() fills every latent's .grad; the forward's bits are the plain decode's
    lat = base.requires_grad_()
    assert isinstance(lat, Latents) and all(t.is_leaf and t.requires_grad for t in lat.tensors())
    with torch.enable_grad():
        x = glow.decode_latents(lat, safe=False)
        assert x.grad_fn is not None and torch.equal(x.detach(), x_plain)
        x.sum().backward()
    assert lat.z.grad is not None and all(e.grad is not None for e in lat.eps)
    assert all(p.grad is None for p in glow.parameters()), "parameter gradients do not flow through the decode"
    det = lat.detach()
    assert isinstance(det, Latents) and not any(t.requires_grad for t in det.tensors())
    # an input that does not require grad gets None
    z = dev(ref["z"]).requires_grad_()
    eps = [dev(e) for e in ref["eps"]]
    with torch.enable_grad():
        x = glow.reverse_flow(z, eps=eps)
        x.backward(torch.ones_like(x), retain_graph=True)
        gz = z.grad
        assert eps[0].grad is None and torch.equal(gz, lat.z.grad)
        # the node keeps nothing but the image: a second differentiation of the same forward works and agrees to the bit
        gz2, = torch.autograd.grad(x, [z], torch.ones_like(x))
        assert torch.equal(gz2, gz)
    # z = None: eps_top gets its gradient through plain torch on top of the node
    n = ref["z"].shape[0]
    eps_top = torch.randn((n,) + tuple(ref["z"].shape[1:]), device=DEV, requires_grad=True)
    with torch.enable_grad():
        x = glow.reverse_flow(None, eps=eps, eps_top=eps_top)
        x.sum().backward()
    z_top = eps_top.detach().clone().requires_grad_()
    with torch.enable_grad():
        glow.reverse_flow(z_top, eps=eps).sum().backward()
    assert eps_top.grad is not None and torch.equal(eps_top.grad, z_top.grad)      # (zero prior: z = eps_top)
    # a parameter changed in place between forward and backward raises
    with torch.enable_grad():
        x = glow.decode_latents(base.requires_grad_(), safe=False)
        with torch.no_grad():
            glow.flow.layers[1].actnorm.bias.add_(0.125)
        with pytest.raises(_lib.GlowHipError, match="parameter changed"):
            x.sum().backward()


def test_c_abi_argument_checks_on_the_device():
    ref = D.reference(**TINY_AFF)
    glow = make_glow(ref)
    plan = plan_of(glow, ref)
    x = torch.rand(3, 3, 16, 16, device=DEV)
    with pytest.raises(AssertionError):
        plan.decode_vjp(x, x, want_eps=[])
    gz, geps = plan.decode_vjp(x, torch.zeros_like(x), want_z=False)
    assert gz is None and len(geps) == 1 and float(geps[0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ fit_latents
FIT_RATIO = 0.1


def test_fit_latents_inpaints_the_masked_half():
    """In-painting on the 16x16 / hidden 32 model: the target is a decoded image, the mask its left half, the start the latents of
    the image with that half blanked (a start that already matches under the mask would have nothing to fit).  20 Adam steps at
    lr 0.2.  The same optimisation through the fp64 oracle on the CPU: masked loss 3.318e-01 -> 2.778e-02, falling at every step,
    final / first = 0.084 -- below a tenth, so the ratio asked of the HIP path is the tenth."""
    ref = D.reference(**TINY_AFF)
    glow = make_glow(ref)
    inf = Inferer(D.hps_for(ref["cfg"], ref["cfg"]["batch"]), glow, [DEV], DEV)
    with torch.no_grad():
        target = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    mask = torch.zeros_like(target)
    mask[..., : target.shape[-1] // 2] = 1.0
    init = inf.encode_full(target * (1.0 - mask))      # starts from the image with the masked half blanked: the fit has to paint it back
    lat, hist = inf.fit_latents(target, mask=mask, steps=20, lr=0.2, init=init)
    print("masked loss:", " ".join(f"{v:.3e}" for v in hist))
    assert isinstance(lat, Latents) and len(hist) == 20
    assert all(b < a for a, b in zip(hist[:5], hist[1:6])), hist
    assert hist[-1] <= FIT_RATIO * hist[0], (hist[0], hist[-1])


# ------------------------------------------------------------------------------------------------ class-conditional plan
def test_conditional_plan_with_z_given_meets_the_strict_bound():
    """The VJP of the flow does not involve the head: g10's tiny conditional config, learn_top on, z given."""
    from conftest import load_golden
    import ycond_oracle as Y
    from test_ycond_host import ycond_hps
    g = load_golden("g10_glow_tiny_ycond")
    sd = Y.case_state(g, 1)
    cfg = dict(Y.TINY, learn_top=True, y_condition=True)
    np.random.seed(3)
    glow = G.Glow(ycond_hps(learn_top=True, weight_y=float(g["weight_y"]), device=DEV))
    glow.load_state_dict(sd, strict=True)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).eval()
    x0 = g["x"] + g["noise"]
    with torch.no_grad():
        z, eps = D.encode_latents(x0, sd, cfg)
    gx = torch.randn(x0.shape, generator=torch.Generator().manual_seed(11))
    margin = D.decode_margin(z.double(), [e.double() for e in eps], {k: v.double() for k, v in sd.items()}, cfg)
    assert margin >= D.MIN_MARGIN, margin
    _, gz_ref, geps_ref = D.decode_grads(z, eps, gx, sd, cfg)
    glow.normal_flow(dev(g["x"]), g["y_onehot_ce"].to(DEV), noise=dev(g["noise"]))      # (attaches the head to the plan)
    lat = Latents(dev(z), [dev(e) for e in eps]).requires_grad_()
    with torch.enable_grad():
        grads = torch.autograd.grad(glow.decode_latents(lat, safe=False), lat.tensors(), dev(gx))
    check_strict(dict(gz=gz_ref, geps=geps_ref), grads[0], list(grads[1:]), "y_condition")

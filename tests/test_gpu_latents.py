"""GPU tests of the full-latent encode (-m gpu): every Split2d's prior kernel also stores eps = (z2 - mean) * exp(-logs) when
latent buffers are bound (glowhip_plan_bind_latents), so decode(encode(x)) is x.

References: tests/golden/g11_glow_latents.npz (recorded from the real reference by tests/golden/make_golden_latents.py) and the
CPU oracle's walk (tests/latents_oracle.py) on a seeded config.  Tolerances: the project's z / decode tolerance 1e-4;
for eps itself the same bar carried through the division, 1e-4 * max exp(-logs_ref)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from pytorch_glow_amd.network import Inferer, Latents  # noqa: E402
from pytorch_glow_amd.network import model as gmodel  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402

import latents_oracle as LO  # noqa: E402

DEV = "cuda:0"
FAMILIES = [pytest.param(0, id="auto"), pytest.param(1, id="exact_fp32")]     # GLOWHIP_FAMILY_AUTO / _EXACT_FP32


def dev(t):
    return t.to(DEV)


def maxerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item()


def make_glow(cfg, sd, batch, num_classes=1):
    hps = util.AttrDict(dict(
        model=dict(image_shape=cfg["image_shape"], hidden_channels=cfg["hidden_channels"], K=cfg["K"], L=cfg["L"],
                   actnorm_scale=cfg["actnorm_scale"], n_bits_x=cfg["n_bits_x"], weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False,
                      flow_permutation=cfg["flow_permutation"], flow_coupling=cfg["flow_coupling"]),
        optim=dict(num_batch_train=batch), dataset=dict(num_classes=num_classes), device=dict(graph=["cuda:0"])))
    glow = G.Glow(hps)
    sd = {k: v.clone() for k, v in sd.items()}
    sd["h_top"] = torch.zeros_like(glow.h_top)
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    return glow.to(DEV).eval(), hps


def g11_case(golden):
    g = golden("g11_glow_latents")
    refs = [{name: g[f"{name}_{k}"] for name in ("z2", "mean", "logs", "eps")} for k in range(2)]
    return LO.G11, LO.g11_state(g), g["x"], g["noise"], refs, g["z"], g["nll"]


def seeded_case():
    cfg, sd, x, noise = LO.seeded_case()
    z, _, refs = LO.flow_encode_latents(x + noise, torch.zeros(x.shape[0]), sd, cfg)
    _, nll, _ = O.glow_forward(x, noise, sd, cfg)
    return cfg, sd, x, noise, refs, z, nll


def case(name, golden):
    return g11_case(golden) if name == "g11" else seeded_case()


class family:
    """Run a block with the plan on one kernel family (a property of the plan; restored afterwards)."""

    def __init__(self, plan, fam):
        self.plan, self.fam = plan, fam

    def __enter__(self):
        self.prev = self.plan.family
        self.plan.set_family(self.fam)

    def __exit__(self, *a):
        self.plan.set_family(self.prev)


def check_eps(eps_hip, refs, what):
    """Both forms of the bar: z2 rebuilt from the reference prior and the HIP eps within 1e-4 of the reference z2, and eps itself
    within 1e-4 * max exp(-logs_ref).  Prints the figures before asserting."""
    assert len(eps_hip) == len(refs)
    for k, (e, r) in enumerate(zip(eps_hip, refs)):
        e = e.cpu()
        assert e.shape == r["eps"].shape, (e.shape, r["eps"].shape)
        assert torch.isfinite(e).all()
        ez2 = maxerr(r["mean"] + torch.exp(r["logs"]) * e, r["z2"])
        bound = 1e-4 * torch.exp(-r["logs"]).max().item()
        ee = maxerr(e, r["eps"])
        print(f"{what} split {k}: z2-form err {ez2:.2e} (bar 1e-4); eps err {ee:.2e} (bar {bound:.2e}); |eps| max {e.abs().max().item():.2f}")
        assert ez2 <= 1e-4, f"{what} split {k}: z2 form {ez2:.2e}"
        assert ee <= bound, f"{what} split {k}: eps {ee:.2e} > {bound:.2e}"


# ------------------------------------------------------------------------------------------------ 1. eps against the reference
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("name", ["g11", "seeded"])
def test_eps_of_the_whole_model_vs_reference(golden, name, fam):
    cfg, sd, x, noise, refs, z_ref, nll_ref = case(name, golden)
    glow, _ = make_glow(cfg, sd, x.shape[0])
    plan = glow.flow.plan_for(dev(x))
    with family(plan, fam):
        plan.launch_counts(reset=True)
        lat = glow.encode_latents(dev(x), noise=dev(noise), safe=False)
        counts = plan.launch_counts(reset=True)
    assert counts.get("split_prior(k_conv_tail)") == cfg["L"] - 1, counts      # 16x16 and 8x8 maps, 6 / 12 input channels
    assert [tuple(e.shape[1:]) for e in lat.eps] == glow.flow.split_shapes((3, 32, 32))
    ez, en = maxerr(lat.z, z_ref), maxerr(lat.nll, nll_ref)
    print(f"{name} family {fam}: z err {ez:.2e} nll err {en:.2e}")
    assert ez <= 1e-4 and en <= 1e-4
    check_eps(lat.eps, refs, f"{name} family {fam}")


def _split_module(c, seed):
    g = torch.Generator().manual_seed(seed)
    sp = G.Split2d(c)
    with torch.no_grad():
        sp.conv2d_zeros.weight.copy_(torch.randn(sp.conv2d_zeros.weight.shape, generator=g) * 0.05)
        sp.conv2d_zeros.bias.copy_(torch.randn(sp.conv2d_zeros.bias.shape, generator=g) * 0.3)
        sp.conv2d_zeros.logs.copy_(torch.randn(sp.conv2d_zeros.logs.shape, generator=g) * 0.1)
    sd = {k: v.clone() for k, v in sp.state_dict().items()}
    return sp.to(DEV).eval(), sd, g


def _check_split_module(c, h, w, n, fam, want_route=None):
    sp, sd, g = _split_module(c, seed=c * 100 + h)
    x = torch.randn(n, c, h, w, generator=g)
    plan = sp._plans.get([sp], (c, h, w), torch.device(DEV))
    with family(plan, fam):
        sp(dev(x), 0.)                      # (the first call packs: kept out of the launch counts)
        plan.launch_counts(reset=True)
        z1, ld, eps = sp(dev(x), 0., return_eps=True)
        counts = plan.launch_counts(reset=True)
        z1b, ldb = sp(dev(x), 0.)
        counts_b = plan.launch_counts(reset=True)
        xr, _ = sp(z1, 0., reverse=True, eps=eps[0])
    routes = {k: v for k, v in counts.items() if k.startswith("split_prior(")}
    if want_route is not None:
        assert routes == {f"split_prior({want_route})": 1}, counts
    else:
        assert len(routes) == 1 and next(iter(routes)).startswith("split_prior(k_conv_tail"), counts
    assert counts == counts_b, "binding latents must not add a launch"
    assert torch.equal(z1, z1b) and torch.equal(ld, ldb)
    ref = LO.split_eps(x, sd, "")
    assert torch.equal(z1.cpu(), x[:, :c // 2])
    check_eps(eps, [ref], f"Split2d({c}) {h}x{w} {routes}")
    exr = maxerr(xr, x)
    print(f"  reverse with its own eps: {exr:.2e}")
    assert exr <= 1e-4


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("route,c,h,w", [
    ("k_split_tail", 12, 4, 4),          # maps narrower than the MFMA tail kernels take: direct conv + k_split_tail
    ("k_split_tail", 8, 6, 10),          # width not a multiple of 4
    ("k_split_tail", 6, 3, 5),
    ("k_conv_tail", 12, 32, 32),         # register-staged MFMA tail (fewer than 32 input channels)
    ("k_conv_tail", 24, 16, 16),
    ("k_conv_tail", 48, 8, 8),
    ("k_conv_tail_dma", 64, 16, 16),     # its LDS-DMA twin: 32 / 48 input channels, out-channel tiles split over blockIdx.y
    ("k_conv_tail_dma", 96, 8, 8),
    ("k_conv_tail_dma", 64, 32, 32),
])
def test_eps_on_every_split_route(route, c, h, w, fam):
    _check_split_module(c, h, w, 3, fam, want_route=route)


_TILE_CASES = [(tp, c, h, w, ms) for (c, h, w) in [(12, 32, 32), (24, 16, 16), (48, 8, 8), (64, 16, 16), (96, 8, 8)]
               for tp in (16, 32, 64, 128) for ms in (0x100, 0x200)
               if (h * w) % tp == 0 and tp % w == 0 and not (ms == 0x200 and c > 48)]   # (> 3 out-channel tiles need the split)


@pytest.mark.parametrize("tp,c,h,w,msplit", _TILE_CASES)
def test_eps_on_every_tail_wave_layout(tp, c, h, w, msplit):
    """Each pixel-tile / K-split variant of the two MFMA tail kernels, with and without the out-channel split."""
    with _lib.debug_flags(tp | msplit):
        _check_split_module(c, h, w, 3, 0)


# ------------------------------------------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("name", ["g11", "seeded"])
def test_round_trip(golden, name, fam):
    cfg, sd, x, noise, _, _, _ = case(name, golden)
    glow, _ = make_glow(cfg, sd, x.shape[0])
    with family(glow.flow.plan_for(dev(x)), fam):
        lat = glow.encode_latents(dev(x), noise=dev(noise), safe=False)
        back = glow.decode_latents(lat, safe=False)
        e1 = maxerr(back, x + noise)
        lat0 = glow.encode_latents(dev(x), dequantize=False, safe=False)
        e0 = maxerr(glow.decode_latents(lat0, safe=False), x)
        drawn = glow.encode_latents(dev(x), safe=False)              # in-kernel dequantisation draw: inside [x, x + 1/256)
        d = (glow.decode_latents(drawn, safe=False).cpu() - x)
    print(f"{name} family {fam}: round trip {e1:.2e}; without dequantisation {e0:.2e}")
    assert e1 <= 1e-4 and e0 <= 1e-4
    assert d.min().item() >= -1e-4 and d.max().item() <= 1.0 / 256 + 1e-4 and d.abs().max().item() > 1e-3
    assert not torch.equal(lat0.z, lat.z)


@pytest.mark.parametrize("name", ["g11", "seeded"])
def test_round_trip_from_uint8_pixels(golden, name):
    cfg, sd, x, noise, _, _, _ = case(name, golden)
    glow, _ = make_glow(cfg, sd, x.shape[0])
    u8 = torch.floor(x * 255.0).clamp(0, 255).to(torch.uint8)
    xf = u8.float() / 255.0
    lat = glow.encode_latents(dev(u8), noise=dev(noise), safe=False)
    e1 = maxerr(glow.decode_latents(lat, safe=False), xf + noise)
    lat0 = glow.encode_latents(dev(u8), dequantize=False, safe=False)
    e0 = maxerr(glow.decode_latents(lat0, safe=False), xf)
    print(f"{name} uint8: round trip {e1:.2e}; without dequantisation {e0:.2e}")
    assert e1 <= 1e-4 and e0 <= 1e-4


# ------------------------------------------------------------------------------------------------ 3. nothing else moves
@pytest.mark.parametrize("fam", FAMILIES)
def test_binding_changes_nothing_else(golden, fam):
    cfg, sd, x, noise, _, _, _ = seeded_case()
    glow, _ = make_glow(cfg, sd, x.shape[0])
    xd, nd = dev(x), dev(noise)
    plan = glow.flow.plan_for(xd)
    with family(plan, fam):
        z0, nll0, _ = glow.normal_flow(xd, None, noise=nd)         # warm: packs
        plan.launch_counts(reset=True)
        z0, nll0, _ = glow.normal_flow(xd, None, noise=nd)
        c0 = plan.launch_counts(reset=True)
        lat = glow.encode_latents(xd, noise=nd, safe=False)
        c1 = plan.launch_counts(reset=True)
        assert torch.equal(lat.z, z0) and torch.equal(lat.nll, nll0), "z / nll must be bit-identical with latents bound"
        assert c0 == c1, (c0, c1)
        # unbound again: a further forward leaves the buffers alone
        kept = [e.clone() for e in lat.eps]
        for e in lat.eps:
            e.fill_(-7.0)
        z1, nll1, _ = glow.normal_flow(xd, None, noise=nd)
        torch.cuda.synchronize()
        assert all(bool((e == -7.0).all()) for e in lat.eps), "a forward after the unbind wrote a previously bound buffer"
        assert torch.equal(z1, z0) and torch.equal(nll1, nll0)
        # deterministic
        again = glow.encode_latents(xd, noise=nd, safe=False)
        assert all(torch.equal(a, b) for a, b in zip(again.eps, kept))
        # FlowModel.encode: the two-tuple of before, and the same numbers with the flag
        out = glow.flow.encode(xd + nd, 0.)
        assert isinstance(out, tuple) and len(out) == 2
        z3, ld3, eps3 = glow.flow.encode(xd + nd, 0., return_eps=True)
        assert torch.equal(out[0], z3) and torch.equal(out[1], ld3)
        assert [e.shape for e in eps3] == [e.shape for e in kept]
        xb = glow.flow.decode(z3, eps=eps3)
        assert maxerr(xb, x + noise) <= 1e-4


def test_plan_level_binding_errors_and_training_forward():
    cfg, sd, x, noise = LO.seeded_case()
    glow, _ = make_glow(cfg, sd, x.shape[0])
    xd, nd = dev(x), dev(noise)
    plan = glow.flow.plan_for(xd)
    bufs = plan.latent_buffers(4)
    with pytest.raises(G.GlowHipError, match="1 buffers given"):
        plan.encode(xd, None, None, eps_out=bufs[:1])
    with pytest.raises(G.GlowHipError, match=r"eps_out\[1\]"):
        plan.encode(xd, None, None, eps_out=[bufs[0], bufs[1][:2]])
    arr = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in bufs], bufs[0].data_ptr())
    assert G.lib().glowhip_plan_bind_latents(plan._h, arr, 3) == -1
    msg = G.lib().glowhip_last_error().decode()
    assert "3 latent buffers" in msg and "2 Split2d" in msg, msg
    # the training forward ignores a binding
    for b in bufs:
        b.fill_(-7.0)
    plan._bind_latents(bufs, 4)
    try:
        glow.train()
        with torch.enable_grad():
            z, nll, _ = glow.normal_flow(xd, None, noise=nd)
            assert nll.requires_grad
        torch.cuda.synchronize()
        assert all(bool((b == -7.0).all()) for b in bufs)
        glow.eval()
        z2, _, _ = glow.normal_flow(xd, None, noise=nd)          # ... the inference forward honours it until it is unbound
        torch.cuda.synchronize()
        assert not any(bool((b == -7.0).any()) for b in bufs)
    finally:
        glow.eval()
        plan._unbind_latents()


# ------------------------------------------------------------------------------------------------ 4. range
def test_range_flag_and_the_checked_encode():
    """Weights scaled as in test_split_half_survives_large_and_tiny_activations, far enough that the first coupling network's
    hidden activations (~1e5) leave the fp16 pairs' range: the unchecked encode reports a non-finite nll (and claims nothing about
    eps); the checked one returns the exact-fp32 family's latents."""
    cfg = O.default_cfg(image_shape=(16, 16, 3), hidden_channels=64, K=1, L=2, batch=4)
    sd = O.seeded_state_dict(cfg, seed=3, zeros_std=0.02)
    sd["flow.layers.1.f.0.weight"] = sd["flow.layers.1.f.0.weight"] * 3e5
    sd["flow.layers.1.f.2.weight"] = sd["flow.layers.1.f.2.weight"] / 3e5       # keep h2 modest
    g = torch.Generator().manual_seed(9)
    x = torch.rand(4, 3, 16, 16, generator=g); noise = torch.rand(4, 3, 16, 16, generator=g) / 256
    glow, _ = make_glow(cfg, sd, 4)
    xd, nd = dev(x), dev(noise)
    plan = glow.flow.plan_for(xd)
    unsafe = glow.encode_latents(xd, noise=nd, safe=False)
    assert not bool(torch.isfinite(unsafe.nll).all()), "this input is meant to overflow the split-half range"
    n0 = G.Glow._RANGE_FALLBACKS
    lat = glow.encode_latents(xd, noise=nd, safe=True)
    assert G.Glow._RANGE_FALLBACKS == n0 + 1 and plan.family == plan.FAMILY_AUTO
    assert all(bool(torch.isfinite(t).all()) for t in lat.tensors() + [lat.nll])
    with family(plan, plan.FAMILY_EXACT_FP32):
        exact = glow.encode_latents(xd, noise=nd, safe=False)
    assert torch.equal(lat.z, exact.z) and torch.equal(lat.nll, exact.nll)
    assert all(torch.equal(a, b) for a, b in zip(lat.eps, exact.eps))
    default = glow.encode_latents(xd, noise=nd)                 # eval + range_check: checked by default
    assert G.Glow._RANGE_FALLBACKS == n0 + 2 and torch.equal(default.eps[0], exact.eps[0])


# ------------------------------------------------------------------------------------------------ 5. Inferer
@pytest.fixture()
def inferer(golden):
    cfg, sd, x, noise, _, _, _ = g11_case(golden)
    glow, hps = make_glow(cfg, sd, 4, num_classes=3)
    return Inferer(hps, glow, [0], DEV), glow, x


def test_inferer_reconstruct_and_interpolate(inferer):
    inf, glow, x = inferer
    one = inf.reconstruct(x[1])
    assert one.shape == (3, 32, 32)
    e1 = maxerr(one, x[1])
    eb = maxerr(inf.reconstruct(x), x)                         # a batch, taken as it is
    u8 = torch.floor(x * 255.0).clamp(0, 255).to(torch.uint8)
    eu = maxerr(inf.reconstruct(u8[:3]), u8[:3].float() / 255.0)
    lat = inf.encode_full(x[:2])
    assert isinstance(lat, Latents) and len(lat) == 2 and lat.z.shape == (2, 48, 4, 4)
    assert maxerr(inf.decode_full(lat.to("cpu")), x[:2]) <= 1e-4
    steps = 5
    path = inf.interpolate(x[0], x[2], steps)
    assert path.shape == (steps, 3, 32, 32) and torch.isfinite(path).all()
    ea, eb2 = maxerr(path[0], x[0]), maxerr(path[-1], x[2])
    print(f"reconstruct {e1:.2e} (batch {eb:.2e}, uint8 {eu:.2e}); interpolation ends {ea:.2e} {eb2:.2e}")
    assert max(e1, eb, eu, ea, eb2) <= 1e-4
    assert maxerr(path[2], x[0]) > 1e-2 and maxerr(path[2], x[2]) > 1e-2, "the middle of the path is neither endpoint"


def test_inferer_attribute_delta_keeps_details(inferer):
    inf, glow, x = inferer
    g = torch.Generator().manual_seed(4)
    deltaz = (torch.randn(3, 48, 4, 4, generator=g) * 0.1).numpy()
    img = x[0]
    same = inf.apply_attribute_delta(img, deltaz, [0.0, 0.0, 0.0], keep_details=True)
    assert same.shape == img.shape
    e0 = maxerr(same, img)
    moved = inf.apply_attribute_delta(img, deltaz, [0.5, 0.0, -1.0], keep_details=True)
    again = inf.apply_attribute_delta(img, deltaz, [0.5, 0.0, -1.0], keep_details=True)
    batch = inf.apply_attribute_delta(x[:2], deltaz, [0.5, 0.0, -1.0], keep_details=True)
    print(f"keep_details, zero interpolation: {e0:.2e}; shifted: moves the image by {maxerr(moved, img):.2e}")
    assert e0 <= 1e-4
    assert torch.equal(moved, again), "no random draw is left in a decode of full latents"
    assert maxerr(moved, img) > 1e-3 and batch.shape == (2, 3, 32, 32) and maxerr(batch[0], moved) <= 1e-4
    # the reference's call is what it was: fresh draws for every dropped half
    interp = [0.5, 0.0, -1.0]
    torch.manual_seed(7); gmodel.reset_dequant_stream()
    out = inf.apply_attribute_delta(img, deltaz, interp)
    torch.manual_seed(7); gmodel.reset_dequant_stream()
    z0 = inf.encode(img)
    coef = torch.as_tensor(np.asarray(interp, dtype=np.float32), device=DEV)
    want = inf.decode(z0 + (torch.as_tensor(deltaz, dtype=torch.float32).to(DEV) * coef.view(-1, 1, 1, 1)).sum(0))
    assert torch.equal(out, want)
    assert maxerr(out, moved) > 1e-3


# ------------------------------------------------------------------------------------------------ 6. per-level temperature
def bits_equal(a, b):
    """Bitwise: an untrained model's samples may hold non-finite pixels, which no == compares equal."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_eps_std_per_level(inferer):
    inf, glow, x = inferer
    L = 3
    torch.manual_seed(11)
    a = glow.reverse_flow(None, eps_std=0.6)
    torch.manual_seed(11)
    b = glow.reverse_flow(None, eps_std=[0.6] * L)
    assert a.shape == (4, 3, 32, 32) and bits_equal(a, b)
    mixed = [0.7, 0.5, 0.3]
    torch.manual_seed(12)
    c = glow.reverse_flow(None, eps_std=mixed)
    torch.manual_seed(12)
    top = torch.randn_like(torch.zeros(4, 48, 4, 4, device=DEV)) * 0.7      # the draw of GaussianDiag.eps, scaled by hand
    eps = [torch.randn((4,) + s, dtype=torch.float32, device=DEV) * std
           for s, std in zip(glow.flow.split_shapes((3, 32, 32)), (0.5, 0.3))]
    d = glow.reverse_flow(None, eps=eps, eps_top=top)
    assert bits_equal(c, d) and not bits_equal(c, a)
    torch.manual_seed(12)
    s = inf.sample(z=None, y_onehot=None, eps_std=mixed)
    assert bits_equal(s, c)
    z = torch.randn(4, 48, 4, 4, device=DEV)
    torch.manual_seed(13)
    e = glow.flow.decode(z, eps_std=mixed)
    torch.manual_seed(13)
    f = glow.flow.decode(z, eps=[torch.randn((4,) + s, dtype=torch.float32, device=DEV) * std
                                 for s, std in zip(glow.flow.split_shapes((3, 32, 32)), (0.5, 0.3))])
    assert bits_equal(e, f)
    with pytest.raises(ValueError, match="L = 3"):
        glow.reverse_flow(None, eps_std=[0.5, 0.5])

"""GPU tests of the sampler (-m gpu): Gaussian draws made inside the kernels that consume them (csrc/sampler_rng.h).

The contract is the stream definition of include/glowhip.h, restated in numpy by tests/sampler_oracle.py.  Everything downstream
of the draw is held to BIT equality with the same decode given the stream as an injected tensor (`FlowPlan.normal_noise`).

Bound of the draw against the fp64 oracle, derived (not measured): the uniform words are exact, so the error is that of fp32
logf / sqrtf (a few 1e-7 relative on r <= 5.77) plus r times the error of the angle -- fl(2 pi) is off by 1.7e-7 relative, the
product 2 pi u2 < 6.29 rounds by at most 2.4e-7, cosf / sinf add ~1e-7 -- together below 5.77 * 7e-7 = 4e-6; with a factor 2
over it and the std <= 1 of the cases: 1e-5 absolute."""
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

import sampler_oracle as SO  # noqa: E402
import ycond_oracle as Y  # noqa: E402

DEV = "cuda:0"
FAMILIES = [pytest.param(0, id="auto"), pytest.param(1, id="exact_fp32")]     # GLOWHIP_FAMILY_AUTO / _EXACT_FP32
TRIPLES = [(1234, 0, 0), (99, 7, 3), (2 ** 64 - 3, 2 ** 32 + 1, 1)]           # (seed, call, stream)


class family:
    """Run a block with the plan on one kernel family (a property of the plan; restored afterwards)."""

    def __init__(self, plan, fam):
        self.plan, self.fam = plan, fam

    def __enter__(self):
        self.prev = self.plan.family
        self.plan.set_family(self.fam)

    def __exit__(self, *a):
        self.plan.set_family(self.prev)


def _split_module(c, seed):
    g = torch.Generator().manual_seed(seed)
    sp = G.Split2d(c)
    with torch.no_grad():
        sp.conv2d_zeros.weight.copy_(torch.randn(sp.conv2d_zeros.weight.shape, generator=g) * 0.05)
        sp.conv2d_zeros.bias.copy_(torch.randn(sp.conv2d_zeros.bias.shape, generator=g) * 0.3)
        sp.conv2d_zeros.logs.copy_(torch.randn(sp.conv2d_zeros.logs.shape, generator=g) * 0.1)
    return sp.to(DEV).eval(), g


def _split_plan(c, h, w):
    sp, g = _split_module(c, seed=c * 100 + h)
    return sp, sp._plans.get([sp], (c, h, w), torch.device(DEV)), g


# ------------------------------------------------------------------------------------------------ 1. the stream is the oracle's
@pytest.fixture(scope="module")
def any_plan():
    sp, plan, _ = _split_plan(12, 4, 4)
    return sp, plan


@pytest.mark.parametrize("std", [1.0, 0.7])
@pytest.mark.parametrize("seed,call,stream", TRIPLES)
def test_stream_equals_oracle(any_plan, seed, call, stream, std):
    _, plan = any_plan
    big = None
    for n in (1, 3, 4, 5, 4099):
        e = plan.normal_noise((n,), seed, call, stream, std).cpu().numpy()
        ref = SO.normal(n, seed, call, stream, std)
        err = np.abs(e.astype(np.float64) - ref).max()
        print(f"({seed}, {call}, {stream}) std {std} n {n}: max |draw - oracle| {err:.2e} (bar 1e-5)")
        assert e.shape == (n,) and np.isfinite(e).all()
        assert err <= 1e-5
        if big is not None:
            assert np.array_equal(e[:len(big)], big)      # a longer draw begins with the shorter one (scalar tail = vector body)
        big = e


def test_unaligned_and_odd_outputs_match(any_plan):
    """The 16-byte store path and the scalar path write the same elements: a draw into a buffer offset by one float."""
    _, plan = any_plan
    whole = plan.normal_noise((4099,), 1234, 5, 2, 0.7)
    buf = torch.full((4104,), 7.0, device=DEV)
    _lib.check(G.lib().glowhip_normal_noise(buf.data_ptr() + 4, 4099, 1234, 5, 2, 0.7, _lib.stream_ptr(torch.device(DEV))))
    assert torch.equal(buf[1:4100], whole) and buf[0].item() == 7.0 and bool((buf[4100:] == 7.0).all())


def test_moments_on_the_device(any_plan):
    _, plan = any_plan
    worst = SO.check_moments(lambda n, seed, call, stream: plan.normal_noise((n,), seed, call, stream).cpu().numpy())
    print(f"worst: {worst:.2f} standard errors")


# ------------------------------------------------------------------------------------------------ 2. every Split2d route
def _check_route(c, h, w, n, fam, want_route=None, seed=77, call=2 ** 32 + 5, std=0.7):
    """A decode with the sampler bound and no eps == the decode with eps = normal_noise(same position, stream 1, same std):
    same bits, same launches (+ the advance kernel when asked for), and the device word moves by exactly one."""
    sp, plan, g = _split_plan(c, h, w)
    z1 = torch.randn(n, c // 2, h, w, generator=g).to(DEV)
    with family(plan, fam):
        eps = plan.normal_noise((n, c // 2, h, w), seed, call, 1, std)
        plan.decode(z1, [eps])                      # (the first call packs: kept out of the launch counts)
        plan.launch_counts(reset=True)
        x_inj, _ = plan.decode(z1, [eps])
        counts_inj = plan.launch_counts(reset=True)
        pos = plan.sampler_position(seed, call)
        try:
            plan.bind_sampler(pos, [std], advance=False)
            x_drawn, _ = plan.decode(z1, [None])
            counts_drawn = plan.launch_counts(reset=True)
            x_still, _ = plan.decode(z1, [eps])     # bound, but injected: as before
            counts_still = plan.launch_counts(reset=True)
            assert plan.read_position(pos) == (seed, call)
            plan.bind_sampler(pos, [std], advance=True)
            x_adv, _ = plan.decode(z1, [None])
            counts_adv = plan.launch_counts(reset=True)
            assert plan.read_position(pos) == (seed, call + 1)
            x_next, _ = plan.decode(z1, [None])
            assert plan.read_position(pos) == (seed, call + 2)
        finally:
            plan.bind_sampler(None)
        eps_next = plan.normal_noise((n, c // 2, h, w), seed, call + 1, 1, std)
        x_next_inj, _ = plan.decode(z1, [eps_next])
    routes = {k: v for k, v in counts_inj.items() if k.startswith("split_prior(")}
    if want_route is not None:
        assert routes == {f"split_prior({want_route})": 1}, counts_inj
    else:
        assert len(routes) == 1 and next(iter(routes)).startswith("split_prior(k_conv_tail"), counts_inj
    assert counts_drawn == counts_inj and counts_still == counts_inj, (counts_drawn, counts_inj)
    assert counts_adv == {**counts_inj, "k_sampler_advance": 1}, (counts_adv, counts_inj)
    assert torch.isfinite(x_inj).all()
    assert torch.equal(x_drawn, x_inj), f"{routes}: max diff {(x_drawn - x_inj).abs().max().item():.3e}"
    assert torch.equal(x_still, x_inj) and torch.equal(x_adv, x_inj)
    assert torch.equal(x_next, x_next_inj) and not torch.equal(x_next, x_inj)
    assert torch.equal(x_drawn[:, :c // 2], z1)
    with pytest.raises(_lib.GlowHipError):          # unbound again: a missing eps is the error it always was
        plan.decode(z1, [None])


ROUTES = [
    ("k_split_tail", 12, 4, 4),          # maps narrower than the MFMA tail kernels take: direct conv + k_split_tail
    ("k_split_tail", 8, 6, 10),          # width not a multiple of 4
    ("k_split_tail", 6, 3, 5),
    ("k_conv_tail", 12, 32, 32),         # register-staged MFMA tail (fewer than 32 input channels)
    ("k_conv_tail", 24, 16, 16),
    ("k_conv_tail", 48, 8, 8),
    ("k_conv_tail_dma", 64, 16, 16),     # its LDS-DMA twin: 32 / 48 input channels, out-channel tiles split over blockIdx.y
    ("k_conv_tail_dma", 96, 8, 8),
    ("k_conv_tail_dma", 64, 32, 32),
]


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("route,c,h,w", ROUTES)
def test_every_split_route_draws_the_documented_stream(route, c, h, w, fam):
    _check_route(c, h, w, 3, fam, want_route=route)


_TILE_CASES = [(tp, c, h, w, ms) for (c, h, w) in [(12, 32, 32), (24, 16, 16), (48, 8, 8), (64, 16, 16), (96, 8, 8)]
               for tp in (16, 32, 64, 128) for ms in (0x100, 0x200)
               if (h * w) % tp == 0 and tp % w == 0 and not (ms == 0x200 and c > 48)]   # (> 3 out-channel tiles need the split)


@pytest.mark.parametrize("tp,c,h,w,msplit", _TILE_CASES)
def test_draw_on_every_tail_wave_layout(tp, c, h, w, msplit):
    """Each pixel-tile / K-split variant of the two MFMA tail kernels, with and without the out-channel split."""
    with _lib.debug_flags(tp | msplit):
        _check_route(c, h, w, 3, 0)


# ------------------------------------------------------------------------------------------------ 3. the whole model
CLASSES = 5
_MODELS = {}


def _model_case(image=(32, 32), L=3, K=2, hidden=64, batch=4, seed=1):
    """Seeded weights with data-initialised ActNorms of a small Glow: (cfg, state dict); built once per shape, never written."""
    key = (image, L, K, hidden, batch, seed)
    if key not in _MODELS:
        cfg = O.default_cfg(image_shape=(image[0], image[1], 3), hidden_channels=hidden, K=K, L=L, batch=batch)
        sd = O.seeded_state_dict(cfg, seed=seed, zeros_std=0.02, invconv_perturb=0.05)
        g = torch.Generator().manual_seed(seed + 1)
        x = torch.rand(batch, 3, *image, generator=g)
        noise = torch.rand(batch, 3, *image, generator=g) / 256
        with torch.no_grad():
            sd = O.glow_init_actnorm(x, noise, sd, cfg)
        _MODELS[key] = (cfg, sd)
    return _MODELS[key]


def _glow(variant="plain", batch=4, **case):
    """A model on the GPU: 'plain', 'learn_top', 'ycond' (5 classes, learn_top too) or 'lu' (LU-form 1x1 convolutions)."""
    cfg, sd = _model_case(batch=batch, **case)
    ycond, lt, lu = variant == "ycond", variant in ("learn_top", "ycond"), variant == "lu"
    hps = util.AttrDict(dict(
        model=dict(image_shape=cfg["image_shape"], hidden_channels=cfg["hidden_channels"], K=cfg["K"], L=cfg["L"],
                   actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=lt, y_condition=ycond, lu_decomposition=lu, flow_permutation="invconv", flow_coupling="affine"),
        optim=dict(num_batch_train=batch), dataset=dict(num_classes=CLASSES if ycond else 1), device=dict(graph=["cuda:0"])))
    np.random.seed(3)
    glow = G.Glow(hps)
    own = {k: v.clone() for k, v in sd.items()}
    if lu:
        own = util.lu_state_dict_from_dense(own)
    own["h_top"] = torch.zeros_like(glow.h_top)
    if lt:
        head = Y.seeded_head_state(glow.h_top.shape[1] // 2, CLASSES, True)
        own.update({k: v for k, v in head.items() if k in glow.state_dict()})
    glow.load_state_dict(own, strict=True)
    glow.set_actnorm_inited()
    return glow.to(DEV).eval(), cfg, sd


def _labels(n, shift=0):
    return torch.eye(CLASSES)[(torch.arange(n) + shift) % CLASSES].to(DEV)


@pytest.mark.parametrize("variant", ["plain", "learn_top", "ycond", "lu"])
def test_whole_model_sample_is_its_latents_decode(variant):
    glow, cfg, sd = _glow(variant)
    yo = _labels(4) if variant == "ycond" else None
    stds = [0.9, 0.7, 0.5]
    x, lat = glow.sample(y_onehot=yo, return_latents=True, seed=7, call=3, eps_std=stds, safe=False)
    assert x.shape == (4, 3, 32, 32) and bool(torch.isfinite(x).all())
    assert [tuple(e.shape[1:]) for e in lat.eps] == glow.flow.split_shapes((3, 32, 32))
    assert torch.equal(glow.decode_latents(lat, safe=False), x)
    assert torch.equal(glow.sample(y_onehot=yo, seed=7, call=3, eps_std=stds, safe=False), x)      # the same name, the same bits
    other = glow.sample(y_onehot=yo, seed=7, call=4, eps_std=stds, safe=False)
    assert not torch.equal(other, x) and not torch.equal(x[0], x[1])
    assert not torch.equal(glow.sample(y_onehot=yo, seed=8, call=3, eps_std=stds, safe=False), x)
    # the top latent is the documented one: prior + exp(logs) * stream 0 (zeros prior: the stream itself)
    plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))
    draw = plan.normal_noise(lat.z.shape, 7, 3, 0, stds[0])
    mean, logs = glow.prior(yo)
    if mean is None:
        assert torch.equal(lat.z, draw)
    else:
        want = mean.double() + torch.exp(logs.double()) * draw.double()
        assert (lat.z.double() - want).abs().max().item() <= 1e-5
        if variant == "ycond":
            assert not torch.equal(glow.sample(y_onehot=_labels(4, 1), seed=7, call=3, eps_std=stds, safe=False), x)
    # against the CPU oracle: the decode bar of the project, 1e-4 max-abs
    with torch.no_grad():
        x_ref = O.glow_reverse(lat.z.cpu(), sd, cfg, [e.cpu() for e in lat.eps])
    err = (x.cpu().double() - x_ref.double()).abs().max().item()
    print(f"{variant}: sample vs oracle decode of its latents {err:.2e} (bar 1e-4)")
    assert err <= 1e-4


def test_implicit_position_advances_by_one_per_call():
    glow, _, _ = _glow("plain")
    torch.manual_seed(1234)
    gmodel.reset_sampler_stream()
    key, c0 = gmodel.sampler_position()
    assert (key, c0) == (1234, 0)
    a, b, c = (glow.sample(safe=False) for _ in range(3))
    assert gmodel.sampler_position() == (key, 3)
    for r, img in enumerate((a, b, c)):
        assert torch.equal(img, glow.sample(seed=key, call=r, safe=False)), r      # explicit positions do not move the stream
    assert gmodel.sampler_position() == (key, 3)
    assert torch.equal(glow.sample(safe=True), glow.sample(seed=key, call=3, safe=False))       # in range: the check changes nothing
    assert gmodel.sampler_position() == (key, 4)
    assert glow.sample(n=2, safe=False).shape == (2, 3, 32, 32)


def test_dense_prior_base_and_given_top_latent():
    """FlowPlan.sample with a dense (mean, logs) base: z = mean + exp(logs) * stream 0; with z given: the decode of that z."""
    glow, _, _ = _glow("plain")
    plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))
    plan.ensure_packed(use=plan.PACK_INFERENCE | plan.PACK_INVERSE)
    g = torch.Generator().manual_seed(3)
    mean = (torch.randn((4,) + plan.out_chw, generator=g) * 0.3).to(DEV)
    logs = (torch.randn((4,) + plan.out_chw, generator=g) * 0.2).to(DEV)
    plan.bind_sampler(plan.sampler_position(5, 9), [1.0, 1.0], advance=False)
    try:
        x, _, z = plan.sample(4, 0.8, prior=(mean, logs))
        x2, _, z2 = plan.sample(4, z=z)
    finally:
        plan.bind_sampler(None)
    want = mean.double() + torch.exp(logs.double()) * plan.normal_noise(z.shape, 5, 9, 0, 0.8).double()
    assert (z.double() - want).abs().max().item() <= 1e-5
    assert torch.equal(x2, x) and torch.equal(z2, z)


# ------------------------------------------------------------------------------------------------ 4. mixed injection
def test_mixed_injection_and_resample_details():
    glow, _, _ = _glow("plain")
    plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))
    plan.ensure_packed(use=plan.PACK_INFERENCE | plan.PACK_INVERSE)
    g = torch.Generator().manual_seed(5)
    z = torch.randn((4,) + plan.out_chw, generator=g).to(DEV)
    e0 = (torch.randn((4,) + plan.split_chw[0], generator=g) * 0.7).to(DEV)
    plan.bind_sampler(plan.sampler_position(21, 6), [0.7, 0.6], advance=False)
    try:
        mixed, _ = plan.decode(z, [e0, None])
    finally:
        plan.bind_sampler(None)
    want, _ = plan.decode(z, [e0, plan.normal_noise((4,) + plan.split_chw[1], 21, 6, 2, 0.6)])
    assert torch.equal(mixed, want)

    inf = Inferer(glow.hps, glow, [DEV], DEV)
    img = torch.rand(4, 3, 32, 32, generator=g).to(DEV)
    rec = inf.reconstruct(img)
    assert torch.equal(inf.resample_details(img, levels=0), rec)
    a = inf.resample_details(img, levels=1, seed=3, call=0)
    b = inf.resample_details(img, levels=1, seed=3, call=1)
    assert a.shape == rec.shape and bool(torch.isfinite(a).all()) and not torch.equal(a, b) and not torch.equal(a, rec)
    assert torch.equal(a, inf.resample_details(img, levels=1, seed=3, call=0))
    lat = inf.encode_full(img)
    want = glow.decode_latents(Latents(lat.z, [lat.eps[0], plan.normal_noise(lat.eps[1].shape, 3, 0, 2, 1.0)]), safe=False)
    assert torch.equal(a, want)


# ------------------------------------------------------------------------------------------------ 5. 8-bit output
def _as_u8(x):
    return (x.clamp(0, 1) * 255).to(torch.uint8)


@pytest.mark.parametrize("image,L", [((32, 32), 3), ((24, 40), 2), ((12, 20), 2), ((6, 10), 1)])
def test_uint8_output_is_the_clamped_fp32_sample(image, L):
    """(6, 10): the un-squeezed width is odd (5), the one-thread-per-pixel instance; the others take the register transpose."""
    glow, _, _ = _glow("plain", image=image, L=L)
    with torch.no_grad():      # biases that push pixels out of [0, 1] on both sides: the first ActNorm's inverse ends the decode
        b = glow.flow.layers[1].actnorm.bias
        b.copy_(b + torch.linspace(-0.6, 0.6, b.numel(), device=b.device).view_as(b))
    x = glow.sample(seed=11, call=2, safe=False)
    u = glow.sample(seed=11, call=2, uint8=True, safe=False)
    assert u.dtype == torch.uint8 and u.shape == x.shape
    assert x.min().item() < 0.0 and x.max().item() > 1.0
    assert torch.equal(u, _as_u8(x))
    assert 0 < int((u == 0).sum()) and 0 < int((u == 255).sum())
    plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))
    counts = plan.launch_counts(reset=True)
    assert counts.get("unsqueeze(u8)", 0) >= 1
    us, lat = glow.sample(seed=11, call=2, uint8=True, return_latents=True, safe=True)      # both outputs from one call
    assert torch.equal(us, u) and torch.equal(_as_u8(glow.decode_latents(lat, safe=False)), u)


@pytest.mark.parametrize("h,w", [(8, 8), (6, 10)], ids=["transpose", "per-pixel"])
def test_uint8_rule_on_special_values(h, w):
    """Truncation, saturation, NaN -> 0: hand-made pixels through a plan that is one Squeeze2d, so the byte-storing un-squeeze is
    the whole call.  (6, 10): the squeezed width is odd, the one-thread-per-pixel instance."""
    sq = G.Squeeze2d()
    plan = sq_plan = G.FlowPlan([sq], (3, h, w), torch.device(DEV))
    g = torch.Generator().manual_seed(h)
    img = torch.rand(2, 3, h, w, generator=g) * 1.6 - 0.3
    special = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 0.0, 0.999 / 255, 1.5 / 255, 254.9 / 255, 1.0, 3e38,
                            -3e38, 1e-45, 0.5])
    img.view(-1)[:special.numel()] = special
    img.view(-1)[-special.numel():] = special.flip(0)
    img = img.to(DEV)
    z = G.Squeeze2d.squeeze(img)
    x, u, _ = sq_plan.sample(2, z=z, want_x=True, want_u8=True)
    only_u = plan.sample(2, z=z, want_x=False, want_u8=True)[1]
    assert torch.equal(x.view(torch.int32), img.view(torch.int32))
    want = torch.nan_to_num(img, nan=0.0, posinf=2.0, neginf=-1.0).clamp(0, 1).mul(255).to(torch.uint8)
    assert torch.equal(u, want) and torch.equal(only_u, want)
    assert u.view(-1)[:special.numel()].tolist() == [0, 255, 0, 0, 0, 0, 1, 254, 255, 255, 0, 0, 127]


def test_uint8_needs_a_leading_squeeze():
    sp, plan, g = _split_plan(12, 4, 4)
    z1 = torch.randn(2, 6, 4, 4, generator=g).to(DEV)
    plan.ensure_packed(use=plan.PACK_INFERENCE | plan.PACK_INVERSE)
    plan.bind_sampler(plan.sampler_position(1, 0), [1.0], advance=False)
    try:
        x, _, _ = plan.sample(2, z=z1)                      # fp32 out of a plan without a squeeze: fine
        assert torch.equal(x, plan.decode(z1, [None])[0])
        with pytest.raises(_lib.GlowHipError, match="Squeeze2d"):
            plan.sample(2, z=z1, want_x=False, want_u8=True)
    finally:
        plan.bind_sampler(None)


# ------------------------------------------------------------------------------------------------ 6. the captured sampler
@pytest.mark.parametrize("variant", ["plain", "ycond"])
@pytest.mark.parametrize("uint8", [False, True], ids=["fp32", "uint8"])
def test_captured_sampler_replays_the_eager_positions(variant, uint8):
    glow, _, _ = _glow(variant)
    yo = _labels(4) if variant == "ycond" else None
    s, c = 77, 2 ** 32 - 2                                  # the replays cross a 32-bit boundary of the call number
    gs = glow.capture_sampler(4, y_onehot=yo, eps_std=0.8, uint8=uint8, seed=s, call=c)
    assert gs.last_position is None
    for r in range(3):
        out = gs().clone()
        assert gs.last_position == (s, c + r)
        assert torch.equal(out, glow.sample(y_onehot=yo, eps_std=0.8, uint8=uint8, seed=s, call=c + r, safe=False)), r
    assert gs.plan.read_position(gs.pos) == (s, c + 3)
    if variant == "ycond":
        other = _labels(4, 2)
        gs.y_onehot.copy_(other)
        out = gs().clone()
        assert torch.equal(out, glow.sample(y_onehot=other, eps_std=0.8, uint8=uint8, seed=s, call=c + 3, safe=False))
        assert not torch.equal(out, glow.sample(y_onehot=yo, eps_std=0.8, uint8=uint8, seed=s, call=c + 3, safe=False))
    glow.load_state_dict({k: v.clone() for k, v in glow.state_dict().items()})
    with pytest.raises(_lib.GlowHipError, match="capture again"):
        gs()


def test_captured_sampler_refuses_a_replay_over_a_reallocated_workspace():
    """A plan serves every batch size of its image shape from ONE inference workspace, re-allocated when a larger batch comes
    (`FlowPlan._workspace`): the captured launches hold the old address.  A replay after such an eager call is refused -- with an
    error, the stale graph is never launched -- and a new capture replays the eager sample of its position."""
    glow, _, _ = _glow("plain", image=(16, 16), L=2, K=1)
    gs = glow.capture_sampler(2, eps_std=0.8, seed=21, call=4)
    plan = gs.plan
    assert torch.equal(gs(), glow.sample(2, eps_std=0.8, seed=21, call=4, safe=False))      # (an eager call of the SAME batch moves nothing)
    assert torch.equal(gs(), glow.sample(2, eps_std=0.8, seed=21, call=5, safe=False))
    before = (plan._ws.data_ptr(), plan._ws.numel())
    big = glow.sample(64, eps_std=0.8, seed=21, call=6, safe=False)
    assert bool(torch.isfinite(big).all())
    assert plan._ws.numel() > before[1] and (plan._ws.data_ptr(), plan._ws.numel()) != before, "the larger batch did not re-allocate"
    with pytest.raises(_lib.GlowHipError, match="capture again") as err:
        gs()
    assert "workspace" in str(err.value) and gs.last_position == (21, 5)
    gs2 = glow.capture_sampler(2, eps_std=0.8, seed=21, call=7)
    assert torch.equal(gs2(), glow.sample(2, eps_std=0.8, seed=21, call=7, safe=False))


# ------------------------------------------------------------------------------------------------ 7. range
def test_out_of_range_sample_is_flagged_or_rerun_exactly():
    cfg = O.default_cfg(image_shape=(16, 16, 3), hidden_channels=64, K=1, L=2, batch=4)
    sd = O.seeded_state_dict(cfg, seed=3, zeros_std=0.02)
    sd["flow.layers.1.f.0.weight"] = sd["flow.layers.1.f.0.weight"] * 3e5      # hidden activations ~1e5: beyond the fp16 pairs
    sd["flow.layers.1.f.2.weight"] = sd["flow.layers.1.f.2.weight"] / 3e5      # keep h2 modest
    _MODELS[((16, 16), 2, 1, 64, 4, "range")] = (cfg, sd)
    glow, _, _ = _glow("plain", image=(16, 16), L=2, K=1, seed="range")
    plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))
    raw = glow.sample(seed=5, call=1, safe=False)
    assert bool((plan.status(4, raw) != 0).any()), "this model is meant to overflow the split-half range"
    n0 = G.FlowModel._RANGE_FALLBACKS
    torch.manual_seed(5)
    gmodel.reset_sampler_stream()
    safe = glow.sample(safe=True)                            # implicit position (5, 0)
    assert G.FlowModel._RANGE_FALLBACKS == n0 + 1 and plan.family == plan.FAMILY_AUTO
    assert gmodel.sampler_position() == (5, 1), "the re-run must not advance a second time"
    assert bool(torch.isfinite(safe).all())
    prev = plan.family
    plan.set_family(plan.FAMILY_EXACT_FP32)
    try:
        exact = glow.sample(seed=5, call=0, safe=False)
    finally:
        plan.set_family(prev)
    assert torch.equal(safe, exact)
    nxt = glow.sample(safe=True)                             # the device word is where the host believes it is: (5, 1)
    plan.set_family(plan.FAMILY_EXACT_FP32)
    try:
        assert torch.equal(nxt, glow.sample(seed=5, call=1, safe=False))
    finally:
        plan.set_family(prev)


def test_captured_sampler_on_deep_levels_survives_eager_calls():
    """Levels the deep-level kernels take (dnet_sh.hip) zero their padded operands at the start of every call.  As memset nodes
    of a captured graph those stopped zeroing once an eager decode of the same plan had run in between -- every later replay
    returned NaN (seen at 128x128 L 5 and 256x256 L 6, hidden 512) -- so the level now zeroes them with a kernel of its own.
    Replays before and after eager samples and an eager decode equal the eager sample of their position."""
    cfg = O.default_cfg(image_shape=(128, 128, 3), hidden_channels=512, K=1, L=5, batch=16)
    sd = O.seeded_state_dict(cfg, seed=2, zeros_std=0.02, invconv_perturb=0.05)
    _MODELS[((128, 128), 5, 1, 512, 16, "deep")] = (cfg, sd)      # (ActNorms at zero bias / logs: no init pass needed here)
    glow, _, _ = _glow("plain", image=(128, 128), L=5, K=1, hidden=512, batch=16, seed="deep")
    plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))
    assert "dnet-sh2" in plan.describe(16), plan.describe(16)
    gs = glow.capture_sampler(16, eps_std=0.7, seed=9, call=0)
    want = [glow.sample(16, eps_std=0.7, seed=9, call=c, safe=False) for c in range(4)]      # eager calls after the capture
    assert bool(torch.isfinite(want[0]).all())
    assert torch.equal(gs(), want[0])
    glow.reverse_flow(None, eps_std=0.7, safe=False)                                         # the torch-drawn route, eagerly
    assert torch.equal(gs(), want[1])
    glow.sample(16, eps_std=0.7, safe=False)
    assert torch.equal(gs(), want[2]) and torch.equal(gs(), want[3])

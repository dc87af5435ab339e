"""GPU tests of the per-level terms and of `network.Evaluator` (-m gpu), against tests/evaluate_oracle.py (an fp64 walk of the
oracle's layers).

Bounds.  A level term is held to the project's nll bound, 1e-4 bits/dim, after scaling by 1 / (ln2 D).  The sum of the
terms: (n_levels + 1) fp32 ulps of |objective| -- the terms are exact integer parts, each rounded once.  Evaluator figures
(bits_per_dim, level_bits): 1e-4 bits/dim."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import training  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from pytorch_glow_amd.network import Builder, Evaluator, Trainer  # noqa: E402
from pytorch_glow_amd.network import evaluate as EV  # noqa: E402
from pytorch_glow_amd.network import model as gmodel  # noqa: E402
from pytorch_glow_amd.network.trainer import _ScalarLog  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402

import evaluate_oracle as EO  # noqa: E402

DEV = "cuda:0"
LN2 = EO.LN2
BOUND = 1e-4


def make_glow(cfg, sd, batch, **ablation):
    ab = dict(learn_top=False, y_condition=False, lu_decomposition=False, flow_permutation=cfg["flow_permutation"],
              flow_coupling=cfg["flow_coupling"])
    ab.update(ablation)
    hps = util.AttrDict(dict(
        model=dict(image_shape=cfg["image_shape"], hidden_channels=cfg["hidden_channels"], K=cfg["K"], L=cfg["L"],
                   actnorm_scale=cfg["actnorm_scale"], n_bits_x=cfg["n_bits_x"], weight_y=0.0),
        ablation=ab, optim=dict(num_batch_train=batch), dataset=dict(num_classes=1), device=dict(graph=["cuda:0"])))
    glow = G.Glow(hps)
    sd = {k: v.clone() for k, v in sd.items()}
    sd["h_top"] = torch.zeros_like(glow.h_top)
    glow.load_state_dict(sd, strict=not ablation)      # (a head the state dict does not know keeps its construction values)
    glow.set_actnorm_inited()
    return glow.to(DEV).eval()


def seeded(image, hidden, K, L, batch, coup="affine", seed=5):
    cfg = O.default_cfg(image_shape=(image, image, 3), hidden_channels=hidden, K=K, L=L, flow_coupling=coup, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=seed, zeros_std=0.02, invconv_perturb=0.05)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(batch, 3, image, image, generator=g)
    noise = torch.rand(batch, 3, image, image, generator=g) / 256
    with torch.no_grad():
        sd = O.glow_init_actnorm(x, noise, sd, cfg)
    return cfg, sd, x, noise


def forward_with_terms(glow, x, noise, y_onehot=None):
    """(z, nll, objective, terms, launch counts) of one inference forward with the level terms bound."""
    x = x.to(DEV)
    plan = glow.flow.plan_for(x)
    head = plan.head_call(x.shape[0], None if y_onehot is None else y_onehot.to(DEV)) if glow._attach_head(plan) else None
    terms = plan.level_terms_buffer(x.shape[0])
    plan.set_dequant_rng(0, False)
    plan.ensure_packed()
    plan.launch_counts(reset=True)
    z, nll, obj = plan.glow_forward(x, None if noise is None else noise.to(DEV), None, None, 0, glow.hps.model.n_bits_x, head=head,
                                    level_terms=terms)
    return z, nll, obj, terms, plan.launch_counts(reset=True), (plan, head)


def check_terms(what, terms, obj, ref_terms, offset, dims):
    """Each level against the oracle at 1e-4 bits/dim; the sum of the parts against the objective at (n_levels + 1) ulps."""
    t = terms.cpu().double()
    assert t.shape == ref_terms.shape, (t.shape, ref_terms.shape)
    err = ((t - ref_terms).abs() / (LN2 * dims)).max(dim=1).values
    print(f"{what}: level terms err (bits/dim) {[f'{e:.2e}' for e in err.tolist()]} (bound {BOUND:.0e}); "
          f"level bits {[f'{v:.4f}' for v in (-ref_terms.mean(dim=1) / (LN2 * dims)).tolist()]}")
    assert (err <= BOUND).all(), what
    o = obj.cpu()
    gap = (t.sum(dim=0) + offset - o.double()).abs()
    ulp = torch.from_numpy(np.spacing(np.abs(o.numpy()))).double()
    print(f"{what}: |sum of terms + offset - objective| {gap.max().item():.3e} nats = {(gap / ulp).max().item():.2f} ulps "
          f"(bound {t.shape[0] + 1})")
    assert (gap <= (t.shape[0] + 1) * ulp).all(), what


# ------------------------------------------------------------------------------------------------ 1. level terms against the oracle
@pytest.mark.parametrize("coup", ["additive", "affine"])
def test_level_terms_against_the_oracle(coup):
    cfg, sd, x, noise = seeded(32, 64, 2, 3, 3, coup=coup)      # levels 1 and 2 on k_cnet, level 3 on the per-layer kernels
    glow = make_glow(cfg, sd, 3)
    z, nll, obj, terms, counts, _ = forward_with_terms(glow, x, noise)
    ref, offset, obj_ref = EO.level_terms(x, noise, sd, cfg)
    check_terms(coup, terms, obj, ref, offset, x[0].numel())
    assert any(k.startswith("variant:k_cnet") for k in counts), counts
    assert counts["k_level_snapshot"] == 3 and counts["k_level_terms"] == 1


def test_level_terms_of_an_lu_model():
    import plu_oracle as PLU
    import test_gpu_lu_param_model as M
    sd, x, noise = M.lu_state_dict()
    glow = M.lu_glow()
    z, nll, obj, terms, _, _ = forward_with_terms(glow, x, noise)
    ref, offset, _ = EO.level_terms(x, noise, PLU.dense_state_dict(sd), M.CFG)
    check_terms("lu", terms, obj, ref, offset, x[0].numel())


@pytest.mark.parametrize("lt", [0, 1])
def test_level_terms_with_a_learned_and_class_conditional_head(lt):
    import test_gpu_ycond as TY
    import ycond_oracle as Y
    from conftest import load_golden
    g = load_golden("g10_glow_tiny_ycond")
    glow = TY.build(g, lt)
    yo = g["y_onehot_ce"]
    z, nll, obj, terms, counts, _ = forward_with_terms(glow, g["x"], g["noise"], yo)
    cfg = dict(Y.TINY, learn_top=bool(lt), y_condition=True)
    ref, offset, _ = EO.level_terms(g["x"], g["noise"], Y.case_state(g, lt), cfg, y_onehot=yo)
    check_terms(f"y_condition lt{lt}", terms, obj, ref, offset, g["x"][0].numel())
    assert terms.shape[0] == 2


def test_level_terms_with_learn_top_alone():
    cfg, sd, x, noise = seeded(16, 32, 1, 2, 2)
    glow = make_glow(cfg, sd, 2, learn_top=True)
    gen = torch.Generator().manual_seed(8)
    with torch.no_grad():      # Conv2dZeros initialises to zero, which would hide the head
        glow.learn_top.bias.copy_(torch.randn(glow.learn_top.bias.shape, generator=gen) * 0.1)
        glow.learn_top.logs.copy_(torch.randn(glow.learn_top.logs.shape, generator=gen) * 0.05)
    sd2 = {k: v.detach().cpu() for k, v in glow.state_dict().items()}
    z, nll, obj, terms, _, _ = forward_with_terms(glow, x, noise)
    ref, offset, _ = EO.level_terms(x, noise, sd2, dict(cfg, learn_top=True))
    check_terms("learn_top", terms, obj, ref, offset, x[0].numel())


def test_level_terms_from_8_bit_pixels():
    cfg, sd, x, noise = seeded(16, 32, 2, 3, 3)
    glow = make_glow(cfg, sd, 3)
    x8 = (x * 255).to(torch.uint8)
    z, nll, obj, terms, counts, _ = forward_with_terms(glow, x8, noise)
    ref, offset, _ = EO.level_terms(x8.double() / 255.0, noise, sd, cfg)
    check_terms("uint8", terms, obj, ref, offset, x[0].numel())


def test_level_terms_on_every_executor():
    """128 x 128, hidden 64, K = 1, L = 6 at batch 2 (the geometry of tests/test_gpu_train_deep.py): levels 1 and 2 run k_cnet, level
    3 the per-layer exact-fp32 kernels, levels 4 to 6 the deep-level kernels."""
    cfg, sd, x, noise = seeded(128, 64, 1, 6, 2, seed=3)
    glow = make_glow(cfg, sd, 2)
    z, nll, obj, terms, counts, (plan, _) = forward_with_terms(glow, x, noise)
    desc = plan.describe(2)
    assert "cnet-sh2" in desc and "dnet-sh2" in desc and "f0=" in desc, desc
    assert any(k.startswith("variant:k_cnet") for k in counts) and counts.get("k_dn_fin", 0) >= 1 and counts.get("k_gemm_f32", 0) >= 1, counts
    ref, offset, _ = EO.level_terms(x, noise, sd, cfg)
    check_terms("every executor", terms, obj, ref, offset, x[0].numel())
    assert counts["k_level_snapshot"] == 6


# ------------------------------------------------------------------------------------------------ 2. nothing existing changes
def test_binding_changes_no_result_and_adds_exactly_its_own_launches():
    cfg, sd, x, noise = seeded(16, 32, 2, 3, 3)
    glow = make_glow(cfg, sd, 3)
    xd, nd = x.to(DEV), noise.to(DEV)
    plan = glow.flow.plan_for(xd)
    plan.ensure_packed()
    plan.launch_counts(reset=True)
    z0, nll0, obj0 = plan.glow_forward(xd, nd, None, None, 0, 8)
    off = plan.launch_counts(reset=True)
    z1, nll1, obj1, terms, on, _ = forward_with_terms(glow, x, noise)
    assert torch.equal(z0, z1) and torch.equal(nll0, nll1) and torch.equal(obj0, obj1)
    assert "k_level_snapshot" not in off and "k_level_terms" not in off
    extra = {k: v - off.get(k, 0) for k, v in on.items() if v != off.get(k, 0)}
    assert extra == {"k_level_snapshot": plan.n_levels, "k_level_terms": 1}, extra
    assert sum(on.values()) - sum(off.values()) == plan.n_levels + 1
    # unbound again: the launch list of the call without the feature, the same bits; encode ignores a binding altogether
    z2, nll2, obj2 = plan.glow_forward(xd, nd, None, None, 0, 8)
    assert plan.launch_counts(reset=True) == off and torch.equal(nll2, nll0) and torch.equal(z2, z0)
    plan._bind_level_terms(terms, 3)
    try:
        terms.fill_(-1.0)
        plan.encode(xd, noise=nd)
        enc = plan.launch_counts(reset=True)
    finally:
        plan._unbind_level_terms()
    assert "k_level_snapshot" not in enc and "k_level_terms" not in enc and bool((terms == -1.0).all())
    # a scratch too small for the batch is refused by the forward, not overrun
    small = torch.empty(64, dtype=torch.uint8, device=DEV)
    G._lib.check(G.lib().glowhip_plan_bind_level_terms(plan._h, G._lib.ptr(terms), G._lib.ptr(small), small.numel()))
    try:
        with pytest.raises(G.GlowHipError, match="level scratch too small"):
            plan.glow_forward(xd, nd, None, None, 0, 8)
    finally:
        plan._unbind_level_terms()


# ------------------------------------------------------------------------------------------------ 3. a flagged sample
BIG, SCALE = 5.0, 357.0


def ranged_model():
    """32 x 32, hidden 64, K = 1, L = 3 (levels 1 and 2 run k_cnet) with data-initialised ActNorms, the f.0 ActNorm scale of the
    SECOND level's FlowStep multiplied by SCALE and f.2's divided by it (h2 stays modest) -- the weight scaling of
    tests/test_gpu_fused.py::_range_case -- and 11 images of which number 6 is BIG times brighter.  On the CPU oracle the largest
    |h1| of that step is 4.71 * SCALE = 1 680 for the other ten images and 27.9 * SCALE = 9 960 for image 6: a factor 2.4 inside
    and outside the fp16 pairs' range |v| < 4094 (include/glowhip.h, GLOWHIP_FAMILY_AUTO).  The reference handles image 6: its
    nll is 207 bits/dim."""
    cfg, sd, x, noise = seeded(32, 64, 1, 3, 11, seed=9)
    sd = dict(sd)
    sd["flow.layers.4.f.0.actnorm.logs"] = sd["flow.layers.4.f.0.actnorm.logs"] + float(np.log(SCALE)) / 3.0
    sd["flow.layers.4.f.2.actnorm.logs"] = sd["flow.layers.4.f.2.actnorm.logs"] - float(np.log(SCALE)) / 3.0
    xb = x.clone()
    xb[6] *= BIG
    return cfg, sd, x, xb, noise


def test_a_flagged_sample_has_nan_from_its_level_on_and_nobody_else_is_touched():
    cfg, sd, x, xb, noise = ranged_model()
    x, xb, noise = x[4:8], xb[4:8], noise[4:8]      # image 6 is sample 2 of this batch
    glow = make_glow(cfg, sd, 4)
    ref, offset, obj_ref = EO.level_terms(xb, noise, sd, cfg)
    assert torch.isfinite(ref).all()      # the reference handles this input
    _, nll_ok, _, terms_ok, counts, _ = forward_with_terms(glow, x, noise)
    assert any(k.startswith("variant:k_cnet") for k in counts), counts
    assert torch.isfinite(nll_ok).all() and torch.isfinite(terms_ok).all()
    _, nll, obj, terms, _, _ = forward_with_terms(glow, xb, noise)
    t = terms.cpu()
    print("terms of the flagged sample:", t[:, 2].tolist(), "oracle:", ref[:, 2].tolist())
    assert not torch.isfinite(nll[2]) and torch.isfinite(nll[[0, 1, 3]]).all()
    assert torch.isfinite(t[0, 2]) and torch.isnan(t[1:, 2]).all(), t[:, 2]
    assert abs(float(t[0, 2]) - float(ref[0, 2])) / (LN2 * x[0].numel()) <= BOUND
    others = [0, 1, 3]
    assert torch.equal(t[:, others], terms_ok.cpu()[:, others])
    err = ((t[:, others].double() - ref[:, others]).abs() / (LN2 * x[0].numel())).max().item()
    assert err <= BOUND, err


# ------------------------------------------------------------------------------------------------ 4. the evaluator
_EVAL = {}


def eval_case():
    """The model, 11 images as batches of 4, 4 and 3, and -- per draw count -- the oracle's figures under the named draws."""
    if not _EVAL:
        cfg, sd, x, _ = seeded(32, 64, 2, 3, 11, seed=7)
        _EVAL.update(cfg=cfg, sd=sd, batches=[x[0:4], x[4:8], x[8:11]])
    return _EVAL


def oracle_figures(draws, seed=0, order=(0, 1, 2)):
    """Per-image (bpd, bpd_single, level bits [n_levels, 11]) of the oracle for the batches evaluated in `order`: batch number b
    of the run draws with call b * draws + k, whichever images it holds."""
    c = eval_case()
    key = ("ref", draws, seed, tuple(order))
    if key not in c:
        glow = make_glow(c["cfg"], c["sd"], 4)
        plan = glow.flow.plan_for(c["batches"][0].to(DEV))
        dims = c["batches"][0][0].numel()
        bpd, single, lev = [], [], []
        for b, i in enumerate(order):
            xb = c["batches"][i]
            objs, terms = [], []
            for k in range(draws):
                noise = plan.dequant_noise(xb.shape, EV.stream_seed(seed), b * draws + k, 8).cpu()
                t, offset, o = EO.level_terms(xb, noise, c["sd"], c["cfg"])
                objs.append(o.numpy()); terms.append(t.numpy())
            pb, ps = EO.per_image(np.stack(objs), dims)
            bpd.append(pb); single.append(ps); lev.append(EO.level_bits(np.stack(terms), dims))
        c[key] = (np.concatenate(bpd), np.concatenate(single), np.concatenate(lev, axis=1))
    return c[key]


@pytest.mark.parametrize("draws", [1, 3])
def test_evaluator_against_the_oracle(draws):
    c = eval_case()
    glow = make_glow(c["cfg"], c["sd"], 4)
    bpd, single, lev = oracle_figures(draws)
    torch.manual_seed(21)
    gmodel.dequant_position(advance=True)
    position = gmodel.dequant_position()
    ev = Evaluator(glow, draws=draws, levels=True, seed=0, hist=(32, 0.0, 16.0))
    res = ev.run(c["batches"])
    assert gmodel.dequant_position() == position
    print(f"draws={draws}: {res!r} oracle bpd {bpd.mean():.6f} single {single.mean():.6f}; level bits {res.level_bits} "
          f"oracle {lev.mean(axis=1).tolist()}")
    assert res.count == 11 and res.flagged == 0 and tuple(res.per_image.shape) == (11,)
    assert abs(res.bits_per_dim - bpd.mean()) <= BOUND and abs(res.bits_per_dim_single - single.mean()) <= BOUND
    assert np.abs(np.array(res.level_bits) - lev.mean(axis=1)).max() <= BOUND
    assert np.abs(res.per_image.cpu().numpy() - bpd).max() <= BOUND
    assert res.bits_per_dim <= res.bits_per_dim_single + 1e-9      # Jensen
    assert abs(8 + sum(res.level_bits) - res.bits_per_dim_single) <= 1e-5      # the levels decompose the draw-averaged figure
    assert abs(res.min - bpd.min()) <= BOUND and abs(res.max - bpd.max()) <= BOUND
    assert sum(res.histogram["counts"]) + res.histogram["under"] + res.histogram["over"] == 11
    assert res.min <= res.quantile(0.5) + 0.5 and res.quantile(0.5) <= res.max + 0.5      # (half a bit: the bin width)
    want_se = bpd.std(ddof=1) / np.sqrt(11)
    assert abs(res.std_error - want_se) <= 1e-4
    # the same (seed, data) gives the same bits again; Glow.evaluate is the thin form
    again = glow.evaluate(c["batches"], draws=draws, hist=(32, 0.0, 16.0))
    assert again.state_bytes() == res.state_bytes() and torch.equal(again.per_image, res.per_image)
    # A loader that yields the batches in another order: the draw numbering follows the batch order, so every image meets other
    # noise and the sums move (not compared).  The count is the same; the histogram is the same at the 1-bit bins chosen here; min and
    # max are those of the oracle under THAT order's draws, at the bound -- and so within the oracle's own order-to-order
    # difference of the first run's.
    order = (2, 0, 1)
    ev1 = Evaluator(glow, draws=draws, levels=True, seed=0, hist=(16, 0.0, 16.0))
    first = ev1.run(c["batches"])
    other = ev1.run([c["batches"][i] for i in order])
    bpd_o, _, _ = oracle_figures(draws, order=order)
    assert other.count == first.count == 11 and other.flagged == 0
    assert other.histogram == first.histogram
    assert abs(other.min - bpd_o.min()) <= BOUND and abs(other.max - bpd_o.max()) <= BOUND
    assert abs(other.min - first.min) <= abs(bpd_o.min() - bpd.min()) + 2 * BOUND
    assert abs(other.max - first.max) <= abs(bpd_o.max() - bpd.max()) + 2 * BOUND


def test_another_batch_order_with_the_draws_pinned_gives_the_same_histogram():
    """Draw numbering follows batch order, so a loader in another order draws other noise; with the evaluator's fold alone (the
    objectives of the first order, folded in another order) count, histogram, min and max -- and the sums -- are the same bits."""
    c = eval_case()
    glow = make_glow(c["cfg"], c["sd"], 4)
    ev = Evaluator(glow, draws=2, levels=True, seed=3)
    key = EV.stream_seed(3)
    outs = []
    with torch.no_grad():
        for b, xb in enumerate(c["batches"]):
            obj, terms, _ = ev._forward_draws(xb.to(DEV), None, b, key)
            outs.append((obj, terms))
    states = []
    for order in ((0, 1, 2), (2, 0, 1)):
        st = EV.EvalState(DEV, 3, (32, 0.0, 16.0))
        per = torch.empty(11, dtype=torch.float32, device=DEV)
        offs = {0: 0, 1: 4, 2: 8}
        for b in order:
            st.fold(outs[b][0], outs[b][1], 3 * 32 * 32, per, offs[b])
        states.append((bytes(st.read()), per.clone()))
    assert states[0][0] == states[1][0] and torch.equal(states[0][1], states[1][1])


def test_safe_rerun_rescues_a_batch_out_of_range():
    cfg, sd, _, xb, _ = ranged_model()
    batches = [xb[0:4], xb[4:8], xb[8:11]]      # image 6 (second batch) leaves the fp16 pairs' range at level 2
    glow = make_glow(cfg, sd, 4)
    plan = glow.flow.plan_for(batches[0].to(DEV))
    # the reference: everything on the exact-fp32 family, the same draws
    plan.set_family(plan.FAMILY_EXACT_FP32)
    try:
        exact = Evaluator(glow, draws=2, seed=4, safe=False).run(batches)
    finally:
        plan.set_family(plan.FAMILY_AUTO)
    assert exact.flagged == 0 and exact.count == 11
    unsafe = Evaluator(glow, draws=2, seed=4, safe=False).run(batches)
    assert unsafe.flagged == 1 and unsafe.count == 10
    per = unsafe.per_image.cpu().numpy()
    assert np.isnan(per[6]) and np.isfinite(np.delete(per, 6)).all()
    assert EV._s128(unsafe.state.sum_bpd) == EO.fixed_total(np.delete(per, 6).astype(np.float64))      # the sums exclude exactly that image
    n0 = G.Glow._RANGE_FALLBACKS
    safe = Evaluator(glow, draws=2, seed=4, safe=True).run(batches)
    assert G.Glow._RANGE_FALLBACKS == n0 + 1      # one batch ran again, not three
    assert plan.family == plan.FAMILY_AUTO
    assert safe.flagged == 0 and safe.count == 11
    print(f"safe {safe!r}\nexact {exact!r}")
    assert abs(safe.bits_per_dim - exact.bits_per_dim) <= BOUND and abs(safe.bits_per_dim_single - exact.bits_per_dim_single) <= BOUND
    assert np.abs(np.array(safe.level_bits) - np.array(exact.level_bits)).max() <= BOUND
    sp, ep = safe.per_image.cpu().numpy(), exact.per_image.cpu().numpy()
    assert np.abs(sp - ep).max() <= BOUND * max(1.0, np.abs(ep).max())
    assert np.array_equal(np.delete(sp, 6), np.delete(per, 6))      # nobody else was folded twice
    with pytest.raises(AssertionError, match="one-shot iterator"):
        Evaluator(glow, draws=2, seed=4, safe=True).run(iter(batches))


# ------------------------------------------------------------------------------------------------ 5. Trainer
def test_trainer_evaluates_the_held_out_batches_under_the_average(tmp_path):
    class Synthetic(torch.utils.data.Dataset):
        def __init__(self, n, seed):
            g = torch.Generator().manual_seed(seed)
            base = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(0))
            self.x = (base + 0.05 * torch.rand(n, 3, 16, 16, generator=g)).clamp(0, 1)

        def __len__(self):
            return self.x.shape[0]

        def __getitem__(self, i):
            return {"x": self.x[i]}

    hps = util.AttrDict(dict(
        profile="eval", model=dict(image_shape=[16, 16, 3], hidden_channels=32, K=2, L=2, actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False, flow_permutation="invconv",
                      flow_coupling="affine", max_grad_clip=5, max_grad_norm=100, seed=1),
        optim=dict(optimizer="adam", optimizer_args=dict(lr=1e-3, betas=[0.9, 0.9999], eps=1e-8), lr_scheduler="noam",
                   lr_scheduler_args=dict(warmup_steps=20, min_lr=1e-5), num_batch_train=8, num_epochs=8, interval_scalar=1,
                   interval_snapshot=10 ** 6, interval_valid=10 ** 6, interval_sample=10 ** 6, num_sample=2,
                   ema_decay=0.9, ema_eval=True, interval_eval=2),
        dataset=dict(num_classes=1, num_workers=0), device=dict(graph=["cuda:0"], data=["cuda:0"]),
        general=dict(result_dir=str(tmp_path), warm_start=False, pre_trained="", resume_run_id="", resume_step="")))
    util.manual_seed(3)
    state = Builder(hps).build()
    loader = torch.utils.data.DataLoader(Synthetic(11, 5), batch_size=4, shuffle=False)      # three batches: 4, 4, 3
    trainer = Trainer(hps=hps, dataset=Synthetic(32, 1), eval_loader=loader, **state)
    assert trainer.interval_eval == 2
    trainer.writer = _ScalarLog(str(tmp_path))
    opt = trainer.loop.optimizer
    params = [p for p in trainer.graph.parameters()]
    seen = []
    block = trainer._eval_weights

    def logged():
        before = [p.detach().clone() for p in params]
        ctx = block()

        class Wrapped:
            def __enter__(self):
                return ctx.__enter__()

            def __exit__(self, *a):
                out = ctx.__exit__(*a)
                seen.append(all(torch.equal(p.detach(), b) for p, b in zip(params, before)))
                return out
        return Wrapped()

    trainer._eval_weights = logged
    trainer.train(max_steps=3)      # steps 0, 1, 2: the block runs once, behind step 2
    assert seen == [True], seen     # the parameters are bitwise what they were before the block
    assert trainer.graph.training and not opt.swapped
    scalars = trainer.writer.scalars
    assert [s for s, _ in scalars["eval/bits_per_dim"]] == [2]
    with training.averaged_weights(opt):
        ref = Evaluator(trainer.graph).run(loader)
    assert trainer.graph.training
    assert scalars["eval/bits_per_dim"][0][1] == ref.bits_per_dim and scalars["eval/bits_per_dim_single"][0][1] == ref.bits_per_dim_single
    assert [scalars[f"eval/level_bits/{l}"][0][1] for l in range(2)] == ref.level_bits
    assert trainer.last_eval.state_bytes() == ref.state_bytes() and ref.count == 11
    live = Evaluator(trainer.graph).run(loader)
    assert live.state_bytes() != ref.state_bytes()      # the average is not the live weights: the block really ran under it
    trainer.train(max_steps=1)      # the next training step runs
    assert trainer.step == 4 and trainer.loop.graph_error is None
    assert torch.isfinite(torch.as_tensor(float(trainer.last_loss)))

"""GPU tests of the restoration path (-m gpu): glowhip_restore_objective (csrc/restore.hip) against the fp64 restatement of
tests/restore_oracle.py on every element, its edge cases, the latent gradient of the objective (objective + glowhip_plan_decode_vjp)
against fp64 autograd through `O.flow_decode`, the device-resident loop `network.restore.LatentFit` -- captured, eager and composed
by hand from the public pieces, bit for bit -- its prior term against tests/optim_oracle.py, and `Inferer.restore` on the in-painting
and super-resolution fits whose ratios tests/test_restore_host.py fixes on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import training  # noqa: E402
from pytorch_glow_amd.network import Inferer, LatentFit, Latents, RestoreInfo, restore_objective  # noqa: E402

import decode_grad_oracle as D  # noqa: E402
import optim_oracle as OO  # noqa: E402
import restore_oracle as R  # noqa: E402
from test_decode_grad_host import SHAPE_CASES, SHAPE_MARGIN_FLOOR  # noqa: E402
from test_gpu_decode_grad import DEV, TINY_AFF, assert_margin, check_strict, dev, make_glow, plan_of  # noqa: E402

assert TINY_AFF == R.TINY_AFF


def shifted(t):
    """A device copy of ``t`` that starts one float into a larger buffer: contiguous, 4 bytes past a 16-byte address."""
    n = t.numel()
    view = torch.zeros(n + 4, device=DEV)[1:1 + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 1. the objective, every element
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "ones"])
@pytest.mark.parametrize("shape,pool", R.OBJECTIVE_SHAPES, ids=[f"{'x'.join(map(str, s))}-pool{p}" for s, p in R.OBJECTIVE_SHAPES])
def test_objective_every_element_vs_fp64_oracle(shape, pool, weighted):
    """loss and grad_x within `restore_oracle.bound`, which walks the kernel's fp32 roundings: a gradient element is pool^2 - 1
    additions and one multiplication for P x, the subtraction, and the multiplications by w, 2 inv_wsum and 1 / pool^2 (one more
    rounding each for the constants float(1 / elements) and float(1 / pool^2)); the loss is the fp64 sum of the fp64 products of those
    fp32 residuals, times inv_wsum, rounded once.  tests/test_restore_host.py shows a float32 restatement of that arithmetic inside
    the bound on these very inputs (worst multiple 0.32), and a relative 2^-18 outside it: nothing here was tuned on the device.
    The 64x64 shape (12 288 elements per sample: the 16-byte path) also runs from views one float off a 16-byte address -- x alone,
    then every tensor -- where the kernel must fall back to the element loop: same bound, and the same gradient bits."""
    x, t, w, inv = R.objective_inputs(shape, pool, weighted)
    loss_ref, g_ref = R.objective(x, t, w, inv, pool)
    E_loss, E_g = R.bound(x, t, w, inv, pool)
    opt = lambda v, f=dev: None if v is None else f(v)
    placements = [("aligned", dev, dev)]
    if shape == (2, 3, 64, 64):
        placements += [("x one float off", shifted, dev), ("all one float off", shifted, shifted)]
    first = None
    for name, fx, fo in placements:
        xd, td, wd = fx(x), fo(t), opt(w, fo)
        g_out = fo(torch.zeros(shape))
        if name == "aligned":
            assert all(v is None or v.data_ptr() % 16 == 0 for v in (xd, td, wd, g_out))
        loss, g = restore_objective(xd, td, wd, opt(inv), pool, grad_out=g_out)
        assert g is g_out
        ml, mg = R.worst_multiple(loss, loss_ref, E_loss), R.worst_multiple(g, g_ref, E_g)
        print(f"{shape} pool {pool} {'weighted' if weighted else 'ones'} {name}: worst multiple of the bound  loss {ml:.3f}  grad {mg:.3f}")
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all())
        assert ml <= 1.0 and mg <= 1.0, (name, ml, mg)
        if first is None:
            first = g.clone()
        else:
            assert same_bits(g, first), f"{name}: the element loop's gradient differs from the 16-byte path's"


# ------------------------------------------------------------------------------------------------ 2. edge cases
@pytest.mark.parametrize("shape,pool", [((3, 3, 64, 64), 1), ((3, 3, 6, 10), 2)], ids=["vector", "pool2"])
def test_zero_weight_sample_nan_sample_and_reproducibility(shape, pool):
    x, t, w, _ = R.objective_inputs(shape, pool, True, seed=1)
    run = lambda x_, w_, inv_: restore_objective(dev(x_), dev(t), dev(w_), dev(inv_), pool)
    loss, g = run(x, w, R.inv_wsum_of(w))
    again = run(x, w, R.inv_wsum_of(w))
    assert same_bits(loss, again[0]) and same_bits(g, again[1])                      # two runs of the same call: the same bits
    # a zero-weight sample: exact zeros, the others bit for bit what they were
    w0 = w.clone()
    w0[1] = 0.0
    loss0, g0 = run(x, w0, R.inv_wsum_of(w0))
    assert float(loss0[1]) == 0.0 and float(g0[1].abs().max()) == 0.0
    assert same_bits(loss0[[0, 2]], loss[[0, 2]]) and same_bits(g0[[0, 2]], g[[0, 2]])
    # a NaN in one sample's x: that sample's loss and the gradient under that cell are NaN, the other samples' outputs unchanged
    xn = x.clone()
    xn[1, 0, 2, 3] = float("nan")
    lossn, gn = run(xn, w, R.inv_wsum_of(w))
    assert bool(torch.isnan(lossn[1])) and bool(torch.isnan(gn[1]).any())
    assert same_bits(lossn[[0, 2]], loss[[0, 2]]) and same_bits(gn[[0, 2]], g[[0, 2]])
    # inv_wsum[n] == 0: exact zeros whatever x[n] holds -- the NaN included
    inv = R.inv_wsum_of(w)
    inv[1] = 0.0
    lossz, gz = run(xn, w, inv)
    assert float(lossz[1]) == 0.0 and float(gz[1].abs().max()) == 0.0 and bool(torch.isfinite(gz).all())
    assert same_bits(lossz[[0, 2]], loss[[0, 2]]) and same_bits(gz[[0, 2]], g[[0, 2]])
    # loss_out may be NULL: the gradient is the same
    gl, xd, td = torch.empty_like(g), dev(x), dev(t)
    rc = G.lib().glowhip_restore_objective(xd.data_ptr(), td.data_ptr(), None, None, *shape, pool, gl.data_ptr(), None,
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    _, g1 = restore_objective(xd, td, None, None, pool)
    assert same_bits(gl, g1)


# ------------------------------------------------------------------------------------------------ 3. first-iteration latent gradients
LATENT_CASES = {"tiny": (TINY_AFF, 1, True), "R": (SHAPE_CASES["R"], 1, False), "T": (SHAPE_CASES["T"], 2, True)}


@pytest.mark.parametrize("cid", list(LATENT_CASES))
def test_latent_gradients_of_the_objective_vs_fp64_autograd_oracle(cid):
    """Objective + decode_vjp against fp64 autograd of the same objective through `O.flow_decode`, every entry within the project's
    gradient rule 2e-4 max|g| + 1e-7 per tensor (check_strict).  tiny: the per-layer route; R (12x20): the scalar kernel forms; T
    (64x16, hidden 512): the fused k_cnet chain, with pool 2.  The ReLU masks depend on the decoded image only -- not on the vector
    the VJP is applied to -- so the margins the project holds for these seeds on the CPU carry over: tiny and R are held to
    MIN_MARGIN (assert_margin); T's seed is held to its recorded floor 4e-6 (tests/test_decode_grad_host.py: no seed scanned
    reaches 1e-5 at that shape), and is still compared under the strict rule here, not the capped one."""
    kw, pool, weighted = LATENT_CASES[cid]
    ref = D.reference(**kw)
    if cid == "T":
        assert ref["margin"] >= SHAPE_MARGIN_FLOOR[cid], ref["margin"]
        assert all(bool(torch.isfinite(t).all()) for t in [ref["gz"]] + ref["geps"])
    else:
        assert_margin(ref)
    shape = tuple(ref["x"].shape)
    _, target, weight, inv = R.objective_inputs(shape, pool, weighted, seed=7)
    x_ref, loss_ref, gz_ref, geps_ref = R.latent_grads(ref["z"], ref["eps"], ref["sd"], ref["cfg"], target, weight, inv, pool, ref["tables"])
    glow = make_glow(ref, kw.get("perm", "invconv"))
    plan = plan_of(glow, ref)
    opt = lambda v: None if v is None else dev(v)
    x, _ = plan.decode(dev(ref["z"]), [dev(e) for e in ref["eps"]])
    loss, gx = restore_objective(x, dev(target), opt(weight), opt(inv), pool)
    plan.launch_counts(reset=True)
    gz, geps = plan.decode_vjp(x, gx)
    counts = plan.launch_counts(reset=True)
    ex = float((x.cpu().double() - x_ref).abs().max())
    el = float(((loss.cpu().double() - loss_ref).abs() / loss_ref).max())
    print(f"{cid}: margin {ref['margin']:.2e}, decode err {ex:.2e}, loss rel err {el:.2e}, {counts}")
    assert ex <= 1e-4 and el <= 1e-4
    if cid == "T":
        assert counts.get("k_cnet(tape)") == 4 and counts.get("k_cnet(bwd)") == 4, counts
    else:
        assert not [k for k in counts if k.startswith("k_cnet")], counts
    check_strict(dict(gz=gz_ref, geps=geps_ref), gz, geps, f"restore {cid}")


# ------------------------------------------------------------------------------------------------ the fits' set-up
def fit_setup(kw, pool):
    """(glow, inferer, measurement, weight, start latents): the target is the decode of the case's latents, the measurement its
    pool x pool average, the weights the left half of the measurement, the start the latents of the target with that half blanked
    (`restore_oracle.fit_case`, test_fit_latents_inpaints_the_masked_half)."""
    ref = D.reference(**kw)
    glow = make_glow(ref, kw.get("perm", "invconv"))
    inf = Inferer(D.hps_for(ref["cfg"], ref["cfg"]["batch"]), glow, [DEV], DEV)
    target = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    meas = F.avg_pool2d(target, pool) if pool > 1 else target.clone()
    weight = torch.zeros_like(meas)
    weight[..., : meas.shape[-1] // 2] = 1.0
    blank = torch.ones_like(target)
    blank[..., : target.shape[-1] // 2] = 0.0
    init = inf.encode_full(target * blank)
    return glow, inf, meas, weight, init


# ------------------------------------------------------------------------------------------------ 4. captured = eager = by hand
@pytest.mark.parametrize("cid,pool", [("tiny", 1), ("T", 2)])
def test_captured_eager_and_hand_composed_loops_agree_bitwise(cid, pool):
    """Four iterations with a prior term and a norm clip that binds: the captured loop (one eager iteration, then three replays of
    one hipGraph), the eager loop, and the same iteration written out with `decode_latents`, `restore_objective`, `decode_vjp` and
    `HipAdam.fused_step`: the same latents, loss history and norm history, bit for bit."""
    kw = LATENT_CASES[cid][0]
    glow, inf, meas, weight, init = fit_setup(kw, pool)
    # (the oracle's norms over these four iterations, tests/restore_oracle.py: 0.15 .. 0.04 on tiny, 0.022 .. 0.014 on T)
    lam, clip = 1e-3, 0.01
    args = dict(weight=weight, pool=pool, init=init, steps=4, lr=0.2, prior_weight=lam, max_grad_norm=clip)
    results = {}
    for name, graph in (("captured", True), ("eager", False)):
        fit = LatentFit(glow, meas, graph=graph, **args)
        info = fit.run()
        assert isinstance(info, RestoreInfo) and info.finite and info.fallback == 0
        assert info.captured == graph, f"{name}: captured = {info.captured} ({info.graph_error})"
        assert tuple(info.loss.shape) == (4, len(init)) and tuple(info.grad_norm.shape) == (4,)
        results[name] = (fit.latents().tensors(), info.loss, info.grad_norm)
    # by hand
    plan = glow.flow.plan_for(meas.new_empty((1, 3, meas.shape[2] * pool, meas.shape[3] * pool)))
    leaves = [t.clone().requires_grad_() for t in init.tensors()]
    opt = training.HipAdam(leaves, lr=0.2, weight_decay=lam)
    inv = 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0)
    losses, norms = [], []
    for _ in range(4):
        x = glow.decode_latents(Latents(leaves[0].detach(), [e.detach() for e in leaves[1:]]), safe=False)
        loss, gx = restore_objective(x, meas, weight, inv, pool)
        gz, geps = plan.decode_vjp(x, gx)
        for p, g in zip(leaves, [gz] + geps):
            p.grad = g
        norms.append(opt.fused_step(0.0, clip, skip_nonfinite=True).clone())
        losses.append(loss)
    results["by hand"] = ([p.detach() for p in leaves], torch.stack(losses).cpu(), torch.stack(norms).cpu())
    lat, loss, norm = results["captured"]
    print(f"{cid}: loss {[f'{v:.4e}' for v in loss[:, 0].tolist()]} norm {[f'{v:.4e}' for v in norm.tolist()]}")
    assert float(norm.min()) > clip, "the clip does not bind: pick a smaller max_grad_norm"
    assert not same_bits(lat[0], init.z)
    for name in ("eager", "by hand"):
        other = results[name]
        assert all(same_bits(a, b) for a, b in zip(lat, other[0])), f"{name}: latents differ from the captured loop's"
        assert same_bits(loss, other[1]) and same_bits(norm, other[2]), f"{name}: histories differ from the captured loop's"


def test_a_reallocated_workspace_costs_the_fit_a_recapture_not_an_error():
    """The 8x8 linear-Gaussian model of tests/posterior_oracle.py, two measurements.  A fit whose later iterations ran as replays;
    then an eager decode of a larger batch on the same plan, which re-allocates the inference workspace the recorded launches
    reach.  The next `run` records the iteration again, silently -- ``captured``, no ``graph_error`` -- and its histories and
    latents are the eager fit's, bit for bit."""
    import posterior_oracle as P
    case = P.linear_case("affine")
    glow = make_glow(dict(cfg=case["cfg"], sd=case["sd"]))
    as_batch = lambda a, n: dev(torch.from_numpy(a).float()).expand(n, *a.shape).contiguous()
    zeros = lambda n: [dev(torch.zeros((n,) + s)) for s in case["shapes"]]
    init = Latents(zeros(2)[0], zeros(2)[1:])
    args = dict(weight=as_batch(case["weight"], 2), init=init, steps=3, lr=0.05, prior_weight=1e-3)
    fit = LatentFit(glow, as_batch(case["target"], 2), graph=True, **args)
    first = fit.run()
    assert first.captured and first.graph_error is None and fit.captured
    plan = fit.plan
    before = (plan._ws.data_ptr(), plan._ws.numel())
    big = plan.decode(zeros(64)[0], zeros(64)[1:])[0]
    assert bool(torch.isfinite(big).all())
    assert plan._ws.numel() > before[1] and (plan._ws.data_ptr(), plan._ws.numel()) != before, "the larger batch did not re-allocate"
    assert not fit.captured, "the recorded iteration still counts as valid over a freed workspace"
    info = fit.run()
    assert info.captured and info.graph_error is None and info.finite and fit.captured
    eager = LatentFit(glow, as_batch(case["target"], 2), graph=False, **args)
    ref = eager.run()
    assert not ref.captured and float(ref.loss[0].min()) > 0.0
    assert same_bits(info.loss, ref.loss) and same_bits(info.grad_norm, ref.grad_norm)
    assert same_bits(first.loss, ref.loss) and same_bits(first.grad_norm, ref.grad_norm)
    assert all(same_bits(a, b) for a, b in zip(fit.latents().tensors(), eager.latents().tensors()))


# ------------------------------------------------------------------------------------------------ 5. the prior term
def test_prior_term_is_the_optimiser_oracles_weight_decay_step():
    """An all-zero weight leaves the prior term alone: loss 0, gradient norm 0, and ONE step is tests/optim_oracle.py's Adam step
    with a zero gradient and weight_decay = the prior weight -- p, exp_avg and exp_avg_sq on every element within the bound
    tests/test_gpu_optim.py holds the optimiser to (optim_oracle.bound)."""
    lam, lr = 0.25, 0.05
    glow, inf, meas, weight, init = fit_setup(TINY_AFF, 1)
    fit = LatentFit(glow, meas, weight=torch.zeros_like(weight), init=init, steps=1, lr=lr, prior_weight=lam, graph=False)
    info = fit.run()
    assert info.finite and float(info.loss.abs().max()) == 0.0 and float(info.grad_norm[0]) == 0.0
    host = lambda t: t.detach().cpu().numpy().ravel().copy()
    p0 = OO.cat([host(t) for t in init.tensors()])
    zero = np.zeros_like(p0)
    h = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=lam, step=1, clip_value=0.0, max_norm=0.0)
    ref = OO.step("adam", p0, zero, zero, zero, h, np.float32(1.0))
    E = OO.bound("adam", p0, zero, zero, zero, h, np.float32(1.0))
    opt = fit.optimizer
    got = (OO.cat([host(p.grad) for p in fit.leaves]), OO.cat([host(opt.state[p]["exp_avg"]) for p in fit.leaves]),
           OO.cat([host(opt.state[p]["exp_avg_sq"]) for p in fit.leaves]), OO.cat([host(p) for p in fit.leaves]))
    assert float(np.abs(got[0]).max()) == 0.0                 # the data term's gradient: exact zeros
    mult = [OO.worst_multiple(a, b, e) for a, b, e in zip(got, ref, E)]
    print(f"prior step: worst multiple of the bound  g {mult[0]:.3f}  m {mult[1]:.3f}  v {mult[2]:.3f}  p {mult[3]:.3f}")
    assert max(mult) <= 1.0, mult
    assert float(np.abs(got[3] - p0).max()) > 0.0


# ------------------------------------------------------------------------------------------------ 6. the guard
def test_prior_weight_on_a_learned_top_prior_raises():
    ref = D.reference(**TINY_AFF)
    hps = D.hps_for(ref["cfg"], ref["cfg"]["batch"])
    hps.ablation.learn_top = True
    glow = G.Glow(hps)
    glow.load_state_dict({k: v.clone() for k, v in ref["sd"].items()}, strict=False)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).eval()
    inf = Inferer(hps, glow, [DEV], DEV)
    image = dev(ref["x"].float())
    with pytest.raises(ValueError, match="learn_top"):
        inf.restore(image, steps=2, prior_weight=0.1)
    lat, info = inf.restore(image, steps=2, prior_weight=0.0)      # without the prior term the model is as good as any
    assert isinstance(lat, Latents) and info.finite


# ------------------------------------------------------------------------------------------------ 7. in-painting, super-resolution
@pytest.mark.parametrize("name,cid,pool,ratio", [("inpaint", "tiny", 1, R.INPAINT_RATIO), ("superres", "T", 2, R.SUPERRES_RATIO)])
def test_restore_inpaints_and_super_resolves(name, cid, pool, ratio):
    """`Inferer.restore` on the set-up of test_fit_latents_inpaints_the_masked_half (16x16, the left half masked, the start the
    latents of the blanked image, 20 steps at lr 0.2), and the same on T (64x16, hidden 512) through a 2x2 average pool with the left
    half of the low-resolution image as the measurement.  Every sample: each of the first five losses falls, and final / first <=
    the fp64 oracle's own worst ratio for this per-sample objective rounded up to the next of 0.1 / 0.2 / 0.5
    (tests/test_restore_host.py; the oracle's samples: in-painting 0.082, 0.080, 0.090 -> 0.1; super-resolution 0.025, 0.023,
    0.027 -> 0.1)."""
    kw = LATENT_CASES[cid][0]
    glow, inf, meas, weight, init = fit_setup(kw, pool)
    lat, info = inf.restore(meas, weight=weight, pool=pool, steps=R.FIT_STEPS, lr=R.FIT_LR, init=init)
    hist = info.loss
    ratios = (hist[-1] / hist[0]).tolist()
    print(name, "loss of sample 0:", " ".join(f"{v:.3e}" for v in hist[:, 0].tolist()), "| final / first", [f"{r:.3f}" for r in ratios],
          "| captured", info.captured, info.graph_error)
    assert isinstance(lat, Latents) and tuple(hist.shape) == (R.FIT_STEPS, len(init)) and info.finite and info.fallback == 0
    assert info.captured, info.graph_error
    assert bool((hist[1:6] < hist[:5]).all()), hist[:6]
    assert max(ratios) <= ratio, ratios
    # the returned latents are the fitted ones, not the start: their decode's loss is below the first
    x = glow.decode_latents(lat, safe=False)
    loss, _ = restore_objective(x, meas, weight, 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0), pool)
    assert bool((loss.cpu() < hist[0]).all())


# ------------------------------------------------------------------------------------------------ 8. a non-finite start
def test_non_finite_start_is_skipped_on_the_device_and_reported():
    glow, inf, meas, weight, init = fit_setup(TINY_AFF, 1)
    bad = Latents(init.z.clone(), [e.clone() for e in init.eps])
    bad.z[1, 0, 0, 0] = float("nan")
    assert glow.range_check
    lat, info = inf.restore(meas, weight=weight, steps=4, lr=0.2, init=bad, prior_weight=0.01)
    print("norms", info.grad_norm.tolist(), "fallback", info.fallback, "captured", info.captured, info.graph_error)
    assert not bool(torch.isfinite(info.grad_norm).any()), info.grad_norm
    assert info.finite is False and info.fallback == 1
    assert all(same_bits(a, b) for a, b in zip(lat.tensors(), bad.tensors())), "a skipped step moved the latents"
    plan = glow.flow.plan_for(meas)
    assert plan.family == plan.FAMILY_AUTO                     # the exact-family re-run put the plan's family back
    # exact=True: the one run is the exact family's, so nothing is left to fall back to
    lat, info = inf.restore(meas, weight=weight, steps=2, lr=0.2, init=bad, exact=True)
    assert info.finite is False and info.fallback == 0 and plan.family == plan.FAMILY_AUTO


# ------------------------------------------------------------------------------------------------ 9. no host sync in a replay
def test_replays_make_no_host_sync():
    glow, inf, meas, weight, init = fit_setup(TINY_AFF, 1)
    fit = LatentFit(glow, meas, weight=weight, init=init, steps=8, lr=0.2)
    fit.reset()
    fit.step_eager()
    assert fit.capture(), fit.graph_error
    fit.step_captured()                # (the first replay: whatever the runtime sets up lazily for a graph)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except (AttributeError, RuntimeError, NotImplementedError) as e:
        pytest.skip(f"this torch build does not implement the sync debug mode: {e}")
    try:
        for _ in range(3):
            fit.step_captured()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    hist = fit.loss_hist.cpu()
    assert bool((hist[1:5, 0] < hist[:4, 0]).all()) and float(hist[5:].abs().max()) == 0.0, hist[:, 0]

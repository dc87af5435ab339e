"""GPU tests of blind deblurring (-m gpu): glowhip_restore_psf_grad and glowhip_psf_from_logits (csrc/restore_blind.hip) against the
fp64 restatement of tests/blind_oracle.py on every element; the kernels' structural properties (a sample alone = in a batch, run to
run, zero-weight and NaN samples); `LatentFit(estimate_psf=...)` against the non-blind objective, captured against eager and against
the iteration written out by hand, bit for bit; `Inferer.estimate_psf` and `Inferer.restore(estimate_psf="shared")` on the two fits
whose thresholds tests/test_blind_host.py fixes on the CPU; and the paths without ``estimate_psf``, unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import training  # noqa: E402
from pytorch_glow_amd.network import (LatentFit, Latents, PsfFit, RestoreInfo, psf_from_logits, psf_gradient,  # noqa: E402
                                      restore_objective)
from pytorch_glow_amd.network.restore import blind_start, psf_grad_scratch  # noqa: E402

import blind_oracle as K  # noqa: E402
import deblur_oracle as B  # noqa: E402
import restore_oracle as R  # noqa: E402
from test_gpu_deblur import opt, same_bits, setup, shifted  # noqa: E402
from test_gpu_decode_grad import DEV, dev  # noqa: E402


def gradients(x, t, w, inv, pool, k, f=dev):
    """(grad_psf, grad_logits, resid) of the device for host inputs placed by ``f``: the objective through the PSF, then the
    gradient call on what it left; every output buffer starts as NaN."""
    xd, td, wd, invd, kd = f(x), f(t), opt(w, f), opt(inv, f), f(k)
    resid = f(torch.full(t.shape, float("nan")))
    restore_objective(xd, td, wd, invd, pool, psf=kd, resid_out=resid)
    gk, gl = f(torch.full(k.shape, float("nan"))), f(torch.full(k.shape, float("nan")))
    out = psf_gradient(xd, resid, invd, kd, pool, grad_psf=gk, grad_logits=gl)
    assert out[0] is gk and out[1] is gl
    return gk, gl, resid


# ------------------------------------------------------------------------------------------------ 1. the gradient, every element
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "ones"])
@pytest.mark.parametrize("shape,ksize,pool", K.GRAD_CASES, ids=K.GRAD_IDS)
def test_gradient_every_element_vs_fp64_oracle(shape, ksize, pool, weighted, per_sample):
    """grad_psf and grad_logits within `blind_oracle.bound` on every element: the residual's own bound carried through, two
    roundings for u, 64 u sum |u| |x| for the fp32 chains of at most 64 terms however the pixels are dealt to them, nothing for the
    fp64 folds, one final rounding, and the softmax backward's formula over those errors.  tests/test_blind_host.py shows a float32
    restatement of those sums, in two orders, inside the bound on these very inputs: nothing here was tuned on the device.  The
    64x64 shapes also run with every pointer one float off a 16-byte address: the same bound and the same bits."""
    ref = K.grad_reference(shape, ksize, pool, weighted, per_sample)
    x, t, w, inv, k = (ref[n] for n in ("x", "target", "weight", "inv", "psf"))
    placements = [("aligned", dev)]
    if shape == (2, 3, 64, 64):
        placements += [("all one float off", shifted)]
    first = None
    for name, f in placements:
        gk, gl, _ = gradients(x, t, w, inv, pool, k, f)
        mk, ml = K.worst_multiple(gk, ref["grad_psf"], ref["E_psf"]), K.worst_multiple(gl, ref["grad_logits"], ref["E_logits"])
        print(f"{shape} psf {ksize} pool {pool} {'weighted' if weighted else 'ones'} {'per-sample' if per_sample else 'shared'} {name}: "
              f"worst multiple of the bound  grad_psf {mk:.4f}  grad_logits {ml:.4f}")
        assert bool(torch.isfinite(gk).all()) and bool(torch.isfinite(gl).all())
        assert mk <= 1.0 and ml <= 1.0, (name, mk, ml)
        # the orientation: the PSFs have no symmetry, and the gradient with its taps mirrored is far outside
        assert K.worst_multiple(gk.flip(-2, -1), ref["grad_psf"], ref["E_psf"]) > 1.0
        if first is None:
            first = (gk.clone(), gl.clone())
        else:
            assert same_bits(gk, first[0]) and same_bits(gl, first[1]), f"{name}: bits differ from the aligned call's"


def test_either_output_alone_and_the_python_layer_refusals():
    ref = K.grad_reference((3, 3, 6, 10), (5, 3), 2, True, True)
    x, t, w, inv, k = (ref[n] for n in ("x", "target", "weight", "inv", "psf"))
    gk, gl, resid = gradients(x, t, w, inv, 2, k)
    xd, invd, kd = dev(x), dev(inv), dev(k)
    only_k, none = psf_gradient(xd, resid, invd, kd, 2, grad_psf=torch.empty_like(kd))
    assert none is None and same_bits(only_k, gk)
    none, only_l = psf_gradient(xd, resid, invd, kd, 2, grad_logits=torch.empty_like(kd))
    assert none is None and same_bits(only_l, gl)
    both = psf_gradient(xd, resid, invd, kd, 2, scratch=psf_grad_scratch(x.shape, 5, 3, 2, DEV))
    assert same_bits(both[0], gk) and same_bits(both[1], gl)
    with pytest.raises(G._lib.GlowHipError, match="psf"):
        psf_gradient(xd, resid, invd, k, 2)                                              # on the host
    with pytest.raises(G._lib.GlowHipError, match="psf"):
        psf_gradient(xd, resid, invd, dev(k[:2]), 2)                                     # two PSFs for a batch of three
    with pytest.raises(G._lib.GlowHipError, match="resid"):
        psf_gradient(xd, dev(torch.zeros(3, 3, 6, 10)), invd, kd, 2)
    with pytest.raises(G._lib.GlowHipError, match="scratch"):
        psf_gradient(xd, resid, invd, kd, 2, scratch=torch.empty(64, dtype=torch.uint8, device=DEV))   # too small: the C call's refusal
    with pytest.raises(G._lib.GlowHipError, match="taps"):
        psf_gradient(xd, resid, invd, dev(torch.ones(4, 3)), 2)                          # an even side: the C call's refusal
    with pytest.raises(G._lib.GlowHipError, match="logits"):
        psf_from_logits(torch.zeros(3, 3))


# ------------------------------------------------------------------------------------------------ 2. reproducibility and isolation
@pytest.mark.parametrize("shape,ksize,pool", [((5, 3, 20, 70), (5, 5), 1), ((5, 2, 6, 10), (5, 3), 2)], ids=["tiles", "pool2"])
def test_sample_alone_run_to_run_zero_weight_and_nan_samples(shape, ksize, pool):
    x, t, w, _, k = K.grad_inputs(shape, ksize, pool, True, True, seed=2)
    inv = R.inv_wsum_of(w)
    base = gradients(x, t, w, inv, pool, k)
    again = gradients(x, t, w, inv, pool, k)
    assert all(same_bits(a, b) for a, b in zip(base, again))                         # two runs of the same call: the same bits
    # a sample alone = in the batch of five, bit for bit (per-sample PSFs; buffers placed alike: both at allocation boundaries)
    for n in (0, 3):
        alone = gradients(x[n:n + 1], t[n:n + 1], w[n:n + 1], inv[n:n + 1], pool, k[n:n + 1])
        assert same_bits(alone[0][0], base[0][n]) and same_bits(alone[1][0], base[1][n]), f"sample {n} alone differs from the batch"
    others = lambda out: [v[[0, 1, 3, 4]] for v in out[:2]]
    unchanged = lambda out: all(same_bits(a, b) for a, b in zip(others(out), others(base)))
    # inv_wsum[n] == 0: exact zeros whatever x[n] holds -- a NaN included --, the others bit for bit what they were
    xn = x.clone()
    xn[2, 0, 2, 3] = float("nan")
    inv0 = inv.clone()
    inv0[2] = 0.0
    out = gradients(xn, t, w, inv0, pool, k)
    assert float(out[0][2].abs().max()) == 0.0 and float(out[1][2].abs().max()) == 0.0
    assert all(bool(torch.isfinite(v).all()) for v in out[:2]) and unchanged(out)
    # a NaN in one sample's x: that sample's gradient is NaN, no other sample's moves
    out = gradients(xn, t, w, inv, pool, k)
    assert bool(torch.isnan(out[0][2]).any()) and bool(torch.isnan(out[1][2]).any()) and unchanged(out)
    # a shared PSF: the NaN reaches the shared gradient; the zero-weight NaN sample reaches nothing, and the shared gradient is the
    # oracle's sum over the other four samples
    shared = gradients(xn, t, w, inv, pool, k[0])
    assert bool(torch.isnan(shared[0]).any())
    shared0 = gradients(xn, t, w, inv0, pool, k[0])
    assert bool(torch.isfinite(shared0[0]).all()) and bool(torch.isfinite(shared0[1]).all())
    keep = [0, 1, 3, 4]
    g_ref = K.psf_grad(x[keep], t[keep], w[keep], inv[keep], pool, k[0])
    E_gk, E_gl = K.bound(x[keep], t[keep], w[keep], inv[keep], pool, k[0])
    assert K.worst_multiple(shared0[0], g_ref, E_gk) <= 1.0
    assert K.worst_multiple(shared0[1], K.softmax_backward(k[0], g_ref), E_gl) <= 1.0


# ------------------------------------------------------------------------------------------------ 3. the softmax
@pytest.mark.parametrize("shape", [(15, 15), (4, 5, 3), (3, 1, 9), (2, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_psf_from_logits_is_the_fp64_softmax_rounded_once(shape):
    """Every tap within one fp32 rounding of the fp64 softmax (u |k|, plus 2^-40 |k| for the device's fp64 exponential), the taps of
    a PSF summing to 1 within kh kw 2^-24; logits far from zero overflow nothing (the max is subtracted); a buffer one float off
    gives the same bits."""
    g = torch.Generator().manual_seed(30)
    for scale, shift in ((1.0, 0.0), (4.0, 0.0), (1.0, 1000.0), (1.0, -1000.0)):
        theta = torch.randn(shape, generator=g) * scale + shift
        ref = K.softmax(theta)
        k = psf_from_logits(dev(theta))
        assert tuple(k.shape) == shape and bool((k >= 0).all())
        err = (k.cpu().double() - ref).abs()
        assert bool((err <= (K.U + 2.0 ** -40) * ref + K.FLOOR).all()), float((err / ref).max())
        nk = shape[-2] * shape[-1]
        assert float((k.cpu().double().sum(dim=(-2, -1)) - 1.0).abs().max()) <= nk * 2.0 ** -24
        out = shifted(torch.zeros(shape))
        assert psf_from_logits(shifted(theta), out=out) is out and same_bits(out, k)


# ------------------------------------------------------------------------------------------------ 4. the loop
def theta0_of(start):
    return torch.log(start.double()).float()


def test_first_loss_of_a_blind_fit_is_the_non_blind_objective_on_the_start_psf():
    fit_kw, ref, glow, inf, meas, weight, _ = setup("deblur")
    init = inf.encode_full(meas)
    start = blind_start((5, 5), "shared", meas.shape[0])
    psf0 = psf_from_logits(dev(theta0_of(start)))
    blind = LatentFit(glow, meas, weight=weight, init=init, steps=2, lr=0.05, psf=(5, 5), estimate_psf="shared", graph=False)
    info = blind.run()
    x0 = glow.decode_latents(init, safe=False)
    loss0, _ = restore_objective(x0, meas, weight, 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0), 1, psf=psf0)
    assert same_bits(info.loss[0], loss0.cpu())
    plain = LatentFit(glow, meas, weight=weight, init=init, steps=2, lr=0.05, psf=psf0, graph=False).run()
    assert same_bits(info.loss[0], plain.loss[0]) and same_bits(info.grad_norm[0], plain.grad_norm[0])
    assert not same_bits(info.loss[1], plain.loss[1])                      # the PSF moved
    assert plain.psf is None and plain.psf_grad_norm is None
    assert tuple(info.psf.shape) == (5, 5) and info.psf.is_cuda and tuple(info.psf_grad_norm.shape) == (2,)


@pytest.mark.parametrize("mode", ["shared", "per_sample"])
def test_blind_fit_captured_eager_and_hand_composed_agree_bitwise_without_a_sync_in_a_replay(mode):
    """Four iterations with a prior term on the 16x16 case: the captured loop (one eager iteration, then three replays of one
    hipGraph), the eager loop, and the iteration written out with `psf_from_logits`, `decode_latents`, `restore_objective(psf=)`,
    `psf_gradient`, `decode_vjp` and two `HipAdam.fused_step`s: the same latents, logits, PSF and histories, bit for bit; `run` again
    (a `reset` in between) reproduces them.  Then three replays under torch's sync debug mode: none makes a host sync."""
    fit_kw, ref, glow, inf, meas, weight, _ = setup("deblur")
    n = meas.shape[0]
    init = inf.encode_full(meas)
    lam = 1e-3
    start = B.asymmetric_psf(5, 3) + 0.01
    args = dict(weight=weight, pool=1, init=init, steps=4, lr=0.05, prior_weight=lam, psf=start, estimate_psf=mode, psf_lr=0.2)
    results = {}
    for name, graph in (("captured", True), ("eager", False)):
        fit = LatentFit(glow, meas, graph=graph, **args)
        assert tuple(fit.psf.shape) == ((5, 3) if mode == "shared" else (n, 5, 3))
        for rerun in range(2 if graph else 1):
            info = fit.run()
            assert isinstance(info, RestoreInfo) and info.finite and info.fallback == 0
            assert info.captured == graph, f"{name}: captured = {info.captured} ({info.graph_error})"
            got = (*fit.latents().tensors(), fit.blind.theta.detach().clone(), info.psf, info.loss, info.grad_norm, info.psf_grad_norm)
            if rerun:
                assert all(same_bits(a, b) for a, b in zip(got, results[name])), "reset() and a second run differ from the first"
            results[name] = got
    # by hand
    plan = glow.flow.plan_for(meas)
    k0 = blind_start(start, mode, n)
    theta = dev(theta0_of(k0)).reshape(-1, 5, 3).clone().requires_grad_()
    theta.grad = torch.zeros_like(theta)
    psf = dev(k0).clone()
    leaves = [t.clone().requires_grad_() for t in init.tensors()]
    optim = training.HipAdam(leaves, lr=0.05, weight_decay=lam)
    optim_k = training.HipAdam([theta], lr=0.2, weight_decay=0.0)
    inv = 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0)
    losses, norms, norms_k = [], [], []
    for _ in range(4):
        psf_from_logits(theta.detach().view(psf.shape), out=psf)
        x = glow.decode_latents(Latents(leaves[0].detach(), [e.detach() for e in leaves[1:]]), safe=False)
        resid = torch.empty_like(meas)
        loss, gx = restore_objective(x, meas, weight, inv, 1, psf=psf, resid_out=resid)
        psf_gradient(x, resid, inv, psf, 1, grad_logits=theta.grad.view(psf.shape))
        gz, geps = plan.decode_vjp(x, gx)
        for p, g in zip(leaves, [gz] + geps):
            p.grad = g
        norms.append(optim.fused_step(0.0, 0.0, skip_nonfinite=True).clone())
        norms_k.append(optim_k.fused_step(0.0, 0.0, skip_nonfinite=True).clone())
        losses.append(loss)
    final = psf_from_logits(theta.detach().view(psf.shape).clone())
    results["by hand"] = (*[p.detach() for p in leaves], theta.detach(), final, torch.stack(losses).cpu(), torch.stack(norms).cpu(),
                          torch.stack(norms_k).cpu())
    cap = results["captured"]
    print(f"loss {[f'{v:.4e}' for v in cap[-3][:, 0].tolist()]} psf norm {[f'{v:.4e}' for v in cap[-1].tolist()]}")
    assert not same_bits(cap[-5], dev(theta0_of(k0)).reshape(-1, 5, 3)) and float(cap[-1].min()) > 0.0
    assert float((cap[-4].sum(dim=(-2, -1)) - 1.0).abs().max()) <= 15 * 2.0 ** -24
    for name in ("eager", "by hand"):
        other = results[name]
        assert len(other) == len(cap)
        for i, (a, b) in enumerate(zip(cap, other)):
            assert same_bits(a.reshape(-1), b.reshape(-1)), f"{name}: tensor {i} differs from the captured loop's"
    # replays make no host sync
    fit = LatentFit(glow, meas, **dict(args, steps=8))
    fit.reset()
    fit.step_eager()
    assert fit.capture(), fit.graph_error
    fit.step_captured()                # (the first replay: whatever the runtime sets up lazily for a graph)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            fit.step_captured()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    hist, hist_k = fit.loss_hist.cpu(), fit.blind.norm_hist.cpu()
    assert float(hist[:5].min()) > 0.0 and float(hist[5:].abs().max()) == 0.0, hist[:, 0]
    assert same_bits(hist[:4], cap[-3]) and same_bits(hist_k[:4], cap[-1]) and float(hist_k[5:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 5. the fits
def test_estimate_psf_calibrates():
    """`Inferer.estimate_psf` on the 16x16 case: the images known, the uniform 5x5 start, 60 steps at 0.2: the L1 error of the PSF,
    final / start <= the fp64 oracle's own ratio for the same fit (0.024) rounded up to 0.1 (tests/test_blind_host.py)."""
    fit = K.FITS["calibrate"]
    _, ref, glow, inf, meas, weight, true_psf = setup("deblur")
    target = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    psf, info = inf.estimate_psf(target, meas, psf=(5, 5), steps=fit["steps"], psf_lr=fit["psf_lr"])
    e0, e1 = K.l1(torch.full((5, 5), 1.0 / 25.0), true_psf), K.l1(psf, true_psf)
    print(f"L1 error of the PSF {e0:.4f} -> {e1:.4f}: ratio {e1 / e0:.4f}; loss final / first {(info.loss[-1] / info.loss[0]).tolist()}")
    assert psf is info.psf and tuple(psf.shape) == (5, 5) and psf.is_cuda and info.finite and not info.captured
    assert tuple(info.loss.shape) == (fit["steps"], meas.shape[0]) and tuple(info.psf_grad_norm.shape) == (fit["steps"],)
    assert abs(float(psf.double().sum()) - 1.0) <= 25 * 2.0 ** -24 and bool((psf > 0).all())
    assert e1 / e0 <= fit["ratio"]
    # one PSF per image pair: each is calibrated on its own
    each, info_n = inf.estimate_psf(target, meas, psf=(5, 5), per_sample=True, steps=fit["steps"], psf_lr=fit["psf_lr"])
    assert tuple(each.shape) == (meas.shape[0], 5, 5)
    assert max(K.l1(each[i], true_psf) for i in range(meas.shape[0])) < e0 and info_n.finite
    # the utility is `PsfFit`: the same bits
    again = PsfFit(target, meas, blind_start((5, 5), "shared", meas.shape[0]), weight=weight, steps=fit["steps"], psf_lr=fit["psf_lr"]).run()
    assert same_bits(again.psf, psf) and same_bits(again.loss, info.loss)


def test_restore_deblurs_blind_and_its_estimate_feeds_the_posterior():
    """`Inferer.restore(psf=(5, 5), estimate_psf="shared")` from the default start (the latents of the blurred measurement, the
    uniform PSF), 60 steps at lr 0.05 / psf_lr 0.2: every sample's final / first data term <= the fp64 oracle's own worst ratio for
    the same fit (0.012) rounded up to 0.1 (tests/test_blind_host.py).  The untrained model is no meaningful prior: the data term is
    all that is asserted of the images; the PSF must have moved towards the truth."""
    fit = K.FITS["blind"]
    _, ref, glow, inf, meas, weight, true_psf = setup("deblur")
    lat, info = inf.restore(meas, steps=fit["steps"], lr=fit["lr"], psf=(5, 5), estimate_psf="shared", psf_lr=fit["psf_lr"])
    hist = info.loss
    ratios = (hist[-1] / hist[0]).tolist()
    e0, e1 = K.l1(torch.full((5, 5), 1.0 / 25.0), true_psf), K.l1(info.psf, true_psf)
    print("final / first", [f"{r:.4f}" for r in ratios], f"| L1 error of the PSF {e0:.4f} -> {e1:.4f} | captured", info.captured, info.graph_error)
    assert isinstance(lat, Latents) and tuple(hist.shape) == (fit["steps"], meas.shape[0]) and info.finite and info.fallback == 0
    assert info.captured, info.graph_error
    assert max(ratios) <= fit["ratio"], ratios
    assert e1 < e0 and tuple(info.psf.shape) == (5, 5) and abs(float(info.psf.double().sum()) - 1.0) <= 25 * 2.0 ** -24
    # the intended use: the estimate is the PSF of a posterior run
    _, post = inf.posterior(meas, noise_std=0.2, steps=3, burn_in=1, step_size=1e-3, seed=1, psf=info.psf)
    assert post.finite and tuple(post.energy.shape) == (3, meas.shape[0])


# ------------------------------------------------------------------------------------------------ 6. the paths without estimate_psf
def test_estimate_psf_none_is_the_call_as_it_was():
    """With and without a PSF: `Inferer.restore` and `LatentFit` with ``estimate_psf=None`` (and any ``psf_lr``) give the bits of the
    iteration written out by hand from the calls that existed before -- no softmax, no gradient call, one optimiser."""
    fit_kw, ref, glow, inf, meas, weight, psf = setup("deblur")
    init = inf.encode_full(meas)
    plan = glow.flow.plan_for(meas)
    inv = 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0)
    for k in (psf, None):
        _, a = inf.restore(meas, weight=weight, steps=3, lr=0.05, init=init, psf=k, border="zero")
        lat_b, b = inf.restore(meas, weight=weight, steps=3, lr=0.05, init=init, psf=k, border="zero", estimate_psf=None, psf_lr=0.7)
        fit = LatentFit(glow, meas, weight=weight, init=init, steps=3, lr=0.05, psf=k, estimate_psf=None)
        assert fit.blind is None
        c = fit.run()
        leaves = [t.clone().requires_grad_() for t in init.tensors()]
        optim = training.HipAdam(leaves, lr=0.05, weight_decay=0.0)
        losses, norms = [], []
        for _ in range(3):
            x = glow.decode_latents(Latents(leaves[0].detach(), [e.detach() for e in leaves[1:]]), safe=False)
            loss, gx = restore_objective(x, meas, weight, inv, 1, psf=k)
            gz, geps = plan.decode_vjp(x, gx)
            for p, g in zip(leaves, [gz] + geps):
                p.grad = g
            norms.append(optim.fused_step(0.0, 0.0, skip_nonfinite=True).clone())
            losses.append(loss)
        loss, norm = torch.stack(losses).cpu(), torch.stack(norms).cpu().view(-1)
        for info in (a, b, c):
            assert info.captured and info.psf is None and info.psf_grad_norm is None
            assert same_bits(info.loss, loss) and same_bits(info.grad_norm.view(-1), norm)
        assert all(same_bits(p, q) for p, q in zip(lat_b.tensors(), [p.detach() for p in leaves]))

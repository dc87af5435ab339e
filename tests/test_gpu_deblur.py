"""GPU tests of deblurring (-m gpu): glowhip_restore_objective_psf (csrc/restore.hip) against the fp64 restatement of
tests/deblur_oracle.py on every element of the loss, the gradient and the residual; the kernel's structural properties (orientation,
the bitwise anchor to glowhip_restore_objective, zero-weight and NaN samples, reproducibility); the latent gradient of the objective
against fp64 autograd through `O.flow_decode`; `LatentFit` and `LatentMALA` with a PSF, captured against eager bit for bit; and
`Inferer.restore(psf=, border="valid")` on the two fits whose ratios tests/test_deblur_host.py fixes on the CPU."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import training  # noqa: E402
from pytorch_glow_amd.network import Inferer, LatentFit, LatentMALA, Latents, RestoreInfo, restore_objective  # noqa: E402
from pytorch_glow_amd.network.restore import psf_valid_weight  # noqa: E402

import decode_grad_oracle as D  # noqa: E402
import deblur_oracle as B  # noqa: E402
import restore_oracle as R  # noqa: E402
from test_decode_grad_host import SHAPE_MARGIN_FLOOR  # noqa: E402
from test_gpu_decode_grad import DEV, assert_margin, check_strict, dev, make_glow, plan_of  # noqa: E402


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


opt = lambda v, f=dev: None if v is None else f(v)


# ------------------------------------------------------------------------------------------------ 1. the objective, every element
@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "ones"])
@pytest.mark.parametrize("shape,ksize,pool", B.OBJECTIVE_CASES, ids=B.CASE_IDS)
def test_objective_every_element_vs_fp64_oracle(shape, ksize, pool, weighted, per_sample):
    """loss, grad_x and resid within `deblur_oracle.bound`, which walks the kernel's fp32 roundings for any order of the tap sums,
    fused or not: kh kw u (|k| (*) |x|) for B x, the pool, d, w d, the constants, and the adjoint's own kh kw-term sum over the
    cells' values and their errors.  tests/test_deblur_host.py shows a float32 restatement of those sums, in two tap orders, inside
    the bound on these very inputs: nothing here was tuned on the device.  The 64x64 shapes also run with every pointer -- the PSF's
    and the residual's included -- one float off a 16-byte address: the same bound, and the same gradient and residual bits."""
    x, t, w, inv, k = B.objective_inputs(shape, ksize, pool, weighted, per_sample)
    loss_ref, g_ref, r_ref = B.objective(x, t, w, inv, pool, k)
    E_loss, E_g, E_r = B.bound(x, t, w, inv, pool, k)
    placements = [("aligned", dev)]
    if shape == (2, 3, 64, 64):
        placements += [("all one float off", shifted)]
    first = None
    for name, f in placements:
        xd, td, wd, kd = f(x), f(t), opt(w, f), f(k)
        g_out, r_out = f(torch.full(shape, float("nan"))), f(torch.full(t.shape, float("nan")))
        loss, g = restore_objective(xd, td, wd, opt(inv), pool, grad_out=g_out, psf=kd, resid_out=r_out)
        assert g is g_out
        ml, mg, mr = B.worst_multiple(loss, loss_ref, E_loss), B.worst_multiple(g, g_ref, E_g), B.worst_multiple(r_out, r_ref, E_r)
        print(f"{shape} psf {ksize} pool {pool} {'weighted' if weighted else 'ones'} {name}: worst multiple of the bound  "
              f"loss {ml:.3f}  grad {mg:.3f}  resid {mr:.3f}")
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(r_out).all())
        assert ml <= 1.0 and mg <= 1.0 and mr <= 1.0, (name, ml, mg, mr)
        if first is None:
            first = (g.clone(), r_out.clone())
        else:
            assert same_bits(g, first[0]) and same_bits(r_out, first[1]), f"{name}: bits differ from the aligned call's"


# ------------------------------------------------------------------------------------------------ 2. the kernel's properties
def test_a_point_source_leaves_the_psf_centred_and_not_flipped():
    """x = a single 1 per channel, unit weights: resid + t = A x is the PSF around the source, to the bound -- not its mirror image
    (the PSF has no symmetry; the mirrored one is far outside)."""
    k = B.asymmetric_psf(5, 3)
    x = torch.zeros((1, 2, 9, 8))
    x[0, :, 4, 3] = 1.0
    t = torch.rand((1, 2, 9, 8), generator=torch.Generator().manual_seed(3))
    r_out = dev(torch.zeros_like(t))
    restore_objective(dev(x), dev(t), psf=dev(k), resid_out=r_out)
    _, _, E_r = B.bound(x, t, None, None, 1, k)
    ax = r_out.cpu().double() + t.double()
    E = E_r + R.U * (ax.abs() + t.double().abs())      # (the test's own addition of t, in fp64 of fp32 values: far below this)
    ref = torch.zeros_like(ax)
    ref[0, :, 2:7, 2:5] = k.double()
    assert bool(((ax - ref).abs() <= E).all())
    mirrored = torch.zeros_like(ax)
    mirrored[0, :, 2:7, 2:5] = k.double().flip(0, 1)
    assert not bool(((ax - mirrored).abs() <= E).all())


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (2, 1, 5, 7)], ids=["64x64", "5x7"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "ones"])
def test_a_1x1_psf_of_one_at_pool_1_gives_the_bits_of_restore_objective(shape, weighted):
    """The anchor: a product by 1.0 and a one-term sum round nothing, and the cell's value is formed in `restore_cell`'s order, so
    loss and grad_x are glowhip_restore_objective's, bit for bit (both calls take the same 16-byte or element path: the buffers are
    placed alike); the residual is w (x - t) rounded as the kernel rounds it."""
    x, t, w, inv = R.objective_inputs(shape, 1, weighted)
    xd, td, wd, invd = dev(x), dev(t), opt(w), opt(inv)
    loss0, g0 = restore_objective(xd, td, wd, invd, 1)
    for psf in (torch.ones(1, 1), torch.ones(shape[0], 1, 1)):
        r_out = torch.full_like(td, float("nan"))
        loss1, g1 = restore_objective(xd, td, wd, invd, 1, psf=dev(psf), resid_out=r_out)
        assert same_bits(g1, g0), "grad_x differs from glowhip_restore_objective's"
        assert same_bits(loss1, loss0), "loss differs from glowhip_restore_objective's"
        d = x - t
        assert same_bits(r_out.cpu(), d if w is None else w * d)


@pytest.mark.parametrize("shape,ksize,pool", [((3, 3, 64, 64), (5, 5), 1), ((3, 3, 6, 10), (5, 3), 2)], ids=["tiles", "pool2"])
def test_zero_weight_sample_nan_sample_and_reproducibility(shape, ksize, pool):
    x, t, w, _, k = B.objective_inputs(shape, ksize, pool, True, True, seed=1)
    kd, td = dev(k), dev(t)

    def run(x_, w_, inv_):
        r = torch.full_like(td, float("nan"))
        loss, g = restore_objective(dev(x_), td, dev(w_), dev(inv_), pool, psf=kd, resid_out=r)
        return loss, g, r

    base = run(x, w, R.inv_wsum_of(w))
    again = run(x, w, R.inv_wsum_of(w))
    assert all(same_bits(a, b) for a, b in zip(base, again))                         # two runs of the same call: the same bits
    others = lambda out: [v[[0, 2]] for v in out]
    unchanged = lambda out: all(same_bits(a, b) for a, b in zip(others(out), others(base)))
    # a zero-weight sample: exact zeros, the others bit for bit what they were
    w0 = w.clone()
    w0[1] = 0.0
    out = run(x, w0, R.inv_wsum_of(w0))
    assert float(out[0][1]) == 0.0 and float(out[1][1].abs().max()) == 0.0 and float(out[2][1].abs().max()) == 0.0
    assert unchanged(out)
    # a NaN in one sample's x: that sample's loss and part of its gradient are NaN, the other samples' outputs unchanged
    xn = x.clone()
    xn[1, 0, 2, 3] = float("nan")
    out = run(xn, w, R.inv_wsum_of(w))
    assert bool(torch.isnan(out[0][1])) and bool(torch.isnan(out[1][1]).any())
    assert unchanged(out)
    # inv_wsum[n] == 0: exact zeros whatever x[n] holds -- the NaN included
    inv = R.inv_wsum_of(w)
    inv[1] = 0.0
    out = run(xn, w, inv)
    assert float(out[0][1]) == 0.0 and float(out[1][1].abs().max()) == 0.0 and float(out[2][1].abs().max()) == 0.0
    assert all(bool(torch.isfinite(v).all()) for v in out) and unchanged(out)
    # loss_out may be NULL, weight and inv_wsum too: the gradient is the same
    xd, gl, rl = dev(x), dev(torch.zeros(shape)), torch.zeros_like(td)
    rc = G.lib().glowhip_restore_objective_psf(xd.data_ptr(), td.data_ptr(), None, None, kd.data_ptr(), ksize[0] * ksize[1], *ksize,
                                               *shape, pool, rl.data_ptr(), gl.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    _, g1 = restore_objective(xd, td, None, None, pool, psf=kd)
    assert same_bits(gl, g1)


def test_wrong_tensors_are_refused_by_the_python_layer():
    x, t, w, inv, k = B.objective_inputs((2, 1, 5, 7), (3, 3), 1, True, False)
    xd, td = dev(x), dev(t)
    with pytest.raises(G._lib.GlowHipError, match="psf"):
        restore_objective(xd, td, psf=k)                                   # on the host
    with pytest.raises(G._lib.GlowHipError, match="psf"):
        restore_objective(xd, td, psf=dev(k.expand(3, 3, 3).contiguous()))  # three PSFs for a batch of two
    with pytest.raises(G._lib.GlowHipError, match="resid_out"):
        restore_objective(xd, td, psf=dev(k), resid_out=dev(torch.zeros(2, 1, 5, 6)))
    with pytest.raises(G._lib.GlowHipError, match="taps"):
        restore_objective(xd, td, psf=dev(torch.ones(4, 3)))                # an even side: the C call's refusal


# ------------------------------------------------------------------------------------------------ 3. first-iteration latent gradients
def setup(name):
    """(fit, ref, glow, inferer, measurement, weight, psf) of a `deblur_oracle.FITS` entry on the device: the target is the decode
    of the case's latents, the measurement the oracle's operator applied to it, the weight the valid band."""
    fit = B.FITS[name]
    ref = D.reference(**B.case_kwargs(fit["case"]))
    glow = make_glow(ref)
    inf = Inferer(D.hps_for(ref["cfg"], ref["cfg"]["batch"]), glow, [DEV], DEV)
    psf = B.gaussian_psf(5, 1.0)
    target = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    meas = B.operator(target.cpu().double(), psf.double(), fit["pool"]).float()
    weight = psf_valid_weight(meas.shape, 5, 5, fit["pool"]).expand_as(meas).contiguous()
    return fit, ref, glow, inf, dev(meas), dev(weight), dev(psf)


@pytest.mark.parametrize("name", list(B.FITS))
def test_latent_gradients_of_the_objective_vs_fp64_autograd_oracle(name):
    """decode -> objective with the 5x5 Gaussian PSF -> decode_vjp against fp64 autograd of the same objective through
    `O.flow_decode` and the oracle's operator, every entry within the project's gradient rule 2e-4 max|g| + 1e-7 per tensor
    (check_strict): the 16x16 model at pool 1, and case T (64x16, hidden 512) at pool 2.  The margins are held as
    tests/test_gpu_restore.py holds them."""
    fit = B.FITS[name]
    pool = fit["pool"]
    ref = D.reference(**B.case_kwargs(fit["case"]))
    if fit["case"] == "T":
        assert ref["margin"] >= SHAPE_MARGIN_FLOOR["T"], ref["margin"]
    else:
        assert_margin(ref)
    shape = tuple(ref["x"].shape)
    _, target, weight, inv = R.objective_inputs(shape, pool, True, seed=7)
    psf = B.gaussian_psf(5, 1.0)
    x_ref, loss_ref, gz_ref, geps_ref = B.latent_grads(ref["z"], ref["eps"], ref["sd"], ref["cfg"], target, weight, inv, pool, psf,
                                                       ref["tables"])
    glow = make_glow(ref)
    plan = plan_of(glow, ref)
    x, _ = plan.decode(dev(ref["z"]), [dev(e) for e in ref["eps"]])
    loss, gx = restore_objective(x, dev(target), dev(weight), dev(inv), pool, psf=dev(psf))
    gz, geps = plan.decode_vjp(x, gx)
    ex = float((x.cpu().double() - x_ref).abs().max())
    el = float(((loss.cpu().double() - loss_ref).abs() / loss_ref).max())
    print(f"{name}: margin {ref['margin']:.2e}, decode err {ex:.2e}, loss rel err {el:.2e}")
    assert ex <= 1e-4 and el <= 1e-4
    check_strict(dict(gz=gz_ref, geps=geps_ref), gz, geps, f"deblur {name}")


# ------------------------------------------------------------------------------------------------ 4. the loops
def test_fit_with_a_psf_captured_eager_and_hand_composed_agree_bitwise_without_a_sync_in_a_replay():
    """Four iterations with a prior term on the 16x16 case: the captured loop (one eager iteration, then three replays of one
    hipGraph), the eager loop, and the same iteration written out with `decode_latents`, `restore_objective(psf=)`, `decode_vjp`
    and `HipAdam.fused_step`: the same latents, loss history and norm history, bit for bit.  Then three replays under torch's sync
    debug mode: none makes a host sync."""
    fit_kw, ref, glow, inf, meas, weight, psf = setup("deblur")
    init = inf.encode_full(meas)
    lam = 1e-3
    args = dict(weight=weight, pool=1, init=init, steps=4, lr=0.05, prior_weight=lam, psf=psf)
    results = {}
    for name, graph in (("captured", True), ("eager", False)):
        fit = LatentFit(glow, meas, graph=graph, **args)
        assert fit.psf is not psf and same_bits(fit.psf, psf) and tuple(fit.resid.shape) == tuple(meas.shape)
        info = fit.run()
        assert isinstance(info, RestoreInfo) and info.finite and info.fallback == 0
        assert info.captured == graph, f"{name}: captured = {info.captured} ({info.graph_error})"
        results[name] = (fit.latents().tensors(), info.loss, info.grad_norm)
    plan = glow.flow.plan_for(meas)
    leaves = [t.clone().requires_grad_() for t in init.tensors()]
    optim = training.HipAdam(leaves, lr=0.05, weight_decay=lam)
    inv = 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0)
    losses, norms = [], []
    for _ in range(4):
        x = glow.decode_latents(Latents(leaves[0].detach(), [e.detach() for e in leaves[1:]]), safe=False)
        loss, gx = restore_objective(x, meas, weight, inv, 1, psf=psf)
        gz, geps = plan.decode_vjp(x, gx)
        for p, g in zip(leaves, [gz] + geps):
            p.grad = g
        norms.append(optim.fused_step(0.0, 0.0, skip_nonfinite=True).clone())
        losses.append(loss)
    results["by hand"] = ([p.detach() for p in leaves], torch.stack(losses).cpu(), torch.stack(norms).cpu())
    lat, loss, norm = results["captured"]
    print(f"loss {[f'{v:.4e}' for v in loss[:, 0].tolist()]} norm {[f'{v:.4e}' for v in norm.tolist()]}")
    assert not same_bits(lat[0], init.z) and float(loss.min()) > 0.0
    for name in ("eager", "by hand"):
        other = results[name]
        assert all(same_bits(a, b) for a, b in zip(lat, other[0])), f"{name}: latents differ from the captured loop's"
        assert same_bits(loss, other[1]) and same_bits(norm.view(-1), other[2].view(-1)), f"{name}: histories differ from the captured loop's"
    # the data term without the PSF is another problem: the plumbing is in use
    plain = LatentFit(glow, meas, graph=False, **dict(args, psf=None))
    assert plain.psf is None and plain.resid is None
    assert not same_bits(plain.run().loss, loss)
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
    hist = fit.loss_hist.cpu()
    assert float(hist[:5].min()) > 0.0 and float(hist[5:].abs().max()) == 0.0, hist[:, 0]
    assert same_bits(hist[:4], loss)


def test_chain_with_a_psf_is_a_function_of_its_seed_and_the_same_captured_and_eager():
    """Five iterations of `LatentMALA` on the blurred 16x16 measurement: one seed twice gives the same bits, and the captured
    chain's latents, histories, steps, counters, moments and image are the eager chain's, bit for bit; without the PSF the chain is
    another one."""
    fit_kw, ref, glow, inf, meas, weight, psf = setup("deblur")
    init = inf.encode_full(meas)
    args = dict(weight=weight, noise_std=0.2, init=init, steps=5, burn_in=3, thin=1, step_size=1e-3, seed=11, psf=psf)
    out = {}
    for name, graph in (("captured", True), ("eager", False), ("eager again", False), ("no psf", False)):
        mala = LatentMALA(glow, meas, graph=graph, **dict(args, psf=None if name == "no psf" else psf))
        info = mala.run()
        assert info.finite and info.captured == graph, f"{name}: captured = {info.captured} ({info.graph_error})"
        assert mala.iteration.tolist() == [5]
        out[name] = (*mala.latents().tensors(), mala.hist.clone(), mala.step.clone(), mala.counts.clone(), mala.mean.clone(),
                     mala.m2.clone(), mala.image.clone())
        print(name, "accepted", info.accepted.sum(dim=0).tolist(), "energy", [f"{v:.4e}" for v in info.energy[-1].tolist()])
    a = out["captured"]
    assert float(a[-6][0].abs().min()) > 0.0      # the energy history: every iteration was decided
    for name in ("eager", "eager again"):
        assert all(same_bits(x, y) for x, y in zip(a, out[name])), f"{name}: differs from the captured chain"
    assert not same_bits(a[-6], out["no psf"][-6]), "the chain without the PSF has the same energies: the PSF is not in use"


# ------------------------------------------------------------------------------------------------ 5. the fits
@pytest.mark.parametrize("name", list(B.FITS))
def test_restore_deblurs(name):
    """`Inferer.restore(psf=, border="valid")` from the default start (the latents of the blurred measurement; pool 2: of its
    upsampling): the 16x16 case with the 5x5 Gaussian at pool 1, 40 steps at lr 0.05, and case T (64x16, hidden 512) at pool 2, 20
    steps at lr 0.2.  Every sample's final / first data term <= the fp64 oracle's own worst ratio for the same fit rounded up to
    the next of 0.1 / 0.2 / 0.5 (tests/test_deblur_host.py; the oracle's samples: 0.031, 0.039, 0.027 -> 0.1 and 0.043, 0.050,
    0.049 -> 0.1).  The untrained models are no meaningful prior: the data term is all that is asserted."""
    fit, ref, glow, inf, meas, weight, psf = setup(name)
    pool = fit["pool"]
    lat, info = inf.restore(meas, pool=pool, steps=fit["steps"], lr=fit["lr"], psf=psf.cpu().numpy(), border="valid")
    hist = info.loss
    ratios = (hist[-1] / hist[0]).tolist()
    print(name, "loss of sample 0:", " ".join(f"{v:.3e}" for v in hist[:, 0].tolist()), "| final / first", [f"{r:.3f}" for r in ratios],
          "| captured", info.captured, info.graph_error)
    assert isinstance(lat, Latents) and tuple(hist.shape) == (fit["steps"], meas.shape[0]) and info.finite and info.fallback == 0
    assert info.captured, info.graph_error
    assert max(ratios) <= fit["ratio"], ratios
    # the history is the valid band's data term: the first entry is the objective of the start under that weight
    x0 = glow.decode_latents(inf.encode_full(meas if pool == 1 else meas.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1)),
                             safe=False)
    loss0, _ = restore_objective(x0, meas, weight, 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0), pool, psf=psf)
    assert same_bits(loss0.cpu(), hist[0])
    # the returned latents are the fitted ones: their decode's data term is below the first
    x = glow.decode_latents(lat, safe=False)
    loss, _ = restore_objective(x, meas, weight, 1.0 / weight.sum(dim=(1, 2, 3)).clamp(min=1.0), pool, psf=psf)
    assert bool((loss.cpu() < hist[0]).all())


# ------------------------------------------------------------------------------------------------ 6. the guards
def test_inferer_guards_and_psf_none_is_the_call_as_it_was():
    fit, ref, glow, inf, meas, weight, psf = setup("deblur")
    n = meas.shape[0]
    for bad in (torch.ones(4, 5), torch.ones(5, 4), torch.ones(17, 3), torch.ones(3, 17), torch.ones(n + 1, 3, 3), torch.ones(3)):
        with pytest.raises(ValueError):
            inf.restore(meas, steps=2, psf=bad)
        with pytest.raises(ValueError):
            inf.posterior(meas, steps=2, psf=bad)
    with pytest.raises(ValueError, match="border"):
        inf.restore(meas, steps=2, psf=psf, border="reflect")
    with pytest.raises(ValueError, match="no cell"):
        inf.restore(dev(torch.zeros(1, 3, 5, 7)), steps=2, psf=torch.ones(15, 15) / 225.0, border="valid")
    # border="zero" leaves the weight alone: another problem than the valid band's
    _, zero = inf.restore(meas, steps=2, lr=0.05, psf=psf, border="zero")
    _, valid = inf.restore(meas, steps=2, lr=0.05, psf=psf, border="valid")
    _, banded = inf.restore(meas, weight=weight, steps=2, lr=0.05, psf=psf, border="zero")
    assert not same_bits(zero.loss, valid.loss) and same_bits(banded.loss, valid.loss)
    # one PSF per sample, all the same, is the shared PSF's problem
    _, each = inf.restore(meas, steps=2, lr=0.05, psf=psf.expand(n, 5, 5), border="valid")
    assert same_bits(each.loss, valid.loss)
    # chains=K repeats a single PSF as it repeats the measurement
    lat, info = inf.posterior(meas[0], chains=2, noise_std=0.2, steps=3, burn_in=1, step_size=1e-3, seed=1, psf=psf[None])
    assert len(lat) == 2 and info.finite and tuple(info.energy.shape) == (3, 2)
    # psf=None: the in-painting fit of tests/test_gpu_restore.py, bit for bit what it is without the argument
    half = torch.zeros_like(meas)
    half[..., : meas.shape[-1] // 2] = 1.0
    init = inf.encode_full(meas * (1.0 - half))
    kw = dict(weight=half, steps=4, lr=0.2, init=init)
    lat_a, a = inf.restore(meas, **kw)
    lat_b, b = inf.restore(meas, psf=None, **kw)
    assert a.captured and b.captured
    assert same_bits(a.loss, b.loss) and same_bits(a.grad_norm, b.grad_norm)
    assert all(same_bits(p, q) for p, q in zip(lat_a.tensors(), lat_b.tensors()))

"""GPU tests of compressed sensing (-m gpu): glowhip_restore_objective_linear (csrc/restore_linear.hip) against the fp64 restatement
of tests/linear_oracle.py on every element of the loss, the gradient and the residual; the kernels' structural properties (the
bitwise anchor to glowhip_restore_objective with the identity, batch independence, reproducibility, zero-weight and NaN samples);
the latent gradient of the objective against fp64 autograd through `O.flow_decode`; `LatentFit` and `LatentMALA` with an operator,
captured against eager bit for bit; and `Inferer.restore(operator=gaussian_operator(...))` on the fit whose ratio
tests/test_linear_host.py fixes on the CPU.

The shapes sit where the kernels can go wrong, not at the workload's size (`linear_oracle.CASES`): the forward product's row tile is
8 rows and its D slice 4 096 columns, its SAMPLE TILE is 4; the adjoint's M slice is 128 rows and its sample block 64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd.network import Inferer, LatentFit, LatentMALA, Latents, RestoreInfo, gaussian_operator, restore_objective  # noqa: E402
from pytorch_glow_amd.network.restore import linear_scratch  # noqa: E402

import decode_grad_oracle as D  # noqa: E402
import linear_oracle as L  # noqa: E402
import restore_oracle as R  # noqa: E402
from test_decode_grad_host import SHAPE_MARGIN_FLOOR  # noqa: E402
from test_gpu_decode_grad import DEV, assert_margin, check_strict, dev, make_glow, plan_of  # noqa: E402

FORWARD_SAMPLE_TILE, ADJOINT_SAMPLE_BLOCK = 4, 64      # csrc/restore_linear.hip: LIN_NS, LIN_NB


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


def run(x, t, w, inv, A, f=dev):
    """One call on fresh NaN-filled outputs placed by ``f``: (loss, grad_x, resid)."""
    xd, td = f(x), f(t)
    g_out, r_out = f(torch.full(x.shape, float("nan"))), f(torch.full(t.shape, float("nan")))
    loss, g = restore_objective(xd, td, opt(w, f), opt(inv, f), 1, grad_out=g_out, resid_out=r_out, operator=A if A.is_cuda else f(A))
    assert g is g_out
    return loss, g, r_out


# ------------------------------------------------------------------------------------------------ 1. the objective, every element
@pytest.mark.parametrize("shape,m", L.CASES, ids=L.CASE_IDS)
def test_objective_every_element_vs_fp64_oracle(shape, m):
    """loss, grad_x and resid within `linear_oracle.bound`, which walks the fp32 roundings for ANY summation order: D u (|A| |x|) for
    y, then d, w d, the scaling and the loss as `restore_oracle.bound` does, and the adjoint's own M-term sum over the cells' values
    and their errors.  tests/test_linear_host.py shows a float32 restatement of those sums, in two orders, inside the bound on these
    inputs: nothing here was tuned on the device.  Batches of 1, 3 and 5 (below and above the forward product's sample tile of 4),
    67 (above the adjoint's sample block of 64) where the operator is small and once at the largest shape, weighted and with unit
    weights.  The largest shape also runs with every pointer -- the operator's and the residual's included -- one float off a
    16-byte address: the same bound, and the same gradient and residual bits.  (Worst multiples seen on an MI355X: loss 0.023,
    gradient 0.030, residual 0.036 -- a bound over every summation order is wide for sums reduced as trees.)"""
    assert L.BATCHES[-1] > FORWARD_SAMPLE_TILE and L.BATCH_ABOVE_THE_SAMPLE_BLOCK > ADJOINT_SAMPLE_BLOCK
    worst = [0.0, 0.0, 0.0]
    for n in L.batches_of(shape, m):
        for weighted in (True, False):
            x, t, w, inv, A = L.objective_inputs(n, shape, m, weighted)
            loss_ref, g_ref, r_ref = L.objective(x, t, w, inv, A)
            E_loss, E_g, E_r = L.bound(x, t, w, inv, A)
            placements = [("aligned", dev)]
            if (shape, m, n) == (L.IMAGE_SHAPES[-1], L.ROWS[-1], L.BATCHES[-1]):
                placements += [("all one float off", shifted)]
            first = None
            for name, f in placements:
                loss, g, r = run(x, t, w, inv, A, f)
                ml, mg, mr = L.worst_multiple(loss, loss_ref, E_loss), L.worst_multiple(g, g_ref, E_g), L.worst_multiple(r, r_ref, E_r)
                print(f"{shape} M {m} N {n} {'weighted' if weighted else 'ones'} {name}: worst multiple of the bound  "
                      f"loss {ml:.3f}  grad {mg:.3f}  resid {mr:.3f}")
                assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(r).all())
                assert ml <= 1.0 and mg <= 1.0 and mr <= 1.0, (n, weighted, name, ml, mg, mr)
                worst = [max(a, b) for a, b in zip(worst, (ml, mg, mr))]
                if first is None:
                    first = (g.clone(), r.clone())
                else:
                    assert same_bits(g, first[0]) and same_bits(r, first[1]), f"{name}: bits differ from the aligned call's"
    print(f"{shape} M {m}: worst multiple over the case  loss {worst[0]:.3f}  grad {worst[1]:.3f}  resid {worst[2]:.3f}")


# ------------------------------------------------------------------------------------------------ 2. the kernels' properties
@pytest.mark.parametrize("shape", [(2, 1, 5, 7), (3, 3, 8, 8)], ids=["D35", "D192"])
@pytest.mark.parametrize("weights", ["positive", "with zeros", "ones"])
def test_the_identity_operator_gives_the_bits_of_restore_objective(shape, weights):
    """The anchor: products with +-0 and one-term sums round nothing, the cell's value is formed in `restore_cell`'s order and the
    loss is summed in k_restore_objective's, so loss and grad_x are glowhip_restore_objective's at pool 1, bit for bit (both calls
    read the same x, target and weight and write buffers placed alike: the same 16-byte or element path per sample -- at D = 35 the
    second sample is off the boundary); the residual is w (x - t) rounded as the kernel rounds it.
    The one thing a sum cannot carry is the SIGN of an exact zero: where w == 0 and x < t, glowhip_restore_objective returns
    2 inv (w d) = -0, and here that -0 meets the +0 products of the identity's other rows, -0 + +0 = +0 (IEEE 754).  "with zeros"
    (every seventh weight an exact zero) therefore compares the gradient with both zeros written as +0 -- every other bit, and
    the loss and the residual as they stand; "positive" and "ones" have no such cell and compare every bit."""
    x, t, w, inv = R.objective_inputs(shape, 1, weights != "ones")
    if weights == "positive":
        w = torch.where(w == 0, torch.full_like(w, 0.5), w)
        inv = R.inv_wsum_of(w)
        assert float(((w * (x - t)) == 0).sum()) == 0
    n, dim = shape[0], x[0].numel()
    xd, td, wd, invd = dev(x), dev(t), opt(w), opt(inv)
    loss0, g0 = restore_objective(xd, td, wd, invd, 1)
    eye = dev(torch.eye(dim).view(dim, *shape[1:]).contiguous())
    r_out = torch.full((n, dim), float("nan"), device=DEV)
    loss1, g1 = restore_objective(xd, td.view(n, dim), None if wd is None else wd.view(n, dim), invd, 1, operator=eye, resid_out=r_out)
    if weights == "with zeros":
        assert int((bits(g0) == -2 ** 31).sum()) > 0 and bool((g1[g0 == 0] == 0).all())      # (the case is there: some -0 in g0)
        g0, g1 = g0 + 0.0, g1 + 0.0
    assert same_bits(g1, g0), "grad_x differs from glowhip_restore_objective's"
    assert same_bits(loss1, loss0), "loss differs from glowhip_restore_objective's"
    d = x - t
    assert same_bits(r_out.cpu().view(shape), d if w is None else w * d)


@pytest.mark.parametrize("shape,m", [((1, 5, 7), 67), ((3, 64, 64), 130)], ids=["D35-M67", "D12288-M130"])
def test_a_sample_has_the_same_bits_alone_and_in_a_batch_of_five(shape, m):
    """Slice counts and tile shapes are functions of (M, D), never of N, and no sum mixes samples: sample n of a batch of 5 -- two
    sample tiles of the forward product -- has the bits of the same sample run as a batch of one (views at the same addresses, so
    that the residual pass takes the same access path)."""
    x, t, w, inv, A = L.objective_inputs(5, shape, m, True, seed=2)
    xd, td, wd, invd, Ad = dev(x), dev(t), dev(w), dev(inv), dev(A)
    nan = lambda s: torch.full(s, float("nan"), device=DEV)
    g5, r5, l5 = nan(x.shape), nan(t.shape), nan((5,))
    restore_objective(xd, td, wd, invd, 1, grad_out=g5, loss_out=l5, resid_out=r5, operator=Ad)
    g1, r1, l1 = nan(x.shape), nan(t.shape), nan((5,))
    for k in range(5):
        s = slice(k, k + 1)
        restore_objective(xd[s], td[s], wd[s], invd[s], 1, grad_out=g1[s], loss_out=l1[s], resid_out=r1[s], operator=Ad)
    assert same_bits(g1, g5) and same_bits(r1, r5) and same_bits(l1, l5)
    # whatever its neighbours hold: the others replaced by other images
    x2 = torch.rand(x.shape, generator=torch.Generator().manual_seed(9))
    x2[3] = x[3]
    _, g, r = run(x2, t, w, inv, Ad)
    assert same_bits(g[3], g5[3]) and same_bits(r[3], r5[3]) and not same_bits(g[2], g5[2])


@pytest.mark.parametrize("shape,m", [((3, 64, 64), 130), ((1, 5, 7), 3)], ids=["D12288-M130", "D35-M3"])
def test_zero_weight_sample_nan_sample_and_reproducibility(shape, m):
    n = 5      # samples 0 .. 3 share a sample tile of the forward product -- and a lane's registers in both products
    x, t, w, _, A = L.objective_inputs(n, shape, m, True, seed=1)
    Ad = dev(A)
    base = run(x, t, w, L.inv_wsum_of(w), Ad)
    again = run(x, t, w, L.inv_wsum_of(w), Ad)
    assert all(same_bits(a, b) for a, b in zip(base, again))                         # two runs of the same call: the same bits
    keep = [0, 2, 3, 4]
    others = lambda out: [v[keep] for v in out]
    unchanged = lambda out: all(same_bits(a, b) for a, b in zip(others(out), others(base)))
    # a zero-weight sample: exact zeros, the others bit for bit what they were
    w0 = w.clone()
    w0[1] = 0.0
    out = run(x, t, w0, L.inv_wsum_of(w0), Ad)
    assert float(out[0][1]) == 0.0 and float(out[1][1].abs().max()) == 0.0 and float(out[2][1].abs().max()) == 0.0
    assert unchanged(out)
    # a NaN in one sample's x: that sample's loss and gradient are NaN, the other samples' outputs unchanged
    xn = x.clone()
    xn[1, 0, 2, 3] = float("nan")
    out = run(xn, t, w, L.inv_wsum_of(w), Ad)
    assert bool(torch.isnan(out[0][1])) and bool(torch.isnan(out[1][1]).any())
    assert unchanged(out)
    # inv_wsum[n] == 0: exact zeros whatever x[n] holds -- the NaN included
    inv = L.inv_wsum_of(w)
    inv[1] = 0.0
    out = run(xn, t, w, inv, Ad)
    assert float(out[0][1]) == 0.0 and float(out[1][1].abs().max()) == 0.0 and float(out[2][1].abs().max()) == 0.0
    assert all(bool(torch.isfinite(v).all()) for v in out) and unchanged(out)
    # loss_out may be NULL, weight and inv_wsum too: the gradient is the same
    xd, td = dev(x), dev(t)
    gl, rl = torch.zeros_like(xd), torch.zeros_like(td)
    scratch = linear_scratch(n, m, A[0].numel(), xd.device)
    rc = G.lib().glowhip_restore_objective_linear(xd.data_ptr(), td.data_ptr(), None, None, Ad.data_ptr(), m, n, A[0].numel(),
                                                  rl.data_ptr(), gl.data_ptr(), None, scratch.data_ptr(), scratch.numel(),
                                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    _, g1 = restore_objective(xd, td, None, None, 1, operator=Ad, scratch=scratch)
    assert same_bits(gl, g1)


def test_wrong_tensors_are_refused_by_the_python_layer():
    x, t, w, inv, A = L.objective_inputs(2, (1, 5, 7), 3, True)
    xd, td, Ad = dev(x), dev(t), dev(A)
    with pytest.raises(G._lib.GlowHipError, match="operator"):
        restore_objective(xd, td, operator=A)                                             # on the host
    with pytest.raises(G._lib.GlowHipError, match="operator"):
        restore_objective(xd, td, operator=dev(torch.zeros(3, 1, 5, 6)))                  # another image shape
    with pytest.raises(G._lib.GlowHipError, match="psf"):
        restore_objective(xd, td, operator=Ad, psf=dev(torch.ones(3, 3)))
    with pytest.raises(G._lib.GlowHipError, match="pool"):
        restore_objective(dev(torch.zeros(2, 1, 4, 8)), td, pool=2, operator=dev(torch.zeros(3, 1, 4, 8)))
    with pytest.raises(G._lib.GlowHipError, match="target"):
        restore_objective(xd, dev(torch.zeros(2, 4)), operator=Ad)
    with pytest.raises(G._lib.GlowHipError, match="resid_out"):
        restore_objective(xd, td, operator=Ad, resid_out=dev(torch.zeros(2, 4)))
    with pytest.raises(G._lib.GlowHipError, match="scratch"):
        restore_objective(xd, td, operator=Ad, scratch=torch.zeros(16, dtype=torch.uint8, device=DEV))      # too small: the C call's refusal
    with pytest.raises(G._lib.GlowHipError, match="scratch"):
        restore_objective(xd, dev(torch.zeros(2, 1, 5, 7)), scratch=torch.zeros(16, dtype=torch.uint8, device=DEV))      # no operator


# ------------------------------------------------------------------------------------------------ 3. first-iteration latent gradients
@pytest.mark.parametrize("case", ["tiny", "T"], ids=["16x16", "64x16-hidden512"])
def test_latent_gradients_of_the_objective_vs_fp64_autograd_oracle(case):
    """decode -> objective through 67 Gaussian rows -> decode_vjp against fp64 autograd of the same objective through
    `O.flow_decode` and the oracle's operator, every entry within the project's gradient rule 2e-4 max|g| + 1e-7 per tensor
    (check_strict): the 16x16 model, and case T (64x16, hidden 512).  The margins are held as tests/test_gpu_restore.py holds them."""
    ref = D.reference(**L.case_kwargs(case))
    if case == "T":
        assert ref["margin"] >= SHAPE_MARGIN_FLOOR["T"], ref["margin"]
    else:
        assert_margin(ref)
    n, chw = ref["x"].shape[0], tuple(ref["x"].shape[1:])
    _, target, weight, inv, A = L.objective_inputs(n, chw, 67, True, seed=7)
    x_ref, loss_ref, gz_ref, geps_ref = L.latent_grads(ref["z"], ref["eps"], ref["sd"], ref["cfg"], target, weight, inv, A, ref["tables"])
    glow = make_glow(ref)
    plan = plan_of(glow, ref)
    x, _ = plan.decode(dev(ref["z"]), [dev(e) for e in ref["eps"]])
    loss, gx = restore_objective(x, dev(target), dev(weight), dev(inv), 1, operator=dev(A))
    gz, geps = plan.decode_vjp(x, gx)
    ex = float((x.cpu().double() - x_ref).abs().max())
    el = float(((loss.cpu().double() - loss_ref).abs() / loss_ref).max())
    print(f"{case}: margin {ref['margin']:.2e}, decode err {ex:.2e}, loss rel err {el:.2e}")
    assert ex <= 1e-4 and el <= 1e-4
    check_strict(dict(gz=gz_ref, geps=geps_ref), gz, geps, f"linear {case}")


# ------------------------------------------------------------------------------------------------ 4. the loops
def setup():
    """(fit, ref, glow, inferer, measurement, operator) of `linear_oracle.FIT` on the device: the unknown image is the decode of the
    case's latents, the operator `gaussian_operator` made on the device, the measurement the oracle's operator applied in fp64."""
    fit = L.FIT
    ref = D.reference(**L.case_kwargs(fit["case"]))
    glow = make_glow(ref)
    inf = Inferer(D.hps_for(ref["cfg"], ref["cfg"]["batch"]), glow, [DEV], DEV)
    target = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    A = gaussian_operator(fit["m"], tuple(target.shape[1:]), fit["seed"], DEV)
    meas = L.operator(target.cpu().double(), A.cpu().double()).float()
    return fit, ref, glow, inf, dev(meas), A


def zero_latents(glow, ref, n):
    plan = plan_of(glow, ref)
    zeros = lambda chw: torch.zeros((n,) + tuple(chw), device=DEV)
    return Latents(zeros(plan.out_chw), [zeros(chw) for chw in plan.split_chw])


def test_gaussian_operator_is_the_named_stream_and_never_leaves_the_device():
    """stream 248 at (seed, call 0), element = flat index, times float32(1 / sqrt(m)): the device matrix against the CPU restatement
    within the sampler's bar (1e-5 on a unit normal, tests/test_gpu_sampler.py) scaled by the std; a function of its name."""
    m, shape = 48, (3, 16, 16)
    a = gaussian_operator(m, shape, 11, DEV)
    assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (m,) + shape and a.is_contiguous()
    ref = L.gaussian_operator(m, shape, 11)
    err = float((a.cpu().double() - ref).abs().max())
    print(f"max |device - oracle| {err:.2e} (bar {1e-5 / m ** 0.5:.2e})")
    assert err <= 1e-5 / m ** 0.5
    assert same_bits(a, gaussian_operator(m, shape, 11, DEV)) and not same_bits(a, gaussian_operator(m, shape, 12, DEV))


def test_fit_with_an_operator_captured_eager_and_hand_composed_agree_bitwise_without_a_sync_in_a_replay():
    """Four iterations with a prior term on the 16x16 case from the all-zero latents: the captured loop (one eager iteration, then
    three replays of one hipGraph), the eager loop, and the same iteration written out with `decode_latents`,
    `restore_objective(operator=)`, `decode_vjp` and `HipAdam.fused_step`: the same latents, loss history and norm history, bit for
    bit.  Then three replays under torch's sync debug mode: none makes a host sync.  The loop holds the operator by reference."""
    from pytorch_glow_amd import training
    fit_kw, ref, glow, inf, meas, A = setup()
    n = meas.shape[0]
    init = zero_latents(glow, ref, n)
    lam = 1e-3
    args = dict(init=init, steps=4, lr=0.1, prior_weight=lam, operator=A)
    results = {}
    for name, graph in (("captured", True), ("eager", False)):
        fit = LatentFit(glow, meas, graph=graph, **args)
        assert fit.operator is A and tuple(fit.resid.shape) == tuple(meas.shape) and fit.op_scratch is not None and fit.psf is None
        assert tuple(fit.image.shape) == (n,) + tuple(A.shape[1:])
        info = fit.run()
        assert isinstance(info, RestoreInfo) and info.finite and info.fallback == 0
        assert info.captured == graph, f"{name}: captured = {info.captured} ({info.graph_error})"
        results[name] = (fit.latents().tensors(), info.loss, info.grad_norm)
    plan = plan_of(glow, ref)
    leaves = [t.clone().requires_grad_() for t in init.tensors()]
    optim = training.HipAdam(leaves, lr=0.1, weight_decay=lam)
    losses, norms = [], []
    for _ in range(4):
        x = glow.decode_latents(Latents(leaves[0].detach(), [e.detach() for e in leaves[1:]]), safe=False)
        loss, gx = restore_objective(x, meas, None, None, 1, operator=A)
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


def test_chain_with_an_operator_is_a_function_of_its_seed_and_the_same_captured_and_eager():
    """Five iterations of `LatentMALA` on the compressed measurement from the all-zero latents: one seed twice gives the same bits,
    and the captured chain's latents, histories, steps, counters, moments and image are the eager chain's, bit for bit; another
    operator gives another chain."""
    fit_kw, ref, glow, inf, meas, A = setup()
    init = zero_latents(glow, ref, meas.shape[0])
    other = gaussian_operator(fit_kw["m"], tuple(A.shape[1:]), fit_kw["seed"] + 1, DEV)
    args = dict(noise_std=0.2, init=init, steps=5, burn_in=3, thin=1, step_size=1e-3, seed=11)
    out = {}
    for name, graph in (("captured", True), ("eager", False), ("eager again", False), ("another operator", False)):
        mala = LatentMALA(glow, meas, graph=graph, operator=other if name == "another operator" else A, **args)
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
    assert not same_bits(a[-6], out["another operator"][-6]), "another operator gives the same energies: the operator is not in use"


# ------------------------------------------------------------------------------------------------ 5. the fit
def test_restore_recovers_from_compressed_measurements():
    """`Inferer.restore(t, operator=gaussian_operator(256, (3,16,16), 7))` from the default start -- the all-zero latents -- on the
    16x16x3 model (D = 768, M = D / 3), 40 steps at lr 0.1.  Every sample's final / first data term <= 0.1: the smallest of 0.1 /
    0.2 / 0.5 that is at least twice the fp64 oracle's own worst ratio for the same fit (tests/test_linear_host.py: 0.0034, 0.0041,
    0.0037).  The untrained model is no meaningful prior: the data term is all that is asserted."""
    fit, ref, glow, inf, meas, A = setup()
    lat, info = inf.restore(meas, steps=fit["steps"], lr=fit["lr"], operator=A)
    hist = info.loss
    ratios = (hist[-1] / hist[0]).tolist()
    print("loss of sample 0:", " ".join(f"{v:.3e}" for v in hist[:, 0].tolist()), "| final / first", [f"{r:.4f}" for r in ratios],
          "| captured", info.captured, info.graph_error)
    assert isinstance(lat, Latents) and tuple(hist.shape) == (fit["steps"], meas.shape[0]) and info.finite and info.fallback == 0
    assert info.captured, info.graph_error
    assert max(ratios) <= fit["ratio"], ratios
    # the history's first entry is the objective of the zero start, and the device's start is the oracle's
    x0 = glow.decode_latents(zero_latents(glow, ref, meas.shape[0]), safe=False)
    loss0, _ = restore_objective(x0, meas, None, None, 1, operator=A)
    assert same_bits(loss0.cpu(), hist[0])
    first = L.fit_case()["history"][0]
    assert float(((hist[0].double() - first).abs() / first).max()) <= 1e-3
    # the returned latents are the fitted ones: their decode's data term is below the first
    loss, _ = restore_objective(glow.decode_latents(lat, safe=False), meas, None, None, 1, operator=A)
    assert bool((loss.cpu() < hist[0]).all())
    # a single problem given as (M,): a batch of one
    lat1, info1 = inf.restore(meas[0], steps=2, lr=fit["lr"], operator=A)
    assert len(lat1) == 1 and tuple(info1.loss.shape) == (2, 1) and info1.finite and float(info1.loss.min()) > 0.0


# ------------------------------------------------------------------------------------------------ 6. the guards
def test_inferer_guards_posterior_chains_and_operator_none_is_the_call_as_it_was():
    fit, ref, glow, inf, meas, A = setup()
    n, m = meas.shape
    for kw in (dict(psf=torch.ones(3, 3)), dict(pool=2), dict(weight=torch.ones(n, m - 1)), dict(operator=A[:, :, :, :8].contiguous()),
               dict(operator=A.view(m, -1)), dict(operator=A.cpu())):
        with pytest.raises(ValueError):
            inf.restore(meas, steps=2, **dict(dict(operator=A), **kw))
        with pytest.raises(ValueError):
            inf.posterior(meas, steps=2, **dict(dict(operator=A), **kw))
    with pytest.raises(ValueError):
        inf.restore(meas[:, :-1], steps=2, operator=A)
    with pytest.raises(ValueError, match="chains"):
        inf.posterior(meas, chains=2, steps=2, operator=A)
    # a weight broadcast from (M,) is the (N, M) weight's problem
    wrow = torch.rand(m, generator=torch.Generator().manual_seed(4))
    _, a = inf.restore(meas, weight=wrow, steps=2, lr=0.1, operator=A)
    _, b = inf.restore(meas, weight=wrow.expand(n, m), steps=2, lr=0.1, operator=A)
    assert same_bits(a.loss, b.loss)
    # chains=K repeats the measurement and shares the one operator; the moments are finite
    lat, info = inf.posterior(meas[0], chains=2, noise_std=0.2, steps=4, burn_in=1, step_size=1e-3, seed=1, operator=A)
    assert len(lat) == 2 and info.finite and tuple(info.energy.shape) == (4, 2) and info.count == 3
    assert tuple(info.mean.shape) == (2,) + tuple(A.shape[1:])
    assert all(bool(torch.isfinite(v).all()) for v in (info.mean, info.std, info.pooled_mean, info.pooled_std, info.energy))
    # operator=None: the in-painting fit of tests/test_gpu_restore.py, bit for bit what it is without the argument
    image = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    half = torch.zeros_like(image)
    half[..., : image.shape[-1] // 2] = 1.0
    init = inf.encode_full(image * (1.0 - half))
    kw = dict(weight=half, steps=4, lr=0.2, init=init)
    lat_a, a = inf.restore(image, **kw)
    lat_b, b = inf.restore(image, operator=None, **kw)
    assert a.captured and b.captured
    assert same_bits(a.loss, b.loss) and same_bits(a.grad_norm, b.grad_norm)
    assert all(same_bits(p, q) for p, q in zip(lat_a.tensors(), lat_b.tensors()))
    # ... and its first loss is the fp64 in-painting oracle's (tests/restore_oracle.py: the parent's own yardstick)
    first = R.fit_case("inpaint")["history"][0]
    assert float(((a.loss[0].double() - first).abs() / first).max()) <= 1e-3

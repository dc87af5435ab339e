"""GPU tests of Fourier-domain measurements (-m gpu): glowhip_restore_objective_fourier and glowhip_fourier2d
(csrc/restore_fourier.hip) against the fp64 restatement of tests/fourier_oracle.py on every element of the loss, the gradient and the
residual; the kernels' structural properties (batch independence, reproducibility, zero-weight and NaN samples, refusals that touch
nothing); Parseval against glowhip_restore_objective; the latent gradient of the objective against fp64 autograd through
`O.flow_decode`; `LatentFit` and `LatentMALA` with ``fourier=True``, captured against eager bit for bit; and
`Inferer.restore(kspace, weight=fourier_mask(...), fourier=True)` on the fit whose ratio tests/test_fourier_host.py fixes on the CPU.

The shapes sit where the kernels can go wrong, not at the workload's size (`fourier_oracle.SHAPES`): one stage; H != W both ways;
row tiles of several rows and column tiles of 32; the longest row and column against the shortest; and 256 x 256, the plane that does
not fit in LDS (row tiles of 8 rows, column tiles of 16 columns with the half-line layout)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd.network import (Inferer, LatentFit, LatentMALA, Latents, RestoreInfo, fourier2d, fourier2d_adjoint,  # noqa: E402
                                      fourier_mask, fourier_scratch, restore_objective)

import decode_grad_oracle as D  # noqa: E402
import fourier_oracle as F  # noqa: E402
import restore_oracle as R  # noqa: E402
from test_gpu_decode_grad import DEV, assert_margin, check_strict, dev, make_glow, plan_of  # noqa: E402
from test_gpu_linear import bits, same_bits, shifted  # noqa: E402

opt = lambda v, f=dev: None if v is None else f(v)
real = lambda t: torch.view_as_real(t.contiguous())      # complex64 (..., H, W) -> fp32 (..., H, W, 2)


def run(x, t, w, inv, f=dev):
    """One call on fresh NaN-filled outputs placed by ``f``: (loss, grad_x, resid fp32 (N,C,H,W,2))."""
    xd, td = f(x), f(real(t))
    g_out, r_out = f(torch.full(x.shape, float("nan"))), f(torch.full(td.shape, float("nan")))
    loss, g = restore_objective(xd, td, opt(w, f), opt(inv, f), 1, grad_out=g_out, resid_out=r_out, fourier=True)
    assert g is g_out
    return loss, g, r_out


# ------------------------------------------------------------------------------------------------ 1. the objective, every element
@pytest.mark.parametrize("shape", F.SHAPES, ids=F.SHAPE_IDS)
def test_objective_every_element_vs_fp64_oracle(shape):
    """loss, grad_x and resid (the modulus of the complex difference) within `fourier_oracle.bound`, which walks the fp32 roundings
    of a radix-2 transform of log2 H + log2 W stages in norms (Higham's per-stage constant), the scaling, the subtraction, the
    weighting and the loss, for any butterfly order.  tests/test_fourier_host.py shows a float32 restatement of the transform, in the
    kernels' butterfly order and in the opposite one, inside the bound on these inputs: nothing here was tuned on the device.
    Batches of 1, 3 and 5 (and 67 at 3x4x8: the kernels block over planes only, so there is no sample block to exceed); a 0/1 mask,
    real weights with exact zeros, and NULL.  The largest case also runs with every pointer one float off a 16-byte address: the
    same bound, and the same gradient and residual bits.  (Worst multiples of the bound seen on an MI355X: loss 0.069, gradient
    0.028, residual 0.067, all three at 1x2x2; at 1x256x256 0.005, below 0.001 and 0.009 -- a worst-case bound over log2 H + log2 W stages
    is wide for roundings that add like a random walk.)"""
    worst = [0.0, 0.0, 0.0]
    for n in F.batches_of(shape):
        for weights in F.WEIGHTS:
            x, t, w, inv = F.objective_inputs(n, shape, weights)
            loss_ref, g_ref, r_ref = F.objective(x, t, w, inv)
            E_loss, E_g, E_r = F.bound(x, t, w, inv)
            placements = [("aligned", dev)]
            if (shape, n) == (F.SHAPES[-1], F.BATCHES[-1]):
                placements += [("all one float off", shifted)]
            first = None
            for name, f in placements:
                loss, g, r = run(x, t, w, inv, f)
                ml, mg = F.worst_multiple(loss, loss_ref, E_loss), F.worst_multiple(g, g_ref, E_g)
                mr = F.complex_multiple(r, r_ref, E_r)
                print(f"{shape} N {n} {weights} {name}: worst multiple of the bound  loss {ml:.3f}  grad {mg:.3f}  resid {mr:.3f}")
                assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(r).all())
                assert ml <= 1.0 and mg <= 1.0 and mr <= 1.0, (n, weights, name, ml, mg, mr)
                worst = [max(a, b) for a, b in zip(worst, (ml, mg, mr))]
                if first is None:
                    first = (g.clone(), r.clone())
                else:
                    assert same_bits(g, first[0]) and same_bits(r, first[1]), f"{name}: bits differ from the aligned call's"
    print(f"{shape}: worst multiple over the case  loss {worst[0]:.3f}  grad {worst[1]:.3f}  resid {worst[2]:.3f}")


# ------------------------------------------------------------------------------------------------ 2. the transform alone
@pytest.mark.parametrize("shape", F.SHAPES, ids=F.SHAPE_IDS)
def test_fourier2d_forward_adjoint_round_trip_and_adjoint_identity(shape):
    """glowhip_fourier2d both ways against fp64 within `fourier_oracle.fourier2d_bound` on every element; adjoint(forward(x)) = x
    within the two bounds chained (the forward's error carried by the unitary adjoint with at most its plane's norm, bounded as a
    vector: `fourier_oracle.fourier2d_norm_bound`); <F x, k> = <x, Re F^H k> within what those vector bounds allow."""
    c, h, w = shape
    g = torch.Generator().manual_seed(77)
    x = torch.rand((3, c, h, w), generator=g)
    k = torch.complex(torch.randn(x.shape, generator=g), torch.randn(x.shape, generator=g))
    xd, kd = dev(x), dev(k)
    X = fourier2d(xd)
    assert X.dtype == torch.complex64 and tuple(X.shape) == tuple(x.shape)
    E_f = F.fourier2d_bound(x, h, w)
    mf = F.complex_multiple(X, F.forward(x), E_f)
    a = fourier2d_adjoint(kd)
    assert a.dtype == torch.float32 and tuple(a.shape) == tuple(x.shape)
    E_a = F.fourier2d_bound(k, h, w)
    ma = F.worst_multiple(a, F.adjoint(k), E_a)
    # the round trip: the adjoint's own bound on the exact spectrum, plus the forward's whole error -- bounded as a vector -- which
    # the unitary adjoint carries into any element with at most its 2-norm
    back = fourier2d_adjoint(X)
    E_b = F.fourier2d_bound(F.forward(x), h, w) + F.fourier2d_norm_bound(x, h, w)
    mb = F.worst_multiple(back, x.double(), E_b)
    print(f"{shape}: worst multiple of the bound  forward {mf:.3f}  adjoint {ma:.3f}  round trip {mb:.3f}")
    assert mf <= 1.0 and ma <= 1.0 and mb <= 1.0
    # the adjoint identity on the device's own results, summed in fp64
    lhs = float((F.as_complex(X.cpu()).conj() * F.as_complex(k)).real.sum())
    rhs = float((x.double() * a.cpu().double()).sum())
    pnorm = lambda v: (v.abs() ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()      # Cauchy-Schwarz, plane by plane
    slack = float((F.fourier2d_norm_bound(x, h, w) * pnorm(F.as_complex(k)) + F.fourier2d_norm_bound(k, h, w) * pnorm(x.double())).sum())
    print(f"{shape}: <F x, k> - <x, Re F^H k> = {lhs - rhs:.3e} (allowed {slack:.3e})")
    assert abs(lhs - rhs) <= slack
    # a real buffer with a trailing 2 is the same call; out= is written in place
    buf = torch.full(tuple(x.shape) + (2,), float("nan"), device=DEV)
    assert same_bits(torch.view_as_real(fourier2d(xd, out=buf)), buf) and same_bits(buf, torch.view_as_real(X))
    assert same_bits(fourier2d_adjoint(torch.view_as_real(kd).contiguous()), a)


# ------------------------------------------------------------------------------------------------ 3. the kernels' properties
@pytest.mark.parametrize("shape", [(3, 4, 8), (3, 64, 64), (1, 256, 256)], ids=["3x4x8", "3x64x64", "1x256x256"])
def test_a_sample_has_the_same_bits_alone_and_in_a_batch_of_five(shape):
    """Tile shapes and the butterfly order are functions of (H, W), never of N, and a workgroup works on one plane of one sample:
    sample n of a batch of 5 has the bits of the same sample run as a batch of one."""
    x, t, w, inv = F.objective_inputs(5, shape, "real", seed=2)
    xd, td, wd, invd = dev(x), dev(real(t)), dev(w), dev(inv)
    nan = lambda s: torch.full(tuple(s), float("nan"), device=DEV)
    g5, r5, l5 = nan(x.shape), nan(td.shape), nan((5,))
    restore_objective(xd, td, wd, invd, 1, grad_out=g5, loss_out=l5, resid_out=r5, fourier=True)
    g1, r1, l1 = nan(x.shape), nan(td.shape), nan((5,))
    for k in range(5):
        s = slice(k, k + 1)
        restore_objective(xd[s], td[s], wd[s], invd[s], 1, grad_out=g1[s], loss_out=l1[s], resid_out=r1[s], fourier=True)
    assert same_bits(g1, g5) and same_bits(r1, r5) and same_bits(l1, l5)
    # whatever its neighbours hold: the others replaced by other images
    x2 = torch.rand(x.shape, generator=torch.Generator().manual_seed(9))
    x2[3] = x[3]
    _, g, r = run(x2, t, w, inv)
    assert same_bits(g[3], g5[3]) and same_bits(r[3], r5[3]) and not same_bits(g[2], g5[2])


@pytest.mark.parametrize("shape", [(3, 64, 64), (3, 8, 4), (1, 256, 256)], ids=["3x64x64", "3x8x4", "1x256x256"])
def test_zero_weight_sample_nan_sample_and_reproducibility(shape):
    n = 5
    x, t, w, _ = F.objective_inputs(n, shape, "real", seed=1)
    base = run(x, t, w, F.inv_wsum_of(w))
    again = run(x, t, w, F.inv_wsum_of(w))
    assert all(same_bits(a, b) for a, b in zip(base, again))                         # two runs of the same call: the same bits
    keep = [0, 2, 3, 4]
    others = lambda out: [v[keep] for v in out]
    unchanged = lambda out: all(same_bits(a, b) for a, b in zip(others(out), others(base)))
    zero = lambda out: float(out[0][1]) == 0.0 and float(out[1][1].abs().max()) == 0.0 and float(out[2][1].abs().max()) == 0.0
    # a zero-weight sample: exact zeros, the others bit for bit what they were
    w0 = w.clone()
    w0[1] = 0.0
    out = run(x, t, w0, F.inv_wsum_of(w0))
    assert zero(out) and unchanged(out)
    # a NaN in one sample's x: that sample's loss and gradient are NaN, the other samples' outputs unchanged
    xn = x.clone()
    xn[1, 0, 1, 1] = float("nan")
    out = run(xn, t, w, F.inv_wsum_of(w))
    assert bool(torch.isnan(out[0][1])) and bool(torch.isnan(out[1][1]).any())
    assert unchanged(out)
    # inv_wsum[n] == 0: exact zeros whatever x[n] holds -- the NaN included
    inv = F.inv_wsum_of(w)
    inv[1] = 0.0
    out = run(xn, t, w, inv)
    assert zero(out)
    assert all(bool(torch.isfinite(v).all()) for v in out) and unchanged(out)
    # loss_out may be NULL, weight and inv_wsum too: the gradient is the same
    xd, td = dev(x), dev(real(t))
    gl, rl = torch.zeros_like(xd), torch.zeros_like(td)
    scratch = fourier_scratch(n, *shape, xd.device)
    rc = G.lib().glowhip_restore_objective_fourier(xd.data_ptr(), td.data_ptr(), None, None, n, *shape, rl.data_ptr(), gl.data_ptr(),
                                                   None, scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    _, g1 = restore_objective(xd, td, None, None, 1, fourier=True, scratch=scratch)
    assert same_bits(gl, g1)


def test_refusals_leave_nan_filled_outputs_untouched():
    """Each GLOWHIP_EINVAL case returns before any device call: outputs filled with NaN still hold nothing else."""
    lib = G.lib()
    n, c, h, w = 2, 3, 8, 4
    x, t = torch.rand(n, c, h, w, device=DEV), torch.rand(n, c, h, w, 2, device=DEV)
    g, r, l = (torch.full(s, float("nan"), device=DEV) for s in ((n, c, h, w), (n, c, h, w, 2), (n,)))
    scratch = fourier_scratch(n, c, h, w, DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(x=x.data_ptr(), t=t.data_ptr(), resid=r.data_ptr(), grad=g.data_ptr(), N=n, C=c, H=h, W=w, s=scratch.data_ptr(),
             nbytes=scratch.numel()):
        return lib.glowhip_restore_objective_fourier(x, t, None, None, N, C, H, W, resid, grad, l.data_ptr(), s, nbytes, stream)

    cases = [dict(x=None), dict(t=None), dict(resid=None), dict(grad=None), dict(N=-1), dict(C=0), dict(H=12), dict(W=3), dict(H=512),
             dict(W=1), dict(s=None), dict(nbytes=scratch.numel() - 1), dict(s=scratch.data_ptr() + 4), dict(grad=x.data_ptr()),
             dict(resid=x.data_ptr()), dict(resid=g.data_ptr())]
    for kw in cases:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in (g, r, l))
    out = torch.full((n, c, h, w, 2), float("nan"), device=DEV)
    for args in ((None, out.data_ptr(), n * c, h, w, 0), (x.data_ptr(), None, n * c, h, w, 0), (x.data_ptr(), out.data_ptr(), -1, h, w, 0),
                 (x.data_ptr(), out.data_ptr(), n * c, 12, w, 0), (x.data_ptr(), out.data_ptr(), n * c, h, 512, 0),
                 (x.data_ptr(), out.data_ptr(), n * c, h, w, 2), (out.data_ptr(), out.data_ptr(), n * c, h, w, 0)):
        assert lib.glowhip_fourier2d(*args, stream) == -1, args
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0 and bool(torch.isfinite(g).all()) and bool(torch.isfinite(r).all()) and bool(torch.isfinite(l).all())
    # the Python layer's own refusals
    with pytest.raises(G._lib.GlowHipError, match="psf"):
        restore_objective(x, t, fourier=True, psf=torch.ones(3, 3, device=DEV))
    with pytest.raises(G._lib.GlowHipError, match="target"):
        restore_objective(x, torch.zeros(n, c, h, w, device=DEV), fourier=True)
    with pytest.raises(G._lib.GlowHipError, match="weight"):
        restore_objective(x, t, torch.ones(n, c, h, w, 2, device=DEV), fourier=True)
    with pytest.raises(G._lib.GlowHipError, match="scratch"):
        restore_objective(x, t, fourier=True, scratch=torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(G._lib.GlowHipError, match="power of two"):
        restore_objective(torch.rand(1, 1, 12, 8, device=DEV), torch.zeros(1, 1, 12, 8, 2, device=DEV), fourier=True)


# ------------------------------------------------------------------------------------------------ 4. the full mask: Parseval
@pytest.mark.parametrize("shape", [(3, 8, 4), (3, 64, 64), (1, 256, 256)], ids=["3x8x4", "3x64x64", "1x256x256"])
def test_full_mask_is_the_plain_objective_by_parseval(shape):
    """With all-ones weights and t = F y the loss is sum |F x - F y|^2 / (C H W) = sum (x - y)^2 / (C H W), the loss of
    glowhip_restore_objective(x, y): the two device losses agree within the sum of their two bounds (`fourier_oracle.bound` for this
    call on the rounded spectrum, whose own rounding to complex64 moves the exact loss by what `restore_oracle.bound` plus a carried
    u |t| per coefficient allows).  Equal bits are not expected: the two calls round differently."""
    g = torch.Generator().manual_seed(21)
    x, y = torch.rand((3,) + shape, generator=g), torch.rand((3,) + shape, generator=g)
    t = F.forward(y).to(torch.complex64)
    loss_f, _, _ = run(x, t, None, None)
    loss_p, _ = restore_objective(dev(x), dev(y), None, None, 1)
    E_f, _, _ = F.bound(x, t, None, None)
    E_p, _ = R.bound(x, y, None, None, 1)
    # the rounding of t = F y to complex64, u |t| per coefficient, carried into the exact loss: 2 inv sum |d| u |t|
    d = (F.forward(x) - F.forward(y)).abs()
    E_t = 2.0 / x[0].numel() * (d * F.U * F.forward(y).abs()).sum(dim=(1, 2, 3))
    diff = (loss_f.cpu().double() - loss_p.cpu().double()).abs()
    print(f"{shape}: |fourier - plain| {[f'{v:.2e}' for v in diff.tolist()]}  allowed {[f'{v:.2e}' for v in (E_f + E_p + E_t).tolist()]}")
    assert bool((diff <= E_f + E_p + E_t).all())
    exact, _ = R.objective(x, y, None, None, 1)
    assert bool(((loss_f.cpu().double() - exact).abs() <= E_f + E_t).all())


# ------------------------------------------------------------------------------------------------ 5. first-iteration latent gradients
def test_latent_gradients_of_the_objective_vs_fp64_autograd_oracle():
    """decode -> objective through a quarter of the k-space rows -> decode_vjp against fp64 autograd of the same objective through
    `O.flow_decode` and the oracle's transform, every entry within the project's gradient rule 2e-4 max|g| + 1e-7 per tensor
    (check_strict), on the 16x16 model of tests/test_gpu_decode_grad.py."""
    ref = D.reference(**R.TINY_AFF)
    assert_margin(ref)
    n, chw = ref["x"].shape[0], tuple(ref["x"].shape[1:])
    _, target, _, _ = F.objective_inputs(n, chw, "ones", seed=7)
    weight = fourier_mask(chw[1:], 0.25, seed=1).expand((n,) + chw).contiguous()
    inv = F.inv_wsum_of(weight)
    x_ref, loss_ref, gz_ref, geps_ref = F.latent_grads(ref["z"], ref["eps"], ref["sd"], ref["cfg"], target, weight, inv, ref["tables"])
    glow = make_glow(ref)
    plan = plan_of(glow, ref)
    x, _ = plan.decode(dev(ref["z"]), [dev(e) for e in ref["eps"]])
    loss, gx = restore_objective(x, dev(real(target)), dev(weight), dev(inv), 1, fourier=True)
    gz, geps = plan.decode_vjp(x, gx)
    ex = float((x.cpu().double() - x_ref).abs().max())
    el = float(((loss.cpu().double() - loss_ref).abs() / loss_ref).max())
    print(f"margin {ref['margin']:.2e}, decode err {ex:.2e}, loss rel err {el:.2e}")
    assert ex <= 1e-4 and el <= 1e-4
    check_strict(dict(gz=gz_ref, geps=geps_ref), gz, geps, "fourier tiny")


# ------------------------------------------------------------------------------------------------ 6. the loops
def setup():
    """(fit, ref, glow, inferer, k-space measurement complex64 on the device, mask (H,W) on the host) of `fourier_oracle.FIT`: the
    unknown image is the decode of the case's latents, the measurement `fourier2d` of it, the mask `fourier_mask((H, W), 0.25)`."""
    fit = F.FIT
    ref = D.reference(**R.TINY_AFF)
    glow = make_glow(ref)
    inf = Inferer(D.hps_for(ref["cfg"], ref["cfg"]["batch"]), glow, [DEV], DEV)
    target = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    mask = fourier_mask(tuple(target.shape[-2:]), fit["fraction"], kind=fit["kind"], seed=fit["seed"])
    return fit, ref, glow, inf, fourier2d(target), mask


def zero_filled_start(inf, meas, mask):
    return inf.encode_full(fourier2d_adjoint((torch.view_as_real(meas) * dev(mask).unsqueeze(-1)).contiguous()).clamp_(0.0, 1.0))


def test_fit_with_fourier_captured_and_eager_agree_bitwise_without_a_sync_in_a_replay():
    """Four iterations with a prior term on the 16x16 case from the zero-filled start: the captured loop (one eager iteration, then
    three replays of one hipGraph) and the eager loop give the same latents, loss history and norm history, bit for bit; a real
    measurement with a trailing 2 is the complex one.  Then three replays under torch's sync debug mode: none makes a host sync."""
    fit_kw, ref, glow, inf, meas, mask = setup()
    init = zero_filled_start(inf, meas, mask)
    args = dict(init=init, steps=4, lr=0.1, prior_weight=1e-3, weight=dev(mask), fourier=True)
    results = {}
    for name, graph, m in (("captured", True, meas), ("eager", False, meas), ("trailing 2", False, torch.view_as_real(meas).contiguous())):
        fit = LatentFit(glow, m, graph=graph, **args)
        assert fit.fourier and tuple(fit.resid.shape) == tuple(meas.shape) + (2,) and fit.op_scratch is not None and fit.psf is None
        assert tuple(fit.weight.shape) == tuple(meas.shape) and tuple(fit.image.shape) == tuple(meas.shape)
        assert fit._signature().get("fourier") is True
        info = fit.run()
        assert isinstance(info, RestoreInfo) and info.finite and info.fallback == 0
        assert info.captured == graph, f"{name}: captured = {info.captured} ({info.graph_error})"
        results[name] = (fit.latents().tensors(), info.loss, info.grad_norm)
    lat, loss, norm = results["captured"]
    print(f"loss {[f'{v:.4e}' for v in loss[:, 0].tolist()]} norm {[f'{v:.4e}' for v in norm.tolist()]}")
    assert not same_bits(lat[0], init.z) and float(loss.min()) > 0.0
    for name in ("eager", "trailing 2"):
        other = results[name]
        assert all(same_bits(a, b) for a, b in zip(lat, other[0])), f"{name}: latents differ from the captured loop's"
        assert same_bits(loss, other[1]) and same_bits(norm.view(-1), other[2].view(-1)), f"{name}: histories differ from the captured loop's"
    # the history's first entry is the objective of the start
    w4 = dev(mask).expand(meas.shape).contiguous()
    loss0, _ = restore_objective(glow.decode_latents(init, safe=False), torch.view_as_real(meas).contiguous(), w4,
                                 dev(F.inv_wsum_of(w4.cpu())), 1, fourier=True)
    assert same_bits(loss0.cpu(), loss[0])
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


def test_chain_with_fourier_is_the_same_captured_and_eager_and_chains_share_one_measurement():
    """Five iterations of `LatentMALA(fourier=True)`: one seed twice gives the same bits, the captured chain's latents, histories,
    steps, counters, moments and image are the eager chain's, bit for bit, and another mask gives another chain.  Then
    `Inferer.posterior(kspace[0], chains=3, fourier=True)`: three chains on ONE measurement, finite moments."""
    fit_kw, ref, glow, inf, meas, mask = setup()
    init = zero_filled_start(inf, meas, mask)
    other = fourier_mask(tuple(meas.shape[-2:]), 0.5, seed=3)
    args = dict(noise_std=0.2, init=init, steps=5, burn_in=3, thin=1, step_size=1e-3, seed=11, fourier=True)
    out = {}
    for name, graph in (("captured", True), ("eager", False), ("eager again", False), ("another mask", False)):
        mala = LatentMALA(glow, meas, weight=dev(other if name == "another mask" else mask), graph=graph, **args)
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
    assert not same_bits(a[-6], out["another mask"][-6]), "another mask gives the same energies: the weight is not in use"
    # the energy of the start is sum w |F x - t|^2 / (2 sigma^2): noise_std is the std of each of the real and imaginary parts
    x0 = glow.decode_latents(init, safe=False).cpu().double()
    e0 = (mask.double() * (F.forward(x0) - F.as_complex(meas.cpu())).abs() ** 2).sum(dim=(1, 2, 3)) / (2.0 * 0.2 ** 2)
    mala = LatentMALA(glow, meas, weight=dev(mask), graph=False, **args)
    assert float(((mala.loss.cpu().double() - e0).abs() / e0).max()) <= 1e-4
    lat, info = inf.posterior(meas[0], weight=mask, chains=3, noise_std=0.2, steps=4, burn_in=1, step_size=1e-3, seed=1, fourier=True)
    assert len(lat) == 3 and info.finite and tuple(info.energy.shape) == (4, 3) and info.count == 3
    assert tuple(info.mean.shape) == (3,) + tuple(meas.shape[1:])
    assert all(bool(torch.isfinite(v).all()) for v in (info.mean, info.std, info.pooled_mean, info.pooled_std, info.energy))
    # ... on one measurement, one weight and one start, repeated
    m3, w3, _, init3, _ = inf._problem(meas[0], mask, 1, None, chains=3, fourier=True)
    assert tuple(m3.shape) == (3,) + tuple(meas.shape[1:]) + (2,) and tuple(w3.shape) == (3,) + tuple(meas.shape[1:]) and len(init3) == 3
    assert all(same_bits(t[0], t[k]) for t in (m3, w3, *init3.tensors()) for k in (1, 2))
    assert same_bits(m3[0], torch.view_as_real(meas[0]))


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_restore_recovers_from_undersampled_kspace():
    """`Inferer.restore(kspace, weight=fourier_mask((16, 16), 0.25), fourier=True)` from the default start -- the encode of the
    zero-filled reconstruction -- on the 16x16x3 model, 40 steps at lr 0.1.  Every sample's final / first data term <= 0.1: the
    smallest of 0.1 / 0.2 / 0.5 that is at least twice the fp64 oracle's own worst ratio for the same fit
    (tests/test_fourier_host.py: 0.0042, 0.0048, 0.0045).  The untrained model is no meaningful prior: the data term is all that is
    asserted."""
    fit, ref, glow, inf, meas, mask = setup()
    lat, info = inf.restore(meas, weight=mask, steps=fit["steps"], lr=fit["lr"], fourier=True)
    hist = info.loss
    ratios = (hist[-1] / hist[0]).tolist()
    print("loss of sample 0:", " ".join(f"{v:.3e}" for v in hist[:, 0].tolist()), "| final / first", [f"{r:.4f}" for r in ratios],
          "| captured", info.captured, info.graph_error)
    assert isinstance(lat, Latents) and tuple(hist.shape) == (fit["steps"], meas.shape[0]) and info.finite and info.fallback == 0
    assert bool(torch.isfinite(hist).all()) and bool(torch.isfinite(info.grad_norm).all())
    assert info.captured, info.graph_error
    assert max(ratios) <= fit["ratio"], ratios
    # the device's start is the oracle's
    first = F.fit_case()["history"][0]
    assert float(((hist[0].double() - first).abs() / first).max()) <= 1e-3
    # init=None is an explicit start from the zero-filled reconstruction, bit for bit
    lat2, info2 = inf.restore(meas, weight=mask, steps=fit["steps"], lr=fit["lr"], fourier=True, init=zero_filled_start(inf, meas, mask))
    assert same_bits(info2.loss, hist) and same_bits(info2.grad_norm, info.grad_norm)
    assert all(same_bits(a, b) for a, b in zip(lat.tensors(), lat2.tensors()))
    # the returned latents are the fitted ones: their decode's data term is below the first
    w4 = dev(mask).expand(meas.shape).contiguous()
    loss, _ = restore_objective(glow.decode_latents(lat, safe=False), torch.view_as_real(meas).contiguous(), w4,
                                dev(F.inv_wsum_of(w4.cpu())), 1, fourier=True)
    assert bool((loss.cpu() < hist[0]).all())
    # a single problem given as (C,H,W): a batch of one
    lat1, info1 = inf.restore(meas[0], weight=mask, steps=2, lr=fit["lr"], fourier=True)
    assert len(lat1) == 1 and tuple(info1.loss.shape) == (2, 1) and info1.finite and float(info1.loss.min()) > 0.0
    # fourier=False: the in-painting fit of tests/test_gpu_restore.py, bit for bit what it is without the argument
    image = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    half = torch.zeros_like(image)
    half[..., : image.shape[-1] // 2] = 1.0
    kw = dict(weight=half, steps=4, lr=0.2, init=inf.encode_full(image * (1.0 - half)))
    _, a = inf.restore(image, **kw)
    _, b = inf.restore(image, fourier=False, **kw)
    assert same_bits(a.loss, b.loss) and same_bits(a.grad_norm, b.grad_norm)
    with pytest.raises(ValueError):
        inf.restore(meas, weight=-mask, steps=2, fourier=True)
    with pytest.raises(ValueError):
        inf.restore(meas, weight=mask, steps=2, fourier=True, pool=2)

"""GPU tests of multi-coil k-space (-m gpu): glowhip_restore_objective_coils and glowhip_coils2d (csrc/restore_fourier.hip) against
the fp64 restatement of tests/coil_oracle.py on every element of the loss, the gradient and the residual; the kernels' structural
properties (batch independence, shared against per-sample maps, reproducibility, zero-weight and NaN samples, refusals that touch
nothing); one coil with unit maps against the plain Fourier call; the latent gradient of the objective against fp64 autograd through
`O.flow_decode`; `LatentFit` and `LatentMALA` with ``coils=``, captured against eager bit for bit; and
`Inferer.restore(kspace, weight=fourier_mask(...), fourier=True, coils=coil_maps(...))` on the fit whose ratio
tests/test_coil_host.py fixes on the CPU.

The cases sit where the kernels can go wrong, not at the workload's size (`coil_oracle.CASES`): one stage; H != W both ways with odd
coil counts; row tiles of several rows and column tiles of 32; the largest coil count; the longest row and column against the
shortest; and 256 x 256, the plane that does not fit in LDS."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd.network import (Inferer, LatentFit, LatentMALA, Latents, RestoreInfo, coil_maps, coils2d, coils2d_adjoint,  # noqa: E402
                                      coils_scratch, fourier_mask, restore_objective)

import coil_oracle as C  # noqa: E402
import decode_grad_oracle as D  # noqa: E402
import fourier_oracle as F  # noqa: E402
import restore_oracle as R  # noqa: E402
from test_gpu_decode_grad import DEV, assert_margin, check_strict, dev, make_glow, plan_of  # noqa: E402
from test_gpu_linear import same_bits, shifted  # noqa: E402

opt = lambda v, f=dev: None if v is None else f(v)
real = lambda t: torch.view_as_real(t.contiguous())      # complex64 (..., H, W) -> fp32 (..., H, W, 2)


def run(x, t, maps, w, inv, f=dev):
    """One call on fresh NaN-filled outputs placed by ``f``: (loss, grad_x, resid fp32 (N,C,Q,H,W,2))."""
    xd, td, sd = f(x), f(real(t)), f(real(maps))
    g_out, r_out = f(torch.full(x.shape, float("nan"))), f(torch.full(td.shape, float("nan")))
    loss, g = restore_objective(xd, td, opt(w, f), opt(inv, f), 1, grad_out=g_out, resid_out=r_out, fourier=True, coils=sd)
    assert g is g_out
    return loss, g, r_out


# ------------------------------------------------------------------------------------------------ 1. the objective, every element
@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_objective_every_element_vs_fp64_oracle(case):
    """loss, grad_x and resid (the modulus of the complex difference) within `coil_oracle.bound`: `fourier_oracle.bound` coil plane
    by coil plane with the roundings of the input product, of S.re G.re + S.im G.im and of the fp32 coil sum added.
    tests/test_coil_host.py shows a float32 restatement of the three passes, in the kernels' butterfly order and in the opposite
    one, inside the bound on these inputs: nothing here was tuned on the device.  Batches of 1, 3 and 5 (and 67 at 3x3x4x8); a 0/1
    mask, real weights with exact zeros, and NULL; shared maps, and per-sample maps at the batch of 3.  The largest case also runs
    with every pointer one float off a 16-byte address: the same bound, and the same gradient and residual bits."""
    worst = [0.0, 0.0, 0.0]
    for n in C.batches_of(case):
        for weights in C.WEIGHTS:
            for per_sample in ((False, True) if n == 3 else (False,)):
                x, t, maps, w, inv = C.objective_inputs(n, case, weights, per_sample=per_sample)
                loss_ref, g_ref, r_ref = C.objective(x, t, maps, w, inv)
                E_loss, E_g, E_r = C.bound(x, t, maps, w, inv)
                placements = [("aligned", dev)]
                if (case, n) == (C.CASES[-1], C.BATCHES[-1]):
                    placements += [("all one float off", shifted)]
                first = None
                for name, f in placements:
                    loss, g, r = run(x, t, maps, w, inv, f)
                    ml, mg = C.worst_multiple(loss, loss_ref, E_loss), C.worst_multiple(g, g_ref, E_g)
                    mr = C.complex_multiple(r, r_ref, E_r)
                    print(f"{case} N {n} {weights} per-sample maps {per_sample} {name}: worst multiple of the bound  loss {ml:.3f}  "
                          f"grad {mg:.3f}  resid {mr:.3f}")
                    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(r).all())
                    assert ml <= 1.0 and mg <= 1.0 and mr <= 1.0, (n, weights, per_sample, name, ml, mg, mr)
                    worst = [max(a, b) for a, b in zip(worst, (ml, mg, mr))]
                    if first is None:
                        first = (g.clone(), r.clone())
                    else:
                        assert same_bits(g, first[0]) and same_bits(r, first[1]), f"{name}: bits differ from the aligned call's"
    print(f"{case}: worst multiple over the case  loss {worst[0]:.3f}  grad {worst[1]:.3f}  resid {worst[2]:.3f}")


# ------------------------------------------------------------------------------------------------ 2. the operator alone
@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_coils2d_forward_adjoint_and_adjoint_identity(case):
    """glowhip_coils2d both ways against fp64 within `coil_oracle.coils2d_bound` on every element, with shared and with per-sample
    maps; <A x, k> = <x, A^H k> on the device's own results within what the vector bounds allow (Cauchy-Schwarz, channel by
    channel)."""
    c, q, h, w = case
    g = torch.Generator().manual_seed(77)
    x = torch.rand((3, c, h, w), generator=g)
    k = torch.complex(torch.randn((3, c, q, h, w), generator=g), torch.randn((3, c, q, h, w), generator=g))
    xd, kd = dev(x), dev(k)
    for maps in (C.case_maps(case), C.case_maps(case, 3)):
        sd = dev(maps)
        Y = coils2d(xd, sd)
        assert Y.dtype == torch.complex64 and tuple(Y.shape) == (3, c, q, h, w)
        mf = C.complex_multiple(Y, C.forward(x, maps), C.coils2d_bound(x, maps, h, w))
        a = coils2d_adjoint(kd, sd)
        assert a.dtype == torch.float32 and tuple(a.shape) == tuple(x.shape)
        ma = C.worst_multiple(a, C.adjoint(k, maps), C.coils2d_bound(k, maps, h, w))
        print(f"{case} maps {tuple(maps.shape)}: worst multiple of the bound  forward {mf:.3f}  adjoint {ma:.3f}")
        assert mf <= 1.0 and ma <= 1.0
        lhs = float((C.as_complex(Y.cpu()).conj() * C.as_complex(k)).real.sum())
        rhs = float((x.double() * a.cpu().double()).sum())
        knorm = (C.as_complex(k).abs() ** 2).sum(dim=(2, 3, 4)).sqrt().view(3, c, 1, 1)
        xnorm = (x.double() ** 2).sum(dim=(2, 3)).sqrt().view(3, c, 1, 1)
        slack = float((C.coils2d_norm_bound(x, maps, h, w) * knorm + C.coils2d_norm_bound(k, maps, h, w) * xnorm).sum())
        print(f"{case}: <A x, k> - <x, A^H k> = {lhs - rhs:.3e} (allowed {slack:.3e})")
        assert abs(lhs - rhs) <= slack
        # real buffers with a trailing 2 are the same calls; out= is written in place
        buf = torch.full((3, c, q, h, w, 2), float("nan"), device=DEV)
        assert same_bits(torch.view_as_real(coils2d(xd, real(sd), out=buf)), buf) and same_bits(buf, torch.view_as_real(Y))
        assert same_bits(coils2d_adjoint(real(kd), sd), a)


# ------------------------------------------------------------------------------------------------ 3. the kernels' properties
@pytest.mark.parametrize("case", C.PROPERTY_CASES, ids=C.PROPERTY_IDS)
def test_a_sample_has_the_same_bits_alone_and_in_a_batch_of_five_and_with_shared_or_per_sample_maps(case):
    """Tile shapes and the butterfly order are functions of (H, W), never of N, and a workgroup works on the planes of one sample:
    sample n of a batch of 5 has the bits of the same sample run as a batch of one.  The maps shared by the batch and the same maps
    repeated per sample give the same bits."""
    x, t, maps, w, inv = C.objective_inputs(5, case, "real", seed=2)
    xd, td, wd, invd, sd = dev(x), dev(real(t)), dev(w), dev(inv), dev(real(maps))
    nan = lambda s: torch.full(tuple(s), float("nan"), device=DEV)
    g5, r5, l5 = nan(x.shape), nan(td.shape), nan((5,))
    restore_objective(xd, td, wd, invd, 1, grad_out=g5, loss_out=l5, resid_out=r5, fourier=True, coils=sd)
    g1, r1, l1 = nan(x.shape), nan(td.shape), nan((5,))
    for k in range(5):
        s = slice(k, k + 1)
        restore_objective(xd[s], td[s], wd[s], invd[s], 1, grad_out=g1[s], loss_out=l1[s], resid_out=r1[s], fourier=True, coils=sd)
    assert same_bits(g1, g5) and same_bits(r1, r5) and same_bits(l1, l5)
    # the same maps, one copy per sample
    rep = sd.unsqueeze(0).expand((5,) + tuple(sd.shape)).contiguous()
    gp, rp, lp = nan(x.shape), nan(td.shape), nan((5,))
    restore_objective(xd, td, wd, invd, 1, grad_out=gp, loss_out=lp, resid_out=rp, fourier=True, coils=rep)
    assert same_bits(gp, g5) and same_bits(rp, r5) and same_bits(lp, l5)
    assert same_bits(torch.view_as_real(coils2d(xd, rep)), torch.view_as_real(coils2d(xd, sd)))
    assert same_bits(coils2d_adjoint(td, rep), coils2d_adjoint(td, sd))
    # per-sample maps are per sample: another sample's maps changed, this sample's bits stay
    rep2 = rep.clone()
    rep2[2] = rep2[2].flip(0)
    g2, r2, l2 = nan(x.shape), nan(td.shape), nan((5,))
    restore_objective(xd, td, wd, invd, 1, grad_out=g2, loss_out=l2, resid_out=r2, fourier=True, coils=rep2)
    keep = [0, 1, 3, 4]
    assert same_bits(g2[keep], g5[keep]) and same_bits(r2[keep], r5[keep]) and same_bits(l2[keep], l5[keep])
    assert case[1] == 1 or not same_bits(g2[2], g5[2])
    # whatever its neighbours hold: the others replaced by other images
    x2 = torch.rand(x.shape, generator=torch.Generator().manual_seed(9))
    x2[3] = x[3]
    _, g, r = run(x2, t, maps, w, inv)
    assert same_bits(g[3], g5[3]) and same_bits(r[3], r5[3]) and not same_bits(g[2], g5[2])


@pytest.mark.parametrize("case", C.PROPERTY_CASES, ids=C.PROPERTY_IDS)
def test_zero_weight_sample_nan_sample_and_reproducibility(case):
    n, q = 5, case[1]
    x, t, maps, w, _ = C.objective_inputs(n, case, "real", seed=1)
    base = run(x, t, maps, w, C.inv_wsum_of(w, q))
    again = run(x, t, maps, w, C.inv_wsum_of(w, q))
    assert all(same_bits(a, b) for a, b in zip(base, again))                         # two runs of the same call: the same bits
    keep = [0, 2, 3, 4]
    others = lambda out: [v[keep] for v in out]
    unchanged = lambda out: all(same_bits(a, b) for a, b in zip(others(out), others(base)))
    zero = lambda out: float(out[0][1]) == 0.0 and float(out[1][1].abs().max()) == 0.0 and float(out[2][1].abs().max()) == 0.0
    # a zero-weight sample: exact zeros, the others bit for bit what they were
    w0 = w.clone()
    w0[1] = 0.0
    out = run(x, t, maps, w0, C.inv_wsum_of(w0, q))
    assert zero(out) and unchanged(out)
    # a NaN in one sample's x: that sample's loss and gradient are NaN, the other samples' outputs unchanged
    xn = x.clone()
    xn[1, 0, 1, 1] = float("nan")
    out = run(xn, t, maps, w, C.inv_wsum_of(w, q))
    assert bool(torch.isnan(out[0][1])) and bool(torch.isnan(out[1][1]).any())
    assert unchanged(out)
    # inv_wsum[n] == 0: exact zeros whatever x[n] holds -- the NaN included
    inv = C.inv_wsum_of(w, q)
    inv[1] = 0.0
    out = run(xn, t, maps, w, inv)
    assert zero(out)
    assert all(bool(torch.isfinite(v).all()) for v in out) and unchanged(out)
    # loss_out may be NULL, weight and inv_wsum too: the gradient is the same
    xd, td, sd = dev(x), dev(real(t)), dev(real(maps))
    gl, rl = torch.zeros_like(xd), torch.zeros_like(td)
    scratch = coils_scratch(n, case[0], q, case[2], case[3], xd.device)
    rc = G.lib().glowhip_restore_objective_coils(xd.data_ptr(), td.data_ptr(), None, None, sd.data_ptr(), 0, n, *case, rl.data_ptr(),
                                                 gl.data_ptr(), None, scratch.data_ptr(), scratch.numel(),
                                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    _, g1 = restore_objective(xd, td, None, None, 1, fourier=True, coils=sd, scratch=scratch)
    assert same_bits(gl, g1)


def test_refusals_leave_nan_filled_outputs_untouched():
    """Each GLOWHIP_EINVAL case returns before any device call: outputs filled with NaN still hold nothing else."""
    lib = G.lib()
    n, c, q, h, w = 2, 3, 4, 8, 4
    x, t, s = torch.rand(n, c, h, w, device=DEV), torch.rand(n, c, q, h, w, 2, device=DEV), torch.rand(q, h, w, 2, device=DEV)
    g, r, l = (torch.full(sh, float("nan"), device=DEV) for sh in ((n, c, h, w), (n, c, q, h, w, 2), (n,)))
    scratch = coils_scratch(n, c, q, h, w, DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(x=x.data_ptr(), t=t.data_ptr(), maps=s.data_ptr(), stride=0, resid=r.data_ptr(), grad=g.data_ptr(), N=n, C=c, Q=q, H=h, W=w,
             sc=scratch.data_ptr(), nbytes=scratch.numel()):
        return lib.glowhip_restore_objective_coils(x, t, None, None, maps, stride, N, C, Q, H, W, resid, grad, l.data_ptr(), sc, nbytes, stream)

    cases = [dict(x=None), dict(t=None), dict(maps=None), dict(resid=None), dict(grad=None), dict(N=-1), dict(C=0), dict(Q=0), dict(Q=33),
             dict(stride=8), dict(stride=h * w * 2), dict(H=12), dict(W=3), dict(H=512), dict(W=1), dict(sc=None),
             dict(nbytes=scratch.numel() - 1), dict(sc=scratch.data_ptr() + 4), dict(grad=x.data_ptr()), dict(resid=x.data_ptr()),
             dict(resid=g.data_ptr()), dict(maps=g.data_ptr()), dict(maps=r.data_ptr())]
    for kw in cases:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in (g, r, l))
    out = torch.full((n, c, q, h, w, 2), float("nan"), device=DEV)
    ok = (x.data_ptr(), s.data_ptr(), 0, out.data_ptr(), n, c, q, h, w, 0)
    for k, v in ((0, None), (1, None), (3, None), (2, 8), (4, -1), (5, 0), (6, 0), (6, 33), (7, 12), (8, 512), (9, 2), (1, out.data_ptr())):
        args = list(ok)
        args[k] = v
        assert lib.glowhip_coils2d(*args, stream) == -1, (k, v)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0 and bool(torch.isfinite(g).all()) and bool(torch.isfinite(r).all()) and bool(torch.isfinite(l).all())
    # the Python layer's own refusals
    with pytest.raises(ValueError, match="fourier=True"):
        restore_objective(x, t, coils=s)
    with pytest.raises(G._lib.GlowHipError, match="psf"):
        restore_objective(x, t, fourier=True, coils=s, psf=torch.ones(3, 3, device=DEV))
    with pytest.raises(G._lib.GlowHipError, match="target"):
        restore_objective(x, torch.zeros(n, c, h, w, 2, device=DEV), fourier=True, coils=s)
    with pytest.raises(G._lib.GlowHipError, match="weight"):
        restore_objective(x, t, torch.ones(n, c, q, h, w, device=DEV), fourier=True, coils=s)
    with pytest.raises(G._lib.GlowHipError, match="scratch"):
        restore_objective(x, t, fourier=True, coils=s, scratch=torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        restore_objective(x, t, fourier=True, coils=torch.rand(q, h, h, 2, device=DEV))
    with pytest.raises(G._lib.GlowHipError, match="power of two"):
        restore_objective(torch.rand(1, 1, 12, 8, device=DEV), torch.zeros(1, 1, 2, 12, 8, 2, device=DEV), fourier=True,
                          coils=torch.rand(2, 12, 8, 2, device=DEV))


# ------------------------------------------------------------------------------------------------ 4. one coil, unit maps
@pytest.mark.parametrize("shape", [(3, 8, 4), (3, 64, 64), (1, 256, 256)], ids=["3x8x4", "3x64x64", "1x256x256"])
def test_one_coil_with_unit_maps_equals_the_plain_fourier_call(shape):
    """Q = 1 and S = 1 + 0i: loss, grad_x and resid are `torch.equal` to glowhip_restore_objective_fourier's -- value-equal; the only
    bit that may differ is the sign of a zero (0 * x is -0 for x < 0, and +-0 never changes a non-zero sum).  The images here have
    negative pixels, so that the signed zeros do occur."""
    c, h, w = shape
    for weights in F.WEIGHTS:
        x, t, wt, inv = F.objective_inputs(3, shape, weights)
        x = x - 0.5
        ones = torch.zeros(1, h, w, 2)
        ones[..., 0] = 1.0
        xd, td = dev(x), dev(real(t))
        r_f = torch.full(td.shape, float("nan"), device=DEV)
        loss_f, g_f = restore_objective(xd, td, opt(wt), opt(inv), 1, resid_out=r_f, fourier=True)
        r_c = torch.full((3, c, 1, h, w, 2), float("nan"), device=DEV)
        loss_c, g_c = restore_objective(xd, td.unsqueeze(2).contiguous(), opt(wt), opt(inv), 1, resid_out=r_c, fourier=True, coils=dev(ones))
        assert torch.equal(loss_c, loss_f) and torch.equal(g_c, g_f) and torch.equal(r_c.squeeze(2), r_f), (shape, weights)


# ------------------------------------------------------------------------------------------------ 5. first-iteration latent gradients
def test_latent_gradients_of_the_objective_vs_fp64_autograd_oracle():
    """decode -> multi-coil objective (4 coils, a quarter of the k-space rows) -> decode_vjp against fp64 autograd of the same
    objective through `O.flow_decode` and the oracle's operator, every entry within the project's gradient rule 2e-4 max|g| + 1e-7
    per tensor (check_strict), on the 16x16 model of tests/test_gpu_decode_grad.py: the rule of tests/test_gpu_fourier.py."""
    ref = D.reference(**R.TINY_AFF)
    assert_margin(ref)
    n, chw = ref["x"].shape[0], tuple(ref["x"].shape[1:])
    q = 4
    maps = coil_maps(chw[1:], q, seed=2)
    _, target, _, _, _ = C.objective_inputs(n, (chw[0], q) + chw[1:], "ones", seed=7)
    weight = fourier_mask(chw[1:], 0.25, seed=1).expand((n,) + chw).contiguous()
    inv = C.inv_wsum_of(weight, q)
    x_ref, loss_ref, gz_ref, geps_ref = C.latent_grads(ref["z"], ref["eps"], ref["sd"], ref["cfg"], target, maps, weight, inv, ref["tables"])
    glow = make_glow(ref)
    plan = plan_of(glow, ref)
    x, _ = plan.decode(dev(ref["z"]), [dev(e) for e in ref["eps"]])
    loss, gx = restore_objective(x, dev(real(target)), dev(weight), dev(inv), 1, fourier=True, coils=dev(maps))
    gz, geps = plan.decode_vjp(x, gx)
    ex = float((x.cpu().double() - x_ref).abs().max())
    el = float(((loss.cpu().double() - loss_ref).abs() / loss_ref).max())
    print(f"margin {ref['margin']:.2e}, decode err {ex:.2e}, loss rel err {el:.2e}")
    assert ex <= 1e-4 and el <= 1e-4
    check_strict(dict(gz=gz_ref, geps=geps_ref), gz, geps, "coils tiny")


# ------------------------------------------------------------------------------------------------ 6. the loops
def setup():
    """(fit, ref, glow, inferer, multi-coil measurement complex64 (N,C,Q,H,W) on the device, mask (H,W) and maps (Q,H,W) on the
    host) of `coil_oracle.FIT`: the unknown image is the decode of the case's latents, the measurement `coils2d` of it."""
    fit = C.FIT
    ref = D.reference(**R.TINY_AFF)
    glow = make_glow(ref)
    inf = Inferer(D.hps_for(ref["cfg"], ref["cfg"]["batch"]), glow, [DEV], DEV)
    target = glow.decode_latents(Latents(dev(ref["z"]), [dev(e) for e in ref["eps"]]), safe=False)
    hw = tuple(target.shape[-2:])
    mask = fourier_mask(hw, fit["fraction"], kind=fit["kind"], seed=fit["seed"])
    maps = coil_maps(hw, fit["coils"], seed=fit["coil_seed"])
    return fit, ref, glow, inf, coils2d(target, dev(maps)), mask, maps


def combined_start(inf, meas, mask, maps):
    masked = (torch.view_as_real(meas) * dev(mask).unsqueeze(-1)).contiguous()
    return inf.encode_full(coils2d_adjoint(masked, dev(maps)).clamp_(0.0, 1.0))


def test_fit_with_coils_captured_and_eager_agree_bitwise_without_a_sync_in_a_replay():
    """Four iterations with a prior term on the 16x16 case from the coil-combined start: the captured loop (one eager iteration,
    then three replays of one hipGraph) and the eager loop give the same latents, loss history and norm history, bit for bit; a
    real measurement with a trailing 2 is the complex one.  Then three replays under torch's sync debug mode: none makes a host
    sync."""
    fit_kw, ref, glow, inf, meas, mask, maps = setup()
    q = fit_kw["coils"]
    n, c = meas.shape[:2]
    hw = tuple(meas.shape[-2:])
    init = combined_start(inf, meas, mask, maps)
    args = dict(init=init, steps=4, lr=0.1, prior_weight=1e-3, weight=dev(mask), fourier=True, coils=dev(maps))
    results = {}
    for name, graph, m in (("captured", True, meas), ("eager", False, meas), ("trailing 2", False, torch.view_as_real(meas).contiguous())):
        fit = LatentFit(glow, m, graph=graph, **args)
        assert fit.fourier and fit.n_coils == q and tuple(fit.resid.shape) == tuple(meas.shape) + (2,) and fit.psf is None
        assert fit.op_scratch.numel() == G.lib().glowhip_restore_coils_scratch_bytes(n, c, q, *hw)
        assert tuple(fit.weight.shape) == (n, c) + hw and tuple(fit.image.shape) == (n, c) + hw
        assert tuple(fit.coils.shape) == (q,) + hw + (2,) and fit.coils.data_ptr() != dev(maps).data_ptr()      # the loop's own copy
        sig = fit._signature()
        assert sig["coils"] == q and sig.get("fourier") is True
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
    # the history's first entry is the objective of the start, with inv_wsum = 1 / max(Q sum w, 1)
    w4 = dev(mask).expand((n, c) + hw).contiguous()
    loss0, _ = restore_objective(glow.decode_latents(init, safe=False), torch.view_as_real(meas).contiguous(), w4,
                                 dev(C.inv_wsum_of(w4.cpu(), q)), 1, fourier=True, coils=dev(maps))
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


def test_chain_with_coils_is_the_same_captured_and_eager_and_chains_share_one_measurement():
    """Five iterations of `LatentMALA(coils=)`: the captured chain's latents, histories, steps, counters, moments and image are the
    eager chain's, bit for bit; other maps give other energies; the start's energy is the fp64 formula's.  Then
    `Inferer.posterior(kspace[0], chains=3, fourier=True, coils=S)`: three chains on ONE measurement, finite moments."""
    fit_kw, ref, glow, inf, meas, mask, maps = setup()
    q = fit_kw["coils"]
    init = combined_start(inf, meas, mask, maps)
    other = coil_maps(tuple(meas.shape[-2:]), q, seed=5)
    args = dict(noise_std=0.2, init=init, steps=5, burn_in=3, thin=1, step_size=1e-3, seed=11, fourier=True, weight=dev(mask))
    out = {}
    for name, graph in (("captured", True), ("eager", False), ("other maps", False)):
        mala = LatentMALA(glow, meas, coils=dev(other if name == "other maps" else maps), graph=graph, **args)
        assert mala._signature()["coils"] == q
        info = mala.run()
        assert info.finite and info.captured == graph, f"{name}: captured = {info.captured} ({info.graph_error})"
        assert mala.iteration.tolist() == [5]
        out[name] = (*mala.latents().tensors(), mala.hist.clone(), mala.step.clone(), mala.counts.clone(), mala.mean.clone(),
                     mala.m2.clone(), mala.image.clone())
        print(name, "accepted", info.accepted.sum(dim=0).tolist(), "energy", [f"{v:.4e}" for v in info.energy[-1].tolist()])
    a = out["captured"]
    assert float(a[-6][0].abs().min()) > 0.0      # the energy history: every iteration was decided
    assert all(same_bits(x, y) for x, y in zip(a, out["eager"])), "eager: differs from the captured chain"
    assert not same_bits(a[-6], out["other maps"][-6]), "other maps give the same energies: the maps are not in use"
    # the energy of the start is sum_{c,q,k} w |F (S_q x) - t|^2 / (2 sigma^2)
    x0 = glow.decode_latents(init, safe=False).cpu().double()
    d = C.forward(x0, maps) - C.as_complex(meas.cpu())
    e0 = (mask.double() * d.abs() ** 2).sum(dim=(1, 2, 3, 4)) / (2.0 * 0.2 ** 2)
    mala = LatentMALA(glow, meas, coils=dev(maps), graph=False, **args)
    assert float(((mala.loss.cpu().double() - e0).abs() / e0).max()) <= 1e-4
    lat, info = inf.posterior(meas[0], weight=mask, chains=3, noise_std=0.2, steps=4, burn_in=1, step_size=1e-3, seed=1, fourier=True,
                              coils=maps)
    assert len(lat) == 3 and info.finite and tuple(info.energy.shape) == (4, 3) and info.count == 3
    assert tuple(info.mean.shape) == (3, meas.shape[1]) + tuple(meas.shape[-2:])
    assert all(bool(torch.isfinite(v).all()) for v in (info.mean, info.std, info.pooled_mean, info.pooled_std, info.energy))
    # ... on one measurement, one weight and one start, repeated; the maps stay shared
    m3, w3, _, init3, _, s3 = inf._coils_problem(meas[0], mask, 1, None, 3, None, None, None, maps)
    assert tuple(m3.shape) == (3,) + tuple(meas.shape[1:]) + (2,) and tuple(w3.shape) == (3, meas.shape[1]) + tuple(meas.shape[-2:])
    assert len(init3) == 3 and tuple(s3.shape) == tuple(maps.shape) + (2,)
    assert all(same_bits(t[0], t[k]) for t in (m3, w3, *init3.tensors()) for k in (1, 2))
    assert same_bits(m3[0], torch.view_as_real(meas[0]))


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_restore_recovers_from_undersampled_multi_coil_kspace():
    """`Inferer.restore(kspace, weight=fourier_mask((16, 16), 0.25), fourier=True, coils=coil_maps((16, 16), 4))` from the default
    start -- the encode of the coil-combined zero-filled image -- on the 16x16x3 model, 40 steps at lr 0.1.  Every sample's
    final / first data term <= 0.1: the smallest of 0.1 / 0.2 / 0.5 that is at least twice the fp64 oracle's own worst ratio for the
    same fit (tests/test_coil_host.py: 0.0187, 0.0165, 0.0175).  The untrained model is no meaningful prior: the data term is all
    that is asserted."""
    fit, ref, glow, inf, meas, mask, maps = setup()
    lat, info = inf.restore(meas, weight=mask, steps=fit["steps"], lr=fit["lr"], fourier=True, coils=maps)
    hist = info.loss
    ratios = (hist[-1] / hist[0]).tolist()
    print("loss of sample 0:", " ".join(f"{v:.3e}" for v in hist[:, 0].tolist()), "| final / first", [f"{r:.4f}" for r in ratios],
          "| captured", info.captured, info.graph_error)
    assert isinstance(lat, Latents) and tuple(hist.shape) == (fit["steps"], meas.shape[0]) and info.finite and info.fallback == 0
    assert bool(torch.isfinite(hist).all()) and bool(torch.isfinite(info.grad_norm).all())
    assert info.captured, info.graph_error
    assert max(ratios) <= fit["ratio"], ratios
    # the device's start is the oracle's
    first = C.fit_case()["history"][0]
    assert float(((hist[0].double() - first).abs() / first).max()) <= 1e-3
    # init=None is an explicit start from the coil-combined zero-filled image, bit for bit
    lat2, info2 = inf.restore(meas, weight=mask, steps=fit["steps"], lr=fit["lr"], fourier=True, coils=maps,
                              init=combined_start(inf, meas, mask, maps))
    assert same_bits(info2.loss, hist) and same_bits(info2.grad_norm, info.grad_norm)
    assert all(same_bits(a, b) for a, b in zip(lat.tensors(), lat2.tensors()))
    # a single problem given as (C,Q,H,W): a batch of one
    lat1, info1 = inf.restore(meas[0], weight=mask, steps=2, lr=fit["lr"], fourier=True, coils=maps)
    assert len(lat1) == 1 and tuple(info1.loss.shape) == (2, 1) and info1.finite and float(info1.loss.min()) > 0.0
    # coils=None: the single-coil k-space fit of tests/test_gpu_fourier.py, bit for bit what it is without the argument
    single = torch.view_as_complex(torch.view_as_real(meas)[:, :, 0].contiguous())
    kw = dict(weight=mask, steps=4, lr=fit["lr"], fourier=True)
    la, a = inf.restore(single, **kw)
    lb, b = inf.restore(single, coils=None, **kw)
    assert same_bits(a.loss, b.loss) and same_bits(a.grad_norm, b.grad_norm)
    assert all(same_bits(u, v) for u, v in zip(la.tensors(), lb.tensors()))
    with pytest.raises(ValueError):
        inf.restore(meas, weight=mask, steps=2, coils=maps)
    with pytest.raises(ValueError):
        inf.restore(meas, weight=mask, steps=2, fourier=True, coils=maps, pool=2)

"""GPU tests of the per-sample log-likelihood accumulators (-m gpu): csrc/common.h fix_atomic_add / fix_flag_nonfinite, finished by
k_finalize and read by k_status.  Every objective of the project passes through them; here each kernel that feeds them UNBOUNDED
terms, (x - mean)^2 / exp(2 logs), is held to float64 -- k_gaussian_logp directly through GaussianDiag.logp /
glowhip_gaussian_logp (no other GPU test calls them), k_split_tail and the two MFMA Split2d tails, k_top_head_fwd, one whole model.

Reference: oracle.glow_oracle.gaussian_logps in fp64, summed in fp64 (tests/objective_oracle.py; no second copy of the formula).
Bars are derived there (`bar`), not measured.  The range cases follow the guarantee written in common.h and include/glowhip.h: with
partials of |v| < 2^43 nats a sample comes back FINITE and within 1e-6 relative of fp64, whatever the size of its sum (the
fp32 reference is ~1e-7 from fp64, tests/test_objective_host.py asserts that and the class of every case from the oracle alone); a
partial beyond 2^43 gives -inf with flag bit 4; nothing is ever finite and off.  The other samples of the batch keep the bits they
have without the extreme one.

Left out: the POSITIVE end of the range.  A term is at most -log(2 pi)/2 - logs, and logs >= -103.3 wherever exp(2 logs) is a
positive fp32, so passing +2^31 nats takes more than 7e7 elements in one sample."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib  # noqa: E402

import objective_oracle as OO  # noqa: E402
import test_gpu_sampler as TS  # noqa: E402

DEV = "cuda:0"
FAMILIES = TS.FAMILIES
NAN = float("nan")


def dev(t):
    return None if t is None else t.to(DEV)


def raw_logp(x, xs, mean, logs, mls, n, c, hw, inp, out):
    """glowhip_gaussian_logp on raw pointers (ints; 0 = NULL): returns the flag bits the call left in its scratch."""
    scratch = torch.full((2 * max(n, 1),), -1, dtype=torch.int64, device=DEV)      # (poison: the call zeroes what it uses)
    _lib.check(G.lib().glowhip_gaussian_logp(x, xs, mean or None, logs or None, mls, n, c, hw, inp or None, out.data_ptr(),
                                             scratch.data_ptr(), _lib.stream_ptr(torch.device(DEV))))
    return (scratch[n:2 * n] & 7).cpu()


def p(t):
    return 0 if t is None else t.data_ptr()


def report(what, got, want, bound):
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), (what, got)
    e = (got - want).abs()
    k = int((e / bound).argmax())
    print(f"{what}: finite, error {float(e[k]):.3e} (bar {float(bound[k]):.3e}) = {float((e / bound).max()):.3f} of the bar")
    assert bool((e <= bound).all()), f"{what}: {e.tolist()} against {bound.tolist()}"


# ------------------------------------------------------------------------------------------------ 1. shapes and arguments
@pytest.mark.parametrize("args", OO.ARGS)
@pytest.mark.parametrize("shape", OO.SHAPES, ids=str)
def test_logp_matches_fp64_at_every_shape(shape, args):
    x, mean, logs, _ = OO.logp_case(shape)
    mean, logs = OO.pick(args, mean, logs)
    got = G.GaussianDiag.logp(dev(mean), dev(logs), dev(x))
    assert got.shape == (shape[0],) and got.dtype == torch.float32
    report(f"logp {shape} {args}", got, OO.logp64(mean, logs, x), OO.bar(mean, logs, x))


@pytest.mark.parametrize("shape", OO.SHAPES, ids=str)
def test_logp_accumulates_onto_in_and_overwrites_out(shape):
    """`in` given, the output buffer poisoned beforehand (and its neighbours left alone); then NULL mean, logs and in."""
    x, mean, logs, inp = OO.logp_case(shape)
    n, c, hw = shape[0], shape[1], shape[2] * shape[3]
    xd, md, ld, ind = dev(x), dev(mean), dev(logs), dev(inp)
    out = torch.full((n + 2,), NAN, device=DEV)
    flags = raw_logp(p(xd), c * hw, p(md), p(ld), c * hw, n, c, hw, p(ind), out[1:])
    assert int(flags.sum()) == 0 and bool(torch.isnan(out[0])) and bool(torch.isnan(out[-1]))
    report(f"logp {shape} + in", out[1:n + 1], OO.logp64(mean, logs, x) + inp.double(), OO.bar(mean, logs, x, inp))
    plain = torch.full((n,), NAN, device=DEV)
    raw_logp(p(xd), c * hw, 0, 0, 0, n, c, hw, 0, plain)                        # NULL mean, logs and in
    report(f"logp {shape} NULL prior", plain, OO.logp64(None, None, x), OO.bar(None, None, x))


@pytest.mark.parametrize("shape", OO.SHAPES, ids=str)
def test_logp_on_strided_views_ignores_the_gaps(shape):
    """x_stride and ml_stride larger than C HW (and different from each other): samples are rows of wider buffers whose gaps hold
    NaN.  Same bits as the dense call."""
    x, mean, logs, _ = OO.logp_case(shape)
    n, c, hw = shape[0], shape[1], shape[2] * shape[3]
    per, xs, mls = c * hw, c * hw + 3, c * hw + 70
    xw, mw, lw = (torch.full((n, s), NAN, device=DEV) for s in (xs, mls, mls))
    xw[:, :per], mw[:, :per], lw[:, :per] = dev(x).view(n, per), dev(mean).view(n, per), dev(logs).view(n, per)
    out = torch.full((n,), NAN, device=DEV)
    flags = raw_logp(p(xw), xs, p(mw), p(lw), mls, n, c, hw, 0, out)
    assert int(flags.sum()) == 0
    report(f"logp {shape} strided", out, OO.logp64(mean, logs, x), OO.bar(mean, logs, x))
    assert torch.equal(out, G.GaussianDiag.logp(dev(mean), dev(logs), dev(x)))


def test_logp_of_an_empty_batch():
    out = G.GaussianDiag.logp(None, None, torch.empty(0, 3, 4, 4, device=DEV))
    assert out.shape == (0,) and out.dtype == torch.float32
    e = torch.empty(0, 3, 4, 4, device=DEV)
    assert G.GaussianDiag.logp(e, e, e).shape == (0,)


def test_logp_refuses_more_elements_than_the_guarantee_covers():
    """P = ceil(C HW / 256) partials with 2^14 P < 2^31 (glowhip.h): one sample of 2^25 elements is refused.  (The buffer is real,
    128 MiB of zeros: a library without the check reads all of it and fails this test, it does not read out of bounds.)"""
    x, out = torch.zeros(1 << 25, device=DEV), torch.zeros(1, device=DEV)
    with pytest.raises(_lib.GlowHipError, match="range guarantee"):
        raw_logp(x.data_ptr(), 1 << 25, 0, 0, 0, 1, 1 << 12, 1 << 13, 0, out)
    del x


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_three_calls_give_the_same_bits():
    for shape in [(5, 3, 7, 11), (2, 12, 33, 31), (300, 2, 3, 5)]:
        x, mean, logs, _ = (dev(t) for t in OO.logp_case(shape))
        a, b, c = (G.GaussianDiag.logp(mean, logs, x).clone() for _ in range(3))
        assert torch.equal(a, b) and torch.equal(a, c)
    x, mean, logs, _, _ = (dev(t) if torch.is_tensor(t) else t for t in OO.range_case("b"))
    a, b, c = (G.GaussianDiag.logp(mean, logs, x).clone() for _ in range(3))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_a_sample_has_the_same_bits_at_every_batch_position():
    """Position 0 of N = 1, 2 of N = 5, 299 of N = 300 (the second workgroup of k_finalize): a wrong accumulator, flag-word or
    extra-row index would mix samples."""
    x1, m1, l1 = OO.the_sample()
    alone = G.GaussianDiag.logp(dev(m1), dev(l1), dev(x1))
    report("the sample alone", alone, OO.logp64(m1, l1, x1), OO.bar(m1, l1, x1))
    for n, pos in ((5, 2), (300, 299)):
        g = torch.Generator().manual_seed(n)
        x, m, l = (torch.randn(n, 2, 3, 5, generator=g) * s for s in (1.0, 0.5, 0.4))
        x[pos], m[pos], l[pos] = x1[0], m1[0], l1[0]
        got = G.GaussianDiag.logp(dev(m), dev(l), dev(x))
        assert got[pos].item() == alone[0].item(), (n, pos, got[pos].item(), alone[0].item())
        report(f"batch of {n}", got, OO.logp64(m, l, x), OO.bar(m, l, x))


# ------------------------------------------------------------------------------------------------ 3. range
def check_range(what, got, want, flags, i, cls, got_ordinary):
    """The rule of the range cases.  got / flags: the call on the batch with the extreme sample i; got_ordinary: the same batch with
    ordinary data in sample i."""
    got, flags, got_ordinary = got.detach().cpu(), flags.cpu(), got_ordinary.detach().cpu()
    others = [k for k in range(len(got)) if k != i]
    v = float(got[i])
    if np.isfinite(v):
        e = abs(v - float(want[i]))
        print(f"{what}: finite, error {e:.3e} (bar {OO.REL * abs(float(want[i])):.3e}), value {v:.9e}, fp64 {float(want[i]):.9e}, flags {int(flags[i])}")
        assert e <= OO.REL * abs(float(want[i])), f"{what}: FINITE AND WRONG: {v!r} for {float(want[i])!r}"
    else:
        print(f"{what}: non-finite ({v}), flags {int(flags[i])}, fp64 {float(want[i]):.9e}")
    # which of the two is documented: finite inside the coarse range, -inf and flag bit 4 beyond it
    if cls == "beyond":
        assert v == -float("inf") and int(flags[i]) == 4, (v, int(flags[i]))
    else:
        assert np.isfinite(v) and int(flags[i]) == 0, (v, int(flags[i]))
    assert int(flags[others].abs().sum()) == 0 and bool(torch.isfinite(got[others]).all())
    assert torch.equal(got[others], got_ordinary[others]), f"{what}: the extreme sample moved its neighbours"


@pytest.mark.parametrize("name", list(OO.RANGE_CASES))
def test_range_of_gaussian_logp(name):
    n, i, what, cls, _ = OO.RANGE_CASES[name]
    x, mean, logs, x0, _ = OO.range_case(name)
    xd, md, ld = dev(x), dev(mean), dev(logs)
    got = G.GaussianDiag.logp(md, ld, xd)
    raw = torch.full((n,), NAN, device=DEV)
    flags = raw_logp(p(xd), 1024, p(md), p(ld), 1024, n, 4, 256, 0, raw)
    assert torch.equal(raw.view(torch.int32), got.view(torch.int32))
    ordinary = G.GaussianDiag.logp(md, ld, dev(x0))
    check_range(f"3({name}) {what}, sample {i} of {n}", got, OO.logp64(mean, logs, x), flags, i, cls, ordinary)
    others = [k for k in range(n) if k != i]
    report(f"3({name}) ordinary samples", got[others], OO.logp64(mean, logs, x)[others], OO.bar(mean, logs, x)[others])


# ------------------------------------------------------------------------------------------------ 4. every kernel with unbounded terms
def test_the_route_cases_are_the_sampler_tests():
    assert set(OO.SPLIT_ROUTES) <= set(TS.ROUTES)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("route,c,h,w", OO.SPLIT_ROUTES)
def test_range_through_every_forward_split_route(route, c, h, w, fam):
    """One element of the dropped half at 1e6 in sample 1 of 3.  Reference: the fp64 density of z2 under the ORACLE's fp64 prior
    (z2 does not feed the convolution)."""
    sd, x, x0 = OO.split_case(c, h, w)
    sp = G.Split2d(c)
    sp.load_state_dict(sd, strict=True)
    sp = sp.to(DEV).eval()
    plan = sp._plans.get([sp], (c, h, w), torch.device(DEV))
    n, i = OO.SPLIT_N, OO.SPLIT_I
    with TS.family(plan, fam):
        plan.encode(dev(x0))                           # (the first call packs: kept out of the launch counts)
        plan.launch_counts(reset=True)
        z1_0, ld_0 = plan.encode(dev(x0))
        st_0 = plan.status(n).cpu()
        plan.launch_counts(reset=True)
        z1, ld = plan.encode(dev(x))
        counts = plan.launch_counts(reset=True)
        st = plan.status(n).cpu()
    routes = {k: v for k, v in counts.items() if k.startswith("split_prior(")}
    assert routes == {f"split_prior({route})": 1}, counts
    assert torch.equal(z1.cpu(), x[:, :c // 2]) and torch.equal(z1_0, z1)
    with torch.no_grad():
        mean, logs, z2 = OO.split_prior64(sd, x)
    want = OO.logp64(mean, logs, z2)
    assert int(st_0.abs().sum()) == 0
    check_range(f"4 {route} ({c}, {h}, {w}) family {fam}", ld, want, st & 7, i, "coarse", ld_0)
    bad = ~torch.isfinite(ld.cpu())
    assert torch.equal(st != 0, bad), (st, ld)        # status is non-zero exactly for the samples reported non-finite


def _objective_model(variant):
    cfg, sd, _, _ = OO.model_case()
    key = dict(OO.MODEL_KEY)
    TS._MODELS[(key["image"], key["L"], key["K"], key["hidden"], key["batch"], key["seed"])] = (cfg, sd)
    glow, _, sd_used = TS._glow(variant, **key)
    assert all(torch.equal(sd_used[k], sd[k]) for k in sd)
    return glow


def test_range_through_the_top_head():
    """k_top_head_fwd, exact-fp32 family: pixels whose top latent has one element at 1e6 (the oracle's decode of that latent), so the
    fp32 reference stays finite and only the accumulator is under test.  Reference: the fp64 oracle on the same pixels."""
    cfg, sd, x, yo = OO.head_case()
    glow = _objective_model("ycond")
    _, want = OO.forward64(x, torch.zeros_like(x), sd, cfg, yo)
    plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))
    with TS.family(plan, plan.FAMILY_EXACT_FP32), torch.no_grad():
        glow.normal_flow(dev(x), dev(yo), noise=torch.zeros_like(dev(x)))
        plan.launch_counts(reset=True)
        z, nll, _ = glow.normal_flow(dev(x), dev(yo), noise=torch.zeros_like(dev(x)))
        counts = plan.launch_counts(reset=True)
        st = plan.status(4).cpu()
        _, nll_0, _ = glow.normal_flow(dev(x[[0, 0, 2, 3]]), dev(yo), noise=torch.zeros_like(dev(x)))
    assert counts.get("k_top_head_fwd") == 1 and "k_gaussian_logp" not in counts, counts
    assert float(z[1].abs().max()) > 0.99e6
    check_range("4 k_top_head_fwd", nll, want, st & 7, 1, "coarse", nll_0)
    assert torch.equal(st != 0, ~torch.isfinite(nll.cpu()))
    others = [0, 2, 3]
    assert float((nll.cpu().double()[others] - want[others]).abs().max()) <= 1e-4


# ------------------------------------------------------------------------------------------------ 5. one whole model
def test_whole_model_on_pixels_scaled_by_1e4():
    """32x32, L 3, K 2 (objective_oracle.model_case says why its zero-initialised heads are at 1e-6), pixels times 1e4: the fp64
    oracle's nll is finite, ~3e8 bits/dim = 6e11 nats.  The project's bar on an nll is 1e-4 ABSOLUTE on values of a few bits/dim,
    1e-5 relative; at 3e8 one fp32 ulp is 32, so the range cases' 1e-6 relative (tighter) is the bar here.  Exact-fp32 family: finite
    and within it.  The product family and safe=True: non-finite or within it, never finite and off."""
    cfg, sd, x, noise = OO.scaled_case()
    _, want = OO.forward64(x, noise, sd, cfg)
    assert bool(torch.isfinite(want).all())
    glow = _objective_model("plain")
    plan = glow.flow.plan_for(glow.flow.in_chw, torch.device(DEV))

    def rule(what, nll, must_be_finite):
        nll = nll.detach().cpu().double()
        for k in range(4):
            v, w = float(nll[k]), float(want[k])
            if np.isfinite(v):
                print(f"5 {what} sample {k}: finite, error {abs(v - w):.3e} (bar {OO.REL * abs(w):.3e}), value {v:.9e}, fp64 {w:.9e}")
                assert abs(v - w) <= OO.REL * abs(w), f"{what} sample {k}: FINITE AND WRONG: {v!r} for {w!r}"
            else:
                print(f"5 {what} sample {k}: non-finite ({v}), fp64 {w:.9e}")
                assert not must_be_finite

    with torch.no_grad():
        with TS.family(plan, plan.FAMILY_EXACT_FP32):
            _, nll, _ = glow.normal_flow(dev(x), None, noise=dev(noise))
            st = plan.status(4).cpu()
            rule("exact-fp32 family", nll, True)
            assert int(st.abs().sum()) == 0
        _, nll, _ = glow.normal_flow(dev(x), None, noise=dev(noise))
        st = plan.status(4).cpu()
        rule("product family", nll, False)
        assert torch.equal((st & 7) != 0, ~torch.isfinite(nll.cpu()))
        _, nll, _ = glow.normal_flow(dev(x), None, noise=dev(noise), safe=True)
        rule("safe=True", nll, False)

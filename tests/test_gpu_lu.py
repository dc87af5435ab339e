"""`-m gpu`: every factorisation of the invertible 1x1 convolution weight (csrc/lu.hip, csrc/lu_wave.h) held to ONE fp32 ulp of
an fp64 reference, on matrices that force the pivoting decisions (tests/lu_oracle.py: cyclic, anti, sign, graded, tiny; orth is
the suite's usual matrix).  The kernels work in fp64 and store fp32, so the bounds are derived from the arithmetic (lu_oracle,
DESIGN.md "LU routes against fp64") and are not tuned: a correct kernel that exceeds one is a finding.  Which route ran is read from
the run-time launch counters (plan.launch_counts: the pack kernel and, for k_step_prepare_batched, the factorisation per matrix),
never inferred from C.  The yardstick is numpy's fp64 slogdet / inv, not the reference's fp32 torch.det / inverse
(network/module.py:356-365), which is +-inf or 0 on `sign` and `tiny`; tests/test_lu_oracle_host.py checks it on the host.

Through a plan the FlowStep is additive with its freshly constructed f.4 (zeros) and an identity ActNorm on a 4x4 map, so that
ld_out = 16 * float(lad) (16 is a power of two: the product and the Q31.32 accumulation of a multiple of 2^-20 are exact) and
z = W x."""
import functools

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd._lib import check, lib, ptr, stream_ptr
from oracle import glow_oracle as O
import lu_oracle as LU
from test_gpu_parity import DEV, dev, make_glow

pytestmark = pytest.mark.gpu
DBG = _lib.DBG
HW = 16
MIX_SH2 = "k_dn_gemm(mix)"          # the channel mixer on the split-fp16 GEMM (csrc/dnet_sh.hip) -- from the launch counters


def _report(route, what, case, multiple):
    """One line per checked quantity: the multiple of its bound (collected into DESIGN.md's table by reading the -s output)."""
    print(f"LU-BOUND route={route} what={what} case={case} multiple={multiple:.4f}")
    return multiple


def _ids(cases):
    return ["-".join(str(v).replace("pack:", "").replace("lu:", "") for v in c) for c in cases]


# ---------------------------------------------------------------- the stand-alone call (routes 4 and 5)
def _prepare(W):
    """glowhip_invconv_prepare on a float32 (C, C) numpy matrix, every output and the scratch pre-filled with 0xA5 bytes."""
    C = W.shape[0]
    w = torch.from_numpy(np.array(W, dtype=np.float32)).to(DEV)
    aux = torch.full((4 * (C * C + 1),), 0xA5, dtype=torch.uint8, device=DEV).view(torch.float32)
    winv, lad = aux[:C * C], aux[C * C:]
    scratch = torch.full((int(lib().glowhip_invconv_scratch_bytes(C)),), 0xA5, dtype=torch.uint8, device=DEV)
    check(lib().glowhip_invconv_prepare(ptr(w), C, ptr(winv), ptr(lad), ptr(scratch), stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return winv.cpu().numpy().reshape(C, C).copy(), float(lad.cpu().item())


def _check_standalone(family, C, route):
    W = LU.matrix(family, C)
    ref_ld, ref_inv = LU.reference(family, C)
    winv, lad = _prepare(W)
    assert np.isfinite(lad) and np.isfinite(winv).all(), (family, C)
    m_ld = _report(route, "logdet", f"{family}-{C}", abs(lad - ref_ld) / LU.logdet_bound(ref_ld))
    m_inv = _report(route, "inverse", f"{family}-{C}",
                    float((np.abs(winv.astype(np.float64) - ref_inv) / LU.inverse_bound(ref_inv)).max()))
    assert m_ld <= 1.0, (family, C, lad, ref_ld)
    assert m_inv <= 1.0, (family, C, m_inv)
    if family == "cyclic":
        # every operation on a scaled permutation is exact: the VALUES are the reference's, entry for entry (the sign of a zero
        # is the one thing not held: -0 = 0 / negative pivot is as right as the +0 numpy's elimination order leaves)
        assert np.array_equal(winv.astype(np.float64), ref_inv), (family, C)
        assert np.array_equal(ref_inv, LU.cyclic_exact(C, LU.SEED)[1])


STANDALONE = [(f, C, r) for r, Cs in LU.STANDALONE_C.items() for C in Cs for f in LU.families_for(C)]


@pytest.mark.parametrize("family,C,route", STANDALONE, ids=_ids(STANDALONE))
def test_standalone_prepare_against_fp64(family, C, route):
    """glowhip_invconv_prepare: Gauss-Jordan on [W | I] in LDS (C <= 64) and in the global scratch buffer (above; the widths are
    lu.hip launch_invconv_prepare's -- this call has no plan and so no counters): W^-1 elementwise and log|det W| within one fp32
    ulp of fp64; `cyclic` value for value."""
    _check_standalone(family, C, "gauss_jordan(" + route + ")")


# ---------------------------------------------------------------- one FlowStep as a plan
_STEPS = {}


def _step(C):
    """The FlowStep of width C (hidden 64, additive, fresh zero f.4, identity ActNorm marked inited) and its plan for a 4x4 map;
    built once per width -- the tests write the invconv weight in place, as an optimiser step would."""
    if C not in _STEPS:
        np.random.seed(C)
        torch.manual_seed(C)
        st = G.FlowStep(C, 64, permutation="invconv", coupling="additive")
        for m in st.modules():
            if isinstance(m, G.ActNorm):
                m.bias_inited = m.logs_inited = True
        st = st.to(DEV).eval()
        f4 = st.f[4]
        assert not f4.weight.any() and not f4.bias.any() and not f4.logs.any()
        assert not st.actnorm.logs.any() and not st.actnorm.bias.any()
        _STEPS[C] = (st, st._plan(torch.empty(2, C, 4, 4, device=DEV)))
    return _STEPS[C]


@functools.lru_cache(maxsize=None)
def _pixels(C, seed):
    return torch.randn(2, C, 4, 4, generator=torch.Generator().manual_seed(1000 * seed + C))


def _set_weight(st, W):
    st.invconv.weight.copy_(torch.from_numpy(np.array(W, dtype=np.float32)).to(DEV))


def _run(C, W, flags=0, reverse=False):
    """(output, ld_out, launch counters) of one call with a forced re-pack under the debug `flags`; ld_in = 0."""
    st, plan = _step(C)
    _set_weight(st, W)
    x = dev(_pixels(C, 2 if reverse else 1))
    ld0 = torch.zeros(2, device=DEV)
    plan.launch_counts(reset=True)
    with _lib.debug_flags(flags):
        if reverse:
            out, ld = plan.decode(x, [], ld0, want_logdet=True, repack=True)
        else:
            out, ld = plan.encode(x, None, ld0, want_logdet=True, repack=True)
    torch.cuda.synchronize()
    return out.cpu(), ld.cpu(), plan.launch_counts(reset=True)


def _apply_multiple(M, v, out, counts):
    """max |out - M v| / bound, M (C, C) float64 exact reference matrix, v / out (N, C, 4, 4) fp32.  fp32 mixers: the dot-product
    bound for any accumulation order, (C + 2) 2^-24 (|M| |v|) (lu_oracle.apply_bound).  Mixers on the split-fp16 GEMM (dnet_sh.hip,
    read from the counters): lu_oracle.apply_bound_sh2, derived there from csrc/sh.h."""
    n, C = v.shape[0], v.shape[1]
    vv = v.numpy().astype(np.float64).transpose(1, 0, 2, 3).reshape(C, -1)
    oo = out.numpy().astype(np.float64).transpose(1, 0, 2, 3).reshape(C, -1)
    assert np.isfinite(oo).all()
    bound = LU.apply_bound_sh2(M, vv) if counts.get(MIX_SH2) else LU.apply_bound(M, vv)
    err = np.abs(oo - M @ vv)
    return float((err / np.maximum(bound, 1e-300)).max()), "sh2" if counts.get(MIX_SH2) else "fp32"


def _check_forward(family, C, flags, kernel, route, W=None, ref_ld=None):
    """One forward-only pack + encode: the pack kernel and the factorisation from the counters, ld_out / 16 against fp64 with the
    stand-alone bound, z against W x.  Returns the raw (z, ld_out) for bitwise comparisons."""
    if W is None:
        W, ref_ld = LU.matrix(family, C), LU.reference(family, C)[0]
    z, ld, c = _run(C, W, flags)
    assert c.get(kernel) == 1 and sum(v for k, v in c.items() if k.startswith("pack:k_")) == 1, (kernel, c)
    assert [k for k in c if k.startswith("pack:lu:")] == ([route] if route else []) and (not route or c[route] == 1), (route, c)
    name = route.replace("pack:lu:", "") if route else "wave:" + kernel.replace("pack:", "")
    assert torch.isfinite(ld).all() and ld[0] == ld[1], ld
    m = _report(name, "plan-logdet", f"{family}-{C}", abs(ld[0].item() / HW - ref_ld) / LU.logdet_bound(ref_ld))
    assert m <= 1.0, (family, C, ld[0].item() / HW, ref_ld)
    mz, mixer = _apply_multiple(np.asarray(W, dtype=np.float64), _pixels(C, 1), z, c)
    _report(name, f"z({mixer})", f"{family}-{C}", mz)
    assert mz <= 1.0, (family, C, mz)
    return z, ld


WAVE = [(f, C) for C in LU.WAVE_C for f in LU.ALL]


@pytest.mark.parametrize("family,C", WAVE, ids=_ids(WAVE))
def test_one_wave_lu_three_routes_same_bits(family, C):
    """C = 12 / 24 / 48 on the one-wave LU inside k_pack_fused, the same inside k_step_prepare_small (DBG.PACK_UNFUSED) and on the
    workgroup LU in LDS (DBG.LU_WORKGROUP): each within the bound, and all three the same BITS (lu_wave.h: same operations in the
    same order) -- on `sign`, whose columns are ties, that holds only with the same lowest-row rule in both forms."""
    a = _check_forward(family, C, 0, LU.FUSED, None)
    b = _check_forward(family, C, DBG.PACK_UNFUSED, LU.SMALL, None)
    w = _check_forward(family, C, DBG.LU_WORKGROUP, LU.BATCHED, LU.R_LDS)
    for other in (b, w):
        assert torch.equal(a[1], other[1]) and torch.equal(a[0], other[0]), (family, C, a[1], other[1])


FORWARD = LU.forward_cases()


@pytest.mark.parametrize("family,C,route", FORWARD, ids=_ids(FORWARD))
def test_forward_pack_workgroup_and_blocked_lu(family, C, route):
    """The forward-only pack's log|det W| beyond the one-wave widths: lu_logdet_only in LDS (16 ... 128), the blocked LU (130: a
    2-column last panel, 160: full panels only, 200, 448: the widest) and lu_logdet_only in global scratch (450, 512) -- 64 | 66,
    128 | 130 and 448 | 450 straddle the route borders."""
    _check_forward(family, C, 0, LU.BATCHED, route)


INVERSE = [(f, C) for C in LU.INVERSE_PACK_C for f in LU.INVERSE_PACK_FAMILIES]


@pytest.mark.parametrize("family,C", INVERSE, ids=_ids(INVERSE))
def test_inverse_pack_and_decode(family, C):
    """decode of the same plans: the inverting pack (Gauss-Jordan, LDS up to 64, global above -- from the counters), ld_out =
    -16 lad with the plan bound and x = W^-1 z with the dot-product bound (a wrong offset or a stale winv is what this is for; the
    accuracy of W^-1 itself is the stand-alone test's)."""
    W = LU.matrix(family, C)
    ref_ld, ref_inv = LU.reference(family, C)
    x, ld, c = _run(C, W, reverse=True)
    route = LU.R_GJ_LDS if C <= 64 else LU.R_GJ_GLOBAL          # (which widths each is EXPECTED at; the counter decides)
    assert c.get(LU.BATCHED) == 1 and [k for k in c if k.startswith("pack:lu:")] == [route], c
    name = route.replace("pack:lu:", "")
    assert torch.isfinite(ld).all() and ld[0] == ld[1], ld
    m = _report(name, "plan-logdet(rev)", f"{family}-{C}", abs(-ld[0].item() / HW - ref_ld) / LU.logdet_bound(ref_ld))
    assert m <= 1.0, (family, C, -ld[0].item() / HW, ref_ld)
    mx, mixer = _apply_multiple(ref_inv, _pixels(C, 2), x, c)
    _report(name, f"x({mixer})", f"{family}-{C}", mx)
    assert mx <= 1.0, (family, C, mx)


# ---------------------------------------------------------------- whole plans: mixed widths, many steps
def _model(image, K, L, families, seed):
    """A Glow of K x L FlowSteps (hidden 64) whose invconv weights are the families' matrices and whose ActNorm logs are seeded
    N(0, 0.1); returns (plan, [(HW, logs float32 (C,), family, C)] in layer order)."""
    cfg = O.default_cfg(image_shape=(image, image, 3), hidden_channels=64, K=K, L=L, flow_coupling="additive", batch=1)
    sd = O.seeded_state_dict(cfg, seed=seed, zeros_std=0.01)
    g = torch.Generator().manual_seed(seed + 1)
    steps = []
    for kind, i, (c, h, w) in O.flow_layout(cfg):
        if kind != "step":
            continue
        fam = families(len(steps), c)
        p = f"flow.layers.{i}."
        sd[p + "invconv.weight"] = torch.from_numpy(np.array(LU.matrix(fam, c)))
        sd[p + "actnorm.logs"] = torch.randn(1, c, 1, 1, generator=g) * 0.1
        steps.append((h * w, sd[p + "actnorm.logs"].flatten().numpy().copy(), fam, c))
    glow = make_glow(cfg, sd, 1)
    return glow, glow.flow.plan_for(torch.empty(1, 3, image, image, device=DEV)), steps


def _total_and_bound(steps):
    """sum_i HW_i (3 sum logs_i + lad_i) in fp64 -- each logs * 3 product taken in FLOAT as lu.hip does -- and its bound
    sum_i HW_i 2^-24 (|lad_i| + 3 sum_c |logs_i,c|) + 1e-9 sum_i HW_i."""
    total = bound = 0.0
    for hw, logs, fam, c in steps:
        lad = LU.reference(fam, c)[0]
        total += hw * (float((logs * np.float32(3.0)).astype(np.float64).sum()) + lad)
        bound += hw * 2.0 ** -24 * (abs(lad) + 3.0 * float(np.abs(logs.astype(np.float64)).sum())) + 1e-9 * hw
    return total, bound


def _pack_total(plan, use, flags=0):
    """packed[0] (the plan-wide log-det constant) of a pack into a buffer of 0xA5 bytes, the whole buffer, and the counters."""
    plan.packed = torch.full_like(plan.packed, 0xA5)
    plan.launch_counts(reset=True)
    with _lib.debug_flags(flags):
        plan.pack(use, merge=False)
    plan.pack_sync()
    torch.cuda.synchronize()
    return plan.packed[:8].view(torch.float64).item(), plan.packed.clone(), plan.launch_counts(reset=True)


def test_mixed_widths_in_one_launch():
    """K = 1, L = 6 on 256 x 256: C = 12 ... 384 in ONE k_step_prepare_batched launch, a different family per level, pack only.
    The forward-only pack (LDS LU at 12 ... 96, blocked at 192 and 384) and the inverting pack (Gauss-Jordan, LDS up to 48, global
    above) each within the bound of the fp64 total, and within the sum of both bounds of each other."""
    fams = dict(LU.MIXED)
    glow, plan, steps = _model(256, 1, 6, lambda i, c: fams[c], seed=11)
    assert [c for _, _, _, c in steps] == [c for c, _ in LU.MIXED]
    total, bound = _total_and_bound(steps)
    fwd, _, cf = _pack_total(plan, plan.PACK_INFERENCE)
    inv, _, ci = _pack_total(plan, plan.PACK_INFERENCE | plan.PACK_INVERSE)
    assert cf.get(LU.BATCHED) == 1 and cf.get(LU.R_LDS) == 4 and cf.get(LU.R_BLOCKED) == 2 and LU.R_GLOBAL not in cf, cf
    assert ci.get(LU.BATCHED) == 1 and ci.get(LU.R_GJ_LDS) == 3 and ci.get(LU.R_GJ_GLOBAL) == 3, ci
    mf = _report("mixed(forward)", "total", "K1-L6-256", abs(fwd - total) / bound)
    mi = _report("mixed(inverse)", "total", "K1-L6-256", abs(inv - total) / bound)
    assert mf <= 1.0 and mi <= 1.0, (fwd, inv, total, bound)
    assert abs(fwd - inv) <= 2 * bound, (fwd, inv, bound)


def test_more_than_256_flowsteps():
    """260 FlowSteps of width 12 (L = 1 on a 4 x 4 image): k_sum_konst's loop, and its copy in k_pack_fused's last arriver, take a
    second trip.  The families alternate.  packed[0] from k_pack_fused, from k_step_prepare_small + k_sum_konst and from the
    workgroup LU + k_sum_konst: the same BITS (each sums in layer order), each within the bound."""
    K = 260
    glow, plan, steps = _model(4, K, 1, lambda i, c: LU.MANY_STEPS_FAMILIES[i % len(LU.MANY_STEPS_FAMILIES)], seed=12)
    assert len(steps) == K and all(c == 12 and hw == 4 for hw, _, _, c in steps)
    total, bound = _total_and_bound(steps)
    got = {}
    for name, flags, kernel in (("fused", 0, LU.FUSED), ("small", DBG.PACK_UNFUSED, LU.SMALL), ("workgroup", DBG.LU_WORKGROUP, LU.BATCHED)):
        t, _, c = _pack_total(plan, plan.PACK_INFERENCE, flags)
        assert c.get(kernel) == 1 and sum(v for k, v in c.items() if k.startswith("pack:k_")) == 1, (name, c)
        if name == "workgroup":
            assert c.get(LU.R_LDS) == K, c
        m = _report(f"many-steps({name})", "total", f"K{K}", abs(t - total) / bound)
        assert m <= 1.0, (name, t, total, bound)
        got[name] = t
    assert got["fused"] == got["small"] == got["workgroup"], got


# ---------------------------------------------------------------- never a finite wrong answer
def _bad(kind, C):
    W = np.array(LU.matrix("orth", C))
    if kind == "equal-rows":
        W[C - 1] = W[1 % C]
    elif kind == "zero-column":
        W[:, C // 2] = 0.0
    elif kind == "nan":
        W[C // 3, C // 2] = np.nan
    else:
        W[C // 3, C // 2] = np.inf
    return W


@pytest.mark.parametrize("C", [12, 66, 200])
@pytest.mark.parametrize("kind", ["equal-rows", "zero-column", "nan", "inf"])
def test_singular_or_non_finite_weight_is_never_a_finite_answer(kind, C):
    """Two equal rows, a zero column, one NaN, one +inf: the stand-alone call's lad is non-finite and the forward-only plan's ld_out
    is non-finite (or the plan's status word is flagged) -- and the next call on the same plan with a good W is within the bound
    again: nothing sticky in scratch, LDS or the arrival counter.  No index in lu.hip / lu_wave.h depends on a matrix VALUE (the
    pivot row starts at k and is only replaced by a row the loop visits; the one-wave form's positions stay a permutation, so its
    owner ballot is never empty): defined arithmetic on bad numbers.  The
    log-det itself must be non-finite, not only the flag that z raises (the one-wave LU once returned a finite log-det for a NaN
    entry: a NaN candidate lost every comparison of its pivot search; lu_wave.h).

    Two equal rows: every route eliminates in multiplier form (l = a / pivot, fma(-l, pivot row, a)), so a row equal to the pivot
    row has l = 1 and cancels EXACTLY, its pivot is 0 and log 0 = -inf.  This test found two routes that did not: Gauss-Jordan
    scaled the pivot row first and eliminated with fma(-a, row / pivot, a'), which leaves the rounding residue of the division, and
    the blocked LU subtracted a dot product accumulated from zero from a row whose U part was accumulated from the element -- both
    ended on a pivot ~1e-17 and a FINITE log-det (stand-alone lad = -38.65 / -37.55 / -38.10 at C = 12 / 66 / 200, blocked plan
    ld_out / 16 = -37.70 with status 0) until lu_gauss_jordan took multipliers and lu_logdet_blocked's trailing update started
    from the element."""
    W = _bad(kind, C)
    _, lad = _prepare(W)
    st, plan = _step(C)
    z, ld, c = _run(C, W)
    status = plan.status(2, dev(z)).cpu()
    print(f"LU-BAD kind={kind} C={C} standalone lad={lad} plan ld_out={ld.tolist()} status={status.tolist()}")
    kernel, route = (LU.FUSED, None) if C == 12 else (LU.BATCHED, LU.R_LDS if C == 66 else LU.R_BLOCKED)
    assert c.get(kernel) == 1 and (route is None or c.get(route) == 1), c
    # (the good matrix first: whatever the two asserts below say, nothing sticky may be left behind)
    _check_standalone("orth", C, "gauss_jordan(after-bad)")
    _check_forward("orth", C, 0, kernel, route)
    assert not np.isfinite(lad), (kind, C, lad)
    assert bool(((~torch.isfinite(ld)) | (status != 0)).all()), (kind, C, ld, status)
    assert not torch.isfinite(ld).any(), (kind, C, ld)      # the log-det itself, not only z's flag


@pytest.mark.parametrize("C,route", [(448, LU.R_BLOCKED), (512, LU.R_GLOBAL)])
def test_two_packs_into_poisoned_buffers_same_bits(C, route):
    """`sign` at the widest blocked and the widest supported unblocked width, packed twice into buffers of 0xA5 bytes: every byte
    of `packed` (scratch included) the same -- nothing depends on what the buffer held or on the order workgroups ran in."""
    st, plan = _step(C)
    _set_weight(st, LU.matrix("sign", C))
    a, pa, ca = _pack_total(plan, plan.PACK_INFERENCE)
    b, pb, cb = _pack_total(plan, plan.PACK_INFERENCE)
    assert ca.get(route) == 1 and cb.get(route) == 1, (ca, cb)
    assert torch.equal(pa, pb)
    ref = HW * LU.reference("sign", C)[0]
    assert a == b and abs(a / HW - ref / HW) <= LU.logdet_bound(ref / HW), (a, ref)

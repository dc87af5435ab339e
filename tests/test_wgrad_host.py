"""CPU checks of the weight-gradient GEMM tests' own instruments (tests/wgrad_oracle.py): the fp64 reference against float64
autograd, the packers, and -- the yardstick -- a numpy emulation of the kernel's arithmetic (np.float16 splits, the kept products,
fp32 accumulation per split, the merge, the ordered reduction) that must stay inside bound() on every `random` input set
tests/test_gpu_wgrad.py launches and equal the reference exactly on every `exact` one, and must LEAVE both when it is edited the way
a wrong kernel would be.

What the edits can and cannot show.  An edit breaks exactness on every `exact` set that carries the term it removes: a dropped
a.lo x b.hi on `exact1` (A = +-(1 + j 2^-11): lo plane non-zero; `exact2` has integer A, whose lo plane is zero, and cannot see it),
a dropped a.hi x b.lo on `exact2` (B = i + j 2^-11), a lost k-tile on both, the missing row-sum rescale on every pre-scaled A.  On the
`random` family the bound's accumulation term is a worst case growing with the pixel axis while a dropped plane's error grows with
its square root, so `random` sees a dropped plane only on short axes (SHORT_K pixels and fewer here; the measured ratio is printed
per length); on long axes only `exact` is sensitive, and the bound is not tightened to hide that."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_oracle as W

F32 = np.float32
SHORT_K = 128          # pixels over the whole batch: the `random` sets on which every plane edit must leave the bound


# ---------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------
def split(x, pre):
    """csrc/sh.h on x * pre (fp32): hi = fp16(x'), lo = fp16((x' - hi) 2^11)."""
    xp = (x.astype(F32) * F32(pre)).astype(F32)
    hi = xp.astype(np.float16)
    lo = ((xp - hi.astype(F32)) * F32(W.LO)).astype(np.float16)
    return hi.astype(F32), lo.astype(F32)


def emulate(case, d, splits, per, edit=None, rs_init=None):
    """dW (flat, fp32 as float64) and the row sums (float64) as the split-half kernels compute them, in ONE of the orders they may
    take.  edit: None | 'al_bh' | 'ah_bl' | 'last_tile' | 'rowsum_scale'."""
    Mr, Nr, ps = case["Mreal"], case["Nreal"], case["a"] == "ps"
    A_st = W.expand(d["A_ref"], -1) if case["a"] == "taps" else d["A_ref"]
    B_st = W.expand(d["B_ref"], +1) if case["b"] == "taps" else d["B_ref"]
    a_all, b = W.as_matrix(A_st), W.as_matrix(B_st)[:Nr]
    a = a_all[:Mr]
    sh = d["sh_scale"]
    a_pre = 1.0 / W.LO if ps else sh
    ah, al = split(a, a_pre)
    if case["b"] == "half":
        bh, bl = b.astype(F32), None
    else:
        bh, bl = split(b, 1.0)
    K = a.shape[1]
    dw = np.zeros((Mr, Nr), F32)
    rs = None if rs_init is None else rs_init.astype(np.float64).copy()
    inv = F32(1.0 / sh)
    for s in range(splits):
        k0, k1 = 32 * per * s, min(K, 32 * per * (s + 1))
        if edit == "last_tile":
            k1 -= 32
        sl = slice(k0, max(k0, k1))
        accm = ah[:, sl] @ bh[:, sl].T
        accx = np.zeros_like(accm)
        if bl is not None and edit != "ah_bl":
            accx = accx + ah[:, sl] @ bl[:, sl].T
        if edit != "al_bh":
            accx = (accx + al[:, sl] @ bh[:, sl].T).astype(F32)
        dw = (dw + ((accm + accx * F32(1.0 / W.LO)).astype(F32) * inv).astype(F32)).astype(F32)
        if rs is not None:
            part = a_all[:, sl].astype(F32).sum(1, dtype=F32).astype(np.float64)
            rs += part * (1.0 if edit == "rowsum_scale" else float(F32(a_pre) / F32(sh)))
    return W.to_layout(dw.astype(np.float64), case["mode"], Mr, Nr), rs


def emulate_f32(case, d, splits, per):
    """k_wgrad_gemm<64 / 128>: fp32 products and sums per split, the ordered reduction."""
    Mr, Nr = case["Mreal"], case["Nreal"]
    a, b = W.as_matrix(d["A_ref"])[:Mr].astype(F32), W.as_matrix(d["B_ref"])[:Nr].astype(F32)
    dw = np.zeros((Mr, Nr), F32)
    for s in range(splits):
        sl = slice(32 * per * s, min(a.shape[1], 32 * per * (s + 1)))
        dw = (dw + a[:, sl] @ b[:, sl].T).astype(F32)
    return W.to_layout(dw.astype(np.float64), case["mode"], Mr, Nr)


def launch_shape(case):
    if "splits_per" in case:      # a GEMM of a grouped launch: its share of the workgroups decides
        return case["splits_per"]
    total = case["N"] * case["HW"] // 32
    wide = case["a"] == "ps" and case["b"] == "half" and case["Npad"] % 256 == 0 and total >= 512
    return W.expected_splits(case["Mpad"], case["Npad"], total, wide)


def case_bound(case, d, splits, per):
    return W.bound(d["absd"], splits, per, d["kind"], d["sh_scale"], d["sum_a"], d["sum_b"], case["mode"], case["Mreal"], case["Nreal"])


GROUPS = W.group_cases()
ALL_CASES = W.shape_cases() + W.reduce_cases() + W.loop_cases() + W.wide_cases() + [c for g in GROUPS for c in g["sub"].values()]


def test_case_table_reaches_what_it_claims():
    """Loop lengths 1 .. 8 on the three loop forms, a shorter last split, fewer k-tiles than splits, the reduction's split counts,
    k_wgrad_gemm_ps512's threshold; grouped launches whose live block counts are no multiple of 8 and whose share rounds both ways."""
    loops = {c["name"]: launch_shape(c) for c in W.loop_cases()}
    for form in ("3", "2", "ps"):
        assert [loops[f"loop{form}-per{p}"] for p in range(1, 9)] == [(32, p) for p in range(1, 9)]
        assert loops[f"loop{form}-short-last"] == (32, 3) and 47 * 2 - 31 * 3 == 1
        assert loops[f"loop{form}-one-tile-each"] == (10, 1)
    assert sorted({launch_shape(c)[0] for c in W.reduce_cases()}) == [1, 7, 8, 9, 17]
    assert [launch_shape(c) for c in W.wide_cases()] == [(128, 4), (32, 16)]
    decided = [f for g in GROUPS for f, used in g["frac"].values() if used]
    assert any(f < 0.5 for f in decided) and any(f >= 0.5 for f in decided)
    live = [(k, g["sub"][k]["splits_per"][0] * g["tiles"][k]) for g in GROUPS for k in g["sub"]]
    assert any(k == "f4" and n % 8 for k, n in live) and any(k == "f2" and n % 8 for k, n in live) and any(k == "f0" and n % 8 for k, n in live)


# ---------------------------------------------------------------------------------------------------------------------
# reference and packers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W_", [(8, 4), (6, 10), (16, 16)])
@pytest.mark.parametrize("N", [1, 3])
def test_reference_equals_float64_autograd_of_conv2d(H, W_, N):
    """dw_ref for f.4, f.2 and f.0 against torch.autograd of F.conv2d in float64: 1e-12 relative per element (relative to the
    element's sum of magnitudes: both sides are fp64 sums of the same products in different orders).  Worst seen: 2.5e-16."""
    g = torch.Generator().manual_seed(100 * H + 10 * W_ + N)
    Cin, hid, Cout = 3, 5, 4
    worst = 0.0
    for name, ci, co, ks in (("f.0", Cin, hid, 3), ("f.2", hid, hid, 1), ("f.4", hid, Cout, 3)):
        x = torch.randn(N, ci, H, W_, generator=g, dtype=torch.float64)
        w = torch.randn(co, ci, ks, ks, generator=g, dtype=torch.float64, requires_grad=True)
        gy = torch.randn(N, co, H, W_, generator=g, dtype=torch.float64)
        with torch.enable_grad():
            F.conv2d(x, w, padding=ks // 2).backward(gy)
        want = w.grad.numpy().reshape(-1)
        gyn, xn = gy.numpy(), x.numpy()
        if name == "f.2":
            args = (gyn.reshape(N, co, -1), xn.reshape(N, ci, -1), 0, co, ci, None)
        elif name == "f.4":      # A = gathered g (sign -1), B = the input, mode 1
            args = (gyn, xn.reshape(N, ci, -1), 1, 9 * co, ci, (0, -1))
        else:                    # A = g, B = gathered input (sign +1), mode 0
            args = (gyn.reshape(N, co, -1), xn, 0, co, 9 * ci, (1, +1))
        got, mag = W.dw_ref(*args), W.absdot(*args)
        rel = float((np.abs(got - want) / mag).max())
        worst = max(worst, rel)
        assert rel <= 1e-12, (name, rel)
        if ks == 3:
            d_ref, d_abs = W.direct_ref(gyn, xn, 3)
            assert float((np.abs(d_ref - want) / d_abs).max()) <= 1e-12
    print(f"reference vs float64 autograd {H}x{W_} N={N}: worst {worst:.2e} of the sum of magnitudes")


def test_packers_round_trip():
    rs = np.random.RandomState(0)
    for N, R, HW, rp in ((1, 5, 32, 8), (3, 128, 64, 128), (2, 54, 96, 64)):
        x = rs.randn(N, R, HW).astype(np.float32)
        flat = W.pack_tiled(x, rp)
        assert flat.shape == (N * HW // 32 * rp * 32,)
        assert np.array_equal(W.unpack_tiled(flat, N, R, HW, rp), x)
        # element (pixel tile t, row r, lane l) of the image is pixel 32 t + l of the batch's pixels
        t, r, l = (N * HW // 32) - 1, R - 1, 7
        pix = 32 * t + l
        assert flat[(t * rp + r) * 32 + l] == x[pix // HW, r, pix % HW]
        assert np.array_equal(W.pad_rows(x, rp)[:, :R], x) and not W.pad_rows(x, rp)[:, R:].any()
    t = rs.randn(2, 3, 4, 8)
    e = W.expand(t, +1, 32).reshape(2, 32, 4, 8)
    assert e[1, 2 * 9 + 0, 1, 1] == t[1, 2, 0, 0] and e[1, 2 * 9 + 8, 0, 0] == t[1, 2, 1, 1] and e[0, 4, 3, 7] == t[0, 0, 3, 7]
    assert not e[:, 27:].any() and not e[:, 0::9, 0, :].any() and not e[:, 2::9, :, 7].any()
    m = W.expand(t, -1).reshape(2, 27, 4, 8)
    assert m[0, 9 + 0, 0, 0] == t[0, 1, 1, 1] and not m[:, 0::9, 3, :].any()
    C = np.arange(18 * 5).reshape(18, 5).astype(np.float64)
    assert W.to_layout(C, 1, 18, 4)[(1 * 4 + 2) * 9 + 7] == C[1 * 9 + 7, 2] and W.to_layout(C, 0, 17, 3)[2 * 3 + 1] == C[2, 1]


# ---------------------------------------------------------------------------------------------------------------------
# yardstick and sensitivity
# ---------------------------------------------------------------------------------------------------------------------
_figures = {}


def _ratio(err, bnd):
    return float(np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))))


def test_emulation_stays_inside_the_bound_and_is_exact_on_every_input_set():
    """Every input set of tests/test_gpu_wgrad.py: the `exact` conditions hold (reference an fp32 number on every element, sum of
    magnitudes below 2^24 granules), the unedited emulation returns the reference value for value there and stays inside bound() on
    the `random` sets -- row sums included.  Measured (this run prints them): worst multiple of the bound 0.78 (dW: a gathered A's 1e-7 rows at an image corner, where one
    product carries the fp16-subnormal floor alone), 0.03 (row sums); 10 669 584 exact values compared, none differs."""
    worst, worst_rs, n_exact = 0.0, 0.0, 0
    for case in ALL_CASES:
        splits, per = launch_shape(case)
        for fam in case["families"]:
            d = W.build_mfma(case, fam)
            init = None
            if case["rowsum"]:
                init = np.linspace(-3.0, 5.0, case["Mpad"]) * (1.0 if fam != "random" else 1.0 / d["sh_scale"])
            got, rs = emulate(case, d, splits, per, rs_init=init)
            if fam == "random":
                r = _ratio(np.abs(got - d["ref"]), case_bound(case, d, splits, per))
                worst = max(worst, r)
                assert r <= 1.0, (case["name"], fam, r)
            else:
                assert W.exact_ok(d["ref"], d["absd"], d["granule"]), (case["name"], fam)
                assert np.array_equal(got, d["ref"]), (case["name"], fam, int((got != d["ref"]).sum()))
                n_exact += got.size
            if init is not None:
                r = _ratio(np.abs(rs - (init + d["rs_ref"])), W.bound_rowsum(d["rs_abs"], splits, per, init))
                worst_rs = max(worst_rs, r)
                assert r <= 1.0, (case["name"], fam, "rowsum", r)
    print(f"unedited emulation: worst multiple of the bound {worst:.3f} (dW), {worst_rs:.3f} (row sums); {n_exact} exact values compared, 0 differ")


SENS_CASES = [c for c in W.shape_cases() + W.reduce_cases() if c["sh"]] + [c for c in W.loop_cases() if c["name"].endswith(("per1", "per3", "per8", "short-last"))]


@pytest.mark.parametrize("edit", ["al_bh", "ah_bl", "last_tile", "rowsum_scale"])
def test_an_edited_emulation_leaves_the_bound_and_breaks_exactness(edit):
    """Each edit in turn (module docstring).  Measured factors by which the edited emulation leaves the bound on the short `random`
    sets (smallest over the sets, largest): al_bh 387 .. 1 452 (the rows whose scaled gradient is ~1e-7 have a SUBNORMAL hi plane: without
    lo they are off by tens of per cent), ah_bl 24 .. 77 (7 at 1 024 pixels: the falling sensitivity the module docstring describes),
    last_tile 3.0e4 .. 2.4e5, rowsum_scale 4e9 and more.  Exactness breaks on 155 / 95 / 250 `exact` sets."""
    seen_exact = seen_random = 0
    lo, hi = np.inf, 0.0
    by_k = {}
    for case in SENS_CASES:
        splits, per = launch_shape(case)
        K = case["N"] * case["HW"]
        for fam in case["families"]:
            applies = {"al_bh": fam != "exact2", "ah_bl": case["b"] != "half" and fam != "exact1", "last_tile": True,
                       "rowsum_scale": case["a"] == "ps" and case["rowsum"]}[edit]
            if not applies:
                continue
            d = W.build_mfma(case, fam)
            init = np.linspace(-3.0, 5.0, case["Mpad"]) / d["sh_scale"] if case["rowsum"] else None
            got, rs = emulate(case, d, splits, per, edit=edit, rs_init=init)
            if edit == "rowsum_scale":
                r = _ratio(np.abs(rs - (init + d["rs_ref"])), W.bound_rowsum(d["rs_abs"], splits, per, init))
                assert r > 1.0, (case["name"], fam, r)
                lo, hi = min(lo, r), max(hi, r)
                seen_random += 1
                continue
            if fam == "random":
                r = _ratio(np.abs(got - d["ref"]), case_bound(case, d, splits, per))
                by_k.setdefault(K, []).append(r)
                if K <= SHORT_K or edit == "last_tile":
                    assert r > 1.0, (case["name"], edit, r)
                    lo, hi = min(lo, r), max(hi, r)
                    seen_random += 1
            else:
                assert not np.array_equal(got, d["ref"]), (case["name"], fam, edit)
                seen_exact += 1
    assert seen_random > 0 and (seen_exact > 0 or edit == "rowsum_scale")
    print(f"edit {edit}: leaves the bound by a factor {lo:.3g} .. {hi:.3g} on {seen_random} random sets; breaks exactness on {seen_exact} exact sets")
    for K in sorted(by_k):
        print(f"    random, {K} pixels: worst multiple of the bound {min(by_k[K]):.3g} .. {max(by_k[K]):.3g}")


def test_fp32_instances_yardstick():
    """k_wgrad_gemm<64 / 128> (sh_scale = 0): fp32 products and sums stay inside the 'f32' bound."""
    for npad in (64, 128):
        case = W.mfma_case(f"f32-{npad}", 3, 8, 12, 128, npad, npad, sh=False, families=("random",))
        d = W.build_mfma(case, "random")
        splits, per = launch_shape(case)
        r = _ratio(np.abs(emulate_f32(case, d, splits, per) - d["ref"]), case_bound(case, d, splits, per))
        assert r <= 1.0, r

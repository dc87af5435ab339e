"""CPU checks of tests/sh2_oracle.py, the yardstick tests/test_gpu_sh2_kernels.py holds the split-half MFMA kernels to:

  * the `exact-w` / `exact-a` input sets satisfy the four conditions under which the arithmetic csrc/sh.h promises IS the true sum,
    in every layer of every case, with exact zeros and both signs in front of each ReLU;
  * an emulation of that arithmetic (fp16 splits, three exact products, fp32 accumulation, the partial-sum layout of k_cnet's last
    phase, the fp16 tape and the sign words) returns the fp64 reference value for value on the exact sets and lies inside the
    derived bound on the `random` sets -- and uses a fair share of it, so the bound is not slack;
  * every single fault of sh2_oracle.FAULTS breaks exactness, and every one except the dropped products also leaves the `random`
    bound.  A DROPPED PRODUCT IS INSIDE THE RANDOM BOUND (2^-12 of one layer's terms against a worst-case accumulation term of
    3 K 2^-23): only the exact sets see it, which is why they exist;
  * the sign bits the `random` comparison has to leave out (reference pre-activation closer to zero than its bound) stay below 0.1 %;
  * the instance every case names is the one the library's own selection takes (glowhip_debug_sh2 without operands: a dry run), the
    refusals are refused, and the enumeration over the selection's whole input space reaches every instantiated forward / taping
    instance and no other;
  * lu_oracle.apply_bound_sh2 returns what it returned before it was moved onto the shared function."""
import ctypes

import numpy as np
import pytest

import lu_oracle
import sh2_oracle as S
from pytorch_glow_amd import _lib as L

f32, f64 = np.float32, np.float64
CASES = S.cnet_cases()
# the emulation runs every layer three times per case and family: a sample of the cases with every tiling / row split / group count
EMU_CASES = [c for i, c in enumerate(CASES) if (c["hid"] <= 256 or i % 5 == 0) and not c["bwd"]]      # (the emulation is the forward's)


def ids(cases):
    return [c["name"] for c in cases]


def geo_of(c, info):
    return S.add_geometry(c["N"], c["H"], c["W"], info.R, info.NI, info.MS, c["Cout"])


def dry(c, flags=None, tape=None, bwd=None):
    p, info = L.Sh2Probe(), L.Sh2Info()
    p.op, p.N, p.Cin, p.H, p.W, p.hidden, p.Cout, p.mode = L.SH2_CNET, c["N"], c["Cin"], c["H"], c["W"], c["hid"], c["Cout"], S.ADD_FWD
    p.bwd = int(c.get("bwd", False) if bwd is None else bwd)
    if (c.get("tape") or c.get("bwd")) if tape is None else tape:
        p.tape_h1 = p.tape_h2 = p.mask1 = p.mask2 = 16      # (selection only: a dry run looks at no operand)
        p.in_scale, p.out_scale = 16.0, 1.0 / 16.0
    with L.debug_flags(c["flags"] if flags is None else flags):
        rc = L.lib().glowhip_debug_sh2(ctypes.byref(p), ctypes.byref(info), None)
    return rc, info


def inst_of(info):
    return (info.kernel, info.hid, info.ms, info.upw, info.pxt, info.ng, info.mode)


def test_lu_bound_unchanged():
    r = np.random.RandomState(7)
    M, v = r.randn(48, 48).astype(f32), r.randn(48, 33).astype(f32)
    aM, av = np.abs(M).astype(f64), np.abs(v).astype(f64)
    old = (3 * 2.0 ** -22 + 3 * 48 * 2.0 ** -23 + 2 * 2.0 ** -24) * (aM @ av) + 2.0 ** -37 * aM.max(axis=1)[:, None] * av.sum(axis=0)[None, :] + 2.0 ** -29 * aM.sum(axis=1)[:, None]
    assert (lu_oracle.apply_bound_sh2(M, v) == old).all()


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_case_takes_its_instance(c):
    rc, info = dry(c)
    assert rc == 0, L.lib().glowhip_last_error()
    assert inst_of(info) == c["inst"], (c["name"], inst_of(info))
    g = geo_of(c, info)
    assert (info.tiles, info.lpxt, info.MS) == (g["tiles"], g["lpxt"], c["inst"][2])
    assert info.scratch_floats == S.scratch_floats_plan(c["N"], c["H"], c["W"], c["Cout"]) >= g["floats"]
    assert info.grid[0] == g["tiles"] and info.grid[1] == (1 if info.kernel == S.K_CNET1W else info.ms) and 0 < info.lds_bytes <= 160 * 1024


def test_cases_cover_every_instance_and_tiling():
    assert sorted({c["inst"] for c in CASES}) == S.EXPECTED_INSTANCES
    seen = set()
    for c in CASES:
        _, info = dry(c)
        seen.add((info.NI, min(info.R, 9), c["H"] > info.R and info.NI == 1))
    # whole images per tile (NI = 2), R = 1 (a row both first and last), R = 4 / 8 with halo rows, a single tile without
    assert {(2, 8, False), (1, 1, True), (1, 4, True), (1, 8, True)} <= seen, seen
    assert any(c["bs_extra"] for c in CASES) and any(9 * c["Cout"] % 32 for c in CASES)


HOST_REFUSALS = [c for c in S.REFUSALS if not c.get("short_scratch")]      # (a short scratch is refused once there are operands: GPU file)


@pytest.mark.parametrize("c", HOST_REFUSALS, ids=ids(HOST_REFUSALS))
def test_refusals_without_operands(c):
    cc = dict(c, flags=0, tape=bool(c.get("tape_no_masks")))
    p, info = L.Sh2Probe(), L.Sh2Info()
    p.op, p.N, p.Cin, p.H, p.W, p.hidden, p.Cout, p.mode = L.SH2_CNET, c["N"], c["Cin"], c["H"], c["W"], c["hid"], c["Cout"], S.ADD_FWD
    if cc["tape"]:
        p.tape_h1 = 16
    if c.get("tape_with_masks"):
        p.tape_h1 = p.tape_h2 = p.mask1 = p.mask2 = 16
    assert L.lib().glowhip_debug_sh2(ctypes.byref(p), ctypes.byref(info), None) == -1, c["name"]


def test_enumeration_reaches_exactly_the_instantiated_instances():
    """every (hidden, map, Cin, Cout, batch, switch) combination through the library's own selection: what can be launched at all.
    The six k_cnet<*, *, 2, 64> instances (two T units per wave on 64-pixel tiles) are not among it -- with 64-pixel tiles a unit
    holds two row tiles, so NU4 <= 8 and NU4 * KS <= 8 -- and were removed."""
    reach, refused = set(), 0
    for hid in (64, 128, 256, 512):
        for H, W in ((8, 8), (16, 16), (4, 64), (64, 4), (4, 128), (32, 32), (2, 32), (128, 128)):
            for Cin, Cout in ((6, 6), (6, 12), (12, 24), (24, 48), (48, 48), (48, 96), (28, 56), (24, 35), (3, 1), (50, 100), (56, 112), (12, 6)):
                for N in (1, 3, 64, 300):
                    for tape, bwd in ((False, False), (True, False), (True, True)):
                        for fl in (0, S.DBG_128_ONLY, S.DBG_64, S.DBG_NO_1W) + tuple(r << S.DBG_ROWS_SHIFT | t for r in (1, 2, 4) for t in (S.DBG_128_ONLY, S.DBG_64, S.DBG_NO_1W | S.DBG_128_ONLY)):
                            rc, info = dry(dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, hid=hid), fl, tape, bwd)
                            if rc:
                                refused += 1
                            else:
                                reach.add(inst_of(info))
    assert sorted(reach) == S.EXPECTED_INSTANCES, (sorted(set(S.EXPECTED_INSTANCES) - reach), sorted(reach - set(S.EXPECTED_INSTANCES)))
    assert not any(i[3] == 2 and i[4] == 64 for i in reach) and refused > 0


@pytest.mark.parametrize("c", CASES + list(S.DN_NET_CASES), ids=ids(CASES + list(S.DN_NET_CASES)))
@pytest.mark.parametrize("fam", ("exact-w", "exact-a"))
def test_exact_families_satisfy_their_conditions(c, fam):
    d = S.build(c, fam)
    S.check_exact(c, d, fam)
    for in_scale in (8.0, 32.0):              # the launches at the neighbouring in_scale values: the same window values, exactly
        assert ((S.scaled(d, in_scale)["z1"].astype(f64) * in_scale) == d["z1"].astype(f64) * 16.0).all()


def _compare_exact(c, d, e, ref):
    """the number of values of an emulation that differ from the fp64 reference (pre-activations, partial sums, tape, sign words)"""
    P = c["N"] * c["H"] * c["W"]
    n = int((e["t1"].astype(f64) != S.to_px(ref["t1"][0])).sum() + (e["t2"].astype(f64) != S.to_px(ref["t2"][0])).sum())
    n += int((e["out"] != ref["out"][0]).sum())
    if "tape1" in e:
        for k in ("1", "2"):
            n += int((S.tape_decode(e["tape" + k], c["hid"], P).astype(f64) != S.to_px(ref["h" + k][0]).astype(np.float16).astype(f64)).sum())
            n += int((S.mask_decode(e["mask" + k], c["hid"], P) != (S.to_px(ref["t" + k][0]) > 0)).sum())
    return n


def _outside_random(c, e, ref):
    P = c["N"] * c["H"] * c["W"]
    n = 0
    for k in ("t1", "t2"):
        n += int((np.abs(e[k].astype(f64) - S.to_px(ref[k][0])) > S.to_px(ref[k][1])).sum())
    n += int((~(np.abs(e["out"] - ref["out"][0]) <= ref["out"][1])).sum())
    if "tape1" in e:
        for k in ("1", "2"):
            v, b = S.to_px(ref["h" + k][0]), S.to_px(ref["h" + k][1])
            n += int((np.abs(S.tape_decode(e["tape" + k], c["hid"], P).astype(f64) - v) > S.tape_bound(v, b)).sum())
            t, tb = S.to_px(ref["t" + k][0]), S.to_px(ref["t" + k][1])
            sure = np.abs(t) > tb
            n += int((S.mask_decode(e["mask" + k], c["hid"], P) != (t > 0))[sure].sum())
    return n


@pytest.mark.parametrize("c", EMU_CASES, ids=ids(EMU_CASES))
def test_emulation_is_exact_and_every_fault_is_seen(c):
    _, info = dry(c)
    g = geo_of(c, info)
    needed = {}
    for fam in ("exact-w", "exact-a"):
        d = S.build(c, fam)
        ref = S.reference(d)
        assert _compare_exact(c, d, S.emulate(c, d, g), ref) == 0, (c["name"], fam, "the promised arithmetic is not exact here")
        for fault in S.FAULTS:
            layer, prod = (fault.split(":")[1:] + [None, None])[:2] if fault.startswith("drop") else (None, None)
            if (fault == "ms_misstrided" and g["MS"] == 1) or (fault == "halo_wrong_neighbour" and not g["halos"]) or \
                    (fault in ("sign_word_reversed", "tape_row_next_tile") and not c["tape"]):
                continue
            e = S.emulate(c, d, g, fault)
            if layer:
                # a product is needed if dropping it changes at least 1 % of that layer's outputs (hl on exact-w, lh on exact-a multiply zeros)
                key = dict(f0="t1", f2="t2", f4="out")[layer]
                want = ref[key][0] if key == "out" else S.to_px(ref[key][0])
                needed[(layer, prod)] = max(needed.get((layer, prod), 0.0), float((e[key].astype(f64) != want).mean()))
                continue
            assert _compare_exact(c, d, e, ref) > 0, (c["name"], fam, fault, "not seen by the exact family")
    for layer in ("f0", "f2", "f4"):
        for prod in ("hh", "hl", "lh"):
            assert needed[(layer, prod)] >= 0.01, (c["name"], layer, prod, needed[(layer, prod)], "the exact families do not need this product")


@pytest.mark.parametrize("c", EMU_CASES, ids=ids(EMU_CASES))
def test_emulation_is_inside_the_random_bound_and_layout_faults_are_not(c):
    _, info = dry(c)
    g = geo_of(c, info)
    d = S.build(c, "random")
    ref = S.reference(d)
    e = S.emulate(c, d, g)
    assert _outside_random(c, e, ref) == 0, (c["name"], "the promised arithmetic leaves the bound")
    assert np.isnan(e["scratch"]).sum() == int(np.isnan(S.lay_partial_sums(g, [np.zeros((9, c["Cout"], c["N"], c["H"], c["W"]), f32)] * g["MS"])).sum())
    for fault in S.FAULTS_LAYOUT:
        if (fault == "ms_misstrided" and g["MS"] == 1) or (fault == "halo_wrong_neighbour" and not g["halos"]) or \
                (fault in ("sign_word_reversed", "tape_row_next_tile") and not c["tape"]):
            continue
        assert _outside_random(c, S.emulate(c, d, g, fault), ref) > 0, (c["name"], fault, "stays inside the random bound")
    # the excluded sign bits: reference alone
    for k in ("t1", "t2"):
        assert (np.abs(ref[k][0]) <= ref[k][1]).mean() <= 1e-3, (c["name"], k, "more than 0.1 % of the sign bits are undecided")
    # not slack: the bound of the first layer is within 2^11 of the error fp16 operands WITHOUT their lo parts would make
    nolo = S.emulate(c, d, g, "drop:f0:lh")
    assert (np.abs(nolo["t1"].astype(f64) - S.to_px(ref["t1"][0])) > S.to_px(ref["t1"][1]) * 2.0 ** -11).any()


@pytest.mark.parametrize("c", S.IMAGE_CASES, ids=["%d %dx%d %s" % (c["kind"], c["Cout"], c["Cin"], c["form"]) for c in S.IMAGE_CASES])
def test_image_reference_is_consistent(c):
    """the numpy image against itself: decode(encode) within the fold bound of its own fp64 weights, padding zero, sizes as the hook reports"""
    w, fb, fl, kperm, tr = S.image_operands(c)
    img = S.image_ref(c["kind"], w, kperm, fb, fl, tr)
    p, info = L.Sh2Probe(), L.Sh2Info()
    p.op, p.kind, p.Cin, p.Cout, p.kperm, p.transposed = L.SH2_IMAGE, c["kind"], c["Cin"], c["Cout"], int(kperm), int(tr)
    assert L.lib().glowhip_debug_sh2(ctypes.byref(p), ctypes.byref(info), None) == 0, L.lib().glowhip_last_error()
    buf = S.image_bytes(img)
    assert (info.image_bytes, info.Kp, info.M) == (len(buf), img["Kp"], img["M"])
    worst, pad_zero, in_range = S.image_fold_check(c["kind"], buf, w, kperm, fb, fl, tr)
    assert worst <= 1.0 and pad_zero and in_range, (worst, pad_zero, in_range)


def test_dn_layout_and_instances_are_the_librarys():
    """dn_carve written out again against the library's (the hook without a scratch), and the three k_dn_gemm instances x three
    epilogues are all among the cases"""
    seen = set()
    for c in S.DN_NET_CASES + S.DN_MIX_CASES:
        hid, Cout = c.get("hid", 32), c.get("Cout", c["C"])
        lay = S.dn_carve(c["N"], c["C"], c["H"], c["W"], hid, Cout)
        p, info = L.Sh2Probe(), L.Sh2Info()
        p.op, p.N, p.Cin, p.H, p.W, p.hidden, p.Cout = L.SH2_DN_NET, c["N"], c["C"], c["H"], c["W"], hid, Cout
        assert L.lib().glowhip_debug_sh2(ctypes.byref(p), ctypes.byref(info), None) == 0
        assert (info.part_off, info.scratch_bytes) == (lay["part"], lay["bytes"])
        f, fi = L.FinProbe(), L.FinInfo()
        f.op, f.N, f.C, f.H, f.W, f.hidden, f.Cout = L.FIN_DN_PREP, c["N"], c["C"], c["H"], c["W"], hid, Cout
        assert L.lib().glowhip_debug_fin(ctypes.byref(f), ctypes.byref(fi), None) == 0
        assert (fi.u_off, fi.ypad_off, fi.u_plane, fi.ypad_plane) == (lay["u"], lay["ypad"], c["C"] * lay["P"], (c["C"] // 2) * lay["SLN"])
        P = lay["P"]
        if "hid" in c:
            seen |= {(S.dn_instance(hid, P)[0], "act"), (S.dn_instance(Cout, P)[0], "partial")}
        else:
            seen.add((S.dn_instance(c["C"], P)[0], "mix"))
    assert seen == {(i, e) for i in S.DN_INSTANCES for e in ("mix", "act", "partial")}
    assert len({S.dn_ksplit(c["Cout"], c["N"] * c["H"] * c["W"], S.g0(512) // 2) for c in S.DN_NET_CASES}) > 1

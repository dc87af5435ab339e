"""CPU checks of tests/fin_oracle.py, the host side of tests/test_gpu_fin_kernels.py: the bounds the finishing and channel-mixer
kernels are held to are neither loose nor fitted.

  * an fp32 emulation of the promised arithmetic (numpy float32, the kernels' operation order and index arithmetic; the reverse
    mixer's r * e - b in both the separate and the fused form) stays inside every bound on every case of the tables, and returns
    the reference value for value on the `exact` sets;
  * each of a list of single faults leaves the bound on a case that can show it (one fault, `unclamped`, changes no value -- the
    loaded slot is discarded by a select -- and is shown by the tile index it addresses instead);
  * the tiling and the scratch layout the oracle writes out again are those of the library (glowhip_debug_fin without operands
    launches nothing and reports them: no GPU needed)."""
import ctypes

import numpy as np
import pytest

from pytorch_glow_amd import _lib as L

import fin_oracle as F

f32, f64 = np.float32, np.float64


def ids(cases):
    return [c["name"] for c in cases]


def case(cases, name):
    return next(c for c in cases if c["name"] == name)


def check_cfinish(c, fam, d, got, expect_inside=True):
    """-> True when every output of the emulation `got` is inside its bound"""
    ref = F.cfinish_ref(c, d)
    ok = F.inside_nf(got["z_out"], *ref["z_out"]) and F.inside_nf(got["hout"], *ref["hout"]) and F.inside_nf(got["zback"], *ref["zback"])
    if "ld" in ref:
        tot, b, flags = ref["ld"]
        ok = ok and bool(np.all(np.abs(got["q"].astype(f64) / F.Q - tot) <= b)) and bool((got["flags"] == flags).all())
    if fam == "exact" and expect_inside:
        assert (got["z_out"].astype(f64) == ref["z_out"][0]).all() and (got["hout"].astype(f64) == ref["hout"][0]).all()
    return ok


@pytest.mark.parametrize("c", F.cfinish_cases(), ids=ids(F.cfinish_cases()))
def test_cfinish_emulation_inside_the_bound(c):
    for fam in c["families"]:
        d = F.build_cfinish(c, fam)
        touched = []
        for fused in (False, True):
            assert check_cfinish(c, fam, d, F.cfinish_emu(c, d, fused=fused, touched=touched)), (c["name"], fam, fused)
        g = F.cfin_geometry(c)
        assert not touched or (min(touched) >= 0 and max(touched) < g["tiles"]), "the emulation addressed a tile that does not exist"
        assert np.isnan(d["scratch"][d["used"]:]).all()


CF = F.cfinish_cases()
CFIN_FAULTS = [
    ("hdn_dropped", "cfin-affine-fwd-N3-16x16-t64-MS2-C4-none"),
    ("hdn_dropped", "cfin-affine-fwd-N2-4x64-t64-MS2-C4-none"),
    ("hup_hdn_swapped", "cfin-affine-fwd-N3-16x16-t64-MS2-C4-none"),
    ("hup_hdn_swapped", "cfin-add-fwd-N2-16x16-t64-MS2-C6-none"),
    ("halo_at_image_edge", "cfin-affine-fwd-N3-16x16-t64-MS1-C4-none"),
    ("halo_at_image_edge", "cfin-affine-fwd-N2-4x64-t64-MS4-C4-none"),
    ("ms_copy_dropped", "cfin-affine-fwd-N3-8x8-t128-MS4-C4-none"),
    ("ms_copy_dropped", "cfin-add-rev-N4-64x64-t64-MS2-C4-none"),
    ("paired_offset_hw", "cfin-affine-fwd-N3-16x16-t64-MS2-C4-none"),
    ("paired_offset_hw", "cfin-affine-fwd-N4-32x128-t128-MS2-C4-none"),
    ("coupling_after_staging", "cfin-add-fwd-N3-16x16-t64-MS2-C4-matrix"),
    ("coupling_after_staging", "cfin-add-fwd-N3-16x16-t64-MS2-C6-gather"),
    ("an_wrong_half", "cfin-affine-fwd-N3-16x16-t64-MS2-C4-matrix"),
    ("an_wrong_half", "cfin-add-fwd-N3-16x16-t64-MS2-C6-identity"),
    ("reverse_order", "cfin-add-rev-N3-16x16-t64-MS2-C6-matrix-rev"),
    ("reverse_order", "cfin-add-rev-N3-16x16-t64-MS1-C6-gather-rev"),
    ("logdet_sign", "cfin-affine-rev-N2-16x16-t64-MS2-C6-none"),
    ("gather_inverse", "cfin-add-fwd-N3-16x16-t64-MS2-C6-gather"),
    ("matrix_transposed", "cfin-add-fwd-N3-16x16-t64-MS2-C48-matrix"),
    ("matrix_transposed", "cfin-affine-rev-N3-16x16-t64-MS1-C4-matrix-rev-oop"),
]


@pytest.mark.parametrize("fault,name", CFIN_FAULTS, ids=["%s@%s" % f for f in CFIN_FAULTS])
def test_cfinish_single_fault_leaves_the_bound(fault, name):
    c = case(CF, name)
    for fam in c["families"]:
        d = F.build_cfinish(c, fam)
        assert check_cfinish(c, fam, d, F.cfinish_emu(c, d))
        assert not check_cfinish(c, fam, d, F.cfinish_emu(c, d, fault=fault), expect_inside=False), (fault, name, fam, "stays inside the bound")


def test_unclamped_neighbour_tile_is_seen_by_its_address():
    # the neighbour's slot is loaded unconditionally and discarded by a select where it does not apply: an unclamped index changes no
    # value, it addresses a tile before the first / behind the last
    c = case(CF, "cfin-affine-fwd-N3-16x16-t64-MS2-C4-none")
    d = F.build_cfinish(c, "random")
    good, bad = [], []
    a = F.cfinish_emu(c, d, touched=good)
    b = F.cfinish_emu(c, d, fault="unclamped", touched=bad)
    T = F.cfin_geometry(c)["tiles"]
    assert min(good) == 0 and max(good) == T - 1 and min(bad) == -1 and max(bad) == T
    assert a["z_out"].tobytes() == b["z_out"].tobytes()


@pytest.mark.parametrize("c", F.chanmix_cases(), ids=ids(F.chanmix_cases()))
def test_chanmix_emulation_inside_the_bound(c):
    for fam in c["families"]:
        d = F.build_chanmix(c, fam)
        ref, b = F.chanmix_ref(c, d)
        for fused in (False, True):
            got = F.chanmix_emu(c, d, fused=fused)
            assert F.inside(got, ref, b), (c["name"], fam, fused, F.worst(got, ref, b))
            if fam == "exact":
                assert (got.astype(f64) == ref).all(), (c["name"], "the exact set is not exact")
        want = F.mixer_bitwise(d["mix"], F.chanmix_input(c, d)[2])
        if want is not None:
            assert want.tobytes() == F.chanmix_emu(c, d).tobytes()


CM = F.chanmix_cases()
CHANMIX_FAULTS = [
    ("ca_off_by_one", "mix-matrix-C12-N3x45-Ca6"),
    ("ca_off_by_one", "mix-matrix-C130-N3x45-Ca65"),
    ("matrix_transposed", "mix-matrix-C50-N3x45-Ca25"),
    ("matrix_transposed", "mix-matrix-C384-N3x45-Ca192"),
    ("gather_inverse", "mix-gather-C12-N3x60-Ca12"),
    ("gather_inverse", "mix-gather-rev-C112-N3x45-Ca0"),
    ("reverse_order", "mix-matrix-rev-C12-N3x45-Ca6"),
    ("an_wrong_half", "mix-matrix-C16-N3x45-Ca8"),
    ("squeeze_bit_order", "mix-gather-C12-N3x15-Ca12-sq-f32-none-bs0-Wo5"),
    ("squeeze_bit_order", "mix-matrix-C12-N3x15-Ca12-sq-u8-tensor-bs1-Wo5"),
    ("noise_strided_index", "mix-matrix-C12-N3x15-Ca12-sq-f32-tensor-bs1-Wo5"),
    ("noise_strided_index", "mix-matrix-C12-N3x15-Ca12-sq-u8-philox-bs1-Wo5"),
]


@pytest.mark.parametrize("fault,name", CHANMIX_FAULTS, ids=["%s@%s" % f for f in CHANMIX_FAULTS])
def test_chanmix_single_fault_leaves_the_bound(fault, name):
    c = case(CM, name)
    for fam in c["families"]:
        d = F.build_chanmix(c, fam)
        ref, b = F.chanmix_ref(c, d)
        assert F.inside(F.chanmix_emu(c, d), ref, b)
        assert not F.inside(F.chanmix_emu(c, d, fault=fault), ref, b), (fault, name, fam, "stays inside the bound")


def check_dnfin(c, d, got):
    ref = F.dnfin_ref(c, d)
    ok = F.inside(got["state"], *ref["state"])
    if "ld" in ref:
        ok = ok and bool(np.all(np.abs(got["q"].astype(f64) / F.Q - ref["ld"][0]) <= ref["ld"][1]))
    return ok, ref


@pytest.mark.parametrize("c", F.dnfin_cases(), ids=ids(F.dnfin_cases()))
def test_dnfin_emulation_inside_the_bound(c):
    for fam in c["families"]:
        d = F.build_dnfin(c, fam)
        got = F.dnfin_emu(c, d)
        ok, ref = check_dnfin(c, d, got)
        assert ok, (c["name"], fam)
        if fam == "exact":
            assert (got["state"].astype(f64) == ref["state"][0]).all()
        if c["ks"] > 1:
            assert not check_dnfin(c, d, F.dnfin_emu(c, d, fault="ks_partial_dropped"))[0], (c["name"], fam, "a dropped partial stays inside the bound")
        if c["mode"] == F.AFFINE_REV:
            assert not check_dnfin(c, d, F.dnfin_emu(c, d, fault="logdet_sign"))[0], (c["name"], "a log-det of the wrong sign stays inside the bound")


def test_sh2_split_reconstructs_the_value():
    # sh.h: |V - hi - lo| <= max(2^-22 |V|, 2^-25) for the operand V = 16 v, and the layout puts channel c of slot s at ((c / 8) S + s) 8 + c % 8
    c = F.dnprep_cases()[0]
    d = F.build_dnprep(c)
    hi, lo = F.sh2_split(d["src"], d["mix"]["bias"], d["mix"]["scale"])
    V = ((d["src"] + d["mix"]["bias"][None, :, None]) * d["mix"]["scale"][None, :, None]).astype(f64) * 16.0
    assert (np.abs(V - hi.astype(f64) - lo.astype(f64)) <= np.maximum(2.0 ** -22 * np.abs(V), 2.0 ** -25)).all()
    P = c["N"] * c["HW"]
    plane = F.sh2_plane(hi, P, np.arange(P)).reshape(c["C"] // 8, P, 8)
    assert plane[1, c["HW"] + 2, 3] == hi.view(np.uint16)[1, 11, 2]
    slots = F.pad_slots(c["N"], c["H"], c["W"])
    assert len(set(slots.tolist())) == P and slots.max() < c["N"] * (c["H"] + 2) * (c["W"] + 2) - (c["W"] + 2)


def test_tables_reach_every_instance_and_route():
    seen = {(c["pxb"], c["MS"], c["halo"]) for c in CF}
    want = {(p, m, h) for p in (16, 64) for m in (1, 2, 4) for h in (0, 1)} | {(256, m, 1) for m in (1, 2)}
    assert seen == want
    assert {(c["pxb"], c["affine_order"]) for c in CF} >= {(16, 0), (16, 1), (64, 0), (64, 1), (256, 0)} and not any(c["affine_order"] for c in CF if c["pxb"] == 256)
    assert {(c["kernel"], c["grid"][1] == 1) for c in CM} == {("16", True), ("64", True), ("wide", True), ("wide", False)}
    assert {c["C"] for c in CM if c["kernel"] == "16"} >= {16, 50, 110} and {c["C"] for c in CM if c["kernel"] == "64"} >= {1, 3, 12, 15, 16, 50, 110}
    assert {c["ks"] for c in F.dnfin_cases()} == {1, 2, 4, 8}


def hook(p):
    info = L.FinInfo()
    rc = L.lib().glowhip_debug_fin(ctypes.byref(p), ctypes.byref(info), None)
    return rc, info


def test_library_tiling_and_scratch_layout_are_the_oracles():
    # without operands the hook launches nothing and reports what it derived (host code only)
    for c in CF:
        p = L.FinProbe()
        p.op, p.N, p.C, p.H, p.W, p.Cout, p.hidden, p.mode, p.MS, p.tile = L.FIN_CFINISH, c["N"], c["C"], c["H"], c["W"], c["Cout"], 128, c["mode"], c["MS"], c["tile"]
        rc, info = hook(p)
        g = F.cfin_geometry(c)
        assert rc == 0, (c["name"], L.lib().glowhip_last_error())
        assert (info.R, info.NI, info.tiles, info.lpxt, info.scratch_floats) == (g["R"], g["NI"], g["tiles"], g["lpxt"], F.plan_scratch_floats(c)), c["name"]
    for c in F.dnfin_cases() + F.dnprep_cases():
        p = L.FinProbe()
        p.op, p.N, p.C, p.H, p.W, p.Cout, p.hidden = L.FIN_DN_FIN, c["N"], c["C"], c["H"], c["W"], c["Cout"], F.DN_HIDDEN
        rc, info = hook(p)
        lay = F.dn_layout(c)
        assert rc == 0, (c["name"], L.lib().glowhip_last_error())
        assert (info.part_off, info.u_off, info.ypad_off, info.u_plane, info.ypad_plane, info.scratch_bytes) == \
            (lay["part_off"], lay["u_off"], lay["ypad_off"], lay["u_plane"], lay["ypad_plane"], lay["bytes"]), c["name"]


def test_hook_refuses_bad_geometry_on_the_host():
    def probe(**kw):
        p = L.FinProbe()
        p.op, p.N, p.C, p.H, p.W, p.Cout, p.hidden, p.mode, p.MS, p.tile = L.FIN_CFINISH, 2, 4, 16, 16, 4, 128, F.AFFINE_FWD, 1, 64
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    assert hook(probe())[0] == 0
    for kw in (dict(tile=32), dict(MS=3), dict(mode=0), dict(mode=5), dict(Cout=2), dict(C=5), dict(H=12), dict(W=2), dict(N=0), dict(hidden=100),
               dict(H=128, W=128, tile=64),      # W beyond the tile: k_cnet has no such geometry
               dict(op=7)):
        rc, _ = hook(probe(**kw))
        assert rc == -1 and L.lib().glowhip_last_error(), kw
    p = L.FinProbe()
    p.op, p.N, p.C, p.H, p.W, p.Cout, p.hidden = L.FIN_DN_PREP, 3, 48, 4, 4, 32, 32      # C no multiple of 32
    assert hook(p)[0] == -1
    p = L.FinProbe()
    p.op, p.N, p.C, p.HW, p.Ca = L.FIN_CHANMIX, 3, 12, 16, 13
    assert hook(p)[0] == -1

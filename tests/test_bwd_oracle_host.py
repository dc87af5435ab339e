"""CPU checks of tests/bwd_oracle.py, the reference and bounds tests/test_gpu_bwd_kernels.py holds the gradient kernels of
csrc/backward.hip to.  For every case of the GPU test a numpy fp32 emulation of the promised arithmetic -- one rounding per
operation, fused multiply-add chains where the kernels have them, the same grouping into lane segments, pixel blocks and accumulator
copies, in one fixed order -- must stay inside the bound and, on the `exact` input sets, return the fp64 reference value for value.
Each of eleven single faults must leave the bound on every case it applies to: a bound that survives one is too loose.  This is the
only statement about how tight the bounds are."""
import numpy as np
import pytest

import bwd_oracle as B

f32, f64 = np.float32, np.float64


def fma(a, b, c):
    """fl32(a b + c): the product of two fp32 numbers is exact in fp64"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def expf(x):
    return np.exp(x.astype(f64)).astype(f32)


def segsum(t, L, mut=None):
    """(N, C, HW) fp32 -> (C,) fp64: fp32 sums inside segments of L consecutive pixels, fp64 across segments and images"""
    N, C, HW = t.shape
    L = min(L, HW)
    seg = t.reshape(N, C, HW // L, L).copy()
    if mut == "drop_last_pixel":
        seg[..., L - 1] = 0
    return seg.sum(axis=-1, dtype=f32).astype(f64).sum(axis=(0, 2)) if L > 1 else seg.astype(f64).sum(axis=(0, 2, 3))


def interleave(a, b):
    out = np.empty((a.shape[0], 2 * a.shape[1], a.shape[2]), a.dtype)
    out[:, 0::2], out[:, 1::2] = a, b
    return out


def emu_coupling(case, d, mut=None):
    h, z, g, e, gld = (d[k] for k in ("hout", "z2", "g2", "e4", "gld"))
    if case["affine"]:
        s = f32(1) / (f32(1) + expf(-(h[:, 1::2] + f32(2))))
        gy = g * s
        gh = interleave(gy, ((g * (z / s) + gld[:, None, None] / s) * s) * (f32(1) - s))
    else:
        gy = gh = g
    gpre = gh * e[None, :, None]
    return dict(gy2=gy, gpre=gpre, acc_b=segsum(gpre, case["L"], mut), acc_l=(1.0 if mut == "no3" else 3.0) * segsum(gh * h, case["L"], mut))


def emu_split(case, d, mut=None):
    h, z, e, G = d["hout"], d["z2"], d["e4"], d["gld"][:, None, None]
    dd, q = z - h[:, 0::2], expf(f32(-2) * h[:, 1::2])
    gh = interleave((G * dd) * q, G * ((dd * dd) * q - f32(1)))
    gpre = gh * e[None, :, None]
    return dict(gz2=(-G * dd) * q, gpre=gpre, acc_b=segsum(gpre, 1), acc_l=(1.0 if mut == "no3" else 3.0) * segsum(gh * h, 1))


def emu_act(case, d, mut=None):
    h, g, e = d["h"], d["g"], d["e"]
    gu = np.where(h >= 0 if mut == "ge" else h > 0, g * e[None, :, None], f32(0))
    return dict(gu=gu, acc_b=segsum(gu, case["L"], mut), acc_l=(1.0 if mut == "no3" else 3.0) * segsum(g * h, case["L"], mut))


def emu_gather(geo, scratch, mut=None):
    hpart, hup, hdn = B.split_scratch(geo, scratch)
    N, C, H, W, R, MS, T = (geo[k] for k in ("N", "Cout", "H", "W", "R", "MS", "tiles"))
    se = np.zeros((N, C, H, W), f32)
    for m in range(MS - 1 if mut == "drop_ms" else MS):
        se += hpart[m].reshape(N, C, H, W)
    for n in range(N):      # (every load from a clamped slot, the value selected)
        for y in range(H):
            r, t = y % R, B.tile_of(geo, n, y)
            wd = geo["halos"] and r == 0 and (y > 0 or mut == "edge")
            wu = geo["halos"] and r == R - 1 and (y < H - 1 or mut == "edge")
            td, tu = max(t - 1, 0), min(t + 1, T - 1)
            for m in range(MS):
                d0, u0 = (hup if mut == "updn" else hdn)[m, td], hup[m, tu]
                se[n, :, y] += (d0 if wd else np.zeros_like(d0)) + (u0 if wu else np.zeros_like(u0))
    return se.reshape(N, C, H * W)


def block_chain(a, b, PX):
    """a (A, P), b (Bn, P) fp32 -> (A, Bn) fp64: per block of PX pixels a chain of fused multiply-adds, the blocks' sums added in fp64"""
    P = a.shape[1]
    nb = -(-P // PX)
    ap, bp = (np.zeros((t.shape[0], nb * PX), f32) for t in (a, b))
    ap[:, :P], bp[:, :P] = a, b
    ap, bp = ap.reshape(-1, nb, PX), bp.reshape(-1, nb, PX)
    s = np.zeros((ap.shape[0], bp.shape[0], nb), f32)
    for q in range(PX):
        s = fma(ap[:, None, :, q], bp[None, :, :, q], s)
    return s.astype(f64).sum(axis=2)


def row_chain(a, b, PX):
    """a, b (C, P) fp32 -> (C,) fp64: the same chains row by row"""
    C, P = a.shape
    nb = -(-P // PX)
    ap, bp = np.zeros((C, nb * PX), f32), np.zeros((C, nb * PX), f32)
    ap[:, :P], bp[:, :P] = a, b
    ap, bp = ap.reshape(C, nb, PX), bp.reshape(C, nb, PX)
    s = np.zeros((C, nb), f32)
    for q in range(PX):
        s = fma(ap[:, :, q], bp[:, :, q], s)
    return s.astype(f64).sum(axis=1)


def emu_mixer(case, d, mut=None):
    N, C, HW, PX = case["N"], case["C"], case["HW"], case["PX"]
    x, gy, b, e = d["x"], d["gy"], d["bias"], d["scale"]
    v = (x + b[None, :, None]) * e[None, :, None]
    g = gy.copy()
    if case["add"]:
        aC, sc = case["add"]["C"], d["add_scale"]
        se = emu_gather(B.case_geometry(case), d["scratch"], mut)
        g[:, :aC] = gy[:, :aC] + se * sc
        if mut == "scale_all":
            g[:, aC:] = gy[:, aC:] + se[:, aC - 1:aC] * sc
    if case["mode"] == "matrix":
        Wm = d["matrix"].T if mut == "WT" else d["matrix"]
        gv = np.zeros((N, C, HW), f32)
        for o in range(C):
            gv = fma(Wm[o][None, :, None], g[:, o][:, None, :], gv)
    else:
        gv = g[:, d["inv"]] if case["mode"] == "gather" else g
    gx = gv * e[None, :, None]
    flat = lambda t: np.ascontiguousarray(t.transpose(1, 0, 2)).reshape(C, N * HW)      # noqa: E731  (image-major pixel axis)
    gf, vf, gvf = flat(g), flat(v), flat(gv)
    out = dict(gx=gx, acc_b=row_chain(gvf, np.broadcast_to(e[:, None], gvf.shape), PX),
               acc_l=(1.0 if mut == "no3" else 3.0) * row_chain(gvf, vf, PX))
    if case["mode"] == "matrix":
        out["acc_w"] = block_chain(gf, vf, PX)
    if mut == "drop_slice":
        c0 = (C - 1) // 32 * 32
        out["gx"][:, c0:] = 0
        out["acc_b"][c0:], out["acc_l"][c0:] = 0, 0
        if "acc_w" in out:
            out["acc_w"][:, c0:] = 0
    return out


def emu_reduce(job, partial):
    s = np.zeros(partial.shape[1:], f32)
    for k in range(job["splits"]):
        s = s + partial[k]
    s = s[:job["Mreal"], :job["Nreal"]]
    if job["mode"] == 1:
        s = s.reshape(job["Mreal"] // 9, 9, job["Nreal"]).transpose(0, 2, 1)
    return s.reshape(-1)


def emu_prior(case, d):
    z, gld = d["z"], d["gld"][:, None]
    m, l = (d[k] if case["ml"] != "null" else f32(0) for k in ("mean", "logs"))
    g = ((-gld) * (z - m)) * expf(f32(-2) * np.broadcast_to(l, z.shape))
    return dict(gz=g + d["gz_in"] if case["gz_in"] else g)


def emu_finalize(d, gld, mut=None):
    G = gld.astype(f64).sum()
    res = []
    for j, acc, winv in zip(d["jobs"], d["acc"], d["winv"]):
        v = np.zeros(j["n"])
        for k in range(j["copies"] - 1 if mut == "skip_copy" and j["copies"] > 1 else j["copies"]):
            v = v + acc[k * j["stride"]:k * j["stride"] + j["n"]]
        if j["winv"]:
            v = v + G * j["add_mul"] * (winv if mut == "winv_T" else winv.T).astype(f64).reshape(-1)
        else:
            v = v + G * j["add_mul"]
        res.append(v.astype(f32) if j["out"] else None)
    return res


def all_inside(got, ref):
    return all(B.inside(got[k], *ref[k]) for k in ref)


def check(got, ref, fam, name):
    for k, (r, b) in ref.items():
        assert B.inside(got[k], r, b), (name, fam, k, "emulation outside the bound; worst multiple", B.worst(got[k], r, b))
        if fam == "exact":
            assert np.array_equal(np.asarray(got[k], f64), r), (name, k, "emulation differs from the reference on an exact set")


OPS = dict(coupling=(B.coupling_cases, B.build_coupling, B.coupling_ref, emu_coupling), split=(B.split_cases, B.build_split, B.split_ref, emu_split),
           act=(B.act_cases, B.build_act, B.act_ref, emu_act))
POINTWISE = [(op, c) for op in OPS for c in OPS[op][0]()]
MIXER = B.mixer_cases() + B.mixer_reduce_cases() + B.mixer_add_cases() + B.mixer_wide_cases()


@pytest.mark.parametrize("op,case", POINTWISE, ids=[c["name"] for _, c in POINTWISE])
def test_pointwise_emulation_inside_bound(op, case):
    _, build, ref, emu = OPS[op]
    for fam in case["families"]:
        d = build(case, fam)
        check(emu(case, d), ref(case, d), fam, case["name"])


@pytest.mark.parametrize("case", MIXER, ids=[c["name"] for c in MIXER])
def test_mixer_emulation_inside_bound(case):
    for fam in case["families"]:
        d = B.build_mixer(case, fam)
        check(emu_mixer(case, d), B.mixer_ref(case, d), fam, case["name"])
        for job, part in zip(case["jobs"], d["partials"]):
            r, b = B.reduce_ref(job, part)
            check(dict(dw=emu_reduce(job, part)), dict(dw=(r, b)), fam, case["name"])


def test_gather_reference_uses_no_unused_slot():
    """the NaN-filled slots reach neither the reference nor its magnitudes; every slot the layout assigns is used exactly once"""
    for case in B.mixer_add_cases():
        geo = B.case_geometry(case)
        sc = B.build_scratch(geo, B.rng_of("slots", case["name"]), "random")
        s, m = B.gather_ref(geo, sc)
        assert np.isfinite(s).all() and np.isfinite(m).all()
        assert geo["floats"] == sc.size
        ones = np.where(np.isnan(sc), np.nan, 1.0).astype(f32)
        assert B.gather_ref(geo, ones)[0].sum() == np.isfinite(sc).sum(), case["name"]
        up, dn = B.unused_halo_mask(geo)
        assert geo["halos"] or (up.all() and dn.all())


@pytest.mark.parametrize("case", B.prior_cases(), ids=[c["name"] for c in B.prior_cases()])
def test_prior_emulation_inside_bound(case):
    d = B.build_prior(case, "random")
    check(emu_prior(case, d), B.prior_ref(case, d), "random", case["name"])


def test_flip_and_logs_references():
    for Cout, Cin, k in B.FLIP_CASES:
        w = np.arange(Cout * Cin * k * k, dtype=f32).reshape(Cout, Cin, k, k)
        wT = B.flip_ref(w)
        for o, i, t in ((0, 0, 0), (Cout - 1, Cin - 1, k * k - 1), (Cout // 2, Cin // 2, (k * k) // 2)):
            assert wT[i, o, t] == w[o, i].reshape(-1)[k * k - 1 - t]
    for rows, K in B.LOGS_JOBS:
        d = B.build_logs(rows, K)
        ref, b = B.logs_ref(d)
        assert B.inside(ref.astype(f32), ref, b) and not B.inside((ref / 3.0).astype(f32), ref, b)


@pytest.mark.parametrize("N", B.FINALIZE_N)
def test_finalize_emulation_inside_bound(N):
    for fam in ("exact", "random"):
        d = B.build_finalize(N, fam)
        gr, gb = B.gld_ref(d)
        gld = (-d["nll"].astype(f64) * d["inv"]).astype(f32)
        check(dict(gld=gld), dict(gld=(gr, gb)), fam, "gld")
        for got, rb, j in zip(emu_finalize(d, gld), B.finalize_ref(d, gld), d["jobs"]):
            assert (got is None) == (rb is None) == (not j["out"])
            if rb:
                check(dict(out=got), dict(out=rb), fam, "finalize")


# ---------------------------------------------------------------------------------------------------------------------
# the faults the bounds must notice
# ---------------------------------------------------------------------------------------------------------------------
def _mixer_small(cases):
    return [c for c in cases if c["C"] <= 256]


MUTATIONS = {
    "drop_last_pixel": [("coupling", c) for c in B.coupling_cases() if c["vec4"]] + [("act", c) for c in B.act_cases() if c["vec4"]],
    "no3": [(op, c) for op, c in POINTWISE] + [("mixer", c) for c in _mixer_small(B.mixer_cases() + B.mixer_wide_cases())],
    "ge": [("act", c) for c in B.act_cases()],
    "WT": [("mixer", c) for c in _mixer_small(MIXER) if c["mode"] == "matrix"],
    "drop_slice": [("mixer", c) for c in _mixer_small(B.mixer_wide_cases())],
    "updn": [("mixer", c) for c in B.mixer_add_cases() if B.case_geometry(c)["halos"]],
    "edge": [("mixer", c) for c in B.mixer_add_cases() if B.case_geometry(c)["halos"]],
    "drop_ms": [("mixer", c) for c in B.mixer_add_cases()],
    "scale_all": [("mixer", c) for c in B.mixer_add_cases()],
}


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_single_fault_leaves_the_bound(mut):
    """drop the last pixel of a lane segment; the factor 3 of a log-scale gradient dropped; the mask side h >= 0; W for W^T; the last
    channel slice of a wide level left out; hup read for hdn; a halo added at an image's edge; one MS copy dropped; add_scale on
    channels >= add_C"""
    assert MUTATIONS[mut]
    for op, case in MUTATIONS[mut]:
        build, ref, emu = (B.build_mixer, B.mixer_ref, emu_mixer) if op == "mixer" else OPS[op][1:]
        for fam in case["families"]:
            d = build(case, fam)
            assert not all_inside(emu(case, d, mut), ref(case, d)), (mut, case["name"], fam, "the fault stays inside the bound")


@pytest.mark.parametrize("mut", ["skip_copy", "winv_T"])
def test_single_fault_leaves_the_finalize_bound(mut):
    """one accumulator copy skipped; winv[o C + i] used for winv[i C + o]"""
    for N in B.FINALIZE_N:
        for fam in ("exact", "random"):
            d = B.build_finalize(N, fam)
            gld = (-d["nll"].astype(f64) * d["inv"]).astype(f32)
            hit = [not B.inside(got, *rb) for got, rb, j in zip(emu_finalize(d, gld, mut), B.finalize_ref(d, gld), d["jobs"])
                   if rb and (j["winv"] if mut == "winv_T" else j["copies"] > 1)]
            assert hit and all(hit), (mut, N, fam, hit)

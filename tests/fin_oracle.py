"""Host side of the per-kernel tests of the fp32 code every forward, decode and training step runs between the MFMA launches, numpy
only: the fp64 reference of each operation, the per-element bound each kernel is held to, the two input families, an fp32 emulation
of the promised arithmetic with a switch for single faults, and the tables of cases tests/test_gpu_fin_kernels.py launches through
glowhip_debug_fin and tests/test_fin_oracle_host.py checks on the CPU.

  k_cfinish<PXB, MSV, HALO>   csrc/cnet_sh.hip, body cfinish_chunk in csrc/cnet_fin.h
  launch_chanmix              csrc/pointwise.hip: k_chanmix<16>, k_chanmix<64>, k_chanmix_wide sliced and in place
  k_dn_fin / k_dn_prep        csrc/dnet_sh.hip

THE FORMULAS (the kernels' header comments; network/model.py:105-139).  With h = (sum of partials + bias) * exp(3 logs) per f.4
output channel, z1 = channels [0, Ch) and z2 = [Ch, 2 Ch) of the state:
  additive   z2' = z2 + h[c]  (forward)     z2 - h[c]  (reverse)                                          Cout = Ch
  affine     shift = h[2c], s = sigmoid(h[2c + 1] + 2):  z2' = (z2 + shift) s,  log-det += log s  (forward)
                                                         z2' = z2 / s - shift,  log-det -= log s  (reverse)  Cout = 2 Ch
  mixer      forward: the NEXT step's  y = M ((z + b) * e)  (matrix), y[o] = v[gather[o]] (gather) or y = v;
             reverse: THIS step's  x = (M z) * e - b
The partial sums of k_cnet lie as bwd_oracle documents (hpart | hup | hdn; gather_ref and unused_halo_mask are used from there, not
copied); those of the deep levels as part[ks][N][Cout][HW].  The log-det of an element goes, rounded to 2^-32 nats, into one of
1 + ACC_EXTRA unsigned 64-bit accumulator rows of its sample (row 0 at acc[n], the flag word at acc[N + n], row r >= 1 at
acc[(1 + r) N + n]); a non-finite term raises a flag bit (1 NaN, 2 +inf, 4 -inf) instead and leaves the accumulators alone.
k_dn_fin / k_dn_prep also write the SH2 operand of the next launch: v = 16 * ActNorm(state), hi = fp16(v), lo = fp16(v - hi), at
half index ((c / 8) slots + slot) * 8 + c % 8 of the hi plane and the same index of the lo plane.

THE BOUNDS.  u = 2^-24; every fp32 operation is one rounding to nearest, |error| <= u |result|; expf is taken as 2 u, as
tests/objective_oracle.py and bwd_oracle allow, and logf as 2 u -- AN ASSUMPTION: the device library documents 1 ulp for logf, and
2 u = 1 ulp at the top of a binade.  Nothing is fitted to a kernel's output; tests/test_fin_oracle_host.py shows that the fp32
emulation below stays inside on every case and that every listed single fault leaves.  bnd() (bwd_oracle) adds 2^-10 relative for
second-order terms.
  * gather: the MS copies are added one after the other, then per copy one sum of the two selected halo values and one addition:
    at most 3 MS additions, |err| <= 3 MS u sum|parts|.  The deep levels add ks copies in order: ks u sum|parts|.
  * h = fl(fl(S + b) e):  |e| err S + 2 u |h|.
  * additive: one more addition, err h + u |z2'|.
  * sigmoidf_(x) = 1 / (1 + expf(-x)), x = fl(r + 2): bwd_oracle's count es = 2 + (1 - s)(2 + |x|) roundings relative to s, plus
    what r brings along, (1 - s) err r (d s / d x = s (1 - s)):   ds = u es + (1 - s) err r   relative.
  * affine forward  fl(fl(z2 + shift) s):  s (err shift + u |z2 + shift|) + |z2'| (ds + u)
    affine reverse  fl(fl(z2 / s) - shift):  |z2 / s| (ds + u) + err shift + u |z2'|
    log-det term    logf(s): ds (d log s = ds / s) + 2 u |log s|, then the conversion to 2^-32 nats: + 2^-33.  The per-sample total
    is an exact integer sum over all rows: its bound is the sum of the elements' bounds.
  * ActNorm of the next step  v = fl(fl(z + b) e):  |e| err z + 2 u |v|.
  * matrix: a chain of C fused multiply-adds, i ascending:  C u sum_i |m||v| + sum_i |m| err v.  Gather / pass-through: err v.
  * reverse mixer  r * e - b: hipcc may or may not contract it.  Separate roundings give |e| err r + u |r e| + u |x|, the fused form
    |e| err r + u |x|: the first admits both and is the bound.
Bitwise on top, from the kernel's own fp32 values: a forward gather / pass-through mixer returns fl(fl(x + b) e) of the selected
channel; the SH2 operand is the split of 16 fl(fl(z + b) e) computed from the state the kernel stored.

FAMILIES (those of bwd_oracle).  `exact`: small integers, power-of-two scales and matrix entries, additive coupling: every sum in
every order is an fp32 number and the kernel must return the reference value for value.  `random`: realistic magnitudes, sigmoid
arguments in [-6, 6]: every element within the bound, no outliers."""
import numpy as np

import bwd_oracle as B
from bwd_oracle import U, bnd, f32, f64, ints, pow2, rng_of, inside, worst  # noqa: F401

AFFINE_FWD, AFFINE_REV, ADD_FWD, ADD_REV = 1, 2, 3, 4      # TailMode of csrc/conv_mfma.h
MODE_NAME = {AFFINE_FWD: "affine-fwd", AFFINE_REV: "affine-rev", ADD_FWD: "add-fwd", ADD_REV: "add-rev"}
ACC_EXTRA = 7
Q = 2.0 ** 32
HALF_Q = 2.0 ** -33
SH2 = 16.0


def paired(mode):
    return mode in (AFFINE_FWD, AFFINE_REV)


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


# ---------------------------------------------------------------------------------------------------------------------
# the coupling on gathered sums (shared by k_cfinish and k_dn_fin): fp64 reference and bound
# ---------------------------------------------------------------------------------------------------------------------
def hout_ref(S, mag, nadds, bias, scale):
    """h = (S + b) e of every f.4 output channel -> (h, bound before bnd())"""
    b, e = bias.astype(f64)[None, :, None], scale.astype(f64)[None, :, None]
    h = (S + b) * e
    return h, np.abs(e) * (nadds * U * mag) + 2.0 * U * np.abs(h)


def coupling_ref(mode, h, e_h, z2):
    """-> dict(z2 (ref, raw bound), term, e_term (per element, affine only), finite: the element's log-det term is finite)"""
    z2 = z2.astype(f64)
    with np.errstate(all="ignore"):
        if not paired(mode):
            r = z2 + h if mode == ADD_FWD else z2 - h
            return dict(z2=(r, e_h + U * np.abs(r)), term=None)
        sh, e_sh, rr, e_rr = h[:, 0::2], e_h[:, 0::2], h[:, 1::2], e_h[:, 1::2]
        x = rr + 2.0
        s = sigmoid(x)
        ds = U * (2.0 + (1.0 - s) * (2.0 + np.abs(x))) + (1.0 - s) * e_rr
        lg = np.log(s)
        if mode == AFFINE_FWD:
            t = z2 + sh
            r = t * s
            e = s * (e_sh + U * np.abs(t)) + np.abs(r) * (ds + U)
            term = lg
        else:
            q = z2 / s
            r = q - sh
            e = np.abs(q) * (ds + U) + e_sh + U * np.abs(r)
            term = -lg
        fin = np.isfinite(term)
        e_term = ds + 2.0 * U * np.abs(lg) + HALF_Q
        # an element whose sigmoid argument is not finite: z2' is what IEEE arithmetic gives (0, an infinity or NaN), to be met exactly
        e = np.where(np.isfinite(x), e, 0.0)
    return dict(z2=(r, e), term=np.where(fin, term, 0.0), e_term=np.where(fin, e_term, 0.0), finite=fin, arg=x)


def logdet_ref(c):
    """per-sample (total of the finite terms in nats, its bound, the flag bits of log s: 1 NaN, 2 +inf, 4 -inf -- the reverse modes
    store -log s: flip_inf_flags)"""
    tot, b = c["term"].sum(axis=(1, 2)), bnd(c["e_term"].sum(axis=(1, 2)))
    with np.errstate(all="ignore"):
        lg = np.where(c["finite"], 0.0, np.log(sigmoid(c["arg"])))
    flags = (np.isnan(lg).any(axis=(1, 2)) * 1) | ((lg == np.inf).any(axis=(1, 2)) * 2) | ((lg == -np.inf).any(axis=(1, 2)) * 4)
    return tot, b, flags.astype(np.int64)


def inside_nf(got, ref, bound):
    """inside(), for references that hold infinities or NaN: those elements must be met exactly"""
    got = np.asarray(got, f64).reshape(ref.shape)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        ok = np.where(fin, np.abs(got - ref) <= bound, (np.isnan(ref) & np.isnan(got)) | (got == ref))
    return bool(ok.all())


def flip_inf_flags(flags):
    return (flags & 1) | ((flags & 2) << 1) | ((flags & 4) >> 1)


def acc_total(acc, N):
    """the (2 + ACC_EXTRA) N accumulator words -> (per-sample sum of all rows in nats, exact; flag words)"""
    a = np.asarray(acc, np.uint64).reshape(2 + ACC_EXTRA, N)
    rows = np.concatenate([a[:1], a[2:]]).astype(np.int64)      # two's complement
    return rows.sum(axis=0, dtype=np.int64).astype(f64) / Q, a[1].astype(np.int64)


def mixer_ref(mix, state, e_state):
    """mix: dict(kind 'none' | 'matrix' | 'gather' | 'identity', reverse, bias, scale (None: no ActNorm), matrix, gather);
    state, e_state (N, C, P) fp64 -> (out, raw bound)"""
    if mix["kind"] == "none":
        return state, e_state
    C = state.shape[1]
    an = mix["bias"] is not None
    b = mix["bias"].astype(f64)[None, :, None] if an else 0.0
    e = mix["scale"].astype(f64)[None, :, None] if an else 1.0
    with np.errstate(all="ignore"):
        if not mix["reverse"] and an:
            v = (state + b) * e
            e_v = np.abs(e) * e_state + 2.0 * U * np.abs(v)
        else:
            v, e_v = state, e_state
        if mix["kind"] == "matrix":
            M = mix["matrix"].astype(f64)
            r = np.einsum("oi,nip->nop", M, v)
            e_r = C * U * np.einsum("oi,nip->nop", np.abs(M), np.abs(v)) + np.einsum("oi,nip->nop", np.abs(M), e_v)
        else:
            g = mix["gather"] if mix["kind"] == "gather" else np.arange(C)
            r, e_r = v[:, g], e_v[:, g]
        if mix["reverse"] and an:
            out = r * e - b
            return out, np.abs(e) * e_r + U * np.abs(r * e) + U * np.abs(out)
    return r, e_r


def mixer_bitwise(mix, x32):
    """forward gather / pass-through: the fp32 value the kernel must store, from fp32 inputs (None where no such promise holds)"""
    if mix["kind"] not in ("gather", "identity") or mix["reverse"]:
        return None
    v = x32 if mix["bias"] is None else (x32 + mix["bias"][None, :, None]) * mix["scale"][None, :, None]
    return v[:, mix["gather"]] if mix["kind"] == "gather" else v


def fma_chain(M, v):
    """fp32 emulation of r = fma(m[o][i], v[i], r), i ascending (product exact in fp64, one rounding per step)"""
    N, C, P = v.shape
    r = np.zeros((N, M.shape[0], P), f32)
    M64, v64 = M.astype(f64), v.astype(f64)
    for i in range(C):
        r = (M64[None, :, i, None] * v64[:, None, i, :] + r.astype(f64)).astype(f32)
    return r


def mixer_emu(mix, state, fault=None, fused=False):
    """fp32 emulation of the mixer phase (k_cfinish's, k_chanmix's); fused: the reverse r * e - b as one fused multiply-add"""
    if mix["kind"] == "none":
        return state
    C = state.shape[1]
    an = mix["bias"] is not None
    b = mix["bias"][None, :, None] if an else f32(0.0)
    e = mix["scale"][None, :, None] if an else f32(1.0)
    v = state
    with np.errstate(all="ignore"):
        if not mix["reverse"] and an:
            v = (state + b) * e
            if fault == "an_wrong_half":       # the next ActNorm's tables of the other half
                bb, ee = np.roll(mix["bias"], C // 2)[None, :, None], np.roll(mix["scale"], C // 2)[None, :, None]
                v = (state + bb) * ee
        if mix["kind"] == "matrix":
            r = fma_chain(mix["matrix"].T.copy() if fault == "matrix_transposed" else mix["matrix"], v)
        else:
            g = mix["gather"] if mix["kind"] == "gather" else np.arange(C)
            if fault == "gather_inverse":
                g = np.argsort(g)
            r = v[:, g]
        if mix["reverse"] and an:
            if fault == "reverse_order":       # (r - b) * e
                return (r - b) * e
            if fused:
                return (r.astype(f64) * e.astype(f64) - b).astype(f32)
            return r * e - b
    return r


def coupling_emu(mode, S, bias, scale, z2, fault=None):
    """fp32: gathered sums S (N, Cout, P) -> (z2', hout, per-element Q31.32 integers (affine), non-finite terms mask)"""
    h = (S + bias[None, :, None]) * scale[None, :, None]
    with np.errstate(all="ignore"):
        if not paired(mode):
            return (z2 + h if mode == ADD_FWD else z2 - h), h, None, None
        sh, rr = h[:, 0::2], h[:, 1::2]
        s = f32(1.0) / (f32(1.0) + np.exp(-(rr + f32(2.0))))
        lg = np.log(s)
        fwd = mode == AFFINE_FWD
        if fault == "logdet_sign":
            term = lg
        else:
            term = lg if fwd else -lg
        r = (z2 + sh) * s if fwd else z2 / s - sh
        fin = np.isfinite(term)
        q = np.rint(np.where(fin, term, 0.0).astype(f64) * Q).astype(np.int64)
    return r, h, q, ~fin


# ---------------------------------------------------------------------------------------------------------------------
# k_cfinish
# ---------------------------------------------------------------------------------------------------------------------
def cfin_geometry(c):
    """the tiling cnet_geo gives for (H, W, tile) as an add_geometry dict (asserted against glowhip_fin_info by the tests)"""
    H, W, HW, tile = c["H"], c["W"], c["H"] * c["W"], c["tile"]
    if HW >= tile:
        NI, R = 1, tile // W
    else:
        NI, R = tile // HW, H
    g = B.add_geometry(c["N"], H, W, R, NI, c["MS"], c["Cout"])
    assert g["lpxt"] == int(np.log2(tile)) and R >= 1
    return g


def plan_scratch_floats(c):
    """cnet_scratch_floats: the largest row split over the smaller tile"""
    tiles = -(-c["N"] * c["H"] * c["W"] // 64)
    return 4 * (c["N"] * c["Cout"] * c["H"] * c["W"] + 2 * tiles * c["Cout"] * c["W"])


def _cf(N, H, W, tile, MS, mode=AFFINE_FWD, Ch=2, mix="none", reverse=0, inplace=True, tape=False, bad=None, **kw):
    c = dict(N=N, H=H, W=W, HW=H * W, tile=tile, MS=MS, mode=mode, Ch=Ch, C=2 * Ch, Cout=2 * Ch if paired(mode) else Ch, mix=mix,
             reverse=reverse, inplace=inplace, tape=tape, bad=bad)
    c.update(kw)
    total = N * H * W
    c["pxb"] = 16 if total < 16384 else 256 if (total >= 131072 and total % 256 == 0 and (H * W) % 256 == 0) else 64
    g = cfin_geometry(c)
    c["halo"] = int(g["halos"])
    c["grid"] = total // c["pxb"]
    lr = g["lpxt"] - {16: 4, 64: 6, 256: 8}[c["pxb"]]
    c["affine_order"] = int(lr >= 0 and c["grid"] % (8 << lr) == 0)
    c["lds"] = (c["C"] * c["pxb"] + (c["C"] ** 2 if mix == "matrix" else 0)) * 4
    c["families"] = ("random",) if paired(mode) else ("exact", "random")
    c["name"] = "cfin-%s-N%d-%dx%d-t%d-MS%d-C%d-%s%s%s%s%s" % (MODE_NAME[mode], N, H, W, tile, MS, 2 * Ch, mix, "-rev" if reverse else "",
                                                              "" if inplace else "-oop", "-tape" if tape else "", "-" + bad if bad else "")
    return c


def cfinish_cases():
    out = []
    # PXB 16: whole-image tiles (NI = 2, NI = 1), 64-pixel tiles with R = 4, and R = 1 (both halo rows on every interior row)
    for MS in (1, 2, 4):
        out += [_cf(3, 8, 8, 128, MS), _cf(3, 8, 8, 64, MS), _cf(3, 16, 16, 64, MS), _cf(2, 4, 64, 64, MS)]
    out += [_cf(8, 8, 8, 64, 2), _cf(2, 16, 16, 64, 1)]                     # grids of whole groups of 8 << lr: the XCD-affine order
    out += [_cf(2, 16, 16, 64, 2, mode=m, Ch=3) for m in (AFFINE_REV, ADD_FWD, ADD_REV)]
    out += [_cf(3, 8, 8, 128, 2, mode=m, Ch=3) for m in (AFFINE_REV, ADD_FWD, ADD_REV)]
    # PXB 64: R = 1 and R = 2 at 64 x 64, R = 1 at 32 x 128, no halos at 8 x 8 (also a grid that is no multiple of 8 << lr)
    for MS in (1, 2, 4):
        out += [_cf(4, 64, 64, 64, MS), _cf(256, 8, 8, 64, MS)]
    out += [_cf(4, 64, 64, 128, 2), _cf(4, 32, 128, 128, 2), _cf(256, 8, 8, 128, 1), _cf(257, 8, 8, 64, 1), _cf(4, 64, 64, 64, 2, mode=ADD_REV)]
    # PXB 256
    out += [_cf(8, 128, 128, 128, MS) for MS in (1, 2)] + [_cf(8, 128, 128, 128, 1, mode=ADD_FWD, Ch=3, mix="matrix")]
    # mixers
    out += [_cf(3, 16, 16, 64, 1, inplace=False), _cf(3, 16, 16, 64, 2, mode=ADD_FWD, inplace=False)]
    for Ch, mode in ((2, AFFINE_FWD), (2, ADD_FWD), (3, ADD_FWD), (24, ADD_FWD), (26, ADD_FWD)):
        out.append(_cf(3, 16, 16, 64, 2, mode=mode, Ch=Ch, mix="matrix", inplace=Ch != 3))
    out += [_cf(4, 64, 64, 64, 1, mode=ADD_FWD, Ch=3, mix="matrix"), _cf(4, 64, 64, 64, 1, mode=AFFINE_FWD, Ch=2, mix="matrix", inplace=False)]
    for kind in ("gather", "identity"):
        out += [_cf(3, 16, 16, 64, 2, mode=ADD_FWD, Ch=3, mix=kind), _cf(3, 8, 8, 128, 1, mode=AFFINE_FWD, Ch=3, mix=kind, inplace=False)]
    out += [_cf(3, 16, 16, 64, 2, mode=ADD_REV, Ch=3, mix="matrix", reverse=1), _cf(3, 16, 16, 64, 1, mode=AFFINE_REV, Ch=2, mix="matrix", reverse=1, inplace=False),
            _cf(3, 16, 16, 64, 1, mode=ADD_REV, Ch=3, mix="gather", reverse=1), _cf(4, 64, 64, 64, 1, mode=ADD_REV, Ch=3, mix="matrix", reverse=1)]
    # the training tape: hout, and the z2 write-back when the mixer works out of place
    out += [_cf(3, 16, 16, 64, 2, tape=True), _cf(3, 16, 16, 64, 2, mode=ADD_FWD, Ch=3, tape=True, mix="gather", inplace=False),
            _cf(3, 16, 16, 64, 1, tape=True, mix="matrix", inplace=False), _cf(4, 64, 64, 64, 1, mode=ADD_FWD, tape=True, mix="matrix", inplace=False)]
    # a sigmoid argument of -inf and one of NaN
    out += [_cf(3, 16, 16, 64, 2, mode=m, bad=b) for m in (AFFINE_FWD, AFFINE_REV) for b in ("inf", "nan")]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


def build_mix_tables(r, C, kind, fam, with_an=True):
    mix = dict(kind=kind, reverse=0, bias=None, scale=None, matrix=None, gather=None)
    if kind == "none":
        return mix
    if with_an:
        if fam == "exact":
            mix.update(bias=ints(r, C, 3), scale=pow2(r, C, -1, 1))
        else:
            mix.update(bias=r.normal(0.0, 0.5, C).astype(f32), scale=np.exp(r.uniform(-1.5, 1.5, C)).astype(f32))
    if kind == "matrix":
        mix["matrix"] = pow2(r, (C, C), -1, 1, True) if fam == "exact" else \
            (np.linalg.qr(r.normal(size=(C, C)))[0] + 0.05 * r.normal(size=(C, C))).astype(f32)
    if kind == "gather":
        g = r.permutation(C).astype(np.int32)
        while C > 2 and (np.argsort(g) == g).all():      # (an involution would hide a table used as its inverse)
            g = r.permutation(C).astype(np.int32)
        mix["gather"] = g
    return mix


def build_cfinish(c, fam):
    r = rng_of("cfinish", c["name"], fam)
    N, Ch, C, Cout, HW = c["N"], c["Ch"], c["C"], c["Cout"], c["HW"]
    g = cfin_geometry(c)
    used = g["floats"]
    if fam == "exact":
        sc = ints(r, used, 3)
        bias, scale, z = ints(r, Cout, 3), pow2(r, Cout, -1, 1), ints(r, (N, C, HW), 3)
    else:
        sc = (r.normal(0.0, 1.0, used) / np.sqrt(g["MS"])).astype(f32)
        bias, scale, z = r.normal(0.0, 0.5, Cout).astype(f32), np.exp(r.uniform(-1.0, 1.0, Cout)).astype(f32), r.normal(0.0, 1.0, (N, C, HW)).astype(f32)
    hpart, hup, hdn = B.split_scratch(g, sc)
    if paired(c["mode"]) and fam == "random":      # sigmoid arguments in [-6, 6]: the last copy of the scale logit makes up the difference
        want = r.uniform(-8.0, 4.0, (N, Ch, HW))
        hpart[-1, :, 1::2] = 0.0
        have, _ = B.gather_ref(g, np.nan_to_num(sc))
        hpart[-1, :, 1::2] = (want / scale[1::2].astype(f64)[None, :, None] - bias[1::2].astype(f64)[None, :, None] - have[:, 1::2]).astype(f32)
    up, dn = B.unused_halo_mask(g)
    hup[:, up] = np.nan
    hdn[:, dn] = np.nan
    d = dict(bias=bias, scale=scale, z=z, used=used)
    if c["bad"]:      # one element of sample 1, channel 0, in a row that takes halo rows
        p = (g["R"] if g["halos"] else 0) * g["W"] + 3
        hpart[0, 1, 1, p] = -np.inf if c["bad"] == "inf" else np.nan
        d["bad_at"] = (1, 0, p)
    full = np.full(plan_scratch_floats(c), np.nan, f32)      # sized as the plan sizes it; what this tiling does not use holds NaN
    assert used <= full.size
    full[:used] = sc
    d["scratch"] = full
    d["mix"] = build_mix_tables(r, C, c["mix"], fam)
    d["mix"]["reverse"] = c["reverse"]
    return d


def cfinish_ref(c, d):
    """-> {name: (reference, bound)} for z_out (N, C, HW), hout (N, Cout, HW), zback (N, Ch, HW) and ld = (total, bound, flags)"""
    g = cfin_geometry(c)
    Ch = c["Ch"]
    with np.errstate(all="ignore"):
        S, mag = B.gather_ref(g, d["scratch"][:d["used"]])
        h, e_h = hout_ref(S, mag, 3 * g["MS"], d["bias"], d["scale"])
        z = d["z"].astype(f64)
        cp = coupling_ref(c["mode"], h, e_h, z[:, Ch:])
        z2, e_z2 = cp["z2"]
        state, e_state = np.concatenate([z[:, :Ch], z2], axis=1), np.concatenate([np.zeros_like(z2), e_z2], axis=1)
        out, e_out = mixer_ref(d["mix"], state, e_state)
    res = dict(z_out=(out, bnd(np.nan_to_num(e_out, nan=0.0, posinf=0.0))), hout=(h, bnd(np.nan_to_num(e_h, nan=0.0, posinf=0.0))),
               zback=(z2, bnd(np.nan_to_num(e_z2, nan=0.0, posinf=0.0))))
    if paired(c["mode"]):
        tot, b, flags = logdet_ref(cp)
        res["ld"] = (tot, b, flip_inf_flags(flags) if c["mode"] == AFFINE_REV else flags)
    return res


def gather_emu(g, scratch, Cout, pair, halo_template, fault=None, touched=None):
    """fp32 emulation of fin_gather_t over the whole map, with the kernel's own index arithmetic on the flat buffer: -> S (N, Cout, HW).
    touched: a list that receives the smallest and largest tile index any load addressed."""
    N, H, W, HW, MS, R, T, lpxt = (g[k] for k in ("N", "H", "W", "HW", "MS", "R", "tiles", "lpxt"))
    hp0 = 0
    hu0 = MS * N * Cout * HW
    hd0 = hu0 + MS * T * Cout * W
    if fault == "hup_hdn_swapped":
        hu0, hd0 = hd0, hu0
    n = np.arange(N)[:, None, None, None]
    ch = np.arange(Cout)[None, :, None, None]
    y = np.arange(H)[None, None, :, None]
    x = np.arange(W)[None, None, None, :]
    p = y * W + x
    flat = np.concatenate([scratch, np.full(HW + 1, np.nan, f32)])      # (a faulty offset may run past the buffer: NaN there)
    S = np.zeros((N, Cout, H, W), f32)
    copies = range(MS - 1) if fault == "ms_copy_dropped" else range(MS)
    with np.errstate(all="ignore"):
        for m in copies:
            S = S + flat[hp0 + ((m * N + n) * Cout + ch) * HW + p]
        if halo_template:
            rr = y & (R - 1)
            tile = (n * HW + (y - rr) * W) >> lpxt
            wd = g["halos"] & (rr == 0) & ((y > 0) | (fault == "halo_at_image_edge"))
            wu = g["halos"] & (rr == R - 1) & ((y < H - 1) | (fault == "halo_at_image_edge"))
            if fault == "unclamped":
                td, tu = tile - 1, tile + 1
            else:
                td, tu = np.where(tile > 0, tile - 1, 0), np.where(tile + 1 < T, tile + 1, tile)
            if touched is not None:
                touched += [int(td.min()), int(tu.max())]
            # a paired map: the odd channel's row lies W floats behind the even one's (the fault takes HW, the offset of hpart)
            odd = (ch & 1) if pair else 0
            ce = ch - odd
            step = HW if fault == "paired_offset_hw" else W
            for m in copies:
                hd = ((m * T + td) * Cout + ce) * W + x + odd * step
                hu = ((m * T + tu) * Cout + ce) * W + x + odd * step
                d0 = flat[np.clip(hd0 + hd, 0, flat.size - 1)]
                u0 = flat[np.clip(hu0 + hu, 0, flat.size - 1)]
                if fault == "hdn_dropped":
                    d0 = np.zeros_like(d0)
                S = S + (np.where(wd, d0, f32(0.0)) + np.where(wu, u0, f32(0.0)))
    return S.reshape(N, Cout, HW)


def cfinish_emu(c, d, fault=None, fused=False, touched=None):
    """fp32 emulation of cfinish_chunk -> dict(z_out, hout, zback, q (per-sample Q31.32 integer), flags)"""
    g = cfin_geometry(c)
    Ch, N = c["Ch"], c["N"]
    S = gather_emu(g, d["scratch"][:d["used"]], c["Cout"], paired(c["mode"]), g["halos"], fault, touched)
    z = d["z"]
    z2, h, q, badm = coupling_emu(c["mode"], S, d["bias"], d["scale"], z[:, Ch:], fault)
    state = np.concatenate([z[:, :Ch], z2], axis=1)
    if fault == "coupling_after_staging":      # the mixer staged z2 before the coupling was applied
        state = z.copy()
    out = mixer_emu(d["mix"], state, fault, fused)
    res = dict(z_out=out, hout=h, zback=z2)
    if q is not None:
        res["q"] = q.sum(axis=(1, 2))
        with np.errstate(all="ignore"):
            hh = (S + d["bias"][None, :, None]) * d["scale"][None, :, None]
            lg = np.log(f32(1.0) / (f32(1.0) + np.exp(-(hh[:, 1::2] + f32(2.0)))))
            t = lg if (c["mode"] == AFFINE_FWD or fault == "logdet_sign") else -lg
        res["flags"] = np.array([(1 if np.isnan(t[n][badm[n]]).any() else 0) | (2 if (t[n][badm[n]] == np.inf).any() else 0) |
                                 (4 if (t[n][badm[n]] == -np.inf).any() else 0) for n in range(N)], np.int64)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# launch_chanmix
# ---------------------------------------------------------------------------------------------------------------------
# N * HW -> (N, HW): 45- and 60-pixel images put several samples into one pixel block and leave the last block partial
def _cm(C, N, HW, kind, reverse=0, an=True, Ca=None, big=False, alias=None, sq=None, **kw):
    c = dict(C=C, N=N, HW=HW, kind=kind, reverse=reverse, an=an, Ca=C // 2 if Ca is None else Ca, alias=alias, sq=sq)
    c.update(kw)
    total = N * HW
    wide = C * C * 4 > 48 * 1024
    c["kernel"] = "wide" if wide else "16" if (total < 16384 and C >= 16) else "64"
    px = 64 if c["kernel"] == "64" else 16
    c["grid"] = [-(-total // px), (1 if alias else -(-C // 32)) if wide else 1, 1]
    c["lds"] = (C * 16 + 32 * C) * 4 if wide else (C * px + C * C) * 4
    c["stage"] = 0 if wide else 1
    c["families"] = ("random",) if sq and sq["noise"] == "philox" else ("exact", "random")      # (a draw is no multiple of 2^-8)
    c["name"] = "mix-%s%s-C%d-N%dx%d-Ca%d%s%s%s" % (kind, "-rev" if reverse else "", C, N, HW, c["Ca"], "" if an else "-noan",
                                                  "-" + alias if alias else "", "-sq-%(src)s-%(noise)s-bs%(bs)d-Wo%(Wo)d" % sq if sq else "")
    return c


def chanmix_cases():
    out = []
    for C in (1, 3, 12, 15, 16, 50, 110):
        out.append(_cm(C, 3, 45, "matrix"))                                  # < 16384 pixels: k_chanmix<16> from C = 16 on
        out.append(_cm(C, 3, 60, "gather", Ca=C))
        out.append(_cm(C, 274, 60, "matrix", Ca=0 if C < 50 else C // 2))   # 16440 pixels: k_chanmix<64>, last block partial
    out += [_cm(12, 3, 45, "matrix", reverse=1), _cm(48, 3, 45, "matrix", reverse=1, Ca=48), _cm(48, 3, 60, "gather", reverse=1),
            _cm(12, 3, 45, "identity"), _cm(12, 3, 45, "matrix", an=False), _cm(12, 3, 45, "identity", an=False, Ca=0),
            _cm(12, 274, 60, "matrix", reverse=1), _cm(16, 274, 60, "gather")]
    for C in (112, 130, 384):
        out += [_cm(C, 3, 45, "matrix"), _cm(C, 3, 60, "matrix", alias="inplace", Ca=C), _cm(C, 3, 45, "gather", reverse=1, Ca=0)]
    out += [_cm(130, 3, 60, "matrix", alias="shifted", Ca=130),       # out = in_a + HW: grid y = 1
            _cm(130, 3, 60, "matrix", reverse=1, alias="inplace", Ca=65)]
    # the squeezed view: source type x noise, with and without a batch stride, odd Wo
    for src in ("f32", "u8"):
        for noise in ("none", "tensor", "philox"):
            for bs in (0, 1):
                out.append(_cm(12, 3, 3 * 5, "matrix" if bs else "gather", Ca=12, sq=dict(src=src, noise=noise, bs=bs, Wo=5, Ho=3)))
    out += [_cm(48, 2, 7 * 9, "matrix", Ca=48, sq=dict(src="u8", noise="philox", bs=1, Wo=9, Ho=7)),
            _cm(12, 260, 7 * 9, "matrix", Ca=12, sq=dict(src="f32", noise="tensor", bs=0, Wo=9, Ho=7))]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


SQ_DIV, SQ_BITS = 256.0, 5      # 8-bit scaling of the data loader; U(0, 2^-5) dequantisation noise


def build_chanmix(c, fam):
    """x as (N, C, HW) is what the reference mixes; in the squeezed-view cases it is DERIVED from d['sq'] (N, C/4, 2 Ho, 2 Wo) by
    squeeze_view, and the noise tensor of a Philox case is filled in by the GPU test from glowhip_dequant_noise"""
    r = rng_of("chanmix", c["name"], fam)
    N, C, HW = c["N"], c["C"], c["HW"]
    d = dict(mix=build_mix_tables(r, C, c["kind"], fam, with_an=c["an"]))
    d["mix"]["reverse"] = c["reverse"]
    if c["sq"]:
        s = c["sq"]
        shape = (N, C // 4, 2 * s["Ho"], 2 * s["Wo"])
        if s["src"] == "u8":
            d["sq"] = r.integers(0, 256, shape).astype(np.uint8)
        else:
            d["sq"] = ints(r, shape, 7) if fam == "exact" else r.normal(0.0, 1.0, shape).astype(f32)
        if s["noise"] != "none":      # (exact: multiples of 2^-8 below 2^-5, as a draw's value never is -- the tensor case only)
            d["noise"] = (r.integers(0, 8, shape).astype(f32) * f32(2.0 ** -8)) if fam == "exact" else (r.random(shape) * 2.0 ** -SQ_BITS).astype(f32)
    else:
        d["x"] = ints(r, (N, C, HW), 3) if fam == "exact" else r.normal(0.0, 1.0, (N, C, HW)).astype(f32)
    return d


def squeeze_view(t):
    """(N, C0, 2 Ho, 2 Wo) -> (N, 4 C0, Ho Wo): channel c of pixel (h, w) = t[n][c / 4][2 h + (c / 2) % 2][2 w + c % 2]
    (Squeeze2d, network/module.py:573-592)"""
    N, C0, H2, W2 = t.shape
    v = t.reshape(N, C0, H2 // 2, 2, W2 // 2, 2).transpose(0, 1, 3, 5, 2, 4)
    return np.ascontiguousarray(v).reshape(N, 4 * C0, (H2 // 2) * (W2 // 2))


def chanmix_input(c, d):
    """-> (x fp64, raw bound of x, x as the kernel's fp32 value or None when it is not one rounding chain we emulate bit for bit)"""
    if not c["sq"]:
        return d["x"].astype(f64), np.zeros(d["x"].shape), d["x"]
    src = squeeze_view(d["sq"])
    x = src.astype(f64)
    e = np.zeros(x.shape)
    x32 = src.astype(f32)
    if c["sq"]["src"] == "u8":
        x = x / SQ_DIV
        x32 = x32 / f32(SQ_DIV)
        e = U * np.abs(x)
    if c["sq"]["noise"] != "none":
        nz = squeeze_view(d["noise"])
        x = x + nz.astype(f64)
        x32 = x32 + nz
        e = e + U * np.abs(x)
    return x, e, x32


def chanmix_ref(c, d):
    x, e_x, _ = chanmix_input(c, d)
    out, e = mixer_ref(d["mix"], x, e_x)
    return out, bnd(e)


def sq_layout(c, d):
    """the squeezed-view source as the flat buffer the kernel addresses: (flat array, sq_bs in elements; 0 = dense).  With a batch
    stride every sample is followed by a gap (NaN / 0xA5) no channel may read"""
    t = d["sq"]
    N, per = t.shape[0], t[0].size
    if not c["sq"]["bs"]:
        return t.reshape(-1).copy(), 0
    bs = per + 2 * t.shape[3] + 3
    flat = np.full(N * bs, 0xA5 if t.dtype == np.uint8 else np.nan, t.dtype)
    for n in range(N):
        flat[n * bs:n * bs + per] = t[n].reshape(-1)
    return flat, bs


def chanmix_emu(c, d, fault=None, fused=False):
    """fp32 emulation of k_chanmix / k_chanmix_wide, the squeezed view with the kernel's own index arithmetic"""
    C, N, HW = c["C"], c["N"], c["HW"]
    if c["sq"]:
        s = c["sq"]
        flat, bs = sq_layout(c, d)
        Wo, sqW = s["Wo"], 2 * s["Wo"]
        n = np.arange(N)[:, None, None]
        cc = np.arange(C)[None, :, None]
        p = np.arange(HW)[None, None, :]
        h, w = p // Wo, p % Wo
        b1, b0 = ((cc >> 1) & 1, cc & 1) if fault != "squeeze_bit_order" else (cc & 1, (cc >> 1) & 1)
        rel = ((cc >> 2) * (2 * (HW // Wo)) + 2 * h + b1) * sqW + 2 * w + b0
        dense = n * (C >> 2) * (4 * HW)
        img = n * bs if bs else dense
        x = flat[img + rel].astype(f32)
        if s["src"] == "u8":
            x = x / f32(SQ_DIV)
        if s["noise"] != "none":      # the noise is dense whatever the source's stride
            nz = np.concatenate([d["noise"].reshape(-1), np.full(N * (bs + 1), np.nan, f32)])
            x = x + nz[(img if fault == "noise_strided_index" else dense) + rel]
    else:
        x = d["x"]
        Ca = c["Ca"]
        if fault == "ca_off_by_one" and 0 < Ca < C:      # the split one channel late: channel Ca from the plane behind in_a's Ca channels
            x = x.copy()
            x[:, Ca + 1:] = d["x"][:, Ca:-1]
            x[:, Ca] = np.nan
    return mixer_emu(d["mix"], x, fault, fused)


# ---------------------------------------------------------------------------------------------------------------------
# k_dn_fin / k_dn_prep
# ---------------------------------------------------------------------------------------------------------------------
DN_HW = {3: (1, 3), 12: (3, 4), 16: (4, 4), 64: (8, 8), 96: (8, 12), 128: (8, 16)}
DN_HIDDEN = 32


def dn_layout(c):
    """dn_carve for (N, C, H, W, hidden, Cout): byte offsets and plane sizes (asserted against glowhip_fin_info)"""
    P, SLN = c["N"] * c["H"] * c["W"], c["N"] * (c["H"] + 2) * (c["W"] + 2)
    up = lambda b: -(-b // 256) * 256      # noqa: E731
    sizes = [4 * c["C"] * P, 4 * (c["C"] // 2) * SLN, 4 * DN_HIDDEN * P, 4 * DN_HIDDEN * SLN, 4 * 8 * c["Cout"] * P]
    off = np.concatenate([[0], np.cumsum([up(s) for s in sizes])])
    per = 4 * (c["C"] * c["H"] * c["W"] + (c["C"] // 2) * (c["H"] + 2) * (c["W"] + 2) + DN_HIDDEN * c["H"] * c["W"] +
               DN_HIDDEN * (c["H"] + 2) * (c["W"] + 2) + 8 * c["Cout"] * c["H"] * c["W"]) + 8 * 256
    assert off[5] <= c["N"] * per
    return dict(u_off=int(off[0]), ypad_off=int(off[1]), part_off=int(off[4]), u_plane=c["C"] * P, ypad_plane=(c["C"] // 2) * SLN, bytes=c["N"] * per,
                P=P, SLN=SLN)


def dnfin_cases():
    out = []
    for hw in (3, 12, 16, 64, 96, 128):
        for i, (C, mode) in enumerate(((32, AFFINE_FWD), (64, ADD_FWD), (32, AFFINE_REV), (64, ADD_REV))):
            ks = (1, 2, 4, 8)[(i + list(DN_HW).index(hw)) % 4]
            fwd = mode in (AFFINE_FWD, ADD_FWD)
            want_u, an = (1, fwd) if (hw, i) not in ((16, 0), (64, 1)) else (0, False)
            out.append(dict(N=3, C=C, H=DN_HW[hw][0], W=DN_HW[hw][1], HW=hw, Ch=C // 2, Cout=C if paired(mode) else C // 2, mode=mode, ks=ks,
                            want_u=want_u, an=an))
    out.append(dict(N=3, C=32, H=4, W=4, HW=16, Ch=16, Cout=32, mode=AFFINE_FWD, ks=8, want_u=1, an=False))      # u without an ActNorm
    for c in out:
        c["families"] = ("random",) if paired(c["mode"]) else ("exact", "random")
        c["grid"] = [-(-c["N"] * c["HW"] // 64), (c["C"] // 8 + 3) // 4, 1]
        c["name"] = "dnfin-%s-C%d-HW%d-ks%d%s%s" % (MODE_NAME[c["mode"]], c["C"], c["HW"], c["ks"], "-u" if c["want_u"] else "", "-an" if c["an"] else "")
    return out


def build_dnfin(c, fam):
    r = rng_of("dnfin", c["name"], fam)
    N, C, Ch, Cout, HW, ks = c["N"], c["C"], c["Ch"], c["Cout"], c["HW"], c["ks"]
    if fam == "exact":
        part = ints(r, (ks, N, Cout, HW), 3)
        d = dict(bias=ints(r, Cout, 3), scale=pow2(r, Cout, -1, 1), z=ints(r, (N, C, HW), 3))
    else:
        part = (r.normal(0.0, 1.0, (ks, N, Cout, HW)) / np.sqrt(ks)).astype(f32)
        d = dict(bias=r.normal(0.0, 0.5, Cout).astype(f32), scale=np.exp(r.uniform(-1.0, 1.0, Cout)).astype(f32), z=r.normal(0.0, 1.0, (N, C, HW)).astype(f32))
        if paired(c["mode"]):
            want = r.uniform(-8.0, 4.0, (N, Ch, HW))
            part[-1, :, 1::2] = (want / d["scale"][1::2].astype(f64)[None, :, None] - d["bias"][1::2].astype(f64)[None, :, None] -
                                 part[:-1, :, 1::2].astype(f64).sum(axis=0)).astype(f32)
    d["part"] = part
    d["mix"] = build_mix_tables(r, C, "identity", fam, with_an=c["an"])
    return d


def dnfin_ref(c, d):
    Ch = c["Ch"]
    p = d["part"].astype(f64)
    h, e_h = hout_ref(p.sum(axis=0), np.abs(p).sum(axis=0), c["ks"], d["bias"], d["scale"])
    z = d["z"].astype(f64)
    cp = coupling_ref(c["mode"], h, e_h, z[:, Ch:])
    res = dict(state=(np.concatenate([z[:, :Ch], cp["z2"][0]], axis=1), bnd(np.concatenate([np.zeros_like(cp["z2"][1]), cp["z2"][1]], axis=1))))
    if paired(c["mode"]):
        tot, b, flags = logdet_ref(cp)
        res["ld"] = (tot, b, flags)
    return res


def dnfin_emu(c, d, fault=None):
    S = np.zeros(d["part"].shape[1:], f32)
    for k in range(c["ks"] - (1 if fault == "ks_partial_dropped" else 0)):
        S = S + d["part"][k]
    z2, _, q, _ = coupling_emu(c["mode"], S, d["bias"], d["scale"], d["z"][:, c["Ch"]:], fault)
    res = dict(state=np.concatenate([d["z"][:, :c["Ch"]], z2], axis=1))
    if q is not None:
        res["q"] = q.sum(axis=(1, 2))
    return res


def sh2_split(state32, bias, scale):
    """the SH2 operand of fp32 values: (hi, lo) fp16 of v = 16 fl(fl(z + b) e) (no tables: v = 16 z), shaped like the input"""
    v = state32 if bias is None else (state32 + bias[None, :, None]) * scale[None, :, None]
    v = v * f32(SH2)
    with np.errstate(over="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(f32)).astype(np.float16)
    return hi, lo


def sh2_plane(t, slots, slot_of_pixel):
    """(N, C, HW) fp16 values -> the half plane [C / 8][slots][8] as a flat uint16 array; slots no pixel maps to hold 0xA5A5"""
    N, C, HW = t.shape
    out = np.full((C // 8, slots, 8), 0xA5A5, np.uint16)
    v = t.view(np.uint16).transpose(1, 0, 2).reshape(C // 8, 8, N * HW)      # [chunk][c % 8][p]
    out[:, slot_of_pixel, :] = v.transpose(0, 2, 1)
    return out.reshape(-1)


def pad_slots(N, H, W):
    n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    return (n * (H + 2) * (W + 2) + (y + 1) * (W + 2) + x + 1).reshape(-1)


def dnprep_cases():
    out = []
    for hw in (3, 12, 16, 64, 96, 128):
        for C, reverse, an, copy in ((32, 0, True, True), (64, 0, False, False), (32, 1, False, True), (64, 1, False, False)):
            c = dict(N=3, C=C, H=DN_HW[hw][0], W=DN_HW[hw][1], HW=hw, Ch=C // 2, Cout=32, reverse=reverse, an=an, copy=copy)
            c["grid"] = [-(-3 * hw // 64), (C // 4 + 3) // 4, 1]
            c["name"] = "dnprep-%s-C%d-HW%d%s%s" % ("rev" if reverse else "fwd", C, hw, "-an" if an else "", "-copy" if copy else "")
            out.append(c)
    return out


def build_dnprep(c):
    r = rng_of("dnprep", c["name"])
    d = dict(src=(r.normal(0.0, 1.0, (c["N"], c["C"], c["HW"])) * np.exp2(r.integers(-12, 6, (1, c["C"], 1)))).astype(f32))
    d["mix"] = build_mix_tables(r, c["C"], "identity", "random", with_an=c["an"])
    return d

"""Host side of the per-kernel tests of the training sweep's HBM-bound gradient kernels (csrc/backward.hip), numpy only: the fp64
reference of every operation, the per-element bound each kernel is held to, the two input families, and the table of cases
tests/test_gpu_bwd_kernels.py launches through glowhip_debug_bwd and tests/test_bwd_oracle_host.py checks on the CPU.

The formulas are those of the kernels' header comments (forward: network/model.py:105-113, network/module.py:526-530):

  coupling tail   affine: s = sigmoid(r + 2), r = hout[2c + 1]; g_y2 = g2 s; g_shift = g2 s; g_r = (g2 z2' / s + gld / s) s (1 - s)
                  additive: g_y2 = g_h = g2.            g_pre = g_h e4;  d b = sum g_pre;  d logs = 3 sum g_h hout
  split prior     d = z2 - mean, q = exp(-2 logs): g_z2 = -gld d q; g_mean = gld d q; g_logs = gld (d d q - 1); g_pre, d b, d logs as above
  ReLU / ActNorm  g_u = g_h (h > 0) e;  d b = sum g_u;  d logs = 3 sum g_h h
  channel mixer   v = (x + b) e;  g = g_y (+ add_scale * the add_part gather on the first add_C channels);  g_v = W^T g (gather:
                  g_v[i] = g[inv[i]]);  g_x = g_v e;  dW[o][i] = sum g[o] v[i];  d b = sum g_v e;  d logs = 3 sum g_v v
  top prior       g_z = -gld (z - mean) exp(-2 logs) (+ gz_in)
  flipT           wT[i][o][t] = w[o][i][KK - 1 - t]
  logs_from_dw    out[r] = 3 (<w[r], dw[r]> + b[r] db[r])
  finalize        gld = -nll_grad inv;  out[e] = sum over copies of acc[copy stride + e] + G add_mul (invconv: ... winv[i C + o]),  G = sum gld

THE add_part LAYOUT (written from what csrc/cnet_fin.h documents; gather_ref below).  A backward k_cnet launch leaves, for Cout
channels of an (N, H, W) map cut into tiles of R rows (or of NI whole images), MS row-split copies of every element and the halo
rows a tile contributes to its neighbours, in one scratch buffer of  MS N Cout HW + 2 MS tiles Cout W  floats:
    hpart[MS][N][Cout][HW]   then   hup[MS][tiles][Cout][W]   then   hdn[MS][tiles][Cout][W]
The element (n, c, y, x) is the sum of its MS copies; with halos (NI == 1 and R < H) the first row of a tile (y % R == 0, y > 0)
adds the previous tile's hdn row and the last row (y % R == R - 1, y < H - 1) the next tile's hup row, tile = (n HW + (y - y % R) W)
>> lpxt.  Slots no element uses -- hup of an image's first tile, hdn of its last, every halo row where there are no halos -- may
hold anything: unused_halo_mask marks them and the tests fill them with NaN.

THE BOUNDS.  u = 2^-24; every fp32 operation is taken as one rounding to nearest, |error| <= u |result|; expf as 2 u (as
tests/objective_oracle.py allows).  Nothing below is fitted to a kernel's output; tests/test_bwd_oracle_host.py shows that an fp32
emulation of the promised arithmetic stays inside and that eleven single faults leave.  bnd() adds 2^-10 relative for second-order
terms and 2^-140 for roundings of subnormal intermediates.
  * sigmoidf_(x) = 1 / (1 + expf(-x)), x = fl(r + 2):  the argument's rounding and expf give exp(-x) to (|x| + 2) u, its share of the
    denominator is 1 - s, then one addition and one division:  es = 2 + (1 - s)(2 + |x|)  roundings.
  * affine tail:  g_y2 = g_shift = fl(g2 s): es + 1;  g_pre adds one.  g_r = ((g2 fl(z / s) + gld / s) s)(1 - s):  A = g2 z / s carries
    es + 2, B = gld / s es + 1, their sum one more on |A| + |B|; times s: es + 1; fl(1 - s) is exact in 1 but inherits s's error
    enlarged by the cancellation -- es s / (1 - s), the u / (1 - s) term torch's fp32 autograd carries too -- plus 1; last product 1:
        |err g_r| <= u s (1 - s) (|A| + |B|) (2 es + 6 + es s / (1 - s))
  * split prior:  d one rounding, q two (the argument -2 logs is exact): -gld d q and gld d q 5 u; P = d d q 6 u, P - 1 one on
    |P - 1|, times gld one:  |err g_logs| <= u |gld| (6 P + 2 |P - 1|).
  * ReLU / ActNorm:  g_u one rounding; the mask is a select.
  * mixer:  v two roundings.  The gather adds MS copies, then per copy one sum of the two selected halo values and one addition:
    3 MS additions, one product with add_scale, one addition to g_y:  |err g| <= u ((3 MS + 2) |add_scale| sum|parts| + |g_y|).
    g_v is a chain of C fused multiply-adds: C u sum|W g| + sum|W| err g.  g_x one more.  Block sums (64 pixels, 32 in the wide
    kernel) are chains of fused multiply-adds: PX u sum|terms| + the operands' errors.
  * top prior: 5 u |g| (+ u (|g| + |gz_in|) for the addition).
  * Per-channel sums (d b, d logs): the fp32 partial sums inside a lane segment / a workgroup's slice add L values in some order:
    (L - 1) u sum|terms| on top of the terms' own errors (products with h / hout one rounding each); L = min(HW, 256) in
    k_coupling_bwd4, min(HW, 1024) in k_act_bwd, 1 in the element-per-thread kernels, which sum in fp64.  The fp64 combination
    (shuffles, atomics, the sum over copies) adds 2^-50 sum|terms|.
  * Finalised gradients, gld and logs_from_dw's output: one fp32 store of an fp64 value, u |value| + 2^-50 sum|terms|.
  * split-K reductions beside the mixer: `splits` fp32 additions in order, (splits - 1) u sum|partials|.

FAMILIES.  `exact`: small integers times powers of two with e4 / scale / matrix entries powers of two, so that every product and
every partial sum in any order is an fp32 number: the kernel must return the reference value for value (no expf, so: additive
coupling, ReLU / ActNorm, mixer, flipT, finalize, the add_part gather with add_scale = 2^-18).  `random`: per-sample gld of both
signs near 1 / (N ln2 12288), gradients in per-channel blocks at 1, 1e-3 and 1e-7, sigmoid arguments in [-6, 6], split logs in
[-2, 2], tape h half exact zeros; add_scale = 1 / 3: every element within the bound, no outliers."""
import zlib

import numpy as np

U = 2.0 ** -24
F64 = 2.0 ** -50
f32, f64 = np.float32, np.float64
LN2_CHW = np.log(2.0) * 12288.0


def bnd(x):
    return np.asarray(x, f64) * (1.0 + 2.0 ** -10) + 2.0 ** -140


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def ints(r, shape, hi):
    return r.integers(-hi, hi + 1, size=shape).astype(f32)


def pow2(r, shape, lo, hi, signed=False):
    v = np.exp2(r.integers(lo, hi + 1, size=shape)).astype(f32)
    return v * r.choice(np.array([-1.0, 1.0], f32), size=shape) if signed else v


def chan_blocks(C):
    """per-channel gradient magnitudes 1, 1e-3, 1e-7 (a channel's sums then hold one magnitude)"""
    return np.array([1.0, 1e-3, 1e-7])[np.arange(C) % 3]


def gld_random(r, N):
    return (r.uniform(0.5, 1.5, N) * r.choice([-1.0, 1.0], N) / (N * LN2_CHW)).astype(f32)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def inside(got, ref, bound):
    """every element within its bound (a NaN anywhere is outside)"""
    return bool(np.all(np.abs(np.asarray(got, f64) - ref) <= bound))


def worst(got, ref, bound):
    e = np.abs(np.asarray(got, f64) - ref)
    return float(np.max(np.where(bound > 0, e / np.where(bound > 0, bound, 1.0), np.where(e > 0, np.inf, 0.0)), initial=0.0))


def seg_bound(terms, errs, L, axes):
    """bound of an fp64 accumulator fed with fp32 partial sums of L terms: sum of `errs` + ((L - 1) u + 2^-50) sum|terms|"""
    return bnd(errs.sum(axis=axes) + ((L - 1) * U + F64) * np.abs(terms).sum(axis=axes))


# ---------------------------------------------------------------------------------------------------------------------
# coupling tail
# ---------------------------------------------------------------------------------------------------------------------
def coupling_cases():
    out = []
    for Ch, HW in ((6, 4), (6, 16), (6, 64), (24, 64), (6, 256), (3, 1024)):
        for affine in (1, 0):
            for copies, inplace in ((1, False), (16, True)):
                out.append(dict(Ch=Ch, HW=HW, N=3, affine=affine, copies=copies, inplace=inplace, vec4=True, misalign=None))
    for HW in (2, 60, 320):
        for affine in (1, 0):
            out.append(dict(Ch=6, HW=HW, N=3, affine=affine, copies=1, inplace=bool(affine), vec4=False, misalign=None))
    out.append(dict(Ch=6, HW=64, N=3, affine=1, copies=1, inplace=False, vec4=False, misalign="hout"))
    out.append(dict(Ch=6, HW=64, N=3, affine=0, copies=16, inplace=False, vec4=False, misalign="gpre"))
    for c in out:
        c["Cout"] = 2 * c["Ch"] if c["affine"] else c["Ch"]
        c["families"] = ("random",) if c["affine"] else ("exact", "random")
        c["L"] = min(c["HW"], 256) if c["vec4"] else 1
        c["name"] = "coupling-%s-Ch%d-HW%d-x%d%s%s" % ("affine" if c["affine"] else "add", c["Ch"], c["HW"], c["copies"], "-inplace" if c["inplace"] else "",
                                                         "-off4" + c["misalign"] if c["misalign"] else "")
    return out


def build_coupling(case, fam):
    r = rng_of("coupling", case["name"], fam)
    N, Ch, Cout, HW = case["N"], case["Ch"], case["Cout"], case["HW"]
    if fam == "exact":      # additive only
        return dict(hout=ints(r, (N, Cout, HW), 15), z2=ints(r, (N, Ch, HW), 15), g2=ints(r, (N, Ch, HW), 15) * pow2(r, (1, Ch, 1), -20, 3),
                    e4=pow2(r, Cout, -3, 3), gld=pow2(r, N, -20, -18, True), g1=ints(r, (N, Ch, HW), 15), z1=ints(r, (N, Ch, HW), 15))
    hout = r.normal(0.0, 1.0, (N, Cout, HW))
    if case["affine"]:
        hout[:, 1::2] = r.uniform(-8.0, 4.0, (N, Ch, HW))      # r + 2 in [-6, 6]
    g2 = r.normal(0.0, 1.0, (N, Ch, HW)) * chan_blocks(Ch)[None, :, None]
    return dict(hout=hout.astype(f32), z2=r.normal(0.0, 1.0, (N, Ch, HW)).astype(f32), g2=g2.astype(f32),
                e4=np.exp(r.uniform(-1.5, 1.5, Cout)).astype(f32), gld=gld_random(r, N),
                g1=r.normal(0.0, 1.0, (N, Ch, HW)).astype(f32), z1=r.normal(0.0, 1.0, (N, Ch, HW)).astype(f32))


def coupling_ref(case, d):
    """-> {name: (reference, bound)} for gy2 (N, Ch, HW), gpre (N, Cout, HW), acc_b, acc_l (Cout)"""
    h, z, g, e, gld = (d[k].astype(f64) for k in ("hout", "z2", "g2", "e4", "gld"))
    L = case["L"]
    if not case["affine"]:
        gh, b_gh = g, np.zeros_like(g)
        gy, b_gy = g, np.zeros_like(g)
    else:
        x = h[:, 1::2] + 2.0
        s = sigmoid(x)
        es = 2.0 + (1.0 - s) * (2.0 + np.abs(x))
        gy = g * s
        b_gy = U * np.abs(gy) * (es + 1.0)
        A, B = g * z / s, gld[:, None, None] / s
        gr = (A + B) * s * (1.0 - s)
        b_gr = U * s * (1.0 - s) * (np.abs(A) + np.abs(B)) * (2.0 * es + 6.0 + es * s / (1.0 - s))
        gh, b_gh = np.empty_like(h), np.empty_like(h)
        gh[:, 0::2], gh[:, 1::2], b_gh[:, 0::2], b_gh[:, 1::2] = gy, gr, b_gy, b_gr
    gpre = gh * e[None, :, None]
    b_gpre = b_gh * e[None, :, None] + U * np.abs(gpre)
    tl = gh * h
    b_tl = b_gh * np.abs(h) + U * np.abs(tl)
    return dict(gy2=(gy, bnd(b_gy)), gpre=(gpre, bnd(b_gpre)),
                acc_b=(gpre.sum(axis=(0, 2)), seg_bound(gpre, b_gpre, L, (0, 2))),
                acc_l=(3.0 * tl.sum(axis=(0, 2)), 3.0 * seg_bound(tl, b_tl, L, (0, 2))))


# ---------------------------------------------------------------------------------------------------------------------
# split prior
# ---------------------------------------------------------------------------------------------------------------------
def split_cases():
    return [dict(name="split-Ch%d-HW%d" % (Ch, HW), Ch=Ch, HW=HW, N=3, families=("random",)) for HW in (4, 60, 256, 320) for Ch in (3, 6)]


def build_split(case, fam):
    r = rng_of("split", case["name"], fam)
    N, Ch, HW = case["N"], case["Ch"], case["HW"]
    hout = r.normal(0.0, 1.0, (N, 2 * Ch, HW))
    hout[:, 1::2] = r.uniform(-2.0, 2.0, (N, Ch, HW))
    return dict(hout=hout.astype(f32), z2=r.normal(0.0, 1.5, (N, Ch, HW)).astype(f32), e4=np.exp(r.uniform(-1.5, 1.5, 2 * Ch)).astype(f32),
                gld=gld_random(r, N))


def split_ref(case, d):
    h, z, e, gld = (d[k].astype(f64) for k in ("hout", "z2", "e4", "gld"))
    G = gld[:, None, None]
    dd, q = z - h[:, 0::2], np.exp(-2.0 * h[:, 1::2])
    gm = G * dd * q
    P = dd * dd * q
    gl = G * (P - 1.0)
    gh, b_gh = np.empty_like(h), np.empty_like(h)
    gh[:, 0::2], gh[:, 1::2] = gm, gl
    b_gh[:, 0::2], b_gh[:, 1::2] = 5.0 * U * np.abs(gm), U * np.abs(G) * (6.0 * P + 2.0 * np.abs(P - 1.0))
    gpre = gh * e[None, :, None]
    b_gpre = b_gh * e[None, :, None] + U * np.abs(gpre)
    tl = gh * h
    b_tl = b_gh * np.abs(h) + U * np.abs(tl)
    return dict(gz2=(-gm, bnd(5.0 * U * np.abs(gm))), gpre=(gpre, bnd(b_gpre)),
                acc_b=(gpre.sum(axis=(0, 2)), seg_bound(gpre, b_gpre, 1, (0, 2))),
                acc_l=(3.0 * tl.sum(axis=(0, 2)), 3.0 * seg_bound(tl, b_tl, 1, (0, 2))))


# ---------------------------------------------------------------------------------------------------------------------
# ReLU / ActNorm
# ---------------------------------------------------------------------------------------------------------------------
def act_cases():
    out = [dict(Cm=Cm, HW=HW, N=2, vec4=True) for HW in (4, 64, 256, 512, 1024, 4096) for Cm in (5, 32)]
    out += [dict(Cm=Cm, HW=HW, N=2, vec4=False) for HW in (2, 60, 300) for Cm in (5, 32)]
    for c in out:
        c["name"] = "act-Cm%d-HW%d" % (c["Cm"], c["HW"])
        c["L"] = min(c["HW"], 1024) if c["vec4"] else 1
        c["families"] = ("exact", "random")
    return out


def build_act(case, fam):
    r = rng_of("act", case["name"], fam)
    shape = (case["N"], case["Cm"], case["HW"])
    mask = r.random(shape) < 0.5      # about half the tape exactly 0.0f
    if fam == "exact":
        return dict(h=np.where(mask, 0.0, r.integers(1, 8, shape)).astype(f32), g=ints(r, shape, 7) * pow2(r, (1, case["Cm"], 1), -20, 3),
                    e=pow2(r, case["Cm"], -3, 3))
    g = r.normal(0.0, 1.0, shape) * chan_blocks(case["Cm"])[None, :, None]
    return dict(h=np.where(mask, 0.0, np.abs(r.normal(0.0, 1.0, shape)) + 1e-3).astype(f32), g=g.astype(f32),
                e=np.exp(r.uniform(-1.5, 1.5, case["Cm"])).astype(f32))


def act_ref(case, d):
    h, g, e = (d[k].astype(f64) for k in ("h", "g", "e"))
    gu = np.where(h > 0.0, g * e[None, :, None], 0.0)
    tl = g * h
    return dict(gu=(gu, bnd(U * np.abs(gu))),
                acc_b=(gu.sum(axis=(0, 2)), seg_bound(gu, U * np.abs(gu), case["L"], (0, 2))),
                acc_l=(3.0 * tl.sum(axis=(0, 2)), 3.0 * seg_bound(tl, U * np.abs(tl), case["L"], (0, 2))))


# ---------------------------------------------------------------------------------------------------------------------
# the add_part gather (layout in the module docstring)
# ---------------------------------------------------------------------------------------------------------------------
def add_geometry(N, H, W, R, NI, MS, Cout):
    HW = H * W
    px_tile = R * W if NI == 1 else NI * HW
    lpxt = int(np.log2(px_tile))
    assert 1 << lpxt == px_tile
    tiles = -(-N * HW // px_tile)
    return dict(N=N, H=H, W=W, HW=HW, R=R, NI=NI, MS=MS, Cout=Cout, lpxt=lpxt, tiles=tiles, halos=(NI == 1 and R < H),
                floats=MS * N * Cout * HW + 2 * MS * tiles * Cout * W)


def split_scratch(geo, scratch):
    """the flat scratch buffer as (hpart, hup, hdn) views"""
    MS, N, C, HW, W, T = (geo[k] for k in ("MS", "N", "Cout", "HW", "W", "tiles"))
    a, b = MS * N * C * HW, MS * T * C * W
    return scratch[:a].reshape(MS, N, C, HW), scratch[a:a + b].reshape(MS, T, C, W), scratch[a + b:a + 2 * b].reshape(MS, T, C, W)


def tile_of(geo, n, y):
    return (n * geo["HW"] + (y - y % geo["R"]) * geo["W"]) >> geo["lpxt"]


def unused_halo_mask(geo):
    """(hup, hdn) boolean masks [tiles]: True where no element of the map reads the tile's row"""
    T = geo["tiles"]
    up, dn = np.ones(T, bool), np.ones(T, bool)
    if geo["halos"]:
        for n in range(geo["N"]):
            for y in range(geo["H"]):
                r = y % geo["R"]
                if r == 0 and y > 0:
                    dn[tile_of(geo, n, y) - 1] = False
                if r == geo["R"] - 1 and y < geo["H"] - 1:
                    up[tile_of(geo, n, y) + 1] = False
    return up, dn


def gather_ref(geo, scratch):
    """-> (sum (N, Cout, HW) float64, sum of magnitudes): every element from the slots the layout assigns to it"""
    hpart, hup, hdn = (a.astype(f64) for a in split_scratch(geo, scratch))
    H, W, R = geo["H"], geo["W"], geo["R"]
    s = hpart.sum(axis=0).reshape(geo["N"], geo["Cout"], H, W)
    m = np.abs(hpart).sum(axis=0).reshape(geo["N"], geo["Cout"], H, W)
    if geo["halos"]:
        for n in range(geo["N"]):
            for y in range(H):
                t = tile_of(geo, n, y)
                if y % R == 0 and y > 0:
                    s[n, :, y] += hdn[:, t - 1].sum(axis=0)
                    m[n, :, y] += np.abs(hdn[:, t - 1]).sum(axis=0)
                if y % R == R - 1 and y < H - 1:
                    s[n, :, y] += hup[:, t + 1].sum(axis=0)
                    m[n, :, y] += np.abs(hup[:, t + 1]).sum(axis=0)
    return s.reshape(geo["N"], geo["Cout"], H * W), m.reshape(geo["N"], geo["Cout"], H * W)


def build_scratch(geo, r, fam):
    n = geo["floats"]
    scratch = (ints(r, n, 7) * f32(2.0 ** 18)) if fam == "exact" else r.normal(0.0, 1.0, n).astype(f32)
    _, hup, hdn = split_scratch(geo, scratch)
    up, dn = unused_halo_mask(geo)
    hup[:, up] = np.nan
    hdn[:, dn] = np.nan
    return scratch


# ---------------------------------------------------------------------------------------------------------------------
# channel mixer
# ---------------------------------------------------------------------------------------------------------------------
NARROW_C, WIDE_PX, WIDE_COPIES = 192, 32, 8
REDUCE_JOBS = (dict(splits=3, Mpad=128, Npad=64, Mreal=108, Nreal=50, mode=1), dict(splits=9, Mpad=128, Npad=128, Mreal=100, Nreal=128, mode=0),
               dict(splits=2, Mpad=256, Npad=64, Mreal=130, Nreal=7, mode=0))
# N * HW -> (N, HW); HW = 20: a 64-pixel block spans four images and the last block is partial
PIXELS = {60: (3, 20), 300: (15, 20), 1024: (4, 256), 12: (3, 4), 80: (5, 16), 320: (5, 64)}


def wide_copies(pixels):
    return max(1, min(WIDE_COPIES, -(-pixels // WIDE_PX)))


def _mix(C, px, mode, copies, inplace, **kw):
    N, HW = PIXELS[px]
    c = dict(C=C, N=N, HW=HW, mode=mode, copies=copies, inplace=inplace, misalign_w=False, jobs=(), add=None, families=("exact", "random"))
    c.update(kw)
    wide = C > NARROW_C
    c["PX"] = WIDE_PX if wide else 64
    c["blocks"] = -(-N * HW // c["PX"])
    lds = 3 * C * 65 * 4
    c["w_lds"] = int(mode == "matrix" and not wide and C % 4 == 0 and lds + C * C * 4 <= 64 * 1024 and not c["misalign_w"])
    c["lds"] = ((C * 32 if mode == "matrix" else 0) + C * 33 + 2 * 32 * 33) * 4 if wide else lds + c["w_lds"] * C * C * 4
    c["kernel"] = "wide" if wide else "reduce" if c["jobs"] and c["lds"] <= 48 * 1024 else "plain"
    c["rblocks"] = max(-(-j["Mreal"] * ((j["Nreal"] + 3) // 4) // 256) for j in c["jobs"]) if c["kernel"] == "reduce" else 0
    c["name"] = "mix-%s-C%d-px%d-x%d%s%s%s%s" % (mode, C, px, copies, "-inplace" if inplace else "", "-off4w" if c["misalign_w"] else "",
                                                 "-%djobs" % len(c["jobs"]) if c["jobs"] else "",
                                                 "-add-MS%(MS)d-H%(H)d-R%(R)d-NI%(NI)d" % c["add"] if c["add"] else "")
    return c


def mixer_cases():
    out = []
    for C, mis in ((4, False), (12, False), (6, False), (12, True), (48, False), (96, False), (192, False)):
        for px, copies, inplace in ((60, 1, False), (300, 16, True), (1024, 1, True)):
            out.append(_mix(C, px, "matrix", copies, inplace, misalign_w=mis))
    for C in (12, 48):
        for mode in ("gather", "identity"):
            for px, copies, inplace in ((60, 1, True), (300, 16, False), (1024, 1, False)):
                out.append(_mix(C, px, mode, copies, inplace))
    return out


def mixer_reduce_cases():
    return [_mix(C, 300, "matrix", 16, True, jobs=REDUCE_JOBS[:nj]) for C, nj in ((12, 1), (12, 3), (48, 1), (48, 3), (96, 1))]


def mixer_add_cases():
    out = []
    geos = [(8, 2, 1, ms) for ms in (1, 2, 4)] + [(8, 1, 1, ms) for ms in (1, 2, 4)] + [(8, 8, 1, ms) for ms in (2, 4)] + \
           [(2, 4, 2, ms) for ms in (2, 4)] + [(8, 8, 1, 1)]
    for H, R, NI, MS in geos:
        N, W = 3, 8
        PIXELS[N * H * W] = (N, H * W)
        out.append(_mix(12, N * H * W, "matrix", 16, True, add=dict(H=H, W=W, R=R, NI=NI, MS=MS, C=6)))
    return out


def mixer_wide_cases():
    return [_mix(C, px, mode, wide_copies(px), False) for C in (256, 384, 512, 200) for mode in ("matrix", "gather") for px in (12, 80, 320)]


def case_geometry(case):
    a = case["add"]
    return add_geometry(case["N"], a["H"], a["W"], a["R"], a["NI"], a["MS"], a["C"])


def add_scale_of(fam):
    return f32(2.0 ** -18) if fam == "exact" else f32(1.0 / 3.0)


def build_mixer(case, fam):
    r = rng_of("mixer", case["name"], fam)
    N, C, HW = case["N"], case["C"], case["HW"]
    d = {}
    if fam == "exact":
        gi, xi = (7, 7) if C <= 48 else (3, 3)      # (the d logs block sums stay below 2^24 units at C = 512)
        gs = f32(1.0 if case["add"] else 2.0 ** -10)      # (the gathered sums are integers: g_y on the same grid)
        d.update(x=ints(r, (N, C, HW), xi), bias=ints(r, C, xi), scale=pow2(r, C, -3, 3), gy=ints(r, (N, C, HW), gi) * gs)
        if case["mode"] == "matrix":
            d["matrix"] = pow2(r, (C, C), -1, 1, True)
    else:
        gy = r.normal(0.0, 1.0, (N, C, HW)) * chan_blocks(C)[None, :, None]
        d.update(x=r.normal(0.0, 1.0, (N, C, HW)).astype(f32), bias=r.normal(0.0, 0.5, C).astype(f32),
                 scale=np.exp(r.uniform(-1.5, 1.5, C)).astype(f32), gy=gy.astype(f32))
        if case["mode"] == "matrix":      # a rotation plus noise, as a trained invconv weight
            d["matrix"] = (np.linalg.qr(r.normal(size=(C, C)))[0] + 0.05 * r.normal(size=(C, C))).astype(f32)
    if case["mode"] == "gather":
        d["inv"] = r.permutation(C).astype(np.int32)
    if case["add"]:
        d["scratch"] = build_scratch(case_geometry(case), r, fam)
        d["add_scale"] = add_scale_of(fam)
    d["partials"] = [(ints(r, (j["splits"], j["Mpad"], j["Npad"]), 100) if fam == "exact" else r.normal(0.0, 1.0, (j["splits"], j["Mpad"], j["Npad"])).astype(f32))
                     for j in case["jobs"]]
    return d


def reduce_ref(job, partial):
    """dW of wgrad_reduce.h: the sum over the splits, mode 0 dW[m Nreal + n], mode 1 (m = o 9 + tap) dW[(o Nreal + n) 9 + tap]"""
    M, Nr = job["Mreal"], job["Nreal"]
    p = partial.astype(f64)[:, :M, :Nr]
    s, mag = p.sum(axis=0), np.abs(p).sum(axis=0)
    if job["mode"] == 1:
        s, mag = (a.reshape(M // 9, 9, Nr).transpose(0, 2, 1) for a in (s, mag))
    return s.reshape(-1), bnd((job["splits"] - 1) * U * mag.reshape(-1))


def mixer_ref(case, d, with_add=True):
    """-> {name: (reference, bound)}: gx (N, C, HW), acc_w (C, C) (matrix only), acc_b, acc_l (C)"""
    N, C, HW, PX = case["N"], case["C"], case["HW"], case["PX"]
    x, gy, b, e = (d[k].astype(f64) for k in ("x", "gy", "bias", "scale"))
    v = (x + b[None, :, None]) * e[None, :, None]
    b_v = 2.0 * U * np.abs(v)
    g, b_g = gy.copy(), np.zeros_like(gy)
    if case["add"] and with_add:
        geo, sc, aC = case_geometry(case), float(d["add_scale"]), case["add"]["C"]
        s, m = gather_ref(geo, d["scratch"])
        g[:, :aC] += sc * s
        b_g[:, :aC] = U * ((3 * geo["MS"] + 2) * abs(sc) * m + np.abs(gy[:, :aC]))
    if case["mode"] == "matrix":
        Wm = d["matrix"].astype(f64)
        gv = np.einsum("oi,nop->nip", Wm, g)
        b_gv = C * U * np.einsum("oi,nop->nip", np.abs(Wm), np.abs(g)) + np.einsum("oi,nop->nip", np.abs(Wm), b_g)
    else:
        idx = d["inv"] if case["mode"] == "gather" else np.arange(C)
        gv, b_gv = g[:, idx], b_g[:, idx]
    gx = gv * e[None, :, None]
    out = dict(gx=(gx, bnd(b_gv * e[None, :, None] + U * np.abs(gx))))
    tb = gx
    out["acc_b"] = (tb.sum(axis=(0, 2)), bnd((b_gv * e[None, :, None]).sum(axis=(0, 2)) + (PX * U + F64) * np.abs(tb).sum(axis=(0, 2))))
    tl = gv * v
    out["acc_l"] = (3.0 * tl.sum(axis=(0, 2)), 3.0 * bnd((b_gv * np.abs(v) + np.abs(gv) * b_v).sum(axis=(0, 2)) + (PX * U + F64) * np.abs(tl).sum(axis=(0, 2))))
    if case["mode"] == "matrix":
        absgv = np.einsum("nop,nip->oi", np.abs(g), np.abs(v))
        out["acc_w"] = (np.einsum("nop,nip->oi", g, v), bnd(np.einsum("nop,nip->oi", b_g, np.abs(v)) + ((PX + 2) * U + F64) * absgv))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# top prior, flipT, logs_from_dw, finalize
# ---------------------------------------------------------------------------------------------------------------------
def prior_cases():
    return [dict(name="prior-per%d-%s%s" % (per, ml, "-gzin" if gz else ""), per=per, N=3, ml=ml, gz_in=gz, families=("random",))
            for per in (48 * 4 * 4, 100) for ml in ("null", "sample", "broadcast") for gz in (False, True)]


def build_prior(case, fam):
    r = rng_of("prior", case["name"], fam)
    N, per = case["N"], case["per"]
    rows = {"null": 0, "sample": N, "broadcast": 1}[case["ml"]]
    return dict(z=r.normal(0.0, 1.5, (N, per)).astype(f32), mean=r.normal(0.0, 1.0, (rows, per)).astype(f32), logs=r.uniform(-2.0, 2.0, (rows, per)).astype(f32),
                gld=gld_random(r, N), gz_in=(r.normal(0.0, 1.0, (N, per)) * 1e-5).astype(f32))


def prior_ref(case, d):
    z, gld, gin = d["z"].astype(f64), d["gld"].astype(f64), d["gz_in"].astype(f64)
    m, l = (d[k].astype(f64) if case["ml"] != "null" else np.zeros((1, case["per"])) for k in ("mean", "logs"))
    g = -gld[:, None] * (z - m) * np.exp(-2.0 * l)
    if not case["gz_in"]:
        return dict(gz=(g, bnd(5.0 * U * np.abs(g))))
    return dict(gz=(g + gin, bnd(U * (6.0 * np.abs(g) + np.abs(gin)))))


FLIP_CASES = ((5, 3, 3), (64, 6, 3), (7, 5, 1))


def flip_ref(w):
    """w (Cout, Cin, k, k) -> wT (Cin, Cout, k, k), taps reversed"""
    Cout, Cin, k, _ = w.shape
    return np.ascontiguousarray(w.reshape(Cout, Cin, k * k)[:, :, ::-1].transpose(1, 0, 2))


LOGS_JOBS = ((7, 54), (96, 512), (512, 4608))


def build_logs(rows, K):
    r = rng_of("logs", rows, K)
    return dict(w=r.normal(0.0, 0.05, (rows, K)).astype(f32), dw=r.normal(0.0, 1e-3, (rows, K)).astype(f32), b=r.normal(0.0, 0.5, rows).astype(f32),
                db=r.normal(0.0, 1e-3, rows))


def logs_ref(d):
    w, dw, b = (d[k].astype(f64) for k in ("w", "dw", "b"))
    ref = 3.0 * ((w * dw).sum(axis=1) + b * d["db"])
    return ref, bnd(U * np.abs(ref) + 3.0 * F64 * (np.abs(w * dw).sum(axis=1) + np.abs(b * d["db"])))


FINALIZE_N = (1, 63, 64, 65, 200)


def finalize_jobs():
    """(the job with out = None sits between two live ones)"""
    return [dict(n=37, C=0, copies=1, stride=0, winv=False, out=True, add_mul=0.0), dict(n=96, C=0, copies=16, stride=100, winv=False, out=True, add_mul=3.0 * 256),
            dict(n=144, C=12, copies=16, stride=144, winv=True, out=True, add_mul=256.0), dict(n=10, C=0, copies=1, stride=0, winv=False, out=False, add_mul=1.0),
            dict(n=2304, C=48, copies=3, stride=2400, winv=True, out=True, add_mul=64.0)]


def build_finalize(N, fam):
    r = rng_of("finalize", N, fam)
    d = dict(jobs=finalize_jobs())
    if fam == "exact":
        d.update(nll=r.integers(1, 8, N).astype(f32) * f32(4.0), inv=2.0 ** -12)      # (one sign: G is not zero)
    else:
        d.update(nll=(r.uniform(0.5, 1.5, N) * r.choice([-1.0, 1.0], N) / N).astype(f32), inv=1.0 / LN2_CHW)
    d["acc"], d["winv"] = [], []
    for j in d["jobs"]:
        n = (j["copies"] - 1) * j["stride"] + j["n"]
        d["acc"].append(ints(r, n, 50).astype(f64) if fam == "exact" else r.normal(0.0, 1e-4, n))
        C = j["C"]
        d["winv"].append(None if not j["winv"] else pow2(r, (C, C), -2, 2, True) if fam == "exact" else np.linalg.qr(r.normal(size=(C, C)))[0].astype(f32))
    return d


def gld_ref(d):
    ref = -d["nll"].astype(f64) * d["inv"]
    return ref, bnd(U * np.abs(ref))


def finalize_ref(d, gld):
    """out of every job from the fp32 gld the first launch stored (the operand k_sum_gld receives) -> [(ref, bound) or None]"""
    G = gld.astype(f64).sum()
    magG = np.abs(gld.astype(f64)).sum()
    res = []
    for j, acc, winv in zip(d["jobs"], d["acc"], d["winv"]):
        if not j["out"]:
            res.append(None)
            continue
        cp = np.stack([acc[k * j["stride"]:k * j["stride"] + j["n"]] for k in range(j["copies"])])
        f = winv.astype(f64).T.reshape(-1) if j["winv"] else np.ones(j["n"])      # out[o C + i] takes winv[i C + o]
        ref = cp.sum(axis=0) + G * j["add_mul"] * f
        res.append((ref, bnd(U * np.abs(ref) + F64 * (np.abs(cp).sum(axis=0) + magG * abs(j["add_mul"]) * np.abs(f)))))
    return res

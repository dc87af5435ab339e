"""Host side of the split-half MFMA kernel tests (numpy only): the SH2 weight images of csrc/pack.hip written out independently, the
fp64 reference of the one-kernel coupling network  h = f.4(relu(f.2(relu(f.0(z1)))))  (csrc/cnet_sh.hip k_cnet, csrc/cnet1w_sh.hip
k_cnet1w), the bound the kernels are held to, the input families, an emulation of the arithmetic csrc/sh.h promises with a switch
for single faults, and the table of kernel instances.  tests/test_gpu_sh2_kernels.py runs the kernels against it through the hook
glowhip_debug_sh2; tests/test_sh2_oracle_host.py checks it on the CPU.

WHAT SH2 PROMISES (csrc/sh.h).  Every operand is multiplied by an exact power of two (weights: per image row, so that the row's
largest |w'| lies in [2^12, 2^13); activations: 2^4) and split  hi = fp16(V), lo = fp16(V - hi):  |V - hi - lo| <= max(2^-22 |V|,
2^-25).  A product is  acc += a.hi*b.hi + a.hi*b.lo + a.lo*b.hi  in ONE fp32 accumulator, every fp16 x fp16 product exact; lo*lo
(<= 2^-22 |a b|) is dropped.

BOUND of one layer with K terms per output (bound_sh2; lu_oracle.apply_bound_sh2 is the K = C case of the same function), u = 2^-24:
    3 * 2^-22 (|W||a|)             the two splits and the dropped lo*lo term;
    3 K * 2^-23 (|W||a| + |b|)     3 K exact products and the bias summed in fp32 in ANY order: a summation tree over n terms has n - 1
                                   additions whatever its shape (the 9-tap sums and the K-split parts of f.4 are part of the tree, so
                                   K = 9 hidden there); 2^-23 per addition also covers an accumulator that truncates;
    2 u (|W||a| + |b|)             the stored weight against its fp64 value, the output rounding;
    3 u (|W||a| + |b|)             only where ActNorm is folded into the image: expf at 2 u and one product rounding (the image bound);
    2^-37 max_k |W_ok| sum_k |a_k| the weights' absolute floor (2^-25 at the row scale); per image row: per (tap, channel) for f.4;
    2^-29 sum_k |W_ok|             the activations' floor (2^-25 at the scale 2^4);
    |W| err(previous layer)        ReLU is 1-Lipschitz.
The fp16 tape adds 2^-11 |v| + 2^-25.  Nothing is fitted to a kernel's output.

FAMILIES.  `random`: weights of the magnitudes glow_oracle.seeded_state_dict draws (0.05 randn), ActNorm logs in +-0.3, biases a few
standard deviations of their sums away from zero, |z1| up to a few units: every output element inside the bound, no outliers.  A lost cross product (relative 2^-12 of one
layer's terms, random sign) is INSIDE that bound -- only inputs on which the promised sum is the true sum can see it.  `exact-w` and
`exact-a` are such inputs, and the kernel must return the fp64 reference value for value:
  (a) every operand times its scale equals hi + lo exactly;  (b) no term has both lo parts non-zero;  (c) sum |terms| of every
  accumulator stays below 2^24 units, so every summation order is exact;  (d) logs = 0, biases integers.
  exact-w: activations fit 11 bits (lo = 0), weights carry lo != 0.  A weight row holds PAIRS (m, T - m) of 13-bit integers, m odd,
           T a 2-bit number, on two inputs that are equal by construction (z1 channels 2i, 2i + 1 equal; rows 2i, 2i + 1 of f.0 and
           f.2 equal), so that every output  sum_pairs T a + b  fits 11 bits again for the next layer.
  exact-a: weights are +-2^j (lo = 0), at most two per accumulator, activations carry lo != 0 (z1 = n / 1024, n up to 15 bits).
  Both: a sixteenth of the rows of f.0 / f.2 are zero with a zero bias (pre-activation exactly 0), signs are random."""
import zlib

import numpy as np

from bwd_oracle import add_geometry, gather_ref, split_scratch, unused_halo_mask  # noqa: F401  (the partial-sum layout: one copy)

f16, f32, f64 = np.float16, np.float32, np.float64
U = 2.0 ** -24
ACT = 16.0
GEMM, FIRST, TAIL = 3, 4, 5           # csrc/kernels.h REPACK_SH2_*
K_CNET, K_CNET1W = 1, 2               # glowhip.h GLOWHIP_S2I_*
ADD_FWD, AFFINE_FWD = 3, 1            # TailMode of csrc/conv_mfma.h (the launcher wants a coupling mode; k_cnet does not read it)
DBG_ROWS_SHIFT, DBG_128_ONLY, DBG_64, DBG_NO_1W, DBG_NO_1W_BWD = 22, 0x2000000, 0x4000000, 0x10000, 0x40000


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def split(V):
    """sh.h sh2_split on fp32 values: (hi, lo) as float16"""
    V = np.asarray(V, f32)
    hi = V.astype(f16)
    return hi, (V - hi.astype(f32)).astype(f16)


def kperm_src(P):
    """sh.h sh2_kperm_src: the original k of image position P"""
    P = np.asarray(P)
    b, s, kl, j = P >> 5, (P >> 4) & 1, (P >> 3) & 1, P & 7
    return 32 * b + 16 * s + 8 * (j >> 2) + 4 * kl + (j & 3)


def g0(Cin):
    return (9 * ((Cin + 7) // 8) + 1) // 2 * 2


def mpad4(Cout):
    return (9 * Cout + 31) // 32 * 32


def groups(Cout):
    if Cout <= 56:
        return 1
    for ng in (2, 3, 4):
        if Cout % ng == 0 and Cout // ng <= 56 and (Cout // ng) % 2 == 0:
            return ng
    return 0


def scratch_floats_plan(N, H, W, Cout):
    """csrc/cnet_sh.hip cnet_scratch_floats: what the plan allocates"""
    return 4 * (N * Cout * H * W + 2 * ((N * H * W + 63) // 64) * Cout * W)


# ---------------------------------------------------------------------------------------------------------------------
# bound
# ---------------------------------------------------------------------------------------------------------------------
def bound_sh2(WA, K, wmax_suma, sumW, bias=0.0, err_prev=0.0, fold=False):
    """elementwise bound of one SH2 layer (module docstring): WA = |W||a|, wmax_suma = max_k|W_ok| sum_k|a_k| (per image row), sumW =
    sum_k|W_ok|, bias = |b|, err_prev = |W| err(previous layer)"""
    rel = 3 * 2.0 ** -22 + 3 * K * 2.0 ** -23 + 2 * 2.0 ** -24
    if fold:
        rel = rel + 3 * U
    return rel * (WA + bias) + 2.0 ** -37 * wmax_suma + 2.0 ** -29 * sumW + err_prev


# ---------------------------------------------------------------------------------------------------------------------
# weight images
# ---------------------------------------------------------------------------------------------------------------------
def flip_t(w):
    """csrc/pack.hip k_flipT_batched: dst[i][o][ks-1-tap] = src[o][i][tap]"""
    w = np.asarray(w)
    if w.ndim == 2:
        return np.ascontiguousarray(w.T)
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def image_rows(kind, w, kperm=False):
    """the image's rows in the image's own k order, before scaling: float array (M, Kp), zero where the image is padding"""
    w = np.asarray(w)
    if kind == GEMM:
        Cout, Cin = w.shape
        return w[:, kperm_src(np.arange(Cin))] if kperm else w.copy()
    Cout, Cin = w.shape[:2]
    w9 = w.reshape(Cout, Cin, 9)
    if kind == FIRST:
        G, nch = g0(Cin), (Cin + 7) // 8
        rows = np.zeros((Cout, G, 8), w.dtype)
        wp = np.zeros((Cout, nch * 8, 9), w.dtype)
        wp[:, :Cin] = w9
        rows[:, :nch * 9] = wp.reshape(Cout, nch, 8, 9).transpose(0, 1, 3, 2).reshape(Cout, nch * 9, 8)      # group = (chunk, tap)
        return rows.reshape(Cout, G * 8)
    M = mpad4(Cout)
    rows = np.zeros((M, Cin), w.dtype)
    rows[:9 * Cout] = w9[:, kperm_src(np.arange(Cin))].transpose(2, 0, 1).reshape(9 * Cout, Cin)             # row = tap * Cout + co
    return rows


def row_exponent(mx):
    """csrc/pack.hip sh2_row_exponent: mx * 2^e in [2^12, 2^13); 0 for an all-zero row"""
    mx = np.asarray(mx, f32)
    _, ex = np.frexp(mx)
    return np.where((mx > 0) & (mx < 3.0e38), np.clip(13 - ex, -100, 100), 0).astype(np.int64)


def image_ref(kind, w, kperm=False, fold_bias=None, fold_logs=None, transposed=False):
    """the bytes csrc/pack.hip writes for one image, from the fp32 operands with numpy's exp for the fold (bitwise the kernel's only
    where logs = 0 or there is no fold): dict(hi, lo (2 Kp/8, M, 8 as two planes), rowscale, bias, e, rows32 = the folded fp32 rows)"""
    w = np.asarray(w, f32)
    if transposed:
        w = flip_t(w)
    rows = image_rows(kind, w, kperm or kind == TAIL)
    M, Kp = rows.shape
    fold = np.ones(M, f32)
    if fold_logs is not None and kind != TAIL:
        fold = np.exp((np.asarray(fold_logs, f32) * f32(3.0)).astype(f64)).astype(f32)
    rows32 = (rows * fold[:, None]).astype(f32)
    e = row_exponent(np.abs(rows32).max(axis=1))
    hi, lo = split(rows32 * np.exp2(e).astype(f32)[:, None])
    lay = lambda p: np.ascontiguousarray(p.reshape(M, Kp // 8, 8).transpose(1, 0, 2))      # [Kp/8][M][8]
    rowscale = np.exp2(-e).astype(f32) * (f32(1.0 / ACT) if kind == TAIL else f32(1.0))
    bias = np.zeros(M, f32)
    if fold_bias is not None and kind != TAIL:
        bias = ((np.asarray(fold_bias, f32) * fold).astype(f32) * f32(ACT)).astype(f32)
    return dict(hi=lay(hi), lo=lay(lo), rowscale=rowscale, bias=bias, e=e, rows32=rows32, M=M, Kp=Kp)


def image_bytes(img):
    return img["hi"].tobytes() + img["lo"].tobytes() + img["rowscale"].tobytes() + img["bias"].tobytes()


def image_decode(buf, M, Kp):
    """device bytes -> (hi, lo as (M, Kp) float16 in the image's k order, rowscale, bias)"""
    h = np.frombuffer(buf[:4 * Kp * M], f16).reshape(2, Kp // 8, M, 8)
    t = np.frombuffer(buf[4 * Kp * M:4 * Kp * M + 8 * M], f32)
    plane = lambda p: p.transpose(1, 0, 2).reshape(M, Kp)
    return plane(h[0]), plane(h[1]), t[:M].copy(), t[M:].copy()


def image_fold_check(kind, buf, w, kperm, fold_bias, fold_logs, transposed=False):
    """a folded image against fp64 w e^{3 logs}: -> (worst multiple of the bound, padding exactly zero, exponents in range).  Bound per
    element (3 u)|w'| + max(2^-22 |V|, 2^-25) 2^-e: expf at 2 u, one product rounding, then the split as sh.h states it."""
    w = np.asarray(w, f32)
    if transposed:
        w = flip_t(w)
    rows = image_rows(kind, w.astype(f64), kperm or kind == TAIL)
    real = image_rows(kind, np.ones(w.shape, f64), kperm or kind == TAIL) != 0
    M, Kp = rows.shape
    hi, lo, rs, bias = image_decode(buf, M, Kp)
    fold = np.exp(3.0 * np.asarray(fold_logs, f64)) if fold_logs is not None and kind != TAIL else np.ones(M)
    want = rows * fold[:, None]
    unit = rs.astype(f64) * (ACT if kind == TAIL else 1.0)       # 2^-e
    dec = (hi.astype(f64) + lo.astype(f64)) * unit[:, None]
    V = np.abs(want) / unit[:, None]
    bnd = 3 * U * np.abs(want) + np.maximum(2.0 ** -22 * V, 2.0 ** -25) * unit[:, None]
    worst = float(np.max(np.abs(dec - want)[real] / bnd[real]))
    pad_zero = bool((hi[~real].view(np.uint16) == 0).all() and (lo[~real].view(np.uint16) == 0).all())
    mx = (np.abs(hi.astype(f64) + lo.astype(f64))).max(axis=1)
    nz = np.abs(want).max(axis=1) > 0
    in_range = bool(((mx[nz] >= 2.0 ** 12 * (1 - 2.0 ** -10)) & (mx[nz] <= 2.0 ** 13)).all()) and bool((np.log2(unit) % 1 == 0).all())
    if fold_bias is not None and kind != TAIL:
        bw = np.asarray(fold_bias, f64) * fold * ACT
        worst = max(worst, float(np.max(np.abs(bias.astype(f64) - bw) / (4 * U * np.abs(bw) + 2.0 ** -140))))
    else:
        pad_zero = pad_zero and not bias.any()
    return worst, pad_zero, in_range


# ---------------------------------------------------------------------------------------------------------------------
# the network in fp64
# ---------------------------------------------------------------------------------------------------------------------
def conv3(x, w):
    """zero-padded 3x3 convolution: x (N, C, H, W), w (O, C, 3, 3) -> (N, O, H, W), float64"""
    N, C, H, W = x.shape
    xp = np.zeros((N, C, H + 2, W + 2), f64)
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((N, w.shape[0], H, W), f64)
    for dy in range(3):
        for dx in range(3):
            out += np.einsum("oc,nchw->nohw", w[:, :, dy, dx].astype(f64), xp[:, :, dy:dy + H, dx:dx + W])
    return out


def conv1(x, w):
    return np.einsum("oc,nchw->nohw", w.astype(f64), x)


def folded(d):
    """fp64 folded weights and biases of f.0 / f.2: W' = W e^{3 logs}, b' = b e^{3 logs}"""
    e0, e2 = np.exp(3.0 * d["l0"].astype(f64)), np.exp(3.0 * d["l2"].astype(f64))
    return (d["w0"].astype(f64) * e0[:, None, None, None], d["b0"].astype(f64) * e0, d["w2"].astype(f64) * e2[:, None], d["b2"].astype(f64) * e2)


def reference(d):
    """-> dict of (value, bound) pairs in fp64: t1, t2 (pre-activations), h1, h2, out (= f.4 without bias: what the partial sums
    add up to).  The bound is bound_sh2 layer by layer.  With d["mk1"] / d["mk2"] (bool (hidden, P)) the two ReLUs are replaced by
    those masks: the input-gradient chain of MODE 2, g_u = g_h (h > 0) e^{3 logs}, on the transposed, flipped weights -- the same
    network shape (z1 = d L / d(f.4 output), w0 = flip_t(W4) with f.2's logs, w2 = W2^T with f.0's logs, w4 = flip_t(W0), no biases)"""
    z = d["z1"].astype(f64)
    w0, b0, w2, b2 = folded(d)
    w4 = d["w4"].astype(f64)
    fold = bool(d["l0"].any() or d["l2"].any())
    hid, Cin = w0.shape[:2]
    one = lambda c: np.ones((1, c, 3, 3))
    az = np.abs(z)
    t1 = conv3(z, w0) + b0[None, :, None, None]
    e1 = bound_sh2(conv3(az, np.abs(w0)), 9 * Cin, np.abs(w0).max(axis=(1, 2, 3))[None, :, None, None] * conv3(az, one(Cin)),
                   conv3(np.ones_like(z), np.abs(w0)), np.abs(b0)[None, :, None, None], 0.0, fold)
    N, _, H, W = z.shape
    unpx = lambda m: m.reshape(hid, N, H, W).transpose(1, 0, 2, 3)      # (hid, P) -> (N, hid, H, W)
    h1 = t1 * unpx(d["mk1"]) if "mk1" in d else np.maximum(t1, 0)
    if "mk1" in d:
        e1 = e1 * unpx(d["mk1"])
    t2 = conv1(h1, w2) + b2[None, :, None, None]
    e2 = bound_sh2(conv1(np.abs(h1), np.abs(w2)), hid, np.abs(w2).max(axis=1)[None, :, None, None] * np.abs(h1).sum(axis=1, keepdims=True),
                   np.abs(w2).sum(axis=1)[None, :, None, None], np.abs(b2)[None, :, None, None], conv1(e1, np.abs(w2)), fold)
    h2 = t2 * unpx(d["mk2"]) if "mk2" in d else np.maximum(t2, 0)
    if "mk2" in d:
        e2 = e2 * unpx(d["mk2"])
    out = conv3(h2, w4)
    wmax4 = np.abs(w4).max(axis=1, keepdims=True)                 # per (channel, tap) image row
    e4 = bound_sh2(conv3(np.abs(h2), np.abs(w4)), 9 * hid, conv3(np.abs(h2).sum(axis=1, keepdims=True), wmax4), conv3(np.ones_like(h2), np.abs(w4)),
                   0.0, conv3(e2, np.abs(w4)), False)
    return dict(t1=(t1, e1), t2=(t2, e2), h1=(h1, e1), h2=(h2, e2), out=(out, e4))


def tape_bound(v, err):
    """an activation stored as fp16: the value's own bound, the fp16 rounding of what was computed, fp16's fixed spacing"""
    return err + 2.0 ** -11 * (np.abs(v) + err) + 2.0 ** -25


# ---------------------------------------------------------------------------------------------------------------------
# tape and sign words (layouts of the header comment of k_cnet)
# ---------------------------------------------------------------------------------------------------------------------
def to_px(t):
    """(N, C, H, W) -> (C, P) over the batch's pixels"""
    N, C = t.shape[:2]
    return t.reshape(N, C, -1).transpose(1, 0, 2).reshape(C, -1)


def tape_decode(buf, hid, P):
    """pixel-tile-major [pixel / 32][hidden][pixel % 32] -> (hidden, P)"""
    return np.asarray(buf).reshape(P // 32, hid, 32).transpose(1, 0, 2).reshape(hid, P)


def tape_encode(v):
    hid, P = v.shape
    return np.ascontiguousarray(v.reshape(hid, P // 32, 32).transpose(1, 0, 2)).reshape(-1)


MASK_ROW = np.array([8 * (k // 4) + k % 4 for k in range(16)])      # register k of lane group kl holds row 8 (k / 4) + 4 kl + k % 4


def mask_decode(words, hid, P):
    """mask[(row tile * P + pixel) * 2 + kl], register k in bit 15 - k -> bool (hidden, P)"""
    w = np.asarray(words, np.uint16).reshape(hid // 32, P, 2)
    bits = np.zeros((hid, P), bool)
    for kl in range(2):
        for k in range(16):
            bits[np.arange(hid // 32) * 32 + MASK_ROW[k] + 4 * kl] = (w[:, :, kl] >> (15 - k)) & 1
    return bits


def mask_encode(bits):
    hid, P = bits.shape
    w = np.zeros((hid // 32, P, 2), np.uint16)
    for kl in range(2):
        for k in range(16):
            w[:, :, kl] |= bits[np.arange(hid // 32) * 32 + MASK_ROW[k] + 4 * kl].astype(np.uint16) << (15 - k)
    return w.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("exact-w", "exact-a", "random")
PAIR_TOTALS = (8192, 12288, 10240, 6144)      # 2-bit numbers: T a keeps the bits of a


def _pairs_row(r, nslots, npairs):
    """exact-w: values for 2 * nslots inputs (slot s = inputs 2 s, 2 s + 1, equal by construction): npairs pairs (m, T - m) * sign"""
    row = np.zeros(2 * nslots)
    for s in r.choice(nslots, size=min(npairs, nslots), replace=False):
        while True:
            m, T = 2 * int(r.integers(2048, 4096)) + 1, int(r.choice(PAIR_TOTALS))
            if 0 < T - m < 8192:
                break
        sg = r.choice([-1.0, 1.0])
        row[2 * s], row[2 * s + 1] = (sg * m, sg * (T - m)) if r.integers(2) else (sg * (T - m), sg * m)
    return row


def build(c, fam):
    """the operands of case c: z1 (N, Cin, H, W), w0 (hid, Cin, 3, 3), b0, l0, w2 (hid, hid), b2, l2, w4 (Cout, hid, 3, 3); fp32"""
    N, Cin, H, W, hid, Cout = (c[k] for k in ("N", "Cin", "H", "W", "hid", "Cout"))
    r = rng_of("sh2", c.get("data", c["name"]), fam)      # (data: cases that share their operands)
    if c.get("bwd"):
        return _with_masks(c, fam, r, build(dict(c, bwd=False), fam))
    zero = lambda n: np.zeros(n, f32)
    if fam == "random":
        # biases away from zero: minus the row's mean, plus or minus 2.5 to 4 standard deviations of the sum they are added to (both from
        # an fp64 evaluation of the drawn operands).  A pre-activation is then rarely closer to zero than its bound -- the sign bits
        # that cannot be compared stay below 0.1 % -- and both sides of each ReLU stay populated
        d = dict(z1=(r.standard_normal((N, Cin, H, W)) * 1.5).astype(f32), w0=(0.05 * r.standard_normal((hid, Cin, 3, 3))).astype(f32),
                 l0=r.uniform(-0.3, 0.3, hid).astype(f32), w2=(0.05 * r.standard_normal((hid, hid))).astype(f32),
                 l2=r.uniform(-0.3, 0.3, hid).astype(f32), w4=(0.05 * r.standard_normal((Cout, hid, 3, 3))).astype(f32))
        away = lambda x: (-x.mean(axis=(0, 2, 3)) + r.uniform(2.5, 4.0, hid) * r.choice([-1.0, 1.0], hid) * x.std(axis=(0, 2, 3))).astype(f32)
        x1 = conv3(d["z1"].astype(f64), d["w0"])
        d["b0"] = away(x1)
        h1 = np.maximum((x1 + d["b0"].astype(f64)[None, :, None, None]) * np.exp(3.0 * d["l0"].astype(f64))[None, :, None, None], 0)
        d["b2"] = away(conv1(h1, d["w2"]))
        return d
    dead = (np.arange(hid) % 16) >= 14          # rows with a pre-activation of exactly 0 (pairs 14, 15 of every 16)
    if fam == "exact-w":
        assert Cin % 2 == 0 and hid % 2 == 0
        half = r.integers(-2, 3, (N, Cin // 2, H, W))
        z1 = np.repeat(half, 2, axis=1).astype(f32)                  # channels 2 i and 2 i + 1 equal
        w0 = np.zeros((hid, Cin, 9))
        w2 = np.zeros((hid, hid))
        for o in range(0, hid, 2):
            if dead[o]:
                continue
            row = _pairs_row(r, (Cin // 2) * 9, 3).reshape(Cin // 2, 9, 2)       # slot = (channel pair, tap)
            w0[o] = w0[o + 1] = row.transpose(0, 2, 1).reshape(Cin, 9) * 2.0 ** -13
            w2[o] = w2[o + 1] = _pairs_row(r, hid // 2, 2) * 2.0 ** -13
        w4 = np.zeros((Cout, hid, 9))
        for co in range(Cout):
            for tap in range(9):
                w4[co, :, tap] = _pairs_row(r, hid // 2, 1) * 2.0 ** -13
        b0 = np.repeat(r.integers(-2, 3, hid // 2), 2) * ~dead
        b2 = np.repeat(r.integers(-2, 3, hid // 2), 2) * ~dead
        return dict(z1=z1, w0=w0.reshape(hid, Cin, 3, 3).astype(f32), b0=b0.astype(f32), l0=zero(hid), w2=w2.astype(f32), b2=b2.astype(f32),
                    l2=zero(hid), w4=w4.reshape(Cout, hid, 3, 3).astype(f32))
    assert fam == "exact-a"
    z1 = ((2 * r.integers(2048, 16384, (N, Cin, H, W)) + 1) * r.choice([-1.0, 1.0], (N, Cin, H, W)) / 1024.0).astype(f32)
    pm = lambda n: r.choice([-1.0, 1.0], n)
    w0 = np.zeros((hid, Cin * 9))
    w2 = np.zeros((hid, hid))
    for o in range(hid):
        if dead[o]:
            continue
        w0[o, r.choice(Cin * 9, 2, replace=False)] = pm(2) * 2.0 ** r.integers(-2, 1)
        w2[o, r.choice(hid, 2, replace=False)] = pm(2) * 2.0 ** r.integers(-2, 1)
    w4 = np.zeros((Cout, hid, 9))
    for co in range(Cout):
        for tap in r.choice(9, 2, replace=False):
            w4[co, r.integers(hid), tap] = pm(1)[0] * 2.0 ** r.integers(-1, 1)
    return dict(z1=z1, w0=w0.reshape(hid, Cin, 3, 3).astype(f32), b0=(r.integers(-3, 4, hid) * ~dead).astype(f32), l0=zero(hid), w2=w2.astype(f32),
                b2=(r.integers(-3, 4, hid) * ~dead).astype(f32), l2=zero(hid), w4=w4.reshape(Cout, hid, 3, 3).astype(f32))


def _with_masks(c, fam, r, d):
    """MODE 2 operands from a forward set: no biases; sign words laid out here -- random bits (exact-w: rows 2 i, 2 i + 1 alike, which
    keeps its paired inputs equal), and per (row tile, pixel, lane group) word one in eight all ones and one in eight all zeros"""
    hid, P = c["hid"], c["N"] * c["H"] * c["W"]
    d = dict(d, b0=np.zeros(hid, f32), b2=np.zeros(hid, f32))
    for k in ("mk1", "mk2"):
        bits = r.integers(0, 2, (hid // 2, P)).repeat(2, axis=0).astype(bool) if fam == "exact-w" else r.integers(0, 2, (hid, P)).astype(bool)
        words = mask_encode(bits).reshape(hid // 32, P, 2)
        kind = r.integers(0, 8, words.shape)
        words[kind == 0], words[kind == 1] = 0xFFFF, 0
        d[k] = mask_decode(words.reshape(-1), hid, P)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# emulation of the promised arithmetic, with single faults
# ---------------------------------------------------------------------------------------------------------------------
FAULTS_PRODUCT = tuple("drop:%s:%s" % (layer, p) for layer in ("f0", "f2", "f4") for p in ("hh", "hl", "lh"))
FAULTS_LAYOUT = ("lo_as_hi", "kgroup_swapped", "taps_flipped", "halo_wrong_neighbour", "ms_misstrided", "sign_word_reversed", "tape_row_next_tile")
FAULTS = FAULTS_PRODUCT + FAULTS_LAYOUT


def im2col(x):
    """(N, C, H, W) fp32 -> (C * 9, P) with k = c * 9 + tap, zero padded"""
    N, C, H, W = x.shape
    xp = np.zeros((N, C, H + 2, W + 2), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    cols = np.stack([xp[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=2)      # (N, C, 9, H, W)
    return cols.transpose(1, 2, 0, 3, 4).reshape(C * 9, N * H * W)


def _wsplit(rows32):
    """a weight matrix (M, K) fp32 (already folded) -> hi, lo at the row scale, and 2^-e"""
    e = row_exponent(np.abs(rows32).max(axis=1))
    hi, lo = split(rows32 * np.exp2(e).astype(f32)[:, None])
    return hi.astype(f32), lo.astype(f32), np.exp2(-e)


def _mm(A, B):
    return (A.astype(f64) @ B.astype(f64)).astype(f32)      # the products are exact; one fp32 rounding of the sum stands in for the pipe's order


def _layer(rows32, act16, layer, fault, ks=slice(None)):
    """acc = A.hi B.hi + A.hi B.lo + A.lo B.hi in fp32 over the k range ks of the image rows, the row scale undone (exact)"""
    ahi, alo, unit = _wsplit(rows32)
    ahi, alo = ahi[:, ks], alo[:, ks]
    bhi, blo = (p.astype(f32) for p in split(act16))
    if fault == "lo_as_hi" and layer == "f2":
        alo = ahi
    keep = lambda p: fault != "drop:%s:%s" % (layer, p)
    acc = np.zeros((rows32.shape[0], act16.shape[1]), f32)
    for on, A, B in ((keep("hh"), ahi, bhi), (keep("hl"), ahi, blo), (keep("lh"), alo, bhi)):
        if on:
            acc = (acc + _mm(A, B)).astype(f32)
    return acc.astype(f64) * unit[:, None]


def emulate(c, d, geo=None, fault=None):
    """the kernel's arithmetic in numpy -> dict(t1, t2 (fp32 pre-activations, (hid, P)), out (N, Cout, H, W) from the partial sums the
    emulated P4 laid out, scratch, tape1, tape2 (fp16, pixel-tile-major), mask1, mask2 (sign words)).  geo: bwd_oracle.add_geometry."""
    N, Cin, H, W, hid, Cout = (c[k] for k in ("N", "Cin", "H", "W", "hid", "Cout"))
    P = N * H * W
    fold0 = np.exp((d["l0"] * f32(3.0)).astype(f64)).astype(f32)
    fold2 = np.exp((d["l2"] * f32(3.0)).astype(f64)).astype(f32)
    w0 = (d["w0"].reshape(hid, Cin * 9) * fold0[:, None]).astype(f32)
    if fault == "taps_flipped":
        w0 = w0.reshape(hid, Cin, 9)[:, :, ::-1].reshape(hid, Cin * 9)
    w2 = (d["w2"] * fold2[:, None]).astype(f32)
    if fault == "kgroup_swapped":                  # two 8-wide groups of a 32-k block change places in the image, not in the activations
        w2 = w2.copy()
        w2[:, 0:8], w2[:, 8:16] = w2[:, 8:16].copy(), w2[:, 0:8].copy()
    b0 = (d["b0"] * fold0).astype(f32).astype(f64)
    b2 = (d["b2"] * fold2).astype(f32).astype(f64)
    t1 = (_layer(w0, im2col((d["z1"] * f32(ACT)).astype(f32)), "f0", fault) / ACT + b0[:, None]).astype(f32)
    h1 = np.maximum(t1, 0)
    t2 = (_layer(w2, (h1 * f32(ACT)).astype(f32), "f2", fault) / ACT + b2[:, None]).astype(f32)
    h2 = np.maximum(t2, 0)
    # f.4 with the taps on the output side: T[tap][co] = W4[co][:, tap] h2, one image row (and exponent) per (tap, co)
    w4 = d["w4"].reshape(Cout, hid, 9).transpose(2, 0, 1).reshape(9 * Cout, hid)
    MS = geo["MS"] if geo else 1
    mr = hid // MS
    T = [(_layer(w4, (h2[m * mr:(m + 1) * mr] * f32(ACT)).astype(f32), "f4", fault, slice(m * mr, (m + 1) * mr)) / ACT).astype(f32)
         .reshape(9, Cout, N, H, W) for m in range(MS)]
    res = dict(t1=t1, t2=t2)
    if geo:
        res["scratch"] = lay_partial_sums(geo, T, fault)
        res["out"] = gather_ref(geo, res["scratch"])[0].reshape(N, Cout, H, W)
    else:
        res["out"] = tap_sums(T[0], 0, H).transpose(1, 0, 2, 3)
    if P % 32 == 0:
        for name, t, h in (("1", t1, h1), ("2", t2, h2)):
            tp = tape_encode(h.astype(f16))
            bits = t > 0
            if fault == "tape_row_next_tile" and name == "1":
                tp = tp.reshape(P // 32, hid, 32).copy()
                row = int(np.argmax(h.sum(axis=1)))          # (a row that is alive)
                tp[0, row], tp[1, row] = tp[1, row].copy(), tp[0, row].copy()
                tp = tp.reshape(-1)
            words = mask_encode(bits)
            if fault == "sign_word_reversed" and name == "2":
                words = words.copy()
                words[0] = int("{:016b}".format(int(words[0]))[::-1], 2)
            res["tape" + name], res["mask" + name] = tp, words
    return res


def tap_sums(T, y0, y1, rows=None):
    """out[co][n][y][x] for image rows [y0, y1) from the T values of source rows `rows` (default the same range): fp32 sums"""
    _, Cout, N, H, W = T.shape
    lo, hi = (y0, y1) if rows is None else rows
    Tp = np.zeros((9, Cout, N, H + 2, W + 2), f32)
    Tp[:, :, :, 1 + lo:1 + hi, 1:-1] = T[:, :, :, lo:hi]
    out = np.zeros((Cout, N, y1 - y0, W), f32)
    for dy in range(3):
        for dx in range(3):
            out = (out + Tp[dy * 3 + dx, :, :, y0 + dy:y1 + dy, dx:dx + W]).astype(f32)
    return out


def lay_partial_sums(geo, T, fault=None):
    """P4 of k_cnet: per row-split copy and tile, the tile's own rows from the tile's own T rows -> hpart; what its first / last row
    gives to the image row just outside -> hup / hdn of THAT tile.  Unwritten slots hold NaN."""
    N, H, W, R, NI, MS, Cout, HW = (geo[k] for k in ("N", "H", "W", "R", "NI", "MS", "Cout", "HW"))
    scratch = np.full(geo["floats"], np.nan, f32)
    hpart, hup, hdn = split_scratch(geo, scratch)
    for m in range(MS):
        for n in range(N):
            for y0 in range(0, H, R if NI == 1 else H):
                y1 = min(y0 + R, H) if NI == 1 else H
                hpart[m, n].reshape(Cout, H, W)[:, y0:y1] = tap_sums(T[m][:, :, n:n + 1], y0, y1)[:, 0]
                if geo["halos"]:
                    t = (n * HW + y0 * W) >> geo["lpxt"]
                    up, dn = (hdn, hup) if fault == "halo_wrong_neighbour" else (hup, hdn)
                    if y0 > 0:
                        up[m, t] = tap_sums(T[m][:, :, n:n + 1], y0 - 1, y0, rows=(y0, y0 + 1))[:, 0, 0]
                    if y1 < H:
                        dn[m, t] = tap_sums(T[m][:, :, n:n + 1], y1, y1 + 1, rows=(y1 - 1, y1))[:, 0, 0]
    if fault == "ms_misstrided" and MS > 1:            # the copies one image row short of their stride
        good = hpart.copy()
        flat = hpart.reshape(-1)
        flat[:] = np.nan
        for m in range(MS):
            o = m * (N * Cout * HW - W)
            flat[o:o + N * Cout * HW] = good[m].reshape(-1)
    return scratch


# ---------------------------------------------------------------------------------------------------------------------
# conditions (a) .. (d) of the exact families
# ---------------------------------------------------------------------------------------------------------------------
def _lsb(x):
    """the power of two of the lowest set bit over all non-zero values of x (float64, exact binary fractions)"""
    x = np.abs(np.asarray(x, f64))
    x = x[x > 0]
    if x.size == 0:
        return 1.0
    m, e = np.frexp(x)
    n = (m * 2.0 ** 53).astype(np.int64)
    return float(2.0 ** (e - 53 + np.log2((n & -n).astype(f64))).min())


def check_exact(c, d, fam):
    """asserts (a) .. (d) for every layer of an exact case; -> the fp64 reference values (t1, t2, out)"""
    N, Cin, H, W, hid, Cout = (c[k] for k in ("N", "Cin", "H", "W", "hid", "Cout"))
    assert not d["l0"].any() and not d["l2"].any() and (d["b0"] == np.round(d["b0"])).all() and (d["b2"] == np.round(d["b2"])).all(), "(d)"
    ref = reference(d)
    acts = dict(f0=im2col(d["z1"].astype(f64) * ACT), f2=to_px(ref["h1"][0]) * ACT, f4=to_px(ref["h2"][0]) * ACT)
    wts = dict(f0=d["w0"].reshape(hid, Cin * 9), f2=d["w2"], f4=d["w4"].reshape(Cout, hid, 9).transpose(2, 0, 1).reshape(9 * Cout, hid))
    for layer in ("f0", "f2", "f4"):
        ahi, alo, unit = _wsplit(wts[layer].astype(f32))
        V = wts[layer].astype(f64) / unit[:, None]
        assert (ahi.astype(f64) + alo.astype(f64) == V).all(), (layer, "(a) weights")
        A = acts[layer]
        assert (A.astype(f32).astype(f64) == A).all(), (layer, "the activation is no fp32 number")
        bhi, blo = (p.astype(f64) for p in split(A.astype(f32)))
        assert np.isfinite(bhi).all() and (bhi + blo == A).all(), (layer, "(a) activations")
        assert not (np.abs(alo) @ np.abs(blo)).any(), (layer, "(b) a term has both lo parts")
        if fam == "exact-w":
            assert not blo.any() and alo.any(), (layer, "exact-w: activation lo = 0, weight lo != 0")
        else:
            assert not alo.any() and blo.any(), (layer, "exact-a: weight lo = 0, activation lo != 0")
        # (c) per accumulator: sum |terms| < 2^24 units, the unit = the lowest bit any term of the row can set
        sa = np.abs(ahi) + np.abs(alo)
        sums = sa.astype(f64) @ (np.abs(bhi) + np.abs(blo))
        units = np.array([_lsb(np.concatenate([ahi[r][ahi[r] != 0], alo[r][alo[r] != 0]])) for r in range(sa.shape[0])]) * _lsb(np.concatenate([bhi.ravel(), blo.ravel()]))
        assert (sums < 2.0 ** 24 * units[:, None]).all(), (layer, "(c)", float((sums / units[:, None]).max()))
    # the epilogues and the tap sums: every value an fp32 number with room to spare
    for k in ("t1", "t2", "out"):
        v = ref[k][0]
        assert (v.astype(f32).astype(f64) == v).all(), (k, "no fp32 number")
    mag9 = conv3(ref["h2"][0], np.abs(d["w4"]))                 # the 9-tap sums (and the K-split parts) in the unit of the T values
    assert (mag9 < 2.0 ** 24 * _lsb(ref["h2"][0]) * _lsb(d["w4"])).all(), "(c) 9-tap sums"
    for k in ("t1", "t2"):
        v = ref[k][0]
        assert "mk1" in d or ((v == 0).mean() > 0.01 and (v < 0).mean() > 0.05 and (v > 0).mean() > 0.05), (k, "both sides of ReLU and exact zeros")
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# cases: one per kernel instance (csrc/cnet_sh.hip launch_cnet_main, csrc/cnet1w_sh.hip launch_cnet1w)
# ---------------------------------------------------------------------------------------------------------------------
def _c(hid, ms, upw, pxt, ng, N, H, W, Cin, Cout, tape=False, flags=0, one_wave=False, bs_extra=0, **kw):
    if kw.pop("twin", False):
        kw.update(twin=True, data="twin-bwd" if kw.get("bwd") else "twin")
    rows = ms
    fl = flags | (rows << DBG_ROWS_SHIFT) | (DBG_128_ONLY if pxt == 128 else DBG_64)
    bwd = kw.get("bwd", False)
    mode = 2 if bwd else (1 if tape else 0)
    inst = (K_CNET1W, 512, 1, 0, 128, 1, mode) if one_wave else (K_CNET, hid, ms, upw, pxt, ng, mode)
    name = "%s<%d,ms%d,u%d,px%d,ng%d,mode%d> %dx%dx%d C%d->%d%s" % ("k_cnet1w" if one_wave else "k_cnet", hid, ms, upw, pxt, ng, mode, N, H, W, Cin, Cout,
                                                                   kw.pop("tag", ""))
    kw.setdefault("bwd", False)
    return dict(name=name, hid=hid, N=N, H=H, W=W, Cin=Cin, Cout=Cout, tape=tape and not bwd, flags=fl, inst=inst, bs_extra=bs_extra, **kw)


# the maps: (N, H, W) by tile size -- whole images per tile and a ragged last tile (8x8 N = 3); halo rows both ways at R = 8 and
# R = 4 (16x16); R = 1, a tile's single row both its first and its last (4x128 / 4x64); non-square with the minimum W (64x4), 4x32
MAPS = {128: ((3, 8, 8), (1, 16, 16), (2, 16, 16), (1, 4, 128), (1, 64, 4), (2, 4, 32)),
        64: ((3, 8, 8), (1, 16, 16), (2, 16, 16), (1, 4, 64), (1, 64, 4), (2, 4, 32))}
FWD_128 = ((512, 1), (512, 2), (512, 4), (256, 1), (256, 2), (256, 4), (128, 1), (128, 2), (64, 1))
FWD_128_U2 = ((512, 2), (512, 4), (256, 1), (256, 2), (256, 4), (128, 1), (128, 2), (64, 1))
FWD_64 = ((512, 1), (512, 2), (512, 4), (256, 1), (256, 2), (128, 1))
TAPE = ((512, 1, 128), (512, 2, 128), (512, 4, 128), (512, 1, 64), (512, 2, 64), (512, 4, 64), (256, 1, 128), (256, 2, 128), (256, 1, 64),
        (256, 2, 64), (128, 1, 128), (128, 1, 64))
CHANNELS = ((6, 6), (6, 12), (12, 12), (12, 24), (24, 24), (24, 35))       # (Cin, Cout): additive, affine, and a 9 Cout that is no multiple of 32


def cnet_cases():
    out, i = [], 0

    def nxt(pxt, wide=False):
        nonlocal i
        i += 1
        m = MAPS[pxt][i % 6]
        ch = CHANNELS[i % 6]
        if m[2] >= 64:                       # (the window of a 64- / 128-wide row with more than one channel chunk does not fit the LDS)
            ch = CHANNELS[i % 2]
        if pxt == 128 and ch[1] == 35 and m[1] * m[2] > 64:      # (128 pixels x 9 x 35 rows of T do not fit one staging pass)
            ch = (24, 24)
        return m, ch

    for hid, ms in FWD_128:
        (N, H, W), (Cin, Cout) = nxt(128)
        out.append(_c(hid, ms, 1, 128, 1, N, H, W, Cin, Cout, flags=DBG_NO_1W, bs_extra=8 * (i % 2)))
    for hid, ms in FWD_128_U2:               # Cout = 48: fourteen row tiles of T, two units per wave
        i += 1                               # (their T is staged in two passes, which whole 8x8 images per tile alone allow)
        out.append(_c(hid, ms, 2, 128, 1, (3, 2, 5)[i % 3], 8, 8, 24, 48))
    for hid, ms in FWD_64:
        (N, H, W), (Cin, Cout) = nxt(64)
        out.append(_c(hid, ms, 1, 64, 1, N, H, W, Cin, Cout, bs_extra=8 * (i % 2)))
    for hid, ms in FWD_64:                   # Cout = 96 = 2 x 48: two groups of f.4 output channels
        (N, H, W), _ = nxt(64)
        if W >= 64:
            N, H, W = 1, 16, 16
        out.append(_c(hid, ms, 1, 64, 2, N, H, W, 48, 96))
    for hid, ms, pxt in TAPE:
        (N, H, W), (Cin, Cout) = nxt(pxt)
        if Cout == 35:
            Cin, Cout = 12, 24
        out.append(_c(hid, ms, 1, pxt, 1, N, H, W, Cin, Cout, tape=True, flags=DBG_NO_1W))
    for hid, ms, pxt in TAPE:                # the backward launch: f.4's Cout channels in, C / 2 out
        (N, H, W), (Cout, Cin) = nxt(pxt)
        if Cin == 35:
            Cin, Cout = 24, 12
        if W >= 64:
            Cin, Cout = 6, 6
        out.append(_c(hid, ms, 1, pxt, 1, N, H, W, Cin, Cout, bwd=True, flags=DBG_NO_1W))
    out.append(_c(512, 1, 0, 128, 1, 1, 16, 16, 12, 6, one_wave=True, bwd=True, twin=True))
    out.append(_c(512, 1, 1, 128, 1, 1, 16, 16, 12, 6, bwd=True, flags=DBG_NO_1W_BWD, tag=" (k_cnet1w's shape)", twin=True))
    # k_cnet1w (one wave per SIMD): forward and taping at Cin = 6, Cout = 12, hidden 512 on 16x16, and the same launches on k_cnet
    out.append(_c(512, 1, 0, 128, 1, 1, 16, 16, 6, 12, one_wave=True, twin=True))
    out.append(_c(512, 1, 1, 128, 1, 1, 16, 16, 6, 12, flags=DBG_NO_1W, tag=" (k_cnet1w's shape)", twin=True))
    out.append(_c(512, 1, 0, 128, 1, 1, 16, 16, 6, 12, one_wave=True, tape=True, twin=True))
    out.append(_c(512, 1, 1, 128, 1, 1, 16, 16, 6, 12, tape=True, flags=DBG_NO_1W, tag=" (k_cnet1w's shape)", twin=True))
    return out


# every instance the two launchers instantiate: forward / inverse (mode 0), taping (mode 1) and backward (mode 2) launches
EXPECTED_INSTANCES = sorted({(K_CNET, h, m, 1, 128, 1, 0) for h, m in FWD_128} | {(K_CNET, h, m, 2, 128, 1, 0) for h, m in FWD_128_U2} |
                            {(K_CNET, h, m, 1, 64, 1, 0) for h, m in FWD_64} | {(K_CNET, h, m, 1, 64, 2, 0) for h, m in FWD_64} |
                            {(K_CNET, h, m, 1, p, 1, md) for h, m, p in TAPE for md in (1, 2)} | {(K_CNET1W, 512, 1, 0, 128, 1, md) for md in (0, 1, 2)})

REFUSALS = (dict(name="W no power of two", N=1, H=8, W=12, Cin=6, Cout=6, hid=128), dict(name="hidden 96", N=1, H=8, W=8, Cin=6, Cout=6, hid=96),
            dict(name="HW < 64", N=4, H=4, W=8, Cin=6, Cout=6, hid=128), dict(name="taping without its masks",
                                                                         N=1, H=8, W=8, Cin=6, Cout=6, hid=128, tape_no_masks=True),
            dict(name="taping with HW % 32 != 0", N=1, H=17, W=4, Cin=6, Cout=6, hid=128, tape_with_masks=True),
            dict(name="Cout with no group split", N=1, H=8, W=8, Cin=6, Cout=118, hid=128),
            dict(name="scratch below the plan's", N=1, H=8, W=8, Cin=6, Cout=6, hid=128, short_scratch=True))

IMAGE_FORMS = ("plain", "kperm", "transposed", "folded")
IMAGE_CASES = tuple(
    [dict(kind=GEMM, Cin=ci, Cout=co, form=f) for ci, co in ((64, 64), (512, 192), (192, 200)) for f in ("plain", "transposed", "folded")] +
    [dict(kind=GEMM, Cin=ci, Cout=co, form=f) for ci, co in ((64, 64), (512, 512)) for f in ("kperm", "kperm+folded", "kperm+transposed+folded")] +
    [dict(kind=FIRST, Cin=ci, Cout=co, form=f) for ci, co in ((6, 64), (12, 512), (35, 100), (96, 192), (256, 40)) for f in ("plain", "transposed", "folded", "transposed+folded")] +
    [dict(kind=TAIL, Cin=ci, Cout=co, form=f) for ci, co in ((64, 6), (512, 12), (128, 35), (256, 48)) for f in ("kperm", "kperm+transposed")])


def image_operands(c):
    """(w as the hook takes it, fold_bias, fold_logs, kperm, transposed) of an image case"""
    r = rng_of("image", c["kind"], c["Cin"], c["Cout"], c["form"])
    tr, fo = "transposed" in c["form"], "folded" in c["form"]
    shape = (c["Cout"], c["Cin"]) if c["kind"] == GEMM else (c["Cout"], c["Cin"], 3, 3)
    w = (0.05 * r.standard_normal(shape) * np.exp2(r.integers(-6, 7, c["Cout"])).reshape((-1,) + (1,) * (len(shape) - 1))).astype(f32)
    w[1 % c["Cout"]] = 0                                   # an all-zero row: exponent 0
    if tr:
        w = flip_t(w)                                      # the hook is handed the FORWARD weight of which w is the flipped transpose
    fb = r.uniform(-0.5, 0.5, c["Cout"]).astype(f32) if fo else None
    fl = r.uniform(-0.3, 0.3, c["Cout"]).astype(f32) if fo else None
    return w, fb, fl, "kperm" in c["form"], tr


# in_scale / out_scale of the taping and backward launches: as csrc/plan_train.hip derives them (SH2_ACT_SCALE and SH2_ACT_INV; the
# backward: SH2_ACT_SCALE * grad_scale and SH2_ACT_INV * SH_LO_SCALE = 128, grad_scale = 1 here) and one exact power of two either side
def scales(c):
    return ((16.0, 128.0), (8.0, 64.0), (32.0, 256.0)) if c["bwd"] else ((16.0, 1.0 / 16), (8.0, 1.0 / 8), (32.0, 1.0 / 32))


def scaled(d, in_scale):
    """the input handed to a launch at another in_scale so that its window holds the same values: z1 * 16 / in_scale (exact) -- the
    reference, the exact conditions and the sign-bit margins are then those of d itself, and a kernel that ignored in_scale would
    be off by a factor of two"""
    return dict(d, z1=(d["z1"] * f32(ACT / in_scale)).astype(f32))


# ---------------------------------------------------------------------------------------------------------------------
# the deep levels' k_dn_gemm (csrc/dnet_sh.hip): MIX (state = W u) and the three launches F0 -> F2 -> F4 of dnet_coupling_net
# ---------------------------------------------------------------------------------------------------------------------
DN_KS_MAX = 8


def dn_carve(N, C, H, W, hid, Cout):
    """csrc/dnet_sh.hip dn_carve written out again: byte offsets of u, ypad, h1, h2pad, part (256-byte aligned) and the level's bytes"""
    P, SLN = N * H * W, N * (H + 2) * (W + 2)
    sizes = [4 * C * P, 4 * (C // 2) * SLN, 4 * hid * P, 4 * hid * SLN, 4 * DN_KS_MAX * Cout * P]
    off = np.concatenate([[0], np.cumsum([-(-b // 256) * 256 for b in sizes])]).astype(np.int64)
    per = 4 * (C * H * W + (C // 2) * (H + 2) * (W + 2) + hid * H * W + hid * (H + 2) * (W + 2) + DN_KS_MAX * Cout * H * W) + 8 * 256
    assert off[5] <= N * per
    return dict(u=int(off[0]), ypad=int(off[1]), h1=int(off[2]), h2pad=int(off[3]), part=int(off[4]), end=int(off[5]), bytes=N * per, P=P, SLN=SLN)


def dn_instance(M, P):
    """dn_launch_gemm: (RT, PT, NPF) and the (x, y) grid"""
    pt2, rt2 = P > 32, M % 64 == 0 and P >= 512
    inst = (2, 2, 4) if rt2 and pt2 else ((1, 2, 6) if pt2 else (1, 1, 8))
    return inst, (-(-P // (64 if pt2 else 32)), M // (64 if rt2 else 32))


def dn_ksplit(M, P, S):
    big = P >= 512 and M % 64 == 0
    tiles = -(-M // (64 if big else 32)) * -(-P // 64)
    ks = 1
    while ks < DN_KS_MAX and tiles * ks * 2 <= (256 if big else 512) and S // (ks * 2) >= 32:
        ks *= 2
    return ks


def pad_slots(N, H, W):
    n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    return (n * (H + 2) * (W + 2) + (y + 1) * (W + 2) + x + 1).reshape(-1)


def sh2_planes(v16, slots, slot_of_pixel):
    """(C, P) fp32 values at the SH2 scale -> the operand's two planes half [C / 8][slots][8] as one uint16 array (2, C / 8 * slots * 8);
    slots no pixel maps to hold zero"""
    C, P = v16.shape
    out = np.zeros((2, C // 8, slots, 8), np.uint16)
    for pl, h in enumerate(split(v16)):
        out[pl][:, slot_of_pixel, :] = h.view(np.uint16).reshape(C // 8, 8, P).transpose(0, 2, 1)
    return out.reshape(2, -1)


DN_MIX_CASES = tuple(dict(name="dn_mix C%d %dx%dx%d %s%s" % (C, N, H, W, "rev" if rev else "fwd", " pad" if pad else ""), C=C, N=N, H=H, W=W, reverse=rev, want_pad=pad)
                     for i, (C, N, H, W) in enumerate(((192, 2, 4, 4), (384, 3, 8, 8), (192, 8, 8, 8), (384, 5, 2, 2), (192, 3, 4, 8), (384, 33, 4, 4)))
                     for rev, pad in (((0, 1), (1, 0)) if i % 2 else ((0, 0), (1, 1))))
DN_NET_CASES = tuple(dict(name="dn_net C%d %dx%dx%d" % (C, N, H, W), C=C, Cin=C // 2, Cout=C, hid=512, N=N, H=H, W=W, bwd=False, tape=False)
                     for C, N, H, W in ((192, 2, 4, 4), (384, 1, 8, 8), (192, 3, 4, 8), (384, 8, 8, 8), (384, 5, 2, 2)))      # (ks = 8 but for 384 at P = 512: 2)
DN_INSTANCES = ((1, 1, 8), (1, 2, 6), (2, 2, 4))


def build_mix(c, fam):
    """W (C, C), v (C, P) and, reverse, post_scale / post_bias (C); exact sets as in build(): pairs on equal inputs / powers of two"""
    C, P = c["C"], c["N"] * c["H"] * c["W"]
    r = rng_of("dn_mix", c["name"], fam)
    if fam == "random":
        d = dict(w=(np.linalg.qr(r.standard_normal((C, C)))[0] + 0.05 * r.standard_normal((C, C))).astype(f32), v=(1.5 * r.standard_normal((C, P))).astype(f32))
        ps, pb = np.exp(r.uniform(-0.9, 0.9, C)).astype(f32), r.uniform(-0.5, 0.5, C).astype(f32)
    elif fam == "exact-w":
        d = dict(w=(np.stack([_pairs_row(r, C // 2, 3) for _ in range(C)]) * 2.0 ** -13).astype(f32), v=np.repeat(r.integers(-2, 3, (C // 2, P)), 2, axis=0).astype(f32))
        ps, pb = np.exp2(r.integers(-1, 2, C)).astype(f32), r.integers(-2, 3, C).astype(f32)
    else:
        w = np.zeros((C, C))
        for o in range(C):
            w[o, r.choice(C, 2, replace=False)] = r.choice([-1.0, 1.0], 2) * 2.0 ** r.integers(-2, 1)
        d = dict(w=w.astype(f32), v=((2 * r.integers(2048, 16384, (C, P)) + 1) * r.choice([-1.0, 1.0], (C, P)) / 1024.0).astype(f32))
        ps, pb = np.exp2(r.integers(-1, 2, C)).astype(f32), r.integers(-2, 3, C).astype(f32)
    if c["reverse"]:
        d.update(ps=ps, pb=pb)
    return d


def mix_ref(c, d):
    """(state (C, P) float64, bound): W v by bound_sh2 with K = C (lu_oracle.apply_bound_sh2's formula); reverse y ps - pb: two more roundings"""
    W, v = d["w"].astype(f64), d["v"].astype(f64)
    y = W @ v
    aW, av = np.abs(W), np.abs(v)
    e = bound_sh2(aW @ av, c["C"], aW.max(axis=1)[:, None] * av.sum(axis=0)[None, :], aW.sum(axis=1)[:, None])
    if c["reverse"]:
        ps, pb = d["ps"].astype(f64)[:, None], d["pb"].astype(f64)[:, None]
        e = e * np.abs(ps) + 2 * U * (np.abs(y * ps) + np.abs(pb)) + U * np.abs(y * ps)
        y = y * ps - pb
    return y, e

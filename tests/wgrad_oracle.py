"""Host side of the weight-gradient GEMM tests (numpy only): the fp64 reference of the three GEMMs of csrc/wgrad_mfma.hip, the
packers of its operand layouts, the per-element bound the kernels are held to, the two input families, and the table of cases
tests/test_gpu_wgrad.py launches and tests/test_wgrad_host.py checks on the CPU.

All three weight gradients are one "NT" GEMM over the batch's pixels (header comment of csrc/wgrad_mfma.hip):

    C[m][n] = sum_{img, p} A[img][m][p] * B[img][n][p]
      f.2 (1x1):  A = g_u2, B = h1                                          -> dW2[o][i]            (mode 0)
      f.4 (3x3):  A rows (o*9 + tap) = g[o][p - d(tap)]  (sign = -1), B = h2 -> dW4[o][i][tap]       (mode 1)
      f.0 (3x3):  A = g_u0, B rows (i*9 + tap) = y1[i][p + d(tap)] (sign = +1) -> dW0[o][i][tap] flat (mode 0)
    d(tap) = (tap // 3 - 1, tap % 3 - 1), zero outside the image.

The reference works from the operands EXACTLY as the kernel receives them: an fp16 B is promoted, a pre-scaled ("PS") A is divided by
sh_scale * 2^11 (a power of two), the 3x3 operands are formed by explicit shifts.

THE BOUND (bound() below; nothing in it is fitted to the kernel's output).  u = 2^-11 is fp16's unit roundoff.
  * Operand split (csrc/sh.h).  The kernel carries x' (A times the power of two sh_scale; B as it is) as hi = fp16(x'),
    lo = fp16((x' - hi) 2^11):  x' = hi + lo / 2^11 + rho,  |x' - hi| <= u |x'| exactly in fp32, |rho| <= u^2 |x'| = 2^-22 |x'| while
    lo 2^11 is a normal fp16 number, and <= 2^-25 / 2^11 = 2^-36 (half the fp16 subnormal spacing, scaled back) otherwise:
    |rho| <= max(2^-22 |x'|, 2^-36).  Kept products: hi hi + (hi lo + lo hi) / 2^11, each exact in fp32 (11 x 11 bits).  Missing from
    a' b:  lo_a lo_b / 2^22 + rho_a b + a' rho_b - rho_a rho_b, with |lo / 2^11| <= u (1 + u) |x'|:
        two-plane B:  <= 3 u^2 (1 + u) |a' b|  +  2^-36 (|a'| + |b|)        fp16 B (rho_b = lo_b = 0):  <= u^2 |a' b| + 2^-36 |b|
    Divided by sh_scale on the way out (exact), this is  c_rep * absdot  +  the floor terms  2^-36 (sum|a| + sum|b| / sh_scale).
  * fp32 accumulation.  A split adds its 32 nk products per accumulator in an order the matrix pipe chooses; any order of n
    additions is within n * (one rounding) of the exact sum of the magnitudes.  One rounding is taken as 2^-23 (the pipe's
    internal rounding is not documented to be to-nearest; the LU tests' mixer bound does the same):
        gamma = 32 nk 2^-23,  times (1 + 2^-8) for the cross accumulator's 64 nk addends of relative size 2 u (1 + u) and |hi| <= (1 + u) |x|.
    Summed over the splits it multiplies the whole absdot (nk = the longest split).
  * Epilogue and reduction.  (accm + accx 2^-11) / sh_scale: one rounded addition per split, the scalings exact; the split-K
    reduction adds `splits` partials in order: (splits + 1) 2^-24 absdot (1 + 2^-8).
  * fp32 instances k_wgrad_gemm<64 / 128>: every product rounded once (2^-24) in place of the split term.
  * k_wgrad_direct: products rounded to fp32, summed in fp64, stored as fp32: 2^-24 absdot + 2^-24 |dW| (+ 2^-40 absdot for the fp64 sums).
  * rowsum: the workgroup's fp32 sum of the 32 nk values of a row as stored (a thread's chunk sums, three shuffles), rounding to
    nearest: 32 nk 2^-24 sum|a|; then exact scalings and `splits` fp64 atomic additions: (splits + 1) 2^-52 (|initial| + sum|a|).

LIMIT OF THE RANDOM FAMILY.  The accumulation term is a worst case that grows with nk; an honest bound cannot be smaller, and a
dropped lo plane (u per product, random sign) sinks below it once the pixel axis is long (tests/test_wgrad_host.py measures where).
On long pixel axes only the `exact` family -- every partial sum in every order an fp32 number, so the kernel must return the
reference value for value -- is sensitive to a dropped plane or a lost k-tile.  The bound is not tightened to hide that."""
import numpy as np

U = 2.0 ** -11
LO = 2048.0
EXACT_CAP = 2.0 ** 24          # sum|a||b| < EXACT_CAP * granularity on every output of an `exact` set


def round_up(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def expand(t, sign, rows_pad=None):
    """(N, C, H, W) -> (N, rows_pad, HW): row c*9 + tap holds t[c][p + sign * d(tap)], zero outside the image; rows >= 9 C zero.
    What k_shift_expand writes and a WgradTaps operand stands for.  Keeps the dtype."""
    N, C, H, W = t.shape
    rows = 9 * C if rows_pad is None else rows_pad
    out = np.zeros((N, rows, H, W), t.dtype)
    for tap in range(9):
        dy, dx = (tap // 3 - 1) * sign, (tap % 3 - 1) * sign
        ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))       # destination pixels with a source inside
        yd, xd = slice(max(0, -dy) + dy, min(H, H - dy) + dy), slice(max(0, -dx) + dx, min(W, W - dx) + dx)
        out[:, tap:9 * C:9, ys, xs] = t[:, :, yd, xd]
    return out.reshape(N, rows, H * W)


def as_matrix(x):
    """(N, rows, HW) -> (rows, N * HW): the batch's pixels as one axis, image-major."""
    N, R, HW = x.shape
    return np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(R, N * HW)


def pack_tiled(x, rows_pad=None):
    """(N, rows, HW) -> pixel-tile-major [pixel / 32][rows_pad][pixel % 32] over the batch's pixels (N * HW % 32 == 0), flat."""
    m = as_matrix(x)
    R, K = m.shape
    rp = R if rows_pad is None else rows_pad
    out = np.zeros((K // 32, rp, 32), x.dtype)
    out[:, :R, :] = m.reshape(R, K // 32, 32).transpose(1, 0, 2)
    return out.reshape(-1)


def unpack_tiled(flat, N, rows, HW, rows_pad=None):
    rp = rows if rows_pad is None else rows_pad
    t = np.asarray(flat).reshape(N * HW // 32, rp, 32)[:, :rows, :]
    return np.ascontiguousarray(t.transpose(1, 0, 2).reshape(rows, N, HW).transpose(1, 0, 2))


def pad_rows(x, rows_pad):
    """(N, rows, HW) -> (N, rows_pad, HW), zero rows behind."""
    N, R, HW = x.shape
    out = np.zeros((N, rows_pad, HW), x.dtype)
    out[:, :R] = x
    return out


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def to_layout(C, mode, Mreal, Nreal):
    """(>= Mreal, >= Nreal) matrix -> the flat dW of wgrad_reduce_body: mode 0 dW[m * Nreal + n]; mode 1 (m = o*9 + tap) dW[(o * Nreal + n) * 9 + tap]."""
    C = C[:Mreal, :Nreal]
    if mode == 0:
        return np.ascontiguousarray(C).reshape(-1)
    return np.ascontiguousarray(C.reshape(Mreal // 9, 9, Nreal).transpose(0, 2, 1)).reshape(-1)


def logical(A, B, taps=None, a_div=1.0):
    """The (rows, N * HW) float64 matrices the GEMM contracts.  A, B: (N, rows, HW) arrays as the kernel receives them (fp16 B
    promoted exactly), or -- taps = (operand, sign) -- operand 0 / 1 as the (N, C, H, W) tensor it is gathered from.  a_div: what a
    pre-scaled A is divided by (sh_scale * 2^11)."""
    if taps is not None and taps[0] == 0:
        A = expand(A, taps[1])
    if taps is not None and taps[0] == 1:
        B = expand(B, taps[1])
    return as_matrix(A.astype(np.float64)) / a_div, as_matrix(B.astype(np.float64))


def dw_ref(A, B, mode, Mreal, Nreal, taps=None, a_div=1.0):
    a, b = logical(A, B, taps, a_div)
    return to_layout(a[:Mreal] @ b[:Nreal].T, mode, Mreal, Nreal)


def absdot(A, B, mode, Mreal, Nreal, taps=None, a_div=1.0):
    a, b = logical(A, B, taps, a_div)
    return to_layout(np.abs(a[:Mreal]) @ np.abs(b[:Nreal]).T, mode, Mreal, Nreal)


def rowsum_ref(A, a_div=1.0):
    """(sum over all pixels of every row of plain A, the same of |A|), float64."""
    a = as_matrix(A.astype(np.float64)) / a_div
    return a.sum(1), np.abs(a).sum(1)


def direct_ref(gy, x, ksize):
    """k_wgrad_direct: dW[o][i][ky][kx] = sum gy[n,o,y,x] x[n,i,y+ky-1,x+kx-1] (gy (N, Cout, H, W), x (N, Cin, H, W)) -> (flat dW, flat absdot)."""
    N, Cout, H, W = gy.shape
    g = as_matrix(gy.reshape(N, Cout, H * W).astype(np.float64))
    xe = as_matrix((expand(x, +1) if ksize == 3 else x.reshape(N, x.shape[1], H * W)).astype(np.float64))
    return (g @ xe.T).reshape(-1), (np.abs(g) @ np.abs(xe).T).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# bound
# ---------------------------------------------------------------------------------------------------------------------
def bound(absd, splits, nk, kind, sh_scale=1.0, sum_a=None, sum_b=None, mode=0, Mreal=None, Nreal=None):
    """Per-element bound on |dW - dw_ref| (flat, the layout of `mode`).  absd: absdot in the same layout; splits, nk: from the
    launch (glowhip_wgrad_info); kind: 'sh2' (two-plane B), 'sh1' (fp16 B), 'f32'.  sum_a (Mreal) / sum_b (Nreal): sum over the
    pixels of |a| per row of A / |b| per row of B for the floor terms (sh kinds)."""
    acc = 32.0 * nk * 2.0 ** -23 + (splits + 1) * 2.0 ** -24
    if kind == "f32":
        return absd * (2.0 ** -24 + acc)
    c_rep = 3 * U * U * (1 + U) if kind == "sh2" else U * U
    floor = np.outer(np.zeros(Mreal) if kind == "sh1" else sum_a, np.ones(Nreal)) + np.outer(np.ones(Mreal), sum_b) / sh_scale
    return absd * (c_rep + acc * (1 + 2.0 ** -8)) + 2.0 ** -36 * to_layout(floor, mode, Mreal, Nreal)


def bound_direct(absd, ref):
    return absd * (2.0 ** -24 + 2.0 ** -40) + np.abs(ref) * 2.0 ** -24


def bound_rowsum(sum_abs_a, splits, nk, initial):
    return 32.0 * nk * 2.0 ** -24 * sum_abs_a + (splits + 1) * 2.0 ** -52 * (np.abs(initial) + sum_abs_a)


# ---------------------------------------------------------------------------------------------------------------------
# input families.  Every generator returns float32 / float16 arrays (N, rows, HW) or (N, C, H, W); sh_scale is the caller's.
# ---------------------------------------------------------------------------------------------------------------------
def _rs(*key):
    h = 0
    for k in key:
        h = (h * 1000003 + (hash(k) if not isinstance(k, str) else sum(ord(c) * (i + 1) for i, c in enumerate(k)))) % (2 ** 31 - 1)
    return np.random.RandomState(h)


EXACT_SH_SCALE = 2.0 ** 8
RANDOM_SH_SCALE = 2.0 ** 18         # the training step's: 2^rint(log2(N ln2 CHW)) at a batch of 32 64x64x3 images
ROW_EXP = (0, -4, -8)               # `exact`: row r of A carries 2^ROW_EXP[r % 3]
BLOCKS = (1.0, 1e-3, 1e-7)          # `random`: row r of A times sh_scale has this magnitude


def thin_keep(K):
    """`exact`: A is non-zero at one pixel in `keep` so that sum|a||b| <= K / keep * 12 stays below 2^13 row units = 2^24 granules
    (exact1: |a| < 2 row units, |b| <= 3; exact2: |a| <= 3, |b| < 4)."""
    keep = 1
    while K / keep * 12 >= 8000:
        keep *= 2
    return keep


def gen_a(family, shape, sh_scale, seed):
    """Operand A (plain (N, rows, HW) or the gathered (N, C, H, W)): float32, the TRUE gradient (the kernel multiplies by sh_scale)."""
    rs = _rs("a", family, shape, seed)
    N, R = shape[0], shape[1]
    K = int(np.prod(shape)) // R
    rowix = np.arange(R).reshape((1, R) + (1,) * (len(shape) - 2))
    if family == "random":
        blk = np.asarray(BLOCKS)[rowix % 3]
        return (rs.randn(*shape) * blk).astype(np.float32) / np.float32(sh_scale)
    sgn = rs.randint(0, 2, size=shape) * 2 - 1
    scale = np.exp2(np.asarray(ROW_EXP, np.float64)[rowix % 3])
    if family == "exact1":          # +-(1 + j 2^-11): odd j on most entries -> a non-zero lo plane
        j = rs.randint(0, 2048, size=shape) | (rs.randint(0, 8, size=shape) > 0)
        v = sgn * (1.0 + j / 2048.0)
    else:                           # exact2: integer A, the lo plane is B's
        v = sgn * rs.randint(1, 4, size=shape).astype(np.float64)
    keep = thin_keep(K)
    if keep > 1:
        pix = np.arange(int(np.prod(shape[2:]))).reshape((1, 1) + tuple(shape[2:])) + np.arange(N).reshape((N, 1) + (1,) * (len(shape) - 2)) * int(np.prod(shape[2:]))
        v = v * (((pix + 3 * rowix) % keep) == 0)
    return (v * scale).astype(np.float32)


def gen_b(family, shape, half, relu, seed):
    """Operand B: float16 (half) or float32.  random: relu -> >= 0 with about half zeros (a ReLU output), else signed (y1)."""
    rs = _rs("b", family, shape, seed)
    if family == "random":
        v = rs.randn(*shape)
        if relu:
            v = np.maximum(v, 0.0)
        return v.astype(np.float16) if half else v.astype(np.float32)
    i = rs.randint(0, 4, size=shape).astype(np.float64)
    if relu:
        i = i * rs.randint(0, 2, size=shape)
    else:
        i = i * (rs.randint(0, 2, size=shape) * 2 - 1)
    if family == "exact2":          # i + j 2^-11: fp32, a non-zero lo plane (never an fp16 tensor)
        assert not half
        j = rs.randint(0, 2048, size=shape) | 1
        i = np.where(i != 0, i + np.sign(i) * j / 2048.0, 0.0)      # |b| < 4: hi on fp16's 2^-9 grid there, lo 2^11 an integer <= 2
    return i.astype(np.float16) if half else i.astype(np.float32)


def exact_granule(family, Mreal, mode, Nreal, gathered_a):
    """Granularity of every product on output row m (flat layout): A's row unit times the finest fraction in play."""
    rows = np.arange(Mreal)
    ch = rows // 9 if gathered_a else rows
    g = np.exp2(np.asarray(ROW_EXP, np.float64)[ch % 3]) * 2.0 ** -11
    return to_layout(np.outer(g, np.ones(Nreal)), mode, Mreal, Nreal)


def exact_ok(ref, absd, granule):
    """The two conditions of an `exact` set: the reference is an fp32 number on every element, and sum|a||b| stays below 2^24 granules
    (then every partial sum, in any order, is a multiple of the granule below 2^24 of them: an fp32 number)."""
    return bool(np.all(ref.astype(np.float32).astype(np.float64) == ref)) and bool(np.all(absd < EXACT_CAP * granule)) and \
        bool(np.all(np.round(ref / granule) == ref / granule))


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_wgrad.py (one launch_wgrad_mfma each); tests/test_wgrad_host.py checks every input set on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def mfma_case(name, N, H, W, Mreal, Nreal, Npad, a="plain", b="plain", mode=0, tiled=0, rowsum=False, b_valid=0, families=None, Mpad=None,
              sh=True):
    """a: 'plain' | 'taps' (gathered, Mreal = 9 C) | 'ps' (plain, stored times sh_scale 2^11);  b: 'plain' | 'taps' (Nreal = 9 C) |
    'half' | 'bvalid'.  tiled: bits 0 / 1 as launch_wgrad_mfma's (bit 2 follows from a == 'ps')."""
    fam = families or (("random", "exact1") if b == "half" else ("random", "exact1", "exact2"))
    return dict(name=name, N=N, H=H, W=W, HW=H * W, Mreal=Mreal, Mpad=Mpad or round_up(Mreal, 128), Nreal=Nreal, Npad=Npad, a=a, b=b, mode=mode,
                tiled=tiled | (4 if a == "ps" else 0), rowsum=rowsum, b_valid=b_valid, families=fam, sh=sh)


def build_mfma(case, family, seed=0):
    """Inputs of one launch as flat numpy arrays in the kernel's layouts + the fp64 reference.  Returns a dict:
    A, B (flat device images), a_bs, b_bs, taps (operand, C, H, W, sign) or None, sh_scale, ref, absd, sum_a, sum_b (floor terms),
    rs_ref, rs_abs (row sums over Mpad rows) and `kind` for bound()."""
    c = case
    N, H, W, HW = c["N"], c["H"], c["W"], c["HW"]
    sh_scale = (EXACT_SH_SCALE if family != "random" else RANDOM_SH_SCALE) if c["sh"] else 0.0
    gen_scale = sh_scale if c["sh"] else 1.0
    taps = None
    if c["a"] == "taps":
        Ca = c["Mreal"] // 9
        At = gen_a(family, (N, Ca, H, W), gen_scale, seed)
        taps = (0, Ca, H, W, -1)
        A_dev, a_bs, A_ref = At.reshape(-1), Ca * HW, At
    else:
        Ap = gen_a(family, (N, c["Mpad"], HW), gen_scale, seed)
        A_st = (Ap * np.float32(sh_scale * LO)) if c["a"] == "ps" else Ap
        A_dev = pack_tiled(A_st) if c["tiled"] & 1 else A_st.reshape(-1)
        a_bs, A_ref = c["Mpad"] * HW, A_st
    a_div = sh_scale * LO if c["a"] == "ps" else 1.0
    half = c["b"] == "half"
    if c["b"] == "taps":
        Cb = c["Nreal"] // 9
        Bt = gen_b(family, (N, Cb, H, W), False, False, seed)
        taps = (1, Cb, H, W, +1)
        B_dev, b_bs, B_ref = Bt.reshape(-1), Cb * HW, Bt
    elif c["b"] == "bvalid":            # the first b_valid channels of a wider (N, 2 b_valid, HW) tensor: the rest must not be read as B
        Bw = gen_b(family, (N, 2 * c["b_valid"], HW), False, False, seed)
        B_dev, b_bs, B_ref = Bw.reshape(-1), 2 * c["b_valid"] * HW, Bw[:, :c["b_valid"]]
    else:
        Bp = gen_b(family, (N, c["Npad"], HW), half, c["a"] != "plain" or half, seed)
        B_dev = pack_tiled(Bp) if c["tiled"] & 2 else Bp.reshape(-1)
        b_bs, B_ref = c["Npad"] * HW, Bp
    tp = None if taps is None else (taps[0], taps[4])
    a64, b64 = logical(A_ref, B_ref, tp, a_div)
    Mr, Nr = c["Mreal"], c["Nreal"]
    out = dict(A=A_dev, B=B_dev, a_bs=a_bs, b_bs=b_bs, taps=taps, sh_scale=sh_scale, a_div=a_div, A_ref=A_ref, B_ref=B_ref, tp=tp,
               ref=to_layout(a64[:Mr] @ b64[:Nr].T, c["mode"], Mr, Nr), absd=to_layout(np.abs(a64[:Mr]) @ np.abs(b64[:Nr]).T, c["mode"], Mr, Nr),
               sum_a=np.abs(a64[:Mr]).sum(1), sum_b=np.abs(b64[:Nr]).sum(1), kind=("f32" if not c["sh"] else "sh1" if half else "sh2"))
    if c["a"] != "taps":
        out["rs_ref"], out["rs_abs"] = a64.sum(1), np.abs(a64).sum(1)
    if family != "random":
        out["granule"] = exact_granule(family, Mr, c["mode"], Nr, c["a"] == "taps")
    return out


def expected_splits(Mpad, Npad, total, wide=False):
    """launch_wgrad_mfma's split arithmetic (for choosing shapes; the tests assert what glowhip_wgrad_info reports)."""
    tiles = (Mpad // 128) * (Npad // 256 if wide else Npad // 128 if Npad % 128 == 0 else Npad // 64)
    sp = max(1, min(total, ((256 if wide else 512) + tiles - 1) // tiles))
    per = (total + sp - 1) // sp
    return (total + per - 1) // per, per


MAPS = ((8, 4), (4, 8), (2, 16), (16, 16))


def shape_cases():
    """k_wgrad_gemm_sh<128 / 64> plain, VA, VB, BV, BH; the gather edges ride here: W = 4 (every chunk a whole row), H = 2 (both halo
    rows outside), N = 3 (neighbouring images), rows >= 9 C inside the last row tile (C = 12: rows 108 .. 127 zero)."""
    out = []
    for (H, W) in MAPS:
        for N in (1, 3):
            t = f"{H}x{W}n{N}"
            for npad, nreal in ((128, 100), (64, 54)):
                out.append(mfma_case(f"plain{npad}-{t}", N, H, W, 100, nreal, npad, rowsum=True))
                out.append(mfma_case(f"va{npad}-{t}", N, H, W, 108, nreal, npad, a="taps", mode=1))
            out.append(mfma_case(f"vb128-{t}", N, H, W, 128, 108, 128, b="taps", rowsum=True))
            out.append(mfma_case(f"vb64-{t}", N, H, W, 128, 54, 64, b="taps"))
            for bv in (6, 24):
                out.append(mfma_case(f"bv{bv}-{t}", N, H, W, 108, bv, 64, a="taps", b="bvalid", mode=1, b_valid=bv))
    for (H, W, N) in ((8, 4, 1), (16, 16, 3), (4, 8, 3)):
        t = f"{H}x{W}n{N}"
        for cout in (6, 12, 24):
            for tiled in (0, 2):
                out.append(mfma_case(f"bh-va-c{cout}-t{tiled}-{t}", N, H, W, 9 * cout, 128, 128, a="taps", b="half", mode=1, tiled=tiled))
        for tiled in (0, 2, 3):
            out.append(mfma_case(f"bh-plain128-t{tiled}-{t}", N, H, W, 128, 128, 128, b="half", tiled=tiled, rowsum=True))
            out.append(mfma_case(f"bh-plain64-t{tiled}-{t}", N, H, W, 128, 64, 64, b="half", tiled=tiled))
        out.append(mfma_case(f"bh-va64-{t}", N, H, W, 108, 64, 64, a="taps", b="half", mode=1, tiled=2))
        # pre-scaled A: f.2's kernels (fp16 B, both operands tiled) and f.0's form (tiled A, gathered B)
        out.append(mfma_case(f"ps128-{t}", N, H, W, 128, 128, 128, a="ps", b="half", tiled=3, rowsum=True))
        out.append(mfma_case(f"ps128x2-{t}", N, H, W, 256, 256, 256, a="ps", b="half", tiled=3, rowsum=True))
        out.append(mfma_case(f"ps64-{t}", N, H, W, 128, 64, 64, a="ps", b="half", tiled=3, rowsum=True))
        out.append(mfma_case(f"ps-vb128-{t}", N, H, W, 128, 108, 128, a="ps", b="taps", tiled=1, rowsum=True))
        out.append(mfma_case(f"ps-vb64-{t}", N, H, W, 128, 54, 64, a="ps", b="taps", tiled=1, rowsum=True))
    return out


def loop_cases():
    """ktiles_per_split 1 .. 8 at Mpad = Npad = 512 (16 tiles -> 32 splits) on the three loop forms: three stages (fp16 B on
    k_wgrad_gemm_sh<128, BH>), two stages (two-plane B at 128 columns), and k_wgrad_gemm_ps<128>; one case whose last split is
    shorter (total = 32 * 3 - 2 -> per 3, 32 splits, the last of one tile) and one with fewer k-tiles than splits (every split one tile)."""
    out = []
    for per in range(1, 9):
        N, H, W = per, 32, 32                       # total = 32 * per k-tiles
        fam = ("exact1", "random") if per <= 2 else ("exact1",)      # (random: only where the axis is short enough for it to see anything)
        out.append(mfma_case(f"loop3-per{per}", N, H, W, 512, 512, 512, b="half", tiled=2, families=fam))
        out.append(mfma_case(f"loop2-per{per}", N, H, W, 512, 512, 512, families=fam))
        out.append(mfma_case(f"loopps-per{per}", N, H, W, 512, 512, 512, a="ps", b="half", tiled=3, rowsum=True, families=fam))
    for form, kw in (("3", dict(b="half", tiled=2, families=("exact1",))), ("2", dict(families=("exact1",))),
                     ("ps", dict(a="ps", b="half", tiled=3, rowsum=True, families=("exact1",)))):
        out.append(mfma_case(f"loop{form}-short-last", 47, 8, 8, 512, 512, 512, **kw))       # 94 k-tiles
        out.append(mfma_case(f"loop{form}-one-tile-each", 5, 8, 8, 512, 512, 512, **kw))     # 10 k-tiles < 32
    return out


def wide_cases():
    """k_wgrad_gemm_ps512: Npad 256 and 512 with 512 k-tiles (its threshold), N * HW = 16 384."""
    return [mfma_case("ps512-256", 16, 32, 32, 256, 256, 256, a="ps", b="half", tiled=3, rowsum=True, families=("exact1",)),
            mfma_case("ps512-512", 16, 32, 32, 512, 512, 512, a="ps", b="half", tiled=3, rowsum=True, families=("exact1", "random"))]


def reduce_cases():
    """mode 0 / 1, Nreal 54 (two live columns in the last quad) / 108 / 216, splits 1, 7, 8, 9, 17 (N images of 32 pixels at few tiles)."""
    out = []
    for sp in (1, 7, 8, 9, 17):
        out.append(mfma_case(f"red-m0-n54-s{sp}", sp, 8, 4, 128, 54, 64, b="taps"))
        out.append(mfma_case(f"red-m0-n108-s{sp}", sp, 8, 4, 128, 108, 128, b="taps"))
        out.append(mfma_case(f"red-m0-n216-s{sp}", sp, 8, 4, 128, 216, 256, b="taps"))
        out.append(mfma_case(f"red-m1-c6-s{sp}", sp, 8, 4, 54, 100, 128, a="taps", mode=1))
        out.append(mfma_case(f"red-m1-c24-s{sp}", sp, 8, 4, 216, 54, 64, a="taps", mode=1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the grouped launches: f.4's and f.0's GEMMs (k_wgrad_gemm_pair), with f.2's as the third (k_wgrad_gemm_trio)
# ---------------------------------------------------------------------------------------------------------------------
def expected_group_splits(total, hid, m4, n0, trio):
    """The share arithmetic of launch_wgrad_group: ((splits, per) of f.4, of f.0, of f.2 or None, and the fractional parts of
    512 share / tiles that decided the rounding).  For choosing shapes and for the host yardstick; the GPU tests assert what
    glowhip_wgrad_info reports against it."""
    bn0 = 64 if n0 == 64 else 128
    tiles = dict(f4=(m4 // 128) * (hid // 128), f0=(hid // 128) * (n0 // bn0), f2=(hid // 128) ** 2)
    w = dict(f4=2.0 * m4 * hid, f0=3.0 * hid * n0, f2=2.0 * hid * hid if trio else 0.0)
    wsum = sum(w.values())
    out, frac = {}, {}
    for k in ("f4", "f0") + (("f2",) if trio else ()):
        x = 512.0 * (w[k] / wsum) / tiles[k]
        sp = max(1, min(total, int(x + 0.5)))
        per = (total + sp - 1) // sp
        out[k] = ((total + per - 1) // per, per)
        frac[k] = (x - int(x), int(x + 0.5) <= total)
    return out, frac, tiles


def group_case(name, N, H, W, C, affine, hid, trio, families=("exact1", "random")):
    """One FlowStep's GEMMs at C channels (y1: C / 2; f.4 writes C / 2 or, affine, C output channels).  Three independent operand
    sets in the layouts the backward sweep hands over: f.4 gathered g_pre x fp16 pixel-tile-major h2; f.0 pre-scaled pixel-tile-major
    g_u0 x gathered y1 (+ row sums); f.2 pre-scaled g_u2 x fp16 h1, both pixel-tile-major (+ row sums)."""
    Ch, Cout = C // 2, C if affine else C // 2
    m4, n0 = round_up(9 * Cout, 128), round_up(9 * Ch, 64)
    sub = dict(f4=mfma_case(name + "/f4", N, H, W, 9 * Cout, hid, hid, a="taps", b="half", mode=1, tiled=2, families=families),
               f0=mfma_case(name + "/f0", N, H, W, hid, 9 * Ch, n0, a="ps", b="taps", tiled=1, rowsum=True, families=families))
    if trio:
        sub["f2"] = mfma_case(name + "/f2", N, H, W, hid, hid, hid, a="ps", b="half", tiled=3, rowsum=True, families=families)
    sp, frac, tiles = expected_group_splits(N * H * W // 32, hid, m4, n0, trio)
    for k in sub:
        sub[k]["splits_per"] = sp[k]
    return dict(name=name, N=N, H=H, W=W, HW=H * W, C=C, hid=hid, trio=trio, m4=m4, n0=n0, sub=sub, frac=frac, tiles=tiles, families=families)


def group_cases():
    """C = 12 (n0 = 64), 24, 48 (n0 = 128 / 256), additive and affine, hidden 128 and 256; short axes (every split one k-tile, live
    counts 6 x tiles) and axes long enough for the share arithmetic to decide (128 .. 200 k-tiles), where 512 share / tiles rounds
    both ways and the live block counts are no multiples of 8 (tests/test_wgrad_host.py asserts that of this table)."""
    out = []
    for trio in (False, True):
        t = "trio" if trio else "pair"
        for C in (12, 24, 48):
            for affine in (False, True):
                for hid in (128, 256):
                    out.append(group_case(f"{t}-c{C}-{'aff' if affine else 'add'}-h{hid}-8x8n3", 3, 8, 8, C, affine, hid, trio))
        out.append(group_case(f"{t}-c12-add-h128-16x16n25", 25, 16, 16, 12, False, 128, trio, families=("exact1",)))      # 200 k-tiles
        out.append(group_case(f"{t}-c24-aff-h256-32x32n4", 4, 32, 32, 24, True, 256, trio, families=("exact1",)))        # 128 k-tiles
        out.append(group_case(f"{t}-c48-aff-h128-16x16n19", 19, 16, 16, 48, True, 128, trio, families=("exact1",)))      # 152 k-tiles
    return out

"""Host side of the per-kernel tests of the exact-fp32 convolution kernels (csrc/conv_mfma.hip k_conv_wide / k_splitk_finish /
k_gemm_glds, csrc/conv_mfma_first.hip k_conv_first, csrc/conv_direct.hip k_conv_direct and the REPACK_WIDE / REPACK_FIRST image jobs
of csrc/pack.hip; the tail convolution with its seven epilogue modes has its own section further down), numpy only: the fp64 reference of every operation, the per-element bound each kernel is held to, the launchers'
routing rules written out again, the two input families, and the table of cases tests/test_gpu_conv_kernels.py launches through
glowhip_debug_conv and tests/test_conv_oracle_host.py checks on the CPU.

THE OPERATION ('SAME' convolution, stride 1, network/module.py:252-259):
    conv[n][o][y][x] = sum over ci, ky, kx of w[o][ci][ky][kx] x[n][ci][y + ky - k/2][x + kx - k/2]     (zero outside the map)
    WIDE    y = act((conv + post_bias) post_scale)                                  tables may be absent (0 / 1)
    FIRST   y = act((conv + fold_bias) exp(3 fold_logs))                            the ActNorm folded into the weight image
    DIRECT  y = act((conv + bias + post_bias) s),  s = post_scale, else exp(3 post_logs), else 1
    act = ReLU (relu = 1) or the identity.  transposed: the weight tensor is the FORWARD weight (Cin, Cout, k, k) of which this is
    the input-gradient convolution: w[o][ci][tap] = wf[ci][o][k k - 1 - tap].

THE ROUTES (wide_route / first_route below repeat the launchers' rules; the GPU tests assert them from glowhip_conv_info):
    wide   tile 128 when Cout % 128 == 0 and (Cout / 128) ceil(px / 128) >= 512, else 64;  k_gemm_glds takes 1x1 at tile 128 when
           Cin % 16 == 0, Cin >= 48, HW % 4 == 0 and px % 128 == 0;  split-K with scratch when tiles < 96 and the padded K has >= 16
           tiles of 32: S = min(16, 320 / tiles, ktiles / 4), lowered until S N Cout HW floats fit the scratch
    first  BN = 128 when HW % 128 == 0 and 128 % W == 0, lowered to 64 when that grid has < 512 workgroups (and 64 % W == 0, and the
           window fits the LDS); MB doubles while the output-channel tiles divide and >= 512 workgroups remain

THE BOUNDS.  u = 2^-24; every fp32 operation is one rounding to nearest, |error| <= u |result|; expf as 2 u (one ulp).  Nothing
below is fitted to a kernel's output; tests/test_conv_oracle_host.py shows that an fp32 emulation of the promised arithmetic stays
inside and that the listed single faults leave.  With A = sum |w| |x| over the K = Cin k k terms of an element:
  * accumulation: the MFMA (and the direct kernel's fmaf) adds one product per step with one rounding of a partial sum that never
    exceeds A in magnitude: K u A, in any order of the terms.  Padded k rows add exact zeros.
  * split-K: every slice is such a chain over its own terms (together K u A); k_splitk_finish adds S - 1 partial sums: (S - 1) u A.
  * wide epilogue: one addition of post_bias (when given) on at most A + |post_bias|, one product with post_scale (when given).
        |y - ref| <= u (K + S - 1 + c) (A + |post_bias|) |post_scale|,   c = 2
  * first: the image holds w' = fl(w E'), E' = expf(fl(3 logs)): fl(3 logs) moves the exponential by |3 logs| u, expf by 2 u, the
    product by u: (3 + |3 logs|) u per weight, the same for the folded bias, which starts the accumulator (one more term):
        |y - ref| <= u (K + 1 + 3 + |3 logs|) (A + |fold_bias|) exp(3 logs);   without a fold  u K A
  * direct: one addition each for bias and post_bias, one product for the scale; with post_logs the scale is expf(fl(3 logs)) as
    above, 2 + |3 logs| more:
        |y - ref| <= u (K + c) (A + |bias| + |post_bias|) |s|,   c = [bias] + [post_bias] + [scale: 1 | logs: 3 + |3 logs|]
  * ReLU does not enlarge an error.  bnd() adds 2^-10 relative for second-order terms and 2^-140 for subnormal intermediates.
  * two launches of the same operands with different S both lie inside their bounds, so they differ by at most the two bounds added.
KNOWN LIMIT.  The accumulation term grows with K while the error of one dropped term grows with sqrt(K) at best: at long K the random
family notices a wrong scale, tap or tile but not one missing product.  There only the exact family is sensitive.

FAMILIES.  `exact`: activations are integers in [-7, 7], the weights, bias and post_bias of output row o integers times the row's
granule 2^e[o], scales signed powers of two (passed as post_scale; the FIRST image folds with logs = 0, expf(0) = 1), and
(A + |bias| + |post_bias|) stays below 2^24 granules: every product and every partial sum in every order is an fp32 number, and the
kernel must return the reference value for value, whatever its order of accumulation.  check_exact() asserts the conditions for
every set.  `random` (seeded): activations N(0, 1), half of them zero where they stand for a ReLU output (the wide 1x1), weights 0.05 N(0, 1),
logs and bias 0.1 N(0, 1), rows at magnitudes 1, 1e-3, 1e-7 by output channel: every element within the bound, no outliers."""
import zlib

import numpy as np

U = 2.0 ** -24
f32, f64 = np.float32, np.float64
WIDE, FIRST, DIRECT = "wide", "first", "direct"


def bnd(x):
    return np.asarray(x, f64) * (1.0 + 2.0 ** -10) + 2.0 ** -140


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def inside(got, ref, bound):
    """every element within its bound (a NaN anywhere is outside)"""
    return bool(np.all(np.abs(np.asarray(got, f64) - ref) <= bound))


def worst(got, ref, bound):
    e = np.abs(np.asarray(got, f64) - ref)
    return float(np.max(np.where(bound > 0, e / np.where(bound > 0, bound, 1.0), np.where(e > 0, np.inf, 0.0)), initial=0.0))


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' rules, written out again
# ---------------------------------------------------------------------------------------------------------------------
def kpad(Cin, ks):
    return -(-Cin * ks * ks // 32) * 32


def wide_supported(Cin, H, W, Cout, ks):
    if Cout % 64 or (H * W) % 4:
        return False
    return Cin % 32 == 0 if ks == 1 else (ks == 3 and W % 4 == 0 and Cin >= 1)


def wide_route(c):
    """what launch_conv_mfma_wide picks: dict(kernel, tile, S, grid, launches, image_bytes)"""
    N, Cin, Cout, H, W, ks = c["N"], c["Cin"], c["Cout"], c["H"], c["W"], c["ks"]
    px, HW = N * H * W, H * W
    tile = 128 if Cout % 128 == 0 and (Cout // 128) * -(-px // 128) >= 512 else 64
    image = 0 if c.get("transposed") else kpad(Cin, ks) * Cout * 4
    if ks == 1 and tile == 128 and Cin % 16 == 0 and Cin >= 48 and HW % 4 == 0 and px % 128 == 0:
        return dict(kernel="k_gemm_glds", tile=128, S=1, grid=[(Cout // 128) * (px // 128), 1, 1], launches=1, image_bytes=image)
    tiles = (Cout // tile) * -(-px // tile)
    nkt = kpad(Cin, ks) // 32
    S, per = 1, N * Cout * HW
    if c.get("scratch") and tiles < 96 and nkt >= 16:
        S = min(16, 320 // tiles, nkt // 4)
        while S > 1 and S * per > c["scratch"]:
            S -= 1
    return dict(kernel="k_conv_wide<%d,%d>" % (ks, tile) + ("+k_splitk_finish" if S > 1 else ""), tile=tile, S=S, grid=[tiles, S, 1],
                launches=2 if S > 1 else 1, image_bytes=image)


def first_chs(TR, W):
    v = (TR + 2) * (W + 8)
    return v + ((16 - v % 32) + 32) % 32


def first_lds_ok(Cin, BN, W):
    return (2 * 54 * 128 + Cin * first_chs(BN // W, W)) * 4 <= 150 * 1024


def first_supported(Cin, H, W, Cout):
    if Cin % 6 or Cin > 192 or Cin < 6 or Cout % 128 or W not in (8, 16, 32, 64, 128):
        return False
    HW = H * W
    BN = 128 if HW % 128 == 0 else 64
    return HW % BN == 0 and BN % W == 0 and first_lds_ok(Cin, BN, W)


def first_route(c):
    N, Cin, Cout, H, W = c["N"], c["Cin"], c["Cout"], c["H"], c["W"]
    HW, px, mtiles = H * W, N * H * W, Cout // 128
    BN = 128 if HW % 128 == 0 and 128 % W == 0 else 64
    if BN == 128 and HW % 64 == 0 and 64 % W == 0 and (px // 128) * mtiles < 512 and first_lds_ok(Cin, 64, W):
        BN = 64
    MB = 1
    while MB * 2 <= mtiles and mtiles % (MB * 2) == 0 and (px // BN) * (mtiles // (MB * 2)) >= 512:
        MB *= 2
    return dict(kernel="k_conv_first<%d,%d>" % (BN, W), tile=BN, MB=MB, grid=[(px // BN) * (mtiles // MB), 1, 1], launches=1,
                image_bytes=(9 * Cin + 1) * Cout * 4)


def direct_route(c):
    return dict(kernel="k_conv_direct<%d>" % c["ks"], grid=[-(-c["H"] * c["W"] // 256), -(-c["Cout"] // 8), c["N"]], launches=1)


def route(c):
    return {WIDE: wide_route, FIRST: first_route, DIRECT: direct_route}[c["op"]](c)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _case(op, ks, Cin, Cout, H, W, N, **kw):
    c = dict(op=op, ks=ks, Cin=Cin, Cout=Cout, H=H, W=W, N=N, relu=1, tables=True, families=("exact", "random"))
    c.update(kw)
    return c


def wide_cases():
    out = []
    maps = ((4, 4), (2, 8), (8, 4), (6, 12), (16, 16))
    for i, Cin in enumerate((1, 2, 6, 7, 24, 64)):                       # k_conv_wide<3,64>
        for j, (H, W) in enumerate(maps):
            out.append(_case(WIDE, 3, Cin, 192 if (i + j) % 2 else 64, H, W, 3 if (i + j) % 3 else 1, relu=(i + j) % 4 != 3, tables=(i + j) % 5 != 4))
    for Cin in (32, 96):                                                 # k_conv_wide<1,64>
        for Cout in (64, 128):
            for H, W in ((1, 4), (4, 5), (8, 8)):
                out.append(_case(WIDE, 1, Cin, Cout, H, W, 3, relu=Cout == 64, tables=Cin == 32 or Cout == 128))
    for ks, Cin in ((3, 6), (1, 32), (1, 64), (1, 96)):                  # the 128 tiles: Cout 512 at 16 384 pixels
        out.append(_case(WIDE, ks, Cin, 512, 32, 32, 16, relu=1, tables=True))
        out.append(_case(WIDE, ks, Cin, 512, 32, 32, 16, relu=0, tables=False))
    per = 64 * 64
    for scratch in (4 * per, 3 * per, 2 * per, 2 * per + 100, per):      # split-K: S = 4, 3, 2, 2 and none
        out.append(_case(WIDE, 3, 64, 64, 8, 8, 1, scratch=scratch))
    out.append(_case(WIDE, 3, 64, 64, 16, 76, 5, scratch=3 * 5 * 64 * 16 * 76))      # 95 tiles: on (S = 3)
    out.append(_case(WIDE, 3, 64, 64, 16, 64, 6, scratch=3 * 6 * 64 * 16 * 64))      # 96 tiles: off
    out.append(_case(WIDE, 3, 53, 64, 8, 8, 1, scratch=4 * per, relu=0))             # 15 k-tiles: off
    out.append(_case(WIDE, 3, 55, 64, 8, 8, 1, scratch=4 * per, relu=0))             # 16 k-tiles: on
    out.append(_case(WIDE, 1, 512, 64, 8, 8, 1, scratch=4 * per))                    # 1x1 split-K (16 k-tiles)
    for c in (_case(WIDE, 3, 7, 64, 6, 12, 3), _case(WIDE, 1, 32, 64, 4, 5, 3), _case(WIDE, 1, 64, 512, 32, 32, 16, families=("random",)),
              _case(WIDE, 3, 6, 512, 32, 32, 16, families=("random",))):
        c["xwide"] = True                                                # x is the first half of a tensor twice as wide, NaN behind
        out.append(c)
    for Cin, Cout in ((64, 64), (32, 128)):                              # the input-gradient GEMM of f.2: forward weight as the image
        out.append(_case(WIDE, 1, Cin, Cout, 8, 8, 3, relu=0, tables=False, transposed=1))
    for c in out:
        r = wide_route(c)
        c["name"] = "wide%d-Cin%d-Cout%d-%dx%d-N%d%s%s%s%s%s" % (c["ks"], c["Cin"], c["Cout"], c["H"], c["W"], c["N"], "" if c["relu"] else "-norelu",
                                                                 "" if c["tables"] else "-notables", "-scratch%d" % c["scratch"] if c.get("scratch") else "",
                                                                 "-xwide" if c.get("xwide") else "", "-T" if c.get("transposed") else "")
        c["instance"] = r["kernel"]
    return out


def wide_refusals():
    return [_case(WIDE, 3, 6, 32, 8, 8, 1), _case(WIDE, 3, 6, 64, 3, 6, 1), _case(WIDE, 3, 6, 64, 2, 6, 1), _case(WIDE, 1, 48, 512, 32, 32, 16),
            _case(WIDE, 2, 32, 64, 8, 8, 1), _case(WIDE, 3, 64, 64, 8, 8, 1, transposed=1)]


def first_max_cin(H, W):
    return max(c for c in range(6, 193, 6) if first_supported(c, H, W, 128))


def first_cases():
    out = []
    small = ((8, 8, 2), (16, 16, 1), (4, 32, 3), (2, 64, 2), (1, 128, 3), (2, 128, 2), (4, 16, 3), (16, 8, 1))   # (64,8) (64,16) (64,32) (64,64) (128,128) x2 ...
    for i, (H, W, N) in enumerate(small):
        for j, Cin in enumerate((6, 12, 24, 96)):
            if ((i + j) % 2 == 0 or W == 128) and first_supported(Cin, H, W, 128):
                out.append(_case(FIRST, 3, Cin, 256 if (i + j) % 3 == 0 else 128, H, W, N, fold=(i + j) % 4 != 1, relu=(i + j) % 5 != 2))
    out.append(_case(FIRST, 3, first_max_cin(4, 16), 128, 4, 16, 2, fold=True))                   # the largest window the LDS takes
    out.append(_case(FIRST, 3, first_max_cin(1, 128), 128, 1, 128, 2, fold=True))
    out.append(_case(FIRST, 3, 6, 512, 16, 8, 128, fold=True))                                    # (128,8)  at 16 384 pixels
    out.append(_case(FIRST, 3, 12, 1024, 8, 32, 32, fold=True))                                   # (128,32) at 8 192 pixels, Cout 1024
    out.append(_case(FIRST, 3, 6, 512, 32, 16, 64, fold=True))                                    # (128,16) MB = 2: 32 768 pixels
    out.append(_case(FIRST, 3, 6, 512, 16, 64, 64, fold=True, families=("exact",)))               # (128,64) MB = 4: 65 536 pixels
    for Cin in (12, 24, 48):                                                                      # dg4: transposed image, no ReLU, no fold
        out.append(_case(FIRST, 3, Cin, 128, 8, 8 if Cin != 24 else 16, 3, fold=False, relu=0, transposed=1))
    for c in out:
        r = first_route(c)
        c["name"] = "first-Cin%d-Cout%d-%dx%d-N%d%s%s%s" % (c["Cin"], c["Cout"], c["H"], c["W"], c["N"], "-fold" if c["fold"] else "", "" if c["relu"] else "-norelu",
                                                            "-T" if c.get("transposed") else "")
        c["instance"] = r["kernel"]
        c["MB"] = r["MB"]
    return out


def first_refusals():
    return [_case(FIRST, 3, 5, 128, 8, 8, 1), _case(FIRST, 3, 198, 128, 8, 8, 1), _case(FIRST, 3, 6, 64, 8, 8, 1), _case(FIRST, 3, 6, 128, 8, 12, 1),
            _case(FIRST, 3, first_max_cin(4, 16) + 6, 128, 4, 16, 1), _case(FIRST, 3, first_max_cin(1, 128) + 6, 128, 1, 128, 1), _case(FIRST, 3, 192, 128, 4, 16, 1)]


def direct_cases():
    out = []
    chans = (1, 3, 5, 9, 17)
    maps = ((1, 1), (1, 7), (3, 5), (17, 19))
    epis = ("scale+logs", "scale", "logs", "none")
    i = 0
    for a, Cin in enumerate(chans):
        for b, (H, W) in enumerate(maps):
            Cout = chans[(a + b + 1) % 5]
            for ks in (1, 3):
                epi = epis[(a + b) % 4]                                      # both kernel sizes and every map see every epilogue
                out.append(_case(DIRECT, ks, Cin, Cout, H, W, 3 if i % 3 else 1, relu=(i // 3) % 2, epi=epi, bias=i % 5 != 0, post_bias=i % 3 != 1, xwide=i % 7 == 3,
                                 families=("random",) if epi == "logs" else ("exact", "random")))
                i += 1
    for c in out:
        c["name"] = "direct%d-Cin%d-Cout%d-%dx%d-N%d-%s%s%s%s%s" % (c["ks"], c["Cin"], c["Cout"], c["H"], c["W"], c["N"], c["epi"], "-bias" if c["bias"] else "",
                                                                    "-pbias" if c["post_bias"] else "", "" if c["relu"] else "-norelu", "-xwide" if c["xwide"] else "")
        c["instance"] = direct_route(c)["kernel"]
    return out


def direct_refusals():
    return [_case(DIRECT, 2, 3, 3, 4, 4, 1, epi="none", bias=False, post_bias=False), _case(DIRECT, 5, 3, 3, 4, 4, 1, epi="none", bias=False, post_bias=False)]


def all_cases():
    return wide_cases() + first_cases() + direct_cases()


EXPECTED_INSTANCES = (["k_conv_wide<%d,%d>" % (k, t) for k in (1, 3) for t in (64, 128)] + ["k_conv_wide<3,64>+k_splitk_finish", "k_conv_wide<1,64>+k_splitk_finish",
                      "k_gemm_glds"] + ["k_conv_first<%d,%d>" % bw for bw in ((64, 8), (128, 8), (64, 16), (128, 16), (64, 32), (128, 32), (64, 64), (128, 64),
                                                                             (128, 128))] + ["k_conv_first MB=1", "k_conv_first MB=2", "k_conv_first MB=4",
                                                                                             "k_conv_direct<1>", "k_conv_direct<3>"])


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def build(c, fam):
    """the operands of a case: x (N, Cin, H, W), w in the layout the hook takes, the epilogue tables (absent ones None)"""
    r = rng_of(c["name"], fam)
    N, Cin, Cout, H, W, ks = c["N"], c["Cin"], c["Cout"], c["H"], c["W"], c["ks"]
    wshape = (Cin, Cout, ks, ks) if c.get("transposed") else (Cout, Cin, ks, ks)
    oax = 1 if c.get("transposed") else 0
    row = lambda v: v.reshape([Cout if a == oax else 1 for a in range(4)])
    d = dict(bias=None, post_bias=None, post_scale=None, post_logs=None, fold_bias=None, fold_logs=None)
    if fam == "exact":
        g = np.exp2(r.integers(-12, 4, size=Cout)).astype(f32)
        d["granule"] = g
        d["x"] = r.integers(-7, 8, size=(N, Cin, H, W)).astype(f32)
        d["w"] = r.integers(-7, 8, size=wshape).astype(f32) * row(g)
        tab = lambda: r.integers(-15, 16, size=Cout).astype(f32) * g
        sc = lambda: np.exp2(r.integers(-3, 4, size=Cout)).astype(f32) * r.choice(np.array([-1.0, 1.0], f32), size=Cout)
        logs = lambda: np.zeros(Cout, f32)
    else:
        mag = np.array([1.0, 1e-3, 1e-7])[np.arange(Cout) % 3]
        d["x"] = r.normal(size=(N, Cin, H, W)).astype(f32)
        if ks == 1 and c["op"] == WIDE:      # f.2 reads a ReLU output
            d["x"] *= r.integers(0, 2, size=d["x"].shape).astype(f32)
        d["w"] = (0.05 * r.normal(size=wshape) * row(mag)).astype(f32)
        tab = lambda: (0.1 * r.normal(size=Cout) * mag).astype(f32)
        sc = lambda: np.exp(3.0 * 0.1 * r.normal(size=Cout)).astype(f32)
        logs = lambda: (0.1 * r.normal(size=Cout)).astype(f32)
    if c["op"] == WIDE and c["tables"]:
        d["post_bias"], d["post_scale"] = tab(), sc()
    if c["op"] == FIRST and c["fold"]:
        d["fold_bias"], d["fold_logs"] = tab(), logs()
    if c["op"] == DIRECT:
        if c["bias"]:
            d["bias"] = tab()
        if c["post_bias"]:
            d["post_bias"] = tab()
        if "scale" in c["epi"]:
            d["post_scale"] = sc()
        if "logs" in c["epi"]:
            d["post_logs"] = (0.1 * r.normal(size=Cout)).astype(f32)      # (beside a scale table it is ignored: any value)
    return d


def check_exact(c, d, A):
    """the two conditions of the exact family (A: the reference's sum |w| |x| per element, any subset of the images)"""
    g = d["granule"].astype(f64)
    oax = 1 if c.get("transposed") else 0
    gw = g.reshape([c["Cout"] if a == oax else 1 for a in range(4)])
    assert np.all(d["x"] == np.rint(d["x"])) and np.all(d["w"] / gw == np.rint(d["w"] / gw)), "operands are not integers times the row granule"
    extra = np.zeros(c["Cout"])
    for k in ("bias", "post_bias", "fold_bias"):
        if d[k] is not None:
            assert np.all(d[k] / g == np.rint(d[k] / g))
            extra += np.abs(d[k])
    if d["post_scale"] is not None:
        assert np.all(np.log2(np.abs(d["post_scale"])) == np.rint(np.log2(np.abs(d["post_scale"]))))
    if d["fold_logs"] is not None:
        assert np.all(d["fold_logs"] == 0)
    assert np.all((A + extra[None, :, None]) / g[None, :, None] < 2.0 ** 24), "partial sums may leave the 24-bit range of their granule"


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def effective_weight(c, d, w=None):
    """(Cout, Cin, k, k) float64 weight of the convolution the launch computes"""
    w = np.asarray(d["w"] if w is None else w, f64)
    if c.get("transposed"):
        w = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
    return w


def im2col(x, n, ks, pad="zero"):
    """(Cin k k, HW) float64, row ci k k + tap; pad = "neighbour": the halo rows come from the neighbouring images (a fault)"""
    N, Cin, H, W = x.shape
    if ks == 1:
        return x[n].reshape(Cin, H * W).astype(f64)
    xp = np.zeros((Cin, H + 2, W + 2), f64)
    xp[:, 1:-1, 1:-1] = x[n]
    if pad == "neighbour":
        if n > 0:
            xp[:, 0, 1:-1] = x[n - 1, :, H - 1]
        if n < N - 1:
            xp[:, H + 1, 1:-1] = x[n + 1, :, 0]
    cols = np.empty((Cin, 9, H, W), f64)
    for ky in range(3):
        for kx in range(3):
            cols[:, ky * 3 + kx] = xp[:, ky:ky + H, kx:kx + W]
    return cols.reshape(Cin * 9, H * W)


def conv_sums(x, w, ks, images=None, pad="zero"):
    """(S, A): sum w x and sum |w| |x| per element, float64, shape (len(images), Cout, HW); one image at a time"""
    images = range(x.shape[0]) if images is None else images
    w2 = w.reshape(w.shape[0], -1)
    S = np.empty((len(images), w.shape[0], x.shape[2] * x.shape[3]), f64)
    A = np.empty_like(S)
    for i, n in enumerate(images):
        cols = im2col(x, n, ks, pad)
        S[i] = w2 @ cols
        A[i] = np.abs(w2) @ np.abs(cols)
    return S, A


def epilogue_terms(c, d, S_splits=1):
    """(add (Cout), scale (Cout), count (Cout)): the value added before the scale, the scale, and the roundings beside the K terms"""
    Cout, K = c["Cout"], c["Cin"] * c["ks"] ** 2
    z = np.zeros(Cout)
    v = lambda k: z if d[k] is None else d[k].astype(f64)
    if c["op"] == WIDE:
        return v("post_bias"), (np.ones(Cout) if d["post_scale"] is None else d["post_scale"].astype(f64)), z + K + S_splits - 1 + 2
    if c["op"] == FIRST:
        if d["fold_logs"] is None:
            return z, np.ones(Cout), z + K
        l3 = 3.0 * d["fold_logs"].astype(f64)
        return v("fold_bias"), np.exp(l3), K + 1 + 3 + np.abs(l3)
    cnt = z + K + (d["bias"] is not None) + (d["post_bias"] is not None)
    if d["post_scale"] is not None:
        sc, cnt = d["post_scale"].astype(f64), cnt + 1
    elif d["post_logs"] is not None:
        l3 = 3.0 * d["post_logs"].astype(f64)
        sc, cnt = np.exp(l3), cnt + 3 + np.abs(l3)
    else:
        sc = np.ones(Cout)
    return v("bias") + v("post_bias"), sc, cnt


def finish(c, d, S, A, splits=1, relu_first=False, scale=None, add=None):
    """(ref, bound) from the sums; relu_first / scale / add: the single faults of the host tests"""
    a, sc, cnt = epilogue_terms(c, d, splits)
    absadd = np.zeros(c["Cout"])
    for k in ("bias", "post_bias", "fold_bias"):
        if d[k] is not None:
            absadd = absadd + np.abs(d[k].astype(f64))
    a = a if add is None else add
    sc_used = sc if scale is None else scale
    b3 = lambda t: np.asarray(t, f64)[None, :, None]
    pre = S + b3(a)
    if relu_first and c["relu"]:
        pre = np.maximum(pre, 0.0)
    ref = pre * b3(sc_used)
    if c["relu"]:
        ref = np.maximum(ref, 0.0)
    bound = bnd(U * b3(cnt) * (A + b3(absadd)) * np.abs(b3(sc)))
    return ref, bound


def reference(c, d, images=None, splits=1):
    """(ref, bound, A) of a case, float64 (N or len(images), Cout, HW)"""
    S, A = conv_sums(d["x"], effective_weight(c, d), c["ks"], images)
    ref, bound = finish(c, d, S, A, splits)
    return ref, bound, A


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the promised arithmetic (host tests)
# ---------------------------------------------------------------------------------------------------------------------
def fma_chain(acc, w2, cols, order):
    """acc (Cout, HW) float32 <- the chain acc = fl(acc + w[:, k] cols[k]) over k in `order` (a product of two fp32 numbers is exact in
    fp64, so one rounding per step, as fmaf and the fp32 MFMA have it)"""
    for k in order:
        acc = (acc.astype(f64) + w2[:, k, None].astype(f64) * cols[k][None, :].astype(f64)).astype(f32)
    return acc


def emulate(c, d, images, rt):
    """what the kernels promise, in fp32: products and sums in the kernel's k order, the split-K slices summed in order, the FIRST
    image pre-scaled, the epilogue in the kernel's order.  (len(images), Cout, HW) float32"""
    Cout, Cin, ks = c["Cout"], c["Cin"], c["ks"]
    K = Cin * ks * ks
    w2 = effective_weight(c, d).reshape(Cout, K).astype(f32)
    out = []
    t32 = lambda k, fill: np.full(Cout, fill, f32) if d[k] is None else d[k].astype(f32)
    wimg, start = w2, np.zeros(Cout, f32)
    if c["op"] == FIRST and d["fold_logs"] is not None:      # the image: weights and bias times expf(3 logs), rounded to fp32
        e = np.exp((d["fold_logs"] * f32(3.0)).astype(f32)).astype(f32)
        wimg, start = w2 * e[:, None], d["fold_bias"] * e
    for n in images:
        cols = im2col(d["x"], n, ks).astype(f32)
        zero = np.zeros((Cout, cols.shape[1]), f32)
        if c["op"] == WIDE:
            S, nkt = rt["S"], kpad(Cin, ks) // 32
            parts = [fma_chain(zero, w2, cols, [k for k in range(s * nkt // S * 32, (s + 1) * nkt // S * 32) if k < K]) for s in range(S)]
            acc = parts[0]
            for p in parts[1:]:
                acc = acc + p
            y = (acc + t32("post_bias", 0)[:, None]) * t32("post_scale", 1)[:, None]
        elif c["op"] == FIRST:
            order = [(ch * 6 + cl) * 9 + tap for ch in range(Cin // 6) for tap in range(9) for cl in range(6)]
            y = fma_chain(zero + start[:, None], wimg, cols, order)
        else:
            y = fma_chain(zero, w2, cols, range(K))
            if d["bias"] is not None:
                y = y + d["bias"][:, None]
            if d["post_bias"] is not None:
                y = y + d["post_bias"][:, None]
            if d["post_scale"] is not None:
                y = y * d["post_scale"][:, None]
            elif d["post_logs"] is not None:
                y = y * np.exp((d["post_logs"] * f32(3.0)).astype(f32)).astype(f32)[:, None]
        assert y.dtype == f32
        out.append(np.maximum(y, f32(0)) if c["relu"] else y)
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------------
# single faults (host tests): each returns the faulty output in float64, or None where it does not apply to the case
# ---------------------------------------------------------------------------------------------------------------------
def _with_weight(c, d, images, w, **kw):
    S, A = conv_sums(d["x"], w, c["ks"], images, kw.pop("pad", "zero"))
    return finish(c, d, S, A, **kw)[0]


def fault_ragged_group_dropped(c, d, images, rt):
    """the last, partly filled group of the reduction left out: the ragged k-tile of the wide kernels (K % 32 != 0), the last 6-channel
    chunk of FIRST, the last input channel of DIRECT"""
    w = effective_weight(c, d).copy()
    K = c["Cin"] * c["ks"] ** 2
    if c["op"] == WIDE:
        if K % 32 == 0:
            return None
        w.reshape(c["Cout"], K)[:, K // 32 * 32:] = 0
    elif c["op"] == FIRST:
        w[:, -6:] = 0
    else:
        w[:, -1:] = 0
    return _with_weight(c, d, images, w)


def fault_tap_mirrored(c, d, images, rt):
    """tap 2 (above, right) takes tap 6's weight (below, left): a map of one row or one column only ever sees zeros there"""
    if c["ks"] != 3 or c["H"] < 2 or c["W"] < 2:
        return None
    w = effective_weight(c, d).copy().reshape(c["Cout"], c["Cin"], 9)
    w[:, :, 2] = effective_weight(c, d).reshape(c["Cout"], c["Cin"], 9)[:, :, 6]
    return _with_weight(c, d, images, w.reshape(c["Cout"], c["Cin"], 3, 3))


def fault_w_for_wt(c, d, images, rt):
    """a transposed image read as if the source were (Cout, Cin, k, k)"""
    if not c.get("transposed"):
        return None
    w = d["w"].astype(f64).reshape(c["Cout"], c["Cin"], c["ks"], c["ks"])[:, :, ::-1, ::-1]
    return _with_weight(c, d, images, np.ascontiguousarray(w))


def fault_splitk_slice_skipped(c, d, images, rt):
    if c["op"] != WIDE or rt["S"] < 2:
        return None
    S, nkt, K = rt["S"], kpad(c["Cin"], c["ks"]) // 32, c["Cin"] * c["ks"] ** 2
    w = effective_weight(c, d).copy()
    w.reshape(c["Cout"], K)[:, (S - 1) * nkt // S * 32:] = 0          # the last slice
    return _with_weight(c, d, images, w, splits=S)


def fault_halo_from_neighbour(c, d, images, rt):
    if c["ks"] != 3 or c["N"] < 2:
        return None
    return _with_weight(c, d, images, effective_weight(c, d), pad="neighbour")


def fault_mb_second_tile(c, d, images, rt):
    """the second output-channel tile of a workgroup (MB > 1) computed with the first tile's weights"""
    if c["op"] != FIRST or rt["MB"] < 2:
        return None
    w = effective_weight(c, d).copy()
    w[128:256] = w[0:128]
    return _with_weight(c, d, images, w)


def fault_relu_before_scale(c, d, images, rt):
    if not c["relu"] or c["op"] == FIRST or d["post_scale"] is None or np.all(d["post_scale"] > 0):
        return None
    return _with_weight(c, d, images, effective_weight(c, d), relu_first=True)


def fault_factor3_dropped(c, d, images, rt):
    logs = d["fold_logs"] if c["op"] == FIRST else (d["post_logs"] if d["post_scale"] is None else None)
    if logs is None or np.all(logs == 0):
        return None
    return _with_weight(c, d, images, effective_weight(c, d), scale=np.exp(logs.astype(f64)))


def fault_fold_bias_dropped(c, d, images, rt):
    if c["op"] != FIRST or d["fold_bias"] is None:
        return None
    return _with_weight(c, d, images, effective_weight(c, d), add=np.zeros(c["Cout"]))


FAULTS = dict(ragged_group_dropped=fault_ragged_group_dropped, tap_mirrored=fault_tap_mirrored, w_for_wt=fault_w_for_wt,
              splitk_slice_skipped=fault_splitk_slice_skipped, halo_from_neighbour=fault_halo_from_neighbour, mb_second_tile=fault_mb_second_tile,
              relu_before_scale=fault_relu_before_scale, factor3_dropped=fault_factor3_dropped, fold_bias_dropped=fault_fold_bias_dropped)


def host_images(c):
    """the images the CPU tests look at: all of a small case, the first and the last of a large one"""
    return list(range(c["N"])) if c["N"] * c["H"] * c["W"] * c["Cout"] <= (1 << 18) else sorted({0, c["N"] - 1})


# =====================================================================================================================
# the tail convolution (csrc/conv_mfma_tail.hip k_conv_tail, csrc/conv_mfma_tail_dma.h k_conv_tail_dma and tail_epilogue, k_pack_tail)
# =====================================================================================================================
# 3x3 'SAME' convolution to a few output channels, h = (conv + bias) scale, with the coupling / prior arithmetic of
# network/model.py:105-113, 131-139 and network/module.py:526-536 in the epilogue.  In the paired modes channel 2 c is A (shift / mean)
# and channel 2 c + 1 is B (the sigmoid's argument / logs) of coupling channel c:
#   plain       z2_out = h                                   add_fwd / add_rev   z2_out = z2 + h / z2 - h
#   affine_fwd  s = sigmoid(B + 2); z2_out = (z2 + A) s;  term = + sum log s
#   affine_rev  z2_out = z2 / s - A;                      term = - sum log s
#   split_fwd   term = sum -0.5 (log 2 pi + 2 B + (z2 - A)^2 / exp(2 B));  z2_out (optional) = (z2 - A) exp(-B)
#   split_rev   z2_out = A + exp(B) eps                    (eps passed as z2_in)
#   hout (optional) = h in every mode.  term[n]: the per-sample sum, accumulated in Q31.32 fixed point and finalised to fp32.
#
# BOUNDS (u, expf, bnd() as above; logf as 2 u).  With A_h = sum |w| |x| + |bias| and WK waves sharing the reduction (WK = 1 at 64 and
# 128 pixels per workgroup, 2 at 32, 4 at 16):  e_h = u (9 Cin + WK - 1 + 2) A_h |scale|  bounds h, hence hout and plain.  Below e_A,
# e_B are e_h of the pair's two channels.
#   add          e_h + u (|z2| + |h|)                                                       one addition
#   sigmoid      x = fl(B + 2), s = 1 / (1 + expf(-x)):  relative  r_s = u (2 + (1 - s)(2 + |x|)) + (1 - s) e_B
#   affine_fwd   s (e_A + u (|z2| + |A|)) + |z2 + A| s (r_s + u);        log s:  r_s + 2 u |log s|
#   affine_rev   |z2 / s| (r_s + u) + e_A + u (|z2 / s| + |A|)            -- the division's 1 / s is explicit in |z2 / s|
#   split_fwd    d = fl(z2 - A): e_d = e_A + u |d|;  q = d d / expf(2 B):
#                term  0.5 (2 u + 2 e_B + u |L + 2 B| + 2 |d| e_d / exp(2 B) + q (4 u + 2 e_B) + u |L + 2 B + q|),  L = log 2 pi (2 u: the
#                fp32 constant);  z2_out  exp(-B) e_d + |d| exp(-B) (e_B + 3 u)
#   split_rev    |eps| exp(B) (e_B + 3 u) + e_A + u (|A| + |eps| exp(B))
#   term[n]      the sum of its elements' bounds + 2^-32 per workgroup partial + 2^-50 sum |terms| + u |term| (the fp32 result)
# FAMILIES.  exact: as above, z2 an integer times the row's granule times |scale|, so plain, add_* and hout are exact; the paired modes
# take granules 2^-16 .. 2^-12 and scales 2^-2 .. 1 (arguments of order one) and are held exactly on hout, inside the bound elsewhere.
# random: activations half zeros, weights 0.02 N(0, 1), A rows at 1, 1e-3, 1e-7, the bias of the B rows spread so that the sigmoid's
# argument covers [-6, 6] and the prior's logs [-2, 2].
TAIL = "tail"
MODES = ("plain", "affine_fwd", "affine_rev", "add_fwd", "add_rev", "split_fwd", "split_rev")      # index = TailMode
PAIRED_MODES = ("affine_fwd", "affine_rev", "split_fwd", "split_rev")
LOG_2PI = float(np.log(2.0 * np.pi))
DBG_MSPLIT, DBG_NO_MSPLIT, DBG_NO_DMA = 0x100, 0x200, 0x400


def tail_row_channel(m, Cout, paired):
    """out-row m of the packed image -> output channel, or -1: a lane's four consecutive rows are {A of c0, A of c1, B of c0, B of c1}"""
    if not paired:
        return m if m < Cout else -1
    g, r = m >> 2, m & 3
    c = 2 * g + (r & 1)
    return 2 * c + (r >> 1) if c < Cout // 2 else -1


def tail_mt(Cout, paired):
    rows = 4 * ((Cout // 2 + 1) // 2) if paired else Cout
    return -(-rows // 16)


def tp_ok_reg(tp, H, W):
    return tp % W == 0 and (H * W) % tp == 0 and 32 * (tp // W + 2) * (W // 4) <= 6 * 256


def tp_ok_dma(tp, H, W, Cin, no_dma):
    if no_dma or Cin % 16 or Cin < 32 or W not in (8, 16, 32, 64, 128) or tp % W or (H * W) % tp:
        return False
    xf = -(-16 * first_chs(tp // W, W) // 256) * 256
    return (3 * (xf + 4 * 9 * 64) + 264) * 4 <= 150 * 1024


def tail_supported(Cin, H, W, Cout, no_dma=False):
    return W % 4 == 0 and W >= 8 and 1 <= Cout <= 1024 and Cin >= 1 and any(tp_ok_reg(tp, H, W) or tp_ok_dma(tp, H, W, Cin, no_dma) for tp in (128, 64, 32, 16))


def tail_choose(H, W, px, Cin, mt_total, force_tp, force_ms, no_dma):
    """the launcher's two-term cost model, statement for statement: (pixels per workgroup, out-channel split)"""
    best, best_cost = (0, 0), 1e30
    ok = lambda tp: tp_ok_reg(tp, H, W) or tp_ok_dma(tp, H, W, Cin, no_dma)
    for ms in (0, 1):
        if ms == 1 and mt_total == 1:
            continue
        if force_ms >= 0 and ms != force_ms and mt_total > 1:
            continue
        for tp in (128, 64, 32, 16):
            reg, dma = tp_ok_reg(tp, H, W), tp_ok_dma(tp, H, W, Cin, no_dma)
            if not (reg or dma):
                continue
            mt_blk = 1 if ms else mt_total
            if mt_blk > 3 or (not reg and mt_blk != 1):
                continue
            if force_tp and tp != force_tp and ok(force_tp):
                continue
            wk, ntw = (1 if tp >= 64 else (2 if tp == 32 else 4)), (2 if tp == 128 else 1)
            blocks = float(px // tp) * (mt_total if ms else 1)
            per_cu = 1.0 if blocks <= 256 else blocks / 256.0
            mfma = per_cu * ntw * mt_blk * ((Cin + 3) // 4 * 9.0 / wk) * 32.0
            stream = per_cu * float(Cin) * 9 * mt_blk * 64 / 10.0
            cost = mfma if mfma > stream else stream
            if blocks < 512:
                cost *= 1.15
            if blocks < 256:
                cost *= 2.0
            cost += 1e-3 * stream
            if cost < best_cost:
                best_cost, best = cost, (tp, ms)
    return best


def tail_route(c):
    """what launch_conv_mfma_tail picks under the case's switches, or dict(refused=True)"""
    N, Cin, Cout, H, W = c["N"], c["Cin"], c["Cout"], c["H"], c["W"]
    fl = c.get("flags", 0)
    no_dma = bool(fl & DBG_NO_DMA)
    paired = c["mode"] in PAIRED_MODES
    if not tail_supported(Cin, H, W, Cout, no_dma) or (paired and Cout % 2):
        return dict(refused=True)
    mtt = tail_mt(Cout, paired)
    tp, ms = tail_choose(H, W, N * H * W, Cin, mtt, fl & 0xff, 1 if fl & DBG_MSPLIT else (0 if fl & DBG_NO_MSPLIT else -1), no_dma)
    if tp == 0 or not (tp_ok_reg(tp, H, W) or c.get("zeros")):
        return dict(refused=True)
    MT, Y = (1, mtt) if ms else (mtt, 1)
    dma = MT == 1 and bool(c.get("zeros")) and tp_ok_dma(tp, H, W, Cin, no_dma)
    return dict(kernel=("k_conv_tail_dma<TP=%d,W=%d>" % (tp, W)) if dma else "k_conv_tail<MT=%d,TP=%d>" % (MT, tp), dma=dma, tile=tp, MT=MT,
                WK=1 if tp >= 64 else (2 if tp == 32 else 4), grid=[N * H * W // tp, Y, 1], paired=int(paired), launches=1,
                image_bytes=-(-Cin // 32) * 8 * 9 * max(tail_mt(Cout, 1), tail_mt(Cout, 0)) * 64 * 4)


def _tail(mode, Cin, Cout, H, W, N, tp=0, ms=None, **kw):
    fl = tp | (0 if ms is None else (DBG_MSPLIT if ms else DBG_NO_MSPLIT))
    c = dict(op=TAIL, ks=3, mode=mode, Cin=Cin, Cout=Cout, H=H, W=W, N=N, relu=0, flags=fl, zeros=False, hout=True, z2wide=False, z2out=True, tables=True,
             families=("exact", "random"))
    c.update(kw)
    if kw.get("no_dma"):
        c["flags"] |= DBG_NO_DMA
    return c


def tail_cases():
    out = []
    i = 0
    for mode in MODES:                                       # every mode x forced tile x out-channel split, register-staged
        for tp in (16, 32, 64, 128):
            for ms in (1, 0):
                out.append(_tail(mode, 64, 24 if mode in PAIRED_MODES else 17, 8, 16, 3, tp, ms, hout=i % 2 == 0, z2wide=i % 3 == 0))
                i += 1
    for Cin in (6, 12, 24):                                  # the Split2d priors: Cout = 2 Cin (MT 1, 2, 3)
        for j, mode in enumerate(("split_fwd", "split_rev")):
            out.append(_tail(mode, Cin, 2 * Cin, 8, 8, 3 - 2 * j, (16, 32, 64)[(Cin // 6 + j) % 3], 0, z2out=Cin != 12))
    for j, Cin in enumerate((33, 100, 5, 96)):               # ragged group, ragged chunk, whole chunks (64: the twins below)
        for k, mode in enumerate(("affine_fwd", "add_rev", "plain", "affine_rev")):
            out.append(_tail(mode, Cin, 12 if mode in PAIRED_MODES else 6, 8, 8, 1 + 2 * ((j + k) % 2), (16, 32, 64)[(j + k) % 3], hout=(j + k) % 2 == 1))
    for Cout in (2, 10, 12, 24, 48, 96):                     # paired row groups: half empty, MT 1, 2, 3, six tiles (split forced)
        out.append(_tail("affine_fwd", 8, Cout, 4, 8, 3, 32))
        out.append(_tail("split_rev", 7, Cout, 4, 8, 1, 16, hout=False))
    for Cout in (1, 6, 17, 56):                              # unpaired
        out.append(_tail("add_fwd", 9, Cout, 4, 8, 3, 32))
        out.append(_tail("plain", 4, Cout, 2, 16, 1, 16))
    geo = {8: (16, 8), 16: (8, 16), 32: (4, 32), 64: (2, 64), 128: (1, 128)}
    i = 0
    for W, (H, _) in geo.items():                            # the LDS-DMA kernel: every width, ring of 2, 3, 5 chunks and more
        for Cin in (32, 48, 64, 80):
            tps = [tp for tp in (16, 32, 64, 128) if tp_ok_dma(tp, H, W, Cin, False)]
            mode = MODES[1 + i % 6]
            out.append(_tail(mode, Cin, 12, H, W, 3 if i % 2 else 1, tps[i % len(tps)], zeros=True, hout=i % 2 == 0, z2wide=i % 3 == 1))
            i += 1
    out.append(_tail("affine_fwd", 512, 12, 8, 8, 3, 64, zeros=True))                   # the real width
    out.append(_tail("split_fwd", 512, 24, 8, 8, 1, 16, 1, zeros=True))
    out.append(_tail("plain", 64, 17, 8, 16, 3, 32, 1, zeros=True))                     # out-channel split over DMA blocks
    for tp in (16, 64):                                      # the same operands without the zero block / under NO_DMA: the register kernel
        out.append(_tail("affine_fwd", 64, 12, 8, 8, 3, tp, zeros=False, twin=True))
        out.append(_tail("affine_fwd", 64, 12, 8, 8, 3, tp, zeros=True, twin=True))
        out.append(_tail("affine_fwd", 64, 12, 8, 8, 3, tp, zeros=True, no_dma=True, twin=True))
    out.append(_tail("split_fwd", 12, 24, 8, 8, 3, 64, 0, z2out=False, acc=False))      # nothing but hout
    out.append(_tail("affine_rev", 48, 8, 16, 16, 2, 0, tables=False))                  # the cost model's own choice, no tables
    for c in out:
        r = tail_route(c)
        c["name"] = "tail-%s-Cin%d-Cout%d-%dx%d-N%d-f%x%s%s%s%s%s%s" % (c["mode"], c["Cin"], c["Cout"], c["H"], c["W"], c["N"], c["flags"], "-zeros" if c["zeros"] else "",
                                                                       "-hout" if c["hout"] else "", "-z2wide" if c["z2wide"] else "", "" if c["z2out"] else "-noz2out",
                                                                       "" if c["tables"] else "-notables", "" if c.get("acc", True) else "-noacc")
        assert not r.get("refused"), c["name"]
        c["instance"] = r["kernel"]
    return out


def tail_refusals():
    return [_tail("plain", 8, 6, 8, 6, 1), _tail("plain", 8, 6, 8, 10, 1), _tail("affine_fwd", 8, 7, 8, 8, 1), _tail("split_rev", 8, 13, 8, 8, 1),
            _tail("plain", 32, 6, 1, 128, 1), _tail("plain", 32, 6, 2, 64, 1, 128), _tail("plain", 32, 6, 1, 128, 1, zeros=True, no_dma=True)]


def tail_expected_instances():
    return sorted({c["instance"] for c in tail_cases()})


def build_tail(c, fam):
    r = rng_of(c["name"] if not c.get("twin") else ("twin", c["Cin"], c["flags"] & 0xff), fam)
    N, Cin, Cout, H, W, mode = c["N"], c["Cin"], c["Cout"], c["H"], c["W"], c["mode"]
    paired = mode in PAIRED_MODES
    Cz = Cout // 2 if paired else Cout
    d = dict(bias=None, post_bias=None, post_scale=None, post_logs=None, fold_bias=None, fold_logs=None)
    if fam == "exact":
        g = np.exp2(r.integers(-16, -11, size=Cout) if paired else r.integers(-12, 4, size=Cout)).astype(f32)
        sc = np.exp2(r.integers(-2, 1, size=Cout)).astype(f32) if paired else np.exp2(r.integers(-3, 4, size=Cout)).astype(f32) * r.choice(np.array([-1.0, 1.0], f32), size=Cout)
        d["granule"] = g
        d["x"] = r.integers(-7, 8, size=(N, Cin, H, W)).astype(f32)
        d["w"] = r.integers(-7, 8, size=(Cout, Cin, 3, 3)).astype(f32) * g[:, None, None, None]
        bias = r.integers(-15, 16, size=Cout).astype(f32) * g
        if not c["tables"]:
            sc = np.ones(Cout, f32)
        zg = (g * np.abs(sc))[0::2] if paired else g * np.abs(sc)
        d["z2"] = r.integers(-15, 16, size=(N, Cz, H * W)).astype(f32) * (np.ones(Cz, f32) if paired else zg)[None, :, None]
    else:
        mag = np.array([1.0, 1e-3, 1e-7])[np.arange(Cout) % 3] if not paired else np.where(np.arange(Cout) % 2 == 0, np.array([1.0, 1e-3, 1e-7])[(np.arange(Cout) // 2) % 3], 1.0)
        d["x"] = (r.normal(size=(N, Cin, H, W)) * r.integers(0, 2, size=(N, Cin, H, W))).astype(f32)
        d["w"] = (0.02 * r.normal(size=(Cout, Cin, 3, 3)) * mag[:, None, None, None]).astype(f32)
        bias = 0.1 * r.normal(size=Cout) * mag
        if paired and c["tables"]:
            lo, hi = (-8.0, 4.0) if mode.startswith("affine") else (-2.0, 2.0)
            bias[1::2] = r.uniform(lo, hi, size=Cout // 2)
        bias = bias.astype(f32)
        sc = np.exp(3.0 * 0.1 * r.normal(size=Cout)).astype(f32)
        if paired:
            sc[1::2] = 1.0 + 0.05 * r.normal(size=Cout // 2).astype(f32)
        d["z2"] = r.normal(size=(N, Cz, H * W)).astype(f32)
    if c["tables"]:
        d["bias"], d["post_scale"] = bias, sc.astype(f32)
    return d


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def tail_reference(c, d, rt, w=None, pad="zero", plus2=2.0, swap_rows=False, images=None):
    """{output: (ref, bound)} for hout (N, Cout, HW), z2_out (N, Cz, HW) and term (N); the keyword arguments are the host tests' faults"""
    N, Cin, Cout, HW, mode = c["N"], c["Cin"], c["Cout"], c["H"] * c["W"], c["mode"]
    paired = mode in PAIRED_MODES
    S, A = conv_sums(d["x"], (d["w"] if w is None else w).astype(f64), 3, images, pad)
    if swap_rows:      # the image packed with the pair's rows exchanged, the epilogue's map as it is
        rows = tail_mt(Cout, paired) * 16
        perm = np.arange(Cout)
        for m in range(rows):
            g, r = m >> 2, m & 3
            cc = 2 * g + (r >> 1)
            packed = (2 * cc + (r & 1)) if cc < Cout // 2 else -1
            epi = tail_row_channel(m, Cout, paired)
            if epi >= 0:
                perm[epi] = packed if packed >= 0 else epi
        S, A = S[:, perm], A[:, perm]
    b3 = lambda k, fill: np.full(Cout, fill)[None, :, None] if d[k] is None else d[k].astype(f64)[None, :, None]
    bias, sc = b3("bias", 0.0), b3("post_scale", 1.0)
    h = (S + bias) * sc
    eh = U * (9 * Cin + rt["WK"] - 1 + 2) * (A + np.abs(bias)) * np.abs(sc)
    out = dict(hout=(h, bnd(eh)))
    z = d["z2"].astype(f64) if images is None else d["z2"].astype(f64)[list(images)]
    term = eterm = None
    if mode == "plain":
        out["z2_out"] = (h, bnd(eh))
    elif mode in ("add_fwd", "add_rev"):
        out["z2_out"] = (z + h if mode == "add_fwd" else z - h, bnd(eh + U * (np.abs(z) + np.abs(h))))
    else:
        Av, Bv, eA, eB = h[:, 0::2], h[:, 1::2], eh[:, 0::2], eh[:, 1::2]
        if mode.startswith("affine"):
            x = Bv + plus2
            s = _sigmoid(x)
            rs = U * (2 + (1 - s) * (2 + np.abs(x))) + (1 - s) * eB
            if mode == "affine_fwd":
                out["z2_out"] = ((z + Av) * s, bnd(s * (eA + U * (np.abs(z) + np.abs(Av))) + np.abs(z + Av) * s * (rs + U)))
                term = np.log(s)
            else:
                q = z / s
                out["z2_out"] = (q - Av, bnd(np.abs(q) * (rs + U) + eA + U * (np.abs(q) + np.abs(Av))))
                term = -np.log(s)
            eterm = rs + 2 * U * np.abs(np.log(s))
        elif mode == "split_fwd":
            dl = z - Av
            ed = eA + U * np.abs(dl)
            e2 = np.exp(2 * Bv)
            q = dl * dl / e2
            term = -0.5 * (LOG_2PI + 2 * Bv + q)
            eterm = 0.5 * (2 * U + 2 * eB + U * np.abs(LOG_2PI + 2 * Bv) + 2 * np.abs(dl) * ed / e2 + q * (4 * U + 2 * eB) + U * np.abs(LOG_2PI + 2 * Bv + q))
            out["z2_out"] = (dl * np.exp(-Bv), bnd(np.exp(-Bv) * ed + np.abs(dl) * np.exp(-Bv) * (eB + 3 * U)))
        else:
            t = np.abs(z) * np.exp(Bv)
            out["z2_out"] = (Av + np.exp(Bv) * z, bnd(t * (eB + 3 * U) + eA + U * (np.abs(Av) + t)))
    if term is not None:
        T = term.sum(axis=(1, 2))
        partials = (HW // rt["tile"]) * rt["grid"][1]
        out["term"] = (T, bnd(eterm.sum(axis=(1, 2)) + 2.0 ** -32 * partials + 2.0 ** -50 * np.abs(term).sum(axis=(1, 2)) + U * np.abs(T)))
    return out


def tail_k_order(Cin, WK, dma):
    """per wave of the K-split, the (tap, channel) terms in the kernel's order: chunks of 32 channels (16 in the DMA kernel), inside a chunk
    tap-major over the wave's groups of four channels"""
    ck = 16 if dma else 32
    orders = []
    for wk in range(WK):
        o = []
        for ch in range(-(-Cin // ck)):
            left = Cin - ch * ck
            nc4 = ck // 4 if left >= ck else (left + 3) // 4
            for tap in range(9):
                for c4 in range(wk, nc4, WK):
                    o += [(ch * ck + c4 * 4 + kq) * 9 + tap for kq in range(4) if ch * ck + c4 * 4 + kq < Cin]
        orders.append(o)
    return orders


def emulate_tail(c, d, rt):
    """the tail kernels' promised arithmetic in fp32: the WK partial sums in their k order, merged in order, the epilogue as written"""
    N, Cin, Cout, mode = c["N"], c["Cin"], c["Cout"], c["mode"]
    w2 = d["w"].reshape(Cout, Cin * 9).astype(f32)
    orders = tail_k_order(Cin, rt["WK"], rt["dma"])
    assert sorted(k for o in orders for k in o) == list(range(Cin * 9))
    one = f32(1.0)
    bias = np.zeros(Cout, f32) if d["bias"] is None else d["bias"]
    sc = np.ones(Cout, f32) if d["post_scale"] is None else d["post_scale"]
    hs, zs, terms = [], [], []
    for n in range(N):
        cols = im2col(d["x"], n, 3).astype(f32)
        parts = [fma_chain(np.zeros((Cout, cols.shape[1]), f32), w2, cols, o) for o in orders]
        acc = parts[0]
        for p in parts[1:]:
            acc = acc + p
        h = (acc + bias[:, None]) * sc[:, None]
        z = d["z2"][n]
        t = None
        if mode == "plain":
            zo = h
        elif mode in ("add_fwd", "add_rev"):
            zo = z + h if mode == "add_fwd" else z - h
        else:
            Av, Bv = h[0::2], h[1::2]
            if mode.startswith("affine"):
                s = one / (one + np.exp(-(Bv + f32(2.0))))
                zo = (z + Av) * s if mode == "affine_fwd" else z / s - Av
                t = np.log(s).astype(f64) * (1 if mode == "affine_fwd" else -1)
            elif mode == "split_fwd":
                dl = z - Av
                t = (f32(-0.5) * (f32(LOG_2PI) + f32(2.0) * Bv + (dl * dl) / np.exp(f32(2.0) * Bv))).astype(f64)
                zo = dl * np.exp(-Bv)
            else:
                zo = Av + np.exp(Bv) * z
        assert h.dtype == f32 and zo.dtype == f32
        hs.append(h)
        zs.append(zo)
        terms.append(0.0 if t is None else float(f32(t.sum())))
    return dict(hout=np.stack(hs), z2_out=np.stack(zs), term=np.array(terms))


# the tail's single faults: each returns {output: faulty float64 array}, or None where it does not apply
def tfault_ragged_group_dropped(c, d, rt):
    """Cin % 4 != 0: the last, partly filled group of four channels; else Cin % 32 != 0: the last, partly filled chunk"""
    Cin = c["Cin"]
    if Cin % 32 == 0 or rt["dma"]:
        return None
    w = d["w"].copy()
    w[:, (Cin // 4 * 4 if Cin % 4 else Cin // 32 * 32):] = 0
    return tail_reference(c, d, rt, w=w)


def tfault_wk_partial_skipped(c, d, rt):
    if rt["WK"] < 2 or c["Cin"] < 8:
        return None
    w = d["w"].copy().reshape(c["Cout"], -1)
    w[:, tail_k_order(c["Cin"], rt["WK"], rt["dma"])[1]] = 0
    return tail_reference(c, d, rt, w=w.reshape(d["w"].shape))


def tfault_tap_mirrored(c, d, rt):
    if c["H"] < 2:
        return None
    w = d["w"].copy().reshape(c["Cout"], c["Cin"], 9)
    w[:, :, 2] = d["w"].reshape(c["Cout"], c["Cin"], 9)[:, :, 6]
    return tail_reference(c, d, rt, w=w.reshape(d["w"].shape))


def tfault_halo_from_neighbour(c, d, rt):
    return tail_reference(c, d, rt, pad="neighbour") if c["N"] >= 2 else None


def tfault_paired_rows_swapped(c, d, rt):
    return tail_reference(c, d, rt, swap_rows=True) if c["mode"] in PAIRED_MODES and c["Cout"] >= 4 else None


def tfault_plus2_dropped(c, d, rt):
    return tail_reference(c, d, rt, plus2=0.0) if c["mode"].startswith("affine") else None


TAIL_FAULTS = dict(ragged_group_dropped=tfault_ragged_group_dropped, wk_partial_skipped=tfault_wk_partial_skipped, tap_mirrored=tfault_tap_mirrored,
                   halo_from_neighbour=tfault_halo_from_neighbour, paired_rows_swapped=tfault_paired_rows_swapped, plus2_dropped=tfault_plus2_dropped)


def tail_outputs(c):
    """the outputs a case produces"""
    keys = (["hout"] if c["hout"] else []) + (["z2_out"] if c["z2out"] or c["mode"] != "split_fwd" else [])
    return keys + (["term"] if c.get("acc", True) and c["mode"] in ("affine_fwd", "affine_rev", "split_fwd") else [])


def tail_exact_outputs(c):
    """the outputs an exact set holds value for value"""
    return ("hout", "z2_out") if c["mode"] in ("plain", "add_fwd", "add_rev") else ("hout",)

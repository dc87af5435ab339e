"""Host side of the invconv LU tests (numpy only): seeded matrix families that FORCE the pivoting decisions of csrc/lu.hip and
csrc/lu_wave.h, their fp64 references, the bounds the kernels are held to, and the table of routes.

The reference computes log|det W| as log|torch.det(W)| and W^-1 as W.inverse(), both in fp32 (network/module.py:356-365).  That is
NOT the yardstick here: the fp32 `det` is a PRODUCT of pivots and is +-inf on `sign` from C = 64 and 0 on `tiny` from C = 24, and
an fp32 inverse carries ~1e-5 of its own.  The yardstick is numpy.linalg.slogdet / numpy.linalg.inv on the float32 matrix widened
(exactly) to float64 -- the kernels work in fp64 and store fp32, so they can be held to one fp32 ulp of it.  tests/test_lu_oracle_host.py
keeps that yardstick honest against an independent long-double Gauss-Jordan.

Every family is a function (C, seed) -> float32 (C, C)."""
import numpy as np

LN2 = float(np.log(2.0))
COND_MAX = 2e4          # every matrix the tests use: cond_2(W) <= COND_MAX (checked on the host)


def _rs(C, seed, salt):
    return np.random.RandomState((seed * 1000003 + C * 101 + salt) % (2 ** 31))


def _signed_pow2(rs, n):
    """n values +-2^k, k in -3..3 (float64, exact in float32); also returns k."""
    k = rs.randint(-3, 4, size=n)
    s = rs.randint(0, 2, size=n) * 2 - 1
    return s * np.exp2(k.astype(np.float64)), k


def orth(C, seed):
    """qr(randn) + 0.05 randn: the matrix every other test of the suite uses; any non-zero pivot factors it.  The baseline."""
    rs = _rs(C, seed, 1)
    return (np.linalg.qr(rs.randn(C, C))[0] + 0.05 * rs.randn(C, C)).astype(np.float32)


def cyclic(C, seed):
    """W[i, (i+1) % C] = +-2^k, zero elsewhere.  At EVERY elimination step the only non-zero of column k at or below the diagonal
    is in the last row: every step swaps, the pivot lies beyond the first 64-row trip of the search and in the last panel.  All
    arithmetic is exact: log|det| = ln 2 * sum k, W^-1 has one entry 1 / W[i, (i+1) % C] per row (cyclic_exact)."""
    v, _ = _signed_pow2(_rs(C, seed, 2), C)
    W = np.zeros((C, C), np.float32)
    W[np.arange(C), (np.arange(C) + 1) % C] = v
    return W


def cyclic_exact(C, seed):
    """(log|det|, W^-1) of cyclic(C, seed) in closed form (float64; every entry is a power of two)."""
    v, k = _signed_pow2(_rs(C, seed, 2), C)
    inv = np.zeros((C, C), np.float64)
    inv[(np.arange(C) + 1) % C, np.arange(C)] = 1.0 / v
    return LN2 * float(k.sum()), inv


def anti(C, seed):
    """Scaled anti-diagonal +-2^k plus 1e-3 randn: the pivot of column k comes from the mirrored row C-1-k, so the swaps of the
    first half reach across every panel border."""
    rs = _rs(C, seed, 3)
    v, _ = _signed_pow2(rs, C)
    W = 1e-3 * rs.randn(C, C)
    W[np.arange(C), C - 1 - np.arange(C)] += v
    return W.astype(np.float32)


def sign(C, seed):
    """Every entry +-1: the first column is a C-way tie (the lowest-row rule), elements grow under elimination, log|det| reaches
    ~1337 at C = 512 and the fp32 `det` is +-inf from C = 64.  Redrawn (same stream) until cond_2 <= COND_MAX / 2: a small +-1
    matrix is singular with noticeable probability."""
    rs = _rs(C, seed, 4)
    while True:
        W = (rs.randint(0, 2, size=(C, C)) * 2 - 1).astype(np.float32)
        if np.linalg.cond(W.astype(np.float64)) <= COND_MAX / 2:
            return W


def graded(C, seed):
    """U diag(logspace(-2, 2, C)) V^T, condition number 1e4; log|det| ~ 0, so the ABSOLUTE floor of the bound decides."""
    rs = _rs(C, seed, 5)
    U, V = np.linalg.qr(rs.randn(C, C))[0], np.linalg.qr(rs.randn(C, C))[0]
    return ((U * np.logspace(-2.0, 2.0, C)) @ V.T).astype(np.float32)


def tiny(C, seed):
    """1e-3 qr(randn): log|det| = -6.9 C; `det` underflows fp32 from C = 24 and fp64 from C = 128 -- only a sum of log-pivots survives."""
    return (1e-3 * np.linalg.qr(_rs(C, seed, 6).randn(C, C))[0]).astype(np.float32)


FAMILIES = dict(orth=orth, cyclic=cyclic, anti=anti, sign=sign, graded=graded, tiny=tiny)
ALL = tuple(FAMILIES)
LARGE = ("cyclic", "sign", "orth")      # the families run above C = 200 (a C = 512 Gauss-Jordan is hundreds of ms on the GPU)
SEED = 7

_cache = {}


def matrix(family, C, seed=SEED):
    """The float32 matrix of (family, C, seed); cached, returned read-only."""
    key = (family, C, seed)
    if key not in _cache:
        W = FAMILIES[family](C, seed)
        W.setflags(write=False)
        _cache[key] = W
    return _cache[key]


_ref_cache = {}


def reference(family, C, seed=SEED):
    """(log|det W|, W^-1) in float64 of the float32 matrix: numpy.linalg.slogdet / inv.  Computed once, read-only."""
    key = (family, C, seed)
    if key not in _ref_cache:
        W = matrix(family, C, seed).astype(np.float64)
        inv = np.linalg.inv(W)
        inv.setflags(write=False)
        _ref_cache[key] = (float(np.linalg.slogdet(W)[1]), inv)
    return _ref_cache[key]


def longdouble_gauss_jordan(W):
    """Independent yardstick for the yardstick: Gauss-Jordan with partial pivoting on [W | I] in np.longdouble (x87 80-bit where
    numpy has it).  Returns (log|det|, W^-1) as longdouble."""
    C = W.shape[0]
    A = np.zeros((C, 2 * C), np.longdouble)
    A[:, :C] = W
    A[np.arange(C), C + np.arange(C)] = 1
    logdet = np.longdouble(0)
    for k in range(C):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
        logdet += np.log(np.abs(A[k, k]))
        A[k] /= A[k, k]
        col = A[:, k].copy()
        col[k] = 0
        A -= col[:, None] * A[k][None, :]
    return logdet, A[:, C:]


# ---- bounds (derived from the arithmetic, DESIGN.md "LU routes against fp64"; never tuned on a GPU)
ULP = 2.0 ** -23        # one fp32 ulp, relative: 2^-24 is the store of the fp64 result, the other half covers the fp64 factorisation


def logdet_bound(ref):
    """|lad - ref| <= 2^-23 |ref| + 1e-9 (stand-alone call, and ld_out / HW through a plan with HW a power of two)."""
    return ULP * abs(ref) + 1e-9


def inverse_bound(ref_inv):
    """Elementwise |winv - ref| <= 2^-23 |ref| + 2^-24 * 1e-2 * max|ref|."""
    return ULP * np.abs(ref_inv) + 2.0 ** -24 * 1e-2 * np.abs(ref_inv).max()


def apply_bound(M, v, products_ulp=2.0 ** -24, extra=0.0):
    """Elementwise bound on |fl(M v) - M v| for an fp32 matrix M (C x C) applied to fp32 pixels v (C x P) with ANY accumulation
    order: (C + 2) u (|M| |v|), u = 2^-24 -- C - 1 additions and one product rounding per term (<= C u to first order), one u for
    the rounding of the stored matrix entry against its fp64 value, one for the output store.  `products_ulp` replaces the product
    rounding where the products are not fp32 (split-fp16 GEMM), `extra` adds a relative term on top."""
    C = M.shape[0]
    return ((C + 1) * 2.0 ** -24 + products_ulp + extra) * (np.abs(M).astype(np.float64) @ np.abs(v).astype(np.float64))


def apply_bound_sh2(M, v):
    """The same for a mixer on the split-fp16 GEMM (csrc/dnet_sh.hip), derived from csrc/sh.h "SH2".  Both operands are scaled by
    an exact power of two and carried as hi + lo (two fp16 numbers): |V - hi - lo| <= max(2^-22 |V|, 2^-25); a product is
    hi*hi + hi*lo + lo*hi, each exact in the fp32 accumulator, the lo*lo term (<= 2^-22 |a b|) dropped.  Per output:
      3 * 2^-22 (|M| |v|)        the two splits and the dropped term -- the "22-bit products";
      3 C * 2^-23 (|M| |v|)      3 C exact products summed in fp32 in the matrix pipe's order; 2^-23 per addition also covers an
                                 accumulator that truncates (sh.h does not state its rounding);
      2 * 2^-24 (|M| |v|)        the stored matrix entry against its fp64 value, the output store;
      2^-37 max_k |M_ok| sum_k |v_k|    the weights' absolute floor: 2^-25 at a row scale that puts the row's largest entry in [2^12, 2^13);
      2^-29 sum_k |M_ok|                the activations' floor: 2^-25 at the fixed scale 2^4."""
    from sh2_oracle import bound_sh2      # (the one SH2 bound: the coupling-network kernels are held to the same function layer by layer)
    aM, av = np.abs(M).astype(np.float64), np.abs(v).astype(np.float64)
    return bound_sh2(aM @ av, M.shape[0], aM.max(axis=1)[:, None] * av.sum(axis=0)[None, :], aM.sum(axis=1)[:, None])


# ---- routes.  Names are the launch counters of glowhip_plan_launch_counts (csrc/plan_build.hip glowhip_plan_pack_for; csrc/lu.hip
# step_prepare_route_name).  The GPU tests ASSERT these from the counters; the widths below are where each route is exercised.
FUSED, SMALL, BATCHED = "pack:k_pack_fused", "pack:k_step_prepare_small", "pack:k_step_prepare_batched"
R_LDS, R_BLOCKED, R_GLOBAL = "pack:lu:logdet_only(lds)", "pack:lu:logdet_blocked", "pack:lu:logdet_only(global)"
R_GJ_LDS, R_GJ_GLOBAL = "pack:lu:gauss_jordan(lds)", "pack:lu:gauss_jordan(global)"

WAVE_C = (12, 24, 48)                       # route 1: lu_logdet_wave (k_pack_fused, k_step_prepare_small)
FORWARD_ROUTES = {                          # routes 2 and 3, forward-only pack: counter -> widths
    R_LDS: (16, 64, 66, 96, 128),
    R_BLOCKED: (130, 160, 200, 448),        # 160: full panels only; 130: a 2-column last panel; 448: the widest it takes
    R_GLOBAL: (450, 512),
}
STANDALONE_C = {"lds": (1, 3, 12, 48, 64), "global": (66, 96, 130, 200, 384, 512)}   # routes 4 and 5 (lu.hip launch_invconv_prepare)
INVERSE_PACK_C = (12, 48, 64, 66, 200, 384)
INVERSE_PACK_FAMILIES = ("cyclic", "anti", "sign")
MIXED = ((12, "graded"), (24, "tiny"), (48, "anti"), (96, "sign"), (192, "cyclic"), (384, "orth"))   # one launch, six widths
MANY_STEPS_FAMILIES = ALL                    # > 256 FlowSteps of width 12: the families in turn


def families_for(C):
    return ALL if C <= 200 else LARGE


def standalone_cases():
    return [(f, C) for Cs in STANDALONE_C.values() for C in Cs for f in families_for(C)]


def forward_cases():
    """(family, C, counter) of the forward-only pack tests beyond the one-wave widths."""
    return [(f, C, r) for r, Cs in FORWARD_ROUTES.items() for C in Cs for f in families_for(C)]


def host_checked_cases():
    """Every (family, C) the GPU file uses up to C = 200, and `sign` / `graded` at C = 512 (a long-double elimination at C = 512
    takes seconds: two families go that far)."""
    cs = set(WAVE_C) | {C for Cs in FORWARD_ROUTES.values() for C in Cs} | {C for Cs in STANDALONE_C.values() for C in Cs}
    cs |= set(INVERSE_PACK_C) | {C for C, _ in MIXED}
    return [(f, C) for C in sorted(cs) if C <= 200 for f in ALL] + [("sign", 512), ("graded", 512)]

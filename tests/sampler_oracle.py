"""numpy restatement of the sampler's random stream (include/glowhip.h "The sampler's random stream", csrc/sampler_rng.h):
uint64 Philox4x32-10, fp64 Box-Muller.  Written from the definition, independent of the HIP code.

    key      = the 64-bit seed
    counter  of the group of four elements 4j .. 4j+3 of stream s at call c:
               c0 = j & 0xffffffff, c1 = j >> 32, c2 = c & 0xffffffff, c3 = ((s + 1) << 24) | ((c >> 32) & 0xffffff)
    stream   0 = the top latent, 1 + k = the k-th Split2d in decode order
    normals  (w0, w1) -> elements 0, 1; (w2, w3) -> elements 2, 3:
               u1 = ((w >> 9) + 0.5) 2^-23, u2 = (w' >> 8) 2^-24, r = sqrt(-2 ln u1), e = r cos(2 pi u2), e' = r sin(2 pi u2)
    value    e * std
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
MAX_ABS = float(np.sqrt(48.0 * np.log(2.0)))      # u1 >= 2^-24: |e| <= sqrt(-2 ln 2^-24) = 5.768...


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or scalars) holding 32-bit words, key: two 32-bit ints -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = p1 & MASK, p0 & MASK, n0, n2
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c0, c1, c2, c3


def sampler_counter(j, call, stream):
    """The Philox counter (four 32-bit words as Python ints / uint64 arrays) of group j."""
    j = np.asarray(j, dtype=np.uint64)
    call = int(call)
    return (j & MASK, j >> np.uint64(32), np.uint64(call & 0xffffffff),
            np.uint64(((int(stream) + 1) << 24) | ((call >> 32) & 0xffffff)))


def dequant_counter(i, call):
    """The dequantisation stream's counter for element i (csrc/pointwise.hip dequant_noise)."""
    i = np.asarray(i, dtype=np.uint64)
    call = int(call)
    return ((i >> np.uint64(2)) & MASK, (i >> np.uint64(34)) & MASK, np.uint64(call & 0xffffffff), np.uint64((call >> 32) & 0xffffffff))


def words(n, seed, call, stream):
    """(groups, 4) uint64 array of the 32-bit words behind the first n elements."""
    groups = (int(n) + 3) // 4
    seed = int(seed) & (2 ** 64 - 1)
    w = philox4x32_10(sampler_counter(np.arange(groups, dtype=np.uint64), call, stream), (seed & 0xffffffff, seed >> 32))
    return np.stack([np.broadcast_to(v, (groups,)) for v in w], axis=1)


def uniforms(n, seed, call, stream):
    """(u1, u2) per PAIR of elements, fp64 (both exact in fp32): shape (2 * groups,)."""
    w = words(n, seed, call, stream).reshape(-1, 2)
    u1 = ((w[:, 0] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (w[:, 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normal(n, seed, call, stream, std=1.0):
    """The first n elements of the stream in fp64 (std is taken as the fp32 number the kernels multiply by)."""
    u1, u2 = uniforms(n, seed, call, stream)
    r = np.sqrt(-2.0 * np.log(u1))
    e = np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=1).reshape(-1)
    return e[:int(n)] * float(np.float32(std))


def moments(e):
    """mean, variance - 1, (kurtosis - 3), lag-1 product mean -- each with its standard error for n iid N(0, 1) draws."""
    e = np.asarray(e, dtype=np.float64)
    n = e.size
    return {
        "mean": (e.mean(), 1.0 / np.sqrt(n)),
        "variance": (e.var() - 1.0, np.sqrt(2.0 / n)),
        "kurtosis": ((e ** 4).mean() / e.var() ** 2 - 3.0, np.sqrt(24.0 / n)),
        "lag1": ((e[:-1] * e[1:]).mean(), 1.0 / np.sqrt(n)),
    }


def cross(a, b):
    """Mean product of two streams with its standard error."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a * b).mean(), 1.0 / np.sqrt(a.size)


MOMENT_TRIPLES = [(1234, 0, 0), (1234, 0, 1), (1234, 1, 0), (99, 7, 3)]      # (seed, call, stream)
N_MOMENTS = 1 << 20


def check_moments(draw, report=print):
    """The moments check shared by the host test (draw = this oracle) and the GPU test (draw = the device tensor): for 2^20
    draws of each triple, mean / variance / kurtosis / lag-1 product within 4 standard errors, max |e| < 5.77, and the cross
    products stream 0 x stream 1 and call 0 x call 1 within the same bound.  draw(n, seed, call, stream) -> n float array."""
    got = {t: np.asarray(draw(N_MOMENTS, *t), dtype=np.float64) for t in MOMENT_TRIPLES}
    worst = 0.0
    for t, e in got.items():
        assert e.shape == (N_MOMENTS,)
        assert np.abs(e).max() < 5.77, (t, np.abs(e).max())
        for name, (v, se) in moments(e).items():
            report(f"{t} {name}: {v:+.3e} = {v / se:+.2f} standard errors")
            worst = max(worst, abs(v / se))
            assert abs(v) <= 4.0 * se, (t, name, v, se)
    for a, b in (((1234, 0, 0), (1234, 0, 1)), ((1234, 0, 0), (1234, 1, 0))):
        v, se = cross(got[a], got[b])
        report(f"{a} x {b}: {v:+.3e} = {v / se:+.2f} standard errors")
        worst = max(worst, abs(v / se))
        assert abs(v) <= 4.0 * se, (a, b, v, se)
    return worst

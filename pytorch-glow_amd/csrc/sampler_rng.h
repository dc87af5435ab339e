// sampler_rng.h -- the sampler's random stream: counter-based N(0, 1) draws made inside the kernels that consume them
// (GaussianDiag.sample, network/module.py:470-483, without a noise tensor in HBM).  ONE definition, used by every site.
//
// Generator: Philox4x32-10, the round function and key schedule of the dequantisation noise (pointwise.hip).
//   key     = the 64-bit seed
//   counter for elements 4j .. 4j+3 of stream s at call c:
//             c0 = j & 0xffffffff, c1 = j >> 32, c2 = c & 0xffffffff, c3 = ((s + 1) << 24) | ((c >> 32) & 0xffffff)
//   stream  s = 0: the top latent; s = 1 + k: the k-th Split2d in DECODE order (the order glowhip_plan_decode reads eps);
//             at most 254 splits, so s + 1 fits the top byte of c3
//             s = 128 + leaf (128 .. 247): the posterior chain's proposal draws, s = 254: its accept test (posterior.hip; call =
//             the chain's iteration; the entries refuse more than 120 leaves, so the two ranges never meet a plan's 0 .. n_split)
//   element index = flat index in the contiguous (N, C, H, W) draw tensor
// The top byte of c3 is never zero here and always zero in the dequantisation stream (its c3 is call >> 32, calls < 2^56): the two
// never share a counter under one seed.
// Words (w0, w1) give elements 0 and 1 of the group, (w2, w3) elements 2 and 3, by Box-Muller in fp32:
//   u1 = ((w >> 9) + 0.5) * 2^-23      (exact; never 0 or 1)        u2 = (w' >> 8) * 2^-24      (exact)
//   r  = sqrtf(-2 logf(u1));   even element = r cosf(2 pi u2), odd element = r sinf(2 pi u2)
// with the full-precision device functions; |e| <= sqrt(48 ln 2) = 5.77, never infinite.  The value handed on is e * std, one
// rounded fp32 product.  Floating-point contraction is off inside, so the result is the same rounded value whichever kernel
// inlines it.  numpy restatement: tests/sampler_oracle.py.
#pragma once
#include "common.h"

namespace glowhip {

// Where a kernel finds the stream: pos = the DEVICE word {seed, call} (16 bytes; a captured graph's kernel arguments are frozen,
// the word is not), stream and std by value.  pos == nullptr: no draw.
struct SamplerSpec { const unsigned long long* pos; int stream; float std; };

__device__ __forceinline__ void philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0,
                                              unsigned int k1, unsigned int (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned int)p1; c3 = (unsigned int)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the four words of group j of (seed, call, stream)
__device__ __forceinline__ void sampler_words(unsigned long long seed, unsigned long long call, int stream, unsigned long long j,
                                              unsigned int (&w)[4]) {
    philox4x32_10((unsigned int)j, (unsigned int)(j >> 32), (unsigned int)call,
                  ((unsigned int)(stream + 1) << 24) | ((unsigned int)(call >> 32) & 0xffffffu), (unsigned int)seed,
                  (unsigned int)(seed >> 32), w);
}

// element q (0..3) of a group from its words
__device__ __forceinline__ float sampler_element(const unsigned int (&w)[4], int q, float std) {
#pragma clang fp contract(off)
    const unsigned int wa = (q & 2) ? w[2] : w[0], wb = (q & 2) ? w[3] : w[1];
    const float u1 = ((float)(wa >> 9) + 0.5f) * (1.0f / 8388608.0f);
    const float u2 = (float)(wb >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    const float ang = 6.283185307179586f * u2;
    const float e = r * ((q & 1) ? sinf(ang) : cosf(ang));
    return e * std;
}

// element i of (seed, call, stream), times std: what the epilogues call (one Philox evaluation per element)
__device__ __forceinline__ float sampler_draw(unsigned long long seed, unsigned long long call, int stream, unsigned long long i,
                                              float std) {
    unsigned int w[4];
    sampler_words(seed, call, stream, i >> 2, w);
    return sampler_element(w, (int)(i & 3), std);
}
__device__ __forceinline__ float sampler_draw(const SamplerSpec& s, unsigned long long i) {
    return sampler_draw(s.pos[0], s.pos[1], s.stream, i, s.std);
}

}  // namespace glowhip

// restore_linear.hip -- the restoration objective observed through a dense linear operator (compressed sensing): per sample n,
// with x[n] flattened to D = C H W values and A an (M, D) row-major fp32 matrix shared by the batch,
//     y = A x      resid = w (y - t)      loss[n] = inv_wsum[n] sum_m w (y - t)^2      grad_x = A^T (2 inv_wsum[n] resid)
// (include/glowhip.h has THE definition).  Plain fp32 FMA on the vector pipe: 2 M D N flops per product are nothing beside reading A,
// which paces both products.  Three launches and, where M has more than one slice, a fourth:
//   k_linear_fwd         grid = row blocks of LIN_FR rows x D slices of LIN_DS columns.  A workgroup loads its A tile ONCE, into
//                        registers (LIN_FR x LIN_CV float4 per lane), and loops over the batch in sample tiles of LIN_NS: x from L2,
//                        LIN_FR x LIN_NS accumulators per lane, a fixed-tree reduction over the workgroup, the slice's partial y into
//                        scratch.  No sample shares an accumulator with another
//   k_linear_resid       one workgroup per sample: the partials summed in slice order, then k_restore_objective's own loops over y in
//                        the place of x (the 16-byte or element path by the same address rule, `lin_cell` = its restore_cell, the
//                        fp64 loss per thread in element order, then wave, then workgroup).  Writes resid and u = 2 inv resid, the
//                        latter TRANSPOSED (M, NP) so that the adjoint reads a row's samples as one uniform run
//   k_linear_adj         grid = column blocks of LIN_NT columns x M slices of LIN_MS rows.  A[m, columns] is read coalesced, one
//                        column and one accumulator per sample in each lane (sample blocks of LIN_NB: any N up to 64 reads A once),
//                        u[m, :] uniform per row.  One M slice: straight into grad_x
//   k_linear_adj_reduce  the M slices' partials summed in slice order
// No atomics, no dependence on workgroup order: bitwise the same run to run.  Every tile and slice count is a function of (M, D),
// never of N, and a sample's arithmetic never reads another sample's values: sample n has the same bits in a batch of 1 and of 64,
// and a non-finite x[n] stays in sample n.  inv_wsum[n] == 0 is decided where u and resid are written (k_linear_resid): exact zeros
// there, and the adjoint of zeros is zeros.  With A the identity every sum has one non-zero term and every product is by 1 or 0:
// nothing rounds, and loss and grad_x are glowhip_restore_objective's bits at pool 1.
#include "common.h"

namespace glowhip {

constexpr int LIN_NT = 256;                        // threads of the two product kernels
constexpr int LIN_FR = 8;                          // forward: rows of A per workgroup
constexpr int LIN_CV = 4;                          // forward: float4 per lane and row
constexpr int LIN_NS = 4;                          // forward: the sample tile
constexpr int LIN_DS = LIN_NT * 4 * LIN_CV;        // forward: columns per D slice (4 096)
constexpr int LIN_MS = 128;                        // adjoint: rows per M slice
constexpr int LIN_NB = 64;                         // adjoint: the sample block (one accumulator per sample in each lane)
constexpr int LIN_RNT = 1024;                      // k_linear_resid: k_restore_objective's workgroup (RESTORE_NT), hence its loss order

// p[i .. i + 3], zeros from `end` on.  vec: p is 16-byte aligned and i, end are multiples of 4 (i < end then implies i + 3 < end)
__device__ __forceinline__ float4 lin_load4(const float* __restrict__ p, long i, long end, bool vec) {
    if (vec) return i < end ? *reinterpret_cast<const float4*>(p + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v;
    v.x = i < end ? p[i] : 0.f;
    v.y = i + 1 < end ? p[i + 1] : 0.f;
    v.z = i + 2 < end ? p[i + 2] : 0.f;
    v.w = i + 3 < end ? p[i + 3] : 0.f;
    return v;
}

// ypart: (SD, N, MP) -- slice, sample, row; MP = M rounded up to 4 (every sample's partials start on a 16-byte address)
__global__ void __launch_bounds__(LIN_NT) k_linear_fwd(const float* __restrict__ A, const float* __restrict__ x, long M, int N, long D,
                                                       long MP, int SD, float* __restrict__ ypart) {
    __shared__ float red[2][LIN_NT / 64][LIN_FR * LIN_NS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int sl = (int)(blockIdx.x % (unsigned)SD);
    const long m0 = (long)(blockIdx.x / (unsigned)SD) * LIN_FR;
    const long c0 = (long)sl * LIN_DS + tid * 4;      // the lane's float4 j starts at column c0 + j * 4 LIN_NT
    const bool vec = (D & 3) == 0 && ((((size_t)A) | ((size_t)x)) & 15) == 0;
    float4 a[LIN_FR][LIN_CV];
#pragma unroll
    for (int r = 0; r < LIN_FR; ++r)
#pragma unroll
        for (int j = 0; j < LIN_CV; ++j)
            a[r][j] = m0 + r < M ? lin_load4(A + (size_t)(m0 + r) * (size_t)D, c0 + (long)j * (4 * LIN_NT), D, vec)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
    int pass = 0;
    for (int n0 = 0; n0 < N; n0 += LIN_NS, ++pass) {      // the sample tiles, over the A tile the lanes hold
        float acc[LIN_FR][LIN_NS];
#pragma unroll
        for (int s = 0; s < LIN_NS; ++s) {
#pragma unroll
            for (int r = 0; r < LIN_FR; ++r) acc[r][s] = 0.f;
            if (n0 + s < N) {      // (uniform)
                const float* xs = x + (size_t)(n0 + s) * (size_t)D;
#pragma unroll
                for (int j = 0; j < LIN_CV; ++j) {
                    const float4 xv = lin_load4(xs, c0 + (long)j * (4 * LIN_NT), D, vec);
#pragma unroll
                    for (int r = 0; r < LIN_FR; ++r) {
                        float v = acc[r][s];
                        v = __builtin_fmaf(a[r][j].x, xv.x, v);
                        v = __builtin_fmaf(a[r][j].y, xv.y, v);
                        v = __builtin_fmaf(a[r][j].z, xv.z, v);
                        v = __builtin_fmaf(a[r][j].w, xv.w, v);
                        acc[r][s] = v;
                    }
                }
#pragma unroll
                for (int r = 0; r < LIN_FR; ++r) acc[r][s] = wave_sum(acc[r][s]);
            }
        }
        float(*rb)[LIN_FR * LIN_NS] = red[pass & 1];      // (two buffers: a pass's readers are past the next pass's barrier before it is rewritten)
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < LIN_FR; ++r)
#pragma unroll
                for (int s = 0; s < LIN_NS; ++s) rb[wid][r * LIN_NS + s] = acc[r][s];
        }
        __syncthreads();
        if (tid < LIN_FR * LIN_NS) {
            const int r = tid / LIN_NS, s = tid - r * LIN_NS;
            if (m0 + r < M && n0 + s < N) {
                float v = rb[0][tid];
#pragma unroll
                for (int q = 1; q < LIN_NT / 64; ++q) v += rb[q][tid];
                ypart[((size_t)sl * (size_t)N + (size_t)(n0 + s)) * (size_t)MP + (size_t)(m0 + r)] = v;
            }
        }
    }
}

// k_restore_objective's restore_cell at pool 1, with the residual kept: wd = w (y - t) is `resid`, two_inv wd what the adjoint starts
// from (restore_cell's (two_inv * wd) * 1.f, which rounds the same)
__device__ __forceinline__ float lin_cell(float y, float t, float w, float two_inv, double& acc, float& u) {
    const float d = y - t;
    const float wd = w * d;
    acc += (double)wd * (double)d;
    u = two_inv * wd;
    return wd;
}

// ut: (M, NP) -- row, sample; NP = N rounded up to 8, the pad columns zeroed by the last sample's workgroup
__global__ void __launch_bounds__(LIN_RNT) k_linear_resid(const float* __restrict__ ypart, int SD, long MP, const float* __restrict__ target,
                                                          const float* __restrict__ weight, const float* __restrict__ inv_wsum, long M,
                                                          int N, int NP, float inv_default, float* __restrict__ resid,
                                                          float* __restrict__ ut, float* __restrict__ loss_out) {
    __shared__ double red[LIN_RNT / 64];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* ys = ypart + (size_t)n * (size_t)MP;
    const size_t ystride = (size_t)N * (size_t)MP;      // between slices (a multiple of 4 floats)
    const float* ts = target + (size_t)n * (size_t)M;
    const float* ws = weight ? weight + (size_t)n * (size_t)M : nullptr;
    float* rs = resid + (size_t)n * (size_t)M;
    float* us = ut + n;
    if (n == N - 1)
        for (long i = tid; i < M; i += LIN_RNT)
            for (int c = N; c < NP; ++c) ut[(size_t)i * NP + c] = 0.f;
    const float inv = inv_wsum ? inv_wsum[n] : inv_default;
    if (inv == 0.f) {      // a sample that is not part of the problem: exact zeros whatever its x holds (NaN * 0 would not be one)
        for (long i = tid; i < M; i += LIN_RNT) {
            rs[i] = 0.f;
            us[(size_t)i * NP] = 0.f;
        }
        if (tid == 0 && loss_out) loss_out[n] = 0.f;
        return;
    }
    const float two_inv = 2.f * inv;      // (exact)
    double acc = 0.0;
    // k_restore_objective's access rule on this sample's addresses (the partials are always aligned)
    size_t addr = (size_t)ts | (size_t)ws | (size_t)rs;
    const long n4 = (addr & 15) == 0 ? (M >> 2) : 0;
    const float4* t4 = reinterpret_cast<const float4*>(ts);
    const float4* w4 = reinterpret_cast<const float4*>(ws);
    float4* r4 = reinterpret_cast<float4*>(rs);
    for (long i = tid; i < n4; i += LIN_RNT) {
        float4 yv = *reinterpret_cast<const float4*>(ys + 4 * i);
        for (int q = 1; q < SD; ++q) {
            const float4 p = *reinterpret_cast<const float4*>(ys + q * ystride + 4 * i);
            yv.x += p.x, yv.y += p.y, yv.z += p.z, yv.w += p.w;
        }
        const float4 tv = t4[i];
        const float4 wv = ws ? w4[i] : make_float4(1.f, 1.f, 1.f, 1.f);
        float4 v;
        float u0, u1, u2, u3;
        v.x = lin_cell(yv.x, tv.x, wv.x, two_inv, acc, u0);
        v.y = lin_cell(yv.y, tv.y, wv.y, two_inv, acc, u1);
        v.z = lin_cell(yv.z, tv.z, wv.z, two_inv, acc, u2);
        v.w = lin_cell(yv.w, tv.w, wv.w, two_inv, acc, u3);
        r4[i] = v;
        float* up = us + (size_t)(4 * i) * NP;
        up[0] = u0, up[NP] = u1, up[2 * (size_t)NP] = u2, up[3 * (size_t)NP] = u3;
    }
    for (long i = (n4 << 2) + tid; i < M; i += LIN_RNT) {
        float y = ys[i];
        for (int q = 1; q < SD; ++q) y += ys[q * ystride + i];
        float u;
        rs[i] = lin_cell(y, ts[i], ws ? ws[i] : 1.f, two_inv, acc, u);
        us[(size_t)i * NP] = u;
    }
    const double tot = block_sum<LIN_RNT>(acc, red);
    if (tid == 0 && loss_out) loss_out[n] = (float)(tot * (double)inv);
}

// out: (SM, N, D) partials, or grad_x itself when SM == 1
__global__ void __launch_bounds__(LIN_NT) k_linear_adj(const float* __restrict__ A, const float* __restrict__ ut, long M, int N, int NP,
                                                       long D, int SM, float* __restrict__ out) {
    const int tid = threadIdx.x;
    const int sl = (int)(blockIdx.x % (unsigned)SM);
    const long col = (long)(blockIdx.x / (unsigned)SM) * LIN_NT + tid;
    const bool active = col < D;
    const long mlo = (long)sl * LIN_MS, mhi = min(M, mlo + LIN_MS);
    const float* ac = A + (active ? col : 0);
    for (int nb = 0; nb < N; nb += LIN_NB) {      // (more than LIN_NB samples read A again)
        float acc[LIN_NB];
#pragma unroll
        for (int s = 0; s < LIN_NB; ++s) acc[s] = 0.f;
        for (long m = mlo; m < mhi; m += 8) {
            float av[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) av[k] = (active && m + k < mhi) ? ac[(size_t)(m + k) * (size_t)D] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (m + k < mhi) {      // (uniform)
                    const float* ur = ut + (size_t)(m + k) * NP + nb;
#pragma unroll
                    for (int g = 0; g < LIN_NB / 8; ++g) {
                        if (nb + g * 8 < NP) {      // (uniform; NP is a multiple of 8)
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[g * 8 + e] = __builtin_fmaf(av[k], ur[g * 8 + e], acc[g * 8 + e]);
                        }
                    }
                }
            }
        }
        if (active) {
#pragma unroll
            for (int s = 0; s < LIN_NB; ++s)
                if (nb + s < N) out[((size_t)sl * (size_t)N + (size_t)(nb + s)) * (size_t)D + (size_t)col] = acc[s];
        }
    }
}

__global__ void __launch_bounds__(LIN_NT) k_linear_adj_reduce(const float* __restrict__ part, int SM, size_t total, float* __restrict__ grad_x) {
    for (size_t i = (size_t)blockIdx.x * LIN_NT + threadIdx.x; i < total; i += (size_t)gridDim.x * LIN_NT) {
        float v = part[i];
        for (int q = 1; q < SM; ++q) v += part[(size_t)q * total + i];
        grad_x[i] = v;
    }
}

// the shapes of a call: slice and block counts (functions of M and D only) and the carving of the scratch
struct LinGeo {
    long MP, SD, SM, RB, CB;
    int NP;
    size_t off_u, off_g, bytes;      // ypart at 0
};

static const char* lin_geo(int N, long M, long D, LinGeo& g) {
    if (N < 0) return "N < 0";
    if (M < 1 || D < 1) return "M and D must be >= 1";
    if (D >= (1L << 31)) return "D >= 2^31";
    if ((unsigned __int128)M * (unsigned __int128)D >= ((unsigned __int128)1 << 40)) return "M * D >= 2^40";
    g.MP = (M + 3) & ~3L;
    g.SD = (D + LIN_DS - 1) / LIN_DS;
    g.SM = (M + LIN_MS - 1) / LIN_MS;
    g.RB = (M + LIN_FR - 1) / LIN_FR;
    g.CB = (D + LIN_NT - 1) / LIN_NT;
    g.NP = (int)(((long)N + 7) & ~7L);
    if ((unsigned __int128)g.RB * g.SD >= (1u << 31) || (unsigned __int128)g.CB * g.SM >= (1u << 31)) return "more than 2^31 workgroups";
    const unsigned __int128 y = (unsigned __int128)g.SD * (unsigned)N * g.MP * 4, u = (unsigned __int128)M * (unsigned)g.NP * 4,
                            p = g.SM > 1 ? (unsigned __int128)g.SM * (unsigned)N * D * 4 : 0;
    if (y + u + p >= ((unsigned __int128)1 << 46)) return "scratch of 2^46 bytes or more";
    g.off_u = align_up((size_t)y, 256);
    g.off_g = g.off_u + align_up((size_t)u, 256);
    g.bytes = g.off_g + align_up((size_t)p, 256);
    if (g.bytes == 0) g.bytes = 256;      // (N == 0: zero is the error value)
    return nullptr;
}

}  // namespace glowhip

using namespace glowhip;

extern "C" size_t glowhip_restore_linear_scratch_bytes(int N, long M, long D) {
    LinGeo g;
    if (const char* why = lin_geo(N, M, D, g)) {
        set_error("restore_linear_scratch_bytes: %s (N %d, M %ld, D %ld)", why, N, M, D);
        return 0;
    }
    return g.bytes;
}

extern "C" int glowhip_restore_objective_linear(const float* x, const float* target, const float* weight, const float* inv_wsum,
                                                const float* A, long M, int N, long D, float* resid, float* grad_x, float* loss_out,
                                                void* scratch, size_t scratch_bytes, glowhip_stream_t stream) {
    GH_REQUIRE(x && target && A && resid && grad_x,
               "restore_objective_linear: null argument (x, target, A, resid and grad_x are required)");
    LinGeo g;
    const char* why = lin_geo(N, M, D, g);
    GH_REQUIRE(!why, "restore_objective_linear: %s (N %d, M %ld, D %ld)", why, N, M, D);
    if (N == 0) return GLOWHIP_OK;
    GH_REQUIRE(scratch && scratch_bytes >= g.bytes && ((size_t)scratch & 15) == 0,
               "restore_objective_linear: scratch %p of %zu bytes (16-byte aligned, >= %zu: glowhip_restore_linear_scratch_bytes)", scratch,
               scratch_bytes, g.bytes);
    hipStream_t s = (hipStream_t)stream;
    float* ypart = reinterpret_cast<float*>(scratch);
    float* ut = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + g.off_u);
    float* gpart = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + g.off_g);
    const float inv_default = 1.f / (float)M;
    hipLaunchKernelGGL(k_linear_fwd, dim3((unsigned)(g.RB * g.SD)), dim3(LIN_NT), 0, s, A, x, M, N, D, g.MP, (int)g.SD, ypart);
    GH_LAUNCH_CHECK("k_linear_fwd");
    hipLaunchKernelGGL(k_linear_resid, dim3(N), dim3(LIN_RNT), 0, s, ypart, (int)g.SD, g.MP, target, weight, inv_wsum, M, N, g.NP,
                       inv_default, resid, ut, loss_out);
    GH_LAUNCH_CHECK("k_linear_resid");
    hipLaunchKernelGGL(k_linear_adj, dim3((unsigned)(g.CB * g.SM)), dim3(LIN_NT), 0, s, A, ut, M, N, g.NP, D, (int)g.SM,
                       g.SM > 1 ? gpart : grad_x);
    GH_LAUNCH_CHECK("k_linear_adj");
    if (g.SM > 1) {
        const size_t total = (size_t)N * (size_t)D;
        const unsigned blocks = (unsigned)((total + LIN_NT - 1) / LIN_NT < 2048 ? (total + LIN_NT - 1) / LIN_NT : 2048);
        hipLaunchKernelGGL(k_linear_adj_reduce, dim3(blocks), dim3(LIN_NT), 0, s, gpart, (int)g.SM, total, grad_x);
        GH_LAUNCH_CHECK("k_linear_adj_reduce");
    }
    return GLOWHIP_OK;
}

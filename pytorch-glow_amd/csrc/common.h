// common.h -- shared device helpers and host-side error plumbing for libglowhip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/glowhip.h"

namespace glowhip {

void set_error(const char* fmt, ...);

#define GH_REQUIRE(cond, ...)                    \
    do {                                         \
        if (!(cond)) {                           \
            ::glowhip::set_error(__VA_ARGS__);   \
            return GLOWHIP_EINVAL;               \
        }                                        \
    } while (0)

#define GH_LAUNCH_CHECK(name)                                                        \
    do {                                                                             \
        hipError_t e_ = hipGetLastError();                                           \
        if (e_ != hipSuccess) {                                                      \
            ::glowhip::set_error("%s: %s", name, hipGetErrorString(e_));             \
            return GLOWHIP_ELAUNCH;                                                  \
        }                                                                            \
    } while (0)

#define GH_TRY(expr)               \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != GLOWHIP_OK) return rc_; \
    } while (0)

constexpr float LOG_2PI_F = 1.8378770664093453f;
constexpr float LOGSCALE = 3.0f;  // network/module.py:10 logscale_factor

// ---- per-sample log-determinant accumulators ---------------------------------------------------
// Kept as signed Q31.32 fixed point in a u64 so that atomic accumulation from many workgroups is
// order-independent (bitwise reproducible), unlike float atomics.
constexpr double FIX_SCALE = 4294967296.0;
constexpr int ACC_EXTRA = 7;
// acc: 2 N words -- acc[n] the accumulator of sample n, acc[N + n] its STICKY NON-FINITE FLAG (bits 0-2; the bits above them
// count whole nats of large partials, see RANGE below) -- and, in a plan's workspace,
// ACC_EXTRA more accumulator rows acc[(2 + k) N + n] that k_finalize adds to acc[n]: the finishing kernel of the product path
// spreads its one-per-workgroup atomics over them (1 024 workgroups on the four cache lines of 64 samples' accumulators queue up).  A NaN / inf partial sum cannot
// be represented in fixed point (the conversion would silently turn NaN into 0): it raises the flag instead, and k_finalize
// reports NaN / +inf / -inf for a flagged sample -- an fp16-range overflow in the split-half kernels, diverged weights or out-of-distribution
// input surface as a non-finite nll exactly as in the reference, never as a finite wrong one.
// flag bits: 1 = a NaN term, 2 = a +inf term, 4 = a -inf term (k_finalize: NaN wins, +inf and -inf together give NaN, as in the
// reference's floating-point sum)
//
// RANGE.  Q31.32 holds |sum| < 2^31 nats, and a Gaussian term (x - mean)^2 / exp(2 logs) has no bound.  A workgroup partial v with
// |v| >= FIX_COARSE_MIN is therefore split: its whole nats c = rint(v) go, shifted above the three flag bits, into the 61 spare bits of
// the FLAG word (a signed count of nats; the carries of an add move upward only and the flags are set by atomicOr on bits 0-2, so
// neither disturbs the other), and only the remainder v - c (exact in fp64, |v - c| <= 1/2) enters the fine accumulator.
// rint(v 2^32) = c 2^32 + rint((v - c) 2^32): the two words together hold the very integer the fine word alone would have held, so
// k_finalize (fix_total) returns the same bits as before whenever the sum fits Q31.32, and fine + coarse in fp64 when it does not.
// A partial with |v| >= FIX_COARSE_MAX is not accumulated: it raises the +inf / -inf flag of its sign.
// Guarantee, for a sample that receives P workgroup partials from the Gaussian kernels (k_gaussian_logp, k_split_tail, k_conv_tail,
// k_conv_tail_dma, k_top_head_fwd) and the terms of E affine-coupling elements (|log sigmoid| < 104 each, converted per element):
//     if  2^14 P + 104 E < 2^31                                      (acc_budget in plan_build.hip; glowhip_gaussian_logp)
//     and every partial is finite with |v| < 2^43,
//     then the result is the exact sum of the partials, each rounded once to 2^-32 nats, rounded once more to fp64:
//     the fine word stays below 2^14 P + 104 E < 2^31 in magnitude and the coarse count below 2^43 P < 2^60, neither wraps.
//     A partial that is NaN / inf or has |v| >= 2^43 makes the sample NaN / +inf / -inf with its flag bits set.
// A finite wrong value needs a wrapped word, which the inequality excludes.
constexpr double FIX_COARSE_MIN = 16384.0;              // 2^14 nats
constexpr double FIX_COARSE_MAX = 8796093022208.0;      // 2^43 nats
constexpr double FIX_COUPLING_TERM_MAX = 104.0;         // |logf(sigmoid)| of a positive fp32, denormals included
constexpr unsigned long long FIX_FLAG_MASK = 7ull;
__device__ __forceinline__ void fix_flag_nonfinite(unsigned long long* acc, long n, int N, double v) {
    atomicOr(acc + N + n, isnan(v) ? 1ull : (v > 0 ? 2ull : 4ull));
}
__device__ __forceinline__ void fix_atomic_add(unsigned long long* acc, long n, int N, double v) {
    if (!(fabs(v) < FIX_COARSE_MIN)) {      // rare: NaN / inf, or a partial the fine word must not take whole
        if (!(fabs(v) < FIX_COARSE_MAX)) { fix_flag_nonfinite(acc, n, N, v); return; }
        const double c = rint(v);
        atomicAdd(acc + N + n, (unsigned long long)__double2ll_rn(c) << 3);
        v -= c;
    }
    long long q = __double2ll_rn(v * FIX_SCALE);
    atomicAdd(acc + n, (unsigned long long)q);
}
__device__ __forceinline__ double fix_to_double(unsigned long long a) {
    return (double)(long long)a * (1.0 / FIX_SCALE);
}
// fine word (all rows added) + the coarse count of the flag word, in nats
__device__ __forceinline__ double fix_total(unsigned long long fine, unsigned long long flagword) {
    const long long c = (long long)flagword >> 3, f = (long long)fine;
    const long long hi = c + (f >> 32);
    if (hi >= -2147483648ll && hi < 2147483648ll) return fix_to_double(fine + ((unsigned long long)c << 32));
    return (double)c + fix_to_double(fine);
}

// ---- wave64 / workgroup reductions (fixed tree => deterministic) ------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;  // valid in lane 0
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// Sum over a workgroup of NT threads; result valid in thread 0.  red: NT/64 doubles of LDS.
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NT / 64; ++i) t += red[i];
    }
    __syncthreads();
    return t;
}

// XCD-aware remap (8 XCDs, private L2s): hardware places block b on XCD b%8; give each XCD a contiguous
// run of logical tiles so the tiles that share an operand panel share an L2.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int b, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, xcd = b & 7, slot = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// ReLU that PROPAGATES NaN like the reference's (torch.relu(NaN) = NaN); fmaxf(NaN, 0) = 0 would turn an fp16-range overflow
// (inf - inf = NaN in a split-half operand) into a finite wrong activation
__device__ __forceinline__ float relu_(float v) { return v < 0.f ? 0.f : v; }

// ---- debug build only (-DGLOWHIP_DEBUG_STAMPS): s_memtime stamps of workgroup 0 / wave 0, read back by scripts/stamps.py
#ifdef GLOWHIP_DEBUG_STAMPS
// (one array + one extern "C" reader per translation unit: no relocatable device code in this build)
#define GH_STAMPS_DEFINE(name)                                                                                  \
    namespace glowhip { __device__ unsigned long long g_stamps_local[8 * 64]; }                                 \
    extern "C" int glowhip_debug_read_stamps_##name(unsigned long long* dst) {                                  \
        return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(glowhip::g_stamps_local), sizeof(unsigned long long) * 64); \
    }                                                                                                           \
    extern "C" int glowhip_debug_read_stamps_all_##name(unsigned long long* dst) {   /* [wave][stamp] */        \
        return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(glowhip::g_stamps_local), sizeof(unsigned long long) * 8 * 64); \
    }
// launch timeline: every workgroup of the last stamped launch records (s_memrealtime at start, at end, HW_ID, XCC_ID) -- 100 MHz
// chip-wide clock, comparable across CUs
#define GH_WGTIMES_DEFINE(name)                                                                                 \
    namespace glowhip { __device__ unsigned long long g_wg_times[4096 * 4]; }                                   \
    extern "C" int glowhip_debug_read_wgtimes_##name(unsigned long long* dst, int n) {                          \
        return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(glowhip::g_wg_times), sizeof(unsigned long long) * 4 * n); \
    }
#define GH_WG_BEGIN() do { if ((threadIdx.x) == 0) { const int b_ = blockIdx.y * gridDim.x + blockIdx.x; if (b_ < 4096) { \
        g_wg_times[b_ * 4] = __builtin_amdgcn_s_memrealtime(); g_wg_times[b_ * 4 + 2] = __builtin_amdgcn_s_getreg((31 << 11) | 4); \
        g_wg_times[b_ * 4 + 3] = __builtin_amdgcn_s_getreg((31 << 11) | 20); } } } while (0)
#define GH_WG_END() do { if ((threadIdx.x) == 0) { const int b_ = blockIdx.y * gridDim.x + blockIdx.x; if (b_ < 4096) \
        g_wg_times[b_ * 4 + 1] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#ifndef GH_STAMP_BLOCK
#define GH_STAMP_BLOCK 0
#endif
// lane 0 of EVERY wave of the stamped workgroup records: [wave][stamp] (wave 0's row is what the one-wave readers see)
#define GH_STAMP(i) do { if (blockIdx.x == GH_STAMP_BLOCK && blockIdx.y == 0 && (threadIdx.x & 63) == 0) g_stamps_local[(threadIdx.x >> 6) * 64 + (i)] = __builtin_readcyclecounter(); } while (0)
#define GH_STAMP_VAL(i, v) do { if (blockIdx.x == GH_STAMP_BLOCK && blockIdx.y == 0 && (threadIdx.x & 63) == 0) g_stamps_local[(threadIdx.x >> 6) * 64 + (i)] = (unsigned long long)(v); } while (0)
#else
#define GH_STAMPS_DEFINE(name)
#define GH_WGTIMES_DEFINE(name)
#define GH_WG_BEGIN() do { } while (0)
#define GH_WG_END() do { } while (0)
#define GH_STAMP(i) do { } while (0)
#define GH_STAMP_VAL(i, v) do { } while (0)
#endif

// What a launcher of the exact-fp32 convolution kernels chose (testing: glowhip_debug_conv fills a glowhip_conv_info from it; every
// production caller passes nothing).  kernel: GLOWHIP_CVI_*; tile: 64 / 128 (wide: the square block tile, first: BN; tail: the pixels
// per workgroup TP); splits: split-K slices S (wide) / K-split waves WK (tail); mb: output-channel tiles per workgroup (first: MB,
// tail: MT); launches: kernel launches made; paired: the tail's row map
struct ConvLaunchInfo { int kernel, ksize, tile, splits, mb, grid[3], launches, paired; };

// What a launcher of the fp32 finishing / channel-mixer kernels chose (testing: glowhip_debug_fin fills a glowhip_fin_info from it;
// every production caller passes nothing).  kernel: GLOWHIP_FNI_*; pxb / msv / halo: k_cfinish's template arguments; xcd_affine: the
// launch took its chunks in the XCD-affine order (cnet_fin.h cfin_chunk); stage_matrix: k_chanmix's matrix goes through LDS
struct FinLaunchInfo { int kernel, grid[3], lds_bytes, pxb, msv, halo, xcd_affine, stage_matrix; };

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace glowhip

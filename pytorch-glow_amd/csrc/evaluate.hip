// evaluate.hip -- held-out evaluation on the device (include/glowhip.h "Held-out evaluation").
//   k_level_snapshot / k_level_terms   the split of a sample's objective (Glow.normal_flow, network/model.py:409-452) into per-level
//                                      parts, from snapshots of the integer log-det accumulators (common.h) the inference forward
//                                      takes while glowhip_plan_bind_level_terms is in force
//   k_eval_reset / k_eval_fold         the plan-independent fold of K forwards' objectives into a device-resident
//                                      glowhip_eval_state: importance-weighted bits/dim, per-level bits, histogram
// Every sum of the state is an INTEGER sum of per-image values (128-bit two's complement, 2^-32 bits/dim), min / max are integer
// min / max and the histogram counts: the state after a dataset is the same bits for any split into batches and any order.
#include <math.h>

#include "plan_internal.h"

namespace glowhip {

// ---------------------------------------------------------------- per-level terms
// one copy of the (2 + ACC_EXTRA) N accumulator words: the state of every sample's log-det sum behind the launches before it
__global__ void __launch_bounds__(256) k_level_snapshot(const unsigned long long* __restrict__ acc, unsigned long long* __restrict__ dst,
                                                        int words) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < words) dst[i] = acc[i];
}

int launch_level_snapshot(const unsigned long long* acc, unsigned long long* dst, int N, hipStream_t s) {
    const int words = (2 + ACC_EXTRA) * N;
    if (words == 0) return GLOWHIP_OK;
    hipLaunchKernelGGL(k_level_snapshot, dim3(cdiv(words, 256)), dim3(256), 0, s, acc, dst, words);
    GH_LAUNCH_CHECK("k_level_snapshot");
    return GLOWHIP_OK;
}

// terms[l][n] = sum of level l's konst words (fp64, layer order) + fix(snapshot_l - snapshot_{l-1}); the difference is taken on the
// integer words -- fine rows and the whole-nats count of the flag word alike -- so the parts add up to the total as integers.
// A sample whose flag bits are set in snapshot l has NaN from level l on (the flags are sticky: every later snapshot has them too).
__global__ void __launch_bounds__(256) k_level_terms(const unsigned long long* __restrict__ snap, const char* __restrict__ packed,
                                                     LevelKonst kt, int n_levels, int N, float* __restrict__ terms) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long stride = (long)(2 + ACC_EXTRA) * N;
    unsigned long long fine_prev = 0ull;
    long long coarse_prev = 0ll;
    for (int l = 0; l < n_levels; ++l) {
        const unsigned long long* sl = snap + (long)l * stride;
        unsigned long long fine = sl[n];
        for (int k = 0; k < ACC_EXTRA; ++k) fine += sl[(long)(2 + k) * N + n];
        const unsigned long long fw = sl[N + n];
        const long long coarse = (long long)fw >> 3;
        double konst = 0.0;
        for (unsigned i = kt.first[l]; i < kt.first[l + 1]; ++i) konst += *(const double*)(packed + ((size_t)kt.off8[i] << 3));
        double v = konst + fix_total(fine - fine_prev, (unsigned long long)(coarse - coarse_prev) << 3);
        if (fw & FIX_FLAG_MASK) v = __builtin_nan("");
        terms[(long)l * N + n] = (float)v;
        fine_prev = fine; coarse_prev = coarse;
    }
}

int launch_level_terms(const unsigned long long* snap, const void* packed, const LevelKonst& kt, int n_levels, int N, float* terms,
                       hipStream_t s) {
    if (N == 0) return GLOWHIP_OK;
    hipLaunchKernelGGL(k_level_terms, dim3(cdiv(N, 256)), dim3(256), 0, s, snap, (const char*)packed, kt, n_levels, N, terms);
    GH_LAUNCH_CHECK("k_level_terms");
    return GLOWHIP_OK;
}

// ---------------------------------------------------------------- the fold
constexpr double EVAL_FIX = 4294967296.0;      // 2^32: resolution of every sum
constexpr double EVAL_RANGE = 2048.0;          // |per-image value| below this (glowhip.h): 256 of them and of their squares fit an int64
constexpr unsigned long long EVAL_KEY_BIAS = 0x8000000000000000ull;      // signed Q.32 -> ordered unsigned key of min / max

__global__ void k_eval_reset(glowhip_eval_state* st, int n_levels, int bins, double lo, double hi) {
    unsigned long long* w = (unsigned long long*)st;
    const int words = (int)(sizeof(glowhip_eval_state) / 8);
    for (int i = threadIdx.x; i < words; i += blockDim.x) w[i] = 0ull;
    __syncthreads();
    if (threadIdx.x == 0) {
        st->min_key = ~0ull; st->max_key = 0ull;
        st->n_levels = n_levels; st->bins = bins; st->lo = lo; st->hi = hi;
    }
}

enum { RED_SUM = 0, RED_MIN = 1, RED_MAX = 2 };
template <int OP>
__device__ __forceinline__ unsigned long long block_red(unsigned long long v, unsigned long long* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const unsigned long long a = red[threadIdx.x], b = red[threadIdx.x + s];
            red[threadIdx.x] = OP == RED_SUM ? a + b : (OP == RED_MIN ? (a < b ? a : b) : (a > b ? a : b));
        }
        __syncthreads();
    }
    const unsigned long long r = red[0];
    __syncthreads();
    return r;
}
// sum += q as 128-bit two's complement {lo, hi}: the carry out of the low word is read off the value the atomic returns, so the
// pair ends as the exact sum whatever the order of the adders
__device__ __forceinline__ void add128(uint64_t* sum64, long long q) {
    if (q == 0) return;
    unsigned long long* sum = (unsigned long long*)sum64;
    const unsigned long long add = (unsigned long long)q;
    const unsigned long long old = atomicAdd(sum, add);
    const unsigned long long hi = (q < 0 ? ~0ull : 0ull) + ((old + add < old) ? 1ull : 0ull);
    if (hi) atomicAdd(sum + 1, hi);
}
__device__ __forceinline__ long long eval_q(double v) { return __double2ll_rn(v * EVAL_FIX); }

// One thread per image, 256 images per workgroup; every state word receives at most one atomic per workgroup.
__global__ void __launch_bounds__(256) k_eval_fold(glowhip_eval_state* st, const float* __restrict__ objective,
                                                   const float* __restrict__ terms, int K, int N, int n_levels, double inv_ln2_d,
                                                   const float* only_if_nan, float* per_image, long offset) {
    __shared__ unsigned long long red[256];
    __shared__ unsigned int hist[GLOWHIP_EVAL_MAX_BINS + 2];
    const int n = blockIdx.x * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < GLOWHIP_EVAL_MAX_BINS + 2; i += 256) hist[i] = 0u;
    __syncthreads();
    bool live = n < N;
    if (live && only_if_nan) live = isnan(only_if_nan[n]);      // the re-run: only what the first pass flagged (counted there as flagged)
    bool ok = live;
    double bpd = 0.0, single = 0.0;
    if (live) {
        double m = -__builtin_inf(), sum = 0.0;
        for (int k = 0; k < K; ++k) {
            const double o = (double)objective[(long)k * N + n];
            if (!isfinite(o)) ok = false;
            m = o > m ? o : m;
            sum += o;
        }
        if (ok) {
            double e = 0.0;
            for (int k = 0; k < K; ++k) e += exp((double)objective[(long)k * N + n] - m);
            bpd = (double)(float)(-(m + log(e) - log((double)K)) * inv_ln2_d);      // the per-image output IS what is summed
            single = -(sum / (double)K) * inv_ln2_d;
            ok = fabs(bpd) < EVAL_RANGE && fabs(single) < EVAL_RANGE;
        }
    }
    // per-level bits of the draw-averaged figure (they decompose bits_per_dim_single, not the importance-weighted bound)
    long long qlev[GLOWHIP_EVAL_MAX_LEVELS];
#pragma unroll
    for (int l = 0; l < GLOWHIP_EVAL_MAX_LEVELS; ++l) qlev[l] = 0;
    if (terms && ok) {
#pragma unroll
        for (int l = 0; l < GLOWHIP_EVAL_MAX_LEVELS; ++l) {
            if (l < n_levels) {
                double t = 0.0;
                for (int k = 0; k < K; ++k) t += (double)terms[((long)k * n_levels + l) * N + n];
                const double bits = -(t / (double)K) * inv_ln2_d;
                if (!(fabs(bits) < EVAL_RANGE)) ok = false;
                else qlev[l] = eval_q(bits);
            }
        }
    }
    if (live) per_image[offset + n] = ok ? (float)bpd : __builtin_nanf("");
    const long long q = ok ? eval_q(bpd) : 0, q2 = ok ? eval_q(bpd * bpd) : 0, qs = ok ? eval_q(single) : 0;
    const unsigned long long c_ok = block_red<RED_SUM>(ok ? 1ull : 0ull, red);
    const unsigned long long c_bad = block_red<RED_SUM>(live && !ok ? 1ull : 0ull, red);
    const unsigned long long c_live = block_red<RED_SUM>(live ? 1ull : 0ull, red);
    const long long s1 = (long long)block_red<RED_SUM>((unsigned long long)q, red);
    const long long s2 = (long long)block_red<RED_SUM>((unsigned long long)q2, red);
    const long long ss = (long long)block_red<RED_SUM>((unsigned long long)qs, red);
    const unsigned long long kmin = block_red<RED_MIN>(ok ? (unsigned long long)q ^ EVAL_KEY_BIAS : ~0ull, red);
    const unsigned long long kmax = block_red<RED_MAX>(ok ? (unsigned long long)q ^ EVAL_KEY_BIAS : 0ull, red);
    if (threadIdx.x == 0 && c_live) {
        if (c_ok) atomicAdd((unsigned long long*)&st->count, c_ok);
        // a first pass counts its flagged images; the re-run takes every image it folds OUT of that count and puts back what is
        // still flagged: each image is counted exactly once
        if (only_if_nan) { if (c_ok) atomicAdd((unsigned long long*)&st->flagged, 0ull - c_ok); }
        else if (c_bad) atomicAdd((unsigned long long*)&st->flagged, c_bad);
        if (c_ok) {
            add128(st->sum_bpd, s1); add128(st->sum_bpd2, s2); add128(st->sum_single, ss);
            atomicMin((unsigned long long*)&st->min_key, kmin); atomicMax((unsigned long long*)&st->max_key, kmax);
        }
    }
    if (terms) {
#pragma unroll
        for (int l = 0; l < GLOWHIP_EVAL_MAX_LEVELS; ++l) {
            if (l < n_levels) {      // (n_levels is uniform over the grid: every thread reaches the barriers inside block_red)
                const long long sl = (long long)block_red<RED_SUM>((unsigned long long)(ok ? qlev[l] : 0), red);
                if (threadIdx.x == 0 && c_ok) add128(st->sum_level[l], sl);
            }
        }
    }
    // histogram over [lo, hi): bin = floor((b - lo) * (bins / (hi - lo))) in fp64, b < lo: underflow, b >= hi: overflow
    const int bins = st->bins;
    if (bins > 0) {
        if (ok) {
            const double lo = st->lo, hi = st->hi;
            int slot;
            if (bpd < lo) slot = GLOWHIP_EVAL_MAX_BINS;
            else if (bpd >= hi) slot = GLOWHIP_EVAL_MAX_BINS + 1;
            else {
                slot = (int)floor((bpd - lo) * ((double)bins / (hi - lo)));
                slot = slot > bins - 1 ? bins - 1 : slot;
            }
            atomicAdd(&hist[slot], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < GLOWHIP_EVAL_MAX_BINS + 2; i += 256) {
            const unsigned int c = hist[i];
            if (c) atomicAdd((unsigned long long*)(i < GLOWHIP_EVAL_MAX_BINS ? &st->hist[i] : (i == GLOWHIP_EVAL_MAX_BINS ? &st->under : &st->over)),
                             (unsigned long long)c);
        }
    }
}

}  // namespace glowhip

using namespace glowhip;

extern "C" {

int glowhip_plan_level_count(const glowhip_plan* plan) { return plan ? plan->n_split + 1 : 0; }

size_t glowhip_plan_level_scratch_bytes(const glowhip_plan* plan, int N) {
    return (plan && N >= 0) ? (size_t)(plan->n_split + 1) * (2 + ACC_EXTRA) * (size_t)N * 8 : 0;
}

int glowhip_plan_bind_level_terms(glowhip_plan* plan, float* terms, void* scratch, size_t scratch_bytes) {
    GH_REQUIRE(plan, "plan_bind_level_terms: null plan");
    if (!terms && !scratch && scratch_bytes == 0) {
        plan->level_terms = nullptr; plan->level_scratch = nullptr; plan->level_scratch_bytes = 0;
        return GLOWHIP_OK;
    }
    GH_REQUIRE(terms && scratch, "plan_bind_level_terms: null terms or scratch buffer");
    GH_REQUIRE(((size_t)scratch & 7) == 0 && ((size_t)terms & 3) == 0, "plan_bind_level_terms: scratch must be 8-byte, terms 4-byte aligned");
    GH_REQUIRE(plan->n_split + 1 <= LEVEL_MAX, "plan_bind_level_terms: %d levels, at most %d", plan->n_split + 1, LEVEL_MAX);
    int steps = 0;
    for (const LayerPlan& L : plan->layers) steps += L.d.kind == GLOWHIP_LAYER_FLOWSTEP;
    GH_REQUIRE(steps <= LEVEL_MAX_STEPS, "plan_bind_level_terms: %d FlowSteps, at most %d", steps, LEVEL_MAX_STEPS);
    plan->level_terms = terms; plan->level_scratch = (unsigned long long*)scratch; plan->level_scratch_bytes = scratch_bytes;
    return GLOWHIP_OK;
}

int glowhip_eval_reset(glowhip_eval_state* state, int n_levels, int bins, double lo, double hi, glowhip_stream_t stream) {
    GH_REQUIRE(state && ((size_t)state & 7) == 0, "eval_reset: null or misaligned state");
    GH_REQUIRE(n_levels >= 0 && n_levels <= GLOWHIP_EVAL_MAX_LEVELS, "eval_reset: n_levels %d (0 .. %d)", n_levels, GLOWHIP_EVAL_MAX_LEVELS);
    GH_REQUIRE(bins >= 0 && bins <= GLOWHIP_EVAL_MAX_BINS, "eval_reset: bins %d (0 .. %d)", bins, GLOWHIP_EVAL_MAX_BINS);
    GH_REQUIRE(bins == 0 || (isfinite(lo) && isfinite(hi) && lo < hi), "eval_reset: histogram range [%g, %g)", lo, hi);
    hipLaunchKernelGGL(k_eval_reset, dim3(1), dim3(256), 0, (hipStream_t)stream, state, n_levels, bins, lo, hi);
    GH_LAUNCH_CHECK("k_eval_reset");
    return GLOWHIP_OK;
}

int glowhip_eval_fold(glowhip_eval_state* state, const float* objective, const float* terms, int K, int N, int n_levels, double dims,
                      const float* only_if_nan, float* per_image, long offset, glowhip_stream_t stream) {
    GH_REQUIRE(state && objective && per_image, "eval_fold: null state, objective or per-image buffer");
    GH_REQUIRE(K >= 1 && K <= 65535, "eval_fold: K = %d draws (1 .. 65535)", K);
    GH_REQUIRE(N >= 0 && offset >= 0, "eval_fold: N = %d, offset = %ld", N, offset);
    GH_REQUIRE(dims > 0.0 && isfinite(dims), "eval_fold: dims = %g", dims);
    GH_REQUIRE(!terms || (n_levels >= 1 && n_levels <= GLOWHIP_EVAL_MAX_LEVELS), "eval_fold: n_levels %d (1 .. %d)", n_levels,
               GLOWHIP_EVAL_MAX_LEVELS);
    if (N == 0) return GLOWHIP_OK;
    hipLaunchKernelGGL(k_eval_fold, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, state, objective, terms, K, N,
                       terms ? n_levels : 0, 1.0 / (log(2.0) * dims), only_if_nan, per_image, offset);
    GH_LAUNCH_CHECK("k_eval_fold");
    return GLOWHIP_OK;
}

}  // extern "C"

// posterior.hip -- posterior sampling for inverse problems: the Metropolis-adjusted Langevin chain over the latents (one
// independent chain per sample) and the Welford moments of its images.  The definition is in include/glowhip.h ("Posterior
// sampling"); numpy restatement: tests/posterior_oracle.py.  An iteration is
//     k_mala_propose | decode, glowhip_restore_objective, decode_vjp at the proposal | k_mala_energy | k_mala_select | k_posterior_moments
// and these four kernels are the part that is new: everything between them is the restoration path's.
//
// Layout.  A segment is one pair {current, proposal} of contiguous (N, per) tensors: the leaves, then the leaves' gradients in the
// same order, then whatever else follows an accepted proposal (the image).  The table travels by value in the kernel arguments.
// The grid is (B, N): workgroup (b, n) takes the elements b * 256 + tid, + B * 256, ... of every segment of sample n, element by
// element (any 4-byte alignment, any per; the sizes are a few hundred KB).  B depends on the leaf sizes alone (mala_blocks), so the
// three launches of an iteration agree on it.
//
// Sums.  Every workgroup reduces its terms in fp64 in a fixed order (thread: element order; wave: shuffle tree; workgroup: wave
// order) into its own slot part[q][n][b]; whoever needs a sample's sum adds the B slots in order b = 0 .. B - 1.  No floating-point
// atomics, no dependence on workgroup order: the same bits run to run.
//
// The decision of sample n is a pure function of that sample's slots, loss, proposal loss and step and of the position word, none
// of which any workgroup writes before every workgroup has read them: each workgroup of the sample derives it again (the same
// fixed-order arithmetic, so all agree to the bit) and copies its share of an accepted proposal.  The per-sample state (loss, step,
// counters, history row) and the two device words change only after the last workgroup has arrived at a ticket counter -- the
// last-arriver pattern of k_pack_fused (pack.hip): the ticket is an agent-scope integer atomic, zeroed by a memset node in front of
// every launch (an earlier launch that did not finish cannot poison it), and the last arriver alone writes.  It reads nothing another
// workgroup of this launch wrote.
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "sampler_rng.h"

namespace glowhip {

constexpr int MALA_NT = 256;
constexpr int MALA_MAX_SEGS = 32;
constexpr int MALA_MAX_LEAVES = 120;      // streams 128 + leaf <= 247 < 254 (the accept stream)
constexpr int MALA_MAX_BLOCKS = 64;       // workgroups per sample
constexpr int MALA_LEAF_STREAM = 128;
constexpr int MALA_ACCEPT_STREAM = 254;
constexpr double MALA_TARGET_ACCEPT = 0.574;

struct mala_table {
    float* cur[MALA_MAX_SEGS];
    float* prop[MALA_MAX_SEGS];
    int per[MALA_MAX_SEGS];
    int n_segs, n_leaves;
};

// part[q][n][b], q = 0: a = sum xi^2, 1: b = sum (theta - theta' + h d')^2, 2: p = sum theta^2, 3: p' = sum theta'^2
__device__ __forceinline__ double* mala_slot(double* part, int q, int n, int b, int N, int B) {
    return part + ((size_t)q * N + n) * B + b;
}

__global__ void __launch_bounds__(MALA_NT) k_mala_init(float* step, float* inv_wsum, int N, float step0, float inv0) {
    const int n = blockIdx.x * MALA_NT + threadIdx.x;
    if (n < N) {
        step[n] = step0;
        if (inv_wsum) inv_wsum[n] = inv0;
    }
}

__global__ void __launch_bounds__(MALA_NT) k_mala_propose(const mala_table t, const float* step, const unsigned long long* pos,
                                                          int N, double* part) {
#pragma clang fp contract(off)
    __shared__ double red[MALA_NT / 64];
    const int b = blockIdx.x, B = gridDim.x, n = blockIdx.y, tid = threadIdx.x;
    const unsigned long long seed = pos[0], call = pos[1];
    const float h = step[n], s = sqrtf(2.0f * h);
    double acc = 0.0;
    for (int l = 0; l < t.n_leaves; ++l) {
        const int per = t.per[l];
        const size_t base = (size_t)n * per;
        const float* th = t.cur[l] + base;
        const float* g = t.cur[t.n_leaves + l] + base;
        float* out = t.prop[l] + base;
        for (int i = b * MALA_NT + tid; i < per; i += B * MALA_NT) {
            const float xi = sampler_draw(seed, call, MALA_LEAF_STREAM + l, (unsigned long long)base + i, 1.0f);
            const float th_i = th[i];
            const float d = g[i] + th_i;
            out[i] = (th_i - h * d) + s * xi;
            acc += (double)xi * (double)xi;
        }
    }
    const double tot = block_sum<MALA_NT>(acc, red);
    if (tid == 0) *mala_slot(part, 0, n, b, N, B) = tot;
}

__global__ void __launch_bounds__(MALA_NT) k_mala_energy(const mala_table t, const float* step, int N, double* part) {
    __shared__ double red[MALA_NT / 64];
    const int b = blockIdx.x, B = gridDim.x, n = blockIdx.y, tid = threadIdx.x;
    const double h = (double)step[n];
    double sb = 0.0, sp = 0.0, sq = 0.0;
    for (int l = 0; l < t.n_leaves; ++l) {
        const int per = t.per[l];
        const size_t base = (size_t)n * per;
        const float* th = t.cur[l] + base;
        const float* thp = t.prop[l] + base;
        const float* gp = t.prop[t.n_leaves + l] + base;
        for (int i = b * MALA_NT + tid; i < per; i += B * MALA_NT) {
            const double a = (double)th[i], c = (double)thp[i];
            const double e = (a - c) + h * ((double)gp[i] + c);
            sb += e * e;
            sp += a * a;
            sq += c * c;
        }
    }
    const double tb = block_sum<MALA_NT>(sb, red), tp = block_sum<MALA_NT>(sp, red), tq = block_sum<MALA_NT>(sq, red);
    if (tid == 0) {
        *mala_slot(part, 1, n, b, N, B) = tb;
        *mala_slot(part, 2, n, b, N, B) = tp;
        *mala_slot(part, 3, n, b, N, B) = tq;
    }
}

struct mala_decision {
    double log_alpha, p_now;      // p_now: sum theta^2 of the state AFTER the decision
    bool accept, nonfinite;
};

// one thread, sample n: the B slots in order, then the test.  Everything read here is constant for the whole launch.
__device__ __forceinline__ mala_decision mala_decide(const double* part, int n, int N, int B, float L, float Lp, float h,
                                                     unsigned long long seed, unsigned long long call) {
    double s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double* row = part + ((size_t)q * N + n) * B;
        double v = 0.0;
        for (int b = 0; b < B; ++b) v += row[b];
        s[q] = v;
    }
    mala_decision d;
    d.log_alpha = ((double)L - (double)Lp) + 0.5 * (s[2] - s[3]) + 0.5 * s[0] - s[1] / (4.0 * (double)h);
    d.nonfinite = !(isfinite(Lp) && isfinite(s[1]) && isfinite(s[3]));
    unsigned int w[4];
    sampler_words(seed, call, MALA_ACCEPT_STREAM, (unsigned long long)n, w);
    const double u = ((double)(w[0] >> 8) + 0.5) * (1.0 / 16777216.0);
    d.accept = !d.nonfinite && log(u) < d.log_alpha;      // (a NaN log alpha compares false: rejected)
    d.p_now = d.accept ? s[3] : s[2];
    return d;
}

struct mala_state {
    float* loss; const float* loss_prop; float* step;
    unsigned long long* pos; long long* iteration;
    int* counts;       // (2, N): accepted, rejected as non-finite
    float* hist;       // (3, steps, N): energy after the decision, accept flag, log alpha
    unsigned* ticket;
    int steps, burn_in;
    float adapt_rate, step_min, step_max;
};

__global__ void __launch_bounds__(MALA_NT) k_mala_select(const mala_table t, const mala_state st, int N, const double* part) {
    __shared__ int s_flag;
    const int b = blockIdx.x, B = gridDim.x, n = blockIdx.y, tid = threadIdx.x;
    const unsigned long long seed = st.pos[0], call = st.pos[1];
    const long long it = st.iteration[0];
    if (tid == 0) s_flag = mala_decide(part, n, N, B, st.loss[n], st.loss_prop[n], st.step[n], seed, call).accept ? 1 : 0;
    __syncthreads();
    if (s_flag) {      // element copies: the bits of the proposal
        for (int sgi = 0; sgi < t.n_segs; ++sgi) {
            const int per = t.per[sgi];
            const size_t base = (size_t)n * per;
            const unsigned int* src = reinterpret_cast<const unsigned int*>(t.prop[sgi] + base);
            unsigned int* dst = reinterpret_cast<unsigned int*>(t.cur[sgi] + base);
            for (int i = b * MALA_NT + tid; i < per; i += B * MALA_NT) dst[i] = src[i];
        }
    }
    // every read of the per-sample state and of the two words is behind this workgroup; count it in
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(st.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_flag = old + 1 == (unsigned)(B * N);
    }
    __syncthreads();
    if (!s_flag) return;
    __threadfence();
    for (int m = tid; m < N; m += MALA_NT) {      // the last arriver: the per-sample state, one thread per sample
        const float L = st.loss[m], Lp = st.loss_prop[m], h = st.step[m];
        const mala_decision d = mala_decide(part, m, N, B, L, Lp, h, seed, call);
        const float L_now = d.accept ? Lp : L;
        if (d.accept) {
            st.loss[m] = Lp;
            st.counts[m] += 1;
        }
        if (d.nonfinite) st.counts[N + m] += 1;
        if (it < (long long)st.burn_in) {
            const double prob = d.nonfinite || !(d.log_alpha == d.log_alpha) ? 0.0 : (d.log_alpha >= 0.0 ? 1.0 : exp(d.log_alpha));
            const double gamma = (double)st.adapt_rate / sqrt((double)(it + 1));
            double hn = (double)h * exp(gamma * (prob - MALA_TARGET_ACCEPT));
            hn = hn < (double)st.step_min ? (double)st.step_min : (hn > (double)st.step_max ? (double)st.step_max : hn);
            st.step[m] = (float)hn;
        }
        if (it >= 0 && it < (long long)st.steps) {
            const size_t row = (size_t)it * N + m, plane = (size_t)st.steps * N;
            st.hist[row] = (float)((double)L_now + 0.5 * d.p_now);
            st.hist[plane + row] = d.accept ? 1.0f : 0.0f;
            st.hist[2 * plane + row] = (float)d.log_alpha;
        }
    }
    __syncthreads();
    if (tid == 0) {
        st.pos[1] = call + 1;
        st.iteration[0] = it + 1;
    }
}

// Welford fold of the current images, gated by the device iteration word: fold number c = (t - burn_in) / thin + 1 of iteration
// t = *iteration + offset when t >= burn_in and (t - burn_in) % thin == 0; nothing is written otherwise.  c == 1 starts the
// moments (mean = x, M2 = 0) whatever the buffers held.
__global__ void __launch_bounds__(MALA_NT) k_posterior_moments(const float* __restrict__ x, float* __restrict__ mean,
                                                               float* __restrict__ m2, const long long* iteration, int offset,
                                                               int burn_in, int thin, long long n) {
#pragma clang fp contract(off)
    const long long t = iteration[0] + offset - burn_in;
    if (t < 0 || t % thin != 0) return;
    const long long c = t / thin + 1;
    const float fc = (float)c;
    for (long long i = (long long)blockIdx.x * MALA_NT + threadIdx.x; i < n; i += (long long)gridDim.x * MALA_NT) {
        const float v = x[i];
        if (c == 1) {
            mean[i] = v;
            m2[i] = 0.0f;
        } else {
            const float mu = mean[i], delta = v - mu;
            const float mu_new = mu + delta / fc;
            mean[i] = mu_new;
            m2[i] = m2[i] + delta * (v - mu_new);
        }
    }
}

static int mala_blocks(const mala_table& t) {
    long long total = 0;
    for (int l = 0; l < t.n_leaves; ++l) total += t.per[l];
    const long long blocks = (total + MALA_NT - 1) / MALA_NT;
    return (int)(blocks < 1 ? 1 : (blocks > MALA_MAX_BLOCKS ? MALA_MAX_BLOCKS : blocks));
}

// the argument checks every entry shares; fills the table
static int mala_table_of(const char* who, const glowhip_mala_seg* segs, int n_segs, int n_leaves, int N, mala_table& t) {
    GH_REQUIRE(n_leaves >= 1 && n_leaves <= MALA_MAX_LEAVES, "%s: %d leaves (1 .. %d: streams 128 + leaf stay below the accept stream 254)",
               who, n_leaves, MALA_MAX_LEAVES);
    GH_REQUIRE(n_segs >= 1 && n_segs <= MALA_MAX_SEGS, "%s: n_segs %d (1 .. %d)", who, n_segs, MALA_MAX_SEGS);
    GH_REQUIRE(2 * n_leaves <= n_segs, "%s: %d segments cannot hold %d leaves and their gradients", who, n_segs, n_leaves);
    GH_REQUIRE(N >= 1 && N <= 65535, "%s: N = %d (1 .. 65535)", who, N);
    GH_REQUIRE(segs, "%s: null segment table", who);
    t = {};
    t.n_segs = n_segs;
    t.n_leaves = n_leaves;
    for (int i = 0; i < n_segs; ++i) {
        const glowhip_mala_seg& sg = segs[i];
        GH_REQUIRE(sg.per >= 0 && sg.per < (1LL << 31), "%s: segment %d has %lld elements per sample", who, i, (long long)sg.per);
        GH_REQUIRE(sg.per == 0 || (sg.cur && sg.prop), "%s: segment %d (%lld per sample) has a null pointer", who, i, (long long)sg.per);
        GH_REQUIRE((((uintptr_t)sg.cur | (uintptr_t)sg.prop) & 3) == 0, "%s: segment %d is not 4-byte aligned", who, i);
        GH_REQUIRE(i < n_leaves || i >= 2 * n_leaves || sg.per == segs[i - n_leaves].per,
                   "%s: segment %d (the gradient of leaf %d) has %lld elements per sample, the leaf %lld", who, i, i - n_leaves,
                   (long long)sg.per, (long long)segs[i - n_leaves].per);
        t.cur[i] = sg.cur; t.prop[i] = sg.prop; t.per[i] = (int)sg.per;
    }
    return GLOWHIP_OK;
}

static int mala_scratch_ok(const char* who, const mala_table& t, int N, const void* scratch, size_t bytes) {
    const size_t need = (size_t)4 * N * mala_blocks(t) * sizeof(double);
    GH_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0, "%s: scratch is null or not 8-byte aligned", who);
    GH_REQUIRE(bytes >= need, "%s: scratch holds %zu bytes, %zu needed (glowhip_mala_scratch_bytes)", who, bytes, need);
    return GLOWHIP_OK;
}

static bool positive_finite(float v) { return isfinite(v) && v > 0.f; }

}  // namespace glowhip

using namespace glowhip;

extern "C" size_t glowhip_mala_scratch_bytes(const glowhip_mala_seg* segs, int n_segs, int n_leaves, int N) {
    mala_table t;
    if (mala_table_of("mala_scratch_bytes", segs, n_segs, n_leaves, N, t) != GLOWHIP_OK) return 0;
    return (size_t)4 * N * mala_blocks(t) * sizeof(double);
}

extern "C" int glowhip_mala_init(float* step, float* inv_wsum, int N, float step_size, float noise_std, glowhip_stream_t stream) {
    GH_REQUIRE(N >= 1, "mala_init: N = %d (>= 1)", N);
    GH_REQUIRE(positive_finite(step_size), "mala_init: step size %g (finite, > 0)", (double)step_size);
    GH_REQUIRE(positive_finite(noise_std), "mala_init: noise_std %g (finite, > 0)", (double)noise_std);
    const float inv0 = (float)(1.0 / (2.0 * (double)noise_std * (double)noise_std));
    GH_REQUIRE(positive_finite(inv0), "mala_init: 1 / (2 noise_std^2) = %g is out of the fp32 range", (double)inv0);
    GH_REQUIRE(step && ((uintptr_t)step & 3) == 0 && ((uintptr_t)inv_wsum & 3) == 0, "mala_init: step is null, or a pointer is not 4-byte aligned");
    hipLaunchKernelGGL(k_mala_init, dim3(cdiv(N, MALA_NT)), dim3(MALA_NT), 0, (hipStream_t)stream, step, inv_wsum, N, step_size, inv0);
    GH_LAUNCH_CHECK("k_mala_init");
    return GLOWHIP_OK;
}

extern "C" int glowhip_mala_propose(const glowhip_mala_seg* segs, int n_segs, int n_leaves, int N, const float* step,
                                    const unsigned long long* pos, void* scratch, size_t scratch_bytes, glowhip_stream_t stream) {
    mala_table t;
    GH_TRY(mala_table_of("mala_propose", segs, n_segs, n_leaves, N, t));
    GH_REQUIRE(step && ((uintptr_t)step & 3) == 0, "mala_propose: step is null or not 4-byte aligned");
    GH_REQUIRE(pos && ((uintptr_t)pos & 7) == 0, "mala_propose: the position word is null or not 8-byte aligned");
    GH_TRY(mala_scratch_ok("mala_propose", t, N, scratch, scratch_bytes));
    hipLaunchKernelGGL(k_mala_propose, dim3(mala_blocks(t), N), dim3(MALA_NT), 0, (hipStream_t)stream, t, step, pos, N, (double*)scratch);
    GH_LAUNCH_CHECK("k_mala_propose");
    return GLOWHIP_OK;
}

extern "C" int glowhip_mala_energy(const glowhip_mala_seg* segs, int n_segs, int n_leaves, int N, const float* step, void* scratch,
                                   size_t scratch_bytes, glowhip_stream_t stream) {
    mala_table t;
    GH_TRY(mala_table_of("mala_energy", segs, n_segs, n_leaves, N, t));
    GH_REQUIRE(step && ((uintptr_t)step & 3) == 0, "mala_energy: step is null or not 4-byte aligned");
    GH_TRY(mala_scratch_ok("mala_energy", t, N, scratch, scratch_bytes));
    hipLaunchKernelGGL(k_mala_energy, dim3(mala_blocks(t), N), dim3(MALA_NT), 0, (hipStream_t)stream, t, step, N, (double*)scratch);
    GH_LAUNCH_CHECK("k_mala_energy");
    return GLOWHIP_OK;
}

extern "C" int glowhip_mala_select(const glowhip_mala_seg* segs, int n_segs, int n_leaves, int N, float* loss, const float* loss_prop,
                                   float* step, unsigned long long* pos, long long* iteration, int32_t* counts, float* hist, int steps,
                                   int burn_in, float adapt_rate, float step_min, float step_max, unsigned int* ticket,
                                   const void* scratch, size_t scratch_bytes, glowhip_stream_t stream) {
    mala_table t;
    GH_TRY(mala_table_of("mala_select", segs, n_segs, n_leaves, N, t));
    GH_REQUIRE(loss && loss_prop && step && counts && hist && ticket, "mala_select: null argument (loss, loss_prop, step, counts, hist, ticket)");
    GH_REQUIRE((((uintptr_t)loss | (uintptr_t)loss_prop | (uintptr_t)step | (uintptr_t)counts | (uintptr_t)hist | (uintptr_t)ticket) & 3) == 0,
               "mala_select: a pointer is not 4-byte aligned");
    GH_REQUIRE(pos && iteration && (((uintptr_t)pos | (uintptr_t)iteration) & 7) == 0,
               "mala_select: the position / iteration word is null or not 8-byte aligned");
    GH_REQUIRE(steps >= 1 && burn_in >= 0, "mala_select: steps %d (>= 1), burn_in %d (>= 0)", steps, burn_in);
    GH_REQUIRE(isfinite(adapt_rate) && adapt_rate >= 0.f, "mala_select: adapt_rate %g (finite, >= 0)", (double)adapt_rate);
    GH_REQUIRE(positive_finite(step_min) && positive_finite(step_max) && step_min <= step_max,
               "mala_select: step clamp [%g, %g] (finite, 0 < min <= max)", (double)step_min, (double)step_max);
    GH_TRY(mala_scratch_ok("mala_select", t, N, scratch, scratch_bytes));
    mala_state st = {loss, loss_prop, step, pos, iteration, counts, hist, ticket, steps, burn_in, adapt_rate, step_min, step_max};
    const hipError_t e = hipMemsetAsync(ticket, 0, sizeof(unsigned int), (hipStream_t)stream);
    if (e != hipSuccess) {
        set_error("mala_select: zeroing the ticket: %s", hipGetErrorString(e));
        return GLOWHIP_ELAUNCH;
    }
    hipLaunchKernelGGL(k_mala_select, dim3(mala_blocks(t), N), dim3(MALA_NT), 0, (hipStream_t)stream, t, st, N, (const double*)scratch);
    GH_LAUNCH_CHECK("k_mala_select");
    return GLOWHIP_OK;
}

extern "C" int glowhip_posterior_moments(const float* image, float* mean, float* m2, const long long* iteration, int iter_offset,
                                         int burn_in, int thin, long n, glowhip_stream_t stream) {
    GH_REQUIRE(n >= 0, "posterior_moments: n = %ld", n);
    GH_REQUIRE(burn_in >= 0 && thin >= 1, "posterior_moments: burn_in %d (>= 0), thin %d (>= 1)", burn_in, thin);
    if (n == 0) return GLOWHIP_OK;
    GH_REQUIRE(image && mean && m2, "posterior_moments: null argument (image, mean, m2)");
    GH_REQUIRE((((uintptr_t)image | (uintptr_t)mean | (uintptr_t)m2) & 3) == 0, "posterior_moments: a pointer is not 4-byte aligned");
    GH_REQUIRE(iteration && ((uintptr_t)iteration & 7) == 0, "posterior_moments: the iteration word is null or not 8-byte aligned");
    const long blocks = (n + MALA_NT - 1) / MALA_NT;
    hipLaunchKernelGGL(k_posterior_moments, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(MALA_NT), 0, (hipStream_t)stream, image,
                       mean, m2, iteration, iter_offset, burn_in, thin, (long long)n);
    GH_LAUNCH_CHECK("k_posterior_moments");
    return GLOWHIP_OK;
}

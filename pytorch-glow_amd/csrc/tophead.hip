// tophead.hip -- the top head of Glow as one launch each way (gfx950, wave64).
//
// Reference network/model.py:362-379 (prior), :434-445 (log-density of the top latent + classifier), :508-538 (classification
// losses), network/module.py:152-185 (LinearZeros: out = (x W^T + b) * exp(3 logs)).
//
//   prior     h[n, :, p] = base[:] + e[n, :],  e = LinearZeros_y_emb(y_onehot) (width 2C),  base[c] = learn_top.bias[c] *
//             exp(3 learn_top.logs[c]) (learn_top sees h_top == 0) or 0;  mean = h[:, :C], logs = h[:, C:]
//   forward   logp(z | mean, logs) into the per-sample Q31.32 accumulator;  h_y = mean_{H,W} z;  logits = LinearZeros_classifier(h_y);
//             with a criterion: the per-sample classification-loss term and g_logit = weight_y * d loss / d logits
//   backward  dL/dz, g_h = dL/d[mean, logs] per sample and channel; then the parameter gradients in a second, small launch whose
//             sums over the batch run in a fixed order
//
// The work is tiny (48 x 8 x 8 .. 384 x 4 x 4 elements per sample): one workgroup per sample, one wave per channel, every
// reduction a fixed tree or a fixed-order loop -- two runs give the same bits.
#include <math.h>

#include "plan_internal.h"
#include "tophead.h"

namespace glowhip {

namespace {

__device__ __forceinline__ float head_logp1(float mean, float logs, float x) {
    const float d = x - mean;
    return -0.5f * (LOG_2PI_F + 2.0f * logs + (d * d) / expf(2.0f * logs));
}
__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct HeadFwdArgs {
    const float* z; long z_bs;
    const float* pm; const float* pl; long p_bs;      // optional dense base of the prior (N, C, HW)
    glowhip_head_desc h;
    const float* y_onehot; const long long* y;
    float* state;                                     // head_state_floats
    float* logits; float* cls; float* g_logit;
    unsigned long long* acc;
    int N, C, HW;
};

// [mean | logs] of sample n into ml (2C floats of LDS); e (the y_emb part alone) to e_out when given
__device__ __forceinline__ void head_prior_row(const glowhip_head_desc& h, const float* __restrict__ yo, int C2, float* ml,
                                               float* __restrict__ ml_out, float* __restrict__ e_out) {
    const int K = h.K;
    for (int c = threadIdx.x; c < C2; c += 256) {
        float e = 0.f;
        if (h.ye_w) {
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += yo[k] * h.ye_w[(long)c * K + k];
            e = (s + h.ye_b[c]) * expf(LOGSCALE * h.ye_logs[c]);
        }
        const float base = h.lt_bias ? h.lt_bias[c] * expf(LOGSCALE * h.lt_logs[c]) : 0.f;
        const float v = base + e;
        ml[c] = v;
        if (ml_out) ml_out[c] = v;
        if (e_out) e_out[c] = e;
    }
}

__global__ void __launch_bounds__(256) k_top_head_fwd(HeadFwdArgs a) {
    extern __shared__ float sm[];
    __shared__ double red[4];
    const int C = a.C, C2 = 2 * a.C, HW = a.HW, K = a.h.K;
    float* ml = sm; float* hy = sm + C2; float* lg = hy + C;
    const long n = blockIdx.x;
    float* st = a.state + n * 5 * C;
    head_prior_row(a.h, a.y_onehot ? a.y_onehot + n * K : nullptr, C2, ml, st, st + C2);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double lpw = 0.0;
    for (int c = wave; c < C; c += 4) {
        const float m = ml[c], l = ml[C + c];
        const float* zc = a.z + n * a.z_bs + (long)c * HW;
        double lp = 0.0, sz = 0.0;
        for (int p = lane; p < HW; p += 64) {
            const float zz = zc[p];
            const float mm = a.pm ? m + a.pm[n * a.p_bs + (long)c * HW + p] : m;
            const float ll = a.pl ? l + a.pl[n * a.p_bs + (long)c * HW + p] : l;
            lp += (double)head_logp1(mm, ll, zz);
            sz += (double)zz;
        }
        lp = wave_sum(lp); sz = wave_sum(sz);
        if (lane == 0) {
            lpw += lp;
            const float v = (float)(sz / (double)HW);
            hy[c] = v; st[2 * C2 + c] = v;
        }
    }
    const double tot = block_sum<256>(lpw, red);      // (ends with a barrier: hy is complete)
    if (threadIdx.x == 0) fix_atomic_add(a.acc, n, a.N, tot);
    if (!a.h.cl_w) return;
    for (int k = threadIdx.x; k < K; k += 256) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += hy[c] * a.h.cl_w[(long)k * C + c];
        const float l = (s + a.h.cl_b[k]) * expf(LOGSCALE * a.h.cl_logs[k]);
        lg[k] = l; a.logits[n * K + k] = l;
    }
    if (a.h.criterion == GLOWHIP_CRIT_NONE) return;
    __syncthreads();
    if (wave != 0) return;
    if (a.h.criterion == GLOWHIP_CRIT_CE) {      // CrossEntropyLoss, mean over the batch (network/model.py:508-521)
        const long long t = a.y[n];
        const bool ok = t >= 0 && t < K;
        float mx = -INFINITY;
        for (int k = lane; k < K; k += 64) mx = fmaxf(mx, lg[k]);
        mx = wave_max_all(mx);
        float se = 0.f;
        for (int k = lane; k < K; k += 64) se += expf(lg[k] - mx);
        const float lse = mx + logf(wave_sum_all(se));
        const float sc = a.h.weight_y / (float)a.N;
        for (int k = lane; k < K; k += 64) a.g_logit[n * K + k] = sc * (expf(lg[k] - lse) - (k == t ? 1.f : 0.f));
        if (lane == 0) a.cls[n] = ok ? lse - lg[t] : __builtin_nanf("");
    } else {                                     // BCEWithLogitsLoss, mean over batch and classes (network/model.py:523-538)
        float ls = 0.f;
        const float sc = a.h.weight_y / ((float)a.N * (float)K);
        for (int k = lane; k < K; k += 64) {
            const float l = lg[k], t = a.y_onehot[n * K + k];
            ls += fmaxf(l, 0.f) - l * t + log1pf(expf(-fabsf(l)));
            a.g_logit[n * K + k] = sc * (sigmoidf_(l) - t);
        }
        ls = wave_sum_all(ls);
        if (lane == 0) a.cls[n] = ls / (float)K;
    }
}

struct HeadBwdArgs {
    const float* z; long z_bs;
    const float* pm; const float* pl; long p_bs;
    glowhip_head_desc h;
    const float* gld; const float* gz_in; float* gz;
    const float* state; const float* g_logit; float* gh;      // gh: (N, 2C) = dL/d[mean, logs]
    int N, C, HW;
};

__global__ void __launch_bounds__(256) k_top_head_bwd(HeadBwdArgs a) {
    extern __shared__ float sm[];
    const int C = a.C, C2 = 2 * a.C, HW = a.HW, K = a.h.K;
    float* ml = sm; float* ct = sm + C2; float* gs = ct + C;
    const long n = blockIdx.x;
    const float* st = a.state + n * 5 * C;
    const bool cls = a.h.cl_w && a.g_logit;
    for (int c = threadIdx.x; c < C2; c += 256) ml[c] = st[c];
    if (cls)
        for (int k = threadIdx.x; k < K; k += 256) gs[k] = a.g_logit[n * K + k] * expf(LOGSCALE * a.h.cl_logs[k]);
    __syncthreads();
    if (cls) {      // d (weight_y * classification) / d z through h_y = mean_p z: the same value in every pixel of a channel
        for (int c = threadIdx.x; c < C; c += 256) {
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += gs[k] * a.h.cl_w[(long)k * C + c];
            ct[c] = s / (float)HW;
        }
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float coef = a.gld[n];
    for (int c = wave; c < C; c += 4) {
        const float m = ml[c], l = ml[C + c];
        const long base = n * a.z_bs + (long)c * HW;
        double sd = 0.0, sl = 0.0;
        for (int p = lane; p < HW; p += 64) {
            const float mm = a.pm ? m + a.pm[n * a.p_bs + (long)c * HW + p] : m;
            const float ll = a.pl ? l + a.pl[n * a.p_bs + (long)c * HW + p] : l;
            const float d0 = a.z[base + p] - mm;
            const float iv = expf(-2.0f * ll);
            float g = -coef * d0 * iv;                                  // (k_prior_bwd's expression, term by term)
            if (a.gz_in) g += a.gz_in[base + p];
            if (cls) g += ct[c];
            a.gz[base + p] = g;
            const float d = d0 * iv;
            sd += (double)d; sl += (double)(d * d0 - 1.0f);
        }
        sd = wave_sum(sd); sl = wave_sum(sl);
        if (lane == 0) {
            a.gh[n * C2 + c] = (float)((double)coef * sd);
            a.gh[n * C2 + C + c] = (float)((double)coef * sl);
        }
    }
}

struct HeadReduceArgs {
    glowhip_head_desc h; glowhip_head_grads g;
    const float* gh; const float* state; const float* g_logit; const float* logits; const float* y_onehot;
    int N, C;
};

// Parameter gradients of the head: one thread per gradient element, the sum over the batch as a fixed-order loop in fp64
__global__ void __launch_bounds__(256) k_top_head_reduce(HeadReduceArgs a) {
    const int C = a.C, C2 = 2 * a.C, K = a.h.K, N = a.N;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long nA = a.h.ye_w ? (long)C2 * K : 0, nB = a.h.ye_w ? 2L * C2 : 0, nD = a.h.lt_bias ? 2L * C2 : 0;
    const long nF = a.h.cl_w ? (long)K * C : 0, nG = a.h.cl_w ? 2L * K : 0;
    if (i < nA) {                                   // y_emb.weight (2C, K)
        if (!a.g.ye_w) return;
        const int c = (int)(i / K), k = (int)(i % K);
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += (double)a.gh[(long)n * C2 + c] * (double)a.y_onehot[(long)n * K + k];
        a.g.ye_w[i] = (float)(s * (double)expf(LOGSCALE * a.h.ye_logs[c]));
        return;
    }
    i -= nA;
    if (i < nB) {                                   // y_emb.bias | y_emb.logs
        const int c = (int)(i % C2); const bool is_logs = i >= C2;
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += (double)a.gh[(long)n * C2 + c] * (is_logs ? (double)a.state[(long)n * 5 * C + C2 + c] : 1.0);
        if (is_logs) { if (a.g.ye_logs) a.g.ye_logs[c] = (float)(3.0 * s); }
        else if (a.g.ye_b) a.g.ye_b[c] = (float)(s * (double)expf(LOGSCALE * a.h.ye_logs[c]));
        return;
    }
    i -= nB;
    if (i < nD) {                                   // learn_top.bias | learn_top.logs (its weight multiplies h_top == 0: no gradient)
        const int c = (int)(i % C2); const bool is_logs = i >= C2;
        double s = 0.0;
        for (int n = 0; n < N; ++n) s += (double)a.gh[(long)n * C2 + c];
        const float sc = expf(LOGSCALE * a.h.lt_logs[c]);
        if (is_logs) { if (a.g.lt_logs) a.g.lt_logs[c] = (float)(3.0 * (double)(a.h.lt_bias[c] * sc) * s); }
        else if (a.g.lt_bias) a.g.lt_bias[c] = (float)((double)sc * s);
        return;
    }
    i -= nD;
    if (i < nF) {                                   // classifier.weight (K, C)
        if (!a.g.cl_w) return;
        const int k = (int)(i / C), c = (int)(i % C);
        double s = 0.0;
        if (a.g_logit)
            for (int n = 0; n < N; ++n) s += (double)a.g_logit[(long)n * K + k] * (double)a.state[(long)n * 5 * C + 2 * C2 + c];
        a.g.cl_w[i] = (float)(s * (double)expf(LOGSCALE * a.h.cl_logs[k]));
        return;
    }
    i -= nF;
    if (i < nG) {                                   // classifier.bias | classifier.logs
        const int k = (int)(i % K); const bool is_logs = i >= K;
        double s = 0.0;
        if (a.g_logit)
            for (int n = 0; n < N; ++n) s += (double)a.g_logit[(long)n * K + k] * (is_logs ? (double)a.logits[(long)n * K + k] : 1.0);
        if (is_logs) { if (a.g.cl_logs) a.g.cl_logs[k] = (float)(3.0 * s); }
        else if (a.g.cl_b) a.g.cl_b[k] = (float)(s * (double)expf(LOGSCALE * a.h.cl_logs[k]));
    }
}

// (mean, logs) of the conditional prior as dense (N, C, HW) tensors
__global__ void __launch_bounds__(256) k_top_prior(glowhip_head_desc h, const float* __restrict__ y_onehot, int C, int HW,
                                                   float* __restrict__ mean, float* __restrict__ logs) {
    extern __shared__ float sm[];
    const long n = blockIdx.x;
    head_prior_row(h, y_onehot ? y_onehot + n * h.K : nullptr, 2 * C, sm, nullptr, nullptr);
    __syncthreads();
    const long per = (long)C * HW;
    for (long e = threadIdx.x; e < per; e += 256) {
        const int c = (int)(e / HW);
        mean[n * per + e] = sm[c];
        logs[n * per + e] = sm[C + c];
    }
}

// The sampler's top latent (reference network/model.py:466-468, GaussianDiag.sample network/module.py:470-483): the prior row of
// k_top_prior in LDS (zeros without a head), then z = mean + exp(logs) * draw -- the draw is stream 0 of the sampler at the
// element's flat index (sampler_rng.h), pm / pl the optional dense base as in k_top_head_fwd
__global__ void __launch_bounds__(256) k_top_sample(glowhip_head_desc h, const float* __restrict__ y_onehot, int C, int HW,
                                                    const float* __restrict__ pm, const float* __restrict__ pl, long p_bs,
                                                    SamplerSpec rng, float* __restrict__ z) {
    extern __shared__ float sm[];
    const long n = blockIdx.x;
    head_prior_row(h, y_onehot ? y_onehot + n * h.K : nullptr, 2 * C, sm, nullptr, nullptr);
    __syncthreads();
    const long per = (long)C * HW;
    for (long e = threadIdx.x; e < per; e += 256) {
        const int c = (int)(e / HW);
        const float mean = pm ? sm[c] + pm[n * p_bs + e] : sm[c];
        const float logs = pl ? sm[C + c] + pl[n * p_bs + e] : sm[C + c];
        z[n * per + e] = mean + expf(logs) * sampler_draw(rng, (unsigned long long)(n * per + e));
    }
}

int check_head_desc(const glowhip_head_desc* h, int C) {
    GH_REQUIRE(h->K >= 0 && h->K <= 4096, "top head: K=%d out of range", h->K);
    GH_REQUIRE(C > 0 && ((size_t)3 * C + h->K) * 4 <= 48 * 1024, "top head: C=%d, K=%d do not fit the head kernels' LDS", C, h->K);
    GH_REQUIRE(!h->lt_bias == !h->lt_logs, "top head: learn_top.bias and .logs go together");
    GH_REQUIRE(!h->ye_w == !h->ye_b && !h->ye_w == !h->ye_logs, "top head: y_emb.weight, .bias and .logs go together");
    GH_REQUIRE(!h->cl_w == !h->cl_b && !h->cl_w == !h->cl_logs, "top head: classifier.weight, .bias and .logs go together");
    GH_REQUIRE(!(h->ye_w || h->cl_w) || h->K > 0, "top head: a conditional head needs K > 0");
    GH_REQUIRE(h->criterion == GLOWHIP_CRIT_NONE || h->criterion == GLOWHIP_CRIT_CE || h->criterion == GLOWHIP_CRIT_BCE,
               "top head: unknown criterion %d", h->criterion);
    return GLOWHIP_OK;
}

}  // namespace

int launch_top_logp(glowhip_plan* plan, const float* z, const float* prior_mean, const float* prior_logs, long prior_stride,
                    int N, unsigned long long* acc, hipStream_t s) {
    const int* o = plan->out_shape;
    const int C = o[0], HW = o[1] * o[2];
    if (!plan->head_on)
        return launch_gaussian_logp(z, (long)C * HW, prior_mean, prior_logs, prior_stride, N, C, HW, acc, s);
    const glowhip_head_desc& h = plan->head;
    const glowhip_head_io& io = plan->head_io;
    GH_REQUIRE(io.state, "top head: no per-call binding (glowhip_plan_bind_head) for this forward");
    GH_REQUIRE(!h.ye_w || io.y_onehot, "top head: a class-conditional prior needs y_onehot");
    const int crit = h.cl_w ? h.criterion : GLOWHIP_CRIT_NONE;
    GH_REQUIRE(!h.cl_w || io.y_logits, "top head: the classifier needs a y_logits output");
    GH_REQUIRE(crit == GLOWHIP_CRIT_NONE || (io.cls_loss && io.g_logit), "top head: a criterion needs cls_loss and g_logit outputs");
    GH_REQUIRE(crit != GLOWHIP_CRIT_CE || io.y, "top head: the cross-entropy criterion needs integer targets y");
    GH_REQUIRE(crit != GLOWHIP_CRIT_BCE || io.y_onehot, "top head: the BCE criterion needs y_onehot");
    HeadFwdArgs a{z, (long)C * HW, prior_mean, prior_logs, prior_stride, h, io.y_onehot, (const long long*)io.y, io.state,
                  io.y_logits, io.cls_loss, io.g_logit, acc, N, C, HW};
    a.h.criterion = crit;
    hipLaunchKernelGGL(k_top_head_fwd, dim3(N), dim3(256), (size_t)(3 * C + h.K) * 4, s, a);
    GH_LAUNCH_CHECK("k_top_head_fwd");
    count_launch(plan, "k_top_head_fwd");
    return GLOWHIP_OK;
}

int launch_top_sample(glowhip_plan* plan, const float* prior_mean, const float* prior_logs, long prior_stride, const SamplerSpec& rng,
                      float* z, int N, hipStream_t s) {
    const int* o = plan->out_shape;
    const int C = o[0], HW = o[1] * o[2];
    GH_REQUIRE((size_t)2 * C * 4 <= 48 * 1024, "top sample: C=%d does not fit the kernel's LDS", C);
    const glowhip_head_desc h = plan->head_on ? plan->head : glowhip_head_desc{};
    const float* yo = plan->head_on ? plan->head_io.y_onehot : nullptr;
    GH_REQUIRE(!h.ye_w || yo, "top sample: a class-conditional prior needs y_onehot (glowhip_plan_bind_head)");
    hipLaunchKernelGGL(k_top_sample, dim3(N), dim3(256), (size_t)2 * C * 4, s, h, yo, C, HW, prior_mean, prior_logs, prior_stride, rng, z);
    GH_LAUNCH_CHECK("k_top_sample");
    count_launch(plan, "k_top_sample");
    return GLOWHIP_OK;
}

int launch_top_bwd(glowhip_plan* plan, const float* z, const float* prior_mean, const float* prior_logs, long prior_stride,
                   const float* gld, const float* z_grad, float* gz, float* gh, int N, hipStream_t s) {
    const int* o = plan->out_shape;
    const int C = o[0], HW = o[1] * o[2];
    const long per = (long)C * HW;
    if (!plan->head_on) return launch_prior_bwd(z, prior_mean, prior_logs, prior_stride, gld, z_grad, gz, N, per, s);
    const glowhip_head_desc& h = plan->head;
    const glowhip_head_io& io = plan->head_io;
    GH_REQUIRE(io.state && gh, "top head: no per-call binding (glowhip_plan_bind_head) for this backward");
    GH_REQUIRE(!h.cl_w || !io.g_logit || io.y_logits, "top head: the classifier's backward needs the forward's y_logits");
    HeadBwdArgs b{z, per, prior_mean, prior_logs, prior_stride, h, gld, z_grad, gz, io.state, h.cl_w ? io.g_logit : nullptr, gh, N, C, HW};
    hipLaunchKernelGGL(k_top_head_bwd, dim3(N), dim3(256), (size_t)(3 * C + h.K) * 4, s, b);
    GH_LAUNCH_CHECK("k_top_head_bwd");
    count_launch(plan, "k_top_head_bwd");
    const glowhip_head_grads& g = plan->head_grads;
    const long C2 = 2L * C, K = h.K;
    const long total = (h.ye_w ? C2 * K + 2 * C2 : 0) + (h.lt_bias ? 2 * C2 : 0) + (h.cl_w ? K * C + 2 * K : 0);
    const bool any = g.lt_bias || g.lt_logs || g.ye_w || g.ye_b || g.ye_logs || g.cl_w || g.cl_b || g.cl_logs;
    if (!any || total == 0) return GLOWHIP_OK;
    HeadReduceArgs r{h, g, gh, io.state, b.g_logit, io.y_logits, io.y_onehot, N, C};
    hipLaunchKernelGGL(k_top_head_reduce, dim3(cdiv(total, 256)), dim3(256), 0, s, r);
    GH_LAUNCH_CHECK("k_top_head_reduce");
    count_launch(plan, "k_top_head_reduce");
    return GLOWHIP_OK;
}

}  // namespace glowhip

// ================================================================================================ C ABI
extern "C" {

int glowhip_plan_set_head(glowhip_plan* plan, const glowhip_head_desc* head) {
    GH_REQUIRE(plan, "plan_set_head: null plan");
    plan->head_io = glowhip_head_io{};
    plan->head_grads = glowhip_head_grads{};
    if (!head) { plan->head_on = false; plan->head = glowhip_head_desc{}; return GLOWHIP_OK; }
    GH_TRY(check_head_desc(head, plan->out_shape[0]));
    GH_REQUIRE(head->lt_bias || head->ye_w || head->cl_w, "plan_set_head: an empty head (pass NULL to detach)");
    plan->head = *head;
    plan->head_on = true;
    return GLOWHIP_OK;
}

size_t glowhip_plan_head_state_bytes(const glowhip_plan* plan, int N) {
    return (plan && N >= 0) ? head_state_floats(N, plan->out_shape[0]) * sizeof(float) : 0;
}

int glowhip_plan_bind_head(glowhip_plan* plan, const glowhip_head_io* io) {
    GH_REQUIRE(plan && plan->head_on, "plan_bind_head: no head attached");
    plan->head_io = io ? *io : glowhip_head_io{};
    return GLOWHIP_OK;
}

int glowhip_plan_bind_head_grads(glowhip_plan* plan, const glowhip_head_grads* grads) {
    GH_REQUIRE(plan && plan->head_on, "plan_bind_head_grads: no head attached");
    plan->head_grads = grads ? *grads : glowhip_head_grads{};
    return GLOWHIP_OK;
}

int glowhip_top_prior(const glowhip_head_desc* head, const float* y_onehot, int N, int C, int HW, float* mean, float* logs,
                      glowhip_stream_t stream) {
    GH_REQUIRE(head && mean && logs, "top_prior: null argument");
    GH_REQUIRE(N >= 0 && N <= 65535 && HW > 0, "top_prior: bad shape N=%d HW=%d", N, HW);
    GH_TRY(check_head_desc(head, C));
    GH_REQUIRE(!head->ye_w || y_onehot, "top_prior: a class-conditional prior needs y_onehot");
    if (N == 0) return GLOWHIP_OK;
    hipLaunchKernelGGL(k_top_prior, dim3(N), dim3(256), (size_t)2 * C * 4, (hipStream_t)stream, *head, y_onehot, C, HW, mean, logs);
    GH_LAUNCH_CHECK("k_top_prior");
    return GLOWHIP_OK;
}

}  // extern "C"

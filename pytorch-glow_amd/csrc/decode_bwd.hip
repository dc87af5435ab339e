// decode_bwd.hip -- vector-Jacobian products of the DECODE direction (glowhip_plan_decode_vjp, plan_train.hip): given dL/dx on the
// decoded image, the gradients of the latents (z, eps) the image was decoded from.  Reference decode: network/model.py:119-154
// (FlowStep.reverse_flow), 278-294 (FlowModel.decode), network/module.py:470-483 (Conv2dZeros), 511-536 (Split2d).
//
// The sweep walks the plan in ENCODE order and carries the gradient with respect to a layer's encode-side input; every kernel here
// turns it into (a part of) the gradient with respect to the layer's encode-side output.  No parameter gradients: nothing below
// accumulates over pixels, there is no fp64 atomic and no reduction except the per-sample max-abs that normalises dL/dx.
//   k_grad_norm          per-sample power-of-two normalisation factors of dL/dx (device words, no host sync)
//   k_scale_rows         y[n] = x[n] * word[n]: the first (normalise) and last (undo, dL/dz) kernel of the sweep
//   k_chanmix_inv_bwd    (ActNorm + 1x1 conv / permutation)^-1: g_u = W^-T (g_x * exp(-3 logs)), C <= 192
//   k_chanmix_inv_bwd_wide   the same for 192 < C <= 512: pixel blocks x channel slices, never in place
//   k_cpart_finish       gather-only: g_y1 += the partial sums a backward k_cnet launch left (last FlowStep of a level)
//   k_coupling_inv_bwd(4)  inverse coupling tail: g_z2', g_pre of f.4
//   k_split_inv_bwd      Split2d sampling z2 = mean + exp(logs) eps: g_eps (caller's buffer), g_pre of the prior conv
//   k_relu_bwd           hidden activation backward without the ActNorm parameter sums of k_act_bwd
#include "kernels.h"
#include "backward.h"
#include "sh.h"
#include "cnet_fin.h"

namespace glowhip {

// ------------------------------------------------------------------------------------------------
// words[n] = 2^-e, words[N + n] = 2^e with e = floor(log2 max|g[n]|): the normalised gradient of sample n has max-abs in [1, 2),
// whatever the caller's loss scale, and the factors are exact in every format the sweep uses.  max = 0 (or non-finite): e = 0 --
// a zero gradient stays exactly zero, a non-finite one stays non-finite.  One workgroup per sample, fixed order.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_grad_norm(const float* __restrict__ g, long per, float* __restrict__ words, int N) {
    __shared__ float red[4];
    const long n = blockIdx.x;
    const float* gn = g + n * per;
    float m = 0.f;
    if ((per & 3) == 0 && ((size_t)g & 15) == 0) {
        for (long i = (long)threadIdx.x * 4; i < per; i += 1024) {
            const f32x4_t v = *reinterpret_cast<const f32x4_t*>(gn + i);
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
            if (v[0] != v[0] || v[1] != v[1] || v[2] != v[2] || v[3] != v[3]) m = INFINITY;      // (fmaxf drops a NaN)
        }
    } else {
        for (long i = threadIdx.x; i < per; i += 256) {
            const float v = gn[i];
            m = fmaxf(m, fabsf(v));
            if (v != v) m = INFINITY;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        int e = 0;
        if (m > 0.f && m < INFINITY) e = min(max(ilogbf(m), -100), 100);
        words[n] = ldexpf(1.0f, -e);
        words[N + n] = ldexpf(1.0f, e);
    }
}

int launch_grad_norm(const float* g, long per, float* words, int N, hipStream_t s) {
    if (N == 0) return GLOWHIP_OK;
    hipLaunchKernelGGL(k_grad_norm, dim3(N), dim3(256), 0, s, g, per, words, N);
    GH_LAUNCH_CHECK("k_grad_norm");
    return GLOWHIP_OK;
}

__global__ void __launch_bounds__(256) k_scale_rows(const float* __restrict__ x, float* __restrict__ y, long per,
                                                    const float* __restrict__ word, int vec) {
    const long n = blockIdx.y;
    const float f = word[n];
    if (vec) {
        const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
        if (i >= per) return;
        f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + n * per + i);
        v[0] *= f; v[1] *= f; v[2] *= f; v[3] *= f;
        *reinterpret_cast<f32x4_t*>(y + n * per + i) = v;
    } else {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i < per) y[n * per + i] = x[n * per + i] * f;
    }
}

int launch_scale_rows(const float* x, float* y, long per, const float* word, int N, hipStream_t s) {
    if (N == 0 || per == 0) return GLOWHIP_OK;
    const int vec = (per & 3) == 0 && ((size_t)x & 15) == 0 && ((size_t)y & 15) == 0;
    hipLaunchKernelGGL(k_scale_rows, dim3(cdiv(vec ? per / 4 : per, 256), N), dim3(256), 0, s, x, y, per, word, vec);
    GH_LAUNCH_CHECK("k_scale_rows");
    return GLOWHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Inverse mixer VJP.  Decode: v = M u (M = W^-1; gather: v[idx[o]] = u[o]), x = v * exp(-3 logs) - bias, so with t = g_x * exp(-3 logs)
//   g_u[i] = sum_j M[j][i] t[j]      (gather: g_u[o] = t[idx[o]], the FORWARD table)
// 64 pixels per workgroup, t staged in LDS columns [c][px]; M in LDS where it fits (one 16-byte broadcast read of M[j][i .. i + 3]
// and one read of t[j] per four FMAs), else wave-uniform loads.  The first add_C channels of g_x take the partial sums of the
// PREVIOUS FlowStep's backward k_cnet launch on the way in (ChanMixBwdArgs::add_*).
// ------------------------------------------------------------------------------------------------
constexpr int CI_PX = 64, CI_LD = CI_PX + 1;

__global__ void __launch_bounds__(256) k_chanmix_inv_bwd(ChanMixInvBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ism[];
    const int C = a.C;
    float* t = ism;                  // [C][64 (+1)]
    float* ml = ism + C * CI_LD;     // [C][C]
    if (a.matrix && a.w_lds) {
        for (int e0 = threadIdx.x * 4; e0 < C * C; e0 += 1024)
            *reinterpret_cast<f32x4_t*>(ml + e0) = *reinterpret_cast<const f32x4_t*>(a.matrix + e0);
    }
    const int px = threadIdx.x & (CI_PX - 1);
    const int grp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long gp = (long)blockIdx.x * CI_PX + px;
    const long total = (long)a.N * a.HW;
    const bool valid = gp < total;
    const long n = valid ? gp / a.HW : 0;
    const int p = valid ? (int)(gp - n * a.HW) : 0;
    FinSrc addf{};
    if (a.add_part) {
        CnetPending pd{};
        pd.scratch = a.add_part; pd.MS = a.add_MS; pd.tiles = a.add_tiles; pd.R = a.add_R; pd.NI = a.add_NI; pd.lpxt = a.add_lpxt;
        pd.mode = TAIL_ADD_FWD; pd.Cout = a.add_C;
        addf = fin_src(pd, a.N, a.add_H, a.add_W, a.HW, __builtin_ctz(a.add_W));
    }
    // staging, four channels of the thread at a time: every load unconditional from a clamped address, issued before the first store
    for (int c0 = grp; c0 < C; c0 += 16) {
        float gr[4], se[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            gr[u] = a.gx[n * a.g_bs + (long)min(c0 + 4 * u, C - 1) * a.HW + p];
            se[u] = 0.f;
        }
        if (a.add_part) {      // (uniform)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float so;
                fin_gather_t<0>(addf, n, min(c0 + 4 * u, a.add_C - 1), p, se[u], so);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + 4 * u;
            if (c < C) {
                const float g = gr[u] + ((a.add_part && c < a.add_C) ? se[u] * a.add_scale : 0.f);
                t[c * CI_LD + px] = valid ? g * a.inv_scale[c] : 0.f;
            }
        }
    }
    __syncthreads();
    const bool blk4 = a.matrix && a.w_lds;      // (w_lds implies C % 4 == 0)
    for (int i0 = 4 * grp; blk4 && i0 < C; i0 += 16) {
        f32x4_t r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int j = 0; j < C; ++j) {
            const f32x4_t m4 = *reinterpret_cast<const f32x4_t*>(ml + j * C + i0);
            const float g = t[j * CI_LD + px];
            r[0] = fmaf(m4[0], g, r[0]); r[1] = fmaf(m4[1], g, r[1]); r[2] = fmaf(m4[2], g, r[2]); r[3] = fmaf(m4[3], g, r[3]);
        }
        if (valid) {
#pragma unroll
            for (int u = 0; u < 4; ++u) a.gu[n * a.g_bs + (long)(i0 + u) * a.HW + p] = r[u];
        }
    }
    for (int i = grp; i < C && !blk4; i += 4) {
        float r = 0.f;
        if (a.matrix) {
            for (int j = 0; j < C; ++j) r = fmaf(a.matrix[j * C + i], t[j * CI_LD + px], r);
        } else {
            r = t[(a.gather ? a.gather[i] : i) * CI_LD + px];
        }
        if (valid) a.gu[n * a.g_bs + (long)i * a.HW + p] = r;
    }
}

// Wide levels (192 < C <= 512): workgroup = 32 pixels x a slice of 32 OUTPUT channels i; LDS holds M[:, slice] [C][32] and t of all
// channels [C][33] (132 KB at C = 512).  Every slice reads all of g_x: gu must not alias gx.
constexpr int CIW_PX = 32, CIW_LD = CIW_PX + 1, CIW_SL = 32;
static size_t chanmix_inv_bwd_wide_lds(int C, bool matrix) {
    return ((matrix ? (size_t)C * CIW_SL : 0) + (size_t)C * CIW_LD) * sizeof(float);
}
__global__ void __launch_bounds__(256) k_chanmix_inv_bwd_wide(ChanMixInvBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float iwsm[];
    const int C = a.C;
    float* ml = iwsm;                                    // [C][32]: M[j][i0 + k]
    float* t = iwsm + (a.matrix ? C * CIW_SL : 0);       // [C][32 (+1)]
    const int tid = threadIdx.x, px = tid & (CIW_PX - 1), g8 = tid >> 5;
    const int i0 = blockIdx.y * CIW_SL, nsl = min(CIW_SL, C - i0);
    const long gp = (long)blockIdx.x * CIW_PX + px;
    const long total = (long)a.N * a.HW;
    const bool valid = gp < total;
    const long n = valid ? gp / a.HW : 0;
    const int p = valid ? (int)(gp - n * a.HW) : 0;
    if (a.matrix) {
        const int ne = C * CIW_SL;
        for (int e0 = tid; e0 < ne; e0 += 256 * 16) {
            float mv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = min(e0 + 256 * u, ne - 1);
                mv[u] = a.matrix[(e >> 5) * C + min(i0 + (e & 31), C - 1)];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int e = e0 + 256 * u;
                if (e < ne) ml[e] = (e & 31) < nsl ? mv[u] : 0.f;
            }
        }
    }
    for (int c0 = g8; c0 < C; c0 += 8 * 16) {
        float gr[16], sc[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int c = min(c0 + 8 * u, C - 1);
            gr[u] = a.gx[n * a.g_bs + (long)c * a.HW + p];
            sc[u] = a.inv_scale[c];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int c = c0 + 8 * u;
            if (c < C) t[c * CIW_LD + px] = valid ? gr[u] * sc[u] : 0.f;
        }
    }
    __syncthreads();
    const int k0 = 4 * g8;
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.matrix) {
#pragma unroll 4
        for (int j = 0; j < C; ++j) {
            const f32x4_t m4 = *reinterpret_cast<const f32x4_t*>(ml + j * CIW_SL + k0);
            const float g = t[j * CIW_LD + px];
            r[0] = fmaf(m4[0], g, r[0]); r[1] = fmaf(m4[1], g, r[1]); r[2] = fmaf(m4[2], g, r[2]); r[3] = fmaf(m4[3], g, r[3]);
        }
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = min(i0 + k0 + u, C - 1);
            r[u] = t[(a.gather ? a.gather[i] : i) * CIW_LD + px];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (valid && k0 + u < nsl) a.gu[n * a.g_bs + (long)(i0 + k0 + u) * a.HW + p] = r[u];
}

int launch_chanmix_inv_bwd(const ChanMixInvBwdArgs& a, hipStream_t s) {
    GH_REQUIRE(a.C > 0 && a.C <= CHANMIX_BWD_MAX_C, "chanmix inverse VJP: C=%d unsupported (1..%d)", a.C, CHANMIX_BWD_MAX_C);
    const long total = (long)a.N * a.HW;
    if (total == 0) return GLOWHIP_OK;
    if (chanmix_bwd_wide(a.C)) {
        GH_REQUIRE(!a.add_part, "chanmix inverse VJP: C=%d has no gather of a backward k_cnet launch's partial sums (C <= %d)", a.C, CHANMIX_BWD_NARROW_C);
        const float* g_lo = a.gx; const float* g_hi = a.gx + (long)a.N * a.g_bs;
        GH_REQUIRE(a.gu + (long)a.N * a.g_bs <= g_lo || a.gu >= g_hi, "chanmix inverse VJP: C=%d cannot run in place", a.C);
        const size_t lds = chanmix_inv_bwd_wide_lds(a.C, a.matrix != nullptr);
        if (lds > 32 * 1024)
            (void)hipFuncSetAttribute((const void*)k_chanmix_inv_bwd_wide, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_chanmix_inv_bwd_wide, dim3(cdiv(total, CIW_PX), cdiv(a.C, CIW_SL)), dim3(256), lds, s, a);
        GH_LAUNCH_CHECK("k_chanmix_inv_bwd_wide");
        return GLOWHIP_OK;
    }
    size_t lds = (size_t)a.C * CI_LD * sizeof(float);
    ChanMixInvBwdArgs b = a;
    // (16-byte staging of the matrix: C % 4 == 0 and an aligned source, as in launch_chanmix_bwd)
    b.w_lds = a.matrix && (a.C & 3) == 0 && lds + (size_t)a.C * a.C * sizeof(float) <= 64 * 1024 && (reinterpret_cast<uintptr_t>(a.matrix) & 15) == 0;
    if (b.w_lds) lds += (size_t)a.C * a.C * sizeof(float);
    if (lds > 32 * 1024)
        (void)hipFuncSetAttribute((const void*)k_chanmix_inv_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_chanmix_inv_bwd, dim3(cdiv(total, CI_PX)), dim3(256), lds, s, b);
    GH_LAUNCH_CHECK("k_chanmix_inv_bwd");
    return GLOWHIP_OK;
}

// gather-only: g[n][c][p] += add_scale * (partial sums), c < add_C -- the last FlowStep of a level, whose consumer is a squeeze, a
// Split2d or the end of the sweep and wants a finished gradient
__global__ void __launch_bounds__(256) k_cpart_finish(ChanMixInvBwdArgs a) {
    const long n = blockIdx.y;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    CnetPending pd{};
    pd.scratch = a.add_part; pd.MS = a.add_MS; pd.tiles = a.add_tiles; pd.R = a.add_R; pd.NI = a.add_NI; pd.lpxt = a.add_lpxt;
    pd.mode = TAIL_ADD_FWD; pd.Cout = a.add_C;
    const FinSrc f = fin_src(pd, a.N, a.add_H, a.add_W, a.HW, __builtin_ctz(a.add_W));
    if (e >= (long)a.add_C * a.HW) return;
    const int c = (int)(e / a.HW), p = (int)(e - (long)c * a.HW);
    float se, so;
    fin_gather_t<0>(f, n, c, p, se, so);
    a.gu[n * a.g_bs + e] = a.gx[n * a.g_bs + e] + se * a.add_scale;
}

int launch_cpart_finish(const ChanMixInvBwdArgs& a, hipStream_t s) {
    if (a.N == 0 || !a.add_part) return GLOWHIP_OK;
    hipLaunchKernelGGL(k_cpart_finish, dim3(cdiv((long)a.add_C * a.HW, 256), a.N), dim3(256), 0, s, a);
    GH_LAUNCH_CHECK("k_cpart_finish");
    return GLOWHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Inverse coupling tail VJP.  Decode (network/model.py:136-146): y2 = z2'/s - shift, s = sigmoid(r + 2), (shift, r) = hout[2c], hout[2c+1]
//   g_z2' = g_y2 / s;  g_shift = -g_y2;  g_r = -g_y2 (z2'/s) (1 - s)        additive: y2 = z2' - hout[c]: g_z2' = g_y2, g_h = -g_y2
//   Conv2dZeros: hout = (conv + b) e  =>  g_pre = g_h e
// g (the second half of the gradient) is rewritten in place: g_y2 -> g_z2'.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_coupling_inv_bwd(CouplingInvBwdArgs a) {
    const int c = blockIdx.y;
    const long n = blockIdx.z;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.HW) return;
    const long gi = n * a.g_bs + (long)c * a.HW + p;
    const float g2 = a.g2[gi];
    if (a.affine) {
        const long h0 = (n * a.Cout + 2 * c) * a.HW + p;
        const float s = sigmoidf_(a.hout[h0 + a.HW] + 2.0f);
        const float zs = a.z2out[n * a.z_bs + (long)c * a.HW + p] / s;
        a.g2[gi] = g2 / s;
        a.gpre[h0] = -g2 * a.e4[2 * c];
        a.gpre[h0 + a.HW] = -g2 * zs * (1.0f - s) * a.e4[2 * c + 1];
    } else {
        a.gpre[(n * a.Cout + c) * a.HW + p] = -g2 * a.e4[c];
    }
}

// four consecutive pixels per thread (16-byte accesses): a workgroup takes 1024 consecutive elements of one image's (Ch, HW) plane
__global__ void __launch_bounds__(256) k_coupling_inv_bwd4(CouplingInvBwdArgs a) {
    const long n = blockIdx.y;
    const int HW = a.HW;
    const long off = (long)blockIdx.x * 1024 + threadIdx.x * 4;
    if (off >= (long)a.Ch * HW) return;
    const int c = (int)(off / HW);
    const int p = (int)(off - (long)c * HW);
    float* gp = a.g2 + n * a.g_bs + (long)c * HW + p;
    const f32x4_t g2 = *reinterpret_cast<const f32x4_t*>(gp);
    if (a.affine) {
        const long h0 = (n * a.Cout + 2 * c) * HW + p;
        const f32x4_t hr = *reinterpret_cast<const f32x4_t*>(a.hout + h0 + HW);
        const f32x4_t zz = *reinterpret_cast<const f32x4_t*>(a.z2out + n * a.z_bs + (long)c * HW + p);
        const float e0 = a.e4[2 * c], e1 = a.e4[2 * c + 1];
        f32x4_t gz, gp0, gp1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = sigmoidf_(hr[j] + 2.0f);
            const float zs = zz[j] / s;
            gz[j] = g2[j] / s;
            gp0[j] = -g2[j] * e0;
            gp1[j] = -g2[j] * zs * (1.0f - s) * e1;
        }
        *reinterpret_cast<f32x4_t*>(gp) = gz;
        *reinterpret_cast<f32x4_t*>(a.gpre + h0) = gp0;
        *reinterpret_cast<f32x4_t*>(a.gpre + h0 + HW) = gp1;
    } else {
        const float e0 = a.e4[c];
        const f32x4_t gp0 = {-g2[0] * e0, -g2[1] * e0, -g2[2] * e0, -g2[3] * e0};
        *reinterpret_cast<f32x4_t*>(a.gpre + (n * a.Cout + c) * HW + p) = gp0;
    }
}

int launch_coupling_inv_bwd(const CouplingInvBwdArgs& a, hipStream_t s) {
    if (a.N == 0) return GLOWHIP_OK;
    const bool aligned = a.HW % 4 == 0 && a.g_bs % 4 == 0 && a.z_bs % 4 == 0 && ((size_t)a.g2 & 15) == 0 && ((size_t)a.z2out & 15) == 0 &&
                         ((size_t)a.hout & 15) == 0 && ((size_t)a.gpre & 15) == 0;
    if (aligned) {
        hipLaunchKernelGGL(k_coupling_inv_bwd4, dim3((unsigned)(((long)a.Ch * a.HW + 1023) / 1024), a.N), dim3(256), 0, s, a);
        GH_LAUNCH_CHECK("k_coupling_inv_bwd4");
        return GLOWHIP_OK;
    }
    hipLaunchKernelGGL(k_coupling_inv_bwd, dim3(cdiv(a.HW, 256), a.Ch, a.N), dim3(256), 0, s, a);
    GH_LAUNCH_CHECK("k_coupling_inv_bwd");
    return GLOWHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Split2d sampling VJP.  Decode (network/module.py:531-536): z2 = mean + exp(logs) eps, (mean, logs) = hout[2c], hout[2c+1]
//   g_eps = g_z2 exp(logs) (times the sample's un-normalising factor, into the caller's buffer);  g_mean = g_z2;
//   g_logs = g_z2 (z2 - mean);  g_pre = g_h e
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_split_inv_bwd(SplitInvBwdArgs a) {
    const int c = blockIdx.y;
    const long n = blockIdx.z;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.HW) return;
    const int Cout = 2 * a.Ch;
    const long h0 = (n * Cout + 2 * c) * a.HW + p;
    const float mean = a.hout[h0], logs = a.hout[h0 + a.HW];
    const float g = a.gz2[n * a.g_bs + (long)c * a.HW + p];
    const float z2 = a.z2[n * a.z_bs + (long)c * a.HW + p];
    if (a.geps) a.geps[n * a.eps_bs + (long)c * a.HW + p] = g * expf(logs) * a.unscale[n];
    a.gpre[h0] = g * a.e4[2 * c];
    a.gpre[h0 + a.HW] = g * (z2 - mean) * a.e4[2 * c + 1];
}

int launch_split_inv_bwd(const SplitInvBwdArgs& a, hipStream_t s) {
    if (a.N == 0) return GLOWHIP_OK;
    hipLaunchKernelGGL(k_split_inv_bwd, dim3(cdiv(a.HW, 256), a.Ch, a.N), dim3(256), 0, s, a);
    GH_LAUNCH_CHECK("k_split_inv_bwd");
    return GLOWHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// h = relu((u + b) e): g_u = g_h (h > 0) e, in place on g.  k_act_bwd without its parameter sums.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_relu_bwd4(float* __restrict__ g, const float* __restrict__ h, const float* __restrict__ e,
                                                   int Cm, int HW, long total) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;       // HW % 4 == 0: the four share a channel
    if (i >= total) return;
    const float ec = e[(i / HW) % Cm];
    const f32x4_t hv = *reinterpret_cast<const f32x4_t*>(h + i);
    f32x4_t gh = *reinterpret_cast<const f32x4_t*>(g + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) gh[j] = hv[j] > 0.f ? gh[j] * ec : 0.f;
    *reinterpret_cast<f32x4_t*>(g + i) = gh;
}

__global__ void __launch_bounds__(256) k_relu_bwd1(float* __restrict__ g, const float* __restrict__ h, const float* __restrict__ e,
                                                   int Cm, int HW, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    g[i] = h[i] > 0.f ? g[i] * e[(i / HW) % Cm] : 0.f;
}

int launch_relu_bwd(float* g, const float* h, const float* e, int N, int Cm, int HW, hipStream_t s) {
    const long total = (long)N * Cm * HW;
    if (total == 0) return GLOWHIP_OK;
    if (HW % 4 == 0 && ((size_t)g & 15) == 0 && ((size_t)h & 15) == 0)
        hipLaunchKernelGGL(k_relu_bwd4, dim3(cdiv(total / 4, 256)), dim3(256), 0, s, g, h, e, Cm, HW, total);
    else
        hipLaunchKernelGGL(k_relu_bwd1, dim3(cdiv(total, 256)), dim3(256), 0, s, g, h, e, Cm, HW, total);
    GH_LAUNCH_CHECK("k_relu_bwd");
    return GLOWHIP_OK;
}

}  // namespace glowhip

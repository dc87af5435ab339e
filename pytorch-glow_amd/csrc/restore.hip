// restore.hip -- the data term of an inverse problem under the flow prior (in-painting, denoising, super-resolution, projection):
// per sample n, with P the pool x pool average pool (pool = 1: the identity), t the measurement and w its weights,
//     loss[n] = inv_wsum[n] * sum w (P x - t)^2          grad_x = 2 inv_wsum[n] P^T (w (P x - t))
// in ONE launch that reads x once: the residual of a measurement cell is in a register when both outputs need it.  The gradient is
// what glowhip_plan_decode_vjp takes as grad_x (network/restore.py: LatentFit).
//
// One workgroup per SAMPLE.  That makes three properties of the call structural instead of checked: a sample's loss is summed
// inside one workgroup in a fixed order (per thread in element order, then wave, then workgroup: bitwise the same run to run, no
// scratch buffer, no second launch, no atomics); a non-finite x[n] cannot reach another sample's outputs; and inv_wsum[n] == 0
// is one uniform branch.  The price is that a batch of one runs on one CU -- 12 288 elements at 64x64x3, three 16-byte sweeps of
// 1 024 threads, against the ~700 launches of the decode and its VJP that surround it in an iteration.
#include "common.h"

namespace glowhip {

constexpr int RESTORE_NT = 1024;

// the residual of one measurement cell -> its term of the loss (fp64: the three fp32 factors multiply exactly enough) and the value
// every x under the cell receives.  fp32 operations on the gradient: d = px - t, w * d, * 2 inv, * 1 / pool^2 (px itself: pool^2 - 1
// additions and one multiplication) -- the count tests/test_gpu_restore.py derives its bound from
__device__ __forceinline__ float restore_cell(float px, float t, float w, float two_inv, float inv_p2, double& acc) {
    const float d = px - t;
    const float wd = w * d;
    acc += (double)wd * (double)d;
    return (two_inv * wd) * inv_p2;
}

__global__ void __launch_bounds__(RESTORE_NT) k_restore_objective(const float* __restrict__ x, const float* __restrict__ target,
                                                                  const float* __restrict__ weight, const float* __restrict__ inv_wsum,
                                                                  int C, int H, int W, int pool, float inv_default,
                                                                  float* __restrict__ grad_x, float* __restrict__ loss_out) {
    __shared__ double red[RESTORE_NT / 64];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int h = H / pool, w = W / pool;
    const int per = C * H * W, mper = C * h * w;      // (both < 2^31: checked by the caller)
    const float* xs = x + (size_t)n * per;
    float* gs = grad_x + (size_t)n * per;
    const float* ts = target + (size_t)n * mper;
    const float* ws = weight ? weight + (size_t)n * mper : nullptr;
    const float inv = inv_wsum ? inv_wsum[n] : inv_default;
    if (inv == 0.f) {      // a sample that is not part of the problem: exact zeros whatever its x holds (NaN * 0 would not be one)
        for (int i = tid; i < per; i += RESTORE_NT) gs[i] = 0.f;
        if (tid == 0 && loss_out) loss_out[n] = 0.f;
        return;
    }
    const float two_inv = 2.f * inv;      // (exact)
    double acc = 0.0;
    if (pool == 1) {
        // 16-byte accesses where every address of this sample allows (a sample of C H W % 4 != 0 elements puts every other sample off
        // the boundary; a view may start anywhere), element by element for the rest -- k_optim_ema_swap's pattern
        size_t addr = (size_t)xs | (size_t)gs | (size_t)ts | (size_t)ws;
        const int n4 = (addr & 15) == 0 ? (per >> 2) : 0;
        const float4* x4 = reinterpret_cast<const float4*>(xs);
        const float4* t4 = reinterpret_cast<const float4*>(ts);
        const float4* w4 = reinterpret_cast<const float4*>(ws);
        float4* g4 = reinterpret_cast<float4*>(gs);
        for (int i = tid; i < n4; i += RESTORE_NT) {
            const float4 xv = x4[i], tv = t4[i];
            const float4 wv = ws ? w4[i] : make_float4(1.f, 1.f, 1.f, 1.f);
            float4 g;
            g.x = restore_cell(xv.x, tv.x, wv.x, two_inv, 1.f, acc);
            g.y = restore_cell(xv.y, tv.y, wv.y, two_inv, 1.f, acc);
            g.z = restore_cell(xv.z, tv.z, wv.z, two_inv, 1.f, acc);
            g.w = restore_cell(xv.w, tv.w, wv.w, two_inv, 1.f, acc);
            g4[i] = g;
        }
        for (int i = (n4 << 2) + tid; i < per; i += RESTORE_NT)
            gs[i] = restore_cell(xs[i], ts[i], ws ? ws[i] : 1.f, two_inv, 1.f, acc);
    } else {
        const float inv_p2 = 1.f / (float)(pool * pool);
        for (int cell = tid; cell < mper; cell += RESTORE_NT) {      // one measurement cell per thread: its pool x pool patch of x
            const int c = cell / (h * w), r = cell - c * (h * w);
            const int i = r / w, j = r - i * w;
            const int base = c * H * W + i * pool * W + j * pool;
            float s = 0.f;
            for (int a = 0; a < pool; ++a)
                for (int b = 0; b < pool; ++b) s += xs[base + a * W + b];
            const float g = restore_cell(s * inv_p2, ts[cell], ws ? ws[cell] : 1.f, two_inv, inv_p2, acc);
            for (int a = 0; a < pool; ++a)
                for (int b = 0; b < pool; ++b) gs[base + a * W + b] = g;
        }
    }
    const double tot = block_sum<RESTORE_NT>(acc, red);
    if (tid == 0 && loss_out) loss_out[n] = (float)(tot * (double)inv);
}

}  // namespace glowhip

using namespace glowhip;

extern "C" int glowhip_restore_objective(const float* x, const float* target, const float* weight, const float* inv_wsum,
                                         int N, int C, int H, int W, int pool, float* grad_x, float* loss_out,
                                         glowhip_stream_t stream) {
    GH_REQUIRE(x && target && grad_x, "restore_objective: null argument (x, target and grad_x are required)");
    GH_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, "restore_objective: shape (%d, %d, %d, %d)", N, C, H, W);
    GH_REQUIRE(pool >= 1, "restore_objective: pool %d (>= 1)", pool);
    GH_REQUIRE(H % pool == 0 && W % pool == 0, "restore_objective: pool %d does not divide the image %d x %d", pool, H, W);
    GH_REQUIRE((long long)C * H * W < (1LL << 31), "restore_objective: %d x %d x %d elements per sample out of range", C, H, W);
    if (N == 0) return GLOWHIP_OK;
    const float inv_default = 1.f / (float)((long long)C * (H / pool) * (W / pool));
    hipLaunchKernelGGL(k_restore_objective, dim3(N), dim3(RESTORE_NT), 0, (hipStream_t)stream, x, target, weight, inv_wsum, C, H, W,
                       pool, inv_default, grad_x, loss_out);
    GH_LAUNCH_CHECK("k_restore_objective");
    return GLOWHIP_OK;
}

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

// ---------------------------------------------------------------------------------------------------------------------------
// The same data term observed through a point-spread function: A = P B, with B the zero-padded convolution by the sample's PSF k
// (kh x kw taps, both odd, at most PSF_MAX; ah = (kh-1)/2, aw = (kw-1)/2; the same k for every channel)
//     (B x)[c,i,j] = sum_{a,b} k[a,b] x[c, i + ah - a, j + aw - b]          grad_x = 2 inv_wsum[n] B^T P^T (w (A x - t))
// Still one launch and one workgroup per sample -- what that makes structural above holds here as it stands -- in three phases with
// a __syncthreads() between them.  Producer and consumer of grad_x[n] and resid[n] are the same workgroup on one CU, so the
// barrier's workgroup-scope ordering of the global stores is enough; both are read back with plain loads (no __restrict__).
//   1a  B x into grad_x[n], used as scratch: per channel and PSF_TILE x PSF_TILE tile, the x tile with its halo staged in LDS (zeros
//       outside the image: the border rule), `psf_gather4` against the FLIPPED taps
//   1b  k_restore_objective's own loops, cell for cell and in its order, with B x in the place of x: v = w (A x - t) into resid[n],
//       the loss in fp64.  pool == 1 with a 1x1 PSF of 1.0f therefore gives k_restore_objective's bits, the loss's included (while
//       both take the same 16-byte or element path)
//   2   per tile, u = P^T (2 inv v / pool^2) with its halo staged from resid (zeros outside), `psf_gather4` against the taps as given
// Both gathers are the one correlation routine; correlating with the flipped taps and with the taps themselves, each zero-padded,
// are transposes of each other, so phase 2 is B^T P^T of phase 1's P B exactly as linear maps.
constexpr int PSF_MAX = 15;
constexpr int PSF_TILE = 64;                                   // output pixels per tile side: 16 x 64 threads of 4 pixels in a row
constexpr int PSF_TS = PSF_TILE + PSF_MAX - 1;                 // tile row stride in LDS (floats)

// restore_cell up to the value the adjoint starts from: v = w (px - t), and the cell's term of the loss
__device__ __forceinline__ float psf_cell(float px, float t, float w, double& acc) {
    const float d = px - t;
    const float wd = w * d;
    acc += (double)wd * (double)d;
    return wd;
}

// four neighbouring outputs of a row: out[j] = sum_{a,b} taps[a][b] tile[a][j + b], j = 0..3; a tile value is read once per row of
// taps and slides through three registers.  The sum starts from -0.f, the exact identity of addition (-0 + p == p for every p, the
// sign of a zero included), and fmaf(1, x, -0) == x: a one-tap sum rounds nothing
__device__ __forceinline__ void psf_gather4(const float* tile, const float* taps, int kh, int kw, float (&s)[4]) {
    s[0] = s[1] = s[2] = s[3] = -0.f;
    for (int a = 0; a < kh; ++a) {
        const float* tr = tile + a * PSF_TS;
        const float* ka = taps + a * kw;
        float x0 = tr[0], x1 = tr[1], x2 = tr[2];
        for (int b = 0; b < kw; ++b) {
            const float x3 = tr[b + 3], t = ka[b];
            s[0] = __builtin_fmaf(t, x0, s[0]);
            s[1] = __builtin_fmaf(t, x1, s[1]);
            s[2] = __builtin_fmaf(t, x2, s[2]);
            s[3] = __builtin_fmaf(t, x3, s[3]);
            x0 = x1, x1 = x2, x2 = x3;
        }
    }
}

// one pass of the gather over every channel and tile of a sample: out[c,i,j] = sum_{a,b} taps[a][b] src(c, i - ah + a, j - aw + b),
// src = 0 outside the image.  SRC: (c, y, x) inside the image -> float
template <class SRC>
__device__ __forceinline__ void psf_pass(SRC src, const float* taps, int kh, int kw, int C, int H, int W, float* tile, float* out) {
    const int tid = threadIdx.x, ah = (kh - 1) >> 1, aw = (kw - 1) >> 1;
    const int lr = tid >> 4, lc = (tid & 15) << 2;
    for (int c = 0; c < C; ++c)
        for (int i0 = 0; i0 < H; i0 += PSF_TILE)
            for (int j0 = 0; j0 < W; j0 += PSF_TILE) {
                const int th = min(PSF_TILE, H - i0), tw = min(PSF_TILE, W - j0);
                const int rows = th + kh - 1, cols = ((tw + 3) & ~3) + kw - 1;      // (<= PSF_TS: the last read is column cols - 1)
                for (int e = tid; e < rows * cols; e += RESTORE_NT) {
                    const int r = e / cols, q = e - r * cols;
                    const int y = i0 - ah + r, xx = j0 - aw + q;
                    tile[r * PSF_TS + q] = (y >= 0 && y < H && xx >= 0 && xx < W) ? src(c, y, xx) : 0.f;
                }
                __syncthreads();
                if (lr < th && lc < tw) {
                    float s[4];
                    psf_gather4(tile + lr * PSF_TS + lc, taps, kh, kw, s);
                    float* o = out + (c * H + i0 + lr) * W + j0 + lc;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (lc + j < tw) o[j] = s[j];
                }
                __syncthreads();
            }
}

__global__ void __launch_bounds__(RESTORE_NT) k_restore_objective_psf(const float* __restrict__ x, const float* __restrict__ target,
                                                                      const float* __restrict__ weight, const float* __restrict__ inv_wsum,
                                                                      const float* __restrict__ psf, long psf_stride, int kh, int kw,
                                                                      int C, int H, int W, int pool, float inv_default,
                                                                      float* resid, float* grad_x, float* __restrict__ loss_out) {
    __shared__ double red[RESTORE_NT / 64];
    __shared__ float taps[PSF_MAX * PSF_MAX], taps_flipped[PSF_MAX * PSF_MAX];
    __shared__ float tile[PSF_TS * PSF_TS];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int h = H / pool, w = W / pool;
    const int per = C * H * W, mper = C * h * w;      // (both < 2^31: checked by the caller)
    const float* xs = x + (size_t)n * per;
    float* gs = grad_x + (size_t)n * per;
    float* rs = resid + (size_t)n * mper;
    const float* ts = target + (size_t)n * mper;
    const float* ws = weight ? weight + (size_t)n * mper : nullptr;
    const float inv = inv_wsum ? inv_wsum[n] : inv_default;
    if (inv == 0.f) {      // a sample that is not part of the problem: exact zeros whatever its x holds
        for (int i = tid; i < per; i += RESTORE_NT) gs[i] = 0.f;
        for (int i = tid; i < mper; i += RESTORE_NT) rs[i] = 0.f;
        if (tid == 0 && loss_out) loss_out[n] = 0.f;
        return;
    }
    const float* ks = psf + (size_t)n * psf_stride;
    const int nk = kh * kw;
    for (int q = tid; q < nk; q += RESTORE_NT) {
        const float v = ks[q];
        taps[q] = v;
        taps_flipped[nk - 1 - q] = v;      // [kh-1-a][kw-1-b]
    }
    __syncthreads();

    // 1a: B x -> grad_x[n]
    psf_pass([&](int c, int y, int xx) { return xs[(c * H + y) * W + xx]; }, taps_flipped, kh, kw, C, H, W, tile, gs);
    // (psf_pass ends on a barrier: every B x is written)

    // 1b: k_restore_objective's loops over B x; v = w (A x - t) into resid[n]
    const float two_inv = 2.f * inv;      // (exact)
    const float inv_p2 = pool == 1 ? 1.f : 1.f / (float)(pool * pool);
    double acc = 0.0;
    if (pool == 1) {
        size_t addr = (size_t)xs | (size_t)gs | (size_t)ts | (size_t)ws | (size_t)rs;
        const int n4 = (addr & 15) == 0 ? (per >> 2) : 0;
        const float4* b4 = reinterpret_cast<const float4*>(gs);
        const float4* t4 = reinterpret_cast<const float4*>(ts);
        const float4* w4 = reinterpret_cast<const float4*>(ws);
        float4* r4 = reinterpret_cast<float4*>(rs);
        for (int i = tid; i < n4; i += RESTORE_NT) {
            const float4 bv = b4[i], tv = t4[i];
            const float4 wv = ws ? w4[i] : make_float4(1.f, 1.f, 1.f, 1.f);
            float4 v;
            v.x = psf_cell(bv.x, tv.x, wv.x, acc);
            v.y = psf_cell(bv.y, tv.y, wv.y, acc);
            v.z = psf_cell(bv.z, tv.z, wv.z, acc);
            v.w = psf_cell(bv.w, tv.w, wv.w, acc);
            r4[i] = v;
        }
        for (int i = (n4 << 2) + tid; i < per; i += RESTORE_NT) rs[i] = psf_cell(gs[i], ts[i], ws ? ws[i] : 1.f, acc);
    } else {
        for (int cell = tid; cell < mper; cell += RESTORE_NT) {      // one measurement cell per thread: its pool x pool patch of B x
            const int c = cell / (h * w), r = cell - c * (h * w);
            const int i = r / w, j = r - i * w;
            const int base = c * H * W + i * pool * W + j * pool;
            float s = 0.f;
            for (int a = 0; a < pool; ++a)
                for (int b = 0; b < pool; ++b) s += gs[base + a * W + b];
            rs[cell] = psf_cell(s * inv_p2, ts[cell], ws ? ws[cell] : 1.f, acc);
        }
    }
    const double tot = block_sum<RESTORE_NT>(acc, red);      // (two barriers: every v is written, every B x has been read)
    if (tid == 0 && loss_out) loss_out[n] = (float)(tot * (double)inv);

    // 2: B^T of u = P^T (2 inv v / pool^2) -> grad_x[n]; the cell's value is formed as restore_cell returns it
    psf_pass([&](int c, int y, int xx) { return (two_inv * rs[(c * h + y / pool) * w + xx / pool]) * inv_p2; }, taps, kh, kw, C, H, W,
             tile, gs);
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

extern "C" int glowhip_restore_objective_psf(const float* x, const float* target, const float* weight, const float* inv_wsum,
                                             const float* psf, long psf_stride, int kh, int kw, int N, int C, int H, int W, int pool,
                                             float* resid, float* grad_x, float* loss_out, glowhip_stream_t stream) {
    GH_REQUIRE(x && target && grad_x && psf && resid,
               "restore_objective_psf: null argument (x, target, psf, resid and grad_x are required)");
    GH_REQUIRE(kh >= 1 && kh <= PSF_MAX && (kh & 1) && kw >= 1 && kw <= PSF_MAX && (kw & 1),
               "restore_objective_psf: psf of %d x %d taps (both sides odd, 1 .. %d)", kh, kw, PSF_MAX);
    GH_REQUIRE(psf_stride == 0 || psf_stride >= (long)kh * kw, "restore_objective_psf: psf stride %ld (0: one psf for the batch, or >= %d)",
               psf_stride, kh * kw);
    GH_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, "restore_objective_psf: shape (%d, %d, %d, %d)", N, C, H, W);
    GH_REQUIRE(pool >= 1, "restore_objective_psf: pool %d (>= 1)", pool);
    GH_REQUIRE(H % pool == 0 && W % pool == 0, "restore_objective_psf: pool %d does not divide the image %d x %d", pool, H, W);
    GH_REQUIRE((long long)C * H * W < (1LL << 31), "restore_objective_psf: %d x %d x %d elements per sample out of range", C, H, W);
    if (N == 0) return GLOWHIP_OK;
    const float inv_default = 1.f / (float)((long long)C * (H / pool) * (W / pool));
    hipLaunchKernelGGL(k_restore_objective_psf, dim3(N), dim3(RESTORE_NT), 0, (hipStream_t)stream, x, target, weight, inv_wsum, psf,
                       psf_stride, kh, kw, C, H, W, pool, inv_default, resid, grad_x, loss_out);
    GH_LAUNCH_CHECK("k_restore_objective_psf");
    return GLOWHIP_OK;
}

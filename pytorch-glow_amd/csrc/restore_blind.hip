// restore_blind.hip -- blind deblurring: the point-spread function as an unknown of the fit.  The gradient of the data term of
// glowhip_restore_objective_psf (csrc/restore.hip) with respect to the taps of the PSF, and the softmax that keeps the estimate on
// the simplex (include/glowhip.h has THE definition).  Per sample n, with v = resid as that call leaves it:
//     u[c,i,j]   = (2 inv v[c, i/pool, j/pool]) * (1/pool^2)                 the two roundings of that kernel's phase 2
//     g_k[n,a,b] = sum_{c,i,j} u[c,i,j] x[c, i + ah - a, j + aw - b]         (x = 0 outside the image)
// a cross-correlation of two buffers the iteration already holds.  Two launches:
//   k_psf_grad_partial   grid = samples x (channel, BLIND_TH-row band, BLIND_TW-column tile).  A workgroup stages its u tile and the
//                        x tile with its halo (zeros outside the image) in LDS.  A thread owns one tap and one SLICE of the tile's
//                        columns (S = min(BLIND_NT / (kh kw), BLIND_TW) slices: a 3x3 PSF has 9 taps and 28 slices; slice s takes
//                        columns s, s + S, ...).  Per tile row it runs one fp32 fmaf chain of at most BLIND_CHAIN = BLIND_TW = 64
//                        terms; the chains of the rows, then the slices in slice order, are folded in fp64.  kh kw doubles per
//                        workgroup into the scratch
//   k_psf_grad_finish    one workgroup per PSF: the partials of its sample -- of every sample, in sample order, when the batch
//                        shares one PSF -- in (sample,) channel, band, tile order, dealt as contiguous runs to G = min(BLIND_FNT /
//                        (kh kw), BLIND_FG) groups that are folded in group order, all in fp64; grad_psf with one rounding; the
//                        softmax backward g_theta[q] = k[q] (g_k[q] - sum_r k[r] g_k[r]) in fp64 (the dot product in tap order),
//                        grad_logits with one rounding
// No atomics, nothing depends on workgroup order: the same bits run to run.  Every tile, band, slice and group count is a function
// of (C, H, W, kh, kw) only, never of N, and a sample's partials are computed from that sample's values alone: with per-sample PSFs
// sample n's gradient has the same bits in a batch of 1 and of 5, and a non-finite x[n] reaches only sample n's gradient (or the
// shared one).  inv_wsum[n] == 0 is one uniform branch of the partial launch: exact zeros, whatever x[n] holds.
//
// LDS reads of the inner loop: u is one address per slice (a broadcast); x is read at tile[(li + kh-1-a) * ts + lj + kw-1-b].  With
// the tile row stride ts = BLIND_TW + kw, which is kw (mod 32), the address of tap q = a kw + b is a constant minus q: the lanes of
// one slice read consecutive dwords, and lanes of neighbouring slices that meet read the same one -- no bank is asked for two
// addresses by a 32-lane half (the natural stride BLIND_TW + kw - 1 = 78 at 15 taps is 14 (mod 32): tap rows r and r + 2 collide).
#include "common.h"

namespace glowhip {

constexpr int BLIND_PSF_MAX = 15;                               // restore.hip: PSF_MAX
constexpr int BLIND_NT = 256;                                   // threads of the partial launch (>= 15 x 15 taps)
constexpr int BLIND_TH = 8;                                     // tile rows: 64 x 64 x 3 at batch 1 is 24 workgroups
constexpr int BLIND_TW = 64;                                    // tile columns
constexpr int BLIND_CHAIN = BLIND_TW;                           // the longest fp32 fmaf chain: one tile row (tests/blind_oracle.py)
constexpr int BLIND_TS_MAX = BLIND_TW + BLIND_PSF_MAX;          // the widest tile row stride
constexpr int BLIND_XROWS = BLIND_TH + BLIND_PSF_MAX - 1;
constexpr int BLIND_FNT = 1024;                                 // threads of the finishing launch
constexpr int BLIND_FG = 32;                                    // its groups, at most

__global__ void __launch_bounds__(BLIND_NT) k_psf_grad_partial(const float* __restrict__ x, const float* __restrict__ resid,
                                                               const float* __restrict__ inv_wsum, int kh, int kw, int C, int H, int W,
                                                               int pool, float inv_default, int RB, int CT, double* __restrict__ part) {
    __shared__ float ut[BLIND_TH * BLIND_TW];
    __shared__ float xt[BLIND_XROWS * BLIND_TS_MAX];
    __shared__ double red[BLIND_NT];
    const int tid = threadIdx.x, nk = kh * kw;
    const int P = C * RB * CT;
    const int n = (int)(blockIdx.x / (unsigned)P), p = (int)(blockIdx.x - (unsigned)n * (unsigned)P);
    double* out = part + ((size_t)n * (size_t)P + (size_t)p) * (size_t)nk;
    const float inv = inv_wsum ? inv_wsum[n] : inv_default;
    if (inv == 0.f) {      // a sample that is not part of the problem: exact zeros whatever its x holds
        if (tid < nk) out[tid] = 0.0;
        return;
    }
    const int c = p / (RB * CT), rem = p - c * (RB * CT);
    const int i0 = (rem / CT) * BLIND_TH, j0 = (rem % CT) * BLIND_TW;
    const int th = min(BLIND_TH, H - i0), tw = min(BLIND_TW, W - j0);
    const int ah = (kh - 1) >> 1, aw = (kw - 1) >> 1;
    const int h = H / pool, w = W / pool;
    const int ts = BLIND_TW + kw;
    const float* xs = x + (size_t)n * ((size_t)C * H * W) + (size_t)c * H * W;
    const float* rs = resid + (size_t)n * ((size_t)C * h * w) + (size_t)c * h * w;
    // u: the cell's value exactly as phase 2 of k_restore_objective_psf forms it
    const float two_inv = 2.f * inv;      // (exact)
    const float inv_p2 = pool == 1 ? 1.f : 1.f / (float)(pool * pool);
    for (int e = tid; e < th * tw; e += BLIND_NT) {
        const int li = e / tw, lj = e - li * tw;
        ut[li * BLIND_TW + lj] = (two_inv * rs[((i0 + li) / pool) * w + (j0 + lj) / pool]) * inv_p2;
    }
    // x with its halo: image rows i0 - ah .. i0 + th - 1 + ah, columns j0 - aw .. j0 + tw - 1 + aw
    const int rows = th + kh - 1, cols = tw + kw - 1;      // (rows <= BLIND_XROWS, cols <= ts - 1)
    for (int e = tid; e < rows * cols; e += BLIND_NT) {
        const int r = e / cols, q = e - r * cols;
        const int y = i0 - ah + r, xx = j0 - aw + q;
        xt[r * ts + q] = (y >= 0 && y < H && xx >= 0 && xx < W) ? xs[(size_t)y * W + xx] : 0.f;
    }
    __syncthreads();
    const int S = min(BLIND_NT / nk, BLIND_TW);
    const int s = tid / nk, q = tid - s * nk;
    if (s < S) {
        const int a = q / kw, b = q - a * kw;
        const float* xr = xt + (kh - 1 - a) * ts + (kw - 1 - b);
        double acc = 0.0;
        for (int li = 0; li < th; ++li) {
            const float* ur = ut + li * BLIND_TW;
            const float* xl = xr + li * ts;
            static_assert(BLIND_TW <= BLIND_CHAIN, "a chain is one slice of one tile row");
            float chain = 0.f;      // at most BLIND_CHAIN terms
            for (int lj = s; lj < tw; lj += S) chain = __builtin_fmaf(ur[lj], xl[lj], chain);
            acc += (double)chain;
        }
        red[s * nk + q] = acc;
    }
    __syncthreads();
    if (tid < nk) {
        double g = red[tid];
        for (int r = 1; r < S; ++r) g += red[r * nk + tid];
        out[tid] = g;
    }
}

// part: (N, P, nk) doubles.  One workgroup per PSF: `total` partial rows from row `blockIdx.x * rows_per_psf` on
__global__ void __launch_bounds__(BLIND_FNT) k_psf_grad_finish(const double* __restrict__ part, long total, long rows_per_psf, int nk,
                                                               const float* __restrict__ psf, long psf_stride,
                                                               float* __restrict__ grad_psf, float* __restrict__ grad_logits) {
    __shared__ double red[BLIND_FNT];
    __shared__ double kg[BLIND_PSF_MAX * BLIND_PSF_MAX];
    const int tid = threadIdx.x;
    const int G = min(BLIND_FNT / nk, BLIND_FG);
    const int r = tid / nk, q = tid - r * nk;
    const double* base = part + (size_t)blockIdx.x * (size_t)rows_per_psf * (size_t)nk;
    if (r < G) {
        const long chunk = (total + G - 1) / G;
        const long lo = min(total, (long)r * chunk), hi = min(total, lo + chunk);
        double acc = 0.0;
        long i = lo;
        for (; i + 8 <= hi; i += 8) {      // eight loads in flight, added in row order all the same
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = base[(size_t)(i + j) * nk + q];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];
        }
        for (; i < hi; ++i) acc += base[(size_t)i * nk + q];
        red[r * nk + q] = acc;
    }
    __syncthreads();
    double g = 0.0, k = 0.0;
    if (tid < nk) {
        g = red[tid];
        for (int j = 1; j < G; ++j) g += red[j * nk + tid];
        if (grad_psf) grad_psf[(size_t)blockIdx.x * nk + tid] = (float)g;
        if (grad_logits) {
            k = (double)psf[(size_t)blockIdx.x * (size_t)psf_stride + tid];
            kg[tid] = k * g;
        }
    }
    if (!grad_logits) return;      // (uniform)
    __syncthreads();
    if (tid < nk) {
        double dot = 0.0;
        for (int j = 0; j < nk; ++j) dot += kg[j];      // tap order, the same in every thread
        grad_logits[(size_t)blockIdx.x * nk + tid] = (float)(k * (g - dot));
    }
}

// psf[p] = softmax(logits[p]): the max subtracted, the exponentials and their sum in fp64 in tap order, one rounding per tap
__global__ void __launch_bounds__(256) k_psf_from_logits(const float* __restrict__ logits, float* __restrict__ psf, int nk) {
    __shared__ float lg[BLIND_PSF_MAX * BLIND_PSF_MAX];
    __shared__ double ex[BLIND_PSF_MAX * BLIND_PSF_MAX];
    const int tid = threadIdx.x;
    if (tid < nk) lg[tid] = logits[(size_t)blockIdx.x * nk + tid];
    __syncthreads();
    float m = lg[0];
    for (int j = 1; j < nk; ++j) m = lg[j] > m ? lg[j] : m;      // (a NaN logit is never the max; it still makes its tap NaN)
    if (tid < nk) ex[tid] = exp((double)lg[tid] - (double)m);
    __syncthreads();
    if (tid < nk) {
        double sum = 0.0;
        for (int j = 0; j < nk; ++j) sum += ex[j];
        psf[(size_t)blockIdx.x * nk + tid] = (float)(ex[tid] / sum);
    }
}

// the shapes of a gradient call: band and tile counts (functions of C, H, W only) and the scratch
struct BlindGeo {
    long RB, CT, P;
    size_t bytes;
};

static const char* blind_geo(int N, int C, int H, int W, int kh, int kw, int pool, BlindGeo& g) {
    if (N < 0 || C < 1 || H < 1 || W < 1) return "N < 0 or C, H, W < 1";
    if (!(kh >= 1 && kh <= BLIND_PSF_MAX && (kh & 1) && kw >= 1 && kw <= BLIND_PSF_MAX && (kw & 1)))
        return "psf taps: both sides odd, 1 .. 15";
    if (pool < 1) return "pool < 1";
    if (H % pool != 0 || W % pool != 0) return "pool does not divide the image";
    if ((long long)C * H * W >= (1LL << 31)) return "C*H*W elements per sample out of range (>= 2^31)";
    g.RB = (H + BLIND_TH - 1) / BLIND_TH;
    g.CT = (W + BLIND_TW - 1) / BLIND_TW;
    g.P = (long)C * g.RB * g.CT;
    if ((unsigned __int128)g.P * (unsigned)(N > 0 ? N : 1) >= ((unsigned __int128)1 << 31)) return "more than 2^31 workgroups";
    const unsigned __int128 b = (unsigned __int128)g.P * (unsigned)N * (unsigned)(kh * kw) * 8;
    if (b >= ((unsigned __int128)1 << 46)) return "scratch of 2^46 bytes or more";
    g.bytes = align_up((size_t)b, 256);
    if (g.bytes == 0) g.bytes = 256;      // (N == 0: zero is the error value)
    return nullptr;
}

}  // namespace glowhip

using namespace glowhip;

extern "C" int glowhip_psf_from_logits(const float* logits, float* psf, int n_psf, int kh, int kw, glowhip_stream_t stream) {
    GH_REQUIRE(logits && psf, "psf_from_logits: null argument (logits and psf are required)");
    GH_REQUIRE(kh >= 1 && kh <= BLIND_PSF_MAX && (kh & 1) && kw >= 1 && kw <= BLIND_PSF_MAX && (kw & 1),
               "psf_from_logits: psf of %d x %d taps (both sides odd, 1 .. %d)", kh, kw, BLIND_PSF_MAX);
    GH_REQUIRE(n_psf >= 0, "psf_from_logits: n_psf %d", n_psf);
    if (n_psf == 0) return GLOWHIP_OK;
    hipLaunchKernelGGL(k_psf_from_logits, dim3(n_psf), dim3(256), 0, (hipStream_t)stream, logits, psf, kh * kw);
    GH_LAUNCH_CHECK("k_psf_from_logits");
    return GLOWHIP_OK;
}

extern "C" size_t glowhip_restore_psf_grad_scratch_bytes(int N, int C, int H, int W, int kh, int kw, int pool) {
    BlindGeo g;
    if (const char* why = blind_geo(N, C, H, W, kh, kw, pool, g)) {
        set_error("restore_psf_grad_scratch_bytes: %s (N %d, C %d, H %d, W %d, psf %d x %d, pool %d)", why, N, C, H, W, kh, kw, pool);
        return 0;
    }
    return g.bytes;
}

extern "C" int glowhip_restore_psf_grad(const float* x, const float* resid, const float* inv_wsum, const float* psf, long psf_stride,
                                        int kh, int kw, int N, int C, int H, int W, int pool, float* grad_psf, float* grad_logits,
                                        void* scratch, size_t scratch_bytes, glowhip_stream_t stream) {
    GH_REQUIRE(x && resid && (grad_psf || grad_logits),
               "restore_psf_grad: null argument (x and resid are required, and grad_psf or grad_logits)");
    GH_REQUIRE(psf || !grad_logits, "restore_psf_grad: null argument (grad_logits needs the psf)");
    BlindGeo g;
    const char* why = blind_geo(N, C, H, W, kh, kw, pool, g);
    GH_REQUIRE(!why, "restore_psf_grad: %s (N %d, C %d, H %d, W %d, psf %d x %d taps, pool %d)", why, N, C, H, W, kh, kw, pool);
    GH_REQUIRE(psf_stride == 0 || psf_stride >= (long)kh * kw, "restore_psf_grad: psf stride %ld (0: one psf for the batch, or >= %d)",
               psf_stride, kh * kw);
    if (N == 0) return GLOWHIP_OK;
    GH_REQUIRE(scratch && scratch_bytes >= g.bytes && ((size_t)scratch & 15) == 0,
               "restore_psf_grad: scratch %p of %zu bytes (16-byte aligned, >= %zu: glowhip_restore_psf_grad_scratch_bytes)", scratch,
               scratch_bytes, g.bytes);
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(scratch);
    const float inv_default = 1.f / (float)((long long)C * (H / pool) * (W / pool));
    hipLaunchKernelGGL(k_psf_grad_partial, dim3((unsigned)(g.P * N)), dim3(BLIND_NT), 0, s, x, resid, inv_wsum, kh, kw, C, H, W, pool,
                       inv_default, (int)g.RB, (int)g.CT, part);
    GH_LAUNCH_CHECK("k_psf_grad_partial");
    const bool shared = psf_stride == 0;
    hipLaunchKernelGGL(k_psf_grad_finish, dim3(shared ? 1 : N), dim3(BLIND_FNT), 0, s, part, shared ? g.P * N : g.P, g.P, kh * kw, psf,
                       psf_stride, grad_psf, grad_logits);
    GH_LAUNCH_CHECK("k_psf_grad_finish");
    return GLOWHIP_OK;
}

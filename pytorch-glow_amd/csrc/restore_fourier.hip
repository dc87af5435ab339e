// restore_fourier.hip -- the restoration objective observed in the Fourier domain (MRI k-space undersampling, radio interferometry,
// partial-Fourier compressed sensing), and the transform alone.  Per sample n and channel c, with F the unitary 2-D DFT of the H x W
// plane (torch.fft.fft2(norm="ortho"): unshifted, index (0,0) the DC term),
//     X = F x      resid = w (X - t)      loss[n] = inv_wsum[n] sum_{c,k} w |X - t|^2      grad_x = 2 inv_wsum[n] Re(F^H resid)
// (include/glowhip.h has THE definition).  A separable radix-2 FFT in LDS, fp32, one rounding per operation (no fused multiply-add);
// H and W are powers of two from 2 to 256.  THREE launches for the objective, whatever the shape:
//   k_fourier_rows_fwd   grid = planes x row tiles (FT_ROW_ELEMS / W rows each): a tile's real rows into LDS in bit-reversed order,
//                        log2 W decimation-in-time stages, the complex rows into `resid` -- the intermediate between the passes
//   k_fourier_cols       grid = planes x column tiles (32 columns; 16 where H = 256: an H x TC complex tile is at most 32 KiB of LDS,
//                        a 256 x 256 plane would be 512 KiB): the tile's columns from `resid` in bit-reversed order, log2 H
//                        decimation-in-time stages, then ON THE SAME LDS TILE the scaling 1/sqrt(H W), d = X - t, resid = w d (the
//                        output), the loss partial, u = 2 inv resid, and log2 H decimation-in-frequency stages with the conjugate
//                        twiddles -- the column adjoint acts on the same columns, so the spectrum never makes a round trip through
//                        HBM -- and the tile into the scratch in natural order
//   k_fourier_rows_adj   grid = planes x row tiles: complex rows from the scratch, log2 W decimation-in-frequency stages, the real
//                        part times 1/sqrt(H W) into grad_x.  The workgroup of a sample's first tile also folds that sample's loss
//                        partials, in index order, in fp64: no fourth launch
// glowhip_fourier2d is two of the same kernels (rows then columns; the adjoint columns then rows).
// Multi-coil k-space (glowhip_restore_objective_coils, glowhip_coils2d): Y[n,c,q] = F (S[q] x[n,c]) with Q complex sensitivity maps,
// still three launches -- k_coils_rows_fwd loads its tile as (S.re x, S.im x) on N C Q planes; k_fourier_cols<FT_OBJECTIVE, true> is
// the column kernel on N C Q planes with the weight of plane / Q; k_coils_rows_adj, on N C planes, walks the Q coil planes of its row
// tile and sums Re(conj(S) G) in registers, in coil order, a fixed element <-> thread map, and folds the loss.  The plain instances
// compile the coil code out and keep their bits.
// Twiddles: exp(-i pi k / h) for every stage's half-length h, one contiguous run per stage (L - 1 entries), evaluated in fp64
// (sincospi on the exact argument k / h) and rounded once to fp32, built per launch in LDS.
// LDS banks (a wave's 8-byte accesses are served in two halves of 32 lanes; a half is conflict-free when its 32 complex values fall
// in 32 different 8-byte slots of the 256-byte bank row):
//   columns  the lanes of a half run along the tile's columns, so TC >= 32 is conflict-free at every stage as it stands.  TC = 16
//            (H = 256) puts two butterflies in a half; their rows differ by 2 at the first stage and by 1 afterwards, which no row
//            stride serves both ways, so rows 2m and 2m + 1 share one 32-slot line and row i takes the half (i ^ (i >> 1)) & 1 of
//            it: the two rows of a half-wave always land in opposite halves
//   rows     the lanes of a half run along a row's butterflies, whose first operands at half-length h < 32 are the indices with
//            bit log2 h clear: 32 of them span 64 slots, and index j and j + 32 collide.  A pad cannot separate them at every stage
//            (j + 1 has the same bit clear for every h > 1); the index is XOR-swizzled instead, j ^ 31 where bit 5 of j is set,
//            which maps the upper 32 onto the slots the lower 32 leave free, at every stage, and costs no LDS
// (reasoned from the bank rule, not measured).
// No atomics, nothing depends on workgroup order: bitwise the same run to run.  Tile shapes and the butterfly order are functions of
// (H, W) only, never of N, and a workgroup works on one plane of one sample: sample n has the same bits in a batch of 1 and of 64,
// and a non-finite x[n] stays in sample n.  inv_wsum[n] == 0 is decided in k_fourier_cols (zeros into resid and the scratch, without
// reading the spectrum) and again in k_fourier_rows_adj (zeros into grad_x, loss 0).  Global accesses are 8-byte where the address
// allows and 4-byte otherwise: element-wise, the same bits either way.
#include "common.h"

namespace glowhip {

constexpr int FT_NT = 256;               // threads of every kernel here
constexpr int FT_MAX = 256;              // the largest side
constexpr int FT_COL_ELEMS = 4096;       // complex values of a column tile (32 KiB)
constexpr int FT_ROW_ELEMS = 2048;       // complex values of a row tile (16 KiB)

__device__ __forceinline__ int ft_bitrev(int i, int lg) { return (int)(__brev((unsigned)i) >> (32 - lg)); }      // lg >= 1

// tw[h - 1 + k] = exp(-i pi k / h) for h = 1, 2, .. L / 2 and k < h: the twiddles of the stage of half-length h, contiguous
__device__ __forceinline__ void ft_twiddles(float2* tw, int L) {
    for (int e = threadIdx.x; e < L - 1; e += FT_NT) {
        const int h = 1 << (31 - __clz(e + 1));
        const int k = e + 1 - h;
        double s, c;
        sincospi(-(double)k / (double)h, &s, &c);      // (k / h is exact: h is a power of two)
        tw[e] = make_float2((float)c, (float)s);
    }
}

__device__ __forceinline__ float2 ft_ld2(const float* p, bool a8) {
    return a8 ? *reinterpret_cast<const float2*>(p) : make_float2(p[0], p[1]);
}
__device__ __forceinline__ void ft_st2(float* p, float2 v, bool a8) {
    if (a8) *reinterpret_cast<float2*>(p) = v;
    else p[0] = v.x, p[1] = v.y;
}

__device__ __forceinline__ float2 ft_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// one butterfly.  forward (decimation in time): a' = a + w b, b' = a - w b; adjoint (decimation in frequency, conjugate twiddle):
// a' = a + b, b' = conj(w) (a - b)
template <bool ADJ>
__device__ __forceinline__ void ft_butterfly(float2& a, float2& b, float2 w) {
    if (!ADJ) {
        const float2 t = ft_cmul(b, w);
        b = make_float2(a.x - t.x, a.y - t.y);
        a = make_float2(a.x + t.x, a.y + t.y);
    } else {
        const float2 d = make_float2(a.x - b.x, a.y - b.y);
        a = make_float2(a.x + b.x, a.y + b.y);
        b = ft_cmul(d, make_float2(w.x, -w.y));
    }
}

// the slot of (row i, column c) of a column tile of TC = 1 << lgTC columns (the header has the bank argument)
__device__ __forceinline__ int ft_col_at(int i, int c, int lgTC) {
    if (lgTC == 4) return ((i >> 1) << 5) + ((((i ^ (i >> 1)) & 1) << 4) | c);
    return (i << lgTC) + c;
}
// the slot of (row r, index j) of a row tile of rows of W = 1 << lgW values
__device__ __forceinline__ int ft_row_at(int r, int j, int lgW) { return (r << lgW) + (j ^ ((j & 32) ? 31 : 0)); }

// log2 H stages along the columns of a tile; every stage ends with a barrier
template <bool ADJ>
__device__ __forceinline__ void ft_col_stages(float2* tile, const float2* tw, int lgH, int lgTC) {
    const int nb = (1 << (lgH - 1)) << lgTC;
    for (int q = 0; q < lgH; ++q) {
        const int s = ADJ ? lgH - 1 - q : q, h = 1 << s;
        for (int idx = threadIdx.x; idx < nb; idx += FT_NT) {
            const int c = idx & ((1 << lgTC) - 1), b = idx >> lgTC;
            const int k = b & (h - 1), i0 = ((b >> s) << (s + 1)) | k;
            const int p0 = ft_col_at(i0, c, lgTC), p1 = ft_col_at(i0 | h, c, lgTC);
            float2 a = tile[p0], v = tile[p1];
            ft_butterfly<ADJ>(a, v, tw[h - 1 + k]);
            tile[p0] = a, tile[p1] = v;
        }
        __syncthreads();
    }
}

// log2 W stages along the rows of a tile of R = 1 << lgR rows
template <bool ADJ>
__device__ __forceinline__ void ft_row_stages(float2* tile, const float2* tw, int lgW, int lgR) {
    const int nb = (1 << (lgW - 1)) << lgR;
    for (int q = 0; q < lgW; ++q) {
        const int s = ADJ ? lgW - 1 - q : q, h = 1 << s;
        for (int idx = threadIdx.x; idx < nb; idx += FT_NT) {
            const int b = idx & ((1 << (lgW - 1)) - 1), r = idx >> (lgW - 1);
            const int k = b & (h - 1), j0 = ((b >> s) << (s + 1)) | k;
            const int p0 = ft_row_at(r, j0, lgW), p1 = ft_row_at(r, j0 | h, lgW);
            float2 a = tile[p0], v = tile[p1];
            ft_butterfly<ADJ>(a, v, tw[h - 1 + k]);
            tile[p0] = a, tile[p1] = v;
        }
        __syncthreads();
    }
}

// real rows -> complex rows (the forward transform along W, unscaled).  in: (planes, H, W); out: (planes, H, W, 2)
__global__ void __launch_bounds__(FT_NT) k_fourier_rows_fwd(const float* __restrict__ in, float* __restrict__ out, int lgH, int lgW,
                                                            int lgR) {
    __shared__ float2 tile[FT_ROW_ELEMS];
    __shared__ float2 tw[FT_MAX];
    const int W = 1 << lgW, tid = threadIdx.x;
    const int tiles = 1 << (lgH - lgR);
    const size_t plane = blockIdx.x >> (lgH - lgR);
    const int r0 = (int)(blockIdx.x & (unsigned)(tiles - 1)) << lgR;
    const size_t base = ((plane << lgH) + (size_t)r0) << lgW;      // the tile's first element
    const bool a8 = (((size_t)out) & 7) == 0;
    ft_twiddles(tw, W);
    const int ne = W << lgR;
    for (int e = tid; e < ne; e += FT_NT) {
        const int j = e & (W - 1), r = e >> lgW;
        tile[ft_row_at(r, ft_bitrev(j, lgW), lgW)] = make_float2(in[base + e], 0.f);
    }
    __syncthreads();
    ft_row_stages<false>(tile, tw, lgW, lgR);
    for (int e = tid; e < ne; e += FT_NT) {
        const int j = e & (W - 1), r = e >> lgW;
        ft_st2(out + 2 * (base + e), tile[ft_row_at(r, j, lgW)], a8);
    }
}

// complex rows -> real rows: scale Re(the adjoint transform along W).  in: (planes, H, W, 2); out: (planes, H, W).
// The objective's call (inv_wsum or partials given): planes = N C, exact zeros for a sample with inv_wsum[n] == 0, and the workgroup
// of a sample's first tile folds the sample's loss partials (C * col_tiles doubles) in index order
__global__ void __launch_bounds__(FT_NT) k_fourier_rows_adj(const float* __restrict__ in, float* __restrict__ out, int lgH, int lgW,
                                                            int lgR, float scale, const float* __restrict__ inv_wsum, int C,
                                                            float inv_default, const double* __restrict__ partials, int col_tiles,
                                                            float* __restrict__ loss_out) {
    __shared__ float2 tile[FT_ROW_ELEMS];
    __shared__ float2 tw[FT_MAX];
    const int W = 1 << lgW, tid = threadIdx.x;
    const int tiles = 1 << (lgH - lgR);
    const size_t plane = blockIdx.x >> (lgH - lgR);
    const int tix = (int)(blockIdx.x & (unsigned)(tiles - 1));
    const size_t base = ((plane << lgH) + ((size_t)tix << lgR)) << lgW;
    const int ne = W << lgR;
    if (partials) {      // (uniform)
        const size_t n = plane / (size_t)C;
        const float inv = inv_wsum ? inv_wsum[n] : inv_default;
        if (tix == 0 && plane == n * (size_t)C && tid == 0 && loss_out) {
            double tot = 0.0;
            const double* ps = partials + n * (size_t)C * (size_t)col_tiles;
            for (int i = 0; i < C * col_tiles; ++i) tot += ps[i];
            loss_out[n] = inv == 0.f ? 0.f : (float)(tot * (double)inv);
        }
        if (inv == 0.f) {      // not part of the problem: exact zeros
            for (int e = tid; e < ne; e += FT_NT) out[base + e] = 0.f;
            return;
        }
    }
    const bool a8 = (((size_t)in) & 7) == 0;
    ft_twiddles(tw, W);
    for (int e = tid; e < ne; e += FT_NT) {
        const int j = e & (W - 1), r = e >> lgW;
        tile[ft_row_at(r, j, lgW)] = ft_ld2(in + 2 * (base + e), a8);
    }
    __syncthreads();
    ft_row_stages<true>(tile, tw, lgW, lgR);
    for (int e = tid; e < ne; e += FT_NT) {      // (decimation in frequency leaves index j at slot bitrev(j))
        const int j = e & (W - 1), r = e >> lgW;
        out[base + e] = tile[ft_row_at(r, ft_bitrev(j, lgW), lgW)].x * scale;
    }
}

// ---- multi-coil (SENSE): Y[n,c,q] = F (S[q] x[n,c]) with Q complex sensitivity maps, the same for every channel ----
constexpr int FT_COILS_MAX = 32;
constexpr int FT_ROW_OWN = FT_ROW_ELEMS / FT_NT;      // the most elements of a row tile a thread owns (element e belongs to e % FT_NT)

// real rows times the coil's map -> complex rows.  in: (N C, H, W); maps: (Q, H, W, 2) at n * maps_stride; out: (N C Q, H, W, 2).
// The tile is loaded as (S.re x, S.im x) -- two products, one rounding each -- and the stages are k_fourier_rows_fwd's
__global__ void __launch_bounds__(FT_NT) k_coils_rows_fwd(const float* __restrict__ in, const float* __restrict__ maps, long maps_stride,
                                                          float* __restrict__ out, int lgH, int lgW, int lgR, int C, int Q) {
    __shared__ float2 tile[FT_ROW_ELEMS];
    __shared__ float2 tw[FT_MAX];
    const int W = 1 << lgW, tid = threadIdx.x;
    const int tiles = 1 << (lgH - lgR);
    const size_t plane = blockIdx.x >> (lgH - lgR);      // (n C + c) Q + q
    const size_t nc = plane / (size_t)Q, q = plane - nc * (size_t)Q, n = nc / (size_t)C;
    const int r0 = (int)(blockIdx.x & (unsigned)(tiles - 1)) << lgR;
    const size_t base = ((plane << lgH) + (size_t)r0) << lgW;      // the tile's first element of the output
    const size_t xbase = ((nc << lgH) + (size_t)r0) << lgW;
    const float* S = maps + n * (size_t)maps_stride + 2 * (((q << lgH) + (size_t)r0) << lgW);
    const bool a8 = (((size_t)out) & 7) == 0, s8 = (((size_t)maps) & 7) == 0;      // (maps_stride is even)
    ft_twiddles(tw, W);
    const int ne = W << lgR;
    for (int e = tid; e < ne; e += FT_NT) {
        const int j = e & (W - 1), r = e >> lgW;
        const float xv = in[xbase + e];
        const float2 sv = ft_ld2(S + 2 * (size_t)e, s8);
        tile[ft_row_at(r, ft_bitrev(j, lgW), lgW)] = make_float2(sv.x * xv, sv.y * xv);
    }
    __syncthreads();
    ft_row_stages<false>(tile, tw, lgW, lgR);
    for (int e = tid; e < ne; e += FT_NT) {
        const int j = e & (W - 1), r = e >> lgW;
        ft_st2(out + 2 * (base + e), tile[ft_row_at(r, j, lgW)], a8);
    }
}

// complex rows of Q coil planes -> real rows: scale * sum_q Re(conj(S[q]) (the adjoint transform along W)).  in: (N C Q, H, W, 2);
// out: (N C, H, W).  grid = (N C planes) x row tiles; a workgroup walks q = 0 .. Q - 1 over the same row tile of the Q coil planes,
// and each thread adds S.re G.re + S.im G.im for the elements it owns (element e of the tile belongs to thread e % FT_NT, whatever q)
// into fp32 registers, in coil order; one store at the end.  The objective's call (partials given): exact zeros for a sample with
// inv_wsum[n] == 0, and the workgroup of a sample's first tile folds the sample's C Q col_tiles loss partials in index order
__global__ void __launch_bounds__(FT_NT) k_coils_rows_adj(const float* __restrict__ in, const float* __restrict__ maps, long maps_stride,
                                                          float* __restrict__ out, int lgH, int lgW, int lgR, float scale,
                                                          const float* __restrict__ inv_wsum, int C, int Q, float inv_default,
                                                          const double* __restrict__ partials, int col_tiles,
                                                          float* __restrict__ loss_out) {
    __shared__ float2 tile[FT_ROW_ELEMS];
    __shared__ float2 tw[FT_MAX];
    const int W = 1 << lgW, tid = threadIdx.x;
    const int tiles = 1 << (lgH - lgR);
    const size_t nc = blockIdx.x >> (lgH - lgR);
    const size_t n = nc / (size_t)C;
    const int tix = (int)(blockIdx.x & (unsigned)(tiles - 1));
    const size_t toff = ((size_t)tix << lgR) << lgW;      // the tile's first element inside its plane
    const size_t obase = (nc << (lgH + lgW)) + toff;
    const int ne = W << lgR;
    if (partials) {      // (uniform)
        const float inv = inv_wsum ? inv_wsum[n] : inv_default;
        if (tix == 0 && nc == n * (size_t)C && tid == 0 && loss_out) {
            double tot = 0.0;
            const int np = C * Q * col_tiles;
            const double* ps = partials + n * (size_t)np;
            for (int i = 0; i < np; ++i) tot += ps[i];
            loss_out[n] = inv == 0.f ? 0.f : (float)(tot * (double)inv);
        }
        if (inv == 0.f) {      // not part of the problem: exact zeros
            for (int e = tid; e < ne; e += FT_NT) out[obase + e] = 0.f;
            return;
        }
    }
    const bool a8 = (((size_t)in) & 7) == 0, s8 = (((size_t)maps) & 7) == 0;
    ft_twiddles(tw, W);
    float acc[FT_ROW_OWN];
#pragma unroll
    for (int i = 0; i < FT_ROW_OWN; ++i) acc[i] = 0.f;
    for (int q = 0; q < Q; ++q) {
        const float* src = in + 2 * (((nc * (size_t)Q + (size_t)q) << (lgH + lgW)) + toff);
        const float* S = maps + n * (size_t)maps_stride + 2 * (((size_t)q << (lgH + lgW)) + toff);
        for (int e = tid; e < ne; e += FT_NT) {
            const int j = e & (W - 1), r = e >> lgW;
            tile[ft_row_at(r, j, lgW)] = ft_ld2(src + 2 * (size_t)e, a8);
        }
        __syncthreads();
        ft_row_stages<true>(tile, tw, lgW, lgR);
#pragma unroll
        for (int i = 0; i < FT_ROW_OWN; ++i) {      // (decimation in frequency leaves index j at slot bitrev(j))
            const int e = tid + i * FT_NT;
            if (e < ne) {
                const int j = e & (W - 1), r = e >> lgW;
                const float2 G = tile[ft_row_at(r, ft_bitrev(j, lgW), lgW)];
                const float2 sv = ft_ld2(S + 2 * (size_t)e, s8);
                const float term = sv.x * G.x + sv.y * G.y;
                acc[i] = acc[i] + term;
            }
        }
        __syncthreads();      // the tile is read: the next coil may load
    }
#pragma unroll
    for (int i = 0; i < FT_ROW_OWN; ++i) {
        const int e = tid + i * FT_NT;
        if (e < ne) out[obase + e] = acc[i] * scale;
    }
}

enum { FT_OBJECTIVE = 0, FT_FORWARD = 1, FT_ADJOINT = 2 };


// the column pass.  FT_FORWARD: src -> dst = scale * (the transform along H); FT_ADJOINT: src -> dst = the adjoint transform along H,
// unscaled; FT_OBJECTIVE: src = dst_resid = `resid` (the rows' output, overwritten with w (X - t)), the adjoint of 2 inv resid into
// `dst`, the loss partial of the tile into `partials`.  src may be dst: a workgroup reads its columns before it writes them
// COILS (the multi-coil objective, planes = N C Q, `C` holds C Q): the weight is shared by the Q coil planes of a channel, so its cell
// is that of plane / Q; the plain instance compiles this out
template <int MODE, bool COILS = false>
__global__ void __launch_bounds__(FT_NT) k_fourier_cols(const float* src, float* dst, int lgH, int lgW, int lgTC, float scale,
                                                        const float* __restrict__ target, const float* __restrict__ weight,
                                                        const float* __restrict__ inv_wsum, int C, float inv_default, float* resid,
                                                        double* __restrict__ partials, int Q) {
    __shared__ float2 tile[FT_COL_ELEMS];
    __shared__ float2 tw[FT_MAX];
    __shared__ double red[FT_NT / 64];
    const int H = 1 << lgH, TC = 1 << lgTC, tid = threadIdx.x;
    const int tiles = 1 << (lgW - lgTC);
    const size_t plane = blockIdx.x >> (lgW - lgTC);
    const int v0 = (int)(blockIdx.x & (unsigned)(tiles - 1)) << lgTC;
    const size_t pbase = plane << (lgH + lgW);      // the plane's first element
    const int ne = H << lgTC;
    float two_inv = 0.f;
    if (MODE == FT_OBJECTIVE) {
        const size_t n = plane / (size_t)C;
        const float inv = inv_wsum ? inv_wsum[n] : inv_default;
        if (inv == 0.f) {      // (uniform) exact zeros whatever the spectrum holds: it is not read
            const bool z8 = ((((size_t)dst) | ((size_t)resid)) & 7) == 0;
            for (int e = tid; e < ne; e += FT_NT) {
                const size_t g = pbase + ((size_t)(e >> lgTC) << lgW) + (size_t)(v0 + (e & (TC - 1)));
                ft_st2(resid + 2 * g, make_float2(0.f, 0.f), z8);
                ft_st2(dst + 2 * g, make_float2(0.f, 0.f), z8);
            }
            if (tid == 0) partials[blockIdx.x] = 0.0;
            return;
        }
        two_inv = 2.f * inv;      // (exact)
    }
    const bool a8 = ((((size_t)src) | ((size_t)dst)) & 7) == 0;
    ft_twiddles(tw, H);
    for (int e = tid; e < ne; e += FT_NT) {
        const int c = e & (TC - 1), i = e >> lgTC;
        const size_t g = pbase + ((size_t)i << lgW) + (size_t)(v0 + c);
        const float2 v = ft_ld2(src + 2 * g, a8);
        tile[ft_col_at(MODE == FT_ADJOINT ? i : ft_bitrev(i, lgH), c, lgTC)] = v;
    }
    __syncthreads();
    if (MODE != FT_ADJOINT) ft_col_stages<false>(tile, tw, lgH, lgTC);
    if (MODE == FT_FORWARD) {
        for (int e = tid; e < ne; e += FT_NT) {
            const int c = e & (TC - 1), i = e >> lgTC;
            const size_t g = pbase + ((size_t)i << lgW) + (size_t)(v0 + c);
            const float2 v = tile[ft_col_at(i, c, lgTC)];
            ft_st2(dst + 2 * g, make_float2(v.x * scale, v.y * scale), a8);
        }
        return;
    }
    if (MODE == FT_OBJECTIVE) {
        const bool t8 = ((((size_t)target) | ((size_t)resid)) & 7) == 0;
        const size_t wshift = COILS ? pbase - ((plane / (size_t)Q) << (lgH + lgW)) : 0;      // from the plane's cell to the weight's
        double acc = 0.0;
        for (int e = tid; e < ne; e += FT_NT) {
            const int c = e & (TC - 1), i = e >> lgTC;
            const size_t g = pbase + ((size_t)i << lgW) + (size_t)(v0 + c);
            const int p = ft_col_at(i, c, lgTC);
            const float2 X = tile[p];
            const float2 t = ft_ld2(target + 2 * g, t8);
            const float w = weight ? weight[g - wshift] : 1.f;
            const float dr = X.x * scale - t.x, di = X.y * scale - t.y;
            const float rr = w * dr, ri = w * di;
            acc += (double)rr * (double)dr;
            acc += (double)ri * (double)di;
            ft_st2(resid + 2 * g, make_float2(rr, ri), t8);
            tile[p] = make_float2(two_inv * rr, two_inv * ri);
        }
        const double tot = block_sum<FT_NT>(acc, red);      // thread, wave, workgroup; its barriers also publish the tile
        if (tid == 0) partials[blockIdx.x] = tot;
    }
    ft_col_stages<true>(tile, tw, lgH, lgTC);
    for (int e = tid; e < ne; e += FT_NT) {      // (decimation in frequency leaves row i at slot bitrev(i))
        const int c = e & (TC - 1), i = e >> lgTC;
        const size_t g = pbase + ((size_t)i << lgW) + (size_t)(v0 + c);
        ft_st2(dst + 2 * g, tile[ft_col_at(ft_bitrev(i, lgH), c, lgTC)], a8);
    }
}

// the shapes of a call: functions of (H, W) only, and the carving of the scratch
struct FtGeo {
    int lgH, lgW, lgR, lgTC;
    long planes;
    unsigned row_blocks, col_blocks;
    int col_tiles;
    float scale;
    size_t off_part, bytes;      // the complex intermediate at 0
};

static int ft_log2(int v) {
    int lg = 0;
    while ((1 << lg) < v) ++lg;
    return lg;
}

static const char* ft_geo(long planes, int H, int W, FtGeo& g) {
    if (planes < 0) return "a negative count";
    if (H < 2 || W < 2 || H > FT_MAX || W > FT_MAX || (H & (H - 1)) || (W & (W - 1)))
        return "H and W must each be a power of two from 2 to 256";
    g.lgH = ft_log2(H), g.lgW = ft_log2(W);
    const int R = FT_ROW_ELEMS / W < H ? FT_ROW_ELEMS / W : H;
    const int cap = FT_COL_ELEMS / H < 32 ? FT_COL_ELEMS / H : 32;
    const int TC = cap < W ? cap : W;
    g.lgR = ft_log2(R), g.lgTC = ft_log2(TC);
    g.planes = planes;
    g.col_tiles = W / TC;
    const unsigned __int128 rb = (unsigned __int128)planes * (unsigned)(H / R), cb = (unsigned __int128)planes * (unsigned)(W / TC);
    if (rb >= (1u << 31) || cb >= (1u << 31)) return "more than 2^31 workgroups";
    g.row_blocks = (unsigned)rb, g.col_blocks = (unsigned)cb;
    g.scale = (float)(1.0 / sqrt((double)H * (double)W));
    g.off_part = align_up((size_t)planes * (size_t)H * (size_t)W * 8, 256);
    g.bytes = g.off_part + align_up((size_t)cb * 8, 256);
    if (g.bytes == 0) g.bytes = 256;      // (N == 0: zero is the error value)
    return nullptr;
}

static bool ft_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *p = (const char*)a, *q = (const char*)b;
    return p < q + nb && q < p + na;
}

}  // namespace glowhip

using namespace glowhip;

extern "C" size_t glowhip_restore_fourier_scratch_bytes(int N, int C, int H, int W) {
    FtGeo g;
    const char* why = (N < 0 || C < 1) ? "N < 0 or C < 1" : ft_geo((long)N * (long)C, H, W, g);
    if (why) {
        set_error("restore_fourier_scratch_bytes: %s (N %d, C %d, H %d, W %d)", why, N, C, H, W);
        return 0;
    }
    return g.bytes;
}

extern "C" int glowhip_restore_objective_fourier(const float* x, const float* target, const float* weight, const float* inv_wsum,
                                                 int N, int C, int H, int W, float* resid, float* grad_x, float* loss_out,
                                                 void* scratch, size_t scratch_bytes, glowhip_stream_t stream) {
    GH_REQUIRE(x && target && resid && grad_x, "restore_objective_fourier: null argument (x, target, resid and grad_x are required)");
    GH_REQUIRE(N >= 0 && C >= 1, "restore_objective_fourier: N < 0 or C < 1 (N %d, C %d)", N, C);
    FtGeo g;
    const char* why = ft_geo((long)N * (long)C, H, W, g);
    GH_REQUIRE(!why, "restore_objective_fourier: %s (N %d, C %d, H %d, W %d)", why, N, C, H, W);
    if (N == 0) return GLOWHIP_OK;
    GH_REQUIRE(scratch && scratch_bytes >= g.bytes && ((size_t)scratch & 15) == 0,
               "restore_objective_fourier: scratch %p of %zu bytes (16-byte aligned, >= %zu: glowhip_restore_fourier_scratch_bytes)",
               scratch, scratch_bytes, g.bytes);
    const size_t real_bytes = (size_t)g.planes * (size_t)H * (size_t)W * 4;
    GH_REQUIRE(!ft_overlap(x, real_bytes, grad_x, real_bytes) && !ft_overlap(x, real_bytes, resid, 2 * real_bytes) &&
                   !ft_overlap(grad_x, real_bytes, resid, 2 * real_bytes),
               "restore_objective_fourier: x, grad_x and resid must not overlap");
    hipStream_t s = (hipStream_t)stream;
    float* inter = reinterpret_cast<float*>(scratch);
    double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + g.off_part);
    const float inv_default = 1.f / (float)((long)C * H * W);
    hipLaunchKernelGGL(k_fourier_rows_fwd, dim3(g.row_blocks), dim3(FT_NT), 0, s, x, resid, g.lgH, g.lgW, g.lgR);
    GH_LAUNCH_CHECK("k_fourier_rows_fwd");
    hipLaunchKernelGGL(k_fourier_cols<FT_OBJECTIVE>, dim3(g.col_blocks), dim3(FT_NT), 0, s, (const float*)resid, inter, g.lgH, g.lgW,
                       g.lgTC, g.scale, target, weight, inv_wsum, C, inv_default, resid, partials, 1);
    GH_LAUNCH_CHECK("k_fourier_cols");
    hipLaunchKernelGGL(k_fourier_rows_adj, dim3(g.row_blocks), dim3(FT_NT), 0, s, (const float*)inter, grad_x, g.lgH, g.lgW, g.lgR,
                       g.scale, inv_wsum, C, inv_default, (const double*)partials, g.col_tiles, loss_out);
    GH_LAUNCH_CHECK("k_fourier_rows_adj");
    return GLOWHIP_OK;
}

extern "C" int glowhip_fourier2d(const float* in, float* out, long planes, int H, int W, int adjoint, glowhip_stream_t stream) {
    GH_REQUIRE(in && out, "fourier2d: null argument");
    GH_REQUIRE(adjoint == 0 || adjoint == 1, "fourier2d: adjoint = %d (0: real to complex, 1: complex to real)", adjoint);
    FtGeo g;
    const char* why = ft_geo(planes, H, W, g);
    GH_REQUIRE(!why, "fourier2d: %s (planes %ld, H %d, W %d)", why, planes, H, W);
    if (planes == 0) return GLOWHIP_OK;
    const size_t real_bytes = (size_t)planes * (size_t)H * (size_t)W * 4;
    GH_REQUIRE(!ft_overlap(in, adjoint ? 2 * real_bytes : real_bytes, out, adjoint ? real_bytes : 2 * real_bytes),
               "fourier2d: in and out must not overlap");
    hipStream_t s = (hipStream_t)stream;
    if (!adjoint) {
        hipLaunchKernelGGL(k_fourier_rows_fwd, dim3(g.row_blocks), dim3(FT_NT), 0, s, in, out, g.lgH, g.lgW, g.lgR);
        GH_LAUNCH_CHECK("k_fourier_rows_fwd");
        hipLaunchKernelGGL(k_fourier_cols<FT_FORWARD>, dim3(g.col_blocks), dim3(FT_NT), 0, s, (const float*)out, out, g.lgH, g.lgW,
                           g.lgTC, g.scale, nullptr, nullptr, nullptr, 1, 0.f, nullptr, nullptr, 1);
        GH_LAUNCH_CHECK("k_fourier_cols");
        return GLOWHIP_OK;
    }
    // the adjoint's intermediate is complex and `out` is real: it comes from the stream's memory pool and goes back to it in stream
    // order (no host sync; this direction is therefore not for a captured region -- the objective call above is)
    void* inter = nullptr;
    hipError_t e = hipMallocAsync(&inter, 2 * real_bytes, s);
    if (e != hipSuccess || !inter) {
        set_error("fourier2d: hipMallocAsync of %zu bytes: %s", 2 * real_bytes, hipGetErrorString(e));
        return GLOWHIP_ELAUNCH;
    }
    hipLaunchKernelGGL(k_fourier_cols<FT_ADJOINT>, dim3(g.col_blocks), dim3(FT_NT), 0, s, in, (float*)inter, g.lgH, g.lgW, g.lgTC,
                       g.scale, nullptr, nullptr, nullptr, 1, 0.f, nullptr, nullptr, 1);
    hipError_t e1 = hipGetLastError();
    if (e1 == hipSuccess) {
        hipLaunchKernelGGL(k_fourier_rows_adj, dim3(g.row_blocks), dim3(FT_NT), 0, s, (const float*)inter, out, g.lgH, g.lgW, g.lgR,
                           g.scale, nullptr, 1, 0.f, nullptr, 0, nullptr);
        e1 = hipGetLastError();
    }
    (void)hipFreeAsync(inter, s);
    if (e1 != hipSuccess) {
        set_error("fourier2d (adjoint): %s", hipGetErrorString(e1));
        return GLOWHIP_ELAUNCH;
    }
    return GLOWHIP_OK;
}

// ---- multi-coil ----
// the checks the three coil entry points share: the counts, the stride of the maps and the shapes (planes = N C Q)
static const char* coils_geo(int N, int C, int Q, int H, int W, long maps_stride, bool with_stride, FtGeo& g) {
    if (N < 0 || C < 1) return "N < 0 or C < 1";
    if (Q < 1 || Q > FT_COILS_MAX) return "Q must be from 1 to 32 coils";
    const char* why = ft_geo((long)N * (long)C * (long)Q, H, W, g);
    if (why) return why;
    if (with_stride && maps_stride != 0 && maps_stride != (long)Q * H * W * 2)
        return "maps_stride must be 0 (maps shared by the batch) or Q*H*W*2 (per sample)";
    return nullptr;
}

extern "C" size_t glowhip_restore_coils_scratch_bytes(int N, int C, int Q, int H, int W) {
    FtGeo g;
    const char* why = coils_geo(N, C, Q, H, W, 0, false, g);
    if (why) {
        set_error("restore_coils_scratch_bytes: %s (N %d, C %d, Q %d, H %d, W %d)", why, N, C, Q, H, W);
        return 0;
    }
    return g.bytes;
}

extern "C" int glowhip_restore_objective_coils(const float* x, const float* target, const float* weight, const float* inv_wsum,
                                               const float* maps, long maps_stride, int N, int C, int Q, int H, int W, float* resid,
                                               float* grad_x, float* loss_out, void* scratch, size_t scratch_bytes,
                                               glowhip_stream_t stream) {
    GH_REQUIRE(x && target && maps && resid && grad_x,
               "restore_objective_coils: null argument (x, target, maps, resid and grad_x are required)");
    FtGeo g;
    const char* why = coils_geo(N, C, Q, H, W, maps_stride, true, g);
    GH_REQUIRE(!why, "restore_objective_coils: %s (N %d, C %d, Q %d, H %d, W %d, maps_stride %ld)", why, N, C, Q, H, W, maps_stride);
    if (N == 0) return GLOWHIP_OK;
    GH_REQUIRE(scratch && scratch_bytes >= g.bytes && ((size_t)scratch & 15) == 0,
               "restore_objective_coils: scratch %p of %zu bytes (16-byte aligned, >= %zu: glowhip_restore_coils_scratch_bytes)",
               scratch, scratch_bytes, g.bytes);
    const size_t real_bytes = (size_t)N * (size_t)C * (size_t)H * (size_t)W * 4, resid_bytes = (size_t)g.planes * (size_t)H * (size_t)W * 8;
    const size_t maps_bytes = (maps_stride ? (size_t)N : (size_t)1) * (size_t)Q * (size_t)H * (size_t)W * 8;
    GH_REQUIRE(!ft_overlap(x, real_bytes, grad_x, real_bytes) && !ft_overlap(x, real_bytes, resid, resid_bytes) &&
                   !ft_overlap(grad_x, real_bytes, resid, resid_bytes) && !ft_overlap(maps, maps_bytes, grad_x, real_bytes) &&
                   !ft_overlap(maps, maps_bytes, resid, resid_bytes) && !ft_overlap(maps, maps_bytes, x, real_bytes),
               "restore_objective_coils: x, grad_x, resid and maps must not overlap");
    hipStream_t s = (hipStream_t)stream;
    float* inter = reinterpret_cast<float*>(scratch);
    double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + g.off_part);
    const float inv_default = 1.f / (float)((long)C * Q * H * W);
    const unsigned adj_blocks = g.row_blocks / (unsigned)Q;      // (N C planes) x row tiles
    hipLaunchKernelGGL(k_coils_rows_fwd, dim3(g.row_blocks), dim3(FT_NT), 0, s, x, maps, maps_stride, resid, g.lgH, g.lgW, g.lgR, C, Q);
    GH_LAUNCH_CHECK("k_coils_rows_fwd");
    hipLaunchKernelGGL((k_fourier_cols<FT_OBJECTIVE, true>), dim3(g.col_blocks), dim3(FT_NT), 0, s, (const float*)resid, inter, g.lgH,
                       g.lgW, g.lgTC, g.scale, target, weight, inv_wsum, C * Q, inv_default, resid, partials, Q);
    GH_LAUNCH_CHECK("k_fourier_cols (coils)");
    hipLaunchKernelGGL(k_coils_rows_adj, dim3(adj_blocks), dim3(FT_NT), 0, s, (const float*)inter, maps, maps_stride, grad_x, g.lgH,
                       g.lgW, g.lgR, g.scale, inv_wsum, C, Q, inv_default, (const double*)partials, g.col_tiles, loss_out);
    GH_LAUNCH_CHECK("k_coils_rows_adj");
    return GLOWHIP_OK;
}

extern "C" int glowhip_coils2d(const float* in, const float* maps, long maps_stride, float* out, int N, int C, int Q, int H, int W,
                               int adjoint, glowhip_stream_t stream) {
    GH_REQUIRE(in && maps && out, "coils2d: null argument");
    GH_REQUIRE(adjoint == 0 || adjoint == 1, "coils2d: adjoint = %d (0: real to complex, 1: complex to real)", adjoint);
    FtGeo g;
    const char* why = coils_geo(N, C, Q, H, W, maps_stride, true, g);
    GH_REQUIRE(!why, "coils2d: %s (N %d, C %d, Q %d, H %d, W %d, maps_stride %ld)", why, N, C, Q, H, W, maps_stride);
    if (N == 0) return GLOWHIP_OK;
    const size_t real_bytes = (size_t)N * (size_t)C * (size_t)H * (size_t)W * 4, cplx_bytes = (size_t)g.planes * (size_t)H * (size_t)W * 8;
    const size_t maps_bytes = (maps_stride ? (size_t)N : (size_t)1) * (size_t)Q * (size_t)H * (size_t)W * 8;
    const size_t in_bytes = adjoint ? cplx_bytes : real_bytes, out_bytes = adjoint ? real_bytes : cplx_bytes;
    GH_REQUIRE(!ft_overlap(in, in_bytes, out, out_bytes) && !ft_overlap(maps, maps_bytes, out, out_bytes),
               "coils2d: in, maps and out must not overlap");
    hipStream_t s = (hipStream_t)stream;
    const unsigned adj_blocks = g.row_blocks / (unsigned)Q;
    if (!adjoint) {
        hipLaunchKernelGGL(k_coils_rows_fwd, dim3(g.row_blocks), dim3(FT_NT), 0, s, in, maps, maps_stride, out, g.lgH, g.lgW, g.lgR, C, Q);
        GH_LAUNCH_CHECK("k_coils_rows_fwd");
        hipLaunchKernelGGL(k_fourier_cols<FT_FORWARD>, dim3(g.col_blocks), dim3(FT_NT), 0, s, (const float*)out, out, g.lgH, g.lgW,
                           g.lgTC, g.scale, nullptr, nullptr, nullptr, 1, 0.f, nullptr, nullptr, 1);
        GH_LAUNCH_CHECK("k_fourier_cols");
        return GLOWHIP_OK;
    }
    // as glowhip_fourier2d's adjoint: the complex intermediate comes from the stream's memory pool (not for a captured region)
    void* inter = nullptr;
    hipError_t e = hipMallocAsync(&inter, cplx_bytes, s);
    if (e != hipSuccess || !inter) {
        set_error("coils2d: hipMallocAsync of %zu bytes: %s", cplx_bytes, hipGetErrorString(e));
        return GLOWHIP_ELAUNCH;
    }
    hipLaunchKernelGGL(k_fourier_cols<FT_ADJOINT>, dim3(g.col_blocks), dim3(FT_NT), 0, s, in, (float*)inter, g.lgH, g.lgW, g.lgTC,
                       g.scale, nullptr, nullptr, nullptr, 1, 0.f, nullptr, nullptr, 1);
    hipError_t e1 = hipGetLastError();
    if (e1 == hipSuccess) {
        hipLaunchKernelGGL(k_coils_rows_adj, dim3(adj_blocks), dim3(FT_NT), 0, s, (const float*)inter, maps, maps_stride, out, g.lgH,
                           g.lgW, g.lgR, g.scale, nullptr, C, Q, 0.f, nullptr, 0, nullptr);
        e1 = hipGetLastError();
    }
    (void)hipFreeAsync(inter, s);
    if (e1 != hipSuccess) {
        set_error("coils2d (adjoint): %s", hipGetErrorString(e1));
        return GLOWHIP_ELAUNCH;
    }
    return GLOWHIP_OK;
}

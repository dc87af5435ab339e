// invconv_lu.hip -- the LU-parameterised invertible 1x1 convolution (invconv_lu.h): W = P L U_f with L = tril(l, -1) + I and
// U_f = triu(u, 1) + diag(sign_s exp(log_s)) kept as parameters.  Three kernels, each batched over the LU layers of a plan by a
// device-resident job table (grid.y or grid.z = layer), fp64 accumulation, fp32 stores -- like lu.hip, but nothing here searches a
// pivot or eliminates:
//   k_invconv_lu_assemble   W = P L U_f, one 32 x 32 output tile per workgroup; the first workgroup of a layer also writes the
//                           layer's log-det slot (sum of log_s in fp64) and its constant, as k_step_prepare_* fills them
//   k_invconv_lu_inverse    W^-1 = U_f^-1 L^-1 P^T: grid (column block, layer), 16 right-hand-side columns per workgroup in LDS
//                           (fp64), L and U_f streamed through LDS in 16-row panels; a thread owns (column, row of the panel) for
//                           the panel's update and one thread per column finishes the 16 x 16 triangle
//   k_invconv_lu_backward   dl = strict-lower(P^T G U_f^T), du = strict-upper(L^T P^T G), dlog_s from the diagonal of the latter
// Masked entries (l on / above, u on / below the diagonal) are never LOADED: whatever they hold cannot reach an output.
#include <algorithm>

#include "invconv_lu.h"

namespace glowhip {

template <class J>
__device__ __forceinline__ double lu_diag(const J& j, int i) { return (double)j.sign_s[i] * exp((double)j.log_s[i]); }

// acc[q] (rows ty + 8 q, column tx of the tile) += sA[row][k] * sB[k][col] over one 32-wide k panel
__device__ __forceinline__ void lu_tile_fma(const double (*sA)[33], const double (*sB)[33], int tx, int ty, double (&acc)[4]) {
#pragma unroll 8
    for (int kk = 0; kk < 32; ++kk) {
        const double b = sB[kk][tx];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(sA[ty + 8 * q][kk], b, acc[q]);
    }
}

__global__ void __launch_bounds__(256) k_invconv_lu_assemble(const LuJob* __restrict__ jobs, const LuJob single, char* packed) {
    __shared__ double sA[32][33], sB[32][33];
    __shared__ double red[4];
    const LuJob j = jobs ? jobs[blockIdx.y] : single;
    const int C = j.C, nt = (C + 31) / 32, tid = threadIdx.x;
    if ((int)blockIdx.x >= nt * nt) return;
    const int r0 = ((int)blockIdx.x / nt) * 32, c0 = ((int)blockIdx.x % nt) * 32;
    const int tx = tid & 31, ty = tid >> 5;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int kend = min(C, c0 + 32);            // U_f[k][c] = 0 for k > c
    for (int k0 = 0; k0 < kend; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q, hi = e >> 5, lo = e & 31;
            {   // L row of the permuted output row: sA[row][k]
                const int r = r0 + hi, k = k0 + lo;
                double v = 0.0;
                if (r < C && k < C) {
                    const int pr = j.perm[r];
                    if (k < pr) v = (double)j.l[(long)pr * C + k];
                    else if (k == pr) v = 1.0;
                }
                sA[hi][lo] = v;
            }
            {   // U_f: sB[k][col]
                const int k = k0 + hi, c = c0 + lo;
                double v = 0.0;
                if (k < C && c < C) {
                    if (k < c) v = (double)j.u[(long)k * C + c];
                    else if (k == c) v = lu_diag(j, k);
                }
                sB[hi][lo] = v;
            }
        }
        __syncthreads();
        lu_tile_fma(sA, sB, tx, ty, acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = r0 + ty + 8 * q, c = c0 + tx;
        if (r < C && c < C) j.w[(long)r * C + c] = (float)acc[q];
    }
    if (blockIdx.x != 0) return;
    // log|det W| = sum(log_s), and the step's data-independent log-det term (lu.hip k_step_prepare_batched)
    double a = 0.0;
    for (int i = tid; i < C; i += 256) a += (double)j.log_s[i];
    const double lad = block_sum<256>(a, red);
    double b = 0.0;
    if (j.an_logs)
        for (int k = tid; k < C; k += 256) b += (double)(j.an_logs[k] * LOGSCALE);
    const double tot = block_sum<256>(b, red);
    if (tid == 0) {
        float* lo = packed ? (float*)(packed + j.logabsdet_off) : j.logabsdet;
        if (lo) *lo = (float)lad;
        if (packed && j.an_logs) *(double*)(packed + j.konst_off) = tot * (double)j.HW + (double)(float)lad * (double)j.HW;
    }
}

// LDS of the inverse kernel: Y [Cp][16] doubles | D [Cp] doubles | panel [16][C + 1] floats, Cp = C rounded up to 16
static inline size_t lu_inverse_lds_bytes(int C) {
    const size_t Cp = (size_t)(C + 15) / 16 * 16;
    return Cp * 16 * sizeof(double) + Cp * sizeof(double) + (size_t)16 * (C + 1) * sizeof(float);
}

__global__ void __launch_bounds__(256) k_invconv_lu_inverse(const LuJob* __restrict__ jobs, const LuJob single, char* packed) {
    extern __shared__ __attribute__((aligned(16))) double lu_lds[];
    const LuJob j = jobs ? jobs[blockIdx.y] : single;
    const int C = j.C, tid = threadIdx.x;
    const int cb0 = (int)blockIdx.x * 16;
    if (cb0 >= C) return;
    float* winv = packed ? (float*)(packed + j.winv_off) : j.winv;
    const int Cp = (C + 15) / 16 * 16, ps = C + 1;
    double* Y = lu_lds;                      // Y[i * 16 + cl]: row i of solution column cb0 + cl
    double* D = Y + (size_t)Cp * 16;         // the diagonal of U_f
    float* Pn = (float*)(D + Cp);            // the current 16-row panel of l / u, row stride ps
    const int cl = tid & 15, r = tid >> 4;
    const int c = cb0 + cl;
    const int pc = c < C ? j.perm[c] : -1;   // column c of P^T is e_perm[c]
    for (int i = r; i < Cp; i += 16) Y[i * 16 + cl] = (i == pc) ? 1.0 : 0.0;
    for (int i = tid; i < Cp; i += 256) D[i] = i < C ? lu_diag(j, i) : 1.0;
    // y = L^-1 P^T e_c, top down
    for (int I0 = 0; I0 < C; I0 += 16) {
        __syncthreads();
        {
            const int row = I0 + r;
            for (int k = cl; k < I0 + 16 && k < C; k += 16) Pn[r * ps + k] = (row < C && k < row) ? j.l[(long)row * C + k] : 0.f;
        }
        __syncthreads();
        {
            const int row = I0 + r;
            double acc = Y[row * 16 + cl];
            for (int k = 0; k < I0; ++k) acc = fma(-(double)Pn[r * ps + k], Y[k * 16 + cl], acc);
            Y[row * 16 + cl] = acc;
        }
        __syncthreads();
        if (r == 0) {
            for (int t = 1; t < 16 && I0 + t < C; ++t) {
                double v = Y[(I0 + t) * 16 + cl];
                for (int q = 0; q < t; ++q) v = fma(-(double)Pn[t * ps + I0 + q], Y[(I0 + q) * 16 + cl], v);
                Y[(I0 + t) * 16 + cl] = v;
            }
        }
    }
    // x = U_f^-1 y, bottom up
    for (int I0 = Cp - 16; I0 >= 0; I0 -= 16) {
        __syncthreads();
        {
            const int row = I0 + r;
            for (int k = I0 + cl; k < C; k += 16) Pn[r * ps + k] = (row < C && k > row) ? j.u[(long)row * C + k] : 0.f;
        }
        __syncthreads();
        {
            const int row = I0 + r;
            double acc = Y[row * 16 + cl];
            for (int k = I0 + 16; k < C; ++k) acc = fma(-(double)Pn[r * ps + k], Y[k * 16 + cl], acc);
            Y[row * 16 + cl] = acc;
        }
        __syncthreads();
        if (r == 0) {
            for (int t = 15; t >= 0; --t) {
                if (I0 + t >= C) continue;
                double v = Y[(I0 + t) * 16 + cl];
                for (int q = t + 1; q < 16 && I0 + q < C; ++q) v = fma(-(double)Pn[t * ps + I0 + q], Y[(I0 + q) * 16 + cl], v);
                Y[(I0 + t) * 16 + cl] = v / D[I0 + t];
            }
        }
    }
    __syncthreads();
    if (c < C)
        for (int i = r; i < C; i += 16) winv[(long)i * C + c] = (float)Y[i * 16 + cl];
}

// grid (tile, product, layer): product 0 = dl, product 1 = du and dlog_s
__global__ void __launch_bounds__(256) k_invconv_lu_backward(const LuGradJob* __restrict__ jobs, const LuGradJob single) {
    __shared__ double sA[32][33], sB[32][33];
    __shared__ int s_src[32];                    // source row of dw for a row of P^T G: (P^T G)[perm[i]] = G[i]
    const LuGradJob j = jobs ? jobs[blockIdx.z] : single;
    const int C = j.C, nt = (C + 31) / 32, tid = threadIdx.x;
    if ((int)blockIdx.x >= nt * nt) return;
    const int r0 = ((int)blockIdx.x / nt) * 32, c0 = ((int)blockIdx.x % nt) * 32;
    const int tx = tid & 31, ty = tid >> 5;
    const int which = blockIdx.y;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    auto find_src = [&](int base) {              // s_src[q] = i with perm[i] == base + q
        for (int i = tid; i < C; i += 256) {
            const int pr = j.perm[i] - base;
            if (pr >= 0 && pr < 32) s_src[pr] = i;
        }
    };
    if (which == 0) {
        // dl[r][c] = sum_{k >= c} (P^T G)[r][k] U_f[c][k] for c < r
        if (c0 < r0 + 32) {
            find_src(r0);
            for (int k0 = c0; k0 < C; k0 += 32) {
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = tid + 256 * q, hi = e >> 5, lo = e & 31;
                    {
                        const int r = r0 + hi, k = k0 + lo;
                        sA[hi][lo] = (r < C && k < C) ? (double)j.dw[(long)s_src[hi] * C + k] : 0.0;
                    }
                    {
                        const int cc = c0 + hi, k = k0 + lo;
                        double v = 0.0;
                        if (cc < C && k < C) {
                            if (k > cc) v = (double)j.u[(long)cc * C + k];
                            else if (k == cc) v = lu_diag(j, cc);
                        }
                        sB[lo][hi] = v;
                    }
                }
                __syncthreads();
                lu_tile_fma(sA, sB, tx, ty, acc);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + ty + 8 * q, cc = c0 + tx;
            if (r < C && cc < C) j.dl[(long)r * C + cc] = cc < r ? (float)acc[q] : 0.f;
        }
        return;
    }
    // B[r][c] = sum_{k >= r} L[k][r] (P^T G)[k][c] for c >= r
    if (c0 + 32 > r0) {
        for (int k0 = r0; k0 < C; k0 += 32) {
            __syncthreads();
            find_src(k0);
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = tid + 256 * q, hi = e >> 5, lo = e & 31;
                {
                    const int k = k0 + hi, r = r0 + lo;
                    double v = 0.0;
                    if (k < C && r < C) {
                        if (k > r) v = (double)j.l[(long)k * C + r];
                        else if (k == r) v = 1.0;
                    }
                    sA[lo][hi] = v;
                }
                {
                    const int k = k0 + hi, cc = c0 + lo;
                    sB[hi][lo] = (k < C && cc < C) ? (double)j.dw[(long)s_src[hi] * C + cc] : 0.0;
                }
            }
            __syncthreads();
            lu_tile_fma(sA, sB, tx, ty, acc);
        }
    }
    const double term = j.gsum ? j.gsum[0] * j.term_mul : j.term_mul;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = r0 + ty + 8 * q, cc = c0 + tx;
        if (r < C && cc < C) {
            j.du[(long)r * C + cc] = cc > r ? (float)acc[q] : 0.f;
            if (cc == r) j.dlog_s[r] = (float)(acc[q] * lu_diag(j, r) + term);
        }
    }
}

static inline int lu_tiles(int max_c) { const int nt = (max_c + 31) / 32; return nt * nt; }

int launch_invconv_lu_assemble(const LuJob* jobs_dev, const LuJob* single, int n, int max_c, void* packed, hipStream_t s) {
    if (n <= 0) return GLOWHIP_OK;
    GH_REQUIRE(max_c > 0 && (jobs_dev || (single && n == 1)), "invconv_lu assemble: bad job table");
    hipLaunchKernelGGL(k_invconv_lu_assemble, dim3(lu_tiles(max_c), n), dim3(256), 0, s, jobs_dev, single ? *single : LuJob{}, (char*)packed);
    GH_LAUNCH_CHECK("k_invconv_lu_assemble");
    return GLOWHIP_OK;
}

int launch_invconv_lu_inverse(const LuJob* jobs_dev, const LuJob* single, int n, int max_c, void* packed, hipStream_t s) {
    if (n <= 0) return GLOWHIP_OK;
    GH_REQUIRE(max_c > 0 && max_c <= INVCONV_LU_MAX_C && (jobs_dev || (single && n == 1)), "invconv_lu inverse: C=%d unsupported", max_c);
    const size_t lds = lu_inverse_lds_bytes(max_c);
    if (lds > 32 * 1024)
        (void)hipFuncSetAttribute((const void*)k_invconv_lu_inverse, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_invconv_lu_inverse, dim3((max_c + 15) / 16, n), dim3(256), lds, s, jobs_dev, single ? *single : LuJob{}, (char*)packed);
    GH_LAUNCH_CHECK("k_invconv_lu_inverse");
    return GLOWHIP_OK;
}

int launch_invconv_lu_backward(const LuGradJob* jobs_dev, const LuGradJob* single, int n, int max_c, hipStream_t s) {
    if (n <= 0) return GLOWHIP_OK;
    GH_REQUIRE(max_c > 0 && (jobs_dev || (single && n == 1)), "invconv_lu backward: bad job table");
    hipLaunchKernelGGL(k_invconv_lu_backward, dim3(lu_tiles(max_c), 2, n), dim3(256), 0, s, jobs_dev, single ? *single : LuGradJob{});
    GH_LAUNCH_CHECK("k_invconv_lu_backward");
    return GLOWHIP_OK;
}

}  // namespace glowhip

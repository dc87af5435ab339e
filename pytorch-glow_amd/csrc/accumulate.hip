// accumulate.hip -- gradient accumulation for the reference's training step (network/trainer.py:123-150) run as k micro-batches:
// the gradients of one optimiser step are carried across micro-steps in accumulators parallel to the plan's flat gradient buckets.
// ONE launch for all buckets; the segment table travels by value in the kernel arguments (no device table, no upload; capturable).
//     FIRST : acc = g                    (no memset ever precedes a round)
//     ADD   : acc = acc + g
//     FINISH: g   = (acc + g) * scale    (acc is not written)
// Per element, fp32, one rounding per operation (the build has fp contraction off).  Element-wise: the 16-byte path, the peeled
// head, the tail and the element-by-element path all give the same bits.  No atomics, no LDS, no dependence on workgroup order.
#include <math.h>
#include <stdint.h>

#include "common.h"

namespace glowhip {

constexpr int ACC_MAX_SEGS = 16;
constexpr int ACC_MAX_BLOCKS = 2048;     // memory-bound grid cap; the tiles beyond it are reached by the grid-stride loop
// A tile is 256 threads x ACC_UNROLL accesses of 16 bytes, every load of a full tile in flight before its first store.  Measured on
// config B's 44 M elements: 0.080 ms with 4, 0.085 ms with 1 (which is torch.add's time); on 3 M elements the two do not differ.
constexpr int ACC_UNROLL = 4;
constexpr int ACC_TILE = 256 * 4 * ACC_UNROLL;

// Segment s owns the tiles [tile0[s], tile0[s + 1]).  Its first `head` elements (< 4; n when no common 16-byte phase exists) are
// handled one by one by its first tile; tile t covers the elements [head + t * ACC_TILE, head + (t + 1) * ACC_TILE) below n.
// Entries of tile0 behind the last segment hold the total, so a tile's segment is the number of entries 1 .. 15 it has reached:
// the scan reads the table at constant offsets (one trip to the kernel arguments, not one per entry).
struct acc_table {
    float* grad[ACC_MAX_SEGS];
    float* acc[ACC_MAX_SEGS];
    long long n[ACC_MAX_SEGS];
    int tile0[ACC_MAX_SEGS + 1];
    int head[ACC_MAX_SEGS];     // -1: element by element throughout (grad and acc share no 16-byte phase)
};

template <int MODE>
__device__ __forceinline__ void acc_elem(float& g, float& a, float scale) {
    if (MODE == GLOWHIP_ACC_FIRST) a = g;
    else if (MODE == GLOWHIP_ACC_ADD) a = a + g;
    else g = (a + g) * scale;
}

template <int MODE>
__device__ __forceinline__ void acc_scalar(float* grad, float* acc, long long i, float scale) {
    float g = grad[i], a = MODE == GLOWHIP_ACC_FIRST ? 0.f : acc[i];
    acc_elem<MODE>(g, a, scale);
    if (MODE == GLOWHIP_ACC_FINISH) grad[i] = g;
    else acc[i] = a;
}

template <int MODE>
__device__ __forceinline__ void acc_vec(float4& g, float4& a, float scale) {
    acc_elem<MODE>(g.x, a.x, scale); acc_elem<MODE>(g.y, a.y, scale);
    acc_elem<MODE>(g.z, a.z, scale); acc_elem<MODE>(g.w, a.w, scale);
}

template <int MODE>
__global__ void __launch_bounds__(256) k_grad_accumulate(const acc_table t, float scale) {
    const int total = t.tile0[ACC_MAX_SEGS];
    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
        int s = 0;                                               // the segment of this tile: <= 16 prefix entries, block-uniform
#pragma unroll
        for (int i = 1; i < ACC_MAX_SEGS; ++i) s += tile >= t.tile0[i] ? 1 : 0;
        float* grad = t.grad[s];
        float* acc = t.acc[s];
        const long long n = t.n[s];
        const int local = tile - t.tile0[s];
        const bool vec = t.head[s] >= 0;
        const long long head = vec ? t.head[s] : 0;
        if (local == 0 && (long long)threadIdx.x < head) acc_scalar<MODE>(grad, acc, threadIdx.x, scale);
        const long long lo = head + (long long)local * ACC_TILE;
        const long long hi = lo + ACC_TILE < n ? lo + ACC_TILE : n;
        const int nv = vec ? (int)((hi - lo) >> 2) : 0;           // whole 16-byte accesses of this tile
        float4* g4 = reinterpret_cast<float4*>(grad + lo);
        float4* a4 = reinterpret_cast<float4*>(acc + lo);
        if (nv == ACC_TILE / 4) {                                 // a full tile: every load in flight before the first store
            float4 g[ACC_UNROLL], a[ACC_UNROLL];
#pragma unroll
            for (int u = 0; u < ACC_UNROLL; ++u) {
                g[u] = g4[threadIdx.x + 256 * u];
                if (MODE != GLOWHIP_ACC_FIRST) a[u] = a4[threadIdx.x + 256 * u];
            }
#pragma unroll
            for (int u = 0; u < ACC_UNROLL; ++u) {
                acc_vec<MODE>(g[u], a[u], scale);
                if (MODE == GLOWHIP_ACC_FINISH) g4[threadIdx.x + 256 * u] = g[u];
                else a4[threadIdx.x + 256 * u] = a[u];
            }
        } else {
            for (int v = threadIdx.x; v < nv; v += 256) {
                float4 g = g4[v], a = g;
                if (MODE != GLOWHIP_ACC_FIRST) a = a4[v];
                acc_vec<MODE>(g, a, scale);
                if (MODE == GLOWHIP_ACC_FINISH) g4[v] = g;
                else a4[v] = a;
            }
            for (long long i = lo + 4LL * nv + threadIdx.x; i < hi; i += 256)      // the n % 4 tail (or the whole tile, unaligned)
                acc_scalar<MODE>(grad, acc, i, scale);
        }
    }
}

}  // namespace glowhip

using namespace glowhip;

extern "C" int glowhip_grad_accumulate(const glowhip_grad_seg* segs, int n_segs, int mode, float scale, glowhip_stream_t stream) {
    GH_REQUIRE(n_segs >= 0 && n_segs <= ACC_MAX_SEGS, "grad_accumulate: n_segs %d (0 .. %d)", n_segs, ACC_MAX_SEGS);
    GH_REQUIRE(mode == GLOWHIP_ACC_FIRST || mode == GLOWHIP_ACC_ADD || mode == GLOWHIP_ACC_FINISH,
               "grad_accumulate: mode %d (0 = first, 1 = add, 2 = finish)", mode);
    GH_REQUIRE(mode != GLOWHIP_ACC_FINISH || isfinite(scale), "grad_accumulate: finish with a non-finite scale");
    if (n_segs == 0) return GLOWHIP_OK;
    GH_REQUIRE(segs, "grad_accumulate: null segment table");
    acc_table t = {};
    long long tiles = 0;
    int k = 0;
    for (int i = 0; i < n_segs; ++i) {
        const glowhip_grad_seg& sg = segs[i];
        GH_REQUIRE(sg.n >= 0, "grad_accumulate: segment %d has n = %lld", i, (long long)sg.n);
        if (sg.n == 0) continue;                                  // legal, skipped
        GH_REQUIRE(sg.grad && sg.acc, "grad_accumulate: segment %d (n = %lld) has a null pointer", i, (long long)sg.n);
        GH_REQUIRE((((uintptr_t)sg.grad | (uintptr_t)sg.acc) & 3) == 0, "grad_accumulate: segment %d is not 4-byte aligned", i);
        GH_REQUIRE(sg.n <= (1LL << 36), "grad_accumulate: segment %d has more than 2^36 elements", i);      // (the tile index is an int)
        const uintptr_t pg = (uintptr_t)sg.grad & 15, pa = (uintptr_t)sg.acc & 15;
        long long head = pg == pa ? (long long)((16 - pg) & 15) / 4 : -1;      // elements up to the common 16-byte boundary
        if (head > sg.n) head = sg.n;
        const long long body = sg.n - (head < 0 ? 0 : head);
        t.grad[k] = sg.grad; t.acc[k] = sg.acc; t.n[k] = sg.n; t.head[k] = (int)head;
        t.tile0[k] = (int)tiles;
        tiles += body == 0 ? 1 : (body + ACC_TILE - 1) / ACC_TILE;
        ++k;
    }
    if (k == 0) return GLOWHIP_OK;
    for (int i = k; i <= ACC_MAX_SEGS; ++i) t.tile0[i] = (int)tiles;
    const dim3 grid((unsigned)(tiles < ACC_MAX_BLOCKS ? tiles : ACC_MAX_BLOCKS)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (mode == GLOWHIP_ACC_FIRST) hipLaunchKernelGGL(k_grad_accumulate<GLOWHIP_ACC_FIRST>, grid, block, 0, s, t, scale);
    else if (mode == GLOWHIP_ACC_ADD) hipLaunchKernelGGL(k_grad_accumulate<GLOWHIP_ACC_ADD>, grid, block, 0, s, t, scale);
    else hipLaunchKernelGGL(k_grad_accumulate<GLOWHIP_ACC_FINISH>, grid, block, 0, s, t, scale);
    GH_LAUNCH_CHECK("k_grad_accumulate");
    return GLOWHIP_OK;
}

// backward.h -- launcher interface of the gradient kernels (backward.hip) used by plan_train.hip.
#pragma once
#include "common.h"

namespace glowhip {

// What a launcher of the HBM-bound gradient kernels chose (testing: glowhip_debug_bwd fills a glowhip_bwd_info from it; the sweep
// passes no pointer).  kernel: GLOWHIP_BWI_* of include/glowhip.h; the other fields as in glowhip_bwd_info.
struct BwdLaunchInfo { int kernel, grid[3], threads_per_channel, w_lds, lds_bytes, mix_blocks, rblocks, plain_stores, launches; };

struct CouplingBwdArgs {
    const float* hout;       // (N,Cout,HW) saved post-scale output of f.4
    const float* z2out; long z_bs;   // second half of the step output (z2')
    const float* g2; long g_bs;      // incoming gradient of z2'   (second half of g_out)
    float* gy2;                      // outgoing gradient of y2 (same strides as g2; may alias g2)
    float* gpre;             // (N,Cout,HW) gradient of (conv + bias) of f.4
    const float* e4;         // (Cout) exp(3 logs)
    const float* gld;        // (N) dL/dlogdet_n
    double* acc_b; double* acc_l;    // (Cout) f.4 bias / logs gradient accumulators
    int N, Ch, Cout, HW, affine;
    int acc_copies = 1; long acc_stride = 0;   // as in ChanMixBwdArgs: workgroup b adds into copy b % acc_copies (k_coupling_bwd4)
};
int launch_coupling_bwd(const CouplingBwdArgs& a, hipStream_t s, BwdLaunchInfo* info = nullptr);      // non-null: what was launched (testing)

struct SplitBwdArgs {
    const float* hout;       // (N,2Ch,HW) saved prior conv output
    const float* z2; long z_bs;      // the split-off half
    float* gz2; long g_bs;           // its gradient (written)
    float* gpre;             // (N,2Ch,HW)
    const float* e4; const float* gld;
    double* acc_b; double* acc_l;
    int N, Ch, HW;
};
int launch_split_bwd(const SplitBwdArgs& a, hipStream_t s, BwdLaunchInfo* info = nullptr);

int launch_act_bwd(float* g, const float* h, const float* e, int N, int Cm, int HW, double* acc_b, double* acc_l,
                   hipStream_t s, BwdLaunchInfo* info = nullptr);

struct ChanMixBwdArgs {
    const float* x; long x_bs;       // step input
    const float* gy; float* gx; long g_bs;   // gradient of y in, gradient of x out (may alias)
    const float* bias; const float* scale;   // actnorm bias, exp(3 logs)
    const float* matrix;             // W (C,C) or null
    const int32_t* gather_inv;       // inverse permutation table or null
    double* acc_w; double* acc_b; double* acc_l;
    int N, C, HW;
    // the accumulators exist in acc_copies copies acc_stride doubles apart (workgroup b adds into copy b % acc_copies; the
    // finalize job sums them): 1024 workgroups x (C^2 + 2C) fp64 atomics on ten cache lines ran at the rate of those lines'
    // L2 channels (35 us per launch, whatever the level)
    int acc_copies = 1; long acc_stride = 0;
    // add_part != null: the gradient of y's FIRST add_C channels is gy + add_scale * (the partial sums a backward k_cnet launch left
    // in add_part: MS row-split copies + halo rows, geometry add_*) -- gathered here instead of by a k_cbwd_finish launch
    const float* add_part = nullptr; float add_scale = 0.f;
    int add_C = 0, add_MS = 0, add_tiles = 0, add_R = 0, add_NI = 0, add_lpxt = 0, add_H = 0, add_W = 0;
    int w_lds = 0;     // (set by launch_chanmix_bwd: the matrix is staged in LDS)
};
struct WgradReduceJobs;
// reduce != null: the split-K reductions of the FlowStep's weight-gradient GEMMs run in the same launch (k_chanmix_bwd_reduce)
// C > CHANMIX_BWD_NARROW_C: k_chanmix_bwd_wide (pixel blocks x channel slices) -- gx must not alias gy, add_part is refused
int launch_chanmix_bwd(const ChanMixBwdArgs& a, hipStream_t s, const WgradReduceJobs* reduce = nullptr, BwdLaunchInfo* info = nullptr);
constexpr int CHANMIX_BWD_NARROW_C = 192;      // k_chanmix_bwd's three C x 65 LDS arrays: 150 KB of a CU's 160
constexpr int CHANMIX_BWD_MAX_C = 512;         // (the forward mixer's limit, launch_chanmix)
constexpr int CHANMIX_BWD_WIDE_PX = 32;        // pixels of a k_chanmix_bwd_wide workgroup
constexpr int CHANMIX_BWD_WIDE_COPIES = 8;     // ... whose launch uses one accumulator copy per pixel block, at most this many
inline bool chanmix_bwd_wide(int C) { return C > CHANMIX_BWD_NARROW_C; }
inline int chanmix_bwd_wide_copies(long pixels) {
    const long blocks = (pixels + CHANMIX_BWD_WIDE_PX - 1) / CHANMIX_BWD_WIDE_PX;
    return (int)(blocks < 1 ? 1 : blocks > CHANMIX_BWD_WIDE_COPIES ? CHANMIX_BWD_WIDE_COPIES : blocks);
}

// ---- decode_bwd.hip: vector-Jacobian products of the decode direction (glowhip_plan_decode_vjp); no parameter gradients
// words[n] = 2^-e, words[N + n] = 2^e, e = floor(log2 max|g[n]|) (0 for an all-zero or non-finite sample)
int launch_grad_norm(const float* g, long per, float* words, int N, hipStream_t s);
int launch_scale_rows(const float* x, float* y, long per, const float* word, int N, hipStream_t s);      // y[n] = x[n] * word[n]
struct ChanMixInvBwdArgs {
    const float* gx; float* gu; long g_bs;   // gradient of the step's input x in, of the mixer's input u out (may alias where C <= CHANMIX_BWD_NARROW_C)
    const float* inv_scale;                  // exp(-3 logs)
    const float* matrix;                     // W^-1 (C,C) or null
    const int32_t* gather;                   // FORWARD permutation table or null
    int N, C, HW;
    // add_part != null: the first add_C channels of gx are gx + add_scale * (the partial sums the PREVIOUS step's backward k_cnet
    // launch left: geometry add_*, as in ChanMixBwdArgs); refused above CHANMIX_BWD_NARROW_C
    const float* add_part = nullptr; float add_scale = 0.f;
    int add_C = 0, add_MS = 0, add_tiles = 0, add_R = 0, add_NI = 0, add_lpxt = 0, add_H = 0, add_W = 0;
    int w_lds = 0;
};
int launch_chanmix_inv_bwd(const ChanMixInvBwdArgs& a, hipStream_t s);
int launch_cpart_finish(const ChanMixInvBwdArgs& a, hipStream_t s);      // gather-only: gu[:add_C] = gx[:add_C] + add_scale * partial sums
struct CouplingInvBwdArgs {
    const float* hout;               // (N,Cout,HW) post-scale output of f.4
    const float* z2out; long z_bs;   // second half of the step output (z2')
    float* g2; long g_bs;            // gradient of y2 in, of z2' out (in place)
    float* gpre;                     // (N,Cout,HW) gradient of (conv + bias) of f.4
    const float* e4;                 // (Cout) exp(3 logs)
    int N, Ch, Cout, HW, affine;
};
int launch_coupling_inv_bwd(const CouplingInvBwdArgs& a, hipStream_t s);
struct SplitInvBwdArgs {
    const float* hout;               // (N,2Ch,HW) prior conv output
    const float* z2; long z_bs;      // the sampled half
    const float* gz2; long g_bs;     // its gradient
    float* geps; long eps_bs;        // caller's buffer of this split (null: skipped), its batch stride
    const float* unscale;            // (N) factor that undoes the sweep's normalisation
    float* gpre;                     // (N,2Ch,HW)
    const float* e4;
    int N, Ch, HW;
};
int launch_split_inv_bwd(const SplitInvBwdArgs& a, hipStream_t s);
int launch_relu_bwd(float* g, const float* h, const float* e, int N, int Cm, int HW, hipStream_t s);      // k_act_bwd without accumulators

int launch_prior_bwd(const float* z, const float* mean, const float* logs, long ml_bs, const float* gld,
                     const float* gz_in, float* gz, int N, long per, hipStream_t s, BwdLaunchInfo* info = nullptr);
int launch_weight_flipT(const float* w, float* wT, int Cout, int Cin, int ksize, hipStream_t s);
int launch_wgrad_direct(const float* gy, const float* x, long x_bs, float* dw, int N, int Cin, int H, int W, int Cout,
                        int ksize, hipStream_t s);
// ---- wgrad_mfma.hip
int launch_shift_expand(const float* src, long src_bs, float* out, int N, int C, int H, int W, int rows_pad, int sign,
                        hipStream_t s);
bool wgrad_mfma_supported(int HW, int Mpad, int Npad);
size_t wgrad_mfma_partial_floats(int Mpad, int Npad, int N, int HW);
// operand (0: A, 1: B) of a weight-gradient GEMM given as the (N, C, H, W) tensor whose shift-expanded rows (c * 9 + tap) it stands for
// (what launch_shift_expand would write): the GEMM's loader gathers them itself.  The operand pointer / batch stride are the tensor's.
// operand < 0: none, both operands are plain.
struct WgradTaps { int operand, C, H, W, sign; };
// WgradGemm::layout (f16-pipe kernel, plain operands; the values are those of glowhip_wgrad_gemm.tiled and of the kernels' WgArgs)
constexpr int WGRAD_A_TILED = 1;       // A / B is pixel-tile-major [pixel / 32][rows][pixel % 32] over the batch's pixels (what the taping /
constexpr int WGRAD_B_TILED = 2;       // backward k_cnet write, sh.h), rows = Mpad / Npad; its batch stride is unused
constexpr int WGRAD_A_PRESCALED = 4;   // A holds g * sh_scale * 2^11 (the backward k_cnet's g_u2 / g_u0); row sums and dW come out as for g
// One weight-gradient GEMM: partial[split] = A B^T over a slice of the batch's pixels, dw = their sum in the layer's weight layout
// (wgrad_reduce.h: mode).  The fields of the public glowhip_wgrad_gemm, plus the taps.
struct WgradGemm {
    const float* A; long a_bs; const float* B; long b_bs;   // (Mpad, HW) / (Npad, HW) per image, batch strides in elements
    float* partial; float* dw;
    int Mpad, Npad, Mreal, Nreal, mode;
    double* rowsum = nullptr;          // (f16-pipe kernel) rowsum[m] += sum over all pixels of A's row m -- the bias gradient when A = g_u
    WgradTaps taps{-1, 0, 0, 1, 0};
    int b_valid = 0;                   // > 0 (f16-pipe kernel, plain B): only that many rows of B exist, the rest of the column tile is zero
    int b_half = 0;                    // 1 (f16-pipe kernel, plain B): B points at an fp16 tensor (the taped h1 / h2), b_bs in elements
    int layout = 0;                    // OR of WGRAD_A_TILED / WGRAD_B_TILED / WGRAD_A_PRESCALED
};
// what all GEMMs of a launch share.  sh_scale > 0: f16-pipe kernels, the gradient operand A pre-scaled by it; 0: the fp32 pipe
struct WgradBatch { int N, HW; float sh_scale; };
struct WgradReduceJob;
// What a weight-gradient launcher chose for one GEMM (testing: glowhip_debug_wgrad fills a glowhip_wgrad_info from it; the
// sweep passes no pointer).  instance: GLOWHIP_WGI_* of include/glowhip.h; blocks: workgroups of this GEMM, `live` of them with a tile.
struct WgradLaunchInfo { int instance, splits, ktiles_per_split, blocks, live; };
// defer != null: skip the split-K reduction, describe it in *defer instead;  info != null: what was launched (testing)
int launch_wgrad_mfma(const WgradGemm& g, const WgradBatch& b, hipStream_t s, WgradReduceJob* defer = nullptr, WgradLaunchInfo* info = nullptr);
// The GEMMs of one FlowStep behind the backward k_cnet as ONE launch (wgrad_mfma.hip): g[0] = f.4's (A = gathered g_pre, B = h2 fp16
// pixel-tile-major), g[1] = f.0's (A = g_u0 pixel-tile-major and pre-scaled, B = gathered y1) and, n == 3, g[2] = f.2's (A = g_u2,
// B = h1 fp16, both pixel-tile-major, A pre-scaled).  GLOWHIP_EINVAL (nothing launched) for anything else; the caller asks
// wgrad_pair_ok for the shapes first.  The reduction of g[i] is described in *defer[i]; info[i] <- g[i]'s share of the launch.
bool wgrad_pair_ok(int HW, int m4, int hid, int n0);
int launch_wgrad_group(const WgradGemm* g, int n, const WgradBatch& b, WgradReduceJob* const* defer, hipStream_t s, WgradLaunchInfo* info = nullptr);
// fp16 pixel-tile-major [pixel / 32][R][pixel % 32] -> fp32 (N, R, HW): a taped hidden tensor for the per-layer backward kernels
int launch_half_to_float(const void* src_half, float* dst, int N, int R, int HW, hipStream_t s);
struct WgradReduceJob { const float* partial; float* dw; int splits, Mpad, Npad, Mreal, Nreal, mode; };
struct WgradReduceJobs { WgradReduceJob job[3]; int n; };
int launch_wgrad_reduce_batched(const WgradReduceJobs& j, hipStream_t s);

// one launch for all reduction-type parameter gradients of a backward sweep
struct GradJob {
    const double* acc; float* out; int n;
    double add_mul;          // out[i] = acc[i] + gsum * add_mul            (winv == null)
    const float* winv; int C; // out[o*C+i] = acc[o*C+i] + gsum * add_mul * winv[i*C+o]   (invconv weight)
    int copies = 1; long stride = 0;   // acc[i] = sum over copies of acc[copy * stride + i]
};
int launch_grad_finalize_batched(const GradJob* jobs_dev, int n_jobs, const double* gsum, hipStream_t s);
// ActNorm log-scale gradient of a convolution layer y = (conv(x, W) + b) * exp(3 logs) from its weight and bias gradients:
//   d logs[r] = 3 sum_p g_y y = 3 sum_p g_u (u + b) = 3 (<W[r], dW[r]> + b[r] db[r]),   g_u = g_y exp(3 logs), u = conv(x, W)
// (sum_p g_u[r][p] u[r][p] = sum_k W[r][k] sum_p g_u[r][p] x_k[p] = <W[r], dW[r]>): no pass over the activations at all.
struct LogsJob { const float* w; const float* dw; const float* b; const double* db; float* out; int rows, K; };
int launch_logs_from_dw_batched(const LogsJob* jobs_dev, int n_jobs, hipStream_t s);
int launch_sum_gld(const float* gld, int N, double* gsum, hipStream_t s);
int launch_gld_from_nll(const float* nll_grad, float* gld, int N, double inv, hipStream_t s);

}  // namespace glowhip

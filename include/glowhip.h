/*
 * glowhip.h -- C ABI of the MI355X-native Glow flow engine (libglowhip.so, gfx950).
 *
 * The reference (corenel/pytorch-glow) has no FFI: its hot path is the Python module surface of
 * network/module.py, network/model.py and misc/ops.py.  Each entry point below names the reference
 * function (file:line) whose arithmetic it replaces; the Python shells in
 * pytorch-glow_amd/network/{module,model}.py bind them with ctypes.
 *
 * Conventions
 *   - plain C: device pointers, sizes and an opaque stream handle (a hipStream_t passed as void*);
 *     no torch / C++ types cross the boundary;
 *   - every tensor is fp32, NCHW, contiguous unless a stride argument says otherwise; every pointer is
 *     a DEVICE pointer on the device the stream belongs to (exceptions are marked HOST);
 *   - no allocation, no host synchronisation, no global mutable state inside: workspaces are passed in;
 *     calls are asynchronous on `stream` and re-entrant (one plan must not be executed concurrently on
 *     two streams with the same workspace);
 *   - return value: 0 on success, a negative GLOWHIP_E* code otherwise; glowhip_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 */
#ifndef GLOWHIP_H
#define GLOWHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOWHIP_VERSION 102 /* 0.1.2 */

#define GLOWHIP_OK 0
#define GLOWHIP_EINVAL (-1)    /* bad argument (shape, null pointer, unsupported value) */
#define GLOWHIP_ELAUNCH (-2)   /* HIP launch / runtime error */
#define GLOWHIP_EWORKSPACE (-3)/* workspace too small */

typedef void* glowhip_stream_t; /* hipStream_t */

int glowhip_version(void);
const char* glowhip_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Single-layer primitives (module surface of network/module.py)
 * ---------------------------------------------------------------------------------------------- */

/* Squeeze2d.squeeze / unsqueeze, network/module.py:551-592.
 * reverse=0: x (N,C,H,W) -> y (N,C*f*f,H/f,W/f), y[n, c*f*f+i*f+j, h, w] = x[n, c, h*f+i, w*f+j]
 * reverse=1: x (N,C,H,W) -> y (N,C/(f*f),H*f,W*f) (exact inverse).  C,H,W describe the INPUT. */
int glowhip_squeeze2d(const float* x, float* y, int N, int C, int H, int W, int factor, int reverse,
                      glowhip_stream_t stream);

/* ActNorm data-dependent initialisation, network/module.py:86-120 (batch_variance=False):
 * bias[c] = -mean_{n,h,w} x;  logs[c] = log(scale / (sqrt(mean (x+bias)^2) + 1e-6)) / 3.
 * x may be a channel slice of a wider tensor: element (n,c,p) is x[n*batch_stride + c*HW + p]. */
int glowhip_actnorm_init(const float* x, long batch_stride, int N, int C, int HW, float scale,
                         float* bias, float* logs, glowhip_stream_t stream);
/* The same with ActNorm(batch_variance=True), network/module.py:109-110: bias per channel as above, but ONE log-scale for all
 * channels from the second moment pooled over every dimension: logs[c] = log(scale / (sqrt(mean_{n,c,h,w} (x+bias)^2) + 1e-6)) / 3. */
int glowhip_actnorm_init_batch_variance(const float* x, long batch_stride, int N, int C, int HW, float scale,
                                        float* bias, float* logs, glowhip_stream_t stream);

/* ActNorm.forward, network/module.py:122-149.  reverse=0: y=(x+bias)*exp(3 logs); reverse=1:
 * y = x*exp(-3 logs) - bias.  If logdet_out != NULL: logdet_out[n] = (logdet_in ? logdet_in[n] : 0)
 * +/- 3*sum(logs)*HW. */
int glowhip_actnorm(const float* x, float* y, const float* bias, const float* logs, int N, int C, int HW,
                    int reverse, const float* logdet_in, float* logdet_out, glowhip_stream_t stream);

/* In-kernel LU (Gauss-Jordan, partial pivoting, fp64) of one C x C matrix: replaces torch.det /
 * Tensor.inverse at network/module.py:357,365.  winv (C*C, may be NULL) <- W^-1,
 * logabsdet (1 float) <- log|det W|.  scratch: >= glowhip_invconv_scratch_bytes(C) bytes. */
size_t glowhip_invconv_scratch_bytes(int C);
int glowhip_invconv_prepare(const float* w, int C, float* winv, float* logabsdet, void* scratch,
                            glowhip_stream_t stream);

/* Invertible1x1Conv.forward, network/module.py:344-369: y[n,o,p] = sum_i m[o,i] x[n,i,p] where m is the
 * matrix to APPLY (W forward, W^-1 reverse, from glowhip_invconv_prepare).  If logdet_out != NULL:
 * logdet_out[n] = logdet_in[n] + sign * logabsdet[0] * HW with sign=+1 (reverse=0) / -1 (reverse=1). */
int glowhip_invconv(const float* x, float* y, const float* m, const float* logabsdet, int N, int C, int HW,
                    int reverse, const float* logdet_in, float* logdet_out, glowhip_stream_t stream);

/* Permutation2d.forward, network/module.py:392-397: y[:, o] = x[:, idx[o]] (idx: C int32, device). */
int glowhip_permute_channels(const float* x, float* y, const int32_t* idx, int N, int C, int HW,
                             glowhip_stream_t stream);

/* Conv2d / Conv2dZeros forward, network/module.py:252-259 and :295-297, 'SAME' padding, stride 1,
 * ksize in {1,3}:  v = conv(x, w) + (bias ? bias[o] : 0);
 *                  v = (v + (post_bias ? post_bias[o] : 0)) * (post_logs ? exp(3*post_logs[o]) : 1);
 *                  y = relu ? max(v,0) : v.
 * Conv2d(+ActNorm): bias=NULL, post_bias/post_logs = actnorm.bias/logs.  Conv2dZeros: bias, post_logs=logs.
 * x element (n,ci,p) at x[n*x_batch_stride + ci*H*W + p] (lets z1 = first half of a wider tensor be read
 * in place); y contiguous (N,Cout,H,W); w (Cout,Cin,k,k). */
int glowhip_conv2d(const float* x, long x_batch_stride, const float* w, const float* bias, float* y,
                   int N, int Cin, int H, int W, int Cout, int ksize,
                   const float* post_bias, const float* post_logs, int relu, glowhip_stream_t stream);

/* GaussianDiag.logp, network/module.py:453-467: out[n] = (in ? in[n] : 0) +
 * sum_{c,p} -0.5*(log(2pi) + 2*logs + (x-mean)^2/exp(2*logs)).  mean/logs may be NULL (= 0).
 * Element (n,c,p) of x/mean/logs at base[n*stride + c*HW + p].  scratch16N: 16*N bytes (per-sample fixed-point accumulator +
 * sticky non-finite flag: a NaN / inf term makes out[n] NaN, it is never dropped).
 * Range: the kernel adds one partial sum v per 256 elements of a sample.  With P = ceil(C*HW / 256) <= 2^17 - 1 (checked: more is
 * GLOWHIP_EINVAL) and every |v| < 2^43 nats, out[n] is in[n] + the exact sum of the partials, each rounded to 2^-32 nats, rounded to
 * fp64 and stored as fp32 -- at any magnitude of the sum, beyond the 2^31 nats of the fixed-point word too.  A partial with |v| >= 2^43 makes
 * out[n] -inf / +inf by its sign (NaN when both signs occur).  out[n] is never a finite value that is not that sum. */
int glowhip_gaussian_logp(const float* x, long x_stride, const float* mean, const float* logs, long ml_stride,
                          int N, int C, int HW, const float* in, float* out, void* scratch16N,
                          glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Flow plans: FlowStep / Split2d / Squeeze2d stacks executed by one call
 * (FlowStep.normal_flow/reverse_flow network/model.py:82-154, Split2d.forward network/module.py:511-536,
 *  FlowModel.encode/decode network/model.py:263-294, Glow.normal_flow network/model.py:409-452)
 * ---------------------------------------------------------------------------------------------- */
enum { GLOWHIP_LAYER_SQUEEZE = 0, GLOWHIP_LAYER_FLOWSTEP = 1, GLOWHIP_LAYER_SPLIT2D = 2 };
enum { GLOWHIP_PERM_INVCONV = 0, GLOWHIP_PERM_GATHER = 1 };   /* 'invconv' | 'reverse'/'shuffle' */
enum { GLOWHIP_COUPLING_ADDITIVE = 0, GLOWHIP_COUPLING_AFFINE = 1 };

/* One layer of a FlowModel; C,H,W are the layer's INPUT shape.  Parameter pointers are device pointers
 * to the live parameters (state_dict layout of the reference).  They are read by
 * glowhip_plan_pack (derived data) AND by encode/decode (biases, weights of the direct kernels), so
 * they must stay valid -- same addresses -- for the life of the plan. */
typedef struct glowhip_layer_desc {
    int32_t kind;
    int32_t C, H, W;
    int32_t hidden;        /* FLOWSTEP: hidden_channels */
    int32_t permutation;   /* FLOWSTEP: GLOWHIP_PERM_* */
    int32_t coupling;      /* FLOWSTEP: GLOWHIP_COUPLING_* */
    int32_t reserved;
    const float* an_bias;  const float* an_logs;            /* actnorm.{bias,logs}        (C) */
    const float* invconv_w;                                 /* invconv.weight             (C,C) */
    const int32_t* perm_idx; const int32_t* perm_idx_inv;   /* Permutation2d tables       (C) */
    const float* f0_w; const float* f0_an_bias; const float* f0_an_logs; /* f.0: (hid,C/2,3,3),(hid),(hid) */
    const float* f2_w; const float* f2_an_bias; const float* f2_an_logs; /* f.2: (hid,hid,1,1),(hid),(hid) */
    const float* f4_w; const float* f4_bias;    const float* f4_logs;    /* f.4 / Split2d.conv2d_zeros:
                                                                            (Cout,Cin,3,3),(Cout),(Cout) */
} glowhip_layer_desc;

typedef struct glowhip_plan glowhip_plan;

/* Build a plan (HOST bookkeeping only; descs are copied).  Returns NULL on error. */
glowhip_plan* glowhip_plan_create(const glowhip_layer_desc* layers, int n_layers);
void glowhip_plan_destroy(glowhip_plan* plan);

/* Bytes of the persistent packed-parameter buffer / of the per-call workspace for batch N. */
size_t glowhip_plan_packed_bytes(const glowhip_plan* plan);
size_t glowhip_plan_workspace_bytes(const glowhip_plan* plan, int N);

/* Re-derive everything that depends only on the parameters (exp(3 logs), K-major re-layout of the
 * convolution weights for the MFMA kernels, in-kernel LU -> log|det W| and W^-1) into `packed`.
 * Call after the parameters changed (optimizer step, load_state_dict, ActNorm init). */
int glowhip_plan_pack(glowhip_plan* plan, void* packed, size_t packed_bytes, glowhip_stream_t stream);
/* The same, restricted to the weight images a caller is going to use: GLOWHIP_PACK_INFERENCE = what encode / decode /
 * glow_forward read (the split-half images where those kernels apply), GLOWHIP_PACK_TRAINING = what glow_forward_train /
 * glow_backward read (exact-fp32 images + the flipped/transposed input-gradient images).  glowhip_plan_pack = both.
 * Scale tables and log|det W| are always refreshed, W^-1 with GLOWHIP_PACK_INVERSE or GLOWHIP_PACK_TRAINING. */
#define GLOWHIP_PACK_INFERENCE 1
#define GLOWHIP_PACK_TRAINING 2
#define GLOWHIP_PACK_INVERSE 4   /* W^-1 of the invertible 1x1 convolutions (decode; implied by TRAINING): without it
                                    log|det W| comes from an LU of the matrix alone (C^3/3 instead of 2 C^3 updates) and W^-1 is stale */
int glowhip_plan_pack_for(glowhip_plan* plan, void* packed, size_t packed_bytes, int use, glowhip_stream_t stream);
/* Part of a pack -- the LU factorisations (their log|det W| enters only a forward's final sum) and the weight images only the
 * deep levels read -- runs on a side stream the plan owns, forked from `stream` and joined by event inside whichever plan call
 * consumes the results (on that call's stream): a forward's first kernels do not wait for it.  Nothing for the caller to do,
 * except before capturing plan calls WITHOUT the pack into a hipGraph: glowhip_plan_pack_sync (HOST, blocks) waits for the side
 * part of the last pack so that the captured calls have nothing outside the graph to join. */
int glowhip_plan_pack_sync(glowhip_plan* plan);
/* The pack keeps its (plan-constant) job tables inside `packed` and sends them only once per buffer ADDRESS.  A caller that frees
 * `packed` and passes a new allocation -- which may come back at the same address -- says so with this call (HOST bookkeeping);
 * the next pack uploads the tables again. */
int glowhip_plan_forget_packed(glowhip_plan* plan);

/* FlowModel.encode: x (N, C0,H0,W0 of layer 0) -> z (output shape of the last layer),
 * logdet_out[n] = (logdet_in ? logdet_in[n] : 0) + sum of all layers' log-determinant terms.
 * noise (shape of x, may be NULL) is added to x first (dequantisation, network/model.py:421). */
int glowhip_plan_encode(glowhip_plan* plan, const void* packed, const float* x, const float* noise,
                        const float* logdet_in, float* z, float* logdet_out, int N,
                        void* workspace, size_t workspace_bytes, glowhip_stream_t stream);

/* FlowModel.decode: z -> x, layers run in reverse.  eps[k] (device pointer, shape of the k-th Split2d's
 * z2 in DECODE order, already multiplied by eps_std) is the injected N(0,1) draw of
 * GaussianDiag.sample (network/module.py:470-483).  logdet_out may be NULL. */
int glowhip_plan_decode(glowhip_plan* plan, const void* packed, const float* z, const float* const* eps,
                        int n_eps, const float* logdet_in, float* x, float* logdet_out, int N,
                        void* workspace, size_t workspace_bytes, glowhip_stream_t stream);

/* Full-latent encode: keep what every Split2d scores and drops (network/module.py:526-536 adds logp(z2 | prior(z1)) to the
 * log-determinant and returns z1 alone).  eps_out[k] (device buffer, shape of the k-th Split2d's z2 in DECODE order -- deepest
 * split first, the order glowhip_plan_decode reads, so an encode's output array is a decode's input array) receives
 * eps = (z2 - mean) * exp(-logs), written by the epilogue of the prior kernel that already holds mean, logs and z2: no extra
 * launch, no extra pass.  Per-call binding in the pattern of glowhip_plan_bind_head (pointers copied; HOST bookkeeping): honoured
 * at enqueue time by the next glowhip_plan_encode / glowhip_glow_forward / glowhip_glow_forward_u8 and every one after it until
 * (NULL, 0) unbinds; the training forward ignores it.  n_eps must equal the plan's Split2d count (GLOWHIP_EINVAL otherwise). */
int glowhip_plan_bind_latents(glowhip_plan* plan, float* const* eps_out, int n_eps);

/* ------------------------------------------------------------------------------------------------
 * Held-out evaluation (csrc/evaluate.hip): where the bits of Glow.normal_flow's objective (network/model.py:409-452) go, and the
 * bits per dimension of a data set.  No counterpart in the reference, which reports nll per training batch (network/trainer.py:123-133).
 * ---------------------------------------------------------------------------------------------- */
/* Per-level terms of the objective.  A LEVEL is a maximal run of layers that ends with a Split2d (network/module.py:511-536); the
 * last level ends with the top prior (network/model.py:440-445) or the head: glowhip_plan_level_count = Split2d count + 1 (HOST
 * bookkeeping, no device needed).  glowhip_plan_bind_level_terms is a per-call binding in the pattern of glowhip_plan_bind_latents
 * (pointers copied; HOST bookkeeping): honoured at enqueue time by glowhip_glow_forward / glowhip_glow_forward_u8 until
 * (NULL, NULL, 0) unbinds; the training forward, glowhip_plan_encode and glowhip_plan_decode ignore it.  While bound, the forward
 * enqueues one snapshot launch behind the launches of every Split2d and one behind the top prior's -- each copies the (2 + 7) N
 * words of the per-sample log-det accumulators into scratch (glowhip_plan_level_scratch_bytes(plan, N) bytes, the caller's;
 * glowhip_plan_workspace_bytes does not change) -- and, behind the launch that writes nll / objective, ONE launch that writes
 *     terms[l * N + n] = sum over the FlowSteps of level l of (3 sum(actnorm.logs) + log|det W|) H W      (network/module.py:76-82, 356-357)
 *                        + fix(snapshot_l - snapshot_{l-1})                                               in nats, one fp32 rounding
 * = level l's log-determinants (network/model.py:82-117) + the log-density its Split2d, or the top prior, scores.  The difference
 * is taken on the integer words (the whole-nats count of the flag word included), before any conversion: the parts add up to the
 * total exactly as integers, so  objective[n] = -ln(2^n_bits) C H W + sum_l terms[l][n]  up to the one rounding of each number.
 * A sample whose non-finite flags are set at the snapshot that closes level l has terms[l ..][n] = NaN: a part is never finite and
 * wrong.  z, nll and objective are bit for bit those of the unbound call; n_levels + 1 launches are added.  At most 16 levels and
 * 896 FlowSteps (GLOWHIP_EINVAL at bind time); scratch smaller than the batch needs: GLOWHIP_EWORKSPACE from the forward. */
int glowhip_plan_level_count(const glowhip_plan* plan);
size_t glowhip_plan_level_scratch_bytes(const glowhip_plan* plan, int N);
int glowhip_plan_bind_level_terms(glowhip_plan* plan, float* terms /* [n_levels][N] */, void* scratch, size_t scratch_bytes);

/* The fold: one launch per evaluated batch, plan-independent.  objective [K][N]: the objective_out rows of K forwards of the same N
 * images under K independent dequantisation draws (network/model.py:421; glowhip_plan_set_dequant_stream names them); terms
 * [K][n_levels][N] (may be NULL): their level terms; dims = C H W of an image.  Per image, in fp64 with a max-subtracted log-sum-exp:
 *     L          = logsumexp_k objective_k - ln K          (the importance-weighted bound log p(x) >= L; K = 1: today's nll)
 *     bpd        = fp32(-L / (ln2 dims))                   -> per_image[offset + n]; this rounded value is what the state sums
 *     bpd_single = -mean_k objective_k / (ln2 dims)        (>= bpd for every image, by Jensen)
 *     level_bits[l] = -mean_k terms[k][l] / (ln2 dims)     (n_bits + sum_l level_bits[l] = bpd_single: the levels decompose the
 *                                                           draw-averaged figure; the importance-weighted bound does not decompose)
 * FLAGGED: an image with a non-finite objective_k, or whose |bpd|, |bpd_single| or a |level_bits[l]| is not below 2048 bits/dim
 * (beyond the range the sums are guaranteed for).  It is counted in `flagged`, left out of count, every sum, min, max and the
 * histogram, and its per-image output is NaN.
 * only_if_nan (N floats of this batch, may be NULL; may alias per_image + offset): image n is folded only if only_if_nan[n] is NaN --
 * the re-run of what a first pass flagged: every image the call folds is taken OUT of `flagged` first, so each image stays counted
 * exactly once; the others are not touched, per_image included.
 * STATE, all integers: every sum is the 128-bit two's-complement sum {lo, hi} of rint(v 2^32) over the counted images, v = bpd,
 * bpd^2 (of the fp32 bpd, exact in fp64), bpd_single, level_bits[l]; min_key / max_key = min / max of rint(bpd 2^32) + 2^63 (reset:
 * all ones / 0); hist[i] counts  lo <= bpd < hi  with  i = min(floor((bpd - lo) * (bins / (hi - lo))), bins - 1)  evaluated in fp64 --
 * a value on an edge that this expression meets exactly belongs to the upper bin -- `under` bpd < lo, `over` bpd >= hi.  Integer
 * sums, counts, min and max: the state after a data set is the same bits for any split into batches and any order of the folds.
 * RANGE: |rint(v 2^32)| < 2^43 and rint(v^2 2^32) < 2^54 per image, a workgroup's 256 fit an int64, and the 128-bit sums hold more
 * images than `count` can number: the image count is bounded by the counter alone, count + flagged < 2^64.
 * glowhip_eval_reset zeroes the state and sets n_levels (<= 16), bins (<= 256; 0 = no histogram) and [lo, hi).  No allocation, no
 * host sync, capturable. */
#define GLOWHIP_EVAL_MAX_LEVELS 16
#define GLOWHIP_EVAL_MAX_BINS 256
typedef struct glowhip_eval_state {
    uint64_t count, flagged;
    uint64_t min_key, max_key;
    uint64_t sum_bpd[2], sum_bpd2[2], sum_single[2];
    uint64_t sum_level[GLOWHIP_EVAL_MAX_LEVELS][2];
    double lo, hi;
    int32_t bins, n_levels;
    uint64_t under, over;
    uint64_t hist[GLOWHIP_EVAL_MAX_BINS];
} glowhip_eval_state;
int glowhip_eval_reset(glowhip_eval_state* state /* DEVICE */, int n_levels, int bins, double lo, double hi, glowhip_stream_t stream);
int glowhip_eval_fold(glowhip_eval_state* state /* DEVICE */, const float* objective, const float* terms, int K, int N, int n_levels,
                      double dims, const float* only_if_nan, float* per_image, long offset, glowhip_stream_t stream);

/* Glow.normal_flow (network/model.py:409-452) in one call: z = x + noise; objective = -ln(2^n_bits)*CHW
 * + encode logdet + logp(z | prior_mean, prior_logs);  nll = -objective / (ln2*CHW).
 * prior_mean/prior_logs: (N,Cz,Hz,Wz) with batch stride prior_stride, NULL = zeros.
 * objective_out may be NULL. */
int glowhip_glow_forward(glowhip_plan* plan, const void* packed, const float* x, const float* noise,
                         const float* prior_mean, const float* prior_logs, long prior_stride, int n_bits,
                         float* z, float* nll_out, float* objective_out, int N,
                         void* workspace, size_t workspace_bytes, glowhip_stream_t stream);

/* The same from 8-bit pixels (N,C,H,W) as a data loader holds them: x = x_u8 / divisor (255 for torchvision's ToTensor,
 * dataset/celeba.py:74-86) + noise, converted inside the plan's leading Squeeze2d -- no fp32 copy of the batch is ever
 * made.  The plan must start with a Squeeze2d layer. */
int glowhip_glow_forward_u8(glowhip_plan* plan, const void* packed, const uint8_t* x_u8, float divisor, const float* noise,
                            const float* prior_mean, const float* prior_logs, long prior_stride, int n_bits, float* z,
                            float* nll_out, float* objective_out, int N, void* workspace, size_t workspace_bytes,
                            glowhip_stream_t stream);

/* Kernel family of a plan's coupling networks (network/module.py:300-319) -- a property of the PLAN, not of the process:
 *   GLOWHIP_FAMILY_AUTO        the split-half f16 matrix-pipe kernels wherever the shape allows (default; hidden activations
 *                              |v| < 4094, beyond that the result is non-finite and flagged, never a finite wrong value);
 *   GLOWHIP_FAMILY_EXACT_FP32  v_mfma_f32_32x32x2_f32 kernels only: the reference's full fp32 range at 1/3 of the speed.
 * Takes effect at the next glowhip_plan_pack_for (the family's weight images are packed on demand) + encode / decode /
 * glow_forward.  HOST bookkeeping; the caller serialises it with the plan's own calls as for any other plan call. */
#define GLOWHIP_FAMILY_AUTO 0
#define GLOWHIP_FAMILY_EXACT_FP32 1
int glowhip_plan_set_family(glowhip_plan* plan, int family);
int glowhip_plan_get_family(const glowhip_plan* plan);

/* Range / non-finite status of the encode / decode / glow_forward call that last ran with `workspace` for batch N (enqueue it
 * on the same stream right after that call): status_out[n] (DEVICE, N int32) = bit 0: a NaN term, bit 1: a +inf term, bit 2: a
 * -inf term entered sample n's log-det sum (the sticky flags the nll reports as NaN / inf) | bit 3: an element of
 * result[n*elems_per_sample ..) (the call's output tensor: x of a decode, z of an encode; may be NULL) is not finite.
 * Non-zero means: out of the product kernels' range (or genuinely diverged) -- re-run on GLOWHIP_FAMILY_EXACT_FP32 to get
 * the reference's answer (Glow.reverse_flow network/model.py:454-471 has no nll that would show it).  No host sync.
 * Range of the log-det sum itself: a sample receives P workgroup partial sums from the Gaussian kernels (Split2d priors, top prior)
 * and the terms of E affine-coupling elements; glowhip_plan_create refuses a layer list with 2^14 P + 104 E >= 2^31.  Under that
 * inequality, partials of |v| < 2^43 nats are summed exactly (2^-32 nats each) whatever the size of the sum, and the status bits
 * stay 0; a partial with |v| >= 2^43 sets bit 1 / bit 2 by its sign and the nll is +inf / -inf.  No input gives a finite nll that
 * is not the sum of its terms. */
int glowhip_plan_status(const glowhip_plan* plan, const void* workspace, size_t workspace_bytes, int N, const float* result,
                        long elems_per_sample, int32_t* status_out, glowhip_stream_t stream);

/* Dequantisation noise drawn INSIDE the leading squeeze (network/model.py:421): with enable != 0, every later
 * glowhip_glow_forward / _u8 call whose `noise` is NULL adds U(0, 2^-n_bits) from the counter-based generator
 * Philox4x32-10(key = seed; counter = element index, call number) -- no noise tensor, no RNG launch.  The call number starts at
 * 0 when the seed is (re)set and advances by one per such call; *next_call (HOST, may be NULL) receives its next value
 * (enable < 0: query only).  glowhip_dequant_noise writes the draw of a given call as a tensor (n elements in the order of x):
 * a forward with that tensor as `noise` is bitwise equal to the in-kernel draw. */
int glowhip_plan_set_dequant_rng(glowhip_plan* plan, unsigned long long seed, int enable, unsigned long long* next_call);
int glowhip_dequant_noise(float* out, long n, unsigned long long seed, unsigned long long call, int n_bits, glowhip_stream_t stream);
/* The same switch with the position given by the caller: the next glow_forward without a noise tensor draws with (seed, call),
 * the one after with call + 1 ...  Lets ONE stream serve every plan of a process (each batch shape has its own plan) and lets
 * the ranks of a data-parallel job key it differently (pytorch-glow_amd/network/model.py: torch's seed, the rank folded in). */
int glowhip_plan_set_dequant_stream(glowhip_plan* plan, unsigned long long seed, unsigned long long call);

/* The sampler's random stream: the N(0, 1) draws of GaussianDiag.sample (network/module.py:470-483) made inside the kernels that
 * consume them -- no noise tensor in HBM, and every draw has a name, (seed, call, stream, element).
 *   generator  Philox4x32-10, key = seed (the round function and key schedule of the dequantisation noise above); counter of the
 *              group of four elements 4j .. 4j+3 of stream s at call c:
 *                c0 = j & 0xffffffff, c1 = j >> 32, c2 = c & 0xffffffff, c3 = ((s + 1) << 24) | ((c >> 32) & 0xffffff)
 *   stream     s = 0: the top latent; s = 1 + k: the k-th Split2d in DECODE order (the order of glowhip_plan_decode's eps).  Plans
 *              with more than 254 Split2d layers are refused; call < 2^56.  The top byte of c3 is never zero, the dequantisation
 *              stream's always is: the two share no counter under one seed.  Streams 128 + leaf (128 .. 247) and 254 belong
 *              to the posterior chain ("Posterior sampling" below: the proposal's draws and the accept test's uniform, call =
 *              the chain's iteration); 248 names the Gaussian sensing matrix of compressed sensing
 *              ("a dense linear operator" below: call 0, element = flat index in the (M, C, H, W) matrix); 249 .. 253 are unassigned.
 *   element   flat index in the contiguous (N, C, H, W) draw tensor
 *   normals    words (w0, w1) give elements 0, 1 of the group, (w2, w3) elements 2, 3, by Box-Muller in fp32:
 *                u1 = ((w >> 9) + 0.5) * 2^-23, u2 = (w' >> 8) * 2^-24, r = sqrtf(-2 logf(u1)),
 *                even element = r cosf(2 pi u2), odd element = r sinf(2 pi u2);  |e| <= 5.77, never infinite
 *   value      e * std, one rounded fp32 product (csrc/sampler_rng.h: one device function behind every site)
 * glowhip_normal_noise writes n elements of a stream as a tensor: a decode with that tensor injected as eps[k] is bitwise equal
 * to the in-kernel draw of stream 1 + k. */
int glowhip_normal_noise(float* out, long n, unsigned long long seed, unsigned long long call, int stream_id, float std,
                         glowhip_stream_t stream);
/* Bind the stream to a plan, in the pattern of glowhip_plan_bind_latents (HOST bookkeeping; (NULL, NULL, 0, 0) unbinds).
 * rng_dev: DEVICE word of two uint64 {seed, call}, read by the kernels through the pointer -- the arguments of a captured graph
 * are frozen, the word is not.  std_split (HOST, n_split floats, copied): the std of every Split2d's draw in decode order; n_split
 * must be the plan's Split2d count.  While bound, glowhip_plan_decode accepts eps == NULL, n_eps < the Split2d count or
 * eps[k] == NULL, and the prior kernel of such a Split2d draws its eps itself -- all three Split2d routes, no extra launch; a
 * non-NULL eps[k] is injected as before.  Unbound, a missing eps is the error it always was.  advance != 0: a call that drew
 * ends with a one-thread launch doing call += 1 on the device word (no host upload between the replays of a graph). */
int glowhip_plan_bind_sampler(glowhip_plan* plan, void* rng_dev, const float* std_split, int n_split, int advance);
/* Glow.reverse_flow(z=None) (network/model.py:454-471) as one call: the top draw, the decode and the store.
 *   z_top    NULL: one launch computes the top prior -- zeros, or the head attached with glowhip_plan_set_head (learn_top and / or
 *            y_emb(y_onehot), y_onehot from glowhip_plan_bind_head), plus the optional dense base prior_mean / prior_logs
 *            (N,Cz,Hz,Wz, batch stride prior_stride) -- and writes z = mean + exp(logs) * draw, draw = stream 0 times std_top; no
 *            dense mean / logs exist in HBM.  Non-NULL: that latent is decoded as given.
 *   eps      as for glowhip_plan_decode with the sampler bound: NULL entries are drawn in the Split2d kernels.
 *   x, x_u8  outputs (one may be NULL): fp32 pixels, and / or 8-bit pixels u8 = (uint8) min(max(x * 255, 0), 255), truncating,
 *            NaN -> 0 -- the reference's tensor_to_ndarray (misc/util.py:405-407) on every pixel in [0, 1], saturating where its cast
 *            would wrap -- stored by the final un-squeeze itself; x_u8 needs a plan that starts with a Squeeze2d.
 *   z_out    NULL, or receives the top latent that was decoded.
 * A sampler must be bound unless z_top and every eps are given; with `advance` bound the call's last launch moves the device
 * position by one.  No allocation, no host sync: the call can be captured into a hipGraph. */
int glowhip_plan_sample(glowhip_plan* plan, const void* packed, const float* z_top, const float* prior_mean, const float* prior_logs,
                        long prior_stride, float std_top, const float* const* eps, int n_eps, float* x, uint8_t* x_u8, float* z_out,
                        int N, void* workspace, size_t workspace_bytes, glowhip_stream_t stream);

/* Data-dependent ActNorm initialisation pass over a whole plan (first training-mode forward,
 * network/trainer.py:112-115 + network/module.py:45-46,66-67): runs encode on x and writes every
 * ActNorm's bias/logs THROUGH the parameter pointers of the layer descs (which must be writable).  Ends with
 * glowhip_plan_pack_for(GLOWHIP_PACK_INFERENCE): pack _TRAINING / _INVERSE data before training / decoding. */
int glowhip_plan_actnorm_init(glowhip_plan* plan, void* packed, size_t packed_bytes, const float* x,
                              const float* noise, float actnorm_scale, int N, void* workspace,
                              size_t workspace_bytes, glowhip_stream_t stream);

/* Output shape of the plan for a given direction (HOST). out[3] = {C,H,W}. */
int glowhip_plan_output_shape(const glowhip_plan* plan, int reverse, int32_t out[3]);

/* ------------------------------------------------------------------------------------------------
 * Training step (reference network/trainer.py:123-140: forward, loss = mean(nll), backward)
 * ---------------------------------------------------------------------------------------------- */
/* Writable fp32 gradient tensors of one layer, same shapes as the parameters named in glowhip_layer_desc.
 * Entries of parameters a layer does not have (and any gradient the caller does not want) are NULL. */
typedef struct glowhip_layer_grads {
    float* an_bias; float* an_logs; float* invconv_w;
    float* f0_w; float* f0_an_bias; float* f0_an_logs;
    float* f2_w; float* f2_an_bias; float* f2_an_logs;
    float* f4_w; float* f4_bias; float* f4_logs;
} glowhip_layer_grads;

/* Bytes of the activation tape / of the training workspace for batch N. */
size_t glowhip_plan_tape_bytes(const glowhip_plan* plan, int N);
size_t glowhip_plan_train_workspace_bytes(const glowhip_plan* plan, int N);

/* glowhip_glow_forward that also records the tape (every layer output + the coupling networks' hidden
 * activations) needed by glowhip_glow_backward.  Same results as glowhip_glow_forward. */
int glowhip_glow_forward_train(glowhip_plan* plan, const void* packed, const float* x, const float* noise,
                               const float* prior_mean, const float* prior_logs, long prior_stride, int n_bits,
                               float* z, float* nll_out, float* objective_out, int N, void* tape, size_t tape_bytes,
                               void* workspace, size_t workspace_bytes, glowhip_stream_t stream);

/* Gradients of a scalar loss L given nll_grad[n] = dL/dnll_n (1/B for Glow.generative_loss = mean(nll),
 * network/model.py:496-506) and optionally z_grad = dL/dz (NULL = 0): every non-NULL entry of grads[layer] is
 * OVERWRITTEN with dL/dparameter; grad_x (shape of x, may be NULL) receives dL/dx.  `x`, `tape`, `packed` and the
 * prior arguments must be the ones of the matching glowhip_glow_forward_train call. */
int glowhip_glow_backward(glowhip_plan* plan, const void* packed, const float* x, const void* tape, size_t tape_bytes,
                          const float* nll_grad, const float* z_grad, const float* prior_mean,
                          const float* prior_logs, long prior_stride, const glowhip_layer_grads* grads,
                          float* grad_x, int N, void* workspace, size_t workspace_bytes, glowhip_stream_t stream);

/* Differentiable decode.  Vector-Jacobian product of glowhip_plan_decode at the latents whose decode is x (reference decode:
 * network/model.py:119-154 FlowStep.reverse_flow, 278-294 FlowModel.decode; network/module.py:470-483 Conv2dZeros, 511-536
 * Split2d): grad_z (shape of the plan's output) and grad_eps[k] (shape of the k-th Split2d's z2, DECODE order, as
 * glowhip_plan_decode reads eps; contiguous) receive J^T grad_x.  A NULL grad_z or grad_eps[k] skips that output; n_eps must be the
 * plan's Split2d count (GLOWHIP_EINVAL otherwise).  The call re-encodes x with the taping forward (no noise, no dequantisation
 * draw, no prior or head work) into `tape` -- scratch of glowhip_plan_tape_bytes(plan, N) bytes, overwritten -- and sweeps it; a
 * FlowStep's coupling network sees the same y1 in both directions, so that tape is the decode's to rounding.  packed must hold the
 * GLOWHIP_PACK_TRAINING and GLOWHIP_PACK_INVERSE data.  Each sample's grad_x is normalised by a power of two taken from its own
 * max-abs (on the device) and the factor undone on the outputs: the result is linear in grad_x to the bit over the whole fp32
 * range, and an all-zero grad_x[n] gives exact zeros.  PARAMETER gradients do not flow through the decode.  No allocation, no
 * host sync. */
size_t glowhip_plan_decode_vjp_workspace_bytes(const glowhip_plan* plan, int N);
int glowhip_plan_decode_vjp(glowhip_plan* plan, const void* packed, const float* x, const float* grad_x, float* grad_z,
                            float* const* grad_eps, int n_eps, int N, void* tape, size_t tape_bytes, void* workspace,
                            size_t workspace_bytes, glowhip_stream_t stream);

/* Gradient-ready marks: lets the caller overlap the gradient all-reduce of one process per GPU (the replacement of
 * nn.DataParallel's reduce-to-GPU-0, network/trainer.py:117-123) with the rest of the backward sweep.  The sweep runs from the
 * last layer to the first; glowhip_glow_backward records events[i] (hipEvent_t handles owned by the caller) on its stream as
 * soon as every kernel writing the convolution WEIGHT gradients (f0_w, f2_w, f4_w -- 99.8 % of the gradient bytes) of all layers
 * with index >= after_layer[i] has been enqueued.  after_layer must decrease.  The reduction-type gradients (biases, logs,
 * invconv matrices of ALL layers) are final only after the call's last kernel.  n = 0 clears the marks.  HOST bookkeeping. */
int glowhip_plan_backward_marks(glowhip_plan* plan, const int32_t* after_layer, void* const* events, int n);

/* ------------------------------------------------------------------------------------------------
 * Optimiser step (reference network/trainer.py:142-150: clip_grad_value_, clip_grad_norm_, optimizer.step() with the
 * torch.optim.Adam / Adamax of network/builder.py:10-13,108-113) over ALL parameters as two launches.
 * A chunk is at most 2^16 consecutive elements of one parameter with its gradient and optimiser state (m = exp_avg,
 * v = exp_avg_sq for Adam / exp_inf for Adamax).  partial_dev: n_chunks doubles of scratch.  kind: 0 = Adam (amsgrad off),
 * 1 = Adamax; step: 1-based count of this update (bias corrections); clip_value / max_norm <= 0: that clipping off.
 * grad_norm_out (1 float, may be NULL) <- total gradient norm after the value clipping, before the norm clipping, as
 * clip_grad_norm_ returns it.  Gradients are clipped IN PLACE as the reference's utilities do.
 * skip_if_nonfinite != 0: when that norm is NaN / inf the update launch leaves parameters, state and gradients untouched (the
 * device-side "found inf" of a loss scaler: no host sync) -- the caller reads grad_norm_out at its next natural sync and re-runs
 * the batch on GLOWHIP_FAMILY_EXACT_FP32 (training.TrainLoop).  0 = torch's semantics (NaN gradients give NaN parameters).
 * ---------------------------------------------------------------------------------------------- */
typedef struct glowhip_optim_chunk { float* param; float* grad; float* m; float* v; int32_t n; int32_t pad; } glowhip_optim_chunk;
int glowhip_optim_step(const glowhip_optim_chunk* chunks_dev, int n_chunks, int kind, float lr, double beta1, double beta2,
                       float eps, float weight_decay, int step, float clip_value, float max_norm, double* partial_dev,
                       float* grad_norm_out, int skip_if_nonfinite, glowhip_stream_t stream);
/* The same step with the values that change from step to step read from DEVICE memory -- hyper_dev[3] = {lr (a float's value),
 * 1 - beta1^step, 1 - beta2^step} as doubles, computed by the caller the way glowhip_optim_step does (python-double arithmetic, as
 * torch) -- so that the two launches can sit in a captured hipGraph whose kernel arguments are frozen (training.GraphedTrainStep:
 * the caller uploads the three values before each replay).  Same arithmetic, same bits as glowhip_optim_step. */
int glowhip_optim_step_dev(const glowhip_optim_chunk* chunks_dev, int n_chunks, int kind, const double* hyper_dev, double beta1,
                           double beta2, float eps, float weight_decay, float clip_value, float max_norm, double* partial_dev,
                           float* grad_norm_out, int skip_if_nonfinite, glowhip_stream_t stream);
/* The same two launches with a Polyak average (exponential moving average, EMA) of the weights updated by the update launch, at the
 * moment the new parameter value p' is in a register.  THE definition of the arithmetic, per element, all in fp32 with three
 * roundings (no fused multiply-add):
 *     e' = e + (p' - e) * w
 * w is the float the host passes -- the kernel knows no decay schedule (training._HipOptimizer.ema_weight: w = float(1 - decay_t)).
 * ema_dev: n_chunks device pointers parallel to the chunk table, ema_dev[i] = the average of chunk i's n elements (the chunk struct
 * keeps its 40-byte layout); a NULL entry = that chunk is not averaged.  The 16-byte path of a chunk needs its ema pointer 16-byte
 * aligned like the other four, else the chunk runs element by element (same bits).  Parameters, state, gradients and the norm come
 * out bit for bit as from glowhip_optim_step with the same arguments.  A step skipped by skip_if_nonfinite leaves e untouched too.
 * No allocation, no host sync, capturable; still two launches. */
int glowhip_optim_step_ema(const glowhip_optim_chunk* chunks_dev, float* const* ema_dev, int n_chunks, int kind, float lr, double beta1,
                           double beta2, float eps, float weight_decay, int step, float clip_value, float max_norm, float ema_w,
                           double* partial_dev, float* grad_norm_out, int skip_if_nonfinite, glowhip_stream_t stream);
/* The device form: hyper_dev[4] = {lr, 1 - beta1^step, 1 - beta2^step, w (a float's value)} as doubles.  Same bits as
 * glowhip_optim_step_ema. */
int glowhip_optim_step_ema_dev(const glowhip_optim_chunk* chunks_dev, float* const* ema_dev, int n_chunks, int kind, const double* hyper_dev,
                               double beta1, double beta2, float eps, float weight_decay, float clip_value, float max_norm,
                               double* partial_dev, float* grad_norm_out, int skip_if_nonfinite, glowhip_stream_t stream);
/* param[i] <-> ema_dev[i] for every chunk, ONE launch (16-byte accesses where both addresses allow; NULL entries are left alone):
 * evaluate or sample under the averaged weights without moving an address -- plans, packed buffers and captured graphs stay valid
 * (the caller bumps the parameters' version counters so that the plans re-derive their weight images).  Calling it twice restores
 * both sides to the bit.  The gradient / m / v fields of the table are not read.  No allocation, no host sync, capturable. */
int glowhip_optim_ema_swap(const glowhip_optim_chunk* chunks_dev, float* const* ema_dev, int n_chunks, glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient accumulation: the training step (reference network/trainer.py:123-150: forward, loss.backward(), clippings,
 * optimizer.step()) as k micro-batches whose gradients are combined before the ONE update.  No counterpart in the reference, which
 * trains at the batch its memory allows.  A segment is one flat gradient buffer with its accumulator of the same length
 * (FlowPlan's persistent buckets).  THE definition of the arithmetic, per element, fp32 with one rounding per operation (no fused
 * multiply-add):
 *     GLOWHIP_ACC_FIRST :  acc  = grad                    (no memset ever precedes a round of accumulation; grad is not written)
 *     GLOWHIP_ACC_ADD   :  acc  = acc + grad              (grad is not written)
 *     GLOWHIP_ACC_FINISH:  grad = (acc + grad) * scale    (acc is not written)
 * scale is ignored by FIRST and ADD.  NaN and inf propagate by the IEEE rules, nothing is filtered: what a non-finite accumulated
 * norm means is decided by skip_if_nonfinite of the update launch that follows.
 * segs is a HOST array, copied into the kernel arguments: ONE launch for all segments, no device table, no upload, no allocation,
 * no host sync; capturable when the addresses are persistent.  n_segs <= 16; a segment with n == 0 is legal and skipped;
 * n_segs == 0 (or nothing but empty segments) returns GLOWHIP_OK without a launch.  16-byte accesses where a segment's grad and acc
 * are both 16-byte aligned or reach a 16-byte boundary after the same 1-3 elements (peeled one by one), element by element where
 * they share no such phase; the n % 4 tail one by one.  Element-wise, so every path gives the same bits.  No atomics, no LDS, no
 * dependence on workgroup order.
 * GLOWHIP_EINVAL with a message and no device call: n_segs < 0 or > 16, n < 0, a NULL (or not 4-byte aligned) grad or acc with
 * n > 0, a mode outside the enum, a non-finite scale with FINISH, a segment of more than 2^36 elements.
 * ---------------------------------------------------------------------------------------------- */
typedef struct glowhip_grad_seg { float* grad; float* acc; int64_t n; } glowhip_grad_seg;
enum { GLOWHIP_ACC_FIRST = 0, GLOWHIP_ACC_ADD = 1, GLOWHIP_ACC_FINISH = 2 };
int glowhip_grad_accumulate(const glowhip_grad_seg* segs /* HOST, copied */, int n_segs, int mode, float scale,
                            glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Restoration objective: the data term of an inverse problem under the flow prior (in-painting, denoising, super-resolution).
 * x, grad_x: (N,C,H,W) contiguous; target, weight: (N,C,H/pool,W/pool); inv_wsum: (N).  P = the pool x pool average pool
 * (pool = 1: the identity); weight == NULL means all ones, inv_wsum == NULL means 1 / (C (H/pool) (W/pool)).  Per sample n:
 *     loss_out[n] = inv_wsum[n] * sum w (P x - t)^2                 (overwritten, never accumulated into; loss_out may be NULL)
 *     grad_x      = 2 inv_wsum[n] * P^T (w (P x - t))               (every x under one measurement cell: the cell's value / pool^2)
 * ONE launch, one workgroup per sample; x is read once and feeds both outputs.  pool == 1 moves 16 bytes per access where
 * C H W % 4 == 0 and every address allows, element by element otherwise.  The loss is summed in fp64 in a fixed order inside the
 * sample's workgroup: bitwise the same run to run, no atomics, no scratch buffer.  inv_wsum[n] == 0: exact zeros in grad_x[n] and
 * loss 0, whatever x[n] holds.  A non-finite x[n] makes that sample's loss and gradient non-finite and no other's.  pool < 1,
 * H % pool != 0, W % pool != 0 or a NULL x / target / grad_x: GLOWHIP_EINVAL with a message, no device call.  No allocation, no
 * host sync, capturable.  grad_x is what glowhip_plan_decode_vjp takes: the two make the latent gradient of the objective. */
int glowhip_restore_objective(const float* x, const float* target, const float* weight, const float* inv_wsum,
                              int N, int C, int H, int W, int pool, float* grad_x, float* loss_out, glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The restoration objective observed through a point-spread function (PSF): deblurring, and super-resolution as blur then decimate.
 * THE definition of the operator.  Per sample n and channel c, with k the sample's PSF of kh x kw taps (kh, kw odd, 1 .. 15),
 * ah = (kh - 1) / 2, aw = (kw - 1) / 2:
 *     (B x)[c,i,j] = sum_{a,b} k[a,b] * x[c, i + ah - a, j + aw - b]         (x = 0 outside the image)
 *     A = P B                                                                (P: the pool x pool average pool, as above)
 *     loss_out[n] = inv_wsum[n] * sum w (A x - t)^2
 *     grad_x      = 2 inv_wsum[n] * B^T P^T (w (A x - t))
 *     resid       = w (A x - t)                                              (N,C,H/pool,W/pool): scratch AND output
 * B is a true convolution: k is the image a point source leaves (a single 1 at (i0, j0) blurs to k centred there); it is
 * F.conv2d with the flipped kernel, depthwise.  The same PSF serves every channel of a sample; psf_stride == 0 means one PSF
 * (kh*kw floats, row-major) for the whole batch, otherwise sample n's starts at psf + n * psf_stride (>= kh*kw).  The call does not
 * normalise the PSF.  Zero padding is the only border rule: a caller who wants the border treated honestly gives weight 0 to the
 * measurement cells whose footprint leaves the image.  x, target, weight, inv_wsum, grad_x, loss_out and the NULL defaults are as
 * for glowhip_restore_objective, which this call leaves untouched.
 * ONE launch, one workgroup per sample, three phases separated by workgroup barriers: B x into grad_x[n] (as scratch) from x tiles
 * staged with their halo in LDS; glowhip_restore_objective's own loops over it (resid and the fp64 loss, in the same fixed order:
 * bitwise the same run to run, no atomics); B^T P^T from resid tiles staged the same way.  The two gathers are one routine, with the
 * taps flipped and as given: exact transposes of each other as linear maps.  With pool == 1 and a 1x1 PSF holding 1.0f, loss_out
 * and grad_x are bit-identical to glowhip_restore_objective's on the same inputs (placed so that both take the same access path).
 * inv_wsum[n] == 0: exact zeros in grad_x[n] and resid[n] and loss 0, whatever x[n] holds.  A non-finite x[n] reaches no other
 * sample's outputs.  x, grad_x and resid must not overlap.  No allocation, no host sync, capturable.
 * GLOWHIP_EINVAL with a message and no device call: a NULL x, target, grad_x, psf or resid; kh or kw even, < 1 or > 15; psf_stride
 * neither 0 nor >= kh*kw; pool < 1; H or W not divisible by pool; C*H*W >= 2^31.  N == 0 returns GLOWHIP_OK. */
int glowhip_restore_objective_psf(const float* x, const float* target, const float* weight, const float* inv_wsum,
                                  const float* psf, long psf_stride /* 0: one PSF for the batch; else >= kh*kw */, int kh, int kw,
                                  int N, int C, int H, int W, int pool,
                                  float* resid /* scratch AND output: (N,C,H/pool,W/pool) = w (A x - t) */,
                                  float* grad_x, float* loss_out, glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The restoration objective observed through a dense linear operator: compressed sensing, t = A x + noise with M well below D.
 * THE definition.  Per sample n, with x[n] flattened to D = C*H*W values in (C,H,W) order and A an (M, D) row-major fp32 matrix
 * shared by the batch:
 *     y[n,m]      = sum_d A[m,d] * x[n,d]
 *     resid[n,m]  = w[n,m] * (y[n,m] - t[n,m])                      (N,M): scratch AND output
 *     loss_out[n] = inv_wsum[n] * sum_m w[n,m] * (y[n,m] - t[n,m])^2
 *     grad_x[n,d] = sum_m A[m,d] * u[n,m],    u = 2 * inv_wsum[n] * resid      (the scaling applied to the residual BEFORE A^T, as
 *                                                                               phase 2 of the PSF kernel does)
 * x, grad_x: (N, D) contiguous; target, weight, resid: (N, M); inv_wsum: (N).  weight == NULL means all ones, inv_wsum == NULL means
 * 1 / M; loss_out may be NULL (overwritten, never accumulated into).  The call does not normalise A.  x, grad_x, resid, A and the
 * scratch must not overlap.
 * Plain fp32 FMA on the vector pipe; both products are paced by reading A, which each reads from HBM once for any N up to 64.  The
 * launches (csrc/restore_linear.hip): the forward product over row blocks x D slices of 4 096 columns, a workgroup's A tile held in
 * registers while it loops over the batch in sample tiles of 4, a slice's partial y into the scratch; one workgroup per sample that
 * sums the partials in slice order and runs glowhip_restore_objective's own loops over y (the same 16-byte or element path by the
 * same address rule, the fp64 loss per thread in element order, then wave, then workgroup), writing resid and u; the adjoint product
 * over column blocks x M slices of 128 rows, one accumulator per sample in each lane; and, where M has more than one slice, the sum
 * of the slices' partials in slice order.  No atomics, nothing depends on workgroup order: bitwise the same run to run.  Every slice
 * count and tile shape is a function of (M, D) only, never of N, and no arithmetic of a sample reads another sample's values: sample
 * n's outputs have the same bits in a batch of 1 and in a batch of 64 (buffers placed alike), and a non-finite x[n] reaches no other
 * sample's outputs.  inv_wsum[n] == 0: exact zeros in grad_x[n] and resid[n] and loss 0, whatever x[n] holds.  With A the D x D
 * identity, loss_out and grad_x are bit-identical to glowhip_restore_objective's at pool 1 on the same inputs (placed so that both
 * take the same access path): products with +-0 and one-term sums round nothing.  The one thing a sum cannot carry is the sign
 * of an exact zero: where w == 0 and x < t that call returns -0, and here the -0 meets the +0 products of the identity's other
 * rows (-0 + +0 = +0).  glowhip_restore_objective and glowhip_restore_objective_psf are untouched.
 * scratch: glowhip_restore_linear_scratch_bytes(N, M, D) bytes at a 16-byte aligned address (the D slices' partial y, u, the M
 * slices' partial gradients); the size is monotone in each argument, and 0 only on error (see glowhip_last_error).  No allocation,
 * no host sync, capturable; offsets into A are 64-bit.
 * GLOWHIP_EINVAL with a message and no device call: a NULL x, target, A, resid or grad_x; M < 1, D < 1, D >= 2^31 or M*D >= 2^40
 * (or a shape of more than 2^31 workgroups or 2^46 scratch bytes, which no such matrix in memory reaches); N < 0; a scratch that is
 * NULL, misaligned or too small.  N == 0 returns GLOWHIP_OK. */
size_t glowhip_restore_linear_scratch_bytes(int N, long M, long D);          /* 0: see last_error */
int    glowhip_restore_objective_linear(const float* x, const float* target, const float* weight, const float* inv_wsum,
                                        const float* A, long M, int N, long D,
                                        float* resid, float* grad_x, float* loss_out,
                                        void* scratch, size_t scratch_bytes, glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The restoration objective observed in the Fourier domain: MRI k-space undersampling, radio interferometry, partial-Fourier
 * compressed sensing -- a structured operator of O(D log D) work whose only stored part is a mask (csrc/restore_fourier.hip; fp64
 * restatement tests/fourier_oracle.py).  THE definition.  Per sample n and channel c, F is the unitary 2-D DFT of the H x W plane,
 *     (F x)[u,v] = 1/sqrt(H W) * sum_{i,j} x[i,j] * exp(-2 pi i (u i / H + v j / W))
 * which is torch.fft.fft2(norm="ortho"): unshifted, index (0,0) the DC term.
 *     X[n,c]      = F x[n,c]                                  complex, (H,W)
 *     resid       = w (X - t)                                 (N,C,H,W,2) interleaved re/im: scratch AND output
 *     loss_out[n] = inv_wsum[n] * sum_{c,k} w |X - t|^2       fp64, fixed order, no atomics
 *     grad_x      = 2 inv_wsum[n] * Re( F^H resid )           real (N,C,H,W)
 * x, grad_x: (N,C,H,W) contiguous; target: (N,C,H,W,2) fp32, the memory of torch.view_as_real on a complex64 tensor; weight: real,
 * (N,C,H,W), NULL means all ones; inv_wsum: (N), NULL means 1 / (C H W); loss_out may be NULL (overwritten, never accumulated into).
 * H and W are each a power of two from 2 to 256 (256 is the largest side among the project's configs); H != W is allowed.
 * THREE launches, whatever the shape -- a separable radix-2 FFT in LDS, fp32, one rounding per operation: the forward rows on tiles
 * of rows into resid (the intermediate between the passes); the columns on tiles of 32 columns (16 at H = 256; a whole plane does
 * not fit LDS), where ONE LDS tile sees the forward columns, the scaling, the subtraction, the weighting, the loss partial and the
 * adjoint columns, so the spectrum makes no round trip through HBM; the adjoint rows from the scratch into grad_x, the workgroup of
 * a sample's first tile also folding the loss.  Twiddles: evaluated in fp64 and rounded once to fp32, a table built per launch in
 * LDS.  The column tiles are laid out, and the row tiles XOR-swizzled, against LDS bank conflicts on the strided butterfly stages.
 * Guarantees.  Tile shapes and the butterfly order are functions of (H, W) only, never of N, and a workgroup works on one plane of
 * one sample: sample n's outputs have the same bits in a batch of 1 and in a batch of 64 (whatever the buffers' alignment: every
 * access path is element-wise).  The loss is folded in fp64 in a fixed order -- thread, wave, workgroup, then the partials in index
 * order; no atomics, nothing depends on workgroup order: bitwise reproducible run to run.  inv_wsum[n] == 0: exact zeros in grad_x[n]
 * and resid[n] and loss 0, whatever x[n] holds.  A non-finite x[n] reaches no other sample's outputs.  No allocation, no host sync,
 * capturable.  glowhip_restore_objective, _psf and _linear are untouched.
 * scratch: glowhip_restore_fourier_scratch_bytes(N, C, H, W) bytes at a 16-byte aligned address (the complex intermediate of the
 * adjoint and the loss partials); monotone in N and C, and 0 only on error (see glowhip_last_error).
 * GLOWHIP_EINVAL with a message and no device call: a NULL x, target, resid or grad_x; N < 0 or C < 1; H or W not a power of two
 * from 2 to 256 (or a batch of more than 2^31 workgroups); a scratch that is NULL, misaligned or too small; x, grad_x and resid
 * overlapping.  N == 0 returns GLOWHIP_OK.
 *
 * glowhip_fourier2d is the transform alone, by the same kernels (two launches): adjoint == 0 maps real `in` (planes,H,W) to complex
 * `out` (planes,H,W,2) = F in; adjoint == 1 maps complex `in` (planes,H,W,2) to real `out` (planes,H,W) = Re(F^H in).  It makes
 * measurements and the zero-filled reconstruction without an FFT library.  The adjoint's complex intermediate is taken from and
 * returned to the stream's memory pool in stream order (no host sync, but not for a captured region; the objective call is).
 * GLOWHIP_EINVAL: a NULL pointer, planes < 0, a side that is not a power of two from 2 to 256, adjoint outside {0, 1}, in and out
 * overlapping.  planes == 0 returns GLOWHIP_OK. */
size_t glowhip_restore_fourier_scratch_bytes(int N, int C, int H, int W);      /* 0: see last_error */
int    glowhip_restore_objective_fourier(const float* x, const float* target /* (N,C,H,W,2) */, const float* weight,
                                         const float* inv_wsum, int N, int C, int H, int W,
                                         float* resid /* scratch AND output: (N,C,H,W,2) = w (F x - t) */,
                                         float* grad_x, float* loss_out,
                                         void* scratch, size_t scratch_bytes, glowhip_stream_t stream);
int    glowhip_fourier2d(const float* in, float* out, long planes, int H, int W, int adjoint, glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-coil k-space (parallel imaging, SENSE): the Fourier objective above with Q receive coils, each seeing the image through its
 * own complex sensitivity map (csrc/restore_fourier.hip; fp64 restatement tests/coil_oracle.py).  THE definition.  Per sample n and
 * image channel c: Q coils with complex sensitivity maps S[q] (H x W), 1 <= Q <= 32; F is the unitary 2-D DFT defined above
 * (torch.fft.fft2(norm="ortho"), unshifted).
 *     Y[n,c,q]    = F ( S[q] * x[n,c] )                          complex (H,W); * is the element-wise product
 *     resid       = w[n,c] * (Y[n,c,q] - t[n,c,q])               (N,C,Q,H,W,2) interleaved re/im: scratch AND output
 *     loss_out[n] = inv_wsum[n] * sum_{c,q,k} w |Y - t|^2        fp64, fixed order, no atomics
 *     grad_x[n,c] = 2 inv_wsum[n] * sum_q Re( conj(S[q]) * F^H resid[n,c,q] )     real (N,C,H,W), the sum in coil order q = 0..Q-1
 * x, grad_x: (N,C,H,W) fp32 contiguous; target: (N,C,Q,H,W,2) fp32, the memory of torch.view_as_real on a complex64 tensor; maps:
 * (Q,H,W,2) fp32, shared by the batch when maps_stride == 0, or per sample, (N,Q,H,W,2), when maps_stride == Q*H*W*2 (counted in
 * floats; any other stride is GLOWHIP_EINVAL); the same for every channel; NOT normalised by the kernel.  weight: real (N,C,H,W),
 * shared by the coils -- the sampling mask; per-coil noise whitening is the caller's job -- NULL means all ones.  inv_wsum: (N), NULL
 * means 1 / (C Q H W).  loss_out may be NULL.  H and W: each a power of two from 2 to 256, as above.
 * THREE launches, whatever the shape.  (1) Forward rows on (N C Q planes) x row tiles: the tile is loaded as (S.re x, S.im x) -- two
 * products, one rounding each -- then the stages of the plain call, into resid.  (2) The column kernel of the plain call on N C Q
 * planes, with the sample of a plane plane / (C Q) and the weight cell that of plane / Q: forward columns, scaling, subtraction,
 * weighting, loss partial and adjoint columns on ONE LDS tile.  (3) Adjoint rows with the coil sum on (N C planes) x row tiles: a
 * workgroup walks q = 0..Q-1 over the same row tile of the Q coil planes in the scratch and every thread adds S.re G.re + S.im G.im
 * (one rounding per operation) for the elements it owns -- a fixed element <-> thread map -- into fp32 registers, in coil order; it
 * stores once, times 1/sqrt(H W).  The first tile's workgroup of a sample folds the C Q col_tiles loss partials in index order in
 * fp64.  No atomics, no fourth launch, nothing depends on workgroup order.
 * Guarantees.  Tile shapes and the butterfly order are functions of (H, W) only, never of N or Q: sample n's outputs have the same
 * bits in a batch of 1 and in a batch of 64.  Shared maps and the same maps repeated per sample give the same bits.  Bitwise
 * reproducible run to run.  inv_wsum[n] == 0: exact zeros in grad_x[n] and resid[n] and loss 0; the spectrum is not read.  A
 * non-finite x[n] reaches no other sample's outputs.  No allocation, no host sync, capturable.  With Q == 1 and S == 1 + 0i the
 * loss, grad_x and resid are VALUE-equal to glowhip_restore_objective_fourier's (torch.equal holds): the only bit that can differ is
 * the sign of a zero -- 0 * x is -0 for x < 0, and +-0 never changes a non-zero sum -- so this is not a claim of bit identity.
 * glowhip_restore_objective_fourier, glowhip_fourier2d and the other objective entry points keep the bits they had.
 * scratch: glowhip_restore_coils_scratch_bytes(N, C, Q, H, W) bytes at a 16-byte aligned address (the complex intermediate of the
 * adjoint, N C Q planes, and the loss partials); monotone in N, C and Q, and 0 only on error (see glowhip_last_error).
 * GLOWHIP_EINVAL with a message and no device call: a NULL x, target, maps, resid or grad_x; N < 0 or C < 1; Q outside 1..32; a
 * maps_stride other than 0 and Q*H*W*2; H or W not a power of two from 2 to 256; a grid of more than 2^31 workgroups; a scratch
 * that is NULL, misaligned or too small; x, grad_x, resid or maps overlapping.  N == 0 returns GLOWHIP_OK.
 *
 * glowhip_coils2d is the operator alone (two launches): adjoint == 0 maps real `in` (N,C,H,W) to complex `out` (N,C,Q,H,W,2) =
 * F (S in); adjoint == 1 maps complex `in` (N,C,Q,H,W,2) to real `out` (N,C,H,W) = sum_q Re( conj(S[q]) F^H in[q] ).  It makes
 * measurements and the coil-combined zero-filled start without an FFT library.  Like glowhip_fourier2d's adjoint, the adjoint takes
 * its complex intermediate from the stream's memory pool: not for a captured region.  GLOWHIP_EINVAL as above, and for adjoint
 * outside {0, 1} and in, maps or out overlapping. */
size_t glowhip_restore_coils_scratch_bytes(int N, int C, int Q, int H, int W);      /* 0: see last_error */
int    glowhip_restore_objective_coils(const float* x, const float* target /* (N,C,Q,H,W,2) */, const float* weight,
                                       const float* inv_wsum, const float* maps /* (Q,H,W,2) or (N,Q,H,W,2) */, long maps_stride,
                                       int N, int C, int Q, int H, int W,
                                       float* resid /* scratch AND output: (N,C,Q,H,W,2) = w (F (S x) - t) */,
                                       float* grad_x, float* loss_out,
                                       void* scratch, size_t scratch_bytes, glowhip_stream_t stream);
int    glowhip_coils2d(const float* in, const float* maps, long maps_stride, float* out, int N, int C, int Q, int H, int W,
                       int adjoint, glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Blind deblurring: the PSF as an unknown of the fit -- the gradient of the data term of glowhip_restore_objective_psf with
 * respect to the taps of the PSF, and the softmax that keeps an estimate on the simplex (csrc/restore_blind.hip; fp64 restatement
 * tests/blind_oracle.py).  THE definition.  Notation as for glowhip_restore_objective_psf; per sample n, k the kh x kw PSF,
 * ah = (kh - 1) / 2, aw = (kw - 1) / 2, v = resid = w (A x - t) at measurement resolution, inv = inv_wsum[n] (NULL: that call's
 * default 1 / (C (H/pool) (W/pool))):
 *     u[c,i,j]   = (2 inv * v[c, i/pool, j/pool]) * (1/pool^2)          formed with exactly the two roundings phase 2 of the PSF kernel uses
 *     g_k[n,a,b] = sum_{c,i,j} u[c,i,j] * x[c, i + ah - a, j + aw - b]     (x = 0 outside the image)   = d loss[n] / d k[a,b]
 * For a PSF shared by the batch (psf_stride == 0), g_k = sum_n g_k[n], in sample order.  With k = softmax(theta) over the kh*kw taps
 * of one PSF,
 *     g_theta[q] = k[q] * (g_k[q] - sum_r k[r] g_k[r])
 * The softmax gives taps >= 0 that sum to 1: it fixes the scale ambiguity between PSF and image without a projection step.  A
 * translation ambiguity remains (a shifted PSF and the oppositely shifted image explain the same measurement): the centre of the
 * start PSF and the valid-band weights select the solution.
 *
 * glowhip_psf_from_logits: psf[p] = softmax(logits[p]) for n_psf PSFs of kh*kw taps, both dense.  The max is subtracted, the
 * exponentials and their sum are taken in fp64 in tap order, one rounding to fp32 per tap.  One launch, one workgroup per PSF.
 * GLOWHIP_EINVAL: a NULL pointer, kh or kw even, < 1 or > 15, n_psf < 0.  n_psf == 0 returns GLOWHIP_OK.
 *
 * glowhip_restore_psf_grad runs after glowhip_restore_objective_psf on the same x, resid and inv_wsum.  grad_psf and grad_logits
 * are dense (n_psf, kh*kw) with n_psf = psf_stride ? N : 1; either may be NULL, not both; psf (with psf_stride as in that call) is
 * read only for grad_logits.  Overwritten, never accumulated into.  x, resid, the outputs and the scratch must not overlap.
 * Two launches: the partial launch over samples x (channel, 8-row band, 64-column tile) -- u and the x tile with its zero halo
 * staged in LDS, a thread owns a tap and a slice of the tile's columns, fp32 fmaf chains of at most 64 terms, everything above a
 * chain folded in fp64 in a fixed order, kh*kw doubles per workgroup into the scratch -- and the finishing launch, one workgroup per
 * PSF, which folds the partials in (sample,) channel, band, tile order in fp64, writes grad_psf with one rounding, applies the
 * softmax backward in fp64 and writes grad_logits with one rounding.
 * Guarantees.  inv_wsum[n] == 0: sample n contributes exact zeros, whatever x[n] holds.  A non-finite x[n] reaches no other sample's
 * per-sample output; with a shared PSF it reaches the shared gradient and nothing else.  No atomics, nothing depends on workgroup
 * order: the same bits run to run.  Every tile, band, slice and group count is a function of (C, H, W, kh, kw, pool) only, never of
 * N: with per-sample PSFs sample n's gradient has the same bits in a batch of 1 and in a batch of 5 (buffers placed alike).
 * scratch: glowhip_restore_psf_grad_scratch_bytes(N, C, H, W, kh, kw, pool) bytes at a 16-byte aligned address; the size is monotone
 * in each argument, and 0 only on error (see glowhip_last_error).  No allocation, no host sync, capturable.
 * GLOWHIP_EINVAL with a message and no device call: a NULL x or resid, grad_psf and grad_logits both NULL, grad_logits without psf;
 * kh or kw even, < 1 or > 15; psf_stride neither 0 nor >= kh*kw; N < 0, C, H or W < 1; pool < 1 or not dividing H and W;
 * C*H*W >= 2^31 (or a shape of more than 2^31 workgroups or 2^46 scratch bytes); a scratch that is NULL, misaligned or too small.
 * N == 0 returns GLOWHIP_OK. */
int    glowhip_psf_from_logits(const float* logits, float* psf, int n_psf, int kh, int kw, glowhip_stream_t stream);
size_t glowhip_restore_psf_grad_scratch_bytes(int N, int C, int H, int W, int kh, int kw, int pool);      /* 0: see last_error */
int    glowhip_restore_psf_grad(const float* x, const float* resid, const float* inv_wsum,
                                const float* psf, long psf_stride /* 0: one PSF for the batch; else >= kh*kw */, int kh, int kw,
                                int N, int C, int H, int W, int pool,
                                float* grad_psf /* (n_psf, kh*kw) or NULL */, float* grad_logits /* (n_psf, kh*kw) or NULL */,
                                void* scratch, size_t scratch_bytes, glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Posterior sampling: a Metropolis-adjusted Langevin (MALA) chain over the latents of an inverse problem, one independent chain
 * per sample, and the Welford moments of its images (csrc/posterior.hip; numpy restatement tests/posterior_oracle.py).
 * THE definition.  Per sample n, theta = all latent leaves of that sample (leaf 0 = z, leaf 1 + k = eps[k] in decode order):
 *     U(theta) = L(theta) + 1/2 ||theta||^2,   L = sum w (P decode(theta) - t)^2 / (2 sigma^2)
 *              = glowhip_restore_objective with inv_wsum[n] = 1 / (2 sigma^2);   grad U = g + theta,  g = decode_vjp(grad_x)
 *   proposal   with the per-sample step h (fp32, one rounding per operation, no fused multiply-add):
 *                d = g + theta;   theta' = (theta - h d) + sqrtf(2 h) xi
 *              xi = the sampler's N(0, 1) draw (above) at (seed, call = iteration, stream = 128 + leaf, element = flat index in
 *              the contiguous (N, ...) leaf);   a = sum xi^2
 *   at theta'  L', g' by decode, objective, decode_vjp;   d' = g' + theta';   b = sum (theta - theta' + h d')^2;
 *              p = sum theta^2;   p' = sum theta'^2       (a, b, p, p': fp64 sums of fp64 terms of the fp32 elements, fixed order)
 *   test       log alpha = (L - L') + 1/2 (p - p') + 1/2 a - b / (4 h), in fp64.  Accept iff L', b and p' are finite and
 *              log(u) < log alpha, u = ((w0 >> 8) + 0.5) 2^-24, w0 = word 0 of group n of stream 254 at the same (seed, call).
 *   accept     theta <- theta', g <- g', L <- L', image <- proposal image: element copies, the bits are preserved.  A rejected
 *              sample's state is not written.  A rejection because L', b or p' is not finite bumps the sample's counter: a
 *              proposal outside the fp16 pairs' range is refused on the device, never accepted as a wrong value.
 *   adaptation only while iteration < burn_in:  h <- clamp(h exp(gamma (min(1, e^{log alpha}) - 0.574)), step_min, step_max),
 *              gamma = adapt_rate / sqrt(iteration + 1), a non-finite proposal counting as probability 0; frozen from burn_in on.
 *   streams    128 + leaf (at most 120 leaves: 128 .. 247) and 254 are disjoint from the sampler's 0 .. n_split of any plan with
 *              fewer than 127 Split2d layers, which is every plan whose leaves these entries accept.
 *   moments    per chain and pixel, of the CURRENT image: fold number c = (t - burn_in) / thin + 1 at every iteration t >= burn_in
 *              with (t - burn_in) % thin == 0:  delta = x - mean;  mean += delta / c;  M2 += delta (x - mean)   (c == 1 starts
 *              them: mean = x, M2 = 0, whatever the buffers held).  The count is not stored: it is a function of t.
 * Segments: a HOST array copied into the kernel arguments, in the style of glowhip_grad_seg.  A segment is one pair {current,
 * proposal} of contiguous (N, per) tensors.  Segments 0 .. n_leaves - 1 are the leaves, n_leaves .. 2 n_leaves - 1 their gradients
 * in the same order, the rest (the image) is only copied on acceptance.  n_segs <= 32; any 4-byte alignment; any per.
 * Launches: glowhip_mala_propose (theta', a), glowhip_mala_energy (b, p, p'), glowhip_mala_select (the decision, re-derived by every
 * workgroup of a sample from the same partial sums in the same order; the copies; then, by the workgroup that arrives last at
 * `ticket` -- an integer counter the call zeroes itself with a memset in front of the launch -- L, h, counts (2,N: accepted, non-finite), row
 * `iteration` of hist (3,steps,N: energy U after the decision, accept flag, log alpha; iteration >= steps writes no row), call += 1
 * on pos {seed, call} and *iteration += 1).  scratch: glowhip_mala_scratch_bytes, shared by the three.  glowhip_mala_init fills
 * step[n] = step_size and inv_wsum[n] = 1 / (2 noise_std^2) (inv_wsum may be NULL).  glowhip_posterior_moments folds n elements at
 * t = *iteration + iter_offset (-1 behind a select).  No floating-point atomics, no dependence on workgroup order, bitwise the same
 * run to run; no allocation, no host sync, capturable: nothing per iteration comes from the host.
 * GLOWHIP_EINVAL with a message and no device call: n_leaves < 1 or > 120, n_segs outside 2 n_leaves .. 32, N < 1, a NULL or
 * misaligned pointer of a segment with per > 0 or of any other argument, a gradient segment whose per differs from its leaf's, a
 * scratch that is too small, a step size, noise_std or clamp that is not finite or <= 0, thin < 1, burn_in < 0, steps < 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct glowhip_mala_seg { float* cur; float* prop; int64_t per; } glowhip_mala_seg;
size_t glowhip_mala_scratch_bytes(const glowhip_mala_seg* segs /* HOST */, int n_segs, int n_leaves, int N);   /* 0: see last_error */
int glowhip_mala_init(float* step, float* inv_wsum, int N, float step_size, float noise_std, glowhip_stream_t stream);
int glowhip_mala_propose(const glowhip_mala_seg* segs /* HOST, copied */, int n_segs, int n_leaves, int N, const float* step,
                         const unsigned long long* pos, void* scratch, size_t scratch_bytes, glowhip_stream_t stream);
int glowhip_mala_energy(const glowhip_mala_seg* segs /* HOST, copied */, int n_segs, int n_leaves, int N, const float* step,
                        void* scratch, size_t scratch_bytes, glowhip_stream_t stream);
int glowhip_mala_select(const glowhip_mala_seg* segs /* HOST, copied */, int n_segs, int n_leaves, int N, float* loss,
                        const float* loss_prop, float* step, unsigned long long* pos, long long* iteration, int32_t* counts,
                        float* hist, int steps, int burn_in, float adapt_rate, float step_min, float step_max, unsigned int* ticket,
                        const void* scratch, size_t scratch_bytes, glowhip_stream_t stream);
int glowhip_posterior_moments(const float* image, float* mean, float* m2, const long long* iteration, int iter_offset, int burn_in,
                              int thin, long n, glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Top head: learned / class-conditional top prior + classifier (reference network/model.py:345-348, 362-379, 440-445,
 * 508-538; LinearZeros network/module.py:152-185: out = (x W^T + b) * exp(3 logs)).  All fp32, in both kernel families.
 *   prior    h[n, :, p] = base[:] + e[n, :];  e = y_emb(y_onehot) (width 2C);  base[c] = learn_top.bias[c] * exp(3 learn_top.logs[c])
 *            (learn_top is applied to h_top == 0, network/model.py:372-376) or 0;  mean = h[:, :C], logs = h[:, C:]
 *   logits   classifier(mean_{H,W} z)
 * With a head attached, glowhip_glow_forward / _u8 / _forward_train add logp(z | mean, logs) with ONE launch (k_top_head_fwd)
 * that also writes the logits and, with a criterion, the per-sample classification-loss term and
 * g_logit = weight_y * d classification / d logits; glowhip_glow_backward produces dL/dz with ONE launch (k_top_head_bwd) and
 * the head's parameter gradients with one small reduction launch.  The prior_mean / prior_logs arguments of those calls are
 * added to the head's (a dense base; it gets no gradient).
 * ---------------------------------------------------------------------------------------------- */
enum { GLOWHIP_CRIT_NONE = 0, GLOWHIP_CRIT_CE = 1 /* Glow.single_class_loss, network/model.py:508-521 */,
       GLOWHIP_CRIT_BCE = 2 /* Glow.multi_class_loss, network/model.py:523-538 */ };
/* Device pointers to the live parameters (NULL = that part is absent): learn_top.{bias,logs} (2C), y_emb.{weight (2C,K), bias,
 * logs (2C)}, classifier.{weight (K,C), bias, logs (K)} -- the classifier only when weight_y > 0 (network/model.py:441). */
typedef struct glowhip_head_desc {
    int32_t K;             /* hps.dataset.num_classes */
    int32_t criterion;     /* GLOWHIP_CRIT_*: NONE = logits only (the caller's own loss hands g_logit to the backward) */
    float weight_y;        /* loss = generative + weight_y * classification, network/trainer.py:125-131 */
    int32_t reserved;
    const float* lt_bias; const float* lt_logs;
    const float* ye_w; const float* ye_b; const float* ye_logs;
    const float* cl_w; const float* cl_b; const float* cl_logs;
} glowhip_head_desc;
/* What changes per batch (device pointers).  state: glowhip_plan_head_state_bytes(plan, N) bytes written by the forward and read
 * by the matching backward.  y_onehot (N,K) fp32; y (N) int64 targets (CE); y_logits (N,K) out; cls_loss (N) out: the per-sample
 * term whose mean is the classification loss; g_logit (N,K): written by a forward with a criterion, otherwise the caller's
 * d loss / d logits for the backward (NULL = 0). */
typedef struct glowhip_head_io {
    const float* y_onehot; const int64_t* y;
    float* y_logits; float* cls_loss; float* g_logit; float* state;
} glowhip_head_io;
/* Writable gradients of the head's parameters (NULL = not wanted), next to glowhip_layer_grads. */
typedef struct glowhip_head_grads {
    float* lt_bias; float* lt_logs; float* ye_w; float* ye_b; float* ye_logs; float* cl_w; float* cl_b; float* cl_logs;
} glowhip_head_grads;
/* Attach (head != NULL; copied) or detach a head; clears the bindings below.  HOST bookkeeping, the caller serialises it with
 * the plan's own calls, as glowhip_plan_set_family. */
int glowhip_plan_set_head(glowhip_plan* plan, const glowhip_head_desc* head);
size_t glowhip_plan_head_state_bytes(const glowhip_plan* plan, int N);
/* Per-call bindings (copied; HOST bookkeeping): the io of the next forward / backward, the gradients of the next backward. */
int glowhip_plan_bind_head(glowhip_plan* plan, const glowhip_head_io* io);
int glowhip_plan_bind_head_grads(glowhip_plan* plan, const glowhip_head_grads* grads);
/* Glow.prior(y_onehot), network/model.py:362-379, as dense tensors: mean, logs (N,C,HW) -- for callers that need them as
 * tensors (the top sample of Glow.reverse_flow, network/model.py:466-468). */
int glowhip_top_prior(const glowhip_head_desc* head, const float* y_onehot, int N, int C, int HW, float* mean, float* logs,
                      glowhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LU-parameterised invertible 1x1 convolution (csrc/invconv_lu.hip).  The reference names the option and stops:
 * Invertible1x1Conv(lu_decomposition=True) raises at network/module.py:336-337.  This is the form of the Glow paper:
 *   W = P (tril(l, -1) + I) (triu(u, 1) + diag(sign_s * exp(log_s)))
 * with P a fixed permutation given as its row table perm (C int32: row i of P has its one in column perm[i]), l, u (C,C),
 * log_s, sign_s (C).  Entries of l on or above and of u on or below the diagonal are never read.  C <= 512.
 * No factorisation: log|det W| = sum(log_s) in fp64, W^-1 by forward and back substitution.
 * ---------------------------------------------------------------------------------------------- */
/* Stand-alone twin of glowhip_invconv_prepare (the determinant and inverse of network/module.py:357,365 for the LU form):
 * w_out (C*C) <- W, winv_out (C*C, may be NULL) <- W^-1, logabsdet_out (1 float, may be NULL) <- sum(log_s). */
int glowhip_invconv_lu_prepare(const int32_t* perm, const float* l, const float* u, const float* log_s, const float* sign_s,
                               int C, float* w_out, float* winv_out, float* logabsdet_out, glowhip_stream_t stream);
/* Gradients of the factors from dW (C*C), the gradient w.r.t. the assembled matrix WITHOUT any log-det part, and
 * logdet_term = HW * sum_n dL/dlogdet[n] (the log-det term log|det W| * HW of network/module.py:357 reaches log_s alone):
 *   dl = strict-lower(P^T dW U_f^T), du = strict-upper(L^T P^T dW), dlog_s[i] = (L^T P^T dW)[i][i] sign_s[i] exp(log_s[i]) + logdet_term.
 * Masked entries of dl / du are written as exact zeros. */
int glowhip_invconv_lu_backward(const int32_t* perm, const float* l, const float* u, const float* log_s, const float* sign_s,
                                int C, const float* dW, double logdet_term, float* dl, float* du, float* dlog_s,
                                glowhip_stream_t stream);
/* A FlowStep of a plan in the LU form.  w: writable (C*C) buffer the layer's desc.invconv_w points at -- every pack assembles W
 * into it first, on the caller's stream, and the layer takes part in no factorisation of the pack (network/module.py:336-337 is
 * where the reference would have done the same).  Call once after glowhip_plan_create; pointers copied, HOST bookkeeping, in the
 * pattern of glowhip_plan_bind_head.  W^-1 of such a layer is rebuilt by packs with GLOWHIP_PACK_INVERSE only: the backward
 * sweep does not read it. */
typedef struct glowhip_invconv_lu {
    const int32_t* perm; const float* l; const float* u; const float* log_s; const float* sign_s; float* w;
} glowhip_invconv_lu;
int glowhip_plan_bind_invconv_lu(glowhip_plan* plan, int layer, const glowhip_invconv_lu* lu);
/* Writable gradients of an LU-form layer for the next backward sweeps (copied; NULL unbinds): they take the place of
 * glowhip_layer_grads.invconv_w, which the sweep ignores for such a layer. */
typedef struct glowhip_invconv_lu_grads { float* dl; float* du; float* dlog_s; } glowhip_invconv_lu_grads;
int glowhip_plan_bind_invconv_lu_grads(glowhip_plan* plan, int layer, const glowhip_invconv_lu_grads* grads);

/* Per-launch timing for benchmarks (HIP events recorded on the execution stream around every kernel of
 * the coupling path).  enable=1 creates an event pool (host resource), enable=0 destroys it; while enabled
 * every encode/decode appends records.  glowhip_plan_timing_read synchronises with the recorded events,
 * copies up to `max` records (launch order) and clears the list. */
enum { GLOWHIP_K_CHANMIX = 0, GLOWHIP_K_CONV_F0 = 1, GLOWHIP_K_CONV_F2 = 2, GLOWHIP_K_CONV_F4 = 3, GLOWHIP_K_OTHER = 4,
       GLOWHIP_K_CNET = 5 /* k_cnet: f.0 + f.2 + f.4 of a FlowStep */, GLOWHIP_K_CFINISH = 6 /* its finishing kernel */,
       GLOWHIP_K_CNET_TAPE = 7 /* training forward: k_cnet storing h1 / h2 */, GLOWHIP_K_CNET_BWD = 8 /* input-gradient chain on k_cnet */,
       GLOWHIP_K_WGRAD = 9 /* a FlowStep's three weight-gradient GEMMs + their split-K reduction */ };
typedef struct glowhip_timing_record {
    int32_t kind;   /* GLOWHIP_K_* */
    int32_t layer;  /* index into the plan's layer list */
    int32_t mfma;   /* 1 = MFMA kernel, 0 = direct kernel */
    float ms;       /* elapsed between the two events */
} glowhip_timing_record;
int glowhip_plan_timing_enable(glowhip_plan* plan, int enable);
int glowhip_plan_timing_read(glowhip_plan* plan, glowhip_timing_record* out, int max, int* n_out);

/* Testing hook: forces kernel variants so that every one can be exercised at any batch size (parity tests, A/B runs).  The argument
 * is an OR of the GLOWHIP_DBG_* values below; 0 restores automatic selection.
 * Process-wide, not thread safe: a testing hook, not part of the operator surface. */
enum {
    GLOWHIP_DBG_TAIL_TILE_MASK      = 0xff,       /* low byte: pixels per workgroup of the fused tail convolution (16/32/64/128; 0 = cost model) */
    GLOWHIP_DBG_TAIL_MSPLIT         = 0x100,      /* tail convolution: always split the out-channel tiles over blockIdx.y */
    GLOWHIP_DBG_TAIL_NO_MSPLIT      = 0x200,      /* ... never split them */
    GLOWHIP_DBG_TAIL_NO_DMA         = 0x400,      /* ... no LDS-DMA tail kernels */
    GLOWHIP_DBG_EXACT_FP32          = 0x800,      /* exact-fp32 MFMA kernels only (split-half f16 path off, training included) */
    GLOWHIP_DBG_PACK_UNFUSED        = 0x1000,     /* the forward-only pack as its per-kind launches, not the one k_pack_fused launch (same bytes: A/B) */
    GLOWHIP_DBG_NO_MIXER_FUSION     = 0x8000,     /* k_squeeze + k_chanmix + a plain finishing kernel as separate launches (bitwise equal) */
    GLOWHIP_DBG_NO_CNET1W           = 0x10000,    /* no k_cnet1w (one wave per SIMD, csrc/cnet1w_sh.hip): k_cnet takes its launches (A/B) */
    /* 0x20000: reserved, formerly GLOWHIP_DBG_CNET1W_ROW_SPLIT (removed; last present in commit ffbde06) */
    GLOWHIP_DBG_NO_CNET1W_BWD       = 0x40000,    /* no backward instance of k_cnet1w (level-1 input gradient back on k_cnet: A/B) */
    GLOWHIP_DBG_WGRAD_NARROW        = 0x80000,    /* f.2's weight-gradient GEMM on 128-column tiles at every level (no k_wgrad_gemm_ps512) */
    /* 0x100000: reserved, formerly GLOWHIP_DBG_FUSED_FINISH (removed; last present in commit ffbde06) */
    GLOWHIP_DBG_LU_WORKGROUP        = 0x200000,   /* log|det W| of the 12 / 24 / 48-wide matrices on the workgroup-wide LU (same bits: A/B) */
    GLOWHIP_DBG_CNET_ROWS_SHIFT     = 22,         /* bits 22..24 = 1, 2 or 4: that many row splits of k_cnet (value << SHIFT) */
    GLOWHIP_DBG_CNET_128_ONLY       = 0x2000000,  /* k_cnet with 128-pixel tiles only */
    GLOWHIP_DBG_CNET_64             = 0x4000000,  /* k_cnet with 64-pixel tiles wherever supported */
    /* 0x8000000: reserved, formerly GLOWHIP_DBG_CNET_CHAIN (removed; last present in commit dbe339a) */
    GLOWHIP_DBG_CFINISH_BLOCK_ORDER = 0x10000000, /* the finishing kernel takes its pixel chunks in block order, not the XCD-affine order (A/B) */
    GLOWHIP_DBG_PACK_ONE_STREAM     = 0x20000000, /* glowhip_plan_pack entirely on the caller's stream, no side-stream fork (A/B) */
    GLOWHIP_DBG_TRAIN_PER_LAYER_FWD = 0x40000000, /* glowhip_glow_forward_train on the per-layer kernels, no taping k_cnet (A/B, parity tests) */
    GLOWHIP_DBG_TRAIN_PER_LAYER_BWD = INT32_MIN   /* bit 31 (0x80000000 as the hook's int): glowhip_glow_backward's input-gradient chain on
                                                     the per-layer kernels, no backward k_cnet */
};
void glowhip_debug_force_tail_tile(int pixels_and_flags);

/* Testing hook: ONE launch of the weight-gradient kernels (csrc/wgrad_mfma.hip, csrc/backward.hip) on operands the caller lays
 * out, through the launchers the backward sweep itself calls -- tests/test_gpu_wgrad.py holds every instance to fp64 with it.
 * Not part of the operator surface.  All pointers are device pointers; the layouts are those of the launchers (csrc/backward.h).
 *   op GLOWHIP_WGRAD_MFMA:   gemm[0] through launch_wgrad_mfma with every argument below (taps[0].operand < 0: no gathered operand)
 *   op GLOWHIP_WGRAD_PAIR:   launch_wgrad_group on gemm[0] = f.4 (A = g_pre, B = h2 fp16, Mpad = m4, Npad = hidden), gemm[1] = f.0
 *                            (A = g_u0, B = y1, Mpad = hidden, Npad = n0); taps[0] / taps[1] their gathered tensors;
 *                            then launch_wgrad_reduce_batched on the jobs the launcher returned
 *   op GLOWHIP_WGRAD_TRIO:   the same with gemm[2] = f.2 (A = g_u2, B = h1 fp16, hidden x hidden)
 *   op GLOWHIP_WGRAD_SHIFT_EXPAND:  gemm[0].A (batch stride a_bs) -> gemm[0].dw, taps[0] = (C, H, W, sign), rows_pad = gemm[0].Mpad
 *   op GLOWHIP_WGRAD_DIRECT: gy = gemm[0].A, x = gemm[0].B (batch stride b_bs) -> gemm[0].dw; Cout = Mreal, Cin = Nreal,
 *                            taps[0].H / W the map, ksize (1 or 3)
 *   op GLOWHIP_WGRAD_HALF_TO_FLOAT: gemm[0].B (fp16, pixel-tile-major, Npad rows) -> gemm[0].dw (N, Npad, HW)
 * A NULL gemm[i].partial in one of the three GEMM ops launches nothing: info->partial_floats[i] alone is filled, with what the
 * sweep allocates for that GEMM (N, HW, Mpad, Npad).  Whatever the launchers refuse is refused here: GLOWHIP_EINVAL, no launch. */
enum { GLOWHIP_WGRAD_MFMA = 0, GLOWHIP_WGRAD_PAIR = 1, GLOWHIP_WGRAD_TRIO = 2, GLOWHIP_WGRAD_SHIFT_EXPAND = 3,
       GLOWHIP_WGRAD_DIRECT = 4, GLOWHIP_WGRAD_HALF_TO_FLOAT = 5 };
/* glowhip_wgrad_info.instance: the kernel instance that ran */
enum { GLOWHIP_WGI_F32_128 = 1, GLOWHIP_WGI_F32_64 = 2,                      /* k_wgrad_gemm<128 / 64> */
       GLOWHIP_WGI_SH = 0x100,                                                /* k_wgrad_gemm_sh<...>: OR of the template flags below */
       GLOWHIP_WGI_BN64 = 1, GLOWHIP_WGI_VA = 2, GLOWHIP_WGI_VB = 4, GLOWHIP_WGI_BV = 8, GLOWHIP_WGI_BH = 16,
       GLOWHIP_WGI_PS128 = 0x200, GLOWHIP_WGI_PS64 = 0x201, GLOWHIP_WGI_PS512 = 0x202,   /* k_wgrad_gemm_ps<128 / 64>, k_wgrad_gemm_ps512 */
       GLOWHIP_WGI_PAIR64 = 0x300, GLOWHIP_WGI_PAIR128 = 0x301,              /* k_wgrad_gemm_pair<64 / 128> */
       GLOWHIP_WGI_TRIO64 = 0x400, GLOWHIP_WGI_TRIO128 = 0x401,              /* k_wgrad_gemm_trio<64 / 128> */
       GLOWHIP_WGI_SHIFT_EXPAND = 0x500, GLOWHIP_WGI_DIRECT1 = 0x501, GLOWHIP_WGI_DIRECT3 = 0x503, GLOWHIP_WGI_HALF_TO_FLOAT = 0x600 };
typedef struct glowhip_wgrad_gemm {
    const void* A; const void* B; float* partial; float* dw; double* rowsum;   /* rowsum NULL: none */
    int64_t a_bs, b_bs;                                                         /* batch strides in elements */
    int32_t Mpad, Npad, Mreal, Nreal, mode, b_valid, b_half, tiled;
} glowhip_wgrad_gemm;
typedef struct glowhip_wgrad_taps { int32_t operand, C, H, W, sign; } glowhip_wgrad_taps;
typedef struct glowhip_wgrad_probe {
    int32_t op, N, HW, ksize;
    float sh_scale; int32_t reserved;
    glowhip_wgrad_gemm gemm[3];
    glowhip_wgrad_taps taps[2];
} glowhip_wgrad_probe;
typedef struct glowhip_wgrad_info {
    int32_t instance[3], splits[3], ktiles_per_split[3], blocks[3], live[3];   /* per GEMM, in the order of probe.gemm */
    int32_t reserved;
    int64_t partial_floats[3];
} glowhip_wgrad_info;
int glowhip_debug_wgrad(const glowhip_wgrad_probe* d, glowhip_wgrad_info* info, glowhip_stream_t stream);

/* Testing hook: ONE launch of an HBM-bound gradient kernel of the training sweep (csrc/backward.hip) on operands the caller lays
 * out, through the launchers the backward sweep itself calls (csrc/backward.h) -- tests/test_gpu_bwd_kernels.py holds every route
 * to fp64 with it.  Not part of the operator surface.  All pointers are device pointers except the probe itself; strides are in
 * elements; the accumulators are fp64 and zeroed by the caller, as the sweep zeroes them.  Operands per op (unused ones NULL / 0):
 *   COUPLING     launch_coupling_bwd: src = {hout, z2out, g2, e4, gld}, bs = {z_bs, g_bs}, dst = {gy2 (may be g2), gpre},
 *                acc = {acc_b, acc_l}; C = Ch, C2 = Cout, flag = affine, acc_copies / acc_stride
 *   SPLIT        launch_split_bwd: src = {hout, z2, NULL, e4, gld}, bs = {z_bs, g_bs}, dst = {gz2, gpre}, acc = {acc_b, acc_l}; C = Ch
 *   ACT          launch_act_bwd: src = {h, NULL, NULL, e}, dst = {g (in place)}, acc = {acc_b, acc_l}; C = Cm
 *   CHANMIX      launch_chanmix_bwd: src = {x, gy, bias, scale, matrix or NULL, gather_inv or NULL, add_part or NULL}, bs = {x_bs, g_bs},
 *                dst = {gx (may be gy)}, acc = {acc_w, acc_b, acc_l}, acc_copies / acc_stride, add_scale and add = {C, MS, tiles, R, NI,
 *                lpxt, H, W}; n_jobs (0..3) split-K reductions ride along: job[i] = {a = partial, out = dw, n = {splits, Mpad, Npad,
 *                Mreal, Nreal, mode}} (WgradReduceJob)
 *   PRIOR        launch_prior_bwd: src = {z, mean or NULL, logs or NULL, NULL, gld, gz_in or NULL}, bs = {ml_bs}, dst = {gz}, per
 *   FLIP         launch_weight_flipT: src = {w}, dst = {wT}; C = Cout, C2 = Cin, ksize
 *   LOGS_FROM_DW launch_logs_from_dw_batched on n_jobs jobs {a = w, b = dw, c = b, d = db (fp64), out, n = {rows, K}} (LogsJob)
 *   FINALIZE     launch_gld_from_nll (src[0] = nll_grad -> dst[0] = gld, N values, factor inv), launch_sum_gld (gld -> acc[0], one
 *                double) and launch_grad_finalize_batched on n_jobs jobs {a = acc, b = winv or NULL, out (NULL: the job is skipped),
 *                n = {n, C, copies}, stride, add_mul} (GradJob)
 * The two job tables are copied to the device by the hook, which waits for the stream before it returns in those two ops.
 * Whatever a launcher refuses is refused here: GLOWHIP_EINVAL, no launch. */
enum { GLOWHIP_BWD_COUPLING = 0, GLOWHIP_BWD_SPLIT = 1, GLOWHIP_BWD_ACT = 2, GLOWHIP_BWD_CHANMIX = 3, GLOWHIP_BWD_PRIOR = 4,
       GLOWHIP_BWD_FLIP = 5, GLOWHIP_BWD_LOGS_FROM_DW = 6, GLOWHIP_BWD_FINALIZE = 7 };
/* glowhip_bwd_info.kernel: the kernel that ran */
enum { GLOWHIP_BWI_COUPLING4 = 1, GLOWHIP_BWI_COUPLING1 = 2,       /* k_coupling_bwd4 (16-byte accesses) / k_coupling_bwd */
       GLOWHIP_BWI_SPLIT = 3,
       GLOWHIP_BWI_ACT4 = 4, GLOWHIP_BWI_ACT1 = 5,                 /* k_act_bwd / k_act_bwd1 */
       GLOWHIP_BWI_CHANMIX = 6, GLOWHIP_BWI_CHANMIX_REDUCE = 7, GLOWHIP_BWI_CHANMIX_WIDE = 8,
       GLOWHIP_BWI_PRIOR = 9 };
enum { GLOWHIP_BWD_MAX_JOBS = 8 };
typedef struct glowhip_bwd_job {
    const void* a; const void* b; const void* c; const void* d; void* out;
    int32_t n[6];
    int64_t stride; double add_mul;
} glowhip_bwd_job;
typedef struct glowhip_bwd_probe {
    int32_t op, N, C, C2, HW, flag, ksize, acc_copies, n_jobs, reserved;
    int64_t acc_stride, bs[2], per;
    double inv;
    float add_scale; int32_t add[8], reserved2;
    const void* src[7]; void* dst[2]; double* acc[3];
    glowhip_bwd_job job[GLOWHIP_BWD_MAX_JOBS];
} glowhip_bwd_probe;
typedef struct glowhip_bwd_info {
    int32_t kernel, grid[3];
    int32_t threads_per_channel;       /* the 16-byte kernels of COUPLING / ACT: HW / 4 */
    int32_t w_lds, lds_bytes;          /* CHANMIX: matrix staged in LDS; dynamic LDS bytes of the launch */
    int32_t mix_blocks, rblocks;       /* CHANMIX: pixel blocks; blocks per reduction job (k_chanmix_bwd_reduce) */
    int32_t plain_stores;              /* CHANMIX: every pixel block owns its accumulator copy (stores, no atomics) */
    int32_t launches;                  /* kernel launches made (2: the reductions did not ride along) */
    int32_t reserved;
} glowhip_bwd_info;
int glowhip_debug_bwd(const glowhip_bwd_probe* d, glowhip_bwd_info* info, glowhip_stream_t stream);

/* Testing hook: ONE launch of an exact-fp32 convolution kernel (csrc/conv_mfma.hip, conv_mfma_first.hip, conv_direct.hip) on operands
 * the caller lays out, through the launchers the plan itself calls -- tests/test_gpu_conv_kernels.py holds every instance to fp64
 * with it.  Not part of the operator surface.  All pointers are device pointers except the probe itself; strides are in elements.
 *   WIDE    the image of w (Cout, Cin, k, k) is built by the plan's REPACK_WIDE job (launch_pack_batched) into `image`, then
 *           launch_conv_mfma_wide(x, x_bs, image, post_bias, post_scale, y, N, Cin, H, W, Cout, ksize, stream, relu, scratch,
 *           scratch_floats); scratch may be NULL (no split-K).  transposed (ksize 1 only): w is the forward weight (Cin, Cout), which
 *           is the K-major image of the input-gradient GEMM as it stands: passed to the launcher directly, as the training sweep does
 *   FIRST   the image is built by the REPACK_FIRST job with fold_bias / fold_logs (both or neither) and `transposed` (w is then the
 *           forward weight (Cin, Cout, 3, 3) of which this is the input-gradient convolution), then launch_conv_mfma_first(x, x_bs,
 *           image, image + 9 Cin Cout, y, N, Cin, H, W, Cout, stream, relu)
 *   DIRECT  launch_conv_direct on w in its reference layout with bias, post_bias, post_logs, post_scale (each may be NULL)
 *   TAIL    conv_mfma_tail_pack(w, Cin, Cout, paired, image) -- paired as the mode implies -- then launch_conv_mfma_tail on a
 *           TailConvArgs of x, x_bs, image, bias, scale = post_scale, mode (the TailMode values 0..6 of csrc/conv_mfma.h: PLAIN,
 *           AFFINE_FWD, AFFINE_REV, ADD_FWD, ADD_REV, SPLIT_FWD, SPLIT_REV), z2_in / z2_out with their strides, zeros (NULL or
 *           >= 16 bytes of zeros, 16-byte aligned), hout (NULL or (N, Cout, HW)) and an empty rng; the forced tile and the split /
 *           no-DMA switches of glowhip_debug_force_tail_tile hold as they do for a plan.  acc (NULL, or 2 N 64-bit words): zeroed
 *           with launch_zero_acc before the launch and turned into term[n] (N floats) with launch_finalize after it, as
 *           glowhip_gaussian_logp and the plan do it
 * A NULL `image` in WIDE / FIRST / TAIL launches nothing: info->image_bytes alone is filled, with what the plan allocates for that
 * image.  The hook waits for the stream in WIDE / FIRST (its one-job table is freed before it returns).  Whatever a launcher refuses
 * is refused here: GLOWHIP_EINVAL, no launch. */
enum { GLOWHIP_CONV_WIDE = 0, GLOWHIP_CONV_FIRST = 1, GLOWHIP_CONV_DIRECT = 2, GLOWHIP_CONV_TAIL = 3 };
/* glowhip_conv_info.kernel: the kernel that ran */
enum { GLOWHIP_CVI_WIDE = 1,        /* k_conv_wide<ksize, tile, tile, 32>, with k_splitk_finish behind it when splits > 1 */
       GLOWHIP_CVI_GEMM_GLDS = 2,   /* k_gemm_glds */
       GLOWHIP_CVI_FIRST = 3,       /* k_conv_first<tile, W> */
       GLOWHIP_CVI_DIRECT = 4,      /* k_conv_direct<ksize, 8> */
       GLOWHIP_CVI_TAIL = 5,        /* k_conv_tail<mb, ...> (register-staged), tile pixels per workgroup */
       GLOWHIP_CVI_TAIL_DMA = 6 };  /* k_conv_tail_dma<1, ..., W> */
typedef struct glowhip_conv_probe {
    int32_t op, N, Cin, H, W, Cout, ksize, relu, transposed, mode;
    int64_t x_bs, scratch_floats, z2_in_bs, z2_out_bs;
    const float* x; const float* w; const float* bias; const float* post_bias; const float* post_logs; const float* post_scale;
    const float* fold_bias; const float* fold_logs;
    float* image; float* scratch; float* y;
    const float* z2_in; float* z2_out; float* hout; const float* zeros; void* acc; float* term;      /* TAIL */
} glowhip_conv_probe;
typedef struct glowhip_conv_info {
    int32_t kernel, ksize;
    int32_t tile;                      /* WIDE: 64 / 128 (k_gemm_glds: 128); FIRST: pixels per workgroup BN; TAIL: TP */
    int32_t splits;                    /* WIDE: split-K slices S (1: none); TAIL: waves that share the reduction, WK */
    int32_t mb;                        /* FIRST: output-channel tiles per workgroup MB; TAIL: MT (grid[1] holds the rest) */
    int32_t grid[3];
    int32_t launches;                  /* kernel launches the launcher made (2: k_splitk_finish followed) */
    int32_t paired;                    /* TAIL: the paired row map */
    int64_t image_bytes;
} glowhip_conv_info;
int glowhip_debug_conv(const glowhip_conv_probe* d, glowhip_conv_info* info, glowhip_stream_t stream);

/* Testing hook: ONE launch of the fp32 code between the MFMA launches of a forward / decode / training step -- the finishing kernel
 * of the coupling network (csrc/cnet_sh.hip k_cfinish, csrc/cnet_fin.h), the channel mixer (csrc/pointwise.hip) and the deep levels'
 * finishing and first launches (csrc/dnet_sh.hip k_dn_fin, k_dn_prep) -- on operands the caller lays out, through the launchers
 * the plan itself calls; tests/test_gpu_fin_kernels.py holds every instance to fp64 with it.  Not part of the operator surface.  All
 * pointers are device pointers except the probe itself; strides are in elements.  Operands per op (unused ones NULL / 0):
 *   CFINISH  N, C (channels of the state = 2 Ch), H, W, Cout, hidden, mode (TailMode 1..4: AFFINE_FWD, AFFINE_REV, ADD_FWD, ADD_REV),
 *            MS (row-split copies in the scratch), tile (64 / 128 pixels per k_cnet tile); scratch (the partial sums k_cnet would have
 *            left: csrc/cnet_fin.h documents the layout), scratch_floats (what the caller allocated: refused below the plan's own
 *            size, which info reports), bias / scale (f.4 bias, exp(3 logs): Cout each), z_in / z_out with z_in_bs / z_out_bs, acc
 *            ((2 + ACC_EXTRA) N 64-bit words: accumulator row 0, the flag row, ACC_EXTRA more accumulator rows; zeroed by the caller),
 *            the mixer (mix_C = 0: none) and tape_hout.  The tiling (R, NI, tiles, lpxt) comes from cnet_geo(Ch, H, W, hidden, Cout,
 *            N, tile) through the helper launch_cnet_main fills its hand-over with; then launch_cnet_finish.  Block order:
 *            GLOWHIP_DBG_CFINISH_BLOCK_ORDER of glowhip_debug_force_tail_tile, as for a plan.  A NULL scratch launches nothing:
 *            info reports the tiling and the plan's scratch size alone
 *   CHANMIX  every field of ChanMixArgs (csrc/kernels.h): in_a / in_b with in_a_bs / in_b_bs and Ca, out / out_bs, mix_bias /
 *            mix_scale / mix_matrix / mix_gather, mix_reverse, N, C, HW (H and W are not read), sq_src / sq_u8 / sq_div / sq_noise /
 *            sq_W / sq_bs and the Philox draw rng_on / rng_seed / rng_call / rng_scale; then launch_chanmix
 *   DN_FIN   a DnetLevel (N, C, H, W, hidden, Cout, state with z_in_bs = its batch stride, dn_scratch) over caller memory; ks, bias /
 *            scale, mode, acc ((2 + ACC_EXTRA) N words as above), mix_bias / mix_scale = the next step's ActNorm (NULL: none) and
 *            want_u; then dnet_finish
 *   DN_PREP  the same level; src / src_bs, mix_bias / mix_scale, mix_reverse; then dnet_prep
 * In the two DN ops info reports where dn_carve puts `part`, `u` and `ypad` inside the level scratch (byte offsets; plane sizes in
 * fp16 elements) and the level's scratch bytes (scratch_bytes); a NULL dn_scratch launches nothing and fills only those.
 * Whatever a launcher refuses is refused here: GLOWHIP_EINVAL, no launch. */
enum { GLOWHIP_FIN_CFINISH = 0, GLOWHIP_FIN_CHANMIX = 1, GLOWHIP_FIN_DN_FIN = 2, GLOWHIP_FIN_DN_PREP = 3 };
/* glowhip_fin_info.kernel: the kernel that ran */
enum { GLOWHIP_FNI_CFINISH = 1,         /* k_cfinish<pxb, msv, halo> */
       GLOWHIP_FNI_CHANMIX16 = 2, GLOWHIP_FNI_CHANMIX64 = 3, GLOWHIP_FNI_CHANMIX_WIDE = 4,
       GLOWHIP_FNI_DN_FIN = 5, GLOWHIP_FNI_DN_PREP = 6 };
typedef struct glowhip_fin_probe {
    int32_t op, N, C, H, W, HW, Cout, hidden, mode, MS, tile, ks, want_u, Ca;
    int32_t mix_C, mix_reverse, sq_u8, sq_W, rng_on, reserved;
    float sq_div, rng_scale;
    uint64_t rng_seed, rng_call;
    int64_t z_in_bs, z_out_bs, in_a_bs, in_b_bs, out_bs, sq_bs, src_bs, scratch_floats;
    const float* scratch; const float* bias; const float* scale; const float* z_in; float* z_out; void* acc; float* tape_hout;
    const float* mix_bias; const float* mix_scale; const float* mix_matrix; const int32_t* mix_gather;
    const float* in_a; const float* in_b; float* out; const void* sq_src; const float* sq_noise;
    float* state; void* dn_scratch; const float* src;
} glowhip_fin_probe;
typedef struct glowhip_fin_info {
    int32_t kernel, grid[3], lds_bytes;
    int32_t pxb, msv, halo;            /* CFINISH: the template arguments of the instance */
    int32_t xcd_affine;                /* CFINISH: the launch took its pixel chunks in the XCD-affine order */
    int32_t stage_matrix;              /* CHANMIX (k_chanmix<16 / 64>): the matrix goes through LDS */
    int32_t R, NI, tiles, lpxt;        /* CFINISH: the tiling the hook derived */
    int32_t reserved;
    int64_t scratch_floats;            /* CFINISH: the floats the plan allocates for this launch's partial sums */
    int64_t scratch_bytes;             /* DN: the bytes of the level scratch for N samples */
    int64_t part_off, u_off, ypad_off, u_plane, ypad_plane;      /* DN */
} glowhip_fin_info;
int glowhip_debug_fin(const glowhip_fin_probe* d, glowhip_fin_info* info, glowhip_stream_t stream);

/* Testing hook: ONE SH2 weight image (csrc/pack.hip) or ONE launch of the one-kernel coupling network  h = f.4(relu(f.2(relu(f.0(z1)))))
 * (network/module.py:300-319; the coupling it feeds: network/model.py:105-150) on split-fp16 operands (csrc/sh.h "SH2":
 * csrc/cnet_sh.hip k_cnet, csrc/cnet1w_sh.hip k_cnet1w) on operands the caller lays out, through the pack code and the launcher the
 * plan itself calls -- tests/test_gpu_sh2_kernels.py holds every forward and taping instance to fp64 with it.  Not part of the
 * operator surface.  All pointers are device pointers except the probe itself; strides are in elements.
 *   IMAGE  one image of w into `image`, through the RepackJob fields csrc/plan_build.hip fills (add_sh2_first / _gemm / _tail): kind
 *          (GLOWHIP_SH2_GEMM: w (Cout, Cin); _FIRST: w (Cout, Cin, 3, 3), K = cnet_g0(Cin) groups; _TAIL: w (Cout, Cin, 3, 3), Kpad =
 *          cnet_mpad4(Cout) rows, always k-permuted), kperm (GEMM), fold_bias / fold_logs (GEMM / FIRST; NULL: none), and
 *          launch_pack_batched with the block counts the plan derives.  transposed: w is the FORWARD weight ((Cin, Cout) or
 *          (Cin, Cout, 3, 3)); launch_flipT_batched first writes its transposed, tap-flipped copy into `flip` (Cout Cin ks floats) and
 *          the image is packed from there, as the plan does for the backward images.  The hook waits for the stream (its job tables
 *          are freed before it returns).  A NULL image launches nothing: info->image_bytes alone
 *   CNET   launch_cnet_main on a CnetArgs of x / x_bs, the images w0 / w2 / w4, N, Cin, H, W, hidden, Cout, mode (TailMode 1..4),
 *          scratch; optional tape_h1 / tape_h2 / mask1 / mask2 with in_scale / out_scale, and bwd.  No finishing launch.  The
 *          switches of glowhip_debug_force_tail_tile hold as they do for a plan.  scratch_floats (what the caller allocated) is
 *          refused below the plan's own size, which info reports.  A NULL scratch launches nothing: info reports the instance the
 *          launch would take, its grid, LDS bytes, hand-over tiling and the plan's scratch size alone
 *   DN_MIX a DnetLevel (N, C = Cin, H, W, hidden, Cout, state with x_bs = its batch stride, dn_scratch) over caller memory, in which the
 *          caller has laid the u operand (glowhip_debug_fin's DN ops report the layout); dnet_level_begin, then dnet_mix(w0 = the
 *          SH2_GEMM image of W, or of W^-1 with post_scale / post_bias; want_pad).  info: <RT, PT, NPF> and grid in dn_*[0]
 *   DN_NET the same level; dnet_coupling_net(w0, w2, w4) = F0, F2, F4 on the padded z1 operand.  dnet_level_begin zeroes BOTH padded
 *          operands whole, so it is not called here: the caller lays ypad (zero border included) and zero-fills h2pad, whose
 *          interior F2 writes, as dnet_level_begin leaves them.  info: ks, the three launches in dn_*[0..2], part_off
 * In the two DN ops a NULL dn_scratch launches nothing and reports scratch_bytes and part_off alone.
 * Whatever the launcher refuses is refused here: GLOWHIP_EINVAL, no launch. */
enum { GLOWHIP_SH2_IMAGE = 0, GLOWHIP_SH2_CNET = 1, GLOWHIP_SH2_DN_MIX = 2, GLOWHIP_SH2_DN_NET = 3 };
enum { GLOWHIP_SH2_GEMM = 3, GLOWHIP_SH2_FIRST = 4, GLOWHIP_SH2_TAIL = 5 };      /* probe.kind: the REPACK_SH2_* kinds of csrc/kernels.h */
/* glowhip_sh2_info.kernel: the kernel that ran */
enum { GLOWHIP_S2I_CNET = 1,        /* k_cnet<hid, ms, upw, pxt, ng, mode> */
       GLOWHIP_S2I_CNET1W = 2 };    /* k_cnet1w<hid, g0, nrt4, mode> */
typedef struct glowhip_sh2_probe {
    int32_t op, kind, N, Cin, H, W, hidden, Cout, mode, bwd, kperm, transposed, want_pad, reserved;
    float in_scale, out_scale;
    int64_t x_bs, scratch_floats;
    const float* w; const float* fold_bias; const float* fold_logs; float* flip; void* image;      /* IMAGE */
    const float* x; const void* w0; const void* w2; const void* w4; float* scratch;                  /* CNET */
    void* tape_h1; void* tape_h2; void* mask1; void* mask2;
    float* state; void* dn_scratch; const float* post_scale; const float* post_bias;                 /* DN_MIX / DN_NET */
} glowhip_sh2_probe;
typedef struct glowhip_sh2_info {
    int32_t kernel, hid, ms, upw, pxt, ng, mode, g0, nrt4;      /* the instance's template arguments (upw: k_cnet only; g0 / nrt4 always) */
    int32_t grid[3], lds_bytes;
    int32_t MS, tiles, R, NI, lpxt;    /* the hand-over tiling (CnetPending) */
    int32_t Kp, M;                     /* IMAGE: padded k and rows of the image */
    int32_t dn_launches, ks;           /* DN: k_dn_gemm launches made; DN_NET: K-split copies F4 left in `part` */
    int32_t dn_rt[3], dn_pt[3], dn_npf[3], dn_grid[9];      /* DN: k_dn_gemm<8, RT, PT, NPF> and grid (x, y, z) per launch */
    int64_t part_off, scratch_bytes;   /* DN: where `part` lies in the level scratch (bytes); the level scratch for N samples */
    int64_t scratch_floats;            /* CNET: the floats the plan allocates for this launch's partial sums */
    int64_t image_bytes;               /* IMAGE */
} glowhip_sh2_info;
int glowhip_debug_sh2(const glowhip_sh2_probe* d, glowhip_sh2_info* info, glowhip_stream_t stream);

/* Introspection for tests / benchmarks: which kernels a plan will launch ("mfma" or "direct" per
 * convolution).  Writes a NUL-terminated description into buf. */
int glowhip_plan_describe(const glowhip_plan* plan, char* buf, size_t buf_bytes);
/* The same for a given batch size N: kernel choices that depend on how many workgroups a launch would have (the fused
 * f.0 + f.2 kernel runs only when N*H*W/64 workgroups cover the chip) are resolved as encode/decode would resolve them. */
int glowhip_plan_describe_for(const glowhip_plan* plan, int N, char* buf, size_t buf_bytes);
/* Run-time evidence of kernel selection: "kernel_family=launches\n" lines for every kernel family this plan has launched
 * (coupling path of encode / decode / glow_forward) since creation or the last reset.  HOST bookkeeping, counted at launch. */
int glowhip_plan_launch_counts(glowhip_plan* plan, char* buf, size_t buf_bytes, int reset);

#ifdef __cplusplus
}
#endif
#endif /* GLOWHIP_H */

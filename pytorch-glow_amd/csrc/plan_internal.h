// plan_internal.h -- plan data structures shared by plan_build.hip (plan construction, parameter pack), plan.hip (inference
// executor) and plan_train.hip (training forward with a tape + backward executor).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#include "conv_mfma.h"
#include "sh.h"
#include "backward.h"
#include "tophead.h"
#include "invconv_lu.h"
#include "debug_switches.h"

namespace glowhip {

struct LayerPlan {
    glowhip_layer_desc d;
    int split_idx = -1;  // Split2d: its ordinal in ENCODE order (0 = the shallowest)
    int Cout = 0;  // output channels of f.4 / of the Split2d prior conv
    // byte offsets into the packed buffer
    size_t an_scale = 0, an_inv_scale = 0, winv = 0, logabsdet = 0, konst = 0, lu_scratch = 0;
    size_t f0_scale = 0, f2_scale = 0, f4_scale = 0;
    size_t f0_wt = 0, f2_wt = 0, f4_wp = 0;
    bool mfma_first = false, mfma_mid = false, mfma_last = false;
    // training: input-gradient convolutions run on the forward kernels with flipped/transposed weight images
    size_t f4T_wf = 0, f0T_wp = 0;
    bool dg4_first = false, dg0_tail = false;
    bool cnet = false; size_t cn_w0 = 0, cn_w2 = 0, cn_w4 = 0;   // whole coupling network as one kernel (cnet_sh.hip), SH2 images
    // the input-gradient chain as one k_cnet launch (MODE 2): SH2 images of the transposed weights (cb_w0: f.4^T as the 3x3 first
    // layer, cb_w2: f.2^T, cb_w4: f.0^T as the 3x3 last layer) and the transposed fp32 copies they are built from (wt4 / wt2 / wt0)
    bool cnet_bwd = false; size_t cb_w0 = 0, cb_w2 = 0, cb_w4 = 0, wt4 = 0, wt2 = 0, wt0 = 0;
    // deep levels (dnet_sh.hip): one launch per layer on SH2 images -- the mixer W (and W^-1, built after the LU), f.0 and f.4 as
    // (chunk, tap) implicit-GEMM images, f.2 as a plain GEMM image
    bool dnet = false; size_t dn_mix = 0, dn_mixinv = 0, dn_w0 = 0, dn_w2 = 0, dn_w4 = 0;
    bool wide_last = false; size_t f4_wt = 0;   // f.4 on k_conv_wide<3> (+ separate coupling tail): levels no tail kernel takes (4x4 pixels)
    bool first_halo = false;  // f.0 on k_conv_first (stationary pixel window) instead of k_conv_wide<3>
    size_t f0_init = 0;       // data-dependent init pass: PLAIN K-major image of f.0 for k_conv_wide<3> (the k_conv_first image has
                              // the ActNorm being initialised folded in); 0 = none (the direct kernel runs)
};

// The use mask of a pack (glowhip_plan_pack_for, RepackJob::use): GLOWHIP_PACK_INFERENCE / _TRAINING / _INVERSE of the header, and
enum { PACK_EXACT_FP32 = 8,      // the exact-fp32 images of layers that normally run k_cnet / the deep-level kernels
       PACK_INIT_F0 = 16,        // the init pass' plain f.0 image
       PACK_NO_LU = 32 };        // no LU: weight images and scale tables only
// the bits that select images (INVERSE: the W^-1 images of the deep levels); PACK_NO_LU does not change the repack table
constexpr int PACK_IMAGE_BITS = GLOWHIP_PACK_INFERENCE | GLOWHIP_PACK_TRAINING | GLOWHIP_PACK_INVERSE | PACK_EXACT_FP32 | PACK_INIT_F0;
constexpr int REPACK_SLOTS = PACK_IMAGE_BITS + 1;
static inline int repack_slot(int use) { return use & PACK_IMAGE_BITS; }      // slot of a use mask's selected repack jobs
constexpr size_t PACK_SEG_HEAD = 16;

// Per-level terms of the objective (evaluate.hip; glowhip_plan_bind_level_terms).  A level is a maximal run of layers that ends with a
// Split2d, the last one ends with the top prior.  LevelKonst rides in the kernel arguments of the one k_level_terms launch: the konst
// words (LayerPlan::konst, byte offset / 8) of the FlowSteps of level l are off8[first[l] .. first[l + 1]).
constexpr int LEVEL_MAX = 16, LEVEL_MAX_STEPS = 896;
struct LevelKonst { uint32_t first[LEVEL_MAX + 1]; uint32_t off8[LEVEL_MAX_STEPS]; };
int launch_level_snapshot(const unsigned long long* acc, unsigned long long* dst, int N, hipStream_t s);
int launch_level_terms(const unsigned long long* snap, const void* packed, const LevelKonst& kt, int n_levels, int N, float* terms,
                       hipStream_t s);

}  // namespace glowhip

using namespace glowhip;

struct TimingSlot { int kind, layer, mfma; hipEvent_t a, b; };

struct glowhip_plan {
    std::vector<LayerPlan> layers;
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;     // unused events
    std::vector<TimingSlot> ev_used;     // recorded, not yet read
    int cur_layer = 0;
    // batched pack: host copies of the job tables + their byte offsets inside `packed`
    std::vector<StepPrepJob> prep_jobs;
    std::vector<ScaleJob> scale_jobs;
    std::vector<RepackJob> repack_jobs;
    std::vector<FlipJob> flip_jobs; int flip_tiles[3] = {1, 1, 1}; size_t flip_off = 0;      // (tiles: max per member of a (f.4, f.2, f.0) triple)
    std::vector<RepackJob> repack_sel;    // the subset selected by the last glowhip_plan_pack_for (kept alive for the async copy)
    size_t prep_off = 0, scale_off = 0, repack_off = 0;
    // one-launch forward pack (k_pack_fused): its block table (plan-constant, built by the first such pack), where it lives in
    // `packed` behind PACK_SEG_HEAD bytes that hold the LU workgroups' arrival counter, and whether tables_in holds it already
    std::vector<glowhip::PackSeg> pack_segs; int pack_segs_slot = -1; size_t seg_off = 0, seg_cap = 0; bool segs_in = false;
    // glowhip_plan_pack forks onto a side stream what the first kernels of a forward do not wait for: the round-1 / fp32 weight images
    // (read by the deep levels and the Split2d priors) and the LU factorisations (log|det W| enters only the final sum; W^-1 is
    // read by decode / backward).  Consumers join through these events (join_legacy / join_lu).
    hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_legacy = nullptr, ev_lu = nullptr;
    bool legacy_pending = false, lu_pending = false;
    const void* tables_in = nullptr;      // the `packed` buffer that already holds the job tables (glowhip_plan_forget_packed resets)
    unsigned slots_in = 0;                // ... and which of its repack-table slots (repack_slot) have been filled
    std::vector<RepackJob> repack_slot_host[REPACK_SLOTS];
    bool pending_captured = false;        // ev_legacy / ev_lu were last recorded inside a stream capture (see join_legacy)
    int max_lds_c = 0, max_c = 0;
    size_t packed_bytes = 0;
    int in_shape[3] = {0, 0, 0}, out_shape[3] = {0, 0, 0};
    long max_chw = 0;      // max over layer inputs/outputs of C*H*W
    long max_hidden = 0;   // max over steps of max(hidden, Cout) * H*W
    int n_split = 0;
    // glowhip_plan_bind_level_terms: terms [n_levels][N] and the caller's snapshot scratch (null = nothing bound)
    float* level_terms = nullptr; unsigned long long* level_scratch = nullptr; size_t level_scratch_bytes = 0;
    std::vector<float*> eps_out;               // glowhip_plan_bind_latents: per Split2d in DECODE order, empty = nothing bound
    std::vector<char> tape_has_masks;          // per layer: the last glow_forward_train stored the ReLU sign bits (k_cnet MODE 1)
    std::vector<glowhip::LogsJob> logs_jobs;   // the same for the log-scale gradients derived from dW / db (backward.h)
    std::vector<glowhip::GradJob> grad_jobs;   // host copy of the last backward's finalize table (kept alive for the async copy)
    bool rng_on = false; unsigned long long rng_seed = 0, rng_calls = 0;   // in-kernel dequantisation noise (glowhip_plan_set_dequant_rng)
    // glowhip_plan_bind_sampler: the device word {seed, call} (null = nothing bound), the std of every Split2d's draw in DECODE
    // order, and whether a call that drew ends with call += 1 on the device
    unsigned long long* sampler_pos = nullptr; std::vector<float> sampler_std; bool sampler_advance = false;
    std::vector<std::pair<int, hipEvent_t>> bwd_marks;   // (layer index, event): glowhip_plan_backward_marks
    int family = GLOWHIP_FAMILY_AUTO;          // kernel family of the coupling networks (glowhip_plan_set_family): a property of the plan
    // top head (tophead.hip): learned / class-conditional prior + classifier, its per-call io and gradient bindings
    bool head_on = false; glowhip_head_desc head{}; glowhip_head_io head_io{}; glowhip_head_grads head_grads{};
    // FlowSteps whose 1x1 convolution is kept as P L U factors (glowhip_plan_bind_invconv_lu; invconv_lu.hip): their pack jobs (host
    // copy + offset of the device copy inside `packed`, room reserved for every invconv FlowStep), the widest of them, their
    // gradient bindings (dl == null: none) and the host copy of the last sweep's gradient job table
    struct LuLayer { int layer; glowhip_invconv_lu_grads g; };
    std::vector<LuLayer> lu_layers; std::vector<glowhip::LuJob> lu_jobs; size_t lu_off = 0; int lu_max_c = 0;
    std::vector<glowhip::LuGradJob> lu_grad_jobs;
    std::map<std::string, long> launch_counts; // run-time record of which kernel families this plan launched (glowhip_plan_launch_counts)
};

namespace glowhip {

static inline void count_launch(glowhip_plan* p, const char* name) { if (p) ++p->launch_counts[name]; }

// ---------------------------------------------------------------- optional per-launch timing
struct ScopedTimer {
    glowhip_plan* p; hipStream_t s; TimingSlot slot; bool on;
    ScopedTimer(glowhip_plan* plan, int kind, int mfma, hipStream_t st) : p(plan), s(st), on(plan && plan->timing) {
        if (!on) return;
        auto get = [&]() { hipEvent_t e; if (!p->ev_pool.empty()) { e = p->ev_pool.back(); p->ev_pool.pop_back(); }
                           else (void)hipEventCreate(&e); return e; };
        slot.kind = kind; slot.layer = p->cur_layer; slot.mfma = mfma; slot.a = get(); slot.b = get();
        (void)hipEventRecord(slot.a, s);
    }
    ~ScopedTimer() { if (on) { (void)hipEventRecord(slot.b, s); p->ev_used.push_back(slot); } }
};

static inline bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive;
}
// An event recorded inside a stream capture belongs to that capture: waiting for it from a stream that is not capturing fails with
// hipErrorCapturedEvent -- and there is nothing to wait for: the capture joined its own fork, and replays order themselves as graph
// nodes.  So pending flags set during a capture are dropped by the first join that comes from outside one.
static inline bool drop_captured_pending(glowhip_plan* p, hipStream_t s) {
    if (!p->pending_captured || stream_capturing(s)) return false;
    p->legacy_pending = p->lu_pending = p->pending_captured = false;
    return true;
}
// make stream s wait for the side-stream part of the last pack (no-ops when nothing is pending)
static inline int join_legacy(glowhip_plan* p, hipStream_t s) {
    if (p->legacy_pending && !drop_captured_pending(p, s) && hipStreamWaitEvent(s, p->ev_legacy, 0) != hipSuccess) { set_error("join_legacy: hipStreamWaitEvent failed"); return GLOWHIP_ELAUNCH; }
    return GLOWHIP_OK;
}
static inline int join_lu(glowhip_plan* p, hipStream_t s) {
    if (p->lu_pending && !drop_captured_pending(p, s) && hipStreamWaitEvent(s, p->ev_lu, 0) != hipSuccess) { set_error("join_lu: hipStreamWaitEvent failed"); return GLOWHIP_ELAUNCH; }
    return GLOWHIP_OK;
}

static inline size_t take(size_t& off, size_t bytes) {
    size_t o = align_up(off, 256);
    off = o + bytes;
    return o;
}

template <typename T>
static inline T* at(const void* base, size_t off) {
    return (T*)((char*)base + off);
}

// ---------------------------------------------------------------- per-FlowStep argument builders of the two executors
static inline int tail_mode(const glowhip_layer_desc& d, int reverse) {
    return d.coupling == GLOWHIP_COUPLING_AFFINE ? (reverse ? TAIL_AFFINE_REV : TAIL_AFFINE_FWD) : (reverse ? TAIL_ADD_REV : TAIL_ADD_FWD);
}
static inline CnetMixer mixer_fwd(const LayerPlan& L, const void* packed) {      // ActNorm + permutation of step L, forward
    const glowhip_layer_desc& d = L.d;
    return CnetMixer{d.C, 0, d.an_bias, at<float>(packed, L.an_scale), d.permutation == GLOWHIP_PERM_INVCONV ? d.invconv_w : nullptr,
                     d.permutation == GLOWHIP_PERM_GATHER ? d.perm_idx : nullptr};
}
static inline CnetMixer mixer_rev(const LayerPlan& L, const void* packed) {      // permutation^-1 + ActNorm^-1 of step L
    const glowhip_layer_desc& d = L.d;
    return CnetMixer{d.C, 1, d.an_bias, at<float>(packed, L.an_inv_scale),
                     d.permutation == GLOWHIP_PERM_INVCONV ? at<float>(packed, L.winv) : nullptr,
                     d.permutation == GLOWHIP_PERM_GATHER ? d.perm_idx_inv : nullptr};
}
// the same mixers as their own k_chanmix launch: channels [0, C/2) from in_a, [C/2, C) from in_b (both with batch stride in_bs),
// contiguous (N, C, HW) output.  (A folded squeeze -- ChanMixArgs::sq_* -- is set by the caller.)
static inline ChanMixArgs chanmix_args(const LayerPlan& L, const CnetMixer& mx, int N, const float* in_a, const float* in_b, long in_bs,
                                       float* out) {
    const glowhip_layer_desc& d = L.d;
    const int HW = d.H * d.W;
    ChanMixArgs m{};
    m.in_a = in_a; m.in_a_bs = in_bs; m.in_b = in_b; m.in_b_bs = in_bs; m.Ca = d.C / 2;
    m.out = out; m.out_bs = (long)d.C * HW;
    m.bias = mx.bias; m.scale = mx.scale; m.matrix = mx.matrix; m.gather = mx.gather;
    m.reverse = mx.reverse; m.N = N; m.C = d.C; m.HW = HW;
    return m;
}
static inline ChanMixArgs chanmix_fwd_args(const LayerPlan& L, const void* packed, int N, const float* in, long in_bs, float* out) {
    return chanmix_args(L, mixer_fwd(L, packed), N, in, in + (long)(L.d.C / 2) * L.d.H * L.d.W, in_bs, out);
}
static inline ChanMixArgs chanmix_rev_args(const LayerPlan& L, const void* packed, int N, const float* in_a, const float* in_b, long in_bs,
                                           float* out) {
    return chanmix_args(L, mixer_rev(L, packed), N, in_a, in_b, in_bs, out);
}
// k_cnet of step L in the coupling network's own direction (cnet_sh.hip): weight images, shape, f.4's epilogue, the tail; the
// caller sets the tensors
static inline CnetArgs cnet_base(const LayerPlan& L, const void* packed, int N, int reverse, float* scratch, unsigned long long* acc) {
    const glowhip_layer_desc& d = L.d;
    CnetArgs c{};
    c.w0 = at<char>(packed, L.cn_w0); c.w2 = at<char>(packed, L.cn_w2); c.w4 = at<char>(packed, L.cn_w4);
    c.N = N; c.Cin = d.C / 2; c.H = d.H; c.W = d.W; c.hidden = d.hidden; c.Cout = L.Cout;
    c.scratch = scratch;
    c.bias = d.f4_bias; c.scale = at<float>(packed, L.f4_scale);
    c.mode = tail_mode(d, reverse);
    c.acc = acc;
    return c;
}

}  // namespace glowhip

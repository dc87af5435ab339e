// plan_train.hip -- training step of a flow plan: forward that records a TAPE, and the reverse
// sweep that turns dL/dnll into parameter gradients.
//
// Tape (one contiguous caller-provided buffer): the output of every layer, and per FlowStep the coupling network's
// hidden activations h1, h2 (N,hidden,H,W) -- fp16 where the taping k_cnet wrote them (tape_has_masks; the slot keeps its fp32
// size), fp32 from the per-layer kernels -- and its post-scale output hout (N,Cout,H,W); per Split2d the prior
// conv output.  With 288 GB of HBM keeping them (11.6 GB at B=64 for the celeba64 model) is cheaper than the
// reversible-recompute alternative (a second forward through the MFMA-bound coupling nets).
//
// Backward of one FlowStep (reference forward: network/model.py:82-117), all gradients "g_": see backward.hip for the
// element-wise formulas.  Convolution input gradients are convolutions with flipped/transposed weights and reuse the
// forward kernels -- as ONE backward k_cnet launch on the transposed weight images where the tape holds the ReLU sign bits
// (bwd_cnet), layer by layer elsewhere.  Weight gradients are split-K MFMA GEMMs (wgrad_mfma.hip) where wgrad_fast holds: three
// per FlowStep, sharing launches where the shape allows (WgradRoute), their reductions riding in the mixer backward; the direct
// kernel k_wgrad_direct takes the remaining shapes.  The decode VJP (decode_vjp_sweep) walks the same input-gradient chain in
// encode order and has no parameter gradients.
#include "plan_internal.h"
#include "backward.h"

using namespace glowhip;

namespace glowhip {

struct TapeLayer { size_t out = 0, h1 = 0, h2 = 0, hout = 0, m1 = 0, m2 = 0; };   // m1 / m2: sign bits of h1 / h2 (k_cnet MODE 1)

static size_t tape_layout(const glowhip_plan* p, int N, std::vector<TapeLayer>* tl) {
    size_t off = 0;
    if (tl) tl->resize(p->layers.size());
    for (size_t i = 0; i < p->layers.size(); ++i) {
        const LayerPlan& L = p->layers[i];
        const glowhip_layer_desc& d = L.d;
        TapeLayer t;
        const size_t hw = (size_t)d.H * d.W;
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) {
            t.out = take(off, (size_t)N * d.C * hw * 4);
        } else if (d.kind == GLOWHIP_LAYER_FLOWSTEP) {
            t.out = take(off, (size_t)N * d.C * hw * 4);
            t.h1 = take(off, (size_t)N * d.hidden * hw * 4);
            t.h2 = take(off, (size_t)N * d.hidden * hw * 4);
            t.hout = take(off, (size_t)N * L.Cout * hw * 4);
            if (L.cnet) {
                t.m1 = take(off, (size_t)N * d.hidden * hw / 8);
                t.m2 = take(off, (size_t)N * d.hidden * hw / 8);
            }
        } else {
            t.out = take(off, (size_t)N * (d.C / 2) * hw * 4);
            t.hout = take(off, (size_t)N * d.C * hw * 4);
        }
        if (tl) (*tl)[i] = t;
    }
    return align_up(off, 256);
}
// a FlowStep's tape slots as pointers
struct StepTape { float* out; float* h1; float* h2; float* hout; unsigned short* m1; unsigned short* m2; };
static StepTape step_tape(const char* tape, const TapeLayer& t) {
    return StepTape{at<float>(tape, t.out), at<float>(tape, t.h1), at<float>(tape, t.h2), at<float>(tape, t.hout),
                    at<unsigned short>(tape, t.m1), at<unsigned short>(tape, t.m2)};
}

// the buffers of a gradient sweep (training backward and decode VJP): the status / log-det accumulators, the travelling gradient
// (gA / gB), the hidden gradients, f.4's pre-scale gradient, the partial-sum scratch of the taping / backward k_cnet launches, a
// flipped weight
struct GradBufs { unsigned long long* acc; float* gA; float* gB; float* gh1; float* gh2; float* gpre; float* gsh; float* wT; };
// backward workspace: acc u64 (N) | gld (N) | gsum | gA | gB | gh1 | gh2 | gpre | gsh | wT | fp64 accumulators | ...
struct TrainWs : GradBufs {
    float* gld; double* gsum; double* dacc;
    float* col; float* partial;   // shift-expanded small operand / split-K partial tiles of the MFMA weight gradients
    size_t partial_floats;        // floats of ONE of the three split-K partial regions behind `partial`
    GradJob* jobs;                // device copy of the finalize job table (<= 9 per layer)
    LogsJob* ljobs;               // ... and of the log-scale job table (<= 2 per layer)
    float* ludw; LuGradJob* lujobs;   // LU-form layers: the data-term dW of each (C*C floats, in lu_layers order), their gradient job table
};

static size_t max_weight_floats(const glowhip_plan* p) {
    size_t m = 0;
    for (const LayerPlan& L : p->layers) {
        const glowhip_layer_desc& d = L.d;
        if (d.kind == GLOWHIP_LAYER_FLOWSTEP) {
            m = std::max(m, (size_t)d.hidden * (d.C / 2) * 9);
            m = std::max(m, (size_t)d.hidden * d.hidden);
            m = std::max(m, (size_t)L.Cout * d.hidden * 9);
        } else if (d.kind == GLOWHIP_LAYER_SPLIT2D) {
            m = std::max(m, (size_t)d.C * (d.C / 2) * 9);
        }
    }
    return m;
}

// fp64 accumulators of every layer's reduction-type gradients live side by side: zeroed once, converted once
#ifndef GH_MIX_ACC_COPIES
#define GH_MIX_ACC_COPIES 16
#endif
constexpr int MIX_ACC_COPIES = GH_MIX_ACC_COPIES;     // copies of a FlowStep's mixer accumulators [W C*C][an_b C][an_l C] (backward.h ChanMixBwdArgs).
                                       // (64 copies, one per workgroup of the C = 48 launch and plain stores instead of its 154 k fp64
                                       // atomics, changed nothing in that launch -- it was not waiting for them -- and cost the
                                       // finalize kernel 43 us per step for the 4 x longer sums)
// (wide levels, C > 192: one copy per pixel block of k_chanmix_bwd_wide's launch, at most 8 -- 16 copies of C = 384's 1.2 MB were
// 19 MB to zero per FlowStep, 600 MB per sweep of config E's deepest level, nearly all of it never touched by a launch of 8 blocks)
static int mix_acc_copies(const glowhip_layer_desc& d, int N) {
    return chanmix_bwd_wide(d.C) ? chanmix_bwd_wide_copies((long)N * d.H * d.W) : MIX_ACC_COPIES;
}
static size_t layer_acc_doubles(const LayerPlan& L, int N) {
    const glowhip_layer_desc& d = L.d;
    if (d.kind == GLOWHIP_LAYER_FLOWSTEP)
        return mix_acc_copies(d, N) * ((size_t)d.C * d.C + 2 * d.C) + MIX_ACC_COPIES * ((size_t)2 * L.Cout) + 4 * d.hidden;
    if (d.kind == GLOWHIP_LAYER_SPLIT2D) return (size_t)2 * L.Cout;
    return 0;
}
static size_t max_acc_doubles(const glowhip_plan* p, int N) {
    size_t m = 0;
    for (const LayerPlan& L : p->layers) m += layer_acc_doubles(L, N);
    return m + 64;
}

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// the split-half kernels in the training step: off with the plan's own family (glowhip_plan_set_family: GLOWHIP_FAMILY_EXACT_FP32 keeps
// the f16 pipe out of the training step) or the process-wide testing switch
static bool train_sh_enabled(const glowhip_plan* p) { return !debug_switches().exact_fp32 && !(p && p->family == GLOWHIP_FAMILY_EXACT_FP32); }

// Does FlowStep L run its training forward as the product path's two launches -- k_cnet storing h1 / h2 from its epilogues, the
// finishing kernel storing hout and the step output (cnet_sh.hip, TAPE)?  `scratch_floats`: room for the partial sums.
static bool tape_cnet(const glowhip_plan* p, const LayerPlan& L, int N, size_t scratch_floats);
// ... and its input-gradient chain as one backward k_cnet launch?  Needs the taping forward (the sign bits) and all of the
// coupling network's weight gradients requested (the log-scale gradients are derived from them).
// (the shape / tape conditions alone: the chain launch itself needs no weight gradient -- the decode VJP takes it without any)
static bool bwd_cnet_chain(const glowhip_plan* p, const LayerPlan& L, int li, int N, size_t scratch_floats) {
    const glowhip_layer_desc& d = L.d;
    return !debug_switches().train_per_layer_bwd && L.cnet_bwd && tape_cnet(p, L, N, scratch_floats) &&
           li < (int)p->tape_has_masks.size() && p->tape_has_masks[li] &&      // (the forward that filled this tape stored the sign bits)
           cnet_tape_supported(L.Cout, d.H, d.W, d.hidden, d.C / 2, N) &&
           cnet_scratch_floats(N, d.H, d.W, d.C / 2) <= scratch_floats;
}
static bool bwd_cnet(const glowhip_plan* p, const LayerPlan& L, int li, const glowhip_layer_grads& G, int N, size_t scratch_floats) {
    return G.f0_w && G.f2_w && G.f4_w && bwd_cnet_chain(p, L, li, N, scratch_floats);
}
static bool tape_cnet(const glowhip_plan* p, const LayerPlan& L, int N, size_t scratch_floats) {
    const glowhip_layer_desc& d = L.d;
    return !debug_switches().train_per_layer_fwd && train_sh_enabled(p) && d.kind == GLOWHIP_LAYER_FLOWSTEP && L.cnet && d.C <= 96 &&
           cnet_tape_supported(d.C / 2, d.H, d.W, d.hidden, L.Cout, N) && cnet_scratch_floats(N, d.H, d.W, L.Cout) <= scratch_floats;
}

static bool wgrad_fast(const LayerPlan& L) {
    const glowhip_layer_desc& d = L.d;
    return d.kind == GLOWHIP_LAYER_FLOWSTEP && (d.H * d.W) % 32 == 0 && d.hidden % 128 == 0;
}

// padded sizes of a layer's 3x3 weight-gradient GEMMs: rows of f.4's A (Cout x 9 taps), columns of f.0's B (C / 2 x 9 taps)
struct WgradPads { int m4, n0; };
static WgradPads wgrad_pads(const LayerPlan& L) { return WgradPads{round_up(L.Cout * 9, 128), round_up((L.d.C / 2) * 9, 64)}; }

static void wgrad_scratch_floats(const glowhip_plan* p, int N, size_t* col, size_t* partial) {
    *col = 0; *partial = 0;
    for (const LayerPlan& L : p->layers) {
        if (!wgrad_fast(L)) continue;
        const glowhip_layer_desc& d = L.d;
        const int HW = d.H * d.W, hid = d.hidden;
        const auto [m4, n0] = wgrad_pads(L);
        *col = std::max(*col, (size_t)N * std::max(m4, n0) * HW);
        *partial = std::max(*partial, wgrad_mfma_partial_floats(hid, hid, N, HW));
        *partial = std::max(*partial, wgrad_mfma_partial_floats(m4, hid, N, HW));
        *partial = std::max(*partial, wgrad_mfma_partial_floats(hid, n0, N, HW));
    }
}

// gA .. wT, in this order from `off` on; acc lies in front of the caller's own leading fields, at o_acc
static void carve_grad_bufs(const glowhip_plan* p, int N, size_t& off, size_t o_acc, void* base, GradBufs* b) {
    const size_t chw = (size_t)N * p->max_chw * 4, hid = (size_t)N * p->max_hidden * 4;
    const size_t o_gA = take(off, chw), o_gB = take(off, chw), o_h1 = take(off, hid), o_h2 = take(off, hid);
    const size_t o_gpre = take(off, chw), o_gsh = take(off, hid), o_wT = take(off, max_weight_floats(p) * 4);
    if (!b || !base) return;
    b->acc = at<unsigned long long>(base, o_acc); b->gA = at<float>(base, o_gA); b->gB = at<float>(base, o_gB);
    b->gh1 = at<float>(base, o_h1); b->gh2 = at<float>(base, o_h2); b->gpre = at<float>(base, o_gpre);
    b->gsh = at<float>(base, o_gsh); b->wT = at<float>(base, o_wT);
}

static size_t train_ws_layout(const glowhip_plan* p, int N, void* base, TrainWs* w) {
    size_t off = 0;
    const size_t o_acc = take(off, (size_t)N * 8 * (2 + ACC_EXTRA)), o_gld = take(off, (size_t)N * 4), o_gsum = take(off, 64);
    carve_grad_bufs(p, N, off, o_acc, base, w);
    const size_t nd = max_acc_doubles(p, N);
    const size_t o_dacc = take(off, nd * 8);
    size_t colf, partf;
    wgrad_scratch_floats(p, N, &colf, &partf);
    const size_t o_col = take(off, colf * 4), o_part = take(off, 3 * partf * 4);      // three regions: a FlowStep's three GEMMs, reduced together
    const size_t o_jobs = take(off, p->layers.size() * 9 * sizeof(GradJob));
    const size_t o_ljobs = take(off, p->layers.size() * 2 * sizeof(LogsJob));
    size_t ludw_floats = 0;
    for (const LuJob& lj : p->lu_jobs) ludw_floats += (size_t)lj.C * lj.C;
    const size_t o_ludw = take(off, ludw_floats * 4), o_lujobs = take(off, p->lu_jobs.size() * sizeof(LuGradJob));
    if (w && base) {
        w->col = at<float>(base, o_col); w->partial = at<float>(base, o_part); w->partial_floats = partf; w->jobs = at<GradJob>(base, o_jobs); w->ljobs = at<LogsJob>(base, o_ljobs);
        w->gld = at<float>(base, o_gld); w->gsum = at<double>(base, o_gsum); w->dacc = at<double>(base, o_dacc);
        w->ludw = at<float>(base, o_ludw); w->lujobs = at<LuGradJob>(base, o_lujobs);
    }
    return align_up(off, 256);
}

// ---------------------------------------------------------------- forward with tape
static int forward_train(glowhip_plan* p, const void* packed, const float* x, const float* noise, float* z_out, int N,
                         char* tape, const std::vector<TapeLayer>& tl, unsigned long long* acc, float* sh_scratch,
                         hipStream_t s) {
    const float* cur = x;
    const int nl = (int)p->layers.size();
    const size_t scratch_floats = (size_t)N * p->max_hidden;
    bool premixed = false;      // this step's ActNorm + permutation output is already in its tape slot (the previous step's finishing kernel)
    p->tape_has_masks.assign(nl, 0);
    for (int li = 0; li < nl; ++li) {
        const LayerPlan& L = p->layers[li];
        const glowhip_layer_desc& d = L.d;
        p->cur_layer = li;
        float* dst = at<float>(tape, tl[li].out);
        const int HW = d.H * d.W, Ch = d.C / 2, hid = d.hidden;
        const long chw = (long)d.C * HW;
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) {
            GH_TRY(launch_squeeze(cur, noise, dst, N, d.C, d.H, d.W, 2, 0, s));
            noise = nullptr;
        } else if (d.kind == GLOWHIP_LAYER_FLOWSTEP) {
            GH_REQUIRE(noise == nullptr, "forward_train: the dequantisation noise needs a leading Squeeze2d layer");
            const StepTape T = step_tape(tape, tl[li]);
            float* h1 = T.h1; float* h2 = T.h2; float* hout = T.hout;
            if (!premixed) {
                ChanMixArgs m = chanmix_fwd_args(L, packed, N, cur, chw, dst);
                GH_TRY(launch_chanmix(m, s));
            }
            premixed = false;
            if (tape_cnet(p, L, N, scratch_floats)) {
                // the product path's two launches, taping: k_cnet stores h1 / h2, the finishing kernel hout, the step output
                // (y1, z2') in place and -- when the next layer is a FlowStep of the same shape -- that step's mixer output into
                // ITS tape slot
                CnetArgs c = cnet_base(L, packed, N, 0, sh_scratch, acc);
                c.x = dst; c.x_bs = chw; c.z_in = dst; c.z_in_bs = chw;
                c.z_out = dst; c.z_out_bs = chw;
                c.tape_h1 = h1; c.tape_h2 = h2; c.tape_hout = hout;
                c.mask1 = T.m1; c.mask2 = T.m2;
                c.in_scale = SH2_ACT_SCALE; c.out_scale = SH2_ACT_INV;
                if (li + 1 < nl) {
                    const LayerPlan& Ln = p->layers[li + 1];
                    const glowhip_layer_desc& dn = Ln.d;
                    if (dn.kind == GLOWHIP_LAYER_FLOWSTEP && dn.C == d.C && dn.H == d.H && dn.W == d.W) {
                        c.mix = mixer_fwd(Ln, packed);
                        c.z_out = at<float>(tape, tl[li + 1].out);
                        premixed = true;
                    }
                }
                p->tape_has_masks[li] = 1;
                count_launch(p, "k_cnet(tape)");
                {
                    CnetPending pend{};
                    {
                        ScopedTimer t(p, GLOWHIP_K_CNET_TAPE, 1, s);
                        GH_TRY(launch_cnet_main(c, s, &pend));
                    }
                    if (pend.one_wave) count_launch(p, "k_cnet1w(tape)");      // (run-time evidence for the tests: the taping instance of cnet1w_sh.hip took it)
                    ScopedTimer t(p, GLOWHIP_K_CFINISH, 0, s);
                    GH_TRY(launch_cnet_finish(c, pend, s));
                }
                cur = dst;
                continue;
            }
            // f.0 (shapes the taping k_cnet does not take: the exact-fp32 kernels, layer by layer)
            if (L.first_halo) {
                const float* wf = at<float>(packed, L.f0_wt);
                GH_TRY(launch_conv_mfma_first(dst, chw, wf, wf + (size_t)9 * Ch * hid, h1, N, Ch, d.H, d.W, hid, s, 1));
            } else if (L.mfma_first) {
                GH_TRY(launch_conv_mfma_wide(dst, chw, at<float>(packed, L.f0_wt), d.f0_an_bias,
                                             at<float>(packed, L.f0_scale), h1, N, Ch, d.H, d.W, hid, 3, s));
            } else {
                ConvArgs c{dst, chw, d.f0_w, nullptr, d.f0_an_bias, nullptr, at<float>(packed, L.f0_scale), 1, h1,
                           N, Ch, d.H, d.W, hid, 3};
                GH_TRY(launch_conv_direct(c, s));
            }
            // f.2
            if (L.mfma_mid) {
                GH_TRY(launch_conv_mfma_wide(h1, (long)hid * HW, at<float>(packed, L.f2_wt), d.f2_an_bias,
                                             at<float>(packed, L.f2_scale), h2, N, hid, d.H, d.W, hid, 1, s));
            } else {
                ConvArgs c{h1, (long)hid * HW, d.f2_w, nullptr, d.f2_an_bias, nullptr, at<float>(packed, L.f2_scale), 1, h2,
                           N, hid, d.H, d.W, hid, 1};
                GH_TRY(launch_conv_direct(c, s));
            }
            // f.4 + coupling, hout kept
            float* z2 = dst + (long)Ch * HW;
            const int affine = d.coupling == GLOWHIP_COUPLING_AFFINE;
            if (L.mfma_last) {
                TailConvArgs t{};
                t.x = h2; t.x_bs = (long)hid * HW; t.wp = at<float>(packed, L.f4_wp); t.bias = d.f4_bias;
                t.scale = at<float>(packed, L.f4_scale); t.N = N; t.Cin = hid; t.H = d.H; t.W = d.W; t.Cout = L.Cout;
                t.mode = affine ? TAIL_AFFINE_FWD : TAIL_ADD_FWD;
                t.z2_in = z2; t.z2_in_bs = chw; t.z2_out = z2; t.z2_out_bs = chw; t.acc = acc;
                t.zeros = at<float>(packed, 64); t.hout = hout;
                GH_TRY(launch_conv_mfma_tail(t, s));
            } else {
                ConvArgs c{h2, (long)hid * HW, d.f4_w, d.f4_bias, nullptr, nullptr, at<float>(packed, L.f4_scale), 0, hout,
                           N, hid, d.H, d.W, L.Cout, 3};
                GH_TRY(launch_conv_direct(c, s));
                CouplingTailArgs t{hout, z2, chw, z2, chw, N, Ch, HW, affine, 0, acc};
                GH_TRY(launch_coupling_tail(t, s));
            }
        } else {  // SPLIT2D
            float* hout = at<float>(tape, tl[li].hout);
            if (L.mfma_last) {
                TailConvArgs t{};
                t.x = cur; t.x_bs = chw; t.wp = at<float>(packed, L.f4_wp); t.bias = d.f4_bias;
                t.scale = at<float>(packed, L.f4_scale); t.N = N; t.Cin = Ch; t.H = d.H; t.W = d.W; t.Cout = L.Cout;
                t.mode = TAIL_SPLIT_FWD; t.z2_in = cur + (long)Ch * HW; t.z2_in_bs = chw; t.z2_out = nullptr;
                t.z2_out_bs = 0; t.acc = acc; t.zeros = at<float>(packed, 64); t.hout = hout;
                GH_TRY(launch_conv_mfma_tail(t, s));
            } else {
                ConvArgs c{cur, chw, d.f4_w, d.f4_bias, nullptr, nullptr, at<float>(packed, L.f4_scale), 0, hout,
                           N, Ch, d.H, d.W, L.Cout, 3};
                GH_TRY(launch_conv_direct(c, s));
                SplitTailArgs t{hout, cur + (long)Ch * HW, chw, nullptr, nullptr, 0, N, Ch, HW, 0, acc};
                GH_TRY(launch_split_tail(t, s));
            }
            GH_TRY(launch_copy_strided(cur, chw, dst, (long)Ch * HW, N, (long)Ch * HW, s));
        }
        cur = dst;
    }
    const int* o = p->out_shape;
    if (z_out)
        GH_TRY(launch_copy_strided(cur, (long)o[0] * o[1] * o[2], z_out, (long)o[0] * o[1] * o[2], N,
                                   (long)o[0] * o[1] * o[2], s));
    return GLOWHIP_OK;
}

// input gradient of a 'SAME' convolution y = conv(x, w): g_x (+)= conv(g_y, flipT(w)); generic path
static int dgrad_direct(const float* gy, const float* w, float* wT, float* gx, int N, int Cin, int H, int W, int Cout,
                        int ksize, hipStream_t s) {
    GH_TRY(launch_weight_flipT(w, wT, Cout, Cin, ksize, s));
    ConvArgs c{gy, (long)Cout * H * W, wT, nullptr, nullptr, nullptr, nullptr, 0, gx, N, Cout, H, W, Cin, ksize};
    return launch_conv_direct(c, s);
}

__global__ void __launch_bounds__(256) k_add_inplace(float* __restrict__ dst, long dst_bs, const float* __restrict__ src,
                                                     long src_bs, long per) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = blockIdx.y;
    if (i < per) dst[n * dst_bs + i] += src[n * src_bs + i];
}

static int add_rows(float* dst, long dst_bs, const float* src, int N, long per, hipStream_t s) {      // dst[n][:per] += src[n][:per], src dense
    hipLaunchKernelGGL(k_add_inplace, dim3(cdiv(per, 256), N), dim3(256), 0, s, dst, dst_bs, src, per, per);
    GH_LAUNCH_CHECK("k_add_inplace");
    return GLOWHIP_OK;
}
// the 3x3 input gradient added into dst's first Cin channels (batch stride dst_bs) through the dense (N, Cin, H, W) scratch `tmp`
static int dgrad_direct_add(const float* gy, const float* w, float* wT, float* tmp, float* dst, long dst_bs, int N, int Cin, int H,
                            int W, int Cout, hipStream_t s) {
    GH_TRY(dgrad_direct(gy, w, wT, tmp, N, Cin, H, W, Cout, 3, s));
    return add_rows(dst, dst_bs, tmp, N, (long)Cin * H * W, s);
}

// ---------------------------------------------------------------- a FlowStep's input-gradient chain, shared by the two sweeps
// As ONE k_cnet launch (MODE 2, cnet_sh.hip) on the transposed weight images, the ReLU masks from the tape's sign bits:
// g_pre -> g_u2 (gh2) -> g_u0 (gh1) -> the partial sums of d y1, described by *pend; their gathering rides in the caller's next
// mixer kernel.  The gradients enter times grad_scale; g_u2 / g_u0 are stored times grad_scale * 2^11 (what the weight-gradient
// GEMMs split with two instructions per value).
static int launch_cnet_bwd(glowhip_plan* p, const LayerPlan& L, const void* packed, int N, const StepTape& T, const GradBufs& b,
                           float grad_scale, CnetPending* pend, hipStream_t s) {
    const glowhip_layer_desc& d = L.d;
    const long gpre_bs = (long)L.Cout * d.H * d.W;
    CnetArgs c{};
    c.w0 = at<char>(packed, L.cb_w0); c.w2 = at<char>(packed, L.cb_w2); c.w4 = at<char>(packed, L.cb_w4);
    c.N = N; c.Cin = L.Cout; c.H = d.H; c.W = d.W; c.hidden = d.hidden; c.Cout = d.C / 2;
    c.scratch = b.gsh; c.mode = TAIL_ADD_FWD;
    c.x = b.gpre; c.x_bs = gpre_bs; c.z_in = b.gpre; c.z_in_bs = gpre_bs;
    c.tape_h1 = b.gh2; c.tape_h2 = b.gh1;
    c.mask1 = T.m1; c.mask2 = T.m2;
    c.in_scale = SH2_ACT_SCALE * grad_scale; c.out_scale = SH2_ACT_INV * SH_LO_SCALE; c.bwd = 1;
    *pend = CnetPending{};
    count_launch(p, "k_cnet(bwd)");
    {
        ScopedTimer t(p, GLOWHIP_K_CNET_BWD, 1, s);
        GH_TRY(launch_cnet_main(c, s, pend));
    }
    if (pend->one_wave) count_launch(p, "k_cnet1w(bwd)");      // (run-time evidence for the tests: the backward instance of cnet1w_sh.hip took it)
    return GLOWHIP_OK;
}
// Layer by layer: each helper holds its convolution's route.  The activation backward between them (and, in training, the weight
// gradients) is the caller's.
// The per-layer kernels read fp32: a tape written by the taping k_cnet holds h1 / h2 as fp16 -- converted into the partial-sum
// scratch (unused on this path), h2 first, h1 once h2 has been consumed.
static int tape_to_f32(const float*& h, bool half_tape, const LayerPlan& L, int N, const GradBufs& b, hipStream_t s) {
    if (!half_tape) return GLOWHIP_OK;
    GH_TRY(launch_half_to_float(h, b.gsh, N, L.d.hidden, L.d.H * L.d.W, s));
    h = b.gsh;
    return GLOWHIP_OK;
}
static int dgrad_f4(const LayerPlan& L, const void* packed, int N, const GradBufs& b, hipStream_t s) {      // gpre -> gh2 (raw)
    const glowhip_layer_desc& d = L.d;
    if (!L.dg4_first) return dgrad_direct(b.gpre, d.f4_w, b.wT, b.gh2, N, d.hidden, d.H, d.W, L.Cout, 3, s);
    const float* wf = at<float>(packed, L.f4T_wf);
    return launch_conv_mfma_first(b.gpre, (long)L.Cout * d.H * d.W, wf, wf + (size_t)9 * L.Cout * d.hidden, b.gh2, N, L.Cout, d.H, d.W,
                                  d.hidden, s, 0);
}
static int dgrad_f2(const LayerPlan& L, int N, const GradBufs& b, hipStream_t s) {      // gh2 -> gh1 (raw)
    const glowhip_layer_desc& d = L.d;
    if (!L.mfma_mid) return dgrad_direct(b.gh2, d.f2_w, b.wT, b.gh1, N, d.hidden, d.H, d.W, d.hidden, 1, s);
    // W2 in its reference layout [o][i] is already the K-major image of the transposed GEMM
    return launch_conv_mfma_wide(b.gh2, (long)d.hidden * d.H * d.W, d.f2_w, nullptr, nullptr, b.gh1, N, d.hidden, d.H, d.W, d.hidden, 1, s, 0);
}
static int dgrad_f0_add(const LayerPlan& L, const void* packed, int N, const GradBufs& b, float* g, hipStream_t s) {      // g's y1 half += f.0^T gh1
    const glowhip_layer_desc& d = L.d;
    const int Ch = d.C / 2, HW = d.H * d.W;
    const long chw = (long)d.C * HW;
    if (!L.dg0_tail) return dgrad_direct_add(b.gh1, d.f0_w, b.wT, b.gpre, g, chw, N, Ch, d.H, d.W, d.hidden, s);   // gpre reused: (N,Ch,HW)
    TailConvArgs t{};      // fused: the tail kernel's additive-coupling epilogue
    t.x = b.gh1; t.x_bs = (long)d.hidden * HW; t.wp = at<float>(packed, L.f0T_wp); t.bias = nullptr; t.scale = nullptr;
    t.N = N; t.Cin = d.hidden; t.H = d.H; t.W = d.W; t.Cout = Ch; t.mode = TAIL_ADD_FWD;
    t.z2_in = g; t.z2_in_bs = chw; t.z2_out = g; t.z2_out_bs = chw; t.acc = nullptr;
    t.zeros = at<float>(packed, 64); t.hout = nullptr;
    return launch_conv_mfma_tail(t, s);
}

static int zero_f64(double* p, size_t n, hipStream_t s) {
    if (hipMemsetAsync(p, 0, n * sizeof(double), s) != hipSuccess) {
        set_error("backward: hipMemsetAsync failed");
        return GLOWHIP_ELAUNCH;
    }
    return GLOWHIP_OK;
}

// ---------------------------------------------------------------- backward sweep
// a FlowStep's fp64 accumulators (layer_acc_doubles): mcopies x [W C*C][an_b C][an_l C] | [f0_b hid][f0_l hid][f2_b hid][f2_l hid] |
// MIX_ACC_COPIES x [f4_b Cout][f4_l Cout]
struct StepAcc { double* W; double* Ab; double* Al; double* b0; double* l0; double* b2; double* l2; double* b4; double* l4; int mcopies; long mstride; };
static StepAcc step_acc(double* base, const LayerPlan& L, int N) {
    const glowhip_layer_desc& d = L.d;
    const int hid = d.hidden;
    StepAcc a{};
    a.mcopies = mix_acc_copies(d, N); a.mstride = (long)d.C * d.C + 2 * d.C;       // (one copy of the mixer accumulators)
    a.W = base; a.Ab = a.W + (size_t)d.C * d.C; a.Al = a.Ab + d.C;
    a.b0 = a.W + a.mcopies * a.mstride; a.l0 = a.b0 + hid; a.b2 = a.l0 + hid; a.l2 = a.b2 + hid; a.b4 = a.l2 + hid; a.l4 = a.b4 + L.Cout;
    return a;
}
// the step's mixer backward, gy -> gx (the k_cnet branch adds add_*)
static ChanMixBwdArgs chanmix_bwd_args(const LayerPlan& L, const void* packed, int N, const float* xin, const float* gy, float* gx,
                                       const StepAcc& A) {
    const glowhip_layer_desc& d = L.d;
    const long chw = (long)d.C * d.H * d.W;
    ChanMixBwdArgs mb{xin, chw, gy, gx, chw, d.an_bias, at<float>(packed, L.an_scale),
                      d.permutation == GLOWHIP_PERM_INVCONV ? d.invconv_w : nullptr,
                      d.permutation == GLOWHIP_PERM_GATHER ? d.perm_idx_inv : nullptr, A.W, A.Ab, A.Al, N, d.C, d.H * d.W};
    mb.acc_copies = A.mcopies; mb.acc_stride = A.mstride;
    return mb;
}
// How the three weight-gradient GEMMs of a step behind a backward k_cnet launch are launched.  trio: one launch.  pair: f.4's and
// f.0's in one launch, f.2's alone.  taps: three launches, the 3x3 layers' shift-expanded operands gathered by the GEMM's loader
// (WgradTaps: power-of-two widths).  expanded: three launches on operands written out by launch_shift_expand.
enum class WgradRoute { trio, pair, taps, expanded };
static WgradRoute wgrad_route(const LayerPlan& L, int N) {
    const glowhip_layer_desc& d = L.d;
    const int HW = d.H * d.W;
    const auto [m4, n0] = wgrad_pads(L);
    if (d.W < 4 || (d.W & (d.W - 1)) != 0) return WgradRoute::expanded;
    if (!wgrad_pair_ok(HW, m4, d.hidden, n0)) return WgradRoute::taps;
    // short pixel axes (<= 512 k-tiles of 32 pixels): f.2's GEMM joins the launch as well -- at 12 - 18 pixel slices instead of 32
    // its workgroups' loops are two to three times as long and a third of the partial tiles is left
    return (long)N * HW / 32 <= 512 ? WgradRoute::trio : WgradRoute::pair;
}

// The three weight-gradient GEMMs of FlowStep L behind its backward k_cnet launch, in launch_wgrad_group's order (f.4, f.0, f.2),
// on the operands that launch and the tape hand over; their partial tiles in the three regions behind w.partial.
//   dW4[o][i][tap] = sum_p g_pre[o][p - d(tap)] * h2[i][p]        dW0[o][i][tap] = sum_p g_u0[o][p] * y1[i][p + d(tap)]
// The 3x3 layers' shift-expanded operands are gathered by the GEMM's loader (WgradTaps); the bias gradients are row sums of g_u.
static void cnet_wgrad_gemms(const LayerPlan& L, const glowhip_layer_grads& G, const StepTape& T, const StepAcc& A, const TrainWs& w,
                             WgradGemm g[3]) {
    const glowhip_layer_desc& d = L.d;
    const int HW = d.H * d.W, Ch = d.C / 2, hid = d.hidden;
    const long hb = (long)hid * HW;
    const auto [m4, n0] = wgrad_pads(L);
    g[0] = WgradGemm{w.gpre, (long)L.Cout * HW, T.h2, hb, w.partial, G.f4_w, m4, hid, L.Cout * 9, hid, 1};
    g[0].taps = WgradTaps{0, L.Cout, d.H, d.W, -1}; g[0].b_half = 1; g[0].layout = WGRAD_B_TILED;
    g[1] = WgradGemm{w.gh1, hb, T.out, (long)d.C * HW, w.partial + 2 * w.partial_floats, G.f0_w, hid, n0, hid, Ch * 9, 0};
    g[1].taps = WgradTaps{1, Ch, d.H, d.W, +1}; g[1].rowsum = A.b0; g[1].layout = WGRAD_A_TILED | WGRAD_A_PRESCALED;
    g[2] = WgradGemm{w.gh2, hb, T.h1, hb, w.partial + w.partial_floats, G.f2_w, hid, hid, hid, hid, 0};
    g[2].rowsum = A.b2; g[2].b_half = 1; g[2].layout = WGRAD_A_TILED | WGRAD_B_TILED | WGRAD_A_PRESCALED;
}
// the gathered operand of g written out by launch_shift_expand into `col`, g a GEMM on that plain operand
static int expand_taps(WgradGemm& g, float* col, int N, int HW, hipStream_t s) {
    const WgradTaps t = g.taps;
    const bool a = t.operand == 0;
    const int rows = a ? g.Mpad : g.Npad;
    GH_TRY(launch_shift_expand(a ? g.A : g.B, a ? g.a_bs : g.b_bs, col, N, t.C, t.H, t.W, rows, t.sign, s));
    (a ? g.A : g.B) = col; (a ? g.a_bs : g.b_bs) = (long)rows * HW; g.taps.operand = -1;
    return GLOWHIP_OK;
}

static int backward_sweep(glowhip_plan* p, const void* packed, const float* x_in, const char* tape,
                          const std::vector<TapeLayer>& tl, const glowhip_layer_grads* grads, float* grad_x, int N,
                          TrainWs& w, float* g_top, hipStream_t s) {
    // g: gradient w.r.t. the current layer's OUTPUT (contiguous (N, C_out, H, W)), held in gA/gB
    float* g = g_top;
    // power-of-two pre-scale of the gradients that travel as fp16 pairs (backward k_cnet, weight-gradient GEMMs): 2^round(log2(B ln2 CHW)), the inverse
    // of dL/d(objective) for loss = mean(nll) (network/model.py:448-450, 496-506)
    const float sh_grad_scale = exp2f(rintf(log2f((float)N * 0.6931472f * (float)p->in_shape[0] * p->in_shape[1] * p->in_shape[2])));
    const int nl = (int)p->layers.size();
    std::vector<GradJob>& jobs = p->grad_jobs;
    jobs.clear();
    p->logs_jobs.clear();
    std::vector<size_t> acc_base(nl, 0);
    {
        size_t o = 0;
        for (int i = 0; i < nl; ++i) { acc_base[i] = o; o += layer_acc_doubles(p->layers[i], N); }
        GH_TRY(zero_f64(w.dacc, o, s));
    }
    auto fin = [&](const double* acc, float* out, int n, double add_mul, const float* winv = nullptr, int C = 0, int copies = 1,
                   long stride = 0) {
        if (out) jobs.push_back(GradJob{acc, out, n, add_mul, winv, C, copies, stride});
    };
    // the mixer's weight gradient.  Dense layer: dW + G HW W^-T (the log-det term).  LU-form layer: the data term alone into the
    // layer's scratch -- no W^-1 term: its log-det term goes to dlog_s directly, in the gradient kernel launched behind the finalize
    p->lu_grad_jobs.clear();
    auto fin_w = [&](int li, const LayerPlan& L, const glowhip_layer_grads& G, const double* aW, int HW, int mcopies, long mstride) {
        const glowhip_layer_desc& d = L.d;
        size_t so = 0;
        for (size_t q = 0; q < p->lu_layers.size(); ++q) {
            const LuJob& lj = p->lu_jobs[q];
            if (p->lu_layers[q].layer == li) {
                const glowhip_invconv_lu_grads& g = p->lu_layers[q].g;
                if (!g.dl) return;
                fin(aW, w.ludw + so, d.C * d.C, 0.0, nullptr, 0, mcopies, mstride);
                p->lu_grad_jobs.push_back(LuGradJob{lj.perm, lj.l, lj.u, lj.log_s, lj.sign_s, w.ludw + so, g.dl, g.du, g.dlog_s, d.C, w.gsum, (double)HW});
                return;
            }
            so += (size_t)lj.C * lj.C;
        }
        fin(aW, G.invconv_w, d.C * d.C, (double)HW, at<float>(packed, L.winv), d.C, mcopies, mstride);
    };
    // a FlowStep's reduction-type gradients.  The log-scale gradients of f.0 / f.2 come from their accumulators, or -- logs_from_dw:
    // the chain ran as one k_cnet launch, nothing filled them -- from dW and db (backward.h LogsJob)
    auto fin_step = [&](int li, const LayerPlan& L, const glowhip_layer_grads& G, const StepAcc& A, bool logs_from_dw) {
        const glowhip_layer_desc& d = L.d;
        const int HW = d.H * d.W, hid = d.hidden;
        if (logs_from_dw && G.f2_an_logs) p->logs_jobs.push_back(LogsJob{d.f2_w, G.f2_w, d.f2_an_bias, A.b2, G.f2_an_logs, hid, hid});
        if (logs_from_dw && G.f0_an_logs) p->logs_jobs.push_back(LogsJob{d.f0_w, G.f0_w, d.f0_an_bias, A.b0, G.f0_an_logs, hid, (d.C / 2) * 9});
        if (d.permutation == GLOWHIP_PERM_INVCONV) fin_w(li, L, G, A.W, HW, A.mcopies, A.mstride);
        fin(A.Ab, G.an_bias, d.C, 0.0, nullptr, 0, A.mcopies, A.mstride);
        fin(A.Al, G.an_logs, d.C, 3.0 * HW, nullptr, 0, A.mcopies, A.mstride);
        fin(A.b0, G.f0_an_bias, hid, 0.0); if (!logs_from_dw) fin(A.l0, G.f0_an_logs, hid, 0.0);
        fin(A.b2, G.f2_an_bias, hid, 0.0); if (!logs_from_dw) fin(A.l2, G.f2_an_logs, hid, 0.0);
        fin(A.b4, G.f4_bias, L.Cout, 0.0, nullptr, 0, MIX_ACC_COPIES, 2 * L.Cout); fin(A.l4, G.f4_logs, L.Cout, 0.0, nullptr, 0, MIX_ACC_COPIES, 2 * L.Cout);
    };
    // log-scale gradients of the layers whose input-gradient chain ran as one k_cnet launch: d logs = 3 (<W, dW> + b db) READS the
    // weight gradients, which live in the per-level buckets a data-parallel run all-reduces (in place, on a side stream) as soon as
    // the level's mark has passed.  So the pending jobs are launched BEFORE a mark is recorded (computed after the sweep
    // they could see dW half reduced or summed but not yet averaged); without marks (one GPU) they run as one launch at the end.
    p->logs_jobs.reserve((size_t)nl * 2);      // (the host table is the source of asynchronous copies: it must not move)
    size_t logs_done = 0;
    auto flush_logs = [&]() {
        const size_t n = p->logs_jobs.size() - logs_done;
        if (n == 0) return GLOWHIP_OK;
        if (hipMemcpyAsync(w.ljobs + logs_done, p->logs_jobs.data() + logs_done, n * sizeof(LogsJob), hipMemcpyHostToDevice, s) != hipSuccess) {
            set_error("backward: hipMemcpyAsync of the log-scale job table failed");
            return GLOWHIP_ELAUNCH;
        }
        GH_TRY(launch_logs_from_dw_batched(w.ljobs + logs_done, (int)n, s));
        logs_done = p->logs_jobs.size();
        return GLOWHIP_OK;
    };
    size_t mark_i = 0;      // gradient-ready marks (glowhip_plan_backward_marks), in sweep order
    auto marks_down_to = [&](int li) {
        while (mark_i < p->bwd_marks.size() && p->bwd_marks[mark_i].first >= li) {
            GH_TRY(flush_logs());
            if (hipEventRecord(p->bwd_marks[mark_i].second, s) != hipSuccess) { set_error("backward: hipEventRecord of a mark failed"); return GLOWHIP_ELAUNCH; }
            ++mark_i;
        }
        return GLOWHIP_OK;
    };
    for (int li = nl - 1; li >= 0; --li) {
        GH_TRY(marks_down_to(li + 1));      // every layer above li has been swept
        p->cur_layer = li;
        const LayerPlan& L = p->layers[li];
        const glowhip_layer_desc& d = L.d;
        const glowhip_layer_grads& G = grads[li];
        const float* xin = li > 0 ? at<float>(tape, tl[li - 1].out) : x_in;   // this layer's input
        float* gnext = (g == w.gA) ? w.gB : w.gA;
        const int HW = d.H * d.W, Ch = d.C / 2, hid = d.hidden;
        const long chw = (long)d.C * HW;
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) {
            if (li == 0 && grad_x == nullptr) break;      // nobody wants dL/dx
            float* dst = li == 0 ? grad_x : gnext;
            GH_TRY(launch_squeeze(g, nullptr, dst, N, d.C * 4, d.H / 2, d.W / 2, 2, 1, s));
            g = dst;
        } else if (d.kind == GLOWHIP_LAYER_FLOWSTEP) {
            const StepTape T = step_tape(tape, tl[li]);
            const float* out = T.out; const float* h1 = T.h1; const float* h2 = T.h2;
            const int affine = d.coupling == GLOWHIP_COUPLING_AFFINE;
            const StepAcc A = step_acc(w.dacc + acc_base[li], L, N);
            // (a) coupling tail: g (second half) becomes g_y2 in place; gpre = gradient of f.4's (conv + bias)
            CouplingBwdArgs cb{T.hout, out + (long)Ch * HW, chw, g + (long)Ch * HW, chw, g + (long)Ch * HW, w.gpre,
                               at<float>(packed, L.f4_scale), w.gld, A.b4, A.l4, N, Ch, L.Cout, HW, affine};
            cb.acc_copies = MIX_ACC_COPIES; cb.acc_stride = 2 * L.Cout;
            GH_TRY(launch_coupling_bwd(cb, s));
            // (b) f.4: weight gradient, then input gradient -> g_h2 (raw), then ReLU/ActNorm of f.2
            const bool fastw = wgrad_fast(L);
            if (fastw && bwd_cnet(p, L, li, G, N, (size_t)N * p->max_hidden)) {
                // The input-gradient chain as ONE k_cnet launch (launch_cnet_bwd); the bias gradients are row sums inside the
                // weight-gradient GEMMs that read g_u2 / g_u0 anyway, the log-scale gradients follow from dW and db (backward.h LogsJob).
                const WgradRoute route = wgrad_route(L, N);
                const WgradBatch wb{N, HW, sh_grad_scale};
                WgradGemm gm[3];           // f.4's, f.0's, f.2's
                cnet_wgrad_gemms(L, G, T, A, w, gm);
                WgradReduceJobs rj{};      // the three split-K reductions of this step run as one launch at its end, in the order f.4, f.2, f.0
                rj.n = 3;
                WgradReduceJob* const defer[3] = {&rj.job[0], &rj.job[2], &rj.job[1]};
                auto wgrad_alone = [&](int i) {      // GEMM i in a launch of its own; `expanded`: its gathered operand written out first
                    WgradGemm q = gm[i];
                    if (route == WgradRoute::expanded && q.taps.operand >= 0) GH_TRY(expand_taps(q, w.col, N, HW, s));
                    ScopedTimer tw(p, GLOWHIP_K_WGRAD, 1, s);
                    return launch_wgrad_mfma(q, wb, s, defer[i]);
                };
                // f.4's GEMM does not depend on the chain below, but where it shares a launch with f.0's (and f.2's), which do, it
                // waits for it; alone it runs here
                if (route == WgradRoute::taps || route == WgradRoute::expanded) GH_TRY(wgrad_alone(0));
                CnetPending pend{};
                GH_TRY(launch_cnet_bwd(p, L, packed, N, T, w, sh_grad_scale, &pend, s));
                // (its finishing step -- g_y1 += the partial sums -- rides in k_chanmix_bwd below)
                if (route == WgradRoute::trio) {      // all three GEMMs side by side in one launch
                    count_launch(p, "k_wgrad(trio)");
                    ScopedTimer tw(p, GLOWHIP_K_WGRAD, 1, s);
                    GH_TRY(launch_wgrad_group(gm, 3, wb, defer, s));
                } else {
                    GH_TRY(wgrad_alone(2));
                    if (route == WgradRoute::pair) {      // f.2's alone, then f.4's and f.0's in one launch
                        count_launch(p, "k_wgrad(pair)");
                        ScopedTimer tw(p, GLOWHIP_K_WGRAD, 1, s);
                        GH_TRY(launch_wgrad_group(gm, 2, wb, defer, s));
                    } else {
                        GH_TRY(wgrad_alone(1));
                    }
                }
                // (the three reductions ride in the mixer backward's launch below: k_chanmix_bwd_reduce)
                ChanMixBwdArgs mb = chanmix_bwd_args(L, packed, N, xin, g, g, A);      // (C <= 96 here, tape_cnet: never the wide kernel)
                mb.add_part = pend.scratch; mb.add_scale = 1.0f / sh_grad_scale; mb.add_C = Ch; mb.add_MS = pend.MS;
                mb.add_tiles = pend.tiles; mb.add_R = pend.R; mb.add_NI = pend.NI; mb.add_lpxt = pend.lpxt; mb.add_H = d.H; mb.add_W = d.W;
                GH_TRY(launch_chanmix_bwd(mb, s, &rj));
                fin_step(li, L, G, A, true);
                continue;
            }
            const bool half_tape = li < (int)p->tape_has_masks.size() && p->tape_has_masks[li];
            const WgradBatch wb{N, HW, train_sh_enabled(p) ? sh_grad_scale : 0.f};      // (0: the fp32 pipe)
            const WgradPads pad = wgrad_pads(L);
            const long hb = (long)hid * HW;
            GH_TRY(tape_to_f32(h2, half_tape, L, N, w, s));
            if (fastw) {   // dW4[o][i][tap] = sum_p g_pre[o][p - d(tap)] * h2[i][p]
                GH_TRY(launch_shift_expand(w.gpre, (long)L.Cout * HW, w.col, N, L.Cout, d.H, d.W, pad.m4, -1, s));
                GH_TRY(launch_wgrad_mfma(WgradGemm{w.col, (long)pad.m4 * HW, h2, hb, w.partial, G.f4_w, pad.m4, hid, L.Cout * 9, hid, 1}, wb, s));
            } else {
                GH_TRY(launch_wgrad_direct(w.gpre, h2, hb, G.f4_w, N, hid, d.H, d.W, L.Cout, 3, s));
            }
            GH_TRY(dgrad_f4(L, packed, N, w, s));
            GH_TRY(launch_act_bwd(w.gh2, h2, at<float>(packed, L.f2_scale), N, hid, HW, A.b2, A.l2, s));
            GH_TRY(tape_to_f32(h1, half_tape, L, N, w, s));
            // (c) f.2 (1x1)
            if (fastw) {
                GH_TRY(launch_wgrad_mfma(WgradGemm{w.gh2, hb, h1, hb, w.partial, G.f2_w, hid, hid, hid, hid, 0}, wb, s));
            } else {
                GH_TRY(launch_wgrad_direct(w.gh2, h1, hb, G.f2_w, N, hid, d.H, d.W, hid, 1, s));
            }
            GH_TRY(dgrad_f2(L, N, w, s));
            GH_TRY(launch_act_bwd(w.gh1, h1, at<float>(packed, L.f0_scale), N, hid, HW, A.b0, A.l0, s));
            // (d) f.0: input is y1 = first half of the step output
            if (fastw) {   // dW0[o][i][tap] = sum_p g_u0[o][p] * y1[i][p + d(tap)]
                GH_TRY(launch_shift_expand(out, chw, w.col, N, Ch, d.H, d.W, pad.n0, +1, s));
                GH_TRY(launch_wgrad_mfma(WgradGemm{w.gh1, hb, w.col, (long)pad.n0 * HW, w.partial, G.f0_w, hid, pad.n0, hid, Ch * 9, 0}, wb, s));
            } else {
                GH_TRY(launch_wgrad_direct(w.gh1, out, chw, G.f0_w, N, Ch, d.H, d.W, hid, 3, s));
            }
            GH_TRY(dgrad_f0_add(L, packed, N, w, g, s));
            // (e) ActNorm + invconv / permutation: g (= g_y) -> g_x in place; wide levels (channel slices in separate workgroups, which
            // all read g_y) into the other gradient buffer
            const bool wide = chanmix_bwd_wide(d.C);
            const ChanMixBwdArgs mb = chanmix_bwd_args(L, packed, N, xin, g, wide ? gnext : g, A);
            if (wide) count_launch(p, "k_chanmix_bwd_wide");
            GH_TRY(launch_chanmix_bwd(mb, s));
            if (wide) g = gnext;
            // (f) fp64 accumulators -> fp32 gradients (+ the log-det terms that do not depend on the data): queued,
            // converted by ONE launch after the sweep
            fin_step(li, L, G, A, false);
        } else {  // SPLIT2D: output z1 (N,Ch,HW); input x = (z1, z2)
            const float* hout = at<float>(tape, tl[li].hout);
            double* a4b = w.dacc + acc_base[li]; double* a4l = a4b + L.Cout;
            // g_x first half <- g (gradient of z1), second half <- gradient of the log-density
            GH_TRY(launch_copy_strided(g, (long)Ch * HW, gnext, chw, N, (long)Ch * HW, s));
            SplitBwdArgs sb{hout, xin + (long)Ch * HW, chw, gnext + (long)Ch * HW, chw, w.gpre,
                            at<float>(packed, L.f4_scale), w.gld, a4b, a4l, N, Ch, HW};
            GH_TRY(launch_split_bwd(sb, s));
            {   // Conv2dZeros weight gradient: the split-K GEMM of the FlowSteps (A = gathered taps of g_pre, B = z1's Ch rows)
                const int m4 = wgrad_pads(L).m4;
                const bool mf = train_sh_enabled(p) && G.f4_w && HW % 32 == 0 && Ch <= 64 && d.W >= 4 && (d.W & (d.W - 1)) == 0 &&
                                wgrad_mfma_partial_floats(m4, 64, N, HW) <= w.partial_floats;
                if (mf) {
                    WgradGemm q{w.gpre, (long)L.Cout * HW, xin, chw, w.partial, G.f4_w, m4, 64, L.Cout * 9, Ch, 1};
                    q.taps = WgradTaps{0, L.Cout, d.H, d.W, -1}; q.b_valid = Ch;
                    GH_TRY(launch_wgrad_mfma(q, WgradBatch{N, HW, sh_grad_scale}, s));
                } else {
                    GH_TRY(launch_wgrad_direct(w.gpre, xin, chw, G.f4_w, N, Ch, d.H, d.W, L.Cout, 3, s));
                }
            }
            GH_TRY(dgrad_direct_add(w.gpre, d.f4_w, w.wT, w.gh1, gnext, chw, N, Ch, d.H, d.W, L.Cout, s));
            fin(a4b, G.f4_bias, L.Cout, 0.0); fin(a4l, G.f4_logs, L.Cout, 0.0);
            g = gnext;
        }
    }
    GH_TRY(marks_down_to(0));
    if (!jobs.empty()) {
        if (hipMemcpyAsync(w.jobs, jobs.data(), jobs.size() * sizeof(GradJob), hipMemcpyHostToDevice, s) != hipSuccess) {
            set_error("backward: hipMemcpyAsync of the finalize job table failed");
            return GLOWHIP_ELAUNCH;
        }
        GH_TRY(launch_grad_finalize_batched(w.jobs, (int)jobs.size(), w.gsum, s));
    }
    if (!p->lu_grad_jobs.empty()) {      // dl, du, dlog_s of every LU-form layer from the dW just written: one launch per sweep
        if (hipMemcpyAsync(w.lujobs, p->lu_grad_jobs.data(), p->lu_grad_jobs.size() * sizeof(LuGradJob), hipMemcpyHostToDevice, s) != hipSuccess) {
            set_error("backward: hipMemcpyAsync of the LU gradient job table failed");
            return GLOWHIP_ELAUNCH;
        }
        count_launch(p, "k_invconv_lu_backward");
        GH_TRY(launch_invconv_lu_backward(w.lujobs, nullptr, (int)p->lu_grad_jobs.size(), p->lu_max_c, s));
    }
    GH_TRY(flush_logs());
    return GLOWHIP_OK;
}

// ---------------------------------------------------------------- decode VJP (glowhip_plan_decode_vjp)
// workspace: acc u64 | norm words (2 N) | gA | gB | gh1 | gh2 | gpre | gsh | wT -- no accumulators of any kind
struct VjpWs : GradBufs { float* words; };
static size_t vjp_ws_layout(const glowhip_plan* p, int N, void* base, VjpWs* w) {
    size_t off = 0;
    const size_t o_acc = take(off, (size_t)N * 8 * (2 + ACC_EXTRA)), o_words = take(off, (size_t)N * 2 * 4);
    carve_grad_bufs(p, N, off, o_acc, base, w);
    if (w && base) w->words = at<float>(base, o_words);
    return align_up(off, 256);
}

// The sweep: ENCODE order, layer 0 first -- the reverse of the decode.  g: the gradient with respect to the current layer's
// encode-side INPUT, contiguous (N, C, H, W) in gA / gB and normalised per sample (words); every layer turns it into the gradient
// with respect to its encode-side output.  FlowStep: mixer^-1 VJP, coupling-tail^-1 VJP, then g_y1 += f'(y1)^T g_pre -- the training
// sweep's input-gradient chain, one backward k_cnet launch where the tape has the sign bits (its partial sums are gathered by the
// NEXT layer's first kernel), per layer elsewhere.
static int decode_vjp_sweep(glowhip_plan* p, const void* packed, const float* x_in, const char* tape, const std::vector<TapeLayer>& tl,
                            float* grad_z, float* const* grad_eps, int N, VjpWs& w, hipStream_t s) {
    const int nl = (int)p->layers.size();
    float* g = w.gA;
    bool pending = false;      // g's first pend_C channels still lack the partial sums in pend
    CnetPending pend{};
    int pend_C = 0, pend_H = 0, pend_W = 0;
    auto add_args = [&](ChanMixInvBwdArgs& m) {
        m.add_part = pend.scratch; m.add_scale = 1.0f; m.add_C = pend_C; m.add_MS = pend.MS; m.add_tiles = pend.tiles; m.add_R = pend.R;
        m.add_NI = pend.NI; m.add_lpxt = pend.lpxt; m.add_H = pend_H; m.add_W = pend_W;
    };
    auto finish_pending = [&](long g_bs) {
        if (!pending) return GLOWHIP_OK;
        ChanMixInvBwdArgs m{};
        m.gx = g; m.gu = g; m.g_bs = g_bs; m.N = N; m.C = 2 * pend_C; m.HW = pend_H * pend_W;
        add_args(m);
        pending = false;
        count_launch(p, "k_cpart_finish");
        return launch_cpart_finish(m, s);
    };
    for (int li = 0; li < nl; ++li) {
        p->cur_layer = li;
        const LayerPlan& L = p->layers[li];
        const glowhip_layer_desc& d = L.d;
        const float* xin = li > 0 ? at<float>(tape, tl[li - 1].out) : x_in;   // this layer's encode-side input
        float* gnext = (g == w.gA) ? w.gB : w.gA;
        const int HW = d.H * d.W, Ch = d.C / 2, hid = d.hidden;
        const long chw = (long)d.C * HW;
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) {
            GH_TRY(finish_pending(chw));
            GH_TRY(launch_squeeze(g, nullptr, gnext, N, d.C, d.H, d.W, 2, 0, s));
            g = gnext;
        } else if (d.kind == GLOWHIP_LAYER_FLOWSTEP) {
            const StepTape T = step_tape(tape, tl[li]);
            const float* h1 = T.h1; const float* h2 = T.h2;
            const int affine = d.coupling == GLOWHIP_COUPLING_AFFINE;
            // (a) mixer^-1: g (= g_x) -> g_u = (g_y1 without the coupling network's term, g_y2), into the other buffer
            ChanMixInvBwdArgs mb{};
            mb.gx = g; mb.gu = gnext; mb.g_bs = chw; mb.inv_scale = at<float>(packed, L.an_inv_scale);
            mb.matrix = d.permutation == GLOWHIP_PERM_INVCONV ? at<float>(packed, L.winv) : nullptr;
            mb.gather = d.permutation == GLOWHIP_PERM_GATHER ? d.perm_idx : nullptr;
            mb.N = N; mb.C = d.C; mb.HW = HW;
            if (pending) {
                if (chanmix_bwd_wide(d.C) || pend_C != Ch || pend_H != d.H || pend_W != d.W) GH_TRY(finish_pending(chw));
                else { add_args(mb); pending = false; }
            }
            count_launch(p, chanmix_bwd_wide(d.C) ? "k_chanmix_inv_bwd_wide" : "k_chanmix_inv_bwd");
            GH_TRY(launch_chanmix_inv_bwd(mb, s));
            g = gnext;
            // (b) coupling tail^-1: g's second half g_y2 -> g_z2' in place; gpre = gradient of f.4's (conv + bias)
            CouplingInvBwdArgs cb{T.hout, T.out + (long)Ch * HW, chw, g + (long)Ch * HW, chw, w.gpre, at<float>(packed, L.f4_scale),
                                  N, Ch, L.Cout, HW, affine};
            GH_TRY(launch_coupling_inv_bwd(cb, s));
            // (c) g_y1 += f'(y1)^T g_pre
            if (wgrad_fast(L) && bwd_cnet_chain(p, L, li, N, (size_t)N * p->max_hidden)) {
                // the gradients are normalised per sample (max |dL/dx| in [1, 2)): no further pre-scale.  (g_u2 / g_u0: stored by the
                // instance, read by nobody here)
                GH_TRY(launch_cnet_bwd(p, L, packed, N, T, w, 1.0f, &pend, s));
                pending = true; pend_C = Ch; pend_H = d.H; pend_W = d.W;
                continue;
            }
            const bool half_tape = li < (int)p->tape_has_masks.size() && p->tape_has_masks[li];
            GH_TRY(tape_to_f32(h2, half_tape, L, N, w, s));
            GH_TRY(dgrad_f4(L, packed, N, w, s));
            GH_TRY(launch_relu_bwd(w.gh2, h2, at<float>(packed, L.f2_scale), N, hid, HW, s));
            GH_TRY(tape_to_f32(h1, half_tape, L, N, w, s));
            GH_TRY(dgrad_f2(L, N, w, s));
            GH_TRY(launch_relu_bwd(w.gh1, h1, at<float>(packed, L.f0_scale), N, hid, HW, s));
            GH_TRY(dgrad_f0_add(L, packed, N, w, g, s));
        } else {  // SPLIT2D: input gradient (g_z1, g_z2) (N,C,HW) -> g_z1 + conv(g_pre, flipT(w)) (N,Ch,HW); g_eps to the caller
            GH_TRY(finish_pending(chw));
            const float* hout = at<float>(tape, tl[li].hout);
            const int k = p->n_split - 1 - L.split_idx;      // DECODE order, as glowhip_plan_decode reads eps
            SplitInvBwdArgs sb{hout, xin + (long)Ch * HW, chw, g + (long)Ch * HW, chw, grad_eps ? grad_eps[k] : nullptr, (long)Ch * HW,
                               w.words + N, w.gpre, at<float>(packed, L.f4_scale), N, Ch, HW};
            GH_TRY(launch_split_inv_bwd(sb, s));
            GH_TRY(dgrad_direct(w.gpre, d.f4_w, w.wT, w.gh1, N, Ch, d.H, d.W, L.Cout, 3, s));     // (N,Ch,HW)
            GH_TRY(launch_copy_strided(g, chw, gnext, (long)Ch * HW, N, (long)Ch * HW, s));
            GH_TRY(add_rows(gnext, (long)Ch * HW, w.gh1, N, (long)Ch * HW, s));
            g = gnext;
        }
    }
    const int* o = p->out_shape;
    const long per = (long)o[0] * o[1] * o[2];
    GH_TRY(finish_pending(per));
    if (grad_z) GH_TRY(launch_scale_rows(g, grad_z, per, w.words + N, N, s));
    return GLOWHIP_OK;
}

}  // namespace glowhip

// ================================================================================================ C ABI
extern "C" {

size_t glowhip_plan_tape_bytes(const glowhip_plan* plan, int N) {
    return (plan && N >= 0) ? tape_layout(plan, N, nullptr) : 0;
}

size_t glowhip_plan_train_workspace_bytes(const glowhip_plan* plan, int N) {
    return (plan && N >= 0) ? train_ws_layout(plan, N, nullptr, nullptr) : 0;
}

int glowhip_glow_forward_train(glowhip_plan* plan, const void* packed, const float* x, const float* noise,
                               const float* prior_mean, const float* prior_logs, long prior_stride, int n_bits,
                               float* z, float* nll_out, float* objective_out, int N, void* tape, size_t tape_bytes,
                               void* workspace, size_t workspace_bytes, glowhip_stream_t stream) {
    GH_REQUIRE(plan && packed && x && z && nll_out && tape && workspace, "glow_forward_train: null argument");
    GH_REQUIRE(N > 0 && N <= 65535, "glow_forward_train: batch size %d out of range", N);
    std::vector<TapeLayer> tl;
    GH_REQUIRE(tape_bytes >= tape_layout(plan, N, &tl), "glow_forward_train: tape too small");
    TrainWs w;
    GH_REQUIRE(workspace_bytes >= train_ws_layout(plan, N, workspace, &w), "glow_forward_train: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    GH_TRY(launch_zero_acc(w.acc, N, s, ACC_EXTRA));
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));      // the training kernels read the fp32 images from the first layer on
    GH_TRY(forward_train(plan, packed, x, noise, z, N, (char*)tape, tl, w.acc, w.gsh, s));
    GH_TRY(launch_top_logp(plan, z, prior_mean, prior_logs, prior_stride, N, w.acc, s));
    const double chw = (double)plan->in_shape[0] * plan->in_shape[1] * plan->in_shape[2];
    const double offset = -log(pow(2.0, n_bits)) * chw;
    const double scale = -1.0 / (log(2.0) * chw);
    return launch_finalize(nullptr, w.acc, at<double>(packed, 0), 1.0, offset, scale, nll_out, objective_out, N, s, ACC_EXTRA);
}

int glowhip_plan_backward_marks(glowhip_plan* plan, const int32_t* after_layer, void* const* events, int n) {
    GH_REQUIRE(plan && n >= 0 && (n == 0 || (after_layer && events)), "plan_backward_marks: bad argument");
    plan->bwd_marks.clear();
    for (int i = 0; i < n; ++i) {
        GH_REQUIRE(events[i] != nullptr, "plan_backward_marks: null event %d", i);
        GH_REQUIRE(after_layer[i] >= 0 && after_layer[i] < (int)plan->layers.size(), "plan_backward_marks: layer %d out of range", after_layer[i]);
        GH_REQUIRE(i == 0 || after_layer[i] < after_layer[i - 1], "plan_backward_marks: layer indices must decrease (sweep order)");
        plan->bwd_marks.emplace_back(after_layer[i], (hipEvent_t)events[i]);
    }
    return GLOWHIP_OK;
}

int glowhip_glow_backward(glowhip_plan* plan, const void* packed, const float* x, const void* tape, size_t tape_bytes,
                          const float* nll_grad, const float* z_grad, const float* prior_mean, const float* prior_logs,
                          long prior_stride, const glowhip_layer_grads* grads, float* grad_x, int N, void* workspace,
                          size_t workspace_bytes, glowhip_stream_t stream) {
    GH_REQUIRE(plan && packed && x && tape && nll_grad && grads && workspace, "glow_backward: null argument");
    GH_REQUIRE(N > 0 && N <= 65535, "glow_backward: batch size %d out of range", N);
    std::vector<TapeLayer> tl;
    GH_REQUIRE(tape_bytes >= tape_layout(plan, N, &tl), "glow_backward: tape too small");
    TrainWs w;
    GH_REQUIRE(workspace_bytes >= train_ws_layout(plan, N, workspace, &w), "glow_backward: workspace too small");
    for (const LayerPlan& L : plan->layers)
        GH_REQUIRE(L.d.kind != GLOWHIP_LAYER_FLOWSTEP || L.d.C <= CHANMIX_BWD_MAX_C, "glow_backward: C=%d unsupported (the channel mixer's limit is %d)", L.d.C, CHANMIX_BWD_MAX_C);
    hipStream_t s = (hipStream_t)stream;
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));
    const double chw = (double)plan->in_shape[0] * plan->in_shape[1] * plan->in_shape[2];
    GH_TRY(launch_gld_from_nll(nll_grad, w.gld, N, 1.0 / (log(2.0) * chw), s));
    GH_TRY(launch_sum_gld(w.gld, N, w.gsum, s));
    // top: dL/dz = z_grad + gld * d logp/dz
    const int* o = plan->out_shape;
    const float* zt = at<float>(tape, tl.back().out);
    GH_REQUIRE(!plan->head_on || 2L * o[0] <= plan->max_chw, "glow_backward: top head scratch does not fit");
    GH_TRY(launch_top_bwd(plan, zt, prior_mean, prior_logs, prior_stride, w.gld, z_grad, w.gA, w.gB, N, s));
    return backward_sweep(plan, packed, x, (const char*)tape, tl, grads, grad_x, N, w, w.gA, s);
}

size_t glowhip_plan_decode_vjp_workspace_bytes(const glowhip_plan* plan, int N) {
    return (plan && N >= 0) ? vjp_ws_layout(plan, N, nullptr, nullptr) : 0;
}

int glowhip_plan_decode_vjp(glowhip_plan* plan, const void* packed, const float* x, const float* grad_x, float* grad_z,
                            float* const* grad_eps, int n_eps, int N, void* tape, size_t tape_bytes, void* workspace,
                            size_t workspace_bytes, glowhip_stream_t stream) {
    GH_REQUIRE(plan != nullptr, "plan_decode_vjp: null plan");
    GH_REQUIRE(n_eps == plan->n_split, "plan_decode_vjp: %d eps gradients given, plan has %d Split2d layers", n_eps, plan->n_split);
    GH_REQUIRE(n_eps == 0 || grad_eps, "plan_decode_vjp: null grad_eps table");
    GH_REQUIRE(N >= 0 && N <= 65535, "plan_decode_vjp: batch size %d out of range", N);
    if (N == 0) return GLOWHIP_OK;
    GH_REQUIRE(packed && x && grad_x && tape && workspace, "plan_decode_vjp: null argument");
    std::vector<TapeLayer> tl;
    GH_REQUIRE(tape_bytes >= tape_layout(plan, N, &tl), "plan_decode_vjp: tape too small");
    VjpWs w;
    GH_REQUIRE(workspace_bytes >= vjp_ws_layout(plan, N, workspace, &w), "plan_decode_vjp: workspace too small");
    for (const LayerPlan& L : plan->layers)
        GH_REQUIRE(L.d.kind != GLOWHIP_LAYER_FLOWSTEP || L.d.C <= CHANMIX_BWD_MAX_C, "plan_decode_vjp: C=%d unsupported (the channel mixer's limit is %d)", L.d.C, CHANMIX_BWD_MAX_C);
    hipStream_t s = (hipStream_t)stream;
    // (the flags of a training forward whose backward is still to come are this plan's too: put back on every way out)
    struct KeepMasks { glowhip_plan* p; std::vector<char> v; ~KeepMasks() { p->tape_has_masks.swap(v); } } keep{plan, plan->tape_has_masks};
    GH_TRY(launch_zero_acc(w.acc, N, s, ACC_EXTRA));
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));
    // the tape of the decode = the tape of the training forward on the decoded image (a FlowStep's coupling network sees the same
    // y1 in both directions): no noise, no dequantisation draw, no prior, no head
    GH_TRY(forward_train(plan, packed, x, nullptr, nullptr, N, (char*)tape, tl, w.acc, w.gsh, s));
    const long per = (long)plan->in_shape[0] * plan->in_shape[1] * plan->in_shape[2];
    GH_TRY(launch_grad_norm(grad_x, per, w.words, N, s));
    GH_TRY(launch_scale_rows(grad_x, w.gA, per, w.words, N, s));
    return decode_vjp_sweep(plan, packed, x, (const char*)tape, tl, grad_z, grad_eps, N, w, s);
}

}  // extern "C"

// plan.hip -- flow plans: the host-side executor that turns a FlowModel (Squeeze2d / FlowStep /
// Split2d stack, network/model.py:230-294) into a fixed sequence of kernel launches on one HIP stream.
// There is no tracing compiler: the layer list is static, so the launch sequence is built once and
// replayed; all scratch comes from a caller-provided workspace, all parameter-derived data (exp(3 logs),
// K-major MFMA weight images, W^-1, log|det W|) from a caller-provided `packed` buffer refreshed by
// glowhip_plan_pack.
// Here: the workspace carving, the inference executor (run_forward / run_reverse), the encode / decode / glow_forward / actnorm_init /
// status entries, the describe / launch-count / timing / dequantisation calls and k_pack_scales (the init pass').  Plan construction and the pack: plan_build.hip.
#include <math.h>
#include <stdio.h>

#include "plan_internal.h"

namespace glowhip {

// ---------------------------------------------------------------- pack kernels
__global__ void __launch_bounds__(256) k_pack_scales(const float* __restrict__ logs, int n, float* __restrict__ scale,
                                                     float* __restrict__ inv_scale) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float l3 = logs[i] * LOGSCALE;
    scale[i] = expf(l3);
    if (inv_scale) inv_scale[i] = expf(-l3);
}

static int pack_scales(const float* logs, int n, float* scale, float* inv, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_scales, dim3(cdiv(n, 256)), dim3(256), 0, s, logs, n, scale, inv);
    GH_LAUNCH_CHECK("k_pack_scales");
    return GLOWHIP_OK;
}

// Workspace carving
struct Workspace {
    unsigned long long* acc;
    float* bufA;
    float* bufB;
    float* h1;
    float* h2;
};

// acc | bufA | bufB | h1 | h2; returns the size (w / base null: that alone)
static size_t ws_layout(const glowhip_plan* p, int N, void* base, Workspace* w) {
    size_t off = 0;
    const size_t chw = (size_t)N * p->max_chw * 4, hid = (size_t)N * p->max_hidden * 4;
    const size_t o_acc = take(off, (size_t)N * 8 * (2 + ACC_EXTRA));
    const size_t o_A = take(off, chw), o_B = take(off, chw), o_h1 = take(off, hid), o_h2 = take(off, hid);
    if (w && base)
        *w = Workspace{at<unsigned long long>(base, o_acc), at<float>(base, o_A), at<float>(base, o_B), at<float>(base, o_h1),
                       at<float>(base, o_h2)};
    return align_up(off, 256);
}

static int carve(const glowhip_plan* p, int N, void* ws, size_t bytes, Workspace& w) {
    const size_t need = ws_layout(p, N, ws, &w);
    if (bytes < need || ws == nullptr) {
        set_error("workspace too small: need %zu bytes, got %zu", need, bytes);
        return GLOWHIP_EWORKSPACE;
    }
    return GLOWHIP_OK;
}

// ---------------------------------------------------------------- coupling network f() (network/module.py:300-319)
// Runs conv3x3 -> actnorm -> relu -> conv1x1 -> actnorm -> relu -> conv3x3(zeros) and applies the
// coupling to z2.  x1: first-half channels (batch stride x1_bs).
// split-half f16 kernels off for this plan: its own family (glowhip_plan_set_family) or the process-wide testing hook
static bool sh_off(const glowhip_plan* p) { return debug_switches().exact_fp32 || (p && p->family == GLOWHIP_FAMILY_EXACT_FP32); }
static bool cnet_runs(const glowhip_plan* p, const LayerPlan& L) { return L.cnet && !sh_off(p); }

// deep levels (dnet_sh.hip): layers k_cnet does not take, with an invertible 1x1 convolution, on the product family
static bool dnet_runs(const glowhip_plan* p, const LayerPlan& L) { return L.dnet && !sh_off(p); }
// the run of consecutive FlowSteps of li's shape that take the deep-level kernels, walking in direction `dir` (+1 encode, -1 decode)
static int dnet_run_end(const glowhip_plan* p, int li, int dir) {
    const int nl = (int)p->layers.size();
    const glowhip_layer_desc& d = p->layers[li].d;
    int lj = li;
    while (lj + dir >= 0 && lj + dir < nl) {
        const LayerPlan& Ln = p->layers[lj + dir];
        if (Ln.d.kind != GLOWHIP_LAYER_FLOWSTEP || !dnet_runs(p, Ln) || Ln.d.C != d.C || Ln.d.H != d.H || Ln.d.W != d.W ||
            Ln.d.hidden != d.hidden || Ln.Cout != p->layers[li].Cout) break;
        lj += dir;
    }
    return lj;
}
// A level's run on the deep-level kernels begins at step li: the level's descriptor (state S, scratch h1), the padded operands'
// borders, PREP (encode: with step li's ActNorm)
static int dnet_open(glowhip_plan* p, const void* packed, int li, const float* cur, float* S, int N, const Workspace& w, int reverse,
                     DnetLevel* D, hipStream_t s) {
    const LayerPlan& L0 = p->layers[li];
    const glowhip_layer_desc& d = L0.d;
    const long chw = (long)d.C * d.H * d.W;
    *D = DnetLevel{N, d.C, d.H, d.W, d.hidden, L0.Cout, S, chw, w.h1};
    GH_TRY(dnet_level_begin(*D, s));
    p->cur_layer = li;
    ScopedTimer t(p, GLOWHIP_K_OTHER, 0, s);
    count_launch(p, "k_dn_prep");
    return dnet_prep(*D, cur, chw, reverse ? nullptr : d.an_bias, reverse ? nullptr : at<float>(packed, L0.an_scale), reverse, s);
}
// One level's run of FlowSteps [li .. lj] (encode) on the deep-level kernels: PREP, then MIX -> F0 -> F2 -> F4 -> FIN per step; the
// result is left in `S` (N, C, H, W).
static int run_dnet_forward(glowhip_plan* p, const void* packed, int li, int lj, const float* cur, float* S, int N, const Workspace& w,
                            hipStream_t s) {
    DnetLevel D{};
    GH_TRY(dnet_open(p, packed, li, cur, S, N, w, 0, &D, s));
    for (int k = li; k <= lj; ++k) {
        const LayerPlan& L = p->layers[k];
        p->cur_layer = k;
        {
            ScopedTimer t(p, GLOWHIP_K_CHANMIX, 1, s);
            count_launch(p, "k_dn_gemm(mix)");
            GH_TRY(dnet_mix(D, at<char>(packed, L.dn_mix), nullptr, nullptr, 1, s));
        }
        int ks = 1;
        {
            ScopedTimer t(p, GLOWHIP_K_CONV_F2, 1, s);
            count_launch(p, "k_dn_gemm(f0,f2,f4)");
            GH_TRY(dnet_coupling_net(D, at<char>(packed, L.dn_w0), at<char>(packed, L.dn_w2), at<char>(packed, L.dn_w4), &ks, s));
        }
        const LayerPlan* Ln = k < lj ? &p->layers[k + 1] : nullptr;
        ScopedTimer t(p, GLOWHIP_K_CFINISH, 0, s);
        count_launch(p, "k_dn_fin");
        GH_TRY(dnet_finish(D, ks, L.d.f4_bias, at<float>(packed, L.f4_scale), tail_mode(L.d, 0), w.acc, Ln ? Ln->d.an_bias : nullptr,
                           Ln ? at<float>(packed, Ln->an_scale) : nullptr, Ln != nullptr, s));
    }
    return GLOWHIP_OK;
}
// ... and decode: steps li, li - 1, ..., lj (li >= lj): PREP, then F0 -> F2 -> F4 -> FIN -> MIX^-1 per step
static int run_dnet_reverse(glowhip_plan* p, const void* packed, int li, int lj, const float* cur, float* S, int N, const Workspace& w,
                            hipStream_t s) {
    DnetLevel D{};
    GH_TRY(dnet_open(p, packed, li, cur, S, N, w, 1, &D, s));
    for (int k = li; k >= lj; --k) {
        const LayerPlan& L = p->layers[k];
        p->cur_layer = k;
        int ks = 1;
        {
            ScopedTimer t(p, GLOWHIP_K_CONV_F2, 1, s);
            count_launch(p, "k_dn_gemm(f0,f2,f4)");
            GH_TRY(dnet_coupling_net(D, at<char>(packed, L.dn_w0), at<char>(packed, L.dn_w2), at<char>(packed, L.dn_w4), &ks, s));
        }
        {
            ScopedTimer t(p, GLOWHIP_K_CFINISH, 0, s);
            count_launch(p, "k_dn_fin");
            GH_TRY(dnet_finish(D, ks, L.d.f4_bias, at<float>(packed, L.f4_scale), tail_mode(L.d, 1), w.acc, nullptr, nullptr, 1, s));
        }
        ScopedTimer t(p, GLOWHIP_K_CHANMIX, 1, s);
        count_launch(p, "k_dn_gemm(mix)");
        GH_TRY(dnet_mix(D, at<char>(packed, L.dn_mixinv), at<float>(packed, L.an_inv_scale), L.d.an_bias, k > lj, s));
    }
    return GLOWHIP_OK;
}

// ---- the one-kernel coupling network (cnet_sh.hip).  A FlowStep is k_cnet (partial sums of h = f(z1)) + a finishing step
// (coupling, log-det, channel mixer), which runs as its own kernel right behind it.
// which instance of k_cnet ran (run-time evidence for the tests): "variant:k_cnet<hidden,row split,pixel tile>"
static void count_cnet_variant(glowhip_plan* p, const CnetArgs& c, const CnetPending& pend) {
    char name[64];
    snprintf(name, sizeof name, "variant:k_cnet%s<%d,%d,%d>", pend.one_wave ? "1w" : "", c.hidden, pend.MS, 1 << pend.lpxt);
    count_launch(p, name);
}
// One FlowStep's k_cnet launch and its finishing kernel.
static int run_cnet_step(glowhip_plan* p, const CnetArgs& c, hipStream_t s) {
    CnetPending pend{};
    {
        ScopedTimer t(p, GLOWHIP_K_CNET, 1, s);
        count_launch(p, "k_cnet");
        GH_TRY(launch_cnet_main(c, s, &pend));
        count_cnet_variant(p, c, pend);
    }
    ScopedTimer t(p, GLOWHIP_K_CFINISH, 0, s);
    count_launch(p, c.mix.C ? "k_cfinish+mixer" : "k_cfinish");
    return launch_cnet_finish(c, pend, s);
}

// The coupling network of a FlowStep that neither k_cnet nor the deep-level kernels take (odd hidden widths, tiny images, the
// exact-fp32 family): one exact-fp32 kernel per layer.
static int run_coupling(glowhip_plan* P, const LayerPlan& L, const void* packed, const float* x1, long x1_bs, const float* z2_in,
                        long z2_in_bs, float* z2_out, long z2_out_bs, int N, int reverse, const Workspace& w,
                        hipStream_t s) {
    const glowhip_layer_desc& d = L.d;
    const int Ch = d.C / 2, HW = d.H * d.W, hid = d.hidden;
    {   // f.0: 3x3, Cin=C/2 -> hidden, ActNorm + ReLU epilogue
        ScopedTimer t0(P, GLOWHIP_K_CONV_F0, L.mfma_first || L.first_halo, s);
        if (L.first_halo) {
            const float* wf = at<float>(packed, L.f0_wt);
            count_launch(P, "k_conv_first_f32");
            GH_TRY(launch_conv_mfma_first(x1, x1_bs, wf, wf + (size_t)9 * Ch * hid, w.h1, N, Ch, d.H, d.W, hid, s, 1));
        } else if (L.mfma_first) {
            count_launch(P, "k_conv_wide_f32");
            GH_TRY(launch_conv_mfma_wide(x1, x1_bs, at<float>(packed, L.f0_wt), d.f0_an_bias, at<float>(packed, L.f0_scale),
                                         w.h1, N, Ch, d.H, d.W, hid, 3, s, 1, w.h2, (size_t)N * P->max_hidden));
        } else {
            ConvArgs c{x1, x1_bs, d.f0_w, nullptr, d.f0_an_bias, nullptr, at<float>(packed, L.f0_scale), 1, w.h1,
                       N, Ch, d.H, d.W, hid, 3};
            count_launch(P, "k_conv_direct");
            GH_TRY(launch_conv_direct(c, s));
        }
    }
    {   // f.2: 1x1, hidden -> hidden, ActNorm + ReLU epilogue
        ScopedTimer t2(P, GLOWHIP_K_CONV_F2, L.mfma_mid, s);
        if (L.mfma_mid) {
            count_launch(P, "k_gemm_f32");
            GH_TRY(launch_conv_mfma_wide(w.h1, (long)hid * HW, at<float>(packed, L.f2_wt), d.f2_an_bias,
                                         at<float>(packed, L.f2_scale), w.h2, N, hid, d.H, d.W, hid, 1, s));
        } else {
            ConvArgs c{w.h1, (long)hid * HW, d.f2_w, nullptr, d.f2_an_bias, nullptr, at<float>(packed, L.f2_scale), 1, w.h2,
                       N, hid, d.H, d.W, hid, 1};
            count_launch(P, "k_conv_direct");
            GH_TRY(launch_conv_direct(c, s));
        }
    }
    // f.4: 3x3 zeros conv (+bias, *exp(3 logs)) and the coupling itself
    ScopedTimer t4(P, GLOWHIP_K_CONV_F4, L.mfma_last, s);
    if (L.mfma_last) {
        TailConvArgs t{};
        t.x = w.h2; t.x_bs = (long)hid * HW; t.wp = at<float>(packed, L.f4_wp); t.bias = d.f4_bias;
        t.scale = at<float>(packed, L.f4_scale);
        t.N = N; t.Cin = hid; t.H = d.H; t.W = d.W; t.Cout = L.Cout;
        t.mode = tail_mode(d, reverse);
        t.z2_in = z2_in; t.z2_in_bs = z2_in_bs; t.z2_out = z2_out; t.z2_out_bs = z2_out_bs; t.acc = w.acc;
        t.zeros = at<float>(packed, 64);   // zero block kept by glowhip_plan_pack
        count_launch(P, "k_conv_tail_f32");
        GH_TRY(launch_conv_mfma_tail(t, s));
    } else {
        if (L.wide_last) {     // (conv + bias) * exp(3 logs) on the fp32 MFMA implicit-GEMM kernel
            count_launch(P, "k_conv_wide_f32");
            // split-K partial sums go behind the output in the same (level-1 sized) buffer
            const size_t out_f = (size_t)N * L.Cout * HW, h1_f = (size_t)N * P->max_hidden;
            GH_TRY(launch_conv_mfma_wide(w.h2, (long)hid * HW, at<float>(packed, L.f4_wt), d.f4_bias, at<float>(packed, L.f4_scale),
                                         w.h1, N, hid, d.H, d.W, L.Cout, 3, s, 0, h1_f > out_f ? w.h1 + out_f : nullptr,
                                         h1_f > out_f ? h1_f - out_f : 0));
        } else {
            ConvArgs c{w.h2, (long)hid * HW, d.f4_w, d.f4_bias, nullptr, nullptr, at<float>(packed, L.f4_scale), 0, w.h1,
                       N, hid, d.H, d.W, L.Cout, 3};
            count_launch(P, "k_conv_direct");
            GH_TRY(launch_conv_direct(c, s));
        }
        CouplingTailArgs t{w.h1, z2_in, z2_in_bs, z2_out, z2_out_bs, N, Ch, HW,
                           d.coupling == GLOWHIP_COUPLING_AFFINE, reverse, w.acc};
        GH_TRY(launch_coupling_tail(t, s));
    }
    return GLOWHIP_OK;
}

// Split2d prior conv + tail (network/module.py:498-536).  d.C = channels of the un-split tensor.
// Forward: z2_out (optional) receives the draw z2 implies under the prior, (z2 - mean) * exp(-logs) (glowhip_plan_bind_latents).
// Reverse: eps == null draws it in the epilogue from `rng` (glowhip_plan_bind_sampler): same launches as with eps injected.
static int run_split(glowhip_plan* P, const LayerPlan& L, const void* packed, const float* z1, long z1_bs, const float* z2, long z2_bs,
                     const float* eps, float* z2_out, long z2_out_bs, int N, int reverse, const Workspace& w,
                     hipStream_t s, const SamplerSpec& rng = SamplerSpec{}) {
    const glowhip_layer_desc& d = L.d;
    const int Ch = d.C / 2, HW = d.H * d.W;
    if (L.mfma_last) {
        TailConvArgs t{};
        t.x = z1; t.x_bs = z1_bs; t.wp = at<float>(packed, L.f4_wp); t.bias = d.f4_bias;
        t.scale = at<float>(packed, L.f4_scale);
        t.N = N; t.Cin = Ch; t.H = d.H; t.W = d.W; t.Cout = L.Cout;
        t.mode = reverse ? TAIL_SPLIT_REV : TAIL_SPLIT_FWD;
        t.z2_in = reverse ? eps : z2; t.z2_in_bs = reverse ? (long)Ch * HW : z2_bs;
        t.z2_out = z2_out; t.z2_out_bs = z2_out_bs; t.acc = w.acc;
        t.zeros = at<float>(packed, 64);
        t.rng = rng;
        count_launch(P, conv_mfma_tail_takes_dma(t) ? "split_prior(k_conv_tail_dma)" : "split_prior(k_conv_tail)");
        GH_TRY(launch_conv_mfma_tail(t, s));
    } else {
        ConvArgs c{z1, z1_bs, d.f4_w, d.f4_bias, nullptr, nullptr, at<float>(packed, L.f4_scale), 0, w.h1,
                   N, Ch, d.H, d.W, L.Cout, 3};
        GH_TRY(launch_conv_direct(c, s));
        count_launch(P, "split_prior(k_split_tail)");
        SplitTailArgs t{w.h1, z2, z2_bs, eps, z2_out, z2_out_bs, N, Ch, HW, reverse, w.acc, rng};
        GH_TRY(launch_split_tail(t, s));
    }
    return GLOWHIP_OK;
}

static float* other_buf(const Workspace& w, const float* cur) { return cur == w.bufA ? w.bufB : w.bufA; }

// ---------------------------------------------------------------- encode (network/model.py:263-276)
// A Squeeze2d layer whose output only the NEXT layer's k_chanmix reads (the first FlowStep of a level on the k_cnet path or the
// kernel pairs) is not run at all: the mixer gathers the squeezed view itself, dequantisation noise and 8-bit scaling included
// ("fuse uint8 -> fp32 scaling + noise + first squeeze into the first kernel").
struct SqueezeFold { const void* src; int u8; float div; const float* noise; RngSpec rng; int W; long bs; };
static void apply_fold(ChanMixArgs& m, SqueezeFold& fold) {      // a pending fold becomes this mixer's input
    if (!fold.src) return;
    m.sq_src = fold.src; m.sq_u8 = fold.u8; m.sq_div = fold.div; m.sq_noise = fold.noise; m.sq_rng = fold.rng; m.sq_W = fold.W; m.sq_bs = fold.bs;
    fold = SqueezeFold{};
}
static int run_chanmix(glowhip_plan* p, const ChanMixArgs& m, hipStream_t s) {
    ScopedTimer tm(p, GLOWHIP_K_CHANMIX, 0, s);
    count_launch(p, "k_chanmix");
    return launch_chanmix(m, s);
}
// (testing: the mixer-fusion switch glowhip_debug_force_tail_tile(0x8000) also brings the squeeze kernels back -- the two must
// agree bit for bit)

// the snapshot that closes a level (glowhip_plan_bind_level_terms; evaluate.hip): the accumulator words as every launch before it left them
static int level_snapshot(glowhip_plan* p, unsigned long long* snaps, int level, int N, const Workspace& w, hipStream_t s) {
    count_launch(p, "k_level_snapshot");
    return launch_level_snapshot(w.acc, snaps + (size_t)level * (2 + ACC_EXTRA) * N, N, s);
}

// level_snaps (glow_forward alone, with level terms bound): one snapshot behind the launches of every Split2d
static int run_forward(glowhip_plan* p, const void* packed, const float* x, const float* noise, float* z_out, int N,
                       const Workspace& w, hipStream_t s, int first_layer = 0, const RngSpec* rng = nullptr,
                       const uint8_t* x_u8 = nullptr, float u8_div = 1.f, unsigned long long* level_snaps = nullptr) {
    const float* cur = x;
    SqueezeFold fold{};      // set by a skipped squeeze layer, consumed by the next layer's k_chanmix
    const int nl = (int)p->layers.size();
    bool premixed = false;   // `cur` already holds this step's ActNorm + permutation output (applied by the previous tail)
    int scr_i = 0;
    long cur_bs = 0;         // batch stride of `cur` when it is Split2d's z1 left where it lies (0: dense)
    // does the Squeeze2d at layer `ls` fold into the next layer's mixer?
    auto squeeze_folds = [&](int ls) {
        if (debug_switches().no_mixer_fusion || ls + 1 >= nl - 1 || p->layers[ls].d.W % 2 != 0) return false;
        const LayerPlan& Ln = p->layers[ls + 1];
        return Ln.d.kind == GLOWHIP_LAYER_FLOWSTEP && !dnet_runs(p, Ln) && chanmix_squeeze_foldable(Ln.d.C);
    };
    for (int li = first_layer; li < nl; ++li) {
        const LayerPlan& L = p->layers[li];
        const glowhip_layer_desc& d = L.d;
        p->cur_layer = li;
        float* dst = (li == nl - 1) ? z_out : other_buf(w, cur);
        const int HW = d.H * d.W;
        const long chw = (long)d.C * HW;
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) {
            const bool u8 = x_u8 != nullptr && li == 0;
            const bool foldable = squeeze_folds(li);
            if (foldable) {
                fold = SqueezeFold{u8 ? (const void*)x_u8 : (const void*)cur, u8 ? 1 : 0, u8_div, noise,
                                   (li == 0 && rng) ? *rng : RngSpec{}, d.W, cur_bs};
                cur_bs = 0;
                count_launch(p, "squeeze(folded)");
                noise = nullptr; rng = nullptr;
                continue;      // `cur` stays the un-squeezed tensor; the next layer reads it through `fold`
            }
            if (u8) GH_TRY(launch_squeeze_u8(x_u8, noise, dst, N, d.C, d.H, d.W, 2, u8_div, s, rng));
            else GH_TRY(launch_squeeze(cur, noise, dst, N, d.C, d.H, d.W, 2, 0, s, li == 0 ? rng : nullptr));
            noise = nullptr; rng = nullptr;
        } else {
            if (noise || (rng && li == 0)) {  // dequantisation noise with no leading squeeze (only possible at layer 0, cur == x):
                          // the identity "squeeze" (factor 1) adds it into a workspace buffer
                GH_TRY(launch_squeeze(cur, noise, w.bufA, N, d.C, d.H, d.W, 1, 0, s, rng));
                cur = w.bufA;
                noise = nullptr; rng = nullptr;
                if (li != nl - 1) dst = w.bufB;
            }
            const int Ch = d.C / 2;
            if (d.kind == GLOWHIP_LAYER_FLOWSTEP && dnet_runs(p, L) && !premixed) {
                // ---- deep level: the whole run of same-shape FlowSteps on the per-layer SH2 kernels (dnet_sh.hip)
                const int lj = dnet_run_end(p, li, +1);
                float* S = other_buf(w, cur);
                GH_TRY(run_dnet_forward(p, packed, li, lj, cur, S, N, w, s));
                if (lj == nl - 1) GH_TRY(launch_copy_strided(S, chw, z_out, chw, N, chw, s));
                cur = S;
                li = lj;
                continue;
            }
            if (d.kind == GLOWHIP_LAYER_FLOWSTEP && cnet_runs(p, L)) {
                // ---- k_cnet path.  `cur` holds the input of this step's mixer, or -- `premixed` -- its output
                float* scratch = (scr_i ^= 1) ? w.h1 : w.h2;
                CnetArgs c = cnet_base(L, packed, N, 0, scratch, w.acc);
                if (!premixed) {
                    ChanMixArgs m = chanmix_fwd_args(L, packed, N, cur, chw, dst);
                    apply_fold(m, fold);
                    GH_TRY(run_chanmix(p, m, s));
                    cur = dst;
                }
                c.x = cur; c.x_bs = chw; c.z_in = cur; c.z_in_bs = chw;
                premixed = false;
                // the step is finished right behind its k_cnet: with the NEXT step's mixer when that is a same-shape FlowStep
                float* out = (li == nl - 1) ? z_out : const_cast<float*>(cur);
                c.z_out = out; c.z_out_bs = chw;
                if (li + 1 < nl - 1 && !debug_switches().no_mixer_fusion && d.C <= 96) {
                    const LayerPlan& Ln = p->layers[li + 1];
                    const glowhip_layer_desc& dn = Ln.d;
                    if (dn.kind == GLOWHIP_LAYER_FLOWSTEP && dn.C == d.C && dn.H == d.H && dn.W == d.W) {
                        c.mix = mixer_fwd(Ln, packed);
                        premixed = true;
                    }
                }
                GH_TRY(run_cnet_step(p, c, s));
                cur = out;
                continue;
            }
            if (d.kind == GLOWHIP_LAYER_FLOWSTEP) {
                if (premixed) {
                    dst = const_cast<float*>(cur);   // the step runs in place on the already mixed buffer
                } else {
                    ChanMixArgs m = chanmix_fwd_args(L, packed, N, cur, chw, dst);
                    apply_fold(m, fold);
                    GH_TRY(run_chanmix(p, m, s));
                }
                float* z2 = dst + (long)Ch * HW;
                GH_TRY(join_legacy(p, s));
                GH_TRY(run_coupling(p, L, packed, dst, chw, z2, chw, z2, chw, N, 0, w, s));
                premixed = false;
            } else {  // SPLIT2D: score z2 under the prior predicted from z1, keep z1
                GH_TRY(join_legacy(p, s));
                // bound latents are in DECODE order (deepest split first); contiguous (N, C/2, HW) buffers
                float* eps_out = p->eps_out.empty() ? nullptr : p->eps_out[p->n_split - 1 - L.split_idx];
                GH_TRY(run_split(p, L, packed, cur, chw, cur + (long)Ch * HW, chw, nullptr, eps_out, (long)Ch * HW, N, 0, w, s));
                // z1 is compacted for the next layer -- unless that is a Squeeze2d that folds into the mixer behind it: the fold
                // reads z1 where it lies, through the batch stride of the undivided tensor
                if (li + 1 < nl && p->layers[li + 1].d.kind == GLOWHIP_LAYER_SQUEEZE && squeeze_folds(li + 1)) {
                    count_launch(p, "split2d:z1 in place");
                    cur_bs = chw;
                    if (level_snaps) GH_TRY(level_snapshot(p, level_snaps, L.split_idx, N, w, s));
                    continue;
                }
                GH_TRY(launch_copy_strided(cur, chw, dst, (long)Ch * HW, N, (long)Ch * HW, s));
                if (level_snaps) GH_TRY(level_snapshot(p, level_snaps, L.split_idx, N, w, s));
            }
        }
        cur = dst;
    }
    return GLOWHIP_OK;
}

// ---------------------------------------------------------------- decode (network/model.py:278-294)
// A Split2d without an injected eps (eps == null, k >= n_eps or eps[k] == null) draws stream 1 + k of the bound sampler
// (sampler_rng.h) inside its prior kernel; *drawn (optional) receives how many did.  x_u8 (optional; layer 0 must be a
// Squeeze2d): the final un-squeeze stores 8-bit pixels there -- and the fp32 ones to x_out only when that is given too.
static int run_reverse(glowhip_plan* p, const void* packed, const float* z, const float* const* eps, int n_eps,
                       float* x_out, int N, const Workspace& w, hipStream_t s, int* drawn = nullptr, uint8_t* x_u8 = nullptr) {
    const float* cur = z;
    const int nl = (int)p->layers.size();
    int ke = 0;
    int scr_i = 0;
    for (int li = nl - 1; li >= 0; --li) {
        const LayerPlan& L = p->layers[li];
        const glowhip_layer_desc& d = L.d;
        p->cur_layer = li;
        float* dst = (li == 0) ? x_out : other_buf(w, cur);
        const int HW = d.H * d.W;
        const long chw = (long)d.C * HW;
        const int Ch = d.C / 2;
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) {
            if (li == 0 && x_u8) {
                count_launch(p, "unsqueeze(u8)");
                GH_TRY(launch_unsqueeze2_u8(cur, x_u8, x_out, N, d.C * 4, d.H / 2, d.W / 2, s));
            } else
            GH_TRY(launch_squeeze(cur, nullptr, dst, N, d.C * 4, d.H / 2, d.W / 2, 2, 1, s));
        } else if (d.kind == GLOWHIP_LAYER_FLOWSTEP) {
            float* z2 = dst + (long)Ch * HW;
            if (dnet_runs(p, L)) {
                const int lj = dnet_run_end(p, li, -1);
                float* S = other_buf(w, cur);
                GH_TRY(run_dnet_reverse(p, packed, li, lj, cur, S, N, w, s));
                if (lj == 0) GH_TRY(launch_copy_strided(S, chw, x_out, chw, N, chw, s));
                cur = S;
                li = lj;
                continue;
            }
            if (cnet_runs(p, L)) {
                // coupling^-1, permutation^-1 and ActNorm^-1 by the finishing kernel
                float* scratch = (scr_i ^= 1) ? w.h1 : w.h2;
                CnetArgs c = cnet_base(L, packed, N, 1, scratch, w.acc);
                c.x = cur; c.x_bs = chw; c.z_in = cur; c.z_in_bs = chw;
                if (d.C <= 96) {
                    float* fout = (li == 0) ? x_out : other_buf(w, cur);
                    c.z_out = fout; c.z_out_bs = chw; c.mix = mixer_rev(L, packed);
                    GH_TRY(run_cnet_step(p, c, s));      // (its mixer is set: the finishing counts as "k_cfinish+mixer")
                    cur = fout;
                } else {
                    // wider than the finishing kernel's mixer (additive coupling, 96 < C <= 112: L.cnet holds, the fused mixer
                    // does not): coupling^-1 alone by the finishing kernel, then permutation^-1 + ActNorm^-1 by k_chanmix
                    float* mid = other_buf(w, cur);
                    c.z_out = mid; c.z_out_bs = chw;
                    GH_TRY(run_cnet_step(p, c, s));
                    float* out = (li == 0) ? x_out : other_buf(w, mid);
                    ChanMixArgs m = chanmix_rev_args(L, packed, N, mid, mid + (long)Ch * HW, chw, out);
                    GH_TRY(run_chanmix(p, m, s));
                    cur = out;
                }
                continue;
            }
            // z2 is updated IN PLACE when `cur` is a workspace buffer (every step but the first of a decode, whose input is the
            // caller's z): the mixer's inputs then do not alias its output, and the wide mixer may slice its output channels
            // over workgroups (config E's 4x4 level: 16 workgroups of 384 outputs each took 350 us per step with the alias)
            if (cur == w.bufA || cur == w.bufB) z2 = const_cast<float*>(cur) + (long)Ch * HW;
            GH_TRY(run_coupling(p, L, packed, cur, chw, cur + (long)Ch * HW, chw, z2, chw, N, 1, w, s));
            ChanMixArgs m = chanmix_rev_args(L, packed, N, cur, z2, chw, dst);
            GH_TRY(run_chanmix(p, m, s));
        } else {  // SPLIT2D reverse: z1 = cur (N, C/2, HW) -> cat(z1, mean + exp(logs)*eps)
            const float* e = (eps && ke < n_eps) ? eps[ke] : nullptr;
            GH_REQUIRE(e || p->sampler_pos, "decode: missing eps draw for Split2d #%d", ke);
            SamplerSpec rng{};
            if (!e) {
                rng = SamplerSpec{p->sampler_pos, 1 + ke, p->sampler_std[ke]};
                if (drawn) ++*drawn;
            }
            GH_TRY(run_split(p, L, packed, cur, (long)Ch * HW, nullptr, 0, e, dst + (long)Ch * HW, chw, N, 1, w, s, rng));
            GH_TRY(launch_copy_strided(cur, (long)Ch * HW, dst, chw, N, (long)Ch * HW, s));
            ++ke;
        }
        cur = dst;
    }
    return GLOWHIP_OK;
}

// the last launch of a call that drew from the bound sampler with `advance`: the next call draws at call + 1
static int advance_sampler(glowhip_plan* plan, int drawn, hipStream_t s) {
    if (!drawn || !plan->sampler_advance) return GLOWHIP_OK;
    count_launch(plan, "k_sampler_advance");
    return launch_sampler_advance(plan->sampler_pos, s);
}

static int check_plan_args(const glowhip_plan* plan, const void* packed, int N) {
    GH_REQUIRE(plan != nullptr, "null plan");
    GH_REQUIRE(packed != nullptr, "null packed-parameter buffer (call glowhip_plan_pack first)");
    GH_REQUIRE(N >= 0 && N <= 65535, "batch size %d out of range", N);
    return GLOWHIP_OK;
}
// the workspace of a call on N samples, its log-det accumulators zeroed
static int open_workspace(const glowhip_plan* p, int N, void* ws, size_t bytes, Workspace& w, hipStream_t s) {
    GH_TRY(carve(p, N, ws, bytes, w));
    return launch_zero_acc(w.acc, N, s, ACC_EXTRA);
}

// Glow.normal_flow behind glowhip_glow_forward (x) and glowhip_glow_forward_u8 (x_u8 / divisor: 8-bit pixels, SURVEY.md 8f N4 --
// the leading Squeeze2d reads the bytes itself, and the executor starts from bufA: the ping-pong parity of the workspace buffers
// differs between the two)
static int glow_forward(glowhip_plan* plan, const void* packed, const float* x, const uint8_t* x_u8, float divisor, const float* noise,
                        const float* prior_mean, const float* prior_logs, long prior_stride, int n_bits, float* z, float* nll_out,
                        float* objective_out, int N, void* workspace, size_t workspace_bytes, hipStream_t s) {
    Workspace w;
    GH_TRY(open_workspace(plan, N, workspace, workspace_bytes, w, s));
    RngSpec rng{plan->rng_on && !noise, plan->rng_seed, plan->rng_calls, (float)(1.0 / pow(2.0, n_bits))};
    if (rng.on) ++plan->rng_calls;
    // per-level terms bound (glowhip_plan_bind_level_terms): a snapshot of the accumulators closes every level
    unsigned long long* snaps = plan->level_terms ? plan->level_scratch : nullptr;
    const int n_levels = plan->n_split + 1;
    if (snaps) {
        const size_t need = (size_t)n_levels * (2 + ACC_EXTRA) * (size_t)N * 8;
        if (plan->level_scratch_bytes < need) {
            set_error("glow_forward: level scratch too small: need %zu bytes for batch %d, got %zu", need, N, plan->level_scratch_bytes);
            return GLOWHIP_EWORKSPACE;
        }
    }
    GH_TRY(run_forward(plan, packed, x_u8 ? w.bufA : x, noise, z, N, w, s, 0, rng.on ? &rng : nullptr, x_u8, divisor, snaps));
    GH_TRY(launch_top_logp(plan, z, prior_mean, prior_logs, prior_stride, N, w.acc, s));      // (the head's one launch when one is attached)
    if (snaps) GH_TRY(level_snapshot(plan, snaps, n_levels - 1, N, w, s));
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));      // the sum of the log|det W| terms enters here
    // objective = -ln(n_bins)*CHW + logdet + logp;  nll = -objective / (ln2 * CHW)   (network/model.py:425-450)
    const double chw = (double)plan->in_shape[0] * plan->in_shape[1] * plan->in_shape[2];
    const double offset = -log(pow(2.0, n_bits)) * chw;
    const double scale = -1.0 / (log(2.0) * chw);
    GH_TRY(launch_finalize(nullptr, w.acc, at<double>(packed, 0), 1.0, offset, scale, nll_out, objective_out, N, s, ACC_EXTRA));
    if (!snaps) return GLOWHIP_OK;
    // ONE launch for every level's term: the data-independent konst words of its FlowSteps (final behind join_lu) + the integer
    // difference of the snapshots that open and close it
    LevelKonst kt{};
    int level = 0; uint32_t ks = 0;
    for (const LayerPlan& L : plan->layers) {
        if (L.d.kind == GLOWHIP_LAYER_FLOWSTEP) kt.off8[ks++] = (uint32_t)(L.konst >> 3);
        else if (L.d.kind == GLOWHIP_LAYER_SPLIT2D) kt.first[++level] = ks;
    }
    kt.first[n_levels] = ks;
    count_launch(plan, "k_level_terms");
    return launch_level_terms(snaps, packed, kt, n_levels, N, plan->level_terms, s);
}

}  // namespace glowhip

// ================================================================================================ C ABI
extern "C" {

int glowhip_plan_timing_enable(glowhip_plan* plan, int enable) {
    GH_REQUIRE(plan, "plan_timing_enable: null plan");
    plan->timing = enable != 0;
    if (!enable) {
        for (hipEvent_t e : plan->ev_pool) (void)hipEventDestroy(e);
        for (TimingSlot& t : plan->ev_used) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
        plan->ev_pool.clear();
        plan->ev_used.clear();
    }
    return GLOWHIP_OK;
}

int glowhip_plan_timing_read(glowhip_plan* plan, glowhip_timing_record* out, int max, int* n_out) {
    GH_REQUIRE(plan && n_out, "plan_timing_read: null argument");
    int n = 0;
    for (TimingSlot& t : plan->ev_used) {
        if (hipEventSynchronize(t.b) != hipSuccess) { set_error("plan_timing_read: hipEventSynchronize failed"); return GLOWHIP_ELAUNCH; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, t.a, t.b);
        if (out && n < max) { out[n].kind = t.kind; out[n].layer = t.layer; out[n].mfma = t.mfma; out[n].ms = ms; ++n; }
        plan->ev_pool.push_back(t.a);
        plan->ev_pool.push_back(t.b);
    }
    plan->ev_used.clear();
    *n_out = n;
    return GLOWHIP_OK;
}

size_t glowhip_plan_workspace_bytes(const glowhip_plan* plan, int N) {
    return (plan && N >= 0) ? ws_layout(plan, N, nullptr, nullptr) : 0;
}

int glowhip_plan_output_shape(const glowhip_plan* plan, int reverse, int32_t out[3]) {
    GH_REQUIRE(plan && out, "plan_output_shape: null argument");
    for (int i = 0; i < 3; ++i) out[i] = reverse ? plan->in_shape[i] : plan->out_shape[i];
    return GLOWHIP_OK;
}

int glowhip_plan_set_dequant_rng(glowhip_plan* plan, unsigned long long seed, int enable, unsigned long long* next_call) {
    GH_REQUIRE(plan, "plan_set_dequant_rng: null plan");
    if (enable > 0) {
        if (plan->rng_seed != seed) plan->rng_calls = 0;      // a new seed restarts the stream; switching off and on again does not
        plan->rng_on = true; plan->rng_seed = seed;
    } else if (enable == 0) {
        plan->rng_on = false;
    }
    if (next_call) *next_call = plan->rng_calls;
    return GLOWHIP_OK;
}

int glowhip_plan_set_dequant_stream(glowhip_plan* plan, unsigned long long seed, unsigned long long call) {
    GH_REQUIRE(plan, "plan_set_dequant_stream: null plan");
    plan->rng_on = true; plan->rng_seed = seed; plan->rng_calls = call;
    return GLOWHIP_OK;
}

int glowhip_dequant_noise(float* out, long n, unsigned long long seed, unsigned long long call, int n_bits, glowhip_stream_t stream) {
    GH_REQUIRE(out && n >= 0 && n_bits > 0 && n_bits <= 30, "dequant_noise: bad argument");
    return launch_dequant_noise(out, n, seed, call, (float)(1.0 / pow(2.0, n_bits)), (hipStream_t)stream);
}

int glowhip_plan_describe(const glowhip_plan* plan, char* buf, size_t buf_bytes) {
    return glowhip_plan_describe_for(plan, 0, buf, buf_bytes);
}

int glowhip_plan_launch_counts(glowhip_plan* plan, char* buf, size_t buf_bytes, int reset) {
    GH_REQUIRE(plan && buf && buf_bytes > 0, "plan_launch_counts: null argument");
    std::string out;
    for (const auto& kv : plan->launch_counts) out += kv.first + "=" + std::to_string(kv.second) + "\n";
    GH_REQUIRE(out.size() < buf_bytes, "plan_launch_counts: buffer too small");
    snprintf(buf, buf_bytes, "%s", out.c_str());
    if (reset) plan->launch_counts.clear();
    return GLOWHIP_OK;
}

int glowhip_plan_describe_for(const glowhip_plan* plan, int N, char* buf, size_t buf_bytes) {
    GH_REQUIRE(plan && buf && buf_bytes > 0, "plan_describe: null argument");
    std::string sdesc;
    char line[256];
    int li = 0;
    for (const LayerPlan& L : plan->layers) {
        const glowhip_layer_desc& d = L.d;
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) snprintf(line, sizeof line, "%d squeeze C=%d H=%d W=%d\n", li, d.C, d.H, d.W);
        else if (d.kind == GLOWHIP_LAYER_FLOWSTEP)
        {
            if (dnet_runs(plan, L))
                snprintf(line, sizeof line, "%d flowstep C=%d H=%d W=%d hidden=%d f=dnet-sh2 (mix, f.0, f.2, f.4, finish: one launch per layer)\n", li, d.C,
                         d.H, d.W, d.hidden);
            else if (cnet_runs(plan, L))
                snprintf(line, sizeof line, "%d flowstep C=%d H=%d W=%d hidden=%d f=cnet-sh2 (f.0+f.2+f.4 one kernel + finish)\n", li, d.C, d.H,
                         d.W, d.hidden);
            else      // the exact-fp32 kernels, layer by layer
                snprintf(line, sizeof line, "%d flowstep C=%d H=%d W=%d hidden=%d f0=%s f2=%s f4=%s\n", li, d.C, d.H, d.W, d.hidden,
                         L.first_halo ? "mfma-halo" : (L.mfma_first ? "mfma" : "direct"), L.mfma_mid ? "mfma" : "direct",
                         L.mfma_last ? "mfma" : (L.wide_last ? "mfma-wide" : "direct"));
        }
        else snprintf(line, sizeof line, "%d split2d C=%d H=%d W=%d prior=%s\n", li, d.C, d.H, d.W,
                      L.mfma_last ? "mfma" : "direct");
        sdesc += line;
        ++li;
    }
    snprintf(buf, buf_bytes, "%s", sdesc.c_str());
    return GLOWHIP_OK;
}

int glowhip_normal_noise(float* out, long n, unsigned long long seed, unsigned long long call, int stream_id, float std,
                         glowhip_stream_t stream) {
    GH_REQUIRE(out && n >= 0, "normal_noise: bad argument");
    GH_REQUIRE(stream_id >= 0 && stream_id <= 254, "normal_noise: stream %d out of range (0 = top latent, 1 + k = Split2d k; at most 254 splits)", stream_id);
    GH_REQUIRE(call < (1ull << 56), "normal_noise: call numbers end at 2^56");
    return launch_normal_noise(out, n, seed, call, stream_id, std, (hipStream_t)stream);
}

int glowhip_plan_bind_sampler(glowhip_plan* plan, void* rng_dev, const float* std_split, int n_split, int advance) {
    GH_REQUIRE(plan, "plan_bind_sampler: null plan");
    if (!rng_dev) {
        plan->sampler_pos = nullptr; plan->sampler_std.clear(); plan->sampler_advance = false;
        return GLOWHIP_OK;
    }
    GH_REQUIRE(n_split == plan->n_split, "plan_bind_sampler: %d stds given, plan has %d Split2d layers", n_split, plan->n_split);
    GH_REQUIRE(n_split <= 254, "plan_bind_sampler: %d Split2d layers, the stream layout numbers at most 254", n_split);
    GH_REQUIRE(n_split == 0 || std_split, "plan_bind_sampler: null std list");
    GH_REQUIRE(((size_t)rng_dev & 7) == 0, "plan_bind_sampler: the position word must be 8-byte aligned");
    plan->sampler_pos = (unsigned long long*)rng_dev;
    plan->sampler_std.assign(std_split, std_split + n_split);
    plan->sampler_advance = advance != 0;
    return GLOWHIP_OK;
}

int glowhip_plan_bind_latents(glowhip_plan* plan, float* const* eps_out, int n_eps) {
    GH_REQUIRE(plan, "plan_bind_latents: null plan");
    if (!eps_out && n_eps == 0) {
        plan->eps_out.clear();
        return GLOWHIP_OK;
    }
    GH_REQUIRE(n_eps == plan->n_split, "plan_bind_latents: %d latent buffers given, plan has %d Split2d layers", n_eps, plan->n_split);
    GH_REQUIRE(eps_out, "plan_bind_latents: null buffer list");
    for (int k = 0; k < n_eps; ++k) GH_REQUIRE(eps_out[k], "plan_bind_latents: null buffer for Split2d #%d", k);
    plan->eps_out.assign(eps_out, eps_out + n_eps);
    return GLOWHIP_OK;
}

int glowhip_plan_status(const glowhip_plan* plan, const void* workspace, size_t workspace_bytes, int N, const float* result,
                        long elems_per_sample, int32_t* status_out, glowhip_stream_t stream) {
    GH_REQUIRE(plan && status_out, "plan_status: null argument");
    GH_REQUIRE(N >= 0 && N <= 65535, "batch size %d out of range", N);
    if (N == 0) return GLOWHIP_OK;
    Workspace w;
    GH_TRY(carve(plan, N, const_cast<void*>(workspace), workspace_bytes, w));
    return launch_status(w.acc, N, result, elems_per_sample, status_out, (hipStream_t)stream);
}

int glowhip_plan_encode(glowhip_plan* plan, const void* packed, const float* x, const float* noise,
                        const float* logdet_in, float* z, float* logdet_out, int N, void* workspace,
                        size_t workspace_bytes, glowhip_stream_t stream) {
    GH_TRY(check_plan_args(plan, packed, N));
    GH_REQUIRE(x && z, "plan_encode: null tensor");
    if (N == 0) return GLOWHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    GH_TRY(open_workspace(plan, N, workspace, workspace_bytes, w, s));
    GH_TRY(run_forward(plan, packed, x, noise, z, N, w, s));
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));
    if (logdet_out)
        GH_TRY(launch_finalize(logdet_in, w.acc, at<double>(packed, 0), 1.0, 0.0, 1.0, logdet_out, nullptr, N, s, ACC_EXTRA));
    return GLOWHIP_OK;
}

int glowhip_plan_decode(glowhip_plan* plan, const void* packed, const float* z, const float* const* eps, int n_eps,
                        const float* logdet_in, float* x, float* logdet_out, int N, void* workspace,
                        size_t workspace_bytes, glowhip_stream_t stream) {
    GH_TRY(check_plan_args(plan, packed, N));
    GH_REQUIRE(x && z, "plan_decode: null tensor");
    GH_REQUIRE(plan->sampler_pos || n_eps >= plan->n_split, "plan_decode: %d eps draws given, plan has %d Split2d layers", n_eps,
               plan->n_split);      // (with a sampler bound, the missing ones are drawn)
    if (N == 0) return GLOWHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    GH_TRY(open_workspace(plan, N, workspace, workspace_bytes, w, s));
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));      // decode reads W^-1 and the deep levels' images first
    int drawn = 0;
    GH_TRY(run_reverse(plan, packed, z, eps, n_eps, x, N, w, s, &drawn));
    if (logdet_out)
        GH_TRY(launch_finalize(logdet_in, w.acc, at<double>(packed, 0), -1.0, 0.0, 1.0, logdet_out, nullptr, N, s, ACC_EXTRA));
    return advance_sampler(plan, drawn, s);
}

int glowhip_plan_sample(glowhip_plan* plan, const void* packed, const float* z_top, const float* prior_mean, const float* prior_logs,
                        long prior_stride, float std_top, const float* const* eps, int n_eps, float* x, uint8_t* x_u8, float* z_out,
                        int N, void* workspace, size_t workspace_bytes, glowhip_stream_t stream) {
    GH_TRY(check_plan_args(plan, packed, N));
    GH_REQUIRE(x || x_u8, "plan_sample: no output (x and x_u8 are both null)");
    GH_REQUIRE(!x_u8 || (!plan->layers.empty() && plan->layers[0].d.kind == GLOWHIP_LAYER_SQUEEZE),
               "plan_sample: 8-bit output needs a plan that starts with a Squeeze2d layer");
    GH_REQUIRE(z_top || plan->sampler_pos, "plan_sample: no top latent given and no sampler bound (glowhip_plan_bind_sampler)");
    if (N == 0) return GLOWHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    GH_TRY(open_workspace(plan, N, workspace, workspace_bytes, w, s));
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));
    int drawn = 0;
    const long zchw = (long)plan->out_shape[0] * plan->out_shape[1] * plan->out_shape[2];
    const float* z = z_top;
    if (!z_top) {      // the top latent from the prior, into the caller's buffer or the workspace (where the decode's ping-pong begins)
        float* zb = z_out ? z_out : w.bufA;
        GH_TRY(launch_top_sample(plan, prior_mean, prior_logs, prior_stride, SamplerSpec{plan->sampler_pos, 0, std_top}, zb, N, s));
        z = zb;
        ++drawn;
    } else if (z_out && z_out != z_top) {
        GH_TRY(launch_copy_strided(z_top, zchw, z_out, zchw, N, zchw, s));
    }
    GH_TRY(run_reverse(plan, packed, z, eps, n_eps, x, N, w, s, &drawn, x_u8));
    return advance_sampler(plan, drawn, s);
}

int glowhip_glow_forward(glowhip_plan* plan, const void* packed, const float* x, const float* noise,
                         const float* prior_mean, const float* prior_logs, long prior_stride, int n_bits, float* z,
                         float* nll_out, float* objective_out, int N, void* workspace, size_t workspace_bytes,
                         glowhip_stream_t stream) {
    GH_TRY(check_plan_args(plan, packed, N));
    GH_REQUIRE(x && z && nll_out, "glow_forward: null tensor");
    GH_REQUIRE(n_bits > 0 && n_bits <= 30, "glow_forward: n_bits=%d", n_bits);
    if (N == 0) return GLOWHIP_OK;
    return glow_forward(plan, packed, x, nullptr, 1.f, noise, prior_mean, prior_logs, prior_stride, n_bits, z, nll_out, objective_out, N,
                        workspace, workspace_bytes, (hipStream_t)stream);
}

int glowhip_glow_forward_u8(glowhip_plan* plan, const void* packed, const uint8_t* x_u8, float divisor, const float* noise,
                            const float* prior_mean, const float* prior_logs, long prior_stride, int n_bits, float* z,
                            float* nll_out, float* objective_out, int N, void* workspace, size_t workspace_bytes,
                            glowhip_stream_t stream) {
    GH_TRY(check_plan_args(plan, packed, N));
    GH_REQUIRE(x_u8 && z && nll_out, "glow_forward_u8: null tensor");
    GH_REQUIRE(divisor > 0.f, "glow_forward_u8: divisor must be positive");
    GH_REQUIRE(n_bits > 0 && n_bits <= 30, "glow_forward_u8: n_bits=%d", n_bits);
    GH_REQUIRE(plan->layers.size() >= 2 && plan->layers[0].d.kind == GLOWHIP_LAYER_SQUEEZE,
               "glow_forward_u8: the plan must start with a Squeeze2d layer (and not end with it)");
    if (N == 0) return GLOWHIP_OK;
    return glow_forward(plan, packed, nullptr, x_u8, divisor, noise, prior_mean, prior_logs, prior_stride, n_bits, z, nll_out,
                        objective_out, N, workspace, workspace_bytes, (hipStream_t)stream);
}

int glowhip_plan_actnorm_init(glowhip_plan* plan, void* packed, size_t packed_bytes, const float* x, const float* noise,
                              float actnorm_scale, int N, void* workspace, size_t workspace_bytes,
                              glowhip_stream_t stream) {
    GH_TRY(check_plan_args(plan, packed, N));
    GH_REQUIRE(x && N > 0, "plan_actnorm_init: empty batch");
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    GH_TRY(open_workspace(plan, N, workspace, workspace_bytes, w, s));
    // plain (ActNorm-free) fp32 MFMA weight images of every convolution: the training family's + the init pass's own f.0 image
    // (no LU here: the invertible 1x1 convolutions are applied with W itself, and the pack at the end factorises them)
    GH_TRY(glowhip_plan_pack_for(plan, packed, packed_bytes, GLOWHIP_PACK_TRAINING | PACK_INIT_F0 | PACK_NO_LU, stream));
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));
    // Layer by layer: set the ActNorm statistics from the activations that reach it, refresh the packed
    // data of that layer, then run the layer forward with the fresh parameters (first training-mode
    // forward of the reference: network/module.py:45-46,66-67).
    const float* cur = x;
    const int nl = (int)plan->layers.size();
    for (int li = 0; li < nl; ++li) {
        LayerPlan& L = plan->layers[li];
        const glowhip_layer_desc& d = L.d;
        float* dst = other_buf(w, cur);
        const int HW = d.H * d.W;
        const long chw = (long)d.C * HW;
        const int Ch = d.C / 2;
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) {
            GH_TRY(launch_squeeze(cur, noise, dst, N, d.C, d.H, d.W, 2, 0, s));
            noise = nullptr;
        } else if (d.kind == GLOWHIP_LAYER_SPLIT2D) {
            GH_TRY(launch_copy_strided(cur, chw, dst, (long)Ch * HW, N, (long)Ch * HW, s));
        } else {
            if (noise) {
                GH_TRY(launch_squeeze(cur, noise, dst, N, d.C, d.H, d.W, 1, 0, s));
                cur = dst; dst = other_buf(w, cur); noise = nullptr;
            }
            const int hid = d.hidden;
            GH_TRY(launch_actnorm_init(cur, chw, N, d.C, HW, actnorm_scale, (float*)d.an_bias, (float*)d.an_logs, s));
            GH_TRY(pack_scales(d.an_logs, d.C, at<float>(packed, L.an_scale), at<float>(packed, L.an_inv_scale), s));
            ChanMixArgs m = chanmix_fwd_args(L, packed, N, cur, chw, dst);
            GH_TRY(launch_chanmix(m, s));
            // The statistics of a Conv2d's ActNorm are taken BETWEEN the convolution and the ActNorm (network/module.py:258-259,
            // 86-120), so the init pass needs the un-fused form -- not the slow one: raw convolution on the exact-fp32 MFMA kernels
            // (plain weight images packed above), statistics, then ActNorm + ReLU as one in-place pass.  The generic direct kernel
            // (two launches per convolution before) runs only for shapes no MFMA kernel takes.
            // f.0 (Conv2d's ActNorm uses scale 1, network/module.py:239)
            if (L.f0_init) {
                GH_TRY(launch_conv_mfma_wide(dst, chw, at<float>(packed, L.f0_init), nullptr, nullptr, w.h1, N, Ch, d.H, d.W, hid, 3, s, 0));
            } else {
                ConvArgs c0{dst, chw, d.f0_w, nullptr, nullptr, nullptr, nullptr, 0, w.h1, N, Ch, d.H, d.W, hid, 3};
                GH_TRY(launch_conv_direct(c0, s));
            }
            GH_TRY(launch_actnorm_init(w.h1, (long)hid * HW, N, hid, HW, 1.0f, (float*)d.f0_an_bias, (float*)d.f0_an_logs, s));
            GH_TRY(pack_scales(d.f0_an_logs, hid, at<float>(packed, L.f0_scale), nullptr, s));
            GH_TRY(launch_bias_scale_relu(w.h1, N, hid, HW, d.f0_an_bias, at<float>(packed, L.f0_scale), s));
            // f.2
            if (L.mfma_mid) {
                GH_TRY(launch_conv_mfma_wide(w.h1, (long)hid * HW, at<float>(packed, L.f2_wt), nullptr, nullptr, w.h2, N, hid, d.H, d.W,
                                             hid, 1, s, 0));
            } else {
                ConvArgs c2{w.h1, (long)hid * HW, d.f2_w, nullptr, nullptr, nullptr, nullptr, 0, w.h2, N, hid, d.H, d.W, hid, 1};
                GH_TRY(launch_conv_direct(c2, s));
            }
            GH_TRY(launch_actnorm_init(w.h2, (long)hid * HW, N, hid, HW, 1.0f, (float*)d.f2_an_bias, (float*)d.f2_an_logs, s));
            GH_TRY(pack_scales(d.f2_an_logs, hid, at<float>(packed, L.f2_scale), nullptr, s));
            GH_TRY(launch_bias_scale_relu(w.h2, N, hid, HW, d.f2_an_bias, at<float>(packed, L.f2_scale), s));
            // f.4 + coupling
            GH_TRY(pack_scales(d.f4_logs, L.Cout, at<float>(packed, L.f4_scale), nullptr, s));
            float* z2 = dst + (long)Ch * HW;
            if (L.mfma_last) {
                TailConvArgs t{};
                t.x = w.h2; t.x_bs = (long)hid * HW; t.wp = at<float>(packed, L.f4_wp); t.bias = d.f4_bias;
                t.scale = at<float>(packed, L.f4_scale);
                t.N = N; t.Cin = hid; t.H = d.H; t.W = d.W; t.Cout = L.Cout;
                t.mode = d.coupling == GLOWHIP_COUPLING_AFFINE ? TAIL_AFFINE_FWD : TAIL_ADD_FWD;
                t.z2_in = z2; t.z2_in_bs = chw; t.z2_out = z2; t.z2_out_bs = chw; t.acc = w.acc;     // (the log-det sums are not used)
                t.zeros = at<float>(packed, 64);
                GH_TRY(launch_conv_mfma_tail(t, s));
            } else {
                if (L.wide_last) {
                    const size_t out_f = (size_t)N * L.Cout * HW, h1_f = (size_t)N * plan->max_hidden;
                    GH_TRY(launch_conv_mfma_wide(w.h2, (long)hid * HW, at<float>(packed, L.f4_wt), d.f4_bias, at<float>(packed, L.f4_scale),
                                                 w.h1, N, hid, d.H, d.W, L.Cout, 3, s, 0, h1_f > out_f ? w.h1 + out_f : nullptr,
                                                 h1_f > out_f ? h1_f - out_f : 0));
                } else {
                    ConvArgs c4{w.h2, (long)hid * HW, d.f4_w, d.f4_bias, nullptr, nullptr, at<float>(packed, L.f4_scale), 0, w.h1,
                                N, hid, d.H, d.W, L.Cout, 3};
                    GH_TRY(launch_conv_direct(c4, s));
                }
                CouplingTailArgs t{w.h1, z2, chw, z2, chw, N, Ch, HW, d.coupling == GLOWHIP_COUPLING_AFFINE, 0, nullptr};
                GH_TRY(launch_coupling_tail(t, s));
            }
        }
        cur = dst;
    }
    // everything derived from the parameters is stale now: re-derive what the inference kernels read (log|det W| without W^-1:
    // the inverse and the training images are packed on demand by whoever decodes or trains next -- W^-1 of config E's 384 x 384
    // matrices alone costs more than the rest of the init pass)
    return glowhip_plan_pack_for(plan, packed, packed_bytes, GLOWHIP_PACK_INFERENCE, stream);
}

}  // extern "C"

// plan_build.hip -- what a flow plan IS and how its parameters are PACKED (host code only, no kernel).
// glowhip_plan_create validates the layer list, decides each layer's kernel routes, lays out the caller's `packed` buffer and builds
// the pack's job tables; glowhip_plan_pack_for selects the jobs of a use mask, keeps the tables in `packed` and launches the pack
// kernels (pack.hip, lu.hip, invconv_lu.hip).  The executor that reads the result is plan.hip (training: plan_train.hip).
#include "plan_internal.h"

namespace glowhip {

// a failed runtime call: its message, GLOWHIP_ELAUNCH
static int hip_failed(const char* what) { set_error("%s", what); return GLOWHIP_ELAUNCH; }

// ---------------------------------------------------------------- one builder per weight-image kind
// Each appends its RepackJob and derives K / Kpad / MT / total from the shape.  An image's source is a parameter tensor w or, w null,
// packed + w_off: a transposed copy (launch_flipT_batched) or W^-1.  Fold: the ActNorm behind the convolution, folded into the image;
// transposed: the image of the input-gradient convolution (RepackJob::transposed).
struct Fold { const float* bias = nullptr; const float* logs = nullptr; };
static RepackJob& add_job(glowhip_plan* p, int kind, const float* w, size_t w_off, size_t out_off, int Cin, int Cout, Fold fold, int use) {
    RepackJob r{};
    r.kind = kind; r.w = w; r.w_off = w_off; r.out_off = out_off; r.Cin = Cin; r.Cout = Cout; r.fold_bias = fold.bias; r.fold_logs = fold.logs; r.use = use;
    p->repack_jobs.push_back(r);
    return p->repack_jobs.back();
}
static void add_wide(glowhip_plan* p, const float* w, size_t out_off, int Cin, int Cout, int ksize, int use) {
    RepackJob& r = add_job(p, REPACK_WIDE, w, 0, out_off, Cin, Cout, Fold{}, use);
    r.K = Cin * ksize * ksize; r.Kpad = wide_kpad(Cin, ksize);
}
static void add_tail(glowhip_plan* p, const float* w, size_t out_off, int Cin, int Cout, int paired, int transposed, int use) {
    RepackJob& r = add_job(p, REPACK_TAIL, w, 0, out_off, Cin, Cout, Fold{}, use);
    r.paired = paired; r.MT = tail_mt(Cout, paired); r.total = (long)tail_chunks(Cin) * (TAIL_CK / 4) * 9 * r.MT * 64; r.transposed = transposed;
}
static void add_first(glowhip_plan* p, const float* w, size_t out_off, int Cin, int Cout, Fold fold, int transposed, int use) {
    add_job(p, REPACK_FIRST, w, 0, out_off, Cin, Cout, fold, use).transposed = transposed;
}
// the split-half images (sh.h SH2): a plain GEMM, a 3x3 convolution as (chunk, tap) implicit GEMM, k_cnet's last 3x3 convolution
static void add_sh2_gemm(glowhip_plan* p, const float* w, size_t w_off, size_t out_off, int Cin, int Cout, Fold fold, int kperm, int after_lu, int use) {
    RepackJob& r = add_job(p, REPACK_SH2_GEMM, w, w_off, out_off, Cin, Cout, fold, use);
    r.K = Cin; r.kperm = kperm; r.after_lu = after_lu;
}
static void add_sh2_first(glowhip_plan* p, const float* w, size_t w_off, size_t out_off, int Cin, int Cout, Fold fold, int use) {
    add_job(p, REPACK_SH2_FIRST, w, w_off, out_off, Cin, Cout, fold, use).K = cnet_g0(Cin);
}
static void add_sh2_tail(glowhip_plan* p, const float* w, size_t w_off, size_t out_off, int Cin, int Cout, int use) {
    RepackJob& r = add_job(p, REPACK_SH2_TAIL, w, w_off, out_off, Cin, Cout, Fold{}, use);
    r.Kpad = cnet_mpad4(Cout); r.kperm = 1;      // (always k-permuted: its B operand is f.2's accumulator block)
}

// ---------------------------------------------------------------- create, step 1: validation, kernel routes, layout of `packed`
// Each returns why the layer is refused (null: accepted).  The order of the take() calls is the layout of `packed`.
static const char* layout_flowstep(glowhip_plan* p, LayerPlan& L, size_t& off) {
    const glowhip_layer_desc& d = L.d;
    const int C = d.C, Ch = d.C / 2, H = d.H, W = d.W, hid = d.hidden;
    if (C % 2) return "FlowStep needs an even channel count";  // network/model.py:169
    if (hid <= 0) return "hidden_channels must be positive";
    if (!d.an_bias || !d.an_logs || !d.f0_w || !d.f0_an_bias || !d.f0_an_logs || !d.f2_w || !d.f2_an_bias || !d.f2_an_logs || !d.f4_w ||
        !d.f4_bias || !d.f4_logs)
        return "missing parameter pointer";
    if (d.permutation == GLOWHIP_PERM_INVCONV) {
        if (!d.invconv_w) return "missing invconv weight";
    } else if (d.permutation == GLOWHIP_PERM_GATHER) {
        if (!d.perm_idx || !d.perm_idx_inv) return "missing permutation tables";
    } else return "unknown permutation";
    if (d.coupling != GLOWHIP_COUPLING_ADDITIVE && d.coupling != GLOWHIP_COUPLING_AFFINE) return "unknown coupling";
    L.Cout = d.coupling == GLOWHIP_COUPLING_AFFINE ? C : C / 2;
    L.an_scale = take(off, (size_t)C * 4); L.an_inv_scale = take(off, (size_t)C * 4);
    L.winv = take(off, (size_t)C * C * 4); L.logabsdet = take(off, 4); L.konst = take(off, 8);
    L.lu_scratch = take(off, invconv_scratch_bytes(C));
    L.f0_scale = take(off, (size_t)hid * 4); L.f2_scale = take(off, (size_t)hid * 4); L.f4_scale = take(off, (size_t)L.Cout * 4);
    L.mfma_first = conv_mfma_wide_supported(Ch, H, W, hid, 3); L.mfma_mid = conv_mfma_wide_supported(hid, H, W, hid, 1);
    L.mfma_last = conv_mfma_tail_supported(hid, H, W, L.Cout); L.first_halo = conv_mfma_first_supported(Ch, H, W, hid);
    if (L.first_halo) L.f0_wt = take(off, conv_mfma_first_packed_bytes(Ch, hid));
    else if (L.mfma_first) L.f0_wt = take(off, conv_mfma_wide_packed_bytes(Ch, hid, 3));
    if (L.mfma_mid) L.f2_wt = take(off, conv_mfma_wide_packed_bytes(hid, hid, 1));
    if (L.first_halo && L.mfma_first) L.f0_init = take(off, conv_mfma_wide_packed_bytes(Ch, hid, 3));
    else if (L.mfma_first) L.f0_init = L.f0_wt;      // already the plain K-major image
    L.cnet = cnet_supported(Ch, H, W, hid, L.Cout);
    if (L.cnet) {
        L.cn_w0 = take(off, sh2_image_bytes(cnet_g0(Ch) * 8, hid)); L.cn_w2 = take(off, sh2_image_bytes(hid, hid));
        L.cn_w4 = take(off, cnet_w4_bytes(hid, L.Cout));
        p->max_hidden = std::max(p->max_hidden, (long)cnet_scratch_floats_per_sample(H, W, L.Cout));
        // the input-gradient chain on the same kernel: f.4^T is its first layer (Cin = Cout), f.0^T its last (Cout = C / 2)
        L.cnet_bwd = hid <= 512 && cnet_groups(Ch) == 1 && cnet_supported(L.Cout, H, W, hid, Ch);
    }
    if (L.cnet_bwd) {
        L.cb_w0 = take(off, sh2_image_bytes(cnet_g0(L.Cout) * 8, hid)); L.cb_w2 = take(off, sh2_image_bytes(hid, hid));
        L.cb_w4 = take(off, cnet_w4_bytes(hid, Ch));
        L.wt4 = take(off, (size_t)L.Cout * hid * 9 * 4); L.wt2 = take(off, (size_t)hid * hid * 4); L.wt0 = take(off, (size_t)hid * Ch * 9 * 4);
    }
    L.dnet = !L.cnet && d.permutation == GLOWHIP_PERM_INVCONV && dnet_supported(C, H, W, hid, L.Cout);
    if (L.dnet) {
        L.dn_mix = take(off, sh2_image_bytes(C, C)); L.dn_mixinv = take(off, sh2_image_bytes(C, C));
        L.dn_w0 = take(off, sh2_image_bytes(cnet_g0(Ch) * 8, hid)); L.dn_w2 = take(off, sh2_image_bytes(hid, hid));
        L.dn_w4 = take(off, sh2_image_bytes(cnet_g0(hid) * 8, L.Cout));
        p->max_hidden = std::max(p->max_hidden, (long)((dnet_scratch_bytes_per_sample(C, H, W, hid, L.Cout) + 3) / 4));
    }
    if (L.mfma_last) L.f4_wp = take(off, conv_mfma_tail_packed_bytes(hid, L.Cout));
    L.wide_last = !L.mfma_last && conv_mfma_wide_supported(hid, H, W, L.Cout, 3);
    if (L.wide_last) L.f4_wt = take(off, conv_mfma_wide_packed_bytes(hid, L.Cout, 3));
    L.dg4_first = conv_mfma_first_supported(L.Cout, H, W, hid);
    if (L.dg4_first) L.f4T_wf = take(off, conv_mfma_first_packed_bytes(L.Cout, hid));
    L.dg0_tail = conv_mfma_tail_supported(hid, H, W, Ch);
    if (L.dg0_tail) L.f0T_wp = take(off, conv_mfma_tail_packed_bytes(hid, Ch));
    p->max_hidden = std::max(p->max_hidden, (long)std::max(hid, L.Cout) * H * W);
    return nullptr;
}
static const char* layout_split(glowhip_plan* p, LayerPlan& L, size_t& off) {
    const glowhip_layer_desc& d = L.d;
    if (d.C % 2) return "Split2d needs an even channel count";
    if (!d.f4_w || !d.f4_bias || !d.f4_logs) return "missing conv2d_zeros parameter pointer";
    L.Cout = d.C;
    L.f4_scale = take(off, (size_t)d.C * 4);
    L.mfma_last = conv_mfma_tail_supported(d.C / 2, d.H, d.W, d.C);
    if (L.mfma_last) L.f4_wp = take(off, conv_mfma_tail_packed_bytes(d.C / 2, d.C));
    p->max_hidden = std::max(p->max_hidden, (long)d.C * d.H * d.W);
    L.split_idx = p->n_split++;
    return nullptr;
}
static bool layout_layers(glowhip_plan* p, const glowhip_layer_desc* layers, int n_layers, size_t& off) {
    int C = layers[0].C, H = layers[0].H, W = layers[0].W;
    p->in_shape[0] = C; p->in_shape[1] = H; p->in_shape[2] = W;
    for (int i = 0; i < n_layers; ++i) {
        LayerPlan L;
        L.d = layers[i];
        const glowhip_layer_desc& d = L.d;
        const char* why = d.C != C || d.H != H || d.W != W ? "input shape does not chain from the previous layer"
                          : d.C <= 0 || d.H <= 0 || d.W <= 0 ? "empty shape"
                          : d.kind == GLOWHIP_LAYER_SQUEEZE  ? (H % 2 || W % 2 ? "squeeze needs even H and W" : nullptr)
                          : d.kind == GLOWHIP_LAYER_FLOWSTEP ? layout_flowstep(p, L, off)
                          : d.kind == GLOWHIP_LAYER_SPLIT2D  ? layout_split(p, L, off) : "unknown layer kind";
        if (why) { set_error("plan_create: layer %d: %s (kind=%d C=%d H=%d W=%d)", i, why, d.kind, d.C, d.H, d.W); return false; }
        p->max_chw = std::max(p->max_chw, (long)C * H * W);
        if (d.kind == GLOWHIP_LAYER_SQUEEZE) { C *= 4; H /= 2; W /= 2; }
        else if (d.kind == GLOWHIP_LAYER_SPLIT2D) C /= 2;
        p->max_chw = std::max(p->max_chw, (long)C * H * W);
        p->layers.push_back(L);
    }
    p->out_shape[0] = C; p->out_shape[1] = H; p->out_shape[2] = W;
    return true;
}

// The range guarantee of the per-sample log-det accumulators (common.h RANGE) needs  2^14 P + 104 E < 2^31  per sample.  Both counts
// are fixed by the layer list.  P, workgroup partials of the Gaussian kernels: a Split2d's grid gives every workgroup its own
// elements of the dropped half -- 256 of them in k_split_tail, at least one 16-pixel tile of one channel in the two MFMA tails -- and
// the top prior is k_gaussian_logp's ceil(CHW / 256) workgroups (one, with a head attached).  E: the second half of every affine
// FlowStep.  The same bound holds for the decode, whose only terms are the coupling's.
static const char* acc_budget(const glowhip_plan* p) {
    double P = 0.0, E = 0.0;
    for (const LayerPlan& L : p->layers) {
        const double half = (double)(L.d.C / 2) * L.d.H * L.d.W;
        if (L.d.kind == GLOWHIP_LAYER_FLOWSTEP && L.d.coupling == GLOWHIP_COUPLING_AFFINE) E += half;
        else if (L.d.kind == GLOWHIP_LAYER_SPLIT2D) P += ceil(half / (L.mfma_last ? 16.0 : 256.0));
    }
    P += ceil((double)p->out_shape[0] * p->out_shape[1] * p->out_shape[2] / 256.0);
    return FIX_COARSE_MIN * P + FIX_COUPLING_TERM_MAX * E < 2147483648.0
               ? nullptr : "the per-sample log-det accumulator cannot hold this many terms (common.h RANGE)";
}

// ---------------------------------------------------------------- create, step 2: the pack's job tables
// The order of the pushes is kept: a pack's selection (select_jobs) is a stable filter of repack_jobs, and the one-launch pack's
// segment table indexes into that.
static void flowstep_jobs(glowhip_plan* p, const LayerPlan& L) {
    const glowhip_layer_desc& d = L.d;
    const int Ch = d.C / 2, hid = d.hidden, INF = GLOWHIP_PACK_INFERENCE, TRAIN = GLOWHIP_PACK_TRAINING;
    p->prep_jobs.push_back(StepPrepJob{d.permutation == GLOWHIP_PERM_INVCONV ? d.invconv_w : nullptr, d.an_logs, d.C, d.H * d.W, L.winv, L.logabsdet,
                                       L.konst, L.lu_scratch, 0});
    for (const ScaleJob& sj : {ScaleJob{d.an_logs, L.an_scale, L.an_inv_scale, d.C, 1}, ScaleJob{d.f0_an_logs, L.f0_scale, 0, hid, 0},
                               ScaleJob{d.f2_an_logs, L.f2_scale, 0, hid, 0}, ScaleJob{d.f4_logs, L.f4_scale, 0, L.Cout, 0}})
        p->scale_jobs.push_back(sj);
    // the exact-fp32 images: the training path's, and the inference calls' -- which read those of a layer that runs k_cnet or the
    // deep-level kernels only under the family switches
    const int fp32 = TRAIN | ((L.cnet || L.dnet) ? PACK_EXACT_FP32 : INF);
    if (L.first_halo) add_first(p, d.f0_w, L.f0_wt, Ch, hid, Fold{d.f0_an_bias, d.f0_an_logs}, /*transposed*/ 0, fp32);
    else if (L.mfma_first) add_wide(p, d.f0_w, L.f0_wt, Ch, hid, /*ksize*/ 3, fp32);
    if (L.first_halo && L.f0_init) add_wide(p, d.f0_w, L.f0_init, Ch, hid, /*ksize*/ 3, PACK_INIT_F0);      // read by the data-dependent init pass only
    if (L.mfma_mid) add_wide(p, d.f2_w, L.f2_wt, hid, hid, /*ksize*/ 1, fp32);
    if (L.cnet) {
        add_sh2_first(p, d.f0_w, 0, L.cn_w0, Ch, hid, Fold{d.f0_an_bias, d.f0_an_logs}, INF | TRAIN);
        add_sh2_gemm(p, d.f2_w, 0, L.cn_w2, hid, hid, Fold{d.f2_an_bias, d.f2_an_logs}, /*kperm*/ 1, /*after_lu*/ 0, INF | TRAIN);
        const int ng = cnet_groups(L.Cout), cg = L.Cout / ng;       // one image per group of f.4 output channels
        for (int gi = 0; gi < ng; ++gi)
            add_sh2_tail(p, d.f4_w + (size_t)gi * cg * hid * 9, 0, L.cn_w4 + gi * sh2_image_bytes(hid, cnet_mpad4(cg)), hid, cg, INF | TRAIN);
    }
    if (L.dnet) {      // deep levels: the mixer as a GEMM image (W; W^-1 after the LU), f.0 / f.4 as (chunk, tap) images, f.2
        add_sh2_gemm(p, d.invconv_w, 0, L.dn_mix, d.C, d.C, Fold{}, /*kperm*/ 0, /*after_lu*/ 0, INF);
        add_sh2_gemm(p, nullptr, L.winv, L.dn_mixinv, d.C, d.C, Fold{}, /*kperm*/ 0, /*after_lu*/ 1, GLOWHIP_PACK_INVERSE);
        add_sh2_first(p, d.f0_w, 0, L.dn_w0, Ch, hid, Fold{d.f0_an_bias, d.f0_an_logs}, INF);
        add_sh2_gemm(p, d.f2_w, 0, L.dn_w2, hid, hid, Fold{d.f2_an_bias, d.f2_an_logs}, /*kperm*/ 0, /*after_lu*/ 0, INF);
        add_sh2_first(p, d.f4_w, 0, L.dn_w4, hid, L.Cout, Fold{}, INF);
    }
    if (L.cnet_bwd) {      // (training only) transposed copies, then the same three image kinds over them
        p->flip_jobs.push_back(FlipJob{d.f4_w, L.wt4, L.Cout, hid, 9});     // wt4[k][co][8 - tap] = W4[co][k][tap]
        p->flip_jobs.push_back(FlipJob{d.f2_w, L.wt2, hid, hid, 1});        // wt2[i][o] = W2[o][i]
        p->flip_jobs.push_back(FlipJob{d.f0_w, L.wt0, hid, Ch, 9});         // wt0[ci][k][8 - tap] = W0[k][ci][tap]
        const int th = (hid + 31) / 32;
        p->flip_tiles[0] = std::max(p->flip_tiles[0], th * ((L.Cout + 31) / 32));
        p->flip_tiles[1] = std::max(p->flip_tiles[1], th * th);
        p->flip_tiles[2] = std::max(p->flip_tiles[2], th * ((Ch + 31) / 32));
        add_sh2_first(p, nullptr, L.wt4, L.cb_w0, L.Cout, hid, Fold{nullptr, d.f2_an_logs}, TRAIN);      // g_u2 = g_h2 (h2 > 0) exp(3 logs2)
        add_sh2_gemm(p, nullptr, L.wt2, L.cb_w2, hid, hid, Fold{nullptr, d.f0_an_logs}, /*kperm*/ 1, /*after_lu*/ 0, TRAIN);
        add_sh2_tail(p, nullptr, L.wt0, L.cb_w4, hid, Ch, TRAIN);
    }
    if (L.mfma_last) add_tail(p, d.f4_w, L.f4_wp, hid, L.Cout, /*paired*/ d.coupling == GLOWHIP_COUPLING_AFFINE, /*transposed*/ 0, fp32);
    if (L.wide_last) add_wide(p, d.f4_w, L.f4_wt, hid, L.Cout, /*ksize*/ 3, fp32);
    // input gradients: of f.4 = 3x3 conv Cout -> hidden with w[ci][o][8-tap], of f.0 = 3x3 conv hidden -> C/2
    if (L.dg4_first) add_first(p, d.f4_w, L.f4T_wf, L.Cout, hid, Fold{}, /*transposed*/ 1, TRAIN);
    if (L.dg0_tail) add_tail(p, d.f0_w, L.f0T_wp, hid, Ch, /*paired*/ 0, /*transposed*/ 1, TRAIN);
}
static void split_jobs(glowhip_plan* p, const LayerPlan& L) {
    p->scale_jobs.push_back(ScaleJob{L.d.f4_logs, L.f4_scale, 0, L.Cout, 0});
    if (L.mfma_last) add_tail(p, L.d.f4_w, L.f4_wp, L.d.C / 2, L.Cout, /*paired*/ 1, /*transposed*/ 0, GLOWHIP_PACK_INFERENCE | GLOWHIP_PACK_TRAINING);
}
// the widest matrices left to the pack's factorisations (the LDS kernel takes C <= 64): LU-form layers have w == null
static void lu_widths(glowhip_plan* p) {
    p->max_lds_c = p->max_c = 0;
    for (const StepPrepJob& j : p->prep_jobs)
        if (j.w) { p->max_c = std::max(p->max_c, j.C); if (j.C <= 64) p->max_lds_c = std::max(p->max_lds_c, j.C); }
}

// ---------------------------------------------------------------- create, step 3: the tables' own room at the end of `packed`
// which workgroups of the one-launch pack (k_pack_fused) take a repack job
static int seg_kind(const RepackJob& r) { return r.kind < REPACK_SH2_GEMM ? PACKSEG_LEGACY : PACKSEG_SH2_GEMM + (r.kind - REPACK_SH2_GEMM); }
static void layout_tables(glowhip_plan* p, size_t& off) {
    p->prep_off = take(off, p->prep_jobs.size() * sizeof(StepPrepJob));
    p->scale_off = take(off, p->scale_jobs.size() * sizeof(ScaleJob));
    // one slot of selected repack jobs per combination of the use bits that select images (repack_slot): a pack of one mask never
    // rewrites the table a captured graph of another mask launches over
    p->repack_off = take(off, REPACK_SLOTS * p->repack_jobs.size() * sizeof(RepackJob));
    p->flip_off = take(off, p->flip_jobs.size() * sizeof(FlipJob));
    // room for the LU-form job table (glowhip_plan_bind_invconv_lu comes after the caller sized `packed`): one per invconv FlowStep
    size_t n_inv = 0;
    for (const StepPrepJob& pj : p->prep_jobs) n_inv += pj.w ? 1 : 0;
    p->lu_off = take(off, n_inv * sizeof(LuJob));
    // the one-launch forward pack's table (k_pack_fused): an arrival counter, then at most one PackSeg per block of every job
    size_t nseg = (p->prep_jobs.size() + 3) / 4 + 1;
    for (const RepackJob& r : p->repack_jobs) nseg += pack_fused_job_blocks(seg_kind(r), &r, nullptr);
    for (const ScaleJob& sj : p->scale_jobs) nseg += pack_fused_job_blocks(PACKSEG_SCALE, nullptr, &sj);
    p->seg_cap = nseg;
    p->seg_off = take(off, PACK_SEG_HEAD + nseg * sizeof(PackSeg));
}

// ---------------------------------------------------------------- the steps of a pack
// Step 1: the repack jobs of a use mask, into plan->repack_sel, sorted by kind group (each image kernel is launched over its own jobs
// only): 0 the exact-fp32 ("legacy") kinds, 1..3 SH2 GEMM / FIRST / TAIL, 4 the SH2 GEMM images of W^-1 (after the LU, on its stream)
struct PackSel { int n_kind[5] = {0, 0, 0, 0, 0}, tail_blocks = 1, first_blocks = 2; };
static PackSel select_jobs(glowhip_plan* plan, int use) {
    PackSel sel;
    plan->repack_sel.clear();
    auto group = [](const RepackJob& r) { return r.after_lu ? 4 : (r.kind < REPACK_SH2_GEMM ? 0 : r.kind - REPACK_SH2_GEMM + 1); };
    for (int gk = 0; gk < 5; ++gk)
        for (const RepackJob& r : plan->repack_jobs)
            if ((r.use & use) && group(r) == gk) {
                plan->repack_sel.push_back(r);
                ++sel.n_kind[gk];
                if (gk == 3) sel.tail_blocks = std::max(sel.tail_blocks, (r.Cout + 7) / 8);
                if (gk == 2 && r.Cin >= 64) sel.first_blocks = std::max(sel.first_blocks, std::min(16, (r.Cout + 31) / 32));
            }
    return sel;
}

static bool upload(void* packed, size_t off, const void* src, size_t bytes, hipStream_t s) {
    return bytes == 0 || hipMemcpyAsync((char*)packed + off, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
}
// Step 2.  The job tables are plan constants: they travel once per buffer -- the selected repack jobs once per (buffer, image bits of
// the use mask), each mask into its OWN slot -- and stay in `packed` (re-sent for a new buffer because `packed` is caller memory): a
// re-pack of the same buffer is then kernel launches only (no host-to-device copy per step, and the sequence can be captured in a
// hipGraph whose table no later pack of another mask -- a training step, the exact-fp32 fall-back, the init pass -- overwrites).
static int send_tables(glowhip_plan* plan, void* packed, int slot, size_t slot_off, hipStream_t s) {
    if (plan->tables_in != packed) {
        if (!upload(packed, plan->prep_off, plan->prep_jobs.data(), plan->prep_jobs.size() * sizeof(StepPrepJob), s) ||
            !upload(packed, plan->scale_off, plan->scale_jobs.data(), plan->scale_jobs.size() * sizeof(ScaleJob), s) ||
            !upload(packed, plan->flip_off, plan->flip_jobs.data(), plan->flip_jobs.size() * sizeof(FlipJob), s) ||
            !upload(packed, plan->lu_off, plan->lu_jobs.data(), plan->lu_jobs.size() * sizeof(LuJob), s))
            return hip_failed("plan_pack: hipMemcpyAsync of the job tables failed");
        plan->tables_in = packed; plan->slots_in = 0; plan->segs_in = false;
    }
    if (!(plan->slots_in & (1u << slot))) {
        // (hipMemcpyAsync from pageable memory stages the source before it returns; the per-slot host copy is kept anyway)
        std::vector<RepackJob>& keep = plan->repack_slot_host[slot];
        keep = plan->repack_sel;
        if (!upload(packed, slot_off, keep.data(), keep.size() * sizeof(RepackJob), s))
            return hip_failed("plan_pack: hipMemcpyAsync of the repack job table failed");
        plan->slots_in |= 1u << slot;
    }
    return GLOWHIP_OK;
}
// Step 3: the one-launch pack's segment table, indices into the repack table of THIS slot (repack_sel of this use mask).  Today one
// mask only takes the one launch, so it is a plan constant; it is keyed by the slot all the same: a pack of another slot rebuilds
// it and sends it again, and never launches over job indices of another selection.
static void build_segments(glowhip_plan* plan, const PackSel& sel) {
    std::vector<PackSeg>& t = plan->pack_segs;
    t.clear();
    auto add = [&t](int kind, int jn, int nb) { for (int b = 0; b < nb; ++b) t.push_back(PackSeg{kind, jn, b, nb}); };
    auto add_repack = [&](int jn) { const RepackJob& r = plan->repack_sel[jn]; add(seg_kind(r), jn, pack_fused_job_blocks(seg_kind(r), &r, nullptr)); };
    for (int b = 0; b < ((int)plan->prep_jobs.size() + 3) / 4; ++b) t.push_back(PackSeg{PACKSEG_LU, 0, b, 1});
    // repack_sel lists the legacy kinds first; the launch takes SH2 GEMM, FIRST, TAIL (such a pack has no W^-1 image), then them
    for (int jn = sel.n_kind[0]; jn < (int)plan->repack_sel.size(); ++jn) add_repack(jn);
    for (int jn = 0; jn < sel.n_kind[0]; ++jn) add_repack(jn);
    for (int jn = 0; jn < (int)plan->scale_jobs.size(); ++jn) add(PACKSEG_SCALE, jn, pack_fused_job_blocks(PACKSEG_SCALE, nullptr, &plan->scale_jobs[jn]));
    add(PACKSEG_ZERO, 0, 1);
}
static int send_segments(glowhip_plan* plan, void* packed, const PackSel& sel, int slot, hipStream_t s) {
    GH_REQUIRE(sel.n_kind[4] == 0, "plan_pack: the one-launch pack takes no W^-1 image");      // (build_segments walks repack_sel as SH2 | legacy)
    if (plan->pack_segs.empty() || plan->pack_segs_slot != slot) {
        build_segments(plan, sel);
        plan->pack_segs_slot = slot; plan->segs_in = false;
    }
    GH_REQUIRE(plan->pack_segs.size() <= plan->seg_cap, "plan_pack: segment table larger than its slot");
    if (plan->segs_in) return GLOWHIP_OK;
    static const char zero_head[PACK_SEG_HEAD] = {0};
    if (!upload(packed, plan->seg_off, zero_head, PACK_SEG_HEAD, s) ||
        !upload(packed, plan->seg_off + PACK_SEG_HEAD, plan->pack_segs.data(), plan->pack_segs.size() * sizeof(PackSeg), s))
        return hip_failed("plan_pack: hipMemcpyAsync of the segment table failed");
    plan->segs_in = true;
    return GLOWHIP_OK;
}
// Step 4, the fork: the legacy-kind images and the LU factorisations go to the plan's side stream (created on first use; a host
// resource like the timing events) behind everything enqueued so far; whoever reads their results joins (join_legacy / join_lu).
// What the first kernels of a forward need -- scale tables, the product kernels' images -- stays on `s`.  Only where it pays: plans
// with invertible 1x1 convolutions beyond 128 channels (blocked LU in global memory, 2.4 ms per pack at config E: +5 % on its
// forward).  At config B the side stream's workgroups only get in the way of the k_cnet launch beside them (-0.5 %): *side is s.
static int fork_side(glowhip_plan* plan, hipStream_t s, hipStream_t* side) {
    *side = s;
    if (debug_switches().pack_one_stream || plan->max_c <= 128) return GLOWHIP_OK;
    if (!plan->side && (hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking) != hipSuccess ||
                        hipEventCreateWithFlags(&plan->ev_fork, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&plan->ev_legacy, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&plan->ev_lu, hipEventDisableTiming) != hipSuccess))
        return hip_failed("plan_pack: could not create the side stream / events");
    *side = plan->side;
    if (hipEventRecord(plan->ev_fork, s) != hipSuccess || hipStreamWaitEvent(*side, plan->ev_fork, 0) != hipSuccess)
        return hip_failed("plan_pack: fork onto the side stream failed");
    return GLOWHIP_OK;
}
// ... and what the consumers join through: ev_legacy / ev_lu recorded on the side stream, its pending flag set (nothing without a fork)
static int mark_side(glowhip_plan* plan, hipEvent_t ev, bool* pending, hipStream_t side, hipStream_t s) {
    if (side == s) return GLOWHIP_OK;
    if (hipEventRecord(ev, side) != hipSuccess) return hip_failed("plan_pack: hipEventRecord failed");
    *pending = true; plan->pending_captured = stream_capturing(s);
    return GLOWHIP_OK;
}
// Step 5: log|det W| (inv: and W^-1) of every matrix the pack factorises, then what is built from W^-1
static int launch_lu(glowhip_plan* plan, void* packed, int use, const PackSel& sel, size_t slot_off, bool all_small, hipStream_t side) {
    const bool inv = (use & (GLOWHIP_PACK_INVERSE | GLOWHIP_PACK_TRAINING)) != 0;
    count_launch(plan, (all_small && !inv) ? "pack:k_step_prepare_small" : "pack:k_step_prepare_batched");
    if (!(all_small && !inv)) {      // which factorisation each matrix takes there (tallied first: at most five map updates per pack)
        std::map<const char*, long> routes;
        for (const StepPrepJob& pj : plan->prep_jobs)
            if (pj.w) ++routes[step_prepare_route_name(pj.C, inv ? 1 : 0)];
        for (const auto& kv : routes) plan->launch_counts[kv.first] += kv.second;
    }
    GH_TRY(launch_step_prepare_batched(at<StepPrepJob>(packed, plan->prep_off), (int)plan->prep_jobs.size(), plan->max_lds_c, packed, side,
                                       inv, plan->max_c, all_small ? 1 : 0));
    if (!(use & GLOWHIP_PACK_INVERSE)) return GLOWHIP_OK;
    // W^-1 of the LU-form layers by substitution -- for decode only: the backward sweep does not read it (their GradJob has no
    // W^-1 term), so a training pack without GLOWHIP_PACK_INVERSE skips it
    if (!plan->lu_jobs.empty())
        GH_TRY(launch_invconv_lu_inverse(at<LuJob>(packed, plan->lu_off), nullptr, (int)plan->lu_jobs.size(), plan->lu_max_c, packed, side));
    if (sel.n_kind[4] > 0)
        GH_TRY(launch_repack_sh2_gemm(at<RepackJob>(packed, slot_off) + (sel.n_kind[0] + sel.n_kind[1] + sel.n_kind[2] + sel.n_kind[3]),
                                      sel.n_kind[4], packed, side));
    return GLOWHIP_OK;
}

}  // namespace glowhip

// ================================================================================================ C ABI
extern "C" {

glowhip_plan* glowhip_plan_create(const glowhip_layer_desc* layers, int n_layers) {
    if (!layers || n_layers <= 0) { set_error("plan_create: empty layer list"); return nullptr; }
    glowhip_plan* p = new glowhip_plan();
    size_t off = 0;
    take(off, 256);  // offset 0: plan-wide data-independent log-det total (fp64); offset 64..127: zero block for LDS-DMA padding
    if (!layout_layers(p, layers, n_layers, off)) { delete p; return nullptr; }
    if (const char* why = acc_budget(p)) { set_error("plan_create: %s", why); delete p; return nullptr; }
    for (const LayerPlan& L : p->layers)
        if (L.d.kind == GLOWHIP_LAYER_FLOWSTEP) flowstep_jobs(p, L);
        else if (L.d.kind == GLOWHIP_LAYER_SPLIT2D) split_jobs(p, L);
    lu_widths(p);
    layout_tables(p, off);
    p->packed_bytes = align_up(off, 256);
    return p;
}

void glowhip_plan_destroy(glowhip_plan* plan) {
    if (!plan) return;
    if (plan->side) {      // (the side stream may still be writing into the caller's `packed` buffer)
        (void)hipStreamSynchronize(plan->side);
        (void)hipEventDestroy(plan->ev_fork); (void)hipEventDestroy(plan->ev_legacy); (void)hipEventDestroy(plan->ev_lu);
        (void)hipStreamDestroy(plan->side);
    }
    for (hipEvent_t e : plan->ev_pool) (void)hipEventDestroy(e);
    for (TimingSlot& t : plan->ev_used) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    delete plan;
}

size_t glowhip_plan_packed_bytes(const glowhip_plan* plan) { return plan ? plan->packed_bytes : 0; }

int glowhip_plan_set_family(glowhip_plan* plan, int family) {
    GH_REQUIRE(plan, "plan_set_family: null plan");
    GH_REQUIRE(family == GLOWHIP_FAMILY_AUTO || family == GLOWHIP_FAMILY_EXACT_FP32, "plan_set_family: unknown family %d", family);
    plan->family = family;
    return GLOWHIP_OK;
}

int glowhip_plan_get_family(const glowhip_plan* plan) { return plan ? plan->family : GLOWHIP_EINVAL; }

int glowhip_plan_bind_invconv_lu(glowhip_plan* plan, int layer, const glowhip_invconv_lu* lu) {
    GH_REQUIRE(plan && lu, "plan_bind_invconv_lu: null argument");
    GH_REQUIRE(layer >= 0 && layer < (int)plan->layers.size(), "plan_bind_invconv_lu: layer %d out of range", layer);
    const LayerPlan& L = plan->layers[layer];
    const glowhip_layer_desc& d = L.d;
    GH_REQUIRE(d.kind == GLOWHIP_LAYER_FLOWSTEP && d.permutation == GLOWHIP_PERM_INVCONV, "plan_bind_invconv_lu: layer %d is not an invconv FlowStep", layer);
    GH_REQUIRE(lu->perm && lu->l && lu->u && lu->log_s && lu->sign_s && lu->w, "plan_bind_invconv_lu: null pointer");
    GH_REQUIRE(lu->w == d.invconv_w, "plan_bind_invconv_lu: w must be the buffer the layer's invconv_w points at");
    GH_REQUIRE(d.C <= INVCONV_LU_MAX_C, "plan_bind_invconv_lu: C=%d unsupported (limit %d)", d.C, INVCONV_LU_MAX_C);
    for (const glowhip_plan::LuLayer& q : plan->lu_layers) GH_REQUIRE(q.layer != layer, "plan_bind_invconv_lu: layer %d is bound already", layer);
    int pj = 0;      // the layer's step-prepare job: FlowSteps in layer order
    for (int i = 0; i < layer; ++i) pj += plan->layers[i].d.kind == GLOWHIP_LAYER_FLOWSTEP ? 1 : 0;
    plan->prep_jobs[pj].w = nullptr; plan->prep_jobs[pj].lu_form = 1;
    lu_widths(plan);      // what is left for the factorisations
    plan->lu_jobs.push_back(LuJob{lu->perm, lu->l, lu->u, lu->log_s, lu->sign_s, lu->w, d.an_logs, d.C, d.H * d.W, L.winv, L.logabsdet, L.konst,
                                  nullptr, nullptr});
    plan->lu_layers.push_back(glowhip_plan::LuLayer{layer, glowhip_invconv_lu_grads{nullptr, nullptr, nullptr}});
    plan->lu_max_c = std::max(plan->lu_max_c, d.C);
    plan->lu_grad_jobs.reserve(plan->lu_jobs.size());
    // the tables in `packed` and the one-launch pack's segment table were built for the plan as it was
    plan->tables_in = nullptr; plan->slots_in = 0; plan->segs_in = false; plan->pack_segs.clear(); plan->pack_segs_slot = -1;
    return GLOWHIP_OK;
}

int glowhip_plan_bind_invconv_lu_grads(glowhip_plan* plan, int layer, const glowhip_invconv_lu_grads* grads) {
    GH_REQUIRE(plan, "plan_bind_invconv_lu_grads: null plan");
    for (glowhip_plan::LuLayer& q : plan->lu_layers)
        if (q.layer == layer) {
            GH_REQUIRE(!grads || (grads->dl && grads->du && grads->dlog_s), "plan_bind_invconv_lu_grads: null gradient pointer");
            q.g = grads ? *grads : glowhip_invconv_lu_grads{nullptr, nullptr, nullptr};
            return GLOWHIP_OK;
        }
    set_error("plan_bind_invconv_lu_grads: layer %d is not an LU-form layer", layer);
    return GLOWHIP_EINVAL;
}

int glowhip_plan_pack(glowhip_plan* plan, void* packed, size_t packed_bytes, glowhip_stream_t stream) {
    return glowhip_plan_pack_for(plan, packed, packed_bytes, GLOWHIP_PACK_INFERENCE | GLOWHIP_PACK_TRAINING | GLOWHIP_PACK_INVERSE, stream);
}

int glowhip_plan_pack_for(glowhip_plan* plan, void* packed, size_t packed_bytes, int use, glowhip_stream_t stream) {
    GH_REQUIRE(plan && packed, "plan_pack: null argument");
    GH_REQUIRE(use & (GLOWHIP_PACK_INFERENCE | GLOWHIP_PACK_TRAINING), "plan_pack: empty use mask");
    // with the split-half path switched off through the debug hook, the inference calls read the exact-fp32 images of every layer
    // (OR-ed in: PACK_INIT_F0 and PACK_NO_LU of the caller's mask survive)
    if (debug_switches().exact_fp32) use |= GLOWHIP_PACK_INFERENCE | GLOWHIP_PACK_TRAINING | PACK_EXACT_FP32;
    // a plan on the exact-fp32 family reads the fp32 MFMA images, which are the training path's
    if (plan->family == GLOWHIP_FAMILY_EXACT_FP32) use |= GLOWHIP_PACK_TRAINING;
    const PackSel sel = select_jobs(plan, use);
    GH_REQUIRE(packed_bytes >= plan->packed_bytes, "plan_pack: packed buffer too small (%zu < %zu)", packed_bytes, plan->packed_bytes);
    hipStream_t s = (hipStream_t)stream;
    GH_TRY(join_legacy(plan, s)); GH_TRY(join_lu(plan, s));      // (a previous pack's side-stream part writes the same buffer)
    bool all_small = !debug_switches().lu_workgroup;      // every factorisation of the pack is a one-wave job
    for (const StepPrepJob& pj : plan->prep_jobs) all_small = all_small && step_prepare_small_takes(pj);
    // The forward-only pack of a plan whose LU jobs are all one-wave jobs and that keeps everything on one stream is ONE launch
    // (pack.hip k_pack_fused); every other pack -- inverse, training, wide plans, the init pass -- is the launch sequence below.
    // (the debug switch picks the launches only: the table travels either way, so the two routes leave the same bytes in `packed`)
    const bool fusable = use == GLOWHIP_PACK_INFERENCE && plan->max_c <= 128 && sel.n_kind[4] == 0 && all_small;
    const bool fused = fusable && !debug_switches().pack_unfused;
    if (!fused && hipMemsetAsync(packed, 0, 256, s) != hipSuccess) return hip_failed("plan_pack: hipMemsetAsync failed");
    const int slot = repack_slot(use);
    const size_t slot_off = plan->repack_off + (size_t)slot * plan->repack_jobs.size() * sizeof(RepackJob);
    GH_TRY(send_tables(plan, packed, slot, slot_off, s));
    // LU-form layers first, on the caller's stream and ahead of the fork: W = P L U_f into the layer's own buffer (the mixers and the
    // deep levels' weight images read it) and the layer's log-det and constant slots, which the step-prepare kernels below then
    // leave alone (StepPrepJob::lu_form) and their totals read
    if (!plan->lu_jobs.empty()) {
        plan->launch_counts["pack:invconv_lu"] += (long)plan->lu_jobs.size();
        GH_TRY(launch_invconv_lu_assemble(at<LuJob>(packed, plan->lu_off), nullptr, (int)plan->lu_jobs.size(), plan->lu_max_c, packed, s));
    }
    if (fusable) GH_TRY(send_segments(plan, packed, sel, slot, s));
    if (fused) {
        count_launch(plan, "pack:k_pack_fused");
        return launch_pack_fused(at<PackSeg>(packed, plan->seg_off + PACK_SEG_HEAD), (int)plan->pack_segs.size(),
                                 at<StepPrepJob>(packed, plan->prep_off), (int)plan->prep_jobs.size(), at<RepackJob>(packed, slot_off),
                                 at<ScaleJob>(packed, plan->scale_off), at<unsigned>(packed, plan->seg_off), packed, s);
    }
    hipStream_t side;
    GH_TRY(fork_side(plan, s, &side));
    if (use & GLOWHIP_PACK_TRAINING)      // transposed weight copies for the backward k_cnet images (read by the image kernels below)
        GH_TRY(launch_flipT_batched(at<FlipJob>(packed, plan->flip_off), (int)plan->flip_jobs.size(), plan->flip_tiles, packed, s));
    GH_TRY(launch_pack_batched(at<ScaleJob>(packed, plan->scale_off), (int)plan->scale_jobs.size(), at<RepackJob>(packed, slot_off),
                               sel.n_kind, sel.tail_blocks, packed, s, side, sel.first_blocks));
    GH_TRY(mark_side(plan, plan->ev_legacy, &plan->legacy_pending, side, s));
    if (!(use & PACK_NO_LU)) GH_TRY(launch_lu(plan, packed, use, sel, slot_off, all_small, side));      // (the init pass' first pack: none)
    return mark_side(plan, plan->ev_lu, &plan->lu_pending, side, s);
}

int glowhip_plan_pack_sync(glowhip_plan* plan) {
    GH_REQUIRE(plan, "plan_pack_sync: null plan");
    if (plan->side && (plan->legacy_pending || plan->lu_pending)) {
        if (hipStreamSynchronize(plan->side) != hipSuccess) return hip_failed("plan_pack_sync: hipStreamSynchronize failed");
        plan->legacy_pending = plan->lu_pending = false;
    }
    return GLOWHIP_OK;
}

int glowhip_plan_forget_packed(glowhip_plan* plan) {
    GH_REQUIRE(plan, "plan_forget_packed: null plan");
    plan->tables_in = nullptr; plan->slots_in = 0; plan->segs_in = false;
    return GLOWHIP_OK;
}

}  // extern "C"

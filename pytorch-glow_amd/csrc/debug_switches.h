// debug_switches.h -- the process-wide testing switches behind glowhip_debug_force_tail_tile (include/glowhip.h, GLOWHIP_DBG_*).
// One instance, written only by that hook (api.hip), which decodes its integer straight into these fields; the kernel-selection
// code reads debug_switches().field.  Every field says what it switches ON and defaults to the automatic choice.
// Process-wide and not thread safe: a testing hook, not part of the operator surface.
#pragma once

namespace glowhip {

struct DebugSwitches {
    // ---- fused tail convolution (conv_mfma_tail.hip)
    int tail_tile = 0;               // pixels per workgroup: 0 automatic (cost model), else 16 / 32 / 64 / 128
    int tail_msplit = -1;            // out-channel tiles over blockIdx.y: -1 automatic, 0 never, 1 always
    bool tail_no_dma = false;        // register-staged tail kernels only
    // ---- executor and pack (plan.hip, plan_train.hip; the pack switches: plan_build.hip)
    bool exact_fp32 = false;         // the split-half path off: every coupling network on the exact-fp32 MFMA kernels, training included
    bool no_mixer_fusion = false;    // no mixer of the next step inside the finishing kernel, no squeeze folded into a mixer
    bool lu_workgroup = false;       // log|det W| of the small matrices on the workgroup-wide LU (A/B and bitwise test of the one-wave form)
    bool pack_one_stream = false;    // glowhip_plan_pack without the side-stream fork
    bool pack_unfused = false;       // the forward-only pack as its per-kind launch sequence, not k_pack_fused (A/B, byte comparison)
    bool train_per_layer_fwd = false;   // the training forward on the per-layer kernels (no taping k_cnet)
    bool train_per_layer_bwd = false;   // the input-gradient chain on the per-layer kernels (no backward k_cnet)
    // ---- k_cnet / k_cnet1w / k_cfinish (cnet_sh.hip)
    int cnet_rows = 0;               // row splits of k_cnet: 0 automatic, else 1 / 2 / 4
    bool cnet_128_only = false;      // 128-pixel tiles wherever they exist
    bool cnet_64 = false;            // 64-pixel tiles wherever they exist
    bool cfinish_block_order = false;   // the finishing kernel takes its pixel chunks in block order, not the XCD-affine order
    bool no_cnet1w = false;          // no k_cnet1w (one wave per SIMD): k_cnet takes its launches
    bool no_cnet1w_bwd = false;      // no backward instance of k_cnet1w
    // ---- weight gradients (wgrad_mfma.hip)
    bool wgrad_narrow = false;       // f.2's weight-gradient GEMM on 128-column tiles everywhere
};

const DebugSwitches& debug_switches();

}  // namespace glowhip

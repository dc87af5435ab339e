// api.hip -- extern "C" entry points of the single-layer primitives + error plumbing.
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>

#include "kernels.h"
#include "conv_mfma.h"
#include "cnet_geo.h"
#include "invconv_lu.h"
#include "debug_switches.h"

namespace glowhip {
static DebugSwitches g_debug;      // written by glowhip_debug_force_tail_tile alone
const DebugSwitches& debug_switches() { return g_debug; }

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace glowhip

using namespace glowhip;

extern "C" {

int glowhip_version(void) { return GLOWHIP_VERSION; }
void glowhip_debug_force_tail_tile(int v) {
    auto bit = [v](int flag) { return (v & flag) != 0; };
    DebugSwitches d;
    d.tail_tile = v & GLOWHIP_DBG_TAIL_TILE_MASK;
    d.tail_msplit = bit(GLOWHIP_DBG_TAIL_MSPLIT) ? 1 : (bit(GLOWHIP_DBG_TAIL_NO_MSPLIT) ? 0 : -1);
    d.tail_no_dma = bit(GLOWHIP_DBG_TAIL_NO_DMA);
    d.exact_fp32 = bit(GLOWHIP_DBG_EXACT_FP32);
    d.no_mixer_fusion = bit(GLOWHIP_DBG_NO_MIXER_FUSION);
    d.no_cnet1w = bit(GLOWHIP_DBG_NO_CNET1W);
    d.no_cnet1w_bwd = bit(GLOWHIP_DBG_NO_CNET1W_BWD);
    d.wgrad_narrow = bit(GLOWHIP_DBG_WGRAD_NARROW);
    d.lu_workgroup = bit(GLOWHIP_DBG_LU_WORKGROUP);
    d.cnet_rows = (v >> GLOWHIP_DBG_CNET_ROWS_SHIFT) & 7;
    d.cnet_128_only = bit(GLOWHIP_DBG_CNET_128_ONLY);
    d.cnet_64 = bit(GLOWHIP_DBG_CNET_64);
    d.cfinish_block_order = bit(GLOWHIP_DBG_CFINISH_BLOCK_ORDER);
    d.pack_one_stream = bit(GLOWHIP_DBG_PACK_ONE_STREAM);
    d.pack_unfused = bit(GLOWHIP_DBG_PACK_UNFUSED);
    d.train_per_layer_fwd = bit(GLOWHIP_DBG_TRAIN_PER_LAYER_FWD);
    d.train_per_layer_bwd = bit(GLOWHIP_DBG_TRAIN_PER_LAYER_BWD);
    g_debug = d;
}
const char* glowhip_last_error(void) { return g_err; }

int glowhip_squeeze2d(const float* x, float* y, int N, int C, int H, int W, int factor, int reverse,
                      glowhip_stream_t stream) {
    GH_REQUIRE(x && y, "squeeze2d: null tensor");
    GH_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, "squeeze2d: bad shape");
    return launch_squeeze(x, nullptr, y, N, C, H, W, factor, reverse, (hipStream_t)stream);
}

int glowhip_actnorm_init(const float* x, long batch_stride, int N, int C, int HW, float scale, float* bias, float* logs,
                         glowhip_stream_t stream) {
    GH_REQUIRE(x && bias && logs, "actnorm_init: null tensor");
    return launch_actnorm_init(x, batch_stride, N, C, HW, scale, bias, logs, (hipStream_t)stream);
}

int glowhip_actnorm_init_batch_variance(const float* x, long batch_stride, int N, int C, int HW, float scale, float* bias,
                                        float* logs, glowhip_stream_t stream) {
    GH_REQUIRE(x && bias && logs, "actnorm_init: null tensor");
    return launch_actnorm_init(x, batch_stride, N, C, HW, scale, bias, logs, (hipStream_t)stream, 1);
}

// ActNorm.forward as a stand-alone elementwise pass (network/module.py:122-149)
__global__ void __launch_bounds__(256) k_actnorm_elementwise(const float* __restrict__ x, float* __restrict__ y,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ logs, long total, int C, int HW,
                                                             int reverse) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / HW) % C);
    const float l3 = logs[c] * LOGSCALE;
    y[i] = reverse ? (x[i] * expf(-l3) - bias[c]) : ((x[i] + bias[c]) * expf(l3));
}

int glowhip_actnorm(const float* x, float* y, const float* bias, const float* logs, int N, int C, int HW, int reverse,
                    const float* logdet_in, float* logdet_out, glowhip_stream_t stream) {
    GH_REQUIRE(x && y && bias && logs, "actnorm: null tensor");
    GH_REQUIRE(N >= 0 && C > 0 && C <= 4096 && HW > 0, "actnorm: bad shape N=%d C=%d HW=%d", N, C, HW);
    hipStream_t s = (hipStream_t)stream;
    if (logdet_out)
        GH_TRY(launch_add_const_logdet(logdet_in, logdet_out, N, logs, LOGSCALE * (float)HW, C, reverse ? -1.f : 1.f, s));
    if (N == 0) return GLOWHIP_OK;
    long total = (long)N * C * HW;
    hipLaunchKernelGGL(k_actnorm_elementwise, dim3(cdiv(total, 256)), dim3(256), 0, s, x, y, bias, logs, total, C, HW,
                       reverse);
    GH_LAUNCH_CHECK("k_actnorm_elementwise");
    return GLOWHIP_OK;
}

size_t glowhip_invconv_scratch_bytes(int C) { return C > 0 ? invconv_scratch_bytes(C) : 0; }

int glowhip_invconv_prepare(const float* w, int C, float* winv, float* logabsdet, void* scratch,
                            glowhip_stream_t stream) {
    GH_REQUIRE(w, "invconv_prepare: null weight");
    return launch_invconv_prepare(w, C, winv, logabsdet, scratch, (hipStream_t)stream);
}

int glowhip_invconv_lu_prepare(const int32_t* perm, const float* l, const float* u, const float* log_s, const float* sign_s, int C,
                               float* w_out, float* winv_out, float* logabsdet_out, glowhip_stream_t stream) {
    GH_REQUIRE(perm && l && u && log_s && sign_s && w_out, "invconv_lu_prepare: null argument");
    GH_REQUIRE(C > 0 && C <= INVCONV_LU_MAX_C, "invconv_lu_prepare: C=%d unsupported", C);
    LuJob j{};
    j.perm = perm; j.l = l; j.u = u; j.log_s = log_s; j.sign_s = sign_s; j.w = w_out; j.C = C; j.HW = 1;
    j.winv = winv_out; j.logabsdet = logabsdet_out;
    GH_TRY(launch_invconv_lu_assemble(nullptr, &j, 1, C, nullptr, (hipStream_t)stream));
    if (winv_out) GH_TRY(launch_invconv_lu_inverse(nullptr, &j, 1, C, nullptr, (hipStream_t)stream));
    return GLOWHIP_OK;
}

int glowhip_invconv_lu_backward(const int32_t* perm, const float* l, const float* u, const float* log_s, const float* sign_s, int C,
                                const float* dW, double logdet_term, float* dl, float* du, float* dlog_s, glowhip_stream_t stream) {
    GH_REQUIRE(perm && l && u && log_s && sign_s && dW && dl && du && dlog_s, "invconv_lu_backward: null argument");
    GH_REQUIRE(C > 0 && C <= INVCONV_LU_MAX_C, "invconv_lu_backward: C=%d unsupported", C);
    LuGradJob j{perm, l, u, log_s, sign_s, dW, dl, du, dlog_s, C, nullptr, logdet_term};
    return launch_invconv_lu_backward(nullptr, &j, 1, C, (hipStream_t)stream);
}

int glowhip_invconv(const float* x, float* y, const float* m, const float* logabsdet, int N, int C, int HW, int reverse,
                    const float* logdet_in, float* logdet_out, glowhip_stream_t stream) {
    GH_REQUIRE(x && y && m, "invconv: null tensor");
    GH_REQUIRE(x != y, "invconv: in-place call not supported");
    hipStream_t s = (hipStream_t)stream;
    if (logdet_out) {
        GH_REQUIRE(logabsdet, "invconv: logdet requested without logabsdet");
        GH_TRY(launch_add_const_logdet(logdet_in, logdet_out, N, logabsdet, (float)HW, 1, reverse ? -1.f : 1.f, s));
    }
    ChanMixArgs a{};
    const long chw = (long)C * HW;
    a.in_a = x; a.in_a_bs = chw; a.in_b = x; a.in_b_bs = chw; a.Ca = C;
    a.out = y; a.out_bs = chw; a.matrix = m; a.reverse = 0; a.N = N; a.C = C; a.HW = HW;
    return launch_chanmix(a, s);
}

int glowhip_permute_channels(const float* x, float* y, const int32_t* idx, int N, int C, int HW,
                             glowhip_stream_t stream) {
    GH_REQUIRE(x && y && idx, "permute_channels: null tensor");
    GH_REQUIRE(x != y, "permute_channels: in-place call not supported");
    ChanMixArgs a{};
    const long chw = (long)C * HW;
    a.in_a = x; a.in_a_bs = chw; a.in_b = x; a.in_b_bs = chw; a.Ca = C;
    a.out = y; a.out_bs = chw; a.gather = idx; a.reverse = 0; a.N = N; a.C = C; a.HW = HW;
    return launch_chanmix(a, (hipStream_t)stream);
}

int glowhip_conv2d(const float* x, long x_batch_stride, const float* w, const float* bias, float* y, int N, int Cin,
                   int H, int W, int Cout, int ksize, const float* post_bias, const float* post_logs, int relu,
                   glowhip_stream_t stream) {
    GH_REQUIRE(x && w && y, "conv2d: null tensor");
    ConvArgs a{x, x_batch_stride, w, bias, post_bias, post_logs, nullptr, relu, y, N, Cin, H, W, Cout, ksize};
    return launch_conv_direct(a, (hipStream_t)stream);
}

int glowhip_gaussian_logp(const float* x, long x_stride, const float* mean, const float* logs, long ml_stride, int N,
                          int C, int HW, const float* in, float* out, void* scratch16N, glowhip_stream_t stream) {
    if (N == 0) return GLOWHIP_OK;      // (an empty batch has no storage: its pointers may be null)
    GH_REQUIRE(x && out && scratch16N, "gaussian_logp: null argument");
    // P = ceil(C HW / 256) workgroup partials per sample: 2^14 P < 2^31 (common.h RANGE)
    GH_REQUIRE(FIX_COARSE_MIN * (double)cdiv((long)C * HW, 256) < 2147483648.0, "gaussian_logp: %ld elements per sample are more than the "
               "accumulator's range guarantee covers", (long)C * HW);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* acc = (unsigned long long*)scratch16N;
    GH_TRY(launch_zero_acc(acc, N, s));
    GH_TRY(launch_gaussian_logp(x, x_stride, mean, logs, ml_stride, N, C, HW, acc, s));
    return launch_finalize(in, acc, nullptr, 1.0, 0.0, 1.0, out, nullptr, N, s);
}

// one weight image through the plan's own image kernel (launch_pack_batched on a one-job table); waits for the stream, since the
// table is freed here
static int debug_conv_image(RepackJob r, float* image, hipStream_t s) {
    RepackJob* dev = nullptr;
    GH_REQUIRE(hipMalloc((void**)&dev, sizeof(RepackJob)) == hipSuccess, "debug_conv: no device memory for the job table");
    const int n_kind[4] = {1, 0, 0, 0};
    int rc = hipMemcpy(dev, &r, sizeof(RepackJob), hipMemcpyHostToDevice) == hipSuccess
                 ? launch_pack_batched(nullptr, 0, dev, n_kind, 0, image, s, s) : GLOWHIP_ELAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess && rc == GLOWHIP_OK) rc = GLOWHIP_ELAUNCH;
    (void)hipFree(dev);
    return rc;
}

// Testing hook (include/glowhip.h): one launch of an exact-fp32 convolution launcher on the caller's operands.  No second path: it
// decodes the probe, builds the weight image with the plan's repack job, calls the launcher the plan calls, and copies what the
// launcher reported.
int glowhip_debug_conv(const glowhip_conv_probe* d, glowhip_conv_info* info, glowhip_stream_t stream) {
    GH_REQUIRE(d && info, "debug_conv: null probe / info");
    hipStream_t s = (hipStream_t)stream;
    *info = glowhip_conv_info{};
    ConvLaunchInfo li{};
    auto report = [&]() {
        info->kernel = li.kernel; info->ksize = li.ksize; info->tile = li.tile; info->splits = li.splits; info->mb = li.mb;
        info->grid[0] = li.grid[0]; info->grid[1] = li.grid[1]; info->grid[2] = li.grid[2]; info->launches = li.launches;
    };
    GH_REQUIRE(d->N >= 0 && d->Cin > 0 && d->Cout > 0 && d->H > 0 && d->W > 0, "debug_conv: bad shape");
    GH_REQUIRE(d->x_bs >= (int64_t)d->Cin * d->H * d->W, "debug_conv: batch stride below one sample");
    switch (d->op) {
    case GLOWHIP_CONV_WIDE: {
        GH_REQUIRE(conv_mfma_wide_supported(d->Cin, d->H, d->W, d->Cout, d->ksize), "conv_mfma_wide: unsupported shape");
        // transposed (1x1 only): w is the forward weight (Cin, Cout), which in its reference layout already is the K-major image of the
        // input-gradient GEMM -- the training sweep passes it to the launcher as it is, and so does the hook (no image, no repack)
        GH_REQUIRE(!d->transposed || d->ksize == 1, "debug_conv: the wide image has a transposed source form for 1x1 only");
        info->image_bytes = d->transposed ? 0 : (int64_t)conv_mfma_wide_packed_bytes(d->Cin, d->Cout, d->ksize);
        if (!d->image && !d->transposed) return GLOWHIP_OK;
        GH_REQUIRE(d->x && d->w && d->y && d->scratch_floats >= 0, "debug_conv: wide null operand / output");
        const float* wt = d->w;
        if (!d->transposed) {
            RepackJob r{};
            r.kind = REPACK_WIDE; r.w = d->w; r.Cin = d->Cin; r.Cout = d->Cout;
            r.K = d->Cin * d->ksize * d->ksize; r.Kpad = wide_kpad(d->Cin, d->ksize);
            GH_TRY(debug_conv_image(r, d->image, s));
            wt = d->image;
        }
        GH_TRY(launch_conv_mfma_wide(d->x, (long)d->x_bs, wt, d->post_bias, d->post_scale, d->y, d->N, d->Cin, d->H, d->W, d->Cout,
                                     d->ksize, s, d->relu, d->scratch, (size_t)d->scratch_floats, &li));
        report();
        return GLOWHIP_OK;
    }
    case GLOWHIP_CONV_FIRST: {
        GH_REQUIRE(conv_mfma_first_supported(d->Cin, d->H, d->W, d->Cout), "conv_mfma_first: unsupported shape");
        GH_REQUIRE(!d->fold_bias == !d->fold_logs, "debug_conv: the folded ActNorm is a bias and a logs table, or neither");
        info->image_bytes = (int64_t)conv_mfma_first_packed_bytes(d->Cin, d->Cout);
        if (!d->image) return GLOWHIP_OK;
        GH_REQUIRE(d->x && d->w && d->y, "debug_conv: first null operand / output");
        RepackJob r{};
        r.kind = REPACK_FIRST; r.w = d->w; r.Cin = d->Cin; r.Cout = d->Cout; r.fold_bias = d->fold_bias; r.fold_logs = d->fold_logs;
        r.transposed = d->transposed ? 1 : 0;
        GH_TRY(debug_conv_image(r, d->image, s));
        GH_TRY(launch_conv_mfma_first(d->x, (long)d->x_bs, d->image, d->image + (size_t)9 * d->Cin * d->Cout, d->y, d->N, d->Cin, d->H, d->W,
                                      d->Cout, s, d->relu, &li));
        report();
        return GLOWHIP_OK;
    }
    case GLOWHIP_CONV_DIRECT: {
        GH_REQUIRE(d->x && d->w && d->y, "debug_conv: direct null operand / output");
        ConvArgs a{d->x, (long)d->x_bs, d->w, d->bias, d->post_bias, d->post_logs, d->post_scale, d->relu, d->y, d->N, d->Cin, d->H, d->W,
                   d->Cout, d->ksize};
        GH_TRY(launch_conv_direct(a, s, &li));
        report();
        return GLOWHIP_OK;
    }
    case GLOWHIP_CONV_TAIL: {
        GH_REQUIRE(d->mode >= TAIL_PLAIN && d->mode <= TAIL_SPLIT_REV, "debug_conv: unknown tail mode %d", d->mode);
        GH_REQUIRE(conv_mfma_tail_supported(d->Cin, d->H, d->W, d->Cout), "conv_mfma_tail: unsupported shape");
        const int paired = tail_paired(d->mode);
        GH_REQUIRE(!paired || d->Cout % 2 == 0, "conv_mfma_tail: paired mode needs an even Cout");
        info->image_bytes = (int64_t)conv_mfma_tail_packed_bytes(d->Cin, d->Cout);
        if (!d->image) return GLOWHIP_OK;
        const long chw = (long)(paired ? d->Cout / 2 : d->Cout) * d->H * d->W;
        GH_REQUIRE(d->x && d->w && (d->z2_in || d->mode == TAIL_PLAIN) && (d->z2_out || d->mode == TAIL_SPLIT_FWD), "debug_conv: tail null operand / output");
        GH_REQUIRE((!d->z2_in || d->z2_in_bs >= chw) && (!d->z2_out || d->z2_out_bs >= chw), "debug_conv: tail batch stride below one sample");
        GH_REQUIRE(!d->acc == !d->term, "debug_conv: the accumulator and its finalised term come together");
        GH_REQUIRE(!d->zeros || ((size_t)d->zeros & 15) == 0, "debug_conv: the zero block is 16-byte aligned");
        TailConvArgs a{};
        a.x = d->x; a.x_bs = (long)d->x_bs; a.wp = d->image; a.bias = d->bias; a.scale = d->post_scale;
        a.N = d->N; a.Cin = d->Cin; a.H = d->H; a.W = d->W; a.Cout = d->Cout; a.mode = d->mode;
        a.z2_in = d->z2_in; a.z2_in_bs = (long)d->z2_in_bs; a.z2_out = d->z2_out; a.z2_out_bs = (long)d->z2_out_bs;
        a.acc = (unsigned long long*)d->acc; a.zeros = d->zeros; a.hout = d->hout;
        GH_TRY(conv_mfma_tail_check(a));
        GH_TRY(conv_mfma_tail_pack(d->w, d->Cin, d->Cout, paired, d->image, s));
        if (d->acc) GH_TRY(launch_zero_acc(a.acc, d->N, s));
        GH_TRY(launch_conv_mfma_tail(a, s, &li));
        if (d->acc) GH_TRY(launch_finalize(nullptr, a.acc, nullptr, 1.0, 0.0, 1.0, d->term, nullptr, d->N, s));
        report();
        info->paired = li.paired;
        return GLOWHIP_OK;
    }
    default: break;
    }
    GH_REQUIRE(false, "debug_conv: unknown op %d", d->op);
    return GLOWHIP_EINVAL;
}

// Testing hook (include/glowhip.h): one launch of the finishing kernel, the channel mixer or the deep levels' FIN / PREP on the
// caller's operands.  No second path: it decodes the probe, derives the tiling with the producer's own code, calls the launcher the
// plan calls, and copies what the launcher reported.
int glowhip_debug_fin(const glowhip_fin_probe* d, glowhip_fin_info* info, glowhip_stream_t stream) {
    GH_REQUIRE(d && info, "debug_fin: null probe / info");
    hipStream_t s = (hipStream_t)stream;
    *info = glowhip_fin_info{};
    FinLaunchInfo li{};
    auto report = [&]() {
        info->kernel = li.kernel; info->grid[0] = li.grid[0]; info->grid[1] = li.grid[1]; info->grid[2] = li.grid[2];
        info->lds_bytes = li.lds_bytes; info->pxb = li.pxb; info->msv = li.msv; info->halo = li.halo; info->xcd_affine = li.xcd_affine;
        info->stage_matrix = li.stage_matrix;
    };
    GH_REQUIRE(d->N > 0 && d->C > 0, "debug_fin: bad shape N=%d C=%d", d->N, d->C);
    switch (d->op) {
    case GLOWHIP_FIN_CFINISH: {
        GH_REQUIRE(d->mode >= TAIL_AFFINE_FWD && d->mode <= TAIL_ADD_REV, "debug_fin: coupling modes only (mode %d)", d->mode);
        const bool paired = d->mode == TAIL_AFFINE_FWD || d->mode == TAIL_AFFINE_REV;
        GH_REQUIRE(d->C % 2 == 0 && d->Cout == (paired ? d->C : d->C / 2), "debug_fin: Cout=%d does not fit C=%d in mode %d", d->Cout, d->C, d->mode);
        GH_REQUIRE(d->tile == 64 || d->tile == 128, "debug_fin: k_cnet tiles are 64 or 128 pixels (tile %d)", d->tile);
        GH_REQUIRE(d->MS == 1 || d->MS == 2 || d->MS == 4, "debug_fin: row split %d", d->MS);
        GH_REQUIRE(d->H > 0 && d->W > 0, "debug_fin: bad map");
        CnetGeo g;
        GH_REQUIRE(cnet_geo(d->C / 2, d->H, d->W, d->hidden, d->Cout, d->N, d->tile, &g), "cnet: unsupported shape");
        CnetPending p{};
        cnet_pending_tiling(g, d->MS, &p);
        info->R = p.R; info->NI = p.NI; info->tiles = p.tiles; info->lpxt = p.lpxt;
        info->scratch_floats = (int64_t)cnet_scratch_floats(d->N, d->H, d->W, d->Cout);
        if (!d->scratch) return GLOWHIP_OK;
        const long chw = (long)d->C * d->H * d->W;
        GH_REQUIRE(d->scratch_floats >= info->scratch_floats, "debug_fin: scratch below the plan's %ld floats", (long)info->scratch_floats);
        GH_REQUIRE(d->bias && d->scale && d->z_in && d->z_out && d->acc, "debug_fin: cfinish null operand / output");
        GH_REQUIRE(d->z_in_bs >= chw && d->z_out_bs >= chw, "debug_fin: batch stride below one sample");
        GH_REQUIRE(d->mix_C == 0 || (d->mix_bias && d->mix_scale), "debug_fin: a mixer has its ActNorm tables");
        GH_REQUIRE(!(d->mix_matrix && d->mix_gather), "debug_fin: a mixer is a matrix, a gather or neither");
        p.scratch = d->scratch; p.bias = d->bias; p.scale = d->scale; p.mode = d->mode; p.Cout = d->Cout; p.z = d->z_in; p.z_bs = (long)d->z_in_bs;
        CnetArgs a{};
        a.N = d->N; a.Cin = d->C / 2; a.H = d->H; a.W = d->W; a.hidden = d->hidden; a.Cout = d->Cout; a.mode = d->mode;
        a.z_in = d->z_in; a.z_in_bs = (long)d->z_in_bs; a.z_out = d->z_out; a.z_out_bs = (long)d->z_out_bs;
        a.acc = (unsigned long long*)d->acc; a.tape_hout = d->tape_hout;
        a.mix = CnetMixer{d->mix_C, d->mix_reverse, d->mix_bias, d->mix_scale, d->mix_matrix, d->mix_gather};
        GH_TRY(launch_cnet_finish(a, p, s, &li));
        report();
        return GLOWHIP_OK;
    }
    case GLOWHIP_FIN_CHANMIX: {
        GH_REQUIRE(d->HW > 0 && d->Ca >= 0 && d->Ca <= d->C, "debug_fin: chanmix bad shape");
        GH_REQUIRE(d->out && (d->sq_src || ((d->in_a || d->Ca == 0) && (d->in_b || d->Ca == d->C))), "debug_fin: chanmix null operand / output");
        GH_REQUIRE(!d->mix_bias == !d->mix_scale, "debug_fin: the ActNorm is a bias and a scale table, or neither");
        GH_REQUIRE(!(d->mix_matrix && d->mix_gather), "debug_fin: a mixer is a matrix, a gather or neither");
        GH_REQUIRE(d->out_bs >= (long)d->C * d->HW && (d->sq_src || ((d->Ca == 0 || d->in_a_bs >= (long)d->Ca * d->HW) &&
                   (d->Ca == d->C || d->in_b_bs >= (long)(d->C - d->Ca) * d->HW))), "debug_fin: batch stride below one sample");
        GH_REQUIRE(!d->sq_src || (d->sq_W > 0 && d->sq_W % 2 == 0 && d->HW % (d->sq_W / 2) == 0 && (d->sq_bs == 0 || d->sq_bs >= (long)d->C * d->HW) &&
                                  (!d->sq_u8 || d->sq_div > 0.f)), "debug_fin: bad squeezed view");
        ChanMixArgs a{};
        // (a half without channels is never read: it gets the other half's valid address, as the plan passes one tensor twice)
        a.in_a = d->in_a ? d->in_a : d->in_b; a.in_a_bs = (long)d->in_a_bs; a.in_b = d->in_b ? d->in_b : d->in_a; a.in_b_bs = (long)d->in_b_bs; a.Ca = d->Ca;
        a.out = d->out; a.out_bs = (long)d->out_bs; a.bias = d->mix_bias; a.scale = d->mix_scale; a.matrix = d->mix_matrix; a.gather = d->mix_gather;
        a.reverse = d->mix_reverse; a.N = d->N; a.C = d->C; a.HW = d->HW;
        a.sq_src = d->sq_src; a.sq_u8 = d->sq_u8; a.sq_div = d->sq_div; a.sq_noise = d->sq_noise; a.sq_W = d->sq_W; a.sq_bs = (long)d->sq_bs;
        a.sq_rng = RngSpec{d->rng_on, (unsigned long long)d->rng_seed, (unsigned long long)d->rng_call, d->rng_scale};
        if (a.sq_src) { a.in_a = a.in_b = reinterpret_cast<const float*>(d->sq_src); }      // (pointers the kernel forms but never reads)
        GH_TRY(launch_chanmix(a, s, &li));
        report();
        return GLOWHIP_OK;
    }
    case GLOWHIP_FIN_DN_FIN:
    case GLOWHIP_FIN_DN_PREP: {
        GH_REQUIRE(d->H > 0 && d->W > 0 && dnet_supported(d->C, d->H, d->W, d->hidden, d->Cout), "dnet: unsupported shape");
        DnetLevel L{d->N, d->C, d->H, d->W, d->hidden, d->Cout, d->state, (long)d->z_in_bs, d->dn_scratch};
        DnetScratchLayout lay;
        dnet_scratch_layout(L, &lay);
        info->part_off = lay.part_off; info->u_off = lay.u_off; info->ypad_off = lay.ypad_off; info->u_plane = lay.u_plane; info->ypad_plane = lay.ypad_plane;
        info->scratch_bytes = (int64_t)d->N * (int64_t)dnet_scratch_bytes_per_sample(d->C, d->H, d->W, d->hidden, d->Cout);
        if (!d->dn_scratch) return GLOWHIP_OK;
        GH_REQUIRE(d->state && d->z_in_bs >= (long)d->C * d->H * d->W, "debug_fin: dnet state / batch stride");
        GH_REQUIRE(!d->mix_bias == !d->mix_scale, "debug_fin: the ActNorm is a bias and a scale table, or neither");
        if (d->op == GLOWHIP_FIN_DN_FIN) {
            GH_REQUIRE(d->mode >= TAIL_AFFINE_FWD && d->mode <= TAIL_ADD_REV, "debug_fin: coupling modes only (mode %d)", d->mode);
            const bool paired = d->mode == TAIL_AFFINE_FWD || d->mode == TAIL_AFFINE_REV;
            GH_REQUIRE(d->Cout == (paired ? d->C : d->C / 2), "debug_fin: Cout=%d does not fit C=%d in mode %d", d->Cout, d->C, d->mode);
            GH_REQUIRE(d->ks >= 1 && d->ks <= DNET_KS_MAX && d->bias && d->scale && d->acc, "debug_fin: dn_fin ks / null operand");
            GH_TRY(dnet_finish(L, d->ks, d->bias, d->scale, d->mode, (unsigned long long*)d->acc, d->mix_bias, d->mix_scale, d->want_u, s, &li));
        } else {
            GH_REQUIRE(d->src && d->src_bs >= (long)d->C * d->H * d->W, "debug_fin: dn_prep source / batch stride");
            GH_TRY(dnet_prep(L, d->src, (long)d->src_bs, d->mix_bias, d->mix_scale, d->mix_reverse, s, &li));
        }
        report();
        return GLOWHIP_OK;
    }
    default: break;
    }
    GH_REQUIRE(false, "debug_fin: unknown op %d", d->op);
    return GLOWHIP_EINVAL;
}

// Testing hook (include/glowhip.h): one SH2 weight image through the plan's pack code, or one launch_cnet_main on the caller's
// operands.  No second path: it decodes the probe, fills the RepackJob / CnetArgs fields the plan fills, calls what the plan calls,
// and copies what the launcher reported.
int glowhip_debug_sh2(const glowhip_sh2_probe* d, glowhip_sh2_info* info, glowhip_stream_t stream) {
    GH_REQUIRE(d && info, "debug_sh2: null probe / info");
    hipStream_t s = (hipStream_t)stream;
    *info = glowhip_sh2_info{};
    GH_REQUIRE(d->Cin > 0 && d->Cout > 0, "debug_sh2: bad shape Cin=%d Cout=%d", d->Cin, d->Cout);
    switch (d->op) {
    case GLOWHIP_SH2_IMAGE: {
        GH_REQUIRE(d->kind == REPACK_SH2_GEMM || d->kind == REPACK_SH2_FIRST || d->kind == REPACK_SH2_TAIL, "debug_sh2: unknown image kind %d", d->kind);
        GH_REQUIRE(d->kind != REPACK_SH2_TAIL || (!d->fold_bias && !d->fold_logs), "debug_sh2: the tail image folds nothing");
        GH_REQUIRE(d->kind == REPACK_SH2_FIRST || d->Cin % 8 == 0, "debug_sh2: k of a GEMM / tail image comes in groups of 8 (Cin=%d)", d->Cin);
        GH_REQUIRE((!d->kperm && d->kind != REPACK_SH2_TAIL) || d->Cin % 32 == 0, "debug_sh2: a k-permuted image has whole 32-k blocks (Cin=%d)", d->Cin);
        RepackJob r{};
        r.kind = d->kind; r.Cin = d->Cin; r.Cout = d->Cout; r.fold_bias = d->fold_bias; r.fold_logs = d->fold_logs;
        int n_kind[4] = {0, 0, 0, 0}, tail_blocks = 1, first_blocks = 2;
        if (d->kind == REPACK_SH2_GEMM) { r.K = d->Cin; r.kperm = d->kperm ? 1 : 0; info->Kp = d->Cin; info->M = d->Cout; n_kind[1] = 1; }
        else if (d->kind == REPACK_SH2_FIRST) {
            r.K = cnet_g0(d->Cin); info->Kp = r.K * 8; info->M = d->Cout; n_kind[2] = 1;
            if (d->Cin >= 64) first_blocks = std::max(2, std::min(16, (d->Cout + 31) / 32));
        } else { r.Kpad = cnet_mpad4(d->Cout); r.kperm = 1; info->Kp = d->Cin; info->M = r.Kpad; n_kind[3] = 1; tail_blocks = (d->Cout + 7) / 8; }
        info->image_bytes = (int64_t)sh2_image_bytes(info->Kp, info->M);
        if (!d->image) return GLOWHIP_OK;
        GH_REQUIRE(d->w && (!d->transposed || d->flip), "debug_sh2: image null weight / flip buffer");
        const int ks = d->kind == REPACK_SH2_GEMM ? 1 : 9;
        struct Tables { FlipJob f[3]; RepackJob r; } t{};
        r.w = d->transposed ? d->flip : d->w;
        t.r = r;
        // (flip jobs come in triples, one launch per member: three times the one job, with its tile count)
        for (int k = 0; k < 3; ++k) t.f[k] = FlipJob{d->w, 0, d->Cin, d->Cout, ks};      // forward weight (Cin rows, Cout columns) -> (Cout, Cin)
        const int tiles = ((d->Cin + 31) / 32) * ((d->Cout + 31) / 32);
        const int tiles3[3] = {tiles, tiles, tiles};
        Tables* dev = nullptr;
        GH_REQUIRE(hipMalloc((void**)&dev, sizeof(Tables)) == hipSuccess, "debug_sh2: no device memory for the job tables");
        // (a blocking copy: it is complete before the launches below are queued on s, whatever stream s is; t lives on this frame)
        int rc = hipMemcpy(dev, &t, sizeof(Tables), hipMemcpyHostToDevice) == hipSuccess ? GLOWHIP_OK : GLOWHIP_ELAUNCH;
        if (rc == GLOWHIP_OK && d->transposed) rc = launch_flipT_batched(dev->f, 3, tiles3, d->flip, s);
        if (rc == GLOWHIP_OK) rc = launch_pack_batched(nullptr, 0, &dev->r, n_kind, tail_blocks, d->image, s, s, first_blocks);
        if (hipStreamSynchronize(s) != hipSuccess && rc == GLOWHIP_OK) rc = GLOWHIP_ELAUNCH;
        (void)hipFree(dev);
        return rc;
    }
    case GLOWHIP_SH2_CNET: {
        GH_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "debug_sh2: bad shape N=%d map %dx%d", d->N, d->H, d->W);
        CnetArgs a{};
        a.x = d->x; a.x_bs = (long)d->x_bs; a.w0 = d->w0; a.w2 = d->w2; a.w4 = d->w4;
        a.N = d->N; a.Cin = d->Cin; a.H = d->H; a.W = d->W; a.hidden = d->hidden; a.Cout = d->Cout; a.mode = d->mode;
        a.scratch = d->scratch;
        a.tape_h1 = (float*)d->tape_h1; a.tape_h2 = (float*)d->tape_h2; a.mask1 = (unsigned short*)d->mask1; a.mask2 = (unsigned short*)d->mask2;
        a.in_scale = d->in_scale; a.out_scale = d->out_scale; a.bwd = d->bwd ? 1 : 0;
        CnetLaunchInfo li{};
        CnetPending p{};
        auto report = [&]() {
            info->kernel = li.one_wave ? GLOWHIP_S2I_CNET1W : GLOWHIP_S2I_CNET;
            info->hid = li.hid; info->ms = li.ms; info->upw = li.upw; info->pxt = li.pxt; info->ng = li.ng; info->mode = li.mode;
            info->g0 = li.g0; info->nrt4 = li.nrt4;
            info->grid[0] = li.grid[0]; info->grid[1] = li.grid[1]; info->grid[2] = li.grid[2]; info->lds_bytes = li.lds_bytes;
            info->MS = p.MS; info->tiles = p.tiles; info->R = p.R; info->NI = p.NI; info->lpxt = p.lpxt;
            info->scratch_floats = (int64_t)cnet_scratch_floats(d->N, d->H, d->W, d->Cout);
        };
        // the choice alone first (nothing is launched in a dry run): every refusal of the launcher is made before any operand is looked at
        li.dry_run = 1;
        GH_TRY(launch_cnet_main(a, s, &p, &li));
        report();
        if (!d->scratch) return GLOWHIP_OK;
        GH_REQUIRE(d->scratch_floats >= info->scratch_floats, "debug_sh2: scratch below the plan's %ld floats", (long)info->scratch_floats);
        GH_REQUIRE(d->x && d->w0 && d->w2 && d->w4, "debug_sh2: cnet null operand");
        GH_REQUIRE(d->x_bs >= (int64_t)d->Cin * d->H * d->W, "debug_sh2: batch stride below one sample");
        GH_REQUIRE(!d->bwd || d->tape_h1, "debug_sh2: a backward launch stores its gradient tensors");
        li = CnetLaunchInfo{};
        GH_TRY(launch_cnet_main(a, s, &p, &li));
        report();
        return GLOWHIP_OK;
    }
    case GLOWHIP_SH2_DN_MIX:
    case GLOWHIP_SH2_DN_NET: {
        GH_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && dnet_supported(d->Cin, d->H, d->W, d->hidden, d->Cout), "dnet: unsupported shape");
        DnetLevel L{d->N, d->Cin, d->H, d->W, d->hidden, d->Cout, d->state, (long)d->x_bs, d->dn_scratch};
        DnetScratchLayout lay;
        dnet_scratch_layout(L, &lay);
        info->part_off = lay.part_off;
        info->scratch_bytes = (int64_t)d->N * (int64_t)dnet_scratch_bytes_per_sample(d->Cin, d->H, d->W, d->hidden, d->Cout);
        if (!d->dn_scratch) return GLOWHIP_OK;
        GH_REQUIRE(d->w0 && d->state && d->x_bs >= (int64_t)d->Cin * d->H * d->W, "debug_sh2: dnet null operand / batch stride");
        DnLaunchInfo li{};
        if (d->op == GLOWHIP_SH2_DN_MIX) {
            GH_REQUIRE(!d->post_scale == !d->post_bias, "debug_sh2: the reverse mixer has a scale and a bias table, or neither");
            GH_TRY(dnet_level_begin(L, s));
            GH_TRY(dnet_mix(L, d->w0, d->post_scale, d->post_bias, d->want_pad ? 1 : 0, s, &li));
        } else {
            GH_REQUIRE(d->w2 && d->w4, "debug_sh2: dn_net null image");
            int ks = 0;
            GH_TRY(dnet_coupling_net(L, d->w0, d->w2, d->w4, &ks, s, &li));
            info->ks = ks;
        }
        info->dn_launches = li.n;
        for (int k = 0; k < li.n; ++k) {
            info->dn_rt[k] = li.rt[k]; info->dn_pt[k] = li.pt[k]; info->dn_npf[k] = li.npf[k];
            for (int q = 0; q < 3; ++q) info->dn_grid[3 * k + q] = li.grid[k][q];
        }
        return GLOWHIP_OK;
    }
    default: break;
    }
    GH_REQUIRE(false, "debug_sh2: unknown op %d", d->op);
    return GLOWHIP_EINVAL;
}

}  // extern "C"

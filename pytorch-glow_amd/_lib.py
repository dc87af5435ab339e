"""ctypes binding of libglowhip.so (the C ABI declared in include/glowhip.h).

The library is built in-tree by ``pytorch-glow_amd/csrc/Makefile`` (hipcc, gfx950) and loaded from
``pytorch-glow_amd/libglowhip.so``.  There is NO fallback: if the library is missing every compute
entry point raises, so a GPU test can never pass on a silent PyTorch path.
"""
from __future__ import annotations

import contextlib
import ctypes
import enum
import os
import subprocess
import threading
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_long, c_size_t, c_void_p

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# GLOWHIP_LIB_PATH: kernel-variant experiments (scripts/) load an alternative build of the same ABI
LIB_PATH = os.environ.get("GLOWHIP_LIB_PATH") or os.path.join(_PKG_DIR, "libglowhip.so")
CSRC_DIR = os.path.join(_PKG_DIR, "csrc")

LAYER_SQUEEZE, LAYER_FLOWSTEP, LAYER_SPLIT2D = 0, 1, 2
PERM_INVCONV, PERM_GATHER = 0, 1
COUPLING_ADDITIVE, COUPLING_AFFINE = 0, 1


class GlowHipError(RuntimeError):
    """Non-zero return code from libglowhip (message = glowhip_last_error())."""


class LayerDesc(ctypes.Structure):
    """Mirror of ``glowhip_layer_desc`` (include/glowhip.h)."""
    _fields_ = [
        ("kind", c_int32), ("C", c_int32), ("H", c_int32), ("W", c_int32),
        ("hidden", c_int32), ("permutation", c_int32), ("coupling", c_int32), ("reserved", c_int32),
        ("an_bias", c_void_p), ("an_logs", c_void_p),
        ("invconv_w", c_void_p),
        ("perm_idx", c_void_p), ("perm_idx_inv", c_void_p),
        ("f0_w", c_void_p), ("f0_an_bias", c_void_p), ("f0_an_logs", c_void_p),
        ("f2_w", c_void_p), ("f2_an_bias", c_void_p), ("f2_an_logs", c_void_p),
        ("f4_w", c_void_p), ("f4_bias", c_void_p), ("f4_logs", c_void_p),
    ]


class LayerGrads(ctypes.Structure):
    """Mirror of ``glowhip_layer_grads``."""
    _fields_ = [(n, c_void_p) for n in ("an_bias", "an_logs", "invconv_w", "f0_w", "f0_an_bias", "f0_an_logs",
                                        "f2_w", "f2_an_bias", "f2_an_logs", "f4_w", "f4_bias", "f4_logs")]


CRIT_NONE, CRIT_CE, CRIT_BCE = 0, 1, 2
HEAD_PARAMS = ("lt_bias", "lt_logs", "ye_w", "ye_b", "ye_logs", "cl_w", "cl_b", "cl_logs")


class HeadDesc(ctypes.Structure):
    """Mirror of ``glowhip_head_desc``."""
    _fields_ = [("K", c_int32), ("criterion", c_int32), ("weight_y", c_float), ("reserved", c_int32)] + [(n, c_void_p) for n in HEAD_PARAMS]


class HeadIO(ctypes.Structure):
    """Mirror of ``glowhip_head_io``."""
    _fields_ = [(n, c_void_p) for n in ("y_onehot", "y", "y_logits", "cls_loss", "g_logit", "state")]


class HeadGrads(ctypes.Structure):
    """Mirror of ``glowhip_head_grads``."""
    _fields_ = [(n, c_void_p) for n in HEAD_PARAMS]


class InvconvLU(ctypes.Structure):
    """Mirror of ``glowhip_invconv_lu``."""
    _fields_ = [(n, c_void_p) for n in ("perm", "l", "u", "log_s", "sign_s", "w")]


class InvconvLUGrads(ctypes.Structure):
    """Mirror of ``glowhip_invconv_lu_grads``."""
    _fields_ = [(n, c_void_p) for n in ("dl", "du", "dlog_s")]


class OptimChunk(ctypes.Structure):
    """Mirror of ``glowhip_optim_chunk``."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("m", c_void_p), ("v", c_void_p), ("n", c_int32), ("pad", c_int32)]


class GradSeg(ctypes.Structure):
    """Mirror of ``glowhip_grad_seg``."""
    _fields_ = [("grad", c_void_p), ("acc", c_void_p), ("n", ctypes.c_int64)]


class MalaSeg(ctypes.Structure):
    """Mirror of ``glowhip_mala_seg``."""
    _fields_ = [("cur", c_void_p), ("prop", c_void_p), ("per", ctypes.c_int64)]


class WgradGemm(ctypes.Structure):
    """Mirror of ``glowhip_wgrad_gemm`` (the testing hook ``glowhip_debug_wgrad``)."""
    _fields_ = [(n, c_void_p) for n in ("A", "B", "partial", "dw", "rowsum")] + [("a_bs", ctypes.c_int64), ("b_bs", ctypes.c_int64)] + \
               [(n, c_int32) for n in ("Mpad", "Npad", "Mreal", "Nreal", "mode", "b_valid", "b_half", "tiled")]


class WgradTaps(ctypes.Structure):
    """Mirror of ``glowhip_wgrad_taps``."""
    _fields_ = [(n, c_int32) for n in ("operand", "C", "H", "W", "sign")]


class WgradProbe(ctypes.Structure):
    """Mirror of ``glowhip_wgrad_probe``."""
    _fields_ = [("op", c_int32), ("N", c_int32), ("HW", c_int32), ("ksize", c_int32), ("sh_scale", c_float), ("reserved", c_int32),
                ("gemm", WgradGemm * 3), ("taps", WgradTaps * 2)]


class WgradInfo(ctypes.Structure):
    """Mirror of ``glowhip_wgrad_info``."""
    _fields_ = [(n, c_int32 * 3) for n in ("instance", "splits", "ktiles_per_split", "blocks", "live")] + \
               [("reserved", c_int32), ("partial_floats", ctypes.c_int64 * 3)]


# glowhip.h GLOWHIP_WGRAD_* (op) and GLOWHIP_WGI_* (instance)
WGRAD_MFMA, WGRAD_PAIR, WGRAD_TRIO, WGRAD_SHIFT_EXPAND, WGRAD_DIRECT, WGRAD_HALF_TO_FLOAT = range(6)
WGI_F32_128, WGI_F32_64, WGI_SH = 1, 2, 0x100
WGI_BN64, WGI_VA, WGI_VB, WGI_BV, WGI_BH = 1, 2, 4, 8, 16
WGI_PS128, WGI_PS64, WGI_PS512 = 0x200, 0x201, 0x202
WGI_PAIR64, WGI_PAIR128, WGI_TRIO64, WGI_TRIO128 = 0x300, 0x301, 0x400, 0x401
WGI_SHIFT_EXPAND, WGI_DIRECT1, WGI_DIRECT3, WGI_HALF_TO_FLOAT = 0x500, 0x501, 0x503, 0x600

BWD_MAX_JOBS = 8      # glowhip.h GLOWHIP_BWD_MAX_JOBS


class BwdJob(ctypes.Structure):
    """Mirror of ``glowhip_bwd_job`` (the testing hook ``glowhip_debug_bwd``)."""
    _fields_ = [(n, c_void_p) for n in ("a", "b", "c", "d", "out")] + [("n", c_int32 * 6), ("stride", ctypes.c_int64), ("add_mul", ctypes.c_double)]


class BwdProbe(ctypes.Structure):
    """Mirror of ``glowhip_bwd_probe``."""
    _fields_ = [(n, c_int32) for n in ("op", "N", "C", "C2", "HW", "flag", "ksize", "acc_copies", "n_jobs", "reserved")] + \
               [("acc_stride", ctypes.c_int64), ("bs", ctypes.c_int64 * 2), ("per", ctypes.c_int64), ("inv", ctypes.c_double),
                ("add_scale", c_float), ("add", c_int32 * 8), ("reserved2", c_int32),
                ("src", c_void_p * 7), ("dst", c_void_p * 2), ("acc", c_void_p * 3), ("job", BwdJob * BWD_MAX_JOBS)]


class BwdInfo(ctypes.Structure):
    """Mirror of ``glowhip_bwd_info``."""
    _fields_ = [("kernel", c_int32), ("grid", c_int32 * 3)] + \
               [(n, c_int32) for n in ("threads_per_channel", "w_lds", "lds_bytes", "mix_blocks", "rblocks", "plain_stores", "launches", "reserved")]


# glowhip.h GLOWHIP_BWD_* (op) and GLOWHIP_BWI_* (kernel)
BWD_COUPLING, BWD_SPLIT, BWD_ACT, BWD_CHANMIX, BWD_PRIOR, BWD_FLIP, BWD_LOGS_FROM_DW, BWD_FINALIZE = range(8)
BWI_COUPLING4, BWI_COUPLING1, BWI_SPLIT, BWI_ACT4, BWI_ACT1, BWI_CHANMIX, BWI_CHANMIX_REDUCE, BWI_CHANMIX_WIDE, BWI_PRIOR = range(1, 10)

class ConvProbe(ctypes.Structure):
    """Mirror of ``glowhip_conv_probe`` (the testing hook ``glowhip_debug_conv``)."""
    _fields_ = [(n, c_int32) for n in ("op", "N", "Cin", "H", "W", "Cout", "ksize", "relu", "transposed", "mode")] + \
               [(n, ctypes.c_int64) for n in ("x_bs", "scratch_floats", "z2_in_bs", "z2_out_bs")] + \
               [(n, c_void_p) for n in ("x", "w", "bias", "post_bias", "post_logs", "post_scale", "fold_bias", "fold_logs", "image", "scratch", "y",
                                        "z2_in", "z2_out", "hout", "zeros", "acc", "term")]


class ConvInfo(ctypes.Structure):
    """Mirror of ``glowhip_conv_info``."""
    _fields_ = [(n, c_int32) for n in ("kernel", "ksize", "tile", "splits", "mb")] + [("grid", c_int32 * 3), ("launches", c_int32), ("paired", c_int32),
                                                                                     ("image_bytes", ctypes.c_int64)]


# glowhip.h GLOWHIP_CONV_* (op), GLOWHIP_CVI_* (kernel) and the TailMode values of csrc/conv_mfma.h
CONV_WIDE, CONV_FIRST, CONV_DIRECT, CONV_TAIL = range(4)
CVI_WIDE, CVI_GEMM_GLDS, CVI_FIRST, CVI_DIRECT, CVI_TAIL, CVI_TAIL_DMA = range(1, 7)
TAIL_PLAIN, TAIL_AFFINE_FWD, TAIL_AFFINE_REV, TAIL_ADD_FWD, TAIL_ADD_REV, TAIL_SPLIT_FWD, TAIL_SPLIT_REV = range(7)



class FinProbe(ctypes.Structure):
    """Mirror of ``glowhip_fin_probe`` (the testing hook ``glowhip_debug_fin``)."""
    _fields_ = [(n, c_int32) for n in ("op", "N", "C", "H", "W", "HW", "Cout", "hidden", "mode", "MS", "tile", "ks", "want_u", "Ca",
                                       "mix_C", "mix_reverse", "sq_u8", "sq_W", "rng_on", "reserved")] + \
               [("sq_div", c_float), ("rng_scale", c_float), ("rng_seed", ctypes.c_uint64), ("rng_call", ctypes.c_uint64)] + \
               [(n, ctypes.c_int64) for n in ("z_in_bs", "z_out_bs", "in_a_bs", "in_b_bs", "out_bs", "sq_bs", "src_bs", "scratch_floats")] + \
               [(n, c_void_p) for n in ("scratch", "bias", "scale", "z_in", "z_out", "acc", "tape_hout", "mix_bias", "mix_scale", "mix_matrix",
                                        "mix_gather", "in_a", "in_b", "out", "sq_src", "sq_noise", "state", "dn_scratch", "src")]


class FinInfo(ctypes.Structure):
    """Mirror of ``glowhip_fin_info``."""
    _fields_ = [("kernel", c_int32), ("grid", c_int32 * 3)] + \
               [(n, c_int32) for n in ("lds_bytes", "pxb", "msv", "halo", "xcd_affine", "stage_matrix", "R", "NI", "tiles", "lpxt", "reserved")] + \
               [(n, ctypes.c_int64) for n in ("scratch_floats", "scratch_bytes", "part_off", "u_off", "ypad_off", "u_plane", "ypad_plane")]


# glowhip.h GLOWHIP_FIN_* (op) and GLOWHIP_FNI_* (kernel); csrc/common.h ACC_EXTRA
FIN_CFINISH, FIN_CHANMIX, FIN_DN_FIN, FIN_DN_PREP = range(4)
FNI_CFINISH, FNI_CHANMIX16, FNI_CHANMIX64, FNI_CHANMIX_WIDE, FNI_DN_FIN, FNI_DN_PREP = range(1, 7)
ACC_EXTRA = 7

class Sh2Probe(ctypes.Structure):
    """Mirror of ``glowhip_sh2_probe`` (the testing hook ``glowhip_debug_sh2``)."""
    _fields_ = [(n, c_int32) for n in ("op", "kind", "N", "Cin", "H", "W", "hidden", "Cout", "mode", "bwd", "kperm", "transposed", "want_pad", "reserved")] + \
               [("in_scale", c_float), ("out_scale", c_float), ("x_bs", ctypes.c_int64), ("scratch_floats", ctypes.c_int64)] + \
               [(n, c_void_p) for n in ("w", "fold_bias", "fold_logs", "flip", "image", "x", "w0", "w2", "w4", "scratch",
                                        "tape_h1", "tape_h2", "mask1", "mask2", "state", "dn_scratch", "post_scale", "post_bias")]


class Sh2Info(ctypes.Structure):
    """Mirror of ``glowhip_sh2_info``."""
    _fields_ = [(n, c_int32) for n in ("kernel", "hid", "ms", "upw", "pxt", "ng", "mode", "g0", "nrt4")] + \
               [("grid", c_int32 * 3)] + [(n, c_int32) for n in ("lds_bytes", "MS", "tiles", "R", "NI", "lpxt", "Kp", "M", "dn_launches", "ks")] + \
               [("dn_rt", c_int32 * 3), ("dn_pt", c_int32 * 3), ("dn_npf", c_int32 * 3), ("dn_grid", c_int32 * 9)] + \
               [(n, ctypes.c_int64) for n in ("part_off", "scratch_bytes", "scratch_floats", "image_bytes")]


# glowhip.h GLOWHIP_SH2_* (op, image kind) and GLOWHIP_S2I_* (kernel)
SH2_IMAGE, SH2_CNET, SH2_DN_MIX, SH2_DN_NET = range(4)
SH2_GEMM, SH2_FIRST, SH2_TAIL = 3, 4, 5
S2I_CNET, S2I_CNET1W = 1, 2

EVAL_MAX_LEVELS, EVAL_MAX_BINS = 16, 256      # glowhip.h GLOWHIP_EVAL_MAX_*


class EvalState(ctypes.Structure):
    """Mirror of ``glowhip_eval_state`` (device-resident; read back through a uint8 tensor of ``sizeof``)."""
    _fields_ = [("count", ctypes.c_uint64), ("flagged", ctypes.c_uint64), ("min_key", ctypes.c_uint64), ("max_key", ctypes.c_uint64),
                ("sum_bpd", ctypes.c_uint64 * 2), ("sum_bpd2", ctypes.c_uint64 * 2), ("sum_single", ctypes.c_uint64 * 2),
                ("sum_level", (ctypes.c_uint64 * 2) * EVAL_MAX_LEVELS), ("lo", ctypes.c_double), ("hi", ctypes.c_double),
                ("bins", c_int32), ("n_levels", c_int32), ("under", ctypes.c_uint64), ("over", ctypes.c_uint64),
                ("hist", ctypes.c_uint64 * EVAL_MAX_BINS)]


ACC_FIRST, ACC_ADD, ACC_FINISH = 0, 1, 2      # glowhip.h GLOWHIP_ACC_*
ACC_MAX_SEGS = 16
MALA_MAX_SEGS, MALA_MAX_LEAVES = 32, 120      # csrc/posterior.hip


class TimingRecord(ctypes.Structure):
    """Mirror of ``glowhip_timing_record``."""
    _fields_ = [("kind", c_int32), ("layer", c_int32), ("mfma", c_int32), ("ms", c_float)]


K_CHANMIX, K_CONV_F0, K_CONV_F2, K_CONV_F4, K_OTHER = range(5)


class DBG(enum.IntFlag):
    """Mirror of the ``GLOWHIP_DBG_*`` values of include/glowhip.h: the argument of ``glowhip_debug_force_tail_tile`` (through
    :func:`debug_flags`).  The tail convolution's pixel tile (16 / 32 / 64 / 128) is OR-ed in as a plain integer."""
    TAIL_MSPLIT = 0x100
    TAIL_NO_MSPLIT = 0x200
    TAIL_NO_DMA = 0x400
    EXACT_FP32 = 0x800
    PACK_UNFUSED = 0x1000
    NO_MIXER_FUSION = 0x8000
    NO_CNET1W = 0x10000
    NO_CNET1W_BWD = 0x40000
    WGRAD_NARROW = 0x80000
    LU_WORKGROUP = 0x200000
    CNET_128_ONLY = 0x2000000
    CNET_64 = 0x4000000
    CFINISH_BLOCK_ORDER = 0x10000000
    PACK_ONE_STREAM = 0x20000000
    TRAIN_PER_LAYER_FWD = 0x40000000
    TRAIN_PER_LAYER_BWD = 0x80000000


DBG_CNET_ROWS_SHIFT = 22      # bits 22..24 = 1, 2 or 4 row splits of k_cnet: ``rows << DBG_CNET_ROWS_SHIFT``


@contextlib.contextmanager
def debug_flags(value):
    """Run a block under ``glowhip_debug_force_tail_tile(value)`` (an OR of :class:`DBG` values, the tail tile and the row-split
    field); automatic selection is restored on exit, whatever happens.  Process-wide, not thread safe: a testing hook."""
    value = int(value) & 0xffffffff
    lib().glowhip_debug_force_tail_tile(value - (1 << 32) if value >= (1 << 31) else value)      # bit 31 into the signed c_int
    try:
        yield
    finally:
        lib().glowhip_debug_force_tail_tile(0)


_P = c_void_p
# name -> (restype, argtypes); every symbol include/glowhip.h declares (tests/test_abi.py checks the two agree)
SIGNATURES = {
    "glowhip_version": (c_int, []),
    "glowhip_last_error": (c_char_p, []),
    "glowhip_squeeze2d": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "glowhip_actnorm_init": (c_int, [_P, c_long, c_int, c_int, c_int, c_float, _P, _P, _P]),
    "glowhip_actnorm_init_batch_variance": (c_int, [_P, c_long, c_int, c_int, c_int, c_float, _P, _P, _P]),
    "glowhip_actnorm": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "glowhip_invconv_scratch_bytes": (c_size_t, [c_int]),
    "glowhip_invconv_prepare": (c_int, [_P, c_int, _P, _P, _P, _P]),
    "glowhip_invconv_lu_prepare": (c_int, [_P, _P, _P, _P, _P, c_int, _P, _P, _P, _P]),
    "glowhip_invconv_lu_backward": (c_int, [_P, _P, _P, _P, _P, c_int, _P, ctypes.c_double, _P, _P, _P, _P]),
    "glowhip_plan_bind_invconv_lu": (c_int, [_P, c_int, POINTER(InvconvLU)]),
    "glowhip_plan_bind_invconv_lu_grads": (c_int, [_P, c_int, POINTER(InvconvLUGrads)]),
    "glowhip_invconv": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "glowhip_permute_channels": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P]),
    "glowhip_conv2d": (c_int, [_P, c_long, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P]),
    "glowhip_gaussian_logp": (c_int, [_P, c_long, _P, _P, c_long, c_int, c_int, c_int, _P, _P, _P, _P]),
    "glowhip_plan_create": (_P, [POINTER(LayerDesc), c_int]),
    "glowhip_plan_destroy": (None, [_P]),
    "glowhip_plan_packed_bytes": (c_size_t, [_P]),
    "glowhip_plan_workspace_bytes": (c_size_t, [_P, c_int]),
    "glowhip_plan_pack": (c_int, [_P, _P, c_size_t, _P]),
    "glowhip_plan_pack_for": (c_int, [_P, _P, c_size_t, c_int, _P]),
    "glowhip_plan_pack_sync": (c_int, [_P]),
    "glowhip_plan_forget_packed": (c_int, [_P]),
    "glowhip_plan_encode": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "glowhip_plan_decode": (c_int, [_P, _P, _P, POINTER(c_void_p), c_int, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "glowhip_glow_forward": (c_int, [_P, _P, _P, _P, _P, _P, c_long, c_int, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "glowhip_glow_forward_u8": (c_int, [_P, _P, _P, c_float, _P, _P, _P, c_long, c_int, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "glowhip_plan_set_family": (c_int, [_P, c_int]),
    "glowhip_plan_get_family": (c_int, [_P]),
    "glowhip_plan_status": (c_int, [_P, _P, c_size_t, c_int, _P, c_long, _P, _P]),
    "glowhip_plan_set_dequant_rng": (c_int, [_P, ctypes.c_ulonglong, c_int, POINTER(ctypes.c_ulonglong)]),
    "glowhip_plan_set_dequant_stream": (c_int, [_P, ctypes.c_ulonglong, ctypes.c_ulonglong]),
    "glowhip_dequant_noise": (c_int, [_P, c_long, ctypes.c_ulonglong, ctypes.c_ulonglong, c_int, _P]),
    "glowhip_normal_noise": (c_int, [_P, c_long, ctypes.c_ulonglong, ctypes.c_ulonglong, c_int, c_float, _P]),
    "glowhip_plan_bind_sampler": (c_int, [_P, _P, POINTER(c_float), c_int, c_int]),
    "glowhip_plan_sample": (c_int, [_P, _P, _P, _P, _P, c_long, c_float, POINTER(c_void_p), c_int, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "glowhip_plan_actnorm_init": (c_int, [_P, _P, c_size_t, _P, _P, c_float, c_int, _P, c_size_t, _P]),
    "glowhip_plan_output_shape": (c_int, [_P, c_int, POINTER(c_int32)]),
    "glowhip_plan_describe": (c_int, [_P, c_char_p, c_size_t]),
    "glowhip_plan_describe_for": (c_int, [_P, c_int, c_char_p, c_size_t]),
    "glowhip_plan_launch_counts": (c_int, [_P, c_char_p, c_size_t, c_int]),
    "glowhip_debug_force_tail_tile": (None, [c_int]),
    "glowhip_debug_wgrad": (c_int, [POINTER(WgradProbe), POINTER(WgradInfo), _P]),
    "glowhip_debug_bwd": (c_int, [POINTER(BwdProbe), POINTER(BwdInfo), _P]),
    "glowhip_debug_conv": (c_int, [POINTER(ConvProbe), POINTER(ConvInfo), _P]),
    "glowhip_debug_fin": (c_int, [POINTER(FinProbe), POINTER(FinInfo), _P]),
    "glowhip_debug_sh2": (c_int, [POINTER(Sh2Probe), POINTER(Sh2Info), _P]),
    "glowhip_plan_tape_bytes": (c_size_t, [_P, c_int]),
    "glowhip_plan_train_workspace_bytes": (c_size_t, [_P, c_int]),
    "glowhip_glow_forward_train": (c_int, [_P, _P, _P, _P, _P, _P, c_long, c_int, _P, _P, _P, c_int, _P, c_size_t, _P,
                                           c_size_t, _P]),
    "glowhip_glow_backward": (c_int, [_P, _P, _P, _P, c_size_t, _P, _P, _P, _P, c_long, POINTER(LayerGrads), _P, c_int,
                                      _P, c_size_t, _P]),
    "glowhip_plan_decode_vjp_workspace_bytes": (c_size_t, [_P, c_int]),
    "glowhip_plan_decode_vjp": (c_int, [_P, _P, _P, _P, _P, POINTER(c_void_p), c_int, c_int, _P, c_size_t, _P, c_size_t, _P]),
    "glowhip_plan_backward_marks": (c_int, [_P, POINTER(c_int32), POINTER(c_void_p), c_int]),
    "glowhip_optim_step": (c_int, [_P, c_int, c_int, c_float, ctypes.c_double, ctypes.c_double, c_float, c_float, c_int, c_float, c_float, _P, _P, c_int, _P]),
    "glowhip_optim_step_dev": (c_int, [_P, c_int, c_int, _P, ctypes.c_double, ctypes.c_double, c_float, c_float, c_float, c_float, _P, _P, c_int, _P]),
    "glowhip_optim_step_ema": (c_int, [_P, _P, c_int, c_int, c_float, ctypes.c_double, ctypes.c_double, c_float, c_float, c_int, c_float, c_float, c_float, _P, _P, c_int, _P]),
    "glowhip_optim_step_ema_dev": (c_int, [_P, _P, c_int, c_int, _P, ctypes.c_double, ctypes.c_double, c_float, c_float, c_float, c_float, _P, _P, c_int, _P]),
    "glowhip_optim_ema_swap": (c_int, [_P, _P, c_int, _P]),
    "glowhip_grad_accumulate": (c_int, [POINTER(GradSeg), c_int, c_int, c_float, _P]),
    "glowhip_restore_objective": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "glowhip_restore_objective_psf": (c_int, [_P, _P, _P, _P, _P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "glowhip_restore_linear_scratch_bytes": (c_size_t, [c_int, c_long, c_long]),
    "glowhip_restore_objective_linear": (c_int, [_P, _P, _P, _P, _P, c_long, c_int, c_long, _P, _P, _P, _P, c_size_t, _P]),
    "glowhip_restore_fourier_scratch_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "glowhip_restore_objective_fourier": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "glowhip_fourier2d": (c_int, [_P, _P, c_long, c_int, c_int, c_int, _P]),
    "glowhip_restore_coils_scratch_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "glowhip_restore_objective_coils": (c_int, [_P, _P, _P, _P, _P, c_long, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "glowhip_coils2d": (c_int, [_P, _P, c_long, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "glowhip_psf_from_logits": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "glowhip_restore_psf_grad_scratch_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "glowhip_restore_psf_grad": (c_int, [_P, _P, _P, _P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "glowhip_mala_scratch_bytes":(c_size_t, [POINTER(MalaSeg), c_int, c_int, c_int]),
    "glowhip_mala_init": (c_int, [_P, _P, c_int, c_float, c_float, _P]),
    "glowhip_mala_propose": (c_int, [POINTER(MalaSeg), c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "glowhip_mala_energy": (c_int, [POINTER(MalaSeg), c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "glowhip_mala_select": (c_int, [POINTER(MalaSeg), c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_float, c_float,
                                    c_float, _P, _P, c_size_t, _P]),
    "glowhip_posterior_moments": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_long, _P]),
    "glowhip_plan_set_head": (c_int, [_P, POINTER(HeadDesc)]),
    "glowhip_plan_head_state_bytes": (c_size_t, [_P, c_int]),
    "glowhip_plan_bind_head": (c_int, [_P, POINTER(HeadIO)]),
    "glowhip_plan_bind_head_grads": (c_int, [_P, POINTER(HeadGrads)]),
    "glowhip_plan_bind_latents": (c_int, [_P, POINTER(c_void_p), c_int]),
    "glowhip_plan_level_count": (c_int, [_P]),
    "glowhip_plan_level_scratch_bytes": (c_size_t, [_P, c_int]),
    "glowhip_plan_bind_level_terms": (c_int, [_P, _P, _P, c_size_t]),
    "glowhip_eval_reset": (c_int, [_P, c_int, c_int, ctypes.c_double, ctypes.c_double, _P]),
    "glowhip_eval_fold": (c_int, [_P, _P, _P, c_int, c_int, c_int, ctypes.c_double, _P, _P, c_long, _P]),
    "glowhip_top_prior": (c_int, [POINTER(HeadDesc), _P, c_int, c_int, c_int, _P, _P, _P]),
    "glowhip_plan_timing_enable": (c_int, [_P, c_int]),
    "glowhip_plan_timing_read": (c_int, [_P, POINTER(TimingRecord), c_int, POINTER(c_int)]),
}

_lib = None
_lock = threading.Lock()


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile libglowhip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC_DIR, "clean"], check=True, capture_output=not verbose)
    proc = subprocess.run(["make", "-C", CSRC_DIR, "-j", str(min(8, os.cpu_count() or 1))],
                          capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building libglowhip.so failed:\n" + proc.stdout[-4000:] + proc.stderr[-4000:])
    if verbose:
        print(proc.stdout)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """The loaded library; raises (never falls back) if it is not there."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise GlowHipError(
                        f"{LIB_PATH} not found: build it with `make -C {CSRC_DIR}` (or __graft_entry__.build()). "
                        "There is no CPU/PyTorch fallback for the flow path.")
                handle = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(handle, name)
                    fn.restype, fn.argtypes = res, args
                _lib = handle
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().glowhip_last_error()
        raise GlowHipError(f"libglowhip error {rc}: {msg.decode() if msg else '?'}")


def stream_ptr(device=None) -> c_void_p:
    """hipStream_t of torch's current stream on ``device`` (so kernels order with torch's own work)."""
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t) -> c_void_p:
    return c_void_p(None) if t is None else c_void_p(t.data_ptr())


def require_device_tensor(t: torch.Tensor, what: str = "input", allow_uint8: bool = False) -> torch.Tensor:
    """The HIP path only takes fp32 tensors resident on a GPU (the Glow input also as 8-bit pixels); anything else is an
    error, not a fallback."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise GlowHipError(f"{what} is on {t.device}: the Glow flow path runs only on a HIP device "
                           "(there is no CPU fallback; use oracle/ for CPU checks in tests)")
    if allow_uint8 and t.dtype == torch.uint8:
        return t.contiguous()
    if t.dtype != torch.float32:
        raise GlowHipError(f"{what}: dtype {t.dtype} unsupported, the path computes in fp32")
    return t.contiguous()

"""ctypes binding of the shared libraries csrc/build.sh makes, one per header under include/: LIBRARIES (at the end) is the table of
them, EXTENSIONS, MORE_EXTENSIONS, ZCR_EXTENSIONS and CLS_EXTENSIONS the tables of the second family (xsrc/), _load() the one handshake
of all.
Fails loudly: no fallback."""
import ctypes as C
import os
from typing import NamedTuple

import torch

# ---- every value copied from a `#define DVD_*` of include/dvdgan_hip.h; HEADER_CONSTANTS below names each one
# (tests/test_abi_cpu.py compares them with the header)
F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
(STRUCT_CONV, STRUCT_WGRAD, STRUCT_GRU, STRUCT_SN_ITEM, STRUCT_GRU_STACK, STRUCT_PACK_ITEM, STRUCT_FRAG_ITEM) = range(7)
GRU_TICKETS = 8192      # zero-initialised counters of dvd_gru_desc.tickets
GRU_STACK_MAX = 4       # layers of a dvd_gru_stack_desc
BN_NREP = 16            # copies of the [2C] sums dvd_bn_stats spreads its atomics over
SN_SCRATCH = 512        # floats of dvd_sn_backward's scratch
GUARD_CH = 16384        # elements per workgroup of dvd_grad_guard's norm pass
GUARD_STATE = 8         # doubles of its state block
ORTHO_COLS = 8          # dvd_ortho_grad's table: off, h, w | planner columns
ORTHO_OFF, ORTHO_H, ORTHO_W = 0, 1, 2
METRICS_SIGNED, METRICS_QUANTIZE = 1, 2
METRICS_MIN_SIDE, METRICS_MAX_SIDE = 11, 256        # the 11 x 11 SSIM window, the kernel's widest row
# dvd_clip_gather: columns of a clip row, served sizes
CLIP_COLS = 11
(CLIP_OFF, CLIP_H, CLIP_W, CLIP_FRAMES, CLIP_X0, CLIP_Y0, CLIP_CW, CLIP_CH, CLIP_FLIP, CLIP_XTAB, CLIP_YTAB) = range(CLIP_COLS)
CLIP_MAX_SIDE, CLIP_MAX_OUT = 4096, 256
SHEET_FILL, SHEET_SIGNED = 1, 2
HEADER_CONSTANTS = {"DVD_" + name: value for name, value in list(globals().items())
                    if name.isupper() and not name.startswith("_") and isinstance(value, int)}

_HERE = os.path.dirname(os.path.abspath(__file__))


class ConvDesc(C.Structure):
    _fields_ = [("dtype", C.c_int), ("frames", C.c_int), ("T", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("C", C.c_int), ("ldi", C.c_int), ("Cout", C.c_int), ("ldo", C.c_int),
                ("kt", C.c_int), ("kh", C.c_int), ("kw", C.c_int), ("up2", C.c_int), ("relu_in", C.c_int),
                ("nsplit", C.c_int), ("act", C.c_int), ("out_f32", C.c_int), ("ldres", C.c_int),
                ("ldmask", C.c_int), ("res_up2", C.c_int),
                ("inp", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("res", C.c_void_p),
                ("mask", C.c_void_p), ("out", C.c_void_p), ("ws", C.c_void_p), ("wq", C.c_void_p), ("wq_kind", C.c_int),
                ("pool2", C.c_int)]


class WgradDesc(C.Structure):
    _fields_ = [("dtype", C.c_int), ("frames", C.c_int), ("T", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("C", C.c_int), ("ldx", C.c_int), ("Cin_real", C.c_int), ("Cout", C.c_int), ("Cy", C.c_int),
                ("ldy", C.c_int), ("kt", C.c_int), ("kh", C.c_int), ("kw", C.c_int), ("up2", C.c_int),
                ("relu_in", C.c_int), ("msplit", C.c_int),
                ("s_co", C.c_longlong), ("s_ci", C.c_longlong), ("s_tap", C.c_longlong),
                ("x", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p), ("dbias", C.c_void_p), ("ws", C.c_void_p),
                ("overwrite", C.c_int)]


# Every function include/dvdgan_hip.h declares: return code, then one code per parameter in order (blanks only group them).
# i int, l long long, f float, d double, p any pointer (data, hipStream_t, descriptor, item array, out-parameter: c_void_p takes
# None, an int, a ctypes array or byref()); returns also v void, s const char*.  tests/test_abi_cpu.py parses the header's
# prototypes and compares entry by entry: a new entry point is one line here.
_CTYPES = {"i": C.c_int, "l": C.c_longlong, "f": C.c_float, "d": C.c_double, "p": C.c_void_p, "v": None, "s": C.c_char_p}
SIGNATURES = {
    "dvd_abi_version": "i",
    "dvd_struct_size": "i i",
    "dvd_prof_enable": "v i",
    "dvd_prof_report": "l ipp",
    "dvd_prof_report_variants": "l iippp",
    "dvd_strerror": "s i",
    "dvd_conv_forward": "i pp",
    "dvd_conv_pool2_ok": "i p",
    "dvd_conv_fragment_major_bytes": "l iii",
    "dvd_conv_fragment_major": "i ipp iii p",
    "dvd_conv_fragment_major_batched": "i ipi p",
    "dvd_conv_wants_fragment_major": "i p",
    "dvd_conv_thin_image_bytes": "l i",
    "dvd_conv_thin_image": "i ppi p",
    "dvd_conv_thin_out_image_bytes": "l",
    "dvd_conv_thin_out_image": "i ppi p",
    "dvd_conv_wgrad": "i pp",
    "dvd_conv_wgrad_ws_floats": "l p",
    "dvd_pack_conv_weight": "i ipp iiiiiii pp iiiii p",
    "dvd_pack_conv_weight_batched": "i ipi p",
    "dvd_to_channels_last": "i ipp lil iiii p",
    "dvd_from_channels_last": "i ipp lil iiii p",
    "dvd_convert": "i ipip l p",
    "dvd_convgru_layer_forward": "i pp",
    "dvd_convgru_layer_backward": "i pp",
    "dvd_convgru_ws_floats": "l iiiiii",
    "dvd_conv_pick_nsplit": "i il iii",
    "dvd_convgru_stack_ok": "i pi",
    "dvd_convgru_stack_ws_floats": "l p",
    "dvd_convgru_stack_forward": "i pp",
    "dvd_convgru_stack_backward": "i pp",
    "dvd_debug_stack_ws": "v pi",
    "dvd_bn_stats": "i ip l ii p p",
    "dvd_bn_finalize": "i p l i ff i pppp i p",
    "dvd_cbn_apply": "i ipp l iii pppp i p",
    "dvd_cbn_backward": "i ipppp l iii pppp i pp i p p",
    "dvd_cbn_backward_ws_floats": "l lii",
    "dvd_cbn_backward_reduce": "i ippp l iii pppp i pp i p p",
    "dvd_cbn_backward_apply": "i ipppp l iii ppppp l i p",
    "dvd_pool": "i ipp l iiiiiii f p",
    "dvd_pool_masked": "i ippp l iiiii f p",
    "dvd_unpool": "i ipp l iiiii f p",
    "dvd_colsum": "i ip l ii p p",
    "dvd_add": "i ippp l p",
    "dvd_sum_leading": "i ipp i l p",
    "dvd_act_backward": "i ippp l i p",
    "dvd_vid_downsample": "i pp iiiiii p",
    "dvd_vid_downsample_cat": "i pipip iiiii p",
    "dvd_row_copy": "i ppp ll i p",
    "dvd_sn_power_iter": "i p ii ppp p",
    "dvd_sn_backward": "i ppppp ii pp p",
    "dvd_sn_scale": "i ppp l p",
    "dvd_sn_batched_prepare": "i pip",
    "dvd_sn_batched": "i pp i p p",
    "dvd_linear_forward": "i pppp iii p",
    "dvd_linear_backward": "i pppp i pp iii p",
    "dvd_embedding_backward": "i ppp l i p",
    "dvd_relu_spatial_sum": "i ipp l iii p",
    "dvd_relu_spatial_sum_backward": "i ippp l iii p",
    "dvd_proj_head_forward": "i pppppppp l i p",
    "dvd_proj_head_backward": "i ppppppppppp l i p",
    "dvd_adv_loss": "i p l ii pp f p",
    "dvd_adam_step": "i pppp l ffff i p",
    "dvd_adam_ema_step": "i ppppp l ffff i f p",
    "dvd_ema_step": "i pp l f p",
    "dvd_swap_f32": "i pp l p",
    "dvd_grad_guard_ws_bytes": "l l",
    "dvd_grad_guard": "i p l f i l ppp i p",
    "dvd_adam_guard_step": "i ppppp l ffff i f p p",
    "dvd_frame_metrics_ws_bytes": "l l iiii",
    "dvd_frame_metrics": "i p lll p lll l iiii i ppp p",
    "dvd_ortho_prepare": "l pip",
    "dvd_ortho_grad": "i pp pp i f pp p",
    "dvd_attention_forward": "i ip iiii p ii pppp l i p",
    "dvd_attention_backward": "i ip iiii p ii pppppp l i p",
    "dvd_attention_mfma_ok": "i iiiiiiii",
    "dvd_attention_mfma_forward": "i pipi pppp l i p",
    "dvd_attention_mfma_backward": "i pipi pppppp l i p",
    "dvd_attention_kv_forward": "i ip ii p iii p ii pppp l ii p",
    "dvd_attention_kv_backward": "i ip ii p iii p ii ppppppp l ii p",
    "dvd_maxpool3d": "i ipp l iiii p",
    "dvd_maxpool3d_backward": "i ippp l iiii p",
    "dvd_sepattn_work_floats": "l iiiiii",
    "dvd_sepattn_forward": "i ip iiii p ii pppppppp l iiii p",
    "dvd_sepattn_backward": "i ip iii ppppppppppppp iii p l iiii p",
    "dvd_clip_to_tensor": "i ppp l iii f p p",
    "dvd_clip_gather_band_rows": "i ii",
    "dvd_clip_gather": "i p l ppp l p l ii f p p",
    "dvd_sample_sheet_shape": "i iiiiii ppp",
    "dvd_sample_sheet": "i p lll l iiiiiii f ii p p",
}


# ---- The side libraries, each with a header of its own: every `#define DVD_<KEY>_*` of the header by name, one line of type codes
# per entry point (tests/test_abi_cpu.py compares both with the header and the exports with the table, library by library).
# libdvdgan_hip_adv.so (include/dvdgan_hip_adv.h): the loss launch with LeCam regularization, top-k selection and logit statistics
ADV_MAX_SAMPLES, ADV_NSTAT = 4096, 8        # samples a selection serves, floats of the statistics
(ADV_STAT_MEAN, ADV_STAT_SIGN, ADV_STAT_ACTIVE, ADV_STAT_ADV, ADV_STAT_LECAM, ADV_STAT_ANCHOR, ADV_STAT_KEPT,
 ADV_STAT_NONFINITE) = range(ADV_NSTAT)
ADV_HEADER_CONSTANTS = {"DVD_" + name: value for name, value in list(globals().items())
                        if name.startswith("ADV_") and isinstance(value, int)}
ADV_SIGNATURES = {
    "dvd_adv_loss_ex": "i p l iiii f ppp f pp f p p",
}

# libdvdgan_hip_eval.so (include/dvdgan_hip_eval.h): pooled features, running moments and kernel distances of sample features
# (distmetrics.py)
EVAL_MAX_D, EVAL_TILE, EVAL_MAX_SUBSETS = 4096, 64, 65535
EVAL_HEADER_CONSTANTS = {"DVD_" + name: value for name, value in list(globals().items())
                         if name.startswith("EVAL_") and isinstance(value, int)}
EVAL_SIGNATURES = {
    "dvd_eval_strerror": "s i",
    "dvd_eval_pool_features": "i ip liii p p",
    "dvd_eval_moments_state_doubles": "l i",
    "dvd_eval_moments_update": "i p lil pp i p",
    "dvd_eval_kid_ws_doubles": "l ii",
    "dvd_eval_kid": "i pll pll i pppp ii ppp p",
}

# libdvdgan_hip_prdc.so (include/dvdgan_hip_prdc.h): k-nearest-neighbour radii and ball counts of sample features (precision /
# recall / density / coverage, distmetrics.py)
PRDC_MAX_D, PRDC_MAX_K, PRDC_TILE, PRDC_MAX_ROWS = 4096, 16, 64, 1 << 24
PRDC_HEADER_CONSTANTS = {"DVD_" + name: value for name, value in list(globals().items())
                         if name.startswith("PRDC_") and isinstance(value, int)}
PRDC_SIGNATURES = {
    "dvd_prdc_strerror": "s i",
    "dvd_prdc_column_mean": "i p lil p p",
    "dvd_prdc_knn_ws_doubles": "l li",
    "dvd_prdc_knn_radii": "i p lil p i pp p",
    "dvd_prdc_ball_ws_doubles": "l ll",
    "dvd_prdc_ball_count": "i pll pll i p p p pp p",
}

# libdvdgan_hip_aug.so (include/dvdgan_hip_aug.h): clip-consistent augmentation of the discriminators' inputs and its transpose
# (augment.py)
AUG_ABI_VERSION = 1
AUG_COLS = 9
(AUG_B, AUG_S, AUG_C, AUG_DX, AUG_DY, AUG_CY0, AUG_CX0, AUG_CH, AUG_CW) = range(AUG_COLS)
AUG_MAX_SIDE, AUG_THREADS, AUG_MAX_FRAMES = 4096, 256, (1 << 24) - 1
AUG_HEADER_CONSTANTS = {"DVD_" + name: value for name, value in list(globals().items())
                        if name.startswith("AUG_") and isinstance(value, int)}
AUG_SIGNATURES = {
    "dvd_aug_abi_version": "i",
    "dvd_aug_strerror": "s i",
    "dvd_aug_clip_forward": "i ppp liii p",
    "dvd_aug_clip_backward": "i ppp liii p",
}

# libdvdgan_hip_geom.so (include/dvdgan_hip_geom.h): the clip-consistent affine warp of the discriminators' inputs and its
# transpose (geom_augment.py)
GEOM_ABI_VERSION = 1
GEOM_COLS = 6
(GEOM_A00, GEOM_A01, GEOM_A02, GEOM_A10, GEOM_A11, GEOM_A12) = range(GEOM_COLS)
GEOM_MAX_SIDE, GEOM_THREADS, GEOM_MAX_FRAMES = 4096, 256, (1 << 24) - 1
GEOM_HEADER_CONSTANTS = {"DVD_" + name: value for name, value in list(globals().items())
                         if name.startswith("GEOM_") and isinstance(value, int)}
GEOM_SIGNATURES = {
    "dvd_geom_abi_version": "i",
    "dvd_geom_strerror": "s i",
    "dvd_geom_clip_forward": "i ppp liii p",
    "dvd_geom_clip_backward": "i ppp liii p",
}

# libdvdgan_hip_sv.so (include/dvdgan_hip_sv.h): the top singular values of a table of weight matrices by block power iteration
# (spectral.py)
SV_ABI_VERSION = 1
SV_MAX_BLOCK, SV_MAX_SWEEPS, SV_MAX_ITEMS, SV_MAX_ITERS = 16, 60, 65535, 4096
SV_HEADER_CONSTANTS = {"DVD_" + name: value for name, value in list(globals().items())
                       if name.startswith("SV_") and isinstance(value, int)}
SV_SIGNATURES = {
    "dvd_sv_abi_version": "i",
    "dvd_sv_item_size": "i",
    "dvd_sv_strerror": "s i",
    "dvd_sv_prepare": "i pii pp",
    "dvd_sv_init": "i ppii pp p",
    "dvd_sv_iterate": "i ppii i p p",
    "dvd_sv_ritz": "i ppii i ppp ll p",
}

# ---- The extension family (xsrc/<key>/*.hip -> xsrc/libdvdx_<key>.so, include/dvdx_<key>.h, EXTENSIONS below): same records, same
# handshake.  libdvdx_tsru.so (include/dvdx_tsru.h): warp-and-gate kernels of the TSRU recurrent unit (functional.ConvTSRULayer)
TSRU_ABI_VERSION = 1
TSRU_MAX_FLOW, TSRU_MAX_SIDE, TSRU_THREADS = 8, 1024, 256
TSRU_HEADER_CONSTANTS = {"DVDX_" + name: value for name, value in list(globals().items())
                         if name.startswith("TSRU_") and isinstance(value, int)}
TSRU_SIGNATURES = {
    "dvdx_tsru_abi_version": "i",
    "dvdx_tsru_strerror": "s i",
    "dvdx_tsru_forward": "i i pp iii pi f pp iiii p",
    "dvdx_tsru_backward": "i i pppp iii pi f p iii pi ppp iiii p",
}

# libdvdx_cr.so (include/dvdx_cr.h, MORE_EXTENSIONS below): the pair loss of balanced consistency regularization on a
# discriminator's logits, its two gradients and its statistics row (functional.CRLoss)
CR_ABI_VERSION = 1
CR_MAX_N, CR_THREADS, CR_NSTAT = 1 << 20, 256, 5
(CR_STAT_PENALTY, CR_STAT_MSQ, CR_STAT_MAXABS, CR_STAT_NONZERO, CR_STAT_N) = range(CR_NSTAT)
CR_HEADER_CONSTANTS = {"DVDX_" + name: value for name, value in list(globals().items())
                       if name.startswith("CR_") and isinstance(value, int)}
CR_SIGNATURES = {
    "dvdx_cr_abi_version": "i",
    "dvdx_cr_strerror": "s i",
    "dvdx_cr_pair": "i pp l f ppp p p",
}

# libdvdx_zcr.so (include/dvdx_zcr.h, ZCR_EXTENSIONS below): the clip distance of latent consistency regularization between the
# generator's clips of the base and of the perturbed latents, its statistics row and its gradient (functional.PairDistance)
ZCR_ABI_VERSION = 1
ZCR_MAX_PAIRS, ZCR_MAX_N, ZCR_THREADS, ZCR_MAX_BLOCKS, ZCR_MIN_CHUNK, ZCR_NSTAT = 1 << 16, 1 << 40, 256, 2048, 4096, 6
(ZCR_STAT_TERM, ZCR_STAT_MSQ, ZCR_STAT_MIN_PAIR, ZCR_STAT_MAX_PAIR, ZCR_STAT_MAXABS, ZCR_STAT_PAIRS) = range(ZCR_NSTAT)
ZCR_HEADER_CONSTANTS = {"DVDX_" + name: value for name, value in list(globals().items())
                        if name.startswith("ZCR_") and isinstance(value, int)}
ZCR_SIGNATURES = {
    "dvdx_zcr_abi_version": "i",
    "dvdx_zcr_strerror": "s i",
    "dvdx_zcr_chunks": "l ll",
    "dvdx_zcr_ws_doubles": "l ll",
    "dvdx_zcr_dist": "i pp ll f pl pp p",
    "dvdx_zcr_dist_grad": "i pp ll f p pp p",
}

# libdvdx_cls.so (include/dvdx_cls.h, CLS_EXTENSIONS below): the per-split sums of a classifier's logits behind the Inception Score
# and the class-fidelity metrics (classmetrics.LogitStats)
CLS_ABI_VERSION = 1
CLS_F32, CLS_BF16, CLS_F16 = 0, 1, 2
CLS_MAX_CLASSES, CLS_MAX_ROWS, CLS_MAX_SPLITS, CLS_MAX_TOTAL, CLS_ROW_BYTES, CLS_NSTAT = 4096, 1 << 20, 1024, 1 << 40, 40, 8
(CLS_STAT_N, CLS_STAT_A, CLS_STAT_BAD, CLS_STAT_LABELLED, CLS_STAT_LOGLIK, CLS_STAT_TOP1, CLS_STAT_TOP5,
 CLS_STAT_BAD_LABEL) = range(CLS_NSTAT)
CLS_HEADER_CONSTANTS = {"DVDX_" + name: value for name, value in list(globals().items())
                        if name.startswith("CLS_") and isinstance(value, int)}
CLS_SIGNATURES = {
    "dvdx_cls_abi_version": "i",
    "dvdx_cls_strerror": "s i",
    "dvdx_cls_ws_bytes": "l li",
    "dvdx_cls_update": "i i pp li ll i pp pl p",
}


class SvItem(C.Structure):              # == dvd_sv_item
    _fields_ = [("W", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("state_off", C.c_longlong), ("ws_off", C.c_longlong),
                ("h", C.c_int), ("w", C.c_int), ("slot", C.c_int), ("blk_wv", C.c_int), ("blk_wtv", C.c_int), ("pad_", C.c_int)]


ABI_VERSION = 13


def check(code):
    if code != 0:
        reset_gru_tickets()           # a failed / aborted launch may have left split-K tickets behind: the next one must start from zero
        _fail("core", code)


def dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported storage dtype {t.dtype}")


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA tensors"
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_tickets = {}


def reset_gru_tickets(current_stream_only=False):
    """Zero the cached ticket buffers (all of them, or the current stream's; the fill runs on the current stream).  The in-launch split-K combine assumes zeroed counters and
    restores them itself, but only when a launch runs to completion: called after any failed library call and once per training
    step (one 32 KB fill), so a faulted or killed launch cannot make later ConvGRU passes skip or mis-time their gate epilogues."""
    for (index, st), t in list(_tickets.items()):
        try:
            if current_stream_only and st != torch.cuda.current_stream(t.device).cuda_stream:
                continue
            t.zero_()
        except Exception:
            pass


def gru_tickets(device):
    """The zero-initialised counters of dvd_gru_desc.tickets for the current stream of `device` (every launch leaves them at
    zero, so one buffer per stream serves every ConvGRU layer issued on it)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    t = _tickets.get(key)
    if t is None:
        t = _tickets[key] = torch.zeros(GRU_TICKETS, dtype=torch.int32, device=device)
    return t


class GruDesc(C.Structure):
    _fields_ = [("dtype", C.c_int), ("T", C.c_int), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("hidden", C.c_int), ("k", C.c_int), ("gx_stride", C.c_longlong),
                ("gx", C.c_void_p), ("w_ur", C.c_void_p), ("w_o", C.c_void_p), ("wd_ur", C.c_void_p),
                ("wd_o", C.c_void_p), ("h0", C.c_void_p),
                ("h_all", C.c_void_p), ("u_all", C.c_void_p), ("r_all", C.c_void_p), ("o_all", C.c_void_p),
                ("hr_all", C.c_void_p), ("h32", C.c_void_p), ("ws", C.c_void_p),
                ("dh_out", C.c_void_p), ("dg", C.c_void_p), ("carry", C.c_void_p), ("dh0", C.c_void_p),
                ("infer", C.c_int),
                ("w_ur_q", C.c_void_p), ("w_o_q", C.c_void_p), ("wd_ur_q", C.c_void_p), ("wd_o_q", C.c_void_p),
                ("tickets", C.c_void_p), ("combine_max", C.c_int), ("ns_cap", C.c_int)]


class GruStackDesc(C.Structure):        # == dvd_gru_stack_desc
    _fields_ = [("n_layers", C.c_int), ("layer_policy", C.c_int), ("run", C.c_int), ("cin", C.c_int * GRU_STACK_MAX),
                ("layer", GruDesc * GRU_STACK_MAX),
                ("wx", C.c_void_p * GRU_STACK_MAX), ("wx_q", C.c_void_p * GRU_STACK_MAX), ("bx", C.c_void_p * GRU_STACK_MAX),
                ("wdx", C.c_void_p * GRU_STACK_MAX), ("wdx_q", C.c_void_p * GRU_STACK_MAX), ("dh_mid", C.c_void_p * GRU_STACK_MAX),
                ("ws", C.c_void_p)]


class SnItem(C.Structure):              # == dvd_sn_item
    _fields_ = [("W", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("sigma", C.c_void_p),
                ("wf", C.c_void_p), ("wd", C.c_void_p), ("h", C.c_int), ("w", C.c_int),
                ("dtype", C.c_int), ("cout", C.c_int), ("cin", C.c_int), ("ntaps", C.c_int), ("cip", C.c_int), ("cop", C.c_int),
                ("blk_wtu", C.c_int), ("blk_wv", C.c_int), ("blk_pack", C.c_int), ("pad_", C.c_int)]


class PackItem(C.Structure):            # == dvd_pack_item
    _fields_ = [("w", C.c_void_p), ("sigma", C.c_void_p), ("wf", C.c_void_p), ("wd", C.c_void_p),
                ("Cout", C.c_int), ("Cin", C.c_int), ("ntaps", C.c_int), ("Cip", C.c_int), ("co_off", C.c_int),
                ("co_tot_f", C.c_int), ("co_tot_d", C.c_int), ("kt", C.c_int), ("kh", C.c_int), ("kw", C.c_int),
                ("ci_off", C.c_int), ("ci_tot", C.c_int)]


class FragItem(C.Structure):            # == dvd_frag_item
    _fields_ = [("w", C.c_void_p), ("wq", C.c_void_p), ("ntaps", C.c_int), ("Cout", C.c_int), ("C", C.c_int)]


# dvd_struct_size(which) -> ctypes mirror (DVD_STRUCT_* of include/dvdgan_hip.h)
STRUCT_MIRRORS = {STRUCT_CONV: ConvDesc, STRUCT_WGRAD: WgradDesc, STRUCT_GRU: GruDesc, STRUCT_SN_ITEM: SnItem,
                  STRUCT_GRU_STACK: GruStackDesc, STRUCT_PACK_ITEM: PackItem, STRUCT_FRAG_ITEM: FragItem}


class Library(NamedTuple):
    """One shared library and its published header: everything _load() checks.  so, env and header follow csrc/build.sh's
    convention -- csrc/<key>/*.hip -> libdvdgan_hip_<key>.so, declared by include/dvdgan_hip_<key>.h; the top level is "core"."""
    so: str                 # file name under csrc/
    env: str                # environment variable that overrides the path (A/B builds)
    header: str             # file name under include/
    signatures: dict        # entry point -> type codes (_CTYPES)
    constants: dict         # `#define` of the header -> value
    abi: tuple = None       # (version function, the value it must return)
    structs: object = None  # loaded handle -> [(what, its size as the library was compiled, ctypes mirror)]
    strerror: str = None    # the function that words a return code


def _library(key, signatures, constants, **handshake):
    tag = "" if key == "core" else "_" + key
    return Library(f"libdvdgan_hip{tag}.so", f"DVD{tag.upper()}_LIB_PATH", f"dvdgan_hip{tag}.h", signatures, constants, **handshake)


# Adding a library: a directory csrc/<key>/ of .hip files, include/dvdgan_hip_<key>.h and one entry here (tests/test_abi_cpu.py
# holds the three to one another and runs the whole handshake test over the new key).
LIBRARIES = {
    "core": _library("core", SIGNATURES, HEADER_CONSTANTS, abi=("dvd_abi_version", ABI_VERSION), strerror="dvd_strerror",
                     structs=lambda so: [(f"sizeof descriptor {which}", so.dvd_struct_size(which), mirror)
                                         for which, mirror in STRUCT_MIRRORS.items()]),
    "adv": _library("adv", ADV_SIGNATURES, ADV_HEADER_CONSTANTS),
    "eval": _library("eval", EVAL_SIGNATURES, EVAL_HEADER_CONSTANTS, strerror="dvd_eval_strerror"),
    "prdc": _library("prdc", PRDC_SIGNATURES, PRDC_HEADER_CONSTANTS, strerror="dvd_prdc_strerror"),
    "aug": _library("aug", AUG_SIGNATURES, AUG_HEADER_CONSTANTS, abi=("dvd_aug_abi_version", AUG_ABI_VERSION),
                    strerror="dvd_aug_strerror"),
    "geom": _library("geom", GEOM_SIGNATURES, GEOM_HEADER_CONSTANTS, abi=("dvd_geom_abi_version", GEOM_ABI_VERSION),
                     strerror="dvd_geom_strerror"),
    "sv": _library("sv", SV_SIGNATURES, SV_HEADER_CONSTANTS, abi=("dvd_sv_abi_version", SV_ABI_VERSION), strerror="dvd_sv_strerror",
                   structs=lambda so: [("sizeof(dvd_sv_item)", so.dvd_sv_item_size(), SvItem)]),
}


def _extension(key, signatures, constants, **handshake):
    return Library(f"libdvdx_{key}.so", f"DVDX_{key.upper()}_LIB_PATH", f"dvdx_{key}.h", signatures, constants, **handshake)


# The second family, beside the first because tests/test_abi_cpu.py fixes the first one's set of libraries, directories and headers:
# a directory xsrc/<key>/ of .hip files, include/dvdx_<key>.h and one entry here.
EXTENSIONS = {
    "tsru": _extension("tsru", TSRU_SIGNATURES, TSRU_HEADER_CONSTANTS, abi=("dvdx_tsru_abi_version", TSRU_ABI_VERSION),
                       strerror="dvdx_tsru_strerror"),
}
assert not set(LIBRARIES) & set(EXTENSIONS)
# The rest of the second family -- same directory (xsrc/), same records, same build loop -- in a table of its own because
# tests/test_tsru_cpu.py fixes EXTENSIONS to its one key and load_extensions() to its one handle.
MORE_EXTENSIONS = {
    "cr": _extension("cr", CR_SIGNATURES, CR_HEADER_CONSTANTS, abi=("dvdx_cr_abi_version", CR_ABI_VERSION), strerror="dvdx_cr_strerror"),
}
assert not (set(LIBRARIES) | set(EXTENSIONS)) & set(MORE_EXTENSIONS)
# ... and a fourth table for the same reason: tests/test_cr_cpu.py fixes MORE_EXTENSIONS to its one key and
# load_more_extensions() to its one handle.
ZCR_EXTENSIONS = {
    "zcr": _extension("zcr", ZCR_SIGNATURES, ZCR_HEADER_CONSTANTS, abi=("dvdx_zcr_abi_version", ZCR_ABI_VERSION),
                      strerror="dvdx_zcr_strerror"),
}
assert not (set(LIBRARIES) | set(EXTENSIONS) | set(MORE_EXTENSIONS)) & set(ZCR_EXTENSIONS)
# ... and a fifth: tests/test_zcr_cpu.py fixes ZCR_EXTENSIONS to its one key and load_zcr_extensions() to its one handle.
CLS_EXTENSIONS = {
    "cls": _extension("cls", CLS_SIGNATURES, CLS_HEADER_CONSTANTS, abi=("dvdx_cls_abi_version", CLS_ABI_VERSION),
                      strerror="dvdx_cls_strerror"),
}
assert not (set(LIBRARIES) | set(EXTENSIONS) | set(MORE_EXTENSIONS) | set(ZCR_EXTENSIONS)) & set(CLS_EXTENSIONS)
_handles = {}           # key -> checked handle; _handles.pop(key, None) drops one, and the next accessor call loads it again


def _record(key):
    """The Library record of a key of any of the five tables."""
    for table in (LIBRARIES, EXTENSIONS, MORE_EXTENSIONS, ZCR_EXTENSIONS):
        if key in table:
            return table[key]
    return CLS_EXTENSIONS[key]


def library_path(key):
    """Where the library of `key` is loaded from: its environment variable, read now, or csrc/ (xsrc/ for an extension) of this tree."""
    rec = _record(key)
    return os.environ.get(rec.env) or os.path.join(_HERE, "csrc" if key in LIBRARIES else "xsrc", rec.so)


def _load(key):
    """The loaded library of the table row `key`.  The first call dlopens it and runs its whole handshake; the handle is published only after
    every check has passed.  Raises (never falls back) when the library has not been built or disagrees with this file."""
    if key in _handles:
        return _handles[key]
    rec, path = _record(key), library_path(key)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(dvd_gan_amd has no CPU / eager fallback)")
    loaded = C.CDLL(path)
    # ABI handshake first: a stale build is told to rebuild, not that one of its entry points is missing
    if rec.abi and hasattr(loaded, rec.abi[0]) and getattr(loaded, rec.abi[0])() != rec.abi[1]:
        raise RuntimeError(f"{rec.so} ABI version mismatch: rebuild it")
    # signature handshake: every entry point gets its declared types, so a plain Python int reaches a `long long` whole
    for name, sig in rec.signatures.items():
        fn = getattr(loaded, name, None)
        if fn is None:
            raise RuntimeError(f"{rec.so} exports no {name} -- lib.py and include/{rec.header} disagree")
        fn.restype, fn.argtypes = _CTYPES[sig[0]], [_CTYPES[a] for a in sig[1:].replace(" ", "")]
    # layout handshake: every struct mirror must have the size the library was compiled with
    for what, size, mirror in (rec.structs(loaded) if rec.structs else ()):
        if size != C.sizeof(mirror):
            raise RuntimeError(f"{rec.so}: {what} is {size}, the ctypes mirror {mirror.__name__} has {C.sizeof(mirror)} bytes "
                               f"-- lib.py and include/{rec.header} disagree")
    _handles[key] = loaded
    return loaded


def load_all():
    """Every library of the table, loaded and checked (what __graft_entry__.build() ends with)."""
    return [_load(key) for key in LIBRARIES]


def load_extensions():
    """Every library of the extension table, loaded and checked (__graft_entry__.build() calls it after load_all())."""
    return [_load(key) for key in EXTENSIONS]


def load_more_extensions():
    """Every library of MORE_EXTENSIONS, loaded and checked (__graft_entry__.build() calls it after load_extensions())."""
    return [_load(key) for key in MORE_EXTENSIONS]


def load_zcr_extensions():
    """Every library of ZCR_EXTENSIONS, loaded and checked (__graft_entry__.build() calls it after load_more_extensions())."""
    return [_load(key) for key in ZCR_EXTENSIONS]


def load_cls_extensions():
    """Every library of CLS_EXTENSIONS, loaded and checked (__graft_entry__.build() calls it after load_zcr_extensions())."""
    return [_load(key) for key in CLS_EXTENSIONS]


def _fail(key, code):
    rec = _record(key)
    raise RuntimeError(f"{rec.so[:-3]}: {getattr(_load(key), rec.strerror)(code).decode()} (code {code})")


def _checker(key):
    def check_code(code):
        if code != 0:                   # (once per launch: nothing but this test when the call succeeded)
            _fail(key, code)
    return check_code


def _accessor(key):
    def handle():
        try:                            # once per launch on the hot path: one dict subscript when loaded
            return _handles[key]
        except KeyError:
            return _load(key)
    handle.__doc__ = f"The loaded {_record(key).so}, typed from its signature table.  Raises (never falls back) when it has not been built."
    return handle


# The accessors and checks call sites use: one view of the table each.
lib = _accessor("core")
adv_lib = _accessor("adv")
eval_lib = _accessor("eval")
prdc_lib = _accessor("prdc")
aug_lib = _accessor("aug")
geom_lib = _accessor("geom")
sv_lib = _accessor("sv")
eval_check = _checker("eval")
prdc_check = _checker("prdc")
aug_check = _checker("aug")
geom_check = _checker("geom")
sv_check = _checker("sv")
tsru_lib = _accessor("tsru")
tsru_check = _checker("tsru")
cr_lib = _accessor("cr")
cr_check = _checker("cr")
zcr_lib = _accessor("zcr")
zcr_check = _checker("zcr")
cls_lib = _accessor("cls")
cls_check = _checker("cls")


# the paths as this import found them (tools and tests that inspect the files)
LIB_PATH, ADV_LIB_PATH, EVAL_LIB_PATH, PRDC_LIB_PATH, AUG_LIB_PATH, GEOM_LIB_PATH, SV_LIB_PATH = map(library_path, LIBRARIES)

"""ctypes binding of libdvdgan_hip.so (include/dvdgan_hip.h).  Fails loudly: no fallback."""
import ctypes as C
import os

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
LIB_PATH = os.environ.get("DVD_LIB_PATH") or os.path.join(_HERE, "csrc", "libdvdgan_hip.so")    # (override: A/B builds)
_lib = None


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


def lib():
    """The loaded shared library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(dvd_gan_amd has no CPU / eager fallback)")
        _lib = C.CDLL(LIB_PATH)
        if _lib.dvd_abi_version() != ABI_VERSION:
            raise RuntimeError("libdvdgan_hip.so ABI version mismatch: rebuild it")
        # signature handshake: every entry point gets its declared types, so a plain Python int reaches a `long long` whole
        for name, sig in SIGNATURES.items():
            fn = getattr(_lib, name, None)
            if fn is None:
                _lib = None
                raise RuntimeError(f"libdvdgan_hip.so exports no {name} -- lib.py and include/dvdgan_hip.h disagree")
            fn.restype, fn.argtypes = _CTYPES[sig[0]], [_CTYPES[a] for a in sig[1:].replace(" ", "")]
        # layout handshake: every descriptor mirror below must have the size the library was compiled with
        for which, mirror in STRUCT_MIRRORS.items():
            want = _lib.dvd_struct_size(which)
            if want != C.sizeof(mirror):
                _lib = None
                raise RuntimeError(f"libdvdgan_hip.so: sizeof descriptor {which} is {want}, the ctypes mirror {mirror.__name__} has "
                                   f"{C.sizeof(mirror)} bytes -- lib.py and include/dvdgan_hip.h disagree")
    return _lib


# ---- libdvdgan_hip_adv.so (include/dvdgan_hip_adv.h): the loss launch with LeCam regularization, top-k selection and logit
# statistics, a library of its own with the same handshake -- every `#define DVD_ADV_*` of its header by name, one line of
# type codes per entry point (tests/test_adv_ref_cpu.py compares both with the header and the exports with the table)
ADV_MAX_SAMPLES, ADV_NSTAT = 4096, 8        # samples a selection serves, floats of the statistics
(ADV_STAT_MEAN, ADV_STAT_SIGN, ADV_STAT_ACTIVE, ADV_STAT_ADV, ADV_STAT_LECAM, ADV_STAT_ANCHOR, ADV_STAT_KEPT,
 ADV_STAT_NONFINITE) = range(ADV_NSTAT)
ADV_HEADER_CONSTANTS = {"DVD_" + name: value for name, value in list(globals().items())
                        if name.startswith("ADV_") and isinstance(value, int)}
ADV_SIGNATURES = {
    "dvd_adv_loss_ex": "i p l iiii f ppp f pp f p p",
}
ADV_LIB_PATH = os.environ.get("DVD_ADV_LIB_PATH") or os.path.join(_HERE, "csrc", "libdvdgan_hip_adv.so")
_adv_lib = None


def adv_lib():
    """The loaded libdvdgan_hip_adv.so, typed from ADV_SIGNATURES.  Raises (never falls back) when it has not been built."""
    global _adv_lib
    if _adv_lib is None:
        if not os.path.exists(ADV_LIB_PATH):
            raise RuntimeError(
                f"{ADV_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(dvd_gan_amd has no CPU / eager fallback)")
        loaded = C.CDLL(ADV_LIB_PATH)
        for name, sig in ADV_SIGNATURES.items():
            fn = getattr(loaded, name, None)
            if fn is None:
                raise RuntimeError(f"libdvdgan_hip_adv.so exports no {name} -- lib.py and include/dvdgan_hip_adv.h disagree")
            fn.restype, fn.argtypes = _CTYPES[sig[0]], [_CTYPES[a] for a in sig[1:].replace(" ", "")]
        _adv_lib = loaded
    return _adv_lib


# ---- libdvdgan_hip_eval.so (include/dvdgan_hip_eval.h): pooled features, running moments and kernel distances of sample
# features (distmetrics.py), the third library with the same handshake (tests/test_distmetrics_cpu.py compares the constants and
# the table with the header and the exports with the table)
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
EVAL_LIB_PATH = os.environ.get("DVD_EVAL_LIB_PATH") or os.path.join(_HERE, "csrc", "libdvdgan_hip_eval.so")
_eval_lib = None


def eval_lib():
    """The loaded libdvdgan_hip_eval.so, typed from EVAL_SIGNATURES.  Raises (never falls back) when it has not been built."""
    global _eval_lib
    if _eval_lib is None:
        if not os.path.exists(EVAL_LIB_PATH):
            raise RuntimeError(
                f"{EVAL_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(dvd_gan_amd has no CPU / eager fallback)")
        loaded = C.CDLL(EVAL_LIB_PATH)
        for name, sig in EVAL_SIGNATURES.items():
            fn = getattr(loaded, name, None)
            if fn is None:
                raise RuntimeError(f"libdvdgan_hip_eval.so exports no {name} -- lib.py and include/dvdgan_hip_eval.h disagree")
            fn.restype, fn.argtypes = _CTYPES[sig[0]], [_CTYPES[a] for a in sig[1:].replace(" ", "")]
        _eval_lib = loaded
    return _eval_lib


def eval_check(code):
    if code != 0:
        raise RuntimeError(f"libdvdgan_hip_eval: {eval_lib().dvd_eval_strerror(code).decode()} (code {code})")


# ---- libdvdgan_hip_prdc.so (include/dvdgan_hip_prdc.h): k-nearest-neighbour radii and ball counts of sample features (precision /
# recall / density / coverage, distmetrics.py), the fourth library with the same handshake (tests/test_prdc_cpu.py compares the
# constants and the table with the header and the exports with the table)
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
PRDC_LIB_PATH = os.environ.get("DVD_PRDC_LIB_PATH") or os.path.join(_HERE, "csrc", "libdvdgan_hip_prdc.so")
_prdc_lib = None


def prdc_lib():
    """The loaded libdvdgan_hip_prdc.so, typed from PRDC_SIGNATURES.  Raises (never falls back) when it has not been built."""
    global _prdc_lib
    if _prdc_lib is None:
        if not os.path.exists(PRDC_LIB_PATH):
            raise RuntimeError(
                f"{PRDC_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(dvd_gan_amd has no CPU / eager fallback)")
        loaded = C.CDLL(PRDC_LIB_PATH)
        for name, sig in PRDC_SIGNATURES.items():
            fn = getattr(loaded, name, None)
            if fn is None:
                raise RuntimeError(f"libdvdgan_hip_prdc.so exports no {name} -- lib.py and include/dvdgan_hip_prdc.h disagree")
            fn.restype, fn.argtypes = _CTYPES[sig[0]], [_CTYPES[a] for a in sig[1:].replace(" ", "")]
        _prdc_lib = loaded
    return _prdc_lib


def prdc_check(code):
    if code != 0:
        raise RuntimeError(f"libdvdgan_hip_prdc: {prdc_lib().dvd_prdc_strerror(code).decode()} (code {code})")


# ---- libdvdgan_hip_aug.so (include/dvdgan_hip_aug.h): clip-consistent augmentation of the discriminators' inputs and its
# transpose (augment.py), the fifth library with the same handshake (tests/test_aug_cpu.py compares the constants and the table
# with the header and the exports with the table)
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
AUG_LIB_PATH = os.environ.get("DVD_AUG_LIB_PATH") or os.path.join(_HERE, "csrc", "libdvdgan_hip_aug.so")
_aug_lib = None


def aug_lib():
    """The loaded libdvdgan_hip_aug.so, typed from AUG_SIGNATURES.  Raises (never falls back) when it has not been built."""
    global _aug_lib
    if _aug_lib is None:
        if not os.path.exists(AUG_LIB_PATH):
            raise RuntimeError(
                f"{AUG_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(dvd_gan_amd has no CPU / eager fallback)")
        loaded = C.CDLL(AUG_LIB_PATH)
        for name, sig in AUG_SIGNATURES.items():
            fn = getattr(loaded, name, None)
            if fn is None:
                raise RuntimeError(f"libdvdgan_hip_aug.so exports no {name} -- lib.py and include/dvdgan_hip_aug.h disagree")
            fn.restype, fn.argtypes = _CTYPES[sig[0]], [_CTYPES[a] for a in sig[1:].replace(" ", "")]
        if loaded.dvd_aug_abi_version() != AUG_ABI_VERSION:
            raise RuntimeError("libdvdgan_hip_aug.so ABI version mismatch: rebuild it")
        _aug_lib = loaded
    return _aug_lib


def aug_check(code):
    if code != 0:
        raise RuntimeError(f"libdvdgan_hip_aug: {aug_lib().dvd_aug_strerror(code).decode()} (code {code})")


# ---- libdvdgan_hip_geom.so (include/dvdgan_hip_geom.h): the clip-consistent affine warp of the discriminators' inputs and its
# transpose (geom_augment.py), the sixth library with the same handshake (tests/test_geom_cpu.py compares the constants and the
# table with the header and the exports with the table)
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
GEOM_LIB_PATH = os.environ.get("DVD_GEOM_LIB_PATH") or os.path.join(_HERE, "csrc", "libdvdgan_hip_geom.so")
_geom_lib = None


def geom_lib():
    """The loaded libdvdgan_hip_geom.so, typed from GEOM_SIGNATURES.  Raises (never falls back) when it has not been built."""
    global _geom_lib
    if _geom_lib is None:
        if not os.path.exists(GEOM_LIB_PATH):
            raise RuntimeError(
                f"{GEOM_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(dvd_gan_amd has no CPU / eager fallback)")
        loaded = C.CDLL(GEOM_LIB_PATH)
        for name, sig in GEOM_SIGNATURES.items():
            fn = getattr(loaded, name, None)
            if fn is None:
                raise RuntimeError(f"libdvdgan_hip_geom.so exports no {name} -- lib.py and include/dvdgan_hip_geom.h disagree")
            fn.restype, fn.argtypes = _CTYPES[sig[0]], [_CTYPES[a] for a in sig[1:].replace(" ", "")]
        if loaded.dvd_geom_abi_version() != GEOM_ABI_VERSION:
            raise RuntimeError("libdvdgan_hip_geom.so ABI version mismatch: rebuild it")
        _geom_lib = loaded
    return _geom_lib


def geom_check(code):
    if code != 0:
        raise RuntimeError(f"libdvdgan_hip_geom: {geom_lib().dvd_geom_strerror(code).decode()} (code {code})")


# ---- libdvdgan_hip_sv.so (include/dvdgan_hip_sv.h): the top singular values of a table of weight matrices by block power
# iteration (spectral.py), the seventh library with the same handshake (tests/test_sv_cpu.py compares the constants and the
# table with the header and the exports with the table)
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
SV_LIB_PATH = os.environ.get("DVD_SV_LIB_PATH") or os.path.join(_HERE, "csrc", "libdvdgan_hip_sv.so")
_sv_lib = None


class SvItem(C.Structure):              # == dvd_sv_item
    _fields_ = [("W", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("state_off", C.c_longlong), ("ws_off", C.c_longlong),
                ("h", C.c_int), ("w", C.c_int), ("slot", C.c_int), ("blk_wv", C.c_int), ("blk_wtv", C.c_int), ("pad_", C.c_int)]


def sv_lib():
    """The loaded libdvdgan_hip_sv.so, typed from SV_SIGNATURES.  Raises (never falls back) when it has not been built."""
    global _sv_lib
    if _sv_lib is None:
        if not os.path.exists(SV_LIB_PATH):
            raise RuntimeError(
                f"{SV_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(dvd_gan_amd has no CPU / eager fallback)")
        loaded = C.CDLL(SV_LIB_PATH)
        for name, sig in SV_SIGNATURES.items():
            fn = getattr(loaded, name, None)
            if fn is None:
                raise RuntimeError(f"libdvdgan_hip_sv.so exports no {name} -- lib.py and include/dvdgan_hip_sv.h disagree")
            fn.restype, fn.argtypes = _CTYPES[sig[0]], [_CTYPES[a] for a in sig[1:].replace(" ", "")]
        if loaded.dvd_sv_abi_version() != SV_ABI_VERSION:
            raise RuntimeError("libdvdgan_hip_sv.so ABI version mismatch: rebuild it")
        if loaded.dvd_sv_item_size() != C.sizeof(SvItem):
            raise RuntimeError(f"libdvdgan_hip_sv.so: sizeof(dvd_sv_item) is {loaded.dvd_sv_item_size()}, the ctypes mirror SvItem has "
                               f"{C.sizeof(SvItem)} bytes -- lib.py and include/dvdgan_hip_sv.h disagree")
        _sv_lib = loaded
    return _sv_lib


def sv_check(code):
    if code != 0:
        raise RuntimeError(f"libdvdgan_hip_sv: {sv_lib().dvd_sv_strerror(code).decode()} (code {code})")


ABI_VERSION = 13


def check(code):
    if code != 0:
        reset_gru_tickets()           # a failed / aborted launch may have left split-K tickets behind: the next one must start from zero
        raise RuntimeError(f"libdvdgan_hip: {lib().dvd_strerror(code).decode()} (code {code})")


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

"""Tensor-level wrappers over the C ABI (one Python function per entry point).

Internal activation layout: channels-last, [frames, (T,) H, W, Cp] with Cp = channels padded to a
multiple of 8, storage dtype torch.float32 (exact mode) or torch.bfloat16.
"""
import ctypes as C
import os

import torch

from . import lib as L
from .lib import (GUARD_CH, GUARD_STATE, METRICS_QUANTIZE, METRICS_SIGNED, ORTHO_COLS, ORTHO_H, ORTHO_OFF, ORTHO_W, SHEET_FILL,
                  SHEET_SIGNED)       # (public names of this module; the values live with the other header constants)


def pad8(c):
    return (c + 7) // 8 * 8


def _ksize3(k):
    k = tuple(k)
    return (1,) * (3 - len(k)) + k


# ------------------------------------------------------------------ layout
def to_cl(x, dtype, swap=None):
    """fp32 [F, C, *spatial] -> [F, *spatial, pad8(C)] in `dtype`.  swap=(A, B): the F = A*B source
    frames (a-major) are written b-major."""
    x = x.contiguous()
    F_, Cc = x.shape[0], x.shape[1]
    sp = tuple(x.shape[2:])
    P = 1
    for s in sp:
        P *= s
    out = torch.empty((F_,) + sp + (pad8(Cc),), dtype=dtype, device=x.device)
    A, B = swap if swap else (F_, 1)
    L.check(L.lib().dvd_to_channels_last(L.dt(out), L.ptr(x), L.ptr(out), F_, Cc, P, pad8(Cc), A, B, 1 if swap else 0,
                                         L.stream()))
    return out


def from_cl(t, channels, swap=None):
    """[F, *spatial, Cp] -> fp32 [F, channels, *spatial] (inverse of to_cl, same `swap`)."""
    t = t.contiguous()
    F_, sp, Cp = t.shape[0], tuple(t.shape[1:-1]), t.shape[-1]
    P = 1
    for s in sp:
        P *= s
    out = torch.empty((F_, channels) + sp, dtype=torch.float32, device=t.device)
    A, B = swap if swap else (F_, 1)
    L.check(L.lib().dvd_from_channels_last(L.dt(t), L.ptr(t), L.ptr(out), F_, channels, P, Cp, A, B, 1 if swap else 0,
                                           L.stream()))
    return out


def convert(src, dtype):
    out = torch.empty(src.shape, dtype=dtype, device=src.device)
    L.check(L.lib().dvd_convert(L.dt(src), L.ptr(src), L.dt(out), L.ptr(out), src.numel(), L.stream()))
    return out


# ------------------------------------------------------------------ weights
class PackedConv:
    """Forward pack wf [ntaps][Cout_tot][Cip] and backward-data pack wd [ntaps][Cip][Cop]."""

    def __init__(self, dtype, cout_tot, cin, ksize, device, need_dgrad=True, single_fill=False, covered=False):
        """single_fill: ONE fill() call will cover all cout_tot output channels -- it writes every element of both
        images (zeros in the padded input channels) except the padded output columns of `wd`, so only a `wd` with
        cout_tot % 8 != 0 needs the zero fill.  covered: the caller's SEVERAL fill() calls together cover every output
        channel (the fused gate packs of a ConvGRU layer): same consequence."""
        self.k = _ksize3(ksize)
        self.ntaps = self.k[0] * self.k[1] * self.k[2]
        self.cout, self.cin, self.cip, self.cop = cout_tot, cin, pad8(cin), pad8(cout_tot)
        af = torch.empty if (single_fill or covered) else torch.zeros
        ad = torch.empty if ((single_fill or covered) and self.cop == cout_tot) else torch.zeros
        self.wf = af(self.ntaps, cout_tot, self.cip, dtype=dtype, device=device)
        self.wd = ad(self.ntaps, self.cip, self.cop, dtype=dtype, device=device) if need_dgrad else None

    def fragment_major(self, which="wf"):
        """The forward ("wf") or backward-data ("wd") image once more in fragment-major order (dvd_conv_fragment_major), for
        the convolution kernel that reads its weight operand straight from L2; built on first use, after the last fill()."""
        wants = getattr(self, "wants", None)
        if wants is not None:
            wants.add(which)              # (the owner prepares this image ahead of time from the next forward on: sn_layers.prefetch_spectral_norm)
        q = getattr(self, which + "q", None)
        if q is None:
            src = getattr(self, which)
            cout, c = (self.cout, self.cip) if which == "wf" else (self.cip, self.cop)
            n = L.lib().dvd_conv_fragment_major_bytes(self.ntaps, cout, c)
            q = torch.empty(n // 2, dtype=src.dtype, device=src.device)
            L.check(L.lib().dvd_conv_fragment_major(L.dt(src), L.ptr(src), L.ptr(q), self.ntaps, cout, c, L.stream()))
            setattr(self, which + "q", q)
        return q

    def fill(self, w, sigma=None, co_off=0, ci_off=0):
        """w: fp32 master [Cout_part, Cin_tot, *k] of which input channels [ci_off, ci_off+cin) are
        packed as output rows [co_off, co_off+Cout_part); sigma: device scalar tensor or None."""
        assert w.is_contiguous() and w.dtype == torch.float32
        L.check(L.lib().dvd_pack_conv_weight(
            L.dt(self.wf), L.ptr(w), L.ptr(sigma), w.shape[0], self.cin, self.ntaps, self.cip, co_off,
            self.cout, self.cop, L.ptr(self.wf), L.ptr(self.wd), self.k[0], self.k[1], self.k[2],
            ci_off, w.shape[1], L.stream()))
        return self


PACK_BATCH = os.environ.get("DVD_PACK_BATCH", "1") != "0"
# timing-only experiment (WRONG results): 1 = BN statistics from 4096 rows, 2 = CBN backward sums from two frames -- what folding
# those two passes into the neighbouring convolutions' epilogues could return at most (profiles/HISTORY.md, round 6)
EXP_CBN = int(os.environ.get("DVD_EXP_CBN", "0"))


class PackBatch:
    """Deferred PackedConv.fill / fragment_major calls issued as ONE launch each (dvd_pack_conv_weight_batched,
    dvd_conv_fragment_major_batched): the 18 gate packs and up to 18 fragment-major images of a three-layer ConvGRU were 36+
    launches of 6-18 us on the stream in front of its first convolution."""

    def __init__(self):
        self.fills, self.frags, self.dtype = [], [], None

    def fill(self, pk, w, sigma=None, co_off=0, ci_off=0):
        assert w.is_contiguous() and w.dtype == torch.float32
        it = L.PackItem()
        it.w, it.sigma, it.wf, it.wd = w.data_ptr(), L.ptr(sigma), L.ptr(pk.wf), L.ptr(pk.wd)
        it.Cout, it.Cin, it.ntaps, it.Cip, it.co_off = w.shape[0], pk.cin, pk.ntaps, pk.cip, co_off
        it.co_tot_f, it.co_tot_d = pk.cout, pk.cop
        it.kt, it.kh, it.kw = pk.k
        it.ci_off, it.ci_tot = ci_off, w.shape[1]
        assert self.dtype in (None, pk.wf.dtype)
        self.dtype = pk.wf.dtype
        self.fills.append((it, w, sigma, pk))
        return self

    def fragment_major(self, pk, which="wf"):
        """Schedules the fragment-major image of `pk.<which>` (built by run(), after the fills) and returns the tensor it will be in."""
        q = getattr(pk, which + "q", None)
        if q is None:
            src = getattr(pk, which)
            cout, c = (pk.cout, pk.cip) if which == "wf" else (pk.cip, pk.cop)
            n = L.lib().dvd_conv_fragment_major_bytes(pk.ntaps, cout, c)
            q = torch.empty(n // 2, dtype=src.dtype, device=src.device)
            it = L.FragItem()
            it.w, it.wq, it.ntaps, it.Cout, it.C = src.data_ptr(), q.data_ptr(), pk.ntaps, cout, c
            self.frags.append((it, src, q))
            setattr(pk, which + "q", q)
        return q

    def run(self):
        dt_ = L.BF16 if self.dtype == torch.bfloat16 else L.F32
        if not PACK_BATCH:                # A/B aid: one launch per item, as before round 6
            for it, *_ in self.fills:
                L.check(L.lib().dvd_pack_conv_weight(dt_, it.w, it.sigma, it.Cout, it.Cin, it.ntaps, it.Cip, it.co_off, it.co_tot_f,
                                                     it.co_tot_d, it.wf, it.wd, it.kt, it.kh, it.kw, it.ci_off, it.ci_tot, L.stream()))
            for it, *_ in self.frags:
                L.check(L.lib().dvd_conv_fragment_major(L.BF16, it.w, it.wq, it.ntaps, it.Cout, it.C, L.stream()))
        else:
            if self.fills:
                arr = (L.PackItem * len(self.fills))(*[f[0] for f in self.fills])
                L.check(L.lib().dvd_pack_conv_weight_batched(dt_, arr, len(self.fills), L.stream()))
            if self.frags:
                arr = (L.FragItem * len(self.frags))(*[f[0] for f in self.frags])
                L.check(L.lib().dvd_conv_fragment_major_batched(L.BF16, arr, len(self.frags), L.stream()))
        self.fills, self.frags = [], []


# ------------------------------------------------------------------ convolution
def wants_fragment_major(dtype, frames, H, W, cin, cout, k, nsplit=1):
    """True when a [frames, H, W, C] -> cout convolution with k x k taps (nsplit K slices) runs through the kernel that takes a
    fragment-major weight image (dvd_conv_wants_fragment_major)."""
    if dtype != torch.bfloat16:
        return False
    d = L.ConvDesc()
    d.dtype, d.frames, d.T, d.H, d.W = L.BF16, frames, 1, H, W
    d.C, d.ldi, d.Cout, d.ldo = cin, cin, cout, cout
    d.kt, d.kh, d.kw, d.nsplit = 1, k, k, max(1, nsplit)
    d.inp = d.out = d.w = 1               # (never dereferenced: geometry query)
    if nsplit > 1:
        d.ws = 1
    return bool(L.lib().dvd_conv_wants_fragment_major(C.byref(d)))


def _grid(x, ksize, up2):
    """(frames, T, H, W) of the OUTPUT for input x [F,(T,)H,W,C]."""
    if x.dim() == 5:
        F_, T, H, W = x.shape[:4]
    elif x.dim() == 4:
        F_, H, W = x.shape[:3]
        T = 1
    elif x.dim() == 2:
        F_, T, H, W = x.shape[0], 1, 1, 1
    else:
        raise ValueError("expected [F,(T,)H,W,C] or [F,C]")
    if up2:
        H, W = H * 2, W * 2
    return F_, T, H, W


def _thin_image(wpack, kt):
    """The [tap row][k half][channel block][lane][8] image of a [kt*9][64][8] pack for the thin-input convolution kernel
    (dvd_conv_thin_image); cached on the pack tensor (packs are rebuilt whenever the weights change)."""
    img = getattr(wpack, "_thin_img", None)
    if img is None:
        n = L.lib().dvd_conv_thin_image_bytes(kt)
        img = torch.empty(n // 2, dtype=wpack.dtype, device=wpack.device)
        L.check(L.lib().dvd_conv_thin_image(L.ptr(wpack), L.ptr(img), kt, L.stream()))
        wpack._thin_img = img
    return img


def _thin_out_image(wpack):
    """The [tap][16-channel step][lane][8] image of a [9][rows <= 8][64] pack for the thin-output convolution kernel."""
    img = getattr(wpack, "_thin_img", None)
    if img is None:
        img = torch.empty(L.lib().dvd_conv_thin_out_image_bytes() // 2, dtype=wpack.dtype, device=wpack.device)
        L.check(L.lib().dvd_conv_thin_out_image(L.ptr(wpack), L.ptr(img), wpack.shape[1], L.stream()))
        wpack._thin_img = img
    return img


def conv_forward(x, wpack, ksize, cout, *, bias=None, res=None, mask=None, act=L.ACT_NONE, up2=False,
                 relu_in=False, out=None, out_f32=False, nsplit=1, ws=None, slabs=False, cout_pad=None, res_up2=False, wq=None,
                 pool2=False):
    """Direct (nsplit=1) or split-K convolution.  `wpack`: [ntaps][cout][Cp] tensor.  Returns the
    output tensor [F,(T,)H,W,cout_pad] (direct) or the fp32 slabs [nsplit, M, cout] (split-K).
    pool2: return the 2 x 2 SUMS of the result on the half-size grid [F, H/2, W/2, cout_pad] (`mask` lives there too), formed in the
    kernel's epilogue -- or None when this request is not served that way (the caller then pools a full-size result)."""
    k = _ksize3(ksize)
    F_, T, H, W = _grid(x, ksize, up2)
    Cp = x.shape[-1]
    M = F_ * T * H * W
    d = L.ConvDesc()
    d.dtype, d.frames, d.T, d.H, d.W = L.dt(x), F_, T, H, W
    d.C, d.ldi, d.Cout = Cp, Cp, cout
    d.kt, d.kh, d.kw = k
    d.up2, d.relu_in, d.nsplit, d.act, d.out_f32 = int(up2), int(relu_in), nsplit, act, int(out_f32)
    d.pool2 = int(pool2)                  # before the weight-image query: the thin kernels do not serve pool2 requests
    d.inp, d.w, d.bias = x.data_ptr(), wpack.data_ptr(), (bias.data_ptr() if bias is not None else None)
    if res is not None:
        d.res, d.ldres, d.res_up2 = res.data_ptr(), res.shape[-1], int(res_up2)
    if mask is not None:
        d.mask, d.ldmask = mask.data_ptr(), mask.shape[-1]
    if callable(wq):                      # lazily built fragment-major image: only when this request runs through that kernel
        d.nsplit, d.out = max(1, nsplit), 1          # (placeholders for the geometry query; the real pointers are set below)
        d.ldo = out.shape[-1] if out is not None else (cout_pad or pad8(cout))
        d.ws = 1 if (nsplit > 1 or slabs or ws is not None) else None
        want = L.lib().dvd_conv_wants_fragment_major(C.byref(d)) if x.dtype == torch.bfloat16 else 0
        wq = wq() if want == 1 else _thin_image(wpack, k[0]) if want == 2 else _thin_out_image(wpack) if want == 3 else None
        d.wq_kind = want if wq is not None else 0
    d.wq = wq.data_ptr() if wq is not None else None
    d.out = d.ws = None
    if pool2:
        d.ldo = cout_pad or pad8(cout)
        if x.dim() != 4 or nsplit > 1 or slabs or ws is not None or not L.lib().dvd_conv_pool2_ok(C.byref(d)):
            return None
        shape = (F_, H // 2, W // 2, d.ldo)
        alloc = torch.zeros if d.ldo != cout else torch.empty
        out = alloc(shape, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
        d.out = out.data_ptr()
        L.check(L.lib().dvd_conv_forward(C.byref(d), L.stream()))
        return out
    nk = k[0] * k[1] * k[2] * ((Cp + (31 if x.dtype == torch.bfloat16 else 15)) // (32 if x.dtype == torch.bfloat16 else 16))
    nsplit = d.nsplit = max(1, min(nsplit, nk))
    if nsplit > 1 or slabs or ws is not None:
        if ws is None:
            ws = torch.empty(nsplit, M, cout, dtype=torch.float32, device=x.device)
        d.ws, d.ldo = ws.data_ptr(), cout
        L.check(L.lib().dvd_conv_forward(C.byref(d), L.stream()))
        return ws
    cp_out = cout_pad or pad8(cout)
    if out is None:
        shape = ((F_,) if x.dim() == 2 else (F_, H, W) if x.dim() == 4 else (F_, T, H, W)) + (cp_out,)
        alloc = torch.zeros if cp_out != cout else torch.empty
        out = alloc(shape, dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    d.out, d.ldo = out.data_ptr(), out.shape[-1]
    L.check(L.lib().dvd_conv_forward(C.byref(d), L.stream()))
    return out


def conv_wgrad(x, dy, dw, ksize, cout, cin_real, *, up2=False, relu_in=False, msplit=0, dy_col=0,
               dw_ci_off=0, dw_ci_tot=None, frames=None, x_row0=0, dy_row0=0, dbias=None, overwrite=False):
    """dw[co][dw_ci_off + ci][*k] += sum_rows dy[row][dy_col + co] * x[shifted row][ci]   (fp32 atomics)
    dw: fp32 master-layout tensor [cout][dw_ci_tot][*k].  x / dy may be row-sliced views given by
    (tensor, first frame): `frames` frames starting at frame x_row0 of x and dy_row0 of dy."""
    k = _ksize3(ksize)
    F_, T, H, W = _grid(x, ksize, up2)
    if frames is not None:
        F_ = frames
    ntaps = k[0] * k[1] * k[2]
    esz = x.element_size()
    ci_tot = dw_ci_tot if dw_ci_tot is not None else cin_real
    if dy_col % 8 or dw_ci_off + cin_real > ci_tot:      # dy is read in 16-byte vectors from the shifted pointer; the window lies inside dw
        raise ValueError(f"conv_wgrad: dy_col {dy_col} is not a multiple of 8, or dw window [{dw_ci_off}, {dw_ci_off + cin_real}) exceeds {ci_tot}")
    d = L.WgradDesc()
    d.dtype, d.frames, d.T, d.H, d.W = L.dt(x), F_, T, H, W
    d.C, d.ldx, d.Cin_real = x.shape[-1], x.shape[-1], cin_real
    cy = min(pad8(cout), dy.shape[-1] - dy_col)
    d.Cout, d.Cy, d.ldy = cout, cy, dy.shape[-1]
    d.kt, d.kh, d.kw = k
    d.up2, d.relu_in, d.msplit = int(up2), int(relu_in), msplit
    d.s_co, d.s_ci, d.s_tap = ci_tot * ntaps, ntaps, 1
    rows_in = T * (H // 2 if up2 else H) * (W // 2 if up2 else W)
    d.x = x.data_ptr() + x_row0 * rows_in * x.shape[-1] * esz
    d.dy = dy.data_ptr() + (dy_row0 * T * H * W * dy.shape[-1] + dy_col) * esz
    d.dw = dw.data_ptr() + dw_ci_off * ntaps * 4
    d.dbias = dbias.data_ptr() if dbias is not None else None      # fp32 [cout], accumulated
    d.overwrite = int(overwrite)                                    # dw = result (dense dw only): `dw` may be torch.empty
    nws = L.lib().dvd_conv_wgrad_ws_floats(C.byref(d))              # >0: deterministic two-phase reduction
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws > 0 else None
    d.ws = ws.data_ptr() if ws is not None else None
    L.check(L.lib().dvd_conv_wgrad(C.byref(d), L.stream()))
    return dw


# ------------------------------------------------------------------ pointwise wrappers
def bn_stats(x, C_real, training, eps, momentum, run_mean, run_var, replicas=None, sums=None):
    """-> (mean, rstd) fp32 [C_real]; updates the running buffers in training mode.
    sums: optional PERSISTENT zeroed fp64 workspace [BN_NREP * 2 * C_real] of the caller -- dvd_bn_finalize leaves it zeroed
    again, so no fill is launched per call.
    replicas: None, or (world, all_reduce_sum_) for cross-replica statistics -- the [BN_NREP][2C] fp64 sums are added over the
    replicas before mean / variance are formed from world * rows samples."""
    ld = x.shape[-1]
    rows = x.numel() // ld
    mean = torch.empty(C_real, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    keep = sums is not None and training
    if not keep:
        sums = None
    try:
        if training:
            if sums is None:
                sums = torch.zeros(L.BN_NREP * 2 * C_real, dtype=torch.float64, device=x.device)
            if EXP_CBN & 1:               # timing experiment (wrong statistics): the pass over x reads 4096 rows only
                rows = min(rows, 4096)
            L.check(L.lib().dvd_bn_stats(L.dt(x), L.ptr(x), rows, C_real, ld, L.ptr(sums), L.stream()))
            if replicas is not None:
                replicas[1](sums)
                rows *= replicas[0]
        L.check(L.lib().dvd_bn_finalize(L.ptr(sums), rows, C_real, eps, momentum, int(training),
                                        L.ptr(mean), L.ptr(rstd), L.ptr(run_mean), L.ptr(run_var), int(keep), L.stream()))
    except Exception:
        if keep:
            sums.zero_()                  # a failed call must not leave a dirty workspace behind
        raise
    return mean, rstd


def cbn_apply(x, C_real, mean, rstd, gb, samp, relu):
    y = torch.empty_like(x)
    frames = x.shape[0]
    P = x.numel() // (frames * x.shape[-1])
    L.check(L.lib().dvd_cbn_apply(L.dt(x), L.ptr(x), L.ptr(y), frames, P, C_real, x.shape[-1], L.ptr(mean),
                                  L.ptr(rstd), L.ptr(gb), L.ptr(samp), int(relu), L.stream()))
    return y


def cbn_backward(g, a, x, C_real, mean, rstd, gb, samp, relu, replicas=None):
    """-> (dx, dgb[B][2C]).  replicas: as in bn_stats -- the two per-channel sums of the batch-norm backward are added
    over the replicas between the reduce and the apply stage."""
    dx = torch.empty_like(x)
    frames = x.shape[0]
    P = x.numel() // (frames * x.shape[-1])
    B = gb.shape[0]
    dgb = torch.zeros_like(gb)
    s12 = torch.empty(2 * C_real, dtype=torch.float32, device=x.device)
    part = torch.empty(L.lib().dvd_cbn_backward_ws_floats(frames, P, C_real), dtype=torch.float32, device=x.device)   # fixed-order dgb
    if EXP_CBN & 2 and replicas is None:      # timing experiment (wrong sums): the reduce pass reads two frames only
        L.check(L.lib().dvd_cbn_backward_reduce(L.dt(x), L.ptr(g), L.ptr(a), L.ptr(x), min(frames, 2), P, C_real, x.shape[-1],
                                                L.ptr(mean), L.ptr(rstd), L.ptr(gb), L.ptr(samp), B, L.ptr(dgb), L.ptr(s12),
                                                int(relu), L.ptr(part), L.stream()))
        L.check(L.lib().dvd_cbn_backward_apply(L.dt(x), L.ptr(g), L.ptr(a), L.ptr(x), L.ptr(dx), frames, P, C_real,
                                               x.shape[-1], L.ptr(mean), L.ptr(rstd), L.ptr(gb), L.ptr(samp), L.ptr(s12),
                                               frames * P, int(relu), L.stream()))
        return dx, dgb
    if replicas is None:
        L.check(L.lib().dvd_cbn_backward(L.dt(x), L.ptr(g), L.ptr(a), L.ptr(x), L.ptr(dx), frames, P, C_real,
                                         x.shape[-1], L.ptr(mean), L.ptr(rstd), L.ptr(gb), L.ptr(samp), B, L.ptr(dgb),
                                         L.ptr(s12), int(relu), L.ptr(part), L.stream()))
        return dx, dgb
    L.check(L.lib().dvd_cbn_backward_reduce(L.dt(x), L.ptr(g), L.ptr(a), L.ptr(x), frames, P, C_real, x.shape[-1],
                                            L.ptr(mean), L.ptr(rstd), L.ptr(gb), L.ptr(samp), B, L.ptr(dgb), L.ptr(s12),
                                            int(relu), L.ptr(part), L.stream()))
    replicas[1](s12)
    L.check(L.lib().dvd_cbn_backward_apply(L.dt(x), L.ptr(g), L.ptr(a), L.ptr(x), L.ptr(dx), frames, P, C_real,
                                           x.shape[-1], L.ptr(mean), L.ptr(rstd), L.ptr(gb), L.ptr(samp), L.ptr(s12),
                                           frames * P * replicas[0], int(relu), L.stream()))
    return dx, dgb


def _grid4(x):
    if x.dim() == 5:
        return x.shape[0], x.shape[1], x.shape[2], x.shape[3]
    return x.shape[0], 1, x.shape[1], x.shape[2]


def pool(x, pt=1, scale=None, mask=None):
    """(pt,2,2) window sum * scale (default: average); mask (shape of the result): zero where mask <= 0."""
    F_, T, H, W = _grid4(x)
    To, Ho, Wo = T // pt, H // 2, W // 2
    scale = (1.0 / (4 * pt)) if scale is None else scale
    shape = (F_, To, Ho, Wo, x.shape[-1]) if x.dim() == 5 else (F_, Ho, Wo, x.shape[-1])
    y = torch.empty(shape, dtype=x.dtype, device=x.device)
    if mask is not None:
        assert mask.shape == y.shape and mask.dtype == y.dtype and not ((H | W) & 1)
        L.check(L.lib().dvd_pool_masked(L.dt(x), L.ptr(x), L.ptr(mask), L.ptr(y), F_, To, Ho, Wo, x.shape[-1], pt, scale,
                                        L.stream()))
        return y
    L.check(L.lib().dvd_pool(L.dt(x), L.ptr(x), L.ptr(y), F_, To, Ho, Wo, H, W, x.shape[-1], pt, scale, L.stream()))
    return y


def unpool(x, pt=1, scale=None, out_hw=None):
    """nearest replication to (T*pt, 2H, 2W) times scale (default 1/(4*pt): gradient of avg-pool).  out_hw = (2H+1 | 2H, 2W+1 |
    2W): the grid a floored pooling started from -- its odd last line / column gets zeros."""
    F_, T, H, W = _grid4(x)
    To, Ho, Wo = T * pt, H * 2, W * 2
    if out_hw is not None:
        Ho, Wo = out_hw
        assert Ho // 2 == H and Wo // 2 == W
    scale = (1.0 / (4 * pt)) if scale is None else scale
    shape = (F_, To, Ho, Wo, x.shape[-1]) if x.dim() == 5 else (F_, Ho, Wo, x.shape[-1])
    y = torch.empty(shape, dtype=x.dtype, device=x.device)
    L.check(L.lib().dvd_unpool(L.dt(x), L.ptr(x), L.ptr(y), F_, To, Ho, Wo, x.shape[-1], pt, scale, L.stream()))
    return y


def colsum(x, C_real, out=None):
    ld = x.shape[-1]
    if out is None:
        out = torch.zeros(C_real, dtype=torch.float32, device=x.device)
    L.check(L.lib().dvd_colsum(L.dt(x), L.ptr(x), x.numel() // ld, C_real, ld, L.ptr(out), L.stream()))
    return out


def add(a, b):
    out = torch.empty_like(a)
    L.check(L.lib().dvd_add(L.dt(a), L.ptr(a), L.ptr(b), L.ptr(out), a.numel(), L.stream()))
    return out


def sum_leading(x):
    out = torch.empty(x.shape[1:], dtype=x.dtype, device=x.device)
    L.check(L.lib().dvd_sum_leading(L.dt(x), L.ptr(x), L.ptr(out), x.shape[0], out.numel(), L.stream()))
    return out


def act_backward(dy, y, act):
    dx = torch.empty_like(dy)
    L.check(L.lib().dvd_act_backward(L.dt(dy), L.ptr(dy), L.ptr(y), L.ptr(dx), dy.numel(), act, L.stream()))
    return dx


def vid_downsample_raw(src, backward, shape_fwd_in):
    B, T, Cc, H, W = shape_fwd_in
    out = torch.empty((B, T, Cc, H, W) if backward else (B, Cc, T, H // 2, W // 2), dtype=torch.float32,
                      device=src.device)
    L.check(L.lib().dvd_vid_downsample(L.ptr(src), L.ptr(out), B, T, Cc, H, W, int(backward), L.stream()))
    return out


def vid_downsample_cat_raw(a, b):
    """vid_downsample(cat([a, b], 1)) of two fp32 clips [B, Ta, C, H, W] / [B, Tb, C, H, W] -> [B, C, Ta+Tb, H/2, W/2]."""
    B, Ta, Cc, H, W = a.shape
    Tb = b.shape[1]
    out = torch.empty(B, Cc, Ta + Tb, H // 2, W // 2, dtype=torch.float32, device=b.device)
    L.check(L.lib().dvd_vid_downsample_cat(L.ptr(a), Ta, L.ptr(b), Tb, L.ptr(out), B, Cc, H, W, 0, L.stream()))
    return out


def vid_downsample_cat_backward(g, Ta, shape_b, db=None):
    """Gradient of vid_downsample_cat_raw wrt b from g [B, C, Ta+Tb, H/2, W/2] (the context frames get none)."""
    B, Tb, Cc, H, W = shape_b
    if db is None:
        db = torch.empty(shape_b, dtype=torch.float32, device=g.device)
    L.check(L.lib().dvd_vid_downsample_cat(None, Ta, L.ptr(db), Tb, L.ptr(g), B, Cc, H, W, 1, L.stream()))
    return db


def row_copy(src, idx, nrows_out, L_, scatter, out=None):
    """gather: out[r] = src[idx[r]] ; scatter: out[idx[r]] = src[r] (out pre-zeroed, nrows_out rows)."""
    if out is None:
        out = (torch.zeros if scatter else torch.empty)(nrows_out, L_, dtype=torch.float32, device=src.device)
    L.check(L.lib().dvd_row_copy(L.ptr(src), L.ptr(out), L.ptr(idx), idx.numel(), L_, int(scatter), L.stream()))
    return out


# ------------------------------------------------------------------ spectral norm / small fp32 layers
def sn_power_iter(w_bar, u, v, sigma=None):
    """In-place u, v update; returns the 1-element sigma tensor (a fresh one unless `sigma` is given)."""
    if sigma is None:
        sigma = torch.empty(1, dtype=torch.float32, device=w_bar.device)
    h = w_bar.shape[0]
    L.check(L.lib().dvd_sn_power_iter(L.ptr(w_bar), h, w_bar.numel() // h, L.ptr(u), L.ptr(v), L.ptr(sigma), L.stream()))
    return sigma


def sn_backward(G, w_bar, u, v, sigma, out=None):
    """dL/dW_bar from G = dL/d(W_bar / sigma); `out`: fp32 buffer the result is ADDED to (default: a fresh zero tensor)."""
    dW = torch.zeros_like(w_bar) if out is None else out
    scratch = torch.empty(L.SN_SCRATCH, dtype=torch.float32, device=w_bar.device)
    h = w_bar.shape[0]
    L.check(L.lib().dvd_sn_backward(L.ptr(G), L.ptr(w_bar), L.ptr(u), L.ptr(v), L.ptr(sigma), h, w_bar.numel() // h,
                                    L.ptr(dW), L.ptr(scratch), L.stream()))
    return dW


def linear_forward(inp, W, bias):
    B, K = inp.shape
    J = W.shape[0]
    out = torch.empty(B, J, dtype=torch.float32, device=inp.device)
    L.check(L.lib().dvd_linear_forward(L.ptr(inp), L.ptr(W), L.ptr(bias), L.ptr(out), B, K, J, L.stream()))
    return out


def linear_backward(dout, inp, W, need_in, need_w, has_bias, dW=None, db=None):
    """dW / db given: fp32 buffers the kernels ADD into (persistent .grad); else fresh zero tensors."""
    B, K = inp.shape
    J = W.shape[0]
    din = torch.empty_like(inp) if need_in else None
    if dW is None:
        dW = torch.zeros_like(W) if need_w else None
        db = torch.zeros(J, dtype=torch.float32, device=inp.device) if (need_w and has_bias) else None
    L.check(L.lib().dvd_linear_backward(L.ptr(dout), L.ptr(inp), L.ptr(W), L.ptr(din), 0, L.ptr(dW), L.ptr(db), B, K, J,
                                        L.stream()))
    return din, dW, db


def embedding_backward(dout, idx, nrows, dW=None):
    if dW is None:
        dW = torch.zeros(nrows, dout.shape[1], dtype=torch.float32, device=dout.device)
    L.check(L.lib().dvd_embedding_backward(L.ptr(dout), L.ptr(idx), L.ptr(dW), dout.shape[0], dout.shape[1], L.stream()))
    return dW


def adam_step(p, g, m, v, lr, b1, b2, eps, step):
    L.check(L.lib().dvd_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), float(lr), b1, b2, eps, int(step),
                                  L.stream()))


def adam_ema_step(p, g, m, v, ema, lr, b1, b2, eps, step, decay):
    """adam_step and ema = decay * ema + (1 - decay) * p_new in one launch."""
    L.check(L.lib().dvd_adam_ema_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel(), float(lr), b1, b2, eps,
                                      int(step), float(decay), L.stream()))


GUARD_NORM, GUARD_COEF, GUARD_BAD, GUARD_SKIP, GUARD_SEEN, GUARD_SKIPPED, GUARD_CLIPPED = range(7)


def GUARD_CHAIN(n):
    """The longest chain of fp64 additions between an element of an n-element gradient and the sum of squares dvd_grad_guard takes
    the root of (csrc/guard.hip), every addition counted, the first one into an accumulator's zero (which is exact) included:
    16 rounds of a thread's accumulator (GUARD_CH / (256 threads * 4 accumulators)), 2 to join the four accumulators, 6 xor
    shuffles, 3 to add the four waves; then in the finalizing workgroup ceil(workgroups / 1024) partials per thread, 6 shuffles
    and 15 to add the sixteen waves.  All terms are >= 0, so |S - exact| <= GUARD_CHAIN(n) * 2^-53 * exact to first order; the
    exact first addition leaves room for the second-order terms and for the rounding of a correctly rounded reference sum."""
    nwg = -(-int(n) // GUARD_CH)
    return GUARD_CH // 1024 + 2 + 6 + 3 + -(-nwg // 1024) + 6 + 15


def grad_guard_ws_bytes(n):
    return int(L.lib().dvd_grad_guard_ws_bytes(int(n)))


def grad_guard_ws_views(ws, n):
    """-> (partial float64[W], S float64[1], bad int32[W]): views of a dvd_grad_guard workspace for an n-element gradient."""
    nwg = -(-int(n) // GUARD_CH)
    d = ws[:(nwg + 1) * 8].view(torch.float64)
    return d[:nwg], d[nwg:], ws[(nwg + 1) * 8:(nwg + 1) * 8 + nwg * 4].view(torch.int32)


def grad_guard(g, max_norm, skip_nonfinite, step, ws, state, ring=None):
    """dvd_grad_guard: the fp64 norm of the finite part of the flat fp32 gradient g, the clipping coefficient for `max_norm`
    (float("inf") = measure only) and the skip decision into `state` (float64[GUARD_STATE], zeroed before its first use); `ring`
    (float64[R][4], optional) receives row (step - 1) % R = step, norm, coef, bad.  Two launches, no host sync."""
    assert g.dtype == torch.float32 and state.dtype == torch.float64 and state.numel() == GUARD_STATE
    assert ring is None or (ring.dtype == torch.float64 and ring.dim() == 2 and ring.shape[1] == 4)
    L.check(L.lib().dvd_grad_guard(L.ptr(g), g.numel(), float(max_norm), int(bool(skip_nonfinite)), int(step), L.ptr(ws),
                                   L.ptr(state), L.ptr(ring), 0 if ring is None else int(ring.shape[0]), L.stream()))


def adam_guard_step(p, g, m, v, ema, lr, b1, b2, eps, step, decay, state):
    """adam_ema_step (ema a tensor) or adam_step (ema None) on g * coef32 of `state`; on a skipped step nothing is written."""
    L.check(L.lib().dvd_adam_guard_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel(), float(lr), b1, b2, eps,
                                        int(step), float(decay), L.ptr(state), L.stream()))


def ortho_prepare(items):
    """dvd_ortho_prepare on a contiguous CPU int64 table [n][ORTHO_COLS] whose off / h / w columns are filled: fills the planner's
    columns in place (host only, no device) and returns (tiles of M = penalty slots, workspace floats)."""
    assert items.dtype == torch.int64 and not items.is_cuda and items.is_contiguous() and items.dim() == 2 \
        and items.shape[1] == ORTHO_COLS
    lib = L.lib()
    ws = C.c_longlong(0)
    tiles = lib.dvd_ortho_prepare(items.data_ptr(), int(items.shape[0]), C.byref(ws))
    if tiles < 0:
        L.check(int(tiles))
    return int(tiles), int(ws.value)


def ortho_grad(p, g, items_host, items_dev, strength, ws, penalty=None):
    """g += 2 * strength * M W for every matrix of the prepared table (views of the flat fp32 buffers p and g at equal offsets),
    M = W W^T with a zero diagonal, in two launches; `penalty` (a float64 device scalar) receives sum 1/2 ||M||_F^2."""
    assert p.dtype == g.dtype == torch.float32 and (penalty is None or penalty.dtype == torch.float64)
    L.check(L.lib().dvd_ortho_grad(L.ptr(p), L.ptr(g), items_host.data_ptr(), L.ptr(items_dev),
                                   int(items_host.shape[0]), float(strength), L.ptr(ws), L.ptr(penalty), L.stream()))


def zcr_ws_doubles(pairs, n):
    """Doubles of the workspace zcr_dist needs for fp32 [pairs, n] halves (dvdx_zcr_ws_doubles; 0: a shape it refuses)."""
    return int(L.zcr_lib().dvdx_zcr_ws_doubles(int(pairs), int(n)))


def zcr_dist(a, b, pairs, n, weight, ws, term, stats=None):
    """term[0] <- -weight * mean((a - b)^2) over the fp32 [pairs, n] halves a, b (views welcome: only their data pointers are
    taken), stats (None or fp32 [lib.ZCR_NSTAT]) <- the statistics row; ws: float64 [zcr_ws_doubles(pairs, n)].  Two launches."""
    assert ws.dtype == torch.float64 and term.dtype == torch.float32
    L.zcr_check(L.zcr_lib().dvdx_zcr_dist(L.ptr(a), L.ptr(b), int(pairs), int(n), float(weight), L.ptr(ws), ws.numel(), L.ptr(term),
                                          L.ptr(stats), L.stream()))


def zcr_dist_grad(a, b, pairs, n, weight, upstream, da, db):
    """da, db [pairs, n] <- the gradients of upstream[0] * zcr_dist's term; `upstream` is a DEVICE fp32 scalar, never read here."""
    assert upstream.dtype == torch.float32 and upstream.numel() == 1
    L.zcr_check(L.zcr_lib().dvdx_zcr_dist_grad(L.ptr(a), L.ptr(b), int(pairs), int(n), float(weight), L.ptr(upstream), L.ptr(da),
                                               L.ptr(db), L.stream()))


def ema_step(ema, p, decay):
    L.check(L.lib().dvd_ema_step(L.ptr(ema), L.ptr(p), p.numel(), float(decay), L.stream()))


def swap_(a, b):
    """Exchange the contents of two fp32 tensors of equal size."""
    assert a.numel() == b.numel() and a.dtype == b.dtype == torch.float32
    L.check(L.lib().dvd_swap_f32(L.ptr(a), L.ptr(b), a.numel(), L.stream()))


def frame_metrics(pred, p_strides, target, t_strides, B, T, Cc, H, W, flags, mse, ssim):
    """dvd_frame_metrics on two device fp32 tensors (views welcome: only their data pointers are taken) whose (batch, time,
    channel) strides in elements are p_strides / t_strides and whose H x W planes are contiguous; fills the fp32 device
    buffers mse / ssim (B * T values each, frame b * T + t)."""
    lib = L.lib()
    nbytes = lib.dvd_frame_metrics_ws_bytes(int(B), T, Cc, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device) if nbytes else None
    L.check(lib.dvd_frame_metrics(pred.data_ptr(), *map(int, p_strides), target.data_ptr(), *map(int, t_strides), int(B), T, Cc,
                                  H, W, int(flags), L.ptr(mse), L.ptr(ssim), L.ptr(ws), L.stream()))


def clip_gather(blob, clips_host, clips_dev, tables, out, ms, norm_value=255.0):
    """dvd_clip_gather: uint8 device blob of decoded frames -> `out` fp32 [B, 3, T, S, S] (crop, Pillow's 8-bit bilinear resize,
    flip, normalise, layout in one launch).  clips_host / clips_dev: the same int64 values on the host (checked there before any
    launch) and on the device -- B rows of lib.CLIP_COLS columns, then the B * T frame indices; tables: the device int32 pool the
    rows' CLIP_XTAB / CLIP_YTAB point into; ms: device float[6] = mean RGB | std RGB."""
    B, three, T, S, S2 = out.shape
    assert three == 3 and S == S2 and out.dtype == torch.float32 and blob.dtype == torch.uint8 and tables.dtype == torch.int32
    assert clips_host.dtype == clips_dev.dtype == torch.int64 and not clips_host.is_cuda and clips_host.is_contiguous()
    assert clips_host.numel() == clips_dev.numel() == B * (L.CLIP_COLS + T)
    L.check(L.lib().dvd_clip_gather(L.ptr(blob), blob.numel(), clips_host.data_ptr(), L.ptr(clips_dev), L.ptr(tables),
                                    tables.numel(), L.ptr(out), B, T, S, float(norm_value), L.ptr(ms), L.stream()))
    return out


def sample_sheet_shape(total_slots, H, W, nrow, padding, row_prefix=0):
    """dvd_sample_sheet_shape -> (Hs, Ws, bytes of one sheet) of make_grid's geometry; needs no GPU.  ValueError when refused."""
    hs, ws, nb = C.c_int(0), C.c_int(0), C.c_longlong(0)
    rc = L.lib().dvd_sample_sheet_shape(int(total_slots), int(H), int(W), int(nrow), int(padding), int(row_prefix),
                                        C.byref(hs), C.byref(ws), C.byref(nb))
    if rc != 0:
        raise ValueError(f"no sheet of {total_slots} slots of {H} x {W}, nrow={nrow}, padding={padding}: "
                         f"{L.lib().dvd_strerror(rc).decode()} (code {rc})")
    return hs.value, ws.value, nb.value


def sample_sheet(src, strides, n_sheets, n_tiles, H, W, first_slot, total_slots, nrow, padding, pad_value, row_prefix, flags, dst):
    """dvd_sample_sheet: device fp32 `src` (views welcome: only the data pointer is taken) seen as [n_sheets][n_tiles][3][H][W]
    with (sheet, tile, channel) `strides` in elements -> the uint8 device buffer `dst` [n_sheets][Hs][row_prefix + 3 Ws]."""
    assert src.is_cuda and src.dtype == torch.float32 and dst.dtype == torch.uint8 and dst.device == src.device
    L.check(L.lib().dvd_sample_sheet(src.data_ptr(), *map(int, strides), int(n_sheets), int(n_tiles), int(H),
                                     int(W), int(first_slot), int(total_slots), int(nrow), int(padding), float(pad_value),
                                     int(row_prefix), int(flags), L.ptr(dst), L.stream()))
    return dst


# ------------------------------------------------------------------ libdvdgan_hip_eval.so: distribution distances (distmetrics.py)
def _rows_f32(x, what):
    """(tensor, rows, d, row stride) of a device fp32 matrix whose rows are contiguous (a column slice of a wider matrix is served
    without a copy; anything else is made contiguous)."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"{what} must be a device fp32 matrix [rows, d], got {tuple(x.shape)} {x.dtype} on {x.device}")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what} is empty: {tuple(x.shape)}")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, x.shape[0], x.shape[1], (x.stride(0) if x.shape[0] > 1 else x.shape[1])


def eval_pool_features(act, group=1):
    """dvd_eval_pool_features: channels-last activation [R, *spatial, C] (bf16 / fp32) -> fp32 [R / group, C], the mean over
    `group` consecutive rows of sum_positions relu(act)."""
    act = act.contiguous()
    R, Cc = act.shape[0], act.shape[-1]
    P = act.numel() // max(R * Cc, 1)
    group = int(group)
    if group < 1 or R % group:
        raise ValueError(f"group={group} does not divide the {R} rows of the activation")
    out = torch.empty(R // group, Cc, dtype=torch.float32, device=act.device)
    L.eval_check(L.eval_lib().dvd_eval_pool_features(L.dt(act), L.ptr(act), R, P, Cc, group, L.ptr(out), L.stream()))
    return out


def eval_moments_state(d, device):
    """(pivot fp32 [d], state fp64 [S1 | upper-triangular tiles of S2]) for dvd_eval_moments_update; the first update fills both."""
    nd = L.eval_lib().dvd_eval_moments_state_doubles(int(d))
    if nd < 0:
        raise ValueError(f"feature width d={d} outside [1, {L.EVAL_MAX_D}]")
    return torch.empty(int(d), dtype=torch.float32, device=device), torch.empty(nd, dtype=torch.float64, device=device)


def eval_moments_update(x, pivot, state, first):
    """dvd_eval_moments_update: adds the rows of x [n, d] (device fp32, row stride >= d) to the running state; no host sync."""
    x, n, d, ld = _rows_f32(x, "features")
    assert pivot.numel() == d and pivot.dtype == torch.float32 and state.dtype == torch.float64
    L.eval_check(L.eval_lib().dvd_eval_moments_update(x.data_ptr(), n, d, ld, L.ptr(pivot), L.ptr(state), int(bool(first)),
                                                      L.stream()))


def eval_kid(x, y, ix, iy):
    """dvd_eval_kid: x [n, d], y [m, d] device fp32; ix, iy host int32 [n_sub, s] row tables -> (values fp64 [n_sub], terms fp64
    [n_sub, 3]) on the device.  The tables are range-checked on the host and uploaded once."""
    x, n, d, ldx = _rows_f32(x, "x")
    y, m, d2, ldy = _rows_f32(y, "y")
    if d != d2 or x.device != y.device:
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must share the feature width and the device")
    ix = torch.as_tensor(ix, dtype=torch.int32).contiguous()
    iy = torch.as_tensor(iy, dtype=torch.int32).contiguous()
    if ix.dim() != 2 or ix.shape != iy.shape or ix.is_cuda or iy.is_cuda:
        raise ValueError(f"index tables must be host [n_sub, s] of one shape, got {tuple(ix.shape)} / {tuple(iy.shape)}")
    n_sub, s = ix.shape
    lib = L.eval_lib()
    nws = lib.dvd_eval_kid_ws_doubles(n_sub, s)
    if nws < 0:
        L.eval_check(int(nws))
    tab = torch.stack([ix, iy])
    tab_d = tab.to(x.device, non_blocking=False)
    ws = torch.empty(nws, dtype=torch.float64, device=x.device)
    out = torch.empty(n_sub, dtype=torch.float64, device=x.device)
    terms = torch.empty(n_sub, 3, dtype=torch.float64, device=x.device)
    L.eval_check(lib.dvd_eval_kid(x.data_ptr(), n, ldx, y.data_ptr(), m, ldy, d, tab[0].data_ptr(), tab[1].data_ptr(),
                                  tab_d[0].data_ptr(), tab_d[1].data_ptr(), n_sub, s, L.ptr(ws), L.ptr(out), L.ptr(terms),
                                  L.stream()))
    return out, terms


# ------------------------------------------------------------------ libdvdgan_hip_prdc.so: nearest-neighbour radii and ball counts
def _prdc_pivot(pivot, d, device):
    if pivot is None:
        return None
    if pivot.dtype != torch.float32 or pivot.numel() != d or pivot.device != device or not pivot.is_contiguous():
        raise ValueError(f"pivot must be a contiguous device fp32 vector [{d}], got {tuple(pivot.shape)} {pivot.dtype} on {pivot.device}")
    return pivot


def _prdc_ws(n_doubles, device):
    if n_doubles < 0:
        L.prdc_check(int(n_doubles))
    return torch.empty(int(n_doubles), dtype=torch.float64, device=device)


def eval_column_mean(x):
    """dvd_prdc_column_mean: x [n, d] (device fp32, row stride >= d) -> fp32 [d], the column mean as dvd_eval_moments_update's first
    call computes it; no host sync."""
    x, n, d, ld = _rows_f32(x, "features")
    pivot = torch.empty(d, dtype=torch.float32, device=x.device)
    L.prdc_check(L.prdc_lib().dvd_prdc_column_mean(x.data_ptr(), n, d, ld, L.ptr(pivot), L.stream()))
    return pivot


def eval_knn_radii(x, k, pivot=None):
    """dvd_prdc_knn_radii: x [n, d] (device fp32, row stride >= d) -> fp64 [n] on the device, the squared distance of every row to
    its k-th nearest other row (distances of fl32(x - pivot), pivot fp32 [d] or None = zeros); no host sync."""
    x, n, d, ld = _rows_f32(x, "features")
    pivot = _prdc_pivot(pivot, d, x.device)
    lib = L.prdc_lib()
    ws = _prdc_ws(lib.dvd_prdc_knn_ws_doubles(n, int(k)), x.device)
    r2 = torch.empty(n, dtype=torch.float64, device=x.device)
    L.prdc_check(lib.dvd_prdc_knn_radii(x.data_ptr(), n, d, ld, L.ptr(pivot), int(k), L.ptr(ws), L.ptr(r2), L.stream()))
    return r2


def eval_ball_count(q, r, r2=None, pivot=None):
    """dvd_prdc_ball_count: q [nq, d], r [nr, d] (device fp32), r2 fp64 [nr] or None -> (count int32 [nq] or None, dmin fp64 [nq]):
    in how many balls (centre r_i, squared radius r2_i) every row of q lies, and its squared distance to the nearest row of r;
    no host sync."""
    q, nq, d, ldq = _rows_f32(q, "q")
    r, nr, d2, ldr = _rows_f32(r, "r")
    if d != d2 or q.device != r.device:
        raise ValueError(f"q {tuple(q.shape)} and r {tuple(r.shape)} must share the feature width and the device")
    pivot = _prdc_pivot(pivot, d, q.device)
    count = None
    if r2 is not None:
        if r2.dtype != torch.float64 or r2.shape != (nr,) or r2.device != q.device or not r2.is_contiguous():
            raise ValueError(f"r2 must be a contiguous device fp64 vector [{nr}], got {tuple(r2.shape)} {r2.dtype} on {r2.device}")
        count = torch.empty(nq, dtype=torch.int32, device=q.device)
    lib = L.prdc_lib()
    ws = _prdc_ws(lib.dvd_prdc_ball_ws_doubles(nq, nr), q.device)
    dmin = torch.empty(nq, dtype=torch.float64, device=q.device)
    L.prdc_check(lib.dvd_prdc_ball_count(q.data_ptr(), nq, ldq, r.data_ptr(), nr, ldr, d, L.ptr(pivot), L.ptr(r2), L.ptr(ws),
                                         L.ptr(count), L.ptr(dmin), L.stream()))
    return count, dmin

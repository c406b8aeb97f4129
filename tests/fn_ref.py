"""Float64 statements of the autograd Functions of dvd_gan_amd/functional.py (and disc_nets.QKVConv) other than Conv.

A plain module in the style of tests/autograd_ref.py: torch only, no conftest, CPU or GPU tensors alike; no project kernel and no
oracle code takes part.  Every Function is written as DIFFERENTIABLE float64 torch code on the stored operands -- x, qkv, kv, dy
as they sit in bf16 / fp32 channels-last memory, the fp32 parameters, for the projection head the u, v held before the forward --
and its gradients come from torch.autograd in float64 (`grads`), not from hand-written backward formulas.  Two exceptions, both
stated where they are made: the spectral-norm weight gradient goes through autograd_ref.sn_backward_ref (u, v are constants of
the backward pass, and the LATEST ones: quirk 7), and the MFMA attention takes D from the stored att_out (its ABI; that check
lives in tests/test_gpu_attention.py).  tests/test_fn_ref_cpu.py holds these statements to torch.nn.functional and to gradcheck.

Column layout of a fused projection: q | k | v at [0, dq) | [koff, koff + dq) | [voff, voff + C), koff = pad8(dq), voff = 2 koff.
"""
import torch

import autograd_ref as AR


def pad8(c):
    return (c + 7) // 8 * 8


def leaf(t):
    """a float64 leaf copy of a stored tensor"""
    return t.detach().double().clone().requires_grad_(True)


def grads(out, inputs, dout):
    """d<out, dout> / d inputs by torch.autograd (float64); None for an input the output does not depend on"""
    return torch.autograd.grad([out], list(inputs), [dout.double()], allow_unused=True)


def _pad_cols(t, ld):
    return torch.nn.functional.pad(t, (0, ld - t.shape[-1]))


# ------------------------------------------------------------------ conditional batch norm
def cbn(x, gb, samp, C, relu, *, training=True, run_mean=None, run_var=None, eps=1e-5, world=1):
    """y = relu?(gb[s][:C] * (x - mean) * rstd + gb[s][C:]), s = samp[frame]; x [F, .., ld] (channels from C on ignored), gb [B, 2C].
    training: mean / BIASED variance over all rows of the batch; eval: the running buffers.
    world > 1 (replicas=(world, .)): the batch is the data repeated `world` times.  Returns the output of ALL replicas,
    [world * F, .., ld], replica 0 first; the other replicas' data and gb are constants (x.detach(), gb.detach()), so that
    d/dx and d/dgb of <y, dy repeated> are ONE replica's gradients: the statistics' backward sums span the global batch, dgb stays
    per replica.  Pad channels of y are 0."""
    ld, xs = x.shape[-1], x[..., :C]
    if training:
        allx = torch.cat([xs] + [xs.detach()] * (world - 1))
        flat = allx.reshape(-1, C)
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
        gball = torch.cat([gb[samp.long()]] + [gb.detach()[samp.long()]] * (world - 1))
    else:
        allx, mean, var = xs, run_mean.double(), run_var.double()
        gball = gb[samp.long()]
    xh = (allx - mean) / (var + eps).sqrt()
    per_frame = lambda t: t.reshape(t.shape[0], *([1] * (x.dim() - 2)), C)
    y = per_frame(gball[:, :C]) * xh + per_frame(gball[:, C:])
    return _pad_cols(y.clamp_min(0) if relu else y, ld)


# ------------------------------------------------------------------ pooling
def pool(x, pt):
    """(pt, 2, 2) average with floor: x [F, (T,) H, W, C]; a 4-D x has T = 1 (pt = 1)."""
    five = x.dim() == 5
    x5 = x if five else x.unsqueeze(1)
    F_, T, H, W, Cc = x5.shape
    To, Ho, Wo = T // pt, H // 2, W // 2
    win = x5[:, :To * pt, :Ho * 2, :Wo * 2].reshape(F_, To, pt, Ho, 2, Wo, 2, Cc)
    y = win.mean(dim=(2, 4, 6))
    return y if five else y.squeeze(1)


def maxpool3d_windows(x):
    """x [F, T, H, W, C] (even T, H, W) -> [F, T/2, H/2, W/2, C, 8], the window in (t, h, w) scan order"""
    F_, T, H, W, Cc = x.shape
    w = x.reshape(F_, T // 2, 2, H // 2, 2, W // 2, 2, Cc)
    return w.permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(F_, T // 2, H // 2, W // 2, Cc, 8)


def maxpool3d(x):
    """2 x 2 x 2 maximum as an explicit one-hot routing: the window's FIRST maximum in (t, h, w) scan order is selected, so the
    gradient of a tied window goes to that element alone (the tie rule is stated here, not inherited from a library)."""
    win = maxpool3d_windows(x)
    eq = win == win.amax(-1, keepdim=True)
    first = eq & (eq.cumsum(-1) == 1)
    return (win * first.to(win.dtype)).sum(-1)


# ------------------------------------------------------------------ attention
def attention(qkv, kv, x, gamma, dq, C):
    """y = gamma * softmax_j(q_i . k_j) v + x  (no scale; attn.hip): q = qkv[.., :dq] over the N tokens of a frame, k | v the
    columns [koff, koff + dq) | [voff, voff + C) of kv over its Nk tokens (kv is qkv for self attention).  qkv [F, .., ldq],
    kv [F, .., ldk], x [F, .., ldx] -> [F, N, C]."""
    koff = pad8(dq)
    voff = 2 * koff
    F_ = x.shape[0]
    q = qkv.reshape(F_, -1, qkv.shape[-1])[..., :dq]
    k = kv.reshape(F_, -1, kv.shape[-1])[..., koff:koff + dq]
    v = kv.reshape(F_, -1, kv.shape[-1])[..., voff:voff + C]
    A = torch.softmax(q @ k.transpose(1, 2), -1)
    return gamma * (A @ v) + x.reshape(F_, -1, x.shape[-1])[..., :C]


def sep_cell(qkv, x, gamma, dq, C, axis):
    """SeparableAttnCell (Attention.py:61-111) on channels-last qkv [B, T, W, H, ld], x [B, T, W, H, ldx], raw reshapes included;
    the pair max-pool along the attended axis takes the FIRST maximum of a tie.  -> [B, T, W, H, C]."""
    koff = pad8(dq)
    voff = 2 * koff
    B, T, W, H, _ = qkv.shape
    A = (T, W, H)[axis]
    swap = (lambda t: t) if axis == 0 else (lambda t: t.transpose(2, 3)) if axis == 1 else (lambda t: t.transpose(2, 4))
    ncdhw = lambda a, n: qkv[..., a:a + n].permute(0, 4, 1, 2, 3)

    def pairmax(t):
        t = swap(t).contiguous()
        a0, a1 = t[:, :, 0::2], t[:, :, 1::2]
        return torch.where(a1 > a0, a1, a0)

    Qf = swap(ncdhw(0, dq)).contiguous().view(B, A, -1)
    Kp = pairmax(ncdhw(koff, dq)).contiguous().view(B, -1, A // 2)
    Vp = pairmax(ncdhw(voff, C)).contiguous().view(B, -1, A // 2)
    att = torch.softmax(Qf @ Kp, -1)
    out = Vp @ att.transpose(2, 1)
    if axis == 0:
        o5 = out.view(B, C, W, H, T).permute(0, 1, 4, 2, 3)
    elif axis == 1:
        o5 = out.view(B, C, T, H, W).permute(0, 1, 2, 4, 3)
    else:
        o5 = out.view(B, C, T, W, H)
    return gamma * o5.permute(0, 2, 3, 4, 1) + x[..., :C]


# ------------------------------------------------------------------ projection head
def power_iter(W, u):
    """One power-iteration step of a spectral-norm wrapper (Normalization.py:19-31) from the stored u -> (sigma, u', v')."""
    W = W.double().reshape(W.shape[0], -1)
    vr = W.t() @ u.double()
    v = vr / (vr.norm() + 1e-12)
    wv = W @ v
    n = wv.norm()
    return n * n / (n + 1e-12), wv / (n + 1e-12), v


def proj_head(feat, wl_eff, b_lin, we_eff, cls, C):
    """out[f] = b + sum_c h[f][c] (wl_eff[c] + we_eff[cls[f]][c]), h = sum_p relu(feat)[.., :C]; wl_eff = w_lin / sigma_l [1, C] and
    we_eff = w_emb / sigma_e [classes, C] are the EFFECTIVE weights: their autograd gradients are the G that sn_backward_ref turns
    into the gradients of w_lin / w_emb with the latest u, v (`proj_head_grads`)."""
    F_ = feat.shape[0]
    h = feat[..., :C].clamp_min(0).reshape(F_, -1, C).sum(1)
    return b_lin.reshape(()) + (h * (wl_eff.reshape(1, C) + we_eff[cls.long()])).sum(1)


def proj_head_grads(feat, w_lin, b_lin, w_emb, cls, sn_lin, sn_emb, dout, C, eG=None):
    """sn_lin / sn_emb = (u, v, sigma) as the wrappers hold them when backward runs (after the forward's power iteration).
    eG: None or (bound of G_lin, bound of G_emb), carried through sn_backward_ref.  -> dict of
    out, dfeat [like feat, pad 0], G_lin, G_emb, db, dw_lin = (ref, bound), dw_emb = (ref, bound)."""
    f, b = leaf(feat), leaf(b_lin)
    wl = leaf(w_lin.double() / sn_lin[2].double())
    we = leaf(w_emb.double() / sn_emb[2].double())
    out = proj_head(f, wl, b, we, cls, C)
    df, Gl, db, Ge = grads(out, (f, wl, b, we), dout)
    zero = lambda G: torch.zeros_like(G)
    eGl, eGe = eG if eG is not None else (zero(Gl), zero(Ge))
    return dict(out=out.detach(), dfeat=df, G_lin=Gl, G_emb=Ge, db=db.reshape(-1),
                dw_lin=AR.sn_backward_ref(Gl.reshape(w_lin.shape), eGl.reshape(w_lin.shape), w_lin, *sn_lin),
                dw_emb=AR.sn_backward_ref(Ge, eGe, w_emb, *sn_emb))


# ------------------------------------------------------------------ fused q | k | v projection
def qkv_weight(wq, wk, wv, dq, dqp):
    """the fused [2 dqp + C, C, 1, 1] weight: rows of the gaps [dq, dqp) and [dqp + dq, 2 dqp) are zero"""
    C = wv.shape[0]
    w = torch.zeros(2 * dqp + C, wq.shape[1], 1, 1, dtype=torch.float64, device=wq.device)
    w = torch.cat([wq.double().reshape(dq, -1), w[dq:dqp, :, 0, 0], wk.double().reshape(dq, -1), w[dqp + dq:2 * dqp, :, 0, 0],
                   wv.double().reshape(C, -1)])
    return w.reshape(2 * dqp + C, -1, 1, 1)


def qkv_bias(bq, bk, bv, dq, dqp):
    """the fused bias, assembled from three parts with zero gaps"""
    z = torch.zeros(dqp - dq, dtype=torch.float64, device=bq.device)
    return torch.cat([bq.double(), z, bk.double(), z, bv.double()])


def qkv_conv(x, wq, bq, wk, bk, wv, bv, dq, dqp):
    """qkv[.., :] = x[.., :C] W^T + bias with the fused weight and bias above -> [.., 2 dqp + C] (a multiple of 8 when C is)"""
    w = qkv_weight(wq, wk, wv, dq, dqp)[:, :, 0, 0]
    return x[..., :w.shape[1]] @ w.t() + qkv_bias(bq, bk, bv, dq, dqp)


# ------------------------------------------------------------------ row permutations, as index arithmetic
def swap_index(A, B, device=None):
    """SwapFrameOrder(A, B): out[b * A + a] = x[a * B + b] -> the source row of every output row, [A * B] int64"""
    r = torch.arange(A * B, device=device)
    b, a = r // A, r % A
    return a * B + b


def swap_frames(x, A, B):
    return x[swap_index(A, B, x.device)]


def to_cl(x, dtype, swap=None):
    """fp32 [F, C, *spatial] -> [F, *spatial, pad8(C)] in `dtype` (torch's RNE), pad channels 0; swap = (A, B): source frame
    a * B + b is written at b * A + a."""
    F_, C = x.shape[:2]
    t = x.permute(0, *range(2, x.dim()), 1)
    if swap:
        t = swap_frames(t, *swap)
    return _pad_cols(t, pad8(C)).to(dtype).contiguous()


def from_cl(t, channels, swap=None):
    """the inverse of to_cl with the same swap: [F, *spatial, Cp] -> fp32 [F, channels, *spatial]"""
    if swap:
        t = swap_frames(t, swap[1], swap[0])
    return t[..., :channels].permute(0, t.dim() - 1, *range(1, t.dim() - 1)).float().contiguous()

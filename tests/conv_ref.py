"""Float64 reference of the weight / bias gradient of the library's convolutions (include/dvdgan_hip.h, dvd_wgrad_desc):

    dw[co][ci][tap] = sum over rows m of dy[m][co] * x[pos(m) + tap][ci]          db[co] = sum over rows m of dy[m][co]

A plain module (no conftest, no fixtures), torch only, CPU or GPU tensors alike; no project kernel and no oracle code takes part.
It works on CHANNELS-LAST operands, x [F, (T,) H, W, Cin] and dy [F, (T,) Ho, Wo, Cout], so it can be fed the values a kernel
read from memory (bf16-rounded in bf16 mode): only the fp32 summation order of the kernel under test is then left as a difference.
Stride 1, "same" zero padding, odd taps in two or three dimensions; `relu_in` clamps x at zero first, `up2` then repeats every
pixel of x twice along H and W (nearest x2 upsample; dy lives on the 2H x 2W grid).  The sums are formed tap by tap as one
float64 matrix product each.

gru_gate_wgrad_ref composes the three gate gradients of one ConvGRU layer the way functional._gru_gate_wgrads issues them: per gate
an x-part over every frame, an h0-part on step 0 (when an initial state was supplied) and an h-part on steps 1..T-1, placed in the
[hid][cin + hid][k][k] master of the gate.
"""
import torch


def _ksize3(k):
    k = tuple(k)
    return (1,) * (3 - len(k)) + k


def wgrad_ref(x, dy, ksize, *, up2=False, relu_in=False, chunk=64):
    """x [F, (T,) H, W, Cin], dy [F, (T,) Ho, Wo, Cout] (any float dtype, any device) -> (dw [Cout, Cin, *ksize], db [Cout]),
    float64 on the operands' device.  `chunk`: frames per matrix product (memory only; float64 sums do not notice at 1e-12)."""
    assert x.dim() == dy.dim() and x.dim() in (4, 5) and x.shape[0] == dy.shape[0]
    ksize = tuple(ksize)
    kt, kh, kw = _ksize3(ksize)
    assert kt & kh & kw & 1, "odd taps"
    if x.dim() == 4:
        assert kt == 1
        x, dy = x.unsqueeze(1), dy.unsqueeze(1)
    F_, T, H, W, cin = x.shape
    Ho, Wo, cout = dy.shape[2], dy.shape[3], dy.shape[4]
    assert (Ho, Wo) == ((2 * H, 2 * W) if up2 else (H, W)) and dy.shape[1] == T
    dw = torch.zeros(cout, cin, kt * kh * kw, dtype=torch.float64, device=x.device)
    db = torch.zeros(cout, dtype=torch.float64, device=x.device)
    for f0 in range(0, F_, chunk):
        xc, dc = x[f0:f0 + chunk].double(), dy[f0:f0 + chunk].double()
        if relu_in:
            xc = xc.clamp_min(0.0)
        if up2:
            xc = xc.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        xp = torch.nn.functional.pad(xc, (0, 0, kw // 2, kw // 2, kh // 2, kh // 2, kt // 2, kt // 2))
        dm = dc.reshape(-1, cout)
        db += dm.sum(0)
        for it in range(kt):
            for iy in range(kh):
                for ix in range(kw):
                    win = xp[:, it:it + T, iy:iy + Ho, ix:ix + Wo, :].reshape(-1, cin)
                    dw[:, :, (it * kh + iy) * kw + ix] += dm.t() @ win
    return dw.view(cout, cin, *ksize), db


def gru_gate_wgrad_ref(x, dgx, dg, h_all, hr_all, h0, T, B, hid, k):
    """The three gates (update, reset, out) of one ConvGRU layer -> [(dw [hid][cin + hid][k][k], db [hid])] * 3, float64.
    x [T*B or B, S, S, cin] (B frames: an input shared by every step), dgx [same frames as x, S, S, 3 hid] (the gradient the x-part
    sees: dg, or its sum over T for a shared input), dg [T*B, S, S, 3 hid], h_all / hr_all [T*B, S, S, hid] (h_t and h_{t-1} * r_t),
    h0 [B, S, S, hid] or None.  Update / reset read h_{t-1}: h0 on step 0, h_all[t - 1] after; the out gate reads hr_all[t]."""
    cin = x.shape[-1]
    out = []
    for g in range(3):
        col = slice(g * hid, (g + 1) * hid)
        dw = torch.zeros(hid, cin + hid, k, k, dtype=torch.float64, device=x.device)
        dwx, db = wgrad_ref(x, dgx[..., col], (k, k))
        dw[:, :cin] += dwx
        if h0 is not None:
            dw[:, cin:] += wgrad_ref(h0 if g < 2 else hr_all[:B], dg[:B, ..., col], (k, k))[0]
        if T > 1:
            hin = h_all[:(T - 1) * B] if g < 2 else hr_all[B:]
            dw[:, cin:] += wgrad_ref(hin, dg[B:, ..., col], (k, k))[0]
        out.append((dw, db))
    return out

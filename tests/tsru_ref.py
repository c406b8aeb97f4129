"""Float64 reference and error bounds for the TSRU kernels (dvd_gan_amd/xsrc/tsru/tsru.hip, include/dvdx_tsru.h) and an
end-to-end float64 restatement of one TSRU layer (functional.ConvTSRULayer).

A plain module (no conftest, no fixtures), torch only, CPU or GPU tensors alike; no project kernel and no oracle code takes part.
It is fed the tensors a pass STORED and restarts every step from them, so storage rounding never compounds.  A check reports

    |out - ref| / (bound + half an ulp of the output's type at |ref| + bound)

(`ratio`, as tests/gru_ref.py; a non-finite output counts as infinite error).  Layout: channels-last, h [B][H][W][C], the raw
flow [B][H][W][>= 2] (x, y), everything float64 inside.

The unit (d = flow range, s = sigmoid):
  theta = d tanh(theta_raw);  warped(p) = bilinear sample of h_prev at p + theta(p), zero outside the frame (equal to
  F.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True) on pixel coordinates);  u = s(a_u), c = relu(a_c);
  h = u warped + (1 - u) c.
  da_u = dh (warped - c) u (1 - u);  da_c = dh (1 - u) [a_c > 0];  g = dh u;
  dtheta_x = sum_k g ((1 - fy)(v01 - v00) + fy (v11 - v10)), dtheta_y likewise;  dtheta_raw = dtheta d (1 - tanh^2 theta_raw);
  dh_prev(q) = sum over |p - q|_inf <= R = ceil(d) of w_q(p + theta(p)) g(p)  [+ addend]      (`warpT64`, a gather).

Bounds.  E = 2^-24, TINY = 2^-126.  Every constant counts roundings of the expressions as include/dvdx_tsru.h states them; none is
fitted to what the kernel produces.
  Function terms (tests/gru_ref.py derives them from common.h's gate_sigmoid / gate_tanh and the documented 1-ulp V_EXP_F32 /
  V_RCP_F32, 1-ulp expf, 2-ulp tanhf):  bf16 mode Fs = (2|a| + 5) E s(a), Ft = (4 + (5 + 2|a|) |tanh a|) E;  exact mode
  Fs = 4E s(a), Ft = 4E |tanh a|;  + TINY each.
  Coordinate.  t = tanh(raw) carries Ft; theta = fl(d t) adds E |theta|; sx = fl(x + theta) adds E |sx|:
      delta = d Ft + E (|theta| + |sx|)                                                        per axis.
  sx - floor(sx) is exact (the operands are within a factor 2 of each other or the result is sx itself).  The inputs keep every
  coordinate at least 0.1 away from an integer, and `coordinates` asserts a margin of 1000 delta, so the kernel's cell is the
  reference's.  Inside a cell the bilinear value is linear in each coordinate with slope at most the largest neighbour
  difference of the four taps along that axis (Dx = max(|v01 - v00|, |v11 - v10|), Dy likewise); the sample is continuous
  across cells and towards the zero border, so a coordinate error never costs more than delta times such a slope.
  Warp.  wx0 = fl(1 - wx1) has relative error E, a weight fl(wy . wx) therefore 3E; the chain w00 v00 -> fmaf -> fmaf -> fmaf
  rounds four times, each partial sum bounded by A = sum |w| |v|:
      Dw = deltax Dx + deltay Dy + 7E A                                                       (0 for a pixel that samples nothing).
  Blend.  h = fmaf(u, fl(warped - c), c):  u carries Fs, the difference E |warped - c|, the fmaf E |h|:
      bound(h) = u Dw + (Fs + E u) |warped - c| + E |h|.
  g = fl(dh u):  Dg = |dh| Fs + E |g|   (+ Ddh u, Ddh = E |dh| when dh is the rounded sum dh + dh2).
  da_c = fl(dh fl(1 - u)) where a_c > 0 (the sign of the STORED a_c: no kink):  |dh| Fs + 2E |ref| (+ Ddh (1 - u)).
  da_u = fl(fl(fl(dh fl(warped - c)) u) fl(1 - u)):  five roundings, Dw through the difference, Fs through u (1 - u) whose
      derivative 1 - 2u is at most 1 in magnitude:  |dh| u (1 - u) Dw + |dh (warped - c)| (Fs + Fs^2) + 5E |ref| (+ Ddh ...).
  ex = fmaf(wy1, fl(v11 - v10), fl(wy0 fl(v01 - v00))):  linear in sy with slope Dxy = |v11 - v10 - v01 + v00|, constant in sx
      inside the cell;  three roundings per term (difference, weight, product / fmaf):  Dex = deltay Dxy + 3E Aex,
      Aex = |wy1| |v11 - v10| + |wy0| |v01 - v00|.
  sum_x = sum over C channels of fmaf(g, ex, .) and a butterfly of adds, C addends in all, any order:
      Dsum = sum (Dg |ex| + |g| Dex) + C E sum |g ex|.
  dtheta_raw = fl(fl(sum d) fl(1 - fl(t^2))):  q = 1 - t^2 carries Dq = 2 |t| Ft + Ft^2 + E t^2 + E |q| (fl(t^2) is rounded BEFORE
      the subtraction: absolute):  Dsum d |q| + |sum d| Dq + 2E |ref|;  the output is stored in the compute type (half an ulp).
  dh_prev(q) = fmaf chain over the n(q) pixels p whose cell holds q, + addend:  a weight is a product of two hat functions of the
      coordinates, slope at most 1 per axis, and carries 3E relative:  Dwq = deltax + deltay + 3E w;
      bound = sum_p (Dwq |g| + w Dg) + (n(q) + 1) E (sum_p w |g| + |addend|).
"""
import math

import torch
import torch.nn.functional as F

E = 2.0 ** -24
TINY = 2.0 ** -126

# (B, H, W, C, d) of the kernel tests, CPU and GPU alike
CASES = [(2, 4, 4, 8, 2.0), (3, 6, 6, 24, 1.5), (2, 5, 7, 8, 8.0), (2, 32, 32, 32, 2.0)]


def half_ulp(ref, dtype):
    """Half an ulp of `dtype` at |ref| (0 for fp32: its rounding is inside the fp32 bound)."""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref.abs().float())
    h = torch.ldexp(torch.ones_like(ref), (e - 9).to(ref.dtype))
    return torch.where(ref == 0, torch.zeros_like(h), h)


def ratios(out, ref, bound, dtype):
    """|out - ref| / (bound + half an ulp of `dtype` at |ref| + bound), elementwise; inf where `out` is not finite."""
    err = (out.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    allowed = bound + half_ulp(ref.abs() + bound, dtype)
    return torch.where(err == 0, torch.zeros_like(err), err / allowed.clamp_min(1e-300))


def ratio(out, ref, bound, dtype):
    r = ratios(out, ref, bound, dtype)
    return float(r.max()) if r.numel() else 0.0


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def fn_term(a, kind, dtype):
    """Absolute error of the kernel's sigmoid / tanh at argument a (module docstring)."""
    a = a.double()
    if kind == "sigmoid":
        s = torch.sigmoid(a)
        return ((2 * a.abs() + 5) * E * s if dtype == torch.bfloat16 else 4 * E * s) + TINY
    t = torch.tanh(a).abs()
    return ((4 + (5 + 2 * a.abs()) * t) * E if dtype == torch.bfloat16 else 4 * E * t) + TINY


# ------------------------------------------------------------------ the warp and its transpose
def cells(theta, H, W):
    """theta [B][H][W][2] (x, y) in pixels -> valid [B][H][W] bool, x0, y0 (long), wx1, wy1 of every pixel's bilinear cell."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=theta.device),
                            torch.arange(W, dtype=torch.float64, device=theta.device), indexing="ij")
    sx, sy = xs + theta[..., 0], ys + theta[..., 1]
    valid = (sx > -1) & (sx < W) & (sy > -1) & (sy < H)
    fx, fy = torch.floor(sx), torch.floor(sy)
    return valid, fx.long(), fy.long(), sx - fx, sy - fy, sx, sy


def taps(h, valid, x0, y0):
    """v00, v01, v10, v11 [B][H][W][C]: the four neighbours of every pixel's cell, zero outside the frame (and where not valid)."""
    B, H, W, _ = h.shape
    hp = F.pad(h, (0, 0, 1, 1, 1, 1))
    b = torch.arange(B, device=h.device).view(B, 1, 1)
    xi, yi = (x0 + 1).clamp(0, W), (y0 + 1).clamp(0, H)
    m = valid.unsqueeze(-1).to(h.dtype)
    return tuple(hp[b, yi + j, xi + i] * m for j in (0, 1) for i in (0, 1))


def warp64(h, theta, mode="bilinear"):
    """The warped state [B][H][W][C] in float64.  mode="nearest" is a PLANTED ERROR for tests of the bounds."""
    h, theta = h.double(), theta.double()
    valid, x0, y0, wx1, wy1, _, _ = cells(theta, h.shape[1], h.shape[2])
    if mode == "nearest":
        wx1, wy1 = torch.round(wx1), torch.round(wy1)
    v00, v01, v10, v11 = taps(h, valid, x0, y0)
    wx1, wy1 = wx1.unsqueeze(-1), wy1.unsqueeze(-1)
    return (1 - wy1) * ((1 - wx1) * v00 + wx1 * v01) + wy1 * ((1 - wx1) * v10 + wx1 * v11)


def _transpose(theta, R, fields):
    """The gather over the window |p - q|_inf <= R: for every field (tensor [B][H][W][C'], weighted: bool) the sum over p of
    (w_q(p) if weighted else [q in p's cell]) * field(p), and the number of such p, [B][H][W]."""
    B, H, W, _ = theta.shape
    valid, x0, y0, wx1, wy1, _, _ = cells(theta, H, W)
    ys, xs = torch.meshgrid(torch.arange(H, device=theta.device), torch.arange(W, device=theta.device), indexing="ij")
    outs = [torch.zeros_like(f) for f, _ in fields]
    count = torch.zeros(B, H, W, dtype=torch.float64, device=theta.device)
    for oy in range(-R, R + 1):             # q = p - (oy, ox); lines ascending, within a line left to right, as the kernel
        for ox in range(-R, R + 1):
            jx, jy = (xs - ox) - x0, (ys - oy) - y0
            inq = ((xs - ox) >= 0) & ((xs - ox) < W) & ((ys - oy) >= 0) & ((ys - oy) < H)
            touch = valid & inq & (jx >= 0) & (jx <= 1) & (jy >= 0) & (jy <= 1)
            if not bool(touch.any()):
                continue
            w = torch.where(jy == 1, wy1, 1 - wy1) * torch.where(jx == 1, wx1, 1 - wx1) * touch
            # rows / columns of p that map into the frame
            py0, py1, px0, px1 = max(0, oy), min(H, H + oy), max(0, ox), min(W, W + ox)
            sp = (slice(None), slice(py0, py1), slice(px0, px1))
            sq = (slice(None), slice(py0 - oy, py1 - oy), slice(px0 - ox, px1 - ox))
            for o, (f, weighted) in zip(outs, fields):
                o[sq] += ((w if weighted else touch.double())[sp]).unsqueeze(-1) * f[sp]
            count[sq] += touch.double()[sp]
    return outs, count


def warpT64(g, theta, R):
    """The transpose of the warp as a gather with window radius R (R < ceil(max |theta|) is a PLANTED ERROR)."""
    return _transpose(theta.double(), R, [(g.double(), True)])[0][0]


# ------------------------------------------------------------------ inputs of the kernel tests
def make_case(B, H, W, C, d, dtype, seed=0, pad=8):
    """h_prev, dh, addend fp32 [B,H,W,C]; a `dtype` [B,H,W,pad + 2C] (a_c at column pad, a_u at pad + C: the row stride and the
    offsets are exercised); theta_raw fp32 [B,H,W,2].  No element sits on a kink: the displacements are drawn first, fractional
    parts in [0.1, 0.9] on both axes, |theta| <= 0.9 d + 0.1, theta_raw = atanh(theta / d); a_c = sign(r)(|r| + 0.05)."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * H + W + C)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    theta = (torch.rand(B, H, W, 2, generator=gen, dtype=torch.float64) * 2 - 1) * 0.9 * d
    fl = torch.floor(theta)
    theta = fl + (theta - fl).clamp(0.1, 0.9)
    raw = torch.atanh(theta / d).float()
    r = rn(B, H, W, C)
    a = torch.zeros(B, H, W, pad + 2 * C, dtype=torch.float64)
    a[..., pad:pad + C] = torch.sign(r) * (r.abs() + 0.05)
    a[..., pad + C:] = rn(B, H, W, C)
    return {"h_prev": rn(B, H, W, C).float(), "dh": rn(B, H, W, C).float(), "addend": rn(B, H, W, C).float(), "a": a.to(dtype),
            "theta_raw": raw, "off_c": pad, "off_u": pad + C, "d": d, "dtype": dtype}


# ------------------------------------------------------------------ one step in float64 with its bounds
def coordinates(theta_raw, d, dtype, H, W):
    """theta [B,H,W,2] float64 from the stored raw flow, its coordinate error delta [B,H,W,2], tanh and Ft; asserts the margin."""
    raw = theta_raw[..., :2].double()
    t = torch.tanh(raw)
    Ft = fn_term(raw, "tanh", dtype)
    theta = d * t
    _, _, _, wx1, wy1, sx, sy = cells(theta, H, W)
    delta = d * Ft + E * (theta.abs() + torch.stack([sx, sy], -1).abs())
    frac = torch.stack([wx1, wy1], -1)
    margin = torch.minimum(frac, 1 - frac)
    assert bool((margin > 1000 * delta).all()), "an input coordinate sits on a kink"
    return theta, delta, t, Ft


def step64(h_prev, a, off_c, off_u, theta_raw, d, dtype, dh=None, dh2=None, addend=None, R=None, warp_mode="bilinear",
           drop_one_minus_u=False):
    """Reference values and bounds of one forward (and, with dh, backward) step on the stored operands -> dict name -> (ref, bound).
    warp_mode="nearest", drop_one_minus_u and R < ceil(d) are PLANTED ERRORS (tests of the bounds only)."""
    B, H, W, C = h_prev.shape
    hp = h_prev.double()
    ac, au = a[..., off_c:off_c + C].double(), a[..., off_u:off_u + C].double()
    theta, delta, t, Ft = coordinates(theta_raw, d, dtype, H, W)
    valid, x0, y0, wx1, wy1, _, _ = cells(theta, H, W)
    v00, v01, v10, v11 = taps(hp, valid, x0, y0)
    wx1, wy1 = wx1.unsqueeze(-1), wy1.unsqueeze(-1)
    wx0, wy0 = 1 - wx1, 1 - wy1
    dxe, dye = delta[..., 0:1], delta[..., 1:2]
    hw = warp64(hp, theta, warp_mode)
    A = wy0 * (wx0 * v00.abs() + wx1 * v01.abs()) + wy1 * (wx0 * v10.abs() + wx1 * v11.abs())
    Dx = torch.maximum((v01 - v00).abs(), (v11 - v10).abs())
    Dy = torch.maximum((v10 - v00).abs(), (v11 - v01).abs())
    Dw = (dxe * Dx + dye * Dy + 7 * E * A) * valid.unsqueeze(-1)
    u, Fs = torch.sigmoid(au), fn_term(au, "sigmoid", dtype)
    c = ac.clamp_min(0)
    h = u * hw + (c if drop_one_minus_u else (1 - u) * c)
    out = {"h": (h, u * Dw + (Fs + E * u) * (hw - c).abs() + E * h.abs())}
    if dh is None:
        return out
    dh64 = dh.double() + (dh2.double() if dh2 is not None else 0)
    Ddh = E * dh64.abs() if dh2 is not None else torch.zeros_like(dh64)
    g = dh64 * u
    Dg = dh64.abs() * Fs + Ddh * u + E * g.abs()
    dac = torch.where(ac > 0, dh64 * (1 - u), torch.zeros_like(g))
    out["da_c"] = (dac, torch.where(ac > 0, dh64.abs() * Fs + Ddh * (1 - u) + 2 * E * dac.abs(), torch.zeros_like(g)))
    dau = dh64 * (hw - c) * u * (1 - u)
    out["da_u"] = (dau, dh64.abs() * u * (1 - u) * Dw + (dh64 * (hw - c)).abs() * (Fs + Fs * Fs)
                   + Ddh * ((hw - c) * u * (1 - u)).abs() + 5 * E * dau.abs())
    m = valid.unsqueeze(-1)
    ex = (wy1 * (v11 - v10) + wy0 * (v01 - v00)) * m
    ey = (wx1 * (v11 - v01) + wx0 * (v10 - v00)) * m
    Dxy = (v11 - v10 - v01 + v00).abs()
    Dex = (dye * Dxy + 3 * E * (wy1 * (v11 - v10).abs() + wy0 * (v01 - v00).abs())) * m
    Dey = (dxe * Dxy + 3 * E * (wx1 * (v11 - v01).abs() + wx0 * (v10 - v00).abs())) * m
    q = 1 - t * t
    Dq = 2 * t.abs() * Ft + Ft * Ft + E * t * t + E * q.abs()
    refs, bounds = [], []
    for i, (e_, De) in enumerate(((ex, Dex), (ey, Dey))):
        s = (g * e_).sum(-1)
        Ds = (Dg * e_.abs() + g.abs() * De).sum(-1) + C * E * (g * e_).abs().sum(-1)
        ref = s * d * q[..., i]
        refs.append(ref)
        bounds.append(Ds * d * q[..., i].abs() + (s * d).abs() * Dq[..., i] + 2 * E * ref.abs())
    out["dtheta_raw"] = (torch.stack(refs, -1), torch.stack(bounds, -1))
    R = math.ceil(d) if R is None else R
    ones = torch.ones_like(g)
    (wg, wag, wDg, dg_), n = _transpose(theta, R, [(g, True), (g.abs(), True), (Dg, True), ((dxe + dye) * g.abs() * ones, False)])
    ad = addend.double() if addend is not None else torch.zeros_like(g)
    out["dh_prev"] = (wg + ad, dg_ + 3 * E * wag + wDg + (n.unsqueeze(-1) + 1) * E * (wag + ad.abs()))
    return out


# ------------------------------------------------------------------ one layer, end to end, float64 with autograd
def _warp_autograd(h, theta):
    """The warp with torch operations autograd differentiates (the cell indices are constants, the weights carry the gradient)."""
    valid, x0, y0, wx1, wy1, _, _ = cells(theta, h.shape[1], h.shape[2])
    v00, v01, v10, v11 = taps(h, valid, x0, y0)
    wx1, wy1 = wx1.unsqueeze(-1), wy1.unsqueeze(-1)
    return (1 - wy1) * ((1 - wx1) * v00 + wx1 * v01) + wy1 * ((1 - wx1) * v10 + wx1 * v11)


def _conv(x, w, b=None):
    """'same' cross-correlation of a channels-last tensor with a [Cout][Cin][k][k] weight."""
    return F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=w.shape[-1] // 2).permute(0, 2, 3, 1)


def layer64(x, p, T, shared_x, h0, d):
    """All T steps of one TSRU layer in float64.  x [T*B,S,S,Cin] t-major (or [B,S,S,Cin] when shared), p: the cell's parameters
    by name ({update,out,flow}_gate.{weight,bias}, flow_out.{weight,bias}), h0 [B,S,S,C] or None -> [T*B,S,S,C]."""
    C = p["update_gate.weight"].shape[0]
    B = x.shape[0] if shared_x else x.shape[0] // T
    h = h0 if h0 is not None else torch.zeros(B, x.shape[1], x.shape[2], C, dtype=torch.float64, device=x.device)
    outs = []
    for t in range(T):
        z = torch.cat([x if shared_x else x[t * B:(t + 1) * B], h], -1)
        a_c = _conv(z, p["out_gate.weight"], p["out_gate.bias"])
        a_u = _conv(z, p["update_gate.weight"], p["update_gate.bias"])
        a_f = _conv(z, p["flow_gate.weight"], p["flow_gate.bias"])
        theta = d * torch.tanh(_conv(torch.relu(a_f), p["flow_out.weight"], p["flow_out.bias"]))
        u = torch.sigmoid(a_u)
        h = u * _warp_autograd(h, theta) + (1 - u) * torch.relu(a_c)
        outs.append(h)
    return torch.cat(outs, 0)

"""Step-by-step float64 reference and error bounds for one ConvGRU layer (gru.hip, the gate epilogues of conv_common.h).

A plain module (no conftest, no fixtures), torch only, CPU or GPU tensors alike; no project kernel and no oracle code takes part.
It is fed the tensors a forward / backward pass STORED, recomputes every step in float64 from the stored tensors of that step
and of the step before, and returns per check the worst

    |out - ref| / (bound + half an ulp of the storage type at |ref| + bound)

(`ratio`; a non-finite output counts as infinite error).  Because every step restarts from stored values, storage rounding
never compounds: the bounds stay at half an ulp plus fp32 terms for any T.

Layout: channels-last.  gx [T or 1][B][H][W][3h] (u | r | o), every per-step tensor [T][B][H][W][h], h0 [B][H][W][h] or None,
dg [T][B][H][W][3h], carry / dh0 / h32 slots fp32 with M * h elements.  Weights: the master tensors [Cout][Cin][k][k] ALREADY
ROUNDED to the storage type (w_ur = cat(update, reset) h-part, w_o = out gate h-part), so the reference and the packs hold the
same values; the backward pass uses the adjoint of the same tensors (`convT64`).

Definitions.  E = 2^-24 (unit roundoff of fp32).  For a convolution with n = products per output + extra addends (gx, slabs,
carry) and A = the same convolution of the magnitudes (+ |addends|), e = 2 n E A is the worst-case fp32 accumulation term, any
summation order (profiles/attention_parity_numbers.md makes the same assumption).

Forward step t (h_prev = stored h0 or h_all[t-1]):
  a_ur = conv64(h_prev, W_ur) + gx[t][u|r];   u[t], r[t] against sigmoid(a), bound max(s(a+e) - s(a), s(a) - s(a-e)) + F
  hr[t] BIT-EQUAL to storage(h_prev * r[t])   (the kernel multiplies by the stored r; bf16 x bf16 is exact in fp32)
  a_o  = conv64(hr[t] stored, W_o) + gx[t][o]; o[t] against tanh(a) the same way
  h[t] against hp (1 - u[t]) + o[t] u[t] on the stored u, o.  hp = the reference's own float64 carry when an fp32 carry (h32)
       was given and t > 0 (step 0 reads the stored h0: gru.hip hands no h32p to it), else the stored h_prev.  The carry's bound
       is propagated elementwise, d_t = d_{t-1} (1 - u) + C_H E (|hp| + |o|); the two final h32 slots are held to d alone.
       C_H = 3 is derived, not fitted: fl(1 - u), fl(hp * .), fl(o * u) and the final add are four roundings, each relative E:
       |hp (1 - u)| 2E + |o u| E + |h| E <= 3E |hp| + 2E |o| for u in [0, 1] (an FMA contraction only removes a rounding).

Function term F (absolute; below 2^-20 (1 + |a|) of the gates' unit range, so it masks nothing at bf16 precision).
  bf16 mode (common.h: gate_sigmoid<bf16_t> = rcp(1 + __expf(-x)), gate_tanh<bf16_t> = (1 - t) rcp(1 + t), t = __expf(-2|x|),
  and tanh x = x below |x| = 2e-3).  __expf(y) is the hardware 2^(y log2 e): the product with the fp32 constant log2(e) carries two
  roundings, i.e. an argument error of 2E |y log2 e|, a relative error 2E |y| of the power; the CDNA ISA guide documents V_EXP_F32
  and V_RCP_F32 at 1 ulp = 2E relative each.  Sigmoid: t = exp(-a) has relative error (2|a| + 2) E; 1 + t adds E and t / (1 + t)
  <= 1; the reciprocal 2E  ->  F = (2|a| + 5) E sigmoid(a).  Tanh: t has relative error (4|a| + 2) E; fl(1 - t) has ABSOLUTE error
  (4|a| + 2) E t + E (this is the cancellation: it is not small relative to 1 - t ~ 2|a| near the switch, hence an absolute
  term); with |a| t = |a| exp(-2|a|) <= 1 / (2 e) that is below 4E after the division by 1 + t; the denominator, the reciprocal
  and the last product add (2|a| + 5) E relative  ->  F = (4 + (5 + 2|a|) |tanh a|) E.  Below the switch |x - tanh x| <= |x|^3 / 3
  <= 2.7e-9 < 4E.  Results below 2^-126 may be flushed: + 2^-126.
  exact mode (libm expf / tanhf, IEEE divide; the HIP math documentation gives expf 1 ulp and tanhf 2 ulp): sigmoid: exp 2E,
  1 + t E, divide E -> F = 4E sigmoid(a);  tanh: F = 4E |tanh a|;  + 2^-126.

Backward step t, walking down from T - 1 (carry64 = 0 at the start, bound Dc = 0):
  dh = dh_out[t] + carry64;                            Ddh = Dc + 2E (|dh_out| + |carry64|)
  dg[t][o] against dh u (1 - o^2);                     Ddh |u (1 - o^2)| + |dh u| E (o^2 + |1 - o^2|) + 3E |ref|
                                                       (fl(o^2) is rounded BEFORE the subtraction: absolute, not relative)
  dg[t][u] against dh (o - h_prev) u (1 - u);          Ddh |(o - h_prev) u (1 - u)| + 6E |ref|
  carry' = dh (1 - u);                                 Dc' = Ddh (1 - u) + 2E |carry'|
  d(hr) = convT64(dg[t][o] AS STORED, W_o);            e_hr (n = k k h + 8 slabs)
  carry'' = carry' + d(hr) r;                          Dc'' = Dc' + e_hr r + 2E (|d(hr) r| + |carry''|)
  dg[t][r] against d(hr) h_prev r (1 - r);             e_hr |h_prev r (1 - r)| + 5E |ref|
  carry64 for t - 1 = carry'' + convT64(dg[t][u|r] AS STORED, W_ur);   Dc = Dc'' + e_ur (n = k k 2h + 8 slabs + carry + dh_out)
  without an h_prev (t = 0, no h0): dg[t][r] = 0 exactly and the carry receives no convolution term.
  dh0 and the final `carry` are held to the propagated bound alone (fp32, no ulp term).  Where the [u|r] backward-data
  convolution of step 0 leaves slabs to gru_dh0_kernel (tickets = NULL or more slices than combine_max), the carry BUFFER ends
  as carry'' and only dh0 holds the full sum: `carry_full` says which.
Every elementwise constant above counts roundings of the expression as gru.hip / conv_common.h write it; none is fitted.
"""
import math

import torch
import torch.nn.functional as F

E = 2.0 ** -24
TINY = 2.0 ** -126
C_H = 3.0
SLABS = 8                # dvd_conv_pick_nsplit never asks for more slices


def note(name, value):
    print(f"MEASURED {name}: {value:.3e}")


def half_ulp(ref, dtype):
    """Half an ulp of `dtype` at |ref| (0 for fp32: its rounding is inside the fp32 bound)."""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref.abs().float())
    h = torch.ldexp(torch.ones_like(ref), (e - 9).to(ref.dtype))
    return torch.where(ref == 0, torch.zeros_like(h), h)


def ratio(out, ref, bound, dtype):
    """worst |out - ref| / (bound + half an ulp of the storage type at |ref| + bound); inf where `out` is not finite."""
    err = (out.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    allowed = bound + half_ulp(ref.abs() + bound, dtype)
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def bit_ratio(out, want):
    """0 when bit-equal, else inf (a check that allows nothing)."""
    return 0.0 if torch.equal(bits(out), bits(want)) else math.inf


def conv64(x, w):
    """'same' zero-padded cross-correlation in float64, one matrix product per tap.  x [B][H][W][C], w [Cout][C][k][k]."""
    x, w = x.double(), w.double()
    B, H, W, C = x.shape
    k = w.shape[-1]
    c = k // 2
    xp = F.pad(x, (0, 0, c, c, c, c))
    out = torch.zeros(B, H, W, w.shape[0], dtype=torch.float64, device=x.device)
    for dy in range(k):
        for dx in range(k):
            out += xp[:, dy:dy + H, dx:dx + W, :] @ w[:, :, dy, dx].t()
    return out


def convT64(g, w):
    """The adjoint of conv64 in its input: g [B][H][W][Cout], w [Cout][C][k][k] -> [B][H][W][C]."""
    g, w = g.double(), w.double()
    B, H, W, Co = g.shape
    k = w.shape[-1]
    c = k // 2
    gp = F.pad(g, (0, 0, c, c, c, c))
    out = torch.zeros(B, H, W, w.shape[1], dtype=torch.float64, device=g.device)
    for dy in range(k):
        for dx in range(k):
            out += gp[:, 2 * c - dy:2 * c - dy + H, 2 * c - dx:2 * c - dx + W, :] @ w[:, :, dy, dx]
    return out


def conv_err(x, w, extra_mag, n_extra, transposed=False):
    """e = 2 n E A of a convolution of x with w plus n_extra addends of total magnitude extra_mag."""
    op = convT64 if transposed else conv64
    k = w.shape[-1]
    n = k * k * (w.shape[0] if transposed else w.shape[1]) + n_extra
    A = op(x.abs(), w.abs()) + extra_mag
    return 2.0 * n * E * A


def _fsig(a, exact):
    s = torch.sigmoid(a)
    return (4.0 * E * s if exact else (2.0 * a.abs() + 5.0) * E * s) + TINY


def _ftanh(a, exact):
    t = torch.tanh(a).abs()
    return (4.0 * E * t if exact else (4.0 + (5.0 + 2.0 * a.abs()) * t) * E) + TINY


def _mono_bound(f, a, e):
    """exact propagation of |da| <= e through a monotone f"""
    fa = f(a)
    return torch.maximum(f(a + e) - fa, fa - f(a - e))


def conv_ratio(out, x, w, dtype, bias=None, res=None, transposed=False):
    """A plain convolution (+ fp32 bias + stored residual, summed in fp32 and rounded ONCE at the store: the direct epilogue of
    conv_common.h) against float64: the x-part convolutions of a stack."""
    op = convT64 if transposed else conv64
    ref = op(x, w)
    mag = torch.zeros_like(ref)
    n_extra = SLABS
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
        n_extra += 1
    if res is not None:
        ref = ref + res.double()
        mag = mag + res.double().abs()
        n_extra += 1
    return ratio(out, ref, conv_err(x, w, mag, n_extra, transposed), dtype)


def forward_ratios(name, dtype, gx, h0, h_all, u_all, r_all, o_all, hr_all, h32, w_ur, w_o, stats=None):
    """-> {check: worst ratio} over all T steps; prints a MEASURED line per check.  `stats` (a dict) receives what the input
    regimes assert: the float64 pre-activations a_o of every step ("a_o") and the reference gates ("u", "r", "o")."""
    T = h_all.shape[0]
    h = h_all.shape[-1]
    exact = dtype == torch.float32
    worst = {k: 0.0 for k in ("u", "r", "hr", "o", "h")}
    up = lambda k, v: worst.__setitem__(k, max(worst[k], v))
    carry64 = dcar = None
    slots = {}
    keep = {"a_o": [], "u": [], "r": [], "o": []}
    for t in range(T):
        g = gx[t if gx.shape[0] > 1 else 0].double()
        hprev = h0 if t == 0 else h_all[t - 1]
        u, r, o = u_all[t], r_all[t], o_all[t]
        if hprev is not None:
            a = conv64(hprev, w_ur) + g[..., :2 * h]
            e = conv_err(hprev, w_ur, g[..., :2 * h].abs(), 1 + SLABS)
        else:
            a, e = g[..., :2 * h], torch.zeros_like(g[..., :2 * h])
        bnd = _mono_bound(torch.sigmoid, a, e) + _fsig(a, exact)
        s = torch.sigmoid(a)
        up("u", ratio(u, s[..., :h], bnd[..., :h], dtype))
        up("r", ratio(r, s[..., h:], bnd[..., h:], dtype))
        want_hr = (hprev.float() * r.float()).to(dtype) if hprev is not None else torch.zeros_like(r)
        up("hr", bit_ratio(hr_all[t], want_hr))
        if hprev is not None:
            ao = conv64(hr_all[t], w_o) + g[..., 2 * h:]
            eo = conv_err(hr_all[t], w_o, g[..., 2 * h:].abs(), 1 + SLABS)
        else:
            ao, eo = g[..., 2 * h:], torch.zeros_like(g[..., 2 * h:])
        up("o", ratio(o, torch.tanh(ao), _mono_bound(torch.tanh, ao, eo) + _ftanh(ao, exact), dtype))
        keep["a_o"].append(ao); keep["u"].append(s[..., :h]); keep["r"].append(s[..., h:]); keep["o"].append(torch.tanh(ao))
        ud, od = u.double(), o.double()
        if h32 is not None and t > 0:
            hp, dprev = carry64, dcar
        else:
            hp = hprev.double() if hprev is not None else torch.zeros_like(ud)
            dprev = torch.zeros_like(ud)
        href = hp * (1.0 - ud) + od * ud
        dcar = dprev * (1.0 - ud) + C_H * E * (hp.abs() + od.abs())
        carry64 = href
        up("h", ratio(h_all[t], href, dcar, dtype))
        slots[(t + 1) & 1] = (href, dcar)
    if h32 is not None:
        worst["h32"] = 0.0
        for s_, (ref, d) in slots.items():
            worst["h32"] = max(worst["h32"], ratio(h32[s_].reshape(ref.shape), ref, d, torch.float32))
    if stats is not None:
        stats.update({k: torch.stack(v) for k, v in keep.items()})
    for k, v in worst.items():
        note(f"{name} {k} err/bound", v)
    return worst


def backward_ratios(name, dtype, h0, h_all, u_all, r_all, o_all, dh_out, dg, carry, dh0, w_ur, w_o, carry_full=True):
    """-> {check: worst ratio} of one BPTT pass (dg_u, dg_r, dg_o per step, the final carry, dh0).  dh_out: the gradient wrt
    every h_t as the kernel READ it ([T][B][H][W][h], storage type) or None.  carry_full: the carry buffer ends as the whole
    gradient wrt h0 (False: the [u|r] term of step 0 was left in slabs, the buffer holds carry'')."""
    T = h_all.shape[0]
    h = h_all.shape[-1]
    worst = {k: 0.0 for k in ("dg_u", "dg_r", "dg_o")}
    up = lambda k, v: worst.__setitem__(k, max(worst[k], v))
    shp = h_all[0].shape
    c64 = torch.zeros(shp, dtype=torch.float64, device=h_all.device)
    dc = torch.zeros_like(c64)
    pre = (c64, dc)
    for t in range(T - 1, -1, -1):
        hprev = h0 if t == 0 else h_all[t - 1]
        u, r, o = u_all[t].double(), r_all[t].double(), o_all[t].double()
        dho = dh_out[t].double() if dh_out is not None else torch.zeros_like(c64)
        dh = dho + c64
        ddh = dc + 2.0 * E * (dho.abs() + c64.abs())
        hp = hprev.double() if hprev is not None else torch.zeros_like(u)
        one_o2 = 1.0 - o * o
        ref_o = dh * u * one_o2
        up("dg_o", ratio(dg[t][..., 2 * h:], ref_o,
                         ddh * (u * one_o2).abs() + (dh * u).abs() * E * (o * o + one_o2.abs()) + 3.0 * E * ref_o.abs(), dtype))
        ref_u = dh * (o - hp) * u * (1.0 - u)
        up("dg_u", ratio(dg[t][..., :h], ref_u, ddh * ((o - hp) * u * (1.0 - u)).abs() + 6.0 * E * ref_u.abs(), dtype))
        c1 = dh * (1.0 - u)
        dc1 = ddh * (1.0 - u) + 2.0 * E * c1.abs()
        if hprev is None:
            up("dg_r", ratio(dg[t][..., h:2 * h], torch.zeros_like(c1), torch.zeros_like(c1), dtype))
            c64, dc = c1, dc1
            pre = (c1, dc1)
            continue
        dgo = dg[t][..., 2 * h:]
        dhr = convT64(dgo, w_o)
        ehr = conv_err(dgo, w_o, torch.zeros_like(dhr), SLABS, transposed=True)
        c2 = c1 + dhr * r
        dc2 = dc1 + ehr * r + 2.0 * E * ((dhr * r).abs() + c2.abs())
        ref_r = dhr * hp * r * (1.0 - r)
        up("dg_r", ratio(dg[t][..., h:2 * h], ref_r, ehr * (hp * r * (1.0 - r)).abs() + 5.0 * E * ref_r.abs(), dtype))
        dgur = dg[t][..., :2 * h]
        nxt = dh_out[t - 1].double().abs() if (dh_out is not None and t > 0) else torch.zeros_like(c2)
        pre = (c2, dc2)
        c64 = c2 + convT64(dgur, w_ur)
        dc = dc2 + conv_err(dgur, w_ur, c2.abs() + nxt, SLABS + 2, transposed=True)
    full = (c64, dc)
    if carry is not None:
        ref, d = full if carry_full else pre
        worst["carry"] = ratio(carry.reshape(shp), ref, d, torch.float32)
    if dh0 is not None:
        worst["dh0"] = ratio(dh0.reshape(shp), full[0], full[1], torch.float32)
    for k, v in worst.items():
        note(f"{name} {k} err/bound", v)
    return worst

"""Float64 statement of functional.Conv -- forward AND backward of y = act(conv(x; w_eff) + b [+ res]) -- on STORED operands.

A plain module (no conftest, no fixtures), torch only, CPU or GPU tensors alike; no project kernel and no oracle code takes part.
The forward is conv_ref.forward_ref.  This module states what backward() must return for a given dy, with an elementwise error
bound per output, and checks tensors against it (`check`: ratio <= 1, masked-out and padded elements exactly 0).

Operands, as they sit in memory: x [F, (T,) H, W, pad8(Cin)], res and dy [F, (T,) Ho, Wo, pad8(Cout)] channels-last in the storage
type `st` (bf16, fp32; fp64 for the comparison with autograd, where no rounding is left), the pad columns of dy zero;
w_eff [Cout][Cin][*k] read back from the forward pack (`w_from_pack`: the rounded W_bar / sigma the kernels multiply by); the
fp32 bias; the stored y.  With a spectral norm also the fp32 master W_bar, the u, v the layer holds when backward runs and the
sigma of the forward.

Definitions (those of tests/gru_ref.py and tests/conv_ref.py).  E = 2^-24.  A sum of n fp32 terms, any order: e = 2 n E A with A
the same sum of the magnitudes.  ulp(v) = one ulp of `st` at |v|.  `ratio` adds half an ulp of the output's type for its final store
(nothing for fp32 outputs: that rounding is inside e).  Where the Function rounds an INTERMEDIATE (three places, below), the
kernels' value and the reference's may fall on different sides of a tie, so the bound gains ONE ulp (not half) of the
intermediate's fp64 value -- taken at |value| + its own fp32 bound, and plus that fp32 bound, so that it also holds where fp32 IS
the storage type -- pushed in absolute value through the linear map that follows.

  dy'   act NONE: dy itself.  ReLU: (stored y > 0) ? dy : 0 -- a selection, exact: bound 0, no ulp term.
        tanh: dy (1 - y^2), sigmoid: dy y (1 - y) on the STORED y (dvd_act_backward: "dpre = dy * act'(y) expressed with the
        activation output y"), evaluated in fp32 as g *= 1 - v v  /  g *= v (1 - v): fl(v v) is rounded before the subtraction
        (absolute E y^2), the subtraction and the product are one rounding each:
            tanh     b' = E |dy| (y^2 + |1 - y^2|) + E |dy'|            sigmoid  b' = 3 E |dy'|
        (an FMA contraction only removes a rounding).  The reference rounds dy' ONCE into `st`; everything downstream is computed
        from that rounded tensor, and U = b' + ulp(|dy'| + b') is the first intermediate term (rounding point 1).
  dx    conv_ref.forward_ref of the backward-data request: input dy' (rounded), weights w_bwd[ci][co][tap] = w_eff[co][ci][-tap]
        (the transposed, flipped filter), no bias, Cout = Cin, pad8(Cin) channels.  up2: the 2 x 2 sums onto the input grid
        (pool2).  relu_in: times (stored x > 0) on the INPUT grid, after the sums.  slot: plus the partner as the request's
        residual, added BEFORE the single rounding.  Bound: forward_ref's e (n = taps * pad8(Cout) [+ 3 for the four-way sum]
        [+ 1 partner]) plus |w_bwd| applied to U (summed 2 x 2 under up2), zero where masked out.
        unfused up2 route (conv_forward at full size, rounded into `st`, then dvd_pool(scale = 1, mask)): rounding point 2.  Per
        full-size element the bound is e_full + |w_bwd| U + ulp(|a_full| + that); the 2 x 2 sum adds these, and dvd_pool's own
        four-term fp32 sum adds 4 E sum|.| (the bound tests/test_gpu_pointwise.py holds the pool kernel to).
  G, db G = conv_ref.wgrad_ref(x, dy') with relu_in / up2 applied to x, db = the column sums of dy'.  Both are sums over the
        M = F T Ho Wo output rows: e = 2 M E A with A = wgrad_ref(|x|, |dy'|) (sum |dy'|), plus wgrad_ref(|x|, U) (sum U).
        Accumulated into a prefilled buffer (the direct route), the prefill is one more term of the same sum, whatever the
        number of partial sums the kernel adds to it: e = 2 (M + 1) E (A + |prefill|) + the U term, checked on buffer - prefill.
  dw    without SN: G.  With SN (include/dvdgan_hip.h: dW_bar += G / sigma - (sum G W_bar) / sigma^2 u v^T, u / v the CURRENT
        buffers; tests/test_gpu_sn_helpers.py restates it): G is rounded into fp32 in front of dvd_sn_backward (rounding point 3):
        eG' = eG + 2 E (|G| + eG).  dot = sum G W_bar over n = Cout Cin taps elements: e_dot = sum eG' |W_bar| + 2 n E sum |G W_bar|.
        Per element dw = G / s - dot / (s s) u v evaluates with one division, s s, a division, two products and a subtraction:
        e = eG' / s + e_dot |u v| / s^2 + 6 E (|G| / s + |dot| |u v| / s^2).  Added into a prefilled `out` (one addition per
        element) the prefill form above is used with |dw| + e in the place of A: it contains that one rounding, E |out|.
  dres  dy itself, value for value (bound 0: bit equality).  A half-size residual: the 2 x 2 SUMS of dy, e = 4 E sum |dy|.

Nothing here is fitted to a kernel's output: every constant counts roundings of the expressions as the kernels write them.
"""
import torch

import conv_ref
import gru_ref

E = gru_ref.E
ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = conv_ref.ACT_NONE, conv_ref.ACT_RELU, conv_ref.ACT_TANH, conv_ref.ACT_SIGMOID
_MANT = {torch.bfloat16: 8, torch.float32: 24, torch.float64: 53}


def ulp(v, st):
    """One ulp of the storage type `st` at |v| (float64 tensor in, float64 out; 0 at 0)."""
    _, e = torch.frexp(v.abs())
    u = torch.ldexp(torch.ones_like(v), (e - _MANT[st]).to(v.dtype))
    return torch.where(v == 0, torch.zeros_like(u), u)


def w_from_pack(wf, cin, ksize):
    """The forward pack image [ntaps][Cout][pad8(Cin)] -> w_eff [Cout][Cin][*ksize] in float64: the stored, rounded weights."""
    nt, cout, _ = wf.shape
    return wf.double().permute(1, 2, 0)[:, :cin].reshape(cout, cin, *ksize).contiguous()


def _w_bwd(w_eff):
    """[Cout][Cin][*k] -> the filter of the backward-data request [Cin][Cout][*k], taps reversed"""
    return w_eff.transpose(0, 1).flip(*range(2, w_eff.dim())).contiguous()


def _sum2x2(t):
    """2 x 2 sums over H, W of a channels-last [F, (T,) H, W, C] tensor"""
    s = t.shape
    return t.reshape(*s[:-3], s[-3] // 2, 2, s[-2] // 2, 2, s[-1]).sum(dim=(-4, -2))


def _lin_abs(u, wb, up2):
    """|w_bwd| applied to the nonnegative tensor u (channels-last, any leading layout forward_ref takes), at pad8 channels"""
    lead = u.unsqueeze(1) if u.dim() == 4 else u
    w5 = wb.abs().reshape(wb.shape[0], wb.shape[1], *conv_ref._ksize3(wb.shape[2:]))
    out = conv_ref._conv64(lead[..., :wb.shape[1]].double(), w5)
    if up2:
        out = conv_ref._sum2x2(out)
    out = torch.nn.functional.pad(out, (0, conv_ref.pad8(wb.shape[0]) - wb.shape[0]))
    return out.squeeze(1) if u.dim() == 4 else out


def act_backward_ref(dy, y, act, st):
    """-> (dy' float64 before its store, fp32 bound b', dy' rounded once into `st` as float64, U)"""
    g, v = dy.double(), y.double()
    if act == ACT_NONE:
        d, b = g, torch.zeros_like(g)
    elif act == ACT_RELU:
        d, b = torch.where(v > 0, g, torch.zeros_like(g)), torch.zeros_like(g)
    elif act == ACT_TANH:
        d = g * (1 - v * v)
        b = E * g.abs() * (v * v + (1 - v * v).abs()) + E * d.abs()
    else:
        assert act == ACT_SIGMOID
        d = g * v * (1 - v)
        b = E * g.abs() * v.abs() * (1 - v).abs() * 2 + E * d.abs()
    if act in (ACT_NONE, ACT_RELU):
        return d, b, d, torch.zeros_like(d)
    dr = d.to(st).double()
    return d, b, dr, b + ulp(d.abs() + b, st)


def sn_backward_ref(G, eG, w_bar, u, v, sigma):
    """dW_bar of dvd_sn_backward and its bound from G (float64) with bound eG; w_bar / u / v / sigma fp32 as stored."""
    W, s = w_bar.double(), float(sigma.double().reshape(()))
    h = W.shape[0]
    eG = eG + 2 * E * (G.abs() + eG)                       # rounding point 3: G as an fp32 tensor
    dot = float((G * W).sum())
    e_dot = float((eG * W.abs()).sum()) + 2 * G.numel() * E * float((G * W).abs().sum())
    uv = torch.outer(u.double().reshape(-1), v.double().reshape(-1)).reshape(W.shape)
    assert u.numel() == h and u.numel() * v.numel() == W.numel()
    dw = G / s - dot / (s * s) * uv
    e = eG / abs(s) + e_dot * uv.abs() / (s * s) + 6 * E * (G.abs() / abs(s) + abs(dot) * uv.abs() / (s * s))
    return dw, e


def conv_backward_ref(x, w_eff, y, dy, ksize, st, *, act=ACT_NONE, up2=False, relu_in=False, partner=None, unfused=False,
                      res_up2=None, sn=None):
    """The float64 statement of Conv.backward for one dy.  x, y, dy, partner: stored tensors (see the module docstring);
    unfused: the up2 backward-data pass ran as conv + pool (rounding point 2); res_up2: None = no residual, False = full-size,
    True = half-size; sn: None or (w_bar, u, v, sigma).  Returns a dict  name -> (ref, bound, keep)  for
      dyp   dy' before its store (keep all true)        dx    [.., pad8(Cin)] on the input grid
      G     the raw weight gradient [Cout][Cin][*k]      dw    what the Function returns / accumulates (G, or the SN formula)
      db    [Cout]                                       dres  only with a residual
    keep False = masked out or padded: ref = bound = 0, the output must be exactly 0."""
    cout, cin = w_eff.shape[:2]
    ksize = tuple(ksize)
    out = {}
    d, b, dr, U = act_backward_ref(dy, y, act, st) if act != ACT_NONE else act_backward_ref(dy, dy, ACT_NONE, st)
    out["dyp"] = (d, b, torch.ones_like(d, dtype=torch.bool))
    # ---- dx
    wb = _w_bwd(w_eff.double())
    mask = x if relu_in else None
    if up2 and unfused:
        a, e, _ = conv_ref.forward_ref(dr, wb)
        ef = e + _lin_abs(U, wb, False)
        ef = ef + ulp(a.abs() + ef, st)
        ref, bound = _sum2x2(a), _sum2x2(ef) + 4 * E * _sum2x2(a.abs() + ef)
        keep = torch.zeros_like(ref, dtype=torch.bool)
        keep[..., :cin] = (x[..., :cin] > 0) if relu_in else True
        zero = torch.zeros_like(ref)
        ref, bound = torch.where(keep, ref, zero), torch.where(keep, bound, zero)
    else:
        ref, bound, keep = conv_ref.forward_ref(dr, wb, mask=mask, res=partner, pool2=up2)
        bound = bound + torch.where(keep, _lin_abs(U, wb, up2), torch.zeros_like(bound))
    out["dx"] = (ref, bound, keep)
    # ---- G, db, dw
    xs, ds, Us = x[..., :cin].double(), dr[..., :cout], U[..., :cout]
    G, db = conv_ref.wgrad_ref(xs, ds, ksize, up2=up2, relu_in=relu_in)
    A, Ab = conv_ref.wgrad_ref(xs.abs() if not relu_in else xs, ds.abs(), ksize, up2=up2, relu_in=relu_in)
    UG, Ub = conv_ref.wgrad_ref(xs.abs() if not relu_in else xs, Us, ksize, up2=up2, relu_in=relu_in)
    M = ds.numel() // cout
    out["M"] = M
    eG, eb = 2 * M * E * A + UG, 2 * M * E * Ab + Ub
    allk = lambda t: torch.ones_like(t, dtype=torch.bool)
    out["G"] = (G, eG, allk(G))
    out["db"] = (db, eb, allk(db))
    if sn is not None:
        dw, ew = sn_backward_ref(G, eG, *sn)
        out["dw"] = (dw, ew, allk(dw))
        out["mag"] = {"dw": dw.abs() + ew, "db": Ab}
    else:
        out["dw"] = out["G"]
        out["mag"] = {"dw": A, "db": Ab}
    # ---- dres
    if res_up2 is not None:
        g = dy.double()
        if res_up2:
            out["dres"] = (_sum2x2(g), 4 * E * _sum2x2(g.abs()), allk(_sum2x2(g)))
        else:
            out["dres"] = (g, torch.zeros_like(g), allk(g))
    return out


def accumulated(refs, name, prefill):
    """(ref, bound, keep) of buffer - prefill for an output the kernels ADDED into a prefilled fp32 buffer: the prefill is one
    more term of the sum (see the module docstring)."""
    ref, bound, keep = refs[name]
    return ref, bound + 2 * E * (refs["M"] + 1) * prefill.double().abs() + 2 * E * refs["mag"][name], keep


def ratio(out, ref, bound, dtype):
    """gru_ref.ratio; a float64 output is held to the bound alone"""
    return gru_ref.ratio(out, ref, bound, torch.float32 if dtype == torch.float64 else dtype)


def check(name, out, refs, key=None, dtype=None, entry=None):
    """out against refs[key] = (ref, bound, keep), or against `entry`: masked-out / padded elements exactly 0, ratio <= 1 (with half
    an ulp of `dtype`, default the output's own type, for its final store).  Raises AssertionError; returns the ratio."""
    ref, bound, keep = entry if entry is not None else refs[key]
    dtype = dtype or out.dtype
    if tuple(out.shape) != tuple(ref.shape):
        raise AssertionError(f"{name}: shape {tuple(out.shape)}, expected {tuple(ref.shape)}")
    if bool((out[~keep] != 0).any()):
        raise AssertionError(f"{name}: a masked-out or padded element is not exactly 0")
    r = ratio(out, ref, bound, dtype)
    gru_ref.note(f"{name} err/bound", r)
    if not r <= 1.0:
        raise AssertionError(f"{name}: err / bound = {r:.3e}")
    return r


def check_backward(name, refs, *, dx=None, dres=None, dw=None, db=None, dw_prefill=None, db_prefill=None):
    """Everything one backward() left, against `refs` (conv_backward_ref); None = not produced, not checked.  dw / db: what the
    Function returned, or -- with a prefill -- the .grad buffer it accumulated into, checked on buffer - prefill.  dres of a
    full-size residual must equal dy bit for bit (its bound is 0).  Raises AssertionError naming the output; returns the ratios."""
    r = {}
    if dx is not None:
        r["dx"] = check(f"{name} dx", dx, refs, "dx")
    if dres is not None:
        r["dres"] = check(f"{name} dres", dres, refs, "dres")
    for key, out, pre in (("dw", dw, dw_prefill), ("db", db, db_prefill)):
        if out is None:
            continue
        if out.dtype != torch.float32:
            raise AssertionError(f"{name} {key}: dtype {out.dtype}, parameter gradients are fp32")
        if pre is None:
            r[key] = check(f"{name} {key}", out, refs, key)
        else:
            r[key] = check(f"{name} {key} (buffer - prefill)", out.double() - pre.double(), None, dtype=torch.float32,
                           entry=accumulated(refs, key, pre))
    return r

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

forward_ref / forward_ratio / check_forward are the forward counterpart: the direct epilogue of the forward / backward-data kernels
(conv_epilogue of csrc/conv_common.h, the epilogues of csrc/conv_thin.hip) in float64, in the order the kernels write it,

    a = (conv + bias) + res  ->  activation  ->  (mask > 0 ? v : 0)  ->  zeros in the channels [Cout, pad8(Cout))

or, for a pool2 request, a = 4 bias + the 2 x 2 sum of conv on the half-size grid (no residual, no activation; mask and output live
on that grid), with an elementwise error bound built from the definitions of tests/gru_ref.py: E = 2^-24, e = 2 n E A with
n = taps * Cp + addends (bias 1, residual 1, the four-way sum of pool2 3) and A the same convolution of |x| and |w| plus |bias| and
|res| (under pool2 the 2 x 2 sum of the per-pixel values).  ReLU is 1-Lipschitz: the bound stays e.  tanh / sigmoid: e carried
through the monotone function exactly (gru_ref._mono_bound) plus the function term of gru_ref._ftanh / _fsig, whose derivation is
in that module.  A masked-out or padded element has bound 0: it must be exactly 0.  Nothing here is fitted to a kernel's output.
"""
import torch

import gru_ref

SENT = 0xA5                    # the byte every output buffer and arena gap is prefilled with (tests/test_gpu_gru.py: Arena)
ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3         # DVD_ACT_* of include/dvdgan_hip.h


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


# ------------------------------------------------------------------ forward / backward-data: the direct epilogue
def pad8(c):
    return (c + 7) // 8 * 8


def _up2(t):
    """nearest x2 along H and W of a channels-last [F, T, H, W, C] tensor"""
    return t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def _conv64(x5, w5):
    """'same' zero-padded cross-correlation, one float64 matrix product per tap.  x5 [F, T, H, W, Cin], w5 [Cout, Cin, kt, kh, kw]."""
    F_, T, H, W, cin = x5.shape
    kt, kh, kw = w5.shape[2:]
    xp = torch.nn.functional.pad(x5, (0, 0, kw // 2, kw // 2, kh // 2, kh // 2, kt // 2, kt // 2))
    out = torch.zeros(F_ * T * H * W, w5.shape[0], dtype=torch.float64, device=x5.device)
    for it in range(kt):
        for iy in range(kh):
            for ix in range(kw):
                out += xp[:, it:it + T, iy:iy + H, ix:ix + W, :].reshape(-1, cin) @ w5[:, :, it, iy, ix].t()
    return out.view(F_, T, H, W, -1)


def _sum2x2(t):
    F_, T, H, W, Cc = t.shape
    return t.view(F_, T, H // 2, 2, W // 2, 2, Cc).sum(dim=(3, 5))


def forward_ref(x, w, *, bias=None, res=None, res_up2=False, act=ACT_NONE, mask=None, up2=False, relu_in=False, pool2=False,
                exact=False):
    """x [F, (T,) H, W, Cp] as stored (channels from Cin on are ignored), w [Cout, Cin, *k] the master ALREADY ROUNDED to the storage
    type, bias [Cout] fp32, res [.., >= Cout] on the output grid (res_up2: on the half-size grid), mask [.., >= Cout] on the output
    grid (pool2: the half-size grid) -> (ref, bound, keep) on the output grid with pad8(Cout) channels, ref / bound float64.
    keep = (mask > 0) by the IEEE comparison on the stored mask (all true without a mask); it is False in the padded channels:
    wherever keep is False, ref = 0 and bound = 0.  exact: the fp32 mode's libm activations (gru_ref._ftanh / _fsig)."""
    assert x.dim() in (4, 5)
    cout, cin = w.shape[:2]
    w5 = w.double().reshape(cout, cin, *_ksize3(w.shape[2:]))
    assert w5.shape[2] & w5.shape[3] & w5.shape[4] & 1, "odd taps"
    lead = (lambda t: t.unsqueeze(1)) if x.dim() == 4 else (lambda t: t)
    x5 = lead(x)[..., :cin].double()
    if relu_in:
        x5 = x5.clamp_min(0.0)
    if up2:
        x5 = _up2(x5)
    a, A = _conv64(x5, w5), _conv64(x5.abs(), w5.abs())
    n = w5.shape[2] * w5.shape[3] * w5.shape[4] * x.shape[-1]
    if pool2:
        assert res is None and act == ACT_NONE and not up2 and w5.shape[2] == 1
        a, A = _sum2x2(a), _sum2x2(A)
        n += 3
        if bias is not None:
            a, A, n = 4.0 * bias.double() + a, A + 4.0 * bias.double().abs(), n + 1
    else:
        if bias is not None:
            a, A, n = a + bias.double(), A + bias.double().abs(), n + 1
        if res is not None:
            r = lead(res)[..., :cout].double()
            if res_up2:
                r = _up2(r)
            a, A, n = a + r, A + r.abs(), n + 1
    e = 2.0 * n * gru_ref.E * A
    if act == ACT_RELU:
        v, b = a.clamp_min(0.0), e
    elif act == ACT_TANH:
        v, b = torch.tanh(a), gru_ref._mono_bound(torch.tanh, a, e) + gru_ref._ftanh(a, exact)
    elif act == ACT_SIGMOID:
        v, b = torch.sigmoid(a), gru_ref._mono_bound(torch.sigmoid, a, e) + gru_ref._fsig(a, exact)
    else:
        assert act == ACT_NONE
        v, b = a, e
    keep = (lead(mask)[..., :cout] > 0) if mask is not None else torch.ones_like(v, dtype=torch.bool)
    assert keep.shape == v.shape, (keep.shape, v.shape)
    zero = torch.zeros_like(v)
    padc = (0, pad8(cout) - cout)
    fin = lambda t: torch.nn.functional.pad(t, padc).squeeze(1) if x.dim() == 4 else torch.nn.functional.pad(t, padc)
    return fin(torch.where(keep, v, zero)), fin(torch.where(keep, b, zero)), fin(keep)


def forward_ratio(out, ref, bound, dtype):
    """worst |out - ref| / (bound + half an ulp of `dtype` at |ref| + bound); inf where `out` is not finite (gru_ref.ratio)"""
    return gru_ref.ratio(out, ref, bound, dtype)


def zero_pass_act(act):
    """The zero-input pass runs with no activation or ReLU only (tanh(bias + res) is not a bit-exact statement): a tanh / sigmoid
    request is repeated WITHOUT its activation -- the addresses of bias, residual and mask do not depend on it."""
    return act if act in (ACT_NONE, ACT_RELU) else ACT_NONE


def zero_input_expected(w, shape, *, bias=None, res=None, res_up2=False, act=ACT_NONE, mask=None, pool2=False):
    """What the fp32 output of the request must be, bit for bit, when x = 0 (every accumulator is exactly +0): the same few fp32
    operations on the stored operands.  shape: the output grid [F, (T,) H, W]; returns fp32 [*shape, pad8(Cout)]."""
    cout = w.shape[0]
    ref = bias if bias is not None else res if res is not None else mask
    dev = ref.device if ref is not None else "cpu"
    v = torch.zeros(*shape, cout, dtype=torch.float32, device=dev)
    if bias is not None:
        v = v + (4.0 * bias.float() if pool2 else bias.float())
    if res is not None and not pool2:
        r = res[..., :cout].float()
        if res_up2:
            r = r.repeat_interleave(2, dim=-3).repeat_interleave(2, dim=-2)
        v = v + r
    if zero_pass_act(act) == ACT_RELU:
        v = v.clamp_min(0.0)
    if mask is not None:
        v = torch.where(mask[..., :cout] > 0, v, torch.zeros_like(v))
    return torch.nn.functional.pad(v, (0, pad8(cout) - cout))


def _bytes(t):
    return t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------ the requests the model sends, on stored operands
POISON = 1024.0                # the columns past pad8(Cout) of a residual / mask: finite, 2^10 times the data's scale
KINDS = ("res", "res_up2", "relu", "tanh", "sigmoid", "bwd", "pool2", "pool2_bias")
MASK_EDGE = (0.0, -0.0, 2.0 ** -126, -2.0 ** -126, float("inf"), -float("inf"))


def plant_mask_edges(mask, cp):
    """In every fourth row of mask [.., ld] (so in every 32-row sub-tile of any tile, whatever its row order) and in EVERY 8-column
    group of columns [0, cp): +0, -0, +-2^-126 and +-inf at six of the eight columns, the start rotating with the row."""
    m2 = mask.view(-1, mask.shape[-1])
    rows = torch.arange(0, m2.shape[0], 4, device=mask.device)
    groups = torch.arange(0, cp, 8, device=mask.device)
    for j, val in enumerate(MASK_EDGE):
        cols = groups[None, :] + ((j + rows // 4) % 8)[:, None]
        m2[rows[:, None], cols] = val
    return mask


def make_request(case, kind, dtype, device, seed, with_res=True):
    """Stored operands of one (case, kind) at the scale tests/test_gpu_conv.py uses (randn inputs, residuals and masks, weights
    randn / sqrt(fan-in), randn bias), all drawn in the storage type from a fixed seed.
    case = (frames, output side S, Cin, Cout, k, up2, relu_in).  Returns a dict:
      x          [F, Sin, Sin, pad8(Cin)] stored input
      master     fp32 master [pack Cout][pack Cin][k][k], already rounded to the storage type, for PackedConv(dtype, *pack).fill
      pack       (cout_tot, cin) of that PackedConv;  which: "wf" or "wd", the image the request reads
      w          the weights of the REQUEST [Cout][Cin][k][k] in float64 (for "bwd": the flipped transpose of the master, zero rows up
                 to pad8: the request's Cout is the pack's padded input width)
      req        the options of forward_ref / kern.conv_forward: bias, res (ld = pad8 + 16), mask (ld = pad8 + 24), res_up2, act, up2,
                 relu_in, pool2
    with_res=False: the thin kernels take no residual."""
    F_, S, cin, cout, k, up2, relu_in = case
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    bwd = kind == "bwd"
    pool2 = kind.startswith("pool2")
    if bwd or pool2:
        assert not up2 and not relu_in
    Sin = S // 2 if up2 else S
    x = rn(F_, Sin, Sin, pad8(cin)).to(dtype)
    if bwd:       # the pack of the convolution this request is the backward-data pass of: `cout` -> `cin` channels
        master = (rn(cin, cout, k, k) / (cout * k * k) ** 0.5).to(dtype).float().contiguous()
        pack, which = (cin, cout), "wd"
        w = torch.zeros(pad8(cout), cin, k, k, dtype=torch.float64, device=device)
        w[:cout] = master.double().transpose(0, 1).flip(-1, -2)
    else:
        master = (rn(cout, cin, k, k) / (cin * k * k) ** 0.5).to(dtype).float().contiguous()
        pack, which, w = (cout, cin), "wf", master.double()
    co = w.shape[0]
    cp = pad8(co)
    So = S // 2 if pool2 else S
    req = dict(up2=up2, relu_in=relu_in, pool2=pool2, res_up2=kind == "res_up2",
               act={"relu": ACT_RELU, "tanh": ACT_TANH, "sigmoid": ACT_SIGMOID}.get(kind, ACT_NONE))
    if not bwd and kind != "pool2":
        req["bias"] = rn(co)
    if with_res and not pool2:
        Sr = S // 2 if req["res_up2"] else S
        res = rn(F_, Sr, Sr, cp + 16)
        res[..., cp:] *= POISON
        req["res"] = res.to(dtype)
    if kind in ("relu", "tanh", "sigmoid", "bwd", "pool2", "pool2_bias"):
        mask = rn(F_, So, So, cp + 24)
        mask[..., cp:] *= POISON
        req["mask"] = plant_mask_edges(mask.to(dtype), cp)
    return dict(x=x, master=master, pack=pack, which=which, w=w, req=req)


def check_forward(name, dtype, x, w, out32, out_st, *, zero32=None, sent=SENT, gaps_intact=True, **req):
    """The checks of one (request, fp32-output call, storage-output call) on the buffers the calls wrote INTO: out32 (fp32) and
    out_st (`dtype`) are [.., ldo] with ldo >= pad8(Cout), prefilled with the byte `sent`; zero32: the fp32 output buffer of the
    same request on x = 0 with the activation zero_pass_act(act), or None; gaps_intact: the sentinel gaps around the buffers
    still hold their bytes; req: the options of forward_ref (the float64 reference is formed here, once).  Raises AssertionError
    naming the check; returns the worst err / bound ratio of the fp32 output.
      1 zero-input    zero32 is bit-equal to zero_input_expected
      2 fp64          the fp32 output within its bound (ratio <= 1), every masked-out and padded element exactly 0
      3 storage       out_st is torch.equal to out32.to(dtype): both stores leave the same fp32 value
      4 untouched     columns >= pad8(Cout) keep the sentinel bytes, columns [Cout, pad8(Cout)) are zero, the gaps are intact"""
    cout = w.shape[0]
    cp = pad8(cout)
    exact = dtype == torch.float32
    fail = lambda check, what: AssertionError(f"{name}: check {check}: {what}")
    opts = {k: req.get(k) for k in ("bias", "res", "mask")}
    opts.update(res_up2=req.get("res_up2", False), act=req.get("act", ACT_NONE), pool2=req.get("pool2", False))
    if zero32 is not None:
        want0 = zero_input_expected(w, out32.shape[:-1], **opts)
        got0 = zero32[..., :cp]
        if not torch.equal(got0, want0.to(got0.device)):
            raise fail("1 zero-input", f"{int((got0 != want0.to(got0.device)).sum())} elements differ from the fp32 torch ops")
    want, bound, keep = forward_ref(x, w, exact=exact, **req)
    got = out32[..., :cp]
    r32 = forward_ratio(got, want, bound, torch.float32)
    gru_ref.note(f"{name} fp32 err/bound", r32)
    if not r32 <= 1.0:
        raise fail("2 fp64", f"fp32 output err / bound = {r32:.3e}")
    if bool((got[~keep] != 0).any()):
        raise fail("2 fp64", "a masked-out or padded element is not exactly 0")
    st = out_st[..., :cp]
    if not torch.equal(st, got.to(dtype)):
        raise fail("3 storage", f"{int((st != got.to(dtype)).sum())} elements differ from the rounded fp32 output")
    rst = forward_ratio(st, want, bound, dtype)
    gru_ref.note(f"{name} storage err/bound", rst)
    if not rst <= 1.0:
        raise fail("3 storage", f"storage output err / (bound + half an ulp) = {rst:.3e}")
    for what, buf in (("fp32 output", out32), ("storage output", out_st), ("zero-input output", zero32)):
        if buf is None:
            continue
        if buf.shape[-1] > cp and not bool((_bytes(buf[..., cp:]) == sent).all()):
            raise fail("4 untouched", f"{what}: a column at or past pad8(Cout) lost its sentinel bytes")
        if bool((buf[..., cout:cp] != 0).any()):
            raise fail("4 untouched", f"{what}: a padded channel is not zero")
    if not gaps_intact:
        raise fail("4 untouched", "the sentinel gaps around the output buffers were written")
    return r32

"""GPU parity of the attention kernels (attn_mfma.hip, attn.hip, sepattn.hip) against plain float64 torch references, called
through their C entry points (no 1x1 convolution in front), at the benchmark's shapes and at the edges where their code changes.

Every reference is computed on the GPU in float64 from the operands as stored (q | k | v as they sit in the bf16 or fp32 `qkv`
buffer, x, dy, gamma); no project kernel and no oracle code takes part in it.  Forward, as attn.hip states it:
A = softmax_j(q_i . k_j) (no scale), out = A v, y = gamma * out + x.  Backward: dS = gamma A (dy v^T - D), dq = dS k,
dk = dS^T q, dv = gamma A^T dy, dgamma += sum D.  The MFMA kernels take D_i = dy_i . att_out_i from the STORED att_out (their
ABI); the fp32 kernels derive it from their own A (D_i = sum_j A_ij dA_ij), which the reference restates.

Bounds are elementwise where the kernel has an error model:
  MFMA  : the probabilities (forward, dv) and dS (dq, dk) are rounded to bf16 before their product -> 2^-8 (the unit roundoff
          of bf16, = 2 * 2^-9) * the matching product of magnitudes, plus the fp32 terms (scores, exp, row sums, accumulation,
          lse carried into the backward) and half a bf16 ulp of the stored result: worst-case bounds, c = 1;
  fp32  : c * 2^-24 * a propagated magnitude (score error -> probabilities -> products; sums of n terms count sqrt(n)),
          plus half an ulp of the storage type.
The separable cell's long products (up to 65536 terms per score) are modelled the same way; its gradients, which pass through
the score and datt products and the max-pool routing, are held to rel-L2.  Each check prints a MEASURED line: the worst
err / bound, so that `pytest -s` shows how much room each bound leaves.
"""
import ctypes as ct
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
E32 = 2.0 ** -24
E16 = 2.0 ** -8                  # unit roundoff of bf16 (8 significant bits): |bf16(p) - p| <= 2^-8 |p|

# the constants c of the bounds (see the module docstring); profiles/attention_parity_numbers.md has the measured maxima
C_MFMA = {"att": 1.0, "y": 1.0, "lse": 4.0, "D": 4.0, "dq": 1.0, "dk": 1.0, "dv": 1.0, "dgamma": 0.1}
C_F32 = {"A": 4.0, "att": 4.0, "y": 4.0, "dS": 2.0, "dq": 2.0, "dk": 2.0, "dv": 4.0, "dgamma": 0.5}
C_SEP = {"att": 2.0, "y": 1.5, "dgamma": 0.1, "dq": 5e-6, "dk": 5e-6, "dv": 5e-6, "dq_bf16": 2.5e-3, "dk_bf16": 2.5e-3,
         "dv_bf16": 2.5e-3}
TINY = 2.0 ** -125               # absolute floor of the fp32 probabilities: exp(s - max) below 2^-126 leaves the normal range


def note(name, value):
    print(f"MEASURED {name}: {value:.3e}")


def lib():
    from dvd_gan_amd import lib as L
    return L.lib()


def P(t):
    from dvd_gan_amd import lib as L
    return L.ptr(t)


def S():
    from dvd_gan_amd import lib as L
    return L.stream()


def ok(code):
    from dvd_gan_amd import lib as L
    L.check(code)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(shape, seed):
    return torch.randn(shape, generator=gen(seed), device=DEV)


def half_ulp(ref, dtype):
    """Half an ulp of `dtype` at |ref| (0 for fp32: its rounding is inside the fp32 bound)."""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref.abs().float())
    h = torch.ldexp(torch.ones_like(ref), (e - 9).to(ref.dtype))
    return torch.where(ref == 0, torch.zeros_like(h), h)


def ratio(out, ref, bound, dtype):
    """worst |out - ref| / (bound + half an ulp of the storage type); > 1 = outside the bound, inf where `out` is not finite (the
    outputs start as NaN: an element left unwritten fails).  The ulp is taken at |ref| + bound, the top of the interval the
    unrounded result lies in (just below a power of two it may round into the next binade)."""
    err = (out.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    allowed = bound + half_ulp(ref.abs() + bound, dtype)
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


class Worst:
    """running maxima of err / bound per check over the frame chunks of one case"""

    def __init__(self, name):
        self.name, self.r, self.l2n, self.l2d = name, {}, {}, {}

    def add(self, key, val):
        self.r[key] = max(self.r.get(key, 0.0), math.inf if math.isnan(val) else val)

    def l2(self, key, out, ref):
        self.l2n[key] = self.l2n.get(key, 0.0) + float(((out.double() - ref) ** 2).sum())
        self.l2d[key] = self.l2d.get(key, 0.0) + float((ref ** 2).sum())

    def check(self, consts):
        bad = []
        for k, v in self.r.items():
            note(f"{self.name} {k} err/bound", v)
            if not v <= 1.0:
                bad.append((k, v))
        for k in self.l2n:
            v = (self.l2n[k] / max(self.l2d[k], 1e-300)) ** 0.5
            note(f"{self.name} {k} rel-L2", v)
            if not v <= consts[k]:                          # (a NaN in the output makes the sums NaN)
                bad.append((k, v))
        assert not bad, f"{self.name}: outside the bounds {bad}"


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def frame_chunks(frames, per_frame, budget=1 << 22):
    step = max(1, budget // per_frame)
    for f0 in range(0, frames, step):
        yield f0, min(frames, f0 + step)


# ------------------------------------------------------------------------------------------------ data
def make_qk(F, N, Nk, dq, regime, seed):
    """fp32 q [F, N, dq] and k [F, Nk, dq] in one of the data regimes"""
    if regime == "units":                   # scores of a few units
        return 0.6 * randn((F, N, dq), seed), 0.6 * randn((F, Nk, dq), seed + 1)
    if regime == "large":                   # |s| of 60 .. 100: an exp without a running max overflows fp32
        sc = 5.0 / dq ** 0.25                 # score std 25 whatever dq
        return sc * randn((F, N, dq), seed), sc * randn((F, Nk, dq), seed + 1)
    if regime == "last":                    # every row's maximum among the last keys (the last 256-key chunk): the rescale runs
        u = torch.ones(dq, device=DEV) * (2.0 / math.sqrt(dq))
        q = 0.4 * randn((F, N, dq), seed) + u
        k = 0.4 * randn((F, Nk, dq), seed + 1)
        k[:, max(0, Nk - 32):] += 3 * u
        return q, k
    if regime == "onehot":                  # nearly one-hot rows: q_i = 4 k_{pi(i)} + noise
        k = 3.0 / math.sqrt(dq) * randn((F, Nk, dq), seed + 1)     # |k|^2 = 9 whatever dq: the winner scores 36
        pi = torch.randint(0, Nk, (F, N), generator=gen(seed + 2), device=DEV)
        q = 4 * torch.gather(k, 1, pi[..., None].expand(F, N, dq)) + 0.05 * randn((F, N, dq), seed)
        return q, k
    raise ValueError(regime)


def make_case(F, N, Nk, dq, koff, voff, C, ldq, ldk, ldx, dtype, regime, self_attn, seed):
    """q buffer [F, N, ldq] (q at columns [0, dq)), kv buffer [F, Nk, ldk] (k at [koff, +dq), v at [voff, +C)), x, dy [F, N, ldx];
    pad columns hold finite garbage.  Self attention: one buffer holds q | k | v (N = Nk)."""
    q, k = make_qk(F, N, Nk, dq, regime, seed)
    qb = randn((F, N, ldq), seed + 3)
    qb[..., :dq] = q
    if self_attn:
        qb[..., koff:koff + dq] = k
        qb[..., voff:voff + C] = randn((F, N, C), seed + 4)
        kvb = qb
    else:
        kvb = randn((F, Nk, ldk), seed + 5)
        kvb[..., koff:koff + dq] = k
        kvb[..., voff:voff + C] = randn((F, Nk, C), seed + 4)
        kvb = kvb.to(dtype).contiguous()
    qb = qb.to(dtype).contiguous()
    if self_attn:
        kvb = qb
    x = randn((F, N, ldx), seed + 6).to(dtype).contiguous()
    dy = randn((F, N, ldx), seed + 7).to(dtype).contiguous()
    return qb, kvb, x, dy


def written_columns(ld, spans):
    m = torch.zeros(ld, dtype=torch.bool, device=DEV)
    for a, n in spans:
        m[a:a + n] = True
    return m


def check_columns(buf, spans, name):
    m = written_columns(buf.shape[-1], spans)
    assert bool(torch.isfinite(buf[..., m].float()).all()), name + ": a q | k | v column was not written"
    assert bool(torch.isnan(buf[..., ~m].float()).all()), name + ": a column outside q | k | v was written"


# ------------------------------------------------------------------------------------------------ 2-D attention references
def ref_forward(qb, kvb, x, g, dq, koff, voff, C, f0, f1):
    q = qb[f0:f1, :, :dq].double()
    k = kvb[f0:f1, :, koff:koff + dq].double()
    v = kvb[f0:f1, :, voff:voff + C].double()
    s = q @ k.transpose(1, 2)
    m = s.amax(-1, keepdim=True)
    lse = m + (s - m).exp().sum(-1, keepdim=True).log()
    A = (s - lse).exp()
    out = A @ v
    y = g * out + x[f0:f1, :, :C].double()
    return q, k, v, s, m, lse, A, out, y


def run_mfma(qkv, x, dy, gamma, C, F, N, dgamma=None):
    ldq = qkv.shape[-1]
    y, att = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    lse = torch.full((F, N), float("nan"), device=DEV)
    ok(lib().dvd_attention_mfma_forward(P(qkv), ldq, P(x), C, P(gamma), P(y), P(att), P(lse), ct.c_longlong(F), N, S()))
    D = torch.full((F, N), float("nan"), device=DEV)
    dqkv = torch.full_like(qkv, float("nan"))
    ok(lib().dvd_attention_mfma_backward(P(qkv), ldq, P(dy), C, P(gamma), P(att), P(lse), P(D), P(dqkv), P(dgamma),
                                         ct.c_longlong(F), N, S()))
    return y, att, lse, D, dqkv


def mfma_case(name, F, N, C, regime, g, seed, ldq=None):
    """dvd_attention_mfma_forward / backward against fp64 (bf16 storage, q | k | v at 0 | 16 | 32)"""
    ldq = ldq or 32 + C
    assert lib().dvd_attention_mfma_ok(1, ldq, 16, 16, 32, C, C, N) == 1
    qkv, _, x, dy = make_case(F, N, N, 16, 16, 32, C, ldq, ldq, C, torch.bfloat16, regime, True, seed)
    gamma = torch.tensor([g], device=DEV)
    y, att, lse, D, dqkv = run_mfma(qkv, x, dy, gamma, C, F, N)
    dg0 = torch.tensor([0.375], device=DEV)
    dgamma = dg0.clone()
    y2, att2, lse2, D2, dqkv2 = run_mfma(qkv, x, dy, gamma, C, F, N, dgamma)
    dgamma2 = dg0.clone()
    run_mfma(qkv, x, dy, gamma, C, F, N, dgamma2)
    for a, b, n in ((y, y2, "y"), (att, att2, "att"), (lse, lse2, "lse"), (D, D2, "D"), (dqkv, dqkv2, "dqkv")):
        assert same_bits(a, b), f"{name}: rerun of {n} differs"
    assert same_bits(dgamma, dgamma2), name + ": rerun of dgamma differs"
    check_columns(dqkv, [(0, 16), (16, 16), (32, C)], name + " dqkv")
    if g == 0.0:
        assert same_bits(y, x), name + ": y != x with gamma = 0"
    w = Worst(name)
    dsum, dmag = mfma_bounds(w, F, N, C, g, qkv, x, dy, y, att, lse, D, dqkv)
    w.add("dgamma", abs(float(dgamma) - (0.375 + dsum)) / (C_MFMA["dgamma"] * E32 * (dmag + 0.375)))
    w.check(C_MFMA)


def mfma_bounds(w, F, N, C, g, qkv, x, dy, y, att, lse, D, dqkv):
    """The elementwise checks of the MFMA kernels' outputs (q | k | v at 0 | 16 | 32 of qkv [F, N, ldq]; x, dy, y, att [F, N, C];
    lse, D [F, N]; dqkv like qkv) added to the Worst `w`; lse = None / D = None: that buffer is not at hand (a caller that sees
    only what the autograd Function keeps) and its check is left out -- the bounds of the others do not change.  Returns
    (sum, sum of magnitudes) of dy * att_out, the terms of dgamma."""
    dsum, dmag = 0.0, 0.0
    for f0, f1 in frame_chunks(F, N * N):
        q, k, v, s, m, lse_r, A, out, y_r = ref_forward(qkv, qkv, x, g, 16, 16, 32, C, f0, f1)
        # fp32 terms, worst case under the model "an n-term fp32 sum (an MFMA accumulation included) lies within 2 n 2^-24 of the
        # sum of its magnitudes": sig = relative error of a probability before its bf16 rounding (16-term score: 32 E |q||k|;
        # the exp argument and exp2 scaling: 2 E |s - max|; the exp itself: 4 E); the row sum, the N-term accumulation of P V,
        # the rescales and the final division: E (5 N + 16) relative
        qk = q.abs() @ k.abs().transpose(1, 2)
        sig = E32 * (32 * qk + 2 * (s - m).abs() + 4)
        av = A @ v.abs()
        f32_att = (A * sig) @ v.abs() + av * ((A * sig).sum(-1, keepdim=True) + E32 * (5 * N + 16))
        b_att = C_MFMA["att"] * (E16 * (av + f32_att) + f32_att)
        w.add("att", ratio(att[f0:f1], out, b_att, torch.bfloat16))
        w.add("y", ratio(y[f0:f1], y_r, C_MFMA["y"] * abs(g) * (E16 * (av + f32_att) + f32_att)
                         + 2 * E32 * ((g * out).abs() + x[f0:f1].double().abs()), torch.bfloat16))
        b_lse = C_MFMA["lse"] * E32 * (qk.amax(-1) + lse_r[..., 0].abs() + 1)
        if lse is not None:
            w.add("lse", ratio(lse[f0:f1], lse_r[..., 0], b_lse, torch.float32))
        dyd, atd = dy[f0:f1].double(), att[f0:f1].double()
        D_r = (dyd * atd).sum(-1)
        Dmag = (dyd * atd).abs().sum(-1)
        if D is not None:
            w.add("D", ratio(D[f0:f1], D_r, C_MFMA["D"] * E32 * Dmag, torch.float32))
        dsum += float(D_r.sum())
        dmag += float(Dmag.sum())
        dp = dyd @ v.transpose(1, 2)
        dS = g * A * (dp - D_r[..., None])
        # the backward recomputes the probabilities as exp(s - lse) from the stored lse (checked above: its asserted bound enters
        # here); dp and D are C-term fp32 sums; dS = g p (dp - D) rounds twice more.  dS, dq, dk, dv: N-term accumulations of
        # bf16-rounded operands.
        sigb = E32 * (32 * qk + 2 * (s - lse_r).abs() + 4) + b_lse[..., None]
        ddS = (abs(g) * A * (sigb * (dp - D_r[..., None]).abs()
                             + 2 * C * E32 * (dyd.abs() @ v.abs().transpose(1, 2) + Dmag[..., None])) + 4 * E32 * dS.abs())
        acc = (1 + E16) * (E16 + 2 * N * E32)
        dq_r, dk_r, dv_r = dS @ k, dS.transpose(1, 2) @ q, g * A.transpose(1, 2) @ dyd
        got = dqkv[f0:f1].double()
        w.add("dq", ratio(got[..., :16], dq_r, C_MFMA["dq"] * (acc * ((dS.abs() + ddS) @ k.abs()) + ddS @ k.abs()), torch.bfloat16))
        w.add("dk", ratio(got[..., 16:32], dk_r, C_MFMA["dk"] * (acc * ((dS.abs() + ddS).transpose(1, 2) @ q.abs())
                                                                  + ddS.transpose(1, 2) @ q.abs()), torch.bfloat16))
        pA = A * (1 + sigb)
        w.add("dv", ratio(got[..., 32:32 + C], dv_r, C_MFMA["dv"] * abs(g) * (acc * (pA.transpose(1, 2) @ dyd.abs())
                                                                              + (A * sigb).transpose(1, 2) @ dyd.abs()
                                                                              + 2 * E32 * (A.transpose(1, 2) @ dyd.abs())),
                          torch.bfloat16))
    return dsum, dmag


MFMA_CASES = {
    # benchmark shapes: D_s at B = 64 (512 frames of 16 x 16), D_t (768 frames of 8 x 8); the size-128 configuration
    "D_s_512x256": dict(F=512, N=256, C=128, regime="units", g=0.7, seed=11),
    "D_t_768x64_large": dict(F=768, N=64, C=128, regime="large", g=-0.6, seed=12),
    "D_s128_N1024_last": dict(F=8, N=1024, C=128, regime="last", g=0.8, seed=13),
    "D_t128_N256_onehot": dict(F=32, N=256, C=128, regime="onehot", g=1.1, seed=14),
    # edges
    "N32_one_block": dict(F=3, N=32, C=128, regime="units", g=0.5, seed=15),
    "N96_ragged_C64": dict(F=4, N=96, C=64, regime="large", g=0.9, seed=16),
    "N288_second_chunk_C32": dict(F=3, N=288, C=32, regime="last", g=-1.3, seed=17),
    "N4096_limit_one_frame": dict(F=1, N=4096, C=128, regime="last", g=0.7, seed=18),
    "ldq_padded_C64": dict(F=2, N=128, C=64, regime="onehot", g=0.6, seed=19, ldq=32 + 64 + 24),
    "gamma0": dict(F=4, N=256, C=128, regime="units", g=0.0, seed=20),
}


@pytest.mark.parametrize("case", list(MFMA_CASES))
def test_attention_mfma_vs_fp64(case):
    mfma_case(case, **MFMA_CASES[case])


# ------------------------------------------------------------------------------------------------ fp32 vector kernels
def run_f32(dtype, qb, kvb, x, dy, gamma, dq, koff, voff, C, F, N, Nk, self_attn, dgamma=None):
    ldq, ldk, ldx = qb.shape[-1], kvb.shape[-1], x.shape[-1]
    nan = float("nan")
    y, att = torch.full_like(x, nan), torch.full_like(x, nan)
    A = torch.full((F, N, Nk), nan, device=DEV)
    dS = torch.full((F, N, Nk), nan, device=DEV)
    dqo = torch.full_like(qb, nan)
    dkv = dqo if self_attn else torch.full_like(kvb, nan)
    L = lib()
    if self_attn:
        ok(L.dvd_attention_forward(dtype, P(qb), ldq, dq, koff, voff, P(x), ldx, C, P(gamma), P(y), P(att), P(A),
                                   ct.c_longlong(F), N, S()))
        ok(L.dvd_attention_backward(dtype, P(qb), ldq, dq, koff, voff, P(dy), ldx, C, P(gamma), P(att), P(A), P(dS), P(dqo),
                                    P(dgamma), ct.c_longlong(F), N, S()))
    else:
        ok(L.dvd_attention_kv_forward(dtype, P(qb), ldq, dq, P(kvb), ldk, koff, voff, P(x), ldx, C, P(gamma), P(y), P(att), P(A),
                                      ct.c_longlong(F), N, Nk, S()))
        ok(L.dvd_attention_kv_backward(dtype, P(qb), ldq, dq, P(kvb), ldk, koff, voff, P(dy), ldx, C, P(gamma), P(att), P(A),
                                       P(dS), P(dqo), P(dkv), P(dgamma), ct.c_longlong(F), N, Nk, S()))
    return y, att, A, dS, dqo, dkv


def f32_case(name, dtype, F, N, Nk, dq, C, ldx, regime, g, seed, self_attn=True):
    """dvd_attention_forward / backward (self) or dvd_attention_kv_* against fp64"""
    from dvd_gan_amd import lib as L
    dcode = L.dt(torch.empty(0, dtype=dtype))
    koff = (dq + 7) // 8 * 8
    voff = 2 * koff
    ldq = ldk = (voff + C + 7) // 8 * 8
    qb, kvb, x, dy = make_case(F, N, Nk, dq, koff, voff, C, ldq, ldk, ldx, dtype, regime, self_attn, seed)
    gamma = torch.tensor([g], device=DEV)
    args = (dcode, qb, kvb, x, dy, gamma, dq, koff, voff, C, F, N, Nk, self_attn)
    y, att, A, dS, dqo, dkv = run_f32(*args)                    # dgamma = null: dS stays whole (the partials live in it)
    dg0 = torch.tensor([0.375], device=DEV)
    dgamma, dgamma2 = dg0.clone(), dg0.clone()
    y2, att2, A2, dS2, dqo2, dkv2 = run_f32(*args, dgamma=dgamma)
    run_f32(*args, dgamma=dgamma2)
    for a, b, n in ((y, y2, "y"), (att, att2, "att"), (A, A2, "A"), (dqo, dqo2, "dq"), (dkv, dkv2, "dkv")):
        assert same_bits(a, b), f"{name}: rerun of {n} differs"
    nb = 256 if F * N * Nk >= 256 else 1                        # dgamma partials at the head of dS (attention_bwd)
    assert same_bits(dS.flatten()[nb:], dS2.flatten()[nb:]), name + ": rerun of dS differs"
    assert same_bits(dgamma, dgamma2), name + ": rerun of dgamma differs"
    C8 = (C + 7) // 8 * 8            # a ragged last 8-lane group is stored whole: zeros behind C; whole pad groups are not written
    assert bool(torch.isnan(y[..., C8:].float()).all() and torch.isnan(att[..., C8:].float()).all()), name + ": pad columns of y"
    assert bool((y[..., C:C8] == 0).all() and (att[..., C:C8] == 0).all()), name + ": pad lanes of the last channel group"
    if self_attn:
        check_columns(dqo, [(0, dq), (koff, dq), (voff, C)], name + " dqkv")
    else:
        check_columns(dqo, [(0, dq)], name + " dq_out")
        check_columns(dkv, [(koff, dq), (voff, C)], name + " dkv_out")
    if g == 0.0:
        assert same_bits(y[..., :C], x[..., :C]), name + ": y != x with gamma = 0"
    w = Worst(name)
    dsum, dmag = f32_bounds(w, dtype, F, N, Nk, dq, koff, voff, C, g, qb, kvb, x, dy, y, att, A, dS, dqo, dkv)
    w.add("dgamma", abs(float(dgamma) - (0.375 + dsum)) / (C_F32["dgamma"] * E32 * (dmag + 0.375)))
    w.check(C_F32)


def f32_bounds(w, dtype, F, N, Nk, dq, koff, voff, C, g, qb, kvb, x, dy, y, att, A, dS, dqo, dkv):
    """The elementwise checks of the fp32 attention kernels' outputs added to the Worst `w`: q at [0, dq) of qb [F, N, ldq], k | v
    at koff | voff of kvb [F, Nk, ldk]; x, dy, y, att [F, N, ldx]; A, dS [F, N, Nk]; dqo like qb, dkv like kvb (one buffer for self
    attention).  dS = None: not at hand (scratch of the autograd Function's backward), its check is left out.  Returns (sum, sum of
    magnitudes) of dy * att_out, the terms of dgamma."""
    dsum, dmag = 0.0, 0.0
    for f0, f1 in frame_chunks(F, N * Nk):
        q, k, v, s, m, lse_r, A_r, out, y_r = ref_forward(qb, kvb, x, g, dq, koff, voff, C, f0, f1)
        ms = math.sqrt(dq) * (q * q @ (k * k).transpose(1, 2)).sqrt() + (s - m).abs() + 1
        magA = A_r * (ms + (A_r * ms).sum(-1, keepdim=True))
        w.add("A", ratio(A[f0:f1], A_r, C_F32["A"] * E32 * magA + TINY, torch.float32))
        av = A_r @ v.abs()
        mag_out = magA @ v.abs() + math.sqrt(Nk) * av
        w.add("att", ratio(att[f0:f1, :, :C], out, C_F32["att"] * E32 * mag_out, dtype))
        w.add("y", ratio(y[f0:f1, :, :C], y_r, C_F32["y"] * E32 * (abs(g) * mag_out + (g * out).abs() + x[f0:f1, :, :C].double().abs()),
                         dtype))
        dyd = dy[f0:f1, :, :C].double()
        dA = g * dyd @ v.transpose(1, 2)
        Dp = (A_r * dA).sum(-1, keepdim=True)
        dS_r = A_r * (dA - Dp)
        mag_dS = magA * (dA - Dp).abs() + A_r * (math.sqrt(C) * abs(g) * (dyd.abs() @ v.abs().transpose(1, 2))
                                                  + math.sqrt(Nk) * (A_r * dA.abs()).sum(-1, keepdim=True)
                                                  + (magA * dA.abs()).sum(-1, keepdim=True))
        if dS is not None:
            w.add("dS", ratio(dS[f0:f1], dS_r, C_F32["dS"] * E32 * mag_dS + TINY * ((dA - Dp).abs() + 1), torch.float32))
        dq_r, dk_r, dv_r = dS_r @ k, dS_r.transpose(1, 2) @ q, g * A_r.transpose(1, 2) @ dyd
        aS = dS_r.abs()
        w.add("dq", ratio(dqo[f0:f1, :, :dq], dq_r, C_F32["dq"] * E32 * (mag_dS @ k.abs() + math.sqrt(Nk) * (aS @ k.abs())), dtype))
        w.add("dk", ratio(dkv[f0:f1, :, koff:koff + dq], dk_r, C_F32["dk"] * E32 * (mag_dS.transpose(1, 2) @ q.abs()
                                                                                    + math.sqrt(N) * (aS.transpose(1, 2) @ q.abs())), dtype))
        w.add("dv", ratio(dkv[f0:f1, :, voff:voff + C], dv_r, C_F32["dv"] * E32 * abs(g) * (magA.transpose(1, 2) @ dyd.abs()
                                                                                            + math.sqrt(N) * (A_r.transpose(1, 2) @ dyd.abs())), dtype))
        terms = dyd * att[f0:f1, :, :C].double()
        dsum += float(terms.sum())
        dmag += float(terms.abs().sum())
    return dsum, dmag


F32, BF16 = torch.float32, torch.bfloat16
F32_CASES = {
    # exact mode (--dtype f32) at the discriminators' benchmark shapes
    "exact_D_s_512x256": dict(dtype=F32, F=512, N=256, Nk=256, dq=16, C=128, ldx=128, regime="units", g=0.7, seed=31),
    "exact_D_t_768x64_large": dict(dtype=F32, F=768, N=64, Nk=64, dq=16, C=128, ldx=128, regime="large", g=-0.6, seed=32),
    # ch = 16 in bf16 mode: dq = 8, C = 64 (the MFMA kernels refuse it)
    "bf16_dq8_C64": dict(dtype=BF16, F=8, N=256, Nk=256, dq=8, C=64, ldx=64, regime="units", g=0.9, seed=33),
    # QB = 8 from N = 1024 (16 rows of scores do not fit)
    "qb8_N1024_f32": dict(dtype=F32, F=2, N=1024, Nk=1024, dq=16, C=128, ldx=128, regime="last", g=0.8, seed=34),
    "qb8_N1024_bf16": dict(dtype=BF16, F=2, N=1024, Nk=1024, dq=16, C=128, ldx=128, regime="large", g=0.8, seed=35),
    # the largest N the forward accepts at dq = 8, C = 64 (QB = 8: 8 N + 8 dqp + 32 C <= 16384 floats)
    "largest_N1784": dict(dtype=F32, F=1, N=1784, Nk=1784, dq=8, C=64, ldx=64, regime="onehot", g=0.5, seed=36),
    # N not a multiple of QB, C < ldx, nearly one-hot rows, negative gamma
    "N100_C56_ldx64_f32": dict(dtype=F32, F=3, N=100, Nk=100, dq=8, C=56, ldx=64, regime="onehot", g=-0.7, seed=37),
    "N100_C56_ldx64_bf16": dict(dtype=BF16, F=3, N=100, Nk=100, dq=8, C=56, ldx=64, regime="onehot", g=-0.7, seed=38),
    # frames * N * Nk < 256: one dgamma partial; gamma = 0
    "one_partial_gamma0_f32": dict(dtype=F32, F=1, N=8, Nk=8, dq=8, C=16, ldx=16, regime="units", g=0.0, seed=39),
    "one_partial_gamma0_bf16": dict(dtype=BF16, F=3, N=8, Nk=8, dq=8, C=16, ldx=16, regime="units", g=0.0, seed=40),
    "one_partial_f32": dict(dtype=F32, F=2, N=8, Nk=8, dq=8, C=16, ldx=16, regime="large", g=1.2, seed=41),
    # C no multiple of 8 (the forward takes any C <= ldx, the backward must too): the last 8-lane group of v and dy is ragged
    "ragged_C20_ldx24_f32": dict(dtype=F32, F=3, N=16, Nk=16, dq=2, C=20, ldx=24, regime="units", g=0.7, seed=42),
    "ragged_C20_ldx24_bf16": dict(dtype=BF16, F=3, N=40, Nk=40, dq=2, C=20, ldx=24, regime="onehot", g=-0.8, seed=43),
}


@pytest.mark.parametrize("case", list(F32_CASES))
def test_attention_fp32_kernels_vs_fp64(case):
    f32_case(case, **F32_CASES[case])


KV_CASES = {
    # the generator's 3-D self attention at the benchmark (64 clips of 48 x 4 x 4 latents: 768 queries, 96 pooled keys)
    "gen_768x96_f32": dict(dtype=F32, F=64, N=768, Nk=96, dq=128, C=256, ldx=256, regime="units", g=0.6, seed=51),
    "gen_768x96_bf16": dict(dtype=BF16, F=64, N=768, Nk=96, dq=128, C=256, ldx=256, regime="large", g=-0.9, seed=52),
    # the size-128 geometry: 48 x 8 x 8 = 3072 queries, 384 keys (the column pass walks the queries in two LDS chunks)
    "gen128_3072x384_f32": dict(dtype=F32, F=2, N=3072, Nk=384, dq=128, C=256, ldx=256, regime="last", g=0.7, seed=53),
    "gen128_3072x384_bf16": dict(dtype=BF16, F=2, N=3072, Nk=384, dq=128, C=256, ldx=256, regime="onehot", g=0.7, seed=54),
    # C no multiple of 8 on the kv entry points
    "ragged_C20_ldx24_f32": dict(dtype=F32, F=2, N=32, Nk=4, dq=4, C=20, ldx=24, regime="units", g=0.7, seed=55),
    "ragged_C20_ldx24_bf16": dict(dtype=BF16, F=2, N=32, Nk=4, dq=4, C=20, ldx=24, regime="large", g=0.9, seed=56),
}


@pytest.mark.parametrize("case", list(KV_CASES))
def test_attention_kv_vs_fp64(case):
    f32_case(case, self_attn=False, **KV_CASES[case])


# ------------------------------------------------------------------------------------------------ separable attention cell
def sep_ref(qkv, x, dy, g, Cq, koff, voff, C, axis, b0, b1):
    """SeparableAttnCell (Attention.py:61-111) restated in fp64 on the stored operands, raw reshapes included; the max-pool takes
    the FIRST maximum of a tied pair (torch's max_pool3d, and sepattn.hip)."""
    B, T, W, H, _ = qkv.shape
    b = b1 - b0
    A = (T, W, H)[axis]
    swap = (lambda t: t) if axis == 0 else (lambda t: t.transpose(2, 3)) if axis == 1 else (lambda t: t.transpose(2, 4))
    ncdhw = lambda a, n: qkv[b0:b1, ..., a:a + n].double().permute(0, 4, 1, 2, 3)
    ql = ncdhw(0, Cq).clone().requires_grad_(True)
    kl = ncdhw(koff, Cq).clone().requires_grad_(True)
    vl = ncdhw(voff, C).clone().requires_grad_(True)

    def pool(t):
        t = swap(t).contiguous()
        a0, a1 = t[:, :, 0::2], t[:, :, 1::2]
        sel = a1 > a0
        return torch.where(sel, a1, a0), sel

    q = swap(ql).contiguous()
    Qf = q.view(b, A, -1)
    kp, ksel = pool(kl)
    vp, vsel = pool(vl)
    Kp = kp.contiguous().view(b, -1, A // 2)
    Vp = vp.contiguous().view(b, -1, A // 2)
    sc = Qf @ Kp
    att = torch.softmax(sc, -1)
    out = Vp @ att.transpose(2, 1)
    if axis == 0:
        o5 = out.view(b, C, W, H, T).permute(0, 1, 4, 2, 3)
    elif axis == 1:
        o5 = out.view(b, C, T, H, W).permute(0, 1, 2, 4, 3)
    else:
        o5 = out.view(b, C, T, W, H)
    outc = o5.permute(0, 2, 3, 4, 1)                           # channels-last [b, T, W, H, C]
    y = g * outc + x[b0:b1, ..., :C].double()
    dyd = dy[b0:b1, ..., :C].double()
    outc.backward(g * dyd)
    cl = lambda t: t.grad.permute(0, 2, 3, 4, 1)
    return dict(Qf=Qf.detach(), Kp=Kp.detach(), Vp=Vp.detach(), ksel=ksel, vsel=vsel, sc=sc.detach(), att=att.detach(),
                out=outc.detach(), y=y.detach(), dq=cl(ql), dk=cl(kl), dv=cl(vl), dgamma=(dyd * outc.detach()),
                VpA=(Vp.detach().abs() @ att.detach().transpose(2, 1)))


def run_sep(dtype, qkv, x, dy, gamma, Cq, koff, voff, C, B, T, W, H, axis, dgamma):
    from dvd_gan_amd import lib as L
    d = L.dt(x)
    N = T * W * H
    A = (T, W, H)[axis]
    f32 = lambda n: torch.full((n,), float("nan"), device=DEV)
    u8 = lambda n: torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    Qf, Kp, Vp = f32(B * Cq * N), f32(B * Cq * N // 2), f32(B * C * N // 2)
    ksel, vsel, att = u8(B * Cq * N // 2), u8(B * C * N // 2), f32(B * A * (A // 2))
    y = torch.full_like(x, float("nan"))
    ldq, ldx = qkv.shape[-1], x.shape[-1]
    ok(L.lib().dvd_sepattn_forward(d, P(qkv), ldq, Cq, koff, voff, P(x), ldx, C, P(gamma), P(y), P(Qf), P(Kp), P(Vp), P(ksel),
                                   P(vsel), P(att), ct.c_longlong(B), T, W, H, axis, S()))
    dO, dS = f32(B * C * N), f32(B * A * (A // 2))
    dQf, dKp, dVp = f32(B * Cq * N), f32(B * Cq * N // 2), f32(B * C * N // 2)
    dqkv = torch.full_like(qkv, float("nan"))
    ok(L.lib().dvd_sepattn_backward(d, P(dy), ldx, C, Cq, P(gamma), P(Qf), P(Kp), P(Vp), P(ksel), P(vsel), P(att), P(dO), P(dS),
                                    P(dQf), P(dKp), P(dVp), P(dqkv), ldq, koff, voff, P(dgamma), ct.c_longlong(B), T, W, H, axis,
                                    S()))
    return dict(y=y, Qf=Qf, Kp=Kp, Vp=Vp, ksel=ksel, vsel=vsel, att=att, dqkv=dqkv)


def sep_case(name, dtype, B, T, W, H, Cq, C, axis, g, seed, ties=False, bchunk=8):
    koff = (Cq + 7) // 8 * 8
    voff = 2 * koff
    ldq = (voff + C + 7) // 8 * 8
    N = T * W * H
    A = (T, W, H)[axis]
    qkv = randn((B, T, W, H, ldq), seed)
    qkv[..., :Cq] *= 3.0 / math.sqrt(Cq * N // A)             # scores of a few units whatever the row length L = Cq N / A
    if ties:                                                   # k and v on a grid of 1/4: many tied max-pool pairs
        qkv[..., koff:] = torch.round(qkv[..., koff:] * 4).clamp(-8, 8) / 4
    qkv = qkv.to(dtype).contiguous()
    x = randn((B, T, W, H, C), seed + 1).to(dtype).contiguous()
    dy = randn((B, T, W, H, C), seed + 2).to(dtype).contiguous()
    gamma = torch.tensor([g], device=DEV)
    dgamma, dgamma2 = torch.tensor([0.375], device=DEV), torch.tensor([0.375], device=DEV)
    got = run_sep(dtype, qkv, x, dy, gamma, Cq, koff, voff, C, B, T, W, H, axis, dgamma)
    again = run_sep(dtype, qkv, x, dy, gamma, Cq, koff, voff, C, B, T, W, H, axis, dgamma2)
    for k in got:
        assert same_bits(got[k], again[k]), f"{name}: rerun of {k} differs"
    assert same_bits(dgamma, dgamma2), name + ": rerun of dgamma differs"
    check_columns(got["dqkv"], [(0, Cq), (koff, Cq), (voff, C)], name + " dqkv")
    w = Worst(name)
    dsum, dmag, ntie_k, ntie_v = sep_bounds(w, name, dtype, B, T, W, H, Cq, koff, voff, C, axis, g, qkv, x, dy, got, bchunk)
    w.add("dgamma", abs(float(dgamma) - (0.375 + dsum)) / (C_SEP["dgamma"] * E32 * (dmag + 0.375)))
    if ties:
        note(f"{name} tied k pairs along T", ntie_k)
        note(f"{name} tied v pairs along T", ntie_v)
        assert ntie_k > 0 and ntie_v > 0, f"{name}: no tied max-pool pairs ({ntie_k} k, {ntie_v} v)"
    w.check(C_SEP)


def sep_bounds(w, name, dtype, B, T, W, H, Cq, koff, voff, C, axis, g, qkv, x, dy, got, bchunk=8):
    """The checks of the separable cell's outputs added to the Worst `w`.  got: y, Qf, Kp, Vp, ksel, vsel, att, dqkv as
    dvd_sepattn_forward / backward leave them (flat scratch buffers as the entry points take them).  Returns (sum, sum of magnitudes
    of the dgamma terms, tied k pairs, tied v pairs along T)."""
    N = T * W * H
    A = (T, W, H)[axis]
    L = Cq * N // A
    dsum, dmag, ntie_k, ntie_v = 0.0, 0.0, 0, 0
    for b0 in range(0, B, bchunk):
        b1 = min(B, b0 + bchunk)
        r = sep_ref(qkv, x, dy, g, Cq, koff, voff, C, axis, b0, b1)
        n = b1 - b0
        for k in ("Qf", "Kp", "Vp"):                            # copies of stored values: bit-equal
            per = got[k].numel() // B
            assert torch.equal(got[k][b0 * per:b1 * per].view(n, -1), r[k].float().reshape(n, -1)), f"{name}: {k}"
        for k in ("ksel", "vsel"):
            per = got[k].numel() // B
            assert torch.equal(got[k][b0 * per:b1 * per].view(n, -1).bool(), r[k].reshape(n, -1)), f"{name}: {k} (first maximum)"
        if axis == 0:                                           # tied pairs (t = 2 dp, 2 dp + 1) of the pooled k and v columns
            kk, vv = qkv[b0:b1, ..., koff:koff + Cq], qkv[b0:b1, ..., voff:voff + C]
            ntie_k += int((kk[:, 0::2] == kk[:, 1::2]).sum())
            ntie_v += int((vv[:, 0::2] == vv[:, 1::2]).sum())
        att = got["att"][b0 * A * (A // 2):b1 * A * (A // 2)].view(n, A, A // 2)
        # score error: the L-term products run in 64 sequential lanes per score -> sqrt(L / 64) * ||terms||_2
        ms = math.sqrt(max(1, L / 64)) * ((r["Qf"] ** 2) @ (r["Kp"] ** 2)).sqrt() + r["sc"].abs() + 1
        magA = r["att"] * (ms + (r["att"] * ms).sum(-1, keepdim=True))
        w.add("att", ratio(att, r["att"], C_SEP["att"] * E32 * magA, torch.float32))
        # y: out = Vp att^T (A/2 terms) -> the propagated att error plus the sum's own
        magO = (r["Vp"].abs() @ magA.transpose(2, 1)) + math.sqrt(A) * r["VpA"]
        if axis == 0:
            magO = magO.view(n, C, W, H, T).permute(0, 1, 4, 2, 3)
        elif axis == 1:
            magO = magO.view(n, C, T, H, W).permute(0, 1, 2, 4, 3)
        else:
            magO = magO.view(n, C, T, W, H)
        magO = magO.permute(0, 2, 3, 4, 1)
        w.add("y", ratio(got["y"][b0:b1], r["y"], C_SEP["y"] * E32 * (abs(g) * magO + r["y"].abs() + x[b0:b1].double().abs()), dtype))
        dq, tag = got["dqkv"][b0:b1], "" if dtype == torch.float32 else "_bf16"
        w.l2("dq" + tag, dq[..., :Cq], r["dq"])
        w.l2("dk" + tag, dq[..., koff:koff + Cq], r["dk"])
        w.l2("dv" + tag, dq[..., voff:voff + C], r["dv"])
        dsum += float(r["dgamma"].sum())
        dmag += float(r["dgamma"].abs().sum())
    return dsum, dmag, ntie_k, ntie_v


SEP_CASES = {
    # the generator's clip [B, 48, 32, 32, 128], Cq = 64 (NC = 2 Cq + C = 256: 16-position gather tiles), all three axes; one full B
    "gen_T_B64": dict(dtype=BF16, B=64, T=48, W=32, H=32, Cq=64, C=128, axis=0, g=0.7, seed=61),
    "gen_W_B4": dict(dtype=BF16, B=4, T=48, W=32, H=32, Cq=64, C=128, axis=1, g=-0.8, seed=62),
    "gen_H_B4_f32": dict(dtype=F32, B=4, T=48, W=32, H=32, Cq=64, C=128, axis=2, g=0.9, seed=63),
    # A = 64, the limit
    "A64_W": dict(dtype=BF16, B=2, T=48, W=64, H=64, Cq=64, C=128, axis=1, g=0.6, seed=64),
    # gather tile widths: NC = 128 -> 32 positions, NC = 512 -> 8 positions
    "tp32_T": dict(dtype=F32, B=2, T=16, W=8, H=8, Cq=32, C=64, axis=0, g=0.5, seed=65),
    "tp8_H": dict(dtype=BF16, B=2, T=8, W=8, H=16, Cq=128, C=256, axis=2, g=1.1, seed=66),
    # the byte-wise gather / scatter (Cq not a multiple of 8), tied max-pool pairs
    "bytewise_Cq12_ties": dict(dtype=BF16, B=2, T=12, W=8, H=6, Cq=12, C=24, axis=0, g=0.8, seed=67, ties=True),
    "ties_T_bf16": dict(dtype=BF16, B=2, T=16, W=8, H=8, Cq=32, C=64, axis=0, g=-0.9, seed=68, ties=True),
}


@pytest.mark.parametrize("case", list(SEP_CASES))
def test_sepattn_vs_fp64(case):
    sep_case(case, **SEP_CASES[case])

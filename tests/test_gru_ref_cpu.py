"""The ConvGRU checker's own test (tests/gru_ref.py), on the CPU: an emulation of the layer's forward and backward pass in
fp32 / bf16 -- an fp32 conv2d on storage-rounded operands and the kernels' rounding points as gru.hip and conv_common.h have them
(u stored from the unrounded sigmoid, r rounded BEFORE h * r, o rounded before the state update, the state update on the stored
u, the optional fp32 carry from step 1 on, d(hr) and the carry's convolution term from the STORED dg) -- is fed to gru_ref:

  * the emulation as written stays inside every bound, for both storage types, with and without h0, with and without the carry;
  * each emulated mutant (one per fault the loose rel-L2 bounds of the module tests let through) leaves the named check's bound.
"""
import pytest
import torch
import torch.nn.functional as F

import gru_ref as R

B, S, HID, K, T = 3, 8, 24, 3, 4


def _cl(x):          # NCHW -> channels-last
    return x.permute(0, 2, 3, 1).contiguous()


def _conv32(x_cl, w, transposed=False, drop_slab=False):
    """fp32 convolution of a channels-last tensor (storage values) with storage-rounded weights; drop_slab: the K dimension in
    three channel slabs, the last one left out."""
    x = x_cl.float().permute(0, 3, 1, 2)
    w = w.float()
    if transposed:
        return _cl(F.conv_transpose2d(x, w, padding=w.shape[-1] // 2))
    if drop_slab:
        c = x.shape[1] // 3
        return _cl(sum(F.conv2d(x[:, i * c:(i + 1) * c], w[:, i * c:(i + 1) * c], padding=w.shape[-1] // 2) for i in range(2)))
    return _cl(F.conv2d(x, w, padding=w.shape[-1] // 2))


def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _tanh(x, dtype, switch):
    if dtype == torch.float32:
        return torch.tanh(x)
    ax = x.abs()
    t = torch.exp(-2.0 * ax)
    return torch.copysign(torch.where(ax < switch, ax, (1.0 - t) / (1.0 + t)), x)


def _inputs(dtype, with_h0, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = lambda x: x.to(dtype)
    gx = q(torch.randn(T, B, S, S, 3 * HID, generator=g))
    w_ur = q(torch.randn(2 * HID, HID, K, K, generator=g) / (HID * K * K) ** 0.5)
    w_o = q(torch.randn(HID, HID, K, K, generator=g) / (HID * K * K) ** 0.5)
    h0 = q(torch.randn(B, S, S, HID, generator=g) * 0.5) if with_h0 else None
    dh_out = q(torch.randn(T, B, S, S, HID, generator=g))
    return gx, w_ur, w_o, h0, dh_out


def emulate_forward(dtype, gx, h0, w_ur, w_o, carry, mutant=None):
    st = lambda x: x.to(dtype)
    h_all, u_all, r_all, o_all, hr_all = [], [], [], [], []
    h32 = torch.full((2, B * S * S, HID), float("nan"))
    for t in range(T):
        hprev = h0 if t == 0 else h_all[-1]
        g = gx[t].float()
        pre = g[..., :2 * HID] + (_conv32(hprev, w_ur, drop_slab=mutant == "slab") if hprev is not None else 0.0)
        s = _sig(pre)
        u, r = st(s[..., :HID]), st(s[..., HID:])
        rmul = s[..., HID:] if mutant == "r_unrounded" else r.float()
        hr = st(hprev.float() * rmul) if hprev is not None else torch.zeros_like(r)
        pre_o = g[..., 2 * HID:] + (_conv32(hr, w_o) if hprev is not None else 0.0)
        o = st(_tanh(pre_o, dtype, 0.2 if mutant == "tanh_switch" else 2e-3))
        if carry and t > 0 and mutant != "carry_ignored":
            hp = h32[t & 1].view(B, S, S, HID)
        else:
            hp = hprev.float() if hprev is not None else torch.zeros(B, S, S, HID)
        hn = hp * (1.0 - u.float()) + o.float() * u.float()
        h32[(t + 1) & 1] = hn.reshape(-1, HID)
        for lst, v in ((h_all, st(hn)), (u_all, u), (r_all, r), (o_all, o), (hr_all, hr)):
            lst.append(v)
    out = [torch.stack(v) for v in (h_all, u_all, r_all, o_all, hr_all)]
    return out + [h32 if carry else None]


def emulate_backward(dtype, h0, h_all, u_all, r_all, o_all, dh_out, w_ur, w_o, mutant=None):
    st = lambda x: x.to(dtype)
    dg = torch.empty(T, B, S, S, 3 * HID, dtype=dtype)
    carry = torch.zeros(B, S, S, HID)
    for t in range(T - 1, -1, -1):
        hprev = h0 if t == 0 else h_all[t - 1]
        hp = hprev.float() if hprev is not None else torch.zeros_like(carry)
        u, r, o = u_all[t].float(), r_all[t].float(), o_all[t].float()
        dh = carry + dh_out[(t + 1) % T if mutant == "dh_step" else t].float()
        dg[t][..., 2 * HID:] = st(dh * u * ((1.0 - o) if mutant == "one_minus_o" else (1.0 - o * o)))
        hpu = h_all[t].float() if mutant == "hprev_step" else hp
        dg[t][..., :HID] = st(dh * (o - hpu) * u * (1.0 - u))
        carry = dh * (1.0 - u)
        if hprev is None:
            dg[t][..., HID:2 * HID] = 0
            continue
        dhr = _conv32(dg[t][..., 2 * HID:], w_o, transposed=True)
        carry = carry + dhr * r
        dg[t][..., HID:2 * HID] = st(dhr * hp * r * (1.0 - r))
        carry = carry + _conv32(dg[t][..., :2 * HID], w_ur, transposed=True)
    return dg, carry


def test_conv64_is_the_convolution_and_its_adjoint():
    g = torch.Generator().manual_seed(1)
    for k, (h, w) in ((3, (5, 7)), (5, (4, 4))):
        x = torch.randn(2, 6, h, w, generator=g, dtype=torch.float64, requires_grad=True)
        wt = torch.randn(10, 6, k, k, generator=g, dtype=torch.float64)
        y = F.conv2d(x, wt, padding=k // 2)
        gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(gy)
        assert torch.allclose(R.conv64(_cl(x.detach()), wt), _cl(y.detach()), rtol=1e-12, atol=1e-12)
        assert torch.allclose(R.convT64(_cl(gy), wt), _cl(x.grad), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("carry", [False, True], ids=["nocarry", "carry"])
@pytest.mark.parametrize("with_h0", [False, True], ids=["noh0", "h0"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_emulation_stays_inside_every_bound(dtype, with_h0, carry):
    gx, w_ur, w_o, h0, dh_out = _inputs(dtype, with_h0)
    h_all, u_all, r_all, o_all, hr_all, h32 = emulate_forward(dtype, gx, h0, w_ur, w_o, carry)
    fw = R.forward_ratios("emulation", dtype, gx, h0, h_all, u_all, r_all, o_all, hr_all, h32, w_ur, w_o)
    assert set(fw) == {"u", "r", "hr", "o", "h"} | ({"h32"} if carry else set())
    dg, cy = emulate_backward(dtype, h0, h_all, u_all, r_all, o_all, dh_out, w_ur, w_o)
    bw = R.backward_ratios("emulation", dtype, h0, h_all, u_all, r_all, o_all, dh_out, dg, cy, cy if with_h0 else None, w_ur, w_o)
    for k, v in {**fw, **bw}.items():
        assert v <= 1.0, (k, v)
    if dtype == torch.bfloat16:
        # the bounds are tight: the stored gates sit within a few percent of half an ulp
        assert min(fw["u"], fw["r"], fw["o"], fw["h"]) > 0.9, fw


FORWARD_MUTANTS = [("carry_ignored", "h"), ("r_unrounded", "hr"), ("tanh_switch", "o"), ("slab", "u")]
BACKWARD_MUTANTS = [("hprev_step", "dg_u"), ("one_minus_o", "dg_o"), ("dh_step", "dg_o")]


@pytest.mark.parametrize("mutant,check", FORWARD_MUTANTS, ids=[m for m, _ in FORWARD_MUTANTS])
def test_emulated_forward_mutant_leaves_its_bound(mutant, check):
    dtype = torch.bfloat16
    gx, w_ur, w_o, h0, _ = _inputs(dtype, True)
    h_all, u_all, r_all, o_all, hr_all, h32 = emulate_forward(dtype, gx, h0, w_ur, w_o, True, mutant)
    fw = R.forward_ratios(mutant, dtype, gx, h0, h_all, u_all, r_all, o_all, hr_all, h32, w_ur, w_o)
    assert fw[check] > 1.0, fw


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mutant,check", BACKWARD_MUTANTS, ids=[m for m, _ in BACKWARD_MUTANTS])
def test_emulated_backward_mutant_leaves_its_bound(mutant, check, dtype):
    gx, w_ur, w_o, h0, dh_out = _inputs(dtype, True)
    h_all, u_all, r_all, o_all, hr_all, _ = emulate_forward(dtype, gx, h0, w_ur, w_o, False)
    dg, cy = emulate_backward(dtype, h0, h_all, u_all, r_all, o_all, dh_out, w_ur, w_o, mutant)
    bw = R.backward_ratios(mutant, dtype, h0, h_all, u_all, r_all, o_all, dh_out, dg, cy, cy, w_ur, w_o)
    assert bw[check] > 1.0, bw

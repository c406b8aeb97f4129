"""The weight-gradient reference's own test (tests/conv_ref.py), on the CPU: against float64 autograd of F.conv2d / F.conv3d on
random inputs for every option it has, and its ConvGRU gate composition against autograd of ONE convolution per gate over the
concatenated [x_t | h_{t-1}] input.  Both sides are float64 and differ in summation order only: 1e-12 rel-L2."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

TOL = 1e-12


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def _nc(t):          # channels-last -> channels-first
    return t.movedim(-1, 1).contiguous()


CASES = [
    # frames, Cin, Cout, spatial, ksize, up2, relu_in
    (3, 5, 7, (6, 6), (3, 3), False, False),
    (2, 4, 6, (5, 9), (3, 3), False, True),          # H != W, odd extents
    (2, 6, 3, (8, 4), (5, 5), False, False),         # 5 x 5, the filter wider than half the frame
    (2, 3, 5, (4, 6), (3, 3), True, False),          # nearest x2 upsample, H != W
    (3, 4, 4, (3, 5), (3, 3), True, True),           # ReLU, then the upsample
    (2, 5, 4, (4, 4), (5, 5), True, True),
    (2, 8, 8, (7, 3), (1, 1), False, True),          # 1 x 1
    (2, 3, 4, (4, 5, 6), (3, 3, 3), False, False),   # 3-D
    (1, 4, 3, (3, 6, 4), (3, 3, 3), False, True),
    (2, 4, 5, (2, 4, 4), (1, 1, 1), False, False),
    (2, 3, 4, (5, 4, 4), (3, 1, 1), False, False),   # temporal taps only
]


@pytest.mark.parametrize("case", CASES)
def test_reference_equals_fp64_autograd(case):
    F_, cin, cout, sp, ks, up2, relu_in = case
    g = torch.Generator().manual_seed(sum(sp) * 131 + cin * 17 + cout)
    x = torch.randn(F_, *sp, cin, generator=g, dtype=torch.float64)
    osp = tuple(sp[:-2]) + tuple(v * (2 if up2 else 1) for v in sp[-2:])
    dy = torch.randn(F_, *osp, cout, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, *ks, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    xin = _nc(x)
    if relu_in:
        xin = F.relu(xin)
    if up2:
        xin = F.interpolate(xin, scale_factor=2)
    conv = F.conv3d if len(ks) == 3 else F.conv2d
    y = conv(xin, w, b, padding=[k // 2 for k in ks])
    y.backward(_nc(dy))
    dw, db = R.wgrad_ref(x, dy, ks, up2=up2, relu_in=relu_in, chunk=2)      # (chunk 2: the frame loop takes part)
    assert dw.shape == w.shape and dw.dtype == torch.float64
    assert rel(dw, w.grad) < TOL
    assert rel(db, b.grad) < TOL


def test_reference_reads_storage_dtypes():
    """bf16 / fp32 operands are taken at their stored values."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 6, 8, generator=g).to(torch.bfloat16)
    dy = torch.randn(2, 6, 6, 8, generator=g).to(torch.bfloat16)
    a = R.wgrad_ref(x, dy, (3, 3))
    b = R.wgrad_ref(x.double(), dy.double(), (3, 3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("with_h0", [True, False])
@pytest.mark.parametrize("shared_x", [False, True])
@pytest.mark.parametrize("shape", [(3, 2, 5, 4, 6, 3), (2, 3, 4, 3, 5, 5), (1, 2, 4, 4, 4, 3)])
def test_gate_composition_equals_one_convolution_over_the_concatenated_input(shape, shared_x, with_h0):
    """Gate gradient [hid][cin + hid][k][k] = x-part over all T*B frames + h0-part on step 0 + h-part on steps 1..T-1, against
    autograd of conv2d(cat(x_t, h_{t-1}))  (update / reset)  and  conv2d(cat(x_t, h_{t-1} * r_t))  (out gate); without an initial
    state step 0 reads zeros.  shared_x: one input for every step, the x-part sees the gradient summed over T."""
    T, B, S, cin, hid, k = shape
    g = torch.Generator().manual_seed(T * 100 + B * 10 + k)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rn(B if shared_x else T * B, S, S, cin)
    dg, h_all, hr_all = rn(T * B, S, S, 3 * hid), rn(T * B, S, S, hid), rn(T * B, S, S, hid)
    h0 = rn(B, S, S, hid) if with_h0 else None
    dgx = dg.view(T, B, S, S, 3 * hid).sum(0) if shared_x else dg
    got = R.gru_gate_wgrad_ref(x, dgx, dg, h_all, hr_all, h0, T, B, hid, k)
    zero = torch.zeros(B, S, S, hid, dtype=torch.float64)
    xs = x.repeat(T, 1, 1, 1) if shared_x else x
    for gate in range(3):
        if gate < 2:
            hprev = torch.cat([h0 if with_h0 else zero, h_all[:(T - 1) * B]])
        else:
            hprev = hr_all if with_h0 else torch.cat([zero, hr_all[B:]])
        w = rn(hid, cin + hid, k, k).requires_grad_(True)
        b = torch.zeros(hid, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(_nc(torch.cat([xs, hprev], dim=-1)), w, b, padding=k // 2)
        y.backward(_nc(dg[..., gate * hid:(gate + 1) * hid]))
        assert rel(got[gate][0], w.grad) < TOL
        assert rel(got[gate][1], b.grad) < TOL

"""The weight-gradient reference's own test (tests/conv_ref.py), on the CPU: against float64 autograd of F.conv2d / F.conv3d on
random inputs for every option it has, and its ConvGRU gate composition against autograd of ONE convolution per gate over the
concatenated [x_t | h_{t-1}] input.  Both sides are float64 and differ in summation order only: 1e-12 rel-L2.

The forward reference and its checker (forward_ref, check_forward) likewise: forward_ref against F.conv2d / F.conv3d /
F.interpolate / 4 F.avg_pool2d composed the plain way in float64 (1e-12); an honest fp32 implementation in torch's own CPU ops on
the stored operands must pass check_forward with ratio <= 1 at the small shapes of tests/test_gpu_conv_epilogue.py (the bound is
derived, so it has to admit another summation order); and every wrong output of WRONG, built in torch from the same operands,
must make check_forward raise."""
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


# ------------------------------------------------------------------ forward_ref / check_forward
def _cl(t):          # channels-first -> channels-last
    return t.movedim(1, -1).contiguous()


FWD_CASES = [
    # frames, Cin, Cout, spatial (of x), ksize, options
    (3, 5, 7, (6, 6), (3, 3), dict()),
    (2, 4, 6, (5, 9), (3, 3), dict(bias=True, relu_in=True)),
    (2, 6, 3, (8, 4), (5, 5), dict(bias=True, res=True)),
    (2, 3, 5, (4, 6), (3, 3), dict(up2=True, bias=True, res=True, act=R.ACT_RELU)),
    (3, 4, 4, (3, 5), (3, 3), dict(up2=True, relu_in=True, res=True, res_up2=True, act=R.ACT_TANH, mask=True)),
    (2, 5, 9, (4, 4), (5, 5), dict(bias=True, res=True, res_up2=True, act=R.ACT_SIGMOID, mask=True)),
    (2, 8, 8, (7, 3), (1, 1), dict(res=True, mask=True)),
    (2, 5, 4, (6, 8), (3, 3), dict(pool2=True, mask=True)),
    (2, 3, 11, (4, 4), (5, 5), dict(pool2=True, bias=True)),
    (2, 3, 4, (4, 5, 6), (3, 3, 3), dict(bias=True, res=True, act=R.ACT_TANH, mask=True)),     # 3-D
    (1, 4, 3, (3, 6, 4), (3, 1, 1), dict(relu_in=True, bias=True, res=True, res_up2=True)),   # temporal taps only
]


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_reference_equals_plain_fp64_torch(case):
    """forward_ref against F.conv2d / F.conv3d / F.interpolate / 4 F.avg_pool2d composed the plain way in float64, for every option."""
    F_, cin, cout, sp, ks, o = case
    g = torch.Generator().manual_seed(sum(sp) * 131 + cin * 17 + cout)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    d3 = len(sp) == 3
    x = rn(F_, *sp, R.pad8(cin))                      # the channels from Cin on are ignored
    w = rn(cout, cin, *ks)
    osp = tuple(sp[:-2]) + tuple(v * (2 if o.get("up2") else 1) // (2 if o.get("pool2") else 1) for v in sp[-2:])
    rsp = tuple(osp[:-2]) + tuple(v // (2 if o.get("res_up2") else 1) for v in osp[-2:])
    bias = rn(cout) if o.get("bias") else None
    res = rn(F_, *rsp, cout + 3) if o.get("res") else None            # wider than Cout: the extra columns are ignored
    mask = rn(F_, *osp, cout + 5) if o.get("mask") else None
    act = o.get("act", R.ACT_NONE)
    ref, bound, keep = R.forward_ref(x, w, bias=bias, res=res, res_up2=bool(o.get("res_up2")), act=act, mask=mask,
                                     up2=bool(o.get("up2")), relu_in=bool(o.get("relu_in")), pool2=bool(o.get("pool2")))
    xin = _nc(x[..., :cin])
    if o.get("relu_in"):
        xin = F.relu(xin)
    if o.get("up2"):
        xin = F.interpolate(xin, scale_factor=(1, 2, 2) if d3 else 2)
    y = (F.conv3d if d3 else F.conv2d)(xin, w, None, padding=[k // 2 for k in ks])
    if o.get("pool2"):
        y = 4.0 * F.avg_pool2d(y, 2)
        if bias is not None:
            y = y + 4.0 * bias.view(1, -1, 1, 1)
    else:
        if bias is not None:
            y = y + bias.view(1, -1, *([1] * len(sp)))
        if res is not None:
            r = _nc(res[..., :cout])
            y = y + (F.interpolate(r, scale_factor=(1, 2, 2) if d3 else 2) if o.get("res_up2") else r)
    y = {R.ACT_NONE: lambda t: t, R.ACT_RELU: F.relu, R.ACT_TANH: torch.tanh, R.ACT_SIGMOID: torch.sigmoid}[act](y)
    y = _cl(y)
    if mask is not None:
        y = y * (mask[..., :cout] > 0)
    assert ref.shape == (F_, *osp, R.pad8(cout)) and ref.dtype == bound.dtype == torch.float64 and keep.dtype == torch.bool
    assert rel(ref[..., :cout], y) < TOL
    assert not bool(ref[..., cout:].any()) and not bool(bound[..., cout:].any()) and not bool(keep[..., cout:].any())
    assert torch.equal(keep[..., :cout], mask[..., :cout] > 0) if mask is not None else bool(keep[..., :cout].all())
    assert bool((bound[keep] > 0).all()) and not bool(bound[~keep].any()) and not bool(ref[~keep].any())


# ---- an honest fp32 implementation, and wrong ones, in torch on the stored operands
SMALL = {    # the small shapes of tests/test_gpu_conv_epilogue.py: frames, S, Cin, Cout, k, up2, relu_in
    "halo128": (2, 16, 64, 72, 3, False, False),
    "halo128-up2": (2, 16, 64, 128, 3, True, True),
    "frame8": (5, 8, 64, 72, 3, False, False),
    "frame4": (13, 4, 40, 72, 5, False, False),
    "thin-in": (3, 32, 3, 64, 3, False, False),
    "thin-out": (3, 32, 64, 3, 3, False, False),
    "tap": (2, 12, 24, 40, 3, False, False),
}


def _rows_of(res, F_, H, W, res_up2, mutate):
    """The residual row every output pixel reads, by its FLAT index as a kernel forms it -> [F, H, W, ld]"""
    f, y, xx = torch.meshgrid(torch.arange(F_), torch.arange(H), torch.arange(W), indexing="ij")
    if res_up2:
        yy = (y + 1) >> 1 if mutate == "res_up2_row_rounded_up" else y >> 1
        ff = torch.where(y == H - 1, f + 1, f) if mutate == "res_up2_next_frame_at_last_row" else f
        row = (ff * (H // 2) + yy) * (W // 2) + (xx >> 1)
    else:
        row = (f * H + (y + 1 if mutate == "res_one_row_lower" else y)) * W + xx
    flat = res.reshape(-1, res.shape[-1])
    return flat[row % flat.shape[0]]


def _impl32(rq, dtype, mutate=None, zero_x=False):
    """The request in torch's own fp32 CPU ops (another summation order than any kernel's) -> fp32 [.., pad8(Cout)]."""
    o, w = rq["req"], rq["w"].float()
    cout, cin = w.shape[:2]
    act = R.zero_pass_act(o["act"]) if zero_x else o["act"]
    xin = _nc(rq["x"][..., :cin].float())
    if zero_x:
        xin = torch.zeros_like(xin)
    if o["relu_in"]:
        xin = F.relu(xin)
    if o["up2"]:
        xin = F.interpolate(xin, scale_factor=2)
    y = _cl(F.conv2d(xin, w, None, padding=w.shape[-1] // 2))
    bias = o.get("bias")
    if bias is not None and mutate == "bias_shifted_8_channels":
        bias = bias.roll(8)
    fn = {R.ACT_NONE: lambda t: t, R.ACT_RELU: F.relu, R.ACT_TANH: torch.tanh, R.ACT_SIGMOID: torch.sigmoid}[act]
    if o["pool2"]:
        y = _cl(4.0 * F.avg_pool2d(_nc(y), 2))
        if bias is not None:
            y = y + (bias if mutate == "pool2_bias_added_once" else 4.0 * bias)
    else:
        if bias is not None:
            y = y + bias
        r = None
        if o.get("res") is not None:
            r = _rows_of(o["res"], *y.shape[:3], o["res_up2"], mutate)[..., :cout].float()
        if mutate == "activation_before_residual":
            y = fn(y) + r
        else:
            y = fn(y + r if r is not None else y)
    if o.get("mask") is not None:
        m = o["mask"][..., :cout]
        y = torch.where((m >= 0) if mutate == "mask_rule_ge" else (m > 0), y, torch.zeros_like(y))
    return F.pad(y, (0, R.pad8(cout) - cout))


def _buffers(rq, dtype, mutate=None):
    """(out32, out_st, zero32): [.., pad8(Cout) + 8] buffers prefilled with the sentinel byte, written as a kernel would."""
    def wide(v, dt):
        cp = v.shape[-1]
        n = v[..., 0].numel() * (cp + 8) * torch.empty((), dtype=dt).element_size()
        buf = torch.full((n,), R.SENT, dtype=torch.uint8).view(dt).view(*v.shape[:-1], cp + 8)
        buf[..., :cp] = v.to(dt)
        return buf
    o32 = _impl32(rq, dtype, mutate)
    return wide(o32, torch.float32), wide(o32.to(dtype), dtype), wide(_impl32(rq, dtype, mutate, zero_x=True), torch.float32)


def _check(name, rq, dtype, bufs, **kw):
    return R.check_forward(name, dtype, rq["x"], rq["w"], bufs[0], bufs[1], zero32=bufs[2], **kw, **rq["req"])


ADMIT = [(c, k) for c in SMALL for k in R.KINDS
         if not (c.startswith("thin") and k in ("res", "res_up2", "sigmoid", "pool2", "pool2_bias"))
         and not (k.startswith("pool2") and SMALL[c][1] < 16)
         and not (k in ("bwd", "pool2", "pool2_bias") and SMALL[c][5])]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case,kind", ADMIT)
def test_bound_admits_an_honest_fp32_implementation(case, kind, dtype):
    """torch's fp32 CPU convolution, pooling and activations on the stored operands pass check_forward with ratio <= 1: the bound is
    derived, so an honest fp32 result in another summation order must fit it."""
    rq = R.make_request(SMALL[case], kind, dtype, "cpu", 7, with_res=not case.startswith("thin"))
    r = _check(f"cpu-fp32 {case} {kind} {'bf16' if dtype == torch.bfloat16 else 'fp32'}", rq, dtype, _buffers(rq, dtype))
    assert r <= 1.0


WRONG = [   # mutant, (case, kind) it is built on
    ("res_one_row_lower", "halo128", "res"),
    ("res_one_row_lower", "halo128", "bwd"),
    ("res_up2_row_rounded_up", "halo128", "res_up2"),
    ("res_up2_next_frame_at_last_row", "halo128-up2", "res_up2"),
    ("bias_shifted_8_channels", "halo128", "res"),
    ("bias_shifted_8_channels", "thin-in", "relu"),
    ("mask_rule_ge", "frame8", "relu"),
    ("mask_rule_ge", "halo128", "pool2"),
    ("activation_before_residual", "frame4", "tanh"),
    ("activation_before_residual", "tap", "relu"),
    ("pool2_bias_added_once", "halo128", "pool2_bias"),
    ("nonzero_pad_channel", "thin-out", "tanh"),
    ("sentinel_column_overwritten", "halo128", "res"),
    ("storage_two_ulps_off", "halo128", "sigmoid"),
    ("gap_written", "halo128", "res"),
]


@pytest.mark.parametrize("mutant,case,kind", WRONG)
def test_checker_rejects_wrong_outputs(mutant, case, kind):
    """Every wrong output, built in torch from the same operands, makes check_forward raise (and the unmutated one passes)."""
    dtype = torch.bfloat16
    rq = R.make_request(SMALL[case], kind, dtype, "cpu", 11, with_res=not case.startswith("thin"))
    _check(f"{case} {kind} honest", rq, dtype, _buffers(rq, dtype))
    bufs, kw = _buffers(rq, dtype, mutate=mutant), {}
    cout = rq["w"].shape[0]
    at = (1, 2, 3)
    if mutant == "nonzero_pad_channel":
        assert cout % 8
        for b in bufs:
            b[at][cout] = 2.0 ** -20
    elif mutant == "sentinel_column_overwritten":
        bufs[0][at][R.pad8(cout) + 5] = 0.0
    elif mutant == "storage_two_ulps_off":
        v = bufs[1][at][:cout]
        c = int(v.abs().argmax())                    # (a kept element: nonzero)
        assert float(v[c]) != 0.0
        bufs[1][at].view(torch.int16)[c] += 2
    elif mutant == "gap_written":
        kw["gaps_intact"] = False
    with pytest.raises(AssertionError, match="check [1-4]"):
        _check(f"{case} {kind} {mutant}", rq, dtype, bufs, **kw)

"""tests/fn_ref.py checked on the CPU: its float64 statements agree with torch.nn.functional (batch_norm + affine, avg_pool2d / 3d,
max_pool3d with a planted tie, an explicit attention, embedding + linear) and with the float64 forward / backward formulas of
tests/test_gpu_attention.py, pass torch.autograd.gradcheck at tiny shapes, and the row permutations invert each other."""
import pytest
import torch
import torch.nn.functional as F

import autograd_ref as AR
import conv_ref
import fn_ref as FR
import test_gpu_attention as TA

D = torch.float64


def rn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D)


def close(a, b, tol=1e-12):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) <= tol * (1 + float(b.abs().max()))


# ------------------------------------------------------------------ conditional batch norm
@pytest.mark.parametrize("relu", [False, True])
def test_cbn_is_batch_norm_plus_affine(relu):
    Fr, C, ld, B = 6, 5, 8, 3
    x, gb, dy = rn(1, Fr, 4, 4, ld).requires_grad_(True), rn(2, B, 2 * C).requires_grad_(True), rn(3, Fr, 4, 4, ld)
    samp = torch.tensor([2, 0, 1, 1, 2, 0], dtype=torch.int32)
    y = FR.cbn(x, gb, samp, C, relu)
    assert y.shape == x.shape and bool((y[..., C:] == 0).all())
    dx, dgb = FR.grads(y, (x, gb), dy)
    x2, gb2 = FR.leaf(x), FR.leaf(gb)
    xh = F.batch_norm(x2[..., :C].permute(0, 3, 1, 2), None, None, training=True, eps=1e-5).permute(0, 2, 3, 1)
    g = gb2[samp.long()]
    want = g[:, None, None, :C] * xh + g[:, None, None, C:]
    want = F.relu(want) if relu else want
    wdx, wdgb = FR.grads(want, (x2, gb2), dy[..., :C])
    assert close(y[..., :C], want) and close(dx, wdx) and close(dgb, wdgb)
    assert bool((dx[..., C:] == 0).all())


def test_cbn_eval_uses_the_running_buffers():
    Fr, C, ld = 4, 3, 8
    x, gb = rn(4, Fr, 2, 2, ld), rn(5, 2, 2 * C)
    samp = torch.tensor([1, 0, 0, 1], dtype=torch.int32)
    rm, rv = rn(6, C).float(), rn(7, C).abs().float() + 0.5
    y = FR.cbn(x, gb, samp, C, False, training=False, run_mean=rm, run_var=rv)
    xh = F.batch_norm(x[..., :C].permute(0, 3, 1, 2), rm.double(), rv.double(), training=False, eps=1e-5).permute(0, 2, 3, 1)
    g = gb[samp.long()]
    assert close(y[..., :C], g[:, None, None, :C] * xh + g[:, None, None, C:])


def test_cbn_replicas_are_the_repeated_batch():
    """world = 2 on identical data: y and dx of replica 0 are those of the single-replica batch (same mean and variance; the backward
    sums and the row count both double); dgb is ONE replica's, not the sum over both."""
    Fr, C, ld, B = 6, 4, 8, 3
    x, gb, dy = rn(8, Fr, 2, 2, ld), rn(9, B, 2 * C), rn(10, Fr, 2, 2, ld)
    samp = (torch.arange(Fr) % B).int()
    x1, g1 = FR.leaf(x), FR.leaf(gb)
    dx1, dgb1 = FR.grads(FR.cbn(x1, g1, samp, C, True), (x1, g1), dy)
    x2, g2 = FR.leaf(x), FR.leaf(gb)
    y2 = FR.cbn(x2, g2, samp, C, True, world=2)
    assert y2.shape[0] == 2 * Fr and close(y2[:Fr], y2[Fr:])
    dx2, dgb2 = FR.grads(y2, (x2, g2), dy.repeat(2, 1, 1, 1))
    assert close(dx2, dx1) and close(dgb2, dgb1)


def test_cbn_gradcheck():
    x, gb = rn(11, 4, 2, 2, 8).requires_grad_(True), rn(12, 2, 6).requires_grad_(True)
    samp = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    assert torch.autograd.gradcheck(lambda a, b: FR.cbn(a, b, samp, 3, False), (x, gb))


# ------------------------------------------------------------------ pooling
def test_pool_is_avg_pool_with_floor():
    x = rn(13, 2, 5, 7, 8).requires_grad_(True)
    y = FR.pool(x, 1)
    assert close(y, F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    dx, = FR.grads(y, (x,), rn(14, *y.shape))
    assert bool((dx[:, 4] == 0).all() and (dx[:, :, 6] == 0).all())       # the odd last line and column
    x3 = rn(15, 2, 4, 5, 6, 8).requires_grad_(True)
    assert close(FR.pool(x3, 2), F.avg_pool3d(x3.permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1))
    assert close(FR.pool(x3, 1), F.avg_pool3d(x3.permute(0, 4, 1, 2, 3), (1, 2, 2)).permute(0, 2, 3, 4, 1))
    assert torch.autograd.gradcheck(lambda a: FR.pool(a, 2), (rn(16, 1, 2, 3, 2, 2).requires_grad_(True),))


def test_maxpool3d_routes_to_the_first_maximum():
    x = rn(17, 2, 4, 4, 6, 3)
    win = FR.maxpool3d_windows(x)
    assert torch.equal(win[1, 1, 0, 2, 1], x[1, 2:4, 0:2, 4:6, 1].reshape(8))           # (t, h, w) scan order
    x[0, 0:2, 0:2, 0:2, 0] = 0.25
    x[0, 1, 1, 0, 0] = x[0, 1, 1, 1, 0] = 3.0          # a planted tie at scan positions 6 and 7 ...
    x[1, 0:2, 2:4, 2:4, 2] = -1.0                        # ... and an all-equal window: position 0 wins
    x.requires_grad_(True)
    dy = rn(18, 2, 2, 2, 3, 3)
    y = FR.maxpool3d(x)
    dx, = FR.grads(y, (x,), dy)
    x2 = FR.leaf(x)
    want = F.max_pool3d(x2.permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1)
    wdx, = FR.grads(want, (x2,), dy)
    assert torch.equal(y, want) and torch.equal(dx, wdx)
    assert dx[0, 1, 1, 0, 0] == dy[0, 0, 0, 0, 0] and dx[0, 1, 1, 1, 0] == 0
    assert dx[1, 0, 2, 2, 2] == dy[1, 0, 1, 1, 2] and int((dx[1, 0:2, 2:4, 2:4, 2] != 0).sum()) == 1
    assert int((dx != 0).sum()) == dy.numel()


# ------------------------------------------------------------------ attention
@pytest.mark.parametrize("self_attn", [True, False])
def test_attention_is_the_float64_statement_of_the_kernel_tests(self_attn):
    """against an explicit softmax attention, and against ref_forward / the documented backward of tests/test_gpu_attention.py"""
    Fr, N, Nk, dq, C, g = 2, 6, 6 if self_attn else 3, 3, 5, 0.7
    koff, voff = 8, 16
    ld = voff + 8
    qkv, x, dy = rn(19, Fr, N, ld).requires_grad_(True), rn(20, Fr, N, 8).requires_grad_(True), rn(21, Fr, N, 8)
    kv = qkv if self_attn else rn(22, Fr, Nk, ld).requires_grad_(True)
    gamma = torch.tensor([g], dtype=D, requires_grad=True)
    y = FR.attention(qkv, kv, x, gamma, dq, C)
    q, k, v, s, m, lse, A, out, y_r = TA.ref_forward(qkv.detach(), kv.detach(), x.detach(), g, dq, koff, voff, C, 0, Fr)
    assert close(y, y_r)
    want = g * torch.stack([sum(torch.exp(q[f, :, None] @ k[f].t()[None])[:, 0, j:j + 1] * v[f, j] for j in range(Nk))
                            / torch.exp(q[f] @ k[f].t()).sum(-1, keepdim=True) for f in range(Fr)]) + x.detach()[..., :C]
    assert close(y, want, 1e-10)
    ins = (qkv, x, gamma) if self_attn else (qkv, kv, x, gamma)
    got = FR.grads(y, ins, dy[..., :C])
    dyd = dy[..., :C]
    dA = g * dyd @ v.transpose(1, 2)
    dS = A * (dA - (A * dA).sum(-1, keepdim=True))
    dq_r, dk_r, dv_r = dS @ k, dS.transpose(1, 2) @ q, g * A.transpose(1, 2) @ dyd
    dqkv, dkv = got[0], got[0] if self_attn else got[1]
    if self_attn:
        assert close(dqkv[..., :dq], dq_r) and close(dqkv[..., koff:koff + dq], dk_r) and close(dqkv[..., voff:voff + C], dv_r)
        keep = torch.zeros(ld, dtype=torch.bool)
        keep[:dq] = keep[koff:koff + dq] = keep[voff:voff + C] = True
        assert bool((dqkv[..., ~keep] == 0).all())
    else:
        assert close(dqkv[..., :dq], dq_r) and bool((dqkv[..., dq:] == 0).all())
        assert close(dkv[..., koff:koff + dq], dk_r) and close(dkv[..., voff:voff + C], dv_r) and bool((dkv[..., :koff] == 0).all())
    assert close(got[-2][..., :C], dyd) and bool((got[-2][..., C:] == 0).all())          # dx is dy
    assert close(got[-1], (dyd * out).sum().reshape(1))                                 # dgamma


def test_attention_gradcheck():
    qkv, x = rn(23, 1, 4, 24).requires_grad_(True), rn(24, 1, 4, 8).requires_grad_(True)
    kv = rn(25, 1, 2, 24).requires_grad_(True)
    gamma = torch.tensor([0.7], dtype=D, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b, c: FR.attention(a, a, b, c, 2, 4), (qkv, x, gamma))
    assert torch.autograd.gradcheck(lambda a, k, b, c: FR.attention(a, k, b, c, 2, 4), (qkv, kv, x, gamma))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_sep_cell_is_sep_ref(axis):
    B, T, W, H, dq, C, g = 2, 4, 2, 6, 3, 5, 0.8
    qkv, x, dy = rn(26 + axis, B, T, W, H, 24), rn(30, B, T, W, H, 8), rn(31, B, T, W, H, 8)
    r = TA.sep_ref(qkv, x, dy, g, dq, 8, 16, C, axis, 0, B)
    ql, xl, gl = FR.leaf(qkv), FR.leaf(x), torch.tensor([g], dtype=D, requires_grad=True)
    y = FR.sep_cell(ql, xl, gl, dq, C, axis)
    dqkv, dx, dgamma = FR.grads(y, (ql, xl, gl), dy[..., :C])
    assert close(y, r["y"])
    assert close(dqkv[..., :dq], r["dq"]) and close(dqkv[..., 8:8 + dq], r["dk"]) and close(dqkv[..., 16:16 + C], r["dv"])
    assert close(dgamma, r["dgamma"].sum().reshape(1)) and close(dx[..., :C], dy[..., :C])
    small = rn(32, 1, 2, 2, 2, 24).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: FR.sep_cell(a, xl[:1, :2, :2, :2], gl, 2, 3, axis), (small,))


# ------------------------------------------------------------------ projection head, fused projection
def test_proj_head_is_linear_plus_embedding():
    Fr, C, ld, ncls = 6, 5, 8, 4
    feat, wl, b, we, dout = rn(33, Fr, 2, 2, ld), rn(34, 1, C), rn(35, 1), rn(36, ncls, C), rn(37, Fr)
    cls = torch.tensor([0, 2, 2, 3, 0, 2], dtype=torch.int32)                        # class 1 is never named
    u_l, u_e = rn(38, 1).float(), rn(39, ncls).float()
    s_l, u1_l, v1_l = FR.power_iter(wl, u_l / u_l.norm())
    s_e, u1_e, v1_e = FR.power_iter(we, u_e / u_e.norm())
    assert close(s_e, u1_e @ we @ v1_e) and close(v1_l.norm(), torch.tensor(1.0, dtype=D))
    r = FR.proj_head_grads(feat, wl, b, we, cls, (u1_l, v1_l, s_l), (u1_e, v1_e, s_e), dout, C)
    f2, wl2, b2, we2 = FR.leaf(feat), FR.leaf(wl), FR.leaf(b), FR.leaf(we)
    h = F.relu(f2[..., :C]).sum((1, 2))
    sn = lambda w, u, v: w / (u.detach() @ w @ v.detach())                             # u, v constants, sigma a function of w
    out = F.linear(h, sn(wl2, u1_l, v1_l), b2)[:, 0] + (F.embedding(cls.long(), sn(we2, u1_e, v1_e)) * h).sum(1)
    df, dwl, db, dwe = FR.grads(out, (f2, wl2, b2, we2), dout)
    assert close(r["out"], out) and close(r["dfeat"], df) and bool((r["dfeat"][..., C:] == 0).all())
    assert close(r["dw_lin"][0], dwl, 1e-10) and close(r["dw_emb"][0], dwe, 1e-10) and close(r["db"], db)
    assert bool((r["G_emb"][1] == 0).all())
    assert torch.autograd.gradcheck(lambda a, w, c, e: FR.proj_head(a, w, c, e, cls, C), (rn(40, Fr, 1, 2, ld).requires_grad_(True) + 3,
                                                                                          FR.leaf(wl), FR.leaf(b), FR.leaf(we)))


def test_qkv_conv_is_three_convolutions_with_gaps():
    Fr, C, dq, dqp = 2, 8, 3, 8
    x, dy = rn(41, Fr, 3, 3, C), rn(42, Fr, 3, 3, 2 * dqp + C)
    ws = [rn(43 + i, n, C, 1, 1).requires_grad_(True) for i, n in enumerate((dq, dq, C))]
    bs = [rn(46 + i, n).requires_grad_(True) for i, n in enumerate((dq, dq, C))]
    xl = FR.leaf(x)
    qkv = FR.qkv_conv(xl, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], dq, dqp)
    for (w, b, off, n) in ((ws[0], bs[0], 0, dq), (ws[1], bs[1], dqp, dq), (ws[2], bs[2], 2 * dqp, C)):
        assert close(qkv[..., off:off + n], F.conv2d(x.permute(0, 3, 1, 2), w.detach(), b.detach()).permute(0, 2, 3, 1))
    assert bool((qkv[..., dq:dqp] == 0).all() and (qkv[..., dqp + dq:2 * dqp] == 0).all())
    zero = FR.qkv_conv(torch.zeros_like(x), *[t for p in zip(ws, bs) for t in p], dq, dqp)
    assert torch.equal(zero[0, 0, 0], FR.qkv_bias(*bs, dq, dqp).detach())
    # the forms the GPU test takes its bounds from: conv_ref.forward_ref / wgrad_ref on the fused weight, dy_col = the part's offset
    wf = FR.qkv_weight(*ws, dq, dqp).detach()
    ref, _, _ = conv_ref.forward_ref(x, wf, bias=FR.qkv_bias(*bs, dq, dqp).detach())
    assert close(qkv, ref)
    got = FR.grads(qkv, (xl, *ws, *bs), dy)
    dxr, _, _ = conv_ref.forward_ref(dy, AR._w_bwd(wf))
    assert close(got[0], dxr[..., :C])
    for i, (off, n) in enumerate(((0, dq), (dqp, dq), (2 * dqp, C))):
        dw, db = conv_ref.wgrad_ref(x, dy[..., off:off + n], (1, 1))
        assert close(got[1 + i], dw) and close(got[4 + i], db)
    assert torch.autograd.gradcheck(lambda a, w: FR.qkv_conv(a, w, bs[0], ws[1], bs[1], ws[2], bs[2], dq, dqp), (xl, ws[0]))


# ------------------------------------------------------------------ permutations
@pytest.mark.parametrize("A,B", [(3, 5), (5, 3), (2, 7)])
def test_permutations_invert_each_other(A, B):
    x = rn(50, A * B, 2, 8)
    y = FR.swap_frames(x, A, B)
    assert torch.equal(y.view(B, A, 2, 8), x.view(A, B, 2, 8).transpose(0, 1))         # out[b * A + a] = x[a * B + b]
    assert not torch.equal(y, x) and torch.equal(FR.swap_frames(y, B, A), x)
    assert not torch.equal(FR.swap_frames(y, A, B), x)                                  # the forward permutation is NOT its inverse
    idx = FR.swap_index(A, B)
    assert sorted(idx.tolist()) == list(range(A * B)) and torch.equal(idx[FR.swap_index(B, A)], torch.arange(A * B))
    img = rn(51, A * B, 5, 2, 3).float()
    for dtype in (torch.float32, torch.bfloat16):
        t = FR.to_cl(img, dtype, (A, B))
        assert t.shape == (A * B, 2, 3, 8) and t.dtype == dtype and bool((t[..., 5:] == 0).all())
        assert torch.equal(t[1 * A + (A - 1), ..., :5], img[(A - 1) * B + 1].permute(1, 2, 0).to(dtype))
        assert torch.equal(FR.from_cl(t, 5, (A, B)), img.to(dtype).float())
        assert torch.equal(FR.from_cl(FR.to_cl(img, dtype), 5), img.to(dtype).float())
        # the adjoint pair: <to_cl(x), g> = <x, from_cl(g)> -- to_cl's backward is from_cl with the same swap
        g = rn(52, A * B, 2, 3, 8).float()
        assert abs(float((FR.to_cl(img, torch.float32, (A, B))[..., :5] * g[..., :5]).sum() - (img * FR.from_cl(g, 5, (A, B))).sum())) < 1e-3

"""The autograd Functions of functional.py other than Conv -- CondBatchNorm, Pool, MaxPool3d, SelfAttention2d, SelfAttentionKV,
SeparableAttnCellFn, ProjectionHead, the layout Functions with a swap -- and disc_nets.QKVConv, through `.apply` as their modules call
them: real leaf nn.Parameters, operands drawn in the storage type (bf16 and fp32) from fixed seeds, the backward pass run by the
autograd engine.  The kernels have their own element-wise tests; this file pins the GLUE: which buffer is zero-filled, which route a
parameter gradient takes (returned, or added into a persistent .grad), which permutation / mask / replica count the backward gets.

References: tests/fn_ref.py (float64 torch.autograd on the stored operands) and, for the attention kernels, the float64 statements
of tests/test_gpu_attention.py, which tests/test_fn_ref_cpu.py holds equal to fn_ref's.  BOUNDS: none is new.  Each output is held to
what the kernel-level test of the same kernel holds it to -- C_MFMA / C_F32 / C_SEP and mfma_bounds / f32_bounds / sep_bounds of
test_gpu_attention.py; DX_TOL, check_stats, cbn_apply_check, check_dgb, check_bound of test_gpu_pointwise.py (and its literal 1e-6 of
sum |terms| for the fp32 linear / head kernels, 2e-7 for the statistics, 4 pt E sum |window| for the pool); autograd_ref.check /
conv_backward_ref / sn_backward_ref for the convolution and spectral-norm parts.  Where a reference is taken one stage earlier than
the kernel test takes it (float64 statistics instead of the stored ones, the float64 dgb instead of the stored one) the earlier
stage's own bound is pushed through the later stage's linear map in absolute value and added.  Selections, copies and permutations
are torch.equal.  Where autograd adds two tensors in the storage type the addends are checked separately and the sum bit for bit.

empty_like versus zeros_like: a fresh allocation is often zero by accident.  `poison` fills blocks of the sizes the backward is
about to allocate with NaN and frees them again, so that the caching allocator hands exactly those blocks out.

profiles/autograd_fn_numbers.md has the paths, the ratios and the glue mutants this file was run against.
"""
import contextlib
import math

import pytest
import torch
import torch.nn as nn

import autograd_ref as AR
import conv_ref as R
import fn_ref as FR
import gru_ref
import test_gpu_attention as TA
import test_gpu_pointwise as TP
from test_gpu_mfma16 import _variants
from test_gpu_sn_helpers import SN_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAMES = {BF: "bf16", F32: "fp32"}
DTYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
E32 = TP.E32
POISON = R.POISON
STATS_REL, TERMS, DGB = TP.STATS_TOL, TP.TERMS_TOL, TP.DGB_TOL      # bn_stats; fp32 linear / head sums; dgb (test_gpu_pointwise)
SN_REL = SN_TOL           # u, v, W / sigma after one power iteration (test_gpu_sn_helpers)
note, bits = gru_ref.note, gru_ref.bits


def rn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


@contextlib.contextmanager
def route(direct):
    """the side-stream / direct-accumulation route switched as the Trainer switches it, restored and joined afterwards"""
    from dvd_gan_amd import functional as Fn
    prev = Fn._SIDE["on"]
    Fn.direct_weight_grads(direct)
    try:
        yield
    finally:
        Fn.direct_weight_grads(prev)
        Fn.join_side()
        torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _autograd_route_unless_a_test_switches():
    with route(False):
        yield


def poison(*like):
    """see the module docstring"""
    torch.cuda.synchronize()
    blocks = [torch.full_like(t, float("nan")) for t in like for _ in range(2)]
    torch.cuda.synchronize()
    del blocks


def window(t, dtype, seed):
    """t [.., ld] handed over as a non-contiguous channel window of a wider buffer whose other columns hold finite poison"""
    wide = rn(seed, *t.shape[:-1], t.shape[-1] + 16) * POISON
    wide[..., 8:8 + t.shape[-1]] = t.float()
    w = wide.to(dtype)[..., 8:8 + t.shape[-1]]
    assert not w.is_contiguous() and torch.equal(w, t.to(dtype))
    return w


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def equal(a, b):
    """torch.equal with shape and dtype: value for value (the float64 one-hot routing writes -0 where the kernels write +0)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def rel_l2(a, b):
    a, b = a.detach(), b.detach()
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def entry_check(name, out, ref, bound, keep=None, dtype=None):
    keep = torch.ones_like(ref, dtype=torch.bool) if keep is None else keep
    return AR.check(name, out, None, dtype=dtype, entry=(ref, bound, keep))


# ================================================================== CondBatchNorm
class CBN:
    """Operands of one CondBatchNorm case: 6 frames of 4 x 4, 3 condition rows, gb = LinearF32(cond, W, b) as ConditionalNorm.forward
    builds it."""
    Fr, B, S, NC = 6, 3, 4, 10

    def __init__(self, dtype, C, order, relu, seed=300):
        self.dtype, self.C, self.relu, self.ld = dtype, C, relu, R.pad8(C)
        self.x0 = (rn(seed, self.Fr, self.S, self.S, self.ld) + 0.3).to(dtype)        # pad lanes: finite garbage
        self.cond = rn(seed + 1, self.B, self.NC)
        self.W = nn.Parameter(rn(seed + 2, 2 * C, self.NC) * 0.3)
        self.b = nn.Parameter(torch.cat([torch.ones(C, device=DEV), torch.zeros(C, device=DEV)]) + 0.1 * rn(seed + 3, 2 * C))
        s = [0, 1, 2, 0, 1, 2] if order == "t-major" else [2, 0, 1, 1, 2, 0]
        self.samp = torch.tensor(s, dtype=torch.int32, device=DEV)
        self.P = self.S * self.S
        self.dy = None

    def forward(self, *, training=True, replicas=None, tok=None, slot=None, rm=None, rv=None):
        from dvd_gan_amd import functional as Fn
        from dvd_gan_amd import lib as L
        C = self.C
        self.x = self.x0.clone().requires_grad_(True)
        self.gb = Fn.LinearF32.apply(self.cond, self.W, self.b)
        self.rm = torch.zeros(C, device=DEV) if rm is None else rm
        self.rv = torch.ones(C, device=DEV) if rv is None else rv
        self.sums = torch.zeros(L.BN_NREP * 2 * C, dtype=torch.float64, device=DEV)
        self.y = Fn.CondBatchNorm.apply(self.x, self.gb, self.samp, C, self.relu, training, self.rm, self.rv, 1e-5, 0.1, replicas,
                                        self.sums, tok, slot)
        _, _, _, self.mean, self.rstd = self.y.grad_fn.saved_tensors
        if self.dy is None:                     # drawn once per case; ambiguous ReLU masks carry no gradient (test_gpu_pointwise)
            g = TP.mask_ambiguous(rn(311, self.Fr, self.P, self.ld), self.x0.view(self.Fr, self.P, self.ld), C, self.mean, self.rstd,
                                  self.gb.detach(), self.samp, self.relu)
            self.dy = window(g.view_as(self.x0), self.dtype, 312)
        return self.y

    def reference(self, world=1):
        """float64 autograd through LinearF32 and cbn -> y, dx, dgb, dW, db.  The CBN node's operand is the STORED gb: the float64
        linear layer is shifted onto it by a constant, so the node is differentiated at the values it was given and the gradient
        still flows on to W and b."""
        x, W, b = FR.leaf(self.x0), FR.leaf(self.W), FR.leaf(self.b)
        gb = self.cond.double() @ W.t() + b
        gb = gb + (self.gb.detach().double() - gb).detach()
        y = FR.cbn(x, gb, self.samp, self.C, self.relu, world=world)
        dy = torch.cat([self.dy.double()] * world)
        dx, dgb, dW, db = FR.grads(y, (x, gb, W, b), dy)
        return y.detach()[:self.Fr], dx, dgb, dW, db

    def y_bound(self, mean_rel, rstd_rel, gb_exact):
        """|y - float64 statement| elementwise: cbn_apply's own 3 E (|gamma xhat| + |beta|) (test_gpu_pointwise.cbn_apply_check), plus
        what the stages in front of it may be off by, pushed through the affine map in absolute value: mean and rstd within
        mean_rel / rstd_rel relative (check_stats: 2e-7), gb within 1e-6 of the linear layer's sum |terms| (unless the statement is
        given the stored gb).  |relu(a) - relu(b)| <= |a - b|: the same bound holds behind the ReLU."""
        C = self.C
        g = self.gb.detach().double()[self.samp.long()]
        gam, bet = g[:, None, None, :C], g[:, None, None, C:]
        mu, rs = self.mean.double(), self.rstd.double()
        xh = (self.x0[..., :C].double() - mu) * rs
        bound = 3 * E32 * ((gam * xh).abs() + bet.abs()) + 1.01 * gam.abs() * (rstd_rel * xh.abs() + mean_rel * mu.abs() * rs)
        if not gb_exact:
            egb = TERMS * (self.cond.double().abs() @ self.W.detach().double().abs().t() + self.b.detach().double().abs())
            eg = egb[self.samp.long()]
            bound = bound + 1.01 * (eg[:, None, None, :C] * xh.abs() + eg[:, None, None, C:])
        return torch.nn.functional.pad(bound, (0, self.ld - C))

    def check_forward(self, name, ref_y):
        C, v = self.C, lambda t: t.view(self.Fr, self.P, self.ld)
        assert bool((self.sums == 0).all()), f"{name}: the persistent sums workspace is not left zeroed"
        TP.check_stats(self.mean, self.rstd, self.x0.view(-1, self.ld), C, 1e-5, name + " bn_stats")
        TP.cbn_apply_check(v(self.y.detach()), v(self.x0), C, self.mean, self.rstd, self.gb.detach(), self.samp, self.relu, self.dtype,
                           name + " cbn_apply")              # (asserts the pad lanes of y are 0, as include/dvdgan_hip.h promises)
        live = torch.ones_like(ref_y, dtype=torch.bool)
        live[..., C:] = False
        return entry_check(name + " y vs fp64", self.y.detach(), ref_y, self.y_bound(STATS_REL, STATS_REL, True), live)

    def check_backward(self, name, dx, dgb, ref_dx, ref_dgb):
        C, v = self.C, lambda t: t.reshape(self.Fr, self.P, self.ld)
        assert dx.dtype == self.dtype and dx.shape == self.x0.shape and dx.is_contiguous()
        gbd = self.gb.detach()
        kref, mag, s1, s2 = TP.cbn_backward_ref(v(self.dy), v(self.x0), C, self.mean, self.rstd, gbd, self.samp, self.relu, self.B)
        TP.check_dgb(dgb, kref, mag, self.samp, self.B, name)
        e = TP.dx_rel_l2(v(dx), v(self.dy), v(self.x0), C, self.mean, self.rstd, gbd, self.samp, self.relu, s1, s2, self.Fr * self.P)
        note(name + " dx rel-L2 (stored statistics)", e)
        assert e <= TP.DX_TOL[self.dtype], e
        e = rel_l2(dx[..., :C], ref_dx[..., :C])
        note(name + " dx rel-L2 (fp64 autograd)", e)
        assert e <= TP.DX_TOL[self.dtype], e
        assert bool((dx[..., C:] == 0).all()), f"{name}: pad channels of dx"
        e = float(((dgb.double() - ref_dgb).abs() / mag.clamp_min(1e-300)).max())
        note(name + " dgb err / sum|terms| (fp64 autograd)", e)
        assert e <= DGB, e
        return mag

    def embed_bounds(self, mag, ref_dgb, pw=None, pb=None):
        """LinearF32's backward on an incoming dgb that is itself within DGB * mag: both terms through |cond|"""
        c = self.cond.double().abs()
        bw = TERMS * (ref_dgb.abs().t() @ c + (0 if pw is None else pw.double().abs())) + DGB * (mag.t() @ c)
        bb = TERMS * (ref_dgb.abs().sum(0) + (0 if pb is None else pb.double().abs())) + DGB * mag.sum(0)
        return bw, bb


CBN_CASES = [(C, order, relu) for C in (24, 20) for order in ("t-major", "shuffled") for relu in (True, False)]


@DTYPES
@pytest.mark.parametrize("C,order,relu", CBN_CASES, ids=[f"C{c}-{o}-{'relu' if r else 'lin'}" for c, o, r in CBN_CASES])
def test_cond_batch_norm(C, order, relu, dtype):
    """y, dx, dgb and the embed gradients on the autograd and on the direct route; dy arrives as a channel window of a poisoned buffer."""
    cs = CBN(dtype, C, order, relu)
    name = f"cbn C={C} {order} relu={relu} {NAMES[dtype]}"
    dxs = []
    for direct in (False, True):
        label = f"{name} {'direct' if direct else 'autograd'}"
        cs.W.grad = cs.b.grad = None
        with route(direct):
            y = cs.forward()
            if not direct:
                ref_y, ref_dx, ref_dgb, ref_dW, ref_db = cs.reference()
                cs.check_forward(label, ref_y)
                g = torch.Generator(device=DEV).manual_seed(99)
                pw = torch.randn(ref_dW.shape, generator=g, device=DEV) * ref_dW.abs().mean().float()
                pb = torch.randn(ref_db.shape, generator=g, device=DEV) * ref_db.abs().mean().float()
            else:
                cs.W.grad, cs.b.grad = pw.clone(), pb.clone()
            poison(cs.x0, cs.gb)
            dx, dgb, dW, db = torch.autograd.grad([y], [cs.x, cs.gb, cs.W, cs.b], [cs.dy], allow_unused=True)
        assert bool((cs.sums == 0).all())
        mag = cs.check_backward(label, dx, dgb, ref_dx, ref_dgb)
        if direct:
            assert dW is None and db is None, f"{label}: the direct route returns no embed gradients"
            bw, bb = cs.embed_bounds(mag, ref_dgb, pw, pb)
            entry_check(label + " embed dW (.grad - prefill)", cs.W.grad.double() - pw.double(), ref_dW, bw, dtype=F32)
            entry_check(label + " embed db (.grad - prefill)", cs.b.grad.double() - pb.double(), ref_db, bb, dtype=F32)
        else:
            assert cs.W.grad is None and cs.b.grad is None
            bw, bb = cs.embed_bounds(mag, ref_dgb)
            entry_check(label + " embed dW", dW, ref_dW, bw)
            entry_check(label + " embed db", db, ref_db, bb)
        dxs.append((dx, dgb))
    assert same(dxs[0][0], dxs[1][0]) and same(dxs[0][1], dxs[1][1]), f"{name}: dx / dgb bits depend on the route"


@DTYPES
def test_cond_batch_norm_eval(dtype):
    """eval mode: the running buffers are read and left unchanged; backward raises the documented RuntimeError"""
    cs = CBN(dtype, 20, "shuffled", True)
    rm, rv = rn(320, 20) * 0.2 + 0.3, torch.rand(20, generator=torch.Generator(device=DEV).manual_seed(321), device=DEV) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    cs.dy = cs.x0                                               # (never used: backward raises)
    y = cs.forward(training=False, rm=rm, rv=rv)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and torch.equal(cs.mean, rm0)
    v = lambda t: t.view(cs.Fr, cs.P, cs.ld)
    TP.cbn_apply_check(v(y.detach()), v(cs.x0), 20, cs.mean, cs.rstd, cs.gb.detach(), cs.samp, True, dtype, f"cbn eval {NAMES[dtype]}")
    ref = FR.cbn(cs.x0.double(), cs.gb.detach().double(), cs.samp, 20, True, training=False, run_mean=rm0, run_var=rv0)
    live = torch.ones_like(ref, dtype=torch.bool)
    live[..., 20:] = False
    # mean is the running mean itself; rstd within 1e-6 of 1 / sqrt(running var + eps) (test_bn_stats_running_buffers_eval_and_workspace)
    entry_check(f"cbn eval {NAMES[dtype]} y vs fp64 on the running buffers", y.detach(), ref, cs.y_bound(0.0, TP.RSTD_EVAL_TOL, True), live)
    with pytest.raises(RuntimeError, match="training mode only"):
        torch.autograd.grad([y], [cs.x], [cs.x0])
    torch.cuda.synchronize()


@DTYPES
def test_cond_batch_norm_replicas(dtype):
    """replicas=(2, t -> 2 t): two replicas with identical data.  y and dx pass the single-replica checks, dgb stays per replica,
    and the all-reduce ran exactly twice: on the fp64 statistics sums of the forward and on the fp32 s12 of the BACKWARD."""
    from dvd_gan_amd import lib as L
    cs = CBN(dtype, 20, "shuffled", True)
    calls = []

    def all_reduce(t):
        calls.append((t.dtype, t.numel()))
        t.mul_(2)

    name = f"cbn replicas {NAMES[dtype]}"
    y = cs.forward(replicas=(2, all_reduce))
    ref_y, ref_dx, ref_dgb, _, _ = cs.reference(world=2)
    cs.check_forward(name, ref_y)
    dx, dgb = torch.autograd.grad([y], [cs.x, cs.gb], [cs.dy])
    torch.cuda.synchronize()
    cs.check_backward(name, dx, dgb, ref_dx, ref_dgb)
    assert calls == [(torch.float64, L.BN_NREP * 2 * 20), (torch.float32, 2 * 20)], calls
    # the same bits as the single-replica run would be too much to ask (n and the sums double: other roundings); the same checks hold
    one = CBN(dtype, 20, "shuffled", True)
    y1 = one.forward()
    dx1, dgb1 = torch.autograd.grad([y1], [one.x, one.gb], [cs.dy])
    assert same(dgb, dgb1), f"{name}: dgb is per replica"
    assert rel_l2(dx, dx1) <= TP.DX_TOL[dtype] and rel_l2(y, y1) <= TP.DX_TOL[dtype]


@DTYPES
def test_cond_batch_norm_slot(dtype):
    """slot / tok (GradSlot): the node leaves its dx in the slot, stamped with the running graph task, and x gets no gradient from it"""
    from dvd_gan_amd import functional as Fn
    cs = CBN(dtype, 24, "t-major", True)
    y = cs.forward()
    dx_plain, dgb_plain = torch.autograd.grad([y], [cs.x, cs.gb], [cs.dy])
    slot, tok, tasks = Fn.GradSlot(), torch.empty(0, device=DEV, dtype=dtype, requires_grad=True), []
    y = cs.forward(tok=tok, slot=slot)
    y.register_hook(lambda g: tasks.append(torch._C._current_graph_task_id()))
    dx, dgb, dtok = torch.autograd.grad([y], [cs.x, cs.gb, tok], [cs.dy], allow_unused=True)
    torch.cuda.synchronize()
    assert dx is None and dtok is None, "x must not receive a gradient from this node"
    assert slot.dx is not None and same(slot.dx, dx_plain) and same(dgb, dgb_plain)
    assert len(tasks) == 1 and tasks[0] >= 0 and slot.task == tasks[0]
    # a slot without a token is not armed (ConditionalNorm passes both or neither)
    slot2 = Fn.GradSlot()
    y = cs.forward(tok=None, slot=slot2)
    dx2, = torch.autograd.grad([y], [cs.x], [cs.dy])
    assert slot2.dx is None and slot2.task == -1 and same(dx2, dx_plain)


# ================================================================== Pool / MaxPool3d
@DTYPES
@pytest.mark.parametrize("case", ["2d-5x7", "3d-T4"])
def test_pool(case, dtype):
    from dvd_gan_amd import functional as Fn
    pt, shape = (1, (3, 5, 7, 24)) if case == "2d-5x7" else (2, (2, 4, 6, 4, 24))
    x = rn(400, *shape).to(dtype).requires_grad_(True)
    y = Fn.Pool.apply(x, pt)
    xl = FR.leaf(x)
    ref = FR.pool(xl, pt)
    dy = window(rn(401, *ref.shape).to(dtype), dtype, 402)
    poison(x)
    dx, = torch.autograd.grad([y], [x], [dy])
    torch.cuda.synchronize()
    win, sc = FR.pool(xl.detach().abs(), pt) * (4 * pt), 1.0 / (4 * pt)             # sum |window|, the average's scale
    r = TP.check_bound(y.detach(), ref.detach(), 4 * pt * E32 * win * sc, dtype, f"pool {case}")
    note(f"pool {case} {NAMES[dtype]} y err/bound", r)
    ref_dx, = FR.grads(ref, (xl,), dy)
    assert same(dx, ref_dx.to(dtype)), f"pool {case}: dx is dy / {4 * pt} replicated (a power of two: exact), zero in the floored tail"
    if pt == 1:
        assert bool((dx[:, 4] == 0).all() and (dx[:, :, 6] == 0).all())


@DTYPES
def test_pool_and_maxpool_refuse_what_they_cannot_differentiate(dtype):
    from dvd_gan_amd import functional as Fn
    with pytest.raises(ValueError, match=r"\(2, 5, 4, 4, 8\)"):
        Fn.Pool.apply(torch.zeros(2, 5, 4, 4, 8, device=DEV, dtype=dtype, requires_grad=True), 2)
    with pytest.raises(ValueError, match=r"\(2, 4, 4, 8\)"):
        Fn.Pool.apply(torch.zeros(2, 4, 4, 8, device=DEV, dtype=dtype, requires_grad=True), 2)
    for shape in ((2, 3, 4, 4, 8), (2, 2, 5, 4, 8), (2, 2, 4, 7, 8)):
        with pytest.raises(ValueError, match=str(shape).replace("(", r"\(").replace(")", r"\)")):
            Fn.MaxPool3d.apply(torch.zeros(*shape, device=DEV, dtype=dtype, requires_grad=True))
    assert Fn.Pool.apply(torch.zeros(2, 5, 7, 8, device=DEV, dtype=dtype), 1).shape == (2, 2, 3, 8)      # odd H, W floor as before


def tied_input(dtype, F_, T, H, W, C, seed):
    """[F, T, H, W, C] whose every third 2 x 2 x 2 window holds its maximum twice (at two scan positions that vary)"""
    win = rn(seed, F_, T // 2, H // 2, W // 2, C, 8).to(dtype)
    flat = win.view(-1, 8)
    idx = torch.arange(0, flat.shape[0], 3, device=DEV)
    p1 = idx % 7
    p2 = p1 + 1 + (idx // 7) % (7 - p1)
    top = flat[idx].float().amax(-1) + 1
    flat[idx, p1] = top.to(dtype)
    flat[idx, p2] = top.to(dtype)
    x = win.view(F_, T // 2, H // 2, W // 2, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(F_, T, H, W, C).contiguous()
    w2 = FR.maxpool3d_windows(x).reshape(-1, 8)
    assert torch.equal(w2, flat) and int(((w2 == w2.amax(-1, keepdim=True)).sum(-1) >= 2).sum()) >= idx.numel()
    return x


@DTYPES
def test_maxpool3d(dtype):
    from dvd_gan_amd import functional as Fn
    x = tied_input(dtype, 2, 2, 4, 4, 24, 410).requires_grad_(True)
    y = Fn.MaxPool3d.apply(x)
    xl = FR.leaf(x)
    ref = FR.maxpool3d(xl)
    dy = window(rn(411, *ref.shape).to(dtype), dtype, 412)
    poison(x)
    dx, = torch.autograd.grad([y], [x], [dy])
    torch.cuda.synchronize()
    ref_dx, = FR.grads(ref, (xl,), dy)
    assert same(y.detach(), ref.detach().to(dtype)) and equal(dx, ref_dx.to(dtype)), "max-pool routing (first maximum in scan order)"


# ================================================================== QKVConv
class QKV:
    def __init__(self, dtype, C, dq, seed=500):
        from dvd_gan_amd import functional as Fn
        from dvd_gan_amd import kern as K
        self.dtype, self.C, self.dq, self.dqp = dtype, C, dq, K.pad8(dq)
        self.ctot = 2 * self.dqp + C
        self.parts = ((0, dq), (self.dqp, dq), (2 * self.dqp, C))
        mk = lambda s, n: nn.Parameter((rn(s, n, C, 1, 1) / C ** 0.5).to(dtype).float())
        self.w = [mk(seed + i, n) for i, (_, n) in enumerate(self.parts)]
        self.b = [nn.Parameter(rn(seed + 3 + i, n)) for i, (_, n) in enumerate(self.parts)]
        self.x0 = rn(seed + 6, 2, 8, 8, C).to(dtype)
        dy = rn(seed + 7, 2, 8, 8, R.pad8(self.ctot))
        keep = TA.written_columns(dy.shape[-1], self.parts)
        dy[..., ~keep] = 0                                      # the gaps of an incoming dqkv are zero (the attention Functions' part)
        self.dy = window(dy.to(dtype), dtype, seed + 8)
        self.spec = Fn.ConvSpec((1, 1), self.ctot, C)
        pk = K.PackedConv(dtype, self.ctot, C, (1, 1), DEV)
        pk.fill(self.w[0].data, co_off=0).fill(self.w[1].data, co_off=self.dqp).fill(self.w[2].data, co_off=2 * self.dqp)
        self.spec.pack = pk
        self.w_eff = AR.w_from_pack(pk.wf, C, (1, 1))
        assert torch.equal(self.w_eff, FR.qkv_weight(*self.w, dq, self.dqp).detach()), "the pack is the fused weight, gap rows zero"

    def apply(self, x, frozen=False):
        from dvd_gan_amd.disc_nets import QKVConv
        det = (lambda t: t.detach()) if frozen else (lambda t: t)
        args = [det(t) for pair in zip(self.w, self.b) for t in pair]
        return QKVConv.apply(x, *args, self.spec, self.dq, self.dqp)

    def full(self, ts, shape_tail):
        """three per-part tensors -> one [ctot, ...] tensor with zero gaps"""
        out = torch.zeros(self.ctot, *shape_tail, device=DEV, dtype=ts[0].dtype)
        for (off, n), t in zip(self.parts, ts):
            out[off:off + n] = t
        return out


@DTYPES
@pytest.mark.parametrize("C,dq", [(24, 3), (128, 16)], ids=["C24-dq3-gaps", "C128-dq16"])
def test_qkv_conv(C, dq, dtype):
    q = QKV(dtype, C, dq)
    name = f"qkv C={C} dq={dq} {NAMES[dtype]}"
    bias = FR.qkv_bias(*[b.detach() for b in q.b], dq, q.dqp)
    # the assembled bias through a zero-input call: every pixel is the fp32 bias rounded once, gaps exactly 0
    y0 = q.apply(torch.zeros_like(q.x0))
    want = torch.zeros(y0.shape[-1], device=DEV)
    want[:q.ctot] = bias.float()
    assert same(y0, want.to(dtype).expand_as(y0).contiguous()), f"{name}: the fused bias"
    dxs = {}
    for direct in (False, True):
        label = f"{name} {'direct' if direct else 'autograd'}"
        for p in q.w + q.b:
            p.grad = None
        x = q.x0.clone().requires_grad_(True)
        with route(direct):
            y, var = _variants(lambda: q.apply(x))
            print(f"VARIANT {label}: forward {sorted(var)}")
            if not direct:
                entry_check(label + " y", y.detach(), *R.forward_ref(q.x0, q.w_eff, bias=bias.float()))
                refs = AR.conv_backward_ref(q.x0, q.w_eff, y.detach(), q.dy, (1, 1), dtype)
                g = torch.Generator(device=DEV).manual_seed(98)
                pre = [torch.randn(p.shape, generator=g, device=DEV) * 0.5 for p in q.w + q.b]
            else:
                for p, t in zip(q.w + q.b, pre):
                    p.grad = t.clone()
            poison(q.x0)
            got = torch.autograd.grad([y], [x] + q.w + q.b, [q.dy], allow_unused=True)
        AR.check(label + " dx", got[0], refs, "dx")
        dxs[direct] = got[0]
        if direct:
            assert all(t is None for t in got[1:]), f"{label}: no gradient is returned on the direct route"
            acc_w = AR.accumulated(refs, "dw", q.full(pre[:3], (C, 1, 1)))
            acc_b = AR.accumulated(refs, "db", q.full(pre[3:], ()))
        for i, (off, n) in enumerate(q.parts):
            sl = lambda e: tuple(t[off:off + n] for t in e)
            if direct:
                entry_check(f"{label} dw[{i}] (.grad - prefill)", q.w[i].grad.double() - pre[i].double(), *sl(acc_w), dtype=F32)
                entry_check(f"{label} db[{i}] (.grad - prefill)", q.b[i].grad.double() - pre[3 + i].double(), *sl(acc_b), dtype=F32)
            else:
                assert got[1 + i].dtype == F32 and got[4 + i].dtype == F32 and q.w[i].grad is None
                entry_check(f"{label} dw[{i}]", got[1 + i], *sl(refs["dw"]))
                entry_check(f"{label} db[{i}]", got[4 + i], *sl(refs["db"]))
    x = q.x0.clone().requires_grad_(True)
    dxf, = torch.autograd.grad([q.apply(x, frozen=True)], [x], [q.dy])
    assert same(dxs[False], dxs[True]) and same(dxs[False], dxf), f"{name}: dx bits depend on the requested parameter gradients"


# ================================================================== SelfAttention2d
def dgamma_ratio(got, pre, dsum, dmag, c, times=1):
    return abs(got - (pre + times * dsum)) / (c * E32 * (times * dmag + abs(pre)))


# name: dtype, C, dq, (H, W), ldq (None = 2 pad8(dq) + C rounded up to 8, what QKVConv writes), the path
ATT2D = {
    "mfma-bf16-N32": (BF, 128, 16, (4, 8), None, True),              # N = 32: the smallest dvd_attention_mfma_ok accepts (N >= 32, N % 32 == 0)
    "mfma-bf16-N32-ldq168": (BF, 128, 16, (4, 8), 168, True),        # pad columns behind v: the zero-filled dqkv of the MFMA path
    "f32-fp32-mfma-shape": (F32, 128, 16, (4, 8), None, False),
    "f32-fp32-C20": (F32, 20, 2, (4, 4), None, False),
    "f32-bf16-C20": (BF, 20, 2, (4, 4), None, False),
}


@pytest.mark.parametrize("case", list(ATT2D))
def test_self_attention_2d(case):
    from dvd_gan_amd import functional as Fn
    dtype, C, dq, (H, W), ldq, mfma = ATT2D[case]
    F_, N, g = 3, H * W, 0.7
    koff = R.pad8(dq)
    voff = 2 * koff
    ldq, ldx = ldq or R.pad8(voff + C), R.pad8(C)
    qkv0, _, x0, dy0 = TA.make_case(F_, N, N, dq, koff, voff, C, ldq, ldq, ldx, dtype, "units", True, 600)
    sh = lambda t: t.view(F_, H, W, t.shape[-1])
    dy = window(sh(dy0), dtype, 601)
    spans = [(0, dq), (koff, dq), (voff, C)]
    gaps = ~TA.written_columns(ldq, spans)
    runs = {}
    for mode in ("autograd", "direct", "frozen"):
        gamma = nn.Parameter(torch.tensor([g], device=DEV))          # (the module's initial 0 would hide dqkv)
        pre = 0.375
        x, qkv = sh(x0).clone().requires_grad_(True), sh(qkv0).clone().requires_grad_(True)
        with route(mode == "direct"):
            if mode == "direct":
                gamma.grad = torch.tensor([pre], device=DEV)

            def step():
                y = Fn.SelfAttention2d.apply(x, qkv, gamma.detach() if mode == "frozen" else gamma, dq, C)
                assert y.grad_fn.mfma is mfma, f"{case}: ctx.mfma = {y.grad_fn.mfma}"
                saved = y.grad_fn.saved_tensors
                poison(qkv0, qkv0)
                return y, saved, torch.autograd.grad([y], [x, qkv] + ([gamma] if mode != "frozen" else []), [dy], allow_unused=True)
            y, saved, got = step()
            if mode == "direct":
                once = float(gamma.grad)
                step()                                               # a fresh forward, a second backward: added again
                twice = float(gamma.grad)
        dx, dqkv = got[0], got[1]
        assert same(dx, dy), f"{case} {mode}: x.grad is dy"
        assert dqkv.shape == qkv.shape and dqkv.dtype == dtype and bool((dqkv[..., gaps] == 0).all()), f"{case} {mode}: gap / pad columns of dqkv"
        assert bool((y.detach()[..., C:] == 0).all())
        runs[mode] = (dqkv, y.detach())
        if mode == "frozen":
            continue
        w = TA.Worst(f"{case} {mode}")
        f3 = lambda t: t.detach().reshape(F_, N, t.shape[-1])
        att, aux = saved[2], saved[3]
        if mfma:
            dsum, dmag = TA.mfma_bounds(w, F_, N, C, g, qkv0, x0, dy0, f3(y), f3(att), aux, None, f3(dqkv))
            consts = TA.C_MFMA
        else:
            dsum, dmag = TA.f32_bounds(w, dtype, F_, N, N, dq, koff, voff, C, g, qkv0, qkv0, x0, dy0, f3(y), f3(att), aux, None,
                                       f3(dqkv), f3(dqkv))
            consts = TA.C_F32
        if mode == "autograd":
            assert got[2].shape == (1,) and got[2].dtype == F32 and gamma.grad is None
            w.add("dgamma", dgamma_ratio(float(got[2]), 0.0, dsum, dmag, consts["dgamma"]))
        else:
            assert got[2] is None, f"{case}: dgamma returned on the direct route as well"
            w.add("dgamma (.grad - prefill)", dgamma_ratio(once, pre, dsum, dmag, consts["dgamma"]))
            w.add("dgamma (.grad - prefill, second backward)", dgamma_ratio(twice, pre, dsum, dmag, consts["dgamma"], times=2))
        w.check(consts)
    for mode in ("direct", "frozen"):
        assert same(runs[mode][0], runs["autograd"][0]) and same(runs[mode][1], runs["autograd"][1]), f"{case}: {mode} changes dqkv / y"


# ================================================================== SelfAttentionKV + MaxPool3d
@DTYPES
def test_self_attention_kv_with_maxpool(dtype):
    """Composed as attention3d.SelfAttention.run: qkv feeds the max-pool (-> kv) and the attention node.  The two addends of
    qkv.grad are checked on their own, their sum as torch's own add of them."""
    from dvd_gan_amd import functional as Fn
    F_, T, H, W, C, dq, g = 2, 2, 4, 4, 16, 8, 0.7
    koff, voff, ldq = 8, 16, 32
    N, Nk = T * H * W, (T // 2) * (H // 2) * (W // 2)
    name = f"kv+maxpool {NAMES[dtype]}"
    qkv0 = tied_input(dtype, F_, T, H, W, ldq, 700)
    qkv0 = (qkv0.float() * 0.6).to(dtype)                            # (a common factor keeps the ties)
    x0, dy0 = rn(701, F_, T, H, W, C).to(dtype), rn(702, F_, T, H, W, C).to(dtype)
    dy = window(dy0, dtype, 703)
    gamma = nn.Parameter(torch.tensor([g], device=DEV))
    # (a) the attention node alone, on a detached copy of the pooled tensor
    x, qkv = x0.clone().requires_grad_(True), qkv0.clone().requires_grad_(True)
    kv = Fn.MaxPool3d.apply(qkv)
    ql = FR.leaf(qkv0)
    kv_ref = FR.maxpool3d(ql)
    assert same(kv.detach(), kv_ref.detach().to(dtype)), f"{name}: kv"
    kvl = kv.detach().clone().requires_grad_(True)
    y = Fn.SelfAttentionKV.apply(x, qkv, kvl, gamma, dq, C)
    saved = y.grad_fn.saved_tensors
    poison(qkv0, kvl)
    dx, dq_att, dkv, dgamma = torch.autograd.grad([y], [x, qkv, kvl, gamma], [dy])
    torch.cuda.synchronize()
    assert same(dx, dy), f"{name}: x.grad is dy"
    assert bool((dq_att[..., dq:] == 0).all()), f"{name}: only the q columns of the attention node's dqkv are written"
    assert bool((dkv[..., :koff] == 0).all()), f"{name}: the q columns of dkv are zero"
    w = TA.Worst(name)
    f3 = lambda t, n: t.detach().reshape(F_, n, t.shape[-1])
    dsum, dmag = TA.f32_bounds(w, dtype, F_, N, Nk, dq, koff, voff, C, g, f3(qkv0, N), f3(kvl, Nk), f3(x0, N), f3(dy0, N), f3(y, N),
                               f3(saved[3], N), saved[4], None, f3(dq_att, N), f3(dkv, Nk))
    assert dgamma.shape == (1,)
    w.add("dgamma", dgamma_ratio(float(dgamma), 0.0, dsum, dmag, TA.C_F32["dgamma"]))
    w.check(TA.C_F32)
    # (b) the max-pool node alone: dkv routed to the first maximum of every window
    q2 = qkv0.clone().requires_grad_(True)
    poison(qkv0)
    dpool, = torch.autograd.grad([Fn.MaxPool3d.apply(q2)], [q2], [dkv])
    ref_dpool, = FR.grads(kv_ref, (ql,), dkv)
    assert equal(dpool, ref_dpool.to(dtype)), f"{name}: the max-pool addend"
    # (c) composed: the hook on kv sees (a)'s dkv, qkv.grad is torch's own sum of the two addends
    x, qkv = x0.clone().requires_grad_(True), qkv0.clone().requires_grad_(True)
    kv = Fn.MaxPool3d.apply(qkv)
    seen = []
    kv.register_hook(lambda t: seen.append(t.clone()))
    y2 = Fn.SelfAttentionKV.apply(x, qkv, kv, gamma, dq, C)
    assert same(y2.detach(), y.detach())
    gamma.grad = None
    y2.backward(dy)
    torch.cuda.synchronize()
    assert len(seen) == 1 and same(seen[0], dkv), f"{name}: dkv at the hook"
    assert same(qkv.grad, dq_att + dpool), f"{name}: qkv.grad is the storage-type sum of the two addends"
    assert same(gamma.grad, dgamma) and same(x.grad, dy)


# ================================================================== SeparableAttnCellFn
@DTYPES
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_separable_attn_cell(axis, dtype):
    from dvd_gan_amd import functional as Fn
    B, T, W, H, C, dq, g = 2, 4, 4, 4, 16, 8, 0.7
    koff, voff, ldq = 8, 16, 32
    name = f"sepcell axis={axis} {NAMES[dtype]}"
    A = (T, W, H)[axis]
    qkv0 = rn(800 + axis, B, T, W, H, ldq)
    qkv0[..., :dq] *= 3.0 / math.sqrt(dq * T * W * H // A)
    qkv0 = qkv0.to(dtype)
    x0, dy0 = rn(810, B, T, W, H, C).to(dtype), rn(811, B, T, W, H, C).to(dtype)
    dy = window(dy0, dtype, 812)
    gamma = nn.Parameter(torch.tensor([g], device=DEV))
    x, qkv = x0.clone().requires_grad_(True), qkv0.clone().requires_grad_(True)
    y = Fn.SeparableAttnCellFn.apply(x, qkv, gamma, dq, C, axis)
    _, Qf, Kp, Vp, ksel, vsel, att = y.grad_fn.saved_tensors
    poison(qkv0)
    dx, dqkv, dgamma = torch.autograd.grad([y], [x, qkv, gamma], [dy])
    torch.cuda.synchronize()
    assert same(dx, dy), f"{name}: x.grad is dy"
    assert dqkv.shape == qkv0.shape and dqkv.dtype == dtype and dgamma.shape == (1,)
    gaps = ~TA.written_columns(ldq, [(0, dq), (koff, dq), (voff, C)])
    assert bool((dqkv[..., gaps] == 0).all())
    w = TA.Worst(name)
    got = dict(y=y.detach(), Qf=Qf, Kp=Kp, Vp=Vp, ksel=ksel, vsel=vsel, att=att, dqkv=dqkv)
    dsum, dmag, _, _ = TA.sep_bounds(w, name, dtype, B, T, W, H, dq, koff, voff, C, axis, g, qkv0, x0, dy0, got)
    w.add("dgamma", dgamma_ratio(float(dgamma), 0.0, dsum, dmag, TA.C_SEP["dgamma"]))
    w.check(TA.C_SEP)
    # the float64 autograd statement of the whole cell agrees with what sep_bounds held the outputs to
    ql, xl, gl = FR.leaf(qkv0), FR.leaf(x0), torch.tensor([g], dtype=torch.float64, device=DEV, requires_grad=True)
    ry = FR.sep_cell(ql, xl, gl, dq, C, axis)
    rdq, rdx, rdg = FR.grads(ry, (ql, xl, gl), dy0)
    tag = "" if dtype == F32 else "_bf16"
    for key, a, n in (("dq", 0, dq), ("dk", koff, dq), ("dv", voff, C)):
        e = rel_l2(dqkv[..., a:a + n], rdq[..., a:a + n])
        note(f"{name} {key} rel-L2 (fp64 autograd)", e)
        assert e <= TA.C_SEP[key + tag]
    assert torch.equal(rdx, dy0.double())


# ================================================================== ProjectionHead
class Head:
    Fr, S, C, ld, NCLS = 6, 4, 20, 24, 5

    def __init__(self, dtype, seed=900):
        C = self.C
        self.dtype = dtype
        self.feat0 = rn(seed, self.Fr, self.S, self.S, self.ld).to(dtype)           # pad lanes: finite garbage
        self.w_lin = nn.Parameter(rn(seed + 1, 1, C) * 0.2)
        self.b_lin = nn.Parameter(torch.tensor([0.25], device=DEV))
        self.w_emb = nn.Parameter(rn(seed + 2, self.NCLS, C) * 0.2)
        self.cls = torch.tensor([0, 2, 2, 3, 0, 4], dtype=torch.int32, device=DEV)   # 0 and 2 repeat, 1 is never named
        unit = lambda t: t / t.norm()
        self.u0 = [unit(rn(seed + 3, 1)), unit(rn(seed + 4, self.NCLS))]
        self.v0 = [unit(rn(seed + 5, C)), unit(rn(seed + 6, C))]
        self.dout = rn(seed + 7, self.Fr)
        self.P = self.S * self.S

    def run(self, direct=False, frozen=False, feat_grad=True, prefill=None, log=None):
        """-> out, saved tensors, (dfeat, dw_lin, db, dw_emb) as autograd hands them out, u / v after the forward"""
        from dvd_gan_amd import functional as Fn
        params = (self.w_lin, self.b_lin, self.w_emb)
        for p in params:
            p.grad = None
        u = [t.clone() for t in self.u0]
        v = [t.clone() for t in self.v0]
        feat = self.feat0.clone().requires_grad_(feat_grad)
        det = (lambda t: t.detach()) if frozen else (lambda t: t)
        with route(direct):
            if direct:
                for p, t in zip(params, prefill):
                    p.grad = t.clone()
            out = Fn.ProjectionHead.apply(feat, det(self.w_lin), det(self.b_lin), det(self.w_emb), self.cls, (u[0], v[0]), (u[1], v[1]),
                                          self.C)
            saved = out.grad_fn.saved_tensors
            returned = []
            out.grad_fn.register_hook(lambda gin, gout: returned.append(gin))
            ins = ([feat] if feat_grad else []) + ([] if frozen else list(params))
            poison(self.feat0)
            got = list(torch.autograd.grad([out], ins, [self.dout], allow_unused=True))
        if not feat_grad:
            got.insert(0, None)
            assert returned and returned[0][0] is None, "feat without a gradient: the Function returns None for it"
        if frozen:
            got += [None, None, None]
        return out.detach(), saved, got, u, v


@DTYPES
def test_projection_head(dtype, monkeypatch):
    from dvd_gan_amd import kern as K
    hd = Head(dtype)
    C, name = hd.C, f"head {NAMES[dtype]}"
    sn_calls = []
    orig = K.sn_backward
    monkeypatch.setattr(K, "sn_backward", lambda G, *a, **kw: (sn_calls.append((G.clone(), a[1].clone(), kw.get("out") is not None)), orig(G, *a, **kw))[1])
    out, saved, got, u, v = hd.run()
    s_l, s_e = saved[5], saved[6]
    # one power iteration per wrapper, from the u held before the forward (v is overwritten)
    sn = []
    for i, Wt in enumerate((hd.w_lin, hd.w_emb)):
        s_r, u_r, v_r = FR.power_iter(Wt.detach(), hd.u0[i])
        e = max(rel_l2(u[i], u_r), rel_l2(v[i], v_r), abs(float((s_l, s_e)[i]) - float(s_r)) / float(s_r))
        note(f"{name} power iteration {('lin', 'emb')[i]} sigma / u / v rel", e)
        assert e <= SN_REL
        assert not torch.equal(v[i], hd.v0[i])
        sn.append((u[i], v[i], (s_l, s_e)[i]))                       # the LATEST u, v (quirk 7) and the sigma of the forward
    assert not torch.equal(u[1], hd.u0[1]), "the embedding's u must move, or a backward on the pre-forward u could not be told apart"
    # bounds of the raw gradients, as test_gpu_pointwise.test_proj_head / test_relu_spatial_sum hold the kernels to them
    f64, d64 = hd.feat0[..., :C].double().clamp_min(0), hd.dout.double()
    h = f64.reshape(hd.Fr, -1, C).sum(1)
    eh = hd.P * E32 * h
    weff = hd.w_lin.detach().double() / float(s_l) + hd.w_emb.detach().double()[hd.cls.long()] / float(s_e)
    wabs = hd.w_lin.detach().double().abs() / float(s_l) + hd.w_emb.detach().double()[hd.cls.long()].abs() / float(s_e)
    t_abs = d64.abs()[:, None] * h
    eGl = TERMS * t_abs.sum(0, keepdim=True) + (d64.abs()[:, None] * eh).sum(0, keepdim=True)
    eGe = torch.zeros(hd.NCLS, C, dtype=torch.float64, device=DEV).index_add(0, hd.cls.long(), TERMS * t_abs + d64.abs()[:, None] * eh)
    r = FR.proj_head_grads(hd.feat0, hd.w_lin.detach(), hd.b_lin.detach(), hd.w_emb.detach(), hd.cls, sn[0], sn[1], hd.dout, C, (eGl, eGe))
    e_out = TERMS * ((h * wabs).sum(1) + 0.25) + (eh * wabs).sum(1)
    entry_check(name + " out", out, r["out"], e_out)
    live = torch.zeros_like(hd.feat0, dtype=torch.bool)
    live[..., :C] = hd.feat0[..., :C] > 0
    b_df = torch.nn.functional.pad((4 * E32 * d64.abs()[:, None] * wabs)[:, None, None, :].expand(-1, hd.S, hd.S, -1), (0, hd.ld - C))
    zero = torch.zeros_like(r["dfeat"])

    def check_grads(label, dfeat, dwl, db, dwe, pre=None):
        entry_check(label + " dfeat", dfeat, torch.where(live, r["dfeat"], zero), torch.where(live, b_df, zero), live)
        e_db = TERMS * (float(d64.abs().sum()) + (abs(float(pre[1])) if pre else 0.0))
        for key, got_, p in (("dw_lin", dwl, 0), ("dw_emb", dwe, 2)):
            ref, bound = r[key]
            if pre:
                refs = {key: (ref, bound, torch.ones_like(ref, dtype=torch.bool)), "M": 1, "mag": {key: ref.abs() + bound}}
                ref, bound, _ = AR.accumulated(refs, key, pre[p])
                got_ = got_.double() - pre[p].double()
            entry_check(f"{label} {key}", got_, ref, bound, dtype=F32)
        got_b = float(db) - (float(pre[1]) if pre else 0.0)
        e = abs(got_b - float(r["db"])) / e_db
        note(f"{label} db err/bound", e)
        assert e <= 1.0

    check_grads(name + " autograd", *got)
    assert all(p.grad is None for p in (hd.w_lin, hd.b_lin, hd.w_emb))
    # the class no frame names: its row of the RAW embedding gradient is exactly 0 (what dvd_proj_head_backward promises).  Under the
    # spectral norm the row of dw_emb is the rank-one term -dot / sigma^2 u[1] v alone -- checked above against sn_backward_ref.
    assert [c[2] for c in sn_calls] == [False, False] and bool((sn_calls[1][0][1] == 0).all()) and bool((sn_calls[1][0][[0, 2, 3, 4]] != 0).any())
    assert all(torch.equal(c[1], uu) for c, uu in zip(sn_calls, u)), "sn_backward reads the u the wrapper holds AFTER the forward"
    # direct: the kernel adds into b.grad, sn_backward(out=.grad) into the weights'
    gen = torch.Generator(device=DEV).manual_seed(97)
    pre = [torch.randn(p.shape, generator=gen, device=DEV) * s for p, s in ((hd.w_lin, r["dw_lin"][0].abs().mean().float()),
                                                                            (hd.b_lin, 1.0), (hd.w_emb, r["dw_emb"][0].abs().mean().float()))]
    del sn_calls[:]
    out_d, _, got_d, _, _ = hd.run(direct=True, prefill=pre)
    assert got_d[1] is None and got_d[2] is None and got_d[3] is None, "the direct route returns no parameter gradient"
    assert [c[2] for c in sn_calls] == [True, True] and bool((sn_calls[1][0][1] == 0).all())
    check_grads(name + " direct (.grad - prefill)", got_d[0], hd.w_lin.grad, hd.b_lin.grad, hd.w_emb.grad, pre)
    assert same(out_d, out) and same(got_d[0], got[0])
    # frozen: detached parameters; feat without a gradient
    out_f, _, got_f, _, _ = hd.run(frozen=True)
    assert same(got_f[0], got[0]) and same(out_f, out), f"{name}: dfeat bits depend on the requested parameter gradients"
    _, _, got_n, _, _ = hd.run(feat_grad=False)
    assert got_n[0] is None and all(same(a, b) for a, b in zip(got_n[1:], got[1:]))


# ================================================================== layout
@DTYPES
def test_layout_swaps(dtype):
    """ToChannelsLast / FromChannelsLast with swap=(3, 5) and SwapFrameOrder(3, 5) then (5, 3): forward and backward torch.equal to the
    reference permutation (bf16 rounding is torch's RNE), the round trips the identity."""
    from dvd_gan_amd import functional as Fn
    A, B, C = 3, 5, 5
    img = rn(1000, A * B, C, 2, 3).requires_grad_(True)
    t = Fn.ToChannelsLast.apply(img, dtype, (A, B))
    assert same(t.detach(), FR.to_cl(img.detach(), dtype, (A, B)))
    g = window(rn(1001, *t.shape).to(dtype), dtype, 1002)
    dimg, = torch.autograd.grad([t], [img], [g])
    assert same(dimg, FR.from_cl(g, C, (A, B)))
    tl = t.detach().clone().requires_grad_(True)
    back = Fn.FromChannelsLast.apply(tl, C, (A, B))
    assert same(back.detach(), FR.from_cl(t.detach(), C, (A, B))) and same(back.detach(), img.detach().to(dtype).float())
    g2 = rn(1003, *img.shape).transpose(2, 3).contiguous().transpose(2, 3)
    assert not g2.is_contiguous()
    dt, = torch.autograd.grad([back], [tl], [g2])
    assert same(dt, FR.to_cl(g2, dtype, (A, B)))
    x = rn(1004, A * B, 2, 2, 8).to(dtype).requires_grad_(True)
    y1 = Fn.SwapFrameOrder.apply(x, A, B)
    y2 = Fn.SwapFrameOrder.apply(y1, B, A)
    assert same(y1.detach(), FR.swap_frames(x.detach(), A, B)) and same(y2.detach(), x.detach()) and not same(y1.detach(), x.detach())
    g3 = window(rn(1005, *x.shape).to(dtype), dtype, 1006)
    d1, = torch.autograd.grad([y1], [x], [g3], retain_graph=True)
    assert same(d1, FR.swap_frames(g3, B, A)), "SwapFrameOrder.backward is the INVERSE permutation"
    d2, = torch.autograd.grad([y2], [x], [g3])
    assert same(d2, g3.contiguous())
    torch.cuda.synchronize()

"""tests/autograd_ref.py (the float64 statement of functional.Conv and its checker) proven on the CPU, before any kernel is held
to it (tests/test_gpu_autograd_conv.py):

  a  the reference agrees with torch.autograd on the plain float64 composition of the same function -- F.conv2d / F.conv3d,
     F.interpolate(scale_factor=2), relu / tanh, the residual add, W_bar / (u . W_bar v) under a spectral norm, the partner as a
     second consumer of x -- to 1e-12 rel-L2, for every case kind of the GPU file at CPU-sized shapes.  Storage type float64 here:
     no rounding is left, and the derivative taken from the stored y IS the derivative at the pre-activation;
  b  an honest implementation -- torch's own fp32 CPU ops on the stored operands, rounded where the Function rounds (dy', the
     full-size result of the unfused up2 route, the final stores) -- passes every check in both storage types.  The bounds are
     derived, so they have to admit another summation order.  The ratios are printed (profiles/autograd_conv_numbers.md);
  c  every wrong backward of MUTANTS, built from the same operands by the same code with one switch thrown, makes the checker
     raise, while the honest output of the same request passes in the same test.
"""
import pytest
import torch
import torch.nn.functional as F

import autograd_ref as AR
import conv_ref as R

TOL = 1e-12
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAMES = {BF: "bf16", F32: "fp32", F64: "fp64"}

# name: frames, input grid, Cin, Cout, taps, options      (the case kinds of tests/test_gpu_autograd_conv.py, CPU-sized)
CASES = {
    "up2-fused": (2, (4, 6), 5, 7, (3, 3), dict(up2=True)),
    "up2-fused-relu": (2, (4, 6), 5, 7, (3, 3), dict(up2=True, relu_in=True)),
    "up2-unfused": (2, (3, 5), 5, 7, (3, 3), dict(up2=True, relu_in=True, unfused=True)),
    "plain-res": (2, (6, 6), 6, 9, (3, 3), dict(res="full")),
    "res-up2": (2, (6, 6), 6, 9, (3, 3), dict(res="half")),
    "d-conv0": (2, (6, 5), 8, 8, (3, 3), dict(relu_in=True, act=R.ACT_RELU)),
    "d-conv0-3d": (1, (3, 4, 4), 4, 6, (3, 3, 3), dict(relu_in=True, act=R.ACT_RELU)),
    "shortcut-3d": (1, (3, 4, 4), 4, 6, (1, 1, 1), dict()),
    "stem": (2, (6, 6), 3, 10, (3, 3), dict()),
    "rgb": (2, (6, 6), 10, 3, (3, 3), dict(relu_in=True, act=R.ACT_TANH)),
    "frame": (3, (4, 4), 6, 9, (3, 3), dict()),
    "slot": (2, (6, 6), 6, 9, (1, 1), dict(slot=True)),
}


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def _nc(t):          # channels-last -> channels-first
    return t.movedim(-1, 1).contiguous()


def _cl(t):          # channels-first -> channels-last
    return t.movedim(1, -1).contiguous()


def _padc(t, c):
    return F.pad(t, (0, R.pad8(c) - c))


def compose(x, w, b, res, ks, *, up2=False, relu_in=False, act=R.ACT_NONE, res_half=False):
    """The function, composed the plain way on channels-first tensors (any float type)."""
    xin = F.relu(x) if relu_in else x
    if up2:
        xin = F.interpolate(xin, scale_factor=2)
    y = (F.conv3d if len(ks) == 3 else F.conv2d)(xin, w, b, padding=[k // 2 for k in ks])
    if res is not None:
        y = y + (F.interpolate(res, scale_factor=2) if res_half else res)
    return torch.tanh(y) if act == R.ACT_TANH else F.relu(y) if act == R.ACT_RELU else y


class Ops:
    """Stored operands of one request in storage type `st`, drawn from a fixed seed at the scales conv_ref.make_request uses."""

    def __init__(self, case, st, sn, seed=0):
        F_, sp, cin, cout, ks, opt = CASES[case]
        self.case, self.st, self.cin, self.cout, self.ks, self.sp = case, st, cin, cout, ks, sp
        self.up2, self.relu_in = opt.get("up2", False), opt.get("relu_in", False)
        self.act, self.unfused, self.res_kind = opt.get("act", R.ACT_NONE), opt.get("unfused", False), opt.get("res")
        g = torch.Generator().manual_seed(1000 * list(CASES).index(case) + seed)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
        osp = tuple(sp[:-2]) + tuple(v * (2 if self.up2 else 1) for v in sp[-2:])
        self.x = rn(F_, *sp, R.pad8(cin)).to(st)
        self.bias = rn(cout).to(F32 if st != F64 else F64)
        fan = cin * torch.Size(ks).numel()
        cd = F64 if st == F64 else F32
        if sn:
            self.w_bar = (rn(cout, cin, *ks) / fan ** 0.5).to(cd)
            u, v = rn(cout), rn(fan)
            self.u, self.v = (u / u.norm()).to(cd), (v / v.norm()).to(cd)
            self.sigma = (self.u @ (self.w_bar.view(cout, -1) @ self.v)).reshape(1)        # what one power iteration leaves
            self.w_eff = (self.w_bar / self.sigma).to(st).double()
            self.sn = (self.w_bar, self.u, self.v, self.sigma)
        else:
            self.w_eff, self.sn = (rn(cout, cin, *ks) / fan ** 0.5).to(st).double(), None
        self.res = None
        if self.res_kind:
            rsp = osp if self.res_kind == "full" else tuple(osp[:-2]) + (osp[-2] // 2, osp[-1] // 2)
            self.res = rn(F_, *rsp, R.pad8(cout)).to(st)
        self.dy = _padc(rn(F_, *osp, cout), cout).to(st)                   # zero pad columns, as the ABI promises
        self.partner = rn(F_, *sp, R.pad8(cin)).to(st) if opt.get("slot") else None
        self.dw_prefill, self.db_prefill = rn(cout, cin, *ks).to(F32), rn(cout).to(F32)
        # the stored y: the honest forward (exact under float64 storage)
        y = compose(_nc(self.x[..., :cin]).to(cd), self.w_eff.to(cd), self.bias.to(cd),
                    _nc(self.res[..., :cout]).to(cd) if self.res is not None else None, ks, up2=self.up2, relu_in=self.relu_in,
                    act=self.act, res_half=self.res_kind == "half")
        self.y = _padc(_cl(y), cout).to(st)

    def refs(self):
        return AR.conv_backward_ref(self.x, self.w_eff, self.y, self.dy, self.ks, self.st, act=self.act, up2=self.up2,
                                    relu_in=self.relu_in, partner=self.partner, unfused=self.unfused,
                                    res_up2=None if self.res is None else self.res_kind == "half", sn=self.sn)


# ------------------------------------------------------------------ a: agreement with autograd
@pytest.mark.parametrize("sn", [False, True], ids=["plain", "sn"])
@pytest.mark.parametrize("case", list(CASES))
def test_reference_equals_fp64_autograd(case, sn):
    o = Ops(case, F64, sn)
    x = _nc(o.x[..., :o.cin]).requires_grad_(True)
    b = o.bias.clone().requires_grad_(True)
    res = _nc(o.res[..., :o.cout]).requires_grad_(True) if o.res is not None else None
    if sn:
        wl = o.w_bar.clone().requires_grad_(True)
        w = wl / (o.u @ (wl.view(o.cout, -1) @ o.v))            # u, v constants (Normalization.py:19-31)
        assert rel(w.detach(), o.w_eff) < TOL
    else:
        wl = w = o.w_eff.clone().requires_grad_(True)
    y = compose(x, w, b, res, o.ks, up2=o.up2, relu_in=o.relu_in, act=o.act, res_half=o.res_kind == "half")
    assert rel(_cl(y.detach()), o.y[..., :o.cout]) < TOL
    outs, grads = [y], [_nc(o.dy[..., :o.cout])]
    if o.partner is not None:                                   # the other consumer of x, whose input gradient is the partner
        outs.append((x * _nc(o.partner[..., :o.cin])).sum())
        grads.append(torch.ones((), dtype=F64))
    torch.autograd.backward(outs, grads)
    refs = o.refs()
    assert rel(refs["dx"][0][..., :o.cin], _cl(x.grad)) < TOL
    assert bool((refs["dx"][0][..., o.cin:] == 0).all())
    assert rel(refs["dw"][0], wl.grad) < TOL
    assert rel(refs["db"][0], b.grad) < TOL
    if res is not None:
        assert rel(refs["dres"][0][..., :o.cout], _cl(res.grad)) < TOL
    # with nothing rounded, every bound is a few units of 2^-24 of the magnitudes: the reference passes its own check
    AR.check_backward(f"{case} fp64 self", refs, dx=refs["dx"][0], dw=refs["dw"][0].float(), db=refs["db"][0].float())


# ------------------------------------------------------------------ b / c: an honest fp32 implementation and its mutants
def honest(o, mut=None):
    """Conv.backward in torch's fp32 CPU ops on the stored operands, rounding where the Function rounds; `mut`: one of MUTANTS.
    -> dict(dx, dres, dw, db [returned tensors], dw_buf, db_buf [prefilled buffers after accumulation])"""
    st, cin, cout, ks = o.st, o.cin, o.cout, o.ks
    nd = len(ks)
    pad = [k // 2 for k in ks]
    f = lambda t, c: _nc(t[..., :c]).float()
    w = o.w_eff.float()
    x, dy, y = f(o.x, cin), f(o.dy, cout), f(o.y, cout)
    xin = F.relu(x) if o.relu_in else x
    if o.up2:
        xin = F.interpolate(xin, scale_factor=2)
    if o.act == R.ACT_TANH:
        dyp = dy * ((1 - y) if mut == "tanh-1-minus-y" else (1 - y * y))
    elif o.act == R.ACT_RELU:
        dyp = torch.where((dy if mut == "relu-from-sign-of-dy" else y) > 0, dy, torch.zeros_like(dy))
    else:
        dyp = dy
    dyp = dyp.to(st).float()                                                # rounding point 1
    full = (F.conv_transpose3d if nd == 3 else F.conv_transpose2d)(dyp, w, padding=pad)
    sum2 = lambda t: t.reshape(*t.shape[:-2], t.shape[-2] // 2, 2, t.shape[-1] // 2, 2).sum(dim=(-3, -1))
    if o.up2:
        if o.unfused:
            full = full.to(st).float()                                      # rounding point 2
        if mut == "mask-on-full-grid":          # the mask buffer read at the FULL-size grid's coordinates (wrapped into it), before the sum
            full = full * (x.repeat(1, 1, 2, 2) > 0)
        dx = sum2(full)
    else:
        dx = full
    if o.relu_in and mut not in ("mask-omitted", "mask-on-full-grid"):
        dx = dx * ((y if mut == "mask-from-y" else x) > 0)
    if o.partner is not None:
        dx = dx + {"partner-dropped": 0.0, "partner-twice": 2.0}.get(mut, 1.0) * f(o.partner, cin)
    dx = _padc(_cl(dx), cin).to(st)
    if mut == "pad-channel":
        dx[..., cin] = 2.0 ** -20
    src = dy if mut == "dw-db-from-dy" else dyp
    wgrad = torch.nn.grad.conv3d_weight if nd == 3 else torch.nn.grad.conv2d_weight
    G = wgrad(xin, w.shape, src, padding=pad)
    db = src.sum(dim=[d for d in range(src.dim()) if d != 1])
    if o.sn is not None:
        W, u, v, s = (t.float() for t in o.sn)
        if mut == "sn-sigma-off":
            s = s * 1.01
        dw = G / s
        if mut != "sn-projection-dropped":
            dw = dw - (G * W).sum() / (s * s) * torch.outer(u, v).view_as(W)
    else:
        dw = G
    acc = lambda pre, g: g.clone() if mut == "prefill-lost" else pre + g + g if mut == "added-twice" else pre + g
    dres = None
    if o.res is not None:
        dres = o.dy.clone()
        if o.res_kind == "half":
            dres = _cl(sum2(_nc(o.dy).float()) * (0.25 if mut == "dres-quarter" else 1.0)).to(st)
    return dict(dx=dx, dres=dres, dw=dw, db=db, dw_buf=acc(o.dw_prefill, dw), db_buf=acc(o.db_prefill, db))


def _check(name, o, refs, got, direct):
    if direct:
        return AR.check_backward(name, refs, dx=got["dx"], dres=got["dres"], dw=got["dw_buf"], db=got["db_buf"],
                                 dw_prefill=o.dw_prefill, db_prefill=o.db_prefill)
    return AR.check_backward(name, refs, dx=got["dx"], dres=got["dres"], dw=got["dw"], db=got["db"])


@pytest.mark.parametrize("sn", [False, True], ids=["plain", "sn"])
@pytest.mark.parametrize("st", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", list(CASES))
def test_honest_implementation_passes(case, st, sn):
    o = Ops(case, st, sn)
    refs = o.refs()
    got = honest(o)
    name = f"honest {case} {NAMES[st]} {'sn' if sn else 'plain'}"
    AR.check(f"{name} dy'", _honest_dyp(o), refs, "dyp")
    for direct in (False, True):
        r = _check(f"{name} {'direct' if direct else 'autograd'}", o, refs, got, direct)
        assert max(r.values()) <= 1.0
    assert got["dx"].dtype == st and bool((got["dx"][..., o.cin:] == 0).all())
    if o.res_kind == "full":
        assert torch.equal(got["dres"], o.dy)


def _honest_dyp(o):
    """dy' of the honest implementation, stored (for the check of dy' itself)"""
    dy, y = o.dy.float(), o.y.float()
    if o.act == R.ACT_TANH:
        return (dy * (1 - y * y)).to(o.st)
    if o.act == R.ACT_RELU:
        return torch.where(y > 0, dy, torch.zeros_like(dy)).to(o.st)
    return o.dy


# mutant: (case it is built on, spectral norm, direct route)
MUTANTS = {
    "mask-from-y": ("d-conv0", False, False),                  # mask of dx from y instead of x (Cin = Cout, same grid)
    "mask-omitted": ("d-conv0", False, False),
    "mask-on-full-grid": ("up2-fused-relu", False, False),     # mask applied on the full-size grid, before the 2 x 2 sum
    "tanh-1-minus-y": ("rgb", False, False),                   # 1 - y instead of 1 - y^2
    "relu-from-sign-of-dy": ("d-conv0", False, False),
    "dw-db-from-dy": ("d-conv0", False, False),                # dw and db from dy instead of dy'
    "dres-quarter": ("res-up2", False, False),                 # half-size residual: averaged instead of summed
    "partner-dropped": ("slot", True, False),
    "partner-twice": ("slot", True, False),
    "sn-projection-dropped": ("plain-res", True, False),       # G / sigma only
    "sn-sigma-off": ("plain-res", True, True),                 # a sigma 1 % off
    "prefill-lost": ("plain-res", False, True),                # .grad overwritten instead of added to
    "added-twice": ("plain-res", True, True),
    "pad-channel": ("stem", False, False),                     # one padded channel of dx at 2^-20
}
# which outputs the mutant must break (the others still pass: the switch touches nothing else)
BREAKS = {"mask-from-y": "dx", "mask-omitted": "dx", "mask-on-full-grid": "dx", "tanh-1-minus-y": "dx",
          "relu-from-sign-of-dy": "dx", "dw-db-from-dy": "dw", "dres-quarter": "dres", "partner-dropped": "dx",
          "partner-twice": "dx", "sn-projection-dropped": "dw", "sn-sigma-off": "dw", "prefill-lost": "dw", "added-twice": "dw",
          "pad-channel": "dx"}


@pytest.mark.parametrize("st", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mut", list(MUTANTS))
def test_wrong_backward_is_rejected(mut, st):
    case, sn, direct = MUTANTS[mut]
    o = Ops(case, st, sn, seed=1)
    refs = o.refs()
    name = f"{mut} {case} {NAMES[st]}"
    _check(f"{name} honest", o, refs, honest(o), direct)              # the honest output of the same request passes
    bad = honest(o, mut)
    with pytest.raises(AssertionError, match=f" {BREAKS[mut]}"):
        _check(name, o, refs, bad, direct)
    if mut == "dw-db-from-dy":                                         # db on its own as well
        with pytest.raises(AssertionError, match=" db"):
            AR.check_backward(name, refs, db=bad["db"])
    if mut in ("tanh-1-minus-y", "relu-from-sign-of-dy"):              # and dy' itself is held
        dy, y = o.dy.float(), o.y.float()
        wrong = dy * (1 - y) if mut == "tanh-1-minus-y" else torch.where(dy > 0, dy, torch.zeros_like(dy))
        with pytest.raises(AssertionError):
            AR.check(f"{name} dy'", wrong.to(st), refs, "dyp")

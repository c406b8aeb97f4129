"""functional.Conv ROUTE BY ROUTE against float64 (tests/autograd_ref.py), through Fn.Conv.apply exactly as
sn_layers.SpectralNormConv.forward and the plain-weight callers drive it: a ConvSpec with the caller's pack (filled with sigma under
a spectral norm), real leaf nn.Parameters, the backward pass run by the autograd engine.  The kernels have their own element-wise
tests; this file pins the GLUE -- which operand, which mask, which pack image, which route and which stream each kernel gets.

Call log: the built-in monkeypatch fixture wraps kern.conv_forward / pool / act_backward / conv_wgrad / colsum / sn_backward; the
wrappers record arguments, result and current stream.  Each case asserts its route from that log (CASES below), and in bf16 mode
the kernel family from the library's per-launch records where the case names one (exact mode and frames below 16 pixels take
whatever general kernel the planner picks: printed).

Per run (case x storage type x plain / spectral norm x autograd / direct route):
  1 route      as the case states; on the direct route the weight-gradient launches ran on Fn.side_stream() into the prefilled
               .grad (under SN: overwrite=True into a fresh buffer, then sn_backward(out=param.grad)); else on the current stream
  2 y          conv_ref.check_forward on the stored y (owns the y the derivative is taken from)
  3 dx, dres   ratio <= 1 against autograd_ref, masked-out elements and the channels [Cin, pad8(Cin)) exactly 0, dtype / shape /
               contiguity as the caller expects; a full-size residual's dres equals dy bit for bit
  4 dw, db     ratio <= 1 -- on `.grad - prefill` on the direct route (the returned dw / db are None there), on the returned tensors
               on the autograd route
  5 dx bits    do not depend on which parameter gradients were requested (autograd / direct, trainable / frozen)
Operands: drawn in the storage type from fixed seeds at the scales of conv_ref.make_request; dy with zero pad columns (in one
case handed over as a non-contiguous channel window of a wider, poisoned buffer: the dy.contiguous() path).

Then the GradSlot partner sum on the Function (a test-local Function stands in for the main branch) and on whole GResBlocks
(slot path against the same five layers composed by hand on two leaf copies of x), and Fn.LinearF32 / Fn.Embedding on both routes.

profiles/autograd_conv_numbers.md has the routes, variants and ratios seen.
"""
import copy
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import autograd_ref as AR
import conv_ref as R
import gru_ref
from test_gpu_mfma16 import _variants
from test_gpu_wgrad_strided import profiled

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAMES = {BF: "bf16", F32: "fp32"}
POISON = R.POISON

# name: frames, INPUT grid, Cin, Cout, taps, options, bf16 kernel variants (forward, backward-data) or None = printed only
# (csrc/prof.h: 2 = halo 128 x 128, 8 = whole frames on 128-row tiles, 9 = thin).  res: "full" / "half"; live: which of x, w, b
# require a gradient.  Each is the smallest shape at which its route is still taken.
CASES = {
    "up2-fused": (2, (8, 8), 24, 40, (3, 3), dict(up2=True), None),
    "up2-fused-relu": (2, (8, 8), 24, 40, (3, 3), dict(up2=True, relu_in=True), None),
    "up2-unfused": (2, (6, 6), 24, 40, (3, 3), dict(up2=True, relu_in=True, unfused=True), None),
    "plain-res": (2, (16, 16), 64, 72, (3, 3), dict(res="full", window=True), (2, None)),
    "res-up2": (2, (16, 16), 64, 72, (3, 3), dict(res="half"), None),
    "d-conv0": (2, (16, 16), 24, 40, (3, 3), dict(relu_in=True, act=R.ACT_RELU), None),
    "d-conv0-3d": (1, (4, 8, 8), 16, 24, (3, 3, 3), dict(relu_in=True, act=R.ACT_RELU), None),
    "shortcut-3d": (1, (4, 8, 8), 16, 24, (1, 1, 1), dict(), None),
    "stem": (3, (32, 32), 3, 64, (3, 3), dict(), (9, 9)),
    "rgb": (3, (32, 32), 64, 3, (3, 3), dict(relu_in=True, act=R.ACT_TANH), (9, 9)),
    "frame8": (5, (8, 8), 64, 72, (3, 3), dict(), (8, 8)),
    "frame4": (13, (4, 4), 64, 72, (3, 3), dict(), (8, 8)),
    "frozen": (2, (16, 16), 64, 72, (3, 3), dict(res="full", live="x"), None),
    "bias-only": (2, (16, 16), 64, 72, (3, 3), dict(res="full", live="xb"), None),
    "no-dx": (2, (16, 16), 64, 72, (3, 3), dict(res="full", live="wb"), None),
    "slot": (2, (16, 16), 64, 72, (1, 1), dict(slot=True), None),          # test_slot_partner_sum
}
LOGGED = ("conv_forward", "pool", "act_backward", "conv_wgrad", "colsum", "sn_backward")


class Log:
    """kern.<LOGGED> wrapped through monkeypatch: every call appended as (name, args, kwargs, result, current stream)."""

    def __init__(self, monkeypatch):
        from dvd_gan_amd import kern as K
        self.calls, self.orig = [], {}
        for name in LOGGED:
            self.orig[name] = getattr(K, name)
            monkeypatch.setattr(K, name, self._wrap(name))

    def _wrap(self, name):
        def logged(*a, **kw):
            out = self.orig[name](*a, **kw)
            self.calls.append(SimpleNamespace(name=name, a=a, kw=kw, out=out, stream=torch.cuda.current_stream()))
            return out
        return logged

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _same(a, b):
    """the same stored tensor (autograd hands saved tensors back as new Python objects over the same memory)"""
    return a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype


def _rn(g, *s):
    return torch.randn(*s, generator=g, device=DEV)


class Layer:
    """Operands and parameters of one case, built ONCE per (case, storage type, plain / SN) the way SpectralNormConv.forward builds
    them: one power iteration, the pack filled with sigma, a ConvSpec per forward."""

    def __init__(self, case, dtype, sn):
        from dvd_gan_amd import kern as K
        F_, sp, cin, cout, ks, opt, _ = CASES[case]
        self.case, self.dtype, self.sn_on, self.cin, self.cout, self.ks, self.opt = case, dtype, sn, cin, cout, ks, opt
        self.up2, self.relu_in, self.act = opt.get("up2", False), opt.get("relu_in", False), opt.get("act", R.ACT_NONE)
        g = torch.Generator(device=DEV).manual_seed(7000 + 10 * list(CASES).index(case) + int(sn))
        osp = tuple(sp[:-2]) + tuple(v * (2 if self.up2 else 1) for v in sp[-2:])
        fan = cin * torch.Size(ks).numel()
        self.x0 = _rn(g, F_, *sp, R.pad8(cin)).to(dtype)
        w = _rn(g, cout, cin, *ks) / fan ** 0.5
        self.w = nn.Parameter(w if sn else w.to(dtype).float())
        self.b = nn.Parameter(_rn(g, cout))
        self.res0 = None
        if opt.get("res"):
            rsp = osp if opt["res"] == "full" else tuple(osp[:-2]) + (osp[-2] // 2, osp[-1] // 2)
            self.res0 = _rn(g, F_, *rsp, R.pad8(cout)).to(dtype)
        cp = R.pad8(cout)
        dy = _rn(g, F_, *osp, cp)
        dy[..., cout:] = 0                                  # zero pad columns, as the ABI promises
        if opt.get("window"):                               # a channel window of a wider poisoned buffer: not contiguous
            wide = _rn(g, F_, *osp, cp + 16) * POISON
            wide[..., 8:8 + cp] = dy
            self.dy = wide.to(dtype)[..., 8:8 + cp]
            assert not self.dy.is_contiguous()
        else:
            self.dy = dy.to(dtype)
        self.partner = None
        self.pack = K.PackedConv(dtype, cout, cin, ks, DEV, single_fill=True)
        self.pack.wants = set()
        self.sigma = self.u = self.v = None
        if sn:
            u, v = _rn(g, cout), _rn(g, fan)
            self.u, self.v = u / u.norm(), v / v.norm()
            self.sigma = torch.empty(1, dtype=F32, device=DEV)
            K.sn_power_iter(self.w.data, self.u, self.v, self.sigma)
        self.pack.fill(self.w.data, self.sigma)
        self.w_eff = AR.w_from_pack(self.pack.wf, cin, ks)
        self.prefill = None

    def spec(self):
        from dvd_gan_amd import functional as Fn
        s = Fn.ConvSpec(self.ks, self.cout, self.cin, act=self.act, up2=self.up2, relu_in=self.relu_in,
                        sn=(self.u, self.v) if self.sn_on else None)
        s.sigma, s.pack = self.sigma, self.pack
        return s

    def refs(self, y, partner=None):
        res_up2 = None if self.res0 is None else self.opt["res"] == "half"
        return AR.conv_backward_ref(self.x0, self.w_eff, y, self.dy, self.ks, self.dtype, act=self.act, up2=self.up2,
                                    relu_in=self.relu_in, partner=partner, unfused=self.opt.get("unfused", False), res_up2=res_up2,
                                    sn=(self.w.data, self.u, self.v, self.sigma) if self.sn_on else None)


def run(ly, log, direct, live="xwb", slot_main=None):
    """One forward + backward of the layer through Fn.Conv.apply and the autograd engine -> everything the checks need.
    live: which of x, w, b require a gradient (a frozen w / b is handed over detached, as SpectralNormConv does);
    slot_main: None, or fn(x, tok, slot) -> (tensor, its gradient) standing in for the main branch of a GradSlot pair."""
    from dvd_gan_amd import functional as Fn
    x = ly.x0.clone().requires_grad_("x" in live)
    res = ly.res0.clone().requires_grad_(True) if ly.res0 is not None else None
    w, b = ly.w, ly.b
    w.grad = b.grad = None
    o = SimpleNamespace(x=x, res=res, direct=direct, live=live, pre_w=None, pre_b=None, prev=Fn._SIDE["on"])
    if direct:
        o.pre_w, o.pre_b = ly.prefill[0].clone(), ly.prefill[1].clone()
        w.grad, b.grad = o.pre_w.clone(), o.pre_b.clone()
    wa, ba = (w if "w" in live else w.detach()), (b if "b" in live else b.detach())
    try:
        Fn.direct_weight_grads(direct)
        log.take()
        slot = Fn.GradSlot() if slot_main is not None else None

        def forward():
            out = Fn.Conv.apply(x, wa, ba, res, ly.spec(), slot)
            o.y_out, o.tok = out if slot is not None else (out, None)
            o.y = o.y_out.detach()
        _, o.var_fwd = _variants(forward)
        o.fwd = log.take()
        outs, gouts = [o.y_out], [ly.dy]
        if slot is not None:
            m, gm = slot_main(x, o.tok, slot)
            outs.append(m)
            gouts.append(gm)
        inputs = [t for t, on in ((x, "x" in live), (w, "w" in live), (b, "b" in live), (res, res is not None)) if on]

        def backward(retain=False):
            grads = torch.autograd.grad(outs, inputs, gouts, allow_unused=True, retain_graph=retain)
            got = dict(zip([n for n, on in (("dx", "x" in live), ("dw", "w" in live), ("db", "b" in live), ("dres", res is not None)) if on],
                           grads))
            for n in ("dx", "dw", "db", "dres"):
                setattr(o, n, got.get(n))
        o.backward, o.slot = backward, slot
        box = {}
        o.wgrad_families = profiled(lambda: box.update(v=_variants(lambda: backward(retain=slot is not None))[1]))
        o.var_bwd = box["v"]
        o.bwd = log.take()
        o.side = Fn.side_stream_if_any()
        o.grad_w, o.grad_b = w.grad, b.grad
    finally:
        Fn.direct_weight_grads(o.prev)
        Fn.join_side()
    torch.cuda.synchronize()
    return o


def check_forward_y(name, ly, o, log):
    """check 2: the stored y through conv_ref.check_forward (the fp32 output of the same request from the unwrapped kernel call)"""
    ru = ly.res0 is not None and ly.opt["res"] == "half"
    y32 = log.orig["conv_forward"](ly.x0, ly.pack.wf, ly.ks, ly.cout, bias=ly.b.data, res=ly.res0, act=ly.act, up2=ly.up2,
                                   relu_in=ly.relu_in, res_up2=ru, out_f32=True, wq=lambda: ly.pack.fragment_major("wf"))
    assert o.y.dtype == ly.dtype and o.y.is_contiguous() and o.y.shape[-1] == R.pad8(ly.cout)
    return R.check_forward(f"{name} y", ly.dtype, ly.x0, ly.w_eff, y32, o.y, bias=ly.b.data, res=ly.res0, res_up2=ru, act=ly.act,
                           up2=ly.up2, relu_in=ly.relu_in)


def check_route(name, ly, o):
    """check 1: the route of backward() from the call log"""
    from dvd_gan_amd import functional as Fn
    opt, live = ly.opt, o.live
    by = lambda n: [c for c in o.bwd if c.name == n]
    convs, pools, acts, wgs, cols, sns = (by(n) for n in LOGGED)
    fwd_convs = [c for c in o.fwd if c.name == "conv_forward"]
    assert len(fwd_convs) == 1 and len(o.fwd) == 1, [c.name for c in o.fwd]
    dy_in = None                                           # the dy' every later launch must read
    if ly.act != R.ACT_NONE:
        assert len(acts) == 1 and acts[0].a[2] == ly.act and _same(acts[0].a[1], o.y), f"{name}: act_backward(dy, stored y, act)"
        assert acts[0].a[0].is_contiguous() and torch.equal(acts[0].a[0], ly.dy)
        dy_in = acts[0].out
    else:
        assert not acts
    reads_dy = lambda t: (t is dy_in) if dy_in is not None else (t.is_contiguous() and torch.equal(t, ly.dy))
    mask_ok = lambda c: _same(c.kw.get("mask"), o.x) if ly.relu_in else c.kw.get("mask") is None
    route = []
    if "x" not in live:
        assert not convs and not (pools and opt.get("res") != "half"), f"{name}: a backward-data launch without a gradient for x"
        route.append("no backward-data")
    elif ly.up2 and not opt.get("unfused"):
        assert len(convs) == 1 and convs[0].kw.get("pool2") is True and convs[0].out is not None, f"{name}: one fused pool2 conv"
        assert mask_ok(convs[0]) and not pools and reads_dy(convs[0].a[0]) and _same(convs[0].a[1], ly.pack.wd)
        route.append("conv_forward(pool2)")
    elif ly.up2:
        assert len(convs) == 2 and convs[0].kw.get("pool2") is True and convs[0].out is None, f"{name}: pool2 refused first"
        assert not convs[1].kw.get("pool2") and convs[1].kw.get("mask") is None and reads_dy(convs[1].a[0])
        assert len(pools) == 1 and pools[0].a[0] is convs[1].out and pools[0].kw.get("scale") == 1.0 and _same(pools[0].kw.get("mask"), o.x)
        assert _same(convs[1].a[1], ly.pack.wd)
        route.append("conv_forward + pool(scale=1, mask=x)")
    else:
        assert len(convs) == 1 and not convs[0].kw.get("pool2") and mask_ok(convs[0]) and reads_dy(convs[0].a[0])
        assert _same(convs[0].a[1], ly.pack.wd) and convs[0].a[3] == R.pad8(ly.cin)
        if o.slot is not None:
            assert _same(convs[0].kw.get("res"), ly.partner), f"{name}: the partner is the backward-data conv's residual"
        else:
            assert convs[0].kw.get("res") is None
        route.append("conv_forward(mask=x)" if ly.relu_in else "conv_forward(res=partner)" if o.slot is not None else "conv_forward")
    if opt.get("res") == "half":
        rp = [c for c in pools if c.kw.get("mask") is None]
        assert len(rp) == 1 and reads_dy(rp[0].a[0]) and rp[0].kw.get("scale") == 1.0 and rp[0].a[1] == 1, f"{name}: dres = pool(dy, scale=1)"
        route.append("dres = pool(dy, scale=1)")
    elif opt.get("res") == "full":
        assert len(pools) == 0
    # ---- parameter gradients
    cur = torch.cuda.current_stream()
    if "w" in live:
        assert len(wgs) == 1 and not cols
        c = wgs[0]
        assert _same(c.a[0], o.x) and reads_dy(c.a[1]), f"{name}: conv_wgrad(x, dy')"
        assert c.kw.get("up2", False) == ly.up2 and c.kw.get("relu_in", False) == ly.relu_in
        if o.direct:
            assert o.side is not None and c.stream == o.side and c.stream != cur, f"{name}: weight gradients on the side stream"
            assert _same(c.kw.get("dbias"), o.grad_b) == ("b" in live)
            if ly.sn_on:
                assert c.kw.get("overwrite") is True and not _same(c.a[2], o.grad_w), f"{name}: overwrite into a fresh buffer"
                assert len(sns) == 1 and sns[0].a[0] is c.a[2] and _same(sns[0].kw.get("out"), o.grad_w) and sns[0].stream == o.side
                assert _same(sns[0].a[1], ly.w) and sns[0].a[2] is ly.u and sns[0].a[3] is ly.v and sns[0].a[4] is ly.sigma
                route.append("side: conv_wgrad(overwrite) + sn_backward(out=.grad)")
            else:
                assert _same(c.a[2], o.grad_w) and not c.kw.get("overwrite") and not sns
                route.append("side: conv_wgrad(.grad)")
            assert o.dw is None and o.db is None, f"{name}: the direct route returns no dw / db"
        else:
            assert c.stream == cur and not c.kw.get("overwrite")
            if ly.sn_on:
                assert len(sns) == 1 and sns[0].a[0] is c.a[2] and sns[0].kw.get("out") is None and sns[0].stream == cur
                assert _same(sns[0].a[1], ly.w) and sns[0].a[2] is ly.u and sns[0].a[3] is ly.v and sns[0].a[4] is ly.sigma
                route.append("conv_wgrad + sn_backward")
            else:
                assert not sns
                route.append("conv_wgrad")
    elif "b" in live:
        assert not wgs and not sns and len(cols) == 1 and reads_dy(cols[0].a[0]) and cols[0].a[1] == ly.cout
        route.append("colsum")
    else:
        assert not wgs and not sns and not cols
        route.append("no parameter gradient")
    return " | ".join(route)


def check_outputs(name, ly, o, refs):
    """checks 3 and 4"""
    live = o.live
    if "x" in live:
        assert o.dx.dtype == ly.dtype and o.dx.shape == ly.x0.shape and o.dx.is_contiguous()
        assert bool((o.dx[..., ly.cin:] == 0).all())
    else:
        assert o.dx is None
    if ly.res0 is not None:
        assert o.dres.dtype == ly.dtype and o.dres.shape == ly.res0.shape
        if ly.opt["res"] == "full":
            assert torch.equal(gru_ref.bits(o.dres), gru_ref.bits(ly.dy)), f"{name}: dres is dy bit for bit"
        else:
            assert o.dres.is_contiguous()
    dw = db = pw = pb = None
    if "w" in live:
        dw, pw = (o.grad_w, o.pre_w) if o.direct else (o.dw, None)
        assert dw.shape == ly.w.shape and dw.is_contiguous()
    if "b" in live:
        if o.direct and "w" in live:
            db, pb = o.grad_b, o.pre_b
        else:
            db = o.db                                       # (a live bias under a frozen weight comes back through autograd: colsum)
        assert db.shape == ly.b.shape
    return AR.check_backward(name, refs, dx=o.dx, dres=o.dres, dw=dw, db=db, dw_prefill=pw, db_prefill=pb)


def full_check(name, ly, log, live="xwb", routes=(False, True)):
    """Both routes of one layer: checks 1-5; returns {route: run}."""
    runs, refs = {}, None
    for direct in routes:
        label = f"{name} {'direct' if direct else 'autograd'}"
        if direct and ly.prefill is None:                   # random values of the gradient's own size
            g = torch.Generator(device=DEV).manual_seed(99)
            ref_w = refs["dw"][0].abs().mean().float()
            ref_b = refs["db"][0].abs().mean().float()
            ly.prefill = (_rn(g, *ly.w.shape) * ref_w, _rn(g, ly.cout) * ref_b)
        o = runs[direct] = run(ly, log, direct, live)
        print(f"ROUTE {label}: {check_route(label, ly, o)}")
        print(f"VARIANT {label}: forward {sorted(o.var_fwd)} backward-data {sorted(o.var_bwd)} wgrad families {o.wgrad_families}")
        want = CASES[ly.case][6]
        if ly.dtype == BF and want is not None:
            assert o.var_fwd == {want[0]}, (label, sorted(o.var_fwd))
            if want[1] is not None and "x" in live:
                assert o.var_bwd == {want[1]}, (label, sorted(o.var_bwd))
        if refs is None:
            check_forward_y(label, ly, o, log)
            refs = ly.refs(o.y)
        else:
            assert torch.equal(gru_ref.bits(o.y), gru_ref.bits(runs[routes[0]].y))
        check_outputs(label, ly, o, refs)
    if len(runs) == 2 and "x" in live:                      # check 5
        assert torch.equal(gru_ref.bits(runs[False].dx), gru_ref.bits(runs[True].dx)), f"{name}: dx bits differ between the routes"
    return runs, refs


PARAMS = [(c, d, s) for c in CASES if not CASES[c][5].get("slot") for d in (F32, BF) for s in (False, True)]


@pytest.mark.parametrize("case,dtype,sn", PARAMS, ids=[f"{c}-{NAMES[d]}-{'sn' if s else 'plain'}" for c, d, s in PARAMS])
def test_conv_routes(case, dtype, sn, monkeypatch):
    log = Log(monkeypatch)
    ly = Layer(case, dtype, sn)
    name = f"{case} {NAMES[dtype]} {'sn' if sn else 'plain'}"
    live = CASES[case][5].get("live", "xwb")
    if live == "xwb":
        full_check(name, ly, log)
        return
    # frozen / bias-only / no-dx: the trainable run of the same operands first (it supplies the prefill scale and dx)
    base, refs = full_check(f"{name} (trainable)", ly, log, routes=(False,))
    for direct in (False, True):
        label = f"{name} {'direct' if direct else 'autograd'}"
        if ly.prefill is None:
            g = torch.Generator(device=DEV).manual_seed(99)
            ly.prefill = (_rn(g, *ly.w.shape) * refs["dw"][0].abs().mean().float(), _rn(g, ly.cout) * refs["db"][0].abs().mean().float())
        o = run(ly, log, direct, live)
        print(f"ROUTE {label}: {check_route(label, ly, o)}")
        check_outputs(label, ly, o, refs)
        if "x" in live:
            assert torch.equal(gru_ref.bits(o.dx), gru_ref.bits(base[False].dx)), f"{label}: dx bits depend on the requested gradients"
        if direct:                                          # nothing was asked of the weight: its prefilled .grad is untouched
            if "w" not in live:
                assert torch.equal(ly.w.grad, o.pre_w)
            if "b" not in live or "w" not in live:
                assert torch.equal(ly.b.grad, o.pre_b)


# ------------------------------------------------------------------ the GradSlot partner sum
@pytest.mark.parametrize("sn", [False, True], ids=["plain", "sn"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_slot_partner_sum(dtype, sn, monkeypatch):
    """slot: 2 frames of 16 x 16, 64 -> 72, 1 x 1, slot=GradSlot().  A test-local Function stands in for the main branch: it takes
    x and the token, its backward leaves a known stored tensor in slot.dx and returns no gradient for x.  The shortcut's dx must be
    the float64 sum of its own backward-data result and that partner within the bound with ONE rounding; afterwards slot.dx is None;
    a second backward over the retained graph gives the same dx."""
    log = Log(monkeypatch)
    ly = Layer("slot", dtype, sn)
    g = torch.Generator(device=DEV).manual_seed(5)
    ly.partner = _rn(g, *ly.x0.shape).to(dtype)
    ly.partner[..., ly.cin:] = 0
    ran = []

    class Main(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, tok, slot):
            ctx.slot = slot
            return x.new_zeros(3)

        @staticmethod
        def backward(ctx, gm):
            ran.append(1)
            ctx.slot.dx = ly.partner
            return None, None, None

    main = lambda x, tok, slot: (Main.apply(x, tok, slot), torch.ones(3, device=DEV, dtype=dtype))
    name = f"slot {NAMES[dtype]} {'sn' if sn else 'plain'}"
    refs = None
    dxs = []
    for direct in (False, True):
        label = f"{name} {'direct' if direct else 'autograd'}"
        if direct:
            gp = torch.Generator(device=DEV).manual_seed(99)
            ly.prefill = (_rn(gp, *ly.w.shape) * refs["dw"][0].abs().mean().float(), _rn(gp, ly.cout) * refs["db"][0].abs().mean().float())
        o = run(ly, log, direct, slot_main=main)
        assert o.tok.numel() == 0 and ran and o.slot.dx is None
        print(f"ROUTE {label}: {check_route(label, ly, o)}")
        print(f"VARIANT {label}: forward {sorted(o.var_fwd)} backward-data {sorted(o.var_bwd)}")
        if refs is None:
            check_forward_y(label, ly, o, log)
            refs = ly.refs(o.y, partner=ly.partner)
        check_outputs(label, ly, o, refs)
        dxs.append(o.dx)
        if not direct:                                      # once more over the retained graph
            n = len(ran)
            o.backward(retain=False)
            torch.cuda.synchronize()
            assert len(ran) == n + 1 and o.slot.dx is None
            assert torch.equal(gru_ref.bits(o.dx), gru_ref.bits(dxs[0])), f"{label}: the second backward gives another dx"
    assert torch.equal(gru_ref.bits(dxs[0]), gru_ref.bits(dxs[1]))


@pytest.mark.parametrize("stamped", [False, True], ids=["main-pruned", "main-ran"])
def test_slot_without_partner(stamped, monkeypatch):
    """slot.dx is None when the shortcut's backward runs.  The main node did not run in this pass (nothing stamped the slot: the
    pruned graphs of tests/test_gpu_modules.py): legitimate, dx is the shortcut's own term, held to the same bound.  The main node
    DID run in this pass (it stamped slot.task with the graph task id, as CondBatchNorm.backward does) and its dx is gone: Conv.backward
    raises instead of returning a gradient that silently lacks a term."""
    log = Log(monkeypatch)
    ly = Layer("slot", F32, False)

    class Main(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, tok, slot):
            ctx.slot = slot
            return x.new_zeros(3)

        @staticmethod
        def backward(ctx, gm):
            if stamped:
                ctx.slot.task = torch._C._current_graph_task_id()
            return None, None, None

    main = lambda x, tok, slot: (Main.apply(x, tok, slot), torch.ones(3, device=DEV))
    if stamped:
        with pytest.raises(RuntimeError, match="GradSlot"):
            run(ly, log, False, slot_main=main)
        torch.cuda.synchronize()
        return
    o = run(ly, log, False, slot_main=main)
    assert [c.kw.get("res") for c in o.bwd if c.name == "conv_forward"] == [None]
    check_outputs("slot fp32 plain, main pruned", ly, o, ly.refs(o.y))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cout,up", [(64, 1), (32, 2)])
def test_gresblock_slot_against_two_leaf_copies(cout, up, dtype):
    """GResBlock(64, cout, 12, up) on 2 frames of 8 x 8: run() (the slot path) against the same five layers composed by hand, without
    slot or token, on two leaf copies x_a (shortcut) and x_b (main) of the input; both start from the same parameters, u, v and
    running statistics.  Every parameter gradient is torch.equal (the weight-gradient kernels are fixed-order or one atomic per
    element; the slot changes only where dx is summed).  Exact mode: x.grad is torch.equal to x_a.grad + x_b.grad.  bf16: the slot
    path stores r(S + m), the hand path r(S) and m (S the shortcut's fp32 backward-data sum, m the main branch's stored dx), so
    |x.grad - (x_a.grad + x_b.grad)| <= half a bf16 ulp of x_a.grad + half a bf16 ulp of the sum, element by element."""
    from dvd_gan_amd import functional as Fn
    from dvd_gan_amd.gen_net import GResBlock
    torch.manual_seed(11)
    blk = GResBlock(64, cout, 12, up).to(DEV).train()
    hand = copy.deepcopy(blk)
    g = torch.Generator(device=DEV).manual_seed(12)
    x0 = _rn(g, 2, 8, 8, 64).to(dtype)
    cond = _rn(g, 2, 12)
    samp = torch.arange(2, dtype=torch.int32, device=DEV)
    S = 8 * up
    gy = _rn(g, 2, S, S, R.pad8(cout)).to(dtype)
    prev = Fn._SIDE["on"]
    try:
        Fn.direct_weight_grads(False)
        x = x0.clone().requires_grad_(True)
        y = blk.run(x, cond, samp)
        y.backward(gy)
        xa, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        skip = hand.conv_sc(xa)
        a1 = hand.CBNorm1(xb, cond, samp, relu=True)
        c0 = hand.conv0(a1, up2=up != 1)
        a2 = hand.CBNorm2(c0, cond, samp, relu=True)
        yh = hand.conv1(a2, res=skip)
        yh.backward(gy)
    finally:
        Fn.direct_weight_grads(prev)
        Fn.join_side()
    torch.cuda.synchronize()
    assert torch.equal(gru_ref.bits(y), gru_ref.bits(yh))
    for (n, p), (_, q) in zip(blk.named_parameters(), hand.named_parameters()):
        if p.requires_grad:
            assert p.grad is not None and torch.equal(p.grad, q.grad), f"{n}: the slot path changed a parameter gradient"
    assert x.grad.dtype == dtype and x.grad.shape == x0.shape
    if dtype == F32:
        assert torch.equal(x.grad, xa.grad + xb.grad)
    else:
        total = xa.grad.double() + xb.grad.double()
        allowed = 0.5 * AR.ulp(xa.grad.double(), BF) + 0.5 * AR.ulp(torch.maximum(total.abs(), x.grad.double().abs()), BF)
        err = (x.grad.double() - total).abs()
        gru_ref.note(f"gresblock {cout} up{up} bf16 worst err / allowed", float((err / allowed.clamp_min(1e-300)).max()))
        assert bool((err <= allowed).all())


# ------------------------------------------------------------------ LinearF32 / Embedding on both routes
def _rel_terms(out, ref, mag):
    """worst |out - ref| / sum |terms| (the form tests/test_gpu_pointwise.py holds these kernels to: <= 1e-6)"""
    return float(((out.double() - ref).abs() / mag).max())


@pytest.mark.parametrize("direct", [False, True], ids=["autograd", "direct"])
def test_linear_f32_routes(direct):
    from dvd_gan_amd import functional as Fn
    B, Kk, J = 5, 120, 136
    g = torch.Generator(device=DEV).manual_seed(21)
    x = _rn(g, B, Kk).requires_grad_(True)
    W, b = nn.Parameter(_rn(g, J, Kk) * 0.1), nn.Parameter(_rn(g, J))
    dout = _rn(g, B, J)
    pw, pb = _rn(g, J, Kk), _rn(g, J)
    if direct:
        W.grad, b.grad = pw.clone(), pb.clone()
    prev = Fn._SIDE["on"]
    try:
        Fn.direct_weight_grads(direct)
        y = Fn.LinearF32.apply(x, W, b)
        din, dW, db = torch.autograd.grad([y], [x, W, b], [dout], allow_unused=True)
    finally:
        Fn.direct_weight_grads(prev)
        Fn.join_side()
    torch.cuda.synchronize()
    x64, W64, d64 = x.detach().double(), W.detach().double(), dout.double()
    e = _rel_terms(y.detach(), x64 @ W64.t() + b.detach().double(), x64.abs() @ W64.abs().t() + b.detach().double().abs())
    e = max(e, _rel_terms(din, d64 @ W64, d64.abs() @ W64.abs()))
    if direct:
        assert dW is None and db is None
        e = max(e, _rel_terms(W.grad.double() - pw.double(), d64.t() @ x64, d64.abs().t() @ x64.abs() + pw.double().abs()))
        e = max(e, _rel_terms(b.grad.double() - pb.double(), d64.sum(0), d64.abs().sum(0) + pb.double().abs()))
    else:
        assert W.grad is None and b.grad is None
        e = max(e, _rel_terms(dW, d64.t() @ x64, d64.abs().t() @ x64.abs()), _rel_terms(db, d64.sum(0), d64.abs().sum(0)))
    gru_ref.note(f"LinearF32 {'direct' if direct else 'autograd'} err / sum|terms|", e)
    assert e <= 1e-6


@pytest.mark.parametrize("direct", [False, True], ids=["autograd", "direct"])
def test_embedding_routes(direct):
    from dvd_gan_amd import functional as Fn
    rows, D = 11, 96
    g = torch.Generator(device=DEV).manual_seed(22)
    W = nn.Parameter(_rn(g, rows, D))
    idx = torch.tensor([3, 0, 7, 3, 10, 5, 1], dtype=torch.int32, device=DEV)      # 7 indices, row 3 twice
    dout = _rn(g, 7, D)
    pw = _rn(g, rows, D)
    if direct:
        W.grad = pw.clone()
    prev = Fn._SIDE["on"]
    try:
        Fn.direct_weight_grads(direct)
        y = Fn.Embedding.apply(W, idx)
        dW, = torch.autograd.grad([y], [W], [dout], allow_unused=True)
    finally:
        Fn.direct_weight_grads(prev)
        Fn.join_side()
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), W.detach()[idx.long()])
    ref = torch.zeros(rows, D, dtype=torch.float64, device=DEV).index_add(0, idx.long(), dout.double())
    mag = torch.zeros(rows, D, dtype=torch.float64, device=DEV).index_add(0, idx.long(), dout.double().abs())
    absent = torch.ones(rows, dtype=torch.bool, device=DEV)
    absent[idx.long()] = False
    if direct:
        assert dW is None
        got, mag = W.grad.double() - pw.double(), mag + pw.double().abs()
        assert torch.equal(W.grad[absent], pw[absent])
    else:
        assert W.grad is None
        got = dW
        assert bool((dW[absent] == 0).all())
    e = float(((got.double() - ref).abs() / mag.clamp_min(1e-300)).max())
    gru_ref.note(f"Embedding {'direct' if direct else 'autograd'} err / sum|terms|", e)
    assert e <= 1e-6

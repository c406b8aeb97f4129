"""The ConvGRU entry points (dvd_convgru_layer_forward / _backward, dvd_convgru_stack_forward / _backward; gru.hip and the gate
epilogues of conv_common.h) called through ctypes and checked STEP BY STEP against float64 (tests/gru_ref.py): every tensor a
pass stores is recomputed from the stored tensors of that step and of the step before and held to an elementwise error model
plus half an ulp of the storage type, so storage rounding never compounds and a fault of one bf16 ulp in one gate shows.

The operands are built as functional.ConvGRULayer / ConvGRUStack build them (kern.PackedConv, fragment_major), the descriptors
(lib.GruDesc, lib.GruStackDesc) are filled directly.  Every output buffer, the workspace, the carry and the tickets are carved
from one arena with sentinel gaps between them; outputs, workspace and carry start as NaN (a kernel must write all it reads, an
element left unwritten fails its check); after every call the sentinels must be intact and the tickets zero.  Where a case names a
kernel family, the per-launch records of the library (dvd_prof_enable / dvd_prof_report_variants, enabled around that call
only) must show it; within the halo family the records cannot tell weights-from-LDS from weights-from-L2: the supplied
fragment-major image selects the latter (conv_igemm.hip: dvd_conv_forward_gru), so those cases run with and without it.

Routes: (a) tickets = NULL -- slabs + gate kernels at the policy's split-K factors; (b) tickets, combine_max = 8 -- everything
combined in-launch, run twice, bit-equal; (c) ns_cap = 1 -- fused epilogue, unsplit; (d) the library's defaults.

The wavefront (section "stack"): every layer goes through the same checker; for l >= 1 gx_l[t] is held against conv64(h_{l-1}[t]
stored, Wx_l) + b and dh_mid[l][t] against convT64(dg_l[t] stored, Wx_l) + dh_out_{l-1}[t]; layer l-1's reference takes the STORED
dh_mid[l] as its incoming gradient.  That sum is formed in fp32 -- (acc + bias) + res in the direct epilogue of conv_common.h,
which gru.hip reaches by handing layer[l-1].dh_out to the x-part backward-data member as its residual -- and rounded once, at the
bf16 store of dh_mid.

profiles/gru_parity_numbers.md has the measured maxima and the mutants this file was run against.
"""
import ctypes as C
import math

import pytest
import torch

import gru_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NV = 12
SENT = 0xA5
GAP = 512

#        B, H, W, hidden, k, T
CASES = {
    1: (5, 4, 4, 24, 3, 3),         # M = 80 < one tile; u|r boundary (column 24) inside a 32-column fragment
    2: (64, 4, 4, 40, 5, 3),        # pixel-major rows, out-of-frame filter rows skipped; ragged N (80)
    3: (3, 8, 8, 72, 3, 3),         # ragged K chunk (72 = 2 * 32 + 8), two N tiles, the second ragged; boundary at column 72
    4: (32, 8, 8, 136, 5, 3),       # three N tiles, pixel-major
    5: (2, 16, 16, 24, 5, 3),       # one K chunk: the halo kernel serves it only unsplit
    6: (3, 16, 16, 64, 3, 3),       # halo 128-row tiles, weights from LDS / from L2
    7: (32, 64, 64, 64, 3, 2),      # 512 tiles, unsplit: halo 256-row for u|r, the thin 256 x 64 tile for the out gate and d(hr)
    8: (1024, 8, 8, 128, 3, 2),     # the 8-wave 256 x 256 tile with a gate epilogue (cv_choose_kernel wants t256 >= 256)
    9: (5, 6, 6, 24, 3, 3),         # division indexing
    10: (2, 6, 12, 24, 3, 3),       # division indexing, H != W
    11: (2, 8, 16, 40, 3, 3),       # H != W with shift indexing
}
ROUTES = {"a": dict(tickets=False, combine_max=0, ns_cap=0), "b": dict(tickets=True, combine_max=8, ns_cap=0),
          "c": dict(tickets=False, combine_max=0, ns_cap=1), "d": dict(tickets=True, combine_max=0, ns_cap=0)}
ALL4 = {r: {4} for r in "abcd"}
# kernel variants (dvd_prof_report_variants, kind 0) a (case, fragment-major images supplied) must show per route:
# 1 / 2 / 3 = halo 256 x 128 / 128 x 128 / 256 x 64, 4 = tap-by-tap 128-row, 6 = 8-wave 256 x 256, 8 = whole-frame 128-row tiles
# (4 x 4 frames are always recorded as 8).  The whole-frame and halo kernels take a split only over channel chunks
# (cv_choose_kernel), so under the policy's factors these narrow layers stay on the tap-by-tap kernel and reach them unsplit (route c).
FAMILY = {(1, False): ALL4, (1, True): {"c": {8}}, (2, False): ALL4, (2, True): {"c": {8}}, (3, False): ALL4, (3, True): {"c": {8}},
          (4, False): ALL4, (4, True): {"c": {8}}, (5, False): {"a": {4}, "c": {2}}, (5, True): {"a": {4}, "c": {2}},
          (6, False): {"c": {2}}, (6, True): {"c": {2}}, (7, False): {r: {1, 3} for r in "abcd"}, (7, True): {r: {1, 3} for r in "abcd"},
          (8, False): {"c": {6}}, (9, False): ALL4, (10, False): ALL4, (11, False): ALL4}
NAMES = {torch.bfloat16: "bf16", torch.float32: "fp32"}


def _lib():
    from dvd_gan_amd import lib as L
    return L, L.lib()


class Arena:
    """Buffers carved from ONE allocation, 512 sentinel bytes in front of, between and behind them."""

    def __init__(self, specs):
        offs, n = {}, GAP
        for name, shape, dtype, _ in specs:
            nb = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
            offs[name] = (n, nb)
            n += (nb + 255) // 256 * 256 + GAP
        self.raw = torch.full((n,), SENT, dtype=torch.uint8, device=DEV)
        self.gap = torch.ones(n, dtype=torch.bool, device=DEV)
        self.t = {}
        for name, shape, dtype, fill in specs:
            o, nb = offs[name]
            self.gap[o:o + nb] = False
            self.t[name] = self.raw[o:o + nb].view(dtype).view(shape)
            self.t[name].fill_(fill)

    def intact(self):
        return bool((self.raw[self.gap] == SENT).all())


class Layer:
    """Operands of one layer: storage-rounded inputs and master weights, the packs built from the same masters."""

    def __init__(self, case, dtype, regime="typical", shared=False, seed=0):
        from dvd_gan_amd import kern as K
        self.case, self.dtype = case, dtype
        B, H, W, h, k, T = CASES[case]
        g = torch.Generator(device=DEV).manual_seed(1000 * case + seed)
        rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
        wu, wr, wo = (rn(h, h, k, k) / (h * k * k) ** 0.5 for _ in range(3))
        gx = rn(1 if shared else T, B, H, W, 3 * h)
        if regime == "small_o":
            wo = wo * 3e-3
            gx[..., 2 * h:] *= 3e-3
        if regime == "saturated":
            gx *= 6.0
        self.gx = gx.to(dtype)
        self.h0 = (rn(B, H, W, h) * 0.5).to(dtype)
        self.dh_out = rn(T, B, H, W, h).to(dtype)
        self.pur = K.PackedConv(dtype, 2 * h, h, (k, k), DEV, covered=True).fill(wu.contiguous(), co_off=0).fill(wr.contiguous(), co_off=h)
        self.po = K.PackedConv(dtype, h, h, (k, k), DEV, covered=True).fill(wo.contiguous())
        self.w_ur, self.w_o = torch.cat([wu, wr]).to(dtype), wo.to(dtype)       # what the packs hold, for the reference


def _ns(dtype, M, Cout, Cin, taps, cap):
    L, lib = _lib()
    ns = lib.dvd_conv_pick_nsplit(L.BF16 if dtype == torch.bfloat16 else L.F32, C.c_longlong(M), Cout, Cin, taps)
    return min(ns, cap) if cap > 0 else ns


def _drain(lib):
    n = (C.c_longlong * NV)()
    lib.dvd_prof_report_variants.restype = C.c_longlong
    lib.dvd_prof_report_variants(0, NV, n, None, None)
    return {v for v in range(1, NV) if n[v] > 0}


def run_layer(ly, route, wq, *, h0=True, h32=True, infer=False, dh_out=True, dh0=True, backward=True):
    """One forward (+ backward) call on fresh NaN-filled buffers -> (tensors, kernel variants seen, carry_full)."""
    from dvd_gan_amd import kern as K
    L, lib = _lib()
    B, H, W, h, k, T = CASES[ly.case]
    dtype, M, taps = ly.dtype, B * H * W, k * k
    nan = float("nan")
    Ts = 1 if infer else T
    ws_n = lib.dvd_convgru_ws_floats(L.dt(ly.gx), B, H, W, h, k)
    specs = [("h_all", (T, B, H, W, h), dtype, nan), ("u_all", (Ts, B, H, W, h), dtype, nan), ("hr_all", (Ts, B, H, W, h), dtype, nan),
             ("r_all", (T, B, H, W, h), dtype, nan), ("o_all", (T, B, H, W, h), dtype, nan), ("h32", (2, M, h), torch.float32, nan),
             ("ws", (ws_n,), torch.float32, nan), ("dg", (T, B, H, W, 3 * h), dtype, nan), ("carry", (M, h), torch.float32, nan),
             ("dh0", (M, h), torch.float32, nan), ("tickets", (L.GRU_TICKETS,), torch.int32, 0)]
    ar = Arena(specs)
    t = ar.t
    use_h32 = h32 and dtype == torch.bfloat16
    cap = route["ns_cap"]
    d = L.GruDesc()
    d.dtype, d.T, d.B, d.H, d.W, d.hidden, d.k = L.dt(ly.gx), T, B, H, W, h, k
    d.gx_stride = 0 if ly.gx.shape[0] == 1 else M * 3 * h
    d.gx, d.w_ur, d.w_o = ly.gx.data_ptr(), ly.pur.wf.data_ptr(), ly.po.wf.data_ptr()
    d.wd_ur, d.wd_o = ly.pur.wd.data_ptr(), ly.po.wd.data_ptr()
    if wq:      # as functional.ConvGRULayer: the image goes to the convolutions whose kernel takes one
        if K.wants_fragment_major(dtype, B, H, W, h, 2 * h, k, _ns(dtype, M, 2 * h, h, taps, cap)):
            d.w_ur_q = ly.pur.fragment_major("wf").data_ptr()
        if K.wants_fragment_major(dtype, B, H, W, h, h, k, _ns(dtype, M, h, h, taps, cap)):
            d.w_o_q, d.wd_o_q = ly.po.fragment_major("wf").data_ptr(), ly.po.fragment_major("wd").data_ptr()
        if K.wants_fragment_major(dtype, B, H, W, 2 * h, h, k, _ns(dtype, M, h, 2 * h, taps, cap)):
            d.wd_ur_q = ly.pur.fragment_major("wd").data_ptr()
    d.h0 = ly.h0.data_ptr() if h0 else None
    d.h_all, d.u_all, d.hr_all = t["h_all"].data_ptr(), t["u_all"].data_ptr(), t["hr_all"].data_ptr()
    d.r_all = None if infer else t["r_all"].data_ptr()
    d.o_all = None if infer else t["o_all"].data_ptr()
    d.h32 = t["h32"].data_ptr() if use_h32 else None
    d.ws = t["ws"].data_ptr()
    d.dh_out = ly.dh_out.data_ptr() if dh_out else None
    d.dg, d.carry = t["dg"].data_ptr(), t["carry"].data_ptr()
    d.dh0 = t["dh0"].data_ptr() if dh0 else None
    d.infer = int(infer)
    d.tickets = t["tickets"].data_ptr() if route["tickets"] else None
    d.combine_max, d.ns_cap = route["combine_max"], cap
    torch.cuda.synchronize()
    _drain(lib)
    lib.dvd_prof_enable(1)
    try:
        L.check(lib.dvd_convgru_layer_forward(C.byref(d), L.stream()))
        torch.cuda.synchronize()
        assert ar.intact(), "forward wrote outside its buffers"
        assert int(t["tickets"].abs().sum()) == 0, "forward left tickets behind"
        if backward and not infer:
            L.check(lib.dvd_convgru_layer_backward(C.byref(d), L.stream()))
            torch.cuda.synchronize()
            assert ar.intact(), "backward wrote outside its buffers"
            assert int(t["tickets"].abs().sum()) == 0, "backward left tickets behind"
    finally:
        lib.dvd_prof_enable(0)
        seen = _drain(lib)
    nmax = 1 if not route["tickets"] else (route["combine_max"] or 4)
    carry_full = (not h0) or _ns(dtype, M, h, 2 * h, taps, cap) <= nmax
    out = dict(t)
    out.update(h0=ly.h0 if h0 else None, h32v=t["h32"] if use_h32 else None, dh_out=ly.dh_out if dh_out else None,
               dh0v=t["dh0"] if dh0 else None, arena=ar)
    return out, seen, carry_full


def check_layer(name, ly, o, carry_full, backward=True, stats=None):
    res = R.forward_ratios(name, ly.dtype, ly.gx, o["h0"], o["h_all"], o["u_all"], o["r_all"], o["o_all"], o["hr_all"], o["h32v"],
                           ly.w_ur, ly.w_o, stats)
    if backward:
        res.update(R.backward_ratios(name, ly.dtype, o["h0"], o["h_all"], o["u_all"], o["r_all"], o["o_all"], o["dh_out"], o["dg"],
                                     o["carry"], o["dh0v"], ly.w_ur, ly.w_o, carry_full))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, f"{name}: outside the bounds {bad}"
    return res


STORED = ("h_all", "u_all", "r_all", "o_all", "hr_all", "dg", "carry", "dh0")


def _params():
    out = []
    for c in CASES:
        for dtype in ([torch.bfloat16] if c in (7, 8) else [torch.bfloat16, torch.float32]):
            for wq in ([False, True] if dtype == torch.bfloat16 and (c, True) in FAMILY else [False]):
                out.append(pytest.param(c, dtype, wq, id=f"case{c}-{NAMES[dtype]}{'-wq' if wq else ''}"))
    return out


@pytest.mark.parametrize("case,dtype,wq", _params())
def test_layer_every_route(case, dtype, wq):
    ly = Layer(case, dtype)
    for rname in ("c",) if case == 8 else "abcd":
        name = f"layer case{case} {NAMES[dtype]}{' wq' if wq else ''} route {rname}"
        o, seen, full = run_layer(ly, ROUTES[rname], wq)
        need = FAMILY[(case, wq)].get(rname, set())
        assert need <= seen, f"{name}: kernel variants {sorted(need)} expected, the launches were {sorted(seen)}"
        check_layer(name, ly, o, full)
        if rname == "b":       # the in-launch combine gives the same bits whichever workgroup arrives last
            o2, _, _ = run_layer(ly, ROUTES[rname], wq)
            for k in STORED:
                assert torch.equal(R.bits(o[k]), R.bits(o2[k])), f"{name}: {k} is not reproducible"


@pytest.mark.parametrize("case,dtype,wq", [pytest.param(3, torch.bfloat16, False, id="case3-bf16"),
                                           pytest.param(3, torch.float32, False, id="case3-fp32"),
                                           pytest.param(4, torch.bfloat16, True, id="case4-bf16-wq")])
def test_layer_split_factor_sweep(case, dtype, wq):
    """slab_sum8's blocks of four and its tail (2, 3, 4, 5 and the policy's 8 slabs) and every in-launch combine count, on the
    tap-by-tap kernel (case 3) and the whole-frame 8 x 8 kernel (case 4 with the images; the policy's own factor exceeds its
    channel chunks, so ns_cap = 0 is served tap-by-tap there)."""
    ly = Layer(case, dtype)
    for cap in (2, 3, 4, 5, 0):
        for rname in "ab":
            route = dict(ROUTES[rname], ns_cap=cap)
            name = f"sweep case{case} {NAMES[dtype]}{' wq' if wq else ''} route {rname} ns_cap {cap}"
            o, seen, full = run_layer(ly, route, wq)
            assert (8 if (wq and cap) else 4) in seen, (name, sorted(seen))
            check_layer(name, ly, o, full)


OPTIONS = ["noh0", "noh32", "shared_gx", "infer", "nodhout", "nodh0"]


@pytest.mark.parametrize("opt", OPTIONS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [1, 3, 6])
def test_layer_options(case, dtype, opt):
    ly = Layer(case, dtype, shared=opt == "shared_gx")
    wq = dtype == torch.bfloat16
    for rname in "acd":
        name = f"option {opt} case{case} {NAMES[dtype]} route {rname}"
        kw = dict(h0=opt != "noh0", h32=opt != "noh32", dh_out=opt != "nodhout", dh0=opt != "nodh0")
        o, _, full = run_layer(ly, ROUTES[rname], wq, **kw)
        check_layer(name, ly, o, full)
        if opt == "nodhout":       # no gradient comes in: every dg written, finite and zero
            assert bool((o["dg"] == 0).all()), name
        if opt == "infer":         # same states as the training form; the one-step scratch holds the last step
            i, _, _ = run_layer(ly, ROUTES[rname], wq, infer=True, **kw)
            assert torch.equal(R.bits(i["h_all"]), R.bits(o["h_all"])), name
            assert torch.equal(R.bits(i["u_all"][0]), R.bits(o["u_all"][-1])), name
            assert torch.equal(R.bits(i["hr_all"][0]), R.bits(o["hr_all"][-1])), name
            assert bool(torch.isnan(i["r_all"].float()).all() and torch.isnan(i["o_all"].float()).all()), "r / o are not stored"


@pytest.mark.parametrize("regime", ["small_o", "saturated"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", [1, 3, 6])
def test_layer_input_regimes(case, dtype, regime):
    """small_o: |a_o| on both sides of the 2e-3 switch of gate_tanh<bf16_t>; saturated: gates within 1e-3 of 0 / 1, tanh near
    +-1 (the typical regime, pre-activations O(1), is every other test).  The float64 reference must contain what is claimed."""
    ly = Layer(case, dtype, regime=regime)
    wq = dtype == torch.bfloat16
    for rname in "acd":
        stats = {}
        o, _, full = run_layer(ly, ROUTES[rname], wq)
        check_layer(f"regime {regime} case{case} {NAMES[dtype]} route {rname}", ly, o, full, stats=stats)
        a = stats["a_o"].abs()
        if regime == "small_o":
            assert int((a < 2e-3).sum()) > 100 and int(((a >= 2e-3) & (a <= 0.1)).sum()) > 100
            assert int((a > 0.1).sum()) == 0
        else:
            u = stats["u"]
            assert int((u < 1e-3).sum()) > 100 and int((u > 1 - 1e-3).sum()) > 100
            assert int((stats["o"].abs() > 1 - 1e-3).sum()) > 100


# ------------------------------------------------------------------ the wavefront over a stack
STACKS = [   # T, B, S, hidden sizes, kernel sizes, shared input, supplied initial states
    pytest.param(5, 8, 4, [64, 64, 64], [3, 5, 3], True, (True, False, True), id="T5B8S4"),
    pytest.param(4, 4, 8, [64, 128, 64], [3, 5, 3], False, (False, True, True), id="T4B4S8"),
    pytest.param(3, 3, 16, [64, 64, 64], [3, 5, 3], False, (True, True, True), id="T3B3S16"),
    pytest.param(3, 2, 16, [64, 128, 64], [3, 5, 5], False, (False, False, False), id="T3B2S16wide"),
]


@pytest.mark.parametrize("T,B,S,hids,ks,shared,h0on", STACKS)
def test_stack_wavefront(T, B, S, hids, ks, shared, h0on):
    from dvd_gan_amd import kern as K
    L, lib = _lib()
    dtype, nl, M = torch.bfloat16, len(hids), B * S * S
    g = torch.Generator(device=DEV).manual_seed(77 + S)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    nan = float("nan")
    specs, lay = [("tickets", (L.GRU_TICKETS,), torch.int32, 0)], []
    for l, (h, k) in enumerate(zip(hids, ks)):
        wu, wr, wo = (rn(h, h, k, k) / (h * k * k) ** 0.5 for _ in range(3))
        e = dict(h=h, k=k, w_ur=torch.cat([wu, wr]).to(dtype), w_o=wo.to(dtype),
                 pur=K.PackedConv(dtype, 2 * h, h, (k, k), DEV, covered=True).fill(wu.contiguous()).fill(wr.contiguous(), co_off=h),
                 po=K.PackedConv(dtype, h, h, (k, k), DEV, covered=True).fill(wo.contiguous()),
                 h0=(rn(B, S, S, h) * 0.5).to(dtype) if h0on[l] else None, dh_out=rn(T, B, S, S, h).to(dtype))
        if l == 0:
            e["gx"] = rn(1 if shared else T, B, S, S, 3 * h).to(dtype)
        else:
            ci = hids[l - 1]
            wx = (rn(3 * h, ci, k, k) / (ci * k * k) ** 0.5).contiguous()
            e.update(ci=ci, wx=wx.to(dtype), bx=rn(3 * h) * 0.1, px=K.PackedConv(dtype, 3 * h, ci, (k, k), DEV, single_fill=True).fill(wx))
            specs += [(f"gx{l}", (T, B, S, S, 3 * h), dtype, nan), (f"dh_mid{l}", (T, B, S, S, ci), dtype, nan)]
        for nm in ("h_all", "u_all", "r_all", "o_all", "hr_all"):
            specs.append((f"{nm}{l}", (T, B, S, S, h), dtype, nan))
        specs += [(f"h32{l}", (2, M, h), torch.float32, nan), (f"dg{l}", (T, B, S, S, 3 * h), dtype, nan),
                  (f"carry{l}", (M, h), torch.float32, nan), (f"dh0{l}", (M, h), torch.float32, nan)]
        lay.append(e)
    sd = L.GruStackDesc()
    sd.n_layers, sd.layer_policy, sd.run = nl, 0, 0
    ar = Arena(specs)
    t = ar.t
    for l, e in enumerate(lay):
        h, k = e["h"], e["k"]
        d = sd.layer[l]
        d.dtype, d.T, d.B, d.H, d.W, d.hidden, d.k = L.BF16, T, B, S, S, h, k
        gx = e["gx"] if l == 0 else t[f"gx{l}"]
        d.gx_stride = 0 if gx.shape[0] == 1 else M * 3 * h
        d.gx, d.w_ur, d.w_o, d.wd_ur, d.wd_o = gx.data_ptr(), e["pur"].wf.data_ptr(), e["po"].wf.data_ptr(), e["pur"].wd.data_ptr(), e["po"].wd.data_ptr()
        d.w_ur_q, d.w_o_q = e["pur"].fragment_major("wf").data_ptr(), e["po"].fragment_major("wf").data_ptr()
        d.wd_ur_q, d.wd_o_q = e["pur"].fragment_major("wd").data_ptr(), e["po"].fragment_major("wd").data_ptr()
        d.h0 = e["h0"].data_ptr() if e["h0"] is not None else None
        d.h_all, d.u_all, d.r_all = t[f"h_all{l}"].data_ptr(), t[f"u_all{l}"].data_ptr(), t[f"r_all{l}"].data_ptr()
        d.o_all, d.hr_all, d.h32 = t[f"o_all{l}"].data_ptr(), t[f"hr_all{l}"].data_ptr(), t[f"h32{l}"].data_ptr()
        d.dh_out, d.dg, d.carry = e["dh_out"].data_ptr(), t[f"dg{l}"].data_ptr(), t[f"carry{l}"].data_ptr()
        d.dh0 = t[f"dh0{l}"].data_ptr() if e["h0"] is not None else None
        d.tickets = t["tickets"].data_ptr()
        if l > 0:
            sd.cin[l] = e["ci"]
            sd.wx[l], sd.wx_q[l], sd.bx[l] = e["px"].wf.data_ptr(), e["px"].fragment_major("wf").data_ptr(), e["bx"].data_ptr()
            sd.wdx[l], sd.wdx_q[l] = e["px"].wd.data_ptr(), e["px"].fragment_major("wd").data_ptr()
            sd.dh_mid[l] = t[f"dh_mid{l}"].data_ptr()
    ws = Arena([("ws", (lib.dvd_convgru_stack_ws_floats(C.byref(sd)),), torch.float32, nan)])
    sd.ws = ws.t["ws"].data_ptr()
    assert lib.dvd_convgru_stack_ok(C.byref(sd), 0) and lib.dvd_convgru_stack_ok(C.byref(sd), 1)
    dbg = (C.c_longlong * 2)()
    lib.dvd_debug_stack_ws(dbg, 1)
    torch.cuda.synchronize()
    for fn in (lib.dvd_convgru_stack_forward, lib.dvd_convgru_stack_backward):
        L.check(fn(C.byref(sd), L.stream()))
        torch.cuda.synchronize()
        assert ar.intact() and ws.intact(), "the wavefront wrote outside its buffers"
        assert int(t["tickets"].abs().sum()) == 0, "the wavefront left tickets behind"
    lib.dvd_debug_stack_ws(dbg, 1)
    assert dbg[0] == dbg[1], f"slab workspace sized {dbg[0]}, used {dbg[1]}"
    if ks == [3, 5, 5]:               # the wide case: members are split
        assert dbg[0] > 0, "the production plan splits no member of the wide stack"
    tag = f"stack T{T}B{B}S{S}h{'-'.join(map(str, hids))}"
    res = {}
    for l, e in enumerate(lay):
        gx = e["gx"] if l == 0 else t[f"gx{l}"]
        dh_in = e["dh_out"] if l == nl - 1 else t[f"dh_mid{l + 1}"]
        r = R.forward_ratios(f"{tag} layer{l}", dtype, gx, e["h0"], t[f"h_all{l}"], t[f"u_all{l}"], t[f"r_all{l}"], t[f"o_all{l}"],
                             t[f"hr_all{l}"], t[f"h32{l}"], e["w_ur"], e["w_o"])
        r.update(R.backward_ratios(f"{tag} layer{l}", dtype, e["h0"], t[f"h_all{l}"], t[f"u_all{l}"], t[f"r_all{l}"], t[f"o_all{l}"],
                                   dh_in, t[f"dg{l}"], t[f"carry{l}"], t[f"dh0{l}"] if e["h0"] is not None else None,
                                   e["w_ur"], e["w_o"], True))
        if l > 0:
            r["gx"] = max(R.conv_ratio(t[f"gx{l}"][s], t[f"h_all{l - 1}"][s], e["wx"], dtype, bias=e["bx"]) for s in range(T))
            r["dh_mid"] = max(R.conv_ratio(t[f"dh_mid{l}"][s], t[f"dg{l}"][s], e["wx"], dtype, res=lay[l - 1]["dh_out"][s], transposed=True)
                              for s in range(T))
            R.note(f"{tag} layer{l} gx err/bound", r["gx"])
            R.note(f"{tag} layer{l} dh_mid err/bound", r["dh_mid"])
        res.update({f"layer{l} {k}": v for k, v in r.items()})
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, f"{tag}: outside the bounds {bad}"

"""Orthogonal regularizer on the GPU: dvd_ortho_prepare / dvd_ortho_grad through ctypes, then FlatAdam and the Trainer.

Definition: M = W W^T with a zero diagonal, t = s * M W with s = fl(2 beta), R = 1/2 ||M||_F^2; the call does g = fl(g + fl(s acc)).
Yardstick: the fp64 restatement below on the STORED fp32 p.  Per item two bounds on t (the call into a zeroed g):
  (a) elementwise, rigorous for any summation order (gamma_n = n u / (1 - n u), u = 2^-24):
      |t - t64| <= s [gamma_{h+2} (|M| |W|) + gamma_w ((|W| |W|^T, zero diagonal) |W|)] + u |t64|
  (b) rel-L2(t - t64) <= M_RATIO x the rel-L2 error of THE SAME two products evaluated in fp32 on the CPU inside this file, on
      the same data -- measured here, never taken from the kernel.  M_RATIO = twice the largest ratio measured on an MI355X,
      rounded up (profiles/ortho_parity_numbers.md has the table; a k-ordered MFMA chain errs more than blocked CPU sums).
The penalty is held to 1e-6 relative of the fp64 value.  Every figure is printed before it is asserted ("[ortho] ...", pytest -s)
and goes to $DVD_TEST_NUMBERS_DIR/ortho_numbers.json when that names a directory.
"""
import argparse
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLS = 8
SHAPES = [(1, 16), (3, 36), (3, 576), (4, 8), (8, 8), (16, 16), (33, 50), (64, 577), (65, 4609), (96, 1), (130, 31), (256, 240),
          (256, 4608)]
GAP = 5                      # sentinel floats before, between and behind the items: every base is only 4-byte aligned somewhere
SENTINEL = -12345.5
BETA = 1e-4
M_RATIO = 12.0               # see the module docstring and profiles/ortho_parity_numbers.md
PEN_RTOL = 1e-6
U = 2.0 ** -24
NUMBERS = {}


def _dump():
    d = os.environ.get("DVD_TEST_NUMBERS_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "ortho_numbers.json"), "w") as f:
            json.dump(NUMBERS, f, indent=1, sort_keys=True)


def _gamma(n):
    return n * U / (1.0 - n * U)


def _s_of(beta):
    return float(np.float32(2.0) * np.float32(beta))


def ref64(w32, s):
    """fp64 restatement on a stored fp32 matrix [h, w] -> dict(t, bound of (a), penalty, yardstick rel-L2 of the fp32 CPU products)."""
    w = w32.double()
    h = w.shape[0]
    off = 1.0 - torch.eye(h, dtype=torch.float64)
    m = (w @ w.t()) * off
    t = s * (m @ w)
    aw = w.abs()
    bound = s * (_gamma(h + 2) * (m.abs() @ aw) + _gamma(w.shape[1]) * (((aw @ aw.t()) * off) @ aw)) + U * t.abs()
    m32 = (w32 @ w32.t()) * off.float()
    t32 = np.float32(s) * (m32 @ w32)
    nt = float(t.norm())
    return {"t": t, "bound": bound, "pen": 0.5 * float((m * m).sum()),
            "yard": float((t32.double() - t).norm()) / nt if nt else 0.0}


def check_item(label, t_got, ref, m_ratio=M_RATIO):
    """(a) and (b) for one item; t_got: fp32 [h, w] on any device.  -> (worst error / bound, rel-L2 ratio)."""
    err = (t_got.double().cpu() - ref["t"]).abs()
    nt = float(ref["t"].norm())
    if nt == 0.0:                                            # h = 1: nothing to add
        assert float(err.max()) == 0.0, label
        return 0.0, 0.0
    worst = float((err / ref["bound"].clamp_min(1e-300)).max())
    rel = float(err.norm()) / nt
    ratio = rel / ref["yard"]
    print(f"[ortho] {label}: worst error / bound (a) {worst:.3e}; rel-L2 kernel {rel:.3e}, fp32 CPU {ref['yard']:.3e}, ratio {ratio:.2f}")
    NUMBERS[label] = {"a": worst, "rel": rel, "yard": ref["yard"], "ratio": ratio}
    _dump()
    assert bool((err <= ref["bound"]).all()), (label, worst)
    assert rel <= m_ratio * ref["yard"], (label, rel, ref["yard"], ratio)
    return worst, ratio


def check_penalty(label, got, want):
    rel = abs(got - want) / want if want else abs(got)
    print(f"[ortho] {label}: penalty {got:.9e}, fp64 {want:.9e}, rel {rel:.2e}")
    NUMBERS[label + " penalty"] = rel
    _dump()
    assert rel <= PEN_RTOL, (label, got, want, rel)


# ------------------------------------------------------------------ kernel level
def _lib():
    from dvd_gan_amd import lib as L
    return L.lib()


def _table(rows):
    t = torch.tensor([list(r) + [0] * (COLS - 3) for r in rows], dtype=torch.int64)
    ws = ctypes.c_longlong(0)
    tiles = _lib().dvd_ortho_prepare(ctypes.c_void_p(t.data_ptr()), t.shape[0], ctypes.byref(ws))
    assert tiles >= 0, tiles
    return t, ws.value


def _call(p, g, table, ws_floats, beta, want_penalty=True):
    """One dvd_ortho_grad on the arenas p, g (device fp32) -> (penalty or None, the workspace guard is intact)."""
    ws = torch.full((ws_floats + 8,), float("nan"), dtype=torch.float32, device=DEV)
    ws[ws_floats:] = SENTINEL
    pen = torch.full((), float("nan"), dtype=torch.float64, device=DEV) if want_penalty else None
    dev = table.to(DEV)
    rc = _lib().dvd_ortho_grad(ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(table.data_ptr()),
                               ctypes.c_void_p(dev.data_ptr()), table.shape[0], ctypes.c_float(beta),
                               ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(pen.data_ptr()) if want_penalty else None,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((ws[ws_floats:] == SENTINEL).all())
    return float(pen) if want_penalty else None


@functools.lru_cache(maxsize=None)
def _arena(scale):
    """p and g arenas on the host (gaps hold SENTINEL), the item rows (off, h, w) and the fp64 references; computed once."""
    gen = torch.Generator().manual_seed(23)
    rows, off = [], GAP
    for h, w in SHAPES:
        rows.append((off, h, w))
        off += h * w + GAP
    p = torch.full((off,), SENTINEL, dtype=torch.float32)
    g = torch.full((off,), SENTINEL, dtype=torch.float32)
    inside = torch.zeros(off, dtype=torch.bool)
    for o, h, w in rows:
        p[o:o + h * w] = 0.05 * scale * torch.randn(h * w, generator=gen)
        g[o:o + h * w] = 1e-6 * scale ** 3 * torch.randn(h * w, generator=gen)
        inside[o:o + h * w] = True
    assert bool((g[inside] != 0).all())
    s = _s_of(BETA)
    refs = [ref64(p[o:o + h * w].view(h, w), s) for o, h, w in rows]
    return p, g, inside, rows, refs


@functools.lru_cache(maxsize=None)
def _runs(scale):
    """Every launch the kernel-level tests look at, made once: the batched call on random g (twice) and on a zeroed g, and every
    item alone on a zeroed g.  Results on the host."""
    p, g, inside, rows, refs = _arena(scale)
    table, wsf = _table(rows)
    pd = p.to(DEV)
    out = {"table": table}
    for key in ("first", "second"):
        gd = g.to(DEV)
        out["pen_" + key] = _call(pd, gd, table, wsf, BETA)
        out[key] = gd.cpu()
    zero = torch.where(inside, torch.zeros(()), g)
    gd = zero.to(DEV)
    _call(pd, gd, table, wsf, BETA, want_penalty=False)              # a NULL penalty pointer skips the value
    out["t"] = gd.cpu()
    out["alone"], out["pen_alone"] = [], []
    for row in rows:
        t1, ws1 = _table([row])
        gd = zero.to(DEV)
        out["pen_alone"].append(_call(pd, gd, t1, ws1, BETA))
        out["alone"].append(gd.cpu())
    assert torch.equal(pd.cpu().view(torch.int32), p.view(torch.int32))          # p is read only
    return out


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("scale", [1.0, 100.0], ids=["x1", "x100"])
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=[f"{h}x{w}" for h, w in SHAPES])
def test_gradient_term_against_fp64(idx, scale):
    """(5) batched and alone: both bounds per item, and the item's penalty from the run that holds it alone."""
    p, g, inside, rows, refs = _arena(scale)
    r = _runs(scale)
    o, h, w = rows[idx]
    for tag, arena in (("batched", r["t"]), ("alone", r["alone"][idx])):
        check_item(f"{h}x{w} x{scale:g} {tag}", arena[o:o + h * w].view(h, w), refs[idx])
    check_penalty(f"{h}x{w} x{scale:g} alone", r["pen_alone"][idx], refs[idx]["pen"])


@pytest.mark.parametrize("scale", [1.0, 100.0], ids=["x1", "x100"])
def test_batched_penalty_against_fp64(scale):
    p, g, inside, rows, refs = _arena(scale)
    r = _runs(scale)
    check_penalty(f"all x{scale:g} batched", r["pen_first"], sum(ref["pen"] for ref in refs))
    assert r["pen_first"] == r["pen_second"]


@pytest.mark.parametrize("scale", [1.0, 100.0], ids=["x1", "x100"])
def test_structure_of_the_update(scale):
    """(6) nothing outside the items moves, everything inside does (but the h = 1 item), batched == alone, rerun == run, and
    g_out == fl(g_in + t) bit for bit with t the same call into a zeroed buffer."""
    p, g, inside, rows, refs = _arena(scale)
    r = _runs(scale)
    first, t = r["first"], r["t"]
    for name in ("first", "second", "t"):
        assert torch.equal(_bits(r[name])[~inside], _bits(g)[~inside]), name
    assert torch.equal(_bits(first), _bits(r["second"]))
    for idx, (o, h, w) in enumerate(rows):
        sl = slice(o, o + h * w)
        assert bool(torch.isfinite(first[sl]).all()) and bool(torch.isfinite(t[sl]).all()), (h, w)
        if h == 1:
            assert torch.equal(_bits(first[sl]), _bits(g[sl])) and bool((t[sl] == 0).all())
        else:
            same = int((first[sl] == g[sl]).sum())
            assert same == 0, (h, w, same)
        alone = r["alone"][idx]
        assert torch.equal(_bits(alone[sl]), _bits(t[sl])), (h, w)
        rest = inside.clone()
        rest[sl] = False
        assert bool((alone[rest] == 0).all()) and torch.equal(_bits(alone)[~inside], _bits(g)[~inside]), (h, w)
    want = torch.where(inside, g + t, g)                             # one fp32 add of the rounded term: the two-rounding epilogue
    assert torch.equal(_bits(first), _bits(want)), int((first != want).sum())


# ------------------------------------------------------------------ FlatAdam and the Trainer
def test_flat_adam_regularises_the_selected_matrices_of_a_small_generator():
    """(7) ch = 2 generator in exact mode: after ortho_grad on random gradients the included tensors meet (5), every other element
    is bit-untouched."""
    from dvd_gan_amd.gen_net import Generator
    from dvd_gan_amd.optim import FlatAdam
    torch.manual_seed(5)
    G = Generator(120, 4, 7, ch=2, n_frames=4, compute_dtype=torch.float32).to(DEV)
    opt = FlatAdam(G.parameters(), 1e-3, ortho=BETA, ortho_exclude=G.ortho_exclude())
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        opt.flat.add_((0.05 * torch.randn(opt.flat.numel(), generator=gen)).to(DEV))
    flat0 = opt.flat.clone()
    opt.ortho_grad()                                                 # grad is zero: this leaves t
    torch.cuda.synchronize()
    t = opt.grad.cpu()
    g0 = (1e-6 * torch.randn(opt.flat.numel(), generator=gen)).to(DEV)
    opt.grad.copy_(g0)
    opt.ortho_grad()
    torch.cuda.synchronize()
    assert torch.equal(_bits(opt.flat), _bits(flat0))
    assert torch.equal(_bits(opt.grad.cpu()), _bits(g0.cpu() + t))
    included = torch.zeros(opt.flat.numel(), dtype=torch.bool)
    s, pen, flat = _s_of(BETA), 0.0, flat0.cpu()
    names = [n for n, p in G.named_parameters() if p.requires_grad]
    for row, i in zip(opt.ortho_items.tolist(), opt.ortho_index):
        o, h, w = row[:3]
        included[o:o + h * w] = True
        ref = ref64(flat[o:o + h * w].view(h, w), s)
        pen += ref["pen"]
        check_item(f"G(ch=2) {names[i]} {h}x{w}", t[o:o + h * w].view(h, w), ref)
    assert len(opt.ortho_index) == 62 and bool((t[~included] == 0).all()) and bool((t[included] != 0).all())
    assert torch.equal(_bits(opt.grad.cpu())[~included], _bits(g0.cpu())[~included])
    check_penalty("G(ch=2)", float(opt.ortho_penalty), pen)


def _cfg(ch, T, k, B, ncls, zd, lr=5e-5, **extra):
    return argparse.Namespace(adv_loss="hinge", z_dim=zd, g_chn=ch, ds_chn=ch, dt_chn=ch, n_frames=T, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=B, g_lr=lr, d_lr=lr, beta1=0.0, beta2=0.9,
                              n_class=ncls, k_sample=k, **extra)


def _bf16_step(**extra):
    """One step of tests/test_gpu_ema.py's bf16 run (seed 3, ch = 32, T = 8, B = 2, clips and draws from generator 11) ->
    (trainer, the generator's weights before the step, the six losses)."""
    from dvd_gan_amd.train_step import Trainer
    ch, T, B, ncls, zd = 32, 8, 2, 7, 120
    torch.manual_seed(3)
    tr = Trainer([], _cfg(ch, T, 8, B, ncls, zd, **extra), device=torch.device(DEV), compute_dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(11)
    real = torch.rand(B, 3, T, 64, 64, generator=gen) * 2 - 1
    labels = torch.randint(0, ncls, (B,), generator=gen)
    draws = {"perm_real": torch.randperm(T, generator=gen), "z": torch.randn(B, zd, generator=gen),
             "z_class": torch.randint(0, ncls, (B,), generator=gen), "perm_fake": torch.randperm(T, generator=gen)}
    flat0 = tr.g_optimizer.flat.clone()
    losses = [float(v.detach()) for v in tr.train_step(real, labels, draws)]
    torch.cuda.synchronize()
    return tr, flat0, losses


def _d_state(tr):
    out = {}
    for tag, net, opt in (("Ds", tr.D_s, tr.ds_optimizer), ("Dt", tr.D_t, tr.dt_optimizer)):
        for k, v in net.state_dict().items():
            out[f"{tag}.{k}"] = v.detach().clone()
        for k in ("flat", "m", "v"):
            out[f"{tag}.opt.{k}"] = getattr(opt, k).detach().clone()
    return out


def test_trainer_adds_the_term_to_the_generators_gradient_only():
    """(8) two bf16 Trainers from one seed, one with g_ortho = 1e-4, one step: losses and everything of D_s / D_t bit-equal, the
    generator's gradient buffer == fl(plain gradient + t) bit for bit with t from a direct call on the pre-step weights, the
    generator's weights differ, and ortho_penalty matches the fp64 value of the pre-step weights."""
    from dvd_gan_amd import kern as K
    plain, flat_a, la = _bf16_step()
    opt = plain.g_optimizer
    assert plain.g_ortho == 0.0 and plain.ortho_penalty is None
    assert opt.ortho_items is None and opt.ortho_items_dev is None and opt.ortho_ws is None and opt.ortho_ws_floats == 0
    assert plain.ds_optimizer.ortho_items is None and plain.dt_optimizer.ortho_items is None
    sa, grad_a, g_flat_a = _d_state(plain), opt.grad.clone(), opt.flat.clone()
    del plain, opt
    reg, flat_b, lb = _bf16_step(g_ortho=BETA)
    opt = reg.g_optimizer
    assert la == lb and len(lb) == 6, (la, lb)
    assert torch.equal(flat_a, flat_b)
    sb = _d_state(reg)
    assert set(sa) == set(sb) and not [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert reg.ds_optimizer.ortho_items is None and reg.dt_optimizer.ortho_items is None
    assert opt.ortho_ws is not None and opt.ortho_ws.numel() == opt.ortho_ws_floats

    t = torch.zeros_like(flat_b)
    ws = torch.empty(opt.ortho_ws_floats, dtype=torch.float32, device=DEV)
    pen = torch.zeros((), dtype=torch.float64, device=DEV)
    K.ortho_grad(flat_b, t, opt.ortho_items, opt.ortho_items_dev, BETA, ws, pen)
    torch.cuda.synchronize()
    assert torch.equal(_bits(opt.grad), _bits(grad_a + t)), int((opt.grad != grad_a + t).sum())
    assert int((t != 0).sum()) > 0.9 * sum(r[1] * r[2] for r in opt.ortho_items.tolist())
    assert not torch.equal(opt.flat, g_flat_a)
    assert float(pen) == float(reg.ortho_penalty)
    want = 0.0                                                       # fp64 products of the stored fp32 weights (on the device: 0.1 TFLOP)
    for o, h, w, *_ in opt.ortho_items.tolist():
        wm = flat_b[o:o + h * w].view(h, w).double()
        m = wm @ wm.t()
        m.fill_diagonal_(0.0)
        want += 0.5 * float((m * m).sum())
    check_penalty("Trainer ch=32", float(reg.ortho_penalty), want)

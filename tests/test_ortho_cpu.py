"""CPU checks of the orthogonal regularizer (dvd_ortho_prepare / dvd_ortho_grad, optim.FlatAdam(ortho=...), config.g_ortho):
  1. the fp64 checker the GPU tests use (2 M W and R = 1/2 ||M||_F^2, M = W W^T minus its diagonal) against autograd;
  2. the host-only planner and the argument validation, without a device;
  3. the item table FlatAdam builds for a ch = 2 generator: which tensors are in, which are out, at which offsets;
  4. the compiler's resource report of csrc/ortho.hip: no scratch memory, no spilled vector registers."""
import argparse
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS, OFF, H, W, WS, GRAM0, APPLY0, GORDER, AORDER = 8, 0, 1, 2, 3, 4, 5, 6, 7


def ortho_ref64(w):
    """fp64 restatement: w [h, ...] -> (2 M W as [h, numel / h], R) with M = W W^T, diagonal zeroed, R = 1/2 ||M||_F^2."""
    w2 = w.double().reshape(w.shape[0], -1)
    m = w2 @ w2.t()
    m = m * (1.0 - torch.eye(m.shape[0], dtype=torch.float64))
    return 2.0 * (m @ w2), 0.5 * float((m * m).sum())


def test_checker_equals_autograd_of_the_penalty():
    w = torch.randn(5, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(1), requires_grad=True)
    g = w @ w.t()
    r = 0.5 * ((g - torch.diag(torch.diag(g))) ** 2).sum()
    r.backward()
    t, pen = ortho_ref64(w.detach())
    assert float((t - w.grad).abs().max()) <= 1e-12 and abs(pen - float(r.detach())) <= 1e-12
    t1, pen1 = ortho_ref64(torch.randn(1, 9, dtype=torch.float64))
    assert float(t1.abs().max()) == 0.0 and pen1 == 0.0


def _table(shapes, gap=3):
    rows, off = [], gap
    for h, w in shapes:
        rows.append([off, h, w] + [0] * (COLS - 3))
        off += h * w + gap
    return torch.tensor(rows, dtype=torch.int64)


def _prepare(lib, t):
    ws = ctypes.c_longlong(-7)
    rc = lib.dvd_ortho_prepare(ctypes.c_void_p(t.data_ptr()), t.shape[0], ctypes.byref(ws))
    return rc, ws.value


def test_planner_and_validation_run_without_a_device():
    from dvd_gan_amd import lib as L
    lib = L.lib()
    assert lib.dvd_abi_version() == 13          # additions only
    shapes = [(1, 16), (3, 36), (64, 577), (65, 4609), (96, 1), (130, 31), (256, 240), (1, 5)]
    t = _table(shapes)
    tiles, ws = _prepare(lib, t)
    nb = lambda h: -(-h // 64)
    assert tiles == sum(nb(h) * (nb(h) + 1) // 2 for h, w in shapes if h > 1)
    # workspace: the M_i [h][h] of the items with h > 1 do not overlap, then one fp64 slot per tile on an 8-byte boundary
    spans = sorted((int(r[WS]), int(r[WS]) + int(r[H]) ** 2) for r in t if r[H] > 1)
    assert spans[0][0] >= 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert ws >= spans[-1][1] + 2 * tiles
    # launch orders are permutations; items with h = 1 come last and get no blocks; block ranges are disjoint and gap-free
    for ocol, fcol, count in ((GORDER, GRAM0, lambda h, w: nb(h) * (nb(h) + 1) // 2),
                              (AORDER, APPLY0, lambda h, w: nb(h) * -(-w // 128))):
        order = [int(v) for v in t[:, ocol]]
        assert sorted(order) == list(range(len(shapes)))
        nxt = 0
        for i in order:
            h, w = shapes[i]
            assert int(t[i, fcol]) == nxt, (i, ocol)
            nxt += count(h, w) if h > 1 else 0
        real = [i for i in order if shapes[i][0] > 1]
        assert order[:len(real)] == real and all(shapes[i][0] == 1 for i in order[len(real):])
    depth = [shapes[int(i)][1] for i in t[:, GORDER] if shapes[int(i)][0] > 1]
    assert depth == sorted(depth, reverse=True)          # deepest Gram chains first
    again = t.clone()
    assert _prepare(lib, again) == (tiles, ws) and torch.equal(again, t)

    # errors: null pointers, n < 1, h < 1, w < 1, negative offset -> -1; h past DVD_ORTHO_MAX_H -> -2
    wsv = ctypes.c_longlong(0)
    assert lib.dvd_ortho_prepare(None, 2, ctypes.byref(wsv)) == -1
    assert lib.dvd_ortho_prepare(ctypes.c_void_p(t.data_ptr()), 2, None) == -1
    assert lib.dvd_ortho_prepare(ctypes.c_void_p(t.data_ptr()), 0, ctypes.byref(wsv)) == -1
    for col, bad, want in ((H, 0, -1), (H, -3, -1), (W, 0, -1), (OFF, -1, -1), (H, 32769, -2)):
        b = _table(shapes)
        b[2, col] = bad
        assert _prepare(lib, b)[0] == want, (col, bad)

    # dvd_ortho_grad checks everything before any launch (the placeholder device pointers are never dereferenced)
    p = ctypes.c_void_p(64)
    f = ctypes.c_float
    host = ctypes.c_void_p(t.data_ptr())
    n = t.shape[0]
    grad = lambda p_, g_, ih, idv, n_, s, ws_: lib.dvd_ortho_grad(p_, g_, ih, idv, n_, f(s), ws_, None, None)
    assert grad(None, p, host, p, n, 1e-4, p) == -1
    assert grad(p, None, host, p, n, 1e-4, p) == -1
    assert grad(p, p, None, p, n, 1e-4, p) == -1
    assert grad(p, p, host, None, n, 1e-4, p) == -1
    assert grad(p, p, host, p, n, 1e-4, None) == -1
    assert grad(p, p, host, p, 0, 1e-4, p) == -1
    for bad in (-1e-4, float("nan"), float("inf")):
        assert grad(p, p, host, p, n, bad, p) == -1, bad
    raw = _table(shapes)                                  # a table the planner has not filled
    assert grad(p, p, ctypes.c_void_p(raw.data_ptr()), p, n, 1e-4, p) == -1
    b = t.clone()
    b[1, H] = 0
    assert grad(p, p, ctypes.c_void_p(b.data_ptr()), p, n, 1e-4, p) == -1


def test_flat_adam_builds_the_table_of_a_small_generator():
    from dvd_gan_amd.gen_net import Generator
    from dvd_gan_amd.optim import FlatAdam
    from dvd_gan_amd.train_step import Trainer
    torch.manual_seed(0)
    G = Generator(120, 4, 7, ch=2, n_frames=4)
    off = FlatAdam(G.parameters(), 1e-3)
    assert off.ortho == 0.0 and off.ortho_items is None and off.ortho_items_dev is None and off.ortho_ws is None
    assert off.ortho_penalty is None and off.ortho_ws_floats == 0
    opt = FlatAdam(G.parameters(), 1e-3, ortho=1e-4, ortho_exclude=G.ortho_exclude())
    assert opt.ortho_ws is None and opt.ortho_penalty is None            # allocated at the first step()
    named = [(n, p) for n, p in G.named_parameters() if p.requires_grad]
    assert [id(p) for _, p in named] == [id(p) for p in opt.params]
    offs, o = {}, 0
    for n_, p in named:
        offs[n_] = o
        o += p.numel()
    rows = {named[i][0]: [int(v) for v in opt.ortho_items[r, :3]] for r, i in enumerate(opt.ortho_index)}
    for n_, row in rows.items():
        p = dict(named)[n_]
        assert row == [offs[n_], p.shape[0], p.numel() // p.shape[0]], n_
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * row[0], n_          # the parameter IS that slice of `flat`
    inside, outside = set(rows), {n_ for n_, _ in named} - set(rows)
    assert "embedding.weight" in outside
    embeds = [n_ for n_, _ in named if n_.endswith(".embed.weight")]
    from dvd_gan_amd.sn_layers import ConditionalNorm
    n_cbn = sum(isinstance(m, ConditionalNorm) for m in G.modules())
    assert len(embeds) == n_cbn == 16 and set(embeds) <= outside         # two conditional norms in each of the 8 GResBlocks
    assert all(n_ in outside for n_, p in named if p.dim() < 2)
    assert inside == {n_ for n_, p in named if p.dim() >= 2 and n_ != "embedding.weight" and not n_.endswith(".embed.weight")}
    assert rows["affine_transfrom.weight"][1:] == [256, 240]
    assert rows["colorize.module.weight_bar"][1:] == [3, 36]
    assert rows["conv.11.conv_sc.module.weight_bar"][1:] == [4, 8]
    gates = [n_ for n_ in inside if "_gate.weight" in n_]
    bars = [n_ for n_ in inside if n_.endswith("weight_bar")]
    assert len(gates) == 36 and len(bars) == 25 and len(inside) == 62
    assert opt.ortho_ws_floats >= sum(r[1] ** 2 for r in rows.values())

    with pytest.raises(ValueError, match="ortho"):
        FlatAdam([torch.nn.Parameter(torch.randn(4, 4))], 1e-3, ortho=-1.0)
    cfg = argparse.Namespace(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const", total_epoch=1,
                             d_iters=1, batch_size=2, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9, n_class=3, k_sample=4,
                             g_ortho=-1)
    with pytest.raises(ValueError, match="g_ortho"):
        Trainer([], cfg, device=torch.device("cpu"), compute_dtype=torch.float32)


def test_ortho_kernels_use_no_scratch_memory():
    path = os.path.join(ROOT, "dvd_gan_amd", "csrc", "build", "ortho.res")
    if not os.path.exists(path):
        pytest.skip("no build/ortho.res: the library was not built by csrc/build.sh in this tree")
    recs, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            recs[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and name:
            recs[name][m.group(1).strip()] = int(m.group(2))
    for kernel in ("ortho_gram_kernel", "ortho_apply_kernel", "ortho_penalty_kernel"):
        assert any(kernel in n_ for n_ in recs), (kernel, list(recs))
    for n_, rec in recs.items():
        assert rec["ScratchSize"] == 0 and rec["VGPRs Spill"] == 0, (n_, rec)

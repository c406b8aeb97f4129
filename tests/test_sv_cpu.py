"""Singular-value monitoring without a GPU: the fp64 restatement the GPU tests compare with (tests/sv_ref.py) against the fp64 SVD,
the sv library's item mirror, its refusals (which come back before anything touches the device), its resource file, the
Trainer's settings and the start blocks' private generator."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sv_ref as R

E_ARG, E_SHAPE = -1, -2
P_, Q_, S_ = 64, 128, 256          # non-null placeholder pointers: the refusals come before anything is dereferenced

GAPPED = [(70, 4097), (16, 27), (3, 27), (1, 13), (257, 130)]


def run(W, iters, k=3, block=8, seed=0, **kw):
    h, w = W.shape
    return R.report(W, R.start_blocks([(h, w)], block, seed)[0], iters, k, **kw)


# ------------------------------------------------------------------ the restatement against the fp64 SVD
@pytest.mark.parametrize("shape", GAPPED)
def test_gapped_spectra(shape):
    """s = (4, 3, 2, then <= 0.5), b = 8: the iteration error bound after 8 iterations is (0.5 / 2)^16 = 16^-8 ~ 2e-10 relative."""
    h, w = shape
    W, truth = R.gapped(h, w, [4.0, 3.0, 2.0] + list(np.linspace(0.5, 0.05, 40)), seed=h + w)
    sv, res, fro2, sn = run(W, 8)
    want = np.zeros(3)
    want[:min(3, len(truth))] = truth[:3]
    print(shape, "error / sigma0", np.abs(sv - want).max() / truth[0], "res", res)
    assert np.abs(sv - want).max() <= 1e-8 * truth[0]
    assert np.all(np.diff(sv) <= 0) and np.all(sv[min(h, w):] == 0.0)
    assert abs(fro2 - float((W.astype(np.float64) ** 2).sum())) <= 1e-12 * fro2 and np.isnan(sn)


@pytest.mark.parametrize("shape", [(64, 576), (256, 2304)])
def test_a_posteriori_bound_on_flat_spectra(shape):
    """Gaussian weights: at every iteration count each reported value has a true singular value within its residual (plus the
    rounding of the fp64 products, 1e-12 sigma0), is a lower bound of its own singular value and rises with the iterations."""
    W = np.random.default_rng(shape[0]).standard_normal(shape).astype(np.float32)
    truth = np.linalg.svd(W.astype(np.float64), compute_uv=False)
    h, w = shape
    st = R.State(W, R.start_blocks([(h, w)], 8, 0)[0])
    done, last = 0, np.zeros(3)
    for iters in (4, 8, 16, 32):
        st.iterate(iters - done)
        done = iters
        sv, res, _, _ = st.ritz(3)
        gap = np.abs(sv[:, None] - truth[None, :]).min(1)
        print(shape, iters, "low by", (truth[:3] - sv) / truth[:3], "res", res, "nearest", gap)
        assert np.all(gap <= res + 1e-12 * truth[0])
        assert np.all(sv <= truth[:3] * (1 + 1e-12)) and np.all(sv >= last * (1 - 1e-12))
        last = sv
    assert np.all((truth[:3] - sv) / truth[:3] < 0.02)


def test_repeated_top_value():
    """s = (3, 3, 1, 0 ...) held exactly (an fp32 rounding of a random low-rank matrix would have a fourth value near 1e-8)."""
    W = R.exact_low_rank(16, 40, [3.0, 3.0, 1.0])
    sv, res, _, _ = run(W, 8, k=4)
    assert np.abs(sv[:3] - [3.0, 3.0, 1.0]).max() <= 1e-12
    assert sv[3] < 1e-12 and not np.isnan(res).any() and res.max() < 1e-12


def rank_deficient():
    base = np.array([[1, 2, 0, -1, 3, 1, 0], [0, 1, 1, 2, -2, 0, 1], [2, 0, -1, 1, 0, 3, -2]], dtype=np.float32)
    return base[[0, 1, 2, 0, 1, 2, 0, 1, 0, 0]]            # 10 x 7, rank 3, small integers: every product is exact


def test_exact_rank_deficiency():
    W = rank_deficient()
    truth = np.linalg.svd(W.astype(np.float64), compute_uv=False)
    sv, res, fro2, _ = run(W, 6, k=6)
    assert np.abs(sv[:3] - truth[:3]).max() <= 1e-9 * truth[0]
    assert np.all(sv[3:] == 0.0) and np.all(res[3:] == 0.0) and not np.isnan(sv).any() and not np.isnan(res).any()
    assert fro2 == float((W.astype(np.float64) ** 2).sum())


def test_all_zero_matrix():
    sv, res, fro2, sn = run(np.zeros((5, 9), np.float32), 3, u=np.ones(5, np.float32), v=np.ones(9, np.float32))
    assert np.all(sv == 0.0) and np.all(res == 0.0) and fro2 == 0.0 and sn == 0.0


def test_k_equal_to_block_and_fewer_columns_than_k():
    W, truth = R.gapped(12, 20, [5.0, 4.0, 3.0, 2.0, 0.1, 0.05], seed=2)
    sv, res, _, _ = run(W, 12, k=4, block=4)
    assert np.abs(sv - truth[:4]).max() <= 1e-8 * truth[0]
    W, truth = R.gapped(2, 9, [2.0, 1.0], seed=3)              # r = 2 < k = 3
    sv, res, _, _ = run(W, 4, k=3)
    assert np.abs(sv[:2] - truth[:2]).max() <= 1e-12 * truth[0] and sv[2] == 0.0 and res[2] == 0.0


def test_sn_sigma_is_u_W_v():
    rng = np.random.default_rng(1)
    W = rng.standard_normal((6, 11)).astype(np.float32)
    u, v = rng.standard_normal(6).astype(np.float32), rng.standard_normal(11).astype(np.float32)
    *_, sn = run(W, 2, u=u, v=v)
    assert abs(sn - float(u.astype(np.float64) @ W.astype(np.float64) @ v.astype(np.float64))) < 1e-12


def test_orth_and_jacobi():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((50, 6))
    A[:, 3] = A[:, 0] - 2 * A[:, 1]                              # a dependent column becomes exact zeros
    Q, Rm = R.orth(A)
    live = [0, 1, 2, 4, 5]
    assert np.all(Q[:, 3] == 0.0) and Rm[3, 3] == 0.0
    assert np.abs(Q[:, live].T @ Q[:, live] - np.eye(5)).max() < 1e-14 and np.abs(Q @ Rm - A).max() < 1e-13
    M, J = R.jacobi(Rm)
    assert np.abs(J.T @ J - np.eye(6)).max() < 1e-14 and np.abs(Rm @ J - M).max() < 1e-13
    G = M.T @ M
    assert np.abs(G - np.diag(np.diag(G))).max() < 1e-13 * G.max()
    assert np.abs(np.sort(np.sqrt(np.diag(G)))[::-1] - np.linalg.svd(Rm, compute_uv=False)).max() < 1e-13


# ------------------------------------------------------------------ the start blocks
def test_start_blocks_come_from_a_private_generator():
    from dvd_gan_amd.spectral import draw_start_blocks
    torch.manual_seed(11)
    before = torch.get_rng_state()
    shapes = [(3, 27), (16, 5), (1, 13)]
    a = draw_start_blocks(shapes, 8, 4)
    assert torch.equal(before, torch.get_rng_state())                  # the default generator is not touched
    b = draw_start_blocks(shapes, 8, 4)
    assert [tuple(t.shape) for t in a] == [(27, 3), (5, 5), (13, 1)] and all(t.dtype == torch.float64 for t in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x.numpy(), y) for x, y in zip(a, R.start_blocks(shapes, 8, 4)))
    assert not torch.equal(a[0], draw_start_blocks(shapes, 8, 5)[0])
    gen = torch.Generator().manual_seed(4)                             # item by item in table order
    assert torch.equal(a[0], torch.randn(27, 3, dtype=torch.float64, generator=gen))
    assert torch.equal(a[1], torch.randn(5, 5, dtype=torch.float64, generator=gen))


# ------------------------------------------------------------------ the Trainer's settings
def test_trainer_refuses_bad_settings_before_it_builds_anything():
    from dvd_gan_amd.train_step import Trainer
    base = dict(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const", total_epoch=1, d_iters=1,
                batch_size=2, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=3, k_sample=4)
    for over, word in ((dict(sv_log=-1), "sv_log"), (dict(sv_iters=0), "sv_iters"), (dict(sv_log_rows=0), "sv_log_rows"),
                       (dict(sv_k=0), "sv_k"), (dict(sv_k=9), "sv_k"), (dict(sv_block=17, sv_k=3), "sv_block"),
                       (dict(sv_k=4, sv_block=3), "sv_block")):
        with pytest.raises(ValueError, match=word):
            Trainer([], argparse.Namespace(**dict(base, **over)), device=torch.device("cpu"), compute_dtype=torch.float32)


def test_monitor_refuses_bad_settings():
    from dvd_gan_amd.spectral import SpectrumMonitor, top_singular_values
    for kw in (dict(k=0), dict(k=9), dict(block=17), dict(k=3, block=2)):
        with pytest.raises(ValueError, match="block"):
            SpectrumMonitor([("a", torch.zeros(2, 2))], **kw)
    with pytest.raises(ValueError, match="matrices"):
        SpectrumMonitor([])
    with pytest.raises(ValueError, match="fp32"):
        SpectrumMonitor([("a", torch.zeros(2, 2))])                    # not on a device
    with pytest.raises(ValueError, match="iters"):
        top_singular_values([torch.zeros(2, 2)], iters=0)


# ------------------------------------------------------------------ the sv library (its handshake: tests/test_abi_cpu.py)
def test_item_mirror_has_the_struct_s_fields():
    """lib.SvItem against `dvd_sv_item` of include/dvdgan_hip_sv.h: the size the library was compiled with, and the fields in order
    with matching kinds.  The sweep limit is the restatement's."""
    from test_abi_cpu import ROOT
    from dvd_gan_amd import lib as L
    assert L.sv_lib().dvd_sv_item_size() == C.sizeof(L.SvItem)
    assert L.SV_MAX_SWEEPS == R.MAX_SWEEPS
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvdgan_hip_sv.h")).read(), flags=re.S)
    body = re.search(r"typedef struct dvd_sv_item \{(.*?)\} dvd_sv_item;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "p" if "*" in decl else "l" if "long long" in decl else "i"
        fields += [(n.strip().lstrip("*"), kind) for n in re.sub(r"^(const\s+)?(float|double|long long|int)\s*\*?", "", decl).split(",")]
    kinds = {C.c_void_p: "p", C.c_longlong: "l", C.c_int: "i"}
    assert fields == [(n, kinds[t]) for n, t in L.SvItem._fields_]


def test_resource_file_shows_no_scratch_and_no_spills():
    """csrc/build.sh keeps hipcc's resource remarks of the sv library: the four kernels, in both stored widths (the product
    kernel also in the finish's form), run without scratch memory and without spills."""
    from test_abi_cpu import ROOT
    text = open(os.path.join(ROOT, "dvd_gan_amd", "csrc", "sv", "build", "spectrum.res")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    for kernel, count in (("sv_wv_kernel", 4), ("sv_wtv_kernel", 2), ("sv_orth_kernel", 2), ("sv_ritz_kernel", 2)):
        assert sum(kernel in n for n in names) == count, (kernel, names)
    assert len(names) == 10
    for field in ("ScratchSize \\[bytes/lane\\]", "SGPRs Spill", "VGPRs Spill"):
        values = [int(v) for v in re.findall(field + r": (\d+)", text)]
        assert len(values) == len(names) and max(values) == 0, (field, values)


def table(shapes, u=False):
    from dvd_gan_amd import lib as L
    items = (L.SvItem * len(shapes))()
    for i, (h, w) in enumerate(shapes):
        items[i].W, items[i].h, items[i].w, items[i].slot = P_ + 4 * i, h, w, i
        if u:
            items[i].u, items[i].v = Q_, S_
    return items


def test_prepare_plans_the_table():
    from dvd_gan_amd import lib as L
    sv = L.sv_lib()
    shapes = [(70, 4097), (3, 27), (1, 1), (130, 7)]
    for block, bp, rows in ((1, 8, 16), (8, 8, 16), (9, 16, 8), (16, 16, 8)):
        items = table(shapes)
        sd, wd = C.c_longlong(), C.c_longlong()
        assert sv.dvd_sv_prepare(items, len(shapes), block, C.byref(sd), C.byref(wd)) == 0
        st = ws = b0 = b1 = 0
        for it, (h, w) in zip(items, shapes):
            assert (it.state_off, it.ws_off, it.blk_wv, it.blk_wtv) == (st, ws, b0, b1)
            st += (w + h + bp) * bp
            ws += h * (bp + 2)
            b0 += -(-h // rows)
            b1 += -(-w // 64)
        assert (sd.value, wd.value) == (st, ws)


def test_refusals_come_before_any_launch():
    from dvd_gan_amd import lib as L
    sv = L.sv_lib()
    sd, wd = C.c_longlong(), C.c_longlong()
    shapes = [(4, 9), (3, 3)]

    def prepare(items=None, n=2, block=8, a=C.byref(sd), b=C.byref(wd)):
        return sv.dvd_sv_prepare(table(shapes) if items is None else items, n, block, a, b)
    assert prepare() == 0
    assert prepare(n=0) == E_ARG and prepare(n=L.SV_MAX_ITEMS + 1) == E_ARG and prepare(block=0) == E_ARG
    assert prepare(block=L.SV_MAX_BLOCK + 1) == E_ARG and prepare(a=None) == E_ARG and prepare(b=None) == E_ARG
    assert sv.dvd_sv_prepare(None, 2, 8, C.byref(sd), C.byref(wd)) == E_ARG
    for field, value, code in (("W", None, E_ARG), ("u", Q_, E_ARG), ("v", Q_, E_ARG), ("slot", 2, E_ARG), ("slot", -1, E_ARG),
                               ("slot", 0, E_ARG), ("h", 0, E_SHAPE), ("w", 0, E_SHAPE), ("h", -4, E_SHAPE)):
        items = table(shapes)
        setattr(items[1], field, value)
        assert prepare(items) == code, (field, value)
    assert prepare(table(shapes, u=True)) == 0

    good = table(shapes)
    assert prepare(good) == 0

    def calls(host, n=2, block=8):
        return (sv.dvd_sv_init(P_, host, n, block, Q_, S_, None),
                sv.dvd_sv_iterate(P_, host, n, block, 1, S_, None),
                sv.dvd_sv_ritz(P_, host, n, block, 3, S_, Q_, P_, 0, 1, None))
    raw = table(shapes)                                                  # a table dvd_sv_prepare did not fill
    assert calls(raw) == (E_ARG,) * 3 and calls(None) == (E_ARG,) * 3
    assert calls(good, block=16) == (E_ARG,) * 3                         # prepared for another stored width
    bad = table(shapes)
    prepare(bad)
    bad[0].h = 0
    assert calls(bad) == (E_SHAPE,) * 3
    assert sv.dvd_sv_init(None, good, 2, 8, Q_, S_, None) == E_ARG and sv.dvd_sv_init(P_, good, 2, 8, None, S_, None) == E_ARG
    assert sv.dvd_sv_init(P_, good, 2, 8, Q_, None, None) == E_ARG and sv.dvd_sv_init(P_, good, 2, 8, S_, S_, None) == E_ARG
    assert sv.dvd_sv_iterate(None, good, 2, 8, 1, S_, None) == E_ARG and sv.dvd_sv_iterate(P_, good, 2, 8, 1, None, None) == E_ARG
    assert sv.dvd_sv_iterate(P_, good, 2, 8, -1, S_, None) == E_ARG
    assert sv.dvd_sv_iterate(P_, good, 2, 8, L.SV_MAX_ITERS + 1, S_, None) == E_ARG
    assert sv.dvd_sv_iterate(P_, good, 2, 8, 0, S_, None) == 0           # nothing to do: succeeds, launches nothing

    def ritz(items=P_, k=3, state=S_, ws=Q_, out=P_, row=0, n_rows=1):
        return sv.dvd_sv_ritz(items, good, 2, 8, k, state, ws, out, row, n_rows, None)
    for name in ("items", "state", "ws", "out"):
        assert ritz(**{name: None}) == E_ARG, name
    assert ritz(k=0) == E_ARG and ritz(k=9) == E_ARG and ritz(row=-1) == E_ARG and ritz(row=1) == E_ARG
    assert ritz(row=4, n_rows=4) == E_ARG and ritz(n_rows=0) == E_ARG
    assert sv.dvd_sv_strerror(0) == b"ok" and sv.dvd_sv_strerror(-77) == b"unknown error"
    assert b"dvd_sv_prepare" in sv.dvd_sv_strerror(E_ARG) and b"w < 1" in sv.dvd_sv_strerror(E_SHAPE)
    assert b"launch" in sv.dvd_sv_strerror(-3)
    with pytest.raises(RuntimeError, match="libdvdgan_hip_sv"):
        L.sv_check(E_ARG)

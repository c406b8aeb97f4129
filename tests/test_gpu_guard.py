"""Gradient-norm clipping and non-finite step skipping on the GPU: dvd_grad_guard / dvd_adam_guard_step through kern.py, then the
Trainer (config g_clip_norm / d_clip_norm / skip_nonfinite / grad_log).

Kernel level, every test at n in {1, 3, 255, CH - 1, CH, CH + 1, 2 CH + 5, 2^20 + 5} (CH = kern.GUARD_CH), aligned and one float
off a 16-byte boundary, sentinels around every buffer:
  1. the sum of squares S against math.fsum of the exact fp64 squares of the stored fp32 gradient:
     |S - S_ref| <= GUARD_CHAIN(n) * 2^-53 * S_ref (all terms >= 0: the standard bound for a chain of GUARD_CHAIN(n) additions is
     relative; derived in kern.GUARD_CHAIN, not tuned), norm == sqrt(S) within one fp64 ulp; randn * 10^k for k = -6 .. 0, all
     1e30 (an fp32 accumulator overflows), all 1e-30 (it underflows), all zero;
  2. the state block is bit-equal across alignments and reruns, the partial sums of whole chunks do not change when the gradient
     is the prefix of a longer launch;
  3. one NaN / +inf / -inf at index 0, n - 1, the first element of the scalar tail, the last element of a full chunk: counted,
     left out of the norm;
  4. a guard that does not trigger (max_norm = inf, max_norm = 4 * norm; skip_nonfinite on) leaves p, m, v (and ema, decays 0, 0.9,
     0.9999) bit-equal to dvd_adam_step / dvd_adam_ema_step over three steps, coefficient exactly 1;
  5. clipping: the coefficient within one fp32 ulp of max_norm / (norm + 1e-6), the update bit-equal to the plain launch on
     g * coef formed by torch in fp32; a max_norm a hair above the norm gives exactly 1;
  6. skipping: nothing is written, the next clean step is bit-equal to the plain launch; with skip_nonfinite off the poisoned
     gradient goes through exactly as dvd_adam_step takes it;
  7. the ring log.
Trainer level (bf16, ch = 2, z_dim = 16, 8 frames, batch 2; fresh Trainers seeded alike):
  8. measuring is invisible (losses, flat / m / v, G's state_dict bit-equal to a Trainer with everything off; also with g_ortho and
     ema_decay on) and grad_norms is the fp64 norm of each optimizer's `grad`;  9. g_clip_norm;  10. a poisoned D_s gradient is
     skipped, D_t and G step;  11. all defaults: no guard tensors;  12. the log line of train().
Every figure is printed before it is asserted ("[guard] ...", pytest -s).  Measured maxima and the mutants this file catches:
profiles/guard_numbers.md.
"""
import argparse
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = 16384                   # == kern.GUARD_CH (asserted below)
SIZES = [1, 3, 255, CH - 1, CH, CH + 1, 2 * CH + 5, 2 ** 20 + 5]
PAD = 8                      # sentinel elements around every buffer
SENTINEL = -12345.5
INF = float("inf")
REGIMES = [f"k{k}" for k in range(-6, 1)] + ["big", "tiny", "zero"]
ADAM = (2e-3, 0.0, 0.9, 1e-8)          # lr, beta1, beta2, eps


# ------------------------------------------------------------------ kernel level: buffers and references
def _buf(n, off, fill=None, data=None, dtype=torch.float32):
    """-> (whole, view): `view` = n elements starting `off` elements into a fresh device buffer (fp32, off = 1: one float off a
    16-byte boundary); the elements around the view hold SENTINEL."""
    whole = torch.full((off + n + PAD,), SENTINEL, dtype=dtype, device=DEV)
    view = whole[off:off + n]
    if data is not None:
        view.copy_(data.to(DEV))
    else:
        view.fill_(fill)
    if dtype == torch.float32:
        assert view.data_ptr() % 16 == (4 * off) % 16
    return whole, view


def _intact(whole, n, off):
    return bool((whole[:off] == SENTINEL).all()) and bool((whole[off + n:] == SENTINEL).all())


class Guard:
    """Workspace, state block and (rows > 0) ring of one guarded optimizer, each between sentinels."""

    def __init__(self, n, rows=0):
        from dvd_gan_amd import kern as K
        assert K.GUARD_CH == CH
        self.n, self.rows = n, rows
        self.ws_n = K.grad_guard_ws_bytes(n) // 8
        self.ws_whole, ws = _buf(self.ws_n, PAD, fill=SENTINEL, dtype=torch.float64)
        self.ws = ws.view(torch.uint8)
        self.st_whole, self.state = _buf(K.GUARD_STATE, PAD, fill=0.0, dtype=torch.float64)
        self.ring_whole = self.ring = None
        if rows:
            self.ring_whole, ring = _buf(rows * 4, PAD, fill=float("nan"), dtype=torch.float64)
            self.ring = ring.view(rows, 4)

    def run(self, g, max_norm=INF, skip=0, step=1):
        from dvd_gan_amd import kern as K
        K.grad_guard(g, max_norm, skip, step, self.ws, self.state, self.ring)
        return self

    def views(self):
        from dvd_gan_amd import kern as K
        return K.grad_guard_ws_views(self.ws, self.n)

    def host(self):
        """-> (state as a list of 8 floats, S)"""
        return self.state.cpu().tolist(), float(self.views()[1][0])

    def intact(self):
        return _intact(self.ws_whole, self.ws_n, PAD) and _intact(self.st_whole, 8, PAD) and (
            self.ring is None or _intact(self.ring_whole, self.rows * 4, PAD))


@functools.lru_cache(maxsize=None)
def _data(n, regime):
    """The stored fp32 gradient of a regime (host tensor, shared by every test that needs it, never modified)."""
    if regime == "big":
        return torch.full((n,), 1e30, dtype=torch.float32)
    if regime == "tiny":
        return torch.full((n,), 1e-30, dtype=torch.float32)
    if regime == "zero":
        return torch.zeros(n, dtype=torch.float32)
    k = int(regime[1:])
    return (torch.randn(n, generator=torch.Generator().manual_seed(100 + n % 1000 - k)) * 10.0 ** k).float()


@functools.lru_cache(maxsize=None)
def _sumsq(n, regime, without=()):
    """Exact sum of squares (math.fsum: correctly rounded) of _data(n, regime) with the elements `without` left out; the squares of
    fp32 values are exact in fp64."""
    d = _data(n, regime).double()
    sq = (d * d).tolist()
    for i in without:
        sq[i] = 0.0
    return math.fsum(sq)


def _check_sum(S, norm, S_ref, n, label):
    from dvd_gan_amd import kern as K
    bound = K.GUARD_CHAIN(n) * 2.0 ** -53 * S_ref
    err = abs(S - S_ref)
    root = math.sqrt(S)
    print(f"[guard] {label}: S {S:.17e} ref {S_ref:.17e} |err| {err:.3e} error / bound "
          f"{(err / bound if bound else 0.0):.4f}; norm {norm:.17e} vs sqrt(S) {(norm - root) / math.ulp(root):+.2f} ulp")
    assert err <= bound, (label, err, bound)
    assert abs(norm - root) <= math.ulp(root), (label, norm, root)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ------------------------------------------------------------------ 1. the norm
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_norm_against_the_exact_sum_of_squares(n, off):
    for regime in REGIMES:
        gw, g = _buf(n, off, data=_data(n, regime))
        gd = Guard(n).run(g, INF, 1, 1)
        st, S = gd.host()
        _check_sum(S, st[0], _sumsq(n, regime), n, f"n={n} off={off} {regime}")
        assert all(math.isfinite(v) for v in st), st
        assert st[1:] == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], st         # coef exactly 1, nothing bad, seen once
        if regime == "zero":
            assert st[0] == 0.0 and S == 0.0
        else:
            assert st[0] > 0.0
        assert gd.intact() and _intact(gw, n, off)


# ------------------------------------------------------------------ 2. determinism and independence
@pytest.mark.parametrize("n", SIZES)
def test_state_is_bit_equal_across_alignment_reruns_and_longer_launches(n):
    x = _data(n, "k-2")
    runs = []
    for off in (0, 1, 0, 1):
        gw, g = _buf(n, off, data=x)
        gd = Guard(n).run(g, 1e-3, 1, 3)
        assert gd.intact() and _intact(gw, n, off)
        runs.append(gd)
    partial0, S0, bad0 = runs[0].views()
    for gd in runs[1:]:
        assert torch.equal(_bits(gd.state), _bits(runs[0].state))
        partial, S, bad = gd.views()
        assert torch.equal(_bits(partial), _bits(partial0)) and torch.equal(_bits(S), _bits(S0)) and torch.equal(bad, bad0)
    # the same gradient as the prefix of a longer one: the chunks that are whole in both keep their partial sums
    extra = CH + 77
    whole = n // CH
    for off in (0, 1):
        lw, lg = _buf(n + extra, off, data=torch.cat([x, _data(extra, "k-1")]))
        gd = Guard(n + extra).run(lg, 1e-3, 1, 3)
        partial, _, bad = gd.views()
        assert partial.numel() == -(-(n + extra) // CH)
        assert torch.equal(_bits(partial[:whole]), _bits(partial0[:whole])) and torch.equal(bad[:whole], bad0[:whole])
        assert gd.intact() and _intact(lw, n + extra, off)
    print(f"[guard] n={n}: state, {partial0.numel()} partial sums bit-equal over 4 runs, {whole} whole chunks kept in a longer launch")


# ------------------------------------------------------------------ 3. non-finite elements
def _positions(n):
    pos = {0, n - 1}
    if n % 4:
        pos.add(n // 4 * 4)                  # first element of the scalar tail
    if n >= CH:
        pos.update((CH - 1, n // CH * CH - 1))          # last element of the first / the last full chunk
    return sorted(pos)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_non_finite_elements_are_counted_and_left_out(n, off):
    x = _data(n, "k-1")
    gw, g = _buf(n, off, data=x)
    for i in _positions(n):
        for val in (float("nan"), INF, -INF):
            g[i] = val
            st, S = Guard(n).run(g, INF, 0, 1).host()
            g[i] = float(x[i])
            assert st[2] == 1.0 and st[3] == 0.0 and st[1] == 1.0, (i, val, st)
            _check_sum(S, st[0], _sumsq(n, "k-1", (i,)), n, f"n={n} off={off} {val} at {i}")
    # all of them at once, mixed; with skip_nonfinite the step is refused
    pos = _positions(n)
    for j, i in enumerate(pos):
        g[i] = (float("nan"), INF, -INF)[j % 3]
    gd = Guard(n).run(g, INF, 1, 1)
    st, S = gd.host()
    assert st[2] == float(len(pos)) and st[3] == 1.0 and st[1] == 0.0 and st[5] == 1.0, st
    _check_sum(S, st[0], _sumsq(n, "k-1", tuple(pos)), n, f"n={n} off={off} {len(pos)} non-finite")
    assert gd.intact() and _intact(gw, n, off)


# ------------------------------------------------------------------ 4. nothing triggers => nothing changes
@functools.lru_cache(maxsize=None)
def _grads(n):
    gen = torch.Generator().manual_seed(7 + n % 1000)
    return [torch.randn(n, generator=gen) * 10.0 ** k for k in (-3, -1, -5)], torch.randn(n, generator=gen), \
        torch.randn(n, generator=gen) * 2 + 3


def _adam_bufs(n, off, decay):
    """p, m, v (, ema) as [(whole, view)], from _grads(n)'s start values."""
    _, p0, e0 = _grads(n)
    bufs = [_buf(n, off, data=p0), _buf(n, off, fill=0.0), _buf(n, off, fill=0.0)]
    if decay is not None:
        bufs.append(_buf(n, off, data=e0))
    return bufs


def _plain_step(bufs, g, step, decay):
    from dvd_gan_amd import kern as K
    v = [b[1] for b in bufs]
    if decay is None:
        K.adam_step(v[0], g, v[1], v[2], *ADAM, step)
    else:
        K.adam_ema_step(v[0], g, v[1], v[2], v[3], *ADAM, step, decay)


def _guarded_step(bufs, g, step, decay, state):
    from dvd_gan_amd import kern as K
    v = [b[1] for b in bufs]
    K.adam_guard_step(v[0], g, v[1], v[2], None if decay is None else v[3], *ADAM, step, decay or 0.0, state)


def _same_bits(a, b, n, off, where):
    for (wa, va), (wb, vb), name in zip(a, b, "pmve"):
        assert torch.equal(_bits(va), _bits(vb)), (where, name, int((_bits(va) != _bits(vb)).sum()))
        assert _intact(wa, n, off) and _intact(wb, n, off), (where, name)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_guard_that_does_not_trigger_changes_no_bit(n, off):
    grads = _grads(n)[0]
    for mode in ("inf", "4 x norm"):
        for decay in (None, 0.0, 0.9, 0.9999):
            a, b = _adam_bufs(n, off, decay), _adam_bufs(n, off, decay)
            gd = Guard(n)
            for step, gh in enumerate(grads, 1):
                gw, g = _buf(n, off, data=gh)
                max_norm = INF if mode == "inf" else 4.0 * Guard(n).run(g).host()[0][0]
                gd.run(g, max_norm, 1, step)
                _guarded_step(b, g, step, decay, gd.state)
                _plain_step(a, g, step, decay)
                _same_bits(a, b, n, off, (mode, decay, step))
                st = gd.state.cpu().tolist()
                assert st[1] == 1.0 and st[3] == 0.0 and st[4] == float(step), st
                assert _intact(gw, n, off) and gd.intact()
            assert gd.state.cpu().tolist()[4:7] == [3.0, 0.0, 0.0]
            assert not torch.equal(b[0][1], _grads(n)[1].to(DEV))           # ... and the weights did move


# ------------------------------------------------------------------ 5. clipping
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_clipping_scales_the_gradient_by_the_float_coefficient(n, off):
    gw, g = _buf(n, off, data=_data(n, "k-2"))
    norm = Guard(n).run(g).host()[0][0]
    assert norm > 0.0
    max_norm = float(np.float32(norm / 4))
    for decay in (0.9, None):
        a, b = _adam_bufs(n, off, decay), _adam_bufs(n, off, decay)
        gd = Guard(n).run(g, max_norm, 1, 1)
        st = gd.state.cpu().tolist()
        want = max_norm / (norm + 1e-6)
        ulp = float(np.spacing(np.float32(want)))
        print(f"[guard] clip n={n} off={off}: norm {norm:.9e} max_norm {max_norm:.9e} coef {st[1]:.9e} host {want:.9e} "
              f"({(st[1] - want) / ulp:+.3f} fp32 ulp)")
        assert abs(st[1] - want) <= ulp and 0.0 < st[1] < 1.0 and st[1] == float(np.float32(st[1])), (st, want)
        assert st[0] == norm and st[3] == 0.0 and st[6] == 1.0 and st[5] == 0.0, st
        _guarded_step(b, g, 1, decay, gd.state)
        sw, scaled = _buf(n, off, fill=0.0)
        torch.mul(g, torch.tensor(st[1], dtype=torch.float32, device=DEV), out=scaled)        # torch's fp32 product
        _plain_step(a, scaled, 1, decay)
        _same_bits(a, b, n, off, ("clip", decay))
        assert gd.intact() and _intact(sw, n, off) and _intact(gw, n, off)
        # a max_norm a hair above the norm (norm + 1e-6 rounded up to a float): exactly 1, not counted
        hair = np.float32(norm * (1 + 1e-6) + 2e-6)
        assert float(hair) >= norm + 1e-6
        st = gd.run(g, float(hair), 1, 2).state.cpu().tolist()
        assert st[1] == 1.0 and st[6] == 1.0 and st[4] == 2.0, st


# ------------------------------------------------------------------ 6. skipping
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_skipped_step_writes_nothing_and_the_next_one_is_plain(n, off):
    """A clean step 1 (so that m, v and the average are not at their start values), a poisoned step 2, a clean step 3."""
    grads = _grads(n)[0]
    decay = 0.9
    b, twin = _adam_bufs(n, off, decay), _adam_bufs(n, off, decay)
    gw1, g1 = _buf(n, off, data=grads[2])
    gd = Guard(n).run(g1, INF, 1, 1)
    _guarded_step(b, g1, 1, decay, gd.state)
    _plain_step(twin, g1, 1, decay)
    _same_bits(twin, b, n, off, "before the skip")
    before = [v.clone() for _, v in b]
    assert bool((before[1] != 0).any()) and bool((before[2] != 0).any())
    gw, g = _buf(n, off, data=grads[0])
    g[n // 2] = INF
    gd.run(g, 1.0, 1, 2)
    _guarded_step(b, g, 2, decay, gd.state)
    st = gd.state.cpu().tolist()
    assert st[1] == 0.0 and st[2] == 1.0 and st[3] == 1.0 and st[4:7] == [2.0, 1.0, 0.0], st
    for (w, v), v0, name in zip(b, before, "pmve"):
        assert torch.equal(_bits(v), _bits(v0)), name
        assert _intact(w, n, off)
    # the next clean step, with its own step argument, is the plain launch (bias correction counts the skipped step)
    gw2, g2 = _buf(n, off, data=grads[1])
    gd.run(g2, INF, 1, 3)
    _guarded_step(b, g2, 3, decay, gd.state)
    _plain_step(twin, g2, 3, decay)
    _same_bits(twin, b, n, off, "after the skip")
    assert gd.state.cpu().tolist()[3:7] == [0.0, 3.0, 1.0, 0.0]
    assert not torch.equal(b[0][1], before[0])
    assert _intact(gw1, n, off)
    # skip_nonfinite off: the poisoned gradient goes through as dvd_adam_step takes it (NaN != NaN: compare the bit patterns)
    for val in (INF, float("nan")):
        g[n // 2] = val
        a, c = _adam_bufs(n, off, None), _adam_bufs(n, off, None)
        gd2 = Guard(n).run(g, INF, 0, 1)
        _guarded_step(c, g, 1, None, gd2.state)
        _plain_step(a, g, 1, None)
        _same_bits(a, c, n, off, ("poisoned", val))
        st = gd2.state.cpu().tolist()
        assert st[2] == 1.0 and st[3] == 0.0 and st[1] == 1.0 and st[5] == 0.0, st
        assert not bool(torch.isfinite(c[0][1][n // 2]))
    assert gd.intact() and gd2.intact() and _intact(gw, n, off) and _intact(gw2, n, off)


# ------------------------------------------------------------------ 7. the ring
@pytest.mark.parametrize("n", SIZES)
def test_ring_keeps_the_last_rows(n):
    x = _data(n, "k-1")
    for rows in (4, 8):
        gd = Guard(n, rows)
        want = {}
        for step in range(1, 7):
            gw, g = _buf(n, step % 2, data=x * float(step))
            if step == 4:
                g[n - 1] = float("nan")
            gd.run(g, 2.5 * _sumsq(n, "k-1") ** 0.5, 0, step)                 # clips from step 3 on
            st = gd.state.cpu().tolist()
            want[(step - 1) % rows] = [float(step), st[0], st[1], st[2]]
            assert _intact(gw, n, step % 2)
        ring = gd.ring.cpu()
        print(f"[guard] ring n={n} R={rows}: {ring.tolist()}")
        for r in range(rows):
            if r in want:
                assert ring[r].tolist() == want[r], (r, ring[r].tolist(), want[r])
            else:
                assert bool(torch.isnan(ring[r]).all()), r
        steps = sorted(row[0] for row in want.values())
        assert steps == ([3.0, 4.0, 5.0, 6.0] if rows == 4 else [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
        assert want[3 % rows][3] == 1.0                                      # step 4's NaN is in its row
        coefs = [want[(s - 1) % rows][2] for s in (5, 6)]
        assert all(0.0 < c < 1.0 for c in coefs), coefs
        assert gd.intact()


# ------------------------------------------------------------------ Trainer level
B, T, NCLS, ZD = 2, 8, 3, 16
NETS = (("G", "g_optimizer"), ("Ds", "ds_optimizer"), ("Dt", "dt_optimizer"))


def _trainer(**extra):
    from dvd_gan_amd.train_step import Trainer
    cfg = argparse.Namespace(adv_loss="hinge", z_dim=ZD, g_chn=2, ds_chn=2, dt_chn=2, n_frames=T, lr_schr="const", total_epoch=1,
                             d_iters=1, batch_size=B, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=NCLS, k_sample=4, **extra)
    torch.manual_seed(3)
    return Trainer([], cfg, device=torch.device(DEV), compute_dtype=torch.bfloat16)


def _batches(steps):
    gen = torch.Generator().manual_seed(11)
    out = []
    for _ in range(steps):
        real = torch.rand(B, 3, T, 64, 64, generator=gen) * 2 - 1
        labels = torch.randint(0, NCLS, (B,), generator=gen)
        draws = {"perm_real": torch.randperm(T, generator=gen), "z": torch.randn(B, ZD, generator=gen),
                 "z_class": torch.randint(0, NCLS, (B,), generator=gen), "perm_fake": torch.randperm(T, generator=gen)}
        out.append((real, labels, draws))
    return out


def _snapshot(tr):
    """flat / m / v (and ema) of the three optimizers and G's state_dict (clones)."""
    out = {f"G.{k}": v.detach().clone() for k, v in tr.G.state_dict().items()}
    for tag, name in NETS:
        opt = getattr(tr, name)
        for k in ("flat", "m", "v"):
            out[f"{tag}.opt.{k}"] = getattr(opt, k).detach().clone()
        if opt.ema is not None:
            out[f"{tag}.opt.ema"] = opt.ema.detach().clone()
    return out


def _differing(a, b, only=None):
    assert set(a) == set(b), set(a) ^ set(b)
    return [k for k in a if (only is None or k.startswith(only)) and not torch.equal(a[k], b[k])]


def _run(steps, **extra):
    """-> (trainer, losses per step, snapshot after each step)"""
    tr = _trainer(**extra)
    losses, snaps = [], []
    for real, labels, draws in _batches(steps):
        losses.append([float(v.detach()) for v in tr.train_step(real, labels, draws)])
        torch.cuda.synchronize()
        snaps.append(_snapshot(tr))
    return tr, losses, snaps


@pytest.fixture(scope="module")
def plain_run():
    return _run(2)


@pytest.fixture(scope="module")
def measured_run():
    return _run(2, grad_log=4, skip_nonfinite=True)


def _check_norms(tr, label):
    """grad_norms against the fp64 norm of each optimizer's `grad` as it stands after the step (test 1's bound on S)."""
    from dvd_gan_amd import kern as K
    norms = tr.grad_norms
    assert set(norms) == {"G", "Ds", "Dt"}
    for tag, name in NETS:
        opt = getattr(tr, name)
        assert norms[tag].dtype == torch.float64 and norms[tag].is_cuda and norms[tag].dim() == 0
        d = opt.grad.double().cpu()
        S_ref = math.fsum((d * d).tolist())
        S = float(K.grad_guard_ws_views(opt.guard_ws, opt.grad.numel())[1][0])
        _check_sum(S, float(norms[tag]), S_ref, opt.grad.numel(), f"{label} {tag} ({opt.grad.numel()} elements)")
        assert float(norms[tag]) > 0.0


def test_measuring_is_invisible(plain_run, measured_run):
    """(8) grad_log = 4, skip_nonfinite = True, no clipping norms: two steps are bit-equal to a Trainer with everything off."""
    _, la, sa = plain_run
    tr, lb, sb = measured_run
    assert la == lb, (la, lb)
    for a, b in zip(sa, sb):
        assert not _differing(a, b), _differing(a, b)[:10]
    assert not torch.equal(sa[0]["G.opt.flat"], sa[1]["G.opt.flat"])
    _check_norms(tr, "measure only")
    rep = tr.guard_report()
    for tag in ("G", "Ds", "Dt"):
        r = rep[tag]
        assert (r["seen"], r["skipped"], r["clipped"], r["bad"], r["skip"], r["coef"]) == (2, 0, 0, 0, False, 1.0), (tag, r)
        assert [row[0] for row in r["ring"]] == [1.0, 2.0] and r["ring"][1][1] == r["norm"] == float(tr.grad_norms[tag])
        assert getattr(tr, dict(NETS)[tag]).guard_ring.shape == (4, 4)


def test_measuring_is_invisible_with_regularizer_and_average():
    """(8, second half) with g_ortho > 0 and ema_decay > 0: the norm is taken after the regularizer's term went into `grad`, the
    average is updated by the guarded launch -- still bit-equal, the average included."""
    extra = dict(g_ortho=1e-4, ema_decay=0.9)
    _, la, sa = _run(2, **extra)
    tr, lb, sb = _run(2, grad_log=4, skip_nonfinite=True, **extra)
    assert la == lb, (la, lb)
    for a, b in zip(sa, sb):
        assert "G.opt.ema" in a and not _differing(a, b), _differing(a, b)[:10]
    assert not torch.equal(sb[1]["G.opt.ema"], sb[1]["G.opt.flat"])
    _check_norms(tr, "measure only, ortho + ema")


def test_generator_clipping(plain_run, measured_run):
    """(9) g_clip_norm = a quarter of the generator's norm at step 1: G's update is dvd_adam_step on grad * coef32 from the
    snapshotted p, m, v; D_s and D_t are bit-equal to the unguarded run."""
    from dvd_gan_amd import kern as K
    _, _, plain = plain_run
    seen = measured_run[0].guard_report()["G"]["ring"][0]
    assert seen[0] == 1.0
    tr = _trainer(g_clip_norm=seen[1] / 4)
    opt, snap = tr.g_optimizer, {}
    orig = opt.step

    def stepper():
        snap.update(p=opt.flat.clone(), m=opt.m.clone(), v=opt.v.clone(), g=opt.grad.clone())
        orig()
    opt.step = stepper
    real, labels, draws = _batches(1)[0]
    tr.train_step(real, labels, draws)
    torch.cuda.synchronize()
    rep = tr.guard_report()
    print(f"[guard] Trainer clip: G norm {rep['G']['norm']:.6e} (measured run {seen[1]:.6e}), coef {rep['G']['coef']:.6e}")
    assert rep["G"]["norm"] == seen[1]
    assert 0.2 < rep["G"]["coef"] < 0.3 and rep["G"]["clipped"] == 1 and rep["G"]["skipped"] == 0
    assert rep["Ds"] is None and rep["Dt"] is None and tr.grad_norms["Ds"] is None
    assert tr.ds_optimizer.guard_state is None and tr.dt_optimizer.guard_state is None
    K.adam_step(snap["p"], snap["g"] * torch.tensor(rep["G"]["coef"], dtype=torch.float32, device=DEV), snap["m"], snap["v"],
                2e-3, 0.0, 0.9, 1e-8, 1)
    torch.cuda.synchronize()
    for k in "pmv":
        assert torch.equal(_bits(snap[k]), _bits(getattr(opt, {"p": "flat"}.get(k, k)))), k
    after = _snapshot(tr)
    assert not _differing(plain[0], after, only="Ds.") and not _differing(plain[0], after, only="Dt.")
    assert _differing(plain[0], after, only="G.opt.flat")


def test_poisoned_discriminator_step_is_skipped():
    """(10) one +inf written into D_s's gradient buffer right before its Adam launch of step 1."""
    tr = _trainer(skip_nonfinite=True, grad_log=4)
    opt, calls = tr.ds_optimizer, []
    orig = opt.step

    def stepper():
        calls.append(1)
        if len(calls) == 1:
            opt.grad[5] = INF
        orig()
    opt.step = stepper
    start = _snapshot(tr)
    (b1, b2) = _batches(2)
    tr.train_step(*b1)
    torch.cuda.synchronize()
    one = _snapshot(tr)
    assert not _differing(start, one, only="Ds.opt."), _differing(start, one, only="Ds.opt.")
    rep = tr.guard_report()
    assert rep["Ds"]["skipped"] == 1 and rep["Ds"]["bad"] == 1 and rep["Ds"]["coef"] == 0.0 and rep["Ds"]["skip"] is True
    for tag in ("Dt", "G"):
        assert rep[tag]["skipped"] == 0 and rep[tag]["seen"] == 1
        assert _differing(start, one, only=f"{tag}.opt.flat")
    assert all(bool(torch.isfinite(v).all()) for k, v in one.items() if v.is_floating_point())
    tr.train_step(*b2)
    torch.cuda.synchronize()
    two = _snapshot(tr)
    for tag in ("Ds", "Dt", "G"):
        assert _differing(one, two, only=f"{tag}.opt.flat"), tag
    assert all(bool(torch.isfinite(v).all()) for k, v in two.items() if v.is_floating_point())
    rep = tr.guard_report()
    print(f"[guard] Trainer skip: D_s ring {rep['Ds']['ring']}")
    assert rep["Ds"]["skipped"] == 1 and rep["Ds"]["seen"] == 2 and rep["Ds"]["skip"] is False and rep["Ds"]["coef"] == 1.0
    ring = rep["Ds"]["ring"]
    assert [r[0] for r in ring] == [1.0, 2.0] and ring[0][2] == 0.0 and ring[0][3] == 1.0 and ring[1][2:] == [1.0, 0.0]
    assert len(calls) == 2


def test_defaults_allocate_nothing_on_the_device(plain_run):
    """(11) all four config fields at their defaults, after two steps."""
    tr = plain_run[0]
    assert tr.grad_norms is None and tr.guard_report() is None
    for _, name in NETS:
        opt = getattr(tr, name)
        assert opt.guard is False and opt.guard_ws is None and opt.guard_state is None and opt.guard_ring is None
        assert opt.grad_norm is None and opt.t == 2


def test_train_log_line_names_the_guard_only_when_it_is_on(capsys):
    """train() on a one-batch loader: the line it prints every log_epoch carries norms and skip counts with a guard, and is the
    line it was without one."""
    real, labels, _ = _batches(1)[0]
    lines = {}
    for on in (False, True):
        tr = _trainer(log_epoch=1, **(dict(grad_log=2, d_clip_norm=1e-3) if on else {}))
        tr.data_loader = [(real, labels)]
        capsys.readouterr()
        tr.train()
        lines[on] = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Step: [1/1]")]
        assert len(lines[on]) == 1, lines[on]
    print(lines[True][0])
    assert "|g|" not in lines[False][0] and "skipped" not in lines[False][0] and lines[False][0].rstrip().split(", ")[-1].startswith("lr:")
    for tag in ("G", "Ds", "Dt"):
        assert f", {tag} |g|: " in lines[True][0]
    assert lines[True][0].count("skipped: 0") == 3
    rep = tr.guard_report()
    assert rep["Ds"]["clipped"] == 1 and rep["Dt"]["clipped"] == 1 and rep["G"]["clipped"] == 0 and rep["G"]["coef"] == 1.0

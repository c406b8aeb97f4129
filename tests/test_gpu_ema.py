"""Generator weight average (EMA) on the GPU: the three C entry points called directly, then the Trainer.

Kernel level
  1. dvd_adam_ema_step leaves p, m, v BIT-EQUAL to dvd_adam_step (sizes 1 .. 2^20 + 5, aligned and one float off alignment).
  2. The average against the fp64 recurrence e <- d e + (1 - d) p on the STORED fp32 p of each step, with the float-rounded d and
     1 - d the library forms.  Bound (derived, not tuned): a step adds at most three fp32 roundings of terms no larger than
     M = max(|e|, |p|) over the steps, earlier errors are multiplied by d <= 1, so |ema - ref| <= K * 2^-22 * M after K steps.
     d = 0 gives ema == p bit for bit; dvd_ema_step on the same inputs is bit-equal to the fused average.
  3. dvd_swap_f32 exchanges bit for bit, twice = identity, nothing past n is touched.
Trainer level
  4. training does not notice the average (bf16, ch = 32: losses, state_dicts, flat / m / v bit-equal with and without it);
  5. the average follows the fp64 recurrence over snapshots of the weights, starting from the weights the FIRST STEP started from;
  6. sample(use_ema=True) against the oracle's eval-mode generator on the GPU's own averaged weights;
  7. ema_weights() leaves no trace (state, default RNG, the next step);  8. standing statistics (arithmetic and against the
  oracle);  9. frame-conditional predict(use_ema=True);  10. the `{step}_G_ema.pth` checkpoint.
Every figure is printed before it is asserted ("[ema] ...", pytest -s).  Where each bound comes from and the mutants this file
is built to catch: profiles/ema_numbers.md.
"""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 10007, 2 ** 20 + 5]
PAD = 8                      # guard elements behind every buffer
SENTINEL = -12345.5


# ------------------------------------------------------------------ kernel level
def _buf(n, off, fill=None, gen=None, scale=1.0):
    """-> (whole, view): `view` = n elements starting `off` floats into a fresh device buffer (off = 1: every pointer one float
    off a 16-byte boundary); the elements around the view hold SENTINEL."""
    whole = torch.full((off + n + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = whole[off:off + n]
    if fill is not None:
        view.fill_(fill)
    else:
        view.copy_((torch.randn(n, generator=gen) * scale).to(DEV))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return whole, view


def _guards_intact(whole, n, off):
    return bool((whole[:off] == SENTINEL).all()) and bool((whole[off + n:] == SENTINEL).all())


def _grad(n, gen):
    return (torch.randn(n, generator=gen) * 10 ** float(torch.randint(-6, 1, (), generator=gen))).to(DEV)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_half_of_the_fused_launch_is_bit_equal_to_adam_step(n, off):
    from dvd_gan_amd import kern as K
    gen = torch.Generator().manual_seed(3)
    a = [_buf(n, off, gen=gen), _buf(n, off, fill=0.0), _buf(n, off, fill=0.0)]          # p, m, v of dvd_adam_step
    b = [_buf(n, off, fill=0.0) for _ in range(3)]                                     # ... of dvd_adam_ema_step
    b[0][1].copy_(a[0][1])
    ew, e = _buf(n, off, gen=gen)
    for step in range(1, 4):
        gw, g = _buf(n, off, fill=0.0)
        g.copy_(_grad(n, gen))
        K.adam_step(a[0][1], g, a[1][1], a[2][1], 2e-3, 0.0, 0.9, 1e-8, step)
        K.adam_ema_step(b[0][1], g, b[1][1], b[2][1], e, 2e-3, 0.0, 0.9, 1e-8, step, 0.9)
        for (wa, va), (wb, vb), name in zip(a, b, "pmv"):
            assert torch.equal(va, vb), (name, step, float((va - vb).abs().max()))
            assert _guards_intact(wb, n, off) and _guards_intact(wa, n, off), (name, step)
        assert _guards_intact(ew, n, off) and _guards_intact(gw, n, off)
    assert bool(torch.isfinite(b[0][1]).all()) and not torch.equal(b[0][1], e)


def _decay_pair(d):
    """The float d the library receives and the float (1 - d) it forms in double."""
    d32 = np.float32(d)
    return float(d32), float(np.float32(1.0 - np.float64(d32)))


def _check_average(got, e0, ps, ds, label):
    """got: the device average after len(ps) steps; e0: its start (fp32); ps: the stored fp32 weights after each step; ds: the
    decay of each step.  -> (max |err|, max err / bound)."""
    e = e0.double().cpu()
    big = e.abs()
    for p, d in zip(ps, ds):
        d32, omd32 = _decay_pair(d)
        e = d32 * e + omd32 * p.double().cpu()
        big = torch.maximum(big, torch.maximum(e.abs(), p.double().cpu().abs()))
    err = (got.double().cpu() - e).abs()
    bound = len(ps) * 2.0 ** -22 * big
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"[ema] {label}: max |ema - fp64| {float(err.max()):.3e}, worst error / bound {worst:.3f}")
    assert bool((err <= bound).all()), (label, float(err.max()), worst)
    return float(err.max()), worst


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_average_matches_fp64_recurrence_of_the_stored_weights(n, off):
    from dvd_gan_amd import kern as K
    for d in (0.0, 0.5, 0.9, 0.9999):
        gen = torch.Generator().manual_seed(5)
        pw, p = _buf(n, off, gen=gen)
        mw, m = _buf(n, off, fill=0.0)
        vw, v = _buf(n, off, fill=0.0)
        ew, e = _buf(n, off, gen=gen, scale=2.0)          # far from p: an element the kernel skips keeps a visibly wrong value
        e.add_(3.0)
        e0 = e.clone()
        e2 = e.clone()                                    # dvd_ema_step on the same inputs
        ps = []
        for step in range(1, 4):
            g = _grad(n, gen)
            K.adam_ema_step(p, g, m, v, e, 2e-3, 0.0, 0.9, 1e-8, step, d)
            K.ema_step(e2, p, d)
            ps.append(p.clone())
            assert torch.equal(e, e2), (d, step)
            if d == 0.0:
                assert torch.equal(e, p), step            # decay 0: the average IS the updated weights
        _check_average(e, e0, ps, [d] * 3, f"n={n} off={off} d={d}")
        for w in (pw, mw, vw, ew):
            assert _guards_intact(w, n, off), d


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bit_for_bit(n, off):
    from dvd_gan_amd import kern as K
    gen = torch.Generator().manual_seed(7)
    aw, a = _buf(n, off, gen=gen)
    bw, b = _buf(n, off, gen=gen)
    a0, b0 = a.clone(), b.clone()
    K.swap_(a, b)
    assert torch.equal(a, b0) and torch.equal(b, a0)
    assert _guards_intact(aw, n, off) and _guards_intact(bw, n, off)
    K.swap_(a, b)
    assert torch.equal(a, a0) and torch.equal(b, b0)
    assert _guards_intact(aw, n, off) and _guards_intact(bw, n, off)


# ------------------------------------------------------------------ Trainer level
def _cfg(ch, T, k, B, ncls, zd, lr=5e-5, **extra):
    return argparse.Namespace(adv_loss="hinge", z_dim=zd, g_chn=ch, ds_chn=ch, dt_chn=ch, n_frames=T, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=B, g_lr=lr, d_lr=lr, beta1=0.0, beta2=0.9,
                              n_class=ncls, k_sample=k, **extra)


def _trainer(cfg, dtype, seed):
    from dvd_gan_amd.train_step import Trainer
    torch.manual_seed(seed)
    return Trainer([], cfg, device=torch.device(DEV), compute_dtype=dtype)


def _draws(gen, B, T, ncls, zd, frames=None, size=64):
    """Clips, labels and the step's RNG draws from a private generator (tools/repro_probe.py's run, restated)."""
    real = torch.rand(B, 3, frames or T, size, size, generator=gen) * 2 - 1
    labels = torch.randint(0, ncls, (B,), generator=gen)
    draws = {"perm_real": torch.randperm(T, generator=gen), "z": torch.randn(B, zd, generator=gen),
             "z_class": torch.randint(0, ncls, (B,), generator=gen), "perm_fake": torch.randperm(T, generator=gen)}
    return real, labels, draws


def _state(tr):
    """Every tensor training owns: the three state_dicts and flat / m / v of the three optimizers (clones)."""
    out = {}
    for tag, net, opt in (("G", tr.G, tr.g_optimizer), ("Ds", tr.D_s, tr.ds_optimizer), ("Dt", tr.D_t, tr.dt_optimizer)):
        for k, v in net.state_dict().items():
            out[f"{tag}.{k}"] = v.detach().clone()
        for k in ("flat", "m", "v"):
            out[f"{tag}.opt.{k}"] = getattr(opt, k).detach().clone()
    if tr.g_optimizer.ema is not None:
        out["G.opt.ema"] = tr.g_optimizer.ema.detach().clone()
    return out


def _differing(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def _bf16_run(steps, ch=32, T=8, B=2, ncls=7, **extra):
    """tools/repro_probe.py's run (seed 3, clips and draws from generator 11) with extra config keys."""
    tr = _trainer(_cfg(ch, T, min(8, T), B, ncls, 120, **extra), torch.bfloat16, 3)
    gen = torch.Generator().manual_seed(11)
    losses = []
    for _ in range(steps):
        real, labels, draws = _draws(gen, B, T, ncls, 120)
        losses.append([float(v.detach()) for v in tr.train_step(real, labels, draws)])
    torch.cuda.synchronize()
    return tr, gen, losses


def test_training_does_not_notice_the_average():
    """(4) Two bf16 Trainers from one seed at ch = 32, one with ema_decay = 0.999: after two steps the six losses, every entry of
    the three state_dicts and flat / m / v are bit-equal."""
    plain, _, la = _bf16_run(2)
    sa = _state(plain)
    del plain
    avg, _, lb = _bf16_run(2, ema_decay=0.999)
    sb = _state(avg)
    assert avg.g_optimizer.ema is not None and avg.ds_optimizer.ema is None and avg.dt_optimizer.ema is None
    assert not torch.equal(sb.pop("G.opt.ema"), sb["G.opt.flat"])
    assert la == lb, (la, lb)
    assert sa
    assert not _differing(sa, sb), _differing(sa, sb)[:10]


def test_average_follows_fp64_recurrence_from_the_first_steps_weights():
    """(5) Exact mode, ch = 2, T = 8, B = 2, ema_decay = 0.9.  The generator's weights are overwritten between construction and
    the first step (as a checkpoint load or the rank-0 broadcast does): the average must start from the weights the first step
    started from.  ema_start = 1 (decay 0 through step 1, so after it ema == flat bit for bit) over 4 steps, and ema_start = 0
    over 2 steps -- with ema_start = 1 the first launch overwrites the average whatever it held, so only the second run sees
    where the average started."""
    ch, T, k, B, ncls, zd = 2, 8, 4, 2, 3, 16
    for start, steps in ((1, 4), (0, 2)):
        tr = _trainer(_cfg(ch, T, k, B, ncls, zd, ema_decay=0.9, ema_start=start), torch.float32, 17)
        opt = tr.g_optimizer
        assert opt.ema is None
        with torch.no_grad():
            opt.flat.add_(0.05 * torch.randn(opt.flat.numel(), generator=torch.Generator().manual_seed(1)).to(DEV))
        w0 = opt.flat.clone()
        gen = torch.Generator().manual_seed(19)
        snaps = []
        for s in range(steps):
            real, labels, draws = _draws(gen, B, T, ncls, zd)
            tr.train_step(real, labels, draws)
            snaps.append(opt.flat.clone())
            if s == 0 and start == 1:
                assert torch.equal(opt.ema, opt.flat)
        assert not torch.equal(snaps[0], w0)
        decays = [0.0 if t <= start else 0.9 for t in range(1, steps + 1)]
        _check_average(opt.ema, w0, snaps, decays, f"trajectory ema_start={start}")
        assert tr.ds_optimizer.ema is None and tr.dt_optimizer.ema is None


def _averaged_state(tr):
    """G.state_dict() on the host with the trainable entries replaced by the matching slices of the GPU's `ema`."""
    sd = {k: v.detach().cpu().clone() for k, v in tr.G.state_dict().items()}
    ema, off = tr.g_optimizer.ema.detach().cpu(), 0
    for name, p in tr.G.named_parameters():
        if p.requires_grad:
            sd[name] = ema[off:off + p.numel()].view(p.shape).clone()
            off += p.numel()
    assert off == ema.numel()
    return sd


def _small_exact_trainer(steps, seed=21, **extra):
    ch, T, k, B, ncls, zd = 2, 8, 4, 2, 3, 16
    extra.setdefault("ema_decay", 0.9)
    tr = _trainer(_cfg(ch, T, k, B, ncls, zd, **extra), torch.float32, seed)
    for _ in range(steps):
        tr.train_step(torch.rand(B, 3, T, 64, 64) * 2 - 1, torch.randint(0, ncls, (B,)))
    return tr, (ch, T, k, B, ncls, zd)


def test_sampling_with_the_average_matches_oracle():
    """(6) As test_sampling_path_matches_oracle (same shape, lr 5e-5), after three steps with ema_decay = 0.9, through
    sample(z, y, use_ema=True, standing_stats=0): the oracle's eval-mode generator on the GPU's own averaged weights, 2e-3
    absolute; and more than 4e-3 away from the live-weight sample somewhere, so a swap that never happened fails."""
    from oracle import dvdgan_cpu as O
    tr, (ch, T, k, B, ncls, zd) = _small_exact_trainer(3)
    sd = O.make_state(_averaged_state(tr), requires_grad=False)
    fixed_z, fixed_label = torch.randn(B, zd), torch.randint(0, ncls, (B,))
    with torch.no_grad():
        want = ((O.generator(sd, fixed_z, fixed_label, ch, T, training=False) + 1) / 2).clamp(0, 1)
    got = tr.sample(fixed_z, fixed_label, use_ema=True, standing_stats=0)
    assert tr.G.training
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    err = float((got.cpu() - want).abs().max())
    live = tr.sample(fixed_z, fixed_label)
    apart = float((got - live).abs().max())
    print(f"[ema] sample(use_ema) vs oracle: max abs {err:.3e}; averaged vs live weights: max abs {apart:.3e}")
    assert err < 2e-3, err
    assert apart > 4e-3, apart


def _no_trace_check(tr, twin, gen, sample_fn, B, T, ncls, zd, frames=None):
    """(7): state, default RNG and the next step are what they would be without the sampling in `sample_fn`."""
    before, rng = _state(tr), torch.get_rng_state()
    sample_fn()
    torch.cuda.synchronize()
    assert torch.equal(rng, torch.get_rng_state())
    after = _state(tr)
    assert "G.opt.ema" in before
    assert not _differing(before, after), _differing(before, after)[:10]
    assert tr.G.training
    from dvd_gan_amd.sn_layers import ConditionalNorm
    assert all(m.momentum == 0.1 for m in tr.G.modules() if isinstance(m, ConditionalNorm))
    real, labels, draws = _draws(gen, B, T, ncls, zd, frames=frames)
    la = [float(v.detach()) for v in tr.train_step(real, labels, draws)]
    lb = [float(v.detach()) for v in twin.train_step(real, labels, draws)]
    assert la == lb, (la, lb)
    assert not _differing(_state(tr), _state(twin))


def test_ema_weights_context_leaves_no_trace():
    """(7) bf16, ch = 32: every tensor of the state_dicts, flat, ema, m, v bit-equal before and after a block with two
    standing-statistics passes and a forward; the default generator untouched; the next train_step bit-equal to a twin's."""
    tr, gen, l1 = _bf16_run(2, ema_decay=0.9)
    twin, _, l2 = _bf16_run(2, ema_decay=0.9)
    assert l1 == l2
    B, T, ncls, zd = 2, 8, 7, 120
    z, y = torch.randn(B, zd, generator=gen).to(DEV), torch.randint(0, ncls, (B,), generator=gen).to(DEV)
    seen = {}

    def sample():
        with tr.ema_weights(standing_stats=2) as G:
            assert G is tr.G
            seen["inside"] = not torch.equal(tr.g_optimizer.flat, _state(twin)["G.opt.flat"])
            with torch.no_grad():
                seen["out"] = tr.G(z, y)
    _no_trace_check(tr, twin, gen, sample, B, T, ncls, zd)
    assert seen["inside"] and bool(torch.isfinite(seen["out"]).all())


def _norm_layers(G):
    from dvd_gan_amd.sn_layers import ConditionalNorm
    return [(name, m) for name, m in G.named_modules() if isinstance(m, ConditionalNorm)]


def test_standing_statistics(monkeypatch):
    """(8) Exact mode, ch = 2, N = 3.  (a) Arithmetic, against the GPU's own passes replayed with momentum 1 (running_mean /
    running_var are then that pass's batch mean and unbiased variance): the standing statistics are the plain mean of the three,
    1e-5 relative + 1e-7 absolute (N roundings of the stored float + the order-dependence of the fp64 statistics atomics), all
    sixteen layers.  (b) Semantics, against the oracle's train-mode generator on the averaged weights with its batch-norm
    momentum patched to 1 / i, on the keys and at the 2e-4 of test_two_discriminator_iterations_per_step_match_oracle."""
    from oracle import dvdgan_cpu as O
    N, seed = 3, 5
    tr, (ch, T, k, B, ncls, zd) = _small_exact_trainer(3, ema_stats_seed=seed)
    layers = _norm_layers(tr.G)
    assert len(layers) == 16
    live = {name: (m.bn.running_mean.clone(), m.bn.running_var.clone()) for name, m in layers}
    sd = O.make_state(_averaged_state(tr), requires_grad=False)
    rng = torch.get_rng_state()
    with tr.ema_weights(standing_stats=N):
        stand = {name: (m.bn.running_mean.clone(), m.bn.running_var.clone()) for name, m in layers}
        assert all(int(m.bn.num_batches_tracked) == N for _, m in layers)
    assert torch.equal(rng, torch.get_rng_state())
    assert all(torch.equal(m.bn.running_mean, live[name][0]) and torch.equal(m.bn.running_var, live[name][1]) for name, m in layers)
    # (a) replay with momentum 1
    passes = []
    gen = torch.Generator().manual_seed(seed)
    with tr.ema_weights():
        for _, m in layers:
            m.momentum = 1.0
        for i in range(N):
            z, y = tr.standing_draws(gen, B)
            with torch.no_grad():
                tr.G(z.to(DEV), y.to(DEV))
            passes.append({name: (m.bn.running_mean.double().clone(), m.bn.running_var.double().clone()) for name, m in layers})
    worst = 0.0
    for name, _ in layers:
        for j, what in enumerate(("running_mean", "running_var")):
            want = sum(p[name][j] for p in passes) / N
            got = stand[name][j].double()
            err = (got - want).abs()
            worst = max(worst, float((err / (1e-5 * want.abs() + 1e-7)).max()))
            assert bool((err <= 1e-5 * want.abs() + 1e-7).all()), (name, what, float(err.max()))
        assert not torch.equal(stand[name][0], live[name][0])
    print(f"[ema] standing statistics vs mean of momentum-1 passes: worst error / bound {worst:.3f}")
    # (b) the oracle, momentum 1 / i
    import torch.nn.functional as F
    orig, mom = F.batch_norm, [None]

    def patched(x, rm, rv, w, b, training, momentum, eps):
        return orig(x, rm, rv, w, b, training, mom[0], eps)
    monkeypatch.setattr(F, "batch_norm", patched)
    gen = torch.Generator().manual_seed(seed)
    for i in range(1, N + 1):
        mom[0] = 1.0 / i
        z, y = tr.standing_draws(gen, B)
        with torch.no_grad():
            O.generator(sd, z, y, ch, T, training=True)
    monkeypatch.undo()
    for key in ("conv.1.CBNorm1.bn.running_mean", "conv.1.CBNorm2.bn.running_var"):
        name, what = key.rsplit(".bn.", 1)
        got = stand[name][0 if what == "running_mean" else 1]
        err = float((got.cpu() - sd[key]).abs().max())
        print(f"[ema] standing {key} vs oracle: max abs {err:.3e}")
        assert err < 2e-4, (key, err)


def test_frame_conditional_predict_with_the_average():
    """(9) n_cond = 4 at the small shape of tests/test_gpu_cond.py (bf16, so that a twin Trainer is comparable bit for bit):
    predict(cond, y, z, use_ema=True) with standing statistics on the caller's context runs, lies in [0, 1], differs from
    the live-weight prediction and leaves no trace."""
    ch, K, T, k, B, ncls, zd = 8, 4, 8, 4, 2, 3, 16
    cfg = dict(n_cond=K, ema_decay=0.9, lr=2e-3)
    tr = _trainer(_cfg(ch, T, k, B, ncls, zd, **cfg), torch.bfloat16, 43)
    twin = _trainer(_cfg(ch, T, k, B, ncls, zd, **cfg), torch.bfloat16, 43)
    ga, gb = torch.Generator().manual_seed(47), torch.Generator().manual_seed(47)
    for _ in range(2):
        real, labels, draws = _draws(ga, B, T, ncls, zd, frames=K + T)
        la = [float(v.detach()) for v in tr.train_step(real, labels, draws)]
        lb = [float(v.detach()) for v in twin.train_step(*_draws(gb, B, T, ncls, zd, frames=K + T))]
        assert la == lb, (la, lb)
    cond = real[:, :, :K].permute(0, 2, 1, 3, 4).contiguous()
    z = torch.randn(B, zd, generator=ga)
    seen = {}

    def sample():
        seen["ema"] = tr.predict(cond, labels, z, use_ema=True)
        seen["stand"] = tr.predict(cond, labels, z, use_ema=True, standing_stats=2)
    _no_trace_check(tr, twin, ga, sample, B, T, ncls, zd, frames=K + T)
    for p in seen.values():
        assert tuple(p.shape) == (B, T, 3, 64, 64)
        assert float(p.min()) >= 0.0 and float(p.max()) <= 1.0 and bool(torch.isfinite(p).all())
    assert not torch.equal(seen["ema"], seen["stand"])
    assert not torch.equal(seen["ema"], tr.predict(cond, labels, z))
    with pytest.raises(ValueError, match="truncation"):
        tr.predict(cond, labels, z, truncation=0.5)
    t = tr.predict(cond, labels, use_ema=True, truncation=0.5)
    assert tuple(t.shape) == (B, T, 3, 64, 64) and bool(torch.isfinite(t).all())


@pytest.mark.parametrize("n_stand", [0, 3])
def test_checkpoint_of_the_average(tmp_path, n_stand):
    """(10) `{step}_G_ema.pth`: exactly the keys of `{step}_G.pth`, trainable entries bit-equal to the slices of `ema`, the others
    equal to the live ones (ema_standing_stats = 0) or to the standing statistics (3); a fresh Trainer with pretrained_model
    = step has a bit-equal `ema`; with the file removed its average equals the loaded weights."""
    from dvd_gan_amd.train_step import Trainer
    extra = dict(ema_standing_stats=n_stand, ema_stats_seed=5, model_save_path=str(tmp_path))
    tr, (ch, T, k, B, ncls, zd) = _small_exact_trainer(3, **extra)
    before = _state(tr)
    tr.save_models(3)
    assert not _differing(before, _state(tr))
    assert sorted(os.listdir(str(tmp_path))) == ["3_Ds.pth", "3_Dt.pth", "3_G.pth", "3_G_ema.pth"]
    live = torch.load(os.path.join(str(tmp_path), "3_G.pth"))
    avg = torch.load(os.path.join(str(tmp_path), "3_G_ema.pth"))
    assert list(avg) == list(live)
    want = _averaged_state(tr)
    trainable = {name for name, p in tr.G.named_parameters() if p.requires_grad}
    if n_stand:
        with tr.ema_weights(standing_stats=n_stand):
            stand = {kk: v.detach().cpu().clone() for kk, v in tr.G.state_dict().items()}
    moved = 0
    for key in live:
        if key in trainable:
            assert torch.equal(avg[key], want[key]), key
            moved += int(not torch.equal(avg[key], live[key]))
        elif n_stand == 0:
            assert torch.equal(avg[key], live[key]), key
        elif key.endswith(("running_mean", "running_var")):
            # a second run of the same passes: equal up to the order of the fp64 statistics atomics (bound of test 8)
            err = (avg[key].double() - stand[key].double()).abs()
            assert bool((err <= 1e-5 * stand[key].double().abs() + 1e-7).all()), key
            assert not torch.equal(avg[key], live[key]), key
        elif key.endswith("num_batches_tracked"):
            assert int(avg[key]) == n_stand, key
        else:
            # spectral-norm u / v: advanced by the N passes on the averaged weights, the same way in both runs
            assert key.endswith(("weight_u", "weight_v")), key
            assert torch.equal(avg[key], stand[key]), key
            assert not torch.equal(avg[key], live[key]), key
    assert moved >= len(trainable) // 2
    # the file loads into a plain Generator
    from dvd_gan_amd.gen_net import Generator
    Generator(zd, 4, ncls, ch, T).load_state_dict(avg)
    # a fresh Trainer resumes the average from the file ...
    torch.manual_seed(99)
    cfg = _cfg(ch, T, k, B, ncls, zd, ema_decay=0.9, pretrained_model=3, **extra)
    new = Trainer([], cfg, device=torch.device(DEV), compute_dtype=torch.float32)
    assert torch.equal(new.g_optimizer.ema, tr.g_optimizer.ema)
    assert torch.equal(new.g_optimizer.flat, tr.g_optimizer.flat)
    # ... and without the file starts it from the loaded weights
    os.remove(os.path.join(str(tmp_path), "3_G_ema.pth"))
    new = Trainer([], cfg, device=torch.device(DEV), compute_dtype=torch.float32)
    assert new.g_optimizer.ema is None
    new.train_step(torch.rand(B, 3, T, 64, 64) * 2 - 1, torch.randint(0, ncls, (B,)))
    # decay 0.9 from e0 = the loaded weights w0: ema - p1 = 0.9 (w0 - p1), against 0 had it started anywhere else
    p1 = new.g_optimizer.flat.double()
    w0 = tr.g_optimizer.flat.double()
    assert float((new.g_optimizer.ema.double() - (0.9 * w0 + 0.1 * p1)).abs().max()) < 1e-6

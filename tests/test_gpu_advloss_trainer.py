"""LeCam regularization, top-k generator updates and the logit statistics inside the Trainer's step (train_step.Trainer:
config.lecam / lecam_decay / lecam_start / g_topk / g_topk_decay / d_stats), at the small widths of the other trainer tests.  The
logits every loss call saw are recorded by wrapping `calc_loss`, and tests/adv_ref.py says what had to come of them."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

import adv_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E32 = 2.0 ** -24
CH, T, K, NCLS, ZD = 2, 8, 4, 3, 16
f32 = lambda v: float(np.float32(v))


def _seed(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _trainer(B=2, folder=None, **over):
    from dvd_gan_amd.train_step import Trainer
    cfg = dict(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T, lr_schr="const", total_epoch=1, d_iters=1,
               batch_size=B, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=NCLS, k_sample=K, log_epoch=0)
    if folder is not None:
        cfg.update(model_save_path=str(folder), version="")
    cfg.update(over)
    return Trainer([], argparse.Namespace(**cfg), device=DEV, compute_dtype=torch.float32)


def _clips(B, steps, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, T, 64, 64, generator=g) * 2 - 1, torch.randint(0, NCLS, (B,), generator=g)) for _ in range(steps)]


def _record(tr):
    """Wrap tr.calc_loss: -> list of (site, logits, dout the launch saved for the backward pass), in call order."""
    rec, orig = [], tr.calc_loss

    def calc_loss(x, real_flag, **kw):
        loss = orig(x, real_flag, **kw)
        rec.append((kw.get("_site"), x.detach().reshape(-1).clone(), loss.grad_fn.saved_tensors[0].reshape(-1).clone()))
        return loss
    tr.calc_loss = calc_loss
    return rec


@pytest.mark.parametrize("early", [False, True])
def test_anchors_follow_the_recursion_over_steps(early, monkeypatch):
    """early: the discriminators' passes over the real clips run ahead on a second stream (DVD_D_REAL_EARLY=1), so a network's
    real call and its fake call are issued on different streams: they touch different floats of the anchors."""
    from test_gpu_advloss import sum_bound
    B, lam, decay = 3, f32(0.5), f32(0.9)
    monkeypatch.setenv("DVD_D_REAL_EARLY", "1" if early else "0")
    _seed(5)
    tr = _trainer(B, lecam=lam, lecam_decay=decay, lecam_start=1, d_stats=True)
    assert tr._anchors.shape == (2, 2, 2) and tr._adv_stats.shape == (6, 8) and tr.d_stats()["it"] == 0
    rec = _record(tr)
    anchors = np.zeros((2, 2))                 # [net][kind], the reference's, in fp64
    err = np.zeros((2, 2))                     # ... and how far the fp32 ones may be from them
    for step, (clips, labels) in enumerate(_clips(B, 3)):
        del rec[:]
        losses = tr.train_step(clips, labels)
        torch.cuda.synchronize()
        assert (tr._aux is not None) == early
        assert len(losses) == 6 and [s for s, _, _ in rec] == ([0, 2, 1, 3, 4, 5] if early else [0, 1, 2, 3, 4, 5])
        assert tr._lecam_it == step + 1
        rec.sort(key=lambda r: r[0])
        got = tr._anchors[step & 1].cpu().numpy().astype(np.float64)
        rep = tr.d_stats()
        assert rep["it"] == step + 1
        prev = anchors.copy()
        for site, x, dout in rec[:4]:
            net, kind = divmod(site, 2)
            x64 = x.double().cpu().numpy()
            n, group = x64.size, x64.size // B
            assert group == (K if net == 0 else T // 4)
            d = 0.0 if step == 0 else decay
            ref = R.adv_ref(x64, group, True, kind == 0, 0, lam if step >= 1 else 0.0, prev[net][1 - kind], prev[net][kind], d)
            # the anchor: the mean's rounding bound, the update's four roundings, and what the previous anchor carried
            b_mean = sum_bound(n, ref["abs_x"], n, 0)
            err[net][kind] = d * err[net][kind] + (1 - d) * b_mean + 4 * E32 * (abs(d * prev[net][kind]) + abs((1 - d) * ref["stats"][R.STAT_MEAN]))
            anchors[net][kind] = ref["anchor_next"]
            assert abs(got[net][kind] - anchors[net][kind]) <= err[net][kind], (step, site)
            tag = ("Ds", "Dt")[net]
            assert rep[tag]["anchor_" + ("real", "fake")[kind]] == float(np.float32(got[net][kind]))
            plain = R.adv_ref(x64, group, True, kind == 0)
            dout = dout.cpu().numpy()
            if step == 0:
                # no penalty gradient before lecam_start: the plain hinge gradient, bit for bit, and a penalty of 0
                assert np.array_equal(dout, plain["dout"].astype(np.float32)) and rep[tag]["lecam_" + ("real", "fake")[kind]] == 0.0
            else:
                # the reference measured the penalty against ITS anchor: allow for the fp32 anchor's distance from it
                # (|d dout / d a| = 2 lam / n per element)
                part = np.abs(plain["dout"]) + np.abs(ref["dout"] - plain["dout"])
                slack = 2 * lam / n * np.abs(err).max()
                assert np.all(np.abs(dout - ref["dout"]) <= 6 * E32 * part + slack), (step, site)
                pen = rep[tag]["lecam_" + ("real", "fake")[kind]]
                r = np.sqrt(ref["penalty"])                       # d P / d a is at most 2 sqrt(P) (Cauchy-Schwarz)
                assert abs(pen - ref["penalty"]) <= sum_bound(n, ref["abs_pen"], n, 3) + 2 * r * np.abs(err).max() + np.abs(err).max() ** 2
            if kind == 0:
                assert abs(rep[tag]["r_t"] - ref["stats"][R.STAT_SIGN]) <= E32 * abs(ref["stats"][R.STAT_SIGN])
    # the penalty did something: with the anchors at their values the LeCam gradient of the last step was not zero everywhere
    assert rep["Ds"]["lecam_real"] + rep["Ds"]["lecam_fake"] + rep["Dt"]["lecam_real"] + rep["Dt"]["lecam_fake"] > 0


def test_topk_drops_the_sample_the_reference_drops():
    """wgan-gp form: its gradient is never 0 on a kept logit (the hinge's is on its dead side), so "zero" means "dropped"."""
    B = 2
    _seed(7)
    tr = _trainer(B, adv_loss="wgan-gp", g_topk=0.5, g_topk_decay=0.4)
    tr._epoch = 2                                   # train() counts the epochs it has started: the second one, floor(2 * 0.4) < ceil(0.5 * 2) = 1 = keep
    assert tr._anchors is None and tr._adv_stats is not None
    rec = _record(tr)
    fakes = []

    def keep_grad(module, args, out):               # (returns None: the output stays the generator's)
        out.retain_grad()
        fakes.append(out)
    tr.G.register_forward_hook(keep_grad)
    clips, labels = _clips(B, 1)[0]
    g = torch.Generator().manual_seed(3)
    draws = {"perm_real": torch.randperm(T, generator=g), "z": torch.randn(B, ZD, generator=g),
             "z_class": torch.randint(0, NCLS, (B,), generator=g), "perm_fake": torch.randperm(T, generator=g)}
    tr.train_step(clips, labels, draws)
    torch.cuda.synchronize()
    kept = {}
    for site, x, dout in rec:
        x64, dout = x.double().cpu().numpy(), dout.cpu().numpy()
        group = x64.size // B
        if site < 4:                                # the discriminator steps select nothing
            assert np.all(dout != 0)
            continue
        ref = R.adv_ref(x64, group, False, True, 1)
        s = R.scores(x64, group)
        assert abs(s[0] - s[1]) > 2 * (group + 1) * E32 * np.abs(x64).reshape(B, group).sum(axis=1).max() / group     # no near-tie
        assert np.array_equal(dout != 0, np.repeat(ref["kept"], group)) and ref["kept"].sum() == 1
        assert np.array_equal(dout, ref["dout"].astype(np.float32))        # -1 / (keep * group) or 0
        kept[site] = ref["kept"]
    rep = tr.d_stats()
    assert rep["Ds"]["g_kept"] == 1 and rep["Dt"]["g_kept"] == 1
    # through the gradient of the fake clip [B, T, 3, H, W]: the frames D_s did not sample hear from D_t alone
    assert len(fakes) == 1
    grad = fakes[0].grad
    unsampled = sorted(set(range(T)) - set(draws["perm_fake"][:K].tolist()))
    for b in range(B):
        quiet = bool((grad[b, unsampled] == 0).all())
        assert quiet == (not kept[5][b]), (b, kept)
        if not kept[4][b] and not kept[5][b]:
            assert bool((grad[b] == 0).all())


def test_everything_off_takes_the_old_launch(monkeypatch):
    from dvd_gan_amd import functional as Fn

    def refuse(*a, **kw):
        raise AssertionError("Fn.AdvLossEx entered with every setting off")
    monkeypatch.setattr(Fn.AdvLossEx, "apply", refuse)
    _seed(9)
    tr = _trainer(2)
    assert tr._anchors is None and tr._adv_stats is None and tr.d_stats() is None
    calls = []
    orig = tr.calc_loss
    tr.calc_loss = lambda x, real_flag, **kw: (calls.append(kw), orig(x, real_flag, **kw))[1]
    losses = tr.train_step(*_clips(2, 1)[0])
    assert len(losses) == 6 and all(torch.isfinite(v) for v in losses)
    assert calls == [{}] * 6                                  # calc_loss(x, real_flag), as ever
    assert tr._anchors is None and tr._adv_stats is None and tr._lecam_it == 0


def _bits(t):
    return t.detach().cpu().reshape(-1).view(torch.uint8).clone()


def test_resume_continues_the_anchors_bitwise(tmp_path):
    """Two steps, save_state(wait=True), a fresh Trainer + load_state, one more step: losses, anchors and the iteration count are
    those of the run that was not stopped.  A state written without the anchors loads with a warning and fresh anchors."""
    from dvd_gan_amd import checkpoint as C
    B = 2
    over = dict(lecam=0.5, lecam_decay=0.9, lecam_start=1, g_topk=0.5, g_topk_decay=0.4, d_stats=True)
    clips = _clips(B, 3)
    _seed(3)
    a = _trainer(B, tmp_path / "a", **over)
    a._epoch = 2
    for c in clips[:2]:
        a.train_step(*c)
    want = a.train_step(*clips[2])
    torch.cuda.synchronize()

    _seed(3)
    b = _trainer(B, tmp_path / "b", **over)
    b._epoch = 2
    for c in clips[:2]:
        b.train_step(*c)
    b.save_state(2, wait=True)
    b.close_state()
    path = os.path.join(str(tmp_path / "b"), "2_state.pt")
    sd = C.load_file(path)
    assert tuple(sd["tensors"]["lecam.Ds"].shape) == (2, 2) and tuple(sd["tensors"]["lecam.Dt"].shape) == (2, 2)
    assert sd["host"]["lecam_it"] == 2
    del b
    _seed(1234); torch.rand(7); random.random(); np.random.rand()
    fresh = _trainer(B, tmp_path / "b", **over)
    assert fresh.load_state(path) == [] and fresh._lecam_it == 2 and fresh._epoch == 2
    got = fresh.train_step(*clips[2])
    torch.cuda.synchronize()
    for name, w, g in zip(("ds_real", "ds_fake", "dt_real", "dt_fake", "g_s", "g_t"), want, got):
        assert torch.equal(_bits(w), _bits(g)), name
    assert torch.equal(_bits(a._anchors), _bits(fresh._anchors)) and a._lecam_it == fresh._lecam_it == 3
    assert torch.equal(_bits(a._adv_stats), _bits(fresh._adv_stats))

    # an old-style file: the same state without the anchors
    for k in ("lecam.Ds", "lecam.Dt"):
        del sd["tensors"][k]
    del sd["host"]["lecam_it"]
    old = os.path.join(str(tmp_path), "old_state.pt")
    torch.save(sd, old)
    again = _trainer(B, tmp_path / "b", **over)
    again._lecam_it = 5
    again._anchors.fill_(3.0)
    notes = again.load_state(old)
    assert len(notes) == 1 and "lecam" in notes[0] and "afresh" in notes[0]
    assert again._lecam_it == 0 and float(again._anchors.abs().max()) == 0.0
    # ... and a state with anchors loads into a Trainer that has the feature off as any state does
    off = _trainer(B, tmp_path / "b")
    assert off.load_state(path) == [] and off._anchors is None

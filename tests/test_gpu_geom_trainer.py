"""The Trainer's use of the clip warp (config.d_aug_geom): p = 0 and the unset setting are the step as it was, the tables are
geom_augment.draw_geom's from the seeded private generator in the documented order, the generator's gradient passes through
dvd_geom_clip_backward, exact resume, the context frames of a frame-conditional run, the early real pass.  The smallest widths
and the batch of tests/test_gpu_aug.py."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

import geom_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, T, K, NCLS, ZD = 2, 8, 4, 3, 16
S = 64
GEOM = "xflip,rot90,scale,rotate,aniso"
AUG = "color,translation,cutout"


def _seed(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


def _trainer(B=2, folder=None, **over):
    from dvd_gan_amd.train_step import Trainer
    cfg = dict(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T, lr_schr="const", total_epoch=1, d_iters=1,
               batch_size=B, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=NCLS, k_sample=K, log_epoch=0)
    if folder is not None:
        cfg.update(model_save_path=str(folder), version="")
    cfg.update(over)
    return Trainer([], argparse.Namespace(**cfg), device=DEV, compute_dtype=torch.float32)


def _clips(B, steps, seed=11, frames=T):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, frames, S, S, generator=g) * 2 - 1, torch.randint(0, NCLS, (B,), generator=g)) for _ in range(steps)]


def _flats(tr):
    return [_bits(opt.flat) for _, opt in tr._optimizers()]


def _draws(B, seed=3, **tables):
    g = torch.Generator().manual_seed(seed)
    d = {"perm_real": torch.randperm(T, generator=g), "z": torch.randn(B, ZD, generator=g),
         "z_class": torch.randint(0, NCLS, (B,), generator=g), "perm_fake": torch.randperm(T, generator=g)}
    d.update(tables)
    return d


def _watch(tr):
    """Record what the two discriminators are given, what the generator returns and the tables the step asks for, in order."""
    seen = {"Ds": [], "Dt": [], "G": [], "tables": []}
    for tag, net in (("Ds", tr.D_s), ("Dt", tr.D_t)):
        def forward(*a, _orig=net.forward, _tag=tag, **kw):
            seen[_tag].append(a[0].detach().clone())
            return _orig(*a, **kw)
        net.forward = forward
    tr.G.register_forward_hook(lambda m, a, out: seen["G"].append(out.detach().clone()))
    def tables(*a, _orig=tr._d_tables):                      # the four tables of a D iteration, None for a stage that is off
        out = _orig(*a)
        seen["tables"] += [(key, tab.detach().cpu().clone())
                           for key, tab in zip(("aug_real", "aug_fake", "geom_real", "geom_fake"), out) if tab is not None]
        return out
    tr._d_tables = tables
    return seen


def _downsample(y):
    """[B, T, 3, H, W] fp64 -> the 2 x 2 average as [B, 3, T, H / 2, W / 2]."""
    B, Tn, C, H, W = y.shape
    return y.view(B, Tn, C, H // 2, 2, W // 2, 2).mean((4, 6)).permute(0, 2, 1, 3, 4)


def _warped(clip5, table):
    """-> (reference, bound) of the warp of clips [B, T, 3, S, S] by their table, in the clips' shape."""
    y, mag, slack = R.clip(clip5.reshape(-1, 3, S, S), table, clip5.shape[1])
    return y.view(clip5.shape), R.forward_bound(mag, slack).view(clip5.shape), mag.view(clip5.shape)


def _within(got, want, bound, what):
    err = (got.detach().double().cpu() - want).abs()
    print(f"[geom] {what}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), what


def _within_dt(got, want5, bound5, mag5, what):
    """D_t's input is the 2 x 2 average of the warped clip: the average of the bounds, plus four fp32 roundings of the average
    itself (three additions and the factor) on the averaged magnitude."""
    _within(got, _downsample(want5), _downsample(bound5) + 4 * R.E32 * _downsample(mag5), what)


# ------------------------------------------------------------------ (a) p = 0 and the unset setting
def test_p_zero_and_the_empty_setting_are_the_step_without_it():
    B, runs = 2, []
    for over in ({}, dict(d_aug_geom=GEOM, d_aug_p=0.0), dict(d_aug_geom="")):
        _seed(5)
        tr = _trainer(B, **over)
        losses = [[_bits(v) for v in tr.train_step(*c)] for c in _clips(B, 2)]
        torch.cuda.synchronize()
        runs.append((losses, _flats(tr), torch.get_rng_state()))
        assert (tr._aug_gen is not None) == bool(over.get("d_aug_geom")) and tr._adv_stats is None
    for lb, fb, rb in runs[1:]:
        for step in range(2):
            for a, b in zip(runs[0][0][step], lb[step]):
                assert torch.equal(a, b), step
        for a, b in zip(runs[0][1], fb):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][2], rb)


# ------------------------------------------------------------------ (b) the tables
@pytest.mark.parametrize("d_aug", ["", AUG], ids=["d_aug off", "d_aug on"])
def test_the_trainer_draws_its_tables_in_the_documented_order(d_aug):
    """No table supplied: per D iteration the step draws d_aug's two tables (when d_aug is set), then the warps of the real clips,
    then those of the fake clips, from one generator seeded with d_aug_seed -- and with d_aug off the discriminators are given the
    reference's warp by exactly those tables."""
    from dvd_gan_amd.augment import draw_params
    from dvd_gan_amd.geom_augment import draw_geom
    B, seed, p = 2, 6, 0.8
    _seed(31)
    tr = _trainer(B, d_aug=d_aug, d_aug_geom="xflip,scale,rotate", d_aug_p=p, d_aug_seed=seed)
    seen = _watch(tr)
    (clips, labels), draws = _clips(B, 1)[0], _draws(B)
    tr.train_step(clips, labels, draws)
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(seed)
    want = []
    if d_aug:
        want += [("aug_real", draw_params(B, S, S, d_aug, p, gen)), ("aug_fake", draw_params(B, S, S, d_aug, p, gen))]
    want += [("geom_real", draw_geom(B, S, S, "xflip,scale,rotate", p, gen)), ("geom_fake", draw_geom(B, S, S, "xflip,scale,rotate", p, gen))]
    assert [k for k, _ in seen["tables"]] == [k for k, _ in want]
    for (key, got), (_, tab) in zip(seen["tables"], want):
        assert torch.equal(got, tab), key
    assert torch.equal(gen.get_state(), tr._aug_gen.get_state())
    assert not torch.equal(want[-1][1], want[-2][1]) and not torch.equal(want[-1][1], torch.tensor(R.IDENTITY).repeat(B, 1))
    if d_aug:
        return
    ids_real, ids_fake = draws["perm_real"][:K].sort()[0], draws["perm_fake"][:K].sort()[0]
    for clip5, table, ids, i, what in ((clips.permute(0, 2, 1, 3, 4).contiguous(), want[0][1], ids_real, 0, "real"),
                                       (seen["G"][0].cpu(), want[1][1], ids_fake, 1, "fake")):
        y, bound, mag = _warped(clip5, table)
        _within(seen["Ds"][i], y[:, ids], bound[:, ids], f"D_s {what}, drawn table")
        _within_dt(seen["Dt"][i], y, bound, mag, f"D_t {what}, drawn table")


# ------------------------------------------------------------------ (c) the generator's gradient
class _RefWarp(torch.autograd.Function):
    """ClipWarp's stand-in: the fp64 restatement and its autograd transpose, rounded to fp32 where the launches' results are."""

    @staticmethod
    def forward(ctx, frames, mats):
        ctx.save_for_backward(mats)
        B, Tn = frames.shape[:2]
        y, _, _ = R.clip(frames.detach().reshape(B * Tn, 3, S, S), mats.cpu(), Tn)
        return y.view(frames.shape).float().to(frames.device)

    @staticmethod
    def backward(ctx, g):
        (mats,) = ctx.saved_tensors
        B, Tn = g.shape[:2]
        flat = g.reshape(B * Tn, 3, S, S)
        dx, *_ = R.clip_grad(flat, flat, mats.cpu(), Tn)
        return dx.view(g.shape).float().to(g.device), None


def test_generator_gradient_passes_through_the_transpose(monkeypatch):
    """Fixed draws, one step: the generator's weight gradient with the two launches against the one with the fp64 restatement in
    their place (warp and transpose), and against the one with identity rows.
    Tolerance: the two runs hand the discriminators inputs that differ by the kernels' bound (about 1e-6 of the values) and get
    gradients back that differ by as little; everything else is the same fp32 code on both sides, which answers a perturbation of
    that size as it answers its own roundings.  The package's yardstick for fp32 against a reference computation is 2e-3 relative
    (the smoke run); here: 1e-3 of the gradient's largest element, per element.  The warp itself moves the gradient by far more."""
    from dvd_gan_amd import train_step as TS
    from dvd_gan_amd.geom_augment import draw_geom
    B = 2
    gen = torch.Generator().manual_seed(41)
    tabs = {"geom_real": draw_geom(B, S, S, GEOM, 1.0, gen), "geom_fake": draw_geom(B, S, S, GEOM, 1.0, gen)}
    ident = {k: torch.tensor(R.IDENTITY).repeat(B, 1) for k in tabs}
    grads = []
    for tables, ref in ((tabs, False), (tabs, True), (ident, False)):
        if ref:
            monkeypatch.setattr(TS, "ClipWarp", _RefWarp)
        else:
            monkeypatch.undo()
        _seed(7)
        tr = _trainer(B, d_aug_geom=GEOM, d_aug_p=1.0)
        tr.train_step(*_clips(B, 1)[0], _draws(B, **tables))
        torch.cuda.synchronize()
        grads.append(tr.g_optimizer.grad.detach().double().cpu().clone())
    monkeypatch.undo()
    dev, ref, plain = grads
    scale = float(ref.abs().max())
    err, moved = float((dev - ref).abs().max()), float((plain - ref).abs().max())
    print(f"[geom] G gradient: |launches - restatement| {err:.3e}, |identity rows - restatement| {moved:.3e}, largest element {scale:.3e}")
    assert scale > 0 and err <= 1e-3 * scale
    assert moved > 20e-3 * scale


def test_rows_that_put_the_fake_clips_outside_leave_the_generator_alone():
    """The discriminators see zeros for the fake clips and the generator's gradient is the transpose applied to whatever they
    return: zero.  Adam on a zero gradient moves nothing (beta1 = 0)."""
    B = 2
    _seed(7)
    tr = _trainer(B, d_aug_geom=GEOM, d_aug_p=1.0)
    outside = torch.tensor([R.hand_rows(S, S)["outside"]] * B, dtype=torch.float32)
    before = _flats(tr)
    tr.train_step(*_clips(B, 1)[0], _draws(B, geom_fake=outside))
    torch.cuda.synchronize()
    after = _flats(tr)
    assert torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
    assert float(tr.g_optimizer.grad.abs().max()) == 0.0


# ------------------------------------------------------------------ (d) exact resume with an adaptive p
ADAPTIVE = dict(d_aug_geom=GEOM, d_aug_p=0.5, d_aug_target=0.6, d_aug_interval=1, d_aug_kimg=0.008)       # B = 2: one adjustment is 0.25


def test_resume_continues_p_and_the_tables_bitwise(tmp_path):
    from dvd_gan_amd.geom_augment import draw_geom
    B = 2
    clips = _clips(B, 4)
    _seed(3)
    a = _trainer(B, tmp_path / "a", **ADAPTIVE)
    assert a._adv_stats is not None and a.d_aug == ()                 # the statistics' launch is on without d_aug
    ps = []
    for c in clips:
        a.train_step(*c)
        ps.append(a.d_aug_p)
    torch.cuda.synchronize()
    assert a._aug_adjustments == 4 and any(p != 0.5 for p in ps)

    _seed(3)
    b = _trainer(B, tmp_path / "b", **ADAPTIVE)
    for c in clips[:2]:
        b.train_step(*c)
    b.save_state(2, wait=True)
    b.close_state()
    p_saved = b.d_aug_p
    del b
    path = os.path.join(str(tmp_path / "b"), "2_state.pt")
    _seed(1234); torch.rand(7); random.random(); np.random.rand()
    fresh = _trainer(B, tmp_path / "b", **dict(ADAPTIVE, d_aug_seed=99))       # another seed: the state's generator holds
    assert fresh.load_state(path) == [] and fresh.d_aug_p == p_saved == ps[1] and fresh._aug_steps == 2
    for c in clips[2:]:
        fresh.train_step(*c)
    torch.cuda.synchronize()
    for (tag, _), wa, wf in zip(a._optimizers(), _flats(a), _flats(fresh)):
        assert torch.equal(wa, wf), tag
    assert a.d_aug_p == fresh.d_aug_p and a._aug_adjustments == fresh._aug_adjustments == 4
    assert torch.equal(draw_geom(B, S, S, GEOM, 1.0, a._aug_gen), draw_geom(B, S, S, GEOM, 1.0, fresh._aug_gen))
    from dvd_gan_amd import checkpoint as C
    assert sorted(C.load_file(path)["host"]["aug"]) == ["adjustments", "generator", "p", "steps"]       # no new key


# ------------------------------------------------------------------ (e) context frames
def test_context_frames_take_the_fake_clips_rows():
    from dvd_gan_amd.geom_augment import draw_geom
    B, n_cond = 3, 4
    F = T + n_cond
    _seed(13)
    tr = _trainer(B, d_aug_geom=GEOM, d_aug_p=1.0, n_cond=n_cond)
    seen = _watch(tr)
    gen = torch.Generator().manual_seed(23)
    tabs = {"geom_real": draw_geom(B, S, S, GEOM, 1.0, gen), "geom_fake": draw_geom(B, S, S, GEOM, 1.0, gen)}
    (clips, labels), draws = _clips(B, 1, frames=F)[0], _draws(B, **tabs)
    tr.train_step(clips, labels, draws)
    torch.cuda.synchronize()
    assert [len(seen[k]) for k in ("Ds", "Dt", "G")] == [3, 3, 1]
    real = clips.permute(0, 2, 1, 3, 4).contiguous()                      # [B, F, 3, H, W]
    fake = seen["G"][0].cpu()
    ids_real = draws["perm_real"][:K].sort()[0] + n_cond
    ids_fake = draws["perm_fake"][:K].sort()[0]
    ry, rb, rm = _warped(real, tabs["geom_real"])
    fy, fb, fm = _warped(fake, tabs["geom_fake"])
    _within(seen["Ds"][0], ry[:, ids_real], rb[:, ids_real], "D_s real")
    for i in (1, 2):                                                      # the D step's detached copy, the G step's
        _within(seen["Ds"][i], fy[:, ids_fake], fb[:, ids_fake], "D_s fake")
    cy, cb, cm = _warped(real[:, :n_cond].contiguous(), tabs["geom_fake"])        # the context under the FAKE clips' rows
    fy, fb, fm = torch.cat([cy, fy], 1), torch.cat([cb, fb], 1), torch.cat([cm, fm], 1)
    _within_dt(seen["Dt"][0], ry, rb, rm, "D_t real")
    for i in (1, 2):
        _within_dt(seen["Dt"][i], fy, fb, fm, "D_t [context | fake]")
    assert tuple(seen["Dt"][0].shape) == (B, 3, F, S // 2, S // 2)
    # ... and not under the real clips' rows: that reading of the context misses the bound by far
    wy, _, _ = _warped(real[:, :n_cond].contiguous(), tabs["geom_real"])
    got = seen["Dt"][1].double().cpu()[:, :, :n_cond]
    assert float((got - _downsample(wy)).abs().max()) > 0.05


# ------------------------------------------------------------------ the early real pass
def test_real_clips_early_gives_the_same_losses(monkeypatch):
    B, runs = 2, []
    for early in ("0", "1"):
        monkeypatch.setenv("DVD_D_REAL_EARLY", early)
        _seed(19)
        tr = _trainer(B, d_aug_geom=GEOM, d_aug="color", d_aug_p=1.0, d_aug_seed=4)
        assert (tr._aux is not None) == (early == "1") and tr.d_aug_geom == ("xflip", "rot90", "scale", "rotate", "aniso")
        runs.append([[_bits(v) for v in tr.train_step(*c)] for c in _clips(B, 2)])
        torch.cuda.synchronize()
    for step in range(2):
        for a, b in zip(runs[0][step], runs[1][step]):
            assert torch.equal(a, b), step

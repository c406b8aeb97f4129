"""Clip-consistent augmentation of the discriminators' inputs on the GPU: dvd_aug_clip_forward / dvd_aug_clip_backward against
the fp64 restatement of tests/aug_ref.py, their determinism and frame independence, their refusals, and the Trainer's use of them
(config.d_aug ...: what the discriminators see, where the generator's gradient goes, adaptive p, exact resume), at the small
widths of tests/test_gpu_advloss_trainer.py.

The bound.  The documented order has at most 11 fp32 roundings on the way to an output element (1 brightness, 3 for m1, 3 for the
saturation, 1 for m2, 3 for the contrast), each on a quantity bounded by `mag`, the same expression on absolute values; the bound
is 12 * 2^-24 * mag, and where the reference is exactly 0 (outside the shifted frame, inside the cutout) so is the device."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

import aug_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BOUND = R.ROUNDINGS * R.E32
CH, T, K, NCLS, ZD = 2, 8, 4, 3, 16
ALL = "color,translation,cutout"


def _seed(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


def _within(got, want, mag, what, bound=BOUND):
    got = got.detach().double().cpu()
    zero = want == 0
    assert bool((got[zero] == 0).all()), f"{what}: the device is not 0 where the reference is"
    err = (got - want).abs()
    worst = float((err / mag.clamp_min(1e-300)).max())
    print(f"[aug] {what}: worst error {worst / R.E32:.3f} * 2^-24 * mag")
    assert bool((err <= bound * mag).all()), (what, worst / R.E32)


# ------------------------------------------------------------------ 1. forward and backward against the reference
@pytest.mark.parametrize("shape", [(3, 3, 12, 20), (2, 2, 64, 64), (1, 1, 2, 18)], ids=["3x3x12x20", "2x2x64x64", "1x1x2x18"])
def test_forward_and_backward_against_the_reference(shape):
    from dvd_gan_amd.augment import ClipAugment
    B, Tc, H, W = shape
    rows = R.hand_rows(H, W)
    names = sorted(rows)
    gen = torch.Generator().manual_seed(H * 131 + W)
    for first in range(0, len(names), B):
        chunk = [names[(first + i) % len(names)] for i in range(B)]
        params = torch.tensor([rows[n] for n in chunk], dtype=torch.float32)
        x = torch.rand(B, Tc, 3, H, W, generator=gen) * 2 - 1
        g = torch.randn(B, Tc, 3, H, W, generator=gen)
        xd = x.to(DEV).requires_grad_(True)
        y = ClipAugment.apply(xd, params.to(DEV))
        y.backward(g.to(DEV))
        torch.cuda.synchronize()
        want, mag = R.clip(x.view(-1, 3, H, W), params, Tc)
        dwant, dmag = R.clip_grad(x.view(-1, 3, H, W), g.view(-1, 3, H, W), params, Tc)
        _within(y.view(-1, 3, H, W), want, mag, f"forward {shape} {chunk}")
        _within(xd.grad.view(-1, 3, H, W), dwant, dmag, f"backward {shape} {chunk}")
        for b, name in enumerate(chunk):
            if name == "identity":              # skipped stages, not computed ones: the bits of the input
                assert torch.equal(_bits(y[b]), _bits(x[b])) and torch.equal(_bits(xd.grad[b]), _bits(g[b]))
            if name in ("dx = -W", "cutout covers the frame"):
                assert float(y[b].detach().abs().max()) == 0.0 and float(xd.grad[b].abs().max()) == 0.0


# ------------------------------------------------------------------ 2. determinism and independence
@pytest.mark.parametrize("shape", [(3, 5, 12, 20), (2, 5, 5, 18), (2, 6, 64, 64)], ids=["3x5x12x20", "2x5x5x18", "2x6x64x64"])
def test_determinism_and_frame_independence(shape):
    from dvd_gan_amd.augment import clip_backward, clip_forward
    B, Tc, H, W = shape
    Kc = 2
    rows = R.hand_rows(H, W)
    params = torch.tensor([rows[n] for n in ("everything", "everything, aligned shift", "colour")[:B]], dtype=torch.float32).to(DEV)
    gen = torch.Generator().manual_seed(17)
    x = (torch.rand(B, Tc, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    for fn in (clip_forward, clip_backward):
        flat = x.view(B * Tc, 3, H, W)
        a, b = fn(flat, params, Tc), fn(flat, params, Tc)
        torch.cuda.synchronize()
        assert torch.equal(_bits(a), _bits(b)), fn.__name__                        # two launches
        for n in (0, Tc - 1, B * Tc - 1):                                          # a frame alone
            alone = fn(flat[n:n + 1].clone(), params[n // Tc:n // Tc + 1].clone(), 1)
            assert torch.equal(_bits(alone[0]), _bits(a[n])), (fn.__name__, n)
        ctx = fn(x[:, :Kc].contiguous().view(B * Kc, 3, H, W), params, Kc)         # the context frames with their own clip length
        assert torch.equal(_bits(ctx.view(B, Kc, 3, H, W)), _bits(a.view(B, Tc, 3, H, W)[:, :Kc])), fn.__name__


# ------------------------------------------------------------------ 3. error codes
def test_refusals_leave_the_output_untouched():
    from dvd_gan_amd import lib as L
    au = L.aug_lib()
    x = torch.rand(4, 3, 8, 8, device=DEV)
    y = torch.full_like(x, 7.0)
    params = torch.tensor([R.hand_rows(8, 8)["everything"]] * 2, dtype=torch.float32, device=DEV)
    for fn in (au.dvd_aug_clip_forward, au.dvd_aug_clip_backward):
        assert fn(L.ptr(y), L.ptr(y), L.ptr(params), 4, 2, 8, 8, L.stream()) == -1          # in place
        assert fn(None, L.ptr(y), L.ptr(params), 4, 2, 8, 8, L.stream()) == -1
        assert fn(L.ptr(x), None, L.ptr(params), 4, 2, 8, 8, L.stream()) == -1
        assert fn(L.ptr(x), L.ptr(y), None, 4, 2, 8, 8, L.stream()) == -1
        assert fn(L.ptr(x), L.ptr(y), L.ptr(params), 4, 0, 8, 8, L.stream()) == -1           # frames_per_clip = 0
        assert fn(L.ptr(x), L.ptr(y), L.ptr(params), 4, 2, 8, 4097, L.stream()) == -2
        assert fn(L.ptr(x), L.ptr(y), L.ptr(params), 0, 2, 8, 8, L.stream()) == 0            # no frames: succeeds, launches nothing
        torch.cuda.synchronize()
        assert float(y.min()) == 7.0 and float(y.max()) == 7.0
    with pytest.raises(ValueError, match="parameter table"):
        from dvd_gan_amd.augment import clip_forward
        clip_forward(x, params[:1], 2)


# ------------------------------------------------------------------ 4. the Trainer
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
    return [(torch.rand(B, 3, frames, 64, 64, generator=g) * 2 - 1, torch.randint(0, NCLS, (B,), generator=g)) for _ in range(steps)]


def _flats(tr):
    return [_bits(opt.flat) for _, opt in tr._optimizers()]


def _draws(B, seed=3, **tables):
    g = torch.Generator().manual_seed(seed)
    d = {"perm_real": torch.randperm(T, generator=g), "z": torch.randn(B, ZD, generator=g),
         "z_class": torch.randint(0, NCLS, (B,), generator=g), "perm_fake": torch.randperm(T, generator=g)}
    d.update(tables)
    return d


def test_p_zero_is_the_step_without_augmentation():
    B, runs = 2, []
    for over in ({}, dict(d_aug=ALL, d_aug_p=0.0)):
        _seed(5)
        tr = _trainer(B, **over)
        losses = [[_bits(v) for v in tr.train_step(*c)] for c in _clips(B, 2)]
        torch.cuda.synchronize()
        runs.append((losses, _flats(tr), torch.get_rng_state(), None if tr.noise_gen is None else tr.noise_gen.get_state()))
        assert (tr._aug_gen is not None) == bool(over) and tr._adv_stats is None
    (la, fa, ra, na), (lb, fb, rb, nb) = runs
    for step in range(2):
        for a, b in zip(la[step], lb[step]):
            assert torch.equal(a, b), step
    for a, b in zip(fa, fb):
        assert torch.equal(a, b)
    assert torch.equal(ra, rb) and (na is None) == (nb is None) and (na is None or torch.equal(na, nb))


def test_generator_gradient_passes_through_the_transform():
    """A cutout that covers every frame of every fake clip: the discriminators see zeros for the fake clips and the generator's
    gradient is the transpose applied to whatever they return: zero.  Adam on a zero gradient moves nothing (beta1 = 0)."""
    B = 2
    _seed(7)
    tr = _trainer(B, d_aug=ALL, d_aug_p=1.0)
    cover = torch.tensor([R.hand_rows(64, 64)["cutout covers the frame"]] * B, dtype=torch.float32)
    before = _flats(tr)
    tr.train_step(*_clips(B, 1)[0], _draws(B, aug_fake=cover))
    torch.cuda.synchronize()
    after = _flats(tr)
    assert torch.equal(before[0], after[0])                       # G
    assert not torch.equal(before[1], after[1])                   # D_s (its real clips were augmented by a drawn table)
    assert float(tr.g_optimizer.grad.abs().max()) == 0.0


def _watch(tr):
    """Record what the two discriminators are given and what the generator returns."""
    seen = {"Ds": [], "Dt": [], "G": []}
    for tag, net in (("Ds", tr.D_s), ("Dt", tr.D_t)):
        def forward(*a, _orig=net.forward, _tag=tag, **kw):
            seen[_tag].append(a[0].detach().clone())
            return _orig(*a, **kw)
        net.forward = forward
    tr.G.register_forward_hook(lambda m, a, out: seen["G"].append(out.detach().clone()))
    return seen


def _downsample(y):
    """[B, T, 3, H, W] fp64 -> the 2 x 2 average as [B, 3, T, H / 2, W / 2]."""
    B, Tn, C, H, W = y.shape
    return y.view(B, Tn, C, H // 2, 2, W // 2, 2).mean((4, 6)).permute(0, 2, 1, 3, 4)


@pytest.mark.parametrize("n_cond", [0, 4])
def test_the_discriminators_see_the_transformed_clips(n_cond):
    """D_s is given k frames of the augmented clip (a gather), D_t its 2 x 2 average: both within the kernel's bound,
    12 * 2^-24 * mag, with mag gathered / averaged like the values."""
    from dvd_gan_amd.augment import draw_params
    B, F = 3, T + n_cond
    _seed(13)
    tr = _trainer(B, d_aug=ALL, d_aug_p=1.0, n_cond=n_cond)
    seen = _watch(tr)
    gen = torch.Generator().manual_seed(23)
    tabs = {"aug_real": draw_params(B, 64, 64, ALL, 1.0, gen), "aug_fake": draw_params(B, 64, 64, ALL, 1.0, gen)}
    assert not torch.equal(tabs["aug_real"], tabs["aug_fake"])
    (clips, labels), draws = _clips(B, 1, frames=F)[0], _draws(B, **tabs)
    tr.train_step(clips, labels, draws)
    torch.cuda.synchronize()
    assert [len(seen[k]) for k in ("Ds", "Dt", "G")] == [3, 3, 1]
    real = clips.permute(0, 2, 1, 3, 4).contiguous()                      # [B, F, 3, H, W]
    fake = seen["G"][0].cpu()
    ids_real = draws["perm_real"][:K].sort()[0] + n_cond
    ids_fake = draws["perm_fake"][:K].sort()[0]

    def transformed(clip5, table):
        y, mag = R.clip(clip5.reshape(-1, 3, 64, 64), table, clip5.shape[1])
        return y.view(clip5.shape), mag.view(clip5.shape)
    ry, rm = transformed(real, tabs["aug_real"])
    fy, fm = transformed(fake, tabs["aug_fake"])
    _within(seen["Ds"][0], ry[:, ids_real], rm[:, ids_real], "D_s real")
    for i in (1, 2):                                                      # the D step's detached copy, the G step's
        _within(seen["Ds"][i], fy[:, ids_fake], fm[:, ids_fake], "D_s fake")
    if n_cond:
        cy, cm = transformed(real[:, :n_cond], tabs["aug_fake"])         # the context frames take the fake clips' rows
        fy, fm = torch.cat([cy, fy], 1), torch.cat([cm, fm], 1)
    _within(seen["Dt"][0], _downsample(ry), _downsample(rm), "D_t real")
    for i in (1, 2):
        _within(seen["Dt"][i], _downsample(fy), _downsample(fm), "D_t fake")
    assert tuple(seen["Dt"][0].shape) == (B, 3, F, 32, 32)


def test_the_trainer_draws_its_tables_from_the_seeded_private_generator():
    """No table supplied: what the discriminators are given is the reference's transform by the tables
    draw_params(B, H, W, policy, p) yields from a generator seeded with d_aug_seed, the real clips' first, the fake clips' second."""
    from dvd_gan_amd.augment import draw_params
    B, seed = 2, 6
    _seed(31)
    tr = _trainer(B, d_aug=ALL, d_aug_p=1.0, d_aug_seed=seed)
    seen = _watch(tr)
    (clips, labels), draws = _clips(B, 1)[0], _draws(B)
    tr.train_step(clips, labels, draws)
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(seed)
    tab_real, tab_fake = draw_params(B, 64, 64, ALL, 1.0, gen), draw_params(B, 64, 64, ALL, 1.0, gen)
    assert torch.equal(gen.get_state(), tr._aug_gen.get_state())
    ids_real, ids_fake = draws["perm_real"][:K].sort()[0], draws["perm_fake"][:K].sort()[0]
    for clip5, table, ids, ds, dt, what in ((clips.permute(0, 2, 1, 3, 4).contiguous(), tab_real, ids_real, 0, 0, "real"),
                                            (seen["G"][0].cpu(), tab_fake, ids_fake, 1, 1, "fake")):
        y, mag = R.clip(clip5.reshape(-1, 3, 64, 64), table, T)
        y, mag = y.view(clip5.shape), mag.view(clip5.shape)
        _within(seen["Ds"][ds], y[:, ids], mag[:, ids], f"D_s {what}, drawn table")
        _within(seen["Dt"][dt], _downsample(y), _downsample(mag), f"D_t {what}, drawn table")
    # ... and with p = 0.5 and one group the same call's tables: the policy and p reach draw_params
    _seed(31)
    tr = _trainer(B, d_aug="cutout", d_aug_p=0.5, d_aug_seed=seed + 1)
    seen = _watch(tr)
    tr.train_step(clips, labels, draws)
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(seed + 1)
    tab_real = draw_params(B, 64, 64, "cutout", 0.5, gen)
    y, mag = R.clip(clips.permute(0, 2, 1, 3, 4).reshape(-1, 3, 64, 64), tab_real, T)
    _within(seen["Dt"][0], _downsample(y.view(B, T, 3, 64, 64)), _downsample(mag.view(B, T, 3, 64, 64)), "D_t real, cutout at p = 0.5")


def test_real_clips_early_gives_the_same_losses(monkeypatch):
    B, runs = 2, []
    for early in ("0", "1"):
        monkeypatch.setenv("DVD_D_REAL_EARLY", early)
        _seed(19)
        tr = _trainer(B, d_aug=ALL, d_aug_p=1.0, d_aug_seed=4)
        assert (tr._aux is not None) == (early == "1") and tr.d_aug == ("color", "translation", "cutout")
        runs.append([[_bits(v) for v in tr.train_step(*c)] for c in _clips(B, 2)])
        torch.cuda.synchronize()
    for step in range(2):
        for a, b in zip(runs[0][step], runs[1][step]):
            assert torch.equal(a, b), step


# ------------------------------------------------------------------ 5. adaptive p
ADAPTIVE = dict(d_aug=ALL, d_aug_p=0.5, d_aug_target=0.6, d_aug_interval=1, d_aug_kimg=0.008)       # B = 2: one adjustment is 0.25


def test_adaptive_p_follows_r_t():
    from dvd_gan_amd.augment import ada_update
    B = 2
    _seed(29)
    tr = _trainer(B, **ADAPTIVE)
    assert tr.d_aug_p == 0.5 and tr._adv_stats is not None            # the statistics' launch is on
    p, moved = 0.5, 0
    for step, c in enumerate(_clips(B, 3)):
        tr.train_step(*c)
        rep = tr.d_stats()
        want = ada_update(p, 0.5 * (rep["Ds"]["r_t"] + rep["Dt"]["r_t"]), 0.6, B, 1, 0.008)
        assert tr.d_aug_p == want and tr._aug_adjustments == step + 1, (step, tr.d_aug_p, want, rep)
        moved += want != p
        p = want
    assert moved >= 2 and p in (0.0, 0.25, 0.5, 0.75, 1.0)
    with pytest.raises(ValueError, match="d_aug_target"):
        _trainer(B, **dict(ADAPTIVE, d_aug_target=-0.1))


# ------------------------------------------------------------------ 6. exact resume
def test_resume_continues_p_and_the_tables_bitwise(tmp_path):
    from dvd_gan_amd.augment import draw_params
    B = 2
    clips = _clips(B, 4)
    _seed(3)
    a = _trainer(B, tmp_path / "a", **ADAPTIVE)
    for c in clips:
        a.train_step(*c)
    torch.cuda.synchronize()

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
    assert fresh.load_state(path) == [] and fresh.d_aug_p == p_saved and fresh._aug_steps == 2 and fresh._aug_adjustments == 2
    for c in clips[2:]:
        fresh.train_step(*c)
    torch.cuda.synchronize()
    for (tag, _), wa, wf in zip(a._optimizers(), _flats(a), _flats(fresh)):
        assert torch.equal(wa, wf), tag
    assert a.d_aug_p == fresh.d_aug_p and a._aug_adjustments == fresh._aug_adjustments == 4
    assert torch.equal(draw_params(B, 64, 64, ALL, a.d_aug_p, a._aug_gen), draw_params(B, 64, 64, ALL, fresh.d_aug_p, fresh._aug_gen))

    # a state written without the augmentation loads with a note, the constructor's p and a fresh generator
    from dvd_gan_amd import checkpoint as C
    sd = C.load_file(path)
    assert sorted(sd["host"]["aug"]) == ["adjustments", "generator", "p", "steps"]
    del sd["host"]["aug"]
    old = os.path.join(str(tmp_path), "old_state.pt")
    torch.save(sd, old)
    again = _trainer(B, tmp_path / "b", **ADAPTIVE)
    again.d_aug_p, again._aug_steps = 0.75, 5
    again._aug_gen.manual_seed(77)
    notes = again.load_state(old)
    assert len(notes) == 1 and "d_aug" in notes[0] and "afresh" in notes[0]
    assert again.d_aug_p == 0.5 and again._aug_steps == 0
    assert torch.equal(again._aug_gen.get_state(), torch.Generator().manual_seed(0).get_state())
    # ... and a state with it loads into a Trainer that has the feature off as any state does
    off = _trainer(B, tmp_path / "b")
    assert off.load_state(path) == [] and off._aug_gen is None

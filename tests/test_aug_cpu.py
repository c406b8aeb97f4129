"""Augmentation of the discriminators' inputs without a GPU: the fp64 restatement the GPU tests compare with (tests/aug_ref.py)
is its own transpose's transpose, the parameter tables of augment.draw_params, the rule that moves p, the policy parser, the aug
library's refusals (which come back before anything touches the device) and its resource file."""
import argparse
import os
import re

import pytest
import torch

import aug_ref as R

E_ARG, E_SHAPE = -1, -2
P_, Q_ = 64, 128          # non-null placeholder pointers: the refusals come before anything is dereferenced


# ------------------------------------------------------------------ the fp64 restatement
@pytest.mark.parametrize("name", sorted(R.hand_rows(6, 10)))
def test_reference_backward_is_the_transpose_of_its_forward(name):
    """The map is affine, y = A x + y(0): <A x, g> = <x, A^T g> with A^T g from autograd, in fp64."""
    H, W = 6, 10
    row = R.hand_rows(H, W)[name]
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, H, W, dtype=torch.float64, generator=gen) * 2 - 1
    g = torch.randn(2, 3, H, W, dtype=torch.float64, generator=gen)
    params = torch.tensor([row], dtype=torch.float64)
    y, mag = R.clip(x, params, 2)
    y0, _ = R.clip(torch.zeros_like(x), params, 2)
    dx, dmag = R.clip_grad(x, g, params, 2)
    lhs, rhs = float(((y - y0) * g).sum()), float((x * dx).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((mag * g.abs()).sum() + 1.0), (lhs, rhs)
    assert bool((y.abs() <= mag * (1 + 1e-12)).all()) and bool((dx.abs() <= dmag * (1 + 1e-12) + 1e-300).all())
    if name == "identity":
        assert torch.equal(y, x) and torch.equal(dx, g)
    if name in ("dx = -W", "cutout covers the frame"):
        assert float(y.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0


def test_reference_against_a_hand_computation():
    """One 1 x 2 frame, every value a small dyadic number: b = 0.5, s = 0.5, c = 2, dx = 1.
    x = [[1, 0]], [[0, 0]], [[-1, 3]] -> y0 = x + 0.5; m1 = (0.5, 1.5); y1 = (y0 - m1) / 2 + m1 = [1, 1], [0.5, 1], [0, 2.5];
    m2 = mean(x) + b = 0.5 + 0.5 = 1; y2 = (y1 - 1) 2 + 1 = [1, 1], [0, 1], [-1, 4]; shifted right by one: [0, 1], [0, 0], [0, -1]."""
    x = torch.tensor([[[1.0, 0.0]], [[0.0, 0.0]], [[-1.0, 3.0]]], dtype=torch.float64)
    y = R.frame(x, (0.5, 0.5, 2.0, 1, 0, 0, 0, 0, 0))
    assert torch.equal(y, torch.tensor([[[0.0, 1.0]], [[0.0, 0.0]], [[0.0, -1.0]]], dtype=torch.float64))
    assert torch.equal(R.frame(x, (0.5, 0.5, 2.0, 0, 0, 0, 1, 1, 5)), torch.tensor([[[1.0, 0.0]], [[0.0, 0.0]], [[-1.0, 0.0]]], dtype=torch.float64))


# ------------------------------------------------------------------ the tables
def test_draw_params_leaves_the_stream_where_it_is_whatever_the_policy():
    from dvd_gan_amd.augment import draw_params
    states = []
    for policy, p in (("", 1.0), ("color", 0.0), ("color,translation,cutout", 1.0), ("cutout", 0.3)):
        gen = torch.Generator().manual_seed(5)
        draw_params(4, 12, 20, policy, p, gen)
        states.append(gen.get_state())
    assert all(torch.equal(states[0], s) for s in states[1:])
    gen = torch.Generator().manual_seed(5)
    torch.rand(4, 10, dtype=torch.float64, generator=gen)              # exactly this one call
    assert torch.equal(states[0], gen.get_state())
    before = torch.get_rng_state()
    draw_params(3, 8, 8, "color", 1.0, torch.Generator().manual_seed(1))
    assert torch.equal(before, torch.get_rng_state())                  # the default generator is not touched
    a = draw_params(6, 64, 64, "color,translation,cutout", 0.7, torch.Generator().manual_seed(9))
    b = draw_params(6, 64, 64, "color,translation,cutout", 0.7, torch.Generator().manual_seed(9))
    assert torch.equal(a, b) and a.dtype == torch.float32 and tuple(a.shape) == (6, R.COLS)


def test_draw_params_gates_and_identity_columns():
    from dvd_gan_amd.augment import draw_params
    ident = torch.tensor(R.IDENTITY).repeat(50, 1)
    assert torch.equal(draw_params(50, 12, 20, "color,translation,cutout", 0.0, torch.Generator().manual_seed(2)), ident)
    assert torch.equal(draw_params(50, 12, 20, "", 1.0, torch.Generator().manual_seed(2)), ident)
    groups = {"color": [0, 1, 2], "translation": [3, 4], "cutout": [5, 6, 7, 8]}
    for name, cols in groups.items():
        t = draw_params(50, 12, 20, name, 1.0, torch.Generator().manual_seed(2))
        rest = [c for c in range(R.COLS) if c not in cols]
        assert torch.equal(t[:, rest], ident[:, rest]), name
        assert not torch.equal(t[:, cols], ident[:, cols]), name
    # a gate is one comparison with p: at p = 0.5 about half of the clips take a group, and the groups' gates are independent
    t = draw_params(4000, 12, 20, "color,translation,cutout", 0.5, torch.Generator().manual_seed(4))
    on_c, on_k = t[:, 2] != 1.0, t[:, 7] != 0.0
    assert 0.45 < float(on_c.float().mean()) < 0.55 and 0.45 < float(on_k.float().mean()) < 0.55
    assert 0.2 < float((on_c & on_k).float().mean()) < 0.3


@pytest.mark.parametrize("H,W,ry,rx", [(12, 20, 2, 3), (20, 12, 3, 2), (64, 64, 8, 8), (2, 18, 0, 2), (5, 7, 1, 1)])
def test_draw_params_ranges(H, W, ry, rx):
    """DiffAugment's ranges; floor(12 / 8 + 0.5) = 2 and floor(20 / 8 + 0.5) = 3 (halves round up)."""
    from dvd_gan_amd.augment import draw_params
    t = draw_params(5000, H, W, "color,translation,cutout", 1.0, torch.Generator().manual_seed(8)).double()
    b, s, c, dx, dy, cy0, cx0, ch, cw = t.unbind(1)
    assert -0.5 <= float(b.min()) < -0.49 and 0.49 < float(b.max()) <= 0.5
    assert 0.0 <= float(s.min()) < 0.01 and 1.99 < float(s.max()) <= 2.0
    assert 0.5 <= float(c.min()) < 0.51 and 1.49 < float(c.max()) <= 1.5
    assert torch.equal(t[:, 3:], t[:, 3:].round())                                      # integers
    assert sorted(set(dx.tolist())) == list(range(-rx, rx + 1)) and sorted(set(dy.tolist())) == list(range(-ry, ry + 1))
    hh, ww = int(H / 2 + 0.5), int(W / 2 + 0.5)
    assert set(ch.tolist()) == {hh} and set(cw.tolist()) == {ww}
    assert sorted(set((cy0 + hh // 2).tolist())) == list(range(H)) and sorted(set((cx0 + ww // 2).tolist())) == list(range(W))
    counts = torch.bincount((dx + rx).long(), minlength=2 * rx + 1).double() / 5000       # uniform over the integers
    assert float((counts - 1.0 / (2 * rx + 1)).abs().max()) < 0.03


def test_ada_update():
    from dvd_gan_amd.augment import ada_update
    step = 16 * 4 / (500 * 1000.0)
    assert ada_update(0.5, 0.9, 0.6, 16, 4, 500) == 0.5 + step
    assert ada_update(0.5, 0.1, 0.6, 16, 4, 500) == 0.5 - step
    assert ada_update(0.5, 0.6, 0.6, 16, 4, 500) == 0.5
    assert ada_update(0.5, -1.0, 0.6, 2, 1, 0.008) == 0.25 and ada_update(0.5, 1.0, 0.6, 2, 1, 0.008) == 0.75
    assert ada_update(0.0, 0.1, 0.6, 16, 4, 500) == 0.0 and ada_update(1.0, 0.9, 0.6, 16, 4, 500) == 1.0
    assert ada_update(0.9, 0.9, 0.6, 2, 1, 0.008) == 1.0 and ada_update(0.1, 0.0, 0.6, 2, 1, 0.008) == 0.0


def test_parse_policy():
    from dvd_gan_amd.augment import parse_policy
    assert parse_policy("") == () and parse_policy(None) == ()
    assert parse_policy("cutout, color") == ("color", "cutout")
    assert parse_policy("color,translation,cutout") == ("color", "translation", "cutout")
    with pytest.raises(ValueError, match="flip"):
        parse_policy("color,flip")
    with pytest.raises(ValueError, match="colour"):
        parse_policy("colour")


def test_trainer_refuses_bad_settings_before_it_builds_anything():
    from dvd_gan_amd.train_step import Trainer
    base = dict(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const", total_epoch=1, d_iters=1,
                batch_size=2, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=3, k_sample=4)
    for over, word in ((dict(d_aug="rotation"), "rotation"), (dict(d_aug="color", d_aug_p=1.5), "d_aug_p"),
                       (dict(d_aug="color", d_aug_target=1.0), "d_aug_target"), (dict(d_aug="color", d_aug_interval=0), "d_aug_interval"),
                       (dict(d_aug="color", d_aug_kimg=0), "d_aug_kimg")):
        with pytest.raises(ValueError, match=word):
            Trainer([], argparse.Namespace(**dict(base, **over)), device=torch.device("cpu"), compute_dtype=torch.float32)


# ------------------------------------------------------------------ the aug library (its handshake: tests/test_abi_cpu.py)
def test_table_columns_are_the_restatement_s():
    from dvd_gan_amd import lib as L
    assert L.AUG_COLS == R.COLS == len(R.IDENTITY)


def test_resource_file_shows_no_scratch_and_no_spills():
    """csrc/build.sh keeps hipcc's resource remarks of the aug library: both kernels, in their 16-byte and their dword form, run
    from registers, and their only LDS is the four wave sums."""
    from test_abi_cpu import ROOT
    text = open(os.path.join(ROOT, "dvd_gan_amd", "csrc", "aug", "build", "clip_aug.res")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert sum("aug_forward_kernel" in n for n in names) == 2 and sum("aug_backward_kernel" in n for n in names) == 2
    assert len(names) == 4
    for field, most in (("ScratchSize \\[bytes/lane\\]", 0), ("SGPRs Spill", 0), ("VGPRs Spill", 0), ("LDS Size \\[bytes/block\\]", 32)):
        values = [int(v) for v in re.findall(field + r": (\d+)", text)]
        assert len(values) == len(names) and max(values) <= most, (field, values)


def test_refusals_come_before_any_launch():
    from dvd_gan_amd import lib as L
    au = L.aug_lib()
    for fn in (au.dvd_aug_clip_forward, au.dvd_aug_clip_backward):
        def call(x=P_, y=Q_, params=P_, n=4, fpc=2, H=8, W=8):
            return fn(x, y, params, n, fpc, H, W, None)
        for name in ("x", "y", "params"):
            assert call(**{name: None}) == E_ARG, name
        assert call(y=P_) == E_ARG                                      # in place
        assert call(fpc=0) == E_ARG and call(fpc=-3) == E_ARG and call(n=-1) == E_ARG
        assert call(H=0) == E_SHAPE and call(W=0) == E_SHAPE
        assert call(H=L.AUG_MAX_SIDE + 1) == E_SHAPE and call(W=L.AUG_MAX_SIDE + 1) == E_SHAPE
        assert call(n=1 << 31) == E_SHAPE and call(n=L.AUG_MAX_FRAMES + 1) == E_SHAPE
        assert call(n=0) == 0                                           # nothing to do: succeeds, launches nothing
    assert au.dvd_aug_strerror(0) == b"ok" and au.dvd_aug_strerror(-77) == b"unknown error"
    assert b"frames_per_clip" in au.dvd_aug_strerror(E_ARG) and b"4096" in au.dvd_aug_strerror(E_SHAPE) and str(L.AUG_MAX_FRAMES).encode() in au.dvd_aug_strerror(E_SHAPE)
    with pytest.raises(RuntimeError, match="libdvdgan_hip_aug"):
        L.aug_check(E_ARG)

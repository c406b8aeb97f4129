"""Geometric augmentation of the discriminators' inputs without a GPU: the policy parser, the tables of geom_augment.draw_geom,
the fp64 restatement the GPU tests compare with (tests/geom_ref.py), the geom library's refusals (which come back
before anything touches the device) and its resource file."""
import argparse
import math
import os
import re

import pytest
import torch

import geom_ref as R

E_ARG, E_SHAPE = -1, -2
P_, Q_ = 64, 128          # non-null placeholder pointers: the refusals come before anything is dereferenced
ALL = "xflip,rot90,scale,rotate,aniso"


# ------------------------------------------------------------------ the parser
def test_parse_geom():
    from dvd_gan_amd.geom_augment import GEOM_POLICIES, parse_geom
    assert GEOM_POLICIES == ("xflip", "rot90", "scale", "rotate", "aniso")
    assert parse_geom("") == () and parse_geom(None) == ()
    assert parse_geom("rotate, xflip") == ("xflip", "rotate")
    assert parse_geom(ALL) == GEOM_POLICIES
    with pytest.raises(ValueError, match="yflip"):
        parse_geom("xflip,yflip")
    with pytest.raises(ValueError, match="color"):
        parse_geom("color")


# ------------------------------------------------------------------ the tables
def test_draw_geom_leaves_the_stream_where_it_is_whatever_the_policy():
    from dvd_gan_amd.geom_augment import draw_geom
    states = []
    for policy, p in (("", 1.0), ("xflip", 0.0), (ALL, 1.0), ("rotate,aniso", 0.3)):
        gen = torch.Generator().manual_seed(5)
        draw_geom(4, 16, 16, policy, p, gen)
        states.append(gen.get_state())
    assert all(torch.equal(states[0], s) for s in states[1:])
    gen = torch.Generator().manual_seed(5)
    torch.rand(4, 11, dtype=torch.float64, generator=gen)              # exactly this one call
    assert torch.equal(states[0], gen.get_state())
    before = torch.get_rng_state()
    draw_geom(3, 8, 8, ALL, 1.0, torch.Generator().manual_seed(1))
    assert torch.equal(before, torch.get_rng_state())                  # the default generator is not touched
    a = draw_geom(6, 64, 64, ALL, 0.7, torch.Generator().manual_seed(9))
    b = draw_geom(6, 64, 64, ALL, 0.7, torch.Generator().manual_seed(9))
    assert torch.equal(a, b) and a.dtype == torch.float32 and tuple(a.shape) == (6, R.COLS)


def test_draw_geom_identity_rows_and_gates():
    from dvd_gan_amd.geom_augment import IDENTITY_ROW, draw_geom
    assert IDENTITY_ROW == R.IDENTITY
    ident = torch.tensor(R.IDENTITY).repeat(50, 1)
    for policy, p in ((ALL, 0.0), ("", 1.0)):
        t = draw_geom(50, 12, 12, policy, p, torch.Generator().manual_seed(2))
        assert torch.equal(t, ident) and not bool(torch.signbit(t).any())            # exactly, and no negative zero
    for name in ("xflip", "rot90", "scale", "rotate", "aniso"):
        assert not torch.equal(draw_geom(50, 12, 12, name, 1.0, torch.Generator().manual_seed(2)), ident), name
    # a gate is one comparison with p: at p = 0.5 about half of the clips take a group, and the groups' gates are independent
    flip = draw_geom(4000, 12, 12, "xflip", 0.5, torch.Generator().manual_seed(4))[:, 0] < 0
    turn = (draw_geom(4000, 12, 12, "rotate", 0.5, torch.Generator().manual_seed(4)) != torch.tensor(R.IDENTITY)).any(1)
    assert 0.45 < float(flip.float().mean()) < 0.55 and 0.45 < float(turn.float().mean()) < 0.55
    assert 0.2 < float((flip & turn).float().mean()) < 0.3


def test_draw_geom_mirrors_and_quarter_turns_are_exact():
    """Rows of xflip and rot90 alone: entries 0 or +-1, integer offsets, and the warp they state is torch.flip / torch.rot90."""
    from dvd_gan_amd.geom_augment import draw_geom
    H = W = 12
    t = draw_geom(400, H, W, "xflip,rot90", 0.5, torch.Generator().manual_seed(3)).double()
    assert bool(torch.isin(t[:, [0, 1, 3, 4]], torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)).all())
    assert torch.equal(t[:, [2, 5]], t[:, [2, 5]].round()) and bool((t[:, 0] * t[:, 4] - t[:, 1] * t[:, 3]).abs().eq(1).all())
    assert len({tuple(r) for r in t.tolist()}) == 8                                    # the eight symmetries of the square
    x = torch.rand(3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    u = torch.rand(400, 11, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for i in range(0, 400, 37):
        k = int(u[i, 2] * 4) if u[i, 1] < 0.5 else 0
        want = torch.rot90(x.flip(-1) if u[i, 0] < 0.5 else x, k, (-2, -1))                              # the mirror first
        assert torch.equal(R.frame(x, t[i].tolist()), want), (i, k)
    only = draw_geom(5, H, W, "xflip", 1.0, torch.Generator().manual_seed(3))
    assert torch.equal(only, torch.tensor([R.hand_rows(H, W)["xflip"]]).repeat(5, 1))
    assert torch.equal(R.frame(x, only[0].tolist()), x.flip(-1))


def test_draw_geom_determinant_and_centre():
    """|det| of a row is 1 / s^2 with s the isotropic scale in [2^-0.6, 2^0.6] (rotation, mirror and aniso have |det| 1), and
    every row maps the frame centre to itself."""
    from dvd_gan_amd.geom_augment import draw_geom
    H, W = 10, 16
    lo, hi = 2.0 ** (-2 * 0.2 * 3.0), 2.0 ** (2 * 0.2 * 3.0)
    t = draw_geom(5000, H, W, "xflip,scale,rotate,aniso", 1.0, torch.Generator().manual_seed(8)).double()
    det = t[:, 0] * t[:, 4] - t[:, 1] * t[:, 3]
    assert bool((det < 0).all())                                                        # the mirror
    assert lo * (1 - 1e-6) <= float(det.abs().min()) and float(det.abs().max()) <= hi * (1 + 1e-6)
    assert float(det.abs().min()) < 0.6 and float(det.abs().max()) > 1.7                # the clamp is reached for, both ways
    cx, cy = (W - 1) / 2, (H - 1) / 2
    assert float((t[:, 0] * cx + t[:, 1] * cy + t[:, 2] - cx).abs().max()) < 1e-5
    assert float((t[:, 3] * cx + t[:, 4] * cy + t[:, 5] - cy).abs().max()) < 1e-5
    for name in ("rotate", "aniso"):
        t = draw_geom(500, H, W, name, 1.0, torch.Generator().manual_seed(8)).double()
        assert float(((t[:, 0] * t[:, 4] - t[:, 1] * t[:, 3]) - 1).abs().max()) < 1e-6, name
    # scale alone magnifies the content by s: the row is diag(1 / s) about the centre, log2 s ~ N(0, 0.2^2)
    t = draw_geom(5000, H, W, "scale", 1.0, torch.Generator().manual_seed(8)).double()
    assert torch.equal(t[:, 0], t[:, 4]) and float(t[:, [1, 3]].abs().max()) == 0.0
    n = -torch.log2(t[:, 0]) / 0.2
    assert abs(float(n.mean())) < 0.06 and 0.93 < float(n.std()) < 1.05 and float(n.abs().max()) <= 3.0 + 1e-5
    # rotate alone: the angle covers the circle
    t = draw_geom(5000, H, W, "rotate", 1.0, torch.Generator().manual_seed(8)).double()
    ang = torch.atan2(t[:, 3], t[:, 0])
    assert float(ang.min()) < -3.1 and float(ang.max()) > 3.1 and abs(float(ang.mean())) < 0.1


def test_draw_geom_refuses_quarter_turns_of_oblong_frames():
    from dvd_gan_amd.geom_augment import draw_geom
    with pytest.raises(ValueError, match="rot90"):
        draw_geom(2, 8, 12, "xflip,rot90", 0.0)
    draw_geom(2, 8, 12, "xflip,scale,rotate,aniso", 1.0)


# ------------------------------------------------------------------ the fp64 restatement
@pytest.mark.parametrize("name", [n for n in R.hand_rows(6, 10) if n != "nan"])
def test_reference_backward_is_the_transpose_of_its_forward(name):
    H, W = 6, 10
    row = R.hand_rows(H, W)[name]
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(3, 3, H, W, dtype=torch.float64, generator=gen) * 2 - 1
    g = torch.randn(3, 3, H, W, dtype=torch.float64, generator=gen)
    mats = torch.tensor([row, row], dtype=torch.float32)
    y, mag, slack = R.clip(x, mats, 2)
    dx, dmag, dslack, terms = R.clip_grad(x, g, mats, 2)
    lhs, rhs = float((y * g).sum()), float((x * dx).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((mag * g.abs()).sum() + 1.0), (lhs, rhs)
    assert bool((y.abs() <= mag * (1 + 1e-12)).all()) and bool((dx.abs() <= dmag * (1 + 1e-12)).all())
    assert bool((slack >= 0).all()) and bool((dslack >= 0).all()) and bool((terms >= 0).all())
    if name == "identity":
        assert torch.equal(y, x) and torch.equal(dx, g)
    if name in R.ZERO_ROWS:
        assert float(y.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0
    if name == "magnify by 2":                  # sx moves by 1 / 2 per output pixel: 3 or 4 output pixels per axis reach a source pixel
        assert 9 <= float(terms.max()) <= 16
    if name == "singular":                      # every output pixel sits on source pixel (0, 0)
        assert float(terms[0, 0, 0, 0]) == H * W and float(terms.sum()) == 3 * 3 * H * W


def test_reference_against_a_hand_computation():
    """A 2 x 2 frame, sx = x + 0.5, sy = y: output (0, 0) is the mean of the two pixels of line 0, output (1, 0) half of pixel
    (1, 0) (its right neighbour is outside: zero fill); the transpose hands g back by the same weights.  A NaN row gives zeros."""
    x = torch.tensor([[[1.0, 3.0], [5.0, 8.0]]], dtype=torch.float64).repeat(3, 1, 1)
    y = R.frame(x, (1.0, 0.0, 0.5, 0.0, 1.0, 0.0))
    assert torch.equal(y[0], torch.tensor([[2.0, 1.5], [6.5, 4.0]], dtype=torch.float64))
    g = torch.tensor([[[1.0, 10.0], [100.0, 1000.0]]], dtype=torch.float64).repeat(3, 1, 1)
    dx, *_ = R.clip_grad(x[None], g[None], torch.tensor([[1.0, 0.0, 0.5, 0.0, 1.0, 0.0]]), 1)
    assert torch.equal(dx[0, 0], torch.tensor([[0.5, 5.5], [50.0, 550.0]], dtype=torch.float64))
    assert float(R.frame(x, (math.nan,) * 6).abs().max()) == 0.0


# ------------------------------------------------------------------ the Trainer's settings
def test_trainer_refuses_bad_settings_before_it_builds_anything():
    from dvd_gan_amd.train_step import Trainer
    base = dict(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const", total_epoch=1, d_iters=1,
                batch_size=2, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=3, k_sample=4)
    for over, word in ((dict(d_aug_geom="flip"), "flip"), (dict(d_aug_geom="translation"), "translation"),
                       (dict(d_aug_geom="rotate", d_aug_p=1.5), "d_aug_p"), (dict(d_aug_geom="rotate", d_aug_target=1.0), "d_aug_target")):
        with pytest.raises(ValueError, match=word):
            Trainer([], argparse.Namespace(**dict(base, **over)), device=torch.device("cpu"), compute_dtype=torch.float32)


# ------------------------------------------------------------------ the geom library (its handshake: tests/test_abi_cpu.py)
def test_table_columns_are_the_restatement_s():
    from dvd_gan_amd import lib as L
    assert L.GEOM_COLS == R.COLS == len(R.IDENTITY)


def test_resource_file_shows_no_scratch_and_no_spills():
    """csrc/build.sh keeps hipcc's resource remarks of the geom library: both kernels run from registers, without LDS."""
    from test_abi_cpu import ROOT
    text = open(os.path.join(ROOT, "dvd_gan_amd", "csrc", "geom", "build", "clip_warp.res")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert sum("geom_forward_kernel" in n for n in names) == 1 and sum("geom_backward_kernel" in n for n in names) == 1
    assert len(names) == 2
    for field, most in (("ScratchSize \\[bytes/lane\\]", 0), ("SGPRs Spill", 0), ("VGPRs Spill", 0), ("LDS Size \\[bytes/block\\]", 0)):
        values = [int(v) for v in re.findall(field + r": (\d+)", text)]
        assert len(values) == len(names) and max(values) <= most, (field, values)


def test_refusals_come_before_any_launch():
    from dvd_gan_amd import lib as L
    ge = L.geom_lib()
    for fn in (ge.dvd_geom_clip_forward, ge.dvd_geom_clip_backward):
        def call(x=P_, y=Q_, mats=P_, n=4, fpc=2, H=8, W=8):
            return fn(x, y, mats, n, fpc, H, W, None)
        for name in ("x", "y", "mats"):
            assert call(**{name: None}) == E_ARG, name
        assert call(y=P_) == E_ARG                                      # in place
        assert call(fpc=0) == E_ARG and call(fpc=-3) == E_ARG and call(n=-1) == E_ARG
        assert call(H=0) == E_SHAPE and call(W=0) == E_SHAPE
        assert call(H=L.GEOM_MAX_SIDE + 1) == E_SHAPE and call(W=L.GEOM_MAX_SIDE + 1) == E_SHAPE
        assert call(n=1 << 31) == E_SHAPE and call(n=L.GEOM_MAX_FRAMES + 1) == E_SHAPE
        assert call(n=0) == 0                                           # nothing to do: succeeds, launches nothing
    assert ge.dvd_geom_strerror(0) == b"ok" and ge.dvd_geom_strerror(-77) == b"unknown error"
    assert b"frames_per_clip" in ge.dvd_geom_strerror(E_ARG) and b"4096" in ge.dvd_geom_strerror(E_SHAPE)
    assert str(L.GEOM_MAX_FRAMES).encode() in ge.dvd_geom_strerror(E_SHAPE) and b"launch" in ge.dvd_geom_strerror(-3)
    with pytest.raises(RuntimeError, match="libdvdgan_hip_geom"):
        L.geom_check(E_ARG)

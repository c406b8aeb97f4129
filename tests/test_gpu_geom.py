"""The clip warp on the GPU: dvd_geom_clip_forward / dvd_geom_clip_backward against the fp64 restatement of tests/geom_ref.py
within the bound that module derives (coordinate error times the largest neighbour difference, plus counted fp32 roundings on
`mag`), the adjoint identity on the device results, bit-exact mirrors and quarter turns, rows that must give zeros, determinism
and frame independence.  Frames of 8 x 8, 5 x 7 and 16 x 16; five frames in clips of two, so the last clip is partial."""
import math

import pytest
import torch

import geom_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [(8, 8), (5, 7), (16, 16)]
N_FRAMES, FPC = 5, 2
ALL = "xflip,rot90,scale,rotate,aniso"


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


def _data(H, W, n=N_FRAMES, seed=0):
    gen = torch.Generator().manual_seed(1000 * H + W + seed)
    return torch.rand(n, 3, H, W, generator=gen) * 2 - 1, torch.randn(n, 3, H, W, generator=gen)


def _run(x, g, mats, fpc=FPC):
    from dvd_gan_amd.geom_augment import clip_warp_backward, clip_warp_forward
    m = mats.to(DEV)
    y, dx = clip_warp_forward(x.to(DEV), m, fpc), clip_warp_backward(g.to(DEV), m, fpc)
    torch.cuda.synchronize()
    return y.cpu(), dx.cpu()


def _check(x, g, mats, y, dx, what, fpc=FPC):
    """Forward and backward within the derived bound, and <F x, g> = <x, F^T g> on the device results within the same bound."""
    want, mag, slack = R.clip(x, mats, fpc)
    dwant, dmag, dslack, terms = R.clip_grad(x, g, mats, fpc)
    fb, bb = R.forward_bound(mag, slack), R.backward_bound(dmag, dslack, terms)
    ef, eb = (y.double() - want).abs(), (dx.double() - dwant).abs()
    finite = torch.isfinite(fb) & torch.isfinite(bb)
    print(f"[geom] {what}: forward error / bound {float((ef / fb.clamp_min(1e-300)).max()):.3f}, "
          f"backward {float((eb / bb.clamp_min(1e-300)).max()):.3f}")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()), what
    assert bool((ef <= fb).all()), (what, "forward")
    assert bool((eb <= bb).all()), (what, "backward")
    x64, g64 = x.double(), g.double()
    for n in range(x.shape[0]):
        if bool(finite[n].all()):
            lhs, rhs = float((y[n].double() * g64[n]).sum()), float((x64[n] * dx[n].double()).sum())
            assert abs(lhs - rhs) <= float((fb[n] * g64[n].abs()).sum() + (bb[n] * x64[n].abs()).sum()), (what, n, lhs, rhs)


@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_hand_made_rows_against_the_reference(H, W):
    rows = R.hand_rows(H, W)
    x, g = _data(H, W)
    clips = -(-N_FRAMES // FPC)
    names = list(rows)
    # every row takes each position of the table once or more: the full clips and the partial one
    for first in range(0, len(names), clips):
        chunk = [names[(first + i) % len(names)] for i in range(clips)]
        mats = torch.tensor([rows[n] for n in chunk], dtype=torch.float32)
        y, dx = _run(x, g, mats)
        _check(x, g, mats, y, dx, f"{H}x{W} {chunk}")
        for n in range(N_FRAMES):
            name = chunk[n // FPC]
            if name == "identity":                              # skipped, not computed: the bits of the input
                assert torch.equal(_bits(y[n]), _bits(x[n])) and torch.equal(_bits(dx[n]), _bits(g[n]))
            if name in R.ZERO_ROWS:
                assert float(y[n].abs().max()) == 0.0 and float(dx[n].abs().max()) == 0.0, name
            if name == "singular":                              # every output pixel reads source pixel (0, 0)
                assert torch.equal(y[n], x[n, :, :1, :1].expand_as(y[n]))
                assert float(dx[n].reshape(3, -1)[:, 1:].abs().max()) == 0.0 and float(dx[n, :, 0, 0].abs().min()) > 0.0


@pytest.mark.parametrize("H,W", [(8, 8), (16, 16)], ids=["8x8", "16x16"])
def test_mirror_and_quarter_turns_move_bits(H, W):
    """Integer positions take the source pixel itself; the transpose of a permutation is its inverse."""
    rows = R.hand_rows(H, W)
    x, g = _data(H, W, n=1)
    for name, fwd, inv in (("xflip", lambda t: t.flip(-1), lambda t: t.flip(-1)),
                           ("rot90 k=1", lambda t: torch.rot90(t, 1, (-2, -1)), lambda t: torch.rot90(t, 3, (-2, -1))),
                           ("rot90 k=2", lambda t: torch.rot90(t, 2, (-2, -1)), lambda t: torch.rot90(t, 2, (-2, -1))),
                           ("rot90 k=3", lambda t: torch.rot90(t, 3, (-2, -1)), lambda t: torch.rot90(t, 1, (-2, -1)))):
        y, dx = _run(x, g, torch.tensor([rows[name]], dtype=torch.float32), 1)
        assert torch.equal(_bits(y), _bits(fwd(x))), name
        assert torch.equal(dx, inv(g)), name


def test_absurd_rows_leave_their_neighbours_alone():
    """A row of 1e30 and a NaN row between ordinary clips: zeros for their frames, and the frames before and after are what they
    are without them."""
    H, W = 5, 7
    rows = R.hand_rows(H, W)
    x, g = _data(H, W, n=6)
    for bad in ("huge", "nan"):
        mats = torch.tensor([rows["rotate 45"], rows[bad], rows["everything"]], dtype=torch.float32)
        y, dx = _run(x, g, mats)
        assert float(y[2:4].abs().max()) == 0.0 and float(dx[2:4].abs().max()) == 0.0, bad
        clean = torch.tensor([rows["rotate 45"], rows["identity"], rows["everything"]], dtype=torch.float32)
        y0, dx0 = _run(x, g, clean)
        for n in (0, 1, 4, 5):
            assert torch.equal(_bits(y[n]), _bits(y0[n])) and torch.equal(_bits(dx[n]), _bits(dx0[n])), (bad, n)


@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_backward_is_deterministic_and_frame_independent(H, W):
    from dvd_gan_amd.geom_augment import clip_warp_backward, clip_warp_forward
    rows = R.hand_rows(H, W)
    mats = torch.tensor([rows["everything"], rows["magnify by 2"], rows["singular"]], dtype=torch.float32).to(DEV)
    x, _ = _data(H, W)
    x = x.to(DEV)
    for fn in (clip_warp_forward, clip_warp_backward):
        a, b = fn(x, mats, FPC), fn(x, mats, FPC)
        torch.cuda.synchronize()
        assert torch.equal(_bits(a), _bits(b)), fn.__name__                        # two launches
        # the same frames presented at another n_frames: the first clip alone, the partial last clip alone, a frame alone
        head = fn(x[:2].clone(), mats[:1].clone(), FPC)
        tail = fn(x[4:].clone(), mats[2:].clone(), FPC)
        one = fn(x[3:4].clone(), mats[1:2].clone(), 1)
        assert torch.equal(_bits(head), _bits(a[:2])) and torch.equal(_bits(tail), _bits(a[4:])), fn.__name__
        assert torch.equal(_bits(one), _bits(a[3:4])), fn.__name__


def test_two_hundred_drawn_rows():
    """draw_geom's rows at p = 1 with every group, one frame per clip."""
    from dvd_gan_amd.geom_augment import draw_geom
    H = W = 16
    mats = draw_geom(200, H, W, ALL, 1.0, torch.Generator().manual_seed(12))
    x, g = _data(H, W, n=200)
    y, dx = _run(x, g, mats, 1)
    _check(x, g, mats, y, dx, "200 drawn rows", 1)
    assert float(y.abs().max()) > 0.5 and float(dx.abs().max()) > 0.5


def test_refusals_leave_the_output_untouched():
    from dvd_gan_amd import lib as L
    from dvd_gan_amd.geom_augment import ClipWarp, clip_warp_forward
    ge = L.geom_lib()
    x = torch.rand(4, 3, 8, 8, device=DEV)
    y = torch.full_like(x, 7.0)
    mats = torch.tensor([R.hand_rows(8, 8)["everything"]] * 2, dtype=torch.float32, device=DEV)
    for fn in (ge.dvd_geom_clip_forward, ge.dvd_geom_clip_backward):
        assert fn(L.ptr(y), L.ptr(y), L.ptr(mats), 4, 2, 8, 8, L.stream()) == -1          # in place
        assert fn(None, L.ptr(y), L.ptr(mats), 4, 2, 8, 8, L.stream()) == -1
        assert fn(L.ptr(x), L.ptr(y), None, 4, 2, 8, 8, L.stream()) == -1
        assert fn(L.ptr(x), L.ptr(y), L.ptr(mats), 4, 0, 8, 8, L.stream()) == -1           # frames_per_clip = 0
        assert fn(L.ptr(x), L.ptr(y), L.ptr(mats), 4, 2, 8, 4097, L.stream()) == -2
        assert fn(L.ptr(x), L.ptr(y), L.ptr(mats), 0, 2, 8, 8, L.stream()) == 0            # no frames: succeeds, launches nothing
        torch.cuda.synchronize()
        assert float(y.min()) == 7.0 and float(y.max()) == 7.0
    with pytest.raises(ValueError, match="table"):
        clip_warp_forward(x, mats[:1], 2)
    with pytest.raises(ValueError, match="clips"):
        ClipWarp.apply(x, mats)
    # autograd through ClipWarp is the backward launch
    clips = x.view(2, 2, 3, 8, 8).clone().requires_grad_(True)
    out = ClipWarp.apply(clips, mats)
    gr = torch.randn_like(out)
    out.backward(gr)
    from dvd_gan_amd.geom_augment import clip_warp_backward
    assert torch.equal(clips.grad.view(4, 3, 8, 8), clip_warp_backward(gr.view(4, 3, 8, 8), mats, 2))
    assert math.isfinite(float(out.detach().sum()))

"""Sample sheets on the GPU (sheets.make_sheets -> dvd_sample_sheet; Trainer.save_samples / save_predictions / train): every case
bit for bit against the restatement of tests/test_sheets_cpu.py (which that file checks against Pillow's paste of torch-quantised
tiles).  The bytes are integers from three separately rounded fp32 operations: nothing here has a tolerance."""
import argparse
import itertools
import os

import numpy as np
import pytest
import torch

from test_sheets_cpu import prefixed, quantise, restate, walk_chunks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _frames(seed, *shape):
    """Values that use the whole byte range and leave it on both sides."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.9


def _both_forms(dev_frames, host_tiles, msg, **kw):
    """make_sheets in the plain and the prefixed form == the restatement of host_tiles [n_sheets, n_tiles, 3, H, W]."""
    from dvd_gan_amd import sheets as S
    rkw = {k: v for k, v in kw.items() if k != "layout"}
    want = restate(host_tiles, **rkw)
    plain = S.make_sheets(dev_frames, **kw)
    pre = S.make_sheets(dev_frames, row_prefix=True, **kw)
    assert plain.dtype == pre.dtype == torch.uint8 and plain.is_cuda and pre.is_cuda
    assert tuple(plain.shape) == want.shape and tuple(pre.shape) == prefixed(want).shape, msg
    np.testing.assert_array_equal(plain.cpu().numpy(), want, err_msg=msg)
    np.testing.assert_array_equal(pre.cpu().numpy(), prefixed(want), err_msg=msg + " (prefixed)")
    return want


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("H,W", [(1, 1), (4, 4), (6, 10), (5, 3), (64, 64)])
def test_every_geometry_matches_the_restatement(H, W):
    """tiles 1 / 5 / 8 / 9 x nrow 1 / 2 / 8 (a single column, partial last rows) x padding 0 / 1 / 2 x pad_value x 1 and 3 sheets;
    5 x 3 makes rows of 3 (2 + 3 k) (+ 1) bytes: no multiple of 4, sheets and rows starting at odd addresses.  Fewer tiles than
    the tensor holds are a view of it: the sheet stride is not the tiles' extent."""
    small = H * W < 4096
    host = _frames(H * 131 + W, 3, 9, 3, H, W)
    dev = host.to(DEV)
    cases = list(itertools.product((1, 3), (1, 5, 8, 9), (1, 2, 8), (0, 1, 2), (0.0, 0.5, 1.0)))
    if not small:           # 64 x 64: three sheets of 5 and 9 tiles in every arrangement, and the lone tile
        cases = [c for c in cases if c[4] == 0.5 and (c[:2] in ((3, 5), (3, 9)) or c[:3] == (1, 1, 8))]
    for n_sheets, tiles, nrow, padding, pad_value in cases:
        _both_forms(dev[:n_sheets, :tiles], host[:n_sheets, :tiles], f"{n_sheets} x {tiles} tiles, nrow {nrow}, padding {padding}, "
                    f"pad {pad_value}", nrow=nrow, padding=padding, pad_value=pad_value)


def test_wide_rows_cross_the_chunk_boundaries():
    """A row of 8 tiles of 64 pixels is 1590 bytes, two of a workgroup's 1024-byte chunks; 9 tiles of 150 x 200 in one row make
    5456-byte rows (6 chunks) whose sheets start at every phase of a dword."""
    host = _frames(9, 3, 9, 3, 15, 200)
    _both_forms(host.to(DEV), host, "9 x 15 x 200 in a row", nrow=9, padding=1, pad_value=1.0)


def test_both_layouts_of_one_tensor():
    host = _frames(2, 3, 5, 3, 6, 10)
    dev = host.to(DEV)
    by_clip = _both_forms(dev, host, "frames", layout="frames", nrow=2)
    by_step = _both_forms(dev, host.transpose(0, 1), "clips", layout="clips", nrow=2)
    assert by_clip.shape[0] == 3 and by_step.shape[0] == 5
    # tile (b, t) is the same picture in both
    np.testing.assert_array_equal(by_clip[1, 2:8, 2:12], by_step[0, 2:8, 14:24])
    lead = _frames(2, 2, 2, 5, 3, 6, 10)                               # leading axes fold into one
    _both_forms(lead.to(DEV), lead.reshape(4, 5, 3, 6, 10), "folded")


def test_views_are_read_through_their_strides():
    B, K, T, H, W = 3, 2, 5, 6, 10
    clips = _frames(4, B, 3, K + T, H, W)                              # a loader clip
    dev = clips.to(DEV)
    view = dev[:, :, K:].permute(0, 2, 1, 3, 4)
    assert not view.is_contiguous()
    _both_forms(view, clips[:, :, K:].permute(0, 2, 1, 3, 4), "loader clip, frames", nrow=4)
    _both_forms(view, clips[:, :, K:].permute(2, 0, 1, 3, 4), "loader clip, clips", layout="clips", nrow=2)
    gen = _frames(5, B, K + T, 3, H, W)                                # a generated batch, time-sliced
    _both_forms(gen.to(DEV)[:, 1:4], gen[:, 1:4], "time slice", nrow=2, signed=False)
    _both_forms(gen.to(DEV)[1:, ::2], gen[1:, ::2], "every other frame")


# ------------------------------------------------------------------ values
def _tie_values(signed):
    """For every k in 0 .. 254 the float v whose x * 255 is k + 0.5, and the 64 floats on either side of it."""
    x0 = ((torch.arange(255, dtype=torch.float64) + 0.5) / 255.0)
    v0 = (2 * x0 - 1 if signed else x0).to(torch.float32)
    cols, up, down = [v0], v0, v0
    for _ in range(64):
        up = torch.nextafter(up, torch.full_like(up, float("inf")))
        down = torch.nextafter(down, torch.full_like(down, -float("inf")))
        cols += [up, down]
    return torch.stack(cols).reshape(-1)                                # 129 * 255 = 32 895 values


@pytest.mark.parametrize("signed", [True, False])
def test_ties_and_special_values(signed):
    inf, nan, tiny = float("inf"), float("nan"), 1e-42
    special = torch.tensor([1.0, -1.0, 1.0 + 2 ** -23, -1.0 - 2 ** -23, 2.0, -2.0, 1e30, -1e30, 0.0, -0.0, tiny, -tiny,
                            1.1754944e-38, -1.1754944e-38, inf, -inf, nan, 0.5, -0.5])
    ties = _tie_values(signed)
    H = W = 105                                                         # 3 * 105 * 105 = 33 075 values in one odd-sized tile
    flat = torch.cat([ties, special, torch.zeros(3 * H * W - ties.numel() - special.numel())])
    host = flat.reshape(1, 1, 3, H, W)
    want = _both_forms(host.to(DEV), host, f"ties, signed={signed}", signed=signed, padding=1)
    q = quantise(flat, signed)
    # the ties really straddle a byte boundary: both k and k + 1 occur among the neighbours of every k + 0.5.  (Signed, k = 127 and
    # 128: those v lie within 2^-7 of 0, where 64 floats are far less than one step of x = (v + 1) / 2 near 0.5 -- one byte each.)
    per_k = q[:ties.numel()].reshape(129, 255)
    assert all(set(per_k[:, k].tolist()) <= {k, k + 1} for k in range(255))
    straddled = [k for k in range(255) if set(per_k[:, k].tolist()) == {k, k + 1}]
    assert straddled == [k for k in range(255) if not (signed and k in (127, 128))]
    got_special = want[0, 1:-1, 1:-1].transpose(2, 0, 1).reshape(-1)[ties.numel():ties.numel() + special.numel()].tolist()
    if signed:
        assert got_special == [255, 0, 255, 0, 255, 0, 255, 0, 128, 128, 128, 128, 128, 128, 255, 0, 0, 191, 64]
    else:
        assert got_special == [255, 0, 255, 0, 255, 0, 255, 0, 0, 0, 0, 0, 0, 0, 255, 0, 0, 128, 0]     # NaN: the stated 0


# ------------------------------------------------------------------ composition
def test_launches_with_first_slot_compose_one_sheet():
    from dvd_gan_amd import sheets as S
    H, W, kw = 5, 3, dict(nrow=4, padding=1, pad_value=0.5)
    parts = [_frames(20 + i, 2, n, 3, H, W) for i, n in enumerate((3, 4, 2))]
    whole = torch.cat(parts, 1)
    want = restate(whole, **kw)
    for prefix in (False, True):
        out = S.make_sheets(parts[0].to(DEV), total_slots=9, row_prefix=prefix, **kw)
        S.make_sheets(parts[1].to(DEV), out=out, first_slot=3, total_slots=9, fill=False, row_prefix=prefix, **kw)
        S.make_sheets(parts[2].to(DEV), out=out, first_slot=7, total_slots=9, fill=False, row_prefix=prefix, **kw)
        once = S.make_sheets(whole.to(DEV), row_prefix=prefix, **kw)
        assert torch.equal(out, once)
        np.testing.assert_array_equal(out.cpu().numpy(), prefixed(want) if prefix else want)
    # a filling launch in the middle of the sheet: everything else is pad_value, the slots before it included
    mid = S.make_sheets(parts[1].to(DEV), first_slot=3, total_slots=9, **kw)
    np.testing.assert_array_equal(mid.cpu().numpy(), restate(parts[1], first_slot=3, total_slots=9, **kw))


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("prefix", [False, True])
def test_without_fill_only_the_tiles_are_written_and_nothing_outside_the_buffer(lead, prefix):
    """A sentinel-filled buffer with guard bytes on both sides, starting `lead` bytes off a dword."""
    from dvd_gan_amd import kern as K, sheets as S
    H, W, n_sheets, kw = 5, 3, 3, dict(nrow=2, padding=2)
    tiles = _frames(30, n_sheets, 2, 3, H, W)
    Hs, Ws, nbytes = K.sample_sheet_shape(5, H, W, 2, 2, int(prefix))
    guard, n = 64 + lead, n_sheets * nbytes
    buf = torch.full((guard + n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[guard:guard + n]
    assert out.data_ptr() % 4 == lead
    S.make_sheets(tiles.to(DEV), out=out, first_slot=2, total_slots=5, fill=False, row_prefix=prefix, **kw)
    got = buf.cpu().numpy()
    assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all()
    base = np.full((n_sheets, Hs, Ws, 3), 0xA5, np.uint8)
    want = restate(tiles, first_slot=2, total_slots=5, fill=False, base=base, **kw)
    if prefix:
        want = prefixed(want)
        want[..., 0] = 0xA5                                             # the prefix byte is no tile pixel either
    np.testing.assert_array_equal(got[guard:guard + n].reshape(want.shape), want)
    assert (want == 0xA5).sum() > n // 2                                # most of the sheet is not ours
    S.make_sheets(tiles.to(DEV), out=out, first_slot=2, total_slots=5, fill=True, row_prefix=prefix, **kw)
    got = buf.cpu().numpy()
    assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all()
    full = restate(tiles, first_slot=2, total_slots=5, **kw)
    np.testing.assert_array_equal(got[guard:guard + n].reshape(want.shape), prefixed(full) if prefix else full)


def test_make_sheets_refusals_on_the_device():
    from dvd_gan_amd import sheets as S
    a = torch.zeros(2, 4, 3, 6, 10, device=DEV)
    with pytest.raises(ValueError, match="needs `out`"):
        S.make_sheets(a, fill=False)
    with pytest.raises(ValueError, match=r"out: a contiguous uint8 tensor of 3000 bytes"):
        S.make_sheets(a, out=torch.zeros(10, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="4097"):
        S.make_sheets(torch.zeros(1, 1, 3, 1, 4097, device=DEV))
    assert S.make_sheets(a[:0]).shape == (0, 10, 50, 3)


# ------------------------------------------------------------------ end to end
def _cfg(**extra):
    base = dict(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const", total_epoch=1, d_iters=1,
                batch_size=2, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=2, k_sample=4, log_epoch=0)
    base.update(extra)
    return argparse.Namespace(**base)


def _g_state(tr):
    s = {k: v.detach().clone() for k, v in tr.G.state_dict().items()}
    s["opt.flat"] = tr.g_optimizer.flat.detach().clone()
    if tr.g_optimizer.ema is not None:
        s["opt.ema"] = tr.g_optimizer.ema.detach().clone()
    return s


def _open_rgb(path):
    from PIL import Image
    out = []
    with Image.open(path) as im:
        for i in range(getattr(im, "n_frames", 1)):
            im.seek(i)
            out.append(np.asarray(im.convert("RGB")))
    return out


def test_save_samples_writes_the_references_files_of_sample(tmp_path):
    from dvd_gan_amd.train_step import Trainer
    torch.manual_seed(61)
    tr = Trainer([], _cfg(sample_path=str(tmp_path), version="v1", test_batch_size=2, sample_layout="both", sample_fps=4),
                 device=DEV, compute_dtype=torch.float32)
    gen = torch.Generator().manual_seed(62)
    tr.train_step(torch.rand(2, 3, 8, 64, 64, generator=gen) * 2 - 1, torch.randint(0, 2, (2,), generator=gen))
    z, label = tr.fixed_inputs()
    assert label.tolist() == [0, 0, 1, 1]
    frozen = tr._g_frozen_tensors()
    saved = [t.clone() for t in frozen]
    want = []
    for lo in (0, 2):                                                   # sample() advances u / v: every chunk from the same state
        want.append(tr.sample(z[lo:lo + 2], label[lo:lo + 2]).cpu())
        for t, old in zip(frozen, saved):
            t.copy_(old)
    want = torch.cat(want)                                              # [4, 8, 3, 64, 64] in [0, 1]
    s0, rng = _g_state(tr), torch.get_rng_state()
    tr.save_samples(7)                                                  # chunks of batch_size = 2
    tr.sheet_writer.flush()
    s1 = _g_state(tr)
    assert [k for k in s0 if not torch.equal(s0[k], s1[k])] == [] and torch.equal(rng, torch.get_rng_state()) and tr.G.training
    folder = os.path.join(str(tmp_path), "v1")
    names = ["Class_%d_No.%d_Step_7.png" % (i, j) for i in range(2) for j in range(2)]
    assert sorted(os.listdir(folder)) == sorted(names + ["Step_7.apng"])
    sheets = restate(want, signed=False)                                # make_grid's defaults: 8 frames in one row
    assert sheets.shape == (4, 68, 530, 3)
    assert len({s.tobytes() for s in sheets}) == 4                      # four different pictures: a file under another clip's name shows
    for n, name in enumerate(names):
        walk_chunks(os.path.join(folder, name))
        (got,) = _open_rgb(os.path.join(folder, name))
        np.testing.assert_array_equal(got, sheets[n], err_msg=name)
    frames = _open_rgb(os.path.join(folder, "Step_7.apng"))
    steps = restate(want.transpose(0, 1), signed=False, nrow=2)         # a row per class
    assert len(frames) == 8 and steps.shape == (8, 134, 134, 3)
    for t in range(8):
        np.testing.assert_array_equal(frames[t], steps[t], err_msg=f"frame {t}")
    from PIL import Image
    with Image.open(os.path.join(folder, "Step_7.apng")) as im:
        assert im.info["duration"] == 250.0 and im.info["loop"] == 0
    # one chunk, the caller's own z / labels, and the loader's clips
    tr.sample_layout = "frames"
    tr.save_samples(8, z.cpu(), torch.tensor([1, 0, 1, 1]), chunk=4)
    real = torch.rand(2, 3, 8, 64, 64, generator=gen) * 2 - 1
    tr.save_real(real)
    tr.close_sheets()
    assert tr._sheets is None
    assert {"Class_1_No.0_Step_8.png", "Class_0_No.0_Step_8.png", "Class_1_No.1_Step_8.png", "Class_1_No.2_Step_8.png",
            "real_0.png", "real_1.png"} <= set(os.listdir(folder))
    (got,) = _open_rgb(os.path.join(folder, "real_1.png"))
    np.testing.assert_array_equal(got, restate(real.permute(0, 2, 1, 3, 4))[1])
    s2 = _g_state(tr)
    assert [k for k in s0 if not torch.equal(s0[k], s2[k])] == []


@pytest.mark.parametrize("use_ema", [False, True])
def test_training_with_sample_sheets_is_training_without(tmp_path, use_ema):
    """Three bf16 steps through Trainer.train() with sample_step = 1 and with sample_step = 0: the same six losses bit for bit,
    the same weights, u / v, statistics, averages and default generator afterwards."""
    from dvd_gan_amd.train_step import Trainer
    gen = torch.Generator().manual_seed(71)
    batch = (torch.rand(2, 3, 8, 64, 64, generator=gen) * 2 - 1, torch.randint(0, 2, (2,), generator=gen))
    extra = dict(ema_decay=0.9, sample_use_ema=True, ema_standing_stats=1) if use_ema else {}

    def run(sample_step):
        torch.manual_seed(72)
        tr = Trainer([batch], _cfg(total_epoch=3, sample_step=sample_step, sample_path=str(tmp_path), version=f"s{sample_step}",
                                   test_batch_size=1, sample_layout="both", **extra), device=DEV, compute_dtype=torch.bfloat16)
        losses, step = [], tr.train_step
        tr.train_step = lambda *a, **k: losses.append(step(*a, **k)) or losses[-1]
        tr.train()
        torch.cuda.synchronize()
        return tr, [[float(v.detach()) for v in six] for six in losses], _g_state(tr), torch.get_rng_state()

    tr0, l0, s0, r0 = run(0)
    assert tr0._sheets is None and tr0._fixed is None and not os.path.exists(os.path.join(str(tmp_path), "s0"))
    tr1, l1, s1, r1 = run(1)
    assert len(l0) == len(l1) == 3 and all(len(six) == 6 for six in l1)
    assert l0 == l1
    assert [k for k in s0 if not torch.equal(s0[k], s1[k])] == [] and torch.equal(r0, r1)
    assert tr1._sheets is None                                          # train() closed its writer: the files are complete
    files = sorted(os.listdir(os.path.join(str(tmp_path), "s1")))
    assert files == sorted(["Class_%d_No.0_Step_%d.png" % (c, s) for c in range(2) for s in (1, 2, 3)]
                           + ["Step_%d.apng" % s for s in (1, 2, 3)])
    for name in files:
        walk_chunks(os.path.join(str(tmp_path), "s1", name))
    assert _open_rgb(os.path.join(str(tmp_path), "s1", "Class_1_No.0_Step_3.png"))[0].shape == (68, 530, 3)
    assert [f.shape for f in _open_rgb(os.path.join(str(tmp_path), "s1", "Step_3.apng"))] == [(134, 68, 3)] * 8     # a row per class


def test_save_predictions_rows_are_the_real_clip_and_the_rollouts(tmp_path):
    from dvd_gan_amd.train_step import Trainer
    K_, T, B, horizon, n_samples = 2, 6, 2, 9, 2
    torch.manual_seed(81)
    tr = Trainer([], _cfg(n_frames=T, n_cond=K_, k_sample=2, n_class=3, z_dim=8, sample_path=str(tmp_path), version=""),
                 device=DEV, compute_dtype=torch.float32)
    gen = torch.Generator().manual_seed(82)
    tr.train_step(torch.rand(B, 3, K_ + T, 64, 64, generator=gen) * 2 - 1, torch.randint(0, 3, (B,), generator=gen))
    clips = torch.rand(B, 3, K_ + horizon, 64, 64, generator=gen) * 2 - 1
    labels = torch.randint(0, 3, (B,), generator=gen)
    s0, rng = _g_state(tr), torch.get_rng_state()
    tr.save_predictions(5, clips, labels, n_samples=n_samples, horizon=horizon, seed=9)
    tr.close_sheets()
    s1 = _g_state(tr)
    assert [k for k in s0 if not torch.equal(s0[k], s1[k])] == [] and torch.equal(rng, torch.get_rng_state()) and tr.G.training
    assert sorted(os.listdir(str(tmp_path))) == ["Pred_0_Step_5.png", "Pred_1_Step_5.png"]
    frames = clips.permute(0, 2, 1, 3, 4)                               # [B, K + horizon, 3, H, W] in [-1, 1]
    L = K_ + horizon
    zgen = torch.Generator().manual_seed(9)
    # row 1 + s = the context (raw [-1, 1]) followed by rollout(z_s) (already in [0, 1]: denorm is the kernel's signed path)
    futures = [tr.rollout(frames[:, :K_].contiguous(), labels, horizon, z=torch.randn(B, 8, generator=zgen)).cpu()
               for s in range(n_samples)]
    want_real = restate(frames, nrow=L)
    ctx = restate(frames[:, :K_], nrow=L, total_slots=L)
    split = K_ * 66 + 1                                                 # the first column after the context's last tile
    for b in range(B):
        (got,) = _open_rgb(os.path.join(str(tmp_path), "Pred_%d_Step_5.png" % b))
        assert got.shape == (3 * 66 + 2, L * 66 + 2, 3)
        np.testing.assert_array_equal(got[:68], want_real[b], err_msg="row 0: the real clip")
        for s in range(n_samples):
            band = got[(1 + s) * 66:(2 + s) * 66 + 2]
            fut = restate(futures[s], nrow=L, total_slots=L, first_slot=K_, signed=False)[b]
            np.testing.assert_array_equal(band[:, :split], ctx[b][:, :split], err_msg=f"sample {s}: context")
            np.testing.assert_array_equal(band[:, split:], fut[:, split:], err_msg=f"sample {s}: future")

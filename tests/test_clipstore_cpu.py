"""Device-resident clip store (dvd_gan_amd.data.ClipStore / make_store_loader, kernel dvd_clip_gather), the part that needs no GPU:
the coefficient tables and the two integer passes against the installed Pillow, the store's tables on the F12 folder, the epoch
plan, and the refusals of the entry point before any launch.  The kernel itself: tests/test_gpu_clipstore.py."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch


def _materialise(g, root):
    for rel in [str(x) for x in g["meta.files"]]:
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(g["file." + rel].tobytes())


def _one_pass(a, out_size):
    """Resample axis 1 of uint8 [n, in, 3] to out_size samples: acc = 2^21 + sum pix * k, clamp(acc >> 22), rounded to uint8."""
    from dvd_gan_amd import data as D
    bounds, kk = D.resize_coeffs(a.shape[1], out_size)
    out = np.empty((a.shape[0], out_size, 3), dtype=np.uint8)
    for xx in range(out_size):
        lo, n = (int(v) for v in bounds[xx])
        acc = (1 << 21) + (a[:, lo:lo + n].astype(np.int64) * kk[xx, :n, None].astype(np.int64)).sum(1)
        assert acc.max() < 2 ** 31                                   # the kernel's accumulators are int32
        out[:, xx] = np.clip(acc >> 22, 0, 255)
    return out


def resize_restated(crop, size):
    """The device path's arithmetic in numpy: horizontal pass, rounded to uint8, then the vertical pass on those bytes."""
    h = _one_pass(crop, size)
    return _one_pass(np.ascontiguousarray(h.transpose(1, 0, 2)), size).transpose(1, 0, 2)


@pytest.mark.parametrize("hw", [(30, 40), (17, 23), (64, 64), (240, 320)])
def test_coefficient_builder_reproduces_pillow(hw):
    """data.resize_coeffs + the two integer passes == Image.crop(box).resize((S, S), BILINEAR) of the installed Pillow, bit for
    bit: S in {11, 16, 64}, the five training scales, float boxes as 'random' mode makes them (crop rounds half to even: boxes
    whose corners end in .5 are included), the corner / center boxes, down- and upscaling.  If a future Pillow changes its
    arithmetic, this fails first."""
    from PIL import Image
    from dvd_gan_amd import data as D
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img = Image.fromarray(frame)
    random.seed(H + W)
    n = 0
    for S in (11, 16, 64):
        for scale in D.default_scales():
            crop = D.MultiScaleCrop([scale], S, "random")
            side = int(min(W, H) * scale)
            draws = [(random.random(), random.random()) for _ in range(2)]
            # corners that end in .5: tl * (extent - side) = k + 0.5 for k even and odd (round half to even goes both ways)
            draws += [((k + 0.5) / (W - side), (k + 1.5) / (H - side)) for k in (0, 1, 2) if k + 1.5 < min(W, H) - side]
            for tl in draws:
                crop.randomize_parameters()
                crop.tl_x, crop.tl_y = tl
                x0, y0, cw, ch = D.crop_box(crop, W, H)
                assert abs(cw - side) <= 1 and abs(ch - side) <= 1
                want = np.asarray(crop(img))
                np.testing.assert_array_equal(resize_restated(frame[y0:y0 + ch, x0:x0 + cw], S), want, err_msg=str((S, scale, tl)))
                n += 1
            for mode in ("corner", "center"):
                crop = D.MultiScaleCrop([scale], S, mode)
                for pos in crop.positions:
                    crop.randomize_parameters()
                    crop.crop_position = pos
                    x0, y0, cw, ch = D.crop_box(crop, W, H)
                    np.testing.assert_array_equal(resize_restated(frame[y0:y0 + ch, x0:x0 + cw], S), np.asarray(crop(img)))
                    n += 1
    assert n >= 3 * 5 * 8


def test_half_coordinates_round_to_even():
    from dvd_gan_amd import data as D
    crop = D.MultiScaleCrop([0.5], 8, "random")
    crop.randomize_parameters()
    crop.tl_x, crop.tl_y = 0.5 / 25, 1.5 / 15                      # 40 x 30 frame, side 15: corners 0.5 and 1.5
    assert D.crop_box(crop, 40, 30) == (0, 2, 16, 14)               # 0.5 -> 0, 15.5 -> 16; 1.5 -> 2, 16.5 -> 16


def test_band_plan_fits_the_lds():
    """dvd_clip_gather_band_rows(ch, S) output rows per workgroup: the source rows any such band needs, read from the tables the
    kernel reads, fit the 64 KB the kernel's horizontal results may take -- at the sizes of the GPU test and at the limits."""
    from dvd_gan_amd import data as D
    from dvd_gan_amd import lib as L
    lib = L.lib()
    assert lib.dvd_clip_gather_band_rows(240, 64) == 64 and lib.dvd_clip_gather_band_rows(15, 16) == 16     # one band
    assert lib.dvd_clip_gather_band_rows(100, 256) == 208 and lib.dvd_clip_gather_band_rows(400, 256) == 51
    assert lib.dvd_clip_gather_band_rows(4096, 256) >= 1
    assert lib.dvd_clip_gather_band_rows(4097, 256) == 0 and lib.dvd_clip_gather_band_rows(64, 257) == 0
    for ch, S in ((100, 256), (400, 256), (4096, 256), (1080, 256), (1080, 64), (300, 12), (3, 256)):
        R = lib.dvd_clip_gather_band_rows(ch, S)
        bounds, _ = D.resize_coeffs(ch, S)
        assert (np.diff(bounds[:, 0]) >= 0).all()                   # the kernel takes a band's first row from its first output row
        for lo in range(0, S, R):
            hi = min(S, lo + R) - 1
            assert int(bounds[hi, 0] + bounds[hi, 1] - bounds[lo, 0]) <= 65536 // (3 * S), (ch, S, R, lo)


@pytest.fixture(scope="module")
def f12(golden, tmp_path_factory):
    from dvd_gan_amd import data as D
    root = str(tmp_path_factory.mktemp("f12"))
    _materialise(golden("f12_ucf101_reader"), root)
    ds = D.UCF101(os.path.join(root, "jpg"), os.path.join(root, "ucf101_01.json"), "training", n_frames=8, sample_size=16)
    return root, ds


def test_build_save_load_on_the_f12_folder(f12, tmp_path):
    from PIL import Image
    from dvd_gan_amd import data as D
    root, ds = f12
    store = D.ClipStore.build(ds)
    assert len(store) == 3 and store.record_label.tolist() == [0, 1, 1] and store.video_frames.tolist() == [14, 9, 5]
    assert store.record_video.tolist() == [0, 1, 2] and store.record_first.tolist() == [1, 1, 1]
    assert store.record_last.tolist() == [14, 9, 5]
    sizes = [h * w * 3 * n for h, w, n in zip(store.video_h.tolist(), store.video_w.tolist(), store.video_frames.tolist())]
    assert store.video_offset.tolist() == [0, sizes[0], sizes[0] + sizes[1]] and store.blob.numel() == sum(sizes)
    # the last frame of the second video, as the reader decodes it
    rec = ds.data[1]
    with Image.open(os.path.join(rec["video"], "image_{:05d}.jpg".format(9))) as img:
        want = np.asarray(img.convert("RGB"))
    h, w = want.shape[:2]
    at = int(store.video_offset[1]) + 8 * h * w * 3
    np.testing.assert_array_equal(store.blob[at:at + h * w * 3].numpy().reshape(h, w, 3), want)
    path = str(tmp_path / "store.pt")
    store.save(path)
    assert all(isinstance(v, torch.Tensor) for v in torch.load(path, weights_only=True).values())
    back = D.ClipStore.load(path, device="cpu")
    for k in D.ClipStore.FIELDS:
        assert getattr(back, k).dtype == getattr(store, k).dtype and torch.equal(getattr(back, k), getattr(store, k)), k
    with pytest.raises(RuntimeError, match="no CPU path"):          # a host blob is never gathered from: no fallback
        back.gather([0], [[1, 2]], [(0, 0, 8, 8)], [False], 8)
    # windows of one video share its frames; prescale stores the short side asked for
    many = D.UCF101(os.path.join(root, "jpg"), os.path.join(root, "ucf101_01.json"), "training", n_frames=4, sample_size=16,
                    n_samples_for_each_video=3, sample_duration=4)
    windows = D.ClipStore.build(many, prescale=12)
    assert len(windows) == len(many.data) > 3 and windows.video_frames.tolist() == [14, 9, 5]
    assert [(f, l) for f, l in zip(windows.record_first.tolist(), windows.record_last.tolist())] == \
        [(r["frame_indices"][0], r["frame_indices"][-1]) for r in many.data]
    assert all(min(h, w) == 12 for h, w in zip(windows.video_h.tolist(), windows.video_w.tolist()))


def test_build_refuses_a_video_with_a_missing_frame(golden, tmp_path):
    from dvd_gan_amd import data as D
    root = str(tmp_path)
    _materialise(golden("f12_ucf101_reader"), root)
    ds = D.UCF101(os.path.join(root, "jpg"), os.path.join(root, "ucf101_01.json"), "training", n_frames=8, sample_size=16)
    os.remove(os.path.join(ds.data[1]["video"], "image_00004.jpg"))
    with pytest.raises(FileNotFoundError, match="image_00004.jpg"):
        D.ClipStore.build(ds)


def _plain_store(n):
    from dvd_gan_amd import data as D
    z = torch.zeros(n, dtype=torch.int64)
    return D.ClipStore(blob=torch.zeros(n * 4 * 4 * 3, dtype=torch.uint8), video_offset=torch.arange(n) * 48,
                       video_h=torch.full((n,), 4, dtype=torch.int32), video_w=torch.full((n,), 4, dtype=torch.int32),
                       video_frames=torch.ones(n, dtype=torch.int32), record_video=torch.arange(n), record_label=z,
                       record_first=z + 1, record_last=z + 1)


def test_plan_epoch_orders():
    """shuffle=False: record order, the incomplete batch dropped; world=2: each rank's indices are DistributedSampler's for the
    same seed and epoch (make_loader's sampler), and set_epoch changes them; nothing touches a device."""
    from torch.utils.data.distributed import DistributedSampler
    from dvd_gan_amd import data as D
    store = _plain_store(11)
    plain = D.make_store_loader(store, 4, 2, 4, shuffle=False)
    assert len(plain) == 2 and plain.plan_epoch() == [[0, 1, 2, 3], [4, 5, 6, 7]]
    plans = {}
    for epoch in (0, 3):
        for rank in (0, 1):
            loader = D.make_store_loader(store, 2, 2, 4, shuffle=True, rank=rank, world=2, seed=5)
            loader.set_epoch(epoch)
            sampler = DistributedSampler(range(11), num_replicas=2, rank=rank, shuffle=True, seed=5, drop_last=True)
            sampler.set_epoch(epoch)
            want = list(sampler)
            got = loader.plan_epoch()
            assert len(loader) == len(got) == len(want) // 2 == 2
            assert [i for batch in got for i in batch] == want[:4]
            plans[epoch, rank] = want
    assert plans[0, 0] != plans[3, 0] and not set(plans[0, 0]) & set(plans[0, 1])
    torch.manual_seed(0)
    shuffled = D.make_store_loader(store, 2, 2, 4, shuffle=True).plan_epoch()
    assert len(shuffled) == 5 and len({i for batch in shuffled for i in batch}) == 10


def test_draws_follow_the_reader(f12):
    """StoreLoader.draw consumes Python's `random` exactly as UCF101.__getitem__ does: after the same records the two generators
    are in the same state, in every crop mode, also for windows shorter than n_frames (record 2 has 5 frames)."""
    from dvd_gan_amd import data as D
    root, _ = f12
    for mode in ("corner", "center", "random"):
        ds = D.UCF101(os.path.join(root, "jpg"), os.path.join(root, "ucf101_01.json"), "training", n_frames=8, sample_size=16,
                      train_crop=mode)
        loader = D.make_store_loader(D.ClipStore.build(ds), 3, 8, 16, train_crop=mode, shuffle=False)
        random.seed(11)
        flips = [bool(ds[i][1]) for i in range(3)]
        after_reader = random.random()
        random.seed(11)
        frames, boxes, got_flips, labels = loader.draw([0, 1, 2])
        assert random.random() == after_reader and got_flips == flips and labels == [0, 1, 1]
        assert all(len(f) == 8 for f in frames) and frames[2] == [1, 2, 3, 4, 5, 1, 2, 3]


def test_gather_refusals_need_no_gpu():
    """DVD_E_ARG (-1) / DVD_E_SHAPE (-2) of dvd_clip_gather, all before any launch: placeholder pointers, never dereferenced
    (only the host copy of the clip rows is read)."""
    from dvd_gan_amd import lib as L
    lib = L.lib()
    p, ll = C.c_void_p(1), C.c_longlong
    B, T, S = 2, 3, 16
    blob_bytes = 2 * 5 * 30 * 40 * 3                               # two videos of five 30 x 40 frames
    kx = 2 * 2 + 1                                                  # ksize of 25 -> 16: 2 * ceil(1.5625) + 1
    tab_ints = 2 * S * (2 + kx)

    def call(rows=None, frames=None, blob=p, dev=p, tab=p, dst=p, ms=p, B=B, T=T, S=S, norm=255.0, nbytes=blob_bytes,
             ints=tab_ints, host=True):
        #        off              h   w   n  x0 y0  cw  ch flip xtab ytab
        base = [[0,              30, 40, 5, 0, 0, 25, 25, 0, 0, S * (2 + kx)],
                [5 * 30 * 40 * 3, 30, 40, 5, 15, 5, 25, 25, 1, 0, S * (2 + kx)]]
        for b, col, v in rows or []:
            base[b][col] = v
        fr = frames or [[0, 1, 2], [4, 4, 0]]
        flat = torch.tensor([v for r in base for v in r] + [v for r in fr for v in r], dtype=torch.int64)
        return lib.dvd_clip_gather(blob, ll(nbytes), C.c_void_p(flat.data_ptr()) if host else None, dev, tab, ll(ints), dst, ll(B),
                                   T, S, C.c_float(norm), ms, None)

    for kw in (dict(blob=None), dict(dev=None), dict(tab=None), dict(dst=None), dict(ms=None), dict(host=False), dict(B=0),
               dict(T=0), dict(S=0), dict(norm=0.0), dict(nbytes=0), dict(ints=0)):
        assert call(**kw) == -1, kw
    bad_rows = {
        "box past the right edge": [(1, L.CLIP_X0, 16)], "box past the lower edge": [(0, L.CLIP_Y0, 6)],
        "negative corner": [(0, L.CLIP_X0, -1)], "empty box": [(0, L.CLIP_CW, 0)], "no frames": [(0, L.CLIP_FRAMES, 0)],
        "zero height": [(0, L.CLIP_H, 0)], "negative offset": [(0, L.CLIP_OFF, -1)],
        "video past the blob": [(1, L.CLIP_OFF, 5 * 30 * 40 * 3 + 1)], "more frames than stored": [(1, L.CLIP_FRAMES, 6)],
        "table past the pool": [(1, L.CLIP_YTAB, S * (2 + kx) + 1)], "negative table": [(0, L.CLIP_XTAB, -1)],
    }
    for why, rows in bad_rows.items():
        assert call(rows=rows) == -1, why
    assert call(frames=[[0, 1, 5], [0, 0, 0]]) == -1 and call(frames=[[0, 1, 2], [0, -1, 0]]) == -1
    # a wider box needs a longer table: 40 -> 16 has ksize 7, two more ints per output sample than the pool holds
    assert call(rows=[(0, L.CLIP_CW, 40), (0, L.CLIP_XTAB, S * (2 + kx))]) == -1
    assert call(S=L.CLIP_MAX_OUT + 1, ints=1 << 20) == -2
    assert call(rows=[(0, L.CLIP_W, L.CLIP_MAX_SIDE + 1)], nbytes=1 << 40) == -2
    assert call(B=1 << 30, T=3) == -2                               # B * T past 2^31 - 1 workgroups
    with pytest.raises(RuntimeError, match="bad argument"):
        L.check(call(rows=[(1, L.CLIP_X0, 16)]))

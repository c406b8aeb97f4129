"""Device-resident clip store on the GPU (data.ClipStore.gather -> dvd_clip_gather, data.make_store_loader): the kernel against
Pillow directly, against the reference's clips of fixture F12 (the yardstick tests/test_gpu_data.py holds the host reader to),
against the host loader batch by batch, and under Trainer.train().  Everything is bit-equal: Pillow's 8-bit bilinear resize is
integer arithmetic, and the normalisation is the three fp32 operations of dvd_clip_to_tensor."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _materialise(g, root):
    for rel in [str(x) for x in g["meta.files"]]:
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(g["file." + rel].tobytes())


def _store(videos, lead=0):
    """A ClipStore over synthetic videos (uint8 [n, h, w, 3] each), `lead` unused bytes in front of the first."""
    from dvd_gan_amd import data as D
    sizes = [v.size for v in videos]
    blob = np.concatenate([np.zeros(lead, np.uint8)] + [v.reshape(-1) for v in videos])
    n = len(videos)
    ids = torch.arange(n)
    return D.ClipStore(blob=torch.from_numpy(blob).to(DEV),
                       video_offset=torch.tensor([lead + sum(sizes[:i]) for i in range(n)], dtype=torch.int64),
                       video_h=torch.tensor([v.shape[1] for v in videos], dtype=torch.int32),
                       video_w=torch.tensor([v.shape[2] for v in videos], dtype=torch.int32),
                       video_frames=torch.tensor([v.shape[0] for v in videos], dtype=torch.int32),
                       record_video=ids, record_label=ids, record_first=torch.ones(n, dtype=torch.int64),
                       record_last=torch.tensor([v.shape[0] for v in videos], dtype=torch.int64))


def _pillow(videos, record_ids, frame_ids, boxes, flips, S):
    """What the host path gives: Image.crop(box).resize((S, S), BILINEAR) per frame, then flip / ToTensor / Normalize in fp32 with
    the kernel's three operations (numpy fp32 division and subtraction are the same IEEE operations)."""
    from PIL import Image
    out = np.empty((len(record_ids), 3, len(frame_ids[0]), S, S), dtype=np.float32)
    for b, (r, (x0, y0, cw, ch)) in enumerate(zip(record_ids, boxes)):
        for t, f in enumerate(frame_ids[b]):
            a = np.asarray(Image.fromarray(videos[r][f - 1]).crop((x0, y0, x0 + cw, y0 + ch)).resize((S, S), Image.BILINEAR))
            if flips[b]:
                a = a[:, ::-1]
            v = a.astype(np.float32).transpose(2, 0, 1)
            out[b, :, t] = (v / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
    return out


def _video(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# name -> (videos as (frames, h, w), S, boxes of the two clips (x0, y0, cw, ch), records of the two clips, leading bytes)
KERNEL_CASES = {
    "30x40->16 crop 30 and 25": ([(4, 30, 40)], 16, [(10, 0, 30, 30), (3, 5, 25, 25)], [0, 0], 0),
    "30x40->16 crop 21 and 17": ([(4, 30, 40)], 16, [(19, 9, 21, 21), (0, 13, 17, 17)], [0, 0], 0),
    "30x40->16 crop 15 (upscale) and 16x14": ([(4, 30, 40)], 16, [(12, 7, 15, 15), (0, 2, 16, 14)], [0, 0], 0),
    "17x23->11 cw = ch + 1": ([(3, 17, 23)], 11, [(2, 1, 13, 12), (9, 3, 14, 13)], [0, 0], 0),
    "boxes on the left/top and right/bottom edges": ([(3, 30, 40)], 16, [(0, 0, 21, 22), (19, 8, 21, 22)], [0, 0], 0),
    "64x64->64 full frame (identity)": ([(3, 64, 64)], 64, [(0, 0, 64, 64), (0, 0, 64, 64)], [0, 0], 0),
    "300x20->12 and 20x300->12 (ksize 51)": ([(3, 300, 20), (3, 20, 300)], 12, [(0, 0, 20, 300), (0, 0, 300, 20)], [0, 1], 0),
    "two videos of different size": ([(5, 30, 40), (3, 17, 23)], 16, [(4, 2, 25, 26), (1, 0, 17, 17)], [0, 1], 0),
    "odd byte offset": ([(3, 30, 40), (3, 17, 23)], 11, [(7, 3, 21, 21), (5, 1, 12, 13)], [0, 1], 7),
    # the band limit: a workgroup's horizontally resized source rows take at most 64 KB of LDS = 85 rows at S = 256 (the largest
    # served S, and the smallest shapes that cross it): 100 -> 256 runs in two bands of 208 output rows, 400 -> 256 in six of 51
    "100x90->256 (two bands, upscale)": ([(3, 100, 90)], 256, [(0, 0, 90, 100), (5, 10, 80, 86)], [0, 0], 0),
    "400x130->256 (six bands, downscale)": ([(3, 400, 130)], 256, [(0, 0, 130, 400), (1, 3, 128, 397)], [0, 0], 0),
}


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_reproduces_pillow(name):
    """B = 2, T = 3, the first clip flipped, the second not; fp32 output bit-equal to Pillow + the host normalisation."""
    shapes, S, boxes, records, lead = KERNEL_CASES[name]
    videos = [_video(17 * i + len(name), *s) for i, s in enumerate(shapes)]
    store = _store(videos, lead)
    frame_ids = [[videos[records[0]].shape[0], 1, 2], [2, 2, 3]]
    flips = [True, False]
    got = store.gather(records, frame_ids, boxes, flips, S)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 3, S, S)
    np.testing.assert_array_equal(got.cpu().numpy(), _pillow(videos, records, frame_ids, boxes, flips, S), err_msg=name)
    if "bands" in name:
        from dvd_gan_amd import lib as L
        assert min(L.lib().dvd_clip_gather_band_rows(b[3], S) for b in boxes) < S


def test_gather_refuses_what_the_kernel_would_not_serve():
    store = _store([_video(1, 2, 30, 40)])
    with pytest.raises(ValueError, match="not inside"):
        store.gather([0], [[1, 2]], [(20, 0, 21, 21)], [False], 16)
    with pytest.raises(RuntimeError, match="bad argument"):
        store.gather([0], [[1, 3]], [(0, 0, 21, 21)], [False], 16)          # frame 3 of a two-frame video
    with pytest.raises(RuntimeError, match="unsupported shape"):
        store.gather([0], [[1, 2]], [(0, 0, 21, 21)], [False], 257)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def f12(golden, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("f12"))
    _materialise(golden("f12_ucf101_reader"), root)
    return root


def _dataset(root, **kw):
    from dvd_gan_amd import data as D
    return D.UCF101(os.path.join(root, "jpg"), os.path.join(root, "ucf101_01.json"), "training", **kw)


def test_store_loader_reproduces_the_reference_clips(golden, f12, tmp_path):
    """Every case of F12 (mode.index.seed): random seeded with 100 * seed + index, the record's clip from make_store_loader's
    path == the reference's clip, like test_reader_reproduces_the_reference_clips asks of the host reader.  The store goes
    through save / load on the way."""
    from dvd_gan_amd import data as D
    g = golden("f12_ucf101_reader")
    D.ClipStore.build(_dataset(f12, n_frames=8, sample_size=16)).save(str(tmp_path / "store.pt"))
    store = D.ClipStore.load(str(tmp_path / "store.pt"), DEV)
    loaders = {m: D.make_store_loader(store, 1, 8, 16, train_crop=m, shuffle=False) for m in ("corner", "random", "center")}
    cases = [str(x) for x in g["meta.cases"]]
    assert cases
    for tag in cases:
        mode, index, seed = tag.split(".")
        random.seed(100 * int(seed) + int(index))
        clips, labels = loaders[mode].batch([int(index)])
        assert labels.tolist() == [int(g["out.label." + tag])]
        want = g["out.clip." + tag]
        assert tuple(clips.shape[1:]) == want.shape, (tag, clips.shape, want.shape)
        np.testing.assert_array_equal(clips[0].cpu().numpy(), want, err_msg=tag)


@pytest.mark.parametrize("mode", ["corner", "random"])
def test_store_loader_equals_the_host_loader(f12, mode):
    """F12 folder, n_frames = 8, sample_size = 16, shuffle = False, batch_size = 2, random.seed(0): make_store_loader and
    make_loader(num_workers=0) yield bit-equal clips and equal labels ('corner' is the issue's case; 'random' adds the float boxes)."""
    from dvd_gan_amd import data as D
    ds = _dataset(f12, n_frames=8, sample_size=16, train_crop=mode)
    random.seed(0)
    want = [(c.cpu(), l) for c, l in D.make_loader(ds, batch_size=2, num_workers=0, shuffle=False)]
    loader = D.make_store_loader(D.ClipStore.build(ds, device=DEV), 2, 8, 16, train_crop=mode, shuffle=False)
    random.seed(0)
    got = [(c.cpu(), l) for c, l in loader]
    assert len(loader) == len(got) == len(want) == 1
    for (gc, gl), (wc, wl) in zip(got, want):
        assert gc.dtype == wc.dtype == torch.float32 and tuple(gc.shape) == tuple(wc.shape) == (2, 3, 8, 16, 16)
        np.testing.assert_array_equal(gc.numpy(), wc.numpy())
        assert gl.dtype == wl.dtype and gl.tolist() == wl.tolist() == [0, 1]


def test_trainer_train_loop_on_the_store_loader(f12, tmp_path):
    """Trainer.train() takes the store loader unchanged: two steps with the config of test_trainer_train_loop_on_the_reader
    (64 x 64, T = 8, ch = 2, fp32); parameters move, everything stays finite."""
    import argparse
    from dvd_gan_amd import data as D
    from dvd_gan_amd.train_step import Trainer
    store = D.ClipStore.build(_dataset(f12, n_frames=8, sample_size=64), device=DEV)
    random.seed(4)
    torch.manual_seed(4)
    loader = D.make_store_loader(store, batch_size=2, n_frames=8, sample_size=64, shuffle=False)
    assert len(loader) == 1
    cfg = argparse.Namespace(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const",
                             total_epoch=2, d_iters=1, batch_size=2, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9,
                             n_class=2, k_sample=4, model_save_path=str(tmp_path / "models"), version="t", model_save_epoch=2,
                             log_epoch=1)
    tr = Trainer(loader, cfg, device=DEV, compute_dtype=torch.float32)
    before = {k: v.detach().clone() for k, v in tr.G.state_dict().items()}
    tr.train()                                                  # 2 epochs x 1 step
    torch.cuda.synchronize()
    after = tr.G.state_dict()
    moved = [k for k in before if before[k].is_floating_point() and not torch.equal(before[k], after[k])]
    assert "conv.0.cells.0.update_gate.weight" in moved and "colorize.module.weight_u" in moved
    for net in (tr.G, tr.D_s, tr.D_t):
        assert all(torch.isfinite(v).all() for v in net.state_dict().values() if v.is_floating_point())

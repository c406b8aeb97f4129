"""Sample sheets (dvd_gan_amd.sheets, kernel dvd_sample_sheet), the part that needs no GPU: the restatement the GPU tests compare
the kernel with (checked here against Pillow's paste), the PNG / APNG writers (decoded by Pillow, every CRC walked), the writer
thread on host tensors, the geometry query, every refusal of the C entry point, and Trainer.fixed_inputs.  The bare config of that
last part also serves the two tests of the Trainer's settings table (settings.py) and of its no-trace block (`_g_eval`)."""
import argparse
import binascii
import ctypes as C
import os
import struct
import threading

import numpy as np
import pytest
import torch

from dvd_gan_amd import sheets as S


# ------------------------------------------------------------------ the restatement (geometry + quantisation of the header)
def quantise(x, signed):
    """fp32 tensor -> uint8, every operation rounded on its own: helpers.denorm, then torchvision's save_image.  NaN -> 0."""
    x = x.to(torch.float32)
    if signed:
        x = x.add(1).div(2)
    x = torch.nan_to_num(x, nan=0.0, posinf=float("inf"), neginf=-float("inf"))         # NaN is DEFINED as 0 (torch leaves it open)
    return x.clamp_(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def geometry(total_slots, H, W, nrow, padding):
    xmaps = min(nrow, total_slots)
    ymaps = -(-total_slots // xmaps)
    return xmaps, ymaps, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def restate(tiles, *, nrow=8, padding=2, pad_value=0.0, signed=True, first_slot=0, total_slots=None, fill=True, base=None):
    """tiles: host fp32 [n_sheets, n_tiles, 3, H, W] -> uint8 numpy [n_sheets, Hs, Ws, 3].  fill=False starts from `base`."""
    tiles = torch.as_tensor(tiles)
    n_sheets, n_tiles, _, H, W = tiles.shape
    total_slots = first_slot + n_tiles if total_slots is None else total_slots
    xmaps, _, Hs, Ws = geometry(total_slots, H, W, nrow, padding)
    if fill:
        pad = int(quantise(torch.tensor([pad_value]), False)[0])
        out = np.full((n_sheets, Hs, Ws, 3), pad, dtype=np.uint8)
    else:
        out = np.array(base, dtype=np.uint8).reshape(n_sheets, Hs, Ws, 3).copy()
    q = quantise(tiles, signed).numpy()
    for k in range(n_tiles):
        slot = first_slot + k
        y0, x0 = (slot // xmaps) * (H + padding) + padding, (slot % xmaps) * (W + padding) + padding
        out[:, y0:y0 + H, x0:x0 + W, :] = q[:, k].transpose(0, 2, 3, 1)
    return out


def prefixed(sheets):
    """[..., Hs, Ws, 3] -> [..., Hs, 1 + 3 Ws] with PNG's filter byte 0 in front of every row."""
    sheets = np.asarray(sheets)
    rows = sheets.reshape(sheets.shape[:-2] + (-1,))
    return np.concatenate([np.zeros(rows.shape[:-1] + (1,), np.uint8), rows], axis=-1)


@pytest.mark.parametrize("padding", [0, 2])
@pytest.mark.parametrize("pad_value", [0.0, 0.5, 1.0])
def test_restatement_equals_pillow_paste_of_torch_quantised_tiles(padding, pad_value):
    from PIL import Image
    n, nrow, H, W = 5, 2, 6, 10
    tiles = torch.randn(1, n, 3, H, W, generator=torch.Generator().manual_seed(3)) * 0.8
    got = restate(tiles, nrow=nrow, padding=padding, pad_value=pad_value)[0]
    Hs, Ws = 3 * (H + padding) + padding, 2 * (W + padding) + padding
    p = int(torch.tensor([pad_value]).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)[0])
    canvas = Image.new("RGB", (Ws, Hs), (p, p, p))
    for k in range(n):
        x = tiles[0, k]
        q = x.add(1).div(2).clamp_(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
        tile = Image.fromarray(q.permute(1, 2, 0).contiguous().numpy(), "RGB")
        canvas.paste(tile, ((k % nrow) * (W + padding) + padding, (k // nrow) * (H + padding) + padding))
    want = np.asarray(canvas)
    assert got.shape == want.shape == (Hs, Ws, 3)
    np.testing.assert_array_equal(got, want)
    if padding:
        assert (got[-(H + padding):-padding, -(W + padding):-padding] == p).all()          # the empty sixth slot


def test_restatement_defines_nan_and_infinities():
    x = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 0.0, 1e-42, -1e-42, 1.0, -1.0, 7.0, -7.0])
    assert quantise(x, True).tolist() == [0, 255, 0, 128, 128, 128, 128, 255, 0, 255, 0]
    assert quantise(x, False).tolist() == [0, 255, 0, 0, 0, 0, 0, 255, 0, 255, 0]


# ------------------------------------------------------------------ writers
def walk_chunks(path):
    """[(tag, data)] of a PNG file; asserts the signature and every chunk's CRC."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])
        assert crc == binascii.crc32(tag + data) & 0xffffffff, tag
        out.append((tag, data))
        pos += 12 + n
    assert pos == len(raw) and out[-1] == (b"IEND", b"")
    return out


def _random_sheet(seed, Hs, Ws, n=None):
    shape = (Hs, Ws, 3) if n is None else (n, Hs, Ws, 3)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("Hs,Ws", [(7, 5), (1, 1), (26, 26), (5, 33)])
def test_write_png_decodes_to_the_sheet_from_both_forms(tmp_path, Hs, Ws):
    from PIL import Image
    sheet = _random_sheet(Hs * 100 + Ws, Hs, Ws)
    for tag, form in (("plain", sheet), ("prefixed", prefixed(sheet)), ("tensor", torch.from_numpy(prefixed(sheet)))):
        path = str(tmp_path / f"{tag}.png")
        S.write_png(path, form)
        with Image.open(path) as im:
            assert im.format == "PNG" and im.mode == "RGB" and im.size == (Ws, Hs)
            np.testing.assert_array_equal(np.asarray(im), sheet, err_msg=tag)
        chunks = walk_chunks(path)
        assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        assert chunks[0][1] == struct.pack(">IIBBBBB", Ws, Hs, 8, 2, 0, 0, 0)
    assert open(str(tmp_path / "plain.png"), "rb").read() == open(str(tmp_path / "prefixed.png"), "rb").read()


def test_write_png_refuses_what_is_no_sheet(tmp_path):
    path = str(tmp_path / "x.png")
    with pytest.raises(ValueError, match=r"\(4, 5, 4\)"):
        S.write_png(path, np.zeros((4, 5, 4), np.uint8))
    with pytest.raises(ValueError, match=r"\(4, 15\)"):
        S.write_png(path, np.zeros((4, 15), np.uint8))                    # 15 - 1 is no multiple of 3
    with pytest.raises(ValueError, match="uint8"):
        S.write_png(path, np.zeros((4, 5, 3), np.float32))
    bad = prefixed(_random_sheet(0, 4, 5))
    bad[2, 0] = 1
    with pytest.raises(ValueError, match="filter"):
        S.write_png(path, bad)
    assert not os.path.exists(path)


@pytest.mark.parametrize("form", ["plain", "prefixed"])
@pytest.mark.parametrize("n,fps,loops", [(1, 8, 0), (4, 8, 0), (3, 25, 2), (2, 12.5, 1)])
def test_write_apng_frames_timing_and_chunk_order(tmp_path, form, n, fps, loops):
    from PIL import Image
    Hs, Ws = 7, 5
    frames = _random_sheet(n, Hs, Ws, n)
    path = str(tmp_path / "a.apng")
    S.write_apng(path, frames if form == "plain" else prefixed(frames), fps, loops)
    with Image.open(path) as im:
        assert im.size == (Ws, Hs) and getattr(im, "n_frames", 1) == n
        if n > 1:
            assert im.info["loop"] == loops
        for i in range(n):
            im.seek(i)
            np.testing.assert_array_equal(np.asarray(im.convert("RGB")), frames[i], err_msg=f"frame {i}")
            if n > 1:
                assert im.info["duration"] == pytest.approx(1000.0 / fps)
    chunks = walk_chunks(path)
    tags = [t for t, _ in chunks]
    assert tags == [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n - 1) + [b"IEND"]
    assert chunks[1][1] == struct.pack(">II", n, loops)
    seq = [struct.unpack(">I", d[:4])[0] for t, d in chunks if t in (b"fcTL", b"fdAT")]
    assert seq == list(range(2 * n - 1))                                    # one numbering over fcTL and fdAT, in file order
    for t, d in chunks:
        if t == b"fcTL":
            _, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", d)
            assert (w, h, x, y, dispose, blend) == (Ws, Hs, 0, 0, 0, 0) and num / den == 1.0 / fps


def test_write_apng_refusals(tmp_path):
    path = str(tmp_path / "a.apng")
    with pytest.raises(ValueError, match="at least one"):
        S.write_apng(path, [], 8)
    with pytest.raises(ValueError, match="one size"):
        S.write_apng(path, [_random_sheet(0, 4, 5), _random_sheet(0, 5, 4)], 8)
    for fps in (0, -1):
        with pytest.raises(ValueError, match="fps"):
            S.write_apng(path, _random_sheet(0, 4, 5, 2), fps)


# ------------------------------------------------------------------ the writer thread, on host tensors
def test_sheet_writer_writes_in_order_and_holds_back_at_max_pending(tmp_path, monkeypatch):
    from PIL import Image
    gate, order, real_write = threading.Event(), [], S.write_png

    def gated(path, sheet, level=S.LEVEL):
        gate.wait(30)
        order.append(os.path.basename(path))
        real_write(path, sheet, level)

    monkeypatch.setattr(S, "write_png", gated)
    sheets = [torch.from_numpy(_random_sheet(i, 6, 4)) for i in range(3)]
    w = S.SheetWriter(max_pending=2)
    w.submit("png", str(tmp_path / "0.png"), sheets[0])
    w.submit("png", str(tmp_path / "1.png"), sheets[1])               # two outstanding: both calls came back
    third = threading.Event()

    def late():
        w.submit("png", str(tmp_path / "2.png"), sheets[2])
        third.set()

    t = threading.Thread(target=late)
    t.start()
    assert not third.wait(0.05) and order == []                         # the third waits for room
    sheets[0].zero_()                                                   # the job owns a copy of the bytes
    gate.set()
    assert third.wait(30)
    t.join()
    w.flush()
    assert order == ["0.png", "1.png", "2.png"]
    for i in range(3):
        with Image.open(str(tmp_path / f"{i}.png")) as im:
            np.testing.assert_array_equal(np.asarray(im), _random_sheet(i, 6, 4))
    w.close()
    w.close()                                                           # idempotent
    with pytest.raises(RuntimeError, match="closed"):
        w.submit("png", str(tmp_path / "3.png"), sheets[1])


def test_sheet_writer_batches_animations_and_errors(tmp_path):
    from PIL import Image
    stack = torch.from_numpy(prefixed(_random_sheet(5, 6, 4, 3)))
    with S.SheetWriter(max_pending=2) as w:
        w.submit("png", [str(tmp_path / f"b{i}.png") for i in range(3)], stack)
        w.submit("apng", str(tmp_path / "a.apng"), stack, fps=4, loops=3)
        w.flush()
        with Image.open(str(tmp_path / "a.apng")) as im:
            assert im.n_frames == 3 and im.info["loop"] == 3 and im.info["duration"] == 250.0
        for i in range(3):
            with Image.open(str(tmp_path / f"b{i}.png")) as im:
                np.testing.assert_array_equal(np.asarray(im), _random_sheet(5, 6, 4, 3)[i])
        # an unwritable path surfaces at flush(), once; the writer lives on
        w.submit("png", str(tmp_path / "no" / "such" / "dir.png"), stack[0])
        w.submit("png", str(tmp_path / "after.png"), stack[0])
        with pytest.raises(OSError):
            w.flush()
        w.flush()
        assert os.path.exists(str(tmp_path / "after.png"))
        with pytest.raises(ValueError, match="kind"):
            w.submit("gif", str(tmp_path / "x.gif"), stack)
        with pytest.raises(ValueError, match="2 file names for 3 sheets"):
            w.submit("png", ["a", "b"], stack)
        with pytest.raises(ValueError, match="fps"):
            w.submit("apng", str(tmp_path / "x.apng"), stack)
        with pytest.raises(ValueError, match="uint8"):
            w.submit("png", str(tmp_path / "x.png"), stack[0].float())
    assert w._closed and not w._thread.is_alive()
    with pytest.raises(ValueError, match="max_pending"):
        S.SheetWriter(max_pending=0)


# ------------------------------------------------------------------ the C entry points, without a GPU
SHAPES = [  # (total_slots, H, W, nrow, padding, row_prefix) -> (Hs, Ws, bytes of one sheet)
    ((48, 64, 64, 8, 2, 0), (398, 530, 632820)),
    ((48, 64, 64, 8, 2, 1), (398, 530, 633218)),
    ((808, 64, 64, 8, 2, 1), (6668, 530, 10608788)),
    ((5, 6, 10, 2, 2, 0), (26, 26, 2028)),
    ((5, 6, 10, 2, 0, 0), (18, 20, 1080)),
    ((1, 1, 1, 8, 2, 1), (5, 5, 80)),               # a single tile keeps its border
    ((9, 5, 3, 8, 1, 1), (13, 33, 1300)),
    ((3, 4, 4, 1, 0, 0), (12, 4, 144)),
    ((4, 4096, 4096, 2, 0, 0), (8192, 8192, 8192 * 8192 * 3)),
]


def _lib():
    from dvd_gan_amd import lib as L
    return L.lib()


def test_abi_version_and_symbols():
    from dvd_gan_amd import lib as L
    lib = _lib()
    assert lib.dvd_abi_version() == 13 == L.ABI_VERSION
    for name in ("dvd_sample_sheet_shape", "dvd_sample_sheet"):
        assert hasattr(lib, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvdgan_hip.h")).read()
    assert "int dvd_sample_sheet(" in header and "int dvd_sample_sheet_shape(" in header
    from dvd_gan_amd import kern as K
    assert f"#define DVD_SHEET_FILL {K.SHEET_FILL}\n" in header and f"#define DVD_SHEET_SIGNED {K.SHEET_SIGNED}\n" in header


@pytest.mark.parametrize("args,want", SHAPES)
def test_sheet_shape_values(args, want):
    from dvd_gan_amd import kern as K
    assert K.sample_sheet_shape(*args) == want
    assert S.sheet_shape(args[0], args[1], args[2], args[3], args[4]) == want[:2]
    assert geometry(*args[:5])[2:] == want[:2]                         # the restatement's geometry is the library's


def test_sheet_shape_refusals():
    lib = _lib()
    hs, ws, nb = C.c_int(-7), C.c_int(-7), C.c_longlong(-7)

    def q(total=5, H=6, W=10, nrow=2, padding=2, prefix=0, out=(hs, ws, nb)):
        return lib.dvd_sample_sheet_shape(total, H, W, nrow, padding, prefix, *(C.byref(o) if o is not None else None for o in out))

    assert q() == 0 and (hs.value, ws.value, nb.value) == (26, 26, 2028)
    ARG, SHAPE = -1, -2
    assert q(total=0) == ARG and q(nrow=0) == ARG and q(padding=-1) == ARG and q(padding=65) == ARG and q(prefix=2) == ARG
    assert q(out=(None, ws, nb)) == ARG and q(out=(hs, None, nb)) == ARG and q(out=(hs, ws, None)) == ARG
    assert q(H=0) == SHAPE and q(W=0) == SHAPE and q(H=4097) == SHAPE and q(W=4097) == SHAPE
    assert q(padding=64) == 0 and q(H=4096, W=4096, total=1, padding=0) == 0
    assert q(total=4, H=4096, W=16, nrow=1) == SHAPE                    # Hs = 4 * 4098 + 2
    assert q(total=4, H=16, W=4096, nrow=4) == SHAPE                    # Ws likewise
    assert q(total=2 ** 31 - 1, H=1, W=1, nrow=2 ** 31 - 1, padding=0) == SHAPE
    with pytest.raises(ValueError, match="4097"):
        S.sheet_shape(5, 4097, 10)


def test_sample_sheet_refuses_before_any_launch():
    """DVD_E_ARG (-1) / DVD_E_SHAPE (-2) of dvd_sample_sheet: placeholder pointers, never dereferenced (no GPU here: a launch
    would be DVD_E_LAUNCH, -3)."""
    lib = _lib()
    ll, ARG, SHAPE = C.c_longlong, -1, -2
    src, dst = C.c_void_p(0x1000), C.c_void_p(0x2000)

    def run(src=src, ss=5 * 180, st=180, sc=60, n_sheets=2, n_tiles=5, H=6, W=10, first=0, total=5, nrow=2, padding=2, pad=0.0,
            prefix=1, flags=3, dst=dst):
        return lib.dvd_sample_sheet(src, ll(ss), ll(st), ll(sc), ll(n_sheets), n_tiles, H, W, first, total, nrow, padding,
                                    C.c_float(pad), prefix, flags, dst, None)

    for kw in (dict(src=None), dict(dst=None), dict(n_sheets=0), dict(n_tiles=0), dict(first=-1), dict(total=4),
               dict(first=1), dict(first=3, total=7), dict(nrow=0), dict(padding=-1), dict(padding=65), dict(prefix=2),
               dict(prefix=-1), dict(flags=4), dict(flags=-1), dict(sc=59), dict(sc=0), dict(ss=-1), dict(st=-1)):
        assert run(**kw) == ARG, kw
    big = 2 ** 62
    for kw in (dict(H=0), dict(W=0), dict(H=4097, sc=4097 * 10), dict(W=4097, sc=6 * 4097),
               dict(total=8, nrow=1, H=4096, W=4, sc=4096 * 4),                         # Hs above 16384
               dict(total=8, nrow=8, H=4, W=4096, sc=4096 * 4),                         # Ws above 16384
               dict(ss=big), dict(st=big), dict(sc=big),                                # offsets leave 63 bits
               dict(ss=2 ** 61, n_sheets=3), dict(sc=2 ** 60),                          # ... as BYTE offsets
               dict(n_sheets=2 ** 31, ss=0),                                            # more rows than a grid has blocks
               dict(n_sheets=2 ** 62, ss=0)):                                           # more bytes than 63 bits count
        assert run(**kw) == SHAPE, kw


def test_make_sheets_refusals_name_the_shape():
    a = torch.zeros(2, 4, 3, 6, 10)
    with pytest.raises(ValueError, match="no CPU path"):
        S.make_sheets(a)
    with pytest.raises(ValueError, match=r"\(2, 4, 1, 6, 10\)"):
        S.make_sheets(a[:, :, :1])
    with pytest.raises(ValueError, match="fp32"):
        S.make_sheets(a.double())
    with pytest.raises(ValueError, match="contiguous"):
        S.make_sheets(a[..., :8])
    with pytest.raises(ValueError, match="layout"):
        S.make_sheets(a, layout="grid")
    with pytest.raises(ValueError, match="overlap"):
        S.make_sheets(a[:, :, :1].expand(2, 4, 3, 6, 10))
    with pytest.raises(ValueError, match="do not fit 5 slots"):
        S.make_sheets(a, first_slot=2, total_slots=5)


# ------------------------------------------------------------------ Trainer.fixed_inputs
def _cfg(**extra):
    return argparse.Namespace(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=2, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9,
                              n_class=3, k_sample=4, **extra)


def test_fixed_inputs_are_the_references_labels_and_leave_the_default_generator_alone():
    from dvd_gan_amd.train_step import Trainer
    tr = Trainer([], _cfg(test_batch_size=4, sample_seed=11), device=torch.device("cpu"), compute_dtype=torch.float32)
    assert tr.sample_step == 0 and tr._sheets is None and tr._fixed is None           # off: nothing was set up
    torch.manual_seed(5)
    before = torch.get_rng_state()
    z, label = tr.fixed_inputs()
    assert torch.equal(torch.get_rng_state(), before)
    n_class, tbs = 3, 4
    assert label.tolist() == [i for i in range(n_class) for j in range(tbs)] and label.dtype == torch.int64
    assert tuple(z.shape) == (n_class * tbs, 16) and z.dtype == torch.float32
    assert torch.equal(z, torch.randn(n_class * tbs, 16, generator=torch.Generator().manual_seed(11)))
    z2, label2 = tr.fixed_inputs()
    assert z2 is z and label2 is label                                                # drawn once
    other = Trainer([], _cfg(test_batch_size=4, sample_seed=12), device=torch.device("cpu"), compute_dtype=torch.float32)
    assert not torch.equal(other.fixed_inputs()[0], z)
    assert Trainer._class_and_number(label) == [(i, j) for i in range(n_class) for j in range(tbs)]
    assert Trainer([], _cfg(), device=torch.device("cpu"), compute_dtype=torch.float32).test_batch_size == 8


def test_trainer_sample_configuration_is_checked():
    from dvd_gan_amd.train_step import Trainer
    for bad in (dict(sample_step=-1), dict(test_batch_size=0), dict(sample_layout="grid"), dict(sample_fps=0)):
        with pytest.raises(ValueError, match="sample_layout"):
            Trainer([], _cfg(**bad), device=torch.device("cpu"), compute_dtype=torch.float32)
    tr = Trainer([], _cfg(sample_path="/s", version="v7", sample_epoch=2), device=torch.device("cpu"), compute_dtype=torch.float32)
    assert tr.sample_path == os.path.join("/s", "v7") and tr.sample_epoch == 2 and tr.sample_layout == "frames"


# ------------------------------------------------------------------ Trainer on the CPU: the settings table and the no-trace block
def _cpu_trainer(**extra):
    from dvd_gan_amd.train_step import Trainer
    return Trainer([], _cfg(**extra), device=torch.device("cpu"), compute_dtype=torch.float32)


# a second valid value for every row's config field (resume and pretrained_model exclude one another: two Trainers)
SECOND = dict(n_cond=4, g_self_attn=True, g_sep_attn=True, ema_decay=0.5, ema_start=3, ema_standing_stats=2, ema_stats_seed=9,
              g_ortho=1e-3, g_clip_norm=2.0, d_clip_norm=3.0, skip_nonfinite=True, grad_log=5, lecam=0.25, lecam_decay=0.5,
              lecam_start=2, g_topk=0.5, g_topk_decay=0.75, d_stats=True, d_aug="cutout,color", d_aug_geom="rotate,xflip",
              d_aug_p=0.25, d_aug_target=0.5, d_aug_interval=2, d_aug_kimg=100, d_aug_seed=4, sv_log=7, sv_iters=2, sv_log_rows=16,
              sv_k=2, sv_block=4, sv_seed=5, lr_decay=0.5, model_save_epoch=3, log_epoch=0, state_save_step=10, state_keep=3,
              sample_step=20, sample_epoch=2, test_batch_size=4, sample_layout="both", sample_fps=12, sample_use_ema=True,
              sample_seed=6)


def test_settings_table_gives_the_constructor_and_the_class_their_defaults(tmp_path):
    from dvd_gan_amd import settings as S
    from dvd_gan_amd.train_step import Trainer
    fields = [row[1] for row in S.SETTINGS]
    assert len(set(fields)) == len(fields) == len({row[0] for row in S.SETTINGS})
    assert ("_d_stats_on", "d_stats") in [row[:2] for row in S.SETTINGS]
    assert set(SECOND) | {"resume", "pretrained_model"} == set(fields)                 # every row is exercised below
    tr, bare = _cpu_trainer(), Trainer.__new__(Trainer)
    for attr, field, cast, default in S.SETTINGS:
        want = cast(default)
        assert getattr(tr, attr) == want and type(getattr(tr, attr)) is type(want), attr
        assert getattr(Trainer, attr) == want and type(getattr(Trainer, attr)) is type(want), attr
        assert getattr(bare, attr) == want, attr                                       # a Trainer that never ran __init__
    assert S.DEFAULTS == {attr: getattr(Trainer, attr) for attr, *_ in S.SETTINGS}
    assert tr.d_aug == () and tr.d_aug_geom == () and tr.resume is None and tr.sample_epoch == 0 and tr.d_aug_p == 1.0
    for name, want in (("_adv_ex", False), ("_adv_stats", None), ("_anchors", None), ("_ema_block", False), ("_epoch", 0),
                       ("_labels_registered", None), ("_sheets", None), ("_state_writer", None), ("g_optimizer", None)):
        assert getattr(bare, name) is want or getattr(bare, name) == want, name        # the run state that used to be guarded
    # a second valid value of every field reaches its attribute, through the row's cast
    other = _cpu_trainer(model_save_path=str(tmp_path), version="", **SECOND)
    by_field = {row[1]: row for row in S.SETTINGS}
    for field, value in SECOND.items():
        attr, _, cast, default = by_field[field]
        assert getattr(other, attr) == cast(value) != cast(default), field
    assert other.d_aug == ("color", "cutout") and other.d_aug_geom == ("xflip", "rotate") and other._d_stats_on is True
    assert other.fingerprint()["g_self_attn"] is True and hasattr(other.G, "self_attn") and hasattr(other.G, "sep_attn")
    other.save_models(5)                                                               # pretrained_model needs its files
    loaded = _cpu_trainer(model_save_path=str(tmp_path), version="", pretrained_model=5, **SECOND)
    assert loaded.pretrained_model == 5
    assert all(torch.equal(a, b) for a, b in zip(loaded.G.state_dict().values(), other.G.state_dict().values()))
    assert _cpu_trainer(resume="latest").resume == "latest" and _cpu_trainer(resume="").resume is None
    assert getattr(Trainer, "d_aug_p") == 1.0 and other.d_aug_p == 0.25                # the class keeps the table's default


@pytest.mark.parametrize("restore", [True, False])
def test_no_trace_block_puts_the_generators_frozen_tensors_back(restore):
    tr = _cpu_trainer()
    G = tr.G
    u = next(p.data for n, p in G.named_parameters() if n.endswith("weight_u"))
    mean = next(b for n, b in G.named_buffers() if n.endswith("running_mean"))
    count = next(b for n, b in G.named_buffers() if n.endswith("num_batches_tracked"))
    assert not next(p for n, p in G.named_parameters() if n.endswith("weight_u")).requires_grad
    mean.copy_(torch.randn(mean.shape))
    count.fill_(3)
    watched = (u, mean, count)
    before = [t.clone() for t in watched]
    everything = [t.clone() for t in tr._g_frozen_tensors()]

    def overwrite():
        u.add_(1.5)
        mean.mul_(2.0).add_(1.0)
        count.add_(4)
        assert not any(torch.equal(t, old) for t, old in zip(watched, before))

    class Boom(Exception):
        pass

    assert G.training
    with pytest.raises(Boom):
        with tr._g_eval(restore=restore) as put_back:
            assert not G.training
            overwrite()
            dirty = [t.clone() for t in watched]
            put_back()
            for t, old, d in zip(watched, before, dirty):
                assert torch.equal(t, old if restore else d)
            if restore:
                overwrite()
            raise Boom()
    assert G.training                                                                  # back in train mode either way
    if restore:
        assert all(torch.equal(t, old) for t, old in zip(watched, before))
        assert all(torch.equal(t, old) for t, old in zip(tr._g_frozen_tensors(), everything))
    else:
        assert all(torch.equal(t, d) for t, d in zip(watched, dirty))                  # quirk 2: what the passes left stays

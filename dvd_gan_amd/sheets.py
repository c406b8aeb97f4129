"""Sample sheets and animations of generated clips: the output side of a training run (trainer.py:323-334's
save_image(denorm(clip)), i.e. torchvision's make_grid over the frames of one clip, written as a PNG).

make_sheets turns device fp32 frames into 8-bit RGB sheets in one kernel launch (csrc/sheet.hip, dvd_sample_sheet): denormalise,
quantise, tile with borders, planar -> interleaved, optionally already in PNG scanline form.  write_png / write_apng are the file
writers (standard library only: zlib, struct, binascii), SheetWriter moves the deflate and the file system off the training loop:
the bytes travel through pinned memory behind an event and one worker thread compresses and writes.

Geometry is make_grid(nrow, padding, pad_value) with one deliberate deviation: a single tile keeps its border (torchvision returns
a lone image bare).  GIF / MP4 and tensorboard stay out."""
import binascii
import queue
import struct
import threading
import zlib
from fractions import Fraction

import numpy as np
import torch

from . import kern as K
from .metrics import _batch_strides

_PNG_SIG = b"\x89PNG\r\n\x1a\n"
LEVEL = 6                       # zlib's default


def sheet_shape(n_tiles, H, W, nrow=8, padding=2):
    """-> (Hs, Ws) of a sheet of n_tiles tiles of H x W (dvd_sample_sheet_shape: the geometry is stated once, in the library)."""
    return K.sample_sheet_shape(n_tiles, H, W, nrow, padding)[:2]


def make_sheets(frames, *, layout="frames", nrow=8, padding=2, pad_value=0.0, signed=True, row_prefix=False, out=None,
                first_slot=0, total_slots=None, fill=True):
    """frames: device fp32 tensor or view [..., T, 3, H, W] with contiguous H x W planes (any other strides: the generator's
    [B, T, 3, H, W], a time slice of it, and `clips.permute(0, 2, 1, 3, 4)` of a loader clip are all served without a copy); the
    leading axes fold into one batch axis B.
    layout="frames": one sheet per clip, its tiles are the T frames (the reference's sheet) -> B sheets.
    layout="clips": one sheet per time step, its tiles are the B clips -> T sheets, the frames of an animation.
    signed: the values are in [-1, 1] and go through helpers.denorm first; otherwise they are taken as [0, 1].  Then torchvision's
    save_image quantisation: clamp(x * 255 + 0.5, 0, 255) truncated.  NaN -> 0.
    The tiles fill slots [first_slot, first_slot + n_tiles) of sheets laid out for total_slots (default: just these tiles).
    fill=True also writes borders and every other slot with pad_value; fill=False writes the tiles' own pixels only, into `out`:
    several calls on one stream compose a sheet from several sources.
    -> device uint8 [n_sheets, Hs, Ws, 3], or with row_prefix=True [n_sheets, Hs, 1 + 3 Ws]: every row led by PNG's filter byte
    0, what write_png / write_apng deflate as it stands.  out: a contiguous uint8 device tensor of that size to fill.
    No host sync, no CPU path."""
    if layout not in ("frames", "clips"):
        raise ValueError(f"layout={layout!r}: 'frames' (a sheet per clip) or 'clips' (a sheet per time step)")
    if frames.dim() < 4 or frames.shape[-3] != 3:
        raise ValueError(f"frames {tuple(frames.shape)} must be [..., T, 3, H, W]")
    if frames.dtype != torch.float32:
        raise ValueError(f"sheets take fp32 frames, got {frames.dtype} {tuple(frames.shape)}")
    T, _, H, W = frames.shape[-4:]
    B, sb = _batch_strides(frames, "frames")
    st, sc = frames.stride(-4), frames.stride(-3)
    if sc < H * W:
        raise ValueError(f"frames {tuple(frames.shape)}: channel stride {sc} is below H * W = {H * W} (planes overlap)")
    n_sheets, n_tiles, ss, s_tile = (B, T, sb, st) if layout == "frames" else (T, B, st, sb)
    first_slot = int(first_slot)
    total_slots = first_slot + n_tiles if total_slots is None else int(total_slots)
    if n_tiles < 1 or first_slot < 0 or first_slot + n_tiles > total_slots:
        raise ValueError(f"frames {tuple(frames.shape)}: {n_tiles} tiles from slot {first_slot} do not fit {total_slots} slots")
    prefix = 1 if row_prefix else 0
    Hs, Ws, nbytes = K.sample_sheet_shape(total_slots, H, W, nrow, padding, prefix)
    shape = (n_sheets, Hs, 1 + 3 * Ws) if prefix else (n_sheets, Hs, Ws, 3)
    if not frames.is_cuda:
        raise ValueError(f"sheets take frames on a GPU (there is no CPU path), got {frames.device} {tuple(frames.shape)}")
    if out is None:
        if not fill:
            raise ValueError("fill=False leaves every byte outside the tiles as it was: it needs `out`")
        out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    elif (out.dtype != torch.uint8 or out.device != frames.device or not out.is_contiguous() or out.numel() != n_sheets * nbytes):
        raise ValueError(f"out: a contiguous uint8 tensor of {n_sheets * nbytes} bytes {shape} on {frames.device}, got "
                         f"{out.dtype} {tuple(out.shape)} on {out.device}")
    if n_sheets == 0:
        return out.view(shape)
    last = (n_sheets - 1) * ss + (n_tiles - 1) * s_tile + 2 * sc + H * W - 1
    if frames.storage_offset() + last >= frames.untyped_storage().nbytes() // 4:
        raise ValueError(f"frames {tuple(frames.shape)} with strides {frames.stride()} reach past their storage")
    flags = (K.SHEET_FILL if fill else 0) | (K.SHEET_SIGNED if signed else 0)
    K.sample_sheet(frames, (ss, s_tile, sc), n_sheets, n_tiles, H, W, first_slot, total_slots, nrow, padding, pad_value, prefix,
                   flags, out)
    return out.view(shape)


# ------------------------------------------------------------------ files
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", binascii.crc32(tag + data) & 0xffffffff)


def _scanlines(sheet):
    """Host uint8 [Hs, Ws, 3] or prefixed [Hs, 1 + 3 Ws] -> (Hs, Ws, buffer of Hs rows of filter byte 0 + RGB)."""
    a = sheet.numpy() if isinstance(sheet, torch.Tensor) else np.asarray(sheet)
    if a.dtype != np.uint8:
        raise ValueError(f"a sheet is uint8, got {a.dtype} {a.shape}")
    if a.ndim == 3 and a.shape[2] == 3 and a.shape[0] and a.shape[1]:
        rows = np.zeros((a.shape[0], 1 + 3 * a.shape[1]), dtype=np.uint8)
        rows[:, 1:] = a.reshape(a.shape[0], -1)
        return a.shape[0], a.shape[1], rows
    if a.ndim == 2 and a.shape[0] and a.shape[1] > 1 and (a.shape[1] - 1) % 3 == 0:
        if a[:, 0].any():
            raise ValueError(f"prefixed sheet {a.shape}: the first byte of every row must be 0 (PNG filter type None)")
        return a.shape[0], (a.shape[1] - 1) // 3, np.ascontiguousarray(a)
    raise ValueError(f"a sheet is [Hs, Ws, 3] or, with the row prefix, [Hs, 1 + 3 Ws]; got {a.shape}")


def _ihdr(Hs, Ws):
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", Ws, Hs, 8, 2, 0, 0, 0))          # 8-bit RGB, no interlace


def write_png(path, sheet, level=LEVEL):
    """One host sheet -> an 8-bit RGB PNG with a single IDAT."""
    Hs, Ws, rows = _scanlines(sheet)
    with open(path, "wb") as f:
        f.write(_PNG_SIG + _ihdr(Hs, Ws) + _chunk(b"IDAT", zlib.compress(rows, level)) + _chunk(b"IEND", b""))


def write_apng(path, sheets, fps, loops=0, level=LEVEL):
    """Host sheets of one size (a stack [N, ...] or a sequence) -> an animated PNG: acTL, then per frame an fcTL and the image
    (IDAT for the first frame, fdAT after it); every frame is shown 1 / fps seconds, replaces the canvas (blend: source) and is
    left in place (dispose: none); loops = 0 plays for ever.  A plain PNG reader shows the first frame."""
    frames = [_scanlines(s) for s in sheets]
    if not frames:
        raise ValueError("an animation needs at least one sheet")
    Hs, Ws = frames[0][:2]
    if any(f[:2] != (Hs, Ws) for f in frames):
        raise ValueError(f"the sheets of an animation share one size, got {sorted({f[:2] for f in frames})}")
    rate = Fraction(fps).limit_denominator(1000) if fps > 0 else None
    if rate is None or not 0 < rate.numerator <= 0xffff or int(loops) < 0:
        raise ValueError(f"fps={fps} (positive, the delay 1 / fps as a ratio of two 16-bit integers), loops={loops} (>= 0)")
    seq = 0
    with open(path, "wb") as f:
        f.write(_PNG_SIG + _ihdr(Hs, Ws) + _chunk(b"acTL", struct.pack(">II", len(frames), int(loops))))
        for n, (_, _, rows) in enumerate(frames):
            f.write(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, Ws, Hs, 0, 0, rate.denominator, rate.numerator, 0, 0)))
            seq += 1
            data = zlib.compress(rows, level)
            if n == 0:
                f.write(_chunk(b"IDAT", data))
            else:
                f.write(_chunk(b"fdAT", struct.pack(">I", seq) + data))
                seq += 1
        f.write(_chunk(b"IEND", b""))


class SheetWriter:
    """Writes sheets to files behind the training loop.  submit() queues a copy of the bytes into a pinned host block on the
    caller's stream (non_blocking), records an event and returns; one worker thread waits for that event, deflates and writes.
    The worker starts no GPU work.  At most max_pending jobs are outstanding: submit() blocks only then.  A pinned block is
    handed out again only after its job is done.  The first exception of a job is kept and re-raised by flush()."""

    KINDS = ("png", "apng")

    def __init__(self, max_pending=2, level=LEVEL):
        if int(max_pending) < 1:
            raise ValueError(f"max_pending={max_pending}")
        self.max_pending, self.level = int(max_pending), level
        self._room = threading.Semaphore(self.max_pending)
        self._jobs = queue.Queue()
        self._lock = threading.Lock()
        self._blocks = []                   # pinned blocks no job holds
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._work, name="sheet-writer", daemon=True)
        self._thread.start()

    def _block(self, nbytes, pin):
        with self._lock:
            fit = [b for b in self._blocks if b.numel() >= nbytes and b.is_pinned() == pin]
            if fit:
                best = min(fit, key=lambda b: b.numel())
                self._blocks = [b for b in self._blocks if b is not best]
                return best
            if len(self._blocks) >= self.max_pending:          # outgrown: the pool never holds more than max_pending blocks
                small = min(self._blocks, key=lambda b: b.numel())
                self._blocks = [b for b in self._blocks if b is not small]
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=pin)

    def submit(self, kind, path, device_sheets, **meta):
        """kind "png": `path` is one file name for one sheet, or a list of names for a stack of sheets [n, ...].
        kind "apng": one file, the stack is its frames; meta: fps, loops.  Sheets in either form make_sheets returns."""
        if self._closed:
            raise RuntimeError("this SheetWriter is closed")
        if kind not in self.KINDS:
            raise ValueError(f"kind={kind!r}: one of {self.KINDS}")
        t = device_sheets
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError(f"sheets are contiguous uint8 tensors, got {t.dtype} {tuple(t.shape)}")
        single = kind == "png" and (isinstance(path, (str, bytes)) or hasattr(path, "__fspath__"))
        if kind == "png" and not single and len(path) != t.shape[0]:
            raise ValueError(f"{len(path)} file names for {t.shape[0]} sheets {tuple(t.shape)}")
        if kind == "apng" and "fps" not in meta:
            raise ValueError("an animation needs fps=")
        self._room.acquire()
        try:
            block = self._block(t.numel(), t.is_cuda)
            host = block[:t.numel()].view(t.shape)
            host.copy_(t, non_blocking=True)
            event = None
            if t.is_cuda:
                event = torch.cuda.Event()
                event.record(torch.cuda.current_stream(t.device))
        except BaseException:
            self._room.release()
            raise
        self._jobs.put((kind, path, single, host, block, event, meta))

    def _work(self):
        while True:
            job = self._jobs.get()
            if job is None:
                self._jobs.task_done()
                return
            kind, path, single, host, block, event, meta = job
            try:
                if event is not None:
                    event.synchronize()
                if kind == "apng":
                    write_apng(path, host, meta["fps"], meta.get("loops", 0), self.level)
                elif single:
                    write_png(path, host, self.level)
                else:
                    for name, sheet in zip(path, host):
                        write_png(name, sheet, self.level)
            except BaseException as e:             # kept for flush(); the worker lives on
                with self._lock:
                    if self._error is None:
                        self._error = e
            finally:
                with self._lock:
                    self._blocks.append(block)
                self._room.release()
                self._jobs.task_done()

    def flush(self):
        """Wait for every submitted job; re-raise the first exception one of them hit (once)."""
        self._jobs.join()
        with self._lock:
            e, self._error = self._error, None
        if e is not None:
            raise e

    def close(self):
        """flush(), then end the worker.  A second close() does nothing."""
        if self._closed:
            return
        self._closed = True
        try:
            self.flush()
        finally:
            self._jobs.put(None)
            self._thread.join()
            self._blocks.clear()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                               # the block's own exception is the one to report
            try:
                self.close()
            except Exception:
                pass
        return False

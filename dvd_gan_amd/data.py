"""Real-data input path: the UCF-101 JPEG-folder reader of the reference (Dataloader/datasets/ucf101.py:82-199 with the
training transforms main.py:42-55 builds) feeding the HIP trainer.

Split of work:
  host (DataLoader workers): JSON annotation index (`make_dataset`, same records as the reference), JPEG decode, temporal
      crop, the multi-scale crop + bilinear resize -- done with PIL exactly like the reference, so pixels are identical;
      a clip leaves the worker as uint8 [T, S, S, 3] plus its flip flag (4x smaller than the reference's fp32 tensor over
      PCIe);
  device (`clips_to_device`, kernel dvd_clip_to_tensor): horizontal flip, ToTensor(norm_value) + Normalize(mean, std) and the
      [T, S, S, 3] -> [3, T, S, S] layout change, one pass, into the fp32 [B, 3, T, S, S] batch `Trainer.train_step` takes.
Random draws come from Python's `random` in the reference's order (temporal crop, then scale, crop position, flip), so a seeded
run reproduces the reference's clips bit for bit (tests/test_gpu_data.py, fixture F12).

Second path, for data that fits in device memory (`ClipStore`, `make_store_loader`; tests/test_gpu_clipstore.py): the host reader
above decodes and resizes every frame of every step on DataLoader workers (measured on small synthetic JPEGs: 16 workers deliver
about six times the benchmark step's clip rate; the store, with no worker at all, fifty times that: profiles/clipstore_numbers.md).
Split of work there:
  host, once (`ClipStore.build`): every frame of every video decoded with the reader's own PIL call and packed into one uint8 blob
      [frame][h][w][3] that lives on the device, plus per-video (offset, h, w, frames) and per-record (video, label, window);
  host, per step (`make_store_loader`): the reader's random draws in the reader's order -- temporal crop, scale, position, flip --
      turned into an integer crop box per clip with the reader's own expressions and PIL's rounding, the coefficient tables of
      PIL's 8-bit bilinear resize for every new (crop side, output side) pair (`resize_coeffs`, fp64, cached on the device), and ONE
      small upload of the clip rows and frame indices;
  device, per step (`ClipStore.gather`, kernel dvd_clip_gather): crop, the two integer resize passes, flip, normalise and layout
      in one launch.  The bytes equal the host reader's: PIL's 8-bit resize is integer arithmetic on those tables.
"""
import json
import math
import os
import random

import torch
import torch.utils.data as data

from . import lib as L


def load_value_file(path):                      # utils.py:54-58
    with open(path, "r") as f:
        return float(f.read().rstrip("\n\r"))


def make_dataset(root_path, annotation_path, subset, n_samples_for_each_video=1, sample_duration=16):
    """Index of the clips to draw from: one record per video of `subset`, or per `sample_duration`-frame window when
    n_samples_for_each_video > 1 -- the records Dataloader/datasets/ucf101.py:82-140 builds (same order, same keys), so a
    seeded run picks the same videos as the reference.  -> (records, {class index: class name})."""
    with open(annotation_path, "r") as f:
        ann = json.load(f)
    index_of = {label: n for n, label in enumerate(ann["labels"])}
    records = []
    for vid, entry in ann["database"].items():                 # file order = the reference's order
        cls = entry["annotations"]["label"]
        folder = os.path.join(root_path, cls, vid)
        if entry["subset"] != subset or not os.path.exists(folder) or cls not in index_of:
            continue
        total = int(load_value_file(os.path.join(folder, "n_frames")))
        if total <= 0:
            continue
        if n_samples_for_each_video == 1:
            windows = [(1, total + 1)]
        else:                                                   # windows spread evenly over the video, at least one frame apart;
            # n_samples_for_each_video < 1: back-to-back windows (ucf101.py:124-129: step = sample_duration)
            stride = (max(1, math.ceil((total - 1 - sample_duration) / (n_samples_for_each_video - 1)))
                      if n_samples_for_each_video > 1 else sample_duration)
            windows = [(first, min(total + 1, first + sample_duration)) for first in range(1, total, stride)]
        for lo, hi in windows:
            records.append({"video": folder, "segment": [1, total], "n_frames": total, "video_id": vid,
                            "label": index_of[cls], "frame_indices": list(range(lo, hi))})
    return records, {n: label for label, n in index_of.items()}


def temporal_random_crop(frame_indices, size):
    """`size` consecutive frames from a random start; a shorter clip is repeated cyclically up to `size`
    (Dataloader/transform/temporal_transforms.py:80-110; ONE random.randint draw, like the reference)."""
    first = random.randint(0, max(0, len(frame_indices) - size - 1))
    window = frame_indices[first:first + size]
    if not window or len(window) >= size:
        return list(window)
    return [window[i % len(window)] for i in range(size)]


class MultiScaleCrop:
    """MultiScaleCornerCrop / MultiScaleRandomCrop of Dataloader/transform/spatial_transforms.py:271-367 (crop box + PIL
    bilinear resize to `size`); `mode` = 'corner' | 'center' | 'random' as main.py:42-50 selects them."""

    def __init__(self, scales, size, mode="corner"):
        if mode not in ("corner", "center", "random"):
            raise ValueError("train_crop must be 'random', 'corner' or 'center'")
        self.scales, self.size, self.mode = scales, size, mode
        self.positions = ["c"] if mode == "center" else ["c", "tl", "tr", "bl", "br"]

    def randomize_parameters(self):
        self.scale = self.scales[random.randint(0, len(self.scales) - 1)]
        if self.mode == "random":
            self.tl_x, self.tl_y = random.random(), random.random()
        else:
            self.crop_position = self.positions[random.randint(0, len(self.positions) - 1)]

    def box(self, w, h):
        """The crop box (left, upper, right, lower) for a w x h frame under the drawn parameters, as handed to `img.crop`
        (floats in 'random' mode: crop rounds them half to even)."""
        crop = int(min(w, h) * self.scale)
        if self.mode == "random":
            x1, y1 = self.tl_x * (w - crop), self.tl_y * (h - crop)
            return (x1, y1, x1 + crop, y1 + crop)
        p = self.crop_position
        if p == "c":
            cx, cy, half = w // 2, h // 2, crop // 2
            return (cx - half, cy - half, cx + half, cy + half)
        if p == "tl":
            return (0, 0, crop, crop)
        if p == "tr":
            return (w - crop, 0, w, crop)
        if p == "bl":
            return (0, h - crop, crop, h)
        return (w - crop, h - crop, w, h)

    def __call__(self, img):
        from PIL import Image
        w, h = img.size
        return img.crop(self.box(w, h)).resize((self.size, self.size), Image.BILINEAR)


def default_scales(initial_scale=1.0, n_scales=5, scale_step=0.84089641525):     # main.py:38-40, parameter.py:73-75
    scales = [initial_scale]
    for _ in range(1, n_scales):
        scales.append(scales[-1] * scale_step)
    return scales


class UCF101(data.Dataset):
    """Training-set view of a UCF-101 JPEG folder (`<root>/<class>/<video>/image_%05d.jpg` + `n_frames`, annotation JSON of
    utils/ucf101_json.py).  __getitem__ -> (uint8 clip [T, S, S, 3], flip flag, class index)."""

    def __init__(self, root_path, annotation_path, subset="training", n_frames=16, sample_size=64, scales=None,
                 train_crop="corner", n_samples_for_each_video=1, sample_duration=16):
        self.data, self.class_names = make_dataset(root_path, annotation_path, subset, n_samples_for_each_video, sample_duration)
        self.n_frames = n_frames
        self.crop = MultiScaleCrop(scales or default_scales(), sample_size, train_crop)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        import numpy as np
        from PIL import Image
        rec = self.data[index]
        frame_indices = temporal_random_crop(list(rec["frame_indices"]), self.n_frames)
        self.crop.randomize_parameters()
        flip = random.random() < 0.5                   # RandomHorizontalFlip.randomize_parameters / __call__ (:253-268)
        frames = []
        for i in frame_indices:                        # video_loader (:37-46): stops at the first missing frame
            path = os.path.join(rec["video"], "image_{:05d}.jpg".format(i))
            if not os.path.exists(path):
                break
            with open(path, "rb") as f, Image.open(f) as img:
                frames.append(np.asarray(self.crop(img.convert("RGB")), dtype=np.uint8))
        clip = torch.from_numpy(np.stack(frames, 0))
        return clip, torch.tensor(bool(flip)), rec["label"]


def clips_to_device(clips, flips, device, norm_value=255.0, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    """uint8 [B, T, S, S, 3] (host or device) + flip flags [B] -> fp32 [B, 3, T, S, S] on `device`:
    ((x / norm_value) - mean) / std with the flagged clips mirrored (main.py:34-36,51-54 defaults: [-1, 1])."""
    clips = clips.to(device, non_blocking=True).contiguous()
    flips = flips.to(device=device, dtype=torch.uint8).contiguous()
    B, T, S1, S2, ch = clips.shape
    assert ch == 3 and clips.dtype == torch.uint8
    out = torch.empty(B, 3, T, S1, S2, dtype=torch.float32, device=device)
    ms = torch.tensor(list(mean) + list(std), dtype=torch.float32, device=device)
    L.check(L.lib().dvd_clip_to_tensor(L.ptr(clips), L.ptr(flips), L.ptr(out), B, T, S1, S2, float(norm_value), L.ptr(ms),
                                       L.stream()))
    return out


def make_loader(dataset, batch_size, num_workers=0, shuffle=True, device=None, rank=None, world=None, seed=0):
    """DataLoader whose batches are (fp32 [B,3,T,S,S] on `device`, labels [B]) -- what Trainer.train expects.
    Two deliberate differences from the reference's DataLoader (main.py:57-62): the last, incomplete batch is DROPPED
    (the generator's batch size is fixed by z, and the ConvGRU / CBN buffers are sized for it), so len(loader) -- and with it
    steps_per_epoch / total_step / the log and save cadence of Trainer.train -- is floor(N / B), not ceil(N / B); and in a
    data-parallel run (rank / world given, or read from torch.distributed) every rank iterates ITS OWN 1/world of a common
    permutation (DistributedSampler seeded alike on all ranks; call `loader.set_epoch(e)` per epoch), so an epoch covers
    the data once instead of world times.
    The object has state_dict() / load_state_dict() (the running epoch's record order, the batches yielded, the epoch number): the
    next `iter()` after load_state_dict() continues that epoch.  With num_workers=0 its first batch is bit-equal to the one the
    saved loader would have yielded next once Python's `random` is restored too (the global streams are the caller's to save).
    With num_workers > 0 only the records and their order are promised: crop and flip are drawn in worker processes that
    DataLoader seeds anew for every iterator."""
    if world is None and torch.distributed.is_available() and torch.distributed.is_initialized():
        world, rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
    sampler = None
    if world is not None and world > 1:
        sampler = data.distributed.DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
                                                      drop_last=True)
    # the order comes from the sampler DataLoader would have built itself (same draws from the default generator at the same
    # moment: its __iter__ runs at the first batch); _Resumable lists it, so that the position can be saved
    base = sampler if sampler is not None else (data.RandomSampler(dataset) if shuffle else data.SequentialSampler(dataset))
    pos = _EpochPosition(batch_size)

    class _Resumable(data.Sampler):
        def __len__(self):
            return len(base)

        def __iter__(self):
            order, first = pos.begin(lambda: base)
            yield from order[first * batch_size:]

    loader = data.DataLoader(dataset, batch_size=batch_size, sampler=_Resumable(), num_workers=num_workers, pin_memory=True,
                             drop_last=True)

    class _OnDevice:
        def __len__(self):
            return len(loader)

        def set_epoch(self, epoch):
            pos.epoch = int(epoch)
            if sampler is not None:
                sampler.set_epoch(epoch)

        def state_dict(self):
            return pos.state_dict()

        def load_state_dict(self, sd):
            pos.load_state_dict(sd, len(dataset))
            if sampler is not None:
                sampler.set_epoch(pos.epoch)

        def host_batches(self):
            """(uint8 clips, flips, labels) per batch, still on the host; the position kept as it goes."""
            if pos.pending:
                # DataLoader draws a seed for its workers from the default generator whenever an iterator is made; the epoch
                # that is being continued drew it when it began, so here the generator is left as it was
                keep = torch.get_rng_state()
                it = iter(loader)
                torch.set_rng_state(keep)
            else:
                it = iter(loader)
            for batch in it:
                pos.cursor += 1
                yield batch

        def __iter__(self):
            dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
            for clips, flips, labels in self.host_batches():
                yield clips_to_device(clips, flips, dev), labels
    return _OnDevice()


class _EpochPosition:
    """Where a loader stands inside an epoch: `order`, the record ids of the running epoch as its sampler produced them (never
    re-derived from a generator state), `cursor`, the batches yielded so far, and `epoch`, the number last given to set_epoch.
    Plain integers, so a state file holding it loads with weights_only=True."""

    def __init__(self, batch_size):
        self.batch_size, self.epoch, self.order, self.cursor, self.pending = int(batch_size), 0, None, 0, False

    def begin(self, make_order):
        """-> (order, batches already yielded) of the epoch to iterate now: the one load_state_dict() left pending, else a new one
        from make_order()."""
        if self.pending:
            self.pending = False
        else:
            self.order, self.cursor = [int(i) for i in make_order()], 0
        return self.order, self.cursor

    def state_dict(self):
        return {"order": list(self.order or []), "cursor": self.cursor, "epoch": self.epoch, "batch_size": self.batch_size,
                "started": self.order is not None}

    def load_state_dict(self, sd, n_records):
        if int(sd["batch_size"]) != self.batch_size:
            raise ValueError(f"batch_size: the loader state was written with {sd['batch_size']}, this loader has {self.batch_size}")
        order = [int(i) for i in sd["order"]]
        if order and not 0 <= min(order) <= max(order) < n_records:
            raise ValueError(f"order: record ids [{min(order)}, {max(order)}] for a dataset of {n_records} records")
        if not 0 <= int(sd["cursor"]) <= len(order) // self.batch_size:
            raise ValueError(f"cursor: {sd['cursor']} batches of {len(order) // self.batch_size} in the saved epoch")
        self.epoch, self.cursor, self.pending = int(sd["epoch"]), int(sd["cursor"]), bool(sd["started"])
        self.order = order if self.pending else None


# ------------------------------------------------------------------ device-resident clip store
PRECISION_BITS = 22         # Resample.c: 8-bit coefficients are scaled by 2^22, accumulators start at 2^21


def resize_coeffs(in_size, out_size):
    """Pillow's coefficient table for resampling in_size -> out_size samples of an 8-bit image with the bilinear filter
    (Resample.c: precompute_coeffs + normalize_coeffs_8bpc, fp64 like there).  -> (bounds int32 [out, 2] = first source sample and
    count per output sample, coefficients int32 [out, ksize], zero past the count).  Bilinear weights are never negative."""
    import numpy as np
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs                                            # filter support 1.0 * filterscale
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5)) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(xmax)]
        ww = 0.0
        for v in w:                                         # summed in order, like the C loop
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = xmin, xmax
        kk[xx, :xmax] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return bounds, kk


def crop_box(crop, w, h):
    """The integer box (x0, y0, cw, ch) `crop(img)` cuts from a w x h frame: MultiScaleCrop.box rounded as Image.crop rounds it
    (Python's round: half to even), so in 'random' mode cw and ch are each crop - 1, crop or crop + 1, independently."""
    x0, y0, x1, y1 = (int(round(v)) for v in crop.box(w, h))
    return x0, y0, x1 - x0, y1 - y0


class ClipStore:
    """Every frame of a `UCF101` dataset decoded once into one uint8 blob [frame][h][w][3] ON THE DEVICE, with the tables that find
    a record's frames in it; `gather` cuts a batch of clips from it in one kernel launch (dvd_clip_gather).  The whole blob must fit
    in the memory of one device next to the model (UCF-101 at 240 x 320 is 2.5 M frames = 580 GB: use `prescale`; at a short side
    of 64 it is 41 GB); stores larger than device memory, or kept in host memory, are not served -- `make_loader` is the path for
    those.

    Tensors (what `save` writes): blob uint8 [bytes]; video_offset int64, video_h / video_w / video_frames int32 [videos];
    record_video / record_label / record_first / record_last int64 [records] (first / last: the 1-based frame numbers that bound
    the record's `frame_indices`; the windows of n_samples_for_each_video > 1 point into the same stored video)."""

    FIELDS = ("blob", "video_offset", "video_h", "video_w", "video_frames", "record_video", "record_label", "record_first",
              "record_last")

    def __init__(self, **tensors):
        assert set(tensors) == set(self.FIELDS), sorted(set(tensors) ^ set(self.FIELDS))
        for k, v in tensors.items():
            setattr(self, k, v)
        self._videos = list(zip(self.video_offset.tolist(), self.video_h.tolist(), self.video_w.tolist(), self.video_frames.tolist()))
        self._records = list(zip(self.record_video.tolist(), self.record_label.tolist(), self.record_first.tolist(),
                                 self.record_last.tolist()))
        self._tables, self._pool, self._pool_used, self._ms = {}, None, 0, {}

    def __len__(self):
        return len(self._records)

    @property
    def device(self):
        return self.blob.device

    def record(self, index):
        """-> (label, first frame number, last frame number, h, w) of record `index`."""
        video, label, first, last = self._records[index]
        return label, first, last, self._videos[video][1], self._videos[video][2]

    @classmethod
    def build(cls, dataset, prescale=None, device="cpu"):
        """Decode every frame `image_00001 .. image_{n_frames}` of every distinct video of `dataset` (a `UCF101`) with the reader's
        call, `Image.open(f).convert("RGB")`.  A video with a missing frame file, or with frames of different sizes, raises (the
        host reader silently returns a short clip there, which cannot be batched).
        prescale=P: every frame is resized with PIL bilinear so that its short side is P (the long side int(P * long / short))
        before it is stored.  This CHANGES THE PIXELS relative to the host reader, which crops the original frames: only a store
        built with prescale=None reproduces the reader bit for bit."""
        import numpy as np
        from PIL import Image
        videos, frames, tables, records = {}, [], [], []
        offset = 0
        for rec in dataset.data:
            folder = rec["video"]
            if folder not in videos:
                size, n = None, int(rec["n_frames"])
                for i in range(1, n + 1):
                    path = os.path.join(folder, "image_{:05d}.jpg".format(i))
                    if not os.path.exists(path):
                        raise FileNotFoundError(f"{path}: frame {i} of {n} is missing (ClipStore needs every frame of a video)")
                    with open(path, "rb") as f, Image.open(f) as img:
                        img = img.convert("RGB")
                        if prescale is not None:
                            w, h = img.size
                            to = (prescale, int(prescale * h / w)) if w <= h else (int(prescale * w / h), prescale)
                            img = img.resize(to, Image.BILINEAR)
                        a = np.asarray(img, dtype=np.uint8)
                    if size is None:
                        size = a.shape
                    elif a.shape != size:
                        raise ValueError(f"{path}: frame size {a.shape[:2]} differs from the video's {size[:2]}")
                    frames.append(a.reshape(-1))
                videos[folder] = len(tables)
                tables.append((offset, size[0], size[1], n))
                offset += n * size[0] * size[1] * 3
            ids = rec["frame_indices"]
            records.append((videos[folder], rec["label"], ids[0], ids[-1]))
        blob = torch.from_numpy(np.concatenate(frames)) if frames else torch.empty(0, dtype=torch.uint8)
        col = lambda rows, j, dtype: torch.tensor([r[j] for r in rows], dtype=dtype)
        return cls(blob=blob.to(device), video_offset=col(tables, 0, torch.int64), video_h=col(tables, 1, torch.int32),
                   video_w=col(tables, 2, torch.int32), video_frames=col(tables, 3, torch.int32),
                   record_video=col(records, 0, torch.int64), record_label=col(records, 1, torch.int64),
                   record_first=col(records, 2, torch.int64), record_last=col(records, 3, torch.int64))

    def save(self, path):
        """One file of plain tensors (torch.save of a dict; `load` reads it with weights_only=True)."""
        torch.save({k: getattr(self, k).cpu() for k in self.FIELDS}, path)

    @classmethod
    def load(cls, path, device):
        """The store `save` wrote, its blob on `device` (the tables stay on the host: only the draws read them)."""
        t = torch.load(path, map_location="cpu", weights_only=True)
        t["blob"] = t["blob"].to(device)
        return cls(**t)

    def to(self, device):
        return ClipStore(**{k: getattr(self, k).to(device) if k == "blob" else getattr(self, k) for k in self.FIELDS})

    def _table(self, in_size, out_size):
        """Position (in ints) of the coefficient table in_size -> out_size in the device pool; built and uploaded on first use (a
        training run needs a handful: five scales, in 'random' mode three widths each)."""
        from .helpers import to_device_async
        pos = self._tables.get((in_size, out_size))
        if pos is None:
            bounds, kk = resize_coeffs(in_size, out_size)
            flat = torch.cat([torch.from_numpy(bounds).reshape(-1), torch.from_numpy(kk).reshape(-1)])
            need = self._pool_used + flat.numel()
            if self._pool is None or need > self._pool.numel():
                pool = torch.zeros(max(1 << 16, 2 * need), dtype=torch.int32, device=self.device)
                if self._pool is not None:
                    pool[:self._pool_used].copy_(self._pool[:self._pool_used])
                self._pool = pool
            self._pool[self._pool_used:need].copy_(to_device_async(flat, self.device))
            pos = self._tables[(in_size, out_size)] = self._pool_used
            self._pool_used = need
        return pos

    def gather(self, record_ids, frame_ids, boxes, flips, size, norm_value=255.0, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        """The batch of clips -> fp32 [B, 3, T, size, size] on the store's device, one launch, nothing waited for: per clip b the
        record index record_ids[b], its T frame numbers frame_ids[b] (1-based, as in the file names and `frame_indices`), the
        integer crop box boxes[b] = (x0, y0, cw, ch) inside the frame and the flip flag flips[b]; each frame is cropped, resized
        with PIL's 8-bit bilinear arithmetic, mirrored if flagged and written as ((v / norm_value) - mean) / std: the bytes of
        `clips_to_device` on the host reader's clip."""
        from . import kern as K
        from .helpers import to_device_async
        B, T = len(record_ids), len(frame_ids[0])
        if not self.blob.is_cuda:
            raise RuntimeError("ClipStore.gather needs the blob on the GPU (ClipStore.load(path, device) / .to(device)): there is "
                               "no CPU path")
        head, tail = [], []                              # B rows of L.CLIP_COLS columns, then the B * T frame indices
        for b in range(B):
            off, h, w, n = self._videos[self._records[record_ids[b]][0]]
            x0, y0, cw, ch = (int(v) for v in boxes[b])
            if not (0 < cw and 0 < ch and 0 <= x0 <= w - cw and 0 <= y0 <= h - ch):
                raise ValueError(f"clip {b}: box {tuple(boxes[b])} is not inside the {w} x {h} frame")
            if len(frame_ids[b]) != T:
                raise ValueError(f"clip {b}: {len(frame_ids[b])} frames, the batch has {T} (short clips cannot be batched)")
            head += [off, h, w, n, x0, y0, cw, ch, int(bool(flips[b])), self._table(cw, size), self._table(ch, size)]
            tail += [int(f) - 1 for f in frame_ids[b]]
        rows = torch.tensor(head + tail, dtype=torch.int64)
        key = (float(norm_value), tuple(mean), tuple(std))
        if key not in self._ms:
            self._ms[key] = to_device_async(torch.tensor(list(mean) + list(std), dtype=torch.float32), self.device)
        out = torch.empty(B, 3, T, size, size, dtype=torch.float32, device=self.device)
        return K.clip_gather(self.blob, rows, to_device_async(rows, self.device), self._pool, out, self._ms[key], norm_value)


class StoreLoader:
    """What `make_store_loader` returns: len / iter / set_epoch like `make_loader`'s object, plus `plan_epoch` and `batch`."""

    def __init__(self, store, batch_size, n_frames, crop, shuffle, sampler):
        self.store, self.batch_size, self.n_frames, self.crop, self.shuffle, self.sampler = store, batch_size, n_frames, crop, shuffle, sampler
        self._pos = _EpochPosition(batch_size)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.store)
        return n // self.batch_size

    def set_epoch(self, epoch):
        self._pos.epoch = int(epoch)
        if self.sampler is not None:
            self.sampler.set_epoch(epoch)

    def state_dict(self):
        """Where iteration stands: the running epoch's record ids in order, the batches already yielded and the epoch number
        (_EpochPosition).  No random state: `draw` reads Python's `random`, `plan_epoch` torch's default generator -- global
        streams whoever saves the run saves with it."""
        return self._pos.state_dict()

    def load_state_dict(self, sd):
        """The next `iter()` continues the epoch `sd` was taken in: its first batch is the one the saved loader would have
        yielded next (bit-equal when Python's `random` is restored with it), and `plan_epoch` is not called for that epoch."""
        self._pos.load_state_dict(sd, len(self.store))
        if self.sampler is not None:
            self.sampler.set_epoch(self._pos.epoch)

    def plan_epoch(self):
        """The record indices of every batch of one epoch, in order; touches no device.  (Single process with shuffle: draws a
        permutation from torch's default generator, so every call gives another one.)"""
        if self.sampler is not None:
            order = list(self.sampler)
        elif self.shuffle:
            order = torch.randperm(len(self.store)).tolist()
        else:
            order = list(range(len(self.store)))
        B = self.batch_size
        return [order[i:i + B] for i in range(0, len(order) - B + 1, B)]

    def draw(self, record_ids):
        """The reader's draws from Python's `random` for these records, one record after the other, each in the order of
        UCF101.__getitem__: temporal crop (cyclic repeat of short windows included), scale, position (or the two random() of
        'random' mode), flip.  -> (frame numbers [B][T], boxes [B] = (x0, y0, cw, ch), flips [B], labels [B])."""
        frames, boxes, flips, labels = [], [], [], []
        for index in record_ids:
            label, first, last, h, w = self.store.record(index)
            frames.append(temporal_random_crop(list(range(first, last + 1)), self.n_frames))
            self.crop.randomize_parameters()
            flips.append(random.random() < 0.5)
            boxes.append(crop_box(self.crop, w, h))
            labels.append(label)
        return frames, boxes, flips, labels

    def batch(self, record_ids):
        """-> (fp32 [B, 3, T, S, S] on the store's device, labels [B]) for these records, drawn as `draw` says."""
        frames, boxes, flips, labels = self.draw(record_ids)
        return self.store.gather(record_ids, frames, boxes, flips, self.crop.size), torch.tensor(labels)

    def plans(self):
        """The host half of one epoch: (record ids, `draw` of them) per batch, the position kept as it goes.  Touches no device.
        After load_state_dict() it continues the saved epoch instead of planning a new one.  One iteration at a time: the
        position belongs to the loader, not to the iterator."""
        order, first = self._pos.begin(lambda: [i for ids in self.plan_epoch() for i in ids])
        B = self.batch_size
        for lo in range(first * B, len(order) - B + 1, B):
            self._pos.cursor += 1
            yield order[lo:lo + B], self.draw(order[lo:lo + B])

    def __iter__(self):
        for record_ids, (frames, boxes, flips, labels) in self.plans():
            yield self.store.gather(record_ids, frames, boxes, flips, self.crop.size), torch.tensor(labels)


def make_store_loader(store, batch_size, n_frames, sample_size, scales=None, train_crop="corner", shuffle=True, rank=None,
                      world=None, seed=0):
    """`make_loader` for a `ClipStore`: batches are (fp32 [B, 3, T, S, S] on the store's device, labels [B]) -- what Trainer.train
    expects --, the last, incomplete batch is dropped, and the clips are the ones `UCF101(n_frames, sample_size, scales, train_crop)`
    yields for the same records under the same state of Python's `random`, bit for bit: the draws are made per sample, in the
    batch's record order, exactly as UCF101.__getitem__ makes them (so with shuffle=False and num_workers=0 the two loaders agree
    batch by batch).  The host only draws and uploads one small block per batch; it never waits for the device.
    Sample order: shuffle=False: record order.  Data parallel (rank / world given, or read from torch.distributed): the same
    DistributedSampler(seed, drop_last=True) as `make_loader`, so the rank splits are identical; call `set_epoch(e)` per epoch.
    Single process with shuffle=True: a permutation from torch's default generator -- NOT promised to be the order DataLoader's
    RandomSampler would give from the same generator state."""
    if world is None and torch.distributed.is_available() and torch.distributed.is_initialized():
        world, rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
    sampler = None
    if world is not None and world > 1:
        sampler = data.distributed.DistributedSampler(range(len(store)), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
                                                      drop_last=True)
    return StoreLoader(store, batch_size, n_frames, MultiScaleCrop(scales or default_scales(), sample_size, train_crop), shuffle,
                       sampler)

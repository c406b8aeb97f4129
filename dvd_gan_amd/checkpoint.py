"""Training-state files for exact resume (`Trainer.save_state` / `load_state`): the file format, the atomic
write, pruning and look-up of `{step}_state.pt`, the host-side random streams, and `StateWriter`, which takes a snapshot off the
device behind the training loop.

A state file is one dict of CPU tensors and plain Python scalars / lists / strings -- it loads with
`torch.load(path, weights_only=True)` and is only ever loaded that way:
    format_version  FORMAT_VERSION
    step            the step the state was taken after
    fingerprint     the configuration fields that decide shapes and arithmetic (FINGERPRINT)
    tensors         name -> tensor: "net.<G|Ds|Dt>.<state_dict key>" for every entry that is not a trained weight (spectral-norm
                    u / v, batch-norm running statistics and counters), "opt.<G|Ds|Dt>.<flat|m|v|ema>" (the trained weights ARE
                    `flat`, in parameter order), "opt.<..>.<guard_state|guard_ring|ortho_penalty>"
    host            everything kept on the host: step counts, learning rates, schedulers, epoch, loader position, random streams,
                    and "params": per network the trained tensors' names and shapes in `flat`'s order (parameter_table)
There is no arithmetic here and no kernel: the snapshot is copies on streams, pinned memory and events.
"""
import os
import queue
import random
import re
import threading

import torch

FORMAT_VERSION = 1
FINGERPRINT = ("g_chn", "ds_chn", "dt_chn", "n_frames", "n_cond", "n_class", "z_dim", "latent_dim", "g_self_attn", "g_sep_attn",
               "compute_dtype", "adv_loss", "d_iters", "k_sample", "batch_size", "world_size", "dp_mode")
_STATE_FILE = re.compile(r"^(\d+)_state\.pt$")
_ANY_STATE_FILE = re.compile(r"^(\d+)_state(\.rank\d+)?\.pt$")
_ALIGN = 256                    # bytes: every tensor starts on a boundary any dtype and any copy engine likes


# ------------------------------------------------------------------ files
def state_path(folder, step, rank=None):
    return os.path.join(folder, "%d_state.pt" % step if rank is None else "%d_state.rank%d.pt" % (step, rank))


def atomic_save(obj, path, _before_replace=None):
    """torch.save(obj) under `path` so that a file of that name is always complete: written to `path + ".tmp"`, flushed and
    fsync'ed, then renamed over `path` (os.replace).  A failure on the way leaves whatever was under `path` before untouched.
    (_before_replace: a callable run between the two halves, for tests of exactly that.)"""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        torch.save(obj, f)
        f.flush()
        os.fsync(f.fileno())
    if _before_replace is not None:
        _before_replace()
    os.replace(tmp, path)


def load_file(path):
    """-> the dict of a state file, read with weights_only=True; ValueError on a format_version this code does not know."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or sd.get("format_version") != FORMAT_VERSION:
        version = sd.get("format_version") if isinstance(sd, dict) else None
        raise ValueError(f"format_version: {path} has {version!r}, this code reads {FORMAT_VERSION}")
    return sd


def check_fingerprint(saved, mine):
    """ValueError naming the first field of FINGERPRINT in which the file's configuration differs from this Trainer's."""
    for k in FINGERPRINT:
        if saved.get(k) != mine[k]:
            raise ValueError(f"{k}: the state was written with {k}={saved.get(k)!r}, this Trainer has {k}={mine[k]!r} (a state "
                             "continues only the configuration that wrote it)")


def parameter_table(net):
    """[[name, shape], ...] of a network's trained tensors, in the order the optimizer's `flat` holds them."""
    return [[k, [int(d) for d in p.shape]] for k, p in net.named_parameters() if p.requires_grad]


def check_parameters(tag, saved, net):
    """ValueError naming the first trained tensor of `net` the file lacks or holds in another shape (or the first one the file
    holds and the network lacks): two architectures whose fingerprints agree -- a ConvGRU and a TSRU generator -- differ here.
    saved: the file's parameter_table of this network, or None (a file from before the table: the optimizer's element count is
    the only check then)."""
    if saved is None:
        return
    held = {k: list(shape) for k, shape in saved}
    mine = parameter_table(net)
    for k, shape in mine:
        if held.get(k) != shape:
            raise ValueError(f"net.{tag}.{k}: the state holds {None if k not in held else tuple(held[k])}, the network "
                             f"{tuple(shape)}")
    names = {k for k, _ in mine}
    for k, shape in saved:
        if k not in names:
            raise ValueError(f"net.{tag}.{k}: the state holds {tuple(shape)}, the network has no such tensor")


def latest_state(folder):
    """-> (step, path) of the complete state file with the highest step in `folder`, or None.  Complete = under its final name:
    `.tmp` files and per-rank files do not count."""
    best = None
    if os.path.isdir(folder):
        for name in os.listdir(folder):
            m = _STATE_FILE.match(name)
            if m and (best is None or int(m.group(1)) > best[0]):
                best = (int(m.group(1)), os.path.join(folder, name))
    return best


def prune_states(folder, keep):
    """Delete the state files (`{step}_state.pt` with their `{step}_state.rank{r}.pt`) of all but the `keep` highest steps that
    have a complete `{step}_state.pt`; keep = 0 keeps all.  Nothing else in the folder is touched, `.tmp` files included.
    -> the names removed."""
    if keep <= 0 or not os.path.isdir(folder):
        return []
    found = [(int(m.group(1)), m.group(2), name) for name in os.listdir(folder) for m in [_ANY_STATE_FILE.match(name)] if m]
    steps = sorted({step for step, rank, _ in found if rank is None}, reverse=True)[:keep]
    if not steps:
        return []
    gone = sorted(name for step, _, name in found if step < steps[-1])
    for name in gone:
        os.remove(os.path.join(folder, name))
    return gone


# ------------------------------------------------------------------ host-side random streams
def host_rng_state(generators=()):
    """The random streams a step draws from on the host, as tensors and plain lists: torch's default CPU generator, Python's
    `random`, numpy's global state, and the named private generators (`generators`: (name, torch.Generator or None) pairs)."""
    import numpy as np
    version, words, gauss = random.getstate()
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    out = {"torch": torch.get_rng_state().clone(),
           "python": {"version": version, "words": list(words), "gauss_next": gauss},
           "numpy": {"kind": str(kind), "keys": torch.from_numpy(keys.astype("int64")), "pos": int(pos), "has_gauss": int(has_gauss),
                     "cached_gaussian": float(cached)}}
    for name, gen in generators:
        out[name] = None if gen is None else gen.get_state().clone()
    return out


def set_host_rng_state(state, generators=()):
    """Put host_rng_state() back.  A private generator is restored only where both sides have it."""
    import numpy as np
    torch.set_rng_state(state["torch"])
    py = state["python"]
    random.setstate((py["version"], tuple(py["words"]), py["gauss_next"]))
    n = state["numpy"]
    np.random.set_state((n["kind"], n["keys"].numpy().astype("uint32"), n["pos"], n["has_gauss"], n["cached_gaussian"]))
    for name, gen in generators:
        if gen is not None and state.get(name) is not None:
            gen.set_state(state[name])


# ------------------------------------------------------------------ the asynchronous snapshot
class StateWriter:
    """Takes a training state off the device and writes it behind the training loop; the shape of sheets.SheetWriter.

    submit(): (1) on the caller's current stream every tensor of the state is copied device-to-device into ONE staging slab
    owned by this object (the optimizers' flat | m | v | ema through FlatAdam.snapshot_into, the small tensors one copy each)
    and an event is recorded -- from there on the training step may overwrite every live buffer; (2) a copy stream of its own
    waits for that event and copies the slab into ONE pinned host buffer, followed by a second event; (3) the worker thread
    waits for the second event, wraps views of the pinned buffer into the file's dict and writes it atomically (atomic_save),
    then prunes older files.  The calling thread never waits for the device.  At most one snapshot is outstanding: a second
    submit() first waits for the worker to be done with both buffers.  An exception of the worker is raised by the next
    submit(), by flush() or by close().

    Memory, with S = 4 * sum over the three networks of numel * (3, or 4 with a weight average) + the small tensors, each
    rounded up to 256 bytes (2.4 GB at the benchmark's widths): S bytes of device memory for the staging slab and S bytes of
    pinned host memory, both allocated at the first submit() and kept until close().  The slab is never returned to the caching
    allocator while a copy is queued: it lives as long as the writer, and is marked as used by the copy stream
    (record_stream) for the day it is freed."""

    def __init__(self):
        self._jobs = queue.Queue()
        self._lock = threading.Lock()
        self._error = None
        self._closed = False
        self._staging = self._pinned = self._copy_stream = None
        self._thread = threading.Thread(target=self._work, name="state-writer", daemon=True)
        self._thread.start()

    @staticmethod
    def _layout(entries):
        """entries: (name, dtype, shape) -> [(name, dtype, shape, offset, nbytes)], total bytes."""
        out, off = [], 0
        for name, dtype, shape in entries:
            n = 1
            for d in shape:
                n *= int(d)
            nbytes = n * torch.empty((), dtype=dtype).element_size()
            out.append((name, dtype, tuple(shape), off, nbytes))
            off += -(-max(nbytes, 1) // _ALIGN) * _ALIGN
        return out, off

    @staticmethod
    def _view(block, dtype, shape, off, nbytes):
        return block[off:off + nbytes].view(dtype).view(shape)

    def _raise_pending(self):
        with self._lock:
            e, self._error = self._error, None
        if e is not None:
            raise e

    def submit(self, path, items, make_file, *, device, after=None, wait=False):
        """items: (name, dtype, shape, fill) per tensor of the state, fill(dst) copying it into the staging view `dst` on the
        current stream.  make_file(tensors) -> the dict to write, `tensors` being name -> CPU tensor (views of the pinned buffer,
        valid until the write is done); it runs on the worker.  after(): run on the worker once the file is complete (pruning).
        wait=True returns when the file is complete (or raises what went wrong)."""
        if self._closed:
            raise RuntimeError("this StateWriter is closed")
        self._jobs.join()                          # one snapshot at a time: the worker is done with both buffers
        self._raise_pending()
        layout, total = self._layout([(name, dtype, shape) for name, dtype, shape, _ in items])
        cuda = torch.device(device).type == "cuda"
        if self._staging is None or self._staging.numel() < total:
            self._staging = self._pinned = None                 # outgrown (a weight average appeared): drop before allocating anew
            self._staging = torch.empty(total, dtype=torch.uint8, device=device)
            self._pinned = torch.empty(total, dtype=torch.uint8, pin_memory=cuda)
            if cuda:
                if self._copy_stream is None:
                    self._copy_stream = torch.cuda.Stream(device=device)
                self._staging.record_stream(self._copy_stream)
        for (name, dtype, shape, off, nbytes), item in zip(layout, items):
            item[3](self._view(self._staging, dtype, shape, off, nbytes))
        done = None
        if cuda:
            taken = torch.cuda.Event()
            taken.record(torch.cuda.current_stream(device))
            self._copy_stream.wait_event(taken)
            with torch.cuda.stream(self._copy_stream):
                self._pinned[:total].copy_(self._staging[:total], non_blocking=True)
                done = torch.cuda.Event()
                done.record(self._copy_stream)
        else:
            self._pinned[:total].copy_(self._staging[:total])
        self._jobs.put((path, layout, make_file, after, done))
        if wait:
            self.flush()

    def _work(self):
        while True:
            job = self._jobs.get()
            if job is None:
                self._jobs.task_done()
                return
            path, layout, make_file, after, done = job
            try:
                if done is not None:
                    done.synchronize()
                # torch.save writes one storage once, but refuses views of it under two dtypes: the fp32 bulk stays views of the
                # pinned buffer, the few other tensors (int64 counters, the guard's fp64) are copied out
                tensors = {name: v if dtype == torch.float32 else v.clone() for name, dtype, shape, off, nbytes in layout
                           for v in [self._view(self._pinned, dtype, shape, off, nbytes)]}
                atomic_save(make_file(tensors), path)
                if after is not None:
                    after()
            except BaseException as e:             # kept for the caller; the worker lives on
                with self._lock:
                    if self._error is None:
                        self._error = e
            finally:
                self._jobs.task_done()

    def flush(self):
        """Wait until the outstanding file is complete; raise what its job hit (once)."""
        self._jobs.join()
        self._raise_pending()

    def close(self):
        """flush(), then end the worker and give both buffers back.  A second close() does nothing."""
        if self._closed:
            return
        self._closed = True
        try:
            self.flush()
        finally:
            self._jobs.put(None)
            self._thread.join()
            self._staging = self._pinned = None

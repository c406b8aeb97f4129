"""Exact resume, the parts that need no GPU: scheduler, FlatAdam and loader state round trips, the state file's atomic write,
pruning, look-up and refusals.  No kernel runs here: FlatAdam is constructed and its state moved, never stepped;
the loaders are compared on their host-side plans and draws."""
import os
import random
import types

import numpy as np
import pytest
import torch


# ------------------------------------------------------------------ schedulers
def _sched(kind, base=1e-3):
    from dvd_gan_amd.train_step import _PlateauLR, _StepLR
    opt = types.SimpleNamespace(param_groups=[{"lr": base}])
    if kind == "reduce":
        return _PlateauLR(opt, 0.5, base, patience=2), opt
    return _StepLR(opt, kind, base), opt


def _internal(s):
    return {k: v for k, v in vars(s).items() if k != "opt"}


@pytest.mark.parametrize("kind", ["const", "step", "exp", "multi", "reduce"])
def test_scheduler_continues(kind):
    n, k = 4, 6
    # 'reduce' (patience 2): the loss improves up to the save point and stalls after it -> one reduction at step n + 3
    losses = [1.0, 0.9, 0.8, 0.7] + [0.7] * k
    whole, opt = _sched(kind)
    want = []
    for i in range(n + k):
        whole.step(losses[i])
        want.append(opt.param_groups[0]["lr"])
    first, opt1 = _sched(kind)
    got = []
    for i in range(n):
        first.step(losses[i])
        got.append(opt1.param_groups[0]["lr"])
    sd = first.state_dict()
    second, opt2 = _sched(kind)                      # a fresh object over a fresh optimizer, at the base rate
    second.load_state_dict(sd)
    assert opt2.param_groups[0]["lr"] == want[n - 1]
    for i in range(n, n + k):
        second.step(losses[i])
        got.append(opt2.param_groups[0]["lr"])
    assert got == want
    assert _internal(second) == _internal(whole)
    if kind == "reduce":
        assert want[n - 1] == 1e-3 and want[n + 2] == 5e-4 and want[-1] < want[n - 1], want
    if kind == "exp":
        assert len(set(want)) == n + k
    other = "exp" if kind != "exp" else "step"
    with pytest.raises(ValueError, match="lr_schr"):
        _sched(other)[0].load_state_dict(sd)


# ------------------------------------------------------------------ FlatAdam
def _adam(seed=0, shapes=((3, 4), (5,), (2, 2, 3)), **kw):
    from dvd_gan_amd.optim import FlatAdam
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    return FlatAdam(params, 1e-3, **kw), params


def _fill(opt, seed):
    """Give every state tensor distinct values, as some steps would have left them (no kernel runs on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    n = opt.flat.numel()
    opt.m.copy_(torch.randn(n, generator=g))
    opt.v.copy_(torch.rand(n, generator=g))
    if opt.ema_decay:
        opt.load_ema(torch.randn(n, generator=g))
    if opt.guard:
        opt._alloc_guard()
        opt.guard_state.copy_(torch.rand(opt.guard_state.numel(), generator=g, dtype=torch.float64))
        if opt.guard_ring is not None:
            opt.guard_ring.copy_(torch.rand(opt.guard_ring.shape, generator=g, dtype=torch.float64))
    opt.t = 7
    opt.param_groups[0]["lr"] = 7.5e-4


FULL = dict(ema_decay=0.9, ema_start=3, clip_norm=1.0, skip_nonfinite=True, norm_log=4)


def test_flat_adam_state_round_trip():
    a, _ = _adam(0, **FULL)
    _fill(a, 1)
    sd = a.state_dict()
    assert sd["numel"] == 29 and sd["t"] == 7 and sd["lr"] == 7.5e-4 and sd["norm_log"] == 4 and sd["betas"] == [0.0, 0.9]
    a.m.zero_()                                         # state_dict() holds copies, not the live buffers
    assert sd["m"].abs().sum() > 0
    a.m.copy_(sd["m"])
    b, params = _adam(5, **FULL)
    ptrs = [(p.data_ptr(), p.grad.data_ptr()) for p in params]
    flat_ptr = b.flat.data_ptr()
    assert b.load_state_dict(sd) == []
    for k in ("flat", "m", "v", "ema", "guard_state", "guard_ring"):
        assert torch.equal(getattr(b, k), getattr(a, k)), k
        assert torch.equal(getattr(b, k), sd[k]), k
    assert b.t == 7 and b.param_groups[0]["lr"] == 7.5e-4 and b.guard_ws is not None
    # the parameters are still views of the same flat buffers, and they show the loaded weights
    assert b.flat.data_ptr() == flat_ptr
    off = 0
    for p, (dp, gp) in zip(params, ptrs):
        assert p.data_ptr() == dp == b.flat.data_ptr() + 4 * off and p.grad.data_ptr() == gp == b.grad.data_ptr() + 4 * off
        assert torch.equal(p.data.reshape(-1), a.flat[off:off + p.numel()])
        off += p.numel()
    again = b.state_dict()
    for k, v in sd.items():
        assert torch.equal(again[k], v) if isinstance(v, torch.Tensor) else again[k] == v, k


def test_flat_adam_state_before_first_step_and_plain():
    a, _ = _adam(0, **FULL)                              # nothing allocated yet: ema, guard tensors are None
    sd = a.state_dict()
    assert sd["ema"] is None and sd["guard_state"] is None and sd["guard_ring"] is None and sd["t"] == 0
    b, _ = _adam(1, **FULL)
    assert b.load_state_dict(sd) == [] and b.ema is None and b.guard_state is None and torch.equal(b.flat, a.flat)
    c, _ = _adam(0)                                      # the dvd_adam_step path: no average, no guard
    _fill(c, 2)
    d, _ = _adam(3)
    assert d.load_state_dict(c.state_dict()) == []
    assert torch.equal(d.m, c.m) and torch.equal(d.v, c.v) and torch.equal(d.flat, c.flat) and d.ema is None and d.guard_state is None


def test_flat_adam_snapshot_into():
    a, _ = _adam(0, **FULL)
    _fill(a, 1)
    n = a.flat.numel()
    assert a.snapshot_numel() == 4 * n
    slab = torch.full((4 * n + 3,), -1.0)
    assert a.snapshot_into(slab) == ["flat", "m", "v", "ema"]
    assert torch.equal(slab[:4 * n], torch.cat([a.flat, a.m, a.v, a.ema])) and bool((slab[4 * n:] == -1).all())
    b, _ = _adam(0)
    assert b.snapshot_numel() == 3 * n and b.snapshot_into(slab) == ["flat", "m", "v"]
    with pytest.raises(ValueError):
        a.snapshot_into(torch.empty(4 * n - 1))
    with pytest.raises(ValueError):
        a.snapshot_into(torch.empty(4 * n, dtype=torch.float64))


def test_flat_adam_state_mismatches_name_the_field():
    a, _ = _adam(0, **FULL)
    _fill(a, 1)
    sd = a.state_dict()
    with pytest.raises(ValueError, match="numel"):
        _adam(0, shapes=((3, 4), (6,), (2, 2, 3)), **FULL)[0].load_state_dict(sd)
    with pytest.raises(ValueError, match="norm_log"):
        _adam(0, **dict(FULL, norm_log=5))[0].load_state_dict(sd)
    with pytest.raises(ValueError, match="norm_log"):
        _adam(0, **dict(FULL, norm_log=0))[0].load_state_dict(sd)
    with pytest.raises(ValueError, match="ema"):                      # an average in the state, none kept here
        _adam(0, **dict(FULL, ema_decay=0.0))[0].load_state_dict(sd)
    plain, _ = _adam(0, **dict(FULL, ema_decay=0.0))
    _fill(plain, 1)
    with pytest.raises(ValueError, match="ema"):                      # none in the state, one kept here
        _adam(0, **FULL)[0].load_state_dict(plain.state_dict())
    stale = dict(sd, ema=None)
    with pytest.raises(ValueError, match="ema"):                      # seven steps old and the average is missing
        _adam(0, **FULL)[0].load_state_dict(stale)
    # settings that only steer future steps: the constructor's hold, the difference is reported
    b, _ = _adam(0, **dict(FULL, clip_norm=2.0, ema_start=9))
    b.lr = 3e-3
    notes = b.load_state_dict(sd)
    assert len(notes) == 2 and any(n.startswith("clip_norm") for n in notes) and any(n.startswith("ema_start") for n in notes)
    assert b.clip_norm == 2.0 and b.ema_start == 9 and torch.equal(b.m, a.m)


# ------------------------------------------------------------------ loader position
def _store(n_videos=7):
    """A CPU ClipStore over synthetic videos of different sizes and lengths (the layout of tests/test_gpu_clipstore.py::_store)."""
    from dvd_gan_amd import data as D
    rng = np.random.default_rng(0)
    videos = [rng.integers(0, 256, (9 + 2 * i, 20 + 3 * i, 31 - i, 3), dtype=np.uint8) for i in range(n_videos)]
    sizes = [v.size for v in videos]
    ids = torch.arange(n_videos)
    return D.ClipStore(blob=torch.from_numpy(np.concatenate([v.reshape(-1) for v in videos])),
                       video_offset=torch.tensor([sum(sizes[:i]) for i in range(n_videos)], dtype=torch.int64),
                       video_h=torch.tensor([v.shape[1] for v in videos], dtype=torch.int32),
                       video_w=torch.tensor([v.shape[2] for v in videos], dtype=torch.int32),
                       video_frames=torch.tensor([v.shape[0] for v in videos], dtype=torch.int32),
                       record_video=ids, record_label=ids % 3, record_first=torch.ones(n_videos, dtype=torch.int64),
                       record_last=torch.tensor([v.shape[0] for v in videos], dtype=torch.int64))


def _global_rng():
    return torch.get_rng_state(), random.getstate()


def _set_global_rng(state):
    torch.set_rng_state(state[0])
    random.setstate(state[1])


def _consume(loader, host_iter, epoch, it, n):
    """n more batches of `loader`, the way Trainer.train() walks it: set_epoch + a new iterator whenever one runs out."""
    out = []
    while len(out) < n:
        if it is None:
            loader.set_epoch(epoch)
            epoch += 1
            it = host_iter(loader)
        try:
            out.append(next(it))
        except StopIteration:
            it = None
    return out, epoch, it


STORE_MODES = [("shuffle", True, None), ("ordered", False, None), ("rank1of2", True, (1, 2)), ("rank1of2_ordered", False, (1, 2))]


@pytest.mark.parametrize("mode,shuffle,dist", STORE_MODES, ids=[m[0] for m in STORE_MODES])
def test_store_loader_continues_mid_epoch(mode, shuffle, dist):
    from dvd_gan_amd import data as D
    store = _store(17 if dist else 9)                 # 4 batches of 2 per epoch either way (rank 1 of 2 holds 8 of 17 records)

    def make():
        rank, world = dist or (None, None)
        return D.make_store_loader(store, 2, 4, 16, train_crop="random", shuffle=shuffle, rank=rank, world=world, seed=5)
    host = lambda loader: loader.plans()
    assert len(make()) == 4
    torch.manual_seed(11); random.seed(11)
    want, _, _ = _consume(make(), host, 0, None, 6)            # 1 1/2 epochs, never stopped
    torch.manual_seed(11); random.seed(11)
    first = make()
    got, epoch, it = _consume(first, host, 0, None, 3)         # 3/4 of an epoch
    sd, rng = first.state_dict(), _global_rng()
    assert sd["cursor"] == 3 and sd["epoch"] == 0 and len(sd["order"]) == 8 and sd["batch_size"] == 2
    assert all(type(i) is int for i in sd["order"])
    torch.manual_seed(99); random.seed(99); torch.randperm(5); random.random()          # another process, other streams
    second = make()
    second.load_state_dict(sd)
    _set_global_rng(rng)
    rest, epoch2, _ = _consume(second, host, 1, host(second), 3)      # the saved epoch continued, then the next one
    assert epoch2 == 2
    got += rest
    assert [g[0] for g in got] == [w[0] for w in want]                 # record ids
    for (_, (frames, boxes, flips, labels)), (_, (wf, wb, wfl, wl)) in zip(got, want):
        assert frames == wf and boxes == wb and flips == wfl and labels == wl
    if shuffle:
        assert [w[0] for w in want[:2]] != [w[0] for w in want[4:]]          # the two epochs' orders do differ
    # a state taken right at the end of an epoch: the continued iterator is empty and the next epoch is planned as usual
    third = make()
    _set_global_rng(rng)
    third.load_state_dict(dict(sd, cursor=4))
    assert list(third.plans()) == []
    with pytest.raises(ValueError, match="batch_size"):
        D.make_store_loader(store, 3, 4, 16).load_state_dict(sd)


class _Clips(torch.utils.data.Dataset):
    """What data.UCF101 hands a DataLoader -- (uint8 clip, flip flag, label) -- with its draws from Python's `random`."""

    def __len__(self):
        return 9

    def __getitem__(self, i):
        shift = random.randint(0, 100)
        return torch.full((2, 4, 4, 3), (i + shift) % 256, dtype=torch.uint8), torch.tensor(random.random() < 0.5), i


@pytest.mark.parametrize("shuffle,dist", [(True, None), (False, None), (True, (1, 2))])
def test_make_loader_continues_mid_epoch(shuffle, dist):
    from dvd_gan_amd import data as D
    rank, world = dist or (None, None)
    make = lambda: D.make_loader(_Clips(), 1 if dist else 2, num_workers=0, shuffle=shuffle, rank=rank, world=world, seed=5)
    host = lambda loader: loader.host_batches()
    assert len(make()) == 4
    torch.manual_seed(11); random.seed(11)
    want, _, _ = _consume(make(), host, 0, None, 6)
    tail = torch.rand(3)                                        # where the default generator stands after the whole run
    torch.manual_seed(11); random.seed(11)
    first = make()
    got, _, _ = _consume(first, host, 0, None, 3)
    sd, rng = first.state_dict(), _global_rng()
    torch.manual_seed(99); random.seed(99)
    second = make()
    second.load_state_dict(sd)
    _set_global_rng(rng)
    rest, _, _ = _consume(second, host, 1, host(second), 3)
    got += rest
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g, w))
    assert torch.equal(torch.rand(3), tail)                     # continuing drew nothing the uninterrupted run did not draw


# ------------------------------------------------------------------ the file
def _fingerprint(**over):
    from dvd_gan_amd.checkpoint import FINGERPRINT
    base = dict(g_chn=8, ds_chn=8, dt_chn=8, n_frames=8, n_cond=0, n_class=7, z_dim=120, latent_dim=4, g_self_attn=False,
                g_sep_attn=False, compute_dtype="torch.bfloat16", adv_loss="hinge", d_iters=1, k_sample=8, batch_size=2,
                world_size=1, dp_mode="replica")
    assert set(base) == set(FINGERPRINT)
    return dict(base, **over)


def test_atomic_save_leaves_the_previous_file(tmp_path):
    from dvd_gan_amd import checkpoint as C
    path = C.state_path(str(tmp_path), 4)
    assert os.path.basename(path) == "4_state.pt" and os.path.basename(C.state_path("x", 4, 1)) == "4_state.rank1.pt"

    def fail():
        raise OSError("the disk went away")
    with pytest.raises(OSError):
        C.atomic_save({"x": torch.ones(3)}, path, _before_replace=fail)
    assert not os.path.exists(path) and os.path.exists(path + ".tmp")        # nothing under the final name
    assert C.latest_state(str(tmp_path)) is None
    C.atomic_save({"x": torch.ones(3)}, path)
    assert not os.path.exists(path + ".tmp")
    with pytest.raises(OSError):
        C.atomic_save({"x": torch.zeros(3)}, path, _before_replace=fail)
    assert torch.equal(torch.load(path, weights_only=True)["x"], torch.ones(3))      # the earlier state is intact


def test_latest_and_pruning(tmp_path):
    from dvd_gan_amd import checkpoint as C
    folder = str(tmp_path)
    assert C.latest_state(os.path.join(folder, "nowhere")) is None
    names = ["2_state.pt", "10_state.pt", "9_state.pt", "9_state.rank0.pt", "9_state.rank1.pt", "2_state.rank1.pt",
             "12_state.pt.tmp", "12_state.rank0.pt", "10_G.pth", "2_G.pth", "2_G_ema.pth", "2_state.txt", "x2_state.pt"]
    for name in names:
        (tmp_path / name).write_bytes(b"0")
    assert C.latest_state(folder) == (10, os.path.join(folder, "10_state.pt"))       # not the .tmp of step 12, not "9" > "10"
    assert C.prune_states(folder, 0) == [] and sorted(os.listdir(folder)) == sorted(names)
    assert C.prune_states(folder, 2) == ["2_state.pt", "2_state.rank1.pt"]
    assert sorted(os.listdir(folder)) == sorted(set(names) - {"2_state.pt", "2_state.rank1.pt"})
    assert C.prune_states(folder, 1) == ["9_state.pt", "9_state.rank0.pt", "9_state.rank1.pt"]
    assert C.latest_state(folder) == (10, os.path.join(folder, "10_state.pt"))


def test_resume_setting_picks_the_file(tmp_path):
    from dvd_gan_amd.train_step import Trainer
    tr = Trainer.__new__(Trainer)                        # no GPU here: only the look-up
    tr.model_save_path = str(tmp_path)
    assert tr._resume_file() is None                     # unset
    tr.resume = "latest"
    assert tr._resume_file() is None                     # no complete state yet: start fresh
    for name in ("3_state.pt", "20_state.pt", "21_state.pt.tmp"):
        (tmp_path / name).write_bytes(b"0")
    assert tr._resume_file() == os.path.join(str(tmp_path), "20_state.pt")
    tr.resume = str(tmp_path / "3_state.pt")
    assert tr._resume_file() == str(tmp_path / "3_state.pt")


def test_state_writer_file_loads_weights_only_and_refuses(tmp_path):
    from dvd_gan_amd import checkpoint as C
    folder = str(tmp_path)
    opt, _ = _adam(0, **FULL)
    _fill(opt, 1)
    n = opt.flat.numel()
    counter = torch.tensor(5, dtype=torch.int64)
    torch.manual_seed(3); random.seed(3); np.random.seed(3)
    gen = torch.Generator().manual_seed(8)
    host = {"rng": C.host_rng_state((("noise_gen", gen), ("frame_gen", None))), "t": opt.t, "best": float("inf"),
            "loader": {"order": [3, 1, 2], "cursor": 1}}
    want_draws = (torch.rand(2), random.random(), np.random.rand(), torch.rand(2, generator=gen))
    items = [("opt.slab", torch.float32, (opt.snapshot_numel(),), opt.snapshot_into),
             ("guard_ring", torch.float64, (4, 4), lambda dst: dst.copy_(opt.guard_ring)),
             ("counter", torch.int64, (), lambda dst: dst.copy_(counter))]

    def make_file(version):
        def make(tensors):
            slab = tensors.pop("opt.slab")
            for i, k in enumerate(("flat", "m", "v", "ema")):
                tensors["opt." + k] = slab[i * n:(i + 1) * n]
            return {"format_version": version, "step": 6, "fingerprint": _fingerprint(), "tensors": tensors, "host": host}
        return make
    w = C.StateWriter()
    w.submit(C.state_path(folder, 6), items, make_file(C.FORMAT_VERSION), device="cpu", after=lambda: C.prune_states(folder, 1))
    opt.m.zero_(); counter.zero_()                       # the live tensors move on while the file is written
    w.submit(C.state_path(folder, 8), items, make_file(C.FORMAT_VERSION + 1), device="cpu", wait=True)
    sd = C.load_file(C.state_path(folder, 6))            # torch.load(weights_only=True) inside
    assert sd["step"] == 6 and sd["host"]["loader"] == {"order": [3, 1, 2], "cursor": 1} and sd["host"]["best"] == float("inf")
    T = sd["tensors"]
    assert torch.equal(T["opt.flat"], opt.flat) and torch.equal(T["opt.v"], opt.v) and torch.equal(T["opt.ema"], opt.ema)
    assert T["opt.m"].abs().sum() > 0 and int(T["counter"]) == 5 and T["counter"].dtype == torch.int64
    assert torch.equal(T["guard_ring"], opt.guard_ring)
    torch.manual_seed(77); random.seed(77); np.random.seed(77)
    other = torch.Generator().manual_seed(1)
    C.set_host_rng_state(sd["host"]["rng"], (("noise_gen", other), ("frame_gen", None)))
    got = (torch.rand(2), random.random(), np.random.rand(), torch.rand(2, generator=other))
    assert torch.equal(got[0], want_draws[0]) and got[1:3] == want_draws[1:3] and torch.equal(got[3], want_draws[3])
    with pytest.raises(ValueError, match="format_version"):
        C.load_file(C.state_path(folder, 8))
    # a worker's exception surfaces at the next submit() or at close()
    w.submit(os.path.join(folder, "missing", "9_state.pt"), items, make_file(C.FORMAT_VERSION), device="cpu")
    with pytest.raises(OSError):
        w.close()
    w.close()
    for k in C.FINGERPRINT:
        changed = _fingerprint(**{k: "other"})
        with pytest.raises(ValueError, match="^" + k + ":"):
            C.check_fingerprint(sd["fingerprint"], changed)
    C.check_fingerprint(sd["fingerprint"], _fingerprint())
    with pytest.raises(ValueError, match="^g_chn:"):                   # the FIRST differing field
        C.check_fingerprint(sd["fingerprint"], _fingerprint(g_chn=16, n_class=3))

"""Exact resume on the GPU: a run that is saved, stopped and continued is BIT-EQUAL to the run that was never
stopped -- FlatAdam alone, the whole Trainer through an asynchronous save_state() with the training loop running on behind it,
and Trainer.train() end to end with config.state_save_step / config.resume.  The weights-only path (save_models +
pretrained_model) is shown not to be enough, and unchanged."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _seed(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


# ------------------------------------------------------------------ FlatAdam
GUARDED = dict(ema_decay=0.9, ema_start=3, clip_norm=1.0, skip_nonfinite=True, norm_log=4)


def _adam_run(grads, first, last, kw, state=None, seed=0):
    """Steps first..last (1-based) of a FlatAdam over one fresh parameter; `state`: continue from that state_dict()."""
    from dvd_gan_amd.optim import FlatAdam
    g = torch.Generator().manual_seed(seed)
    p = torch.nn.Parameter(torch.randn(grads[0].numel(), generator=g).to(DEV))
    opt = FlatAdam([p], 2e-3, **kw)
    if state is not None:
        assert opt.load_state_dict(state) == []
        assert p.data_ptr() == opt.flat.data_ptr() and p.grad.data_ptr() == opt.grad.data_ptr()
    for s in range(first, last + 1):
        opt.grad.copy_(grads[s - 1])
        opt.step()
    return opt


@pytest.mark.parametrize("kw", [GUARDED, {}], ids=["guard_ema", "plain"])
def test_flat_adam_continues_bitwise(kw):
    """3 + 3 steps against 6: across ema_start = 3, a wrap of the 4-row norm log, a skipped step (NaN, step 2) before the save
    and a clipped one (step 5) after it; n = three guard chunks and a ragged tail."""
    from dvd_gan_amd import kern as K
    n = 3 * K.GUARD_CH + 5
    g = torch.Generator().manual_seed(21)
    grads = [torch.randn(n, generator=g) * 1e-3 for _ in range(6)]            # norm ~0.22: under clip_norm = 1
    grads[4] *= 100.0                                                         # step 5: norm ~22, clipped
    if kw:
        grads[1][n // 2] = float("nan")                                       # step 2: skipped
    grads = [t.to(DEV) for t in grads]
    a = _adam_run(grads, 1, 6, kw)
    b1 = _adam_run(grads, 1, 3, kw)
    b = _adam_run(grads, 4, 6, kw, state=b1.state_dict(), seed=9)            # fresh parameters, other values
    names = ("flat", "m", "v") + (("ema", "guard_state", "guard_ring") if kw else ())
    for k in names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.t == b.t == 6 and (b.ema is None) == (not kw) and (b.guard_state is None) == (not kw)
    assert not torch.equal(a.flat, b1.flat)
    if kw:
        rep = b.guard_report()
        assert rep["seen"] == 6 and rep["skipped"] == 1 and rep["clipped"] == 1, rep
        assert [int(r[0]) for r in rep["ring"]] == [3, 4, 5, 6] and rep["ring"][2][2] < 1.0, rep


# ------------------------------------------------------------------ Trainer
def _config(folder, **over):
    """tools/repro_probe.build's shape (hinge, T = 8, B = 2, 64 x 64, 7 classes, 8 sampled frames) with everything that carries
    state from step to step switched on: a schedule that moves, the weight average, the guard with its log, the regularizer.
    ch = 32, the width tests/test_gpu_trainer.py::test_bf16_step_is_bitwise_reproducible pins: at ch = 8 the step is not
    reproducible from run to run (the discriminators' attention has 4 query channels there and takes the fp32 kernels; two
    identical 4-step runs differed in 29 tensors, D_s's attn.gamma / query / key / value weights and biases and their Adam
    moments first), so nothing could be compared bitwise.  The state file is 2.4 GB at this width."""
    cfg = dict(adv_loss="hinge", z_dim=120, g_chn=32, ds_chn=32, dt_chn=32, n_frames=8, lr_schr="exp", total_epoch=1, d_iters=1,
               batch_size=2, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9, n_class=7, k_sample=8, ema_decay=0.99, g_clip_norm=10.0,
               skip_nonfinite=True, grad_log=4, g_ortho=1e-4, model_save_path=str(folder), version="", log_epoch=0)
    cfg.update(over)
    return argparse.Namespace(**cfg)


def _trainer(folder, loader=(), **over):
    from dvd_gan_amd.train_step import Trainer
    return Trainer(loader, _config(folder, **over), device=DEV, compute_dtype=torch.bfloat16)


def _clips(steps=4):
    """The real clips and labels of every step, from a private generator (z, labels and frame ids come from the global ones)."""
    g = torch.Generator().manual_seed(11)
    return [(torch.rand(2, 3, 8, 64, 64, generator=g) * 2 - 1, torch.randint(0, 7, (2,), generator=g)) for _ in range(steps)]


def _state(tr):
    """Every tensor a step leaves for the next, by name, and the host-side scalars.  The optimizers' m / v / ema are listed per
    parameter, so that a mismatch names the layer."""
    tensors, scalars = {}, {}
    for (tag, net), (_, opt), (_, sched) in zip(tr._nets(), tr._optimizers(), tr._schedulers()):
        for k, v in net.state_dict().items():
            tensors[f"{tag}.{k}"] = v.detach().clone()
        off = 0
        for k, p in net.named_parameters():
            if p.requires_grad:
                for part in ("m", "v") + (("ema",) if opt.ema is not None else ()):
                    tensors[f"{tag}.{part}.{k}"] = getattr(opt, part)[off:off + p.numel()].clone()
                off += p.numel()
        assert off == opt.flat.numel()
        for part in ("guard_state", "guard_ring"):          # (`flat` is the trained entries of state_dict(), listed above)
            if getattr(opt, part) is not None:
                tensors[f"{tag}.opt.{part}"] = getattr(opt, part).clone()
        scalars[f"{tag}.t"], scalars[f"{tag}.lr"], scalars[f"{tag}.sched"] = opt.t, opt.param_groups[0]["lr"], sched.state_dict()
    return tensors, scalars


def _run(folder, clips, first, last, tr=None):
    tr = tr if tr is not None else _trainer(folder)
    losses = [tr.train_step(*clips[s - 1]) for s in range(first, last + 1)]
    return tr, losses


def _result(tr, losses):
    tensors, scalars = _state(tr)
    for i, step in enumerate(losses[-2:]):
        for name, v in zip(("ds_real", "ds_fake", "dt_real", "dt_fake", "g_s", "g_t"), step):
            tensors[f"loss.{i}.{name}"] = v.detach().clone()
    return tensors, scalars


def _differing(a, b):
    assert set(a) == set(b)
    # bit-equal: same dtype and shape, and equal bytes (so that a NaN equals itself and -0.0 differs from 0.0)
    return [k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
            or not torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8))]


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """Run A: 4 uninterrupted steps from seed 3.  -> (tensors, scalars, the global random streams as step 2 left them)."""
    from dvd_gan_amd.checkpoint import host_rng_state
    clips = _clips()
    _seed(3)
    tr, first = _run(tmp_path_factory.mktemp("a"), clips, 1, 2)
    rng = host_rng_state()
    _, rest = _run(None, clips, 3, 4, tr)
    return _result(tr, first + rest) + (rng,)


def test_trainer_continues_bitwise_through_async_save(run_a, tmp_path):
    """The acceptance test.  (A) 4 steps; (A') 4 steps again, the control; (B) 2 steps, save_state(2, wait=False), then -- with no
    synchronisation whatever -- steps 3 and 4 on the same Trainer, which overwrite every live buffer while the snapshot is still
    in flight, close_state(), other seeds, a fresh Trainer, load_state(), steps 3 and 4.  B == A bit for bit."""
    clips = _clips()
    want_t, want_s, _ = run_a
    _seed(3)
    ctl_t, ctl_s = _result(*_run(tmp_path, clips, 1, 4))
    bad = _differing(want_t, ctl_t)
    assert not bad and ctl_s == want_s, f"the step is not reproducible at this width: {len(bad)} tensors differ, {bad[:40]}"

    _seed(3)
    tr, _ = _run(tmp_path, clips, 1, 2)
    tr.save_state(2, wait=False)
    _run(None, clips, 3, 4, tr)                          # discarded: they only race the snapshot
    tr.close_state()
    path = os.path.join(str(tmp_path), "2_state.pt")
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    del tr
    _seed(1234); torch.rand(7); random.random(); np.random.rand()
    fresh = _trainer(tmp_path)                           # another initialisation altogether
    assert fresh.g_optimizer.ema is None and fresh.g_optimizer.guard_state is None
    assert fresh.load_state(path) == []
    got_t, got_s = _result(*_run(None, clips, 3, 4, fresh))
    assert len(want_t) >= 600, len(want_t)               # an empty comparison cannot pass
    bad = _differing(want_t, got_t)
    assert not bad, f"{len(bad)} of {len(want_t)} tensors differ after the resume: {bad[:10]}"
    assert got_s == want_s
    assert want_s["G.t"] == 4 and want_s["G.sched"]["n"] == 4 and want_s["G.lr"] == 5e-5 * 0.9999 ** 4


def test_weights_only_resume_is_not_enough(run_a, tmp_path):
    """The existing path -- save_models + pretrained_model -- continued with the very same inputs and random streams: step 3's
    discriminator losses still agree (same weights, same draws), the generator losses do not (they pass through discriminators
    updated by an Adam whose m, v, t and learning rate started over).  What exact resume fixes; and that path is unchanged."""
    from dvd_gan_amd.checkpoint import set_host_rng_state
    clips = _clips()
    want_t, _, rng = run_a
    _seed(3)
    tr, _ = _run(tmp_path, clips, 1, 2)
    tr.save_models(2)
    assert sorted(os.listdir(tmp_path)) == ["2_Ds.pth", "2_Dt.pth", "2_G.pth", "2_G_ema.pth"]
    del tr
    _seed(1234)
    again = _trainer(tmp_path, pretrained_model=2)
    assert again.g_optimizer.t == 0 and again.g_lr_scher.n == 0
    set_host_rng_state(rng)
    # run A's last two steps are 3 and 4: "loss.0.*" is step 3
    got = dict(zip(("ds_real", "ds_fake", "dt_real", "dt_fake", "g_s", "g_t"), again.train_step(*clips[2])))
    differ = [k for k, v in got.items() if not torch.equal(v.detach(), want_t[f"loss.0.{k}"])]
    assert "g_s" in differ and "g_t" in differ, differ


# ------------------------------------------------------------------ Trainer.train()
def _store_loader():
    """3 batches of 2 per epoch over 6 synthetic videos on the device (the layout of tests/test_gpu_clipstore.py::_store)."""
    from dvd_gan_amd import data as D
    rng = np.random.default_rng(2)
    videos = [rng.integers(0, 256, (10 + i, 72 + 4 * i, 90 - 2 * i, 3), dtype=np.uint8) for i in range(6)]
    sizes = [v.size for v in videos]
    ids = torch.arange(6)
    store = D.ClipStore(blob=torch.from_numpy(np.concatenate([v.reshape(-1) for v in videos])).to(DEV),
                        video_offset=torch.tensor([sum(sizes[:i]) for i in range(6)], dtype=torch.int64),
                        video_h=torch.tensor([v.shape[1] for v in videos], dtype=torch.int32),
                        video_w=torch.tensor([v.shape[2] for v in videos], dtype=torch.int32),
                        video_frames=torch.tensor([v.shape[0] for v in videos], dtype=torch.int32),
                        record_video=ids, record_label=ids, record_first=torch.ones(6, dtype=torch.int64),
                        record_last=torch.tensor([v.shape[0] for v in videos], dtype=torch.int64))
    return D.make_store_loader(store, 2, 8, 64, train_crop="random", shuffle=True)


def test_train_resumes_from_latest(tmp_path):
    """train() over 2 epochs of 3 steps with a state every 2 steps, against the same run stopped by an exception right after the
    save at step 4 was issued and continued by a fresh Trainer with resume="latest": the final state is bit-equal.
    Six state files are written here, so the generator is narrow (g_chn = 8: 0.4 GB a file instead of 2.4); the discriminators
    keep ch = 32, where their attention runs the reproducible kernels (_config)."""
    over = dict(total_epoch=2, state_save_step=2, g_chn=8)
    whole, cut = tmp_path / "whole", tmp_path / "cut"
    _seed(5)
    tr = _trainer(whole, _store_loader(), **over)
    tr.train()
    want_t, want_s = _state(tr)
    assert tr._state_writer is None and sorted(os.listdir(whole)) == ["4_state.pt", "6_state.pt"]       # state_keep = 2
    del tr

    _seed(5)
    tr = _trainer(cut, _store_loader(), **over)
    step, calls = tr.train_step, []

    def stops(*args, **kw):
        calls.append(1)
        if len(calls) == 5:                              # the call for step 5: the save at step 4 has just been issued
            raise RuntimeError("stopped here")
        return step(*args, **kw)
    tr.train_step = stops
    with pytest.raises(RuntimeError, match="stopped here"):
        tr.train()
    assert tr._state_writer is None and sorted(os.listdir(cut)) == ["2_state.pt", "4_state.pt"]          # complete, no .tmp
    del tr
    _seed(77); torch.rand(3); random.random()
    tr = _trainer(cut, _store_loader(), resume="latest", **over)
    tr.train()
    assert tr._resumed_step == 4 and sorted(os.listdir(cut)) == ["4_state.pt", "6_state.pt"]
    got_t, got_s = _state(tr)
    bad = _differing(want_t, got_t)
    assert len(want_t) >= 600 and not bad, f"{len(bad)} of {len(want_t)} tensors differ: {bad[:10]}"
    assert got_s == want_s and got_s["G.t"] == 6
    with pytest.raises(ValueError, match="resume"):
        _trainer(cut, resume="latest", pretrained_model=4)
    # the file: plain enough for weights_only=True, and refused by a Trainer that differs in a fingerprint field
    sd = torch.load(cut / "6_state.pt", map_location="cpu", weights_only=True)
    assert sd["step"] == 6 and sd["host"]["opt"]["G"]["t"] == 6 and sd["host"]["epoch"] == 2 and "opt.G.ema" in sd["tensors"]
    assert sd["host"]["loader"]["cursor"] == 3 and len(sd["host"]["loader"]["order"]) == 6
    tr.k_sample = 4
    with pytest.raises(ValueError, match="^k_sample:"):
        tr.load_state(str(cut / "6_state.pt"))

"""Trainer.evaluate_classes on the device at smoke()'s size (ch = 2, T = 8, 64 x 64) with 4 classes: 6 samples in batches of 4 + 2
and 3 splits, under a classifier written with torch here that records the logits it returns -- the result must be the numpy
restatement (tests/cls_ref.py) of exactly those logits and the labels the generator was given; the default labels, the `real=`
path, the refusals, and the no-trace contract of evaluate_samples."""
import argparse
import random

import numpy as np
import pytest
import torch

import cls_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH, T, KS, B, NCLS, ZD = 2, 8, 4, 2, 4, 16
KEYS = ("is_mean", "is_std", "is_all", "h_marginal", "h_conditional", "top1", "top5", "mean_log_lik")


def _cfg(**extra):
    return argparse.Namespace(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=B, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9,
                              n_class=NCLS, k_sample=KS, **extra)


def _trainer(seed):
    from dvd_gan_amd.train_step import Trainer
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    return Trainer([], _cfg(), device=torch.device(DEV), compute_dtype=torch.float32)


def _clips(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, T, 64, 64, generator=gen) * 2 - 1, torch.randint(0, NCLS, (n,), generator=gen)


@pytest.fixture(scope="module")
def trainer():
    return _trainer(3)


class _Classifier:
    """A fixed seeded linear map of the spatially pooled clip, [B, 3, T, H, W] -> [B, n_classes]; keeps what it returned."""

    def __init__(self, n_classes, seed=5, dtype=torch.float32):
        gen = torch.Generator().manual_seed(seed)
        self.w = (2.0 * torch.randn(3 * T, n_classes, generator=gen)).to(DEV)
        self.dtype, self.seen = dtype, []

    def __call__(self, clips):
        assert clips.is_cuda and clips.dtype == torch.float32 and clips.dim() == 5 and tuple(clips.shape[1:]) == (3, T, 64, 64)
        assert float(clips.min()) >= -1.0 and float(clips.max()) <= 1.0
        logits = (clips.mean(dim=(3, 4)).reshape(clips.shape[0], -1) @ self.w).to(self.dtype)
        self.seen.append(logits.detach().float().cpu().numpy())
        return logits


class _SpyOnG:
    """Records the labels every generator call receives while the block is open."""

    def __init__(self, tr):
        self.tr, self.labels = tr, []

    def __enter__(self):
        self.hook = self.tr.G.register_forward_pre_hook(lambda mod, args: self.labels.append(args[1].detach().cpu()))
        return self

    def __exit__(self, *exc):
        self.hook.remove()


def _compare(res, logits, labels, *, splits, confusion, prefix=""):
    ref = R.metrics(logits, labels, splits=splits, confusion=confusion)
    for key in KEYS:
        if key in ref:
            np.testing.assert_allclose(res[prefix + key], ref[key], rtol=1e-9, atol=1e-11 * ref["is_mean"] if key == "is_std" else 0,
                                       err_msg=prefix + key)
    assert (res[prefix + "n"], res[prefix + "n_bad"], res[prefix + "n_bad_label"]) == (ref["n"], ref["n_bad"], ref["n_bad_label"])
    if confusion:
        assert np.array_equal(res[prefix + "confusion"], ref["confusion"])
        np.testing.assert_array_equal(res[prefix + "per_class_top1"], ref["per_class_top1"])
    else:
        assert res[prefix + "confusion"] is None
    return ref


def test_generated_clips_with_the_balanced_default_labels(trainer):
    clf = _Classifier(NCLS)
    with _SpyOnG(trainer) as spy:
        res = trainer.evaluate_classes(clf, n_samples=6, batch=4, splits=3, confusion=True, seed=1)
    assert [tuple(y.shape) for y in spy.labels] == [(4,), (2,)]                     # an uneven last batch
    used = torch.cat(spy.labels).numpy()
    assert used.tolist() == [0, 1, 2, 3, 0, 1]                                      # arange(n_samples) % n_class
    # the classifier was asked once for its width on one all-zero clip, then once per batch
    assert [s.shape for s in clf.seen] == [(1, NCLS), (4, NCLS), (2, NCLS)] and not np.any(clf.seen[0])
    ref = _compare(res, np.concatenate(clf.seen[1:]), used, splits=3, confusion=True)
    assert res["n_classes"] == NCLS and res["n"] == 6 and not [k for k in res if k.startswith("real_")]
    assert ref["confusion"].sum() == 6 and 1.0 - 1e-12 <= res["is_mean"] <= NCLS
    # one seed: the same clips, so the same bits; another seed: other z
    clf2, clf3 = _Classifier(NCLS), _Classifier(NCLS)
    again = trainer.evaluate_classes(clf2, n_samples=6, batch=4, splits=3, confusion=True, seed=1)
    other = trainer.evaluate_classes(clf3, n_samples=6, batch=4, splits=3, confusion=True, seed=2)
    assert all(again[k] == res[k] for k in KEYS) and np.array_equal(again["confusion"], res["confusion"])
    assert not np.array_equal(np.concatenate(clf3.seen[1:]), np.concatenate(clf.seen[1:])) and other["n"] == 6
    # explicit labels win; half-precision logits are scored as stored
    clf4 = _Classifier(NCLS, dtype=torch.bfloat16)
    mine = torch.tensor([3, 3, 2, 2, 1, 0])
    with _SpyOnG(trainer) as spy:
        res4 = trainer.evaluate_classes(clf4, n_samples=6, labels=mine, batch=4, splits=3, seed=1)
    assert torch.equal(torch.cat(spy.labels), mine)
    _compare(res4, np.concatenate(clf4.seen[1:]), mine.numpy(), splits=3, confusion=False)


def test_real_clips_give_the_labels_and_the_ceiling(trainer):
    clips, labels = _clips(8, 6)
    real = [(clips[:4], labels[:4]), (clips[4:], labels[4:])]
    clf = _Classifier(NCLS)
    with _SpyOnG(trainer) as spy:
        res = trainer.evaluate_classes(clf, n_samples=6, real=real, batch=4, splits=3, confusion=True, seed=1)
    # the first 6 real clips in batches of 4 + 2, then the generated ones; no call to learn the width
    assert [s.shape[0] for s in clf.seen] == [4, 2, 4, 2]
    assert torch.equal(torch.cat(spy.labels), labels[:6])
    host = (clips[:6].mean(dim=(3, 4)).reshape(6, -1).double() @ clf.w.cpu().double()).numpy()
    np.testing.assert_allclose(np.concatenate(clf.seen[:2]), host, rtol=1e-4, atol=1e-3)       # the real clips went in as they are
    _compare(res, np.concatenate(clf.seen[:2]), labels[:6].numpy(), splits=3, confusion=True, prefix="real_")
    _compare(res, np.concatenate(clf.seen[2:]), labels[:6].numpy(), splits=3, confusion=True)
    assert res["n_classes"] == NCLS and res["real_n"] == 6
    with pytest.raises(ValueError, match="delivered 4 clips"):
        trainer.evaluate_classes(_Classifier(NCLS), n_samples=6, real=real[:1], batch=4, splits=3)


def test_refusals_come_before_any_generation(trainer):
    three = _Classifier(3)
    gen_state, default_state = trainer.noise_gen.get_state() if isinstance(trainer.noise_gen, torch.Generator) else None, torch.get_rng_state()
    with _SpyOnG(trainer) as spy:
        with pytest.raises(ValueError, match="fidelity=True: class id 3 has no logit among the classifier's 3"):
            trainer.evaluate_classes(three, n_samples=6, batch=4, splits=3)
        clips, labels = _clips(6, 8)
        labels[5] = 3
        with pytest.raises(ValueError, match="fidelity=True"):
            trainer.evaluate_classes(three, n_samples=6, real=[(clips, labels)], batch=4, splits=3)
        assert not spy.labels                                                       # the generator never ran
        for kw in (dict(n_samples=0), dict(n_samples=6, splits=7), dict(n_samples=6, splits=0), dict(n_samples=6, batch=0),
                   dict(n_samples=6, fidelity=False, confusion=True), dict(n_samples=6, labels=torch.zeros(5, dtype=torch.long))):
            with pytest.raises(ValueError):
                trainer.evaluate_classes(three, **kw)
        with pytest.raises(IndexError, match="class id out of range"):
            trainer.evaluate_classes(three, n_samples=2, labels=torch.tensor([0, NCLS]), splits=1)
        assert not spy.labels
        # the same classifier over another label set: the score alone
        three.seen.clear()
        res = trainer.evaluate_classes(three, n_samples=6, batch=4, splits=3, fidelity=False, seed=1)
    assert [s.shape for s in three.seen] == [(4, 3), (2, 3)] and res["n_classes"] == 3 and "top1" not in res
    _compare(res, np.concatenate(three.seen), None, splits=3, confusion=False)
    assert torch.equal(torch.get_rng_state(), default_state)
    if gen_state is not None:
        assert torch.equal(trainer.noise_gen.get_state(), gen_state)


def test_a_frame_conditional_trainer_is_refused():
    from dvd_gan_amd.train_step import Trainer
    tr = Trainer([], _cfg(n_cond=4), device=torch.device("cpu"), compute_dtype=torch.float32)
    with pytest.raises(RuntimeError, match=r"evaluate_classes\(\) measures generation from noise \(n_cond = 0\)"):
        tr.evaluate_classes(lambda clips: None, n_samples=6)


def _everything(tr):
    out = {}
    for tag, net, opt in (("G", tr.G, tr.g_optimizer), ("Ds", tr.D_s, tr.ds_optimizer), ("Dt", tr.D_t, tr.dt_optimizer)):
        for k, v in net.state_dict().items():                 # weights, spectral-norm u / v, batch-norm running statistics
            out[f"{tag}.{k}"] = v.detach().clone()
        for k in ("flat", "m", "v"):
            out[f"{tag}.opt.{k}"] = getattr(opt, k).detach().clone()
    out["rng.torch"] = torch.get_rng_state()
    out["rng.numpy"] = torch.from_numpy(np.random.get_state()[1].astype(np.int64))
    out["rng.python"] = torch.tensor(random.getstate()[1], dtype=torch.int64)
    for name in ("noise_gen", "frame_gen"):
        g = getattr(tr, name, None)
        if isinstance(g, torch.Generator):
            out["rng." + name] = g.get_state()
    return out


def test_a_training_step_does_not_notice_an_evaluation():
    """Weights, u / v of all three networks, batch-norm statistics, Adam state and the torch / numpy / python / noise_gen random
    streams are bit-equal before and after evaluate_classes -- with a SHUFFLING loader as `real` (iterating it draws from torch's
    default generator) and without -- and two Trainers from one seed, one of which evaluated, take the same step."""
    clips, labels = _clips(8, 9)
    step_clips, step_labels = _clips(B, 10)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(clips, labels), batch_size=4, shuffle=True)
    runs = []
    for evaluate in (False, True):
        tr = _trainer(21)
        if evaluate:
            before = _everything(tr)
            res = tr.evaluate_classes(_Classifier(NCLS), n_samples=6, real=loader, batch=4, splits=3, confusion=True)
            assert np.isfinite(res["is_mean"]) and np.isfinite(res["real_is_mean"])
            res = tr.evaluate_classes(_Classifier(NCLS), n_samples=6, batch=4, splits=3, truncation=1.0)
            assert np.isfinite(res["is_mean"])
            torch.cuda.synchronize()
            after = _everything(tr)
            assert set(before) == set(after)
            differing = [k for k in before if not torch.equal(before[k], after[k])]
            assert not differing, differing
        losses = [float(v.detach()) for v in tr.train_step(step_clips, step_labels)]
        torch.cuda.synchronize()
        runs.append((losses, _everything(tr)))
    (la, sa), (lb, sb) = runs
    assert la == lb, (la, lb)
    assert set(sa) == set(sb)
    differing = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not differing, differing

"""Distribution distances on the GPU (libdvdgan_hip_eval.so, dvd_gan_amd/distmetrics.py, Trainer.evaluate_samples).

Every reference is numpy / torch fp64 on the SAME stored fp32 (bf16) inputs, every tolerance is derived from the number formats
(tests/distmetrics_ref.py says how) and computed here for the inputs at hand; figures are printed before they are asserted
("[distmetrics] ...", pytest -s).
  moments   S1 / S2 / pivot / mean against fp64: d in {1, 33, 70, 128} (below one tile, ragged edge tiles, a diagonal plus an
            off-diagonal tile) x n in {1, 37, 130} (one row, a ragged slab, more than one slab of 32 rows); a strided view; three
            unequal updates against one pass; features with mean 100 (cov to 1e-4 relative Frobenius); bit-equal reruns.
  kid       against the fp64 restatement: the three sizes of the issue, overlapping subsets, identical tables (the diagonal
            rule), a strided operand, bit-equal reruns.
  pool      against torch fp64 on the stored activation, bf16 and fp32, vector and scalar path.
  Trainer   evaluate_samples with a stub generator that returns the real clips (fd against 0, kid against fp64), the built-in
            "Dt" / "Ds" extractors, bit-equal repeats, and a training step after an evaluation against the same step without it."""
import argparse
import random

import numpy as np
import pytest
import torch

import distmetrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _features(n, d, seed, mean=0.0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=gen) * scale + mean).to(torch.float32)


def _run_moments(batches):
    """FeatureStats over the device copies of `batches` (host fp32 tensors or views) -> (stats, pivot, S1, S2) fp64 numpy."""
    from dvd_gan_amd.distmetrics import FeatureStats
    st = FeatureStats(batches[0].shape[1], DEV)
    for b in batches:
        st.update(b)
    return (st,) + st._host()


def _check_moments(tag, host_batches, got):
    st, pivot, s1, s2 = got
    xs = [b.numpy() for b in host_batches]
    want_pivot, tol_pivot = R.pivot_tolerance(xs[0])
    assert np.all(np.abs(pivot - want_pivot) <= tol_pivot), tag
    r1, r2, b1, b2 = R.moments_ref(xs, pivot)
    e1, e2 = np.abs(s1 - r1), np.abs(s2 - r2)
    print(f"[distmetrics] moments {tag}: max S2 err / bound {np.max(e2 / b2):.3f}, max S1 err / bound {np.max(e1 / b1):.3f}")
    assert np.all(e2 <= b2), tag
    assert np.all(e1 <= b1), tag
    assert np.array_equal(s2, s2.T)
    allx = np.concatenate(xs).astype(np.float64)
    n = allx.shape[0]
    assert st.n == n
    # mean = pivot + S1 / n: the error of S1 over n, plus fp64 noise on values of the size of the mean
    assert np.all(np.abs(st.mean() - allx.mean(0)) <= b1 / n + 2.0 ** -50 * np.abs(allx.mean(0))), tag
    if n < 2:
        return None, None
    want = np.cov(allx, rowvar=False).reshape(len(pivot), len(pivot))
    tol = R.cov_tolerance(r1, b1, b2, n, want)
    ec = np.abs(st.cov() - want)
    print(f"[distmetrics] moments {tag}: max cov err / bound {np.max(ec / tol):.3f}")
    assert np.all(ec <= tol), tag
    return want, tol


@pytest.mark.parametrize("d", [1, 33, 70, 128])
@pytest.mark.parametrize("n", [1, 37, 130])
def test_moments_against_fp64(n, d):
    x = _features(n, d, 100 * n + d, mean=0.5)
    _check_moments(f"n={n} d={d}", [x], _run_moments([x.to(DEV)]))


def test_moments_strided_view():
    n, d = 37, 70
    wide = _features(n, d + 3, 5, mean=-1.0)
    view = wide.to(DEV)[:, :d]
    assert view.stride(0) == d + 3
    got = _run_moments([view])
    _check_moments("strided", [wide[:, :d]], got)
    # the same rows from a dense copy: the same bits
    dense = _run_moments([wide[:, :d].contiguous().to(DEV)])
    assert np.array_equal(got[2], dense[2]) and np.array_equal(got[3], dense[3])


def test_moments_three_unequal_updates():
    d = 70
    parts = [_features(n, d, 30 + n, mean=2.0) for n in (130, 1, 37)]
    got = _run_moments([p.to(DEV) for p in parts])
    _check_moments("three updates", parts, got)          # S1, S2, mean and cov against ONE fp64 pass over the concatenation


def test_moments_far_from_zero():
    """Mean 100, unit spread: x^T x sums products near 1e4 whose fp32 rounding (6e-4 each) buries a covariance of order one; about
    the pivot the products are of order one.  The elementwise bound of cov() (distmetrics_ref.cov_tolerance: the S2 bound over
    n - 1 plus the S1 term), evaluated for this input, is below 1e-4 of the covariance in the Frobenius norm: that is asserted
    first, so the 1e-4 after it follows from the derived bound and is no figure of its own."""
    n, d = 130, 70
    x = _features(n, d, 77, mean=100.0)
    got = _run_moments([x.to(DEV)])
    want, tol = _check_moments("mean 100", [x], got)
    bound = np.linalg.norm(tol) / np.linalg.norm(want)
    err = np.linalg.norm(got[0].cov() - want) / np.linalg.norm(want)
    x32 = x.numpy()
    naive = (x32.T @ x32 - n * np.outer(x32.mean(0), x32.mean(0))) / (n - 1)             # fp32 throughout, no pivot
    print(f"[distmetrics] mean 100: cov relative Frobenius error {err:.3e}, bound {bound:.3e}; pivot-free fp32 "
          f"{np.linalg.norm(naive - want) / np.linalg.norm(want):.3e}")
    assert bound <= 1e-4            # the justification: the derived bound itself is below the issue's figure for this input
    assert err <= 1e-4


def test_moments_state_round_trip_and_rerun_bit_equal():
    from dvd_gan_amd.distmetrics import FeatureStats
    parts = [_features(n, 33, 60 + n).to(DEV) for n in (37, 130)]
    a, b = _run_moments(parts), _run_moments(parts)
    assert torch.equal(a[0]._state, b[0]._state) and torch.equal(a[0]._pivot, b[0]._pivot)
    # the running state moves to another object and goes on accumulating there, bit for bit
    half = FeatureStats(33, DEV).update(parts[0])
    moved = FeatureStats(33, DEV).load_state_dict(half.state_dict()).update(parts[1])
    assert moved.n == a[0].n and torch.equal(moved._state, a[0]._state)
    with pytest.raises(RuntimeError, match="at least two"):
        FeatureStats(4, DEV).update(torch.zeros(1, 4, device=DEV)).cov()
    with pytest.raises(ValueError):
        FeatureStats(4, DEV).update(torch.zeros(3, 5, device=DEV))
    with pytest.raises(ValueError):
        FeatureStats(4097, DEV)


# ------------------------------------------------------------------ kid
def _check_kid(tag, x, y, ix, iy, xd=None, yd=None):
    from dvd_gan_amd import kern as K
    xd = x.to(DEV) if xd is None else xd
    yd = y.to(DEV) if yd is None else yd
    out, terms = K.eval_kid(xd, yd, torch.from_numpy(ix), torch.from_numpy(iy))
    out2, terms2 = K.eval_kid(xd, yd, torch.from_numpy(ix), torch.from_numpy(iy))
    assert torch.equal(out, out2) and torch.equal(terms, terms2), tag
    got, worst = out.cpu().numpy(), 0.0
    xn, yn = x.numpy().astype(np.float64), y.numpy().astype(np.float64)
    for b in range(ix.shape[0]):
        want, tol = R.mmd2_poly(xn[ix[b]], yn[iy[b]]), R.mmd2_tolerance(xn[ix[b]], yn[iy[b]])
        worst = max(worst, abs(got[b] - want) / tol)
        assert abs(got[b] - want) <= tol, (tag, b, got[b], want, tol)
    print(f"[distmetrics] kid {tag}: max err / bound {worst:.4f} over {ix.shape[0]} subsets")
    return got


@pytest.mark.parametrize("n,m,d,s", [(5, 7, 3, 2), (40, 33, 70, 17), (130, 130, 128, 64)])
def test_kid_against_fp64(n, m, d, s):
    from dvd_gan_amd.distmetrics import kid_subsets
    x, y = _features(n, d, 1000 + n, scale=1.5), _features(m, d, 2000 + m, mean=0.3)
    ix, iy = kid_subsets(n, m, n_subsets=3, subset_size=s, seed=n)
    _check_kid(f"n={n} m={m} d={d} s={s}", x, y, ix, iy)


def test_kid_more_than_one_tile_and_a_strided_operand():
    """s = 130: three tiles a side, the last one ragged; x is a column slice with row stride d + 3."""
    n, m, d, s = 150, 140, 33, 130
    from dvd_gan_amd.distmetrics import kid_subsets
    wide, y = _features(n, d + 3, 8, scale=2.0), _features(m, d, 9, mean=-0.5)
    ix, iy = kid_subsets(n, m, n_subsets=2, subset_size=s, seed=1)
    xd = wide.to(DEV)[:, :d]
    assert xd.stride(0) == d + 3
    _check_kid("s=130 strided", wide[:, :d].contiguous(), y, ix, iy, xd=xd)


def test_kid_overlapping_subsets_and_identical_tables():
    n, d, s = 40, 70, 17
    x = _features(n, d, 11, scale=1.5)
    ix = np.stack([np.arange(b, b + s) for b in range(4)]).astype(np.int32)               # neighbours share s - 1 rows
    iy = np.stack([np.arange(b + 2, b + 2 + s) for b in range(4)]).astype(np.int32)
    _check_kid("overlapping, X = Y", x, x, ix, iy)
    got = _check_kid("identical tables", x, x, ix, ix)
    xn = x.numpy().astype(np.float64)
    for b in range(4):
        want = R.mmd2_same_tables(xn[ix[b]])
        assert abs(got[b] - want) <= R.mmd2_tolerance(xn[ix[b]], xn[ix[b]]), (b, got[b], want)
        assert got[b] < 0                         # -2 / s^2 sum_i k(x_i, x_i) dominates: a kernel that keeps no diagonal gives 0


def test_kid_public_call():
    from dvd_gan_amd.distmetrics import kid, kid_subsets
    x, y = _features(40, 33, 21), _features(33, 33, 22, mean=0.5)
    res = kid(x.to(DEV), y.to(DEV), n_subsets=5, subset_size=1000, seed=3)
    ix, iy = kid_subsets(40, 33, 5, 1000, 3)
    xn, yn = x.numpy().astype(np.float64), y.numpy().astype(np.float64)
    want = np.array([R.mmd2_poly(xn[ix[b]], yn[iy[b]]) for b in range(5)])
    tol = max(R.mmd2_tolerance(xn[ix[b]], yn[iy[b]]) for b in range(5))
    assert res["values"].shape == (5,) and np.all(np.abs(res["values"] - want) <= tol)
    assert abs(res["mean"] - want.mean()) <= tol and abs(res["std"] - want.std()) <= 2 * tol
    assert res["mean"] > 0                        # the sets differ in their means


# ------------------------------------------------------------------ pool
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("R_,P,C_,g", [(6, 4, 128, 1), (6, 4, 128, 3), (4, 1, 40, 2), (3, 5, 13, 3)])
def test_pool_features_against_fp64(R_, P, C_, g, dtype):
    """fp32 sums of at most P * g non-negative terms, then one division: (P g - 1 + 1) roundings of 2^-24 each at the very most,
    below 1e-6 for the P g <= 15 of these cases.  C = 13 takes the scalar path."""
    from dvd_gan_amd import kern as K
    gen = torch.Generator().manual_seed(R_ * 1000 + C_ + g)
    x = torch.randn(R_, P, C_, generator=gen).to(dtype).to(DEV)
    got = K.eval_pool_features(x, g)
    want = torch.relu(x.double()).sum(1).view(R_ // g, g, C_).sum(1) / g
    assert got.shape == (R_ // g, C_) and got.dtype == torch.float32
    assert P * g * R.U < 1e-6
    torch.testing.assert_close(got.double(), want, rtol=1e-6, atol=0.0)
    assert torch.equal(got, K.eval_pool_features(x, g))
    if g == 3:
        with pytest.raises(ValueError, match="does not divide"):
            K.eval_pool_features(x[:R_ - 1], g)


# ------------------------------------------------------------------ Trainer.evaluate_samples
CH, T, KS, B, NCLS, ZD = 2, 8, 4, 4, 3, 16


def _cfg():
    return argparse.Namespace(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=B, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9,
                              n_class=NCLS, k_sample=KS)


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


class _Replay(torch.nn.Module):
    """A generator that answers with the real clips, batch by batch: frames [B, T, 3, H, W] like Generator.forward."""

    def __init__(self, clips):
        super().__init__()
        self.clips, self.at = clips, 0

    def forward(self, z, labels):
        out = self.clips[self.at:self.at + z.shape[0]].permute(0, 2, 1, 3, 4).contiguous().to(z.device)
        self.at += z.shape[0]
        return out


def _plain_embed(clips):
    """[B, 3, T, H, W] -> [B, 3 T] frame means plus a constant: a feature extractor the test can restate on the host."""
    return clips.mean(dim=(3, 4)).reshape(clips.shape[0], -1) + 2.0


def test_evaluate_samples_of_the_real_clips_themselves(trainer):
    """The stub generator returns the real clips, so both feature sets are the same rows: the Frechet distance is 0 up to (a) what
    the two covariances can be off by, twice the trace of the S2 bound over n - 1, and (b) the host's square roots: eigvalsh is off
    by up to d eps lambda_max^2 on the eigenvalues of S^(1/2) S S^(1/2), i.e. sqrt(d eps) lambda_max on a root near zero, d roots.
    kid_mean is compared with the fp64 restatement on the same features and subsets."""
    from dvd_gan_amd.distmetrics import kid_subsets
    clips, labels = _clips(12, 5)
    real = [(clips[i:i + B], labels[i:i + B]) for i in range(0, 12, B)]
    live = trainer.G
    trainer.G = _Replay(clips)
    try:
        res = trainer.evaluate_samples(real, n_samples=12, embed=_plain_embed, seed=4)
    finally:
        trainer.G = live
    feats = _plain_embed(clips.to(DEV)).cpu().numpy()
    d, n = feats.shape[1], 12
    assert (res["n_real"], res["n_fake"], res["d"]) == (n, n, d) and d == 3 * T
    f64 = feats.astype(np.float64)
    pivot = f64[:B].mean(0).astype(np.float32)
    _, _, _, b2 = R.moments_ref([feats[i:i + B] for i in range(0, n, B)], pivot)
    lam_max = np.linalg.eigvalsh(np.cov(f64, rowvar=False))[-1]
    tol_fd = 2 * 2 * np.trace(b2) / (n - 1) + 2 * d * np.sqrt(d * np.finfo(np.float64).eps) * lam_max
    print(f"[distmetrics] replayed clips: fd {res['fd']:.3e} (tolerance {tol_fd:.3e}), kid_mean {res['kid_mean']:.6e}")
    assert abs(res["fd"]) <= tol_fd
    ix, iy = kid_subsets(n, n, seed=4)
    want = np.array([R.mmd2_poly(f64[ix[b]], f64[iy[b]]) for b in range(ix.shape[0])])
    tol = max(R.mmd2_tolerance(f64[ix[b]], f64[iy[b]]) for b in range(0, ix.shape[0], 10))
    assert abs(res["kid_mean"] - want.mean()) <= tol and abs(res["kid_std"] - want.std()) <= 2 * tol
    # real_stats from a file serve the same distance
    from dvd_gan_amd.distmetrics import FeatureStats
    st = FeatureStats(d, DEV)
    for i in range(0, n, B):
        st.update(torch.from_numpy(feats[i:i + B]).to(DEV))
    trainer.G = _Replay(clips)
    try:
        res2 = trainer.evaluate_samples(real, n_samples=12, embed=_plain_embed, seed=4, real_stats=st, kid=False)
    finally:
        trainer.G = live
    assert res2["fd"] == res["fd"] and res2["kid_mean"] is None


@pytest.mark.parametrize("embed", ["Dt", "Ds"])
def test_evaluate_samples_with_the_discriminator_features(trainer, embed):
    clips, labels = _clips(8, 6)
    real = [(clips[:B], labels[:B]), (clips[B:], labels[B:])]
    a = trainer.evaluate_samples(real, n_samples=8, embed=embed, seed=1)
    b = trainer.evaluate_samples(real, n_samples=8, embed=embed, seed=1)
    c = trainer.evaluate_samples(real, n_samples=8, embed=embed, seed=2)
    print(f"[distmetrics] embed={embed}: {a}")
    assert a == b                                             # one seed: the same bits
    assert (a["n_real"], a["n_fake"], a["d"]) == (8, 8, 16 * CH)
    assert np.isfinite(a["fd"]) and np.isfinite(a["kid_mean"]) and a["fd"] > 0
    assert c["fd"] != a["fd"]                                 # another seed: other z
    # fewer clips than the iterable holds: only the first n_samples are used
    assert trainer.evaluate_samples(real, n_samples=6, embed=embed, seed=1)["n_real"] == 6
    with pytest.raises(ValueError, match="embed"):
        trainer.evaluate_samples(real, n_samples=8, embed="I3D")


def test_disc_features_leave_the_network_untouched(trainer):
    from dvd_gan_amd.distmetrics import DiscFeatures
    from dvd_gan_amd.helpers import vid_downsample
    clips, _ = _clips(B, 7)
    frames = clips.to(DEV).permute(0, 2, 1, 3, 4).contiguous()
    for net, x, per_clip in ((trainer.D_t, vid_downsample(frames), T // 4), (trainer.D_s, frames[:, :KS].contiguous(), KS)):
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        f1 = DiscFeatures(net)(x)
        f2 = DiscFeatures(net)(x)
        per_frame = DiscFeatures(net, group=1)(x)
        after = net.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before) and net.training
        assert f1.shape == (B, 16 * CH) and per_frame.shape == (B * per_clip, 16 * CH) and torch.equal(f1, f2)
        torch.testing.assert_close(per_frame.view(B, per_clip, -1).double().mean(1), f1.double(), rtol=1e-6, atol=1e-30)
        assert "_head" not in net.__dict__


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
    """Two Trainers from one seed take the same step, one of them after evaluate_samples over a SHUFFLING loader (iterating it
    draws from torch's default generator) with the built-in D_t features: losses, weights, u / v, batch-norm statistics, Adam
    state and the torch / numpy / python random streams are bit-equal."""
    clips, labels = _clips(8, 9)
    step_clips, step_labels = _clips(B, 10)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(clips, labels), batch_size=B, shuffle=True)
    runs = []
    for evaluate in (False, True):
        tr = _trainer(21)
        if evaluate:
            res = tr.evaluate_samples(loader, n_samples=8, embed="Dt", seed=0)
            assert np.isfinite(res["fd"])
            res = tr.evaluate_samples(loader, n_samples=8, embed="Ds", seed=0, kid=False)
            assert np.isfinite(res["fd"])
        losses = [float(v.detach()) for v in tr.train_step(step_clips, step_labels)]
        torch.cuda.synchronize()
        runs.append((losses, _everything(tr)))
    (la, sa), (lb, sb) = runs
    assert la == lb, (la, lb)
    assert set(sa) == set(sb)
    differing = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not differing, differing

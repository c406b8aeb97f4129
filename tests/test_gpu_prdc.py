"""Precision / recall / density / coverage on the GPU (libdvdgan_hip_prdc.so, distmetrics.knn_radii / prdc,
Trainer.evaluate_samples(prdc_k=...)).

Every reference is numpy fp64 on the SAME stored fp32 features, centred with the pivot the device computed.  The device decides a
comparison of distances only up to the rounding of its fp32 dot products, so the references are brackets (tests/prdc_ref.py says
how they are derived): a device radius must lie inside its bracket, a device count between the counts at the two ends, and where
the bracket is collapsed -- in all seven cases of prdc_ref.CASES, which tests/test_prdc_cpu.py establishes without a GPU -- the
metrics must be EQUAL to the reference.  Every test caps the undecided pairs at 0.1 %; figures are printed before they are
asserted ("[prdc] ...", pytest -s)."""
import argparse
import functools
import random

import numpy as np
import pytest
import torch

import prdc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METRICS = ("precision", "recall", "density", "coverage")


def _normal(n, d, seed, scale=1.0, shift=0.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale + shift).astype(np.float32)


def _dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float32, order="C")).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(index):
    """Features of a prdc_ref.CASES row (computed once, shared, never written to)."""
    real, fake = R.case_features(R.CASES[index])
    real.setflags(write=False)
    fake.setflags(write=False)
    return real, fake


def _check_radii(tag, x, k, pivot_d, xd=None):
    """knn_radii of x (host fp32) on the device against the bracket; -> the device radii (fp64 numpy)."""
    from dvd_gan_amd.distmetrics import knn_radii
    xd = _dev(x) if xd is None else xd
    got_d = knn_radii(xd, k, pivot_d)
    assert got_d.dtype == torch.float64 and got_d.shape == (x.shape[0],) and got_d.is_cuda
    assert torch.equal(got_d, knn_radii(xd, k, pivot_d)), tag                     # two runs: the same bits
    got = got_d.cpu().numpy()
    lo, hi = R.radii_bracket(R.centre(x, None if pivot_d is None else pivot_d.cpu().numpy()), k)
    width = np.max((hi - lo) / np.maximum(hi, 1e-300))
    print(f"[prdc] radii {tag}: n={x.shape[0]} d={x.shape[1]} k={k}: widest bracket {width:.2e} of the radius, "
          f"worst position {np.max((got - lo) / np.maximum(hi - lo, 1e-300)):.3f} (0 = lower end, 1 = upper end)")
    assert np.all(np.isfinite(got)) and np.all(lo <= got) and np.all(got <= hi), tag
    return got


def _check_ball(tag, q, r, r2, pivot_d, qd=None, rd=None):
    """ball_count of q against the balls (r_i, r2_i), r2 = the values handed to the device (fp64 numpy) -> (count, dmin)."""
    from dvd_gan_amd import kern as K
    qd = _dev(q) if qd is None else qd
    rd = _dev(r) if rd is None else rd
    r2_d = torch.from_numpy(r2).to(DEV)
    count_d, dmin_d = K.eval_ball_count(qd, rd, r2_d, pivot_d)
    again = K.eval_ball_count(qd, rd, r2_d, pivot_d)
    assert torch.equal(count_d, again[0]) and torch.equal(dmin_d, again[1]), tag
    assert count_d.dtype == torch.int32 and dmin_d.dtype == torch.float64
    count, dmin = count_d.cpu().numpy(), dmin_d.cpu().numpy()
    pivot = None if pivot_d is None else pivot_d.cpu().numpy()
    br = R.ball_bracket(R.centre(q, pivot), R.centre(r, pivot), r2, r2)
    print(f"[prdc] ball {tag}: nq={q.shape[0]} nr={r.shape[0]}: {br['undecided']} undecided of {q.shape[0] * r.shape[0]} pairs, "
          f"counts {count.min()}..{count.max()}")
    assert br["undecided"] <= 1e-3 * q.shape[0] * r.shape[0], tag
    assert np.all(br["count_lo"] <= count) and np.all(count <= br["count_hi"]), tag
    assert np.all(br["dmin_lo"] <= dmin) and np.all(dmin <= br["dmin_hi"]), tag
    # only dmin wanted: the same minima without radii and counts
    none, dmin_only = K.eval_ball_count(qd, rd, None, pivot_d)
    assert none is None and torch.equal(dmin_only, dmin_d), tag
    return count, dmin


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=[c[0] for c in R.CASES])
def test_cases_against_fp64(index):
    """Radii of both sets, counts and minima in both directions, and the four metrics of prdc() for a prdc_ref.CASES row."""
    from dvd_gan_amd import kern as K
    from dvd_gan_amd.distmetrics import FeatureStats, prdc
    name, n, m, d, k = R.CASES[index][:5]
    real, fake = _case(index)
    real_d, fake_d = _dev(real), _dev(fake)
    pivot_d = K.eval_column_mean(real_d)
    assert torch.equal(pivot_d, FeatureStats(d, DEV).update(real_d)._pivot)        # the pivot of dvd_eval_moments_update(first = 1)
    pivot = pivot_d.cpu().numpy()
    want = real.astype(np.float64).mean(0)
    assert np.all(np.abs(pivot - want) <= R.U * np.abs(want) + 2.0 ** -45 * np.abs(real).mean(0) + 2.0 ** -149)
    r2_real = _check_radii(f"{name} real", real, k, pivot_d, real_d)
    r2_fake = _check_radii(f"{name} fake", fake, k, pivot_d, fake_d)
    _check_ball(f"{name} fake in real balls", fake, real, r2_real, pivot_d, fake_d, real_d)
    _check_ball(f"{name} real in fake balls", real, fake, r2_fake, pivot_d, real_d, fake_d)
    br = R.prdc_bracket(real, fake, k, pivot)
    got = prdc(real_d, fake_d, k=k)
    print(f"[prdc] {name}: device {[got[key] for key in METRICS]}, reference {[br[key] for key in METRICS]}, "
          f"undecided {br['undecided']} of {br['pairs']}")
    assert (got["k"], got["n_real"], got["n_fake"]) == (k, n, m) and sorted(got) == sorted(METRICS + ("k", "n_real", "n_fake"))
    assert br["undecided"] <= 1e-3 * br["pairs"]
    for key in METRICS:
        lo, hi = br[key]
        assert lo == hi and got[key] == lo, (key, got[key], br[key])               # collapsed: equality
        if name != "tiny":
            assert 0.0 < lo and (key == "density" or lo < 1.0), key                # no metric is saturated: nothing passes vacuously
    assert got == prdc(real_d, fake_d, k=k)


def test_strided_views():
    """Column slices with row stride d + 3 (radii) and d + 3 / d + 5 (ball) give the bits of the dense copies."""
    from dvd_gan_amd import kern as K
    from dvd_gan_amd.distmetrics import knn_radii
    n, m, d, k = 97, 70, 33, 3
    wide_x, wide_y = _normal(n, d + 3, 11), _normal(m, d + 5, 12, 0.9, 0.1)
    x, y = np.ascontiguousarray(wide_x[:, :d]), np.ascontiguousarray(wide_y[:, 2:2 + d])
    xv, yv = _dev(wide_x)[:, :d], _dev(wide_y)[:, 2:2 + d]
    assert xv.stride(0) == d + 3 and yv.stride(0) == d + 5
    pivot_d = K.eval_column_mean(xv)
    assert torch.equal(pivot_d, K.eval_column_mean(_dev(x)))
    r2 = _check_radii("strided", x, k, pivot_d, xv)
    assert np.array_equal(r2, knn_radii(_dev(x), k, pivot_d).cpu().numpy())
    count, dmin = _check_ball("strided", y, x, r2, pivot_d, yv, xv)
    dense = K.eval_ball_count(_dev(y), _dev(x), torch.from_numpy(r2).to(DEV), pivot_d)
    assert np.array_equal(count, dense[0].cpu().numpy()) and np.array_equal(dmin, dense[1].cpu().numpy())


@pytest.mark.parametrize("n", [64, 65, 128])
def test_tile_edges(n):
    """n an exact multiple of the 64-row tile, and one row more: padded rows are never a neighbour and never counted.  Without a
    pivot (NULL = zeros)."""
    d, k = 20, 4
    x, y = _normal(n, d, 20 + n), _normal(n + 1, d, 40 + n, 1.1)
    r2 = _check_radii(f"edge n={n}", x, k, None)
    count, _ = _check_ball(f"edge n={n}", y, x, r2, None)
    assert count.max() <= n
    count, _ = _check_ball(f"edge n={n} (queries at the edge)", x, y, _check_radii(f"edge n={n + 1}", y, k, None), None)
    assert count.shape == (n,)


def test_largest_rank_and_every_list_capacity():
    """k = 16 at n = 40 (the largest rank the library serves), and k = 4 / 5 / 8 / 9: both sides of the register lists' capacities."""
    x = _normal(40, 12, 31)
    for k in (16, 4, 5, 8, 9, 1):
        _check_radii(f"k={k}", x, k, None)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        _check_radii("k=17", x, 17, None)
    with pytest.raises(RuntimeError, match="bad argument"):
        _check_radii("k=n", x, 40, None)


def test_many_tiles_per_workgroup():
    """n = 3210: 51 strips and tiles, split into 26 chunks: a workgroup walks two tiles of the other set (the last chunk one), and
    the chunks' lists are merged."""
    from dvd_gan_amd import kern as K
    n, m, d, k = 3210, 300, 6, 5
    x, y = _normal(n, d, 51), _normal(m, d, 52, 0.9, 0.2)
    xd, yd = _dev(x), _dev(y)
    pivot_d = K.eval_column_mean(xd)
    r2 = _check_radii("n=3210", x, k, pivot_d, xd)
    _check_ball("300 in 3210 balls", y, x, r2, pivot_d, yd, xd)
    _check_ball("3210 in 300 balls", x, y, _check_radii("m=300", y, k, pivot_d, yd), pivot_d, xd, yd)


def test_permuted_rows_give_permuted_radii():
    """The same rows in another order: the same multiset of distances per row (a dot product does not depend on where its rows
    sit in a tile), so the radii are permuted-EQUAL -- a selection that depends on tile position fails this."""
    from dvd_gan_amd.distmetrics import knn_radii
    n, d, k = 200, 40, 5
    x = _normal(n, d, 61)
    perm = np.random.default_rng(62).permutation(n)
    a = knn_radii(_dev(x), k).cpu().numpy()
    b = knn_radii(_dev(x[perm]), k).cpu().numpy()
    assert np.array_equal(a[perm], b)


def test_duplicate_rows_give_zero_radii():
    """j != i is by position: a row stored twice has its copy as a neighbour at distance 0 up to the bound of a row with itself,
    and both copies get the same radius."""
    from dvd_gan_amd.distmetrics import knn_radii
    x = _normal(70, 9, 71)
    x[66] = x[3]
    r1 = knn_radii(_dev(x), 1).cpu().numpy()
    assert r1[3] <= R.pair_d2(x[3:4].astype(np.float64), x[3:4].astype(np.float64))[1][0, 0] and r1[3] == r1[66]
    assert np.all(r1[[i for i in range(70) if i not in (3, 66)]] > 0)


def test_a_set_against_its_own_balls():
    """Every BALL holds its centre and its k nearest neighbours.  count[q] is per QUERY row (in how many balls q lies; the
    neighbour relation is not symmetric, so only count[q] >= 1 holds per row), hence the statement is about the sum: the counts of
    a set against itself add up to at least n (k + 1).  The k-th neighbour sits exactly ON the sphere, which a reference bracket
    cannot decide; the device can, because its distance is symmetric to the bit (a + b and a b commute, k runs in the same order)
    and a value compared with itself is inside.  prdc(x, x): every row is in its own ball, so precision = recall = coverage = 1
    and density >= (k + 1) / k."""
    from dvd_gan_amd import kern as K
    from dvd_gan_amd.distmetrics import knn_radii, prdc
    n, d, k = 130, 24, 3
    x = _normal(n, d, 81)
    xd = _dev(x)
    pivot_d = K.eval_column_mean(xd)
    r2_d = knn_radii(xd, k, pivot_d)
    count_d, dmin_d = K.eval_ball_count(xd, xd, r2_d, pivot_d)
    count, dmin = count_d.cpu().numpy(), dmin_d.cpu().numpy()
    y = R.centre(x, pivot_d.cpu().numpy())
    _, e = R.pair_d2(y, y)
    assert np.all(dmin <= np.diag(e))                                              # the row itself, at distance 0 up to its bound
    d2, e = R.pair_d2(y, y)
    r2 = r2_d.cpu().numpy()
    inside_ball = (d2 - e <= r2[None, :]).sum(0)                                   # per ball: rows that may lie in it
    assert np.all(inside_ball >= k + 1)
    print(f"[prdc] self: counts sum {count.sum()}, n (k + 1) = {n * (k + 1)}")
    assert count.sum() >= n * (k + 1)              # the device compares the k-th neighbour's distance with itself: never outside
    assert np.all(count >= 1)
    res = prdc(xd, xd, k=k)
    assert res["precision"] == 1.0 and res["recall"] == 1.0 and res["coverage"] == 1.0
    assert res["density"] == count.sum() / (k * n) and res["density"] >= (k + 1) / k


def test_wrapper_argument_errors():
    from dvd_gan_amd import kern as K
    x = _dev(_normal(10, 4, 91))
    with pytest.raises(ValueError, match="pivot"):
        K.eval_knn_radii(x, 2, torch.zeros(5, device=DEV))
    with pytest.raises(ValueError, match="r2"):
        K.eval_ball_count(x, x, torch.zeros(10, device=DEV))                      # fp32 radii
    with pytest.raises(ValueError, match="feature width"):
        K.eval_ball_count(x, _dev(_normal(10, 5, 92)))


# ------------------------------------------------------------------ Trainer.evaluate_samples(prdc_k=...)
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


class _Replay(torch.nn.Module):
    """A generator that answers with stored clips, batch by batch: frames [B, T, 3, H, W] like Generator.forward."""

    def __init__(self, clips):
        super().__init__()
        self.clips, self.at = clips, 0

    def forward(self, z, labels):
        out = self.clips[self.at:self.at + z.shape[0]].permute(0, 2, 1, 3, 4).contiguous().to(z.device)
        self.at += z.shape[0]
        return out


def _plain_embed(clips):
    """[B, 3, T, H, W] -> [B, 3 T] frame means plus a constant: a feature extractor the test can restate by hand."""
    return clips.mean(dim=(3, 4)).reshape(clips.shape[0], -1) + 2.0


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


TODAYS_KEYS = ["d", "fd", "kid_mean", "kid_std", "n_fake", "n_real"]


def test_evaluate_samples_with_prdc_k():
    """A stub generator answers with stored clips, so both feature sets can be embedded again by hand, batch by batch as the
    Trainer does: the four values are those of prdc() on these features, the other keys are untouched, and without prdc_k the
    result has exactly the keys it had."""
    from dvd_gan_amd.distmetrics import prdc
    tr = _trainer(3)
    clips, labels = _clips(12, 5)
    shown, _ = _clips(12, 6)
    shown = 0.8 * shown + 0.1 * clips                          # generated clips near, not at, the real ones
    real = [(clips[i:i + B], labels[i:i + B]) for i in range(0, 12, B)]
    live = tr.G
    results = []
    try:
        for kwargs in ({"prdc_k": 3}, {}, {"prdc_k": 3, "kid": False}):
            tr.G = _Replay(shown)
            results.append(tr.evaluate_samples(real, n_samples=12, embed=_plain_embed, seed=4, **kwargs))
    finally:
        tr.G = live
    with_k, without, no_kid = results
    assert sorted(without) == TODAYS_KEYS
    assert sorted(with_k) == sorted(TODAYS_KEYS + list(METRICS) + ["prdc_k"]) and with_k["prdc_k"] == 3
    assert all(with_k[key] == without[key] for key in TODAYS_KEYS)
    assert no_kid["kid_mean"] is None and all(no_kid[key] == with_k[key] for key in METRICS + ("fd",))

    def by_hand(c):
        return torch.cat([_plain_embed(c[i:i + B].to(DEV).to(torch.float32)) for i in range(0, 12, B)])
    want = prdc(by_hand(clips), by_hand(shown), k=3)
    print(f"[prdc] evaluate_samples: {[with_k[key] for key in METRICS]}")
    assert all(with_k[key] == want[key] for key in METRICS)
    assert all(0.0 <= with_k[key] <= 1.0 for key in ("precision", "recall", "coverage"))
    with pytest.raises(ValueError, match="prdc_k"):
        tr.evaluate_samples(real, n_samples=12, embed=_plain_embed, prdc_k=0)
    with pytest.raises(ValueError, match="k=12"):
        tr.evaluate_samples(real, n_samples=12, embed=_plain_embed, prdc_k=12)


def test_a_training_step_does_not_notice_an_evaluation_with_prdc():
    """Two Trainers from one seed take the same step, one of them after evaluate_samples(prdc_k=3) over a SHUFFLING loader with
    the built-in discriminator features: losses, weights, u / v, batch-norm statistics, Adam state and the torch / numpy /
    python random streams are bit-equal."""
    clips, labels = _clips(8, 9)
    step_clips, step_labels = _clips(B, 10)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(clips, labels), batch_size=B, shuffle=True)
    runs = []
    for evaluate in (False, True):
        tr = _trainer(21)
        if evaluate:
            res = tr.evaluate_samples(loader, n_samples=8, embed="Dt", seed=0, prdc_k=3)
            assert all(np.isfinite(res[key]) for key in METRICS) and res["prdc_k"] == 3
            res = tr.evaluate_samples(loader, n_samples=8, embed="Ds", seed=0, kid=False, prdc_k=2)
            assert all(np.isfinite(res[key]) for key in METRICS)
        losses = [float(v.detach()) for v in tr.train_step(step_clips, step_labels)]
        torch.cuda.synchronize()
        runs.append((losses, _everything(tr)))
    (la, sa), (lb, sb) = runs
    assert la == lb, (la, lb)
    assert set(sa) == set(sb)
    differing = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not differing, differing

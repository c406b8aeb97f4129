"""Distribution distances without a GPU: the eval library's refusals (which come back before anything
touches the device), the host half of the Frechet distance against closed forms, the subset drawing of kid() and the fp64
restatement of MMD^2 the GPU tests compare with (tests/distmetrics_ref.py) against a hand computation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distmetrics_ref as R

E_ARG, E_SHAPE = -1, -2


def test_resource_file_shows_no_scratch():
    """csrc/build.sh keeps hipcc's resource remarks of the eval library: every kernel of it runs from registers."""
    from test_abi_cpu import ROOT
    res = os.path.join(ROOT, "dvd_gan_amd", "csrc", "eval", "build", "distmetrics.res")
    text = open(res).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    for kernel in ("eval_pool_kernel", "eval_pivot_kernel", "eval_moments_kernel", "eval_kid_kernel", "eval_kid_reduce_kernel"):
        assert any(kernel in n for n in names), kernel
    assert len(scratch) == len(names) and not any(scratch), list(zip(names, scratch))


P_ = 64          # a non-null placeholder pointer: the refusals come before anything is dereferenced


def test_pool_features_refusals():
    from dvd_gan_amd import lib as L
    ev = L.eval_lib()
    assert ev.dvd_eval_pool_features(L.BF16, None, 6, 4, 128, 1, P_, None) == E_ARG
    assert ev.dvd_eval_pool_features(L.BF16, P_, 6, 4, 128, 1, None, None) == E_ARG
    assert ev.dvd_eval_pool_features(7, P_, 6, 4, 128, 1, P_, None) == E_ARG                 # unknown dtype
    assert ev.dvd_eval_pool_features(L.F32, P_, 6, 4, 128, 4, P_, None) == E_ARG             # g does not divide R
    assert ev.dvd_eval_pool_features(L.F32, P_, 6, 4, 128, 0, P_, None) == E_ARG
    assert ev.dvd_eval_pool_features(L.F32, P_, 0, 4, 128, 1, P_, None) == E_ARG
    assert ev.dvd_eval_pool_features(L.F32, P_, 6, 0, 128, 1, P_, None) == E_ARG
    assert ev.dvd_eval_pool_features(L.F32, P_, 1 << 30, 1 << 10, 1 << 10, 1, P_, None) == E_SHAPE


def test_moments_refusals_and_state_size():
    from dvd_gan_amd import lib as L
    ev = L.eval_lib()
    T = L.EVAL_TILE
    assert [ev.dvd_eval_moments_state_doubles(d) for d in (0, 1, 64, 70, 128, 129, 4096, 4097)] == \
        [-1, 1 + T * T, 64 + T * T, 70 + 3 * T * T, 128 + 3 * T * T, 129 + 6 * T * T, 4096 + 2080 * T * T, -1]
    assert ev.dvd_eval_moments_update(None, 4, 8, 8, P_, P_, 1, None) == E_ARG
    assert ev.dvd_eval_moments_update(P_, 4, 8, 8, None, P_, 1, None) == E_ARG
    assert ev.dvd_eval_moments_update(P_, 4, 8, 8, P_, None, 1, None) == E_ARG
    assert ev.dvd_eval_moments_update(P_, 0, 8, 8, P_, P_, 1, None) == E_ARG
    assert ev.dvd_eval_moments_update(P_, 4, 0, 8, P_, P_, 1, None) == E_SHAPE               # d out of range
    assert ev.dvd_eval_moments_update(P_, 4, L.EVAL_MAX_D + 1, 8192, P_, P_, 1, None) == E_SHAPE
    assert ev.dvd_eval_moments_update(P_, 4, 8, 7, P_, P_, 1, None) == E_ARG                 # stride below the row length
    assert ev.dvd_eval_moments_update(P_, 4, 8, 8, P_, P_ + 4, 1, None) == E_ARG             # misaligned fp64 state
    assert ev.dvd_eval_moments_update(P_, 1 << 30, 8, 1 << 20, P_, P_, 1, None) == E_SHAPE


def test_kid_refusals():
    from dvd_gan_amd import lib as L
    ev = L.eval_lib()
    assert ev.dvd_eval_kid_ws_doubles(2, 17) == 2 * 3 and ev.dvd_eval_kid_ws_doubles(1, 130) == 3 * 4 + 9
    assert ev.dvd_eval_kid_ws_doubles(1, 1) == E_ARG and ev.dvd_eval_kid_ws_doubles(0, 4) == E_ARG
    assert ev.dvd_eval_kid_ws_doubles(L.EVAL_MAX_SUBSETS + 1, 4) == E_SHAPE
    ok = (C.c_int * 4)(0, 1, 2, 1)
    bad_hi = (C.c_int * 4)(0, 1, 5, 1)
    bad_lo = (C.c_int * 4)(0, -1, 2, 1)

    def call(X=P_, n=5, ldx=3, Y=P_, m=3, ldy=3, d=3, ixh=ok, iyh=ok, ixd=P_, iyd=P_, n_sub=2, s=2, ws=P_, out=P_, terms=None):
        return ev.dvd_eval_kid(X, n, ldx, Y, m, ldy, d, ixh, iyh, ixd, iyd, n_sub, s, ws, out, terms, None)
    for name in ("X", "Y", "ixh", "iyh", "ixd", "iyd", "ws", "out"):
        assert call(**{name: None}) == E_ARG, name
    assert call(s=1) == E_ARG and call(n_sub=0) == E_ARG and call(n=0) == E_ARG and call(m=0) == E_ARG
    assert call(d=0) == E_SHAPE and call(d=L.EVAL_MAX_D + 1, ldx=8192, ldy=8192) == E_SHAPE
    assert call(ldx=2) == E_ARG and call(ldy=2) == E_ARG
    assert call(ixh=bad_hi) == E_ARG and call(ixh=bad_lo) == E_ARG
    assert call(iyh=bad_hi) == E_ARG                          # 5 is no row of Y (m = 3) ...
    assert call(n=6, ixh=bad_hi, iyh=bad_hi) == E_ARG         # ... and stays none where it is a row of X (n = 6)
    assert call(ws=P_ + 4) == E_ARG and call(out=P_ + 4) == E_ARG
    assert b"index" in ev.dvd_eval_strerror(E_ARG) and b"shape" in ev.dvd_eval_strerror(E_SHAPE)
    assert ev.dvd_eval_strerror(0) == b"ok" and ev.dvd_eval_strerror(-77) == b"unknown error"


# ------------------------------------------------------------------ Frechet distance (host, fp64)
def _spd(rng, d, lo=0.1, hi=3.0):
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = rng.uniform(lo, hi, d)
    return (q * lam) @ q.T, q, lam


def test_frechet_identical_statistics_give_zero():
    from dvd_gan_amd.distmetrics import frechet_distance
    rng = np.random.default_rng(0)
    cov, _, _ = _spd(rng, 48)
    mean = rng.standard_normal(48) * 5
    fd = frechet_distance((mean, cov), (mean, cov))
    print(f"[distmetrics] identical: fd {fd:.3e}, tr {np.trace(cov):.3f}")
    assert abs(fd) <= 1e-9 * np.trace(cov)


def test_frechet_diagonal_covariances():
    from dvd_gan_amd.distmetrics import frechet_distance
    rng = np.random.default_rng(1)
    a, b = rng.uniform(0.05, 4.0, 40), rng.uniform(0.05, 4.0, 40)
    ma, mb = rng.standard_normal(40), rng.standard_normal(40)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((ma - mb) ** 2).sum()
    got = frechet_distance((ma, np.diag(a)), (mb, np.diag(b)))
    assert abs(got - want) <= 1e-10 * (a.sum() + b.sum() + want)


def test_frechet_rotated_commuting_pair():
    """S_a = Q diag(a) Q^T, S_b = Q diag(b) Q^T commute: tr (S_a S_b)^(1/2) = sum sqrt(a b) whatever Q is."""
    from dvd_gan_amd.distmetrics import frechet_distance
    rng = np.random.default_rng(2)
    _, q, a = _spd(rng, 33)
    b = rng.uniform(0.1, 3.0, 33)
    ma, mb = rng.standard_normal(33), rng.standard_normal(33)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((ma - mb) ** 2).sum()
    got = frechet_distance((ma, (q * a) @ q.T), (mb, (q * b) @ q.T))
    assert abs(got - want) <= 1e-10 * (a.sum() + b.sum() + want)


def test_frechet_rank_deficient_pair_is_real_finite_and_symmetric():
    """n = 20 rows of d = 64 features: covariances of rank 19.  scipy's sqrtm returns complex noise here; the symmetric form does
    not, and swapping the arguments changes the value by rounding only."""
    from dvd_gan_amd.distmetrics import frechet_distance
    rng = np.random.default_rng(3)
    xa, xb = rng.standard_normal((20, 64)), rng.standard_normal((20, 64)) * 1.5 + 0.3
    sa, sb = (xa.mean(0), np.cov(xa, rowvar=False)), (xb.mean(0), np.cov(xb, rowvar=False))
    ab, ba = frechet_distance(sa, sb), frechet_distance(sb, sa)
    print(f"[distmetrics] rank-deficient: fd(a, b) {ab!r}, fd(b, a) {ba!r}")
    assert isinstance(ab, float) and np.isfinite(ab) and np.isfinite(ba) and ab > 0
    assert abs(ab - ba) <= 1e-9 * abs(ab)
    assert abs(frechet_distance(sa, sa)) <= 1e-9 * np.trace(sa[1])


def test_feature_stats_file_round_trip(tmp_path):
    """save() writes n / mean / cov; load() serves them without a device and refuses update()."""
    import torch
    from dvd_gan_amd.distmetrics import FeatureStats, frechet_distance
    rng = np.random.default_rng(4)
    x = rng.standard_normal((30, 6))
    path = str(tmp_path / "real_stats.npz")
    with open(path, "wb") as f:
        np.savez(f, n=np.int64(30), mean=x.mean(0), cov=np.cov(x, rowvar=False))
    st = FeatureStats.load(path)
    assert (st.n, st.d) == (30, 6) and np.array_equal(st.mean(), x.mean(0)) and np.array_equal(st.cov(), np.cov(x, rowvar=False))
    assert abs(frechet_distance(st, (x.mean(0), np.cov(x, rowvar=False)))) <= 1e-9 * np.trace(st.cov())
    with pytest.raises(RuntimeError, match="no running state"):
        st.update(torch.zeros(2, 6))
    again = str(tmp_path / "again.npz")
    st.save(again)
    with np.load(again) as z:
        assert sorted(z.files) == ["cov", "mean", "n"] and int(z["n"]) == 30 and np.array_equal(z["cov"], st.cov())
    with pytest.raises(ValueError, match="different widths"):
        frechet_distance(st, (np.zeros(5), np.eye(5)))


# ------------------------------------------------------------------ kid(): subsets and the fp64 restatement
def test_kid_subsets_are_reproducible_distinct_and_clipped():
    from dvd_gan_amd.distmetrics import kid_subsets
    ix, iy = kid_subsets(50, 40, n_subsets=7, subset_size=16, seed=5)
    ix2, iy2 = kid_subsets(50, 40, n_subsets=7, subset_size=16, seed=5)
    ix3, _ = kid_subsets(50, 40, n_subsets=7, subset_size=16, seed=6)
    assert ix.dtype == iy.dtype == np.int32 and ix.shape == iy.shape == (7, 16)
    assert np.array_equal(ix, ix2) and np.array_equal(iy, iy2) and not np.array_equal(ix, ix3)
    for tab, hi in ((ix, 50), (iy, 40)):
        assert tab.min() >= 0 and tab.max() < hi
        assert all(len(set(row)) == 16 for row in tab.tolist())          # no row twice within a subset
    # subset_size is clipped to min(n, m): every subset is then a permutation of the smaller set
    ix, iy = kid_subsets(50, 9, n_subsets=3, subset_size=1000, seed=0)
    assert ix.shape == iy.shape == (3, 9) and all(sorted(row) == list(range(9)) for row in iy.tolist())
    state = np.random.get_state()[1].copy()
    kid_subsets(50, 40, seed=1)
    assert np.array_equal(np.random.get_state()[1], state)               # numpy's global stream is not drawn from
    with pytest.raises(ValueError):
        kid_subsets(50, 1)


def test_mmd2_restatement_against_a_hand_computation():
    """Three points per set in d = 2, every kernel value worked out by hand (t = a.b / 2 + 1, k = t^3):
       x = (0,0), (2,0), (0,2);  y = (2,2), (0,0), (-2,0).
       k(x_i, x_j), i != j: all dot products 0 -> k = 1; six ordered pairs -> sum 6.
       k(y_i, y_j), i != j: y0.y1 = 0 -> 1; y0.y2 = -4 -> t = -1 -> -1; y1.y2 = 0 -> 1; ordered pairs double: 2 (1 - 1 + 1) = 2.
       k(x_i, y_j): x0 -> 1, 1, 1; x1.y = 4, 0, -4 -> 27, 1, -1; x2.y = 4, 0, 0 -> 27, 1, 1; sum 3 + 27 + 29 = 59.
       MMD^2 = 6/6 + 2/6 - 2 * 59 / 9."""
    x = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0]])
    y = np.array([[2.0, 2.0], [0.0, 0.0], [-2.0, 0.0]])
    assert R.mmd2_poly(x, y) == pytest.approx(1.0 + 1.0 / 3.0 - 118.0 / 9.0, rel=1e-14)
    # identical tables: k(x_i, x_i) = 1, 27, 27 -> 2 * 6 / (9 * 2) - 2 * 55 / 9
    assert R.mmd2_same_tables(x) == pytest.approx(12.0 / 18.0 - 110.0 / 9.0, rel=1e-14)
    assert R.mmd2_poly(x, x) == pytest.approx(R.mmd2_same_tables(x), rel=1e-14)
    assert R.mmd2_tolerance(x, y) > 0 and R.mmd2_tolerance(x, y) < 1e-4

"""Precision / recall / density / coverage without a GPU: the prdc library's refusals (which come back before
anything touches the device), its resource file, the fp64 restatement the GPU tests compare with (tests/prdc_ref.py) against a
hand computation, the GPU tests' cases (decided by their brackets) and the argument checks of distmetrics.prdc()."""
import os
import re

import numpy as np
import pytest

import prdc_ref as R

E_ARG, E_SHAPE = -1, -2
P_ = 64          # a non-null placeholder pointer: the refusals come before anything is dereferenced


def test_resource_file_shows_no_scratch():
    """csrc/build.sh keeps hipcc's resource remarks of the prdc library: every kernel of it runs from registers -- the sorted
    neighbour lists (a dynamically indexed per-thread array would live in scratch memory) included, at every capacity."""
    from test_abi_cpu import ROOT
    text = open(os.path.join(ROOT, "dvd_gan_amd", "csrc", "prdc", "build", "prdc.res")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    for kernel in ("prdc_mean_kernel", "prdc_norm_kernel", "prdc_pair_kernel", "prdc_knn_merge_kernel", "prdc_ball_merge_kernel"):
        assert any(kernel in n for n in names), kernel
    assert sum("prdc_pair_kernel" in n for n in names) == 4            # radii at three list capacities, the ball count
    assert len(scratch) == len(names) and not any(scratch), list(zip(names, scratch))


def test_column_mean_refusals():
    from dvd_gan_amd import lib as L
    pr = L.prdc_lib()
    assert pr.dvd_prdc_column_mean(None, 4, 8, 8, P_, None) == E_ARG
    assert pr.dvd_prdc_column_mean(P_, 4, 8, 8, None, None) == E_ARG
    assert pr.dvd_prdc_column_mean(P_, 0, 8, 8, P_, None) == E_ARG
    assert pr.dvd_prdc_column_mean(P_, 4, 8, 7, P_, None) == E_ARG                       # stride below the row length
    assert pr.dvd_prdc_column_mean(P_, 4, 0, 8, P_, None) == E_SHAPE
    assert pr.dvd_prdc_column_mean(P_, 4, L.PRDC_MAX_D + 1, 8192, P_, None) == E_SHAPE
    assert pr.dvd_prdc_column_mean(P_, 1 << 30, 8, 1 << 20, P_, None) == E_SHAPE
    assert pr.dvd_prdc_strerror(0) == b"ok" and pr.dvd_prdc_strerror(-77) == b"unknown error"
    assert b"neighbour rank" in pr.dvd_prdc_strerror(E_ARG) and b"shape" in pr.dvd_prdc_strerror(E_SHAPE)


def _split(n_own, n_cand):
    """The documented split of the other set's tiles into chunks: (S, tiles per chunk)."""
    strips, nct = -(-n_own // 64), -(-n_cand // 64)
    want = min(nct, -(-(-(-2048 // strips)) // 8) * 8)          # ceil(2048 / strips), rounded up to a multiple of 8
    tpc = -(-nct // want)
    return -(-nct // tpc), tpc


def test_knn_refusals_and_workspace_size():
    from dvd_gan_amd import lib as L
    pr = L.prdc_lib()
    for n, k in ((5, 2), (64, 1), (65, 16), (130, 3), (10000, 5), (70000, 5), (200000, 3)):
        S, _ = _split(n, n)
        assert pr.dvd_prdc_knn_ws_doubles(n, k) == n + S * -(-n // 64) * 64 * k, (n, k)
    assert _split(130, 130) == (3, 1) and _split(10000, 10000) == (16, 10) and _split(3210, 3210) == (26, 2)
    assert _split(200000, 200000) == (8, 391)
    assert pr.dvd_prdc_knn_ws_doubles(5, 0) == E_ARG and pr.dvd_prdc_knn_ws_doubles(5, 5) == E_ARG
    assert pr.dvd_prdc_knn_ws_doubles(0, 1) == E_ARG and pr.dvd_prdc_knn_ws_doubles(1, 1) == E_ARG
    assert pr.dvd_prdc_knn_ws_doubles(40, L.PRDC_MAX_K + 1) == E_SHAPE
    assert pr.dvd_prdc_knn_ws_doubles(L.PRDC_MAX_ROWS + 1, 3) == E_SHAPE

    def call(X=P_, n=40, d=8, ldx=8, pivot=None, k=3, ws=P_, r2=P_):
        return pr.dvd_prdc_knn_radii(X, n, d, ldx, pivot, k, ws, r2, None)
    for name in ("X", "ws", "r2"):
        assert call(**{name: None}) == E_ARG, name
    assert call(n=0) == E_ARG and call(k=0) == E_ARG
    assert call(k=40, n=40) == E_ARG and call(n=3, k=3) == E_ARG and call(n=3, k=7) == E_ARG         # k >= n
    assert call(k=L.PRDC_MAX_K + 1) == E_SHAPE                                                       # 17 < n = 40
    assert call(d=0) == E_SHAPE and call(d=L.PRDC_MAX_D + 1, ldx=8192) == E_SHAPE
    assert call(ldx=7) == E_ARG
    assert call(ws=P_ + 4) == E_ARG and call(r2=P_ + 4) == E_ARG and call(pivot=P_ + 2) == E_ARG     # misaligned
    assert call(n=1 << 22, ldx=1 << 20) == E_SHAPE                                                   # n * ldx above 2^40
    assert call(n=L.PRDC_MAX_ROWS + 1) == E_SHAPE


def test_ball_refusals_and_workspace_size():
    from dvd_gan_amd import lib as L
    pr = L.prdc_lib()
    for nq, nr in ((7, 5), (97, 130), (65, 64), (10000, 10000), (70, 50000)):
        S, _ = _split(nq, nr)
        assert pr.dvd_prdc_ball_ws_doubles(nq, nr) == nq + nr + 2 * S * -(-nq // 64) * 64, (nq, nr)
    assert pr.dvd_prdc_ball_ws_doubles(0, 5) == E_ARG and pr.dvd_prdc_ball_ws_doubles(5, 0) == E_ARG
    assert pr.dvd_prdc_ball_ws_doubles(L.PRDC_MAX_ROWS + 1, 5) == E_SHAPE
    assert pr.dvd_prdc_ball_ws_doubles(5, L.PRDC_MAX_ROWS + 1) == E_SHAPE

    def call(Q=P_, nq=7, ldq=3, R_=P_, nr=5, ldr=3, d=3, pivot=None, r2=P_, ws=P_, count=P_, dmin=P_):
        return pr.dvd_prdc_ball_count(Q, nq, ldq, R_, nr, ldr, d, pivot, r2, ws, count, dmin, None)
    for name in ("Q", "R_", "ws", "dmin"):
        assert call(**{name: None}) == E_ARG, name
    assert call(r2=None) == E_ARG and call(count=None) == E_ARG                  # one of the pair without the other
    assert call(nq=0) == E_ARG and call(nr=0) == E_ARG
    assert call(ldq=2) == E_ARG and call(ldr=2) == E_ARG
    assert call(d=0) == E_SHAPE and call(d=L.PRDC_MAX_D + 1, ldq=8192, ldr=8192) == E_SHAPE
    assert call(ws=P_ + 4) == E_ARG and call(dmin=P_ + 4) == E_ARG and call(r2=P_ + 4) == E_ARG and call(count=P_ + 2) == E_ARG
    assert call(nq=1 << 22, ldq=1 << 20) == E_SHAPE and call(nr=1 << 22, ldr=1 << 20) == E_SHAPE
    assert call(nq=L.PRDC_MAX_ROWS + 1) == E_SHAPE and call(nr=L.PRDC_MAX_ROWS + 1) == E_SHAPE


# ------------------------------------------------------------------ the fp64 restatement
def test_restatement_against_a_hand_computation():
    """Five real points 0, 1, 3, 6, 10 and three fake points 0.5, 2.25, 20 on a line, k = 1, no pivot; every value is a multiple of
    1 / 16, so fp64 is exact.
       real radii: nearest neighbours at distance 1, 1, 2, 3, 4 -> 1, 1, 4, 9, 16   (k = 2: 3, 2, 3, 4, 7 -> 9, 4, 9, 16, 49)
       fake radii: 0.5 <-> 2.25: 1.75^2 = 3.0625 both; 20 -> 2.25: 17.75^2 = 315.0625
       fake in real balls: 0.5 lies in the balls of 0 and 1 (0.25 <= 1); 2.25 only in the ball of 3 (0.5625 <= 4; 1.5625 > 1,
                           14.0625 > 9); 20 in none (100 > 16)                       -> counts 2, 1, 0
       real in fake balls: 0 -> {0.5}; 1 -> {0.5, 2.25} (0.25, 1.5625 <= 3.0625); 3 -> {2.25, 20} (0.5625; 289 <= 315.0625);
                           6 -> {20} (196); 10 -> {20} (100)                         -> counts 1, 2, 2, 1, 1
       nearest fake of each real: 0.25, 0.25, 0.5625, 14.0625, 60.0625 against the real radii: inside for 0, 1, 3 only
       precision 2 / 3, density (2 + 1 + 0) / (1 * 3) = 1, recall 5 / 5, coverage 3 / 5."""
    real = np.array([[0.0], [1.0], [3.0], [6.0], [10.0]])
    fake = np.array([[0.5], [2.25], [20.0]])
    yr, yf = R.centre(real, None), R.centre(fake, None)
    assert np.array_equal(R.radii(yr, 1), [1, 1, 4, 9, 16]) and np.array_equal(R.radii(yr, 2), [9, 4, 9, 16, 49])
    assert np.array_equal(R.radii(yf, 1), [3.0625, 3.0625, 315.0625])
    cnt, dmin = R.ball_exact(yf, yr, R.radii(yr, 1))
    assert np.array_equal(cnt, [2, 1, 0]) and np.array_equal(dmin, [0.25, 0.5625, 100.0])
    cnt, dmin = R.ball_exact(yr, yf, R.radii(yf, 1))
    assert np.array_equal(cnt, [1, 2, 2, 1, 1]) and np.array_equal(dmin, [0.25, 0.25, 0.5625, 14.0625, 60.0625])
    assert R.prdc_exact(real, fake, 1) == {"precision": 2 / 3, "recall": 1.0, "density": 1.0, "coverage": 0.6}
    # the brackets enclose the exact values and are collapsed here: no comparison of this example is closer than its bound
    lo, hi = R.radii_bracket(yr, 1)
    assert np.all(lo <= R.radii(yr, 1)) and np.all(R.radii(yr, 1) <= hi) and np.all(hi - lo <= 1e-4)
    br = R.prdc_bracket(real, fake, 1)
    assert br["undecided"] == 0 and br["pairs"] == 2 * 15 + 5
    assert all(br[key] == (want, want) for key, want in R.prdc_exact(real, fake, 1).items())
    # a pivot moves every row alike: the centred rows, and with them every distance, stay
    assert np.array_equal(R.centre(real + 2.0, np.array([2.0])), yr)
    # a tie the bound cannot decide is reported as such: the fake point 2 is at distance exactly 1 from the real point 1
    tie = R.prdc_bracket(real, np.array([[0.5], [2.0], [20.0]]), 1)
    assert tie["undecided"] >= 1


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_the_gpu_cases_are_decided_by_their_brackets(case):
    """What makes the GPU tests of these cases strict: at most 0.1 % undecided pairs, collapsed metric brackets, and no metric
    saturated at 0 or 1 other than where the case is built to (precision of the tiny case and coverage there)."""
    real, fake = R.case_features(case)
    k = case[4]
    br = R.prdc_bracket(real, fake, k, R.column_mean_f32(real))
    exact = R.prdc_exact(real, fake, k, R.column_mean_f32(real))
    print(f"[prdc] {case[0]}: {exact}, undecided {br['undecided']} of {br['pairs']}")
    assert br["undecided"] <= 1e-3 * br["pairs"]
    for key, want in exact.items():
        assert br[key] == (want, want), key
        if case[0] != "tiny":
            assert 0.0 < want and (key == "density" or want < 1.0), key
    if case[0] == "narrow fake":              # the figures of this case as they were published with it
        assert [round(exact[key], 3) for key in ("precision", "recall", "density", "coverage")] == [0.979, 0.023, 5.251, 0.992]


def test_centring_shrinks_the_bound():
    """Features at mean 50: the bound E on a distance is some thousand times smaller about the column mean than about zero."""
    real, _ = R.case_features(R.CASES[5])
    _, e_raw = R.pair_d2(R.centre(real, None), R.centre(real, None))
    _, e_ctr = R.pair_d2(R.centre(real, R.column_mean_f32(real)), R.centre(real, R.column_mean_f32(real)))
    print(f"[prdc] mean 50: median bound {np.median(e_raw):.3e} about zero, {np.median(e_ctr):.3e} about the column mean")
    assert np.median(e_raw) > 1000 * np.median(e_ctr)


def test_prdc_argument_errors():
    import torch
    from dvd_gan_amd.distmetrics import prdc
    x, y = torch.zeros(10, 4), torch.zeros(8, 4)
    with pytest.raises(ValueError, match="k=8"):
        prdc(x, y, k=8)                                        # k >= min(n, m)
    with pytest.raises(ValueError, match="k=0"):
        prdc(x, y, k=0)
    with pytest.raises(ValueError, match="above 16"):
        prdc(torch.zeros(40, 4), torch.zeros(40, 4), k=17)
    with pytest.raises(ValueError, match="feature width"):
        prdc(x, torch.zeros(8, 5))
    with pytest.raises(ValueError, match=r"\[rows, d\]"):
        prdc(x.view(10, 2, 2), y)
    with pytest.raises(ValueError, match="device fp32 matrix"):
        prdc(x, y, k=3)                                        # host tensors: refused before any launch

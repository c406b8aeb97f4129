"""fp64 restatements of what libdvdgan_hip_prdc.so computes (include/dvdgan_hip_prdc.h), with the brackets the GPU tests assert
against (numpy only).

The device's squared distance of two centred rows is  max(0, |a|^2 + |b|^2 - 2 dot(a, b))  with fp64 norms and a dot product of
d fp32 products accumulated in fp32.  With U = 2^-24 that dot product is within (d + 2) U |a|.|b| of the exact one (the Higham
first-order form tests/distmetrics_ref.py uses), so the distance is within
    E = 2 (d + 2) U |a|.|b| + 2^-50 (|a|^2 + |b|^2)
of the fp64 value D2 (the second term: fp64 noise of both sides).  Every comparison the device makes -- which neighbour is the
k-th, whether a row lies in a ball -- is therefore decided only up to E, and the references below return BRACKETS:
    radius in [k-th smallest of max(0, D2 - E), k-th smallest of D2 + E]      (order statistics are monotone in every entry)
    count  in [#{D2 + E <= r_lo}, #{D2 - E <= r_hi}]
and the four metrics by propagating both.  A pair on which the two ends of the bracket disagree is UNDECIDED; the tests cap the
undecided pairs (a bracket wide enough to swallow everything would make them pass vacuously)."""
import numpy as np

U = 2.0 ** -24


def centre(x, pivot):
    """The rows the device multiplies: fl32(x - pivot), returned as fp64."""
    x = np.asarray(x, np.float32)
    c = np.zeros(x.shape[1], np.float32) if pivot is None else np.asarray(pivot, np.float32)
    return (x - c).astype(np.float64)


def pair_d2(ya, yb):
    """(D2, E) [na, nb] of centred fp64 rows: the fp64 squared distances and the bound on |device - D2|."""
    ya, yb = np.asarray(ya, np.float64), np.asarray(yb, np.float64)
    d = ya.shape[1]
    na, nb = (ya * ya).sum(1), (yb * yb).sum(1)
    s = na[:, None] + nb[None, :]
    d2 = np.maximum(0.0, s - 2.0 * (ya @ yb.T))
    e = 2.0 * (d + 2) * U * (np.abs(ya) @ np.abs(yb).T) + 2.0 ** -50 * s
    return d2, e


def _kth(a, k):
    return np.partition(a, k - 1, axis=1)[:, k - 1]


def radii(y, k):
    """fp64 squared distance of every row to its k-th nearest other row (other by position)."""
    d2, _ = pair_d2(y, y)
    np.fill_diagonal(d2, np.inf)
    return _kth(d2, k)


def radii_bracket(y, k):
    d2, e = pair_d2(y, y)
    lo, hi = np.maximum(0.0, d2 - e), d2 + e
    np.fill_diagonal(lo, np.inf)
    np.fill_diagonal(hi, np.inf)
    return _kth(lo, k), _kth(hi, k)


def ball_bracket(yq, yr, r_lo, r_hi):
    """Queries yq against the balls (yr_i, r_i) with r_i in [r_lo_i, r_hi_i] -> dict: count_lo / count_hi [nq] (int), dmin_lo /
    dmin_hi [nq], undecided = number of (query, ball) pairs whose membership the bracket leaves open."""
    d2, e = pair_d2(yq, yr)
    lo, hi = np.maximum(0.0, d2 - e), d2 + e
    surely, maybe = hi <= np.asarray(r_lo)[None, :], lo <= np.asarray(r_hi)[None, :]
    return {"count_lo": surely.sum(1), "count_hi": maybe.sum(1), "dmin_lo": lo.min(1), "dmin_hi": hi.min(1),
            "undecided": int((maybe & ~surely).sum())}


def ball_exact(yq, yr, r2):
    d2, _ = pair_d2(yq, yr)
    return (d2 <= np.asarray(r2)[None, :]).sum(1), d2.min(1)


def prdc_exact(real, fake, k, pivot=None):
    """The four metrics in plain fp64 (every comparison taken at face value)."""
    yr, yf = centre(real, pivot), centre(fake, pivot)
    n, m = yr.shape[0], yf.shape[0]
    r_real, r_fake = radii(yr, k), radii(yf, k)
    cnt_fr, _ = ball_exact(yf, yr, r_real)
    cnt_rf, dmin_rf = ball_exact(yr, yf, r_fake)
    return {"precision": np.count_nonzero(cnt_fr) / m, "recall": np.count_nonzero(cnt_rf) / n,
            "density": int(cnt_fr.sum()) / (k * m), "coverage": np.count_nonzero(dmin_rf <= r_real) / n}


def prdc_bracket(real, fake, k, pivot=None):
    """name -> (lo, hi) for the four metrics, plus "undecided" (pairs, the rows whose coverage test is open included) and
    "pairs" (2 n m + n, what undecided is a share of)."""
    yr, yf = centre(real, pivot), centre(fake, pivot)
    n, m = yr.shape[0], yf.shape[0]
    rr_lo, rr_hi = radii_bracket(yr, k)
    rf_lo, rf_hi = radii_bracket(yf, k)
    fr = ball_bracket(yf, yr, rr_lo, rr_hi)
    rf = ball_bracket(yr, yf, rf_lo, rf_hi)
    cov_lo, cov_hi = rf["dmin_hi"] <= rr_lo, rf["dmin_lo"] <= rr_hi
    return {"precision": (np.count_nonzero(fr["count_lo"]) / m, np.count_nonzero(fr["count_hi"]) / m),
            "recall": (np.count_nonzero(rf["count_lo"]) / n, np.count_nonzero(rf["count_hi"]) / n),
            "density": (int(fr["count_lo"].sum()) / (k * m), int(fr["count_hi"].sum()) / (k * m)),
            "coverage": (np.count_nonzero(cov_lo) / n, np.count_nonzero(cov_hi) / n),
            "undecided": fr["undecided"] + rf["undecided"] + int((cov_hi & ~cov_lo).sum()), "pairs": 2 * n * m + n}


# ------------------------------------------------------------------ the cases the GPU tests run (checked on the CPU: no undecided
# pair and collapsed metric brackets in every one of them; tests/test_prdc_cpu.py repeats that check)
#        name             n    m    d  k seed  real_shift  fake_scale  fake_shift
CASES = [("tiny",          5,   7,   3, 2, 0,  0.0,  1.0,  0.0),
         ("d=1 k=1",      37,  33,   1, 1, 1,  0.0,  1.0,  0.0),
         ("ragged",      130,  97,  70, 3, 2,  0.0,  1.0,  0.0),
         ("narrow fake", 130,  97,  70, 3, 2,  0.0,  0.8,  0.3),
         ("shifted",     200, 150, 128, 5, 3,  0.0,  1.0,  0.2),
         ("mean 50",     130,  97,  33, 3, 4, 50.0,  1.0, 50.5),
         ("wide fake",    70, 260,  16, 5, 5,  0.0,  0.7,  0.5)]


def case_features(case):
    """(real [n, d], fake [m, d]) fp32 of a CASES row: standard-normal draws of numpy's default_rng(seed), real before fake."""
    _, n, m, d, _, seed, real_shift, fake_scale, fake_shift = case
    rng = np.random.default_rng(seed)
    real = rng.standard_normal((n, d)) + real_shift
    fake = rng.standard_normal((m, d)) * fake_scale + fake_shift
    return real.astype(np.float32), fake.astype(np.float32)


def column_mean_f32(x):
    return np.asarray(x, np.float64).mean(0).astype(np.float32)

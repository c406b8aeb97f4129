"""fp64 restatements of what libdvdgan_hip_eval.so computes, and the error bounds the GPU tests assert against (numpy only).

U = 2^-24 is the unit roundoff of fp32.  A dot product of K fp32 numbers accumulated in fp32 in any order (an fma chain on the
MFMA path) is within gamma_K sum |a||b| of the exact one, gamma_K = K U / (1 - K U) (Higham, Accuracy and Stability, section
3.1).  The bounds below are the first-order forms K U: the second-order remainder is K U of the bound itself (8e-6 of it at the
K <= 130 of the tests), and a worst-case bound is met only when every rounding error has the same sign."""
import numpy as np

U = 2.0 ** -24


# ------------------------------------------------------------------ moments
def moments_ref(batches, pivot):
    """batches: the fp32 arrays of the update calls, pivot: the device's fp32 pivot -> (S1, S2, bound1, bound2), fp64:
    S1 = sum (x - c), S2 = sum (x - c)^T (x - c) over all rows, and elementwise bounds for the device's values.
    The device forms y = fl(x - c) = (x - c)(1 + e), |e| <= U, so a product y_i y_j carries (1 + e)^2 and the fp32 sum of the
    n_call products of one call adds gamma_n: |S2_call - exact| <= (n_call + 2) U |X - c|^T |X - c|  -- the issue's bound, which
    therefore already covers the rounding of the subtraction (no further factor is taken).  The calls' bounds add up.  S1 sums
    the same y in fp64: |S1 - exact| <= U sum |x - c|.  fp64 noise: 2^-50 relative to the same matrices."""
    c = np.asarray(pivot, np.float64)
    d = c.shape[0]
    s1, s2, b1, b2 = np.zeros(d), np.zeros((d, d)), np.zeros(d), np.zeros((d, d))
    for x in batches:
        y = np.asarray(x, np.float64) - c
        a = np.abs(y)
        s1 += y.sum(0)
        s2 += y.T @ y
        b1 += U * a.sum(0)
        b2 += (y.shape[0] + 2) * U * (a.T @ a)
    noise = 2.0 ** -50
    return s1, s2, b1 + noise * np.abs(s1) + 1e-300, b2 + noise * np.abs(s2) + 1e-300


def cov_tolerance(s1, b1, b2, n, want):
    """Elementwise bound on |device cov - fp64 cov|.  cov = (S2 - S1 S1^T / n) / (n - 1) holds exactly for the exact sums about any
    pivot, so the device's value is off by the bound of S2, plus what the error of S1 (at most b1) does to the outer product;
    fp64 noise of both sides: 2^-40 of sqrt(cov_ii cov_jj)."""
    a = np.abs(s1)
    sd = np.sqrt(np.abs(np.diag(want)))
    return (b2 + (np.outer(a, b1) + np.outer(b1, a) + np.outer(b1, b1)) / n) / (n - 1) + 2.0 ** -40 * np.outer(sd, sd)


def pivot_tolerance(first):
    """|device pivot - fp64 column mean of the first batch| <= one fp32 rounding of the mean, plus the difference of two fp64 sums
    of n <= 256 terms in different orders (n 2^-53 mean |x|) and the smallest subnormal."""
    x = np.asarray(first, np.float64)
    m = x.mean(0)
    return m, U * np.abs(m) + 2.0 ** -45 * np.abs(x).mean(0) + 2.0 ** -149


# ------------------------------------------------------------------ kernel distance
def poly_kernel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a @ b.T / a.shape[1] + 1.0) ** 3


def mmd2_poly(x, y):
    """Unbiased MMD^2 of two equally long fp64 sets with k(a, b) = (a.b / d + 1)^3 (Binkowski et al. 2018, eq. 4 with m = n):
    1/(s(s-1)) sum_{i != j} k(x_i, x_j) + 1/(s(s-1)) sum_{i != j} k(y_i, y_j) - 2/s^2 sum_{i, j} k(x_i, y_j)."""
    s = x.shape[0]
    assert y.shape[0] == s and s >= 2
    kxx, kyy, kxy = poly_kernel(x, x), poly_kernel(y, y), poly_kernel(x, y)
    off = ~np.eye(s, dtype=bool)
    return kxx[off].sum() / (s * (s - 1)) + kyy[off].sum() / (s * (s - 1)) - 2.0 * kxy.sum() / (s * s)


def mmd2_same_tables(x):
    """mmd2_poly(x, x) in closed form: 2 / (s^2 (s-1)) sum_{i != j} k(x_i, x_j) - 2 / s^2 sum_i k(x_i, x_i).  (A kernel that
    drops the diagonal of the cross term, or keeps it in the within terms, misses this value.)"""
    s = x.shape[0]
    k = poly_kernel(x, x)
    off = ~np.eye(s, dtype=bool)
    return 2.0 * k[off].sum() / (s * s * (s - 1)) - 2.0 * np.trace(k) / (s * s)


def mmd2_tolerance(x, y):
    """Bound on |device - mmd2_poly| for one subset.  A dot product is off by at most e = (d + 2) U sum |a||b|, so t = a.b / d + 1
    by e / d, and t^3 by 3 (|t| + 1)^2 e / d (the mean value theorem on an interval of length e / d <= 1 around t); three fp32
    roundings of the cube add 3 U |t|^3 (the library cubes in fp64: a bound it meets with room).  The pairs' bounds are added with
    the weights of the statistic."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    s, d = x.shape

    def pair_bound(a, b):
        t = a @ b.T / d + 1.0
        e = (d + 2) * U * (np.abs(a) @ np.abs(b).T) / d
        return 3.0 * (np.abs(t) + 1.0) ** 2 * e + 3.0 * U * np.abs(t) ** 3

    off = ~np.eye(s, dtype=bool)
    return (pair_bound(x, x)[off].sum() / (s * (s - 1)) + pair_bound(y, y)[off].sum() / (s * (s - 1))
            + 2.0 * pair_bound(x, y).sum() / (s * s))

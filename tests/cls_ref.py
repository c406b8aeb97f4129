"""A numpy fp64 restatement of include/dvdx_cls.h and of classmetrics.LogitStats.result(): the per-split sums behind the Inception
Score and the class-fidelity metrics of a classifier's logits, with the bound each fp64 accumulator of the device must keep.

A plain module (no conftest, no fixtures), numpy only; no project kernel and no oracle code takes part.  It works on the logits AS
STORED: hand it fp32 or fp16 arrays, or bf16 values widened to fp32 (every widening to fp64 is exact), so the split rule, the tie
rule and the bad-row rule are part of it and the counts must match exactly.

The bounds.  Device and restatement evaluate the same expressions on the same fp64 inputs; they differ in the ORDER of the sums and
in the last bits of exp / log.  U = 2^-53 is the unit roundoff, one ulp is at most 2 U relative.
  * exp / log: ROCm's HIP math API documents a maximum error of 1 ulp for the double-precision `exp` and of 1 ulp for `log`
    ("HIP math API", device functions, double precision floating-point mathematical functions); glibc documents its double `exp` /
    `log` within 1 ulp as well ("Known Maximum Errors in Math Functions").  Two evaluations of one argument are therefore within
    E = (DEV_ULPS + HOST_ULPS) ulps = 4 U relative of one another.
  * a sum of k terms, in any order, is within (k - 1) U sum|t_i| of the exact sum of its terms (first order), so two orders are
    within twice that; the device adds at most 4 more times per call (its four partial sums and the state).
Per good row with d_c = l_c - m (one correctly rounded subtraction: identical on both sides):
  Z      = sum_c exp(d_c)           relative  eZ  = E + 2 (C - 1) U                 (C positive terms)
  logZ   = log Z                    absolute  eL  = eZ + E |logZ|
  logp_c = d_c - logZ               absolute  elp = eL + 2 U |logp_c|               (one rounding on either side)
  p_c    = exp(logp_c)              relative  ep  = elp + E
  p_c * logp_c                      absolute  |p logp| (ep + 2 U) + p elp           (one rounding of the product on either side)
and the row's sum of those over c adds 2 (C - 1) U sum_c |p logp|.  A value that underflows (p below 2^-1022) is kept to an
absolute 2^-1060 (1 + |logp|) instead.  Everything is first order in U; the tests' sums stay below 2^-38 relative, so second-order
terms are 2^-76.
"""
import numpy as np

F64 = np.float64
U = 2.0 ** -53
DEV_ULPS_EXP = DEV_ULPS_LOG = 1          # ROCm, HIP math API: double exp 1 ulp, double log 1 ulp
HOST_ULPS_EXP = HOST_ULPS_LOG = 1        # glibc, known maximum errors: exp 1 ulp, log 1 ulp
E_EXP = 2.0 * U * (DEV_ULPS_EXP + HOST_ULPS_EXP)
E_LOG = 2.0 * U * (DEV_ULPS_LOG + HOST_ULPS_LOG)
TINY = 2.0 ** -1060

NSTAT = 8
N, A, BAD, LABELLED, LOGLIK, TOP1, TOP5, BAD_LABEL = range(NSTAT)
COUNTS = (N, BAD, LABELLED, TOP1, TOP5, BAD_LABEL)


def split_of(i, n_total, splits):
    """Split of the global rows i: (i * S) / n_total in 64-bit integers."""
    return (np.asarray(i, np.int64) * np.int64(splits)) // np.int64(n_total)


def accumulate(logits, labels=None, *, splits=10, n_total=None, row0=0, confusion=False, calls=1):
    """-> (state, bound, confusion): what dvdx_cls_update adds to a zeroed fp64 state [S, C + NSTAT] for logits [rows, C] (any
    float array; widened exactly) and int labels [rows] or None, the rows row0 .. of n_total (default: rows); `bound` [S, C + NSTAT]
    is the most |device - state| may be after the rows went in through `calls` device calls (0 for the counts); confusion int64
    [C, C] or None."""
    L = np.asarray(logits).astype(F64)
    assert L.ndim == 2
    rows, C = L.shape
    n_total = rows if n_total is None else int(n_total)
    S = int(splits)
    assert 1 <= S <= n_total and 0 <= row0 and row0 + rows <= n_total
    split = split_of(row0 + np.arange(rows), n_total, S)
    state, bound = np.zeros((S, C + NSTAT)), np.zeros((S, C + NSTAT))
    conf = np.zeros((C, C), np.int64) if confusion else None
    good = np.isfinite(L).all(axis=1)
    if labels is not None:
        y = np.asarray(labels).astype(np.int64)
        in_range = good & (y >= 0) & (y < C)
    # ---- per good row
    G = L[good]
    m = G.max(axis=1, keepdims=True)
    d = G - m
    Z = np.exp(d).sum(axis=1, keepdims=True)
    logZ = np.log(Z)
    lp = d - logZ
    p = np.exp(lp)
    t = p * lp
    eZ = E_EXP + 2.0 * (C - 1) * U
    eL = eZ + E_LOG * np.abs(logZ)
    elp = eL + 2.0 * U * np.abs(lp)
    ep = elp + E_EXP
    floor = TINY * (1.0 + np.abs(lp))
    p_err = p * ep + floor
    a_row = t.sum(axis=1)
    a_err = (np.abs(t) * (ep + 2.0 * U) + p * elp + floor).sum(axis=1) + 2.0 * (C - 1) * U * np.abs(t).sum(axis=1)
    g_split = split[good]
    if labels is not None:
        yg, ok = y[good], in_range[good]
        idx = np.where(ok, yg, 0)[:, None]
        ll = np.take_along_axis(lp, idx, 1)[:, 0]
        ll_err = np.take_along_axis(elp, idx, 1)[:, 0]
        ly = np.take_along_axis(G, idx, 1)
        rank = (G > ly).sum(axis=1) + ((G == ly) & (np.arange(C)[None, :] < idx)).sum(axis=1)
        arg = G.argmax(axis=1)                            # numpy: the first of equal maxima
    for s in range(S):
        bad_here = int((~good & (split == s)).sum())
        state[s, C + BAD] = bad_here
        sel = g_split == s
        k = int(sel.sum())
        if not k:
            continue
        order = (2.0 * k + 4.0 * calls) * U               # two summation orders and the device's per-call additions
        state[s, :C] = p[sel].sum(axis=0)
        bound[s, :C] = p_err[sel].sum(axis=0) + order * p[sel].sum(axis=0)
        state[s, C + N] = k
        state[s, C + A] = a_row[sel].sum()
        bound[s, C + A] = a_err[sel].sum() + order * np.abs(a_row[sel]).sum()
        if labels is None:
            continue
        lab = sel & ok
        state[s, C + LABELLED] = int(lab.sum())
        state[s, C + BAD_LABEL] = int((sel & ~ok).sum())
        state[s, C + LOGLIK] = ll[lab].sum()
        bound[s, C + LOGLIK] = ll_err[lab].sum() + order * np.abs(ll[lab]).sum()
        state[s, C + TOP1] = int((rank[lab] == 0).sum())
        state[s, C + TOP5] = int((rank[lab] < 5).sum())
    if confusion:
        assert labels is not None
        np.add.at(conf, (yg[ok], arg[ok]), 1)
    return state, bound, conf


def _entropy(q):
    q = q[q > 0]
    return float(-(q * np.log(q)).sum())


def finish(state, confusion=None, labelled=True):
    """The metrics of a state [S, C + NSTAT] (and a confusion matrix), as classmetrics.LogitStats.result() returns them.
    IS_s = exp(A_s / n_s + H(colsum_s / n_s)); splits without a good row are left out of is_mean / is_std."""
    state = np.asarray(state, F64)
    C = state.shape[1] - NSTAT
    col, st = state[:, :C], state[:, C:]
    scores = [np.exp(st[s, A] / st[s, N] + _entropy(col[s] / st[s, N])) for s in range(state.shape[0]) if st[s, N] > 0]
    tot, n = st.sum(axis=0), float(st[:, N].sum())
    nan = float("nan")
    out = {"n": int(n), "n_bad": int(tot[BAD]), "n_bad_label": int(tot[BAD_LABEL]) if labelled else 0,
           "is_mean": float(np.mean(scores)) if scores else nan, "is_std": float(np.std(scores)) if scores else nan,
           "h_marginal": _entropy(col.sum(axis=0) / n) if n else nan, "h_conditional": float(-tot[A] / n) if n else nan,
           "confusion": None if confusion is None else np.asarray(confusion, np.int64)}
    out["is_all"] = float(np.exp(out["h_marginal"] - out["h_conditional"])) if n else nan
    if labelled:
        k = float(tot[LABELLED])
        out.update(top1=float(tot[TOP1] / k) if k else nan, top5=float(tot[TOP5] / k) if k else nan,
                   mean_log_lik=float(tot[LOGLIK] / k) if k else nan, per_class_top1=None)
        if confusion is not None:
            per = out["confusion"].sum(axis=1).astype(F64)
            out["per_class_top1"] = np.where(per > 0, np.diag(out["confusion"]) / np.where(per > 0, per, 1.0), nan)
    return out


def metrics(logits, labels=None, *, splits=10, confusion=False):
    """finish(accumulate(...)) of one array: the whole statistic from the definitions."""
    state, _, conf = accumulate(logits, labels, splits=splits, confusion=confusion)
    return finish(state, conf, labelled=labels is not None)


def make_logits(rows, C, seed=0, scale=3.0):
    """fp32 [rows, C] logits and int32 labels [rows]: normal logits with the label's class raised in two rows of three, so that
    top-1 is neither 0 nor 1."""
    rng = np.random.default_rng(9000 + 131 * rows + C + seed)
    L = (scale * rng.standard_normal((rows, C))).astype(np.float32)
    y = rng.integers(0, C, rows).astype(np.int32)
    lift = np.arange(rows) % 3 != 0
    L[np.arange(rows)[lift], y[lift]] += np.float32(4.0 * scale)
    return L, y

"""fp64 numpy statement of dvd_adv_loss_ex (include/dvdgan_hip.h): top-k selection with its tie rule, the adversarial and the
LeCam term, their gradient, the anchor update and the statistics.  Shared by tests/test_adv_ref_cpu.py (which holds it against
torch autograd and torch.topk) and the GPU tests (which hold the kernel against it)."""
import numpy as np

(STAT_MEAN, STAT_SIGN, STAT_ACTIVE, STAT_ADV, STAT_LECAM, STAT_ANCHOR, STAT_KEPT, STAT_NONFINITE) = range(8)
NSTAT = 8


def scores(x, group):
    """Per-sample mean logit; x is sample-major."""
    return np.asarray(x, dtype=np.float64).reshape(-1, group).sum(axis=1) / group


def select(score, keep):
    """bool [B]: sample b is kept when fewer than `keep` samples c have score_c > score_b, or score_c == score_b with c < b.
    A NaN compares false everywhere: nothing is ahead of it (it is kept) and it is ahead of nothing."""
    s = np.asarray(score, dtype=np.float64)
    idx = np.arange(s.size)
    with np.errstate(invalid="ignore"):
        ahead = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (idx[None, :] < idx[:, None]))
    return ahead.sum(axis=1) < keep


def adv_ref(x, group=1, hinge=True, real=True, keep=0, lecam=0.0, anchor_other=None, anchor_prev=0.0, decay=None,
            grad_scale=1.0, kept=None):
    """kept: a selection computed before (select() is quadratic in the samples), else it is made here.
    -> dict: kept [B] bool, adv (the adversarial term, what is added to *loss), penalty (P), dout [n], anchor_next (None when
    decay is None = no anchor pointer), stats [NSTAT], and abs_adv / abs_pen / abs_x = the sums of |terms| of the three means (what
    a rounding bound of the fp32 sums scales with)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    assert n % group == 0
    B = n // group
    if kept is None:
        kept = select(scores(x, group), keep) if keep > 0 else np.ones(B, dtype=bool)
    k = np.repeat(kept, group)
    div = float(keep * group if keep > 0 else n)
    sgn = -1.0 if real else 1.0
    with np.errstate(invalid="ignore"):
        v = sgn * x
        terms = np.maximum(1.0 + v, 0.0) if hinge else v
        terms = np.where(np.isnan(v), 0.0 if hinge else v, terms)      # C's fmaxf(NaN, 0) is 0: the hinge term of a NaN logit is 0
        active = (1.0 + v > 0.0)
        slope = np.where(hinge & ~active, 0.0, sgn)
        adv = terms[k].sum() / div
        dout = np.where(k, slope * grad_scale / div, 0.0)
        a = 0.0 if anchor_other is None else float(anchor_other)
        pen, abs_pen = 0.0, 0.0
        if lecam > 0:
            r = np.maximum(x - a, 0.0) if real else np.maximum(a - x, 0.0)
            pen = (r * r).sum() / n
            abs_pen = float((r * r).sum())
            dout = dout + grad_scale * lecam * ((2.0 if real else -2.0) * r / n)
        mean = x.sum() / n
        nxt = None
        if decay is not None:
            nxt = (1.0 - decay) * mean + (decay * float(anchor_prev) if decay != 0 else 0.0)
        stats = np.zeros(NSTAT)
        stats[STAT_MEAN] = mean
        stats[STAT_SIGN] = np.sign(np.nan_to_num(x, nan=0.0)).sum() / n
        stats[STAT_ACTIVE] = active.sum() / n
        stats[STAT_ADV] = adv
        stats[STAT_LECAM] = pen
        stats[STAT_ANCHOR] = a
        stats[STAT_KEPT] = kept.sum()
        stats[STAT_NONFINITE] = (~np.isfinite(x)).sum()
    return {"kept": kept, "adv": adv, "penalty": pen, "dout": dout, "anchor_next": nxt, "stats": stats,
            "abs_adv": float(np.abs(terms[k]).sum()), "abs_pen": abs_pen, "abs_x": float(np.abs(x).sum())}


def anchor_recursion(means_real, means_fake, decay):
    """The anchors after every D iteration: it 0 takes the batch mean itself (decay 0), later ones the moving average.
    -> list of (anchor_real, anchor_fake)."""
    out, ar, af = [], 0.0, 0.0
    for it, (mr, mf) in enumerate(zip(means_real, means_fake)):
        d = 0.0 if it == 0 else decay
        ar, af = d * ar + (1.0 - d) * mr, d * af + (1.0 - d) * mf
        out.append((ar, af))
    return out

"""The Inception Score (Salimans et al. 2016) and the class-fidelity metrics of a classifier's logits on generated samples: does a
clip conditioned on class c look like class c to a classifier, and which classes collapse into which.  No counterpart in the
reference.

The classifier is the caller's: any callable `clips -> logits [B, C]` on the device -- a C3D network fine-tuned on UCF-101 gives the
Inception Score video GANs publish.  The statistic is this package's: per-split softmax column sums, sum p log p, top-1 / top-5
hits, the labels' log likelihood and a confusion matrix, accumulated in fp64 on the device by libdvdx_cls.so (deterministic, no
atomics; include/dvdx_cls.h), streamed batch by batch so that no logits are kept.  Only the small state crosses to the host, where
the metrics are finished in numpy fp64."""
import numpy as np
import torch

from . import lib as L
from .helpers import to_device_async

_DTYPES = {torch.float32: L.CLS_F32, torch.bfloat16: L.CLS_BF16, torch.float16: L.CLS_F16}


class LogitStats:
    """Running sums of logits rows [n, n_classes] (device fp32 / bf16 / fp16) over a sample set of n_total rows cut into `splits`
    contiguous splits: global row i belongs to split (i * splits) // n_total.  `update(logits, labels=None)` takes the next rows
    (labels: integers [n], the classes the samples were conditioned on; either every update of a set has them or none), keeps
    the running row offset, and makes no host sync; `result()` is the one synchronising read.  confusion=True also keeps the
    int64 [n_classes, n_classes] matrix [label, argmax]."""

    def __init__(self, n_classes, n_total, *, splits=10, confusion=False, device=None):
        self.n_classes, self.n_total, self.splits = int(n_classes), int(n_total), int(splits)
        if not 1 <= self.n_classes <= L.CLS_MAX_CLASSES:
            raise ValueError(f"n_classes={n_classes}: 1 to {L.CLS_MAX_CLASSES}")
        if not 1 <= self.n_total <= L.CLS_MAX_TOTAL:
            raise ValueError(f"n_total={n_total}")
        if not 1 <= self.splits <= min(L.CLS_MAX_SPLITS, self.n_total):
            raise ValueError(f"splits={splits}: 1 to min({L.CLS_MAX_SPLITS}, n_total={self.n_total})")
        self.device = torch.device("cuda" if device is None else device)
        self.rows, self.labelled = 0, None
        self._state = torch.zeros(self.splits, self.n_classes + L.CLS_NSTAT, dtype=torch.float64, device=self.device)
        self._confusion = (torch.zeros(self.n_classes, self.n_classes, dtype=torch.int64, device=self.device) if confusion
                           else None)

    def update(self, logits, labels=None):
        if logits.dim() != 2 or logits.shape[1] != self.n_classes:
            raise ValueError(f"logits must be [n, {self.n_classes}], got {tuple(logits.shape)}")
        if logits.dtype not in _DTYPES:
            raise TypeError(f"logits of dtype {logits.dtype}: float32, bfloat16 or float16")
        n = logits.shape[0]
        if labels is not None and (labels.dim() != 1 or labels.shape[0] != n or labels.dtype.is_floating_point):
            raise ValueError(f"labels must be integers [{n}], got {labels.dtype} {tuple(labels.shape)}")
        if self.rows and (labels is not None) != self.labelled:
            raise ValueError("either every update of a sample set has labels or none has")
        if self._confusion is not None and labels is None:
            raise ValueError("a confusion matrix needs labels")
        if self.rows + n > self.n_total:
            raise ValueError(f"{self.rows} + {n} rows, but n_total={self.n_total}")
        if n == 0:
            return self
        self.labelled = labels is not None
        logits = to_device_async(logits, self.device).contiguous()
        if labels is not None:                                              # host labels go up through pinned memory: no stall
            labels = to_device_async(labels.to(torch.int32), self.device).contiguous()
        so = L.cls_lib()
        for lo in range(0, n, L.CLS_MAX_ROWS):
            part = logits[lo:lo + L.CLS_MAX_ROWS]
            ws = torch.empty(so.dvdx_cls_ws_bytes(part.shape[0], self.n_classes), dtype=torch.uint8, device=self.device)
            L.cls_check(so.dvdx_cls_update(_DTYPES[part.dtype], L.ptr(part), None if labels is None else L.ptr(labels[lo:lo + L.CLS_MAX_ROWS]),
                                           part.shape[0], self.n_classes, self.rows, self.n_total, self.splits, L.ptr(self._state),
                                           L.ptr(self._confusion), L.ptr(ws), ws.numel(), L.stream()))
            self.rows += part.shape[0]
        return self

    def result(self):
        """-> dict, finished on the host in fp64 from the [splits, n_classes + 8] state:
        is_mean, is_std: mean and population standard deviation (numpy's default, as in the common implementation) over the splits
        of IS_s = exp(A_s / n_s - sum_c q_sc log q_sc), q_s = colsum_s / n_s (a split without a good row is left out);
        is_all: the score of all rows as one split = exp(h_marginal - h_conditional); h_marginal = H(y), the entropy of the mean
        prediction (diversity), h_conditional = H(y | x), the mean entropy of a prediction (sharpness);
        n, n_bad: rows that entered the sums, rows left out for a non-finite logit; n_bad_label: good rows whose label lay outside
        [0, n_classes) (they enter the sums above only);  confusion: int64 numpy [label, argmax] or None.
        With labels also top1, top5 (the label's rank among the logits, ties broken towards the lower index), mean_log_lik (mean
        log p of the label) and per_class_top1 [n_classes] = confusion[c, c] / sum(confusion[c]) (NaN for a class without rows;
        None when no confusion matrix is kept).
        The sums hold the rows given so far, split as rows of the whole set of n_total."""
        C = self.n_classes
        state = self._state.cpu().numpy()                                   # the one wait for the device
        conf = None if self._confusion is None else self._confusion.cpu().numpy()
        col, st = state[:, :C], state[:, C:]

        def entropy(q):
            q = q[q > 0]
            return float(-(q * np.log(q)).sum())

        nan = float("nan")
        scores = np.array([np.exp(st[s, L.CLS_STAT_A] / st[s, L.CLS_STAT_N] + entropy(col[s] / st[s, L.CLS_STAT_N]))
                           for s in range(self.splits) if st[s, L.CLS_STAT_N] > 0])
        tot = st.sum(axis=0)
        n = float(tot[L.CLS_STAT_N])
        out = {"is_mean": float(scores.mean()) if scores.size else nan, "is_std": float(scores.std()) if scores.size else nan,
               "h_marginal": entropy(col.sum(axis=0) / n) if n else nan, "h_conditional": float(-tot[L.CLS_STAT_A] / n) if n else nan,
               "n": int(n), "n_bad": int(tot[L.CLS_STAT_BAD]), "n_bad_label": int(tot[L.CLS_STAT_BAD_LABEL]), "confusion": conf}
        out["is_all"] = float(np.exp(out["h_marginal"] - out["h_conditional"])) if n else nan
        if self.labelled:
            k = float(tot[L.CLS_STAT_LABELLED])
            out["top1"] = float(tot[L.CLS_STAT_TOP1] / k) if k else nan
            out["top5"] = float(tot[L.CLS_STAT_TOP5] / k) if k else nan
            out["mean_log_lik"] = float(tot[L.CLS_STAT_LOGLIK] / k) if k else nan
            out["per_class_top1"] = None
            if conf is not None:
                per = conf.sum(axis=1).astype(np.float64)
                out["per_class_top1"] = np.where(per > 0, np.diag(conf) / np.where(per > 0, per, 1.0), nan)
        return out


def inception_score(logits, splits=10):
    """(mean, std) of the Inception Score over `splits` splits of logits [n, C] on the device."""
    res = LogitStats(logits.shape[1], logits.shape[0], splits=splits, device=logits.device).update(logits).result()
    return res["is_mean"], res["is_std"]


def class_fidelity(logits, labels):
    """The result() of logits [n, C] against the labels [n] the samples were conditioned on, as one split with the confusion
    matrix: top1, top5, mean_log_lik, per_class_top1, confusion, ..."""
    stats = LogitStats(logits.shape[1], logits.shape[0], splits=1, confusion=True, device=logits.device)
    return stats.update(logits, labels).result()

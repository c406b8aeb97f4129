"""Distribution distances of sample features: the statistic of FID / FVD (Frechet distance between the Gaussians fitted to two
feature sets; Heusel et al. 2017, Unterthiner et al. 2018) and of KID (unbiased MMD^2 with the cubic polynomial kernel; Binkowski
et al. 2018).  No counterpart in the reference.

The feature extractor is the caller's: any callable `clips -> features [B, d]` (fp32, on the device) -- an I3D or Inception
network with the published weights gives FVD / FID / KID.  The project ships one extractor it owns, `DiscFeatures`: the pooled
final activation of a discriminator.  Distances in that space compare generator checkpoints, averaged against live weights and
truncation values -- but ONLY under one fixed discriminator snapshot: the live discriminator moves with every step, and numbers
taken under different discriminator weights are not comparable.

Second moments and kernel sums run on the device (libdvdgan_hip_eval.so, fp32 MFMA with fp64 state, deterministic); only the
final small tables cross to the host.  The last step of the Frechet distance, O(d^3) on two d x d matrices once per evaluation,
is numpy fp64 on the host on purpose.

prdc() adds the k-nearest-neighbour manifold statistics -- improved precision / recall (Kynkaanniemi et al. 2019) and density /
coverage (Naeem et al. 2020) -- which tell poor samples from too few kinds of samples; their pairwise distances run on
libdvdgan_hip_prdc.so."""
import numpy as np
import torch

from . import kern as K
from . import lib as L


class FeatureStats:
    """Running mean and covariance of feature rows [n, d] (device fp32), accumulated about a pivot: the column mean of the first
    batch, computed on the device.  Products of fl(x - pivot) stay small where the features sit far from zero, so the fp32
    products do not cancel; the state is fp64 (dvd_eval_moments_update).  `update` makes no host sync; `mean` / `cov` copy the
    state to the host once and finish in fp64:  mean = pivot + S1 / n,  cov = (S2 - S1 S1^T / n) / (n - 1)."""

    def __init__(self, d, device):
        self.d, self.device, self.n = int(d), torch.device(device), 0
        self._pivot, self._state = K.eval_moments_state(self.d, self.device)
        self._fixed = None                    # (mean, cov) of statistics read from a file: no state to add to

    def update(self, feats):
        if self._fixed is not None:
            raise RuntimeError("these statistics were loaded as (n, mean, cov): there is no running state to add to")
        if feats.dim() != 2 or feats.shape[1] != self.d:
            raise ValueError(f"features must be [n, {self.d}], got {tuple(feats.shape)}")
        if feats.shape[0] == 0:
            return self
        K.eval_moments_update(feats.to(self.device, torch.float32), self._pivot, self._state, first=self.n == 0)
        self.n += feats.shape[0]
        return self

    def _host(self):
        """(pivot [d], S1 [d], S2 [d, d] mirrored from the upper triangle), fp64 numpy."""
        d, T = self.d, L.EVAL_TILE
        nb = (d + T - 1) // T
        state = self._state.cpu().numpy()
        tiles = state[d:].reshape(-1, T, T)
        full = np.zeros((nb * T, nb * T))
        t = 0
        for i in range(nb):
            for j in range(i, nb):
                full[i * T:(i + 1) * T, j * T:(j + 1) * T] = tiles[t]
                t += 1
        full = full[:d, :d]
        s2 = np.triu(full) + np.triu(full, 1).T
        return self._pivot.cpu().numpy().astype(np.float64), state[:d].copy(), s2

    def mean(self):
        if self._fixed is not None:
            return self._fixed[0].copy()
        if self.n < 1:
            raise RuntimeError("no features yet")
        c, s1, _ = self._host()
        return c + s1 / self.n

    def cov(self):
        if self._fixed is not None:
            return self._fixed[1].copy()
        if self.n < 2:
            raise RuntimeError(f"a covariance needs at least two rows, got {self.n}")
        _, s1, s2 = self._host()
        return (s2 - np.outer(s1, s1) / self.n) / (self.n - 1)

    # ---- the running state (to go on accumulating elsewhere) and the finished statistics (computed once for the real set)
    def state_dict(self):
        if self._fixed is not None:
            return {"d": self.d, "n": self.n, "mean": self._fixed[0].copy(), "cov": self._fixed[1].copy()}
        return {"d": self.d, "n": self.n, "pivot": self._pivot.cpu(), "state": self._state.cpu()}

    def load_state_dict(self, sd):
        if int(sd["d"]) != self.d:
            raise ValueError(f"statistics of width {sd['d']} do not fit d={self.d}")
        self.n = int(sd["n"])
        if "mean" in sd:
            mean, cov = np.asarray(sd["mean"], np.float64), np.asarray(sd["cov"], np.float64)
            if mean.shape != (self.d,) or cov.shape != (self.d, self.d):
                raise ValueError(f"mean {mean.shape} / cov {cov.shape} do not fit d={self.d}")
            self._fixed = (mean.copy(), cov.copy())
        else:
            self._fixed = None
            self._pivot.copy_(sd["pivot"])
            self._state.copy_(sd["state"])
        return self

    def save(self, path):
        """n, mean, cov as an .npz (the path is used as given: hand it a name ending in .npz)."""
        with open(path, "wb") as f:
            np.savez(f, n=np.int64(self.n), mean=self.mean(), cov=self.cov())

    @classmethod
    def load(cls, path, device="cpu"):
        """Statistics written by save(): mean / cov are served from the file, update() is refused.  Needs no GPU."""
        with np.load(path) as z:
            n, mean, cov = int(z["n"]), z["mean"].astype(np.float64), z["cov"].astype(np.float64)
        self = cls.__new__(cls)
        self.d, self.device, self.n = int(mean.shape[0]), torch.device(device), n
        self._pivot = self._state = None
        self._fixed = (mean, cov)
        if cov.shape != (self.d, self.d):
            raise ValueError(f"{path}: mean {mean.shape} and cov {cov.shape} do not fit")
        return self


def _mean_cov(s):
    if isinstance(s, FeatureStats):
        return s.mean(), s.cov()
    mean, cov = s
    return np.asarray(mean, np.float64), np.asarray(cov, np.float64)


def _psd_eigenvalues(m):
    """Eigenvalues of a symmetric matrix that is positive semi-definite up to rounding: negative ones and those below the
    rank cutoff d eps max(lambda) (the noise level of eigvalsh for a zero eigenvalue) are exact zeros."""
    w = np.linalg.eigvalsh((m + m.T) * 0.5)
    top = max(float(w[-1]), 0.0)
    return np.where(w > top * m.shape[0] * np.finfo(np.float64).eps, w, 0.0)


def frechet_distance(a, b):
    """|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a S_b)^(1/2) of two FeatureStats or (mean, cov) pairs, fp64 on the host.
    The trace term is the sum of sqrt(lambda) over the eigenvalues of the symmetric matrix S_a^(1/2) S_b S_a^(1/2), with S_a^(1/2)
    from an eigendecomposition of S_a: symmetric matrices throughout, so no complex numbers appear and rank-deficient
    covariances (fewer rows than features) are served."""
    (ma, ca), (mb, cb) = _mean_cov(a), _mean_cov(b)
    if ma.shape != mb.shape or ca.shape != cb.shape or ca.shape != (ma.shape[0],) * 2:
        raise ValueError(f"statistics of different widths: {ma.shape} {ca.shape} / {mb.shape} {cb.shape}")
    w, v = np.linalg.eigh((ca + ca.T) * 0.5)
    top = max(float(w[-1]), 0.0)
    w = np.where(w > top * ca.shape[0] * np.finfo(np.float64).eps, w, 0.0)
    root = (v * np.sqrt(w)) @ v.T
    lam = _psd_eigenvalues(root @ cb @ root)
    diff = ma - mb
    return float(diff @ diff + np.trace(ca) + np.trace(cb) - 2.0 * np.sqrt(lam).sum())


def kid_subsets(n, m, n_subsets=100, subset_size=1000, seed=0):
    """The row tables of kid(): (ix, iy) int32 [n_subsets, s] with s = min(subset_size, n, m); every subset is drawn without
    replacement from a private numpy generator seeded with `seed`, x's rows before y's, subset by subset."""
    s = min(int(subset_size), int(n), int(m))
    if s < 2:
        raise ValueError(f"a subset needs at least two rows of each set (subset_size={subset_size}, n={n}, m={m})")
    if int(n_subsets) < 1:
        raise ValueError(f"n_subsets={n_subsets}")
    rng = np.random.default_rng(int(seed))
    ix = np.empty((int(n_subsets), s), np.int32)
    iy = np.empty((int(n_subsets), s), np.int32)
    for b in range(int(n_subsets)):
        ix[b] = rng.choice(int(n), s, replace=False)
        iy[b] = rng.choice(int(m), s, replace=False)
    return ix, iy


def kid(x, y, *, n_subsets=100, subset_size=1000, seed=0):
    """Kernel distance of two feature sets x [n, d], y [m, d] (device fp32): the unbiased MMD^2 with k(a, b) = (a.b / d + 1)^3 on
    n_subsets subsets of subset_size rows of each (kid_subsets; subset_size is clipped to min(n, m)) ->
    {"mean", "std" (over the subsets, population form), "values" fp64 [n_subsets]}.  dvd_eval_kid; one copy to the host."""
    ix, iy = kid_subsets(x.shape[0], y.shape[0], n_subsets, subset_size, seed)
    values, _ = K.eval_kid(x, y, torch.from_numpy(ix), torch.from_numpy(iy))
    values = values.cpu().numpy()
    return {"mean": float(values.mean()), "std": float(values.std()), "values": values}


def knn_radii(x, k, pivot=None):
    """Squared distance of every row of x [n, d] (device fp32) to its k-th nearest OTHER row (by position: duplicate rows give zero
    radii) -> device fp64 [n].  Distances are those of fl32(x - pivot): d2 = |a|^2 + |b|^2 - 2 a.b with fp64 norms and the dot
    product on fp32 MFMA (dvd_prdc_knn_radii); pivot fp32 [d], None = zeros.  No host sync."""
    return K.eval_knn_radii(x, k, pivot)


def prdc(real, fake, k=5):
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of generated features
    fake [m, d] against real features real [n, d] (device fp32), with B(x_i) the ball about x_i through its k-th nearest
    neighbour WITHIN ITS OWN SET:
      precision = share of fake rows inside some real ball          recall   = share of real rows inside some fake ball
      density   = sum_j #{real balls holding fake_j} / (k m)        coverage = share of real rows whose ball holds a fake row
    -> {"precision", "recall", "density", "coverage", "k", "n_real", "n_fake"}.  The paper of precision / recall uses k = 3, the
    one of density / coverage k = 5.  All distances are taken about one pivot, the column mean of `real` (far from the origin the
    fp32 dot products would otherwise cancel); radii and counts run on the device (libdvdgan_hip_prdc.so: fp32 MFMA products,
    fp64 norms and comparisons, deterministic), one copy of the per-row tables crosses to the host, and the ratios are integers
    and fp64 there.  A comparison d2 <= r2 is decided up to the rounding of the fp32 dot product (include/dvdgan_hip_prdc.h).
    As for FeatureStats: with discriminator features ("Dt" / "Ds") the values compare ONLY under one fixed discriminator
    snapshot."""
    if real.dim() != 2 or fake.dim() != 2:
        raise ValueError(f"feature sets must be [rows, d], got {tuple(real.shape)} / {tuple(fake.shape)}")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"real {tuple(real.shape)} and fake {tuple(fake.shape)} differ in the feature width")
    n, m, k = real.shape[0], fake.shape[0], int(k)
    if k < 1 or k >= min(n, m):
        raise ValueError(f"k={k} needs 1 <= k < min(n, m) = {min(n, m)}")
    if k > L.PRDC_MAX_K:
        raise ValueError(f"k={k} above {L.PRDC_MAX_K}")
    pivot = K.eval_column_mean(real)
    r2_real, r2_fake = K.eval_knn_radii(real, k, pivot), K.eval_knn_radii(fake, k, pivot)
    cnt_fr, _ = K.eval_ball_count(fake, real, r2_real, pivot)                # per fake row: real balls that hold it
    cnt_rf, dmin_rf = K.eval_ball_count(real, fake, r2_fake, pivot)          # per real row: fake balls that hold it; nearest fake row
    table = torch.cat([cnt_fr.double(), cnt_rf.double(), dmin_rf, r2_real]).cpu().numpy()      # the one copy to the host
    cnt_fr, cnt_rf = table[:m].astype(np.int64), table[m:m + n].astype(np.int64)
    dmin_rf, r2_real = table[m + n:m + 2 * n], table[m + 2 * n:]
    return {"precision": float(np.count_nonzero(cnt_fr > 0)) / m, "recall": float(np.count_nonzero(cnt_rf > 0)) / n,
            "density": float(int(cnt_fr.sum())) / (k * m), "coverage": float(np.count_nonzero(dmin_rf <= r2_real)) / n,
            "k": k, "n_real": n, "n_fake": m}


class DiscFeatures:
    """A SpatialDiscriminator / TemporalDiscriminator as a feature extractor: its forward pass up to the tensor it hands to the
    projection head, then dvd_eval_pool_features -- the head's pooled feature sum_positions relu(.) [frames, 16 chn], averaged
    over `group` consecutive frames (None: all frames of a clip, i.e. the k sampled frames of D_s or the T / 4 of D_t; 1: per
    frame).  Input in the network's own layout (D_s: [B, k, 3, H, W], D_t: [B, 3, T, h, w] after vid_downsample) -> fp32
    [B * frames / group, 16 chn].  Runs without gradients in eval mode; the spectral-norm u / v, which advance with every forward
    pass, are put back afterwards, so the network's state is bit-equal before and after."""

    def __init__(self, net, *, group=None):
        from .disc_nets import _DiscBase
        if not isinstance(net, _DiscBase):
            raise TypeError(f"DiscFeatures takes a SpatialDiscriminator / TemporalDiscriminator, got {type(net).__name__}")
        self.net, self.group = net, group

    @torch.no_grad()
    def __call__(self, x):
        from .sn_layers import clear_spectral_norm, prefetch_spectral_norm
        net, seen = self.net, []
        frozen = [p.data for p in net.parameters() if not p.requires_grad] + list(net.buffers())
        saved = [t.clone() for t in frozen]
        was_training = net.training

        def capture(feat, class_id, repeat):
            seen.append((feat, repeat))
            return None

        net.eval()
        net._head = capture                                   # shadows the method for this call
        sn = prefetch_spectral_norm(net, net.compute_dtype)
        try:
            net._forward(x, None)
        finally:
            clear_spectral_norm(sn)
            del net._head
            net.train(was_training)
            for t, old in zip(frozen, saved):
                t.copy_(old)
        feat, frames = seen[0]
        return K.eval_pool_features(feat, frames if self.group is None else self.group)

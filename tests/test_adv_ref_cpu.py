"""CPU checks of tests/adv_ref.py, the fp64 statement of dvd_adv_loss_ex the GPU tests compare the kernel with: its gradient
against torch autograd of the written formula, its selection against torch.topk and the tie rule, the identity behind the
data-parallel anchor exchange, the schedule of the kept count, and the entry point's refusals (return codes, nothing launched)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import adv_ref as R


def _formula(x, group, hinge, real, kept, keep, lecam, a, gs):
    """The loss whose gradient dvd_adv_loss_ex writes, in torch fp64: adversarial mean over the kept logits + lecam * P."""
    n = x.numel()
    sgn = -1.0 if real else 1.0
    v = sgn * x
    terms = torch.relu(1.0 + v) if hinge else v
    mask = torch.as_tensor(np.repeat(kept, group))
    div = float(keep * group if keep > 0 else n)
    loss = terms[mask].sum() / div
    if lecam > 0:
        r = torch.relu(x - a) if real else torch.relu(a - x)
        loss = loss + lecam * ((r * r).sum() / n)
    return loss * gs


@pytest.mark.parametrize("hinge", [True, False])
@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("keep", [0, 1, 2, 3])
@pytest.mark.parametrize("lecam", [0.0, 0.3])
def test_dout_is_the_gradient_of_the_formula(hinge, real, keep, lecam):
    g = torch.Generator().manual_seed(11 + keep)
    group, B, gs, a = 4, 3, 0.37, 0.21
    x = (torch.randn(B * group, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    ref = R.adv_ref(x.detach().numpy(), group, hinge, real, keep, lecam, anchor_other=a, grad_scale=gs)
    loss = _formula(x, group, hinge, real, ref["kept"], keep, lecam, a, gs)
    loss.backward()
    want = x.grad.numpy()
    if lecam == 0:
        assert np.array_equal(ref["dout"], want)          # piecewise constant: exactly sgn * gs / div or 0
        assert set(np.unique(np.abs(ref["dout"]))) <= {0.0, gs / (keep * group if keep else B * group)}
    else:
        np.testing.assert_allclose(ref["dout"], want, rtol=1e-13, atol=1e-16)
    assert math.isclose(ref["adv"] * gs + lecam * ref["penalty"] * gs, float(loss.detach()), rel_tol=1e-13, abs_tol=1e-15)
    if keep:
        assert ref["kept"].sum() == keep
        if lecam == 0:
            assert np.all(ref["dout"][~np.repeat(ref["kept"], group)] == 0)


@pytest.mark.parametrize("B,group,keep", [(3, 8, 1), (3, 8, 2), (7, 1, 3), (64, 4, 17), (64, 4, 64), (4096, 2, 1000)])
def test_selection_is_topk_of_the_group_means(B, group, keep):
    g = torch.Generator().manual_seed(B + keep)
    x = torch.randn(B, group, generator=g, dtype=torch.float64)
    s = x.mean(dim=1)
    assert torch.unique(s).numel() == B                        # no ties: the set is decided by the values alone
    want = np.zeros(B, dtype=bool)
    want[torch.topk(s, keep).indices.numpy()] = True
    assert np.array_equal(R.select(R.scores(x.numpy().reshape(-1), group), keep), want)


def test_ties_go_to_the_lower_index_and_nan_is_kept():
    s = np.array([2.0, 5.0, 5.0, 1.0, 5.0, 2.0])
    assert R.select(s, 1).tolist() == [False, True, False, False, False, False]
    assert R.select(s, 2).tolist() == [False, True, True, False, False, False]
    assert R.select(s, 4).tolist() == [True, True, True, False, True, False]
    assert R.select(s, 6).all()
    # through the logits: integer values, equal group sums
    x = np.array([1, 3, 2, 2, 0, 4, 5, -5], dtype=np.float64)            # means 2, 2, 2, 0
    assert R.adv_ref(x, group=2, keep=2)["kept"].tolist() == [True, True, False, False]
    # a NaN score is ahead of nothing and nothing is ahead of it: it is kept on top of the `keep` best of the others
    s = np.array([1.0, np.nan, 3.0, 2.0])
    assert R.select(s, 1).tolist() == [False, True, True, False]
    out = R.adv_ref(np.array([1.0, np.nan, np.inf, 2.0]), group=1, keep=1)
    assert out["stats"][R.STAT_NONFINITE] == 2 and out["kept"].tolist() == [False, True, True, False]


def test_average_of_anchors_is_the_anchor_of_the_average():
    """What the one all-reduce per D iteration relies on: the update is linear in the batch mean, so with equal shards the
    moving average of the ranks' mean logit equals the mean of the ranks' moving averages."""
    rng = np.random.default_rng(5)
    ranks, iters, decay = 4, 50, 0.99
    means = rng.normal(size=(ranks, iters))
    per_rank = np.array([[a for a, _ in R.anchor_recursion(m, m, decay)] for m in means])
    of_global = np.array([a for a, _ in R.anchor_recursion(means.mean(axis=0), means.mean(axis=0), decay)])
    np.testing.assert_allclose(per_rank.mean(axis=0), of_global, rtol=0, atol=1e-15)
    # ... and exchanging every iteration (each rank continues from the averaged anchor) gives the same
    a = np.zeros(ranks)
    for it in range(iters):
        d = 0.0 if it == 0 else decay
        a = d * a + (1.0 - d) * means[:, it]
        a[:] = a.mean()
        assert abs(a[0] - of_global[it]) < 1e-15
    assert R.anchor_recursion([2.0], [-3.0], 0.9) == [(2.0, -3.0)]       # iteration 0 needs no initial value


def test_keep_schedule():
    from dvd_gan_amd.train_step import topk_keep
    assert topk_keep(64, 0.5, 0.99, 0) == 64
    assert topk_keep(64, 0.5, 0.99, 1) == 63                   # floor(63.36)
    assert topk_keep(64, 0.5, 0.99, 10) == 57                  # floor(64 * 0.99^10 = 57.88)
    assert topk_keep(64, 0.5, 0.99, 68) == 32 and topk_keep(64, 0.5, 0.99, 10 ** 4) == 32     # 64 * 0.99^68 = 32.3: the floor holds
    assert topk_keep(3, 0.5, 0.5, 5) == 2                      # ceil(1.5)
    assert topk_keep(2, 0.5, 0.5, 1) == 1 and topk_keep(2, 0.5, 0.5, 0) == 2
    assert topk_keep(5, 1.0, 0.1, 9) == 5 and topk_keep(8, 0.01, 0.1, 9) == 1
    for B in (1, 2, 3, 64):
        ks = [topk_keep(B, 0.3, 0.9, e) for e in range(60)]
        assert ks[0] == B and ks == sorted(ks, reverse=True) and ks[-1] == max(1, math.ceil(0.3 * B))


def test_entry_point_is_declared_and_refuses_bad_arguments():
    """dvd_adv_loss_ex: typed from lib.ADV_SIGNATURES, its constants are the header's, and the refusals come back as codes before
    any launch (the placeholder pointers are never dereferenced)."""
    from dvd_gan_amd import lib as L
    lib = L.adv_lib()
    assert L.ADV_SIGNATURES["dvd_adv_loss_ex"].replace(" ", "") == "ipliiiifpppfppfpp"
    assert (L.ADV_NSTAT, L.ADV_MAX_SAMPLES) == (R.NSTAT, 4096)
    assert [getattr(L, "ADV_STAT_" + k) for k in ("MEAN", "SIGN", "ACTIVE", "ADV", "LECAM", "ANCHOR", "KEPT", "NONFINITE")] == list(range(8))
    p = C.c_void_p(16)
    call = lambda n, group, keep, lecam=0.0, other=None, prev=None, nxt=None, decay=0.0: lib.dvd_adv_loss_ex(
        p, n, group, 1, 1, keep, lecam, other, prev, nxt, decay, p, p, 1.0, None, None)
    assert call(25, 8, 0) == -1                                 # n % group != 0
    assert call(24, 8, 4) == -1 and call(24, 8, -1) == -1       # keep > n / group, keep < 0
    assert call(24, 0, 0) == -1 and call(0, 1, 0) == -1
    assert call(24, 8, 0, lecam=0.1) == -1                      # the LeCam term needs the other kind's anchor
    assert call(24, 8, 0, lecam=-1.0, other=p) == -1 and call(24, 8, 0, lecam=float("nan"), other=p) == -1
    assert call(24, 8, 0, nxt=p, decay=1.0) == -1 and call(24, 8, 0, nxt=p, decay=0.5) == -1      # decay range; decay > 0 reads prev
    assert call((L.ADV_MAX_SAMPLES + 1) * 2, 2, 1) == -2        # more samples than the selection serves
    assert call(2 ** 33 + 2, 2, 2 ** 31 - 1) == -2              # a long long n survives whole

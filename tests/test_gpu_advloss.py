"""dvd_adv_loss_ex (csrc/adv/adv_loss_ex.hip, libdvdgan_hip_adv.so) against tests/adv_ref.py, the fp64 statement of its header comment: top-k selection, the
adversarial and the LeCam term, the anchor update and the logit statistics in one launch of one workgroup.

Exact where the header makes it exact: with everything off the results are dvd_adv_loss's bits, the kept set is the reference's,
the adversarial gradient is sgn * grad_scale / (keep * group) evaluated in fp32 or exactly 0.  The sums are held to a rounding
bound that is counted, not measured (sum_bound)."""
import numpy as np
import pytest
import torch

import adv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
E32 = 2.0 ** -24
# (n, group): one logit; a few, group 1; B = 3 samples of 8; past one stride of the 1024 threads; the selection's cap of 4096 samples
SHAPES = [(1, 1), (7, 1), (24, 8), (1030, 1), (4096 * 2, 2)]
f32 = lambda v: float(np.float32(v))       # the parameters reach the kernel as floats: the reference takes the same values
ANCHOR = f32(0.2137)


def note(name, value):
    print(f"MEASURED {name}: {value:.3e}")


def sum_bound(n, sum_abs_terms, divisor, term_roundings):
    """|fp32 mean - exact mean| of the kernel's reductions, first order in 2^-24, by counting the roundings one term passes
    through on its way to the result, times 2^-24, times the sum of |terms|, over the divisor:
      term_roundings   forming the term from the stored logit (0 for x itself, 1 for 1 + x, 3 for relu(x - a)^2: the
                       difference, and its square's two factors and product -- (1 + e)^2 (1 + e') ~ 1 + 3 e)
      ceil(n/1024) - 1 additions of the thread's strided sum (thread t adds x[t], x[t + 1024], ... in order)
      6                xor-shuffle levels of wave_sum over the 64 lanes
      6                the same levels over the 16 per-wave partials (block_sum's second stage; the upper lanes add zeros)
      1                the division
    + 1 for everything of second order (R^2 2^-48 against R 2^-24: R < 2^12 here)."""
    R_ = term_roundings + (-(-n // 1024) - 1) + 6 + 6 + 1 + 1
    return R_ * E32 * sum_abs_terms / divisor


def grid_logits(n, group, seed):
    """Logits on the grid 2^-8 whose group sums are (a permutation of the samples) * 2^-8: all sums are exact in fp32 and pairwise
    different, so the group means differ by 2^-8 / group -- asserted against the rounding bound of the score in the test."""
    B = n // group
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-512, 513, (B, group), generator=g).double()                  # [-2, 2] in units of 2^-8
    target = (torch.randperm(B, generator=g).double() - B // 2)
    x[:, 0] = target - x[:, 1:].sum(dim=1)
    return (x / 256.0).reshape(-1).float()


def run(x, group, hinge, real, keep=0, lecam=0.0, other=None, prev=None, decay=None, gs=1.0, loss0=0.0, stats=True):
    """One dvd_adv_loss_ex call -> (code, loss, dout, anchor_next, stats) as numpy (None where not requested)."""
    from dvd_gan_amd import lib as L
    xd = x.to(DEV)
    loss = torch.tensor([loss0], dtype=torch.float32, device=DEV)
    dout = torch.full_like(xd, 7.0)
    anc = torch.tensor([0.0 if other is None else other, 0.0 if prev is None else prev, -9.0], dtype=torch.float32, device=DEV)
    st = torch.full((L.ADV_NSTAT,), -9.0, dtype=torch.float32, device=DEV) if stats else None
    code = L.adv_lib().dvd_adv_loss_ex(L.ptr(xd), xd.numel(), group, int(hinge), int(real), keep, lecam,
                                   L.ptr(anc[0:1]) if other is not None else None, L.ptr(anc[1:2]) if prev is not None else None,
                                   L.ptr(anc[2:3]) if decay is not None else None, 0.0 if decay is None else decay,
                                   L.ptr(loss), L.ptr(dout), gs, L.ptr(st), L.stream())
    torch.cuda.synchronize()
    return (code, loss.cpu().numpy()[0], dout.cpu().numpy(), anc.cpu().numpy()[2] if decay is not None else None,
            st.cpu().numpy() if stats else None)


@pytest.mark.parametrize("n,group", SHAPES + [(3000, 1)])
def test_everything_off_is_the_old_launch_bit_for_bit(n, group):
    from dvd_gan_amd import lib as L
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 2
    x[::7] = 1.0
    x[3::7] = -1.0                                                        # on the hinge's kink
    for hinge in (1, 0):
        for real in (1, 0):
            xd = x.to(DEV)
            loss = torch.tensor([0.125], device=DEV)
            dout = torch.empty_like(xd)
            L.check(L.lib().dvd_adv_loss(L.ptr(xd), n, hinge, real, L.ptr(loss), L.ptr(dout), 0.75, L.stream()))
            code, loss2, dout2, _, _ = run(x, group, hinge, real, gs=0.75, loss0=0.125, stats=False)
            assert code == 0
            assert loss.cpu().numpy().view(np.uint32)[0] == np.array([loss2]).view(np.uint32)[0]
            assert np.array_equal(dout.cpu().numpy().view(np.uint32), dout2.view(np.uint32))
            # ... and asking for the statistics changes neither
            code, loss3, dout3, _, st = run(x, group, hinge, real, gs=0.75, loss0=0.125)
            assert code == 0 and loss3 == loss2 and np.array_equal(dout3.view(np.uint32), dout2.view(np.uint32))
            assert st[R.STAT_KEPT] == n // group and st[R.STAT_NONFINITE] == 0 and st[R.STAT_LECAM] == 0


@pytest.mark.parametrize("n,group", SHAPES)
def test_selection_gradient_and_sums(n, group):
    """Kept set (no ties), the adversarial gradient bit for bit, dropped logits exactly 0, the LeCam gradient per element, and every
    sum within sum_bound -- keep in {1, B - 1, B}, both real flags, hinge and wgan-gp, grad_scale != 1, an accumulating *loss."""
    B = n // group
    x = grid_logits(n, group, 31 + n)
    x64 = x.double().numpy()
    s = R.scores(x64, group)
    # the fp64 reference alone fixes the set: neighbouring scores differ by more than twice the rounding bound of a score (group
    # additions and a division; on this grid the fp32 sums are even exact)
    gap = np.diff(np.sort(s)).min() if B > 1 else np.inf
    assert gap > 2 * (group + 1) * E32 * np.abs(x64).reshape(B, group).sum(axis=1).max() / group
    gs, loss0, decay, prev, lecam = f32(0.37), 1.5, f32(0.9), f32(-0.4321), f32(0.3)
    worst = {}
    for keep in sorted({1, B - 1, B} - {0}):
        kept = R.select(s, keep)
        assert kept.sum() == keep
        for hinge in (True, False):
            for real in (True, False):
                ref = R.adv_ref(x64, group, hinge, real, keep, lecam, ANCHOR, prev, decay, gs, kept=kept)
                plain = R.adv_ref(x64, group, hinge, real, keep, 0.0, grad_scale=gs, kept=kept)
                code, loss, dout, nxt, st = run(x, group, hinge, real, keep, lecam, ANCHOR, prev, decay, gs, loss0)
                code0, _, dout0, _, _ = run(x, group, hinge, real, keep, gs=gs)
                assert code == 0 and code0 == 0
                # ---- kept set, read off the gradient of the wgan form (never 0 on a kept logit) and the statistics
                assert st[R.STAT_KEPT] == keep
                k = np.repeat(kept, group)
                if not hinge:
                    assert np.array_equal(dout0 != 0, k)
                # ---- adversarial gradient: sgn * gs / (keep * group) in fp32, or exactly 0
                sgn = np.float32(-1.0 if real else 1.0)
                step = sgn * np.float32(gs) / np.float32(keep * group)
                live = (1.0 + float(sgn) * x64 > 0) if hinge else np.ones(n, dtype=bool)
                want = np.where(k & live, step, np.float32(0.0)).astype(np.float32)
                assert np.array_equal(dout0.view(np.uint32), want.view(np.uint32))
                assert np.array_equal(dout0, plain["dout"].astype(np.float32))
                # ---- with the LeCam term: a handful of roundings per element (x - a, / n, gs * lecam, the product, the sum, and
                # the adversarial part's own division): 6 * 2^-24 of the two parts' magnitudes
                part = np.abs(plain["dout"]) + np.abs(ref["dout"] - plain["dout"])
                e = np.abs(dout - ref["dout"]) / np.maximum(6 * E32 * part, 1e-300)
                worst["lecam dout / bound"] = max(worst.get("lecam dout / bound", 0), float(e.max()))
                assert e.max() <= 1
                # ---- sums
                b_adv = sum_bound(n, ref["abs_adv"], keep * group, 1)
                b_pen = sum_bound(n, ref["abs_pen"], n, 3)
                b_mean = sum_bound(n, ref["abs_x"], n, 0)
                checks = {"adv": (st[R.STAT_ADV], ref["adv"], b_adv), "penalty": (st[R.STAT_LECAM], ref["penalty"], b_pen),
                          "mean": (st[R.STAT_MEAN], ref["stats"][R.STAT_MEAN], b_mean),
                          # *loss += adv: the term's bound and the rounding of the sum
                          "loss": (loss, loss0 + ref["adv"], b_adv + E32 * abs(loss0 + ref["adv"])),
                          # decay * prev + (1 - decay) * mean: (1 - decay), two products, one sum
                          "anchor": (nxt, ref["anchor_next"], (1 - decay) * b_mean + 4 * E32 * (abs(decay * prev) + abs((1 - decay) * ref["stats"][R.STAT_MEAN])))}
                for name, (got, want_, bound) in checks.items():
                    ratio = abs(float(got) - want_) / max(bound, 1e-300) if got != want_ else 0.0
                    worst[name + " / bound"] = max(worst.get(name + " / bound", 0), ratio)
                    assert ratio <= 1, (name, keep, hinge, real, got, want_, bound)
                # counts are exact (integers below 2^24), their division rounds once
                for idx in (R.STAT_SIGN, R.STAT_ACTIVE):
                    assert abs(st[idx] - ref["stats"][idx]) <= E32 * abs(ref["stats"][idx])
                assert st[R.STAT_ANCHOR] == np.float32(ANCHOR) and st[R.STAT_NONFINITE] == 0
    for name, v in worst.items():
        note(f"adv_loss_ex n={n} group={group} {name}", v)


@pytest.mark.parametrize("n,group", SHAPES)
def test_random_logits_without_selection(n, group):
    """Sums on logits that are on no grid (keep = 0), the first anchor update (decay 0 reads no previous value) and NULL stats."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(77 + n)) * 1.7
    x64 = x.double().numpy()
    for hinge in (True, False):
        for real in (True, False):
            lecam = f32(0.05)
            ref = R.adv_ref(x64, group, hinge, real, 0, lecam, ANCHOR, None, 0.0, 2.5)
            code, loss, dout, nxt, st = run(x, group, hinge, real, 0, lecam, ANCHOR, None, 0.0, 2.5, -0.75)
            assert code == 0
            b_mean = sum_bound(n, ref["abs_x"], n, 0)
            assert abs(st[R.STAT_ADV] - ref["adv"]) <= sum_bound(n, ref["abs_adv"], n, 1)
            assert abs(st[R.STAT_LECAM] - ref["penalty"]) <= sum_bound(n, ref["abs_pen"], n, 3)
            assert abs(st[R.STAT_MEAN] - ref["stats"][R.STAT_MEAN]) <= b_mean
            assert abs(nxt - ref["anchor_next"]) <= b_mean + 2 * E32 * abs(ref["anchor_next"])
            assert nxt == st[R.STAT_MEAN]                                   # decay 0: the mean itself
            assert abs(loss - (-0.75 + ref["adv"])) <= sum_bound(n, ref["abs_adv"], n, 1) + E32 * abs(-0.75 + ref["adv"])
            plain = R.adv_ref(x64, group, hinge, real, 0, 0.0, grad_scale=2.5)
            part = np.abs(plain["dout"]) + np.abs(ref["dout"] - plain["dout"])
            assert np.all(np.abs(dout - ref["dout"]) <= 6 * E32 * part)
            assert st[R.STAT_KEPT] == n // group
            code, loss_b, dout_b, nxt_b, none = run(x, group, hinge, real, 0, lecam, ANCHOR, None, 0.0, 2.5, -0.75, stats=False)
            assert code == 0 and none is None and loss_b == loss and nxt_b == nxt and np.array_equal(dout_b, dout)


def test_ties_go_to_the_lower_index():
    """Integer logits: the group sums are exact and many are equal."""
    g = torch.Generator().manual_seed(5)
    for B, group in ((3, 8), (7, 1), (200, 2), (1500, 1)):
        x = torch.randint(-2, 3, (B, group), generator=g).float()
        x[-1] = x[0].flip(0)                                                # the same logits in another order: the same sum
        x = x.reshape(-1)
        s = R.scores(x.double().numpy(), group)
        assert np.unique(s).size < B                                        # there are ties
        for keep in sorted({1, B // 2, B - 1, B}):
            kept = R.select(s, keep)
            code, _, dout, _, st = run(x, group, False, False, keep)
            assert code == 0 and st[R.STAT_KEPT] == keep == kept.sum()
            assert np.array_equal(dout != 0, np.repeat(kept, group)), (B, group, keep)


def test_non_finite_logits_are_counted_and_a_nan_sample_is_kept():
    x = torch.tensor([0.5, -1.0, 2.0, 3.0, float("nan"), 0.25, float("inf"), 1.0, -0.5, -0.25])       # B = 5 samples of 2
    ref = R.adv_ref(x.double().numpy(), 2, False, False, 1)
    assert ref["kept"].tolist() == [False, False, True, True, False]        # the NaN sample, and the inf one as the best of the rest
    code, loss, dout, _, st = run(x, 2, False, False, 1)
    assert code == 0 and st[R.STAT_NONFINITE] == 2 and st[R.STAT_KEPT] == 2
    assert np.array_equal(dout != 0, np.repeat(ref["kept"], 2))
    assert np.isnan(st[R.STAT_MEAN]) and np.isnan(loss)                     # it reaches the loss, the statistics and so the guard
    code, _, _, _, st = run(x, 2, True, True, 0)
    assert code == 0 and st[R.STAT_NONFINITE] == 2 and st[R.STAT_KEPT] == 5


def test_refusals_return_codes_and_launch_nothing():
    from dvd_gan_amd import lib as L
    x = torch.zeros(24)
    loss0 = 0.5
    for kw, want in ((dict(group=5), -1), (dict(group=8, keep=4), -1), (dict(group=8, keep=-1), -1), (dict(group=8, lecam=0.1), -1)):
        code, loss, dout, _, st = run(x, kw.get("group"), True, True, kw.get("keep", 0), kw.get("lecam", 0.0), loss0=loss0)
        assert code == want and loss == loss0 and np.all(dout == 7.0) and np.all(st == -9.0), kw
    big = torch.zeros((L.ADV_MAX_SAMPLES + 1) * 2)
    code, loss, dout, _, st = run(big, 2, True, True, 1, loss0=loss0)
    assert code == -2 and loss == loss0 and np.all(dout == 7.0) and np.all(st == -9.0)
    code, _, _, _, st = run(big, 2, True, True, 0)                           # without selection any n is served
    assert code == 0 and st[R.STAT_KEPT] == L.ADV_MAX_SAMPLES + 1

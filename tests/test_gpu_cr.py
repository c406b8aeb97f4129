"""dvdx_cr_pair on the device against the float64 restatement (tests/cr_ref.py) within its counted bounds, its bit-level
properties, its refusals, and functional.CRLoss on top of it.  A few thousand floats at the most."""
import pytest
import torch

import cr_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [1, 3, 64, 255, 256, 257, 1000, 4097]            # below a wave, a wave, around the workgroup's stride, several strides
WEIGHTS = [0.0, 0.5, 10.0]
SENTINEL = 12345.5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _launch(aug, clean, weight, want_stats=True):
    """-> (code, loss, d_aug, d_clean, stats) with every output pre-filled with SENTINEL."""
    from dvd_gan_amd import lib as L
    a, c = aug.to(DEV), clean.to(DEV)
    n = a.numel()
    loss = torch.full((1,), SENTINEL, device=DEV)
    da, dc = torch.full((n,), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)
    stats = torch.full((L.CR_NSTAT,), SENTINEL, device=DEV)
    code = L.cr_lib().dvdx_cr_pair(L.ptr(a), L.ptr(c), n, weight, L.ptr(loss), L.ptr(da), L.ptr(dc),
                                   L.ptr(stats) if want_stats else None, L.stream())
    torch.cuda.synchronize()
    return code, loss.cpu(), da.cpu(), dc.cpu(), stats.cpu()


@pytest.mark.parametrize("n", SIZES)
def test_kernel_parity_and_bits(n):
    from dvd_gan_amd import lib as L
    aug, clean = R.make_logits(n)
    same = aug == clean
    for weight in WEIGHTS:
        ref = R.pair64(aug, clean, weight)
        code, loss, da, dc, stats = _launch(aug, clean, weight)
        assert code == 0
        worst = {"loss": R.ratio(loss, *ref["loss"]), "d_aug": R.ratio(da, *ref["d_aug"]), "d_clean": R.ratio(dc, *ref["d_clean"]),
                 "msq": R.ratio(stats[L.CR_STAT_MSQ], *ref["msq"]), "maxabs": R.ratio(stats[L.CR_STAT_MAXABS], *ref["maxabs"])}
        print(f"[cr] n={n} weight={weight}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, worst
        # the statistics row: the penalty is the loss to the bit, the counts are exact
        assert torch.equal(_bits(stats[L.CR_STAT_PENALTY:L.CR_STAT_PENALTY + 1]), _bits(loss))
        assert float(stats[L.CR_STAT_NONZERO]) == ref["nonzero"] == int((~same).sum()) and float(stats[L.CR_STAT_N]) == n
        # d_clean is d_aug with the sign bit flipped; an identical pair gives zeros
        assert torch.equal(_bits(dc), _bits(da) ^ torch.tensor(-2 ** 31, dtype=torch.int32))
        assert bool((da[same] == 0).all()) and bool((dc[same] == 0).all())
        if weight == 0.0:
            assert float(loss) == 0.0 and bool((da == 0).all())
        elif n > 2:
            assert bool((da[~same] != 0).all())           # the pair one bit apart has a gradient
        # a second launch: the same bits, with and without the statistics row
        again = _launch(aug, clean, weight, want_stats=False)
        assert again[0] == 0 and float(again[4][0]) == SENTINEL
        for x, y in zip((loss, da, dc), again[1:4]):
            assert torch.equal(_bits(x), _bits(y))


def test_all_pairs_identical():
    aug, _ = R.make_logits(1000)
    code, loss, da, dc, stats = _launch(aug, aug.clone(), 10.0)
    assert code == 0 and float(loss) == 0.0 and bool((da == 0).all()) and bool((dc == 0).all())
    assert stats.tolist() == [0.0, 0.0, 0.0, 0.0, 1000.0]


def test_nonfinite_logits_reach_the_loss_and_their_own_pair_only():
    aug, clean = R.make_logits(257)
    aug[5], clean[200] = float("inf"), float("nan")
    code, loss, da, dc, _ = _launch(aug, clean, 10.0)
    assert code == 0 and not bool(torch.isfinite(loss).any())
    bad = torch.zeros(257, dtype=torch.bool)
    bad[5] = bad[200] = True
    assert not bool(torch.isfinite(da[bad]).any()) and bool(torch.isfinite(da[~bad]).all()) and bool(torch.isfinite(dc[~bad]).all())


def test_refusals_write_nothing():
    from dvd_gan_amd import lib as L
    so = L.cr_lib()
    n = 64
    aug, clean = (t.to(DEV) for t in R.make_logits(n))
    outs = [torch.full((m,), SENTINEL, device=DEV) for m in (1, n, n, L.CR_NSTAT)]
    ok = dict(aug=L.ptr(aug), clean=L.ptr(clean), n=n, weight=10.0, loss=L.ptr(outs[0]), d_aug=L.ptr(outs[1]), d_clean=L.ptr(outs[2]),
              stats=L.ptr(outs[3]), stream=L.stream())
    call = lambda **kw: so.dvdx_cr_pair(*{**ok, **kw}.values())
    for name in ("aug", "clean", "loss", "d_aug", "d_clean"):
        assert call(**{name: None}) == -1, name
    assert call(n=0) == -1 and call(n=-4) == -1 and call(n=(1 << 20) + 1) == -2
    for w in (-1.0, float("inf"), float("nan")):
        assert call(weight=w) == -1, w
    with pytest.raises(RuntimeError, match=r"libdvdx_cr: .*weight.*\(code -1\)"):
        L.cr_check(call(weight=-2.0))
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all())
    assert call() == 0                                     # ... and the same arguments unchanged are served
    torch.cuda.synchronize()
    assert not bool((outs[1] == SENTINEL).any()) and float(outs[3][L.CR_STAT_N]) == n


def test_crloss_function_scales_the_saved_gradients():
    from dvd_gan_amd import functional as Fn
    from dvd_gan_amd import lib as L
    n = 257
    aug, clean = R.make_logits(n)
    ref = R.pair64(aug, clean, 0.5)
    logits = torch.cat([aug, clean]).to(DEV).requires_grad_(True)          # one call's logits: [transformed | clean]
    stats = torch.zeros(L.CR_NSTAT, device=DEV)
    loss = Fn.CRLoss.apply(logits[:n], logits[n:], 0.5, stats)
    assert loss.dim() == 0 and R.ratio(loss, *ref["loss"]) <= 1.0
    (loss * 4.0).backward()                                               # a power of two: the scaling is exact
    g = logits.grad.cpu()
    assert R.ratio(g[:n] / 4.0, *ref["d_aug"]) <= 1.0 and R.ratio(g[n:] / 4.0, *ref["d_clean"]) <= 1.0
    assert torch.equal(g[n:], -g[:n])           # (autograd adds the halves into zeros: a -0 of the launch arrives as +0)
    assert float(stats[L.CR_STAT_N]) == n
    with pytest.raises(ValueError, match="CRLoss"):
        Fn.CRLoss.apply(logits[:n], logits[n:n + 3], 0.5, None)

"""dvdx_zcr_dist / dvdx_zcr_dist_grad on the device against the numpy restatement of the header (tests/zcr_ref.py), their bit-level
properties, their refusals, and functional.PairDistance on top of them.  16 MB at the most."""
import numpy as np
import pytest
import torch

import zcr_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = 12345.5
GUARD = 64                     # sentinel floats on either side of every output
# [pairs, n, layout]: "views" = the halves are rows [:pairs] and [pairs:] of ONE tensor, as the Trainer passes them (so the second
# half is 16-byte aligned only when pairs * n is a multiple of 4); "separate" = two allocations, both aligned
SHAPES = [
    (1, 1, "views"), (2, 1, "views"), (3, 1, "separate"),          # n = 1
    (3, 37, "views"),                                              # below a wave; pairs * n odd: the 4-byte path throughout
    (3, 4099, "views"),                                            # two chunks a row, pairs * n odd: the 4-byte path, its 4-way loop
    (1, 4099, "separate"),                                         # aligned rows, n no multiple of 4: a last group of 3 elements
    (2, 4098, "views"),                                            # pairs * n = 0 mod 4, n = 2 mod 4: row 0 by vectors, row 1 not
    (2, 13524, "views"),                                           # n = 0 mod 4: four chunks a row (3384, 3384, 3384, 3372)
    (3, 13523, "separate"),                                        # ... and rows of every alignment with a ragged last chunk
    (2050, 8, "views"),                                            # more work units than workgroups: the loop over units
    (2, 1048584, "views"),                                         # more vectors than grid * threads: the gradient's grid stride
]
IDS = [f"{p}x{n}-{lay}" for p, n, lay in SHAPES]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _halves(pairs, n, layout, seed=0):
    both = R.make_halves(pairs, n, seed)
    if layout == "views":
        dev = torch.from_numpy(both).to(DEV)
        return both[:pairs], both[pairs:], dev[:pairs], dev[pairs:]
    return both[:pairs], both[pairs:], torch.from_numpy(both[:pairs].copy()).to(DEV), torch.from_numpy(both[pairs:].copy()).to(DEV)


def _guarded(numel):
    """A sentinel-filled buffer with GUARD more floats on either side -> (whole, the middle view)."""
    whole = torch.full((numel + 2 * GUARD,), SENTINEL, device=DEV)
    return whole, whole[GUARD:GUARD + numel]


def _dist(a, b, weight, want_stats=True):
    from dvd_gan_amd import lib as L
    pairs, n = a.shape
    need = L.zcr_lib().dvdx_zcr_ws_doubles(pairs, n)
    ws = torch.zeros(need, dtype=torch.float64, device=DEV)
    term, stats = torch.full((1,), SENTINEL, device=DEV), torch.full((L.ZCR_NSTAT,), SENTINEL, device=DEV)
    code = L.zcr_lib().dvdx_zcr_dist(L.ptr(a), L.ptr(b), pairs, n, weight, L.ptr(ws), need, L.ptr(term),
                                     L.ptr(stats) if want_stats else None, L.stream())
    torch.cuda.synchronize()
    return code, term.cpu(), stats.cpu()


def _grad(a, b, weight, upstream, layout):
    """-> (code, da, db) on the host; the outputs lie like the inputs (halves of one buffer, or two) between sentinels."""
    from dvd_gan_amd import lib as L
    pairs, n = a.shape
    up = torch.tensor([upstream], dtype=torch.float32, device=DEV)
    if layout == "views":
        whole, mid = _guarded(2 * pairs * n)
        da, db = mid[:pairs * n], mid[pairs * n:]
        wholes = [whole]
    else:
        (wa, da), (wb, db) = _guarded(pairs * n), _guarded(pairs * n)
        wholes = [wa, wb]
    code = L.zcr_lib().dvdx_zcr_dist_grad(L.ptr(a), L.ptr(b), pairs, n, weight, L.ptr(up), L.ptr(da), L.ptr(db), L.stream())
    torch.cuda.synchronize()
    for w in wholes:
        assert bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all()), "a write outside the gradient"
    return code, da.cpu().numpy().reshape(pairs, n), db.cpu().numpy().reshape(pairs, n)


@pytest.mark.parametrize("pairs,n,layout", SHAPES, ids=IDS)
def test_forward_against_the_restatement(pairs, n, layout):
    """Term, mean_sq_dist, min_pair, max_pair: within 2 fp32 ulps (the fp64 sums differ from the restatement's only in their
    order, far below one fp32 rounding at these sizes: the slack is the final rounding falling on either side).  max_abs_diff and
    pairs: exact.  Two launches: the same bits."""
    from dvd_gan_amd import lib as L
    a, b, da, db = _halves(pairs, n, layout)
    assert (db.data_ptr() % 16 == 0) == (layout == "separate" or (pairs * n) % 4 == 0)
    for weight in (0.5, 8.0, 0.0):
        ref = R.dist(a, b, weight)
        code, term, stats = _dist(da, db, weight)
        assert code == 0
        got = {"term": stats[L.ZCR_STAT_TERM], "mean_sq_dist": stats[L.ZCR_STAT_MSQ], "min_pair": stats[L.ZCR_STAT_MIN_PAIR],
               "max_pair": stats[L.ZCR_STAT_MAX_PAIR]}
        off = {k: R.ulps(np.float32(v), ref[k]) for k, v in got.items()}
        print(f"[zcr] {pairs} x {n} {layout} weight={weight}: ulps " + ", ".join(f"{k} {v:.0f}" for k, v in off.items())
              + f"; term {float(term):.6e}, min / mean / max pair {float(got['min_pair']):.4e} / {float(got['mean_sq_dist']):.4e} / "
              f"{float(got['max_pair']):.4e}")
        assert max(off.values()) <= 2, off
        assert torch.equal(_bits(stats[L.ZCR_STAT_TERM:L.ZCR_STAT_TERM + 1]), _bits(term))
        assert float(stats[L.ZCR_STAT_MAXABS]) == float(ref["max_abs_diff"]) and float(stats[L.ZCR_STAT_PAIRS]) == pairs
        if weight == 0.0:
            assert float(term) == 0.0
        else:
            assert float(term) < 0.0
        again = _dist(da, db, weight, want_stats=False)
        assert again[0] == 0 and torch.equal(_bits(again[1]), _bits(term)) and bool((again[2] == SENTINEL).all())


@pytest.mark.parametrize("pairs,n,layout", SHAPES, ids=IDS)
def test_gradient_is_the_restatement_to_the_bit(pairs, n, layout):
    """db = fl32(fl32(upstream * scale) * fl32(a - b)) with scale rounded once on the host: three roundings in a stated order and
    no sum, so the restatement promises the bits.  da is db with the sign bit flipped.  upstream is read on the device: 0.5
    halves every element exactly, 0 leaves signed zeros."""
    a, b, dev_a, dev_b = _halves(pairs, n, layout, seed=1)
    for weight, upstream in ((0.5, 1.0), (8.0, 0.5), (0.3125, 0.75), (8.0, 0.0), (0.0, 1.0)):
        want_da, want_db = R.grad(a, b, weight, upstream)
        code, got_da, got_db = _grad(dev_a, dev_b, weight, upstream, layout)
        assert code == 0
        assert np.array_equal(got_db.view(np.uint32), want_db.view(np.uint32)), (weight, upstream)
        assert np.array_equal(got_da.view(np.uint32), got_db.view(np.uint32) ^ np.uint32(0x80000000))
        assert np.array_equal(got_da.view(np.uint32), want_da.view(np.uint32))
        if weight == 0.0 or upstream == 0.0:
            assert not got_db.any() and not got_da.any()
        else:
            assert np.array_equal(got_db != 0, a != b)
    code, again_da, again_db = _grad(dev_a, dev_b, 0.3125, 0.75, layout)
    want_da, want_db = R.grad(a, b, 0.3125, 0.75)
    assert code == 0 and np.array_equal(again_db.view(np.uint32), want_db.view(np.uint32))


def test_identical_halves():
    pairs, n = 3, 5000
    _, _, a, _ = _halves(pairs, n, "separate")
    b = a.clone()
    code, term, stats = _dist(a, b, 8.0)
    assert code == 0 and float(term) == 0.0                    # (as -0: the sign does not matter)
    assert stats.tolist() == [float(term), 0.0, 0.0, 0.0, 0.0, float(pairs)]
    code, da, db = _grad(a, b, 8.0, 1.0, "separate")
    assert code == 0 and not da.any() and not db.any()


def test_refusals_write_nothing():
    from dvd_gan_amd import lib as L
    so = L.zcr_lib()
    pairs, n = 2, 600
    _, _, a, b = _halves(pairs, n, "views")
    need = so.dvdx_zcr_ws_doubles(pairs, n)
    outs = [torch.full((m,), SENTINEL, device=DEV) for m in (1, L.ZCR_NSTAT, pairs * n, pairs * n)]
    ws = torch.full((need,), SENTINEL, dtype=torch.float64, device=DEV)
    up = torch.ones(1, device=DEV)
    ok = dict(a=L.ptr(a), b=L.ptr(b), pairs=pairs, n=n, weight=0.5, ws=L.ptr(ws), ws_doubles=need, term=L.ptr(outs[0]),
              stats=L.ptr(outs[1]), stream=L.stream())
    okg = dict(a=L.ptr(a), b=L.ptr(b), pairs=pairs, n=n, weight=0.5, upstream=L.ptr(up), da=L.ptr(outs[2]), db=L.ptr(outs[3]),
               stream=L.stream())
    call = lambda **kw: so.dvdx_zcr_dist(*{**ok, **kw}.values())
    callg = lambda **kw: so.dvdx_zcr_dist_grad(*{**okg, **kw}.values())
    for name in ("a", "b", "ws", "term"):
        assert call(**{name: None}) == -1, name
    for name in ("a", "b", "upstream", "da", "db"):
        assert callg(**{name: None}) == -1, name
    for fn in (call, callg):
        assert fn(pairs=0) == -1 and fn(n=0) == -1 and fn(n=-4) == -1 and fn(pairs=(1 << 16) + 1) in (-1, -2)
        for w in (-1.0, float("inf"), float("nan")):
            assert fn(weight=w) == -1, w
    assert call(ws_doubles=need - 1) == -1 and callg(pairs=(1 << 16) + 1) == -2
    with pytest.raises(RuntimeError, match=r"libdvdx_zcr: .*weight.*\(code -1\)"):
        L.zcr_check(call(weight=-2.0))
    torch.cuda.synchronize()
    for t in outs + [ws]:
        assert bool((t == SENTINEL).all())
    assert call() == 0 and callg() == 0                      # ... and the same arguments unchanged are served
    torch.cuda.synchronize()
    assert not bool((outs[2] == SENTINEL).any()) and float(outs[1][L.ZCR_STAT_PAIRS]) == pairs


def test_pair_distance_function():
    """functional.PairDistance on the generator's [2 * pairs, ...] output: the term, one [2 * pairs, ...] gradient written by the
    backward launch (rows [:pairs] = da, rows [pairs:] = db), the upstream scalar taken from autograd on the device."""
    from dvd_gan_amd import functional as Fn
    from dvd_gan_amd import lib as L
    pairs, shape = 2, (2, 3, 3, 20, 24)                      # [B, T, 3, H, W] clips: n = 8640
    n = int(np.prod(shape[1:]))
    both = R.make_halves(pairs, n)
    ref = R.dist(both[:pairs], both[pairs:], 0.5)
    want_da, want_db = R.grad(both[:pairs], both[pairs:], 0.5, 0.25)
    x = torch.from_numpy(both).to(DEV).view(2 * pairs, *shape[1:]).requires_grad_(True)
    stats = torch.zeros(L.ZCR_NSTAT, device=DEV)
    term = Fn.PairDistance.apply(x, 0.5, stats)
    assert term.dim() == 0 and R.ulps(np.float32(term.item()), ref["term"]) <= 2
    (term * 0.25).backward()
    g = x.grad.cpu().numpy().reshape(2 * pairs, n)
    assert np.array_equal(g[:pairs], want_da) and np.array_equal(g[pairs:], want_db) and np.array_equal(g[:pairs], -g[pairs:])
    assert float(stats[L.ZCR_STAT_PAIRS]) == pairs and R.ulps(np.float32(stats[L.ZCR_STAT_MIN_PAIR].item()), ref["min_pair"]) <= 2
    for bad in (x.detach().double(), x.detach().transpose(1, 2), x.detach()[:3]):
        with pytest.raises(ValueError, match="PairDistance"):
            Fn.PairDistance.apply(bad, 0.5, None)

"""dvdx_cls_update on the device, through classmetrics.LogitStats, against the fp64 numpy restatement (tests/cls_ref.py): every
count and the confusion matrix exactly, every fp64 accumulator within the bound the restatement derives, the finished metrics to
rtol 1e-9; streaming in calls that cut through the splits; bit-equal repeats.  The largest case is 257 x 4096 logits (4 MB).

Measured on an MI355X (profiles/cls_numbers.md): the largest |device - restatement| / bound over all cases is 0.189 for fp32
(2 x 1 logits), 0.049 for bf16 and 0.050 for fp16 logits."""
import numpy as np
import pytest
import torch

import cls_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CLASSES = [1, 2, 63, 64, 65, 101, 600, 4096]          # below, at and above a wave of 64 lanes; UCF-101, Kinetics-600, the limit
ROWS = [1, 2, 63, 65, 257]                            # one row, below and above a workgroup of launch 1, several per split and phase
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
METRICS = ("is_mean", "is_all", "h_marginal", "h_conditional", "top1", "top5", "mean_log_lik")
_worst = {}


def _stored(L, dtype):
    """fp32 numpy logits -> (the device tensor in `dtype`, the stored values widened to fp32 numpy)."""
    t = torch.from_numpy(np.ascontiguousarray(L)).to(DEV).to(dtype)
    return t, t.float().cpu().numpy()


def _run(t, y, splits, *, cuts=None, confusion=True):
    """LogitStats over the device logits t and int labels y (numpy or None), fed whole or cut at `cuts` -> (state, confusion,
    result)."""
    from dvd_gan_amd.classmetrics import LogitStats
    n, C = t.shape
    st = LogitStats(C, n, splits=splits, confusion=confusion, device=DEV)
    edges = [0] + list(cuts or []) + [n]
    for a, b in zip(edges[:-1], edges[1:]):
        st.update(t[a:b], None if y is None else torch.from_numpy(y[a:b]))
    assert st.rows == n
    res = st.result()
    return st._state.cpu().numpy(), None if st._confusion is None else st._confusion.cpu().numpy(), res


def _check(tag, got, stored, y, splits, *, calls=1, confusion=True):
    """Counts and confusion exactly, accumulators within the restatement's bound, metrics to rtol 1e-9."""
    state, conf, res = got
    C = stored.shape[1]
    want, bound, want_conf = R.accumulate(stored, y, splits=splits, confusion=confusion, calls=calls)
    counts = [C + k for k in R.COUNTS]
    assert np.array_equal(state[:, counts], want[:, counts]), (tag, state[:, counts], want[:, counts])
    assert not bound[:, counts].any()
    if confusion:
        assert conf.dtype == np.int64 and np.array_equal(conf, want_conf), tag
    err = np.abs(state - want)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    _worst[tag.split()[0]] = max(_worst.get(tag.split()[0], 0.0), ratio)
    print(f"[cls] {tag}: max |device - reference| / bound = {ratio:.3f}")
    assert (err <= bound).all(), (tag, ratio)
    ref = R.finish(want, want_conf, labelled=y is not None)
    for key in METRICS:
        if key in ref:
            np.testing.assert_allclose(res[key], ref[key], rtol=1e-9, atol=0, err_msg=f"{tag} {key}")
    # the standard deviation moves by no more than a score does (it is 1-Lipschitz in the largest change of a score), and a
    # score is within 1e-11 relative by the accumulators' bounds: where the splits score alike it is a rounding, not a digit
    np.testing.assert_allclose(res["is_std"], ref["is_std"], rtol=1e-9, atol=1e-11 * ref["is_mean"], err_msg=f"{tag} is_std")
    assert (res["n"], res["n_bad"], res["n_bad_label"]) == (ref["n"], ref["n_bad"], ref["n_bad_label"])
    if y is not None and confusion:
        np.testing.assert_array_equal(res["per_class_top1"], ref["per_class_top1"])
    return want, bound


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("C", CLASSES)
def test_every_shape_in_fp32(C, rows):
    L, y = R.make_logits(rows, C)
    t, stored = _stored(L, torch.float32)
    assert np.array_equal(stored, L)
    splits = min(3, rows)
    confusion = C < 4096 or rows == 257                    # the 128 MB matrix of the widest case once
    _check(f"fp32 {rows}x{C}", _run(t, y, splits, confusion=confusion), stored, y, splits, confusion=confusion)


@pytest.mark.parametrize("rows", [1, 65, 257])
@pytest.mark.parametrize("C", [1, 65, 101, 4096])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_half_precision_logits(dtype, C, rows):
    """The stored half values are the inputs: rounding the logits makes exact ties, which the rank and the argmax must break alike."""
    L, y = R.make_logits(rows, C)
    t, stored = _stored(L, DTYPES[dtype])
    splits = min(3, rows)
    _check(f"{dtype} {rows}x{C}", _run(t, y, splits, confusion=C < 4096), stored, y, splits, confusion=C < 4096)


@pytest.mark.parametrize("splits", [1, 3, 10])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_splits_streaming_and_determinism(dtype, splits):
    """257 rows in 1, 3 or 10 splits (none divides 257), in one call and in calls of 100 + 100 + 57 rows that cut through the
    splits' boundaries: both within the bound, the counts and the confusion matrix equal, and a repeat of either bit-equal."""
    L, y = R.make_logits(257, 101, seed=splits)
    t, stored = _stored(L, DTYPES[dtype])
    one = _run(t, y, splits)
    three = _run(t, y, splits, cuts=[100, 200])
    _check(f"{dtype} 257x101 S={splits} one call", one, stored, y, splits)
    want, bound = _check(f"{dtype} 257x101 S={splits} three calls", three, stored, y, splits, calls=3)
    assert (np.abs(three[0] - one[0]) <= bound).all() and np.array_equal(three[1], one[1])
    counts = [101 + k for k in R.COUNTS]
    assert np.array_equal(three[0][:, counts], one[0][:, counts])
    assert np.bincount(R.split_of(np.arange(257), 257, splits)).tolist() == want[:, 101 + R.N].tolist()
    for again, first in ((_run(t, y, splits), one), (_run(t, y, splits, cuts=[100, 200]), three)):
        assert np.array_equal(again[0].view(np.int64), first[0].view(np.int64)) and np.array_equal(again[1], first[1])
        assert {k: v for k, v in again[2].items() if k not in ("confusion", "per_class_top1")} == \
            {k: v for k, v in first[2].items() if k not in ("confusion", "per_class_top1")}
    # without labels: the same sums bit for bit, the five label columns untouched
    bare = _run(t, None, splits, confusion=False)
    assert np.array_equal(bare[0][:, :101 + R.LABELLED].view(np.int64), one[0][:, :101 + R.LABELLED].view(np.int64))
    assert not bare[0][:, 101 + R.LABELLED:].any() and bare[1] is None and "top1" not in bare[2]
    _check(f"{dtype} 257x101 S={splits} no labels", bare, stored, None, splits, confusion=False)


def _value_cases(C, big):
    """fp32 [16, C] logits and labels with one row per special case (C >= 7)."""
    rng = np.random.default_rng(77 + C)
    L = rng.standard_normal((16, C)).astype(np.float32)
    y = (np.arange(16) * 3 % C).astype(np.int32)
    L[0] = big * np.sign(L[0])                             # +-big: the stable softmax
    L[1, :] = -big
    L[1, C - 1] = big
    y[1] = C - 1
    L[2] = 0.25                                            # all equal: rank = label
    y[2] = 3
    L[3] = -big                                            # all equal and large
    y[3] = 0
    L[4, [1, 3, 5]] = 4.0                                  # an exact tie for the maximum that includes the label, on either side of it
    y[4] = 3
    L[5, [1, 3, 5]] = 4.0
    y[5] = 1
    L[6, [1, 3, 5]] = 4.0
    y[6] = 5
    L[7, [0, C - 1]] = L[7].max() + 1.0                    # a tie across the row's ends (different lanes above 64 classes)
    y[7] = C - 1
    L[8, [0, 1, 2, 3, 4, 6]] = 9.0                         # the label ties with five classes below it and one above: rank 5
    y[8] = 6
    L[9, 2] = np.nan
    L[10, C - 1] = np.inf
    L[11, 0] = -np.inf
    y[10] = C - 1
    y[12], y[13] = -1, C                                   # labels out of range on either side
    L[14, 4] = np.nan                                      # a bad row whose label is out of range too: counted as bad only
    y[14] = C + 5
    return L, y


@pytest.mark.parametrize("C", [7, 130])
@pytest.mark.parametrize("dtype,big", [("fp32", 80.0), ("bf16", 80.0), ("fp16", 3.0e4)])
def test_value_cases(dtype, big, C):
    L, y = _value_cases(C, big)
    t, stored = _stored(L, DTYPES[dtype])
    assert np.abs(stored[0]).max() == big and np.isnan(stored[9, 2]) and np.isposinf(stored[10, C - 1]) and np.isneginf(stored[11, 0])
    for splits, cuts in ((1, None), (4, None), (4, [5, 11])):
        got = _run(t, y, splits, cuts=cuts)
        _check(f"{dtype} values C={C} S={splits} cuts={cuts}", got, stored, y, splits, calls=3 if cuts else 1)
        state, conf, res = got
        assert (res["n"], res["n_bad"], res["n_bad_label"]) == (12, 4, 2)
        assert all(np.isfinite(res[k]) for k in METRICS + ("is_std",)), res
        tot = state[:, C:].sum(axis=0)
        assert tot[R.LABELLED] == 10 and conf.sum() == 10
        # the ties: rows 4, 5, 6 share the argmax 1; only the label 1 is a top-1 hit; row 8 has rank 5 and misses top-5
        assert conf[3, 1] >= 1 and conf[1, 1] >= 1 and conf[5, 1] >= 1 and conf[C - 1, 0] >= 1 and conf[6, 0] >= 1
    no_top5 = R.accumulate(stored[8:9], y[8:9], splits=1)[0][0, C:]
    assert no_top5[R.TOP1] == 0 and no_top5[R.TOP5] == 0 and no_top5[R.LABELLED] == 1


def test_the_convenience_functions_and_refusals():
    from dvd_gan_amd.classmetrics import LogitStats, class_fidelity, inception_score
    L, y = R.make_logits(120, 11)
    t = torch.from_numpy(L).to(DEV)
    ref = R.metrics(L, y, splits=10)
    mean, std = inception_score(t)
    np.testing.assert_allclose([mean, std], [ref["is_mean"], ref["is_std"]], rtol=1e-9)
    one = R.metrics(L, y, splits=1, confusion=True)
    fid = class_fidelity(t, torch.from_numpy(y).to(DEV))
    assert np.array_equal(fid["confusion"], one["confusion"]) and fid["top1"] == one["top1"] and fid["top5"] == one["top5"]
    np.testing.assert_array_equal(fid["per_class_top1"], one["per_class_top1"])
    np.testing.assert_allclose(fid["mean_log_lik"], one["mean_log_lik"], rtol=1e-9)
    assert 0.0 < fid["top1"] < 1.0
    for kw in (dict(n_classes=0, n_total=5), dict(n_classes=4097, n_total=5), dict(n_classes=3, n_total=0),
               dict(n_classes=3, n_total=5, splits=6), dict(n_classes=3, n_total=5000, splits=1025), dict(n_classes=3, n_total=5, splits=0)):
        with pytest.raises(ValueError):
            LogitStats(device=DEV, **kw)
    st = LogitStats(11, 100, splits=2, device=DEV)
    with pytest.raises(ValueError, match="logits must be"):
        st.update(t[:, :10])
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        st.update(t[:10].double())
    with pytest.raises(ValueError, match="n_total=100"):
        st.update(t)
    st.update(t[:50], torch.from_numpy(y[:50]))
    with pytest.raises(ValueError, match="every update"):
        st.update(t[50:100])
    with pytest.raises(ValueError, match="confusion matrix needs labels"):
        LogitStats(11, 100, confusion=True, device=DEV).update(t[:50])
    assert st.rows == 50 and st.result()["n"] == 50


def test_report_the_largest_ratios():
    """Not a check of its own: prints what the cases above measured, for profiles/cls_numbers.md."""
    print("[cls] largest |device - reference| / bound per dtype:", {k: round(v, 3) for k, v in sorted(_worst.items())})

"""The Inception Score / class-fidelity sums without a GPU: self-tests of the numpy restatement (tests/cls_ref.py), the handshake, the
sizing query, the argument checks and the resource report of libdvdx_cls.so."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cls_ref as R  # noqa: E402


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_uniform_logits_score_one(dtype):
    for value in (0.0, -7.5, 300.0):
        res = R.metrics(np.full((40, 7), value, dtype), np.arange(40) % 7, splits=4, confusion=True)
        assert abs(res["is_mean"] - 1.0) <= 1e-14 and res["is_std"] <= 1e-14 and abs(res["is_all"] - 1.0) <= 1e-14
        assert abs(res["h_marginal"] - math.log(7)) <= 1e-14 and abs(res["h_conditional"] - math.log(7)) <= 1e-14
        # every class ties: the rank of label y is y, the argmax is class 0
        assert res["top1"] == np.count_nonzero(np.arange(40) % 7 == 0) / 40 and res["top5"] == np.count_nonzero(np.arange(40) % 7 < 5) / 40
        assert res["confusion"][:, 0].sum() == 40 and res["confusion"][:, 1:].sum() == 0
        assert abs(res["mean_log_lik"] + math.log(7)) <= 1e-14


def test_confident_balanced_logits_score_the_class_count():
    C, k = 11, 6
    y = np.arange(k * C) % C
    L = np.zeros((k * C, C), np.float32)
    L[np.arange(k * C), y] = 60.0
    res = R.metrics(L, y, splits=k, confusion=True)             # every split holds each class once
    assert abs(res["is_mean"] - C) <= 1e-9 * C and res["is_std"] <= 1e-9 and abs(res["is_all"] - C) <= 1e-9 * C
    assert res["top1"] == 1.0 and res["top5"] == 1.0 and abs(res["mean_log_lik"]) <= 1e-20
    assert np.array_equal(res["confusion"], k * np.eye(C, dtype=np.int64)) and np.array_equal(res["per_class_top1"], np.ones(C))
    assert (res["n"], res["n_bad"], res["n_bad_label"]) == (k * C, 0, 0)
    # the same clips all conditioned on one class: diverse to the score, wrong to the fidelity
    wrong = R.metrics(L, np.zeros(k * C, np.int64), splits=k, confusion=True)
    assert wrong["is_mean"] == res["is_mean"] and wrong["top1"] == 1.0 / C and np.array_equal(wrong["confusion"][0], np.full(C, k))


def test_a_case_by_hand():
    ln = math.log
    L = np.array([[0.0, ln(3.0)], [ln(3.0), 0.0], [0.0, 0.0]], np.float64)      # p = (1/4, 3/4), (3/4, 1/4), (1/2, 1/2)
    y = np.array([1, 0, 1])
    state, bound, conf = R.accumulate(L, y, splits=1, confusion=True)
    a = 2 * (0.25 * ln(0.25) + 0.75 * ln(0.75)) + ln(0.5)
    want = [1.5, 1.5, 3, a, 0, 3, 2 * ln(0.75) + ln(0.5), 2, 3, 0]                # row 2 ties: label 1 has rank 1, argmax 0
    assert state.shape == (1, 2 + R.NSTAT) and np.allclose(state[0], want, rtol=1e-15, atol=1e-15)
    assert np.array_equal(conf, [[1, 0], [1, 1]])
    assert not bound[0, [2 + k for k in R.COUNTS]].any() and (bound[0, [0, 1, 2 + R.A, 2 + R.LOGLIK]] > 0).all()
    assert (bound[0] <= 64 * R.U * np.abs(state[0]).clip(1.0)).all()
    res = R.finish(state, conf)
    assert abs(res["is_all"] - math.exp(a / 3 + ln(2))) <= 1e-15 and res["is_mean"] == res["is_all"] and res["is_std"] == 0.0
    assert res["top1"] == 2 / 3 and res["top5"] == 1.0 and abs(res["mean_log_lik"] - (2 * ln(0.75) + ln(0.5)) / 3) <= 1e-15
    assert np.array_equal(res["per_class_top1"], [1.0, 0.5])


def test_splits_bad_rows_and_labels_out_of_range():
    assert R.split_of(np.arange(7), 7, 3).tolist() == [0, 0, 0, 1, 1, 2, 2]      # ceil(7s / 3) = 0, 3, 5
    assert np.bincount(R.split_of(np.arange(257), 257, 10)).tolist() == [26, 26, 26, 25, 26, 26, 25, 26, 26, 25]
    L, y = R.make_logits(30, 5)
    L[3, 2], L[4, 0], L[11, 4] = np.nan, np.inf, -np.inf
    y[7], y[8], y[3] = -1, 5, 9                                                  # row 3 is bad: its label is not looked at
    state, _, conf = R.accumulate(L, y, splits=3, confusion=True)
    st = state[:, 5:]
    assert st[:, R.BAD].tolist() == [2, 1, 0] and st[:, R.N].tolist() == [8, 9, 10] and st[:, R.BAD_LABEL].tolist() == [2, 0, 0]
    assert st[:, R.LABELLED].tolist() == [6, 9, 10] and conf.sum() == 25
    assert np.allclose(state[:, :5].sum(axis=1), st[:, R.N], rtol=1e-14)         # every good row's p sums to one
    # streamed in calls that cut through the splits: the same counts, the same sums to a rounding
    parts = [R.accumulate(L[a:b], y[a:b], splits=3, n_total=30, row0=a, confusion=True) for a, b in ((0, 9), (9, 10), (10, 30))]
    total = sum(p[0] for p in parts)
    assert np.array_equal(total[:, [5 + k for k in R.COUNTS]], state[:, [5 + k for k in R.COUNTS]])
    assert np.allclose(total, state, rtol=1e-14, atol=1e-300) and np.array_equal(sum(p[2] for p in parts), conf)
    # without labels the five label columns stay zero
    bare = R.accumulate(L, splits=3)[0]
    assert not bare[:, 5 + R.LABELLED:].any() and np.array_equal(bare[:, :5 + R.LABELLED], state[:, :5 + R.LABELLED])


def test_large_logits_do_not_overflow():
    for dtype, big in ((np.float32, 80.0), (np.float16, 3.0e4)):
        L = np.array([[big, -big, 0.0], [-big, -big, -big], [big, big, -big]], dtype)
        res = R.metrics(L, np.array([0, 1, 1]), splits=1)
        assert all(math.isfinite(res[k]) for k in ("is_mean", "is_all", "h_marginal", "h_conditional", "mean_log_lik")), res
        assert res["n"] == 3 and res["top1"] == 1 / 3 and abs(res["h_conditional"] - (math.log(3) + math.log(2)) / 3) <= 1e-14


# ------------------------------------------------------------------ the library
NAMES = ["dvdx_cls_abi_version", "dvdx_cls_strerror", "dvdx_cls_ws_bytes", "dvdx_cls_update"]
_PARAM_CODES = {"long long": "l", "int": "i", "float": "f", "double": "d"}


def _declared(header):
    """name -> codes of every prototype, by the rule of tests/test_abi_cpu.py: any `*` -> p, the four scalar types, void -> none."""
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(const\s+char\s*\*|void|int|long\s+long)\s*(dvdx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        ret = "s" if "*" in ret else "v" if ret == "void" else _PARAM_CODES[" ".join(ret.split())]
        codes = ""
        for p in ([] if params.strip() == "void" else params.split(",")):
            if "*" in p:
                codes += "p"
                continue
            kind = " ".join([w for w in p.split() if w != "const"][:-1])
            assert kind in _PARAM_CODES, (name, p)
            codes += _PARAM_CODES[kind]
        assert name not in out
        out[name] = ret + codes
    return out, sorted(set(re.findall(r"\b(dvdx_[a-z0-9_]+)\s*\(", src)))


def test_cls_handshake():
    import shutil
    import subprocess
    from dvd_gan_amd import lib as L
    assert list(L.CLS_EXTENSIONS) == ["cls"]
    rec = L.CLS_EXTENSIONS["cls"]
    assert L._record("cls") is rec
    assert (rec.so, rec.header, rec.env) == ("libdvdx_cls.so", "dvdx_cls.h", "DVDX_CLS_LIB_PATH")
    assert L.library_path("cls") == os.path.join(ROOT, "dvd_gan_amd", "xsrc", "libdvdx_cls.so")
    header = os.path.join(ROOT, "include", rec.header)
    want, called = _declared(header)
    assert sorted(want) == called == sorted(NAMES)
    assert {n: s.replace(" ", "") for n, s in rec.signatures.items()} == want
    loaded = L._load("cls")
    assert L.load_cls_extensions() == [loaded] and L.cls_lib() is loaded
    for name, sig in rec.signatures.items():
        fn, sig = getattr(loaded, name), sig.replace(" ", "")
        assert fn.restype is L._CTYPES[sig[0]] and list(fn.argtypes) == [L._CTYPES[c] for c in sig[1:]], name
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", L.library_path("cls")]).decode()
        exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1] not in ("_init", "_fini"))
        assert exported == sorted(want), exported
    text = open(header).read()
    defines = {n: int(v) for n, v in re.findall(r"^#define (DVDX_[A-Z0-9_]+)\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", text, flags=re.M)}
    assert defines == rec.constants and len(defines) == 18
    assert defines["DVDX_CLS_MAX_CLASSES"] == 4096 and defines["DVDX_CLS_MAX_ROWS"] == 1 << 20 and defines["DVDX_CLS_MAX_SPLITS"] == 1024
    assert (defines["DVDX_CLS_F32"], defines["DVDX_CLS_BF16"], defines["DVDX_CLS_F16"]) == (0, 1, 2)
    assert defines["DVDX_CLS_NSTAT"] == R.NSTAT == 8 and sorted(v for k, v in defines.items() if "_STAT_" in k) == list(range(8))
    assert [defines["DVDX_CLS_STAT_" + k] for k in ("N", "A", "BAD", "LABELLED", "LOGLIK", "TOP1", "TOP5", "BAD_LABEL")] == \
        [R.N, R.A, R.BAD, R.LABELLED, R.LOGLIK, R.TOP1, R.TOP5, R.BAD_LABEL]
    assert rec.abi == ("dvdx_cls_abi_version", L.CLS_ABI_VERSION) and loaded.dvdx_cls_abi_version() == defines["DVDX_CLS_ABI_VERSION"]
    with pytest.raises(RuntimeError, match=r"^libdvdx_cls: .*more splits than rows.* \(code -1\)$"):
        L.cls_check(-1)
    with pytest.raises(RuntimeError, match=r"^libdvdx_cls: .*4096 classes.* \(code -2\)$"):
        L.cls_check(-2)
    assert loaded.dvdx_cls_strerror(0) == b"ok" and loaded.dvdx_cls_strerror(-3) == b"kernel launch failed"
    assert loaded.dvdx_cls_strerror(-77) == b"unknown error"
    try:
        rec.signatures["dvdx_no_such_entry"] = "i p"
        L._handles.pop("cls", None)
        with pytest.raises(RuntimeError, match="libdvdx_cls.so exports no dvdx_no_such_entry -- lib.py and include/dvdx_cls.h disagree"):
            L._load("cls")
        assert "cls" not in L._handles
    finally:
        del rec.signatures["dvdx_no_such_entry"]
        L._handles.pop("cls", None)
        assert L._load("cls") is L._handles["cls"]


def test_the_other_tables_are_what_they_were():
    from dvd_gan_amd import lib as L
    assert list(L.LIBRARIES) == ["core", "adv", "eval", "prdc", "aug", "geom", "sv"] and list(L.EXTENSIONS) == ["tsru"]
    assert list(L.MORE_EXTENSIONS) == ["cr"] and list(L.ZCR_EXTENSIONS) == ["zcr"]
    assert L.load_extensions() == [L._load("tsru")] and L.load_more_extensions() == [L._load("cr")]
    assert L.load_zcr_extensions() == [L._load("zcr")]
    assert L._load("cls") not in L.load_all() + L.load_extensions() + L.load_more_extensions() + L.load_zcr_extensions()
    for table in (L.LIBRARIES, L.EXTENSIONS, L.MORE_EXTENSIONS, L.ZCR_EXTENSIONS):
        for key, rec in table.items():
            assert L._record(key) is rec
            assert not [n for n in rec.signatures if n.startswith("dvdx_cls")] and not [n for n in rec.constants if "_CLS_" in n]
    assert L.library_path("zcr") == os.path.join(ROOT, "dvd_gan_amd", "xsrc", "libdvdx_zcr.so")


def test_build_loads_the_new_library():
    import inspect
    import __graft_entry__ as G
    assert "lib.load_cls_extensions()" in inspect.getsource(G.build)


def test_the_sizing_query():
    from dvd_gan_amd import lib as L
    so = L.cls_lib()
    for rows, classes in ((1, 1), (257, 101), (50000, 1000), (1 << 20, 4096)):
        assert so.dvdx_cls_ws_bytes(rows, classes) == rows * L.CLS_ROW_BYTES == rows * 40, (rows, classes)
    for rows, classes in ((0, 8), (8, 0), (-1, 8), (8, -1), ((1 << 20) + 1, 8), (8, 4097), (1 << 40, 8), (-(1 << 40), 8)):
        assert so.dvdx_cls_ws_bytes(rows, classes) == 0, (rows, classes)


def test_every_refusal_needs_no_device():
    from dvd_gan_amd import lib as L
    so = L.cls_lib()
    ARG, SHAPE = -1, -2
    P = [0x1000 * (i + 1) for i in range(5)]              # never dereferenced: every check comes before any launch
    need = so.dvdx_cls_ws_bytes(100, 101)
    ok = dict(dtype=L.CLS_F32, logits=P[0], labels=P[1], rows=100, classes=101, row0=100, n_total=257, splits=10, state=P[2],
              confusion=P[3], ws=P[4], ws_bytes=need, stream=None)
    call = lambda **kw: so.dvdx_cls_update(*{**ok, **kw}.values())
    for name in ("logits", "state", "ws"):
        assert call(**{name: None}) == ARG, name
    assert call(labels=None) == ARG                        # a confusion matrix without labels
    assert call(ws=P[4] + 4) == ARG
    for dtype in (-1, 3, 7):
        assert call(dtype=dtype) == ARG, dtype
    for name in ("rows", "classes", "n_total", "splits"):
        for v in (0, -1):
            assert call(**{name: v}) == ARG, (name, v)
    assert call(row0=-1) == ARG and call(rows=-(1 << 40)) == ARG
    assert call(classes=4097) == SHAPE and call(rows=(1 << 20) + 1, n_total=1 << 30, ws_bytes=1 << 40) == SHAPE
    assert call(splits=1025, n_total=1 << 30) == SHAPE and call(n_total=(1 << 40) + 1) == SHAPE
    assert call(splits=258) == ARG and call(n_total=5, row0=0, rows=5, splits=6) == ARG      # splits > n_total
    assert call(row0=158) == ARG and call(n_total=199) == ARG and call(row0=1 << 62) == ARG   # row0 + rows > n_total
    for short in (need - 1, 0, -5):
        assert call(ws_bytes=short) == ARG, short


def test_the_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(ROOT, "dvd_gan_amd", "xsrc", "cls", "build", "cls.res")
    assert os.path.exists(path), "xsrc/cls/build/cls.res: the library was not built by csrc/build.sh in this tree"
    text = open(path).read()
    kernels = {"cls_row_kernel": 3, "cls_split_kernel": 3, "cls_confusion_kernel": 1}      # one per logits dtype
    for kernel, count in kernels.items():
        assert len(re.findall(r"Function Name: \S*" + kernel, text)) == count, kernel
    total = sum(kernels.values())
    assert text.count("Function Name:") == total
    found = {k: [int(v) for v in re.findall(r"remark:\s+" + re.escape(k) + r": (\d+)", text)]
             for k in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill")}
    assert found == {k: [0] * total for k in found}, found
    assert text.count("Dynamic Stack: False") == total

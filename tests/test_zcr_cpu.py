"""Latent consistency regularization without a GPU: the numpy restatement (tests/zcr_ref.py) against torch's autograd in fp64, the
handshake, the argument checks and the resource report of libdvdx_zcr.so, and the Trainer's three keywords."""
import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zcr_ref as R  # noqa: E402

E32 = 2.0 ** -24


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("pairs,n", [(1, 1), (1, 37), (2, 1000), (3, 4099), (5, 8)])
@pytest.mark.parametrize("weight", [0.0, 0.5, 8.0])
def test_restatement_against_autograd(pairs, n, weight):
    both = R.make_halves(pairs, n)
    a, b = both[:pairs], both[pairs:]
    ref = R.dist(a, b, weight)
    ta = torch.from_numpy(a.copy()).double().requires_grad_(True)
    tb = torch.from_numpy(b.copy()).double().requires_grad_(True)
    msq = ((ta - tb) ** 2).mean()
    term = -weight * msq
    (0.5 * term).backward()                                                # upstream = 0.5
    term, msq = term.detach(), msq.detach()
    # the restatement rounds each gap to fp32 before squaring ((1 + E)^2 on every addend) and the result once more
    assert abs(float(ref["term"]) - float(term)) <= 4 * E32 * abs(float(term))
    assert abs(float(ref["mean_sq_dist"]) - float(msq)) <= 4 * E32 * float(msq)
    per_pair = ((ta - tb) ** 2).mean(1).detach()
    assert abs(float(ref["min_pair"]) - float(per_pair.min())) <= 4 * E32 * float(per_pair.min())
    assert abs(float(ref["max_pair"]) - float(per_pair.max())) <= 4 * E32 * float(per_pair.max())
    assert float(ref["min_pair"]) <= float(ref["mean_sq_dist"]) * (1 + 2 * E32) and float(ref["mean_sq_dist"]) <= float(ref["max_pair"]) * (1 + 2 * E32)
    assert float(ref["max_abs_diff"]) == float((torch.from_numpy(a) - torch.from_numpy(b)).abs().max()) and ref["pairs"] == pairs
    # the gradient: three fp32 roundings (gap, g, product) against fp64
    da, db = R.grad(a, b, weight, 0.5)
    assert da.dtype == db.dtype == np.float32 and np.array_equal(da, -db)
    scale = float(ta.grad.abs().max())
    assert float(np.abs(da.astype(np.float64) - ta.grad.numpy()).max()) <= 4 * E32 * scale
    assert float(np.abs(db.astype(np.float64) - tb.grad.numpy()).max()) <= 4 * E32 * scale
    if weight == 0.0:
        assert float(ref["term"]) == 0.0 and not da.any()
    # the inputs hold what the kernel tests need: identical elements, a pair of elements one bit apart, distinct rows
    if n >= 37:
        assert 0 < int((a == b).sum()) < a.size and float(np.abs(a - b)[np.abs(a - b) > 0].min()) <= 2.0 ** -24
    if pairs > 1 and n > 100:
        assert float(ref["min_pair"]) < 0.5 * float(ref["max_pair"])


def test_ulps_counts_fp32_spacings():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    assert R.ulps(one, one) == 0.0 and R.ulps(up, one) == 1.0 and R.ulps(np.nextafter(up, np.float32(2.0)), one) == 2.0
    assert R.ulps(np.float32(-0.0), np.float32(0.0)) == 0.0 and R.ulps(np.float32(1.001), one) > 1000


# ------------------------------------------------------------------ the library
NAMES = ["dvdx_zcr_abi_version", "dvdx_zcr_strerror", "dvdx_zcr_chunks", "dvdx_zcr_ws_doubles", "dvdx_zcr_dist", "dvdx_zcr_dist_grad"]
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


def test_zcr_handshake():
    import shutil
    import subprocess
    from dvd_gan_amd import lib as L
    assert list(L.ZCR_EXTENSIONS) == ["zcr"]
    rec = L.ZCR_EXTENSIONS["zcr"]
    assert L._record("zcr") is rec
    assert (rec.so, rec.header, rec.env) == ("libdvdx_zcr.so", "dvdx_zcr.h", "DVDX_ZCR_LIB_PATH")
    assert L.library_path("zcr") == os.path.join(ROOT, "dvd_gan_amd", "xsrc", "libdvdx_zcr.so")
    header = os.path.join(ROOT, "include", rec.header)
    want, called = _declared(header)
    assert sorted(want) == called == sorted(NAMES)
    assert {n: s.replace(" ", "") for n, s in rec.signatures.items()} == want
    loaded = L._load("zcr")
    assert L.load_zcr_extensions() == [loaded] and L.zcr_lib() is loaded
    for name, sig in rec.signatures.items():
        fn, sig = getattr(loaded, name), sig.replace(" ", "")
        assert fn.restype is L._CTYPES[sig[0]] and list(fn.argtypes) == [L._CTYPES[c] for c in sig[1:]], name
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", L.library_path("zcr")]).decode()
        exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1] not in ("_init", "_fini"))
        assert exported == sorted(want), exported
    text = open(header).read()
    defines = {n: int(v) for n, v in re.findall(r"^#define (DVDX_[A-Z0-9_]+)\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", text, flags=re.M)}
    assert defines == rec.constants and len(defines) == 13
    assert defines["DVDX_ZCR_MAX_PAIRS"] == 1 << 16 and defines["DVDX_ZCR_MAX_N"] == 1 << 40 and defines["DVDX_ZCR_THREADS"] == 256
    assert defines["DVDX_ZCR_NSTAT"] == 6 and sorted(v for k, v in defines.items() if "_STAT_" in k) == list(range(6))
    assert rec.abi == ("dvdx_zcr_abi_version", L.ZCR_ABI_VERSION) and loaded.dvdx_zcr_abi_version() == defines["DVDX_ZCR_ABI_VERSION"]
    with pytest.raises(RuntimeError, match=r"^libdvdx_zcr: .*weight.* \(code -1\)$"):
        L.zcr_check(-1)
    with pytest.raises(RuntimeError, match=r"^libdvdx_zcr: .*65536 pairs.* \(code -2\)$"):
        L.zcr_check(-2)
    assert loaded.dvdx_zcr_strerror(0) == b"ok" and loaded.dvdx_zcr_strerror(-3) == b"kernel launch failed"
    assert loaded.dvdx_zcr_strerror(-77) == b"unknown error"
    try:
        rec.signatures["dvdx_no_such_entry"] = "i p"
        L._handles.pop("zcr", None)
        with pytest.raises(RuntimeError, match="libdvdx_zcr.so exports no dvdx_no_such_entry -- lib.py and include/dvdx_zcr.h disagree"):
            L._load("zcr")
        assert "zcr" not in L._handles
    finally:
        del rec.signatures["dvdx_no_such_entry"]
        L._handles.pop("zcr", None)
        assert L._load("zcr") is L._handles["zcr"]


def test_the_other_tables_are_what_they_were():
    from dvd_gan_amd import lib as L
    assert list(L.LIBRARIES) == ["core", "adv", "eval", "prdc", "aug", "geom", "sv"] and list(L.EXTENSIONS) == ["tsru"]
    assert list(L.MORE_EXTENSIONS) == ["cr"]
    assert L.load_more_extensions() == [L._load("cr")] and L._load("zcr") not in L.load_all() + L.load_more_extensions()
    for rec in list(L.LIBRARIES.values()) + list(L.EXTENSIONS.values()) + list(L.MORE_EXTENSIONS.values()):
        assert not [n for n in rec.signatures if n.startswith("dvdx_zcr")] and not [n for n in rec.constants if "_ZCR_" in n]
    assert L.library_path("cr") == os.path.join(ROOT, "dvd_gan_amd", "xsrc", "libdvdx_cr.so")


def test_build_loads_the_new_library():
    import inspect
    import __graft_entry__ as G
    assert "lib.load_zcr_extensions()" in inspect.getsource(G.build)


def test_the_sizing_query():
    from dvd_gan_amd import lib as L
    so = L.zcr_lib()
    # C = min(ceil(n / 4096), max(1, 2048 / pairs)); the workspace holds a sum and a maximum per chunk
    for pairs, n, chunks in ((1, 1, 1), (1, 4096, 1), (1, 4097, 2), (3, 13001, 4), (64, 589824, 32), (2, 1 << 33, 1024),
                             (2048, 1 << 20, 1), (3000, 1 << 20, 1), (1 << 16, 5, 1)):
        assert so.dvdx_zcr_chunks(pairs, n) == chunks and so.dvdx_zcr_ws_doubles(pairs, n) == 2 * pairs * chunks, (pairs, n)
    for pairs, n in ((0, 8), (8, 0), (-1, 8), (8, -1), ((1 << 16) + 1, 8), (8, (1 << 40) + 1)):
        assert so.dvdx_zcr_chunks(pairs, n) == 0 and so.dvdx_zcr_ws_doubles(pairs, n) == 0, (pairs, n)


def test_every_refusal_needs_no_device():
    from dvd_gan_amd import lib as L
    so = L.zcr_lib()
    ARG, SHAPE = -1, -2
    P = [0x1000 * (i + 1) for i in range(8)]              # never dereferenced: every check comes before any launch
    need = so.dvdx_zcr_ws_doubles(3, 13001)
    ok = dict(a=P[0], b=P[1], pairs=3, n=13001, weight=0.5, ws=P[2], ws_doubles=need, term=P[3], stats=None, stream=None)
    call = lambda **kw: so.dvdx_zcr_dist(*{**ok, **kw}.values())
    okg = dict(a=P[0], b=P[1], pairs=3, n=13001, weight=0.5, upstream=P[4], da=P[5], db=P[6], stream=None)
    callg = lambda **kw: so.dvdx_zcr_dist_grad(*{**okg, **kw}.values())
    for name in ("a", "b", "ws", "term"):
        assert call(**{name: None}) == ARG, name
    for name in ("a", "b", "upstream", "da", "db"):
        assert callg(**{name: None}) == ARG, name
    for fn in (call, callg):
        for v in (0, -1, -(1 << 40)):
            assert fn(pairs=v) == ARG and fn(n=v) == ARG, v
        for w in (-1.0, -1e-30, float("inf"), float("-inf"), float("nan")):
            assert fn(weight=w) == ARG, w
        for pairs in ((1 << 16) + 1, 1 << 31, 1 << 40):
            assert fn(pairs=pairs, ws_doubles=1 << 62) == SHAPE if fn is call else fn(pairs=pairs) == SHAPE, pairs
        assert fn(n=(1 << 40) + 1) == SHAPE
    for short in (need - 1, 0, -5):
        assert call(ws_doubles=short) == ARG, short


def test_the_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(ROOT, "dvd_gan_amd", "xsrc", "zcr", "build", "zcr.res")
    assert os.path.exists(path), "xsrc/zcr/build/zcr.res: the library was not built by csrc/build.sh in this tree"
    text = open(path).read()
    kernels = ("zcr_dist_kernel", "zcr_finish_kernel", "zcr_grad_kernel")
    for kernel in kernels:
        assert len(re.findall(r"Function Name: \S*" + kernel, text)) == 1, kernel
    found = {k: [int(v) for v in re.findall(r"remark:\s+" + re.escape(k) + r": (\d+)", text)]
             for k in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill")}
    assert found == {k: [0] * len(kernels) for k in found}, found
    assert text.count("Dynamic Stack: False") == len(kernels)


# ------------------------------------------------------------------ the Trainer's keywords
def _cfg(**extra):
    return argparse.Namespace(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=2, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9,
                              n_class=3, k_sample=4, **extra)


def _cpu_trainer(cfg=None, **kw):
    from dvd_gan_amd.train_step import Trainer
    return Trainer([], cfg if cfg is not None else _cfg(), device=torch.device("cpu"), compute_dtype=torch.float32, **kw)


def test_constructor_keywords():
    from dvd_gan_amd import lib as L
    from dvd_gan_amd.train_step import Trainer
    bare = Trainer.__new__(Trainer)                       # the class-level "off"
    assert (bare.z_cr, bare.z_cr_gen, bare.z_cr_sigma) == (0.0, 0.0, 0.03)
    assert bare._zcr_stats is None and bare._zcr_stats_g is None and bare.zcr_report() is None
    bad = (-1.0, -1e-30, float("inf"), float("-inf"), float("nan"))
    for name in ("z_cr", "z_cr_gen", "z_cr_sigma"):
        for v in bad:
            with pytest.raises(ValueError, match="z_cr="):
                _cpu_trainer(**{name: v})
            with pytest.raises(ValueError, match="z_cr="):
                Trainer([], None, **{name: v})            # refused before the config is read
    off = _cpu_trainer()
    assert (off.z_cr, off.z_cr_gen, off.z_cr_sigma) == (0.0, 0.0, 0.03) and off._zcr_stats is None and off.zcr_report() is None
    assert _cpu_trainer(z_cr=0.0, z_cr_gen=0.0, z_cr_sigma=0.5)._zcr_stats is None          # a sigma alone turns nothing on
    for kw in (dict(z_cr=5.0), dict(z_cr_gen=0.5), dict(z_cr=5.0, z_cr_gen=0.5, z_cr_sigma=0.0)):  # either weight does; no d_aug needed
        on = _cpu_trainer(**kw)
        assert tuple(on._zcr_stats.shape) == (2, L.CR_NSTAT) and tuple(on._zcr_stats_g.shape) == (L.ZCR_NSTAT,)
        assert on._cr_stats is None and on.cr_report() is None                               # tables of their own
        rep = on.zcr_report()
        assert list(rep) == ["Ds", "Dt", "G"]
        assert all(list(rep[k]) == ["penalty", "mean_sq_gap", "max_abs_gap", "nonzero", "n"] for k in ("Ds", "Dt"))
        assert list(rep["G"]) == ["term", "mean_sq_dist", "min_pair", "max_pair", "max_abs_diff", "pairs"]
    both = _cpu_trainer(_cfg(d_aug="color,cutout"), d_cr=10.0, z_cr=5.0, z_cr_gen=0.5, z_cr_sigma=0.1)
    assert (both.z_cr, both.z_cr_gen, both.z_cr_sigma) == (5.0, 0.5, 0.1) and tuple(both._cr_stats.shape) == (4, L.CR_NSTAT)
    # settings that steer future steps: the fingerprint does not know them
    assert off.fingerprint() == _cpu_trainer(z_cr=5.0, z_cr_gen=0.5, z_cr_sigma=0.1).fingerprint()
    from dvd_gan_amd import settings as S
    assert not [row for row in S.SETTINGS if "z_cr" in row[0] or "z_cr" in row[1]]


def test_pinned_draws_need_the_perturbation():
    """A `draws` dict without "z_delta" is a KeyError before anything is launched (no device here); with the feature off the key
    is not asked for."""
    clips, labels = torch.zeros(2, 3, 8, 64, 64), torch.zeros(2, dtype=torch.long)
    draws = {"perm_real": torch.randperm(8), "z": torch.randn(2, 16), "z_class": torch.zeros(2, dtype=torch.long),
             "perm_fake": torch.randperm(8)}
    for kw in (dict(z_cr=5.0), dict(z_cr_gen=0.5)):
        tr = _cpu_trainer(**kw)
        with pytest.raises(KeyError, match="z_delta"):
            tr.train_step(clips, labels, draws)
        with pytest.raises(KeyError, match="z_delta"):
            tr.train_step(clips, labels, [dict(draws, z_delta=torch.zeros(2, 16)), draws])


def test_pair_distance_refuses_what_it_cannot_stream():
    from dvd_gan_amd import functional as Fn
    for both in (torch.zeros(4, 8, dtype=torch.float64), torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(8, 4).t(),
                 torch.zeros(3, 8), torch.zeros(8)):
        with pytest.raises(ValueError, match="PairDistance"):
            Fn.PairDistance.apply(both, 0.5, None)

"""Balanced consistency regularization without a GPU: the float64 restatement (tests/cr_ref.py) against torch's autograd, the
handshake, the argument checks and the resource report of libdvdx_cr.so, and the Trainer's two keywords."""
import argparse
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cr_ref as R  # noqa: E402


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n", [1, 3, 64, 257, 4097])
@pytest.mark.parametrize("weight", [0.0, 0.5, 10.0])
def test_reference_against_autograd(n, weight):
    aug, clean = R.make_logits(n)
    ref = R.pair64(aug, clean, weight)
    a = aug.double().requires_grad_(True)
    c = clean.double().requires_grad_(True)
    loss = weight * ((a - c) ** 2).mean()
    loss.backward()
    loss = loss.detach()
    # fp64 against fp64 in another order of operations: a few roundings of 1.1e-16, relative to the largest term (n addends)
    tol = 4 * (n + 4) * R.D
    assert abs(ref["loss"][0] - float(loss)) <= tol * max(float(loss), 1e-300)
    scale = max(float(a.grad.abs().max()), 1e-300)
    assert float((ref["d_aug"][0] - a.grad).abs().max()) <= tol * scale
    assert float((ref["d_clean"][0] - c.grad).abs().max()) <= tol * scale
    assert ref["n"] == n and ref["nonzero"] == int((aug != clean).sum())
    assert math.isclose(ref["maxabs"][0], float((aug.double() - clean.double()).abs().max()), rel_tol=0, abs_tol=0)
    if weight:
        assert math.isclose(ref["loss"][0], weight * ref["msq"][0], rel_tol=2 * R.D)
    # the inputs hold what the kernel tests need: identical pairs, the two zeros, large values
    if n >= 64:
        assert 0 < ref["nonzero"] < n and float(clean.abs().max()) > 9e3
        assert bool((torch.signbit(aug[0]) != torch.signbit(clean[0])) & (aug[0] == clean[0]))


def test_the_bounds_bite():
    """Planted errors exceed the bounds: a gradient scaled by 1 / n instead of 2 / n, a sum over the first n - 1 pairs, a gap
    rounded to bf16; the reference rounded to fp32 passes them."""
    aug, clean = R.make_logits(257)
    ref = R.pair64(aug, clean, 10.0)
    for name in ("loss", "d_aug", "d_clean", "msq", "maxabs"):
        want, bound = ref[name]
        assert R.ratio(torch.as_tensor(want, dtype=torch.float64).float(), want, bound) <= 1.0, name
    assert R.ratio(0.5 * ref["d_aug"][0], *ref["d_aug"]) > 1e3
    short = R.pair64(aug[:-1], clean[:-1], 10.0)
    assert R.ratio(short["loss"][0] * 256 / 257, *ref["loss"]) > 1e3
    coarse = (aug - clean).bfloat16().double() * (2.0 * 10.0 / 257)
    assert R.ratio(coarse, *ref["d_aug"]) > 1e3


# ------------------------------------------------------------------ the library
NAMES = ["dvdx_cr_abi_version", "dvdx_cr_strerror", "dvdx_cr_pair"]
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


def test_cr_handshake():
    import shutil
    import subprocess
    from dvd_gan_amd import lib as L
    assert list(L.MORE_EXTENSIONS) == ["cr"]
    rec = L.MORE_EXTENSIONS["cr"]
    assert L._record("cr") is rec
    assert (rec.so, rec.header, rec.env) == ("libdvdx_cr.so", "dvdx_cr.h", "DVDX_CR_LIB_PATH")
    assert L.library_path("cr") == os.path.join(ROOT, "dvd_gan_amd", "xsrc", "libdvdx_cr.so")
    header = os.path.join(ROOT, "include", rec.header)
    want, called = _declared(header)
    assert sorted(want) == called == sorted(NAMES)
    assert {n: s.replace(" ", "") for n, s in rec.signatures.items()} == want
    loaded = L._load("cr")
    assert L.load_more_extensions() == [loaded] and L.cr_lib() is loaded
    for name, sig in rec.signatures.items():
        fn, sig = getattr(loaded, name), sig.replace(" ", "")
        assert fn.restype is L._CTYPES[sig[0]] and list(fn.argtypes) == [L._CTYPES[c] for c in sig[1:]], name
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", L.library_path("cr")]).decode()
        exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1] not in ("_init", "_fini"))
        assert exported == sorted(want), exported
    text = open(header).read()
    defines = {n: int(v) for n, v in re.findall(r"^#define (DVDX_[A-Z0-9_]+)\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", text, flags=re.M)}
    assert defines == rec.constants and len(defines) == 9
    assert defines["DVDX_CR_MAX_N"] == 1 << 20 and defines["DVDX_CR_THREADS"] == 256
    assert rec.abi == ("dvdx_cr_abi_version", L.CR_ABI_VERSION) and loaded.dvdx_cr_abi_version() == defines["DVDX_CR_ABI_VERSION"]
    with pytest.raises(RuntimeError, match=r"^libdvdx_cr: .*weight.* \(code -1\)$"):
        L.cr_check(-1)
    with pytest.raises(RuntimeError, match=r"^libdvdx_cr: .*2\^20 pairs \(code -2\)$"):
        L.cr_check(-2)
    assert loaded.dvdx_cr_strerror(0) == b"ok" and loaded.dvdx_cr_strerror(-3) == b"kernel launch failed"
    try:
        rec.signatures["dvdx_no_such_entry"] = "i p"
        L._handles.pop("cr", None)
        with pytest.raises(RuntimeError, match="libdvdx_cr.so exports no dvdx_no_such_entry -- lib.py and include/dvdx_cr.h disagree"):
            L._load("cr")
        assert "cr" not in L._handles
    finally:
        del rec.signatures["dvdx_no_such_entry"]
        L._handles.pop("cr", None)
        assert L._load("cr") is L._handles["cr"]


def test_the_first_two_tables_are_what_they_were():
    from dvd_gan_amd import lib as L
    assert list(L.LIBRARIES) == ["core", "adv", "eval", "prdc", "aug", "geom", "sv"] and list(L.EXTENSIONS) == ["tsru"]
    had_tsru = "tsru" in L._handles
    try:
        assert L.load_extensions() == [L._load("tsru")] and len(L.load_all()) == 7
        assert L._load("cr") not in L.load_all() + L.load_extensions()
    finally:
        if not had_tsru:                                   # tests/test_gpu_tsru.py starts from "not loaded yet"
            L._handles.pop("tsru", None)
    for rec in list(L.LIBRARIES.values()) + list(L.EXTENSIONS.values()):
        assert not [n for n in rec.signatures if n.startswith("dvdx_cr")] and not [n for n in rec.constants if "_CR_" in n]
    assert L.library_path("tsru") == os.path.join(ROOT, "dvd_gan_amd", "xsrc", "libdvdx_tsru.so")
    assert L.library_path("adv") == os.path.join(ROOT, "dvd_gan_amd", "csrc", "libdvdgan_hip_adv.so")


def test_every_refusal_needs_no_device():
    from dvd_gan_amd import lib as L
    so = L.cr_lib()
    ARG, SHAPE = -1, -2
    P = [0x1000 * (i + 1) for i in range(6)]              # never dereferenced: every check comes before any launch
    ok = dict(aug=P[0], clean=P[1], n=8, weight=10.0, loss=P[2], d_aug=P[3], d_clean=P[4], stats=None, stream=None)
    call = lambda **kw: so.dvdx_cr_pair(*{**ok, **kw}.values())
    for name in ("aug", "clean", "loss", "d_aug", "d_clean"):
        assert call(**{name: None}) == ARG, name
    for n in (0, -1, -(1 << 40)):
        assert call(n=n) == ARG, n
    for n in ((1 << 20) + 1, 1 << 31, 1 << 40):
        assert call(n=n) == SHAPE, n
    for w in (-1.0, -1e-30, float("inf"), float("-inf"), float("nan")):
        assert call(weight=w) == ARG, w


def test_the_kernel_uses_no_scratch_and_spills_nothing():
    path = os.path.join(ROOT, "dvd_gan_amd", "xsrc", "cr", "build", "cr.res")
    assert os.path.exists(path), "xsrc/cr/build/cr.res: the library was not built by csrc/build.sh in this tree"
    text = open(path).read()
    assert len(re.findall(r"Function Name: \S*cr_pair_kernel", text)) == 1
    found = {k: [int(v) for v in re.findall(r"remark:\s+" + re.escape(k) + r": (\d+)", text)]
             for k in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill")}
    assert found == {"ScratchSize [bytes/lane]": [0], "SGPRs Spill": [0], "VGPRs Spill": [0]}, found
    assert "Dynamic Stack: False" in text


# ------------------------------------------------------------------ the Trainer's keywords
def _cfg(**extra):
    return argparse.Namespace(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=2, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9,
                              n_class=3, k_sample=4, **extra)


def _cpu_trainer(cfg=None, **kw):
    from dvd_gan_amd.train_step import Trainer
    return Trainer([], cfg if cfg is not None else _cfg(d_aug="color,cutout"), device=torch.device("cpu"),
                   compute_dtype=torch.float32, **kw)


def test_constructor_keywords():
    from dvd_gan_amd import lib as L
    from dvd_gan_amd.train_step import Trainer
    bare = Trainer.__new__(Trainer)                       # the class-level "off"
    assert bare.d_cr == 0.0 and bare.d_cr_fake == 0.0 and bare._cr_stats is None and bare.cr_report() is None
    for kw in (dict(d_cr=-1.0), dict(d_cr=float("nan")), dict(d_cr=float("inf")), dict(d_cr=1.0, d_cr_fake=-0.5),
               dict(d_cr_fake=float("nan")), dict(d_cr_fake=float("inf"))):
        with pytest.raises(ValueError, match="d_cr="):
            _cpu_trainer(**kw)
        with pytest.raises(ValueError, match="d_cr="):
            Trainer([], None, **kw)                       # refused before the config is read
    for kw in (dict(d_cr=10.0), dict(d_cr_fake=1.0), dict(d_cr=0.0, d_cr_fake=2.0)):
        with pytest.raises(ValueError, match="no transform"):
            _cpu_trainer(_cfg(), **kw)                    # neither d_aug nor d_aug_geom
    off = _cpu_trainer()
    assert off.d_cr == 0.0 and off.d_cr_fake == 0.0 and off._cr_stats is None and off.cr_report() is None
    assert _cpu_trainer(_cfg(), d_cr=0.0, d_cr_fake=0.0)._cr_stats is None       # off needs no transform
    same = _cpu_trainer(d_cr=10.0)
    assert same.d_cr == 10.0 and same.d_cr_fake == 10.0                           # None takes d_cr
    two = _cpu_trainer(_cfg(d_aug_geom="xflip"), d_cr=10.0, d_cr_fake=5.0)
    assert (two.d_cr, two.d_cr_fake) == (10.0, 5.0) and tuple(two._cr_stats.shape) == (4, L.CR_NSTAT)
    assert _cpu_trainer(d_cr=0.0, d_cr_fake=5.0)._cr_stats is not None            # either weight turns it on
    rep = two.cr_report()
    assert list(rep) == ["Ds_real", "Ds_fake", "Dt_real", "Dt_fake"]
    assert all(list(v) == ["penalty", "mean_sq_gap", "max_abs_gap", "nonzero", "n"] for v in rep.values())
    # settings that steer future steps: the fingerprint does not know them
    assert off.fingerprint() == same.fingerprint() == _cpu_trainer(d_cr=10.0, d_cr_fake=5.0).fingerprint()
    from dvd_gan_amd import settings as S
    assert not [row for row in S.SETTINGS if "d_cr" in row[0] or "d_cr" in row[1]]

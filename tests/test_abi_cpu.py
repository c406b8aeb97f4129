"""CPU checks of the C-ABI library: it loads, exports every symbol include/dvdgan_hip.h declares, reports
its ABI version, validates arguments without touching a GPU, and the Python host layer reproduces the
reference state_dict layout; the same handshake of every side library of lib.LIBRARIES against its own header, and the table
against the directories and headers of the tree.  (No compute calls: there is no GPU in this tier.)"""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvdgan_hip.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dvd_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from dvd_gan_amd import lib as L
    lib = L.lib()
    names = declared_symbols()
    assert len(names) >= 35
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.dvd_abi_version() == L.ABI_VERSION
    assert b"unsupported shape" in lib.dvd_strerror(-2)
    # ... and nothing else: the internal cross-file entry points (common.h) have hidden visibility
    import shutil
    import subprocess
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", L.library_path("core")]).decode()
        # EVERY defined text symbol, whatever its name (C++ helpers and kernel stubs included): -fvisibility=hidden + the
        # header's visibility pragma leave exactly the declared entry points (_init / _fini come from the C runtime)
        exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1] not in ("_init", "_fini"))
        assert exported == names, sorted(set(exported) ^ set(names))


def test_descriptor_layouts_match_the_library():
    """Layout handshake: sizeof() of every descriptor struct as the .so was compiled == the ctypes mirror in
    dvd_gan_amd/lib.py == (for dvd_conv_desc) the stub INTEGRATION.md section 2 prints.  Changing a descriptor in the header without
    touching lib.py or the document fails here, on the CPU."""
    import ctypes as C
    from dvd_gan_amd import lib as L
    lib = L.lib()
    assert set(L.STRUCT_MIRRORS) == {0, 1, 2, 3, 4, 5, 6}
    for which, mirror in L.STRUCT_MIRRORS.items():
        assert lib.dvd_struct_size(which) == C.sizeof(mirror), (which, mirror.__name__)
    assert lib.dvd_struct_size(99) == -1
    # the struct literally as INTEGRATION.md prints it
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    a = doc.index("class ConvDesc(C.Structure):")
    b = doc.index("assert lib.dvd_abi_version()", a)
    ns = {"C": C}
    exec(doc[a:b], ns)
    stub = ns["ConvDesc"]
    assert C.sizeof(stub) == lib.dvd_struct_size(0)
    assert [(n, getattr(stub, n).offset) for n, _ in stub._fields_] == [(n, getattr(L.ConvDesc, n).offset) for n, _ in L.ConvDesc._fields_]
    assert "dvd_abi_version() == %d" % L.ABI_VERSION in doc
    # a mirror that lost its tail is refused at load
    saved = L.STRUCT_MIRRORS[0]

    class Short(C.Structure):
        _fields_ = L.ConvDesc._fields_[:-2]
    try:
        L.STRUCT_MIRRORS[0] = Short
        L._handles.pop("core", None)
        with pytest.raises(RuntimeError, match="sizeof descriptor 0"):
            L.lib()
        assert "core" not in L._handles                                   # a half-checked handle is never published
    finally:
        L.STRUCT_MIRRORS[0] = saved
        L._handles.pop("core", None)
        L.lib()


_PARAM_CODES = {"long long": "l", "int": "i", "float": "f", "double": "d"}


def declared_signatures(header=HEADER):
    """name -> "<return code><parameter codes>" of every prototype of the header, by a fixed rule: any `*` -> p, long long -> l,
    int -> i, float -> f, double -> d, a lone void -> no parameters; returns also v (void) and s (const char*).  Raises on a
    parameter type outside the rule; a prototype the pattern misses shows as a name declared_symbols() has and this has not."""
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(const\s+char\s*\*|void|int|long\s+long)\s*(dvd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        ret = "s" if "*" in ret else "v" if ret == "void" else _PARAM_CODES[" ".join(ret.split())]
        codes = ""
        for p in ([] if params.strip() == "void" else params.split(",")):
            if "*" in p:
                codes += "p"
                continue
            words = [w for w in p.split() if w != "const"]
            kind = " ".join(words[:-1])                  # (the last word is the parameter's name)
            if kind not in _PARAM_CODES:
                raise ValueError(f"{name}: parameter {p.strip()!r} has a type the signature codes do not cover")
            codes += _PARAM_CODES[kind]
        assert name not in out, name
        out[name] = ret + codes
    return out


def signature_mismatches(table):
    want = declared_signatures()
    assert sorted(want) == declared_symbols() and len(want) == 90       # the pattern missed no prototype
    assert sorted(table) == sorted(want), sorted(set(table) ^ set(want))
    return sorted(n for n in want if table[n].replace(" ", "") != want[n])


def test_signature_table_matches_the_header():
    """Signatures, the third part of the handshake (symbols and descriptor sizes above): lib.SIGNATURES, which types every
    entry point of the loaded library, says what the header's prototypes say."""
    from dvd_gan_amd import lib as L
    assert signature_mismatches(L.SIGNATURES) == []
    # the check can fail: one `long long` declared as `int` is named ...
    wrong = dict(L.SIGNATURES)
    assert wrong["dvd_adam_step"].replace(" ", "")[5] == "l"
    wrong["dvd_adam_step"] = "i pppp i ffff i p"
    assert signature_mismatches(wrong) == ["dvd_adam_step"]
    wrong = dict(L.SIGNATURES, dvd_strerror="i i")                        # ... a return type too ...
    assert signature_mismatches(wrong) == ["dvd_strerror"]
    del wrong["dvd_swap_f32"]                                             # ... and a missing line
    with pytest.raises(AssertionError, match="dvd_swap_f32"):
        signature_mismatches(wrong)


def test_unknown_parameter_types_are_refused(tmp_path):
    path = tmp_path / "h.h"
    path.write_text("int dvd_abi_version(void);\nint dvd_new_thing(const float* p, size_t n, void* stream);\n")
    with pytest.raises(ValueError, match="dvd_new_thing.*size_t n"):
        declared_signatures(str(path))


def test_loaded_library_is_fully_typed():
    import ctypes as C
    from dvd_gan_amd import lib as L
    lib = L.lib()
    kinds = {"i": C.c_int, "l": C.c_longlong, "f": C.c_float, "d": C.c_double, "p": C.c_void_p, "v": None, "s": C.c_char_p}
    for name, sig in L.SIGNATURES.items():
        fn, sig = getattr(lib, name), sig.replace(" ", "")
        assert fn.restype is kinds[sig[0]], name
        assert list(fn.argtypes) == [kinds[c] for c in sig[1:]], name
        assert "v" not in sig[1:] and "s" not in sig[1:], name
    # a table line without a function in the library is refused at load
    try:
        L.SIGNATURES["dvd_no_such_entry"] = "i p"
        L._handles.pop("core", None)
        with pytest.raises(RuntimeError, match="exports no dvd_no_such_entry"):
            L.lib()
        assert "core" not in L._handles
    finally:
        del L.SIGNATURES["dvd_no_such_entry"]
        L._handles.pop("core", None)
        L.lib()


# ------------------------------------------------------------------ the side libraries: one handshake, library by library
SIDE_LIBRARIES = {      # key of lib.LIBRARIES -> the entry points its header declares, the number of its #defines
    "adv": (["dvd_adv_loss_ex"], 10),
    "eval": (["dvd_eval_strerror", "dvd_eval_pool_features", "dvd_eval_moments_state_doubles", "dvd_eval_moments_update",
              "dvd_eval_kid_ws_doubles", "dvd_eval_kid"], 3),
    "prdc": (["dvd_prdc_strerror", "dvd_prdc_column_mean", "dvd_prdc_knn_ws_doubles", "dvd_prdc_knn_radii",
              "dvd_prdc_ball_ws_doubles", "dvd_prdc_ball_count"], 4),
    "aug": (["dvd_aug_abi_version", "dvd_aug_strerror", "dvd_aug_clip_forward", "dvd_aug_clip_backward"], 14),
    "geom": (["dvd_geom_abi_version", "dvd_geom_strerror", "dvd_geom_clip_forward", "dvd_geom_clip_backward"], 11),
    "sv": (["dvd_sv_abi_version", "dvd_sv_item_size", "dvd_sv_strerror", "dvd_sv_prepare", "dvd_sv_init", "dvd_sv_iterate",
            "dvd_sv_ritz"], 5),
}


@pytest.mark.parametrize("key", sorted(SIDE_LIBRARIES))
def test_side_library_handshake(key):
    """libdvdgan_hip_<key>.so against include/dvdgan_hip_<key>.h, the checks made of the core library above, with the same parser:
    the library exports exactly the header's declarations, the signature table says what the prototypes say and types every loaded
    function, the constants dict holds every #define of the header by name and value, the ABI version (where the library has
    one) is the expected one, and a table line without a function in the library is refused at load."""
    import shutil
    import subprocess
    from dvd_gan_amd import lib as L
    rec = L.LIBRARIES[key]
    names, n_defines = SIDE_LIBRARIES[key]
    assert (rec.so, rec.header) == (f"libdvdgan_hip_{key}.so", f"dvdgan_hip_{key}.h")
    header = os.path.join(ROOT, "include", rec.header)
    text = open(header).read()
    want = declared_signatures(header)
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(want) == sorted(set(re.findall(r"\b(dvd_[a-z0-9_]+)\s*\(", src))) == sorted(names)
    assert {n: sig.replace(" ", "") for n, sig in rec.signatures.items()} == want
    loaded = L._load(key)
    for name, sig in rec.signatures.items():
        fn, sig = getattr(loaded, name), sig.replace(" ", "")
        assert fn.restype is L._CTYPES[sig[0]] and list(fn.argtypes) == [L._CTYPES[c] for c in sig[1:]], name
    if shutil.which("nm"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", L.library_path(key)]).decode()
        exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1] not in ("_init", "_fini"))
        assert exported == sorted(want), exported
    defines = {n: int(v) for n, v in re.findall(r"^#define (DVD_[A-Z0-9_]+)\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", text, flags=re.M)}
    assert defines == rec.constants and len(defines) == n_defines
    assert (rec.abi is not None) == (f"dvd_{key}_abi_version" in names)
    if rec.abi:
        assert rec.abi[0] == f"dvd_{key}_abi_version" and getattr(loaded, rec.abi[0])() == rec.abi[1]
    # a table line without a function in the library is refused at load, and the library loads again afterwards
    try:
        rec.signatures["dvd_no_such_entry"] = "i p"
        L._handles.pop(key, None)
        with pytest.raises(RuntimeError, match=f"{rec.so} exports no dvd_no_such_entry -- lib.py and include/{rec.header} disagree"):
            L._load(key)
        assert key not in L._handles
    finally:
        del rec.signatures["dvd_no_such_entry"]
        L._handles.pop(key, None)
        assert L._load(key) is L._handles[key]


def test_libraries_know_nothing_of_one_another():
    """Over every ordered pair of lib.LIBRARIES, the core library included: no entry point of one table is in the other's, no
    constant of one is among the other's, and the loaded other has no such function.  A side library also owns its prefix,
    dvd_<key>* and DVD_<KEY>_*, in every other table (dvd_adv_loss of the core library is older than the adv library)."""
    import itertools
    from dvd_gan_amd import lib as L
    assert list(L.LIBRARIES) == ["core"] + list(SIDE_LIBRARIES)
    for a, b in itertools.permutations(L.LIBRARIES, 2):
        mine, other = L.LIBRARIES[a], L.LIBRARIES[b]
        assert not set(mine.signatures) & set(other.signatures), (a, b)
        assert not set(mine.constants) & set(other.constants), (a, b)
        assert not [n for n in mine.signatures if hasattr(L._load(b), n)], (a, b)
        if a != "core":
            assert [n for n in other.signatures if n.startswith("dvd_" + a)] == (["dvd_adv_loss"] if (a, b) == ("adv", "core") else []), (a, b)
            assert not [n for n in other.constants if n.startswith("DVD_" + a.upper() + "_")], (a, b)


def test_library_table_names_the_directories_and_headers():
    """lib.LIBRARIES, the *.hip-holding sub-directories of csrc/ (csrc/build.sh makes a library of each) and the dvdgan_hip_*.h
    files under include/ name the same set, and the module-level names call sites use are views of the table."""
    import glob
    from dvd_gan_amd import lib as L
    csrc = os.path.join(ROOT, "dvd_gan_amd", "csrc")
    dirs = {os.path.basename(os.path.dirname(f)) for f in glob.glob(os.path.join(csrc, "*", "*.hip"))}
    headers = {os.path.basename(f)[len("dvdgan_hip_"):-2] for f in glob.glob(os.path.join(ROOT, "include", "dvdgan_hip_*.h"))}
    assert dirs == headers == set(L.LIBRARIES) - {"core"} and dirs
    assert glob.glob(os.path.join(csrc, "*.hip")) and os.path.exists(HEADER)
    for key, rec in L.LIBRARIES.items():
        suffix, pre = ("", "") if key == "core" else ("_" + key, key.upper() + "_")
        assert (rec.so, rec.header, rec.env) == (f"libdvdgan_hip{suffix}.so", f"dvdgan_hip{suffix}.h", f"DVD_{pre}LIB_PATH"), key
        assert getattr(L, pre + "SIGNATURES") is rec.signatures and getattr(L, pre + "HEADER_CONSTANTS") is rec.constants, key
        assert getattr(L, pre + "LIB_PATH") == L.library_path(key) == (os.environ.get(rec.env) or os.path.join(csrc, rec.so)), key
        assert getattr(L, pre.lower() + "lib")() is L._load(key) is L._handles[key], key
        assert rec.abi is None or rec.abi[1] == getattr(L, pre + "ABI_VERSION"), key
        assert (rec.strerror is None) == (key == "adv") and (rec.strerror is None or rec.strerror in rec.signatures), key
        if rec.strerror:
            with pytest.raises(RuntimeError, match=rf"^libdvdgan_hip{suffix}: .* \(code -1\)$"):
                getattr(L, pre.lower() + "check")(-1)


def test_load_all_refuses_a_missing_library(monkeypatch):
    """What __graft_entry__.build() ends with: every library of the table is loaded, so a missing one (here libdvdgan_hip_geom.so,
    by its path override, which is read at load time) is an error there."""
    from dvd_gan_amd import lib as L
    assert L.load_all() == [L._load(key) for key in L.LIBRARIES]
    monkeypatch.setenv("DVD_GEOM_LIB_PATH", "/nonexistent/libdvdgan_hip_geom.so")
    monkeypatch.delitem(L._handles, "geom")
    with pytest.raises(RuntimeError, match="/nonexistent/libdvdgan_hip_geom.so is missing: build it with .*no CPU / eager fallback"):
        L.load_all()


def test_long_long_arguments_survive_as_plain_ints():
    """A plain Python int reaches a `long long` parameter whole (untyped, ctypes would pass its low 32 bits as an int)."""
    import ctypes as C
    from dvd_gan_amd import lib as L
    lib = L.lib()
    for n in (2 ** 31 + 5, 2 ** 33):
        got = lib.dvd_grad_guard_ws_bytes(n)
        assert got == lib.dvd_grad_guard_ws_bytes(C.c_longlong(n))
        assert got >= 12 * -(-n // L.GUARD_CH)                            # the bound of tests/test_guard_cpu.py
    P_, C_ = 64, 8
    for frames in (2 ** 31 // P_ + 3, 2 ** 33 + 16):                      # frames * P > 2^31; a frame count above 2^32 whose low word is 16
        got = lib.dvd_cbn_backward_ws_floats(frames, P_, C_)
        assert got == lib.dvd_cbn_backward_ws_floats(C.c_longlong(frames), P_, C_)
        assert got == 0 or got >= frames * 2 * C_                         # refused, or [2C] partial sums for every frame: never for 16 of them


def test_float_arguments_convert_by_declaration():
    import ctypes as C
    from dvd_gan_amd import lib as L
    lib = L.lib()
    p = C.c_void_p(16)                                                    # never dereferenced: refused before any launch
    for decay in (1.0, 1.5, -0.1, float("nan")):                          # the decay check of tests/test_ema_cpu.py
        assert lib.dvd_ema_step(p, p, 100, decay, None) == lib.dvd_ema_step(p, p, C.c_longlong(100), C.c_float(decay), None) == -1
    for max_norm in (0.0, -1.0, float("nan")):                            # the max_norm check of tests/test_guard_cpu.py
        plain = lib.dvd_grad_guard(p, 100, max_norm, 1, 1, p, p, None, 0, None)
        assert plain == lib.dvd_grad_guard(p, C.c_longlong(100), C.c_float(max_norm), 1, C.c_longlong(1), p, p, None, 0, None) == -1
    assert lib.dvd_ema_step(None, p, 100, 0.5, None) == -1                # a good decay gets as far as the pointer check


def test_missing_arguments_raise():
    from dvd_gan_amd import lib as L
    lib = L.lib()
    assert lib.dvd_grad_guard_ws_bytes(0) == 0
    with pytest.raises(TypeError):
        lib.dvd_grad_guard_ws_bytes()
    with pytest.raises(TypeError):
        lib.dvd_ema_step(None, None, 100, 0.5)                            # the stream is missing
    with pytest.raises(ctypes.ArgumentError):
        lib.dvd_grad_guard_ws_bytes(1.5)                                  # and a float is no element count


def test_header_constants_match_the_header():
    """Every value lib.py copies from a #define of the header, compared by name."""
    from dvd_gan_amd import kern as K, lib as L, metrics
    src = open(HEADER).read()
    defines = {n: int(v) for n, v in re.findall(r"^#define (DVD_[A-Z0-9_]+)\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", src, flags=re.M)}
    assert len(L.HEADER_CONSTANTS) >= 43
    for name, value in L.HEADER_CONSTANTS.items():
        assert name in defines, name
        assert defines[name] == value, (name, value, defines[name])
    # the groups modules re-export are the checked values, and the descriptor indices are the mirrors' keys
    for name in ("GUARD_CH", "GUARD_STATE", "ORTHO_COLS", "ORTHO_OFF", "ORTHO_H", "ORTHO_W", "METRICS_SIGNED", "METRICS_QUANTIZE",
                 "SHEET_FILL", "SHEET_SIGNED"):
        assert getattr(K, name) is L.HEADER_CONSTANTS["DVD_" + name], name
    assert (metrics.MIN_SIDE, metrics.MAX_SIDE) == (defines["DVD_METRICS_MIN_SIDE"], defines["DVD_METRICS_MAX_SIDE"])
    assert set(L.STRUCT_MIRRORS) == {v for n, v in L.HEADER_CONSTANTS.items() if n.startswith("DVD_STRUCT_")}
    assert {n for n in defines if n.startswith("DVD_STRUCT_")} == {n for n in L.HEADER_CONSTANTS if n.startswith("DVD_STRUCT_")}


def test_argument_validation_needs_no_gpu():
    from dvd_gan_amd import lib as L
    lib = L.lib()
    d = L.ConvDesc()                        # all-zero descriptor: null pointers
    assert lib.dvd_conv_forward(ctypes.byref(d), None) == -1
    w = L.WgradDesc()
    assert lib.dvd_conv_wgrad(ctypes.byref(w), None) == -1
    assert lib.dvd_conv_pick_nsplit(L.BF16, 1024, 512, 512, 25) == 8       # capped
    assert lib.dvd_conv_pick_nsplit(L.BF16, 65536, 512, 256, 25) == 1
    with pytest.raises(RuntimeError):
        L.check(-2)


def test_dispatch_queries_need_no_gpu():
    """The shape queries behind the round-4 kernels (which weight image a convolution wants, whether the MFMA attention serves a
    call, workspace sizes) are pure host logic."""
    from dvd_gan_amd import lib as L
    lib = L.lib()

    def conv(C_, cout, k, H, W, T=1, kt=1, frames=64, **kw):
        d = L.ConvDesc()
        d.dtype, d.frames, d.T, d.H, d.W = L.BF16, frames, T, H, W
        d.C, d.ldi, d.Cout, d.ldo = C_, C_, cout, max(8, (cout + 7) // 8 * 8)
        d.kt, d.kh, d.kw, d.nsplit = kt, k, k, 1
        d.inp = d.out = d.w = 1                      # never dereferenced by the query
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    want = lambda d: lib.dvd_conv_wants_fragment_major(ctypes.byref(d))
    assert want(conv(256, 256, 5, 32, 32)) == 1               # halo-staged kernel, fragment-major image
    assert want(conv(8, 64, 3, 64, 64)) == 2                  # a discriminator stem: thin-input image
    assert want(conv(8, 64, 3, 32, 32, T=12, kt=3)) == 2
    assert want(conv(64, 3, 3, 64, 64)) == 3                  # the RGB layer: thin-output image
    assert want(conv(8, 64, 3, 64, 64, out_f32=1)) == 2       # fp32 output (parity tests): the thin-input kernel as well
    assert want(conv(8, 64, 3, 128, 128)) == 1                # 128-pixel lines: the general kernel
    assert want(conv(128, 128, 1, 64, 64)) == 0               # 1 x 1: tap-by-tap kernel, no image
    d = conv(8, 64, 3, 64, 64)
    d.wq, d.wq_kind = 1, 3                                    # a thin-output image handed to a thin-input request
    assert lib.dvd_conv_forward(ctypes.byref(d), None) == -1
    ok = lib.dvd_attention_mfma_ok
    assert ok(L.BF16, 160, 16, 16, 32, 128, 128, 256) == 1 and ok(L.BF16, 160, 16, 16, 32, 128, 128, 1024) == 1
    assert ok(L.F32, 160, 16, 16, 32, 128, 128, 256) == 0 and ok(L.BF16, 80, 8, 8, 16, 64, 64, 256) == 0
    assert ok(L.BF16, 160, 16, 16, 32, 128, 128, 48) == 0     # not whole 32-token blocks
    assert ok(L.BF16, 160, 16, 16, 32, 128, 128, 32) == 1 and ok(L.BF16, 160, 16, 16, 32, 128, 128, 4096) == 1
    assert ok(L.BF16, 160, 16, 16, 32, 128, 128, 4128) == 0   # past the 4096-token limit
    w = L.WgradDesc()
    w.dtype, w.frames, w.T, w.H, w.W = L.BF16, 64, 12, 32, 32
    w.C, w.ldx, w.Cin_real, w.Cout, w.Cy, w.ldy = 8, 8, 3, 64, 64, 64
    w.kt, w.kh, w.kw = 3, 3, 3
    w.s_co, w.s_ci, w.s_tap = 81, 27, 1
    w.x = w.dy = w.dw = 1
    thin = lib.dvd_conv_wgrad_ws_floats(ctypes.byref(w))
    assert thin == (2048 + 16) * (18 * 1024 + 8)              # persistent workgroups + the 16 partials of the first reduce stage
    w.dtype = L.F32
    assert lib.dvd_conv_wgrad_ws_floats(ctypes.byref(w)) != thin     # exact mode: the general kernels
    ws = lib.dvd_convgru_ws_floats
    assert ws(L.BF16, 64, 4, 4, 256, 3) == 8 * 1024 * 512     # 8 slices of [1024 rows][2h = 512]
    assert ws(L.BF16, 64, 32, 32, 128, 3) == 65536 * 256      # unsplit: one slab of whole 256-column tiles


@pytest.mark.parametrize("frames,S,cin,cout,k,up2,floats", [
    (3072, 16, 256, 256, 3, 0, 24837120),
    (3072, 32, 128, 128, 3, 0, 12566400),
    (3072, 32, 128, 256, 5, 0, 20544000),
    (3072, 32, 256, 128, 5, 0, 20512000),
    (3072, 32, 256, 384, 5, 0, 19691520),
    (3072, 64, 64, 64, 3, 0, 9486336),
    (3008, 4, 256, 256, 3, 0, 6521856),
    (3072, 4, 256, 256, 3, 0, 7114752),
    (3072, 64, 128, 64, 3, 1, 12615680),
    (64, 32, 128, 256, 3, 0, 4743168),
    (64, 8, 256, 512, 3, 0, 0),
])
def test_wgrad_workspace_sizes_are_pinned(frames, S, cin, cout, k, up2, floats):
    """dvd_conv_wgrad_ws_floats on benchmark shapes: the planner's tile, slice count and the slice-workspace layout (partial tiles +
    bias partials) together decide this number, so a change of any of them shows here without a GPU.  Values computed on the CPU from
    the code before the planner was split into steps.  (Equal totals do not prove equal plans: 256 x 64 and 128 x 128 tiles give the
    same size.)"""
    from dvd_gan_amd import lib as L
    lib = L.lib()
    pad8 = lambda c: (c + 7) // 8 * 8
    w = L.WgradDesc()
    w.dtype, w.frames, w.T, w.H, w.W = L.BF16, frames, 1, S, S
    w.C, w.ldx, w.Cin_real, w.Cout, w.Cy, w.ldy = pad8(cin), pad8(cin), cin, cout, pad8(cout), pad8(cout)
    w.kt, w.kh, w.kw, w.up2, w.msplit = 1, k, k, up2, 0
    w.s_co, w.s_ci, w.s_tap = cin * k * k, k * k, 1
    w.x = w.dy = w.dw = 1                            # never dereferenced by the query
    assert lib.dvd_conv_wgrad_ws_floats(ctypes.byref(w)) == floats


@pytest.mark.parametrize("hw", [32, 64])
@pytest.mark.parametrize("cin,cout,kind", [(8, 64, 2), (64, 8, 3)])
def test_pool2_requests_skip_the_thin_kernels(cin, cout, kind, hw):
    """A pool2 request (the 2 x 2 sums of an x2-upsampling conv's input gradient, written on the half-size grid) must not be handed
    to the thin-input / thin-output kernels: they have no pool2 epilogue and would write a full-size result into the quarter-size
    buffer.  It goes to the halo-staged kernel's epilogue instead; without pool2 the same geometry keeps its thin kernel.  Queries
    only: dvd_conv_forward is never called with the placeholder pointers."""
    from dvd_gan_amd import lib as L
    lib = L.lib()
    d = L.ConvDesc()
    d.dtype, d.frames, d.T, d.H, d.W = L.BF16, 2, 1, hw, hw
    d.C, d.ldi, d.Cout, d.ldo = cin, cin, cout, cout
    d.kt, d.kh, d.kw, d.nsplit = 1, 3, 3, 1
    d.inp = d.out = d.w = 1                          # never dereferenced by the queries
    assert lib.dvd_conv_wants_fragment_major(ctypes.byref(d)) == kind
    assert lib.dvd_conv_pool2_ok(ctypes.byref(d)) == 0
    d.pool2 = 1
    assert lib.dvd_conv_pool2_ok(ctypes.byref(d)) == 1
    assert lib.dvd_conv_wants_fragment_major(ctypes.byref(d)) == 1


CONV_QUERY_PINS = [    # per case of test_gpu_conv.CASES: "forward backward-data", each (nsplit 1, 2) x (pool2 0, 1) -> wants digit, pool2_ok digit
    "10000000 10000000", "10001000 10001000", "00000000 00000000", "10000000 10111000", "10110000 10110000", "10110000 10110000",
    "00000000 00000000", "00000000 00000000", "10001000 10001000", "10110000 10111000", "00000000 00000000", "10111000 10111000",
    "10000000 10111000", "10110000 10110000", "10001000 10001000", "10110000 10111000", "10000000 10111000", "10110000 10111000",
    "10111000 10111000", "10111000 10111000", "10111000 10111000", "10111000 10111000", "10001000 10001000", "00000000 00000000",
    "10001000 10001000", "10110000 10111000", "10111000 10111000", "10111000 10111000", "10001000 10001000", "10111000 10111000",
    "10111000 10111000", "10001000 10001000", "10001000 10111000", "10001000 10111000", "10001000 10111000", "10001000 10111000",
    "10001000 10111000", "10001000 10001000", "10111000 10111000", "10110000 10111000", "00000000 00000000", "10001000 10001000",
    "10000000 10000000", "10000000 10001000", "10000000 10001000", "10001000 10001000", "10001000 10001000", "20110000 30111000",
    "10001000 10001000", "30111000 20110000", "10001000 20001000", "00000000 00000000", "00000000 00000000", "00000000 00000000",
    "00000000 00000000", "00000000 00000000", "00000000 00000000", "10001000 20110000", "10000000 30111000",
]


def test_conv_queries_are_pinned():
    """dvd_conv_wants_fragment_major / dvd_conv_pool2_ok over the forward and the backward-data geometry of every case of
    tests/test_gpu_conv.py::CASES (bf16) x nsplit {1, 2} x pool2 {0, 1}: both read the forward planner's plan (cv_plan, made
    "geometry only"), so a change of a family rule shows here without a GPU.  The values were generated on the CPU from the library
    of the commit before the planner was split into steps, with this loop.  Queries only, nothing is launched.
    (The refusals of dvd_conv_forward_group: test_group_refusals_are_pinned.)"""
    from dvd_gan_amd import lib as L
    from test_gpu_conv import CASES
    lib = L.lib()
    pad8 = lambda c: (c + 7) // 8 * 8
    assert len(CONV_QUERY_PINS) == len(CASES)
    bad = []
    for case, want in zip(CASES, CONV_QUERY_PINS):
        F_, Cin, Cout, sp, ks, up2, relu = case
        H, W = (v * (2 if up2 else 1) for v in sp[-2:])
        got = []
        for cin, cout, u, r in ((pad8(Cin), Cout, up2, relu), (pad8(Cout), pad8(Cin), False, False)):
            s = ""
            for ns in (1, 2):
                for p2 in (0, 1):
                    d = L.ConvDesc()
                    d.dtype, d.frames, d.T, d.H, d.W = L.BF16, F_, sp[0] if len(sp) == 3 else 1, H, W
                    d.C, d.ldi, d.Cout, d.ldo = cin, cin, cout, pad8(cout)
                    d.kt, d.kh, d.kw = ks if len(ks) == 3 else (1,) + tuple(ks)
                    d.up2, d.relu_in, d.nsplit, d.pool2 = int(u), int(r), ns, p2
                    d.inp = d.w = d.out = 1               # never dereferenced by the queries
                    if ns > 1:
                        d.ws = 1                          # (split-K writes slabs)
                    s += "%d%d" % (lib.dvd_conv_wants_fragment_major(ctypes.byref(d)), lib.dvd_conv_pool2_ok(ctypes.byref(d)))
            got.append(s)
        if " ".join(got) != want:
            bad.append((case, " ".join(got), want))
    assert not bad, bad


GROUP_REFUSALS = dict(
    [("n=0", -1), ("n=7", -1), ("kind=-1", -1), ("kind=5", -1)]
    + [("side=%d,kind=%d" % (s, k), -2) for s, fits in ((16, (0, 1)), (8, (2, 3)), (4, (4,))) for k in range(5) if k not in fits]
    + [("side=%d,%s" % (s, f), -1) for s in (16, 8, 4) for f in ("relu_in", "up2", "ws")])


def test_group_refusals_are_pinned(tmp_path):
    """The refusals of dvd_conv_forward_group that return before any launch, with their codes (DVD_E_ARG = -1, DVD_E_SHAPE = -2): n
    and kind out of range, a member whose geometry does not fit `kind` (every frame side under every kind of kGroupKind it does not
    belong to), a member with relu_in, up2 or ws.  The entry point is hidden from the shared library's exports, so
    tests/native/group_refusals.cpp is linked against the object files build.sh left (static linking ignores visibility) and run: no
    GPU is touched.  The codes are those of the same program linked against the objects of the commit before the group kinds became
    a table."""
    import glob
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "dvd_gan_amd", "csrc")
    objs = sorted(glob.glob(os.path.join(csrc, "build", "*.o")))
    if not objs or not shutil.which("hipcc"):
        pytest.skip("no build/*.o or no hipcc: the library was not built by csrc/build.sh in this tree")
    main_o, prog = str(tmp_path / "main.o"), str(tmp_path / "group_refusals")
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-I", csrc, "-c",
                           os.path.join(ROOT, "tests", "native", "group_refusals.cpp"), "-o", main_o])
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-o", prog, main_o] + objs)
    out = subprocess.check_output([prog]).decode()
    got = {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}
    assert got == GROUP_REFUSALS


def test_stack_schedule_is_pinned(tmp_path):
    """The wavefront schedule of a ConvGRU stack (gru.hip: record_forward / record_backward) as the library records it before it
    launches anything: every launch in issue order -- the elementwise gate kernels (kernel, hidden, step) and the grouped launches
    (pass, kind, per member C, ldi, Cout, filter size, epilogue mode after the mode-6 rewrite, bias / res set, split-K factor and
    slab offset in floats) -- plus the slab floats and the largest group of the pass.  tests/native/stack_schedule.cpp lists the
    stacks: the generator's four ConvGRUs at B = 64, supplied initial states, B = 16, the per-layer policy with a split-K cap,
    T = 1 and 2, one layer, and a four-layer stack with six-member groups (the coordinate-descent split-K search).  The program is
    linked against the object files build.sh left, as in test_group_refusals_are_pinned; no GPU is touched.  The expected text was
    printed by the commit before the schedule became a recorded value (profiles/gru_schedule_refactor_numbers.md says how)."""
    import glob
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "dvd_gan_amd", "csrc")
    objs = sorted(glob.glob(os.path.join(csrc, "build", "*.o")))
    if not objs or not shutil.which("hipcc"):
        pytest.skip("no build/*.o or no hipcc: the library was not built by csrc/build.sh in this tree")
    main_o, prog = str(tmp_path / "main.o"), str(tmp_path / "stack_schedule")
    subprocess.check_call(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-I", csrc, "-c",
                           os.path.join(ROOT, "tests", "native", "stack_schedule.cpp"), "-o", main_o])
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-o", prog, main_o] + objs)
    got = subprocess.check_output([prog]).decode().splitlines()
    want = open(os.path.join(ROOT, "tests", "native", "stack_schedule.txt")).read().splitlines()
    assert len(want) > 500 and sum(l.startswith("==") for l in want) == 26
    bad = [(i + 1, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad and len(got) == len(want), (len(got), len(want), bad[:3])


def test_attention_refusal_rules_need_no_gpu():
    """The shapes the attention entry points refuse before any launch (DVD_E_SHAPE): the MFMA kernels past 4096 tokens, the
    separable cell past an attended size of 64, the fp32 kernels' LDS limits -- forward [QB][Nk] scores + queries + partial
    outputs, backward [QB][Nk + C].  The fp32 backward walks the query axis in chunks, so N itself has no limit there (the
    generator's 3-D attention at 128 x 128 has N = 3072: tests/test_gpu_attention.py runs it).  Every call below is refused by
    its host-side checks; the placeholder pointers are never dereferenced and nothing is launched."""
    from dvd_gan_amd import lib as L
    lib = L.lib()
    p = ctypes.c_void_p(1)
    one = 1
    assert lib.dvd_attention_mfma_ok(L.BF16, 160, 16, 16, 32, 128, 128, 4128) == 0
    assert lib.dvd_attention_mfma_forward(p, 160, p, 128, p, p, p, p, one, 4128, None) == -2
    assert lib.dvd_attention_mfma_backward(p, 160, p, 128, p, p, p, p, p, p, one, 4128, None) == -2
    # sepattn: A = W = 66 > 64 (the 64 x 32 product tiles)
    assert lib.dvd_sepattn_work_floats(8, 66, 8, 1, 64, 32) == 0 and lib.dvd_sepattn_work_floats(8, 64, 8, 1, 64, 32) > 0
    assert lib.dvd_sepattn_forward(L.BF16, p, 128, 32, 32, 64, p, 64, 64, p, p, p, p, p, p, p, p, one, 8, 66, 8, 1, None) == -2
    assert lib.dvd_sepattn_backward(L.BF16, p, 64, 64, 32, p, p, p, p, p, p, p, p, p, p, p, p, p, 128, 32, 64, p, one,
                                    8, 8, 66, 2, None) == -2
    # fp32 forward at dq = 8, C = 64: 8 N + 8 dqp + 32 C floats of LDS -> N = 1784 is the largest (the GPU suite runs it)
    assert lib.dvd_attention_forward(L.F32, p, 80, 8, 8, 16, p, 64, 64, p, p, p, p, one, 1785, None) == -2
    # fp32 backward: [8][Nk + C] floats past 64 KB (Nk = 1800, C = 256); the forward of the same call is refused as well
    assert lib.dvd_attention_kv_backward(L.F32, p, 8, 8, p, 512, 8, 16, p, 256, 256, p, p, p, p, p, p, p, one, 64, 1800,
                                         None) == -2
    assert lib.dvd_attention_backward(L.BF16, p, 2072, 8, 8, 16, p, 2056, 2056, p, p, p, p, p, p, one, 8, None) == -2


def test_missing_library_fails_loudly(monkeypatch):
    from dvd_gan_amd import lib as L
    monkeypatch.delitem(L._handles, "core", raising=False)
    monkeypatch.setenv("DVD_LIB_PATH", "/nonexistent/libdvdgan_hip.so")
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        L.lib()


def test_state_dict_layout_matches_reference(golden):
    """Key names and shapes of the three networks == the reference's (golden sd0 of F9)."""
    from conftest import sub
    from dvd_gan_amd.gen_net import Generator
    from dvd_gan_amd.disc_nets import SpatialDiscriminator, TemporalDiscriminator
    g = golden("f9_trainer_hinge")
    nets = {"G": Generator(16, 4, 3, 2, 8), "Ds": SpatialDiscriminator(2, 3), "Dt": TemporalDiscriminator(2, 3)}
    for tag, net in nets.items():
        want = sub(g, tag + ".sd0")
        have = net.state_dict()
        assert set(have) == set(want), (tag, set(have) ^ set(want))
        for k, v in want.items():
            assert tuple(have[k].shape) == tuple(v.shape), (tag, k)
        # u / v are parameters that do not train (Normalization.py:49-50)
        for k, p in net.named_parameters():
            assert p.requires_grad == (not k.endswith(("weight_u", "weight_v"))), k


def test_condition_index_table_reproduces_quirk1():
    """samp[t*B+b] must be the row the reference's condition.repeat(T,1) gives frame b*T+t."""
    B, T = 3, 4
    t_idx = torch.arange(T).view(T, 1)
    b_idx = torch.arange(B).view(1, B)
    samp = ((b_idx * T + t_idx) % B).reshape(-1)
    cond_rows = torch.arange(B).repeat(T)           # condition.repeat(T,1): row i holds sample i % B
    for t in range(T):
        for b in range(B):
            assert int(samp[t * B + b]) == int(cond_rows[b * T + t])


def test_convgru_stack_queries_need_no_gpu():
    """dvd_convgru_stack_ok / dvd_convgru_stack_ws_floats (layer wavefront over a ConvGRU, Module/ConvGRU.py:57-133) are pure host
    logic: which stacks the grouped-launch path serves, and how much split-K slab space its schedule needs."""
    import ctypes as C
    from dvd_gan_amd import lib as L
    lib = L.lib()

    def stack(S, hids, ks, dtype=L.BF16, B=64, T=48, cin0=256, layer_policy=0, ns_cap=0):
        sd = L.GruStackDesc()
        sd.n_layers, sd.layer_policy = len(hids), layer_policy
        for l, (h, k) in enumerate(zip(hids, ks)):
            d = sd.layer[l]
            d.dtype, d.T, d.B, d.H, d.W, d.hidden, d.k = dtype, T, B, S, S, h, k
            d.gx_stride, d.ns_cap = B * S * S * 3 * h, ns_cap
            for f in ("gx", "w_ur", "w_o", "w_ur_q", "w_o_q", "wd_ur", "wd_o", "wd_ur_q", "wd_o_q", "h_all", "u_all", "r_all", "o_all",
                      "hr_all", "tickets", "dg", "carry"):
                setattr(d, f, 1)                     # never dereferenced by the queries
            if l:
                sd.cin[l] = hids[l - 1]
                sd.wx[l] = sd.wx_q[l] = sd.bx[l] = sd.wdx[l] = sd.wdx_q[l] = sd.dh_mid[l] = 1
        sd.ws = 1
        return sd

    ok = lambda sd, bwd=0: lib.dvd_convgru_stack_ok(C.byref(sd), bwd)
    g3 = stack(32, [128, 256, 128], [3, 5, 5])
    assert ok(g3) == 1 and ok(g3, 1) == 1
    assert ok(stack(4, [256, 512, 256], [3, 5, 3])) == 1 and ok(stack(8, [256, 512, 256], [3, 5, 3])) == 1
    assert ok(stack(12, [256, 512, 256], [3, 5, 3])) == 0          # not a power of two
    assert ok(stack(32, [128, 256, 128], [3, 7, 5])) == 0          # 7 x 7 taps
    assert ok(stack(32, [128, 256, 128], [3, 5, 5], dtype=L.F32)) == 0
    bad = stack(32, [128, 256, 128], [3, 5, 5])
    bad.wx_q[1] = None
    assert ok(bad) == 0 and ok(bad, 1) == 1                        # the forward pass needs the x-part image, the backward pass does not
    assert lib.dvd_convgru_stack_ws_floats(C.byref(g3)) >= 1       # one-round groups at 32 x 32: nothing is split
    small = lib.dvd_convgru_stack_ws_floats(C.byref(stack(4, [256, 512, 256], [3, 5, 3])))
    assert small > 16384 and small % 16384 == 0                    # 4 x 4 frames: split-K slabs of whole 128 x 128 tiles
    # the sizing query walks exactly the schedule of the launch: repeatable, and a supplied initial state (more members in the
    # pipeline-fill groups) changes the plan without ever yielding less than one float
    for S in (4, 8, 16):
        sd = stack(S, [256, 512, 256], [3, 5, 3])
        a = lib.dvd_convgru_stack_ws_floats(C.byref(sd))
        assert a == lib.dvd_convgru_stack_ws_floats(C.byref(sd)) and a >= 1
        for l in range(3):
            sd.layer[l].h0 = 1
        b = lib.dvd_convgru_stack_ws_floats(C.byref(sd))
        assert b >= 1 and b % 16384 == 0
    assert lib.dvd_convgru_stack_forward(C.byref(stack(12, [256], [3])), None) == -2
    # a stack is served only if no grouped launch of its recorded schedule needs more than six members (kGroupMax, the limit of
    # dvd_conv_forward_group: test_group_refusals_are_pinned).  Four layers in steady state on 16-pixel frames: 4 gate + 3 x-part
    # members in the O group -> refused by every query instead of from the middle of the launch's time loop; at T = 2 the pipeline
    # never fills; on 8 x 8 frames one x-part rides in the other group of a pair (5 and 6 members)
    wsf = lambda sd: lib.dvd_convgru_stack_ws_floats(C.byref(sd))
    four = stack(16, [64, 64, 64, 64], [3, 3, 3, 3])
    assert ok(four) == 0 and ok(four, 1) == 0 and wsf(four) == 0
    assert lib.dvd_convgru_stack_forward(C.byref(four), None) == -2 and lib.dvd_convgru_stack_backward(C.byref(four), None) == -2
    short = stack(16, [64, 64, 64, 64], [3, 3, 3, 3], T=2)
    assert ok(short) == 1 and ok(short, 1) == 1 and wsf(short) >= 1
    four8 = stack(8, [256, 512, 256, 256], [3, 5, 3, 3])
    assert ok(four8) == 1 and ok(four8, 1) == 1
    # slab space of the benchmark's schedules (B = 64, T = 48, no h0, production policy unless stated): the answers of the library
    # before the schedule became a recorded value
    g, k = [256, 512, 256], [3, 5, 3]
    assert wsf(stack(4, g, k)) == 7340032
    assert wsf(stack(8, g, k)) == 14680064
    assert wsf(stack(16, g, k)) == 12582912
    assert wsf(stack(32, [128, 256, 128], [3, 5, 5])) == 16777216
    assert wsf(four8) == 14680064
    assert wsf(stack(4, g, k, layer_policy=1)) == 16777216
    assert wsf(stack(4, g, k, ns_cap=2)) == 5767168


def test_hot_kernels_use_no_scratch_memory():
    """hipcc's own resource report of every kernel (dvd_gan_amd/csrc/build.sh keeps it as build/<file>.res): the convolution, weight-
    gradient, ConvGRU and attention kernels must keep their accumulators in registers -- no scratch, no spilled vector registers.
    (Round 6: a runtime-indexed accumulator array in a new epilogue branch put EVERY convolution kernel's accumulators into scratch;
    parity stayed green, the step ran 3x slower.)  Known exception: a few scalar-register spills in rarely used 5-tap ReLU variants."""
    import glob
    build = os.path.join(ROOT, "dvd_gan_amd", "csrc", "build")
    files = sorted(glob.glob(os.path.join(build, "*.res")))
    if not files:
        pytest.skip("no build/*.res: the library was not built by csrc/build.sh in this tree")
    hot = ("conv_halo", "conv_group", "conv_igemm", "conv_wgrad", "conv_thin", "wgrad_thin", "attn_", "gru_", "cbn_", "bn_stats")
    seen, bad = 0, []
    for path in files:
        name, rec = None, {}
        for line in open(path):
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                name, rec = m.group(1), {}
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
            if m and name:
                rec[m.group(1).strip()] = int(m.group(2))
                if m.group(1).strip() == "VGPRs Spill" and any(h in name for h in hot):
                    seen += 1
                    if rec.get("ScratchSize", 0) != 0 and rec.get("SGPRs Spill", 0) == 0 or rec["VGPRs Spill"] != 0:
                        bad.append((os.path.basename(path), name, rec))
    assert seen >= 100, seen
    assert not bad, bad[:5]

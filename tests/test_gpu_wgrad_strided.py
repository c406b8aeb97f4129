"""The weight-gradient kernels (conv_wgrad.hip) on the requests the model's heaviest callers send: a column window of a wider dy
(`dy_col`, `ldy > Cy`), a channel window of a wider, already filled dw master (`dw_ci_off`, `s_co`), row slices that begin and end
inside live tensors (`frames`, `x_row0`, `dy_row0`) -- functional._gru_gate_wgrads and the attention projections of disc_nets.py.
tests/test_gpu_conv.py covers the same kernels on dense requests only.

Every request goes through kern.conv_wgrad.  Whatever lies outside the window -- the other columns of dy, the frames of x and dy
before and after the slice -- is LOUD POISON: finite random values 2^10 times the data's scale (finite, not NaN: a kernel may load
a neighbour and multiply it by a masked zero).  The checks, against tests/conv_ref.py (fp64 on the STORED operands):

  a  every element of the dw master outside [dw_ci_off, dw_ci_off + Cin) and of the bias buffer outside its window keeps its
     prefill bit for bit;
  b  dw[window] - prefill and dbias - prefill against the reference: rel-L2 < 5e-6 (automatic split), < 1e-5 (forced msplit 1 / 2),
     dbias < 5e-6 -- the bounds tests/test_gpu_conv.py holds for the same sums;
  c  stride invariance: from a zero prefill, the strided result equals a dense call (ldy == Cy, dense dw, whole tensors) on
     compacted copies of the same data at the same msplit, torch.equal.  Neither the tile choice nor the split looks at a stride
     (except the 32-bit offset cap, tested on its own below), and dw comes out of one atomic per element or of the fixed-order
     reduce kernels.  dbias too is bit-equal in EVERY case here: with a slice workspace it comes out of the fixed-order bias reduce
     kernels, and on a single-slice launch exactly one workgroup per out-channel tile (centre tap / centre filter row, first
     in-channel tile: `do_bias` in the three kernels) adds its column sums, one atomic per channel -- no case of this file has
     several workgroups' atomics meet in one dbias element, so none takes the 5e-6 tolerance instead;
  d  the kernel family the wgrad profile hook reports (dvd_prof_report_variants, kind 1: 1 = 8-wave filter row, 2 = one tap,
     4 = one wave per SIMD) is the one the case was written for.
"""
import ctypes as C

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROW, TAP, ROW4 = 1, 2, 4
POISON = 1024.0
DY_SCALE = 0.25
BF, F32 = torch.bfloat16, torch.float32


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def pad8(c):
    return (c + 7) // 8 * 8


def profiled(fn):
    """Runs fn with the launch records on -> {family: launches} of the weight-gradient launches it made (drains the records as
    tests/test_gpu_gru.py::_drain does)."""
    from dvd_gan_amd import lib as L
    lib = L.lib()
    lib.dvd_prof_report_variants.restype = C.c_longlong
    lib.dvd_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.dvd_prof_enable(0)
    n = (C.c_longlong * 6)()
    total = lib.dvd_prof_report_variants(1, 6, n, None, None)
    seen = {v: int(n[v]) for v in range(1, 6) if n[v] > 0}
    assert sum(seen.values()) == total
    return seen


class Request:
    """One strided request and the compacted copies of what it selects.  x lives in [x_pre + frames + post, *sp, Cp], dy in
    [dy_pre + frames + post, *osp, ld]; the window is frames [pre, pre + frames) and columns [dy_col, dy_col + Cy), whose pad columns
    [Cout, Cy) are zero as the ABI promises.  dw is a master [Cout][ci_tot][*k] written at [ci_off, ci_off + Cin)."""

    def __init__(self, dtype, frames, cin, cout, sp, ks, *, dy_col, ld, up2=False, seed=0, x_pre=1, dy_pre=2, post=1, ci_off=5,
                 ci_extra=3, fill_dy=None):
        g = torch.Generator(device=DEV).manual_seed(seed)
        rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
        self.dtype, self.frames, self.cin, self.cout, self.sp, self.ks, self.up2 = dtype, frames, cin, cout, tuple(sp), tuple(ks), up2
        self.cp, self.cy = pad8(cin), min(pad8(cout), ld - dy_col)
        self.ld, self.dy_col, self.x_pre, self.dy_pre = ld, dy_col, x_pre, dy_pre
        self.ci_off, self.ci_tot = ci_off, ci_off + cin + ci_extra
        osp = tuple(sp[:-2]) + tuple(v * (2 if up2 else 1) for v in sp[-2:])
        assert ld % 8 == 0 and dy_col + self.cy <= ld and self.cy >= cout
        xs = rn(frames, *sp, self.cp)
        xs[..., cin:] = 0
        dys = rn(frames, *osp, self.cy) * DY_SCALE
        dys[..., cout:] = 0
        xbuf = rn(x_pre + frames + post, *sp, self.cp) * POISON
        xbuf[x_pre:x_pre + frames] = xs
        self.xbuf = xbuf.to(dtype)
        if fill_dy is not None:          # a very wide dy: poison drawn in place, in the storage type
            dybuf = fill_dy((dy_pre + frames + post,) + osp + (ld,))
        else:
            dybuf = (rn(dy_pre + frames + post, *osp, ld) * (POISON * DY_SCALE)).to(dtype)
        dybuf[dy_pre:dy_pre + frames, ..., dy_col:dy_col + self.cy] = dys.to(dtype)
        self.dybuf = dybuf
        # what the request selects, as stored
        self.xs = self.xbuf[x_pre:x_pre + frames].contiguous()
        self.dys = self.dybuf[dy_pre:dy_pre + frames, ..., dy_col:dy_col + self.cy].contiguous()
        self.dw_ref, self.db_ref = R.wgrad_ref(self.xs[..., :cin], self.dys[..., :cout], ks, up2=up2)
        # prefills of the gradient's own magnitude; the bias gradient is window 1 of a [3 * Cout] buffer
        self.dw_pre = rn(cout, self.ci_tot, *ks) * float(self.dw_ref.std())
        self.db_pre = rn(3 * cout) * float(self.db_ref.std())
        self.db_win = slice(cout, 2 * cout)

    def strided(self, dw, msplit, dbias, **kw):
        from dvd_gan_amd import kern as K
        return K.conv_wgrad(self.xbuf, self.dybuf, dw, self.ks, self.cout, self.cin, up2=self.up2, msplit=msplit, dy_col=self.dy_col,
                            dw_ci_off=self.ci_off, dw_ci_tot=self.ci_tot, frames=self.frames, x_row0=self.x_pre,
                            dy_row0=self.dy_pre, dbias=dbias, **kw)

    def dense(self, dw, msplit, dbias):
        from dvd_gan_amd import kern as K
        return K.conv_wgrad(self.xs, self.dys, dw, self.ks, self.cout, self.cin, up2=self.up2, msplit=msplit, dbias=dbias)

    def window(self, dw):
        return dw[:, self.ci_off:self.ci_off + self.cin]

    def check_untouched(self, dw, db):
        assert torch.equal(dw[:, :self.ci_off], self.dw_pre[:, :self.ci_off])
        assert torch.equal(dw[:, self.ci_off + self.cin:], self.dw_pre[:, self.ci_off + self.cin:])
        if db is not None:
            keep = torch.ones(db.numel(), dtype=torch.bool, device=DEV)
            keep[self.db_win] = False
            assert torch.equal(db[keep], self.db_pre[keep])


# ------------------------------------------------------------------------------------------------ single launches
# frames, Cin, Cout, spatial (of x), k, up2, dtypes, family with the automatic split, family with a forced split (bf16; fp32 = one tap)
SINGLE = {
    1: (6, 16, 24, (8, 8), (3, 3), False, (BF, F32), ROW, ROW),            # 64-channel filter-row tile; fp32: one tap
    2: (3, 40, 72, (16, 16), (3, 3), False, (BF,), ROW, ROW),             # 128 x 64, ragged both ways
    3: (4, 72, 136, (16, 16), (5, 5), False, (BF,), ROW, ROW4),           # 256 x 64; forced: one wave per SIMD 256 x 64
    4: (2, 128, 128, (32, 32), (3, 3), False, (BF,), ROW, ROW4),          # forced: 128 x 128, W = 32 lines
    5: (4, 128, 256, (16, 16), (3, 3), False, (BF,), ROW, ROW4),          # forced: 256 x 128, one staging set with dbias, two without
    6: (4, 128, 120, (8, 16), (5, 5), False, (BF,), ROW, ROW4),           # 128 x 128 five-tap tile, H != W, two lines per step
    7: (12, 40, 72, (4, 4), (3, 3), False, (BF,), ROW, ROW),              # 4 x 4 frames, even count: a step is two whole frames
    8: (3, 40, 72, (4, 4), (3, 3), False, (BF,), TAP, TAP),               # 4 x 4 frames, odd count: one tap
    9: (5, 24, 200, (6, 6), (3, 3), False, (BF,), TAP, TAP),              # not a power of two: one tap, 256-wide tile
    10: (2, 16, 40, (3, 8, 8), (3, 3, 3), False, (BF,), ROW, ROW),        # 3-D taps
    # x2-upsampled input (x on 32 x 32, dy on 64 x 64).  A forced split takes the folded one-wave-per-SIMD form (a workspace is
    # always supplied); the AUTOMATIC split does not at this size -- wg_choose_tile wants WG_ROW4_MIN_WGS workgroups of 4096 rows
    # unless msplit is forced, so the fold is refused and the direct x2 filter-row tile (64 channels) serves the request
    12: (4, 128, 64, (32, 32), (3, 3), True, (BF,), ROW, ROW4),
}
SINGLE_PARAMS = [(n, dt, col) for n, c in SINGLE.items() for dt in c[6] for col in (1, 2)]
_requests = {}


def single_request(n, dtype, col):
    key = (n, dtype, col)
    if key not in _requests:
        frames, cin, cout, sp, ks, up2 = SINGLE[n][:6]
        _requests[key] = Request(dtype, frames, cin, cout, sp, ks, dy_col=col * cout, ld=3 * cout, up2=up2, seed=1000 * n + col)
    return _requests[key]


def expected_family(n, dtype, msplit):
    return TAP if dtype == F32 else SINGLE[n][7 if msplit == 0 else 8]


def run_checks(r, msplit, with_bias, family, note=""):
    """Checks a-d of one request; every figure is formed and printed before the first assertion."""
    tol = 5e-6 if msplit == 0 else 1e-5
    dw = r.dw_pre.clone()
    db = r.db_pre.clone() if with_bias else None
    seen = profiled(lambda: r.strided(dw, msplit, db[r.db_win] if with_bias else None))
    e_dw = rel(r.window(dw).double() - r.window(r.dw_pre).double(), r.dw_ref)
    e_db = rel(db[r.db_win].double() - r.db_pre[r.db_win].double(), r.db_ref) if with_bias else 0.0
    # c: zero prefill against the dense call on the compacted copies
    dwz, dwd = torch.zeros_like(r.dw_pre), torch.zeros(r.cout, r.cin, *r.ks, device=DEV)
    dbz, dbd = (torch.zeros(3 * r.cout, device=DEV), torch.zeros(r.cout, device=DEV)) if with_bias else (None, None)
    r.strided(dwz, msplit, dbz[r.db_win] if with_bias else None)
    r.dense(dwd, msplit, dbd)
    same_dw = torch.equal(r.window(dwz), dwd)
    same_db = torch.equal(dbz[r.db_win], dbd) if with_bias else True
    print(f"wgrad {note} msplit={msplit} dbias={with_bias}: family {seen}, dw {e_dw:.2e}, dbias {e_db:.2e}, "
          f"equal to the dense call: dw {same_dw}, dbias {same_db}")
    assert seen == {family: 1}, (seen, family)                   # d
    r.check_untouched(dw, db)                                    # a
    assert e_dw < tol and e_db < 5e-6                            # b
    assert same_dw and same_db                                   # c
    assert not bool(dwz[:, :r.ci_off].any()) and not bool(dwz[:, r.ci_off + r.cin:].any())      # (nothing outside the window either)
    if with_bias:
        keep = torch.ones(3 * r.cout, dtype=torch.bool, device=DEV)
        keep[r.db_win] = False
        assert not bool(dbz[keep].any())


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("msplit", [0, 1, 2])
@pytest.mark.parametrize("n,dtype,col", SINGLE_PARAMS)
def test_single_launch_on_a_column_window_and_a_row_slice(n, dtype, col, msplit, with_bias):
    """The smallest shapes that reach each family, tile and line geometry; ld = 3 * Cout, the window at column Cout and 2 * Cout."""
    r = single_request(n, dtype, col)
    run_checks(r, msplit, with_bias, expected_family(n, dtype, msplit), note=f"case {n} {dtype} col {col}")


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("msplit", [0, 1, 2])
def test_attention_projection_request(msplit, with_bias):
    """Case 11, the q | k | v request of disc_nets.py: one dqkv [M][16 + 16 + 96], three 1 x 1 launches with Cout = 12, 12, 96 at
    dy_col = 0, 16, 32 (Cout % 8 != 0: zero pad columns inside the window), the bias gradients windows of ONE buffer at the same
    offsets (128 floats, as the caller allocates it: its elements [12, 16) and [28, 32) belong to no window)."""
    from dvd_gan_amd import kern as K
    frames, cin, S = 3, 96, 16
    parts = ((0, 12), (16, 12), (32, 96))
    g = torch.Generator(device=DEV).manual_seed(11)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    xbuf = rn(1 + frames + 1, S, S, cin) * POISON
    xbuf[1:1 + frames] = rn(frames, S, S, cin)
    xbuf = xbuf.to(BF)
    dq = rn(2 + frames + 1, S, S, 128) * (POISON * DY_SCALE)
    dq[2:2 + frames] = rn(frames, S, S, 128) * DY_SCALE
    dq[2:2 + frames, ..., 12:16] = 0
    dq[2:2 + frames, ..., 28:32] = 0
    dq = dq.to(BF)
    xs, dys = xbuf[1:1 + frames].contiguous(), dq[2:2 + frames].contiguous()
    tol = 5e-6 if msplit == 0 else 1e-5
    db_pre = rn(128)
    db, dbz = db_pre.clone(), torch.zeros(128, device=DEV)
    touched = torch.zeros(128, dtype=torch.bool, device=DEV)
    for off, n in parts:
        dw_ref, db_ref = R.wgrad_ref(xs, dys[..., off:off + n], (1, 1))
        pre = rn(n, 5 + cin + 3, 1, 1) * float(dw_ref.std())
        dw = pre.clone()
        seen = profiled(lambda: K.conv_wgrad(xbuf, dq, dw, (1, 1), n, cin, msplit=msplit, dy_col=off, dw_ci_off=5, dw_ci_tot=5 + cin + 3,
                                             frames=frames, x_row0=1, dy_row0=2, dbias=db[off:off + n] if with_bias else None))
        e_dw = rel(dw[:, 5:5 + cin].double() - pre[:, 5:5 + cin].double(), dw_ref)
        e_db = rel(db[off:off + n].double() - db_pre[off:off + n].double(), db_ref) if with_bias else 0.0
        print(f"wgrad case 11 col {off} msplit={msplit} dbias={with_bias}: family {seen}, dw {e_dw:.2e}, dbias {e_db:.2e}")
        assert seen == {TAP: 1}
        assert torch.equal(dw[:, :5], pre[:, :5]) and torch.equal(dw[:, 5 + cin:], pre[:, 5 + cin:])
        assert e_dw < tol and e_db < 5e-6
        touched[off:off + n] = True
        # stride invariance against the dense call: dy compacted to its Cy = pad8(n) columns
        dwz, dwd, dbd = torch.zeros_like(pre), torch.zeros(n, cin, 1, 1, device=DEV), torch.zeros(n, device=DEV)
        K.conv_wgrad(xbuf, dq, dwz, (1, 1), n, cin, msplit=msplit, dy_col=off, dw_ci_off=5, dw_ci_tot=5 + cin + 3, frames=frames,
                     x_row0=1, dy_row0=2, dbias=dbz[off:off + n] if with_bias else None)
        K.conv_wgrad(xs, dys[..., off:off + pad8(n)].contiguous(), dwd, (1, 1), n, cin, msplit=msplit, dbias=dbd if with_bias else None)
        assert torch.equal(dwz[:, 5:5 + cin], dwd)
        if with_bias:
            assert torch.equal(dbz[off:off + n], dbd)
    if with_bias:
        assert torch.equal(db[~touched], db_pre[~touched]) and float(dbz[~touched].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ ConvGRU gate composition
# T, B, S, cin, hid, k, dtypes, {family: launches} with a supplied h0 / without (bf16; fp32: all one tap)
GRU = [
    (3, 2, 8, 16, 24, 3, (BF, F32), {ROW: 9}, {ROW: 6}),
    # 4 x 4 frames: the x-part (9 frames) and the h0-part (3 frames) have odd frame counts and take the one-tap kernel, the h-part
    # (6 frames) the filter-row kernel -- two families add into one master window
    (3, 3, 4, 40, 72, 3, (BF,), {TAP: 6, ROW: 3}, {TAP: 3, ROW: 3}),
    (2, 2, 4, 256, 256, 3, (BF,), {ROW: 9}, {ROW: 6}),            # a configs[1] layer at its smallest frame
    (2, 2, 8, 256, 512, 5, (BF,), {ROW: 9}, {ROW: 6}),            # the wide middle layer, ldy = 1536
    (2, 1, 32, 128, 256, 5, (BF,), {ROW: 9}, {ROW: 6}),           # the 32-pixel stage
]
GRU_PARAMS = [(i, dt, h0, False) for i, c in enumerate(GRU) for dt in c[6] for h0 in (True, False)] + [(0, BF, True, True), (0, F32, False, True)]


@pytest.mark.parametrize("case,dtype,with_h0,shared_x", GRU_PARAMS)
def test_convgru_gate_composition(case, dtype, with_h0, shared_x):
    """The launch sequence of functional._gru_gate_wgrads: per gate the x-part with dbias, the h0-part on `frames = B`, the h-part on
    `frames = (T-1) B` with row offsets (x_row0 = 0 for update / reset, B for the out gate on h * r), all into prefilled masters
    [hid][cin + hid][k][k] and windows of one prefilled [3 hid] bias buffer; against the fp64 composition of tests/conv_ref.py.
    The other gates' columns and the other steps' frames are live data of the data's own scale here, as in the model.
    shared_x: x has B frames and the x-part reads the (stored) sum of dg over T."""
    from dvd_gan_amd import kern as K
    T, B, S, cin, hid, k = GRU[case][:6]
    g = torch.Generator(device=DEV).manual_seed(77 + case)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    x = rn(B if shared_x else T * B, S, S, cin).to(dtype)
    dg = (rn(T * B, S, S, 3 * hid) * DY_SCALE).to(dtype)
    dgx = dg.view(T, B, S, S, 3 * hid).float().sum(0).to(dtype) if shared_x else dg
    h_all, hr_all = rn(T * B, S, S, hid).to(dtype), rn(T * B, S, S, hid).to(dtype)
    h0 = rn(B, S, S, hid).to(dtype) if with_h0 else None
    ref = R.gru_gate_wgrad_ref(x, dgx, dg, h_all, hr_all, h0, T, B, hid, k)
    ctot = cin + hid
    pres = [rn(hid, ctot, k, k) * float(ref[gate][0].std()) for gate in range(3)]
    db_pre = rn(3 * hid) * float(ref[0][1].std())
    dws, db3 = [p.clone() for p in pres], db_pre.clone()

    def launches():
        for gate in range(3):
            dw = dws[gate]
            K.conv_wgrad(x, dgx, dw, (k, k), hid, cin, dy_col=gate * hid, dw_ci_off=0, dw_ci_tot=ctot, dbias=db3[gate * hid:(gate + 1) * hid])
            if h0 is not None:
                K.conv_wgrad(h0 if gate < 2 else hr_all, dg, dw, (k, k), hid, hid, dy_col=gate * hid, dw_ci_off=cin, dw_ci_tot=ctot,
                             frames=B, x_row0=0, dy_row0=0)
            if T > 1:
                K.conv_wgrad(h_all if gate < 2 else hr_all, dg, dw, (k, k), hid, hid, dy_col=gate * hid, dw_ci_off=cin, dw_ci_tot=ctot,
                             frames=(T - 1) * B, x_row0=0 if gate < 2 else B, dy_row0=B)

    seen = profiled(launches)
    want = {TAP: 9 if with_h0 else 6} if dtype == F32 else GRU[case][7 if with_h0 else 8]
    if shared_x and dtype == BF:
        want = {ROW: 9}                                   # (case 0: B = 2 frames of 8 x 8 for the x-part, still the filter-row kernel)
    errs = []
    for gate in range(3):
        e_dw = rel(dws[gate].double() - pres[gate].double(), ref[gate][0])
        win = slice(gate * hid, (gate + 1) * hid)
        e_db = rel(db3[win].double() - db_pre[win].double(), ref[gate][1])
        errs.append((e_dw, e_db))
    print(f"gru wgrad case {GRU[case][:6]} {dtype} h0={with_h0} shared_x={shared_x}: families {seen}, (dw, dbias) per gate "
          + ", ".join(f"({a:.2e}, {b:.2e})" for a, b in errs))
    assert seen == want, (seen, want)
    for e_dw, e_db in errs:
        assert e_dw < 5e-6 and e_db < 5e-6


# ------------------------------------------------------------------------------------------------ the 32-bit offset cap
@pytest.mark.parametrize("dtype,ld,family", [(BF, 65536, ROW4), (F32, 32768, TAP)])
def test_offset_cap_reslices_a_forced_single_slice(dtype, ld, family):
    """wg_choose_split, correction 3: a slice spans at most 2^31 bytes of dy whatever msplit the caller forces.  18 frames of
    32 x 32 = 18432 rows behind a row stride of 131072 bytes: 2^31 / 131072 = 16384 rows per slice, so the forced msplit = 1 becomes
    two slices (16384 + 2048 rows) through the workspace.  The dy buffer is 2.4 GB of poison around a 128-column window.

    Offsets, on paper, for the kernels the two cases take.  Both kernels address dy through a buffer resource whose base is
    dy + dy_col * esz + m_begin * ldy * esz (64-bit arithmetic: conv_wgrad.hip, `ybase_b`) and whose size is what is left of
    dy_bytes = ((M - 1) * ldy + Cy) * esz from there, clamped to 2^32 - 2; loads past it return zeros in hardware.  The 32-bit
    offset is (row - m_begin) * ldy * esz + channel bytes with row - m_begin <= 16383 (one-tap kernel: `yoff`; one wave per SIMD:
    `yld + g.yoff + op * ystep`, rra + 16 op <= 31 rows inside the sub-step that starts at mk - m_begin <= 16352):
    16383 * 131072 + 512 = 2 147 353 088 < 2^31, no wrap.  The last byte a slice may read is row M - 1, column dy_col + Cy - 1 of the
    buffer: inside the allocation because dy_col + Cy <= ld.  x has a 256 / 512-byte row stride: its offsets stay below 2^23."""
    frames, S, C_ = 18, 32, 128
    poison = lambda shape: torch.empty(shape, dtype=dtype, device=DEV).normal_(0.0, POISON * DY_SCALE)
    r = Request(dtype, frames, C_, C_, (S, S), (3, 3), dy_col=40000 if dtype == BF else 20000, ld=ld, seed=31, x_pre=1, dy_pre=0, post=0,
                fill_dy=poison)
    try:
        assert r.dybuf.numel() * r.dybuf.element_size() == 18432 * 131072
        dw, db = r.dw_pre.clone(), r.db_pre.clone()
        seen = profiled(lambda: r.strided(dw, 1, db[r.db_win]))
        e_dw = rel(r.window(dw).double() - r.window(r.dw_pre).double(), r.dw_ref)
        e_db = rel(db[r.db_win].double() - r.db_pre[r.db_win].double(), r.db_ref)
        dwd, dbd = torch.zeros(C_, C_, 3, 3, device=DEV), torch.zeros(C_, device=DEV)
        r.dense(dwd, 2, dbd)
        dwz, dbz = torch.zeros_like(r.dw_pre), torch.zeros(3 * C_, device=DEV)
        r.strided(dwz, 1, dbz[r.db_win])
        e_dense, e_dense_b = rel(r.window(dwz), dwd), rel(dbz[r.db_win], dbd)
        print(f"wgrad offset cap {dtype}: family {seen}, dw {e_dw:.2e}, dbias {e_db:.2e}, against dense msplit 2: dw {e_dense:.2e}, dbias {e_dense_b:.2e}")
        assert seen == {family: 1}
        r.check_untouched(dw, db)
        assert e_dw < 1e-5 and e_db < 5e-6
        # the dense call cuts the rows 9216 + 9216, the capped one 16384 + 2048: other fp32 summation orders of the same sums, each
        # within its bound of the fp64 reference, hence within the sum of the two bounds of each other
        assert rel(dwd, r.dw_ref) < 1e-5
        assert e_dense < 2e-5 and e_dense_b < 1e-5
    finally:
        del r
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_requests_launch_nothing():
    """overwrite = 1 into a strided master is refused by the library; a dy_col that is not a multiple of 8 (dy is read in 16-byte
    vectors from the shifted pointer) and a dw window that leaves the master are refused by kern.conv_wgrad before the library is
    called.  Nothing is launched and dw keeps its prefill."""
    from dvd_gan_amd import kern as K
    r = single_request(1, BF, 1)
    dw = r.dw_pre.clone()
    common = dict(frames=r.frames, x_row0=r.x_pre, dy_row0=r.dy_pre)

    def none_launched(**kw):
        def call():
            with pytest.raises(ValueError):
                K.conv_wgrad(r.xbuf, r.dybuf, dw, r.ks, r.cout, r.cin, **common, **kw)
        assert profiled(call) == {}
        assert torch.equal(dw, r.dw_pre)

    none_launched(dy_col=r.dy_col + 4, dw_ci_off=r.ci_off, dw_ci_tot=r.ci_tot)
    none_launched(dy_col=r.dy_col + 2, dw_ci_off=r.ci_off, dw_ci_tot=r.ci_tot)
    none_launched(dy_col=r.dy_col, dw_ci_off=r.ci_off + 4, dw_ci_tot=r.ci_tot)           # 5 + 4 + 16 > 24
    none_launched(dy_col=r.dy_col, dw_ci_off=1)                                          # dw_ci_tot defaults to Cin
    # overwrite into the strided master: refused by the library ahead of its memset and its launch
    assert profiled(lambda: pytest.raises(RuntimeError, r.strided, dw, 0, None, overwrite=True)) == {}
    assert torch.equal(dw, r.dw_pre)

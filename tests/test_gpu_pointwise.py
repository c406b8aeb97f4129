"""GPU parity of the memory-bound kernels (pointwise.hip, misc.hip) against plain float64 torch references, at the benchmark's
own launch sizes (ch = 32, B = 64 clips, T = 48 frames) and at the edges where their size-dependent code paths change.

Every reference is computed on the GPU in float64 from the operands as stored (fp32 or bf16); no project kernel and no oracle
code takes part in it.  Elementwise bounds are written as "what an fp32 evaluation may lose" (a few units of 2^-24 times the
magnitudes involved) plus half an ulp of the storage type where the result is stored in bf16.  Each check prints a MEASURED
line (error over its bound, or a plain error) so that `pytest -s` shows how much room the bounds leave.
"""
import ctypes as ct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
E32 = 2.0 ** -24
DTYPES = [torch.float32, torch.bfloat16]
DX_TOL = {torch.float32: 5e-7, torch.bfloat16: 2.5e-3}     # rel-L2 of the CBN input gradient (bf16: its storage rounding)
STATS_TOL = 2e-7          # mean and rstd of bn_stats, relative (check_stats)
RSTD_EVAL_TOL = 1e-6      # eval-mode rstd against 1 / sqrt(running var + eps), relative
DGB_TOL = 2e-6            # dgb error over the sum of |terms| (check_dgb)
TERMS_TOL = 1e-6          # the fp32 linear / embedding / projection-head sums: error over the sum of |terms|


def note(name, value):
    print(f"MEASURED {name}: {value:.3e}")


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=gen(seed), device=DEV).to(dtype)


def half_ulp(ref, dtype):
    """Half an ulp of `dtype` at |ref| (0 for fp32: its final rounding is part of the fp32 bound; 0 where ref == 0)."""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref.abs().float())                    # |ref| = m * 2^e, m in [0.5, 1): ulp of bf16 = 2^(e - 8)
    h = torch.ldexp(torch.ones_like(ref), (e - 9).to(ref.dtype))
    return torch.where(ref == 0, torch.zeros_like(h), h)


def check_bound(out, ref, bound32, dtype, name):
    """|out - ref| <= bound32 + half an ulp of the storage dtype at ref, elementwise; returns the worst err / allowed."""
    err = (out.double() - ref).abs()
    allowed = bound32 + half_ulp(ref, dtype)
    bad = ~(err <= allowed)                                  # (a NaN or inf in `out` is outside every bound)
    ratio = float((err / allowed.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements outside the bound (worst err / allowed {ratio:.3g})"
    return ratio


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def samp_generator(B, T):
    """The generator's condition table (gen_net.py): frame t*B + b is conditioned on row (b*T + t) mod B."""
    t_idx = torch.arange(T, device=DEV).view(T, 1)
    b_idx = torch.arange(B, device=DEV).view(1, B)
    return ((b_idx * T + t_idx) % B).reshape(-1).to(torch.int32).contiguous()


def samp_uneven(frames, B, seed):
    """Uneven hit counts; rows 1 and B - 1 get no frame at all."""
    w = torch.rand(B, generator=torch.Generator().manual_seed(seed)) ** 3 + 0.01
    w[1] = w[B - 1] = 0
    s = torch.multinomial(w, frames, replacement=True, generator=torch.Generator().manual_seed(seed + 1))
    return s.to(torch.int32).to(DEV).contiguous()


def make_x(frames, P, ld, dtype, seed):
    """[frames, P, ld] storage tensor; the pad lanes hold finite garbage that no kernel may let through."""
    return (randn((frames, P, ld), seed) + 0.3).to(dtype)


def chunks(frames, P, ld, budget=1 << 25):
    step = max(1, budget // (P * ld))
    for f0 in range(0, frames, step):
        yield f0, min(frames, f0 + step)


# ------------------------------------------------------------------------------------------------ batch-norm statistics
def stats_ref(x2, C):
    """fp64 mean / biased variance per channel of the [rows, ld] tensor x2 (two passes, row chunks)."""
    rows = x2.shape[0]
    step = max(1, (1 << 25) // x2.shape[1])
    s = torch.zeros(C, dtype=torch.float64, device=DEV)
    for r0 in range(0, rows, step):
        s += x2[r0:r0 + step, :C].double().sum(0)
    m = s / rows
    q = torch.zeros(C, dtype=torch.float64, device=DEV)
    for r0 in range(0, rows, step):
        q += ((x2[r0:r0 + step, :C].double() - m) ** 2).sum(0)
    return m, q / rows


def check_stats(mean, rstd, x2, C, eps, name):
    m, var = stats_ref(x2, C)
    rs = 1.0 / (var + eps).sqrt()
    em = float(((mean.double() - m).abs() / m.abs()).max())
    er = float(((rstd.double() - rs).abs() / rs).max())
    note(name + " mean rel", em)
    note(name + " rstd rel", er)
    assert em <= STATS_TOL and er <= STATS_TOL, (em, er)
    return m, var


# ------------------------------------------------------------------------------------------------ CBN references
def cbn_apply_check(y, x, C, mean, rstd, gb, samp, relu, dtype, name):
    frames, P, ld = x.shape
    mu, rs = mean.double(), rstd.double()
    worst, num, den = 0.0, 0.0, 0.0
    for f0, f1 in chunks(frames, P, ld):
        s = samp[f0:f1].long()
        gam, bet = gb[s, :C].double()[:, None], gb[s, C:].double()[:, None]
        xh = (x[f0:f1, :, :C].double() - mu) * rs
        pre = gam * xh + bet
        ref = pre.clamp_min(0) if relu else pre
        bound = 3 * E32 * ((gam * xh).abs() + bet.abs())
        worst = max(worst, check_bound(y[f0:f1, :, :C], ref, bound, dtype, name))
        num += float(((y[f0:f1, :, :C].double() - ref) ** 2).sum())
        den += float((ref ** 2).sum())
        assert bool((y[f0:f1, :, C:] == 0).all()), name + ": pad lanes"
    note(name + " err/bound", worst)
    note(name + " rel-L2", (num / den) ** 0.5)
    if dtype == torch.float32:
        assert (num / den) ** 0.5 <= 2e-7


def mask_ambiguous(g, x, C, mean, rstd, gb, samp, relu):
    """g := 0 where the fp64 pre-activation is within 1e-4 of zero: the ReLU mask of those elements is a matter of fp32 rounding."""
    if not relu:
        return g
    frames, P, ld = x.shape
    for f0, f1 in chunks(frames, P, ld):
        s = samp[f0:f1].long()
        pre = gb[s, :C].double()[:, None] * ((x[f0:f1, :, :C].double() - mean.double()) * rstd.double()) + gb[s, C:].double()[:, None]
        g[f0:f1, :, :C].masked_fill_(pre.abs() < 1e-4, 0)
    return g


def cbn_backward_ref(g, x, C, mean, rstd, gb, samp, relu, B):
    """-> (dgb [B][2C], sum of |terms| [B][2C], s1 [C], s2 [C]) in fp64."""
    frames, P, ld = x.shape
    mu, rs = mean.double(), rstd.double()
    dgb = torch.zeros(B, 2 * C, dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(dgb)
    for f0, f1 in chunks(frames, P, ld):
        s = samp[f0:f1].long()
        xh = (x[f0:f1, :, :C].double() - mu) * rs
        gm = g[f0:f1, :, :C].double()
        if relu:
            gm = gm * ((gb[s, :C].double()[:, None] * xh + gb[s, C:].double()[:, None]) > 0)
        dgb.index_add_(0, s, torch.cat([(gm * xh).sum(1), gm.sum(1)], 1))
        mag.index_add_(0, s, torch.cat([(gm * xh).abs().sum(1), gm.abs().sum(1)], 1))
    gam = gb[:, :C].double()
    return dgb, mag, (gam * dgb[:, C:]).sum(0), (gam * dgb[:, :C]).sum(0)


def dx_rel_l2(dx, g, x, C, mean, rstd, gb, samp, relu, s1, s2, n):
    frames, P, ld = x.shape
    mu, rs = mean.double(), rstd.double()
    num = den = 0.0
    for f0, f1 in chunks(frames, P, ld):
        s = samp[f0:f1].long()
        gam = gb[s, :C].double()[:, None]
        xh = (x[f0:f1, :, :C].double() - mu) * rs
        gm = g[f0:f1, :, :C].double()
        if relu:
            gm = gm * ((gam * xh + gb[s, C:].double()[:, None]) > 0)
        ref = rs * (gm * gam - s1 / n - xh * s2 / n)
        num += float(((dx[f0:f1, :, :C].double() - ref) ** 2).sum())
        den += float((ref ** 2).sum())
        assert bool((dx[f0:f1, :, C:] == 0).all()), "dx pad lanes"
    return (num / den) ** 0.5


def check_dgb(dgb, ref, mag, samp, B, name):
    err = float(((dgb.double() - ref).abs() / mag.clamp_min(1e-300)).max())
    note(name + " dgb err / sum|terms|", err)
    assert err <= DGB_TOL, err
    hit = torch.zeros(B, dtype=torch.bool, device=DEV)
    hit[samp.long()] = True
    assert bool((dgb[~hit] == 0).all()), name + ": rows without frames"


def cbn_case(dtype, frames, P, C, ld, samp, B, relu, seed, name, with_stats):
    from dvd_gan_amd import kern as K
    x = make_x(frames, P, ld, dtype, seed)
    if with_stats:                      # the production pairing: statistics of the same tensor through bn_stats
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        x2 = x.view(-1, ld)
        mean, rstd = K.bn_stats(x2, C, True, 1e-5, 0.1, rm, rv)
        check_stats(mean, rstd, x2, C, 1e-5, name + " bn_stats")
    else:
        mean = randn(C, seed + 1) * 0.3
        rstd = torch.rand(C, generator=gen(seed + 2), device=DEV) * 1.5 + 0.5
    gb = torch.cat([1 + 0.5 * randn((B, C), seed + 3), 0.5 * randn((B, C), seed + 4)], 1).contiguous()
    y = K.cbn_apply(x, C, mean, rstd, gb, samp, relu)
    cbn_apply_check(y, x, C, mean, rstd, gb, samp, relu, dtype, name + " cbn_apply")
    del y
    g = mask_ambiguous(randn((frames, P, ld), seed + 5), x, C, mean, rstd, gb, samp, relu).to(dtype)
    dx, dgb = K.cbn_backward(g, None, x, C, mean, rstd, gb, samp, relu)
    ref, mag, s1, s2 = cbn_backward_ref(g, x, C, mean, rstd, gb, samp, relu, B)
    check_dgb(dgb, ref, mag, samp, B, name)
    e = dx_rel_l2(dx, g, x, C, mean, rstd, gb, samp, relu, s1, s2, frames * P)
    note(name + " dx rel-L2", e)
    assert e <= DX_TOL[dtype], e
    dx2, dgb2 = K.cbn_backward(g, None, x, C, mean, rstd, gb, samp, relu)
    assert torch.equal(dgb, dgb2) and torch.equal(dx, dx2), name + ": not reproducible"


GEN_SITES = [(16, 256), (64, 256), (256, 256), (1024, 128), (4096, 64)]      # (P, C) of the generator's CBN layers at ch = 32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("site", GEN_SITES)
def test_bn_cbn_generator_sites(site, dtype):
    """bn_stats + cbn_apply + cbn_backward at the benchmark's 3072 frames (B = 64, T = 48), with the generator's own condition
    table: every row has 48 frames, 32 of them in the gather's first 2048-frame round."""
    P, C = site
    torch.cuda.empty_cache()
    cbn_case(dtype, 3072, P, C, C, samp_generator(64, 48), 64, True, 100 + P, f"G P={P} C={C} {dtype}", True)


CBN_EDGES = [
    # frames, P, C, ld, table, B, relu
    (96, 100, 3, 16, "uneven", 7, True),        # ragged C, ld > pad8(C): two pad groups in the apply kernels, one in the reduce
    (64, 2500, 12, 24, "uneven", 5, False),     # P not a multiple of any chunk (2048 reduce, 16 nj apply, 64 nj bwd apply)
    (40, 777, 120, 136, "single", 1, True),     # one condition row
    (9, 40, 2048, 2048, "uneven", 4, True),     # ld / 8 = 256: one row group per workgroup
    (4097, 64, 64, 64, "uneven", 11, True),     # three gather rounds, uneven rows: `carry` != 0
    (3072, 300, 40, 48, "uneven", 64, False),   # a data-parallel-like table at the benchmark's frame count
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CBN_EDGES)
def test_bn_cbn_edges(case, dtype):
    frames, P, C, ld, table, B, relu = case
    samp = samp_uneven(frames, B, frames + C) if table == "uneven" else torch.zeros(frames, dtype=torch.int32, device=DEV)
    cbn_case(dtype, frames, P, C, ld, samp, B, relu, frames * 7 + C, f"edge {case} {dtype}", True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cbn_dgb_gather_order(dtype):
    """cbn_dgb_gather_kernel adds the per-frame chunk partials of condition row s in an order fixed by `samp` alone: lane q takes
    hits q, q+4, ... of the WHOLE frame-ordered hit list (`carry` re-aligns the lanes from one 2048-frame round to the next), each
    hit's chunk partials in chunk order, then ((l0 + l1) + l2) + l3.  One nonzero gradient pixel per (frame, chunk) makes every
    partial an exactly known fp32 number, so that order can be replayed bit for bit; values spread over 2^+-10 make a different
    order round differently."""
    from dvd_gan_amd import kern as K
    frames, P, C, ld, B = 4097, 2100, 12, 16, 6
    samp = samp_uneven(frames, B, 5)
    first = torch.bincount(samp[:2048].long(), minlength=B)
    assert bool(((first % 4) != 0).any()), "the first round must leave some row's lanes misaligned"
    x = make_x(frames, P, ld, dtype, 17)
    mean = randn(C, 18) * 0.3
    rstd = torch.rand(C, generator=gen(19), device=DEV) + 0.5
    gb = torch.cat([1 + 0.5 * randn((B, C), 20), 0.5 * randn((B, C), 21)], 1).contiguous()
    f = torch.arange(frames, device=DEV)
    pix = torch.stack([f % 2048, 2048 + f % (P - 2048)], 1)                   # one pixel in each of the two 2048-pixel chunks
    scale = torch.ldexp(torch.ones(frames, 2, C, device=DEV),
                        torch.randint(-10, 11, (frames, 2, C), generator=gen(22), device=DEV).float())
    val = (randn((frames, 2, C), 23) * scale).to(dtype)
    g = torch.zeros(frames, P, ld, dtype=dtype, device=DEV)
    g[f[:, None], pix, :C] = val
    dx, dgb = K.cbn_backward(g, None, x, C, mean, rstd, gb, samp, False)
    # the exact partials: db = the one value, dg = fl(value * fl(fl(x - mean) * rstd)) (all other products are 0 * finite)
    xh = (x[f[:, None], pix, :C].float() - mean) * rstd
    part = torch.cat([val.float() * xh, val.float()], 2).cpu().numpy()          # [frames][2 chunks][2C]
    want = np.zeros((B, 2 * C), np.float32)
    sp = samp.cpu().numpy()
    for s in range(B):
        lanes = np.zeros((4, 2 * C), np.float32)
        for i, fr in enumerate(np.nonzero(sp == s)[0]):
            for k in range(2):
                lanes[i % 4] += part[fr, k]
        want[s] = ((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]
    got = dgb.cpu().numpy()
    diff = int((got != want).sum())
    note(f"gather order {dtype} mismatching elements", diff)
    assert diff == 0, f"{diff} dgb elements differ from the documented summation order"


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_cbn_replicas(dtype):
    """The data-parallel form: the [NREP][2C] statistics sums and the backward's s12 are added over two half batches between
    the reduce and the apply stages; the result must be the whole batch's."""
    from dvd_gan_amd import lib as L
    from dvd_gan_amd import kern as K
    frames, P, C, ld, B = 128, 256, 40, 48, 8
    samp = samp_uneven(frames, B, 77)
    x = make_x(frames, P, ld, dtype, 31)
    h = frames // 2
    xa, xb = x[:h].contiguous(), x[h:].contiguous()
    x2 = x.view(-1, ld)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, rstd = K.bn_stats(x2, C, True, 1e-5, 0.1, rm, rv)
    sums_b = torch.zeros(L.BN_NREP * 2 * C, dtype=torch.float64, device=DEV)
    L.check(L.lib().dvd_bn_stats(L.dt(xb), L.ptr(xb), ct.c_longlong(h * P), C, ld, L.ptr(sums_b), L.stream()))
    rm2, rv2 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean_r, rstd_r = K.bn_stats(xa.view(-1, ld), C, True, 1e-5, 0.1, rm2, rv2, replicas=(2, lambda s: s.add_(sums_b)))
    check_stats(mean_r, rstd_r, x2, C, 1e-5, f"replicas {dtype} bn_stats")
    assert float((mean_r - mean).abs().max()) <= 1e-6 * float(mean.abs().max())
    assert float(((rv2 - rv).abs() / rv).max()) <= 1e-6 and float((rm2 - rm).abs().max()) <= 1e-7

    gb = torch.cat([1 + 0.5 * randn((B, C), 32), 0.5 * randn((B, C), 33)], 1).contiguous()
    g = mask_ambiguous(randn((frames, P, ld), 34), x, C, mean, rstd, gb, samp, True).to(dtype)
    ga, gbh = g[:h].contiguous(), g[h:].contiguous()
    sa, sb = samp[:h].contiguous(), samp[h:].contiguous()

    def reduce_only(gh, xhf, sh):
        dgb = torch.zeros_like(gb)
        s12 = torch.empty(2 * C, dtype=torch.float32, device=DEV)
        part = torch.empty(L.lib().dvd_cbn_backward_ws_floats(ct.c_longlong(h), P, C), dtype=torch.float32, device=DEV)
        L.check(L.lib().dvd_cbn_backward_reduce(L.dt(xhf), L.ptr(gh), None, L.ptr(xhf), ct.c_longlong(h), P, C, ld, L.ptr(mean),
                                                L.ptr(rstd), L.ptr(gb), L.ptr(sh), B, L.ptr(dgb), L.ptr(s12), 1, L.ptr(part),
                                                L.stream()))
        return dgb, s12

    dgb_a0, s12_a = reduce_only(ga, xa, sa)
    dgb_b0, s12_b = reduce_only(gbh, xb, sb)
    dxa, dgba = K.cbn_backward(ga, None, xa, C, mean, rstd, gb, sa, True, replicas=(2, lambda s: s.add_(s12_b)))
    dxb, dgbb = K.cbn_backward(gbh, None, xb, C, mean, rstd, gb, sb, True, replicas=(2, lambda s: s.add_(s12_a)))
    assert torch.equal(dgba, dgb_a0) and torch.equal(dgbb, dgb_b0)
    ref, mag, s1, s2 = cbn_backward_ref(g, x, C, mean, rstd, gb, samp, True, B)
    check_dgb(dgba + dgbb, ref, mag, samp, B, f"replicas {dtype}")
    dx = torch.cat([dxa, dxb])
    e = dx_rel_l2(dx, g, x, C, mean, rstd, gb, samp, True, s1, s2, frames * P)
    note(f"replicas {dtype} dx rel-L2", e)
    assert e <= DX_TOL[dtype], e
    dx_whole, _ = K.cbn_backward(g, None, x, C, mean, rstd, gb, samp, True)
    assert rel_l2(dx, dx_whole) <= DX_TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_stats_running_buffers_eval_and_workspace(dtype):
    """Running mean / UNBIASED running variance (few rows, so n / (n - 1) is visible), eval mode reading the running buffers, a
    persistent sums workspace left exactly zero, and (fp32) a channel whose mean is 3000 standard deviations."""
    from dvd_gan_amd import lib as L
    from dvd_gan_amd import kern as K
    C, ld, rows, eps, mom = 12, 16, 37, 1e-5, 0.3
    x = (randn((rows, ld), 41) * 2 + 0.7).to(dtype)
    rm0, rv0 = randn(C, 42) * 0.1, torch.rand(C, generator=gen(43), device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    ws = torch.zeros(L.BN_NREP * 2 * C, dtype=torch.float64, device=DEV)
    mean, rstd = K.bn_stats(x, C, True, eps, mom, rm, rv, sums=ws)
    assert bool((ws == 0).all()), "the persistent workspace must be left zeroed"
    m, var = check_stats(mean, rstd, x, C, eps, f"small {dtype}")
    want_rm = (1 - mom) * rm0.double() + mom * m
    want_rv = (1 - mom) * rv0.double() + mom * var * rows / (rows - 1)
    erm = float(((rm.double() - want_rm).abs() / want_rm.abs()).max())
    erv = float(((rv.double() - want_rv).abs() / want_rv).max())
    note(f"running buffers {dtype} rel", max(erm, erv))
    assert erm <= 5e-7 and erv <= 5e-7, (erm, erv)
    # a second pass through the same workspace gives the same statistics (nothing left behind by the first)
    mean2, rstd2 = K.bn_stats(x, C, True, eps, mom, rm.clone(), rv.clone(), sums=ws)
    assert torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    # eval mode: the running buffers, untouched
    rm_c, rv_c = rm.clone(), rv.clone()
    me, re = K.bn_stats(x, C, False, eps, mom, rm, rv)
    assert torch.equal(me, rm_c) and torch.equal(rm, rm_c) and torch.equal(rv, rv_c)
    assert float(((re.double() - 1 / (rv_c.double() + eps).sqrt()).abs() * (rv_c.double() + eps).sqrt()).max()) <= RSTD_EVAL_TOL
    if dtype == torch.float32:
        rows2 = 300000
        xf = randn((rows2, 8), 44) * 0.01
        xf[:, 2] += 30.0
        mean3, rstd3 = K.bn_stats(xf, 8, True, eps, mom, torch.zeros(8, device=DEV), torch.ones(8, device=DEV))
        check_stats(mean3, rstd3, xf, 8, eps, "large |mean| / std")


@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_group_limit(dtype):
    """ld / 8 = 256 channel groups is the last shape the statistics, column-sum and CBN entries take; 257 is DVD_E_SHAPE before
    anything is launched."""
    from dvd_gan_amd import lib as L
    from dvd_gan_amd import kern as K
    x = (randn((3000, 2048), 51) + 0.5).to(dtype)
    mean, rstd = K.bn_stats(x, 2048, True, 1e-5, 0.1, torch.zeros(2048, device=DEV), torch.ones(2048, device=DEV))
    check_stats(mean, rstd, x, 2048, 1e-5, f"C=2048 {dtype}")
    cs = K.colsum(x, 2048)
    ref = x.double().sum(0)
    assert float(((cs.double() - ref).abs() / x.double().abs().sum(0)).max()) <= 5e-6
    lib, s = L.lib(), L.stream()
    xw = torch.zeros(1, 2056, dtype=dtype, device=DEV)
    f = torch.zeros(2 * 2056, device=DEV)
    sums = torch.zeros(L.BN_NREP * 2 * 2056, dtype=torch.float64, device=DEV)
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    dt, p, ll = L.dt(xw), L.ptr(xw), ct.c_longlong(1)
    assert lib.dvd_bn_stats(dt, p, ll, 2056, 2056, L.ptr(sums), s) == -2
    assert lib.dvd_colsum(dt, p, ll, 2056, 2056, L.ptr(f), s) == -2
    assert lib.dvd_cbn_apply(dt, p, p, ll, 1, 2056, 2056, L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(one), 1, s) == -2
    assert lib.dvd_cbn_backward_reduce(dt, p, None, p, ll, 1, 2056, 2056, L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(one), 1, L.ptr(f),
                                       L.ptr(f), 1, L.ptr(f), s) == -2
    assert lib.dvd_cbn_backward_apply(dt, p, None, p, p, ll, 1, 2056, 2056, L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(one), L.ptr(f),
                                      ll, 1, s) == -2


# ------------------------------------------------------------------------------------------------ pooling / resampling
POOLS = [
    # frames, T, H, W, C, ld, pt, scale
    (512, 1, 64, 64, 64, 64, 1, None),          # D_s after its stem: 512 frames of 64 x 64
    (64, 48, 32, 32, 64, 64, 2, None),          # D_t after its stem: 64 clips x 48 frames of 32 x 32, (2, 2, 2) windows
    (3, 6, 7, 9, 12, 16, 2, 1.0),               # odd grids (floor), pad lanes, scale = 1 (the gradient of nearest x2)
    (5, 1, 13, 3, 3, 8, 1, 0.3),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", POOLS)
def test_pool_masked_pool_unpool(case, dtype):
    from dvd_gan_amd import kern as K
    Fr, T, H, W, Cc, ld, pt, scale = case
    shape = (Fr, T, H, W, ld) if T > 1 else (Fr, H, W, ld)
    x = randn(shape, Fr + H, dtype)
    sc = (1.0 / (4 * pt)) if scale is None else scale
    y = K.pool(x, pt, scale)
    To, Ho, Wo = T // pt, H // 2, W // 2
    xs = x.double().view(Fr, T, H, W, ld)[:, :To * pt, :Ho * 2, :Wo * 2]
    win = xs.reshape(Fr, To, pt, Ho, 2, Wo, 2, ld)
    ref = win.sum((2, 4, 6)) * sc
    bound = 4 * pt * E32 * win.abs().sum((2, 4, 6)) * abs(sc)
    note(f"pool {case} {dtype} err/bound", check_bound(y.view(Fr, To, Ho, Wo, ld), ref, bound, dtype, "pool"))
    if not (H | W) & 1:                          # masked form (output-grid ReLU mask; even grids only)
        mask = randn(y.shape, Fr + 99, dtype).clamp_min(0)     # half of it exactly zero
        ym = K.pool(x, pt, scale, mask=mask)
        on = mask.view(Fr, To, Ho, Wo, ld).double() > 0
        assert bool((ym.view(Fr, To, Ho, Wo, ld)[~on] == 0).all())
        check_bound(ym.view(Fr, To, Ho, Wo, ld), ref * on, bound, dtype, "masked pool")
        del ym, mask
    del x, y, xs, win, ref, bound
    # unpool: the transpose, onto the grid the pooling started from (odd last line / column exactly zero)
    xi = randn(((Fr, To, Ho, Wo, ld) if T > 1 else (Fr, Ho, Wo, ld)), Fr + 7, dtype)
    yu = K.unpool(xi, pt, scale, out_hw=(H, W)).view(Fr, T, H, W, ld)
    up = (xi.float() * sc).to(dtype).view(Fr, To, Ho, Wo, ld)
    want = torch.zeros(Fr, T, H, W, ld, dtype=dtype, device=DEV)
    want[:, :, :Ho * 2, :Wo * 2] = up.repeat_interleave(pt, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert torch.equal(yu, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(4, 8, 16, 16, 64), (3, 6, 10, 6, 24)])
def test_maxpool3d(shape, dtype):
    """2 x 2 x 2 max pooling and its gradient, bitwise against torch's CPU max_pool3d (first maximum in (t, h, w) order gets the
    gradient); inputs drawn from five values so that ties are everywhere."""
    from dvd_gan_amd import lib as L
    Fr, T, H, W, ld = shape
    cpu = torch.Generator().manual_seed(sum(shape))
    x = (torch.randint(-2, 3, shape, generator=cpu).float() * 0.5).to(dtype)
    dy = torch.randn(Fr, T // 2, H // 2, W // 2, ld, generator=cpu).to(dtype)
    xd, dyd = x.to(DEV), dy.to(DEV)
    y = torch.empty(dy.shape, dtype=dtype, device=DEV)
    dx = torch.empty_like(xd)
    lib, s = L.lib(), L.stream()
    L.check(lib.dvd_maxpool3d(L.dt(xd), L.ptr(xd), L.ptr(y), ct.c_longlong(Fr), T // 2, H // 2, W // 2, ld, s))
    L.check(lib.dvd_maxpool3d_backward(L.dt(xd), L.ptr(xd), L.ptr(dyd), L.ptr(dx), ct.c_longlong(Fr), T // 2, H // 2, W // 2, ld, s))
    xr = x.float().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    yr = F.max_pool3d(xr, 2, 2)
    yr.backward(dy.float().permute(0, 4, 1, 2, 3))
    assert torch.equal(y.cpu().float(), yr.detach().permute(0, 2, 3, 4, 1))
    assert torch.equal(dx.cpu().float(), xr.grad.permute(0, 2, 3, 4, 1))


# ------------------------------------------------------------------------------------------------ sums / elementwise
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(3072 * 1024, 128, 128), (4_000_000, 3, 8), (700_001, 120, 136)])
def test_colsum(case, dtype):
    from dvd_gan_amd import kern as K
    rows, Cc, ld = case
    x = (randn((rows, ld), rows % 1000) + 1.0).to(dtype)
    out0 = randn(Cc, 3)
    out = K.colsum(x, Cc, out=out0.clone())
    step = 1 << 20
    ref = out0.double().clone()
    mag = out0.double().abs()
    for r0 in range(0, rows, step):
        xs = x[r0:r0 + step, :Cc].double()
        ref += xs.sum(0)
        mag += xs.abs().sum(0)
    e = float(((out.double() - ref).abs() / mag).max())
    note(f"colsum {case} {dtype} err / sum|x|", e)
    assert e <= 5e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_sum_leading_and_act_backward(dtype):
    from dvd_gan_amd import kern as K
    from dvd_gan_amd import lib as L
    Lh, n = 48, 64 * 16 * 16 * 24
    x = randn((Lh, n), 61, dtype)
    out = K.sum_leading(x)
    xd = x.double()
    r = check_bound(out, xd.sum(0), Lh * E32 * xd.abs().sum(0), dtype, "sum_leading")
    note(f"sum_leading {dtype} err/bound", r)
    n = 1 << 20
    dy = randn(n, 62, dtype)
    yr = randn(n, 63, dtype)
    assert torch.equal(K.act_backward(dy, yr, L.ACT_RELU), torch.where(yr > 0, dy, torch.zeros_like(dy)))
    yt = torch.tanh(randn(n, 64) * 2).to(dtype)
    g, y = dy.double(), yt.double()
    r = check_bound(K.act_backward(dy, yt, L.ACT_TANH), g * (1 - y * y), 3 * E32 * g.abs() * (1 + y * y), dtype, "tanh'")
    note(f"tanh' {dtype} err/bound", r)
    ys = torch.sigmoid(randn(n, 65) * 3).to(dtype)
    y = ys.double()
    r = check_bound(K.act_backward(dy, ys, L.ACT_SIGMOID), g * y * (1 - y), 4 * E32 * g.abs() * (y.abs() + y * y), dtype, "sigmoid'")
    note(f"sigmoid' {dtype} err/bound", r)


# ------------------------------------------------------------------------------------------------ spectral norm
def power_iter_ref(W, u):
    W = W.double().view(W.shape[0], -1)
    vr = W.t() @ u.double()
    v = vr / (vr.norm() + 1e-12)
    wv = W @ v
    n = wv.norm()
    return n * n / (n + 1e-12), wv / (n + 1e-12), v


SN_ITEMS = [
    # cout, cin, kernel taps, pack dtype (None: power iteration only)
    (8, 3, (3, 3), torch.bfloat16),             # the stems' size: one block of every launch
    (512, 512, (3, 3), torch.bfloat16),         # 512 x 4608, the largest matrix
    (6, 40, (1, 1), torch.float32),             # h not a multiple of 4
    (24, 40, (5, 5), torch.float32),            # w = 1000: not a multiple of 256
    (1, 512, None, None),                       # the projection head's linear weight
    (13, 7, (3, 3, 3), torch.bfloat16),         # 3-D taps, odd h
    (300, 260, (3, 3), torch.float32),          # several blocks of each launch on both sides
]


def test_sn_batched():
    """dvd_sn_batched over a mixed item table: sigma / u / v against one fp64 power-iteration step from the same u, the packs
    bitwise equal to W / sigma rounded to the storage type in the [tap][co][ci] and flipped [tap'][ci][co] layouts."""
    from dvd_gan_amd import kern as K
    from dvd_gan_amd import lib as L
    items = (L.SnItem * len(SN_ITEMS))()
    keep = []
    for i, (co, ci, k, pdt) in enumerate(SN_ITEMS):
        ntaps = int(np.prod(k)) if k else 1
        W = randn((co, ci) + (tuple(k) if k else ()), 200 + i) / (ci * ntaps) ** 0.5
        u = randn(co, 300 + i)
        u /= u.norm()
        v = torch.full((ci * ntaps,), float("nan"), device=DEV)
        sigma = torch.zeros(1, device=DEV)
        it = items[i]
        it.W, it.u, it.v, it.sigma = W.data_ptr(), u.data_ptr(), v.data_ptr(), sigma.data_ptr()
        it.h, it.w = co, ci * ntaps
        pk = None
        if pdt is not None:
            pk = K.PackedConv(pdt, co, ci, k, DEV)
            pk.wf.fill_(float("nan"))
            it.wf, it.wd = pk.wf.data_ptr(), pk.wd.data_ptr()
            it.dtype, it.cout, it.cin, it.ntaps, it.cip, it.cop = L.dt(pk.wf), co, ci, pk.ntaps, pk.cip, pk.cop
        keep.append((W, u.clone(), u, v, sigma, pk))
    nfl = ct.c_longlong()
    L.check(L.lib().dvd_sn_batched_prepare(items, len(SN_ITEMS), ct.byref(nfl)))
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(DEV)
    scratch = torch.empty(max(1, nfl.value), dtype=torch.float32, device=DEV)
    L.check(L.lib().dvd_sn_batched(items, ct.c_void_p(table.data_ptr()), len(SN_ITEMS), ct.c_void_p(scratch.data_ptr()), L.stream()))
    torch.cuda.synchronize()
    worst = 0.0
    for (co, ci, k, pdt), (W, u0, u, v, sigma, pk) in zip(SN_ITEMS, keep):
        s_ref, u_ref, v_ref = power_iter_ref(W, u0)
        es = abs(float(sigma) - float(s_ref)) / float(s_ref)
        eu, ev = float((u.double() - u_ref).abs().max()), float((v.double() - v_ref).abs().max())
        worst = max(worst, es, eu, ev)
        assert es <= 1e-6 and eu <= 1e-6 and ev <= 1e-6, ((co, ci, k), es, eu, ev)
        if pk is None:
            continue
        ntaps = pk.ntaps
        wn = (W / sigma).to(pdt).view(co, ci, ntaps)                       # the IEEE fp32 quotient, rounded to the pack type
        wf = torch.zeros(ntaps, co, pk.cip, dtype=pdt, device=DEV)
        wf[:, :, :ci] = wn.permute(2, 0, 1)
        assert torch.equal(pk.wf, wf), (co, ci, k)
        wd = torch.zeros(ntaps, pk.cip, pk.cop, dtype=pdt, device=DEV)
        wd[:, :ci, :co] = wn.permute(2, 1, 0).flip(0)
        assert torch.equal(pk.wd, wd), (co, ci, k)
    note("sn_batched sigma/u/v", worst)


def test_sn_backward_past_the_partial_cap():
    """512 x 4608 = 2.4 M elements: 1152 blocks' worth of partial sums, capped at DVD_SN_SCRATCH = 512; the gradient
    G / sigma - (sum G*W) / sigma^2 u v^T against fp64 (the rank-one term dominates here), and bit-identical on a rerun."""
    from dvd_gan_amd import kern as K
    h, w = 512, 4608
    W = randn((h, w), 401) * 0.02
    u = randn(h, 402)
    u /= u.norm()
    v = randn(w, 403)
    v /= v.norm()
    sigma = torch.tensor([1.7], device=DEV)
    G = (W + randn((h, w), 404) * 0.02).contiguous()
    dW0 = randn((h, w), 405) * 0.1
    dW = K.sn_backward(G, W, u, v, sigma, out=dW0.clone())
    s = float(sigma)
    g64 = G.double()
    dot = float((g64 * W.double()).sum())
    rank1 = dot / (s * s) * torch.outer(u.double(), v.double())
    ref = g64 / s - rank1
    assert float(rank1.norm()) > 0.5 * float(ref.norm())
    e = rel_l2(dW - dW0, ref)
    note("sn_backward rel-L2", e)
    assert e <= 1e-6
    dW2 = K.sn_backward(G, W, u, v, sigma, out=dW0.clone())
    assert torch.equal(dW, dW2)


# ------------------------------------------------------------------------------------------------ discriminator head / losses
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(512, 16, 512, 512), (100, 9, 120, 128)])
def test_relu_spatial_sum(case, dtype):
    from dvd_gan_amd import lib as L
    Fr, P, Cc, ld = case
    feat = randn((Fr, P, ld), 501, dtype)
    hsum = torch.empty(Fr, Cc, device=DEV)
    L.check(L.lib().dvd_relu_spatial_sum(L.dt(feat), L.ptr(feat), L.ptr(hsum), ct.c_longlong(Fr), P, Cc, ld, L.stream()))
    r = feat[..., :Cc].double().clamp_min(0)
    e = check_bound(hsum, r.sum(1), P * E32 * r.sum(1), torch.float32, "relu_spatial_sum")
    note(f"relu_spatial_sum {case} {dtype} err/bound", e)
    dh = randn((Fr, Cc), 502)
    dfeat = torch.full_like(feat, float("nan"))
    L.check(L.lib().dvd_relu_spatial_sum_backward(L.dt(feat), L.ptr(dh), L.ptr(feat), L.ptr(dfeat), ct.c_longlong(Fr), P, Cc, ld,
                                                  L.stream()))
    want = torch.zeros_like(feat)
    want[..., :Cc] = torch.where(feat[..., :Cc] > 0, dh[:, None, :].to(dtype), torch.zeros((), dtype=dtype, device=DEV))
    assert torch.equal(dfeat, want)


def test_proj_head():
    """Projection head at D_s's 512 frames, 512 channels, 101 classes drawn with repeats (some absent): out / dh against fp64,
    g_lin / g_bias / g_emb (accumulated into prefilled buffers) within 1e-6 of the sum of |terms|, absent classes' g_emb rows
    untouched, bit-identical on a rerun."""
    from dvd_gan_amd import lib as L
    Fr, Cc, ncls = 512, 512, 101
    cls = torch.randint(0, ncls - 10, (Fr,), generator=gen(601), device=DEV).to(torch.int32)     # classes 91..100 absent
    hsum = randn((Fr, Cc), 602).abs() * 3
    wl, emb = randn(Cc, 603) * 0.05, randn((ncls, Cc), 604) * 0.05
    sl, se = torch.tensor([1.3], device=DEV), torch.tensor([0.7], device=DEV)
    bias = torch.tensor([0.25], device=DEV)
    lib, s = L.lib(), L.stream()
    out = torch.empty(Fr, device=DEV)
    L.check(lib.dvd_proj_head_forward(L.ptr(hsum), L.ptr(wl), L.ptr(sl), L.ptr(bias), L.ptr(emb), L.ptr(se), L.ptr(cls), L.ptr(out),
                                      ct.c_longlong(Fr), Cc, s))
    h64, cl = hsum.double(), cls.long()
    weff = wl.double() / 1.3 + emb.double()[cl] / 0.7
    terms = h64 * weff
    ref = terms.sum(1) + 0.25
    e = float(((out.double() - ref).abs() / (terms.abs().sum(1) + 0.25)).max())
    note("proj_head out err / sum|terms|", e)
    assert e <= TERMS_TOL
    dout = randn(Fr, 605)
    g0 = [randn(Cc, 606), randn((ncls, Cc), 607), randn(1, 608)]

    def bwd():
        dh = torch.empty(Fr, Cc, device=DEV)
        gl, ge, gbias = (t.clone() for t in g0)
        L.check(lib.dvd_proj_head_backward(L.ptr(dout), L.ptr(hsum), L.ptr(wl), L.ptr(sl), L.ptr(emb), L.ptr(se), L.ptr(cls),
                                           L.ptr(dh), L.ptr(gl), L.ptr(ge), L.ptr(gbias), ct.c_longlong(Fr), Cc, s))
        return dh, gl, ge, gbias

    dh, gl, ge, gbias = bwd()
    d64 = dout.double()
    wabs = wl.double().abs() / 1.3 + emb.double()[cl].abs() / 0.7
    e = float(((dh.double() - d64[:, None] * weff).abs() / (d64.abs()[:, None] * wabs)).max())
    note("proj_head dh err / (|d| (|w_l / s_l| + |e / s_e|))", e)
    assert e <= 4 * E32
    t = d64[:, None] * h64
    err = []
    ref_l, mag_l = g0[0].double() + t.sum(0), g0[0].double().abs() + t.abs().sum(0)
    err.append(float(((gl.double() - ref_l).abs() / mag_l).max()))
    ref_b, mag_b = float(g0[2]) + float(d64.sum()), abs(float(g0[2])) + float(d64.abs().sum())
    err.append(abs(float(gbias) - ref_b) / mag_b)
    ref_e = g0[1].double().index_add(0, cl, t)
    mag_e = g0[1].double().abs().index_add(0, cl, t.abs())
    present = torch.zeros(ncls, dtype=torch.bool, device=DEV)
    present[cl] = True
    err.append(float(((ge.double() - ref_e).abs() / mag_e)[present].max()))
    note("proj_head g_lin / g_bias / g_emb err / sum|terms|", max(err))
    assert max(err) <= TERMS_TOL, err
    assert torch.equal(ge[~present], g0[1][~present])
    dh2, gl2, ge2, gb2 = bwd()
    assert torch.equal(dh, dh2) and torch.equal(gl, gl2) and torch.equal(ge, ge2) and torch.equal(gbias, gb2)


@pytest.mark.parametrize("hinge", [1, 0])
@pytest.mark.parametrize("real", [1, 0])
def test_adv_loss(hinge, real):
    """One workgroup reduces n = 3000 > 1024 values; values of exactly +-1 sit on the hinge's kink (gradient 0 there)."""
    from dvd_gan_amd import lib as L
    n, gs = 3000, 0.75
    out = randn(n, 701 + 2 * hinge + real) * 2
    out[::7] = 1.0
    out[3::7] = -1.0
    loss = torch.tensor([0.125], device=DEV)
    dout = torch.empty_like(out)
    L.check(L.lib().dvd_adv_loss(L.ptr(out), ct.c_longlong(n), hinge, real, L.ptr(loss), L.ptr(dout), ct.c_float(gs), L.stream()))
    sgn = -1.0 if real else 1.0
    xv = sgn * out.double()
    terms = (1 + xv).clamp_min(0) if hinge else xv
    ref = 0.125 + float(terms.sum()) / n
    e = abs(float(loss) - ref) / (0.125 + float(terms.abs().sum()) / n)
    note(f"adv_loss hinge={hinge} real={real} rel", e)
    assert e <= 1e-6
    step = torch.tensor(sgn * gs, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    live = (1 + sgn * out > 0) if hinge else torch.ones_like(out, dtype=torch.bool)
    want = torch.where(live, step.to(DEV), torch.zeros((), device=DEV))
    assert torch.equal(dout, want)


def test_linear_and_embedding_backward():
    """fp32 linear with K = 221 (not a multiple of 64) and J = 4096 (the generator's first layer shape), and the embedding
    backward with repeated indices (first occurrence owns the row; absent rows untouched; bit-identical on a rerun)."""
    from dvd_gan_amd import kern as K
    B, Kk, J = 64, 221, 4096
    x, W, b = randn((B, Kk), 801), randn((J, Kk), 802) * 0.1, randn(J, 803)
    y = K.linear_forward(x, W, b)
    x64, W64 = x.double(), W.double()
    e = float(((y.double() - (x64 @ W64.t() + b.double())).abs() / (x64.abs() @ W64.abs().t() + b.double().abs())).max())
    note("linear fwd err / sum|terms|", e)
    assert e <= TERMS_TOL
    dout = randn((B, J), 804)
    din, dW, db = K.linear_backward(dout, x, W, True, True, True)
    d64 = dout.double()
    checks = [(din, d64 @ W64, d64.abs() @ W64.abs()), (dW, d64.t() @ x64, d64.abs().t() @ x64.abs()),
              (db, d64.sum(0), d64.abs().sum(0))]
    e = max(float(((a.double() - r).abs() / m).max()) for a, r, m in checks)
    note("linear bwd err / sum|terms|", e)
    assert e <= TERMS_TOL
    n, D, rows = 512, 120, 101
    idx = torch.randint(0, rows - 20, (n,), generator=gen(805), device=DEV).to(torch.int32)
    g = randn((n, D), 806)
    dW0 = randn((rows, D), 807)
    dW1 = K.embedding_backward(g, idx, rows, dW=dW0.clone())
    ref = dW0.double().index_add(0, idx.long(), g.double())
    mag = dW0.double().abs().index_add(0, idx.long(), g.double().abs())
    e = float(((dW1.double() - ref).abs() / mag).max())
    note("embedding bwd err / sum|terms|", e)
    assert e <= TERMS_TOL
    absent = torch.ones(rows, dtype=torch.bool, device=DEV)
    absent[idx.long()] = False
    assert torch.equal(dW1[absent], dW0[absent])
    assert torch.equal(dW1, K.embedding_backward(g, idx, rows, dW=dW0.clone()))

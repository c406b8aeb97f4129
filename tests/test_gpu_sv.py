"""libdvdgan_hip_sv.so on the device against its fp64 restatement (tests/sv_ref.py): parity of sv, res, fro2 and sn_sigma on the
smallest shapes at which the kernels can go wrong (ragged heads and tails, one row, one column, more rows than columns, every
float offset inside a flat buffer, both stored widths), and the invariants, bit for bit.  Both sides are fp64 and differ in the
order of sums of at most 2^13 terms and at most 17 products: differences sit near 1e-12, the bound is 1e-9 sigma0 per item."""
import numpy as np
import pytest
import torch

import sv_ref as R
from test_sv_cpu import GAPPED, rank_deficient

pytestmark = pytest.mark.gpu

ITERS = 8
TAIL = [4.0, 3.0, 2.0] + list(np.linspace(0.5, 0.05, 40))


def matrices():
    """name -> fp32 [h, w]; the parity cases, the degenerate ones included."""
    out = {f"gap{h}x{w}": R.gapped(h, w, TAIL, seed=h + w)[0] for h, w in GAPPED}
    rng = np.random.default_rng(7)
    for h, w in ((4, 1), (6, 5), (9, 255), (130, 7), (64, 576)):
        out[f"rnd{h}x{w}"] = rng.standard_normal((h, w)).astype(np.float32)
    out["repeat16x40"] = R.exact_low_rank(16, 40, [3.0, 3.0, 1.0])
    out["rank3_10x7"] = rank_deficient()
    out["zero5x9"] = np.zeros((5, 9), np.float32)
    out["two2x9"] = R.gapped(2, 9, [2.0, 1.0], seed=3)[0]
    return out


class Case:
    """All matrices in ONE flat fp32 buffer, matrix i at a float offset = i mod 4 past a multiple of 4; u, v for every second."""

    def __init__(self, block, k, names=None):
        dev = torch.device("cuda", 0)
        mats = matrices()
        self.names = list(mats) if names is None else list(names)
        self.block, self.k = block, k
        offs, off = [], 0
        for i, n in enumerate(self.names):
            off = (off + 3) // 4 * 4 + i % 4
            offs.append(off)
            off += mats[n].size
        host = torch.full((off + 8,), 7.0, dtype=torch.float32)
        for n, o in zip(self.names, offs):
            host[o:o + mats[n].size] = torch.from_numpy(mats[n]).reshape(-1)
        self.flat = host.to(dev)
        self.host = {n: mats[n] for n in self.names}
        self.W = {n: self.flat[o:o + mats[n].size].view(*mats[n].shape) for n, o in zip(self.names, offs)}
        assert {self.W[n].data_ptr() // 4 % 4 for n in self.names} == set(range(min(4, len(self.names))))
        gen = torch.Generator().manual_seed(3)
        self.uv_host = {n: (torch.randn(mats[n].shape[0], generator=gen), torch.randn(mats[n].shape[1], generator=gen))
                        for i, n in enumerate(self.names) if i % 2 == 0}
        self.uv = {n: (u.to(dev), v.to(dev)) for n, (u, v) in self.uv_host.items()}
        shapes = [mats[n].shape for n in self.names]
        self.start = dict(zip(self.names, R.start_blocks(shapes, block, 0)))

    def monitor(self, names=None, rows=1):
        from dvd_gan_amd.spectral import SpectrumMonitor
        names = self.names if names is None else names
        return SpectrumMonitor([(n, self.W[n]) for n in names], k=self.k, block=self.block, sn={n: self.uv[n] for n in names if n in self.uv},
                               rows=rows, start=[torch.from_numpy(self.start[n]) for n in names])

    def rows(self, names=None, iters=(ITERS,)):
        mon = self.monitor(names)
        for t in iters:
            mon.update(t)
        mon.snapshot(0)
        return mon.read()[0]

    def reference(self):
        out = []
        for n in self.names:
            u, v = self.uv_host.get(n, (None, None))
            sv, res, fro2, sn = R.report(self.host[n], self.start[n], ITERS, self.k, None if u is None else u.numpy(),
                                         None if v is None else v.numpy())
            out.append(np.concatenate([sv, res, [fro2, sn]]))
        return np.stack(out)


@pytest.fixture(scope="module")
def case():
    c = Case(8, 3)
    c.got = c.rows().numpy()
    c.want = c.reference()
    return c


def check_parity(c, got, want):
    k, worst = c.k, {}
    for i, n in enumerate(c.names):
        s0 = want[i, 0]
        d_sv, d_res = np.abs(got[i, :k] - want[i, :k]).max(), np.abs(got[i, k:2 * k] - want[i, k:2 * k]).max()
        d_fro = abs(got[i, 2 * k] - want[i, 2 * k])
        print(f"{n}: sigma0 {s0:.6g}  |d sv| {d_sv:.3g}  |d res| {d_res:.3g}  |d fro2| / fro2 {d_fro / max(want[i, 2 * k], 1e-300):.3g}", end="")
        assert d_sv <= 1e-9 * s0 and d_res <= 1e-9 * s0 and d_fro <= 1e-9 * want[i, 2 * k], n
        if n in c.uv:
            d_sn = abs(got[i, 2 * k + 1] - want[i, 2 * k + 1])
            print(f"  |d sn_sigma| {d_sn:.3g}", end="")
            assert d_sn <= 1e-9 * s0, n
        else:
            assert np.isnan(got[i, 2 * k + 1]), n
        print()
        worst[n] = max(d_sv, d_res) / s0 if s0 > 0 else 0.0
    top = max(worst, key=worst.get)
    print("largest difference / sigma0:", worst[top], "at", top)
    assert not np.isnan(got[:, :2 * k + 1]).any()


def test_parity_with_the_restatement_one_table_for_all(case):
    check_parity(case, case.got, case.want)


def test_degenerate_cases_on_the_device(case):
    row = dict(zip(case.names, case.got))
    assert np.abs(row["repeat16x40"][:3] - [3.0, 3.0, 1.0]).max() <= 1e-12 and row["repeat16x40"][3:6].max() < 1e-12
    assert np.all(row["zero5x9"][:7] == 0.0)                            # sv, res, fro2: exact zeros, never a NaN
    assert row["two2x9"][2] == 0.0 and row["two2x9"][5] == 0.0         # r = 2 < k = 3
    assert row["rnd4x1"][1] == 0.0 and row["rnd4x1"][2] == 0.0 and row["gap1x13"][1] == 0.0
    truth = np.linalg.svd(rank_deficient().astype(np.float64), compute_uv=False)
    assert np.abs(row["rank3_10x7"][:3] - truth[:3]).max() <= 1e-9 * truth[0]
    for h, w in GAPPED:                                                  # and against the fp64 SVD, the CPU list's bound
        truth = np.zeros(3)
        s = np.linalg.svd(case.host[f"gap{h}x{w}"].astype(np.float64), compute_uv=False)
        truth[:min(3, len(s))] = s[:3]
        assert np.abs(row[f"gap{h}x{w}"][:3] - truth).max() <= 1e-8 * s[0]


def test_values_beyond_the_rank_are_exact_zeros():
    c = Case(8, 6, names=["rank3_10x7", "zero5x9", "repeat16x40"])
    got = c.rows().numpy()
    assert np.abs(got[2, :3] - [3.0, 3.0, 1.0]).max() <= 1e-12 and got[2, 3:6].max() < 1e-12       # the 4th value of (3, 3, 1, 0 ...)
    assert np.all(got[0, 3:6] == 0.0) and np.all(got[0, 9:12] == 0.0) and np.all(got[0, :3] > 1.0)
    assert np.all(got[1, :13] == 0.0) and not np.isnan(got[:, :13]).any()


@pytest.mark.parametrize("block,k", [(16, 16), (4, 4), (12, 3)])
def test_parity_at_other_block_widths(block, k):
    """k = b; the 16-column kernels; a block wider than 8 that is not 16."""
    c = Case(block, k, names=["gap70x4097", "gap16x27", "gap3x27", "gap1x13", "rnd9x255", "rnd130x7", "rank3_10x7", "zero5x9"])
    check_parity(c, c.rows().numpy(), c.reference())


def same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_two_runs_agree_and_an_item_does_not_depend_on_its_table(case):
    again = case.rows()
    assert same_bits(again, torch.from_numpy(case.got))
    back = case.rows(case.names[::-1])
    assert same_bits(back.flip(0), again)
    for i, n in enumerate(case.names):
        assert same_bits(case.rows([n])[0], again[i]), n
    some = [case.names[j] for j in (5, 0, 9, 2)]
    mixed = case.rows(some)
    for j, n in enumerate(some):
        assert same_bits(mixed[j], again[case.names.index(n)]), n


def test_iterations_compose(case):
    assert same_bits(case.rows(iters=(4, 4)), torch.from_numpy(case.got))
    assert same_bits(case.rows(iters=(1, 0, 7)), torch.from_numpy(case.got))


def test_reset_puts_the_start_blocks_back(case):
    mon = case.monitor()
    mon.update(3).reset().update(ITERS)
    mon.snapshot(0)
    assert same_bits(mon.read()[0], torch.from_numpy(case.got))
    mon.reset()
    with pytest.raises(RuntimeError, match="no iteration"):
        mon.snapshot(0)


def test_inputs_are_left_alone_and_canaries_survive(case):
    flat0 = case.flat.clone()
    uv0 = {n: (u.clone(), v.clone()) for n, (u, v) in case.uv.items()}
    mon = case.monitor(rows=3)
    n, width = len(case.names), 2 * case.k + 2
    guard = torch.full((5, n, width), -123.25, dtype=torch.float64, device=case.flat.device)
    mon.ring = guard[1:4]                                                # the ring, one row of canaries on either side
    mon.update(ITERS)
    assert mon.snapshot(1) == 1
    host = guard.cpu()
    assert same_bits(host[2], torch.from_numpy(case.got))
    assert bool((host[[0, 1, 3, 4]] == -123.25).all())
    assert mon.snapshot() == 0 and mon.snapshot() == 1 and mon.snapshot() == 2 and mon.snapshot() == 0       # the ring wraps
    host = guard.cpu()
    assert bool((host[[0, 4]] == -123.25).all()) and all(same_bits(host[r], host[2]) for r in (1, 3))
    with pytest.raises(ValueError, match="row"):
        mon.snapshot(3)
    assert torch.equal(case.flat.view(torch.int32), flat0.view(torch.int32))
    for name, (u, v) in case.uv.items():
        assert torch.equal(u.view(torch.int32), uv0[name][0].view(torch.int32)), name
        assert torch.equal(v.view(torch.int32), uv0[name][1].view(torch.int32)), name


def test_top_singular_values_is_a_pure_function(case):
    from dvd_gan_amd.spectral import top_singular_values
    names = [f"gap{h}x{w}" for h, w in GAPPED]
    before = torch.get_rng_state()
    sv, res = top_singular_values([case.W[n] for n in names], k=3, iters=8)
    sv2, res2 = top_singular_values([case.W[n] for n in names], k=3, iters=8)
    assert torch.equal(before, torch.get_rng_state())
    assert same_bits(sv, sv2) and same_bits(res, res2) and tuple(sv.shape) == (5, 3) == tuple(res.shape)
    for i, n in enumerate(names):
        s = np.linalg.svd(case.host[n].astype(np.float64), compute_uv=False)
        truth = np.zeros(3)
        truth[:min(3, len(s))] = s[:3]
        assert np.abs(sv[i].numpy() - truth).max() <= 1e-8 * s[0], n
    # a conv weight is viewed [shape[0], -1]
    w4 = case.W["rnd64x576"].view(64, 64, 3, 3)
    a, _ = top_singular_values([w4], iters=4)
    b, _ = top_singular_values([case.W["rnd64x576"]], iters=4)
    assert same_bits(a, b)

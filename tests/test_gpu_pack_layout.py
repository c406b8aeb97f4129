"""conv_pack.hip and layout.hip against torch, bit for bit: the operand packs of a master weight (sigma, co_off, ci_off, the zero
padding of both images), their batched forms beyond one launch (more than 24 fills / 32 fragment-major images), the
fragment-major image against a restatement of its documented layout, to_cl / from_cl with the frame swap, and dvd_convert's scalar
tail.  Everything else in the suite sees these kernels only through convolution results and whole-network fixtures.

Expectation everywhere: torch.equal.  The pack divides by sigma with ONE fp32 division (correctly rounded: the library is not
built with fast-math; the expected value is formed on the CPU) and casts with the round-to-nearest-even that
tests/test_gpu_conv.py::test_f32_to_bf16_is_round_to_nearest_even pins; the other kernels only move or cast values."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
KS = {1: (1, 1), 9: (3, 3), 25: (5, 5), 27: (3, 3, 3)}


def pad8(c):
    return (c + 7) // 8 * 8


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def same(a, b):
    """bit equality (also tells -0.0 from 0.0, which torch.equal on floats does not)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def garbage(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * 37.0 + 5.0).to(dtype)


def expected_packs(w, sigma, dtype, cin, ci_off, cip):
    """w: master [co][ci_tot][*k] (device) -> (wf rows [ntaps][co][cip], wd slabs [ntaps][cip][co]) of this fill, formed on the CPU:
    one IEEE fp32 division, RNE cast, zeros in the padded input channels."""
    wc = w.detach().cpu()
    co, ntaps = wc.shape[0], wc[0, 0].numel()
    v = wc.reshape(co, wc.shape[1], ntaps)[:, ci_off:ci_off + cin]
    if sigma is not None:
        v = v / sigma.detach().cpu()
    wf = torch.zeros(ntaps, co, cip)
    wf[:, :, :cin] = v.permute(2, 0, 1)
    wf = wf.to(dtype)
    wd = wf.flip(0).transpose(1, 2).contiguous()          # wd[ntaps - 1 - tap][ci][co]
    return wf.to(DEV), wd.to(DEV)


@pytest.mark.parametrize("ntaps", [1, 9, 25, 27])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_pack_through_packedconv(dtype, ntaps):
    """PackedConv allocated with zeros, one fill: wf[tap][co][ci] = cast(w[co][ci][tap] / sigma), zero for Cin <= ci < Cip;
    wd[ntaps-1-tap][ci][co] the same values, zero in the padded output columns.  Cin 3, 8, 13; with and without sigma."""
    from dvd_gan_amd import kern as K
    ks, cout = KS[ntaps], 10
    g = torch.Generator(device=DEV).manual_seed(ntaps)
    for cin in (3, 8, 13):
        for sigma in (None, torch.tensor(0.7315, device=DEV)):
            w = torch.randn(cout, cin, *ks, device=DEV, generator=g)
            pk = K.PackedConv(dtype, cout, cin, ks, DEV).fill(w, sigma=sigma)
            wf, wd = expected_packs(w, sigma, dtype, cin, 0, pad8(cin))
            assert same(pk.wf, wf), (cin, sigma)
            assert same(pk.wd[:, :, :cout], wd), (cin, sigma)
            assert not bool(pk.wd[:, :, cout:].any())


@pytest.mark.parametrize("ntaps", [1, 9, 25, 27])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_fused_pack_on_garbage_prefilled_buffers(dtype, ntaps):
    """The library directly: three fills at co_off 0, h, 2h of a [3h + 2]-row pack, each from input channels [ci_off, ci_off + Cin)
    of a wider master, with sigma; the buffers start as garbage.  Rows [3h, 3h + 2) of wf and columns [3h, Cop) of wd, which no fill
    addressed, keep their prefill; everything addressed is written, zeros in the padded input channels included."""
    from dvd_gan_amd import lib as L
    ks = KS[ntaps]
    k3 = (1,) * (3 - len(ks)) + ks
    g = torch.Generator(device=DEV).manual_seed(100 + ntaps)
    for cin, h, ci_off in ((3, 5, 2), (8, 8, 4), (13, 6, 7)):
        cip, rows = pad8(cin), 3 * h + 2
        cop = pad8(rows)
        wf0, wd0 = garbage((ntaps, rows, cip), dtype, 1), garbage((ntaps, cip, cop), dtype, 2)
        wf, wd = wf0.clone(), wd0.clone()
        sigma = torch.tensor(1.377, device=DEV)
        ws = [torch.randn(h, ci_off + cin + 3, *ks, device=DEV, generator=g) for _ in range(3)]
        for i, w in enumerate(ws):
            L.check(L.lib().dvd_pack_conv_weight(L.dt(wf), L.ptr(w), L.ptr(sigma), h, cin, ntaps, cip, i * h, rows, cop, L.ptr(wf), L.ptr(wd),
                                                 k3[0], k3[1], k3[2], ci_off, w.shape[1], L.stream()))
        for i, w in enumerate(ws):
            ef, ed = expected_packs(w, sigma, dtype, cin, ci_off, cip)
            assert same(wf[:, i * h:(i + 1) * h], ef), (cin, i)
            assert same(wd[:, :, i * h:(i + 1) * h], ed), (cin, i)
        assert same(wf[:, 3 * h:], wf0[:, 3 * h:])
        assert same(wd[:, :, 3 * h:], wd0[:, :, 3 * h:])


def fragment_major_restated(w):
    """[ntaps][Cout][C] -> the image as include/dvdgan_hip.h and the head of conv_gb.hip describe it: records [tap][32-channel chunk]
    [32-column block, padded to whole 128-column tiles][k-half pair kk][lane l][8 channels]; lane l holds channels
    chunk * 32 + (2 kk + (l >> 5)) * 8 .. + 7 of output column nb * 32 + (l & 31); zeros wherever the column or channel does not exist."""
    ntaps, cout, c = w.shape
    kch, nb32 = (c + 31) // 32, (cout + 127) // 128 * 4
    wp = torch.zeros(ntaps, nb32 * 32, kch * 32, dtype=w.dtype, device=w.device)
    wp[:, :cout, :c] = w
    v = wp.view(ntaps, nb32, 32, kch, 2, 2, 8)            # tap, nb, l & 31, chunk, kk, l >> 5, channel
    return v.permute(0, 3, 1, 4, 5, 2, 6).contiguous().view(-1)


@pytest.mark.parametrize("cout", [24, 128, 136])
def test_fragment_major_image_equals_its_documented_layout(cout):
    from dvd_gan_amd import lib as L
    for c in (8, 32, 40):
        for ntaps in (1, 9):
            w = garbage((ntaps, cout, c), BF, cout + c)
            want = fragment_major_restated(w)
            nbytes = L.lib().dvd_conv_fragment_major_bytes(ntaps, cout, c)
            assert nbytes == want.numel() * 2
            q = garbage((nbytes // 2,), BF, 9)
            L.check(L.lib().dvd_conv_fragment_major(L.BF16, L.ptr(w), L.ptr(q), ntaps, cout, c, L.stream()))
            assert same(q, want), (c, ntaps)
            assert int((want == 0).sum()) >= want.numel() - w.numel()           # (the padded positions are there)


# cin, hid, k of six tiny ConvGRU layers: 6 fills and 6 images (wf and wd of the x, [u|r] and out-gate packs) each
GRU_LAYERS = [(3, 8, 3), (8, 16, 5), (16, 24, 3), (13, 8, 5), (24, 16, 3), (8, 24, 5)]


def _gru_weights(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [[torch.randn(hid, cin + hid, k, k, device=DEV, generator=g) for _ in range(3)] for cin, hid, k in GRU_LAYERS]


@pytest.mark.parametrize("dtype", [BF, F32])
def test_batched_packs_of_six_convgru_layers(dtype):
    """One PackBatch with 36 fills and (bf16) 36 fragment-major images -- two launches of each batched kernel (24 + 12 fills,
    32 + 4 images): every wf, wd, wfq, wdq equals the same pack built item by item."""
    from dvd_gan_amd import functional as Fn, kern as K
    weights = _gru_weights(5)
    pb = K.PackBatch()
    batched = [Fn._gru_packs(*w3, dtype, DEV, pb) for w3 in weights]
    if dtype == BF:
        for packs in batched:
            for pk in packs:
                pb.fragment_major(pk, "wf")
                pb.fragment_major(pk, "wd")
    assert len(pb.fills) == 36 and len(pb.frags) == (36 if dtype == BF else 0)
    pb.run()
    single = [Fn._gru_packs(*w3, dtype, DEV) for w3 in weights]
    for pb_packs, one_packs in zip(batched, single):
        for a, b in zip(pb_packs, one_packs):
            assert same(a.wf, b.wf) and same(a.wd, b.wd)
            if dtype == BF:
                assert same(a.wfq, b.fragment_major("wf")) and same(a.wdq, b.fragment_major("wd"))


@pytest.mark.parametrize("n", [24, 25, 32, 33])
def test_batched_packs_at_the_launch_boundaries(n):
    """n fills and n images in one PackBatch: exactly one launch, one item into the second launch, for both batched kernels."""
    from dvd_gan_amd import kern as K
    g = torch.Generator(device=DEV).manual_seed(n)
    ws = [torch.randn(8 + i % 3, 5 + i % 7, 3, 3, device=DEV, generator=g) for i in range(n)]
    sig = torch.tensor(0.9, device=DEV)
    pb = K.PackBatch()
    got = []
    for i, w in enumerate(ws):
        pk = K.PackedConv(BF, w.shape[0], w.shape[1], (3, 3), DEV)
        pb.fill(pk, w, sigma=sig if i % 2 else None)
        pb.fragment_major(pk, "wf")
        got.append(pk)
    assert len(pb.fills) == n and len(pb.frags) == n
    pb.run()
    for i, (w, pk) in enumerate(zip(ws, got)):
        one = K.PackedConv(BF, w.shape[0], w.shape[1], (3, 3), DEV).fill(w, sigma=sig if i % 2 else None)
        assert same(pk.wf, one.wf) and same(pk.wd, one.wd), i
        assert same(pk.wfq, one.fragment_major("wf")), i


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("sp", [(5, 7), (2, 3, 5)])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_channels_last_round_trip_and_frame_swap(dtype, sp):
    """to_cl = permute + zero pad + cast, from_cl its inverse; swap = (A, B), A != B: source frame (a, b) <-> internal frame (b, a).
    F * P = 210 / 180 positions: not a multiple of the 256-thread block."""
    from dvd_gan_amd import kern as K
    A, B = 2, 3
    g = torch.Generator(device=DEV).manual_seed(len(sp))
    for c in (3, 8, 13):
        x = torch.randn(A * B, c, *sp, device=DEV, generator=g)
        cl = K.to_cl(x, dtype)
        want = torch.zeros(A * B, *sp, pad8(c), device=DEV, dtype=dtype)
        want[..., :c] = x.movedim(1, -1).to(dtype)
        assert same(cl, want), c
        assert not bool(cl[..., c:].any())
        back = K.from_cl(cl, c)
        assert back.dtype == F32 and same(back, x if dtype == F32 else x.to(BF).float())
        # a-major source frames written b-major
        sw = K.to_cl(x, dtype, swap=(A, B))
        want_sw = want.view(A, B, *want.shape[1:]).transpose(0, 1).reshape(want.shape)
        assert same(sw, want_sw), c
        assert same(K.from_cl(sw, c, swap=(A, B)), back)              # a swapped round trip is the identity


@pytest.mark.parametrize("n", [3, 8, 8 * 300 + 5])
def test_convert_scalar_tail(n):
    """Lengths that are no multiple of 8: the last thread converts element by element.  All four dtype pairs, bit-equal to torch's
    cast; the destination past n is untouched."""
    from dvd_gan_amd import kern as K, lib as L
    g = torch.Generator(device=DEV).manual_seed(n)
    for sdt in (F32, BF):
        src = (torch.randn(n, device=DEV, generator=g) * 3.0).to(sdt)
        for ddt in (F32, BF):
            assert same(K.convert(src, ddt), src.to(ddt)), (sdt, ddt)
            dst0 = garbage((n + 11,), ddt, 3)
            dst = dst0.clone()
            L.check(L.lib().dvd_convert(L.dt(src), L.ptr(src), L.dt(dst), L.ptr(dst), C.c_longlong(n), L.stream()))
            assert same(dst[:n], src.to(ddt)) and same(dst[n:], dst0[n:]), (sdt, ddt)

"""The weights-from-L2 convolution tiles (conv_gb.hip) on v_mfma_f32_16x16x32_bf16, through kern.conv_forward with a
fragment-major image: the operand maps exactly (one-hot inputs, no tolerance), the ragged edges against float64, and the
in-launch split-K combine on the new accumulator order.

One-hot lane map: the input is zero except 1.0 at one (frame, pixel, channel) and the weights are
w[co][ci][tap] = bf16(1 + (co mod 7)/8 + (ci mod 5)/64 + tap/512), so every output the filter reaches IS one weight (under the
nearest x2 upsample: the exact fp32 sum of the up to four weights whose taps see a copy of the hot pixel) and every other output
is zero: a permuted K group, a swapped half of a sub-tile, a wrong column block or a wrong row of the staged epilogue image shows
as a different weight or a misplaced one.
"""
import pytest
import torch

import test_gpu_gru as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _variants(fn):
    """fn() with the library's per-launch records on -> (result, kernel variants seen)."""
    L, lib = G._lib()
    torch.cuda.synchronize()
    G._drain(lib)
    lib.dvd_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.dvd_prof_enable(0)
        seen = G._drain(lib)
    return out, seen


# name: frames, S (output side), C, Cout, up2, kernel variant (csrc/prof.h: 1 / 2 / 3 = halo 256 x 128 / 128 x 128 / 256 x 64,
# 7 / 8 = whole frames on 256- / 128-row tiles)
TILES = {
    "halo256x128": (64, 32, 64, 256, False, 1),
    "halo128x128": (2, 16, 64, 128, False, 2),
    "halo128x128-up2": (2, 16, 64, 128, True, 2),
    "halo256x64": (128, 64, 64, 64, False, 3),
    "halo256x64-up2": (128, 64, 64, 64, True, 3),
    "frame8": (4, 8, 64, 128, False, 8),
    "frame8-256": (2048, 8, 64, 128, False, 7),
    "frame4": (8, 4, 64, 128, False, 8),
}
HOT_CHANNELS = (3, 13, 16, 31, 32, 42, 55, 57)      # one per 8-channel slot of both 32-channel chunks of C = 64


def _hot_pixels(F_, S):
    """(frame, y, x) on the OUTPUT grid: both lines of a sub-tile, a patch corner, frame corners, the last frame."""
    m = S - 1
    pts = [(0, 0, 0), (0, 1, min(5, m)), (0, min(2, m), min(9, m)), (0, min(3, m), m), (0, m, 0), (F_ - 1, m, m), (F_ // 2, S // 2, S // 2 - 1)]
    if S > 16:
        pts += [(1, 15, 15), (1, 16, 16), (F_ - 1, 17, 4)]
    return pts


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("tile", list(TILES))
def test_one_hot_lane_map(tile, k):
    from dvd_gan_amd import kern as K
    F_, S, Cin, Cout, up2, variant = TILES[tile]
    Sin = S // 2 if up2 else S
    co, ci, tap = torch.arange(Cout).view(-1, 1, 1), torch.arange(Cin).view(1, -1, 1), torch.arange(k * k).view(1, 1, -1)
    w = (1.0 + (co % 7) / 8.0 + (ci % 5) / 64.0 + tap / 512.0).to(BF).float().view(Cout, Cin, k, k).contiguous()
    pk = K.PackedConv(BF, Cout, Cin, (k, k), DEV).fill(w.to(DEV))
    wq = pk.fragment_major("wf")
    assert K.wants_fragment_major(BF, F_, S, S, Cin, Cout, k) or up2
    wd = w.to(DEV)
    pad = k // 2
    x = torch.zeros(F_, Sin, Sin, Cin, device=DEV, dtype=BF)
    hots = [(f, y, xx, c) for (f, y, xx), c in zip(_hot_pixels(F_, S) * 2, HOT_CHANNELS * 3)]
    hots += [(0, 1, min(5, S - 1), c) for c in HOT_CHANNELS]
    first = True
    for f, y, xx, c in hots:
        yi, xi = (y // 2, xx // 2) if up2 else (y, xx)
        x[f, yi, xi, c] = 1.0
        if first:
            got, seen = _variants(lambda: K.conv_forward(x, pk.wf, (k, k), Cout, up2=up2, out_f32=True, wq=wq))
            assert seen == {variant}, (tile, k, sorted(seen))
            first = False
        else:
            got = K.conv_forward(x, pk.wf, (k, k), Cout, up2=up2, out_f32=True, wq=wq)
        x[f, yi, xi, c] = 0.0
        want = torch.zeros(F_, S, S, Cout, device=DEV)
        # output (oy, ox) reads the (upsampled) input at (oy + iy - pad, ox + ix - pad)
        for iy in range(k):
            for ix in range(k):
                for sy in ((0, 1) if up2 else (0,)):
                    for sx in ((0, 1) if up2 else (0,)):
                        oy = (2 * yi + sy if up2 else yi) - iy + pad
                        ox = (2 * xi + sx if up2 else xi) - ix + pad
                        if 0 <= oy < S and 0 <= ox < S:
                            want[f, oy, ox] += wd[:, c, iy, ix]
        assert torch.equal(got, want), (tile, k, (f, y, xx, c), int((got != want).sum()))


def _ref64(x, w, relu_in):
    """x [F, S, S, C] channels-last, w [Cout, C, k, k] -> float64 [F, S, S, Cout]"""
    xd = x.double().permute(0, 3, 1, 2)
    if relu_in:
        xd = xd.clamp_min(0.0)
    return torch.nn.functional.conv2d(xd, w.double(), padding=w.shape[-1] // 2).permute(0, 2, 3, 1)


RAGGED = [  # frames, S, C, Cout, k, relu_in, nsplit
    (13, 16, 40, 8, 3, False, 1), (13, 16, 8, 40, 5, True, 1), (61, 16, 40, 72, 3, False, 1), (13, 32, 72, 40, 5, False, 2),
    (61, 8, 40, 72, 3, True, 1), (13, 8, 8, 8, 5, False, 1), (61, 8, 72, 40, 3, False, 2),
    (13, 4, 40, 72, 5, True, 2), (61, 4, 8, 40, 3, False, 1), (61, 4, 40, 8, 3, False, 1),
]


@pytest.mark.parametrize("case", RAGGED)
def test_ragged_edges_against_float64(case):
    """Cout with its last 16-column block partly or wholly past Cout, K groups past C, frame counts that leave an M tail, ReLU on
    the fragments and two K slices with slabs: rel-L2 <= 2e-6 against float64 on the bf16 operands (fp32 output: only the
    summation order differs)."""
    from dvd_gan_amd import kern as K
    F_, S, Cin, Cout, k, relu, ns = case
    g = torch.Generator(device=DEV).manual_seed(sum(case))
    x = torch.randn(F_, S, S, K.pad8(Cin), generator=g, device=DEV).to(BF)
    w = (torch.randn(Cout, Cin, k, k, generator=g, device=DEV) / (Cin * k * k) ** 0.5).to(BF).float().contiguous()
    pk = K.PackedConv(BF, Cout, Cin, (k, k), DEV).fill(w)
    wq = pk.fragment_major("wf")
    assert K.wants_fragment_major(BF, F_, S, S, K.pad8(Cin), Cout, k, ns)
    got = K.conv_forward(x, pk.wf, (k, k), Cout, relu_in=relu, out_f32=True, nsplit=ns, slabs=ns > 1, wq=wq)
    want = _ref64(x[..., :Cin], w, relu)
    if ns > 1:
        got = got.double().sum(0).view(F_, S, S, Cout)
    else:
        assert not bool(got[..., Cout:].any()), "padded output channels must stay zero"
        got = got[..., :Cout]
    r = rel(got, want)
    print(f"ragged {case}: rel-L2 {r:.3e}")
    assert r <= 2e-6, (case, r)


# two ConvGRU steps per frame size (the second reads the first's stored state) with enough channel chunks for four K slices
# (the halo / whole-frame tiles split over chunks only)
G.CASES.update({116: (3, 16, 16, 128, 3, 2), 104: (24, 4, 4, 128, 3, 2)})


@pytest.mark.parametrize("case", [116, 104])
def test_split_k_combine_in_launch(case):
    """nsplit 2, 3, 4 combined in-launch (route b) on the 16 x 16 halo tile and the 4 x 4 whole-frame tile: the same bits on five
    repeats whichever workgroup arrives last, and, like the slabs + gate-kernel route (a) at the same factor, inside the float64
    bounds of tests/test_gpu_gru.py (the two routes add the slices in a different fp32 order)."""
    ly = G.Layer(case, BF)
    for cap in (2, 3, 4):
        name = f"mfma16 combine case{case} ns_cap {cap}"
        oa, seen_a, full_a = G.run_layer(ly, dict(G.ROUTES["a"], ns_cap=cap), True)
        G.check_layer(name + " route a", ly, oa, full_a)
        ob, seen_b, full_b = G.run_layer(ly, dict(G.ROUTES["b"], ns_cap=cap), True)
        assert (2 if case == 116 else 8) in seen_b, (name, sorted(seen_b))
        G.check_layer(name + " route b", ly, ob, full_b)
        for _ in range(4):
            o2, _, _ = G.run_layer(ly, dict(G.ROUTES["b"], ns_cap=cap), True)
            for key in G.STORED:
                assert torch.equal(G.R.bits(ob[key]), G.R.bits(o2[key])), f"{name}: {key} is not reproducible"

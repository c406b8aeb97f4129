"""The direct epilogue of the forward / backward-data convolution kernels (conv_epilogue of csrc/conv_common.h, the epilogues of
csrc/conv_thin.hip) ELEMENTWISE against float64 (tests/conv_ref.py: forward_ref, check_forward), on the kernels training runs:
every call goes through kern.conv_forward with wq=lambda: pk.fragment_major(...), as functional.Conv calls it, so bf16 requests
land on the weights-from-L2 halo tiles, the whole-frame tiles and the thin kernels, and the kernel variant of every case is
asserted from the library's per-launch records.

Operands (conv_ref.make_request): inputs, residuals and masks drawn in the storage type, weights through kern.PackedConv.fill
from a master already rounded to it, fixed seeds.  Every buffer is WIDER than the request needs: out has ldo = pad8(Cout) + 8 and
is prefilled with sentinel bytes inside an arena with sentinel gaps (tests/test_gpu_gru.py: Arena), the residual has
ldres = pad8(Cout) + 16 and the mask ldmask = pad8(Cout) + 24, their extra columns holding finite poison 2^10 times the data's
scale (the convention of tests/test_gpu_wgrad_strided.py).  The mask carries +0, -0, +-2^-126 and +-inf in every 8-column group of
every fourth row, so `mask > 0` is decided at its edge in every sub-tile.  (A pool2 request allocates its own output in
kern.conv_forward: no sentinel columns there.)

Per (case, kind), conv_ref.check_forward:
  1 zero-input   x = 0, no activation or ReLU: the fp32 output is torch.equal to bias + res (ReLU, mask; 4 bias under pool2) formed
                 by the same few fp32 torch ops -- a misaddressed bias column, residual row or mask row is a bit mismatch
  2 fp64         random input: the fp32 output within the derived bound (ratio <= 1), masked-out and padded elements exactly 0
  3 storage      the same request with out_f32=False is torch.equal to the fp32 output rounded by torch
  4 untouched    sentinel columns and gaps intact, the columns [Cout, pad8(Cout)) zero although the buffer was not zero-filled
and here 5: a second fp32 run is bit-equal (the direct epilogue has no atomics).

Kinds: res (bias + residual), res_up2 (bias + residual on the half-size grid), relu / tanh / sigmoid (bias + residual + activation
+ mask), bwd (the backward-data request: the `wd` image, no bias, a mask, a residual `partner`, Cout = pk.cip), pool2 / pool2_bias
(2 x 2 sums, mask on the half grid).  The thin kernels take no residual (a request with one is not theirs), thin-input takes ReLU
only, thin-output ReLU and tanh; pool2 is served by the halo tiles only (dvd_conv_pool2_ok).

profiles/conv_epilogue_numbers.md has the variants seen and the measured ratios.
"""
import pytest
import torch

import conv_ref as R
import test_gpu_gru as G
from test_gpu_mfma16 import _variants

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
assert R.SENT == G.SENT

# name: (frames, output side S, Cin, Cout, k, up2, relu_in), kernel variant in bf16 mode (csrc/prof.h: 1 / 2 / 3 = halo 256 x 128 /
# 128 x 128 / 256 x 64, 4 / 5 = tap-by-tap 128 x 128 / 256 x 128, 7 / 8 = whole frames on 256- / 128-row tiles, 9 = thin).  The
# smallest shapes at which cv_choose_kernel (csrc/conv_igemm.hip) still picks the family.
CASES = {
    "halo256x128": ((64, 32, 64, 132, 3, False, False), 1),          # two N tiles, the last 8-column group has 4 valid columns
    "halo256x128-k5-relu": ((64, 32, 64, 132, 5, False, True), 1),
    "halo128x128": ((2, 16, 64, 72, 3, False, False), 2),
    "halo128x128-k5": ((2, 16, 64, 128, 5, False, False), 2),
    "halo128x128-up2-relu": ((2, 16, 64, 128, 3, True, True), 2),
    "halo256x64": ((128, 32, 32, 40, 3, False, False), 3),           # 512 tiles: the threshold of the 256 x 64 tile
    "halo256x64-up2": ((128, 32, 32, 40, 3, True, False), 3),        # input 16 x 16
    "frame8": ((5, 8, 64, 72, 3, False, False), 8),                  # M tail, two frames per tile
    "frame8-256": ((2049, 8, 32, 72, 3, False, False), 7),           # 513 tiles, the last holds one frame of four
    "frame4": ((13, 4, 40, 72, 5, False, False), 8),                 # eight frames per tile, tail
    "thin-in-32": ((3, 32, 3, 64, 3, False, False), 9),              # 3 (stored as 8) -> 64 channels, rows of 32 pixels
    "thin-in-64": ((2, 64, 3, 64, 3, False, False), 9),
    "thin-out": ((3, 32, 64, 3, 3, False, False), 9),
    "tap128-1x1": ((2, 16, 64, 72, 1, False, False), 4),
    "tap128-odd": ((2, 12, 24, 40, 3, False, False), 4),             # extents that are no power of two: division indexing
    "tap256": ((57, 48, 16, 24, 3, False, False), 5),
    # a last 8-column group with 5 / 5 / 4 / 3 valid columns on the other tiles: the padded channels are written as zeros there too
    "halo128x128-ragged": ((2, 16, 64, 69, 3, False, False), 2),
    "halo256x64-ragged": ((128, 32, 32, 37, 3, False, False), 3),
    "frame8-ragged": ((5, 8, 64, 68, 3, False, False), 8),
    "tap128-ragged": ((2, 12, 24, 35, 3, False, False), 4),
}
NAMES = {BF: "bf16", F32: "fp32"}


def _kinds(name):
    case, variant = CASES[name]
    if name.startswith("thin-in"):
        return ["relu", "bwd"]
    if name == "thin-out":
        return ["relu", "tanh", "bwd"]
    kinds = ["res", "res_up2", "relu", "tanh", "sigmoid"]
    if not (case[5] or case[6]):               # a backward-data request carries neither an upsample nor an input ReLU
        kinds.append("bwd")
        if variant in (1, 2, 3):
            kinds += ["pool2", "pool2_bias"]
    return kinds


def _rows(name):
    F_, S = CASES[name][0][:2]
    return F_ * S * S


PARAMS = [(n, k, BF) for n in CASES for k in _kinds(n)]
# exact mode: the cases of at most 65536 rows as well (they take the LDS-staged / tap-by-tap kernels; the variant is recorded)
PARAMS += [(n, k, F32) for n in CASES if _rows(n) <= 65536 for k in _kinds(n)]


@pytest.mark.parametrize("name,kind,dtype", PARAMS, ids=[f"{n}-{k}-{NAMES[d]}" for n, k, d in PARAMS])
def test_direct_epilogue(name, kind, dtype):
    from dvd_gan_amd import kern as K
    case, variant = CASES[name]
    F_, S, cin, cout, k, up2, relu_in = case
    thin = name.startswith("thin")
    seed = 1000 * list(CASES).index(name) + R.KINDS.index(kind)
    rq = R.make_request(case, kind, dtype, DEV, seed, with_res=not thin)
    req = rq["req"]
    pk = K.PackedConv(dtype, *rq["pack"], (k, k), DEV).fill(rq["master"])
    wpack = getattr(pk, rq["which"])
    co = rq["w"].shape[0]                      # the request's Cout ("bwd": pk.cip)
    assert kind != "bwd" or co == pk.cip
    So = S // 2 if req["pool2"] else S
    shape = (F_, So, So, R.pad8(co) + 8)
    ar = G.Arena([(b, shape, dt, 0) for b, dt in (("o32", F32), ("ost", dtype), ("z32", F32), ("again", F32))])
    ar.raw.fill_(G.SENT)                       # the buffers start as sentinel bytes too: nothing here was zero-filled

    def call(x, buf, f32, act=req["act"]):
        y = K.conv_forward(x, wpack, (k, k), co, bias=req.get("bias"), res=req.get("res"), mask=req.get("mask"), act=act,
                           up2=up2, relu_in=relu_in, res_up2=req["res_up2"], pool2=req["pool2"], out_f32=f32,
                           out=None if req["pool2"] else ar.t[buf], wq=lambda: pk.fragment_major(rq["which"]))
        assert y is not None, "the request was not served"
        return y

    o32, seen = _variants(lambda: call(rq["x"], "o32", True))
    label = f"{name} {kind} {NAMES[dtype]}"
    print(f"VARIANT {label}: {sorted(seen)}")
    if dtype == BF:
        assert seen == {variant}, (label, sorted(seen))
    ost = call(rq["x"], "ost", False)
    z32 = call(torch.zeros_like(rq["x"]), "z32", True, act=R.zero_pass_act(req["act"]))
    again = call(rq["x"], "again", True)
    assert torch.equal(R._bytes(o32), R._bytes(again)), f"{label}: check 5 rerun: the fp32 output is not reproducible"
    r = R.check_forward(label, dtype, rq["x"], rq["w"], o32, ost, zero32=z32, gaps_intact=ar.intact(), **req)
    assert r <= 1.0

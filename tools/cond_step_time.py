"""Frame-conditional prediction step (Trainer with config.n_cond = K) against the random-state hook bench.py --state-carry times,
at BASELINE configs[4]'s shape, plus the split of the added time and the kernel that serves each conditioning-encoder convolution.

usage: python tools/cond_step_time.py [--steps N] [--warmup W] [--batch B] [--ch C] [--frames T] [--n-cond K] [--size S]
Prints one JSON line per measurement:
  step       ms per train_step (HIP events around N steps after W warm-up steps, one Trainer per mode, same seeds):
             "cond" = clips [B, 3, K+T, S, S], the encoder feeding the twelve states; "carry" = clips [B, 3, T, S, S] and random
             states that require grad (what bench.py --state-carry times)
  parts      the added work in isolation: encoder forward + backward at batch B; D_t forward + backward on K+T against T frames
  encoder    one bf16 forward + backward of the encoder with the library's per-launch records (dvd_prof_enable): every
             convolution launch with its shape and the kernel variant that served it
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd import lib as L                      # noqa: E402
from dvd_gan_amd.train_step import Trainer           # noqa: E402

VARIANTS = {0: {1: "conv_halo_gb 256x128", 2: "conv_halo_gb 128x128", 3: "conv_halo_gb 256x64", 4: "conv_igemm 128x128",
                5: "conv_igemm 256x128", 6: "conv_igemm 256x256", 7: "conv_halo_gbs whole-frame 256x128 (4x4 / 8x8 frames)",
                8: "conv_halo_gbs whole-frame 128x128 (4x4 / 8x8 frames)", 9: "conv_thin_in"},
            1: {1: "conv_wgrad_row (filter rows)", 2: "conv_wgrad (one tap)", 3: "wgrad_thin", 4: "conv_wgrad_row4"}}


def cfg(a, n_cond):
    return argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                              lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                              beta2=0.9, n_class=101, k_sample=8, n_cond=n_cond)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def step_time(a, mode):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    K = a.n_cond if mode == "cond" else 0
    tr = Trainer([], cfg(a, K), device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16)
    gen = torch.Generator().manual_seed(1)
    real = (torch.rand(a.batch, 3, K + a.frames, a.size, a.size, generator=gen) * 2 - 1).to(dev)
    labels = torch.randint(0, 101, (a.batch,), generator=gen).to(dev)
    tr.register_label_buffer(labels)
    hidden = None
    if mode == "carry":
        c8, c4, ld = 8 * a.ch, 4 * a.ch, a.size // 16
        hidden = [[torch.randn(a.batch, h, s, s, device=dev, requires_grad=True) for h in (c, 2 * c, c)]
                  for c, s in ((c8, ld), (c8, 2 * ld), (c8, 4 * ld), (c4, 8 * ld))]
    torch.manual_seed(100)
    ms = timed(lambda: tr.train_step(real, labels, hidden=hidden), a.steps, a.warmup)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    del tr, real, hidden
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return ms, peak


def parts(a):
    from dvd_gan_amd.cond_encoder import FrameEncoder
    from dvd_gan_amd.disc_nets import TemporalDiscriminator
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    enc = FrameEncoder(a.n_cond, a.size // 16, a.ch, torch.bfloat16).to(dev)
    cond = torch.rand(a.batch, a.n_cond, 3, a.size, a.size, device=dev) * 2 - 1

    def enc_step():
        states = enc(cond)
        sum(h.float().mean() for hs in states for h in hs).backward()
    out = {"encoder_fwd_bwd_ms": round(timed(enc_step, a.steps, a.warmup), 2)}
    del enc
    Dt = TemporalDiscriminator(a.ch, 101, torch.bfloat16).to(dev)
    labels = torch.randint(0, 101, (a.batch,), device=dev)
    for T in (a.frames, a.frames + a.n_cond):
        x = (torch.rand(a.batch, 3, T, a.size // 2, a.size // 2, device=dev) * 2 - 1).requires_grad_(True)
        out[f"dt_fwd_bwd_ms_T{T}"] = round(timed(lambda: Dt(x, labels).mean().backward(), a.steps, a.warmup), 2)
    del Dt
    torch.cuda.empty_cache()
    return out


def encoder_kernels(a):
    """One forward + backward of the encoder with every conv launch recorded: which kernel serves which convolution."""
    from dvd_gan_amd.cond_encoder import FrameEncoder
    dev = torch.device("cuda", 0)
    lib = L.lib()
    torch.manual_seed(0)
    enc = FrameEncoder(a.n_cond, a.size // 16, a.ch, torch.bfloat16).to(dev)
    cond = torch.rand(a.batch, a.n_cond, 3, a.size, a.size, device=dev) * 2 - 1
    for _ in range(2):                         # warm: fragment-major weight images requested on the first call
        states = enc(cond)
        sum(h.float().mean() for hs in states for h in hs).backward()
    torch.cuda.synchronize()
    lib.dvd_prof_report_variants.restype = C.c_longlong
    for kind in (0, 1):
        lib.dvd_prof_report_variants(kind, 0, None, None, None)          # drop earlier records
    lib.dvd_prof_enable(1)
    states = enc(cond)
    sum(h.float().mean() for hs in states for h in hs).backward()
    torch.cuda.synchronize()
    lib.dvd_prof_enable(0)
    fd, path = tempfile.mkstemp(suffix=".csv")
    os.close(fd)
    os.environ["DVD_PROF_CSV"] = path
    for kind in (0, 1):
        lib.dvd_prof_report_variants(kind, 0, None, None, None)
    del os.environ["DVD_PROF_CSV"]
    rows = []
    for line in open(path):
        f = line.strip().split(",")
        kind, M, Cin, Cout, taps, split, flags, ms = int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), float(f[7])
        var = int(f[9])
        rows.append({"pass": "fwd/bwd-data" if kind == 0 else "wgrad", "M": M, "C": Cin, "Cout": Cout, "taps": taps, "split": split,
                     "flags": flags, "ms": round(ms, 3), "kernel": VARIANTS[kind].get(var, f"variant {var}")})
    os.unlink(path)
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--frames", type=int, default=12)
    p.add_argument("--n-cond", type=int, default=4)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--what", default="step,parts,encoder")
    a = p.parse_args()
    what = a.what.split(",")
    if "encoder" in what:
        for r in encoder_kernels(a):
            print(json.dumps({"encoder_launch": r}), flush=True)
    if "parts" in what:
        print(json.dumps({"parts": parts(a)}), flush=True)
    if "step" in what:
        res = {}
        for mode in ("carry", "cond"):
            ms, peak = step_time(a, mode)
            res[mode] = {"ms_per_step": round(ms, 2), "peak_gb": round(peak, 1)}
            print(json.dumps({"step": mode, **res[mode]}), flush=True)
        print(json.dumps({"summary": {"cond_over_carry": round(res["cond"]["ms_per_step"] / res["carry"]["ms_per_step"], 4),
                                      "added_ms": round(res["cond"]["ms_per_step"] - res["carry"]["ms_per_step"], 2),
                                      "shape": f"B={a.batch}, K={a.n_cond}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16"}}))


if __name__ == "__main__":
    main()

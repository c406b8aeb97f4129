"""What the generator weight average (config.ema_decay > 0) costs: the optimizer launches in isolation, and the training step.

usage: python tools/ema_step_time.py [--launches N] [--blocks R] [--steps N] [--warmup W] [--repeats R] [--batch B] [--ch C]
                                     [--frames T] [--size S] [--what kernel,step]
Prints one JSON line per measurement:
  kernel     n = the generator's trainable parameter count at --ch, taken from the model.  Per block (R blocks, for the
             spread): dvd_adam_step (what a Trainer without the average launches), dvd_ema_step (a separate averaging pass)
             and dvd_adam_ema_step (the fused launch), one after the other, each N launches between HIP events after 3 warm-up
             launches; ms per launch and GB/s from 28 / 12 / 36 bytes per element.  The summary line compares the fused launch
             with the sum of the other two of the same block.
  step       ms per train_step (a HIP event after every step, --steps steps after --warmup), max_memory_allocated and the device
             segments the caching allocator requested during the timed steps, for three variants: "off" (ema_decay = 0, the step
             bench.py times), "on" (0.9999, the average allocated by the first step) and "on_prealloc" (0.9999, the average handed
             over with load_ema right after construction).  --repeats rounds, the order rotating, EVERY TRAINER IN A CHILD
             PROCESS OF ITS OWN: a Trainer built after another one was torn down in the same process can run 3-8 % slower with
             the same launches (its buffers land elsewhere: cbn_bwd_reduce, conv_halo_gb, conv_group_gbs take longer), whatever
             ema_decay is -- in one process that reads as a cost of whichever variant comes later.  --in-process shows it.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd import kern as K                      # noqa: E402
from dvd_gan_amd.train_step import Trainer           # noqa: E402

BYTES = {"adam": 28, "ema": 12, "adam_ema": 36}        # per element: 4 reads + 3 writes | 2 + 1 | 5 + 4


def cfg(a, ema_decay):
    return argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                              lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                              beta2=0.9, n_class=101, k_sample=8, ema_decay=ema_decay)


def events(fn, launches, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def kernel_level(a):
    from dvd_gan_amd.gen_net import Generator
    with torch.device("meta"):                          # shapes only
        G = Generator(120, a.size // 16, 101, a.ch, a.frames)
    n = sum(p.numel() for p in G.parameters() if p.requires_grad)
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    p, g = (torch.randn(n, generator=gen) * 0.05).to(dev), (torch.randn(n, generator=gen) * 1e-3).to(dev)
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    t = [0]

    def adam():
        t[0] += 1
        K.adam_step(p, g, m, v, 5e-5, 0.0, 0.9, 1e-8, t[0])

    def ema_only():
        K.ema_step(ema, p, 0.9999)

    def fused():
        t[0] += 1
        K.adam_ema_step(p, g, m, v, ema, 5e-5, 0.0, 0.9, 1e-8, t[0], 0.9999)
    blocks = []
    for b in range(a.blocks):
        row = {}
        for name, fn in (("adam", adam), ("ema", ema_only), ("adam_ema", fused)):
            ms = events(fn, a.launches)
            row[name] = {"ms": round(ms, 4), "GBps": round(BYTES[name] * n / ms / 1e6, 1)}
        row["separate_minus_fused_ms"] = round(row["adam"]["ms"] + row["ema"]["ms"] - row["adam_ema"]["ms"], 4)
        blocks.append(row)
        print(json.dumps({"kernel": {"block": b, "n": n, "launches": a.launches, **row}}), flush=True)
    spread = {k: round(max(r[k]["ms"] for r in blocks) - min(r[k]["ms"] for r in blocks), 4) for k in BYTES}
    gains = [r["separate_minus_fused_ms"] for r in blocks]
    print(json.dumps({"kernel_summary": {"n": n, "spread_ms": spread, "separate_minus_fused_ms_min": min(gains),
                                         "separate_minus_fused_ms_max": max(gains),
                                         "fused_beats_two_launches_by_more_than_spread": min(gains) > max(spread.values()),
                                         "fused_minus_adam_ms_max": round(max(r["adam_ema"]["ms"] - r["adam"]["ms"] for r in blocks), 4)}}),
          flush=True)


VARIANTS = {"off": (0.0, False), "on": (0.9999, False), "on_prealloc": (0.9999, True)}


def step_time(a, variant):
    """One Trainer: --warmup steps, then --steps steps with a HIP event between every two (no host sync inside the loop).
    "on_prealloc" hands the optimizer its average right after construction (load_ema(flat)), on the caller's stream, instead of
    letting the first step allocate it.  -> per-step ms, peak GiB, and how many device segments the caching allocator had to
    request from the driver during the timed steps (hipMalloc calls: each one stalls the step)."""
    ema_decay, prealloc = VARIANTS[variant]
    dev = torch.device("cuda", 0)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(0)
    tr = Trainer([], cfg(a, ema_decay), device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16)
    if prealloc:
        tr.g_optimizer.load_ema(tr.g_optimizer.flat)
    gen = torch.Generator().manual_seed(1)
    real = (torch.rand(a.batch, 3, a.frames, a.size, a.size, generator=gen) * 2 - 1).to(dev)
    labels = torch.randint(0, 101, (a.batch,), generator=gen).to(dev)
    tr.register_label_buffer(labels)
    torch.manual_seed(100)
    for _ in range(a.warmup):
        tr.train_step(real, labels)
    torch.cuda.synchronize()
    seg0 = torch.cuda.memory_stats()["segment.all.allocated"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    ev[0].record()
    for i in range(a.steps):
        tr.train_step(real, labels)
        ev[i + 1].record()
    torch.cuda.synchronize()
    per_step = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)]
    segs = torch.cuda.memory_stats()["segment.all.allocated"] - seg0
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    del tr, real
    torch.cuda.empty_cache()
    return per_step, peak, segs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--blocks", type=int, default=3)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--frames", type=int, default=48)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--what", default="kernel,step")
    p.add_argument("--variants", default="off,on,on_prealloc", help="step level: which Trainers, in this order (rotated per repeat)")
    p.add_argument("--in-process", action="store_true", help="step level: all Trainers in THIS process, one after the other")
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=180.0)
    a = p.parse_args()
    what = a.what.split(",")
    if a.one:                                       # child of the step level: one Trainer in this process
        per_step, peak, segs = step_time(a, a.one)
        print(json.dumps({"variant": a.one, "ema_decay": VARIANTS[a.one][0], "ms_per_step": round(sum(per_step) / len(per_step), 2),
                          "per_step_ms": [round(x, 1) for x in per_step], "segments_allocated_in_timed_steps": segs,
                          "peak_gb": round(peak, 2)}), flush=True)
        return
    if "kernel" in what:
        kernel_level(a)
        torch.cuda.empty_cache()
    if "step" in what:
        names = a.variants.split(",")
        res = {v: [] for v in names}
        for r in range(a.repeats):
            for v in names[r % len(names):] + names[:r % len(names)]:          # the order rotates
                if a.in_process:
                    per_step, peak, segs = step_time(a, v)
                    row = {"variant": v, "ema_decay": VARIANTS[v][0], "ms_per_step": round(sum(per_step) / len(per_step), 2),
                           "per_step_ms": [round(x, 1) for x in per_step], "segments_allocated_in_timed_steps": segs,
                           "peak_gb": round(peak, 2)}
                else:
                    # every Trainer in a process of its own: see the module docstring.  A child that fails ends the run.
                    cmd = [sys.executable, os.path.abspath(__file__), "--one", v] + [
                        f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "batch", "ch", "frames", "size")]
                    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout, check=True).stdout.decode()
                    row = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
                res[v].append(row["ms_per_step"])
                print(json.dumps({"step": {"repeat": r, "in_process": bool(a.in_process), **row}}), flush=True)
        mean = {v: sum(x) / len(x) for v, x in res.items()}
        print(json.dumps({"step_summary": {**{v + "_ms": [round(x, 2) for x in res[v]] for v in names},
                                           **{v + "_minus_off_ms_mean": round(mean[v] - mean["off"], 2) for v in names
                                              if v != "off" and "off" in mean},
                                           **{v + "_spread_ms": round(max(res[v]) - min(res[v]), 2) for v in names},
                                           "in_process": bool(a.in_process),
                                           "shape": f"B={a.batch}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16"}}))

if __name__ == "__main__":
    main()

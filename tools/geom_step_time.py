"""What the geometric augmentation of the discriminators' inputs (Trainer with config.d_aug_geom) costs, at the benchmark's
configuration: the training step with it off, on at p = 0, at p = 1 and adaptive, and the two kernels alone on the benchmark's clip
against a device-to-device copy of the same bytes.

usage: python tools/geom_step_time.py [--steps N] [--warmup W] [--batch B] [--ch C] [--frames T] [--size S] [--what step,kernel]
                                      [--modes off,p0,p1,adaptive]
Prints one JSON line per measurement:
  step       ms per train_step (HIP events around N steps after W warm-up steps, same seeds; every Trainer in a child process
             of its own, in the order of --modes, where a name may repeat; the summary gives the range of each difference):
             "off" = d_aug_geom "" (the step of the parent commit: the setting unset changes nothing), "p0" = all five groups at
             p = 0 (the launches, every row the identity), "p1" = at p = 1, "adaptive" = from p = 0.5 with d_aug_target = 0.6
  kernel     us per launch of dvd_geom_clip_forward / dvd_geom_clip_backward on a [B * T, 3, S, S] fp32 clip (HIP events around
             N launches) for the identity row (a copy), a mirror, a rotation by 30 degrees, a magnification by 1.5 (the widest
             backward window of the drawn range) and drawn rows of all groups, with the GB/s of one read and one write of the clip;
             Tensor.copy_ between two device buffers of the clip's size for comparison
The kernel names a trace shows are geom_forward_kernel and geom_backward_kernel (profiles/geom_numbers.md).
"""
import argparse
import json
import math
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd.train_step import Trainer           # noqa: E402

ALL = "xflip,rot90,scale,rotate,aniso"
MODES = {"off": {}, "p0": dict(d_aug_geom=ALL, d_aug_p=0.0), "p1": dict(d_aug_geom=ALL, d_aug_p=1.0),
         "adaptive": dict(d_aug_geom=ALL, d_aug_p=0.5, d_aug_target=0.6)}


def cfg(a, **over):
    return argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                              lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                              beta2=0.9, n_class=101, k_sample=8, **over)


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
    tr = Trainer([], cfg(a, **MODES[mode]), device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16)
    gen = torch.Generator().manual_seed(1)
    real = (torch.rand(a.batch, 3, a.frames, a.size, a.size, generator=gen) * 2 - 1).to(dev)
    labels = torch.randint(0, 101, (a.batch,), generator=gen).to(dev)
    tr.register_label_buffer(labels)
    torch.manual_seed(100)
    ms = timed(lambda: tr.train_step(real, labels), a.steps, a.warmup)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    p = tr.d_aug_p if mode != "off" else None
    del tr, real
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return ms, peak, p


def about_centre(m00, m01, m10, m11, S):
    c = (S - 1) / 2.0
    return (m00, m01, c - m00 * c - m01 * c, m10, m11, c - m10 * c - m11 * c)


def kernel_times(a):
    from dvd_gan_amd.geom_augment import IDENTITY_ROW, clip_warp_backward, clip_warp_forward, draw_geom
    dev = torch.device("cuda", 0)
    S = a.size
    x = torch.rand(a.batch * a.frames, 3, S, S, device=dev) * 2 - 1
    nbytes = 2 * x.numel() * 4
    co, si = math.cos(math.pi / 6), math.sin(math.pi / 6)
    rows = {"identity": [IDENTITY_ROW] * a.batch, "xflip": [(-1.0, 0.0, S - 1.0, 0.0, 1.0, 0.0)] * a.batch,
            "rotate 30": [about_centre(co, -si, si, co, S)] * a.batch,
            "magnify 1.5": [about_centre(1 / 1.5, 0.0, 0.0, 1 / 1.5, S)] * a.batch,
            "drawn, all groups": draw_geom(a.batch, S, S, ALL, 1.0, torch.Generator().manual_seed(0)).tolist()}
    out = []
    for name, table in rows.items():
        mats = torch.tensor(table, dtype=torch.float32, device=dev)
        for tag, fn in (("forward", clip_warp_forward), ("backward", clip_warp_backward)):
            ms = timed(lambda: fn(x, mats, a.frames), a.steps * 4, a.warmup)
            out.append({"kernel": tag, "row": name, "us": round(ms * 1e3, 1), "gb_per_s": round(nbytes / ms / 1e6, 1)})
    y = torch.empty_like(x)
    ms = timed(lambda: y.copy_(x), a.steps * 4, a.warmup)
    out.append({"kernel": "device-to-device copy", "us": round(ms * 1e3, 1), "gb_per_s": round(nbytes / ms / 1e6, 1)})
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--frames", type=int, default=48)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--what", default="kernel,step")
    p.add_argument("--modes", default="off,p0,p1,adaptive", help="Trainers to time, in this order (a name may repeat)")
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=180.0)
    a = p.parse_args()
    if a.one:                                  # a child: one Trainer, one line
        ms, peak, prob = step_time(a, a.one)
        print(json.dumps({"step": a.one, "ms_per_step": round(ms, 2), "peak_gb": round(peak, 1), "p_after": prob}), flush=True)
        return
    what = a.what.split(",")
    if "step" in what:
        # every Trainer in a process of its own, and before this process touches the device (tools/aug_step_time.py says why)
        res = {}
        for mode in a.modes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", mode] + [
                f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "batch", "ch", "frames", "size")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout, check=True).stdout.decode()
            row = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            res.setdefault(mode, []).append(row["ms_per_step"])
            print(json.dumps(row), flush=True)
        off = res.get("off")
        print(json.dumps({"summary": {**{f"{m}_minus_off_ms": [round(min(v) - max(off), 2), round(max(v) - min(off), 2)]
                                         for m, v in res.items() if m != "off" and off},
                                      "off_spread_ms": None if not off else round(max(off) - min(off), 2),
                                      "shape": f"B={a.batch}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16"}}), flush=True)
    if "kernel" in what:
        for r in kernel_times(a):
            print(json.dumps({"launch": r}), flush=True)


if __name__ == "__main__":
    main()

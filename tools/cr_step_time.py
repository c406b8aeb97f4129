"""What balanced consistency regularization of the discriminators (Trainer(d_cr=...)) costs, at the benchmark's configuration with
d_aug on: the training step without and with it, and the pair-loss launch alone.

usage: python tools/cr_step_time.py [--steps N] [--warmup W] [--batch B] [--ch C] [--frames T] [--size S] [--what step,kernel]
                                    [--modes aug,cr,aug,cr,aug,cr]
Prints one JSON line per measurement:
  step       ms per train_step (HIP events around N steps after W warm-up steps, same seeds; every Trainer in a child process
             of its own, in the order of --modes, where a name may repeat; the summary gives the range of the ratio):
             "aug" = d_aug "color,translation,cutout" at p = 1 (what the penalty is measured on top of), "cr" = the same with
             d_cr = 10: every discriminator call of the D iteration on twice the samples, four more launches
  kernel     us per launch of dvdx_cr_pair (HIP events around N launches) at the pairs of a D_s call (B * k) and of a D_t call
             (B * T / 4) of that configuration
The kernel name a trace shows is cr_pair_kernel (profiles/cr_numbers.md).
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd.train_step import Trainer           # noqa: E402

ALL = "color,translation,cutout"
MODES = {"aug": {}, "cr": dict(d_cr=10.0)}
K_SAMPLE = 8


def cfg(a):
    return argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                              lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                              beta2=0.9, n_class=101, k_sample=K_SAMPLE, d_aug=ALL, d_aug_p=1.0)


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
    tr = Trainer([], cfg(a), device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16, **MODES[mode])
    gen = torch.Generator().manual_seed(1)
    real = (torch.rand(a.batch, 3, a.frames, a.size, a.size, generator=gen) * 2 - 1).to(dev)
    labels = torch.randint(0, 101, (a.batch,), generator=gen).to(dev)
    tr.register_label_buffer(labels)
    torch.manual_seed(100)
    ms = timed(lambda: tr.train_step(real, labels), a.steps, a.warmup)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    rep = tr.cr_report()
    return ms, peak, None if rep is None else {site: round(row["mean_sq_gap"], 6) for site, row in rep.items()}


def kernel_times(a):
    from dvd_gan_amd import lib as L
    dev = torch.device("cuda", 0)
    out = []
    for what, n in (("D_s call", a.batch * K_SAMPLE), ("D_t call", a.batch * a.frames // 4)):
        aug, clean = torch.randn(n, device=dev), torch.randn(n, device=dev)
        loss, da, dc = torch.zeros(1, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
        stats = torch.zeros(L.CR_NSTAT, device=dev)
        so, st = L.cr_lib(), L.stream()
        launch = lambda: L.cr_check(so.dvdx_cr_pair(L.ptr(aug), L.ptr(clean), n, 10.0, L.ptr(loss), L.ptr(da), L.ptr(dc),
                                                    L.ptr(stats), st))
        ms = timed(launch, a.steps * 40, a.warmup * 10)
        out.append({"kernel": "dvdx_cr_pair", "site": what, "pairs": n, "us": round(ms * 1e3, 2)})
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--frames", type=int, default=48)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--what", default="step,kernel")
    p.add_argument("--modes", default="aug,cr,aug,cr,aug,cr", help="Trainers to time, in this order (a name may repeat)")
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=180.0)
    a = p.parse_args()
    if a.one:                                  # a child: one Trainer, one line
        ms, peak, gaps = step_time(a, a.one)
        print(json.dumps({"step": a.one, "ms_per_step": round(ms, 2), "peak_gb": round(peak, 1), "mean_sq_gap": gaps}), flush=True)
        return
    what = a.what.split(",")
    if "step" in what:
        # every Trainer in a process of its own: a Trainer built after another one in the same process can run 3-8 % slower
        # on the same launches, which reads as a cost of whichever mode comes later.  The children come
        # first, while this process has not touched the device.
        res = {}
        for mode in a.modes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", mode] + [
                f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "batch", "ch", "frames", "size")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout, check=True).stdout.decode()
            row = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            res.setdefault(mode, []).append(row["ms_per_step"])
            print(json.dumps(row), flush=True)
        aug, cr = res.get("aug"), res.get("cr")
        summary = {"shape": f"B={a.batch}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16, d_aug at p = 1"}
        if aug and cr:
            summary.update(aug_ms=[min(aug), max(aug)], cr_ms=[min(cr), max(cr)],
                           cr_over_aug=[round(min(cr) / max(aug), 4), round(max(cr) / min(aug), 4)],
                           cr_minus_aug_ms=[round(min(cr) - max(aug), 2), round(max(cr) - min(aug), 2)])
        print(json.dumps({"summary": summary}), flush=True)
    if "kernel" in what:
        for r in kernel_times(a):
            print(json.dumps({"launch": r}), flush=True)


if __name__ == "__main__":
    main()

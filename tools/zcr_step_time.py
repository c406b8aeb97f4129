"""What latent consistency regularization (Trainer(z_cr=..., z_cr_gen=...)) costs at the benchmark's configuration: the training
step without and with it, and the two streaming launches of the generator's term alone against a plain copy.

usage: python tools/zcr_step_time.py [--steps N] [--warmup W] [--batch B] [--ch C] [--frames T] [--size S] [--what step,kernel]
                                     [--modes base,zcr,base,zcr,base,zcr]
Prints one JSON line per measurement:
  step       ms per train_step (HIP events around N steps after W warm-up steps, same seeds; every Trainer in a child process
             of its own, in the order of --modes, where a name may repeat; the summary gives the range of the ratio):
             "base" = the benchmark's configuration (the parent's step), "zcr" = the same with z_cr = 5, z_cr_gen = 0.5: the
             generator on 2B rows, the fake calls of D_s / D_t on 2B samples, two more pair-loss launches and the three
             launches of the generator's term; "dis" = z_cr = 5 alone (no term, the generator still on 2B rows)
  kernel     us per call and bytes / time of dvdx_zcr_dist (reads both halves) and dvdx_zcr_dist_grad (reads both, writes both)
             on halves [B, T * 3 * S * S] of one tensor, and of torch's copy_ of one half (reads one, writes one) as the copy
             this box reaches; HIP events around N * 20 back-to-back launches
The kernel names a trace shows are zcr_dist_kernel, zcr_finish_kernel and zcr_grad_kernel (profiles/zcr_numbers.md).
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd.train_step import Trainer           # noqa: E402

MODES = {"base": {}, "zcr": dict(z_cr=5.0, z_cr_gen=0.5), "dis": dict(z_cr=5.0)}
K_SAMPLE = 8


def cfg(a):
    return argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                              lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                              beta2=0.9, n_class=101, k_sample=K_SAMPLE)


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
    return ms, peak, tr.zcr_report()


def kernel_times(a):
    from dvd_gan_amd import kern as K
    from dvd_gan_amd import lib as L
    dev = torch.device("cuda", 0)
    pairs, n = a.batch, a.frames * 3 * a.size * a.size
    both = torch.rand(2 * pairs, n, device=dev) * 2 - 1
    grad = torch.empty_like(both)
    ws = torch.empty(K.zcr_ws_doubles(pairs, n), dtype=torch.float64, device=dev)
    term, stats, up = torch.zeros(1, device=dev), torch.zeros(L.ZCR_NSTAT, device=dev), torch.ones(1, device=dev)
    half = 4 * pairs * n
    runs = (("dvdx_zcr_dist", 2 * half, lambda: K.zcr_dist(both[:pairs], both[pairs:], pairs, n, 0.5, ws, term, stats)),
            ("dvdx_zcr_dist_grad", 4 * half,
             lambda: K.zcr_dist_grad(both[:pairs], both[pairs:], pairs, n, 0.5, up, grad[:pairs], grad[pairs:])),
            ("torch copy_ of one half", 2 * half, lambda: grad[:pairs].copy_(both[:pairs])))
    out = []
    for _ in range(2):                               # twice, in turn: the second round shows the spread
        for name, nbytes, fn in runs:
            ms = timed(fn, a.steps * 20, a.warmup * 5)
            out.append({"kernel": name, "pairs": pairs, "n": n, "mb": round(nbytes / 1e6, 1), "us": round(ms * 1e3, 1),
                        "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3)})
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
    p.add_argument("--modes", default="base,zcr,base,zcr,base,zcr", help="Trainers to time, in this order (a name may repeat)")
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=180.0)
    a = p.parse_args()
    if a.one:                                  # a child: one Trainer, one line
        ms, peak, rep = step_time(a, a.one)
        print(json.dumps({"step": a.one, "ms_per_step": round(ms, 2), "peak_gb": round(peak, 1), "zcr_report": rep}), flush=True)
        return
    what = a.what.split(",")
    if "step" in what:
        # every Trainer in a process of its own, before this process touches the device (tools/cr_step_time.py has the reason)
        res = {}
        for mode in a.modes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", mode] + [
                f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "batch", "ch", "frames", "size")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout, check=True).stdout.decode()
            row = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            res.setdefault(mode, []).append(row["ms_per_step"])
            print(json.dumps(row), flush=True)
        summary = {"shape": f"B={a.batch}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16"}
        base = res.get("base")
        for mode, ms in res.items():
            summary[mode + "_ms"] = [min(ms), max(ms)]
            if base and mode != "base":
                summary[mode + "_over_base"] = [round(min(ms) / max(base), 4), round(max(ms) / min(base), 4)]
                summary[mode + "_minus_base_ms"] = [round(min(ms) - max(base), 2), round(max(ms) - min(base), 2)]
        print(json.dumps({"summary": summary}), flush=True)
    if "kernel" in what:
        for r in kernel_times(a):
            print(json.dumps({"launch": r}), flush=True)


if __name__ == "__main__":
    main()

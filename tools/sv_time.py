"""What the singular-value monitoring of the weights costs (Trainer with config.sv_log, Trainer.sv_report; dvd_gan_amd/spectral.py),
at the benchmark's widths.

usage: python tools/sv_time.py [--steps N] [--warmup W] [--batch B] [--ch C] [--frames T] [--size S] [--what report,svdvals,step]
                               [--modes off,every,off,every]
Prints one JSON line per measurement:
  report     per network (G, Ds, Dt): ms of one report = 4 iterations + the finish at k = 3, block = 8 on that network's monitor (HIP
             events around N reports after W warm-up reports; warm blocks -- the time does not depend on what they hold), the
             matrices, the bytes of W, and the achieved rate over (2 * 4 + 1) * bytes(W): every W is read 9 times and nothing else
             of that size is.  Also the three largest matrices of the network alone, each in a monitor of its own.
  svdvals    the same matrices through torch.linalg.svdvals, one call per matrix: on the device when the installed torch serves it
             there, otherwise on the host with the copy included -- what a user could do before
  step       ms per train_step (HIP events around N steps after W warm-up steps, same seeds; every Trainer in a child process of
             its own, in the order of --modes): "off" = sv_log 0 (the step of the parent commit: the setting unset changes
             nothing), "every" = sv_log 1, a report's launches in EVERY step; the cost per step at sv_log = 100 is a hundredth of
             the difference
The kernel names a trace shows are sv_wv_kernel, sv_orth_kernel, sv_wtv_kernel and sv_ritz_kernel (profiles/sv_numbers.md).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd.train_step import Trainer           # noqa: E402

MODES = {"off": {}, "every": dict(sv_log=1)}
ITERS, K, BLOCK = 4, 3, 8


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
    return ms, peak


def report_times(a, what):
    from dvd_gan_amd.spectral import SpectrumMonitor
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tr = Trainer([], cfg(a), device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16)
    out = []
    reps = max(a.steps * 4, 20)

    def one(tag, mats, label):
        mon = SpectrumMonitor(mats, k=K, block=BLOCK)
        ms = timed(lambda: (mon.update(ITERS), mon.snapshot(0)), reps, a.warmup)
        nbytes = sum(t.numel() * 4 for _, t in mats)
        return {"report": tag, "what": label, "matrices": len(mats), "mbytes_W": round(nbytes / 1e6, 2), "ms": round(ms, 3),
                "gb_per_s_over_9_reads": round(9 * nbytes / ms / 1e6, 1), "launches": 4 * ITERS + 2}
    for tag, net in (("G", tr.G), ("Ds", tr.D_s), ("Dt", tr.D_t)):
        mats = [(n, p.data) for n, p in net.named_parameters() if p.requires_grad and p.dim() >= 2]
        if "report" in what:
            out.append(one(tag, mats, "all matrices"))
            for n, t in sorted(mats, key=lambda m: -m[1].numel())[:3]:
                out.append(one(tag, [(n, t)], f"{n} {t.shape[0]} x {t.numel() // t.shape[0]} alone"))
            print("\n".join(json.dumps(r) for r in out[-4:]), flush=True)
        if "svdvals" in what:
            views = [t.reshape(t.shape[0], -1) for _, t in mats]
            try:
                torch.linalg.svdvals(views[0])
                where = "device"
                ms = timed(lambda: [torch.linalg.svdvals(v) for v in views], 2, 1)
            except Exception as e:                      # not served on the device: the host route, copy included
                where = f"host ({type(e).__name__} on the device)"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for v in views:
                    torch.linalg.svdvals(v.cpu().double())
                ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"svdvals": tag, "where": where, "matrices": len(views), "ms": round(ms, 2)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--frames", type=int, default=48)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--what", default="step,report,svdvals")
    p.add_argument("--modes", default="off,every,off,every", help="Trainers to time, in this order (a name may repeat)")
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=180.0)
    a = p.parse_args()
    if a.one:                                  # a child: one Trainer, one line
        ms, peak = step_time(a, a.one)
        print(json.dumps({"step": a.one, "ms_per_step": round(ms, 2), "peak_gb": round(peak, 2)}), flush=True)
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
    if "report" in what or "svdvals" in what:
        report_times(a, what)


if __name__ == "__main__":
    main()

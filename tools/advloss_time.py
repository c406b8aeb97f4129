"""What the loss launch with LeCam regularization, top-k selection and logit statistics (dvd_adv_loss_ex; config lecam / g_topk /
d_stats) costs: the launch in isolation against dvd_adv_loss, the launch it replaces, and the training step.

usage: python tools/advloss_time.py [--launches N] [--blocks R] [--steps N] [--warmup W] [--repeats R] [--batch B] [--ch C]
                                    [--frames T] [--size S] [--what kernel,step]
Prints one JSON line per measurement:
  kernel     n = 512 and 768 (the benchmark's D_s and D_t logits at B = 64: 64 samples of 8 and of 12) and 8192 (4096 samples of 2,
             the selection's cap).  Per block (R blocks; the median over them is reported beside every block) and n, N launches
             back to back between HIP events after 3 warm-up launches, microseconds per launch: "old" = dvd_adv_loss, "off" =
             dvd_adv_loss_ex with everything off (the same results), "stats" = with the statistics, "topk" = selection of half
             the samples + statistics, "all" = selection, the LeCam term, the anchor update and the statistics.  One workgroup
             of work each: the figure is the launch-to-launch time of a stream of such launches, not a bandwidth.
  step       ms per train_step (a HIP event after every step, --steps steps after --warmup) for "off" (the new fields unset: the
             step bench.py times, through dvd_adv_loss) and "on" (lecam = 0.3 from the first iteration, g_topk = 0.5 in epoch 50,
             where 38 of 64 samples are kept, d_stats).  --repeats rounds, the order rotating, every Trainer in a child process of
             its own (tools/guard_step_time.py says why).  The summary gives the difference of the means beside the spread of
             each variant's repeats: the spread of "off" is that of the unchanged step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd import lib as L                       # noqa: E402
from dvd_gan_amd.train_step import Trainer           # noqa: E402

SHAPES = ((512, 8), (768, 12), (8192, 2))
VARIANTS = {"off": {}, "on": dict(lecam=0.3, lecam_start=0, g_topk=0.5, g_topk_decay=0.99, d_stats=True)}


def cfg(a, extra):
    return argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                              lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                              beta2=0.9, n_class=101, k_sample=8, **extra)


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
    dev = torch.device("cuda", 0)
    lib, adv = L.lib(), L.adv_lib()
    gen = torch.Generator().manual_seed(0)
    summary = {}
    for n, group in SHAPES:
        x = torch.randn(n, generator=gen).to(dev)
        loss, dout = torch.zeros(1, device=dev), torch.empty(n, device=dev)
        anc, stats = torch.zeros(3, device=dev), torch.zeros(L.ADV_NSTAT, device=dev)
        half = n // group // 2
        px, pl, pd, ps = L.ptr(x), L.ptr(loss), L.ptr(dout), L.ptr(stats)
        other, prev, nxt = L.ptr(anc[0:1]), L.ptr(anc[1:2]), L.ptr(anc[2:3])
        st = L.stream()
        calls = {
            "old": lambda: lib.dvd_adv_loss(px, n, 1, 1, pl, pd, 1.0, st),
            "off": lambda: adv.dvd_adv_loss_ex(px, n, group, 1, 1, 0, 0.0, None, None, None, 0.0, pl, pd, 1.0, None, st),
            "stats": lambda: adv.dvd_adv_loss_ex(px, n, group, 1, 1, 0, 0.0, None, None, None, 0.0, pl, pd, 1.0, ps, st),
            "topk": lambda: adv.dvd_adv_loss_ex(px, n, group, 1, 1, half, 0.0, None, None, None, 0.0, pl, pd, 1.0, ps, st),
            "all": lambda: adv.dvd_adv_loss_ex(px, n, group, 1, 1, half, 0.3, other, prev, nxt, 0.99, pl, pd, 1.0, ps, st),
        }
        for name, fn in calls.items():
            L.check(fn())
        rows = []
        for b in range(a.blocks):
            row = {name: round(events(fn, a.launches) * 1e3, 2) for name, fn in calls.items()}
            rows.append(row)
            print(json.dumps({"kernel": {"n": n, "group": group, "block": b, "launches": a.launches, "us_per_launch": row}}), flush=True)
        summary[f"n={n}"] = {name: round(statistics.median(r[name] for r in rows), 2) for name in calls}
    print(json.dumps({"kernel_summary_median_us": summary}), flush=True)


def step_time(a, variant):
    """One Trainer: --warmup steps, then --steps steps with a HIP event between every two (no host sync inside the loop)."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tr = Trainer([], cfg(a, VARIANTS[variant]), device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16)
    tr._epoch = 51                                      # the 51st epoch has begun: floor(B * 0.99^50) samples are kept
    gen = torch.Generator().manual_seed(1)
    real = (torch.rand(a.batch, 3, a.frames, a.size, a.size, generator=gen) * 2 - 1).to(dev)
    labels = torch.randint(0, 101, (a.batch,), generator=gen).to(dev)
    tr.register_label_buffer(labels)
    torch.manual_seed(100)
    for _ in range(a.warmup):
        tr.train_step(real, labels)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    ev[0].record()
    for i in range(a.steps):
        tr.train_step(real, labels)
        ev[i + 1].record()
    torch.cuda.synchronize()
    per_step = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)]
    return per_step, torch.cuda.max_memory_allocated() / 2 ** 30, tr.d_stats()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=2000)
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--frames", type=int, default=48)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--what", default="kernel,step")
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=180.0)
    a = p.parse_args()
    what = a.what.split(",")
    if a.one:                                       # child of the step level: one Trainer in this process
        per_step, peak, report = step_time(a, a.one)
        row = {"variant": a.one, "ms_per_step": round(sum(per_step) / len(per_step), 2),
               "per_step_ms": [round(x, 1) for x in per_step], "peak_gb": round(peak, 2)}
        if report is not None:
            row["r_t"] = {tag: round(report[tag]["r_t"], 3) for tag in ("Ds", "Dt")}
            row["g_kept"] = {tag: report[tag]["g_kept"] for tag in ("Ds", "Dt")}
        print(json.dumps(row), flush=True)
        return
    if "kernel" in what:
        kernel_level(a)
        torch.cuda.empty_cache()
    if "step" in what:
        names = list(VARIANTS)
        res = {v: [] for v in names}
        for r in range(a.repeats):
            for v in names[r % len(names):] + names[:r % len(names)]:          # the order rotates
                cmd = [sys.executable, os.path.abspath(__file__), "--one", v] + [
                    f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "batch", "ch", "frames", "size")]
                out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout, check=True).stdout.decode()
                row = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
                res[v].append(row["ms_per_step"])
                print(json.dumps({"step": {"repeat": r, **row}}), flush=True)
        mean = {v: sum(x) / len(x) for v, x in res.items()}
        print(json.dumps({"step_summary": {**{v + "_ms": [round(x, 2) for x in res[v]] for v in names},
                                           "on_minus_off_ms_mean": round(mean["on"] - mean["off"], 2),
                                           **{v + "_spread_ms": round(max(res[v]) - min(res[v]), 2) for v in names},
                                           "shape": f"B={a.batch}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16"}}))


if __name__ == "__main__":
    main()

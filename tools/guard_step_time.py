"""What the gradient guard (config g_clip_norm / d_clip_norm / skip_nonfinite / grad_log) costs: the norm pass in isolation, and
the training step.

usage: python tools/guard_step_time.py [--launches N] [--blocks R] [--steps N] [--warmup W] [--repeats R] [--batch B] [--ch C]
                                       [--frames T] [--size S] [--what kernel,step]
Prints one JSON line per measurement:
  kernel     n = the trainable parameter counts of G, D_s and D_t at --ch, taken from the models.  Per block (R blocks, for the
             spread) and size: dvd_grad_guard (both of its launches: the pass over the gradient and the finalizing workgroup),
             dvd_ema_step on the same n (the yardstick: it moves three streams where the guard moves one), dvd_adam_step and
             dvd_adam_guard_step (the launch the guard replaces it with), one after the other, each N launches between HIP events
             after 3 warm-up launches; ms per launch and GB/s from 4 / 12 / 28 / 28 bytes per element.  The summary line says
             whether the guard pass took no longer than the averaging pass at the generator's size in every block.
  step       ms per train_step (a HIP event after every step, --steps steps after --warmup) for two variants: "off" (the four
             fields at their defaults: the step bench.py times) and "on" (skip_nonfinite, grad_log = 16 and clipping norms no
             gradient reaches: the same launches as any other guard setting).  --repeats rounds, the order rotating, EVERY TRAINER
             IN A CHILD PROCESS OF ITS OWN (a Trainer built after another one was torn down in the same process can run 3-8 %
             slower with the same launches: tools/ema_step_time.py).  The summary reports the difference of the means beside the
             spread of each variant's repeats.
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

BYTES = {"guard": 4, "ema": 12, "adam": 28, "adam_guard": 28}        # per element: 1 read | 2 + 1 | 4 reads + 3 writes
VARIANTS = {"off": {}, "on": dict(skip_nonfinite=True, grad_log=16, g_clip_norm=1e30, d_clip_norm=1e30)}


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


def network_sizes(a):
    from dvd_gan_amd.disc_nets import SpatialDiscriminator, TemporalDiscriminator
    from dvd_gan_amd.gen_net import Generator
    with torch.device("meta"):                          # shapes only
        nets = {"G": Generator(120, a.size // 16, 101, a.ch, a.frames), "Ds": SpatialDiscriminator(a.ch, 101),
                "Dt": TemporalDiscriminator(a.ch, 101)}
    return {tag: sum(p.numel() for p in net.parameters() if p.requires_grad) for tag, net in nets.items()}


def kernel_level(a):
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    blocks = {}
    for tag, n in network_sizes(a).items():
        p, g = (torch.randn(n, generator=gen) * 0.05).to(dev), (torch.randn(n, generator=gen) * 1e-3).to(dev)
        m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
        ws = torch.empty(K.grad_guard_ws_bytes(n), dtype=torch.uint8, device=dev)
        state = torch.zeros(K.GUARD_STATE, dtype=torch.float64, device=dev)
        t = [0]

        def guard():
            t[0] += 1
            K.grad_guard(g, 1e30, True, t[0], ws, state)

        def ema_only():
            K.ema_step(ema, p, 0.9999)

        def adam():
            t[0] += 1
            K.adam_step(p, g, m, v, 5e-5, 0.0, 0.9, 1e-8, t[0])

        def adam_guard():
            t[0] += 1
            K.adam_guard_step(p, g, m, v, None, 5e-5, 0.0, 0.9, 1e-8, t[0], 0.0, state)
        blocks[tag] = []
        for b in range(a.blocks):
            row = {}
            for name, fn in (("guard", guard), ("ema", ema_only), ("adam", adam), ("adam_guard", adam_guard)):
                ms = events(fn, a.launches)
                row[name] = {"ms": round(ms, 4), "GBps": round(BYTES[name] * n / ms / 1e6, 1)}
            blocks[tag].append(row)
            print(json.dumps({"kernel": {"net": tag, "block": b, "n": n, "launches": a.launches, **row}}), flush=True)
        assert state.cpu().tolist()[1:4] == [1.0, 0.0, 0.0]           # the timed guard never clipped or skipped
        del p, g, m, v, ema, ws
    summary = {}
    for tag, rows in blocks.items():
        summary[tag] = {k + "_ms": [r[k]["ms"] for r in rows] for k in BYTES}
        summary[tag]["guard_minus_ema_ms_max"] = round(max(r["guard"]["ms"] - r["ema"]["ms"] for r in rows), 4)
        summary[tag]["adam_guard_minus_adam_ms_max"] = round(max(r["adam_guard"]["ms"] - r["adam"]["ms"] for r in rows), 4)
    summary["guard_no_longer_than_ema_at_G"] = all(r["guard"]["ms"] <= r["ema"]["ms"] for r in blocks["G"])
    print(json.dumps({"kernel_summary": summary}), flush=True)


def step_time(a, variant):
    """One Trainer: --warmup steps, then --steps steps with a HIP event between every two (no host sync inside the loop)."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tr = Trainer([], cfg(a, VARIANTS[variant]), device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16)
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
    return per_step, torch.cuda.max_memory_allocated() / 2 ** 30, tr.guard_report()


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
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=180.0)
    a = p.parse_args()
    what = a.what.split(",")
    if a.one:                                       # child of the step level: one Trainer in this process
        per_step, peak, report = step_time(a, a.one)
        row = {"variant": a.one, "ms_per_step": round(sum(per_step) / len(per_step), 2),
               "per_step_ms": [round(x, 1) for x in per_step], "peak_gb": round(peak, 2)}
        if report is not None:
            row["norms"] = {tag: r["norm"] for tag, r in report.items()}
            row["seen_skipped_clipped"] = {tag: [r["seen"], r["skipped"], r["clipped"]] for tag, r in report.items()}
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
                # every Trainer in a process of its own: see the module docstring.  A child that fails ends the run.
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

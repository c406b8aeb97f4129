"""What a full training-state save (Trainer.save_state, exact resume) costs the training loop at the benchmark configuration
(bench.py's default shape: B = 64, T = 48, 64 x 64, ch = 32, 101 classes, bf16; about 2 GB of state).

usage: python tools/state_save_time.py [--steps 20] [--warmup 3] [--repeats 2] [--batch B] [--ch C] [--frames T] [--size S]
                                       [--dir DIR]
Three variants, every Trainer in a child process of its own (a second Trainer in one process misleads), the order
rotating from repeat to repeat, all on the same box:
  none    --steps steps, no save
  async   the same steps with one save_state(wait=False) after step --steps / 2
  sync    the same with save_state(wait=True)
One JSON line per run: ms_per_step (wall clock over all steps between two device synchronisations, the save call inside it),
save_call_ms (host time inside save_state), file_complete_ms (from the call until `{step}_state.pt` exists under its final name,
polled every 2 ms), the file's size; then a summary line with the means and the spread per variant.  The files go to --dir
(default: a temporary directory) and are removed."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd.train_step import Trainer           # noqa: E402

VARIANTS = ("none", "async", "sync")
SHAPE = ("steps", "warmup", "batch", "ch", "frames", "size")


def one(a, variant, folder):
    dev = torch.device("cuda", 0)
    cfg = argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames, lr_schr="const",
                             total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9, n_class=101,
                             k_sample=8, model_save_path=folder, version="")
    torch.manual_seed(0)
    tr = Trainer([], cfg, device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16)
    gen = torch.Generator().manual_seed(1)
    real = (torch.rand(a.batch, 3, a.frames, a.size, a.size, generator=gen) * 2 - 1).to(dev)
    labels = torch.randint(0, 101, (a.batch,), generator=gen).to(dev)
    tr.register_label_buffer(labels)
    torch.manual_seed(100)
    for _ in range(a.warmup):
        tr.train_step(real, labels)
    torch.cuda.synchronize()
    at = a.steps // 2
    path = os.path.join(folder, "%d_state.pt" % at)
    seen = {}

    def watch(t_call):
        while not os.path.exists(path):
            time.sleep(0.002)
        seen["ms"] = (time.perf_counter() - t_call) * 1e3
    call_ms, watcher = None, None
    t0 = time.perf_counter()
    for i in range(1, a.steps + 1):
        tr.train_step(real, labels)
        if variant != "none" and i == at:
            t_call = time.perf_counter()
            watcher = threading.Thread(target=watch, args=(t_call,), daemon=True)
            watcher.start()
            tr.save_state(at, wait=variant == "sync")
            call_ms = (time.perf_counter() - t_call) * 1e3
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    row = {"variant": variant, "ms_per_step": round(ms, 2)}
    if watcher is not None:
        tr.close_state()
        watcher.join()
        row.update(save_call_ms=round(call_ms, 2), file_complete_ms=round(seen["ms"], 1),
                   file_gb=round(os.path.getsize(path) / 1e9, 3))
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--frames", type=int, default=48)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--dir", default=None)
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=240.0)
    a = p.parse_args()
    if a.one:                                       # a child: one Trainer in this process
        folder = tempfile.mkdtemp(prefix="state_save_time_", dir=a.dir)
        try:
            print(json.dumps(one(a, a.one, folder)), flush=True)
        finally:
            shutil.rmtree(folder, ignore_errors=True)
        return
    rows = {v: [] for v in VARIANTS}
    for r in range(a.repeats):
        for v in VARIANTS[r % 3:] + VARIANTS[:r % 3]:              # the order rotates; a child that fails ends the run
            cmd = [sys.executable, os.path.abspath(__file__), "--one", v] + [f"--{k}={getattr(a, k)}" for k in SHAPE]
            if a.dir:
                cmd.append(f"--dir={a.dir}")
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout, check=True).stdout.decode()
            row = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
            rows[v].append(row)
            print(json.dumps({"repeat": r, **row}), flush=True)
    mean = lambda v, k: round(sum(x[k] for x in rows[v]) / len(rows[v]), 2)
    summary = {"shape": f"B={a.batch}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16, {a.steps} steps, one save after step {a.steps // 2}"}
    for v in VARIANTS:
        steps = [x["ms_per_step"] for x in rows[v]]
        summary[v] = {"ms_per_step": steps, "mean": mean(v, "ms_per_step"), "spread": round(max(steps) - min(steps), 2)}
        if v != "none":
            summary[v].update(save_call_ms=mean(v, "save_call_ms"), file_complete_ms=mean(v, "file_complete_ms"),
                              minus_none_ms_per_step=round(mean(v, "ms_per_step") - mean("none", "ms_per_step"), 2),
                              file_gb=rows[v][0]["file_gb"])
    print(json.dumps({"summary": summary}))


if __name__ == "__main__":
    main()

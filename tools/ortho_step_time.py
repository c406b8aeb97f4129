"""What orthogonal regularization of the generator (config.g_ortho > 0) costs: the kernel pair in isolation, and the training step.

usage: python tools/ortho_step_time.py [--launches N] [--blocks R] [--steps N] [--warmup W] [--repeats R] [--batch B] [--ch C]
                                       [--frames T] [--size S] [--what kernel,step]
Prints one JSON line per measurement:
  kernel     dvd_ortho_grad (Gram launch + apply launch + the penalty's reduce) on the item table optim.FlatAdam builds for the
             generator at --ch, weights 0.05 * N(0, 1): per block (R blocks, for the spread) N calls between HIP events after 3
             warm-up calls; ms per call and TF/s against two FLOP counts the tool derives from the table -- `full` = 4 h numel per
             matrix (both products in full) and `done` = 3 h numel (the Gram pass computes the upper triangle of 64 x 64 tiles
             only; counted per tile) -- plus the workspace bytes.  For scale: the guide's figures for v_mfma_f32_32x32x2_f32 are
             155 TF/s peak and 122 TF/s for an untuned 4096^3 GEMM.
  step       ms per train_step (a HIP event after every step, --steps steps after --warmup) and max_memory_allocated with g_ortho
             off and on (1e-4), alternating.
Every measurement runs in a child process of its own, under its own time limit (--child-timeout), and the first child that
fails ends the run: a Trainer built after another one in the same process can run 3-8 % slower with the same launches
(tools/ema_step_time.py), and nothing is started on a device after a failure.
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cfg(a, g_ortho):
    return argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                              lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                              beta2=0.9, n_class=101, k_sample=8, g_ortho=g_ortho)


def kernel_level(a):
    import torch
    from dvd_gan_amd.gen_net import Generator
    from dvd_gan_amd.optim import FlatAdam
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    G = Generator(120, a.size // 16, 101, a.ch, a.frames).to(dev)
    opt = FlatAdam(G.parameters(), 5e-5, ortho=1e-4, ortho_exclude=G.ortho_exclude())
    opt.flat.copy_(0.05 * torch.randn(opt.flat.numel(), device=dev))
    rows = [r[:3] for r in opt.ortho_items.tolist()]
    full = sum(4 * h * h * w for _, h, w in rows if h > 1)
    done = sum(2 * h * h * w + 2 * (-(-h // 64) * (-(-h // 64) + 1) // 2) * 64 * 64 * w for _, h, w in rows if h > 1)
    out = []
    for b in range(a.blocks):
        for _ in range(3):
            opt.ortho_grad()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            opt.ortho_grad()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.launches
        out.append(ms)
        print(json.dumps({"kernel": {"block": b, "items": len(rows), "elements": sum(h * w for _, h, w in rows), "ms": round(ms, 4),
                                     "flop_full": full, "flop_done": done, "TFps_full": round(full / ms / 1e9, 1),
                                     "TFps_done": round(done / ms / 1e9, 1), "workspace_bytes": 4 * opt.ortho_ws_floats,
                                     "penalty": float(opt.ortho_penalty)}}), flush=True)
    print(json.dumps({"kernel_summary": {"ms": [round(x, 4) for x in out], "spread_ms": round(max(out) - min(out), 4),
                                         "guide_TFps_peak": 155, "guide_TFps_untuned_gemm": 122}}), flush=True)


VARIANTS = {"off": 0.0, "on": 1e-4}


def step_time(a, variant):
    import torch
    from dvd_gan_amd.train_step import Trainer
    dev = torch.device("cuda", 0)
    torch.cuda.reset_peak_memory_stats()
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
    pen = tr.ortho_penalty
    print(json.dumps({"variant": variant, "g_ortho": VARIANTS[variant], "ms_per_step": round(sum(per_step) / len(per_step), 2),
                      "per_step_ms": [round(x, 1) for x in per_step], "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                      "ortho_penalty": None if pen is None else float(pen)}), flush=True)


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
    if a.one == "kernel":
        return kernel_level(a)
    if a.one:
        return step_time(a, a.one)
    what = a.what.split(",")

    def child(which):
        # a process of its own per measurement; a child that fails or runs past its limit raises and ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--one", which] + [
            f"--{k}={getattr(a, k)}" for k in ("launches", "blocks", "steps", "warmup", "batch", "ch", "frames", "size")]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout, check=True).stdout.decode()
        return [json.loads(l) for l in out.splitlines() if l.startswith("{")]

    if "kernel" in what:
        for row in child("kernel"):
            print(json.dumps(row), flush=True)
    if "step" in what:
        names = list(VARIANTS)
        res = {v: [] for v in names}
        for r in range(a.repeats):
            for v in names[r % 2:] + names[:r % 2]:                  # off, on | on, off | ...
                row = child(v)[-1]
                res[v].append(row["ms_per_step"])
                print(json.dumps({"step": {"repeat": r, **row}}), flush=True)
        mean = {v: sum(x) / len(x) for v, x in res.items()}
        print(json.dumps({"step_summary": {**{v + "_ms": res[v] for v in names},
                                           "on_minus_off_ms_mean": round(mean["on"] - mean["off"], 2),
                                           **{v + "_spread_ms": round(max(res[v]) - min(res[v]), 2) for v in names},
                                           "shape": f"B={a.batch}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16"}}))


if __name__ == "__main__":
    main()

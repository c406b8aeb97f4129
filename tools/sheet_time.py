"""What sample sheets cost: dvd_sample_sheet against a torch-op restatement of the same sheets, the bytes that cross to the host,
and how long Trainer.save_samples keeps the host.

usage: python tools/sheet_time.py [--classes 101] [--per-class 8] [--frames 48] [--size 64] [--iters 30] [--ch 32] [--batch 16]
                                  [--calls 3] [--what kernel,torch,save]
Prints one JSON line per measurement (one process; HIP events around every single launch / pass, 3 warm-up runs, the MEDIAN of
--iters runs, min and max beside it):
  kernel   sheets.make_sheets(row_prefix=True) on a [classes * per-class, frames, 3, size, size] fp32 tensor in [-1, 1], both
           layouts: ms, GB/s against one read of the floats plus one write of the bytes.
  torch    the same "frames" sheets from torch operations on the same device, every pass timed on its own: add, div, clamp, mul,
           add, clamp (in place on one fp32 copy), the byte cast, the canvas fill and the permuted tile copy; the result is
           compared with the kernel's bytes (must be equal) before anything is timed.
  save     Trainer.save_samples (bf16, --ch, chunks of --batch, layout "frames") --calls times: seconds the call keeps the host
           with the writer running, seconds until flush() returns, bytes copied to the host per call (and the fp32 tensor's size
           a blocking copy of the generator's output would move).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd import sheets as S                     # noqa: E402


def timed(fn, iters, warmup=3):
    """-> (median, min, max) ms of fn(), one pair of events per run."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in pairs]
    return statistics.median(ms), min(ms), max(ms)


def row(tag, ms, **more):
    med, lo, hi = ms
    print(json.dumps({tag: dict(ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), **more)}), flush=True)


def kernel_level(a, frames):
    n, T = frames.shape[:2]
    for layout, nrow in (("frames", 8), ("clips", a.per_class)):
        out = S.make_sheets(frames, layout=layout, nrow=nrow, row_prefix=True)
        moved = frames.numel() * 4 + out.numel()
        ms = timed(lambda: S.make_sheets(frames, layout=layout, nrow=nrow, row_prefix=True, out=out), a.iters)
        row("kernel", ms, layout=layout, sheets=out.shape[0], sheet=list(out.shape[1:]), read_MB=round(frames.numel() * 4 / 1e6, 1),
            write_MB=round(out.numel() / 1e6, 1), GBps=round(moved / ms[0] / 1e6, 1))
        del out


def torch_level(a, frames):
    n, T, _, H, W = frames.shape
    Hs, Ws = S.sheet_shape(T, H, W)
    rows_, cols = (T + 7) // 8, min(8, T)
    if rows_ * cols != T:
        raise SystemExit("the torch restatement tiles full rows only: --frames must be a multiple of 8 (or below 8)")
    work = torch.empty_like(frames)
    q8 = torch.empty(frames.shape, dtype=torch.uint8, device=frames.device)
    canvas = torch.empty(n, Hs, Ws, 3, dtype=torch.uint8, device=frames.device)
    inner = canvas[:, 2:, 2:].unflatten(1, (rows_, H + 2)).unflatten(3, (cols, W + 2))[:, :, :H, :, :W]      # [n, r, H, c, W, 3]
    tiles = q8.view(n, rows_, cols, 3, H, W).permute(0, 1, 4, 2, 5, 3)
    passes = [("copy (stands for the first out-of-place op)", lambda: work.copy_(frames)),
              ("add 1", lambda: work.add_(1)), ("div 2", lambda: work.div_(2)), ("clamp 0 1", lambda: work.clamp_(0, 1)),
              ("mul 255", lambda: work.mul_(255)), ("add 0.5", lambda: work.add_(0.5)), ("clamp 0 255", lambda: work.clamp_(0, 255)),
              ("byte cast", lambda: q8.copy_(work)), ("canvas fill", lambda: canvas.fill_(0)),
              ("tile + permute", lambda: inner.copy_(tiles))]
    for _, fn in passes:                # once, in order: the chain's result
        fn()
    mine = S.make_sheets(frames).view(n, Hs, Ws, 3)
    equal = bool(torch.equal(mine, canvas))
    print(json.dumps({"torch_equals_kernel": equal}), flush=True)
    total = 0.0
    for name, fn in passes:             # (in-place passes run on their own output again: same traffic, other values)
        ms = timed(fn, a.iters)
        total += ms[0]
        row("torch_pass", ms, name=name)
    print(json.dumps({"torch_chain": {"ms_sum_of_medians": round(total, 4), "passes": len(passes)}}), flush=True)


def save_level(a):
    from dvd_gan_amd.train_step import Trainer
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        cfg = argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                                 lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                                 beta2=0.9, n_class=a.classes, k_sample=8, sample_path=tmp, version="t",
                                 test_batch_size=a.per_class, sample_layout="frames")
        torch.manual_seed(0)
        tr = Trainer([], cfg, device=dev, compute_dtype=torch.bfloat16, latent_dim=a.size // 16)
        n = a.classes * a.per_class
        Hs, Ws = S.sheet_shape(a.frames, a.size, a.size)
        for call in range(a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.save_samples(call)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            tr.sheet_writer.flush()
            t3 = time.perf_counter()
            print(json.dumps({"save_samples": {"call": call, "clips": n, "host_s": round(t1 - t0, 4),
                                               "device_done_s": round(t2 - t0, 4), "flush_done_s": round(t3 - t0, 4),
                                               "bytes_to_host_MB": round(n * Hs * (1 + 3 * Ws) / 1e6, 1),
                                               "fp32_output_MB": round(n * a.frames * 3 * a.size * a.size * 4 / 1e6, 1),
                                               "png_MB": round(sum(os.path.getsize(os.path.join(tmp, "t", f))
                                                                   for f in os.listdir(os.path.join(tmp, "t"))
                                                                   if f.endswith("_Step_%d.png" % call)) / 1e6, 1)}}), flush=True)
        tr.close_sheets()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--classes", type=int, default=101)
    p.add_argument("--per-class", type=int, default=8)
    p.add_argument("--frames", type=int, default=48)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--calls", type=int, default=3)
    p.add_argument("--what", default="kernel,torch,save")
    a = p.parse_args()
    what = a.what.split(",")
    if "kernel" in what or "torch" in what:
        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(0)
        frames = torch.rand(a.classes * a.per_class, a.frames, 3, a.size, a.size, device=dev, generator=gen) * 2.2 - 1.1
        if "kernel" in what:
            kernel_level(a, frames)
        if "torch" in what:
            torch_level(a, frames)
        del frames
        torch.cuda.empty_cache()
    if "save" in what:
        save_level(a)


if __name__ == "__main__":
    main()

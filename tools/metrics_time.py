"""What the prediction metrics cost: dvd_frame_metrics in isolation, and one predict() at the same batch for scale.

usage: python tools/metrics_time.py [--launches N] [--blocks R] [--batch B] [--frames T] [--samples S] [--sizes 64,128]
                                    [--ch C] [--what kernel,predict]
Prints one JSON line per measurement (one process, HIP events, 3 warm-up launches before every timed block):
  kernel     F = B * T and F = B * T * S frames of 3 x size x size (defaults: 64 * 16 and 64 * 16 * 8), `pred` a [F / T, T, 3, H, W]
             tensor in [-1, 1], `target` the [:, :, K:] view of a loader-shaped clip tensor, flags signed + quantize (what
             Trainer.evaluate_prediction launches): ms per launch and GB/s against the floor of reading both operands once
             (2 * F * 3 * H * W * 4 bytes; the two result vectors are negligible).  R blocks for the spread.
  predict    ms per Trainer.predict (bf16, --ch) at B clips of T frames, per size: the generator pass one evaluated future costs.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd import metrics as M                   # noqa: E402
from dvd_gan_amd.train_step import Trainer           # noqa: E402

K_CTX = 4


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


def kernel_level(a, size):
    dev = torch.device("cuda", 0)
    for B in (a.batch, a.batch * a.samples):
        T = a.frames
        gen = torch.Generator(device=dev).manual_seed(0)
        pred = torch.rand(B, T, 3, size, size, device=dev, generator=gen) * 2 - 1
        clips = torch.rand(B, 3, K_CTX + T, size, size, device=dev, generator=gen) * 2 - 1
        target = clips[:, :, K_CTX:].permute(0, 2, 1, 3, 4)
        out = (torch.empty(B, T, device=dev), torch.empty(B, T, device=dev))
        floor_bytes = 2 * B * T * 3 * size * size * 4
        rows = []
        for b in range(a.blocks):
            ms = events(lambda: M.frame_metrics(pred, target, signed=True, quantize=True, out=out), a.launches)
            rows.append(ms)
            print(json.dumps({"kernel": {"block": b, "frames": B * T, "size": size, "ms": round(ms, 4),
                                         "GBps_vs_read_once": round(floor_bytes / ms / 1e6, 1),
                                         "us_per_frame": round(1e3 * ms / (B * T), 4)}}), flush=True)
        print(json.dumps({"kernel_summary": {"frames": B * T, "size": size, "ms_min": round(min(rows), 4),
                                             "ms_max": round(max(rows), 4), "input_MB": round(floor_bytes / 1e6, 1),
                                             "GBps_vs_read_once_best": round(floor_bytes / min(rows) / 1e6, 1)}}), flush=True)
        del pred, clips, target
        torch.cuda.empty_cache()


def predict_level(a, size):
    dev = torch.device("cuda", 0)
    cfg = argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                             lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                             beta2=0.9, n_class=101, k_sample=8, n_cond=K_CTX)
    torch.manual_seed(0)
    tr = Trainer([], cfg, device=dev, compute_dtype=torch.bfloat16, latent_dim=size // 16)
    gen = torch.Generator().manual_seed(1)
    cond = (torch.rand(a.batch, K_CTX, 3, size, size, generator=gen) * 2 - 1).to(dev)
    labels = torch.randint(0, 101, (a.batch,), generator=gen)
    z = torch.randn(a.batch, 120, generator=gen).to(dev)
    ms = events(lambda: tr.predict(cond, labels, z), max(1, a.launches // 4), warmup=2)
    print(json.dumps({"predict": {"batch": a.batch, "frames": a.frames, "size": size, "ch": a.ch, "ms": round(ms, 2)}}), flush=True)
    del tr
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--blocks", type=int, default=3)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--frames", type=int, default=16)
    p.add_argument("--samples", type=int, default=8)
    p.add_argument("--sizes", default="64,128")
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--what", default="kernel,predict")
    a = p.parse_args()
    for size in (int(s) for s in a.sizes.split(",")):
        if "kernel" in a.what.split(","):
            kernel_level(a, size)
        if "predict" in a.what.split(","):
            predict_level(a, size)


if __name__ == "__main__":
    main()

"""What the Inception Score / class-fidelity statistic costs: one classmetrics.LogitStats.update plus result() on logits
[rows, classes] with labels and 10 splits, against the same statistic written with torch fp64 ops on the same device.

usage: python tools/cls_numbers.py [--rows 50000] [--classes 101,1000] [--dtypes fp32,bf16] [--repeats R] [--limit SECONDS]
Every (classes, dtype) configuration runs in a child process of its own under its own time limit and prints one JSON line:
  hip_ms     median over R repeats of update() + result() (a host clock around work that ends in result()'s copy to the host, so
             the workspace allocation, the three launches and the read of the [10, classes + 8] state are all in it)
  torch_ms   median of the torch restatement: log_softmax and exp in fp64 on the device, index_add_ of the rows into the splits,
             topk for the ranks, one copy of the same-sized state to the host
  is_mean    of both, and their relative difference (the two are the same statistic, not the same bits)
A first untimed repeat of each warms up code objects and the caching allocator (profiles/cls_numbers.md).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DTYPES = {"fp32": "float32", "bf16": "bfloat16", "fp16": "float16"}


def torch_statistic(logits, labels, splits):
    """The state LogitStats keeps, with torch ops in fp64 on the device -> (colsum [S, C], stats [S, 5]) on the host."""
    import torch
    n, C = logits.shape
    split = (torch.arange(n, device=logits.device) * splits) // n
    logp = torch.log_softmax(logits.double(), dim=1)
    p = logp.exp()
    col = torch.zeros(splits, C, dtype=torch.float64, device=logits.device).index_add_(0, split, p)
    k = min(5, C)
    top = logits.topk(k, dim=1).indices
    hit1 = (top[:, 0] == labels).double()
    hit5 = (top == labels[:, None]).any(dim=1).double()
    rows = torch.stack([torch.ones(n, dtype=torch.float64, device=logits.device), (p * logp).sum(dim=1),
                        logp.gather(1, labels[:, None].long())[:, 0], hit1, hit5], dim=1)
    st = torch.zeros(splits, 5, dtype=torch.float64, device=logits.device).index_add_(0, split, rows)
    return col.cpu().numpy(), st.cpu().numpy()


def one(a):
    import numpy as np
    import torch
    from dvd_gan_amd.classmetrics import LogitStats
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    rows, C, S = a.rows, int(a.classes), 10
    logits = (3.0 * torch.randn(rows, C, generator=gen)).to(dev).to(getattr(torch, DTYPES[a.dtypes]))
    labels = torch.randint(0, C, (rows,), generator=gen).to(dev).to(torch.int32)

    def hip():
        return LogitStats(C, rows, splits=S, device=dev).update(logits, labels).result()

    def ref():
        return torch_statistic(logits, labels, S)

    times = {}
    for name, fn in (("hip", hip), ("torch", ref), ("hip", hip), ("torch", ref)):          # alternating; the first of each warms up
        fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = fn()
            times.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        times[name + "_out"] = out
    res, (col, st) = times["hip_out"], times["torch_out"]
    q = col / st[:, :1]
    scores = np.exp(st[:, 1] / st[:, 0] - (q * np.log(np.where(q > 0, q, 1.0))).sum(axis=1))
    print(json.dumps({"rows": rows, "classes": C, "dtype": a.dtypes, "splits": S, "repeats": 2 * a.repeats,
                      "hip_ms": round(statistics.median(times["hip"]), 3), "hip_ms_min": round(min(times["hip"]), 3),
                      "torch_ms": round(statistics.median(times["torch"]), 3), "torch_ms_min": round(min(times["torch"]), 3),
                      "is_mean": res["is_mean"], "torch_is_mean": float(scores.mean()),
                      "rel_diff": abs(res["is_mean"] - float(scores.mean())) / res["is_mean"],
                      "top1": res["top1"], "torch_top1": float(st[:, 3].sum() / rows)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--classes", default="101,1000")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds a configuration may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return one(a)
    for C in a.classes.split(","):
        for dtype in a.dtypes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows), "--classes", C, "--dtypes", dtype,
                   "--repeats", str(a.repeats)]
            done = subprocess.run(["timeout", "-k", "10", str(a.limit)] + cmd)
            if done.returncode != 0:                       # a fault, an abort or the time limit: start nothing more on the device
                print(json.dumps({"classes": int(C), "dtype": dtype, "failed": done.returncode}), flush=True)
                return done.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

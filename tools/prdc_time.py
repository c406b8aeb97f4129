"""What precision / recall / density / coverage cost (libdvdgan_hip_prdc.so, distmetrics.prdc) at three sizes, against what a user
would otherwise write on the same device with torch (fp32 torch.cdist in row chunks, kthvalue for the radii, comparisons and
sums for the counts), and against the rate of v_mfma_f32_32x32x2_f32.

usage: python tools/prdc_time.py [--repeats R] [--sizes fvd,10k,50k] [--limit SECONDS] [--no-torch] [--out profiles/prdc_numbers.md]
       python tools/prdc_time.py --size NAME [--repeats R]          (one size in this process: what the first form starts)
The first form never touches the device itself: it starts one child process per size, each under its own time limit, and stops at
the first child that fails or runs out of time (nothing more is started on a device that may have faulted).
  fvd   n = m = 2048,  d = 400,  k = 5        10k   n = m = 10 000, d = 2048, k = 5        50k   n = m = 50 000, d = 512, k = 5
Every figure is the median of --repeats runs between HIP events after one warm-up run of the same shape (min / max beside it).
FLOP counts come from the shapes: "useful" 2 d (n^2 + m^2 + 2 n m), the products of the four distance tables; "computed" counts
the 64 x 64 tiles the pair kernel multiplies (ragged edges included).  The metrics of both paths are printed side by side (the
torch path decides its comparisons in fp32 without a pivot, so a few counts differ near the spheres)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TF = 155.0          # measured rate of v_mfma_f32_32x32x2_f32 on one MI355X (157.3 by the data sheet)
SIZES = {"fvd": (2048, 2048, 400, 5), "10k": (10000, 10000, 2048, 5), "50k": (50000, 50000, 512, 5)}
COLS = ["size", "n", "m", "d", "k", "S", "tiles_per_chunk", "hip_ms", "hip_ms_min", "hip_ms_max", "torch_ms", "torch_ms_min",
        "torch_ms_max", "torch_over_hip", "useful_tflop", "tf_s_useful", "tf_s_computed", "share_of_peak_computed",
        "metrics_hip", "metrics_torch"]


def timed(fn, repeats):
    """ms of fn() between two events: one warm-up run, then the median, min and max of `repeats` runs."""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def torch_prdc(real, fake, k, chunk_bytes=1 << 30):
    """The four metrics with torch alone: distance tables of at most chunk_bytes at a time, never the whole n x m matrix."""
    import torch

    def chunks(x, other):
        step = max(1, chunk_bytes // (4 * other.shape[0]))
        for lo in range(0, x.shape[0], step):
            yield lo, torch.cdist(x[lo:lo + step], other)

    def radii(x):
        # the row itself is in the table at distance 0 (or rounding noise): the k-th other row is the (k + 1)-th smallest
        return torch.cat([dm.kthvalue(k + 1, dim=1).values for _, dm in chunks(x, x)])

    n, m = real.shape[0], fake.shape[0]
    r_real, r_fake = radii(real), radii(fake)
    in_real = torch.cat([(dm <= r_real[None, :]).sum(1) for _, dm in chunks(fake, real)])
    in_fake, covered = [], []
    for lo, dm in chunks(real, fake):
        in_fake.append((dm <= r_fake[None, :]).sum(1))
        covered.append(dm.min(1).values <= r_real[lo:lo + dm.shape[0]])
    in_fake, covered = torch.cat(in_fake), torch.cat(covered)
    table = torch.stack([(in_real > 0).sum().double() / m, (in_fake > 0).sum().double() / n,
                         in_real.sum().double() / (k * m), covered.sum().double() / n]).cpu().tolist()
    return dict(zip(("precision", "recall", "density", "coverage"), table))


def one_size(name, repeats, with_torch=True):
    import torch
    sys.path.insert(0, ROOT)
    from dvd_gan_amd import distmetrics as DM
    n, m, d, k = SIZES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    real = (torch.randn(n, d, generator=gen) + 1.0).to(dev)
    fake = (torch.randn(m, d, generator=gen) * 0.9 + 1.1).to(dev)
    hip = timed(lambda: DM.prdc(real, fake, k=k), repeats)
    res_hip = DM.prdc(real, fake, k=k)
    res_torch = dict.fromkeys(("precision", "recall", "density", "coverage"), float("nan"))
    tch = (float("nan"),) * 3
    if with_torch:
        tch = timed(lambda: torch_prdc(real, fake, k), max(2, repeats // 2))
        res_torch = torch_prdc(real, fake, k)
    tn, tm = -(-n // 64), -(-m // 64)

    def split(own, cand):
        want = min(cand, -(-(-(-2048 // own)) // 8) * 8)
        tpc = -(-cand // want)
        return -(-cand // tpc), tpc
    computed = 2.0 * d * 64 * 64 * (tn * tn + tm * tm + 2 * tn * tm)
    useful = 2.0 * d * (n * n + m * m + 2.0 * n * m)
    keys = ("precision", "recall", "density", "coverage")
    row = {"size": name, "n": n, "m": m, "d": d, "k": k, "S": split(tn, tn)[0], "tiles_per_chunk": split(tn, tn)[1],
           "hip_ms": round(hip[0], 2), "hip_ms_min": round(hip[1], 2), "hip_ms_max": round(hip[2], 2),
           "torch_ms": round(tch[0], 2), "torch_ms_min": round(tch[1], 2), "torch_ms_max": round(tch[2], 2),
           "torch_over_hip": round(tch[0] / hip[0], 2), "useful_tflop": round(useful / 1e12, 3),
           "tf_s_useful": round(useful / hip[0] / 1e9, 1), "tf_s_computed": round(computed / hip[0] / 1e9, 1),
           "share_of_peak_computed": round(computed / hip[0] / 1e9 / PEAK_TF, 3),
           "metrics_hip": [round(res_hip[key], 4) for key in keys], "metrics_torch": [round(res_torch[key], 4) for key in keys],
           "note": "whole prdc() call: pivot, 6 norm passes, 4 pair launches, 4 merges and the one copy to the host"}
    print(json.dumps(row), flush=True)


def table(rows, cols):
    out = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        out.append("| " + " | ".join(str(r.get(c, "")) for c in cols) + " |")
    return "\n".join(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--sizes", default="fvd,10k,50k")
    p.add_argument("--size", default=None)
    p.add_argument("--limit", type=int, default=240)
    p.add_argument("--no-torch", action="store_true", help="time the library alone (A/B runs of DVD_PRDC_LIB_PATH builds)")
    p.add_argument("--out", default=os.path.join("profiles", "prdc_numbers.md"))
    a = p.parse_args()
    if a.size is not None:
        one_size(a.size, a.repeats, not a.no_torch)
        return 0
    rows = []
    for name in a.sizes.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", name, "--repeats", str(a.repeats)]
        cmd += ["--no-torch"] if a.no_torch else []
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            print(f"size {name}: exit status {done.returncode}; nothing more is started", flush=True)
            return done.returncode
        rows += [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]
    parts = ["# Precision / recall / density / coverage: measured cost", "",
             f"`python tools/prdc_time.py` on one MI355X: median of {a.repeats} runs of the whole `distmetrics.prdc()` call between HIP "
             f"events after a warm-up run of the same shape (min / max beside it), against the same four metrics written with "
             f"`torch.cdist` (fp32, row chunks of 1 GiB), `kthvalue` and comparisons.  Peak of `v_mfma_f32_32x32x2_f32`: {PEAK_TF} TF/s "
             "measured.  \"useful\" counts 2 d (n^2 + m^2 + 2 n m), \"computed\" the 64 x 64 tiles the pair kernel multiplies.", "",
             table(rows, COLS), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(parts))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

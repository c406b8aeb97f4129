"""What the distribution distances cost (libdvdgan_hip_eval.so, dvd_gan_amd/distmetrics.py): the three launches at the sizes of a
real evaluation, and one Trainer.evaluate_samples against one training step.

usage: python tools/distmetrics_time.py [--repeats R] [--rows N] [--d D] [--batch B] [--subsets S] [--subset-size Z]
                                        [--what moments,kid,pool,trainer] [--out profiles/distmetrics_numbers.md]
Every figure is the median of --repeats runs between HIP events after one warm-up run of the same shape (the spread is given
beside it); FLOP counts come from the shapes: "computed" counts the 64 x 64 tiles the kernels multiply (upper triangle for the
symmetric products, padding of ragged tiles included), "useful" the products of the definition (n d^2 for a second moment,
3 s^2 d per subset for the three kernel sums).  Peak: 157.3 TF/s of v_mfma_f32_32x32x2_f32.
  moments   FeatureStats.update over --rows x --d features in batches of --batch (the last one ragged)
  kid       kern.eval_kid on --subsets subsets of --subset-size rows of two sets of 10 000 x --d (tables built before the clock)
  pool      kern.eval_pool_features at the benchmark's D_t and D_s head inputs (B = 64, T = 48, k = 8, ch = 32, bf16)
  trainer   bf16 Trainer at the benchmark shape: ms per train_step (the step's code is what the parent commit runs), then
            evaluate_samples(n_samples = 4 batches) with embed "Dt" and "Ds"
Writes the tables to --out (markdown) and prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd import distmetrics as DM              # noqa: E402
from dvd_gan_amd import kern as K                      # noqa: E402
from dvd_gan_amd import lib as L                       # noqa: E402

PEAK_TF = 157.3
DEV = torch.device("cuda", 0)


def timed(fn, repeats):
    """ms of fn() between two events: one warm-up run, then the median, min and max of `repeats` runs."""
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


def tiles(n):
    return (n + L.EVAL_TILE - 1) // L.EVAL_TILE


def moments(a):
    gen = torch.Generator().manual_seed(0)
    x = (torch.randn(a.rows, a.d, generator=gen) + 3.0).to(DEV)
    st = DM.FeatureStats(a.d, DEV)

    def run():
        st.n = 0
        for lo in range(0, a.rows, a.batch):
            st.update(x[lo:lo + a.batch])
    med, lo, hi = timed(run, a.repeats)
    nb = tiles(a.d)
    computed = 2.0 * a.rows * (nb * (nb + 1) // 2) * L.EVAL_TILE ** 2
    useful = 2.0 * a.rows * a.d * a.d
    row = {"what": "moments", "rows": a.rows, "d": a.d, "batch": a.batch, "ms": round(med, 3), "ms_min": round(lo, 3),
           "ms_max": round(hi, 3), "computed_tflop": round(computed / 1e12, 4), "tf_s_computed": round(computed / med / 1e9, 1),
           "tf_s_useful": round(useful / med / 1e9, 1), "share_of_peak_computed": round(computed / med / 1e9 / PEAK_TF, 3)}
    print(json.dumps(row), flush=True)
    return row


def kid(a):
    gen = torch.Generator().manual_seed(1)
    n = max(10000, a.subset_size)
    x, y = torch.randn(n, a.d, generator=gen).to(DEV), (torch.randn(n, a.d, generator=gen) + 0.1).to(DEV)
    ix, iy = DM.kid_subsets(n, n, a.subsets, a.subset_size, 0)
    ix, iy = torch.from_numpy(ix), torch.from_numpy(iy)
    med, lo, hi = timed(lambda: K.eval_kid(x, y, ix, iy), a.repeats)
    nb, s = tiles(a.subset_size), a.subset_size
    computed = 2.0 * a.d * a.subsets * (nb * (nb + 1) + nb * nb) * L.EVAL_TILE ** 2
    useful = 2.0 * a.d * a.subsets * 3 * s * s
    row = {"what": "kid", "subsets": a.subsets, "subset_size": s, "d": a.d, "ms": round(med, 3), "ms_min": round(lo, 3),
           "ms_max": round(hi, 3), "computed_tflop": round(computed / 1e12, 4), "tf_s_computed": round(computed / med / 1e9, 1),
           "tf_s_useful": round(useful / med / 1e9, 1), "share_of_peak_computed": round(computed / med / 1e9 / PEAK_TF, 3),
           "note": "includes the host range check and the upload of the two tables"}
    print(json.dumps(row), flush=True)
    return row


def pool(a):
    rows = []
    for tag, shape, g in (("D_t head input", (64 * 12, 1, 1, 512), 12), ("D_s head input", (64 * 8, 2, 2, 512), 8)):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)
        launches = 200
        med, lo, hi = timed(lambda: [K.eval_pool_features(x, g) for _ in range(launches)], a.repeats)
        nbytes = x.numel() * 2 + shape[0] // g * shape[-1] * 4
        row = {"what": "pool", "shape": tag, "R_P_C_g": [shape[0], shape[1] * shape[2], shape[3], g],
               "us_per_launch": round(med / launches * 1e3, 2), "us_min": round(lo / launches * 1e3, 2),
               "us_max": round(hi / launches * 1e3, 2), "bytes": nbytes,
               "note": "launch-to-launch time of a stream of launches: a megabyte or two of traffic, latency-sized"}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def trainer(a):
    from dvd_gan_amd.train_step import Trainer
    B, T, S, ch, ncls = 64, 48, 64, 32, 101
    cfg = argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=ch, ds_chn=ch, dt_chn=ch, n_frames=T, lr_schr="const",
                             total_epoch=1, d_iters=1, batch_size=B, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9, n_class=ncls,
                             k_sample=8)
    torch.manual_seed(0)
    tr = Trainer([], cfg, device=DEV, compute_dtype=torch.bfloat16, latent_dim=S // 16)
    gen = torch.Generator().manual_seed(1)
    real = (torch.rand(B, 3, T, S, S, generator=gen) * 2 - 1).to(DEV)
    labels = torch.randint(0, ncls, (B,), generator=gen)
    for _ in range(2):
        tr.train_step(real, labels)
    step, s_lo, s_hi = timed(lambda: tr.train_step(real, labels), a.repeats)
    batches = [(real, labels)] * 4
    rows = []
    for embed in ("Dt", "Ds"):
        med, lo, hi = timed(lambda: tr.evaluate_samples(batches, n_samples=4 * B, embed=embed, seed=0), max(3, a.repeats // 2))
        row = {"what": "trainer", "embed": embed, "n_samples": 4 * B, "evaluate_ms": round(med, 1), "evaluate_ms_min": round(lo, 1),
               "evaluate_ms_max": round(hi, 1), "train_step_ms": round(step, 1), "train_step_ms_min": round(s_lo, 1),
               "train_step_ms_max": round(s_hi, 1), "evaluate_over_step": round(med / step, 2),
               "per_clip_over_step_per_clip": round(med / (4 * B) / (step / B), 3)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def table(rows, cols):
    out = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        out.append("| " + " | ".join(str(r.get(c, "")) for c in cols) + " |")
    return "\n".join(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--rows", type=int, default=50000)
    p.add_argument("--d", type=int, default=2048)
    p.add_argument("--batch", type=int, default=1024)
    p.add_argument("--subsets", type=int, default=100)
    p.add_argument("--subset-size", type=int, default=1000)
    p.add_argument("--what", default="moments,kid,pool,trainer")
    p.add_argument("--out", default=os.path.join("profiles", "distmetrics_numbers.md"))
    a = p.parse_args()
    what = a.what.split(",")
    parts = ["# Distribution distances: measured cost", "",
             f"`python tools/distmetrics_time.py` on one MI355X: median of {a.repeats} runs between HIP events after a warm-up run of the "
             f"same shape (min / max beside it).  Peak of `v_mfma_f32_32x32x2_f32`: {PEAK_TF} TF/s.  \"computed\" counts the 64 x 64 "
             "tiles the kernels multiply, \"useful\" the products of the definition.", ""]
    if "moments" in what:
        parts += ["## Second moments", "", table([moments(a)], ["rows", "d", "batch", "ms", "ms_min", "ms_max", "computed_tflop",
                                                                "tf_s_computed", "tf_s_useful", "share_of_peak_computed"]), ""]
        torch.cuda.empty_cache()
    if "kid" in what:
        parts += ["## Kernel distance", "", table([kid(a)], ["subsets", "subset_size", "d", "ms", "ms_min", "ms_max", "computed_tflop",
                                                             "tf_s_computed", "tf_s_useful", "share_of_peak_computed", "note"]), ""]
        torch.cuda.empty_cache()
    if "pool" in what:
        parts += ["## Pooled features", "", table(pool(a), ["shape", "R_P_C_g", "us_per_launch", "us_min", "us_max", "bytes", "note"]), ""]
    if "trainer" in what:
        parts += ["## One evaluation against one training step (bf16, B = 64, T = 48, 64 x 64, ch = 32)", "",
                  table(trainer(a), ["embed", "n_samples", "evaluate_ms", "evaluate_ms_min", "evaluate_ms_max", "train_step_ms",
                                     "train_step_ms_min", "train_step_ms_max", "evaluate_over_step", "per_clip_over_step_per_clip"]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(parts))
    print("wrote", a.out)


if __name__ == "__main__":
    main()

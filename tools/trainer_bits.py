"""Digests of everything a Trainer computes on the paths the benchmark leaves off, for comparing two checkouts bit for bit.

usage: python tools/trainer_bits.py --out FILE.json [--only a|b]
Uses nothing but the public Trainer API, so the same file runs in a checkout of another commit (copy it there: the package it
imports is the one of the tree it lies in).  At the smoke shape (ch = 2, T = 8, 64 x 64, B = 2, n_class = 3, z_dim = 16,
k_sample = 4, the default compute dtype, d_iters = 2, seeded inputs) two configurations:
  a   n_cond = 0 with ema_decay, ema_standing_stats = 2, g_ortho, both clip norms, skip_nonfinite, grad_log, lecam, g_topk, d_stats,
      every d_aug and d_aug_geom group with d_aug_target and d_aug_interval = 1, and sv_log = 1
  b   n_cond = 4 with ema_decay
each: three steps; sample, save_samples, evaluate_samples(embed="Dt", n_samples=4, prdc_k=3), sv_report, guard_report, d_stats
(b: predict, rollout(horizon=12), evaluate_prediction(n_samples=2), save_predictions as well), save_models; one more step;
save_state(wait=True).  FILE.json maps "<configuration>/<what>" to the SHA-256 of every tensor in the state file, every returned
tensor, array or number, and every file written.  Two files are compared with a dict comparison:
  python -c "import json, sys; a, b = (json.load(open(p)) for p in sys.argv[1:]); print(sorted(k for k in a.keys() | b.keys() if a.get(k) != b.get(k)))" A.json B.json
"""
import argparse
import hashlib
import json
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd.train_step import Trainer           # noqa: E402

CH, T, SIZE, B, NCLS, ZD, KS = 2, 8, 64, 2, 3, 16, 4
CONFIGS = {
    "a": dict(n_cond=0, ema_decay=0.9, ema_standing_stats=2, g_ortho=1e-4, g_clip_norm=5.0, d_clip_norm=5.0, skip_nonfinite=True,
              grad_log=4, lecam=0.1, g_topk=0.5, d_stats=True, d_aug="color,translation,cutout",
              d_aug_geom="xflip,rot90,scale,rotate,aniso", d_aug_p=0.7, d_aug_target=0.6, d_aug_interval=1, sv_log=1,
              sample_use_ema=True, sample_layout="both", test_batch_size=2),
    "b": dict(n_cond=4, ema_decay=0.9),
}


def digest(obj, path, out):
    """Flatten `obj` (tensors, arrays, numbers, strings, None in dicts / lists / tuples) into out[path...] = SHA-256."""
    if isinstance(obj, dict):
        for k in obj:
            digest(obj[k], f"{path}/{k}", out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            digest(v, f"{path}/{i}", out)
    elif isinstance(obj, torch.Tensor):
        t = obj.detach().cpu().contiguous()
        raw = t.reshape(-1).view(torch.uint8).numpy().tobytes()
        out[path] = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode() + raw).hexdigest()
    elif isinstance(obj, np.ndarray):
        a = np.ascontiguousarray(obj)
        out[path] = hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()
    else:
        out[path] = hashlib.sha256(repr(obj).encode()).hexdigest()


def run(tag, over, out):
    torch.manual_seed(7)
    random.seed(7)
    np.random.seed(7)
    dev = torch.device("cuda", 0)
    folder = tempfile.mkdtemp(prefix="trainer_bits_")
    cfg = argparse.Namespace(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T, lr_schr="const",
                             total_epoch=1, d_iters=2, batch_size=B, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=NCLS,
                             k_sample=KS, model_save_path=os.path.join(folder, "models"),
                             sample_path=os.path.join(folder, "samples"), version="", **over)
    tr = Trainer([], cfg, device=dev)
    Kc = over["n_cond"]
    gen = torch.Generator().manual_seed(11)
    clips = [(torch.rand(B, 3, Kc + T, SIZE, SIZE, generator=gen) * 2 - 1, torch.randint(0, NCLS, (B,), generator=gen))
             for _ in range(4)]
    for i in range(3):
        digest(tr.train_step(*clips[i]), f"{tag}/step{i}", out)
    z, y = torch.randn(B, ZD, generator=gen), torch.randint(0, NCLS, (B,), generator=gen)
    if Kc:
        long = torch.rand(B, 3, Kc + 12, SIZE, SIZE, generator=gen) * 2 - 1
        cond = clips[0][0][:, :, :Kc].permute(0, 2, 1, 3, 4).contiguous()
        digest(tr.predict(cond, y, z), f"{tag}/predict", out)
        digest(tr.predict(cond, y, truncation=0.8), f"{tag}/predict_drawn", out)
        digest(tr.rollout(cond, y, 12, use_ema=True, standing_stats=1), f"{tag}/rollout", out)
        digest(tr.evaluate_prediction(long, y, horizon=12, n_samples=2, seed=3, truncation=1.5), f"{tag}/evaluate_prediction", out)
        tr.save_predictions(5, long, y, n_samples=2, horizon=12, seed=3)
    else:
        digest(tr.sample(z, y), f"{tag}/sample", out)
        digest(tr.sample(None, y, use_ema=True, truncation=0.8), f"{tag}/sample_drawn", out)
        tr.save_samples(5)
        digest(tr.evaluate_samples(clips[:2], n_samples=4, embed="Dt", prdc_k=3, seed=3), f"{tag}/evaluate_samples", out)
    tr.save_real(clips[0][0])
    digest(tr.sv_report(), f"{tag}/sv_report", out)
    digest(tr.sv_history(), f"{tag}/sv_history", out)
    digest(tr.guard_report(), f"{tag}/guard_report", out)
    digest(tr.d_stats(), f"{tag}/d_stats", out)
    tr.save_models(5)
    digest(tr.train_step(*clips[3]), f"{tag}/step3", out)
    tr.save_state(4, wait=True)
    tr.close_sheets()
    tr.close_state()
    torch.cuda.synchronize()
    state = torch.load(os.path.join(folder, "models", "4_state.pt"), map_location="cpu", weights_only=False)
    digest(state, f"{tag}/state", out)
    digest(torch.get_rng_state(), f"{tag}/default_generator", out)
    for sub in ("models", "samples"):
        for name in sorted(os.listdir(os.path.join(folder, sub))):
            with open(os.path.join(folder, sub, name), "rb") as f:
                out[f"{tag}/file/{sub}/{name}"] = hashlib.sha256(f.read()).hexdigest()
    shutil.rmtree(folder)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", choices=sorted(CONFIGS), default=None)
    a = ap.parse_args()
    out = {}
    for tag, over in CONFIGS.items():
        if a.only in (None, tag):
            run(tag, over, out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(json.dumps({"entries": len(out), "out": a.out}))


if __name__ == "__main__":
    main()

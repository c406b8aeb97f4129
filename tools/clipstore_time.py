"""What producing a batch of real-data clips costs: the device-resident clip store against the host reader.

usage: python tools/clipstore_time.py [--root DIR] [--videos V] [--frames F] [--batch B] [--n-frames T] [--size S]
                                      [--workers W] [--host-batches N] [--store-batches N] [--launches N] [--blocks R]
                                      [--what host,store,kernel]
Writes a synthetic UCF-101-style folder under --root (V videos of F JPEG frames, 240 x 320, two classes; kept if already there),
then prints one JSON line per measurement.  Defaults: the benchmark's clip shape, B = 64 clips of T = 48 frames at 64 x 64.
  host     clips/s of the host reader on that folder: UCF101 + torch DataLoader(batch_size=B, num_workers=W, drop_last=True), the
           dataset and DataLoader arguments of data.make_loader, on a listing that names every video 32 times (so an epoch has
           N batches, N several times W: the workers deliver in bursts of W batches and prefetch 2 W).  Two rates: the whole
           run, worker start-up included, and from the end of the first burst of W batches to the last batch.  Runs in a child
           process of its own that is started BEFORE this process touches the GPU and has no device visible -- workers forked
           from a process with an initialised HIP runtime inherit its device handles, W more holders of a GPU they never
           use --, so it leaves out make_loader's pinning and its device step dvd_clip_to_tensor (asynchronous, timed under
           `kernel` for scale): an upper bound of make_loader's rate.
  store    clips/s of data.make_store_loader over a ClipStore built from the same folder (the build is timed too): R blocks of
           N batches after a warm-up epoch, host clock around iteration that ends in a device synchronise; plus where the host
           time of a batch goes: the draws alone (StoreLoader.draw), and the whole batch() call without waiting for the device.
  kernel   dvd_clip_gather alone on one batch's rows (HIP events, 3 warm-up launches, R blocks of N launches): ms and effective
           GB/s = (crop bytes read once + fp32 bytes written) / time; dvd_clip_to_tensor on a batch of the same shape for scale.
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 240, 320


def _write_video(job):
    import numpy as np
    from PIL import Image
    folder, seed, frames = job
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    ph = rng.uniform(0, 6.28, (3, 2))
    fr = rng.uniform(0.01, 0.08, (3, 2))
    for i in range(1, frames + 1):                  # drifting low-frequency colour fields + mild noise: JPEGs of realistic size
        img = np.stack([127 + 90 * np.sin(fr[c, 0] * x + ph[c, 0] + 0.1 * i) * np.cos(fr[c, 1] * y + ph[c, 1] - 0.07 * i)
                        for c in range(3)], -1) + rng.normal(0, 6, (H, W, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(folder, "image_{:05d}.jpg".format(i)), quality=90)
    with open(os.path.join(folder, "n_frames"), "w") as f:
        f.write(str(frames))


def make_folder(a):
    """<root>/jpg/<class>/<video>/image_%05d.jpg + n_frames; once.json lists every video once, many.json 32 times (links)."""
    import multiprocessing as mp
    jpg = os.path.join(a.root, "jpg")
    once, many = os.path.join(a.root, "once.json"), os.path.join(a.root, "many.json")
    if os.path.exists(many):
        return jpg, once, many
    classes = ["ClassA", "ClassB"]
    jobs, db1, db32 = [], {}, {}
    for v in range(a.videos):
        cls, vid = classes[v % 2], "v_%04d" % v
        jobs.append((os.path.join(jpg, cls, vid), v, a.frames))
        db1[vid] = {"subset": "training", "annotations": {"label": cls}}
    t0 = time.time()
    with mp.Pool(min(16, a.videos)) as pool:
        pool.map(_write_video, jobs)
    for rep in range(32):
        for v in range(a.videos):
            cls, vid = classes[v % 2], "v_%04d" % v
            name = vid if rep == 0 else "%s_r%d" % (vid, rep)
            if rep:
                os.symlink(vid, os.path.join(jpg, cls, name))
            db32[name] = {"subset": "training", "annotations": {"label": cls}}
    for path, db in ((once, db1), (many, db32)):
        with open(path, "w") as f:
            json.dump({"labels": classes, "database": db}, f)
    size = sum(os.path.getsize(os.path.join(j[0], n)) for j in jobs for n in os.listdir(j[0]))
    print(json.dumps({"folder": {"videos": a.videos, "frames_each": a.frames, "jpeg_MB": round(size / 1e6, 1),
                                 "write_s": round(time.time() - t0, 1)}}), flush=True)
    return jpg, once, many


def host_child(a):
    """The host reader alone, in a process that sees no GPU (see the module docstring)."""
    import torch.utils.data as data
    from dvd_gan_amd import data as D
    jpg, once, many = make_folder(a)
    ds = D.UCF101(jpg, many, "training", n_frames=a.n_frames, sample_size=a.size)
    loader = data.DataLoader(ds, batch_size=a.batch, shuffle=True, num_workers=a.workers, drop_last=True)
    random.seed(0)
    t0, arrived = time.time(), []
    for clips, flips, labels in loader:
        arrived.append(time.time())
        if len(arrived) == a.host_batches:
            break
    # every worker fills whole batches, so batches arrive in bursts of W, and with prefetching up to 2 W of them are ready or in the
    # making at any time: a window shorter than several bursts measures the queue, not the readers.  Two rates: the whole run from
    # the creation of the workers, and from the end of the first burst to the end of the last one.
    n, w = len(arrived), a.workers
    whole = n * a.batch / (arrived[-1] - t0)
    steady = (n - w) * a.batch / (arrived[-1] - arrived[w - 1]) if n >= 2 * w else None
    print(json.dumps({"host": {"workers": w, "batches": n, "batch": a.batch, "clip": list(clips.shape[1:]),
                               "first_batch_s": round(arrived[0] - t0, 2), "run_s": round(arrived[-1] - t0, 2),
                               "clips_per_s_whole_run": round(whole, 1),
                               "clips_per_s_after_first_burst": round(steady, 1) if steady else None,
                               "ms_per_frame_per_worker": round(1e3 * w / (whole * a.n_frames), 3)}}), flush=True)


def store_level(a, store, torch):
    from dvd_gan_amd import data as D
    loader = D.make_store_loader(store, a.batch, a.n_frames, a.size, shuffle=True)
    random.seed(0)
    for _ in loader:                                # warm-up: code objects, coefficient tables, pinned blocks
        pass
    torch.cuda.synchronize()
    rates = []
    for block in range(a.blocks):
        n, t0 = 0, time.time()
        while n < a.store_batches:
            for clips, labels in loader:
                n += 1
                if n == a.store_batches:
                    break
        torch.cuda.synchronize()
        dt = time.time() - t0
        rates.append(n * a.batch / dt)
        print(json.dumps({"store": {"block": block, "batches": n, "ms_per_batch": round(1e3 * dt / n, 3),
                                    "clips_per_s": round(rates[-1], 1)}}), flush=True)
    ids = loader.plan_epoch()[0]
    t0 = time.time()
    for _ in range(a.store_batches):
        loader.draw(ids)
    draw_ms = 1e3 * (time.time() - t0) / a.store_batches
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(a.store_batches):
        loader.batch(ids)
    call_ms = 1e3 * (time.time() - t0) / a.store_batches           # returns before the kernel has run
    torch.cuda.synchronize()
    print(json.dumps({"store_summary": {"clips_per_s_min": round(min(rates), 1), "clips_per_s_max": round(max(rates), 1),
                                        "host_draw_ms_per_batch": round(draw_ms, 3),
                                        "host_batch_call_ms": round(call_ms, 3), "tables": len(store._tables)}}), flush=True)


def events(fn, launches, torch, warmup=3):
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


def kernel_level(a, store, torch):
    from dvd_gan_amd import data as D
    from dvd_gan_amd import kern as K
    from dvd_gan_amd import lib as L
    loader = D.make_store_loader(store, a.batch, a.n_frames, a.size, shuffle=False)
    random.seed(1)
    ids = loader.plan_epoch()[0]
    frames, boxes, flips, labels = loader.draw(ids)
    out = store.gather(ids, frames, boxes, flips, a.size)          # builds the tables
    rows = []
    for b in range(a.batch):
        off, h, w, n = store._videos[store._records[ids[b]][0]]
        x0, y0, cw, ch = boxes[b]
        rows += [off, h, w, n, x0, y0, cw, ch, int(flips[b]), store._table(cw, a.size), store._table(ch, a.size)]
    host = torch.tensor(rows + [f - 1 for fr in frames for f in fr], dtype=torch.int64)
    dev = host.to(out.device)
    ms6 = store._ms[next(iter(store._ms))]
    nbytes = sum(cw * ch * 3 for _, _, cw, ch in boxes) * a.n_frames + out.numel() * 4
    best = []
    for block in range(a.blocks):
        ms = events(lambda: K.clip_gather(store.blob, host, dev, store._pool, out, ms6), a.launches, torch)
        best.append(ms)
        print(json.dumps({"kernel": {"block": block, "ms": round(ms, 4), "GBps_effective": round(nbytes / ms / 1e6, 1),
                                     "clips_per_s": round(1e3 * a.batch / ms, 1)}}), flush=True)
    u8 = torch.randint(0, 256, (a.batch, a.n_frames, a.size, a.size, 3), dtype=torch.uint8, device=out.device)
    fl = torch.zeros(a.batch, dtype=torch.uint8, device=out.device)
    ms_t = events(lambda: L.check(L.lib().dvd_clip_to_tensor(L.ptr(u8), L.ptr(fl), L.ptr(out), a.batch, a.n_frames, a.size,
                                                             a.size, 255.0, L.ptr(ms6), L.stream())), a.launches, torch)
    print(json.dumps({"kernel_summary": {"crop_sides": sorted({(cw, ch) for _, _, cw, ch in boxes}), "MB_moved": round(nbytes / 1e6, 1),
                                         "ms_min": round(min(best), 4), "ms_max": round(max(best), 4),
                                         "GBps_effective_best": round(nbytes / min(best) / 1e6, 1),
                                         "clip_to_tensor_ms": round(ms_t, 4)}}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=os.path.join(ROOT, "tools", "scratch", "clipstore_time"))
    p.add_argument("--videos", type=int, default=128)
    p.add_argument("--frames", type=int, default=56)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--n-frames", type=int, default=48)
    p.add_argument("--size", type=int, default=64)
    p.add_argument("--workers", type=int, default=16)
    p.add_argument("--host-batches", type=int, default=64)
    p.add_argument("--store-batches", type=int, default=50)
    p.add_argument("--launches", type=int, default=50)
    p.add_argument("--blocks", type=int, default=3)
    p.add_argument("--what", default="host,store,kernel")
    p.add_argument("--host-child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.host_child:
        return host_child(a)
    what = a.what.split(",")
    jpg, once, many = make_folder(a)
    if "host" in what:                              # before this process opens the GPU; the child sees no device
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--host-child"] + sys.argv[1:], env=env, check=True, timeout=900)
    if "store" in what or "kernel" in what:
        import torch
        from dvd_gan_amd import data as D
        if not torch.cuda.is_available():
            raise SystemExit("clipstore_time.py: no GPU (the store and kernel measurements have no CPU path)")
        ds = D.UCF101(jpg, once, "training", n_frames=a.n_frames, sample_size=a.size)
        t0 = time.time()
        store = D.ClipStore.build(ds, device=torch.device("cuda", 0))
        print(json.dumps({"build": {"records": len(store), "blob_GB": round(store.blob.numel() / 1e9, 3),
                                    "s": round(time.time() - t0, 1)}}), flush=True)
        if "store" in what:
            store_level(a, store, torch)
        if "kernel" in what:
            kernel_level(a, store, torch)


if __name__ == "__main__":
    main()

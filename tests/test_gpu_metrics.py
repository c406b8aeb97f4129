"""GPU checks of the prediction metrics (csrc/metrics.hip, dvd_gan_amd/metrics.py, Trainer.rollout / evaluate_prediction).

Yardstick: the SSIM / MSE definition restated below with a separable F.conv2d in float64 on the CPU, on the fp32 input values.
Allowed deviation per case: max(1e-6, 4 x d32) for ssim (absolute) and the same rule relative for mse, where d32 is the deviation
of THE SAME restatement evaluated in float32 on the CPU from the float64 one -- measured here, never taken from the kernel.  The
factor 4 allows another summation order; the 1e-6 floor is 4 x the largest d32 of the non-degenerate cases (<= 2.5e-7).  The
bright-flat case (0.98 + 1e-3 noise) is the E[x^2] - mu^2 cancellation: d32 = 1.3e-4 at 11 x 11, 2.8e-5 at 16 x 16, 2.3e-6 at
64 x 64.  d32 and the kernel's own deviation of every case go to $DVD_TEST_NUMBERS_DIR/metrics_numbers.json when that names a
directory (profiles/metrics_parity_numbers.md).
"""
import argparse
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
NUMBERS = {}
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _dump():
    d = os.environ.get("DVD_TEST_NUMBERS_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "metrics_numbers.json"), "w") as f:
            json.dump(NUMBERS, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------ the restatement
def _window(dtype):
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def restate(x, y, dtype):
    """x, y [F, C, H, W] (fp32 values) -> (mse [F], ssim [F]) computed in `dtype` on the CPU."""
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    Fr, C_, H, W = x.shape
    g = _window(dtype)
    filt = lambda v: F.conv2d(F.conv2d(v.reshape(Fr * C_, 1, H, W), g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))
    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    smap = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return ((x - y) ** 2).reshape(Fr, -1).mean(1).double(), smap.reshape(Fr, -1).mean(1).double()


def check_case(tag, got, x, y, exact_pair=False):
    """got = (mse, ssim) of the kernel, any shape with F elements; x, y: the [F, C, H, W] values the kernel was to see."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    m64, s64 = restate(x, y, torch.float64)
    m32, s32 = restate(x, y, torch.float32)
    gm, gs = got[0].detach().cpu().double().reshape(-1), got[1].detach().cpu().double().reshape(-1)
    assert gm.shape == m64.shape and gs.shape == s64.shape
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gs).all())
    d32_s, dev_s = float((s32 - s64).abs().max()), float((gs - s64).abs().max())
    nz = m64 > 0
    relerr = lambda a: float(((a[nz] - m64[nz]).abs() / m64[nz]).max()) if bool(nz.any()) else 0.0
    d32_m, dev_m = relerr(m32), relerr(gm)
    NUMBERS[tag] = {"ssim_d32": d32_s, "ssim_dev": dev_s, "mse_rel_d32": d32_m, "mse_rel_dev": dev_m}
    _dump()
    print(f"{tag}: ssim d32 {d32_s:.3g} kernel {dev_s:.3g} | mse rel d32 {d32_m:.3g} kernel {dev_m:.3g}")
    assert dev_s <= max(1e-6, 4 * d32_s), (tag, dev_s, d32_s)
    assert dev_m <= max(1e-6, 4 * d32_m), (tag, dev_m, d32_m)
    assert bool((gm[~nz] == 0).all()), tag                       # an exact match has mse exactly 0
    if exact_pair:
        assert bool((gm == 0).all()) and float((gs - 1).abs().max()) <= 1e-6, (tag, gs)
    return m64, s64


def make_pair(content, Fr, H, W, gen):
    if content == "random":
        return torch.rand(Fr, 3, H, W, generator=gen), torch.rand(Fr, 3, H, W, generator=gen)
    if content == "noisy":
        x = torch.rand(Fr, 3, H, W, generator=gen)
        return x, (x + 0.1 * torch.randn(Fr, 3, H, W, generator=gen)).clamp(0, 1)
    if content == "same":
        x = torch.rand(Fr, 3, H, W, generator=gen)
        return x, x.clone()
    if content == "zeros":
        return torch.zeros(Fr, 3, H, W), torch.zeros(Fr, 3, H, W)
    if content == "bright_flat":
        x = 0.98 + 1e-3 * torch.randn(Fr, 3, H, W, generator=gen)
        return x, x + 1e-3 * torch.randn(Fr, 3, H, W, generator=gen)
    if content == "ramp":
        f, c, h, w = torch.meshgrid(torch.arange(Fr), torch.arange(3), torch.arange(H), torch.arange(W), indexing="ij")
        x = ((3 * h + 5 * w + 7 * c + f) % 17).float() / 16
        return x, torch.roll(x, 1, -1)
    raise KeyError(content)


SIZES = [(11, 11), (12, 29), (16, 16), (64, 64), (128, 128), (21, 256)]
CONTENTS = ["random", "noisy", "same", "zeros", "bright_flat", "ramp"]


# ------------------------------------------------------------------ 1. sizes x contents
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_kernel_matches_fp64_restatement(H, W, content):
    from dvd_gan_amd import metrics as M
    gen = torch.Generator().manual_seed(0)
    x, y = make_pair(content, 4, H, W, gen)
    got = M.frame_metrics(x.view(2, 2, 3, H, W).to(DEV), y.view(2, 2, 3, H, W).to(DEV))
    assert tuple(got[0].shape) == tuple(got[1].shape) == (2, 2) and got[0].dtype == got[1].dtype == torch.float32
    check_case(f"{content}.{H}x{W}", got, x, y, exact_pair=content in ("same", "zeros"))


@pytest.mark.parametrize("content", ["noisy", "bright_flat"])
@pytest.mark.parametrize("H,W", [(40, 150), (40, 180)], ids=["40x150", "40x180"])
def test_intermediate_step_heights(H, W, content):
    """The row step follows the row width: 16 rows up to 130 pixels, 12 up to 158, 8 up to 198, 4 beyond.  The size list above
    reaches 16, 4 and whole-frame steps; these two widths take the 12- and 8-row steps (40 rows: three full steps and a short
    one, resp. five full ones), W % 4 != 0 resp. == 0."""
    from dvd_gan_amd import metrics as M
    gen = torch.Generator().manual_seed(0)
    x, y = make_pair(content, 4, H, W, gen)
    got = M.frame_metrics(x.view(2, 2, 3, H, W).to(DEV), y.view(2, 2, 3, H, W).to(DEV))
    check_case(f"{content}.{H}x{W}", got, x, y)


# ------------------------------------------------------------------ 2. frame counts, determinism
@pytest.mark.parametrize("B,T", [(1, 1), (5, 1), (10, 7)])
@pytest.mark.parametrize("H,W", [(12, 29), (64, 64)])
def test_frame_counts(B, T, H, W):
    from dvd_gan_amd import metrics as M
    gen = torch.Generator().manual_seed(0)
    x, y = make_pair("noisy", B * T, H, W, gen)
    xd, yd = x.view(B, T, 3, H, W).to(DEV), y.view(B, T, 3, H, W).to(DEV)
    got = M.frame_metrics(xd, yd)
    check_case(f"frames{B}x{T}.{H}x{W}", got, x, y)
    again = M.frame_metrics(xd, yd)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])            # two calls: bit-equal
    for f in sorted({0, B * T // 2, B * T - 1}):                                       # a frame alone: the same bits
        b, t = divmod(f, T)
        alone = M.frame_metrics(xd[b, t:t + 1], yd[b, t:t + 1])
        assert tuple(alone[0].shape) == (1,)
        assert torch.equal(alone[0][0], got[0][b, t]) and torch.equal(alone[1][0], got[1][b, t]), f


def test_strip_path_frame_alone_is_bit_equal():
    from dvd_gan_amd import metrics as M
    gen = torch.Generator().manual_seed(0)
    x, y = make_pair("noisy", 6, 128, 128, gen)
    xd, yd = x.view(2, 3, 3, 128, 128).to(DEV), y.view(2, 3, 3, 128, 128).to(DEV)
    got = M.frame_metrics(xd, yd)
    alone = M.frame_metrics(xd[1, 2:3], yd[1, 2:3])
    assert torch.equal(alone[0][0], got[0][1, 2]) and torch.equal(alone[1][0], got[1][1, 2])


# ------------------------------------------------------------------ 3. layouts, alignment, guards
@pytest.mark.parametrize("H,W", [(12, 29), (64, 64), (128, 128)])
def test_loader_view_unaligned_bases_and_guards(H, W):
    """pred as the generator's [B, T, 3, H, W] against target as the [:, :, K:] view of a loader clip [B, 3, K + T, H, W]; then
    both operands one float off 16-byte alignment (the scalar path); the outputs sit inside a sentinel-filled buffer."""
    from dvd_gan_amd import metrics as M
    B, T, K = 3, 2, 2
    gen = torch.Generator().manual_seed(0)
    x, _ = make_pair("random", B * T, H, W, gen)
    x = x.view(B, T, 3, H, W)
    clip = torch.rand(B, 3, K + T, H, W, generator=gen)                 # the context frames differ from everything in x
    y = clip[:, :, K:].permute(0, 2, 1, 3, 4)                           # [B, T, 3, H, W] values
    xd, clipd = x.to(DEV), clip.to(DEV)
    view = clipd[:, :, K:].permute(0, 2, 1, 3, 4)
    assert not view.is_contiguous() and view.data_ptr() != clipd.data_ptr()
    buf = torch.full((2, B * T + 16), -7.0, device=DEV)
    out = (buf[0, 8:8 + B * T].view(B, T), buf[1, 8:8 + B * T].view(B, T))
    got = M.frame_metrics(xd, view, out=out)
    assert got[0].data_ptr() == out[0].data_ptr()
    m64, s64 = check_case(f"loader_view.{H}x{W}", got, x.reshape(-1, 3, H, W), y.reshape(-1, 3, H, W))
    guard = torch.ones_like(buf, dtype=torch.bool)
    guard[:, 8:8 + B * T] = False
    assert bool((buf[guard] == -7.0).all())
    # one float off alignment: the same values through the scalar loads
    n = x.numel()
    xo = torch.empty(n + 1, device=DEV)[1:].view(x.shape)
    yo = torch.empty(clip.numel() + 1, device=DEV)[1:].view(clip.shape)
    xo.copy_(xd)
    yo.copy_(clipd)
    assert xo.data_ptr() % 16 == 4 and yo.data_ptr() % 16 == 4
    off = M.frame_metrics(xo, yo[:, :, K:].permute(0, 2, 1, 3, 4))
    check_case(f"unaligned.{H}x{W}", off, x.reshape(-1, 3, H, W), y.reshape(-1, 3, H, W))
    # the time and batch strides of the view are really used: swapping two target frames moves the results with them
    assert not np.allclose(s64.view(B, T)[:, 0].numpy(), s64.view(B, T)[:, 1].numpy(), atol=1e-4)


# ------------------------------------------------------------------ 4. flags
@pytest.mark.parametrize("H,W", [(16, 16), (64, 64)])
def test_signed_and_quantize_flags(H, W):
    from dvd_gan_amd import metrics as M
    from dvd_gan_amd.helpers import denorm
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(4, 3, H, W, generator=gen) * 2.4 - 1.2
    y = (x + 0.2 * torch.randn(4, 3, H, W, generator=gen)).clamp(-1.2, 1.2)
    xd, yd = x.view(1, 4, 3, H, W).to(DEV), y.view(1, 4, 3, H, W).to(DEV)
    dx, dy = denorm(x.clone()), denorm(y.clone())
    assert float(dx.min()) == 0.0 and float(dx.max()) == 1.0            # the clamp is exercised
    check_case(f"signed.{H}x{W}", M.frame_metrics(xd, yd, signed=True), dx, dy)
    q = lambda v: torch.round(255 * v) / 255
    check_case(f"signed_quantize.{H}x{W}", M.frame_metrics(xd, yd, signed=True, quantize=True), q(dx), q(dy))
    u = torch.rand(4, 3, H, W, generator=gen)
    v = (u + 0.05 * torch.randn(4, 3, H, W, generator=gen)).clamp(0, 1)
    got = M.frame_metrics(u.view(4, 1, 3, H, W).to(DEV), v.view(4, 1, 3, H, W).to(DEV), quantize=True)
    m64, _ = check_case(f"quantize.{H}x{W}", got, q(u), q(v))
    plain, _ = restate(u, v, torch.float64)
    assert float(((m64 - plain).abs() / plain).min()) > 1e-5            # quantisation is visible in the yardstick itself


def test_host_refusals_on_device_tensors():
    from dvd_gan_amd import metrics as M
    a = torch.zeros(2, 2, 3, 16, 16, device=DEV)
    with pytest.raises(ValueError):
        M.frame_metrics(a, a[:, :1])
    with pytest.raises(ValueError):
        M.frame_metrics(a.half(), a.half())
    with pytest.raises(ValueError):
        M.frame_metrics(a[..., :12], a[..., :12])                       # rows no longer contiguous
    with pytest.raises(ValueError):
        M.frame_metrics(a[..., :10, :], a[..., :10, :])


# ------------------------------------------------------------------ 5. rollout and evaluation
CH, K_, T_, KS, B_, NCLS, ZD, SIZE = 2, 2, 6, 2, 2, 3, 8, 64


def _cfg(**extra):
    return argparse.Namespace(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T_, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=B_, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9,
                              n_class=NCLS, k_sample=KS, n_cond=K_, **extra)


@pytest.fixture(scope="module")
def trained():
    """The smallest frame-conditional Trainer (exact mode, a weight average) after two steps, with clips for a horizon of
    2 T - 1 frames; every test starts from the same saved generator state."""
    from dvd_gan_amd.train_step import Trainer
    torch.manual_seed(51)
    tr = Trainer([], _cfg(ema_decay=0.9), device=torch.device(DEV), compute_dtype=torch.float32)
    gen = torch.Generator().manual_seed(52)
    for _ in range(2):
        tr.train_step(torch.rand(B_, 3, K_ + T_, SIZE, SIZE, generator=gen) * 2 - 1, torch.randint(0, NCLS, (B_,), generator=gen))
    clips = torch.rand(B_, 3, K_ + 2 * T_ - 1, SIZE, SIZE, generator=gen) * 2 - 1
    labels = torch.randint(0, NCLS, (B_,), generator=gen)
    return tr, clips, labels, _state(tr)


def _state(tr):
    s = {f"{tag}.{k}": v.detach().clone() for tag, net in (("G", tr.G), ("Ds", tr.D_s), ("Dt", tr.D_t))
         for k, v in net.state_dict().items()}
    opt = tr.g_optimizer
    s["opt.flat"] = opt.flat.detach().clone()
    s["opt.ema"] = opt.ema.detach().clone()
    return s


def _restore(tr, s):
    with torch.no_grad():
        for tag, net in (("G", tr.G), ("Ds", tr.D_s), ("Dt", tr.D_t)):
            for k, v in net.state_dict().items():
                v.copy_(s[f"{tag}.{k}"])
        tr.g_optimizer.flat.copy_(s["opt.flat"])
        tr.g_optimizer.ema.copy_(s["opt.ema"])


def _differing(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def _cond(clips):
    return clips[:, :, :K_].permute(0, 2, 1, 3, 4).contiguous()


def test_rollout_of_n_frames_is_predict(trained):
    tr, clips, labels, s0 = trained
    cond, z = _cond(clips), torch.randn(B_, ZD, generator=torch.Generator().manual_seed(1))
    _restore(tr, s0)
    want = tr.predict(cond, labels, z)
    _restore(tr, s0)
    got = tr.rollout(cond, labels, T_, z=z)
    assert tr.G.training and tuple(got.shape) == (B_, T_, 3, SIZE, SIZE)
    assert torch.equal(got, want)
    # z drawn inside: the same draw from the default generator as predict's
    _restore(tr, s0)
    torch.manual_seed(9)
    want = tr.predict(cond, labels)
    _restore(tr, s0)
    torch.manual_seed(9)
    assert torch.equal(tr.rollout(cond, labels, T_), want)
    with pytest.raises(ValueError, match="truncation"):
        tr.rollout(cond, labels, T_, z=z, truncation=0.5)
    with pytest.raises(ValueError):
        tr.rollout(cond, labels, 0)


def test_rollout_second_chunk_continues_from_the_raw_frames(trained):
    from dvd_gan_amd.helpers import denorm
    tr, clips, labels, s0 = trained
    cond, z = _cond(clips), torch.randn(B_, ZD, generator=torch.Generator().manual_seed(2))
    hz = 2 * T_ - 1
    _restore(tr, s0)
    got = tr.rollout(cond, labels, hz, z=z)
    assert tuple(got.shape) == (B_, hz, 3, SIZE, SIZE) and got.is_contiguous()
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    # weights, spectral-norm u / v, BN statistics and counters: all as before (predict itself advances u / v, quirk 2)
    assert not _differing(s0, _state(tr))
    assert torch.equal(got[:, :T_], tr.predict(cond, labels, z))
    assert _differing(s0, _state(tr))
    _restore(tr, s0)
    tr.G.eval()
    with torch.no_grad():
        raw1 = tr.G(z.to(DEV), labels.to(DEV), cond=cond.to(DEV))
        raw2 = tr.G(z.to(DEV), labels.to(DEV), cond=raw1[:, -K_:].contiguous())
    tr.G.train()
    assert torch.equal(got[:, :T_], denorm(raw1))
    assert torch.equal(got[:, T_:], denorm(raw2)[:, :T_ - 1])
    # conditioning on the denormalised frames mapped back is NOT the same computation
    assert not torch.equal(raw1[:, -K_:], denorm(raw1)[:, -K_:] * 2 - 1)


def test_evaluate_prediction_table_seed_and_rng(trained):
    from dvd_gan_amd import metrics as M
    from dvd_gan_amd.helpers import denorm
    tr, clips, labels, s0 = trained
    hz, N, seed = 2 * T_ - 1, 2, 5
    _restore(tr, s0)
    rng = torch.get_rng_state()
    out = tr.evaluate_prediction(clips, labels, horizon=hz, n_samples=N, seed=seed)
    assert torch.equal(torch.get_rng_state(), rng) and tr.noise_gen is None and tr.G.training
    assert not _differing(s0, _state(tr))                              # spectral-norm u / v included
    tm, ts = out["table"]["mse"], out["table"]["ssim"]
    assert tm.shape == ts.shape == (B_, N, hz)
    for k in ("psnr", "ssim", "psnr_best", "ssim_best"):
        assert out[k].shape == (hz,) and out[k].dtype == np.float64 and np.isfinite(out[k]).all()
    agg = M.aggregate_prediction(tm, ts)
    for k in ("psnr", "ssim", "psnr_best", "ssim_best"):
        np.testing.assert_array_equal(out[k], agg[k])
    assert (out["psnr_best"].mean() >= out["psnr"].mean()) and (out["ssim_best"].mean() >= out["ssim"].mean())
    # the table = frame_metrics of rollout() on z from the same private generator (no restore in between: neither leaves a trace)
    gen = torch.Generator().manual_seed(seed)
    target = denorm(clips[:, :, K_:].permute(0, 2, 1, 3, 4).contiguous().to(DEV))
    for s in range(N):
        r = tr.rollout(_cond(clips), labels, hz, z=torch.randn(B_, ZD, generator=gen))
        m, sm = M.frame_metrics(r, target, quantize=True)
        np.testing.assert_array_equal(tm[:, s], m.cpu().double().numpy())
        np.testing.assert_array_equal(ts[:, s], sm.cpu().double().numpy())
    # the yardstick on one sample: the table holds the metrics of 8-bit frames
    q = lambda v: torch.round(255 * v) / 255
    check_case("evaluate.last_sample", (torch.from_numpy(tm[:, N - 1]), torch.from_numpy(ts[:, N - 1])),
               q(r.cpu()).reshape(-1, 3, SIZE, SIZE), q(target.cpu()).reshape(-1, 3, SIZE, SIZE))
    # same seed: the same bits; another seed: other futures; horizon defaults to n_frames
    again = tr.evaluate_prediction(clips, labels, horizon=hz, n_samples=N, seed=seed)
    np.testing.assert_array_equal(again["table"]["mse"], tm)
    np.testing.assert_array_equal(again["table"]["ssim"], ts)
    other = tr.evaluate_prediction(clips, labels, horizon=hz, n_samples=N, seed=seed + 1)
    assert not np.array_equal(other["table"]["mse"], tm)
    short = tr.evaluate_prediction(clips[:, :, :K_ + T_], labels, seed=seed)
    np.testing.assert_array_equal(short["table"]["mse"][:, 0], tm[:, 0, :T_])
    with pytest.raises(ValueError):
        tr.evaluate_prediction(clips, labels, horizon=T_)                # clip length and horizon disagree
    with pytest.raises(ValueError):
        tr.evaluate_prediction(clips, labels, horizon=hz, n_samples=0)
    assert not _differing(s0, _state(tr))


def test_weight_average_block_is_entered_once_and_leaves_no_trace(trained):
    tr, clips, labels, s0 = trained
    hz = 2 * T_ - 1
    _restore(tr, s0)
    entered = []
    orig = tr.ema_weights

    def counting(*a, **kw):
        entered.append((a, kw))
        return orig(*a, **kw)
    tr.ema_weights = counting
    try:
        live = tr.evaluate_prediction(clips, labels, horizon=hz, n_samples=2, seed=3)
        assert entered == []
        assert not _differing(s0, _state(tr))
        avg = tr.evaluate_prediction(clips, labels, horizon=hz, n_samples=2, seed=3, use_ema=True, standing_stats=1)
        assert len(entered) == 1
        assert not _differing(s0, _state(tr))                            # u / v included: the block puts them back
        r = tr.rollout(_cond(clips), labels, hz, use_ema=True)
        assert len(entered) == 2 and tuple(r.shape) == (B_, hz, 3, SIZE, SIZE)
        assert not _differing(s0, _state(tr))
    finally:
        tr.ema_weights = orig
    assert not np.array_equal(avg["table"]["mse"], live["table"]["mse"])
    with pytest.raises(ValueError, match="use_ema"):
        tr.rollout(_cond(clips), labels, hz, standing_stats=1)
    # a Trainer without context frames: the errors of predict()
    tr.n_cond = 0
    try:
        for call in (lambda: tr.predict(_cond(clips), labels), lambda: tr.rollout(_cond(clips), labels, hz),
                     lambda: tr.evaluate_prediction(clips, labels, horizon=hz)):
            with pytest.raises(RuntimeError, match="frame-conditional"):
                call()
    finally:
        tr.n_cond = K_

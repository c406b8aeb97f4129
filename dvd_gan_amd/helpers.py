"""utils.py:60-63 / :77-83 of the reference on HIP kernels (reference-layout fp32 tensors)."""
import math

import torch

from . import functional as Fn


def to_device_async(t, device):
    """Host tensor -> device without stalling the host: through a pinned staging block, non_blocking.  A plain `.to(device)`
    of pageable memory makes the host wait for everything queued on the current stream -- once per step that keeps the host
    from running ahead of the GPU, and every launch gap of the step's Python becomes GPU idle time.  (The pinned block comes
    from torch's caching host allocator, which reuses it only after the copy has executed.)"""
    if t.is_cuda or not torch.cuda.is_available():
        return t.to(device)
    if not t.is_pinned():
        if t.numel() * t.element_size() > (1 << 20):
            return t.to(device)           # a batch of clips: pin it in the loader (make_loader does); no extra host copy here
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def draw_frame_ids(video_length, k_sample, generator=None):
    """`torch.randperm(T)[:k].sort()` on the CPU default generator, like the reference."""
    perm = torch.randperm(video_length, generator=generator)
    return perm[:k_sample].sort()[0]


def sample_k_frames(data, video_length, k_sample, frame_ids=None):
    """data [B,T,C,H,W] -> [B,k,C,H,W]; the same k sorted random frames for the whole batch."""
    if frame_ids is None:
        frame_ids = draw_frame_ids(video_length, k_sample)
    return Fn.GatherFrames.apply(data, frame_ids)


def vid_downsample(data):
    """[B,T,C,H,W] -> per-frame 2x2 average -> [B,C,T,H/2,W/2]"""
    return Fn.VidDownsample.apply(data)


def vid_downsample_cat(context, data):
    """vid_downsample(torch.cat([context, data], 1)) without the concatenated clip: [B,Tc,C,H,W] + [B,T,C,H,W] ->
    [B,C,Tc+T,H/2,W/2]; the gradient reaches `data` only (the context frames are data)."""
    return Fn.VidDownsampleCat.apply(context, data)


def denorm(x):
    """utils.py:41-43: [-1, 1] -> [0, 1], clamped."""
    return ((x + 1) / 2).clamp_(0, 1)


def truncated_z(B, z_dim, tau, generator=None):
    """[B, z_dim] fp32 draws of N(0, 1) truncated to [-tau, tau] (the truncation trick) by the inverse CDF:
    sqrt(2) erfinv(2 p - 1) with p uniform in [Phi(-tau), Phi(tau)], in fp64, clamped, then rounded to float.  One uniform
    draw per element from `generator` (default generator when None): no rejection loop, reproducible."""
    tau = float(tau)
    if not tau > 0.0:
        raise ValueError(f"truncation={tau} must be positive")
    lo = 0.5 * (1.0 + math.erf(-tau / math.sqrt(2.0)))
    hi = 0.5 * (1.0 + math.erf(tau / math.sqrt(2.0)))
    p = lo + (hi - lo) * torch.rand(B, z_dim, dtype=torch.float64, generator=generator)
    z = math.sqrt(2.0) * torch.erfinv(2.0 * p - 1.0)
    t32 = torch.tensor(tau, dtype=torch.float32)
    if float(t32) > tau:                            # the largest float not above tau: |z| <= tau holds in exact arithmetic
        t32 = torch.nextafter(t32, torch.zeros(()))
    return z.clamp_(-tau, tau).float().clamp_(-float(t32), float(t32))

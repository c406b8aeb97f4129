"""Prediction metrics that need no pretrained network: per-frame MSE / PSNR and SSIM (Wang et al. 2004) of predicted frames
against the held-out real ones, on the HIP kernel of csrc/metrics.hip (dvd_frame_metrics), and the best-of-N aggregation of
Trainer.evaluate_prediction.  FVD, IS / FID and LPIPS need a pretrained network and stay out."""
import numpy as np
import torch

from . import kern as K

from .lib import METRICS_MAX_SIDE as MAX_SIDE, METRICS_MIN_SIDE as MIN_SIDE


def _batch_strides(t, name):
    """[..., T, C, H, W] tensor or view -> (B, batch stride) with the leading axes folded into one."""
    H, W = t.shape[-2:]
    if t.stride(-1) != 1 or t.stride(-2) != W:
        raise ValueError(f"{name}: the H x W planes must be contiguous (strides {t.stride()[-2:]} for {H} x {W})")
    B, sb = 1, 0
    for size, stride in zip(reversed(t.shape[:-4]), reversed(t.stride()[:-4])):
        if size == 1:
            continue
        if B != 1 and stride != sb * B:
            raise ValueError(f"{name}: the leading axes {tuple(t.shape[:-4])} with strides {t.stride()[:-4]} do not fold into one "
                             "batch axis")
        if B == 1:
            sb = stride
        B *= size
    return B, sb


def frame_metrics(pred, target, *, signed=False, quantize=False, out=None):
    """pred, target: device fp32 tensors or views shaped [..., T, C, H, W] with contiguous H x W planes (any batch / time / channel
    strides: the generator's [B, T, 3, H, W] and `clips[:, :, K:].permute(0, 2, 1, 3, 4)` of a loader clip [B, 3, K + T, H, W] are
    both served without a copy) -> (mse, ssim), fp32 device tensors of the leading shape + [T].
    signed: the operands are in [-1, 1] and are mapped to [0, 1] like helpers.denorm (clamped) on load; otherwise they are taken
    as [0, 1] values.  quantize: then rounded to 8 bits (round(255 x) / 255), as published numbers are computed on 8-bit images.
    SSIM: 11 x 11 Gaussian window (sigma 1.5), "valid" windows, C1 = 0.01^2, C2 = 0.03^2, mean over windows and channels.
    out = (mse, ssim): contiguous fp32 device buffers of that shape to fill instead of fresh ones.  No host sync."""
    if pred.shape != target.shape or pred.dim() < 4:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must both be [..., T, C, H, W]")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"frame metrics take fp32 frames, got {pred.dtype} / {target.dtype}")
    T, Cc, H, W = pred.shape[-4:]
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f"frames of {H} x {W} are smaller than the {MIN_SIDE} x {MIN_SIDE} SSIM window")
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"frames of {H} x {W}: the kernel serves sides up to {MAX_SIDE}")
    (B, p_sb), (_, t_sb) = _batch_strides(pred, "pred"), _batch_strides(target, "target")
    if not (pred.is_cuda and target.is_cuda and pred.device == target.device):
        raise ValueError("frame metrics take two tensors on one GPU (there is no CPU path)")
    lead = tuple(pred.shape[:-3])
    if out is None:
        mse = torch.empty(lead, dtype=torch.float32, device=pred.device)
        ssim = torch.empty(lead, dtype=torch.float32, device=pred.device)
    else:
        mse, ssim = out
        for t in (mse, ssim):
            if tuple(t.shape) != lead or t.dtype != torch.float32 or not t.is_contiguous() or t.device != pred.device:
                raise ValueError(f"out: contiguous fp32 device tensors of shape {lead}")
    if B * T * Cc == 0:
        return mse, ssim
    flags = (K.METRICS_SIGNED if signed else 0) | (K.METRICS_QUANTIZE if quantize else 0)
    K.frame_metrics(pred, (p_sb, pred.stride(-4), pred.stride(-3)), target, (t_sb, target.stride(-4), target.stride(-3)),
                    B, T, Cc, H, W, flags, mse, ssim)
    return mse, ssim


def psnr(mse):
    """10 log10(1 / mse) for images in [0, 1], in fp64 on the host (a tensor is copied there); +inf where mse is 0.
    -> numpy float64 array of mse's shape."""
    if isinstance(mse, torch.Tensor):
        mse = mse.detach().cpu().numpy()
    m = np.asarray(mse, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(1.0 / m)


def aggregate_prediction(mse, ssim):
    """The tables of Trainer.evaluate_prediction, [B clips, N samples, horizon] each -> the curves over the horizon (fp64):
    psnr / ssim = mean over clips and samples; psnr_best / ssim_best = mean over clips of the ONE sample per clip whose mean over
    the horizon of THAT metric is highest (best-of-N, chosen per metric: the two may pick different samples).  A frame with
    mse = 0 has PSNR +inf, and so has every mean it enters."""
    mse = np.asarray(mse, dtype=np.float64)
    ssim = np.asarray(ssim, dtype=np.float64)
    if mse.shape != ssim.shape or mse.ndim != 3:
        raise ValueError(f"tables must both be [B, n_samples, horizon], got {mse.shape} / {ssim.shape}")
    p = psnr(mse)
    clip = np.arange(mse.shape[0])
    with np.errstate(invalid="ignore"):
        best_p, best_s = p.mean(axis=2).argmax(axis=1), ssim.mean(axis=2).argmax(axis=1)
        return {"psnr": p.mean(axis=(0, 1)), "ssim": ssim.mean(axis=(0, 1)),
                "psnr_best": p[clip, best_p].mean(axis=0), "ssim_best": ssim[clip, best_s].mean(axis=0),
                "table": {"mse": mse, "ssim": ssim}}

"""Clip-consistent differentiable augmentation of what the discriminators see (Zhao et al. 2020, "DiffAugment"), with a
probability that can follow the overfitting indicator r_t (Karras et al. 2020, "ADA").  The transform and its transpose are the
two launches of libdvdgan_hip_aug.so (include/dvdgan_hip_aug.h states the arithmetic); this module draws the parameter tables on
the host, wraps the launches for autograd and holds the rule that moves p.  Every frame of a clip shares one parameter row: a
video discriminator must not see the transform flicker from frame to frame."""
import torch

from . import lib as L
from .clip_op import clip_op

POLICIES = ("color", "translation", "cutout")
IDENTITY_ROW = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)       # b, s, c, dx, dy, cy0, cx0, ch, cw


def parse_policy(policy):
    """"color,translation,cutout" (any subset, any order, "" = none) -> the names in POLICIES order.  ValueError on another name."""
    names = [n.strip() for n in str(policy or "").split(",") if n.strip()]
    unknown = [n for n in names if n not in POLICIES]
    if unknown:
        raise ValueError(f"d_aug: unknown augmentation {unknown[0]!r} (known: {', '.join(POLICIES)})")
    return tuple(n for n in POLICIES if n in names)


def draw_params(B, H, W, policy, p, generator=None):
    """-> [B, lib.AUG_COLS] fp32 host table, one row per clip.  ONE call torch.rand(B, 10, float64) whatever `policy` and `p`
    are, so the position of `generator`'s stream after a call depends on neither.  Columns of the draw: colour gate, b, s, c,
    translation gate, dx, dy, cutout gate, cy, cx; a group applies to a clip when its gate is < p and it is in the policy, every
    other group keeps its identity columns.  Ranges (DiffAugment's): b in [-0.5, 0.5), s in [0, 2), c in [0.5, 1.5); dx uniform
    over the integers of [-rx, rx], rx = floor(W / 8 + 0.5), dy likewise with H; the cutout is floor(H / 2 + 0.5) x
    floor(W / 2 + 0.5) about a centre uniform over the frame's pixels, and may stick out of the frame."""
    policy = parse_policy(policy) if isinstance(policy, str) else tuple(policy)
    B, H, W, p = int(B), int(H), int(W), float(p)
    u = torch.rand(B, 10, dtype=torch.float64, generator=generator)
    out = torch.tensor(IDENTITY_ROW, dtype=torch.float64).repeat(B, 1)
    if "color" in policy:
        on = u[:, 0] < p
        out[:, L.AUG_B] = torch.where(on, u[:, 1] - 0.5, out[:, L.AUG_B])
        out[:, L.AUG_S] = torch.where(on, u[:, 2] * 2.0, out[:, L.AUG_S])
        out[:, L.AUG_C] = torch.where(on, u[:, 3] + 0.5, out[:, L.AUG_C])
    if "translation" in policy:
        on = u[:, 4] < p
        rx, ry = int(W / 8 + 0.5), int(H / 8 + 0.5)
        dx = torch.floor(u[:, 5] * (2 * rx + 1)).clamp_(max=2 * rx) - rx
        dy = torch.floor(u[:, 6] * (2 * ry + 1)).clamp_(max=2 * ry) - ry
        out[:, L.AUG_DX] = torch.where(on, dx, out[:, L.AUG_DX])
        out[:, L.AUG_DY] = torch.where(on, dy, out[:, L.AUG_DY])
    if "cutout" in policy:
        on = u[:, 7] < p
        ch, cw = int(H / 2 + 0.5), int(W / 2 + 0.5)
        cy = torch.floor(u[:, 8] * H).clamp_(max=H - 1)
        cx = torch.floor(u[:, 9] * W).clamp_(max=W - 1)
        zero = torch.zeros(B, dtype=torch.float64)
        out[:, L.AUG_CY0] = torch.where(on, cy - ch // 2, zero)
        out[:, L.AUG_CX0] = torch.where(on, cx - cw // 2, zero)
        out[:, L.AUG_CH] = torch.where(on, torch.full_like(zero, ch), zero)
        out[:, L.AUG_CW] = torch.where(on, torch.full_like(zero, cw), zero)
    return out.float()


_forward, _backward, _ClipOp = clip_op("ClipAugment", L.aug_lib, "dvd_aug_clip_forward", "dvd_aug_clip_backward", L.aug_check,
                                       L.AUG_COLS, "clip augmentation", "the parameter table")


def clip_forward(frames, params, frames_per_clip):
    """frames [N, 3, H, W] fp32 on the device, frame n of clip n // frames_per_clip; params [clips, lib.AUG_COLS] -> the
    transformed frames (dvd_aug_clip_forward).  No autograd."""
    return _forward(frames, params, frames_per_clip)


def clip_backward(grad, params, frames_per_clip):
    """The transpose of clip_forward applied to grad (dvd_aug_clip_backward)."""
    return _backward(grad, params, frames_per_clip)


class ClipAugment(_ClipOp):
    """apply(frames5d [B, T, 3, H, W], params [B, lib.AUG_COLS] on the device) -> the augmented clips.  The map is affine in the
    frames, so only `params` is saved; the table receives no gradient."""


def ada_update(p, r_t, target, batch, interval, kimg):
    """The next augmentation probability (Karras et al. 2020): p moves towards 1 while r_t is above `target` and towards 0 while it
    is below, by the share batch * interval of kimg thousand images -- p crosses [0, 1] in kimg thousand real clips.  Pure."""
    sign = (r_t > target) - (r_t < target)
    return min(1.0, max(0.0, float(p) + sign * float(batch) * float(interval) / (float(kimg) * 1000.0)))

"""Clip-consistent geometric augmentation of what the discriminators see: the geometric group of Karras et al. 2020 ("ADA") --
mirror, quarter turns, isotropic scaling, rotation, anisotropic scaling -- as one affine warp per clip with bilinear interpolation
and zero fill.  The warp and its exact transpose are the two launches of libdvdgan_hip_geom.so (include/dvdgan_hip_geom.h states
the arithmetic: deterministic, no atomics); this module draws the tables on the host and wraps the launches for autograd.  Every
frame of a clip shares one row, as in augment.py, whose probability p and private generator the Trainer shares with this module."""
import math

import torch

from . import lib as L
from .clip_op import clip_op

GEOM_POLICIES = ("xflip", "rot90", "scale", "rotate", "aniso")
IDENTITY_ROW = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)       # a00, a01, a02, a10, a11, a12
SCALE_STD, SCALE_CLAMP = 0.2, 3.0                   # s = 2^(SCALE_STD * n), n standard normal clamped to +-SCALE_CLAMP
_QUARTER = ((1.0, 0.0, 0.0, 1.0), (0.0, 1.0, -1.0, 0.0), (-1.0, 0.0, 0.0, -1.0), (0.0, -1.0, 1.0, 0.0))


def parse_geom(policy):
    """"xflip,rot90,scale,rotate,aniso" (any subset, any order, "" = none) -> the names in GEOM_POLICIES order.  ValueError on
    another name."""
    names = [n.strip() for n in str(policy or "").split(",") if n.strip()]
    unknown = [n for n in names if n not in GEOM_POLICIES]
    if unknown:
        raise ValueError(f"d_aug_geom: unknown augmentation {unknown[0]!r} (known: {', '.join(GEOM_POLICIES)})")
    return tuple(n for n in GEOM_POLICIES if n in names)


def _log_normal(u1, u2):
    """s = 2^(0.2 n), n = sqrt(-2 ln(1 - u1)) cos(2 pi u2) clamped to [-3, 3]: Box-Muller on two uniforms of [0, 1)."""
    n = torch.sqrt(-2.0 * torch.log1p(-u1)) * torch.cos(2.0 * math.pi * u2)
    return torch.exp2(SCALE_STD * n.clamp(-SCALE_CLAMP, SCALE_CLAMP))


def _mat(m00, m01, m10, m11):
    return torch.stack([torch.stack([m00, m01], -1), torch.stack([m10, m11], -1)], -2)


def draw_geom(B, H, W, policy, p, generator=None):
    """-> [B, lib.GEOM_COLS] fp32 host table, one row a00, a01, a02, a10, a11, a12 per clip (output pixel index -> source position,
    include/dvdgan_hip_geom.h).  ONE call torch.rand(B, 11, float64) whatever `policy` and `p` are, so the position of
    `generator`'s stream after a call depends on neither.  Columns of the draw: xflip gate; rot90 gate, k; scale gate, u1, u2;
    rotate gate, theta; aniso gate, u1, u2.  A group applies to a clip when its gate is < p and it is in the policy.
    Each group moves the CONTENT by a 2 x 2 matrix on coordinates (x to the right, y down) about the frame centre
    c = ((W - 1) / 2, (H - 1) / 2); with R(t) = [[cos t, sin t], [-sin t, cos t]], a turn by t counter-clockwise on the screen:
        xflip   F = diag(-1, 1)
        rot90   Q = R(k pi / 2) with its exact entries 0 and +-1, k = floor(4 u) in {0, 1, 2, 3} (torch.rot90(frame, k));
                ValueError when H != W
        scale   S = diag(s, s),      s = 2^(0.2 n), n = sqrt(-2 ln(1 - u1)) cos(2 pi u2) clamped to [-3, 3]
        rotate  R(theta),            theta = (2 u - 1) pi in [-pi, pi)
        aniso   N = diag(s, 1 / s),  s drawn as for scale from its own u1, u2
    (a group that does not apply is the unit matrix).  Composed in fp64 in the order listed, G = N R S Q F, a content point z goes
    to G (z - c) + c; the row is the inverse map, output -> source, rounded once to fp32:
        [[a00, a01], [a10, a11]] = G^-1,      (a02, a12) = c - G^-1 c
    Rows made of xflip and rot90 alone have entries 0 and +-1 and integer offsets; a clip no group applies to gets the identity row
    1, 0, 0, 0, 1, 0 exactly (the launch copies such a clip bit for bit)."""
    policy = parse_geom(policy) if isinstance(policy, str) else tuple(policy)
    B, H, W, p = int(B), int(H), int(W), float(p)
    u = torch.rand(B, 11, dtype=torch.float64, generator=generator)
    if "rot90" in policy and H != W:
        raise ValueError(f"d_aug_geom: rot90 turns square frames only, got {H} x {W}")
    one, zero = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    unit = _mat(one, zero, zero, one)
    G = unit

    def compose(G, name, gate, M):
        if name not in policy:
            return G
        return torch.where((u[:, gate] < p)[:, None, None], M @ G, G)
    G = compose(G, "xflip", 0, _mat(-one, zero, zero, one))
    k = torch.floor(u[:, 2] * 4).clamp_(max=3).long()
    G = compose(G, "rot90", 1, torch.tensor(_QUARTER, dtype=torch.float64)[k].view(B, 2, 2))
    s = _log_normal(u[:, 4], u[:, 5])
    G = compose(G, "scale", 3, _mat(s, zero, zero, s))
    theta = (2.0 * u[:, 7] - 1.0) * math.pi
    G = compose(G, "rotate", 6, _mat(torch.cos(theta), torch.sin(theta), -torch.sin(theta), torch.cos(theta)))
    s = _log_normal(u[:, 9], u[:, 10])
    G = compose(G, "aniso", 8, _mat(s, zero, zero, 1.0 / s))
    det = G[:, 0, 0] * G[:, 1, 1] - G[:, 0, 1] * G[:, 1, 0]
    A = _mat(G[:, 1, 1] / det, -G[:, 0, 1] / det, -G[:, 1, 0] / det, G[:, 0, 0] / det)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    out = torch.stack([A[:, 0, 0], A[:, 0, 1], cx - A[:, 0, 0] * cx - A[:, 0, 1] * cy,
                       A[:, 1, 0], A[:, 1, 1], cy - A[:, 1, 0] * cx - A[:, 1, 1] * cy], 1)
    return (out + 0.0).float()                       # (+ 0.0: no negative zeros in the table)


_forward, _backward, _ClipOp = clip_op("ClipWarp", L.geom_lib, "dvd_geom_clip_forward", "dvd_geom_clip_backward", L.geom_check,
                                       L.GEOM_COLS, "the clip warp", "the table")


def clip_warp_forward(frames, mats, frames_per_clip):
    """frames [N, 3, H, W] fp32 on the device, frame n of clip n // frames_per_clip; mats [clips, lib.GEOM_COLS] -> the warped
    frames (dvd_geom_clip_forward).  No autograd."""
    return _forward(frames, mats, frames_per_clip)


def clip_warp_backward(grad, mats, frames_per_clip):
    """The transpose of clip_warp_forward applied to grad (dvd_geom_clip_backward)."""
    return _backward(grad, mats, frames_per_clip)


class ClipWarp(_ClipOp):
    """apply(frames5d [B, T, 3, H, W], mats [B, lib.GEOM_COLS] on the device) -> the warped clips.  The map is linear in the frames,
    so only `mats` is saved; the table receives no gradient."""

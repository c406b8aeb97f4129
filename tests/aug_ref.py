"""The clip augmentation of include/dvdgan_hip_aug.h restated in fp64 torch with plain indexing, differentiable by autograd: what
the GPU tests compare dvd_aug_clip_forward / dvd_aug_clip_backward with.  Every function also serves `mag`, the same expression
on absolute values -- the size of the quantities the device rounds, which the tests' bound is proportional to."""
import torch

COLS = 9
IDENTITY = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)        # b, s, c, dx, dy, cy0, cx0, ch, cw
E32 = 2.0 ** -24
ROUNDINGS = 12              # the documented order has at most 11 fp32 roundings, each on a quantity bounded by mag; one to spare


def _place(y, row, transpose=False):
    """Translation then cutout of one frame [3, H, W] (zero fill), or the transpose of the two."""
    _, _, _, dx, dy, cy0, cx0, ch, cw = (int(v) if i >= 3 else v for i, v in enumerate(row))
    _, H, W = y.shape
    r0, r1, c0, c1 = max(cy0, 0), min(cy0 + ch, H), max(cx0, 0), min(cx0 + cw, W)
    cut = ch != 0 and cw != 0 and r0 < r1 and c0 < c1
    h0, h1, w0, w1 = max(dy, 0), min(H + dy, H), max(dx, 0), min(W + dx, W)        # the output pixels whose source is inside
    out = torch.zeros_like(y)
    if not transpose:
        if h0 < h1 and w0 < w1:
            out[:, h0:h1, w0:w1] = y[:, h0 - dy:h1 - dy, w0 - dx:w1 - dx]
        if cut:
            out[:, r0:r1, c0:c1] = 0.0
        return out
    g = y.clone()
    if cut:
        g[:, r0:r1, c0:c1] = 0.0
    if h0 < h1 and w0 < w1:
        out[:, h0 - dy:h1 - dy, w0 - dx:w1 - dx] = g[:, h0:h1, w0:w1]
    return out


def frame(x, row):
    """x [3, H, W] fp64 -> the transformed frame.  Stages whose parameter is the identity are skipped, as on the device."""
    b, s, c = (float(v) for v in row[:3])
    y = x
    if b != 0.0:
        y = y + b
    if s != 1.0:
        m1 = (y[0] + y[1] + y[2]) * (1.0 / 3.0)
        y = (y - m1) * s + m1
    if c != 1.0:
        m2 = x.sum() / x.numel() + b
        y = (y - m2) * c + m2
    return _place(y, row)


def frame_mag(x, row):
    """The expression of frame() on absolute values: a = |x| + |b|, a1 = (a + mean_c a) s + mean_c a, (a1 + mean a) c + mean a."""
    b, s, c = (abs(float(v)) for v in row[:3])
    a = x.abs() + b
    mc = (a[0] + a[1] + a[2]) * (1.0 / 3.0)
    a1 = (a + mc) * s + mc
    m = a.sum() / a.numel()
    return _place((a1 + m) * c + m, row)


def grad_mag(g, row):
    """The same expression for the backward pass, |g| in place of |x| (b does not enter a gradient): on the gradient as the
    transposed translation and cutout leave it."""
    return frame_mag(_place(g.abs(), row, transpose=True), (0.0,) + tuple(row[1:3]) + IDENTITY[3:])


def clip(x, params, frames_per_clip):
    """x [N, 3, H, W] (any float dtype), params [clips, 9] -> (y, mag) in fp64 on the host: the transform and its magnitude.
    Frame n takes row n // frames_per_clip."""
    x64 = x.detach().double().cpu()
    rows = torch.as_tensor(params).double().cpu().tolist()
    y = torch.stack([frame(x64[n], rows[n // frames_per_clip]) for n in range(x64.shape[0])])
    mag = torch.stack([frame_mag(x64[n], rows[n // frames_per_clip]) for n in range(x64.shape[0])])
    return y, mag


def clip_grad(x, g, params, frames_per_clip):
    """-> (dx, dmag): autograd's gradient of sum(clip(x) * g) with respect to x, and its magnitude."""
    x64 = x.detach().double().cpu().requires_grad_(True)
    g64 = g.detach().double().cpu()
    rows = torch.as_tensor(params).double().cpu().tolist()
    y = torch.stack([frame(x64[n], rows[n // frames_per_clip]) for n in range(x64.shape[0])])
    # (a row that masks every pixel leaves an output that does not depend on x at all: its gradient is zero)
    dx = torch.autograd.grad(y, x64, g64, allow_unused=True)[0] if y.requires_grad else None
    dx = torch.zeros_like(g64) if dx is None else dx
    dmag = torch.stack([grad_mag(g64[n], rows[n // frames_per_clip]) for n in range(x64.shape[0])])
    return dx, dmag


def hand_rows(H, W):
    """name -> row: the hand-made rows of the GPU tests at a frame size."""
    ch, cw = int(H / 2 + 0.5), int(W / 2 + 0.5)
    ry = int(H / 8 + 0.5)
    return {
        "identity": IDENTITY,
        "colour": (0.3, 1.7, 0.6, 0, 0, 0, 0, 0, 0),
        "saturation only": (0.0, 0.25, 1.0, 0, 0, 0, 0, 0, 0),
        "contrast only": (0.0, 1.0, 1.4, 0, 0, 0, 0, 0, 0),
        "dx = W - 1": (0.0, 1.0, 1.0, W - 1, 0, 0, 0, 0, 0),
        "dx = -W": (0.0, 1.0, 1.0, -W, 0, 0, 0, 0, 0),
        "dy low": (0.0, 1.0, 1.0, 0, -ry, 0, 0, 0, 0),
        "dy high": (0.0, 1.0, 1.0, 0, ry, 0, 0, 0, 0),
        "cutout half outside": (0.0, 1.0, 1.0, 0, 0, -(ch // 2), W - cw // 2 - 1, ch, cw),
        "cutout covers the frame": (0.0, 1.0, 1.0, 0, 0, -1, -2, H + 3, W + 5),
        "everything": (-0.4, 0.1, 1.45, -(W // 8), ry, H // 3, -1, ch, cw),
        "everything, aligned shift": (0.45, 1.9, 0.5, 4 if W > 4 else 1, -1, H // 2, W // 2, ch, cw),
    }

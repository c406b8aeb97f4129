"""The clip warp of include/dvdgan_hip_geom.h restated in fp64 torch with plain indexing, its transpose by autograd: what the GPU
tests compare dvd_geom_clip_forward / dvd_geom_clip_backward with.  It also serves what the tests' bound is made of.

The bound is derived, not measured.  The reference takes the fp32 entries of a row as exact numbers and evaluates
sx = a00 x + a01 y + a02, sy = a10 x + a11 y + a12 in fp64; the device evaluates them with two fmaf each.
  * Coordinates.  Two fp32 roundings on a sum whose partial sums are bounded by |a00| x + |a01| y + |a02|: the device's sx is off
    by at most dsx = 3 * 2^-24 * (|a00| x + |a01| y + |a02|) (2 would do; 3 is the figure the bound is stated with), sy likewise.
  * Continuity.  The zero-extended bilinear image is continuous in (sx, sy), also across the lines where floor() flips and across
    the border of (-1, W) x (-1, H), where it is 0 on both sides; between two neighbouring lattice points it is linear with a slope
    of at most the largest neighbour difference, <= 2 max|x| of the frame.  So a coordinate error changes an output by at most
    slack = (dsx + dsy) * 2 max|x|, whichever cell either side picked.
  * Roundings of the forward.  A weight is a product of two factors, one of them 1 - w (3 roundings); four fmaf accumulate
    (4 more): 7 fp32 roundings, each on a quantity bounded by mag = sum_k w_k |v_k|; FORWARD_ROUNDINGS = 8 leaves one to spare.
        |y_dev - y_ref| <= 8 * 2^-24 * mag + slack
  * The backward.  dx[q] = sum_p w(p, q) g[p].  A weight as a function of (sx, sy) is continuous with slope <= 1 per coordinate,
    so the coordinate error moves term p by at most (dsx_p + dsy_p) |g_p| -- for every p that either side can give a weight
    on q, i.e. |sx_p - qx| < 1 + ds_p and |sy_p - qy| < 1 + ds_p (looked for in the 4 x 4 block around p's cell); p with
    ds_p >= 1 (absurd rows) void the bound of their frame (infinite slack: the tests then assert zeros instead).  With N_q the number of such p, the device adds at most N_q terms to
    the accumulator (N_q roundings) of weights with 3 roundings each:
        |dx_dev[q] - dx_ref[q]| <= (4 + N_q) * 2^-24 * dmag[q] + dslack[q],    dmag = the transpose applied to |g|
"""
import math

import torch

COLS = 6
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)        # a00, a01, a02, a10, a11, a12
E32 = 2.0 ** -24
FORWARD_ROUNDINGS = 8
BACKWARD_ROUNDINGS = 4                            # + the number of window terms of the element


def _cells(row, H, W):
    """One row (six fp64 numbers that are fp32 values) at H x W -> the bilinear cells of the H W output pixels:
    idx [4, HW] (flat source index of the neighbours (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1), clamped into the
    frame), w [4, HW] (their weights, 0 where the neighbour is outside the frame or the pixel takes no part), and the pixel's
    coordinate error bounds dsx + dsy [HW] and its position sx, sy [HW] as computed (NaN and infinity included)."""
    a00, a01, a02, a10, a11, a12 = (torch.tensor(float(v), dtype=torch.float64) for v in row)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    sx, sy = a00 * xs + a01 * ys + a02, a10 * xs + a11 * ys + a12
    ds = 3 * E32 * ((a00.abs() * xs + a01.abs() * ys + a02.abs()) + (a10.abs() * xs + a11.abs() * ys + a12.abs()))
    ds = torch.nan_to_num(ds, nan=math.inf, posinf=math.inf)
    part = (sx > -1) & (sx < W) & (sy > -1) & (sy < H)                 # false for NaN and infinity
    raw = (sx, sy)
    sx, sy = torch.where(part, sx, torch.zeros_like(sx)), torch.where(part, sy, torch.zeros_like(sy))
    fx, fy = torch.floor(sx), torch.floor(sy)
    wx1, wy1 = sx - fx, sy - fy
    x0, y0 = fx.long(), fy.long()
    idx, w = [], []
    for jy, jx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xi, yi = x0 + jx, y0 + jy
        inside = part & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        idx.append(yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1))
        w.append((wy1 if jy else 1 - wy1) * (wx1 if jx else 1 - wx1) * inside)
    return torch.stack(idx), torch.stack(w), ds, raw[0], raw[1]


def frame(x, row):
    """x [3, H, W] fp64 -> the warped frame: plain indexing, differentiable by autograd."""
    _, H, W = x.shape
    idx, w, *_ = _cells(row, H, W)
    flat = x.reshape(3, H * W)
    return sum(w[k] * flat[:, idx[k]] for k in range(4)).reshape(3, H, W)


def _rows(mats):
    return torch.as_tensor(mats).float().double().cpu().tolist()        # the fp32 values the device reads, as exact numbers


def clip(x, mats, frames_per_clip):
    """x [N, 3, H, W] (any float dtype), mats [clips, 6] -> (y, mag, slack) in fp64 on the host: the warp, the same expression on
    absolute values, and the coordinate-error term; |device - y| <= FORWARD_ROUNDINGS * E32 * mag + slack.  Frame n takes row
    n // frames_per_clip."""
    x64 = x.detach().double().cpu()
    rows = _rows(mats)
    N, _, H, W = x64.shape
    y = torch.stack([frame(x64[n], rows[n // frames_per_clip]) for n in range(N)])
    mag = torch.stack([frame(x64[n].abs(), rows[n // frames_per_clip]) for n in range(N)])
    slack = torch.stack([(_cells(rows[n // frames_per_clip], H, W)[2] * (2 * x64[n].abs().max())).reshape(1, H, W).expand(3, H, W)
                         for n in range(N)])
    return y, mag, torch.nan_to_num(slack, nan=math.inf)


def forward_bound(mag, slack):
    return FORWARD_ROUNDINGS * E32 * mag + slack


def _spread(row, g_abs):
    """For one frame: dslack [3, H, W] and the window term count N_q [H, W] of the module docstring: every output pixel p hands
    (dsx + dsy) |g_p| and a count of 1 to the source pixels within 1 + ds of its position."""
    _, H, W = g_abs.shape
    _, _, ds, sx, sy = _cells(row, H, W)
    dslack, count = torch.zeros(3, H * W, dtype=torch.float64), torch.zeros(H * W, dtype=torch.float64)
    if bool((ds >= 1).any()):
        return torch.full((3, H, W), math.inf, dtype=torch.float64), torch.zeros(H, W, dtype=torch.float64)
    # (a pixel that takes no part in the reference may take part on the device when it is within ds of the border: it counts,
    #  with the border cell as its cell)
    near = (sx > -1 - ds) & (sx < W + ds) & (sy > -1 - ds) & (sy < H + ds)          # false for NaN and infinity
    sx, sy = torch.where(near, sx, torch.zeros_like(sx)), torch.where(near, sy, torch.zeros_like(sy))
    x0, y0 = torch.floor(sx.clamp(-1, W - 1)).long(), torch.floor(sy.clamp(-1, H - 1)).long()
    term = ds * g_abs.reshape(3, H * W)
    for jy in range(-1, 3):
        for jx in range(-1, 3):
            xi, yi = x0 + jx, y0 + jy
            ok = near & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H) & ((sx - xi).abs() < 1 + ds) & ((sy - yi).abs() < 1 + ds)
            at = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
            dslack.index_add_(1, at[ok], term[:, ok])
            count.index_add_(0, at[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
    return dslack.reshape(3, H, W), count.reshape(H, W)


def clip_grad(x, g, mats, frames_per_clip):
    """-> (dx, dmag, dslack, terms): autograd's gradient of sum(clip(x) * g) with respect to x, the transpose applied to |g|, the
    coordinate-error term and the window term count N_q (broadcast over the channels);
    |device - dx| <= (BACKWARD_ROUNDINGS + terms) * E32 * dmag + dslack."""
    x64 = x.detach().double().cpu()
    g64 = g.detach().double().cpu()
    rows = _rows(mats)
    N = x64.shape[0]

    def transpose(v):
        with torch.enable_grad():                  # (also when called from inside another Function's backward)
            leaf = torch.zeros_like(x64).requires_grad_(True)
            y = torch.stack([frame(leaf[n], rows[n // frames_per_clip]) for n in range(N)])
            return torch.autograd.grad(y, leaf, v)[0]
    dx, dmag = transpose(g64), transpose(g64.abs())
    spread = [_spread(rows[n // frames_per_clip], g64[n].abs()) for n in range(N)]
    dslack = torch.stack([s[0] for s in spread])
    terms = torch.stack([s[1] for s in spread])[:, None].expand_as(dx)
    return dx, dmag, dslack, terms


def backward_bound(dmag, dslack, terms):
    return (BACKWARD_ROUNDINGS + terms) * E32 * dmag + dslack


def about_centre(m00, m01, m10, m11, H, W):
    """The row whose 2 x 2 part is the given output -> source matrix, about the frame centre ((W - 1) / 2, (H - 1) / 2)."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return (m00, m01, cx - m00 * cx - m01 * cy, m10, m11, cy - m10 * cx - m11 * cy)


def hand_rows(H, W):
    """name -> row: the hand-made rows of the GPU tests at a frame size."""
    c45, s45 = math.cos(math.pi / 4), math.sin(math.pi / 4)
    c90, s90 = math.cos(math.pi / 2), math.sin(math.pi / 2)             # 6.1e-17 and 1: a quarter turn through the general path
    t = 0.7
    ct, st = math.cos(t), math.sin(t)
    # everything: mirror, a quarter turn, scale 1.25, rotation by 0.7, aniso 1.2 -- the 2 x 2 parts multiplied out by hand order
    e = [[-1.0, 0.0], [0.0, 1.0]]
    for m in ([[0.0, -1.0], [1.0, 0.0]], [[0.8, 0.0], [0.0, 0.8]], [[ct, -st], [st, ct]], [[1 / 1.2, 0.0], [0.0, 1.2]]):
        e = [[e[0][0] * m[0][0] + e[0][1] * m[1][0], e[0][0] * m[0][1] + e[0][1] * m[1][1]],
             [e[1][0] * m[0][0] + e[1][1] * m[1][0], e[1][0] * m[0][1] + e[1][1] * m[1][1]]]
    return {
        "identity": IDENTITY,
        "xflip": (-1.0, 0.0, W - 1.0, 0.0, 1.0, 0.0),
        "rot90 k=1": (0.0, -1.0, W - 1.0, 1.0, 0.0, 0.0),
        "rot90 k=2": (-1.0, 0.0, W - 1.0, 0.0, -1.0, H - 1.0),
        "rot90 k=3": (0.0, 1.0, 0.0, -1.0, 0.0, H - 1.0),
        "magnify by 2": about_centre(0.5, 0.0, 0.0, 0.5, H, W),
        "shrink by 2": about_centre(2.0, 0.0, 0.0, 2.0, H, W),
        "rotate 45": about_centre(c45, -s45, s45, c45, H, W),
        "rotate 90, general": about_centre(c90, -s90, s90, c90, H, W),
        "aniso": about_centre(1 / 1.3, 0.0, 0.0, 1.3, H, W),
        "everything": about_centre(e[0][0], e[0][1], e[1][0], e[1][1], H, W),
        "outside": (1.0, 0.0, 3.0 * W, 0.0, 1.0, 0.0),
        "singular": (0.0,) * 6,
        "huge": (1e30,) * 6,
        "nan": (math.nan,) * 6,
    }


ZERO_ROWS = ("outside", "huge", "nan")            # rows under which no output pixel takes part: y and dx are zeros

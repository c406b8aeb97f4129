"""What augment.py and geom_augment.py share: a per-clip transform of frames [N, 3, H, W] that is one launch, its transpose that
is another with the same arguments, and the autograd.Function over clips [B, T, 3, H, W] made of the two.  Each clip has one
row of a device table; the map is affine in the frames, so the Function saves only the table, which receives no gradient."""
import torch
from torch.autograd import Function

from . import lib as L


def clip_op(name, library, forward, backward, check, cols, noun, table_noun):
    """-> (forward(frames, table, frames_per_clip), backward(grad, table, frames_per_clip), a Function to derive `name` from).
    `library` is the accessor of lib.py, `forward` / `backward` its entry points by name (both `i ppp liii p`), `check` its
    return-code check, `cols` the table's row length; `noun` and `table_noun` word the two ValueErrors."""

    def launch(fn, src, table, frames_per_clip):
        """One launch over src [N, 3, H, W] (contiguous fp32 on the device) -> a new tensor of the same shape."""
        if src.dtype != torch.float32 or not src.is_cuda or src.dim() != 4 or src.shape[1] != 3:
            raise ValueError(f"{noun} takes device fp32 frames [N, 3, H, W], got {src.dtype} {tuple(src.shape)}")
        N, _, H, W = src.shape
        clips = -(-N // frames_per_clip)
        if (table.dtype != torch.float32 or table.device != src.device or tuple(table.shape) != (clips, cols)
                or not table.is_contiguous()):
            raise ValueError(f"{noun}: {table_noun} must be a contiguous device fp32 [{clips}, {cols}], got "
                             f"{table.dtype} {tuple(table.shape)} on {table.device}")
        dst = torch.empty_like(src)
        check(fn(L.ptr(src), L.ptr(dst), L.ptr(table), N, int(frames_per_clip), H, W, L.stream()))
        return dst

    def fwd(frames, table, frames_per_clip):
        return launch(getattr(library(), forward), frames.contiguous(), table, frames_per_clip)

    def bwd(grad, table, frames_per_clip):
        return launch(getattr(library(), backward), grad.contiguous(), table, frames_per_clip)

    class ClipOp(Function):
        @staticmethod
        def forward(ctx, frames, table):
            if frames.dim() != 5:
                raise ValueError(f"{name} takes clips [B, T, 3, H, W], got {tuple(frames.shape)}")
            B, T = frames.shape[:2]
            ctx.save_for_backward(table)
            out = fwd(frames.contiguous().view(B * T, *frames.shape[2:]), table, T)
            return out.view(frames.shape)

        @staticmethod
        def backward(ctx, g):
            (table,) = ctx.saved_tensors
            B, T = g.shape[:2]
            return bwd(g.contiguous().view(B * T, *g.shape[2:]), table, T).view(g.shape), None

    return fwd, bwd, ClipOp

"""Conditioning encoder of the frame-conditional video-prediction variant (BASELINE configs[4]): K context frames -> the twelve
initial ConvGRU states of the generator (Generator.forward(..., cond=)).  The reference has no such variant (SURVEY.md:34-36);
the architecture is fixed here and restated in tests/test_gpu_cond.py:

    cond [B, K, 3, 16 ld, 16 ld] -> channels 3 j + c (frame j, colour c) -> stem: SN 3x3, 3K -> 2ch (no activation)
    blocks.0 .. blocks.3: the discriminators' GBlock (ReLU, SN 3x3, ReLU, SN 3x3, + SN 1x1 shortcut, 2x2 average pool)
        2ch -> 4ch @ 8 ld,  4ch -> 8ch @ 4 ld,  8ch -> 8ch @ 2 ld,  8ch -> 8ch @ ld
    heads.s.l (ConvGRU s at ld << s pixels reads blocks.(3 - s), layer l): tanh(SN 3x3(ReLU(.))) of that layer's hidden size

Every convolution goes through the same conv planner and MFMA kernels as the rest of the network (Fn.Conv); each head writes its
state channels-last in the compute dtype, [B, S, S, hidden] -- the layout dvd_gru_desc.h0 reads -- so no conversion pass runs
between the encoder and either ConvGRU path.  The SN convs take part in the generator's batched spectral-norm launch
(prefetch_spectral_norm walks the generator's modules)."""
import torch
import torch.nn as nn

from . import functional as Fn
from . import lib as L
from .disc_nets import GBlock
from .sn_layers import SpectralNormConv


def gru_hidden_sizes(ch):
    """Per ConvGRU of the generator (4, at ld, 2 ld, 4 ld, 8 ld pixels) its three layers' hidden sizes."""
    c8, c4 = 8 * ch, 4 * ch
    return [(c8, 2 * c8, c8)] * 3 + [(c4, 2 * c4, c4)]


class FrameEncoder(nn.Module):
    """FrameEncoder(n_cond, latent_dim, ch).forward(cond [B, K, 3, 16 ld, 16 ld] fp32 in [-1, 1]) -> four lists (one per ConvGRU)
    of three channels-last states [B, S, S, hidden] in the compute dtype, values in (-1, 1)."""

    def __init__(self, n_cond, latent_dim, ch, compute_dtype=torch.bfloat16):
        super().__init__()
        if n_cond < 1:
            raise ValueError(f"n_cond={n_cond}: the encoder needs at least one conditioning frame")
        self.n_cond, self.latent_dim, self.ch, self.compute_dtype = n_cond, latent_dim, ch, compute_dtype
        c8, c4, c2 = 8 * ch, 4 * ch, 2 * ch
        self.stem = SpectralNormConv(3 * n_cond, c2, (3, 3))
        self.blocks = nn.ModuleList([GBlock(c2, c4), GBlock(c4, c8), GBlock(c8, c8), GBlock(c8, c8)])
        self.heads = nn.ModuleList(
            nn.ModuleList(SpectralNormConv(c8 if s < 3 else c4, h, (3, 3)) for h in hs)
            for s, hs in enumerate(gru_hidden_sizes(ch)))

    def check(self, cond, batch):
        fr = 16 * self.latent_dim
        if cond.dim() != 5 or tuple(cond.shape[1:]) != (self.n_cond, 3, fr, fr) or cond.shape[0] != batch:
            raise ValueError(f"cond must be [B={batch}, K={self.n_cond}, 3, {fr}, {fr}] (the generator's output layout), got "
                             f"{tuple(cond.shape)}")

    def forward(self, cond):
        B, K, C_, H, W = cond.shape
        x = Fn.ToChannelsLast.apply(cond.reshape(B, K * C_, H, W), self.compute_dtype, None)     # channel 3 j + c
        x = self.stem(x)
        feats = []
        for blk in self.blocks:
            x = blk(x)
            feats.append(x)
        return [[head(feats[3 - s], relu_in=True, act=L.ACT_TANH) for head in heads] for s, heads in enumerate(self.heads)]

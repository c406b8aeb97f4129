"""Float64 reference and error bounds for the pair loss of balanced consistency regularization (dvd_gan_amd/xsrc/cr/cr.hip,
include/dvdx_cr.h): weight * mean((aug - clean)^2) over a discriminator's logits, its two gradients and its statistics row.

A plain module (no conftest, no fixtures), torch only; no project kernel and no oracle code takes part.  The logits are fp32
values, so their fp64 copies are exact; everything inside is float64.

Bounds.  E = 2^-24 (one rounding to nearest in fp32), D = 2^-53 (one in fp64), SUB = 2^-149 (one rounding of a result below the
normal range).  Every constant counts the roundings of the expressions as include/dvdx_cr.h states them; none is fitted to what
the kernel produces.
  gap_i = fl32(aug_i - clean_i): one rounding, E |gap_i| (a difference of two fp32 values below the normal range is exact).
  d_aug_i = fl32(fl32(2 weight / n) fl32(gap_i)): 2 weight and n are exact, the quotient rounds once, the product once -- two
      roundings on top of the gap's:  ((1 + E)^3 - 1) |d_i| + SUB.  d_clean_i is its negation, to the bit.
  S = sum of the exact fp64 squares of the ROUNDED gaps: every addend is within (1 + E)^2 of its exact value and all are >= 0, so
      the sum is; its n - 1 fp64 additions add (n - 1) D.
  loss = fl32(fl64(fl64(weight S) / n)): two more fp64 roundings and one fp32 rounding:
      ((1 + E)^3 - 1 + (n + 1) D) loss + SUB.       The mean squared gap of the statistics row likewise (one fp64 rounding fewer).
  max |gap|: rounding is monotonic, so the largest rounded gap is the rounding of the largest: E max.
  The count of non-zero gaps and n are exact: fl32(a - c) is zero only when a == c.
"""
import torch

E = 2.0 ** -24
D = 2.0 ** -53
SUB = 2.0 ** -149


def pair64(aug, clean, weight):
    """-> name -> (reference, bound) of what dvdx_cr_pair writes for fp32 logits aug / clean [n] and an fp32-exact weight:
    "loss", "d_aug", "d_clean" and the statistics "msq", "maxabs" (tensors or floats); "nonzero" and "n" are exact ints."""
    assert aug.dtype == clean.dtype == torch.float32 and aug.shape == clean.shape and aug.dim() == 1
    w = float(torch.tensor(weight, dtype=torch.float32))
    assert w == float(weight), "the weight must be an fp32 value"
    a, c = aug.detach().double().cpu(), clean.detach().double().cpu()
    n = a.numel()
    gap = a - c
    msq = float((gap * gap).sum()) / n
    loss = w * msq
    d = (2.0 * w / n) * gap
    three = (1 + E) ** 3 - 1
    d_bound = three * d.abs() + SUB
    return {"loss": (loss, (three + (n + 1) * D) * loss + SUB),
            "d_aug": (d, d_bound),
            "d_clean": (-d, d_bound),
            "msq": (msq, (three + (n + 1) * D) * msq + SUB),
            "maxabs": (float(gap.abs().max()), E * float(gap.abs().max())),
            "nonzero": int((a != c).sum()),
            "n": n}


def ratio(got, want, bound):
    """Worst |got - want| / bound over the elements (0 / 0 counts as 0; a non-finite output as infinite error)."""
    got = torch.as_tensor(got, dtype=torch.float64).detach().cpu().reshape(-1)
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1).expand_as(want)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max())


def make_logits(n, seed=0):
    """fp32 logits of the kernel tests: draws of both signs, every seventh pair identical, +0 against -0, values near 1e4 with gaps
    of about 0.1 (the gap's own rounding matters there), a pair that differs in the last bit."""
    g = torch.Generator().manual_seed(1000 + 7 * n + seed)
    clean = torch.randn(n, generator=g, dtype=torch.float32) * 2
    aug = clean + torch.randn(n, generator=g, dtype=torch.float32) * 0.1
    idx = torch.arange(n)
    aug[idx % 7 == 3] = clean[idx % 7 == 3]                      # identical pairs
    big = idx % 5 == 1
    clean[big] = 1e4 + clean[big]
    aug[big] = clean[big] + 0.1
    if n > 2:
        clean[0], aug[0] = 0.0, -0.0                                 # +0 against -0: a zero gap
        clean[2] = 1.0
        aug[2] = torch.nextafter(clean[2], torch.tensor(2.0))
    return aug.contiguous(), clean.contiguous()

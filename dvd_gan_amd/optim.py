"""Adam on flat fp32 buffers: one kernel launch per network per step (trainer.py:136-141 uses
torch.optim.Adam(lr, betas=(beta1, beta2)) on the requires_grad parameters).

The trainable parameters of a network are re-homed as views into ONE contiguous buffer, their
.grad tensors are views into a second one.  That makes the optimizer a single elementwise launch
and the data-parallel gradient exchange a single RCCL all-reduce per network.

ema_decay > 0 adds an exponential moving average of the weights (`ema`, the BigGAN-family sampling weights), updated in
the same launch from the weights that launch has just written.

ortho > 0 adds BigGAN's orthogonal regularizer (Brock et al. 2019, eq. 3) to the gradient right before the Adam launch:
g += ortho * 2 M W with M = W W^T minus its diagonal, for every trainable matrix (dim() >= 2, viewed as [shape[0], -1]) that is
not excluded -- one table, two batched launches (dvd_ortho_grad), on the weights as they stand before that step's update.

clip_norm > 0, skip_nonfinite or norm_log > 0 turn the gradient guard on: before the Adam launch one pass over `grad` leaves its
fp64 norm, the coefficient min(1, clip_norm / (norm + 1e-6)) and the number of inf / NaN elements on the device
(dvd_grad_guard), and the Adam launch scales the gradient by that coefficient or, with skip_nonfinite and a non-finite element,
leaves p, m, v and ema untouched (dvd_adam_guard_step).  The host never reads any of it back.
"""
import math

import torch

from . import kern as K


class FlatAdam:
    def __init__(self, params, lr, betas=(0.0, 0.9), eps=1e-8, ema_decay=0.0, ema_start=0, ortho=0.0, ortho_exclude=(),
                 clip_norm=0.0, skip_nonfinite=False, norm_log=0):
        """ema_decay = 0: no average (`ema` stays None, step() is dvd_adam_step).  Otherwise `ema` is allocated as a copy of
        `flat` at the first step() -- the weights training starts from, whatever was loaded or broadcast into `flat` after
        construction -- or set by load_ema(); it follows the weights (decay 0) while t <= ema_start, then decays by ema_decay.
        ortho = 0: no regularizer (no table, no workspace, step() is the launch above).  Otherwise the item table is built here
        from the trainable tensors with dim() >= 2 and shape[0] > 1 that are not in `ortho_exclude` (tensors, compared by
        identity) and uploaded once; the workspace and the `ortho_penalty` scalar (float64, sum of 1/2 ||M||_F^2 at the last
        step) are allocated at the first step().
        clip_norm = 0, skip_nonfinite = False, norm_log = 0: no guard (nothing is allocated, step() runs the launches above).
        Otherwise step() measures the norm of `grad` as Adam is about to consume it -- the regularizer's term included, after
        the caller's gradient exchange, so equal ranks decide alike without a collective -- and clips it to clip_norm (0 = only
        measure) and / or skips the update when an element is inf / NaN.  `guard_state` (float64[8] on the device: norm of the
        finite part, coefficient, non-finite elements, skip flag, steps seen / skipped / clipped, 0) and, with norm_log = R
        > 0, `guard_ring` (float64[R][4], NaN until written: row (t - 1) % R = t, norm, coefficient, non-finite elements) are
        allocated at the first step().  A skipped step still advances `t`: the bias correction of the following steps treats
        it as taken (with beta1 = 0 and beta2 = 0.9 the second-moment correction is then a step ahead, a factor that tends to
        1 within tens of steps); there is no step count on the device."""
        clip_norm, norm_log = float(clip_norm), int(norm_log)
        if not 0.0 <= clip_norm < float("inf"):
            raise ValueError(f"clip_norm={clip_norm} must be a finite norm >= 0 (0 = no clipping)")
        if norm_log < 0:
            raise ValueError(f"norm_log={norm_log} must be a number of rows >= 0")
        self.clip_norm, self.skip_nonfinite, self.norm_log = clip_norm, bool(skip_nonfinite), norm_log
        self.guard = bool(self.clip_norm or self.skip_nonfinite or self.norm_log)
        self.guard_ws = self.guard_state = self.guard_ring = None
        if not 0.0 <= float(ortho) < float("inf"):
            raise ValueError(f"ortho={ortho} must be a finite strength >= 0")
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"ema_decay={ema_decay} must lie in [0, 1)")
        self.ema_decay, self.ema_start, self.ema = float(ema_decay), int(ema_start), None
        self.params = [p for p in params if p.requires_grad]
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.flat = torch.empty(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        off = 0
        for p in self.params:
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view(p.shape)
            p.grad = self.grad[off:off + k].view(p.shape)
            off += k
        self.lr, self.betas, self.eps, self.t = lr, betas, eps, 0
        self.param_groups = [{"lr": lr}]          # so torch lr schedulers' arithmetic can be mirrored
        self.ortho = float(ortho)
        self.ortho_items = self.ortho_items_dev = self.ortho_ws = self.ortho_penalty = None
        self.ortho_index, self.ortho_ws_floats = [], 0
        if self.ortho:
            skip = {id(t) for t in ortho_exclude}
            rows, off = [], 0
            for i, p in enumerate(self.params):
                if p.dim() >= 2 and p.shape[0] > 1 and id(p) not in skip:
                    rows.append([off, p.shape[0], p.numel() // p.shape[0]] + [0] * (K.ORTHO_COLS - 3))
                    self.ortho_index.append(i)            # position in self.params of each table row
                off += p.numel()
            if rows:
                self.ortho_items = torch.tensor(rows, dtype=torch.int64)
                _, self.ortho_ws_floats = K.ortho_prepare(self.ortho_items)
                self.ortho_items_dev = self.ortho_items.to(dev)

    def zero_grad(self):
        self.grad.zero_()                         # .grad tensors are views of this buffer

    def rebind(self):
        """Restore the .grad views if foreign code replaced them (e.g. zero_grad(set_to_none=True))."""
        off = 0
        for p in self.params:
            k = p.numel()
            view = self.grad[off:off + k].view(p.shape)
            if p.grad is None:
                p.grad = view
            elif p.grad.data_ptr() != view.data_ptr():
                view.copy_(p.grad)
                p.grad = view
            off += k

    def load_ema(self, flat_tensor):
        """Set the average (a flat fp32 tensor laid out like `flat`)."""
        if not self.ema_decay:
            raise RuntimeError("this optimizer keeps no weight average (ema_decay = 0)")
        if flat_tensor.numel() != self.flat.numel():
            raise ValueError(f"average of {flat_tensor.numel()} elements for {self.flat.numel()} parameters")
        if self.ema is None:
            self.ema = torch.empty_like(self.flat)
        self.ema.copy_(flat_tensor.reshape(-1))

    def ortho_grad(self):
        """Add the regularizer's gradient to `grad` (step() does, right before the Adam launch, on the same stream)."""
        if self.ortho_ws is None:
            self.ortho_ws = torch.empty(self.ortho_ws_floats, dtype=torch.float32, device=self.flat.device)
            self.ortho_penalty = torch.zeros((), dtype=torch.float64, device=self.flat.device)
        K.ortho_grad(self.flat, self.grad, self.ortho_items, self.ortho_items_dev, self.ortho, self.ortho_ws, self.ortho_penalty)

    @property
    def grad_norm(self):
        """Device scalar (float64): the norm of the finite part of the last step's gradient; None without a guard or before the
        first step()."""
        return None if self.guard_state is None else self.guard_state[K.GUARD_NORM]

    def guard_report(self):
        """Host dict of the guard's state (synchronizes): norm, coef, bad, skip of the last step, the seen / skipped / clipped
        counts and `ring`, the written rows [t, norm, coef, bad] of the log in step order; None without a guard or before the
        first step()."""
        if self.guard_state is None:
            return None
        s = self.guard_state.cpu().tolist()
        rows = [] if self.guard_ring is None else [r for r in self.guard_ring.cpu().tolist() if not math.isnan(r[0])]
        return {"norm": s[K.GUARD_NORM], "coef": s[K.GUARD_COEF], "bad": int(s[K.GUARD_BAD]), "skip": bool(s[K.GUARD_SKIP]),
                "seen": int(s[K.GUARD_SEEN]), "skipped": int(s[K.GUARD_SKIPPED]), "clipped": int(s[K.GUARD_CLIPPED]),
                "ring": sorted(rows)}

    def _guarded_step(self, ema, decay):
        if self.guard_state is None:
            dev = self.flat.device
            self.guard_ws = torch.empty(K.grad_guard_ws_bytes(self.grad.numel()), dtype=torch.uint8, device=dev)
            self.guard_state = torch.zeros(K.GUARD_STATE, dtype=torch.float64, device=dev)
            if self.norm_log:
                self.guard_ring = torch.full((self.norm_log, 4), float("nan"), dtype=torch.float64, device=dev)
        K.grad_guard(self.grad, self.clip_norm or float("inf"), self.skip_nonfinite, self.t, self.guard_ws, self.guard_state,
                     self.guard_ring)
        K.adam_guard_step(self.flat, self.grad, self.m, self.v, ema, self.param_groups[0]["lr"], self.betas[0], self.betas[1],
                          self.eps, self.t, decay, self.guard_state)

    def step(self):
        self.t += 1
        if self.ortho_items is not None:
            self.ortho_grad()
        if self.ema_decay and self.ema is None:
            self.ema = self.flat.clone()
        decay = 0.0 if self.t <= self.ema_start else self.ema_decay
        if self.guard:
            self._guarded_step(self.ema, decay)
        elif self.ema_decay:
            K.adam_ema_step(self.flat, self.grad, self.m, self.v, self.ema, self.param_groups[0]["lr"], self.betas[0],
                            self.betas[1], self.eps, self.t, decay)
        else:
            K.adam_step(self.flat, self.grad, self.m, self.v, self.param_groups[0]["lr"], self.betas[0], self.betas[1],
                        self.eps, self.t)

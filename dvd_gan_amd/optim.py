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

    # ---- what one step leaves for the next (exact resume: train_step.Trainer.save_state / load_state)
    def state_dict(self):
        """Copies of the device tensors and the host scalars one step leaves for the next: flat, m, v, ema (None when none is
        kept or before the first step), guard_state / guard_ring (None when not allocated), t, lr (param_groups[0]["lr"], what
        the schedule last set), numel and the settings that decide their shapes and meaning (settings()).  ortho_penalty, a
        report of the last step, rides along and is never required.  The workspaces are not state.  Copies only, on the
        current stream; nothing waits for the device."""
        copy = lambda t: None if t is None else t.detach().clone()
        sd = {"flat": copy(self.flat), "m": copy(self.m), "v": copy(self.v), "ema": copy(self.ema),
              "guard_state": copy(self.guard_state), "guard_ring": copy(self.guard_ring), "ortho_penalty": copy(self.ortho_penalty),
              "t": int(self.t), "lr": float(self.param_groups[0]["lr"]), "numel": int(self.flat.numel())}
        sd.update(self.settings())
        return sd

    def settings(self):
        """The host-side settings of state_dict(), as plain Python values."""
        return {"betas": [float(b) for b in self.betas], "eps": float(self.eps), "ema_decay": self.ema_decay,
                "ema_start": self.ema_start, "clip_norm": self.clip_norm, "skip_nonfinite": self.skip_nonfinite,
                "norm_log": self.norm_log, "ortho": self.ortho}

    def load_state_dict(self, sd):
        """Copy a state_dict() (tensors on any device) INTO the existing buffers: `flat` is never rebound, so the parameters'
        .data / .grad views stay what they are.  ema, guard_state and guard_ring are allocated as the first step() would have
        allocated them.  Raises ValueError naming the field when numel, norm_log (the ring's rows) or the presence of a weight
        average (ema_decay > 0 against `ema`) disagree with this optimizer.  Settings that only steer future steps (betas, eps,
        the decay's value, ema_start, clip_norm, skip_nonfinite, ortho) stay as constructed; lr and t are state and are taken
        from `sd`.  -> list of warning strings, one per setting that differs."""
        n = self.flat.numel()
        if int(sd["numel"]) != n:
            raise ValueError(f"numel: the state holds {int(sd['numel'])} parameters, this optimizer {n}")
        for k in ("flat", "m", "v"):
            if sd[k].numel() != n:
                raise ValueError(f"numel: `{k}` of the state holds {sd[k].numel()} elements, this optimizer {n}")
        if int(sd["norm_log"]) != self.norm_log:
            raise ValueError(f"norm_log: the state logs {int(sd['norm_log'])} rows, this optimizer {self.norm_log}")
        ema, ring, gstate = sd.get("ema"), sd.get("guard_ring"), sd.get("guard_state")
        if ring is not None and tuple(ring.shape) != (self.norm_log, 4):
            raise ValueError(f"norm_log: guard_ring of the state is {tuple(ring.shape)}, this optimizer logs {self.norm_log} rows")
        if bool(float(sd["ema_decay"]) > 0.0) != bool(self.ema_decay) or (ema is not None and not self.ema_decay):
            raise ValueError(f"ema: the state was written with ema_decay={sd['ema_decay']} "
                             f"({'a' if ema is not None else 'no'} weight average), this optimizer has ema_decay={self.ema_decay}")
        if self.ema_decay and ema is None and int(sd["t"]) > 0:
            raise ValueError(f"ema: the state is {int(sd['t'])} steps old and holds no weight average, this optimizer keeps one")
        if ema is not None and ema.numel() != n:
            raise ValueError(f"numel: `ema` of the state holds {ema.numel()} elements, this optimizer {n}")
        notes = []
        for k, mine in self.settings().items():
            theirs = sd.get(k)
            theirs = [float(b) for b in theirs] if k == "betas" and theirs is not None else theirs
            if k != "norm_log" and theirs != mine:
                notes.append(f"{k}: the state was written with {theirs}, this optimizer continues with {mine}")
        for k in ("flat", "m", "v"):
            getattr(self, k).copy_(sd[k].reshape(-1))
        if ema is None:
            self.ema = None                   # a state from before the first step: step() copies the weights
        else:
            self.load_ema(ema)
        if not self.guard:
            if gstate is not None:
                notes.append("guard: the state holds a gradient guard's counters, this optimizer has no guard; they are dropped")
        elif gstate is None:
            self.guard_ws = self.guard_state = self.guard_ring = None
            if int(sd["t"]) > 0:
                notes.append("guard: the state holds no gradient guard's counters; they start from zero")
        else:
            if self.guard_state is None:
                self._alloc_guard()
            self.guard_state.copy_(gstate)
            if self.guard_ring is not None and ring is not None:
                self.guard_ring.copy_(ring)
        if self.ortho_penalty is not None and sd.get("ortho_penalty") is not None:
            self.ortho_penalty.copy_(sd["ortho_penalty"])
        self.t = int(sd["t"])
        self.param_groups[0]["lr"] = float(sd["lr"])
        return notes

    def snapshot_numel(self):
        """Elements of the slab snapshot_into() fills: numel times 3, or 4 while a weight average exists."""
        return self.flat.numel() * (3 if self.ema is None else 4)

    def snapshot_into(self, dst):
        """flat | m | v | ema (when it exists) back to back into `dst`, a flat fp32 tensor on the optimizer's device with at least
        snapshot_numel() elements: three or four device-to-device copies on the current stream, nothing else.  -> the names of
        the parts in slab order, each numel elements long."""
        n, parts = self.flat.numel(), ["flat", "m", "v"] + (["ema"] if self.ema is not None else [])
        if dst.dtype != torch.float32 or dst.dim() != 1 or dst.device != self.flat.device or dst.numel() < n * len(parts):
            raise ValueError(f"the slab must be flat fp32 on {self.flat.device} with >= {n * len(parts)} elements, got "
                             f"{dst.dtype} {tuple(dst.shape)} on {dst.device}")
        for i, k in enumerate(parts):
            dst[i * n:(i + 1) * n].copy_(getattr(self, k))
        return parts

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

    def _alloc_guard(self):
        dev = self.flat.device
        self.guard_ws = torch.empty(K.grad_guard_ws_bytes(self.grad.numel()), dtype=torch.uint8, device=dev)
        self.guard_state = torch.zeros(K.GUARD_STATE, dtype=torch.float64, device=dev)
        if self.norm_log:
            self.guard_ring = torch.full((self.norm_log, 4), float("nan"), dtype=torch.float64, device=dev)

    def _guarded_step(self, ema, decay):
        if self.guard_state is None:
            self._alloc_guard()
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

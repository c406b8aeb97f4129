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
"""
import torch

from . import kern as K


class FlatAdam:
    def __init__(self, params, lr, betas=(0.0, 0.9), eps=1e-8, ema_decay=0.0, ema_start=0, ortho=0.0, ortho_exclude=()):
        """ema_decay = 0: no average (`ema` stays None, step() is dvd_adam_step).  Otherwise `ema` is allocated as a copy of
        `flat` at the first step() -- the weights training starts from, whatever was loaded or broadcast into `flat` after
        construction -- or set by load_ema(); it follows the weights (decay 0) while t <= ema_start, then decays by ema_decay.
        ortho = 0: no regularizer (no table, no workspace, step() is the launch above).  Otherwise the item table is built here
        from the trainable tensors with dim() >= 2 and shape[0] > 1 that are not in `ortho_exclude` (tensors, compared by
        identity) and uploaded once; the workspace and the `ortho_penalty` scalar (float64, sum of 1/2 ||M||_F^2 at the last
        step) are allocated at the first step()."""
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

    def step(self):
        self.t += 1
        if self.ortho_items is not None:
            self.ortho_grad()
        if self.ema_decay:
            if self.ema is None:
                self.ema = self.flat.clone()
            K.adam_ema_step(self.flat, self.grad, self.m, self.v, self.ema, self.param_groups[0]["lr"], self.betas[0],
                            self.betas[1], self.eps, self.t, 0.0 if self.t <= self.ema_start else self.ema_decay)
            return
        K.adam_step(self.flat, self.grad, self.m, self.v, self.param_groups[0]["lr"], self.betas[0], self.betas[1],
                    self.eps, self.t)

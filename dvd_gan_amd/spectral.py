"""The top singular values of weight matrices on the device (libdvdgan_hip_sv.so, include/dvdgan_hip_sv.h): the diagnostic of
Brock et al. 2019 ("BigGAN", section 4, figure 3) -- sigma_0, sigma_1, sigma_2 of every weight over training, which grow slowly and
explode at collapse.  Block power (subspace) iteration in fp64 with a Rayleigh-Ritz finish, every matrix of a table in a fixed
number of launches (4 per iteration, 2 per report); the fp32 weights are read in place and nothing that is read is changed.

What the numbers mean.  The reported values are Ritz values: lower bounds that rise towards sigma_i as the block converges; with
block width b the error of value i shrinks like (sigma_{b+1} / sigma_i)^(2 * iterations).  `res_i` = |W v_i - sv_i u_i| is an
a-posteriori bound: some singular value of W (or 0) lies within res_i of sv_i.  On a flat spectrum (freshly initialised Gaussian
weights) 16 cold iterations are still about 1 % low (measured with the fp64 restatement tests/sv_ref.py on the CPU); a monitor
keeps its blocks between reports (warm start), which is what makes 4 iterations per report enough during training.
"""
import ctypes as C

import torch

from . import lib as L


def _stored_width(block):
    return 8 if block <= 8 else 16


def draw_start_blocks(shapes, block, seed):
    """fp64 normal start blocks [w, min(block, h, w)] for matrices of `shapes` [(h, w)], drawn on the host from a PRIVATE generator
    seeded with `seed`, item by item in table order.  The default generator and every other stream stay where they are."""
    gen = torch.Generator().manual_seed(int(seed))
    return [torch.randn(w, min(block, h, w), dtype=torch.float64, generator=gen) for h, w in shapes]


def check_settings(k, block, what="SpectrumMonitor"):
    if not (isinstance(k, int) and isinstance(block, int) and 1 <= k <= block <= L.SV_MAX_BLOCK):
        raise ValueError(f"{what}: k={k}, block={block} must satisfy 1 <= k <= block <= {L.SV_MAX_BLOCK}")


class SpectrumMonitor:
    """named_matrices: [(name, tensor)], contiguous fp32 device tensors, each viewed [shape[0], -1] and read in place (the
    monitor holds the tensors, not copies).  sn: {name: (u [h], v [w])} fp32 spectral-norm vectors of some of them, read only:
    their items also report sn_sigma = u^T W v.  rows: rows of the device ring snapshot() writes.  start: start blocks
    [w, min(block, h, w)] fp64 in table order instead of the seeded draw (tests).

    update(iters) continues from the blocks the monitor holds; reset() puts the seeded blocks back; snapshot(row) writes one
    ring row [n, 2 k + 2] = sv[k] (descending, 0 beyond min(block, h, w)), res[k], fro2 = |W|_F^2, sn_sigma (NaN without u, v);
    read() is the one call that synchronizes.  Everything runs on the current stream and is deterministic: an item's numbers
    depend on its values, its shape, the block width and its start block alone."""

    def __init__(self, named_matrices, k=3, block=8, seed=0, sn=None, rows=1, start=None):
        check_settings(k, block)
        named_matrices = list(named_matrices)
        if not named_matrices or not isinstance(rows, int) or rows < 1:
            raise ValueError(f"SpectrumMonitor: {len(named_matrices)} matrices, rows={rows} (both >= 1)")
        self.k, self.block, self.seed, self.rows = k, block, int(seed), rows
        self.names = [n for n, _ in named_matrices]
        self.tensors = [t for _, t in named_matrices]
        sn = dict(sn or {})
        self.sn = [sn.get(n) for n in self.names]
        dev = self.tensors[0].device
        for n, t in named_matrices:
            for x, size in ((t, None),) + (() if sn.get(n) is None else ((sn[n][0], t.shape[0]), (sn[n][1], t[0].numel()))):
                if x.dtype != torch.float32 or not x.is_cuda or x.device != dev or not x.is_contiguous() or x.dim() < 1 \
                        or x.numel() < 1 or (size is not None and x.numel() != size):
                    raise ValueError(f"SpectrumMonitor: {n}: contiguous non-empty fp32 tensors on one device, u [h] and v [w], "
                                     f"got {x.dtype}, {tuple(x.shape)} on {x.device}")
        self.shapes = [(t.shape[0], t.numel() // t.shape[0]) for t in self.tensors]
        self.device = dev
        n = len(self.names)
        self._host = (L.SvItem * n)()
        for i, (h, w) in enumerate(self.shapes):
            self._host[i].h, self._host[i].w, self._host[i].slot = h, w, i
        self._fill_pointers()
        sd, wd = C.c_longlong(), C.c_longlong()
        L.sv_check(L.sv_lib().dvd_sv_prepare(self._host, n, block, C.byref(sd), C.byref(wd)))
        bp = _stored_width(block)
        blocks = draw_start_blocks(self.shapes, block, self.seed) if start is None else [torch.as_tensor(s) for s in start]
        host = torch.zeros(sd.value, dtype=torch.float64)
        for i, ((h, w), blk) in enumerate(zip(self.shapes, blocks)):
            r = min(block, h, w)
            if blk.dtype != torch.float64 or tuple(blk.shape) != (w, r):
                raise ValueError(f"SpectrumMonitor: start block {i} must be fp64 [{w}, {r}], got {blk.dtype} {tuple(blk.shape)}")
            off = self._host[i].state_off
            host[off:off + w * bp].view(w, bp)[:, :r] = blk
        self._start = host.to(dev)                                  # uploaded once; reset() copies it on the device
        self._state = torch.empty(sd.value, dtype=torch.float64, device=dev)
        self._ws = torch.empty(wd.value, dtype=torch.float64, device=dev)
        self.ring = torch.zeros(rows, n, 2 * k + 2, dtype=torch.float64, device=dev)
        self._upload()
        self.snapshots = 0            # rows written without an explicit row index
        self.iterations = 0           # iterations since the last reset()
        self.reset()

    def _pointers(self):
        return [(t.data_ptr(), None if s is None else s[0].data_ptr(), None if s is None else s[1].data_ptr())
                for t, s in zip(self.tensors, self.sn)]

    def _fill_pointers(self):
        self._ptrs = self._pointers()
        for it, (w, u, v) in zip(self._host, self._ptrs):
            it.W, it.u, it.v = w, u, v

    def _upload(self):
        raw = torch.frombuffer(bytearray(bytes(self._host)), dtype=torch.uint8)
        self._dev = raw.to(self.device)

    def _table(self):
        if self._pointers() != self._ptrs:          # a tensor's storage moved (foreign code rebound .data): point at it again
            self._fill_pointers()
            self._upload()
        return L.ptr(self._dev), self._host, len(self.names), self.block

    def reset(self):
        """The seeded start blocks again, orthonormalised."""
        L.sv_check(L.sv_lib().dvd_sv_init(*self._table(), L.ptr(self._start), L.ptr(self._state), L.stream()))
        self.iterations = 0
        return self

    def update(self, iters):
        iters = int(iters)
        if iters < 0 or iters > L.SV_MAX_ITERS:
            raise ValueError(f"SpectrumMonitor.update: iters={iters} (in [0, {L.SV_MAX_ITERS}])")
        L.sv_check(L.sv_lib().dvd_sv_iterate(*self._table(), iters, L.ptr(self._state), L.stream()))
        self.iterations += iters
        return self

    def snapshot(self, row=None):
        """Writes ring row `row` (default: the next one, wrapping) and returns its index.  Needs one iteration since reset()."""
        if self.iterations < 1:
            raise RuntimeError("SpectrumMonitor.snapshot: no iteration since reset() -- update(iters >= 1) first")
        ring = self.ring
        n_rows = ring.shape[0]
        if ring.dtype != torch.float64 or tuple(ring.shape[1:]) != (len(self.names), 2 * self.k + 2) or not ring.is_contiguous():
            raise ValueError("SpectrumMonitor.ring must stay a contiguous fp64 [rows, n, 2 k + 2] tensor")
        if row is None:
            row = self.snapshots % n_rows
            self.snapshots += 1
        if not 0 <= int(row) < n_rows:
            raise ValueError(f"SpectrumMonitor.snapshot: row={row} outside the ring of {n_rows}")
        L.sv_check(L.sv_lib().dvd_sv_ritz(*self._table(), self.k, L.ptr(self._state), L.ptr(self._ws), L.ptr(ring), int(row), n_rows,
                                          L.stream()))
        return int(row)

    def read(self):
        """Synchronizes: the ring as a host tensor fp64 [rows, n, 2 k + 2]."""
        return self.ring.cpu()

    def split(self, row):
        """A host row [n, 2 k + 2] -> sv [n, k], res [n, k], fro2 [n], sn_sigma [n]."""
        k = self.k
        return row[:, :k], row[:, k:2 * k], row[:, 2 * k], row[:, 2 * k + 1]


def top_singular_values(tensors, k=3, iters=16, block=8, seed=0):
    """A pure function: a fresh monitor over `tensors` (each viewed [shape[0], -1]), `iters` cold iterations, one report.
    Returns host tensors sv [n, k], res [n, k] (fp64).  Synchronizes."""
    if int(iters) < 1:
        raise ValueError(f"top_singular_values: iters={iters} (>= 1)")
    mon = SpectrumMonitor([(str(i), t) for i, t in enumerate(tensors)], k=k, block=block, seed=seed)
    mon.update(iters)
    mon.snapshot(0)
    sv, res, _, _ = mon.split(mon.read()[0])
    return sv, res

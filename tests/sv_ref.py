"""fp64 numpy restatement of libdvdgan_hip_sv.so (include/dvdgan_hip_sv.h): block power iteration with a Rayleigh-Ritz finish.
The same start blocks, the same zero-column rule, the same Jacobi finish and the same residual as the kernels; only the order of
the long sums differs (numpy's products against the kernels' fixed splits)."""
import numpy as np

MAX_SWEEPS = 60
DROP = 2.0 ** -40
ROT = 2.0 ** -50


def start_blocks(shapes, block, seed):
    """The start blocks of SpectrumMonitor: fp64 normal values from a private torch.Generator, item by item in table order, each
    [w, r] with r = min(block, h, w)."""
    import torch
    gen = torch.Generator().manual_seed(int(seed))
    return [torch.randn(w, min(block, h, w), dtype=torch.float64, generator=gen).numpy() for h, w in shapes]


def orth(A):
    """Classical Gram-Schmidt with a second pass, column by column; A [n, r] -> Q, R with A = Q R.  A column whose norm after
    projection is at most 2^-40 of the largest column norm of A becomes exact zeros (R[j, j] = 0)."""
    A = np.array(A, dtype=np.float64)
    n, r = A.shape
    R = np.zeros((r, r))
    limit = DROP * np.sqrt(max(float((A[:, c] ** 2).sum()) for c in range(r))) if r else 0.0
    for j in range(r):
        for _ in range(2):
            c = A[:, :j].T @ A[:, j]
            A[:, j] -= A[:, :j] @ c
            R[:j, j] += c
        nrm = np.sqrt(float((A[:, j] ** 2).sum()))
        if not nrm > limit:
            A[:, j] = 0.0
            R[j, j] = 0.0
        else:
            A[:, j] /= nrm
            R[j, j] = nrm
    return A, R


def jacobi(R):
    """One-sided Jacobi on the columns of R: M = R J with orthogonal columns, pairs (p, q), p < q, in row-major order."""
    M = np.array(R, dtype=np.float64)
    r = M.shape[0]
    J = np.eye(r)
    for _ in range(MAX_SWEEPS):
        rotated = False
        for p in range(r - 1):
            for q in range(p + 1, r):
                al, be, ga = float(M[:, p] @ M[:, p]), float(M[:, q] @ M[:, q]), float(M[:, p] @ M[:, q])
                if not abs(ga) > ROT * np.sqrt(al * be):
                    continue
                rotated = True
                ze = (be - al) / (2.0 * ga)
                t = (1.0 if ze >= 0.0 else -1.0) / (abs(ze) + np.sqrt(1.0 + ze * ze))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                for X in (M, J):
                    xp, xq = X[:, p].copy(), X[:, q].copy()
                    X[:, p] = c * xp - s * xq
                    X[:, q] = s * xp + c * xq
        if not rotated:
            break
    return M, J


class State:
    def __init__(self, W, start):
        self.W = np.asarray(W, dtype=np.float32).astype(np.float64)
        self.W = self.W.reshape(self.W.shape[0], -1)
        self.V, _ = orth(start)
        r = self.V.shape[1]
        self.Y, self.R = np.zeros((self.W.shape[0], r)), np.zeros((r, r))

    def iterate(self, iters):
        for _ in range(iters):
            self.Y, _ = orth(self.W @ self.V)
            self.V, self.R = orth(self.W.T @ self.Y)
        return self

    def ritz(self, k, u=None, v=None):
        """sv [k], res [k], fro2, sn_sigma of the header's output row."""
        M, J = jacobi(self.R)
        sg = np.sqrt((M ** 2).sum(0))
        order = sorted(range(len(sg)), key=lambda c: (-sg[c], c))
        P = self.W @ self.V
        sv, res = np.zeros(k), np.zeros(k)
        for i, c in enumerate(order[:k]):
            cv = M[:, c] / sg[c] if sg[c] > 0.0 else np.zeros(len(sg))
            d = P @ cv - sg[c] * (self.Y @ J[:, c])
            sv[i], res[i] = sg[c], np.sqrt(float(d @ d))
        fro2 = float((self.W ** 2).sum())
        sn = float(np.asarray(u, np.float64) @ (self.W @ np.asarray(v, np.float64))) if u is not None else float("nan")
        return sv, res, fro2, sn


def report(W, start, iters, k, u=None, v=None):
    return State(W, start).iterate(iters).ritz(k, u, v)


def gapped(h, w, s, seed):
    """W = U diag(s) V^T rounded to fp32 (s padded with zeros to min(h, w)), and the fp64 singular values of that fp32 matrix."""
    rng = np.random.default_rng(seed)
    m = min(h, w)
    U, _ = np.linalg.qr(rng.standard_normal((h, m)))
    V, _ = np.linalg.qr(rng.standard_normal((w, m)))
    sv = np.zeros(m)
    sv[:min(m, len(s))] = np.asarray(s, dtype=np.float64)[:m]
    W = ((U * sv) @ V.T).astype(np.float32)
    return W, np.linalg.svd(W.astype(np.float64), compute_uv=False)


def exact_low_rank(h, w, s):
    """W = sum_i s_i u_i v_i^T with u_i, v_i columns of the 16 x 16 Hadamard matrix / 4, padded with zeros to h and w (>= 16):
    every entry is a multiple of 1 / 16, exact in fp32, so W has exactly the singular values s and exactly rank len(s) <= 8."""
    H = np.array([[1.0]])
    for _ in range(4):
        H = np.block([[H, H], [H, -H]])
    W = np.zeros((h, w))
    for i, si in enumerate(s):
        W[:16, :16] += si * np.outer(H[:, i], H[:, 8 + i]) / 16.0
    assert np.array_equal(W.astype(np.float32).astype(np.float64), W)
    return W.astype(np.float32)

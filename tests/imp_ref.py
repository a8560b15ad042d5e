"""numpy restatement of the IMPMethod stages (src/IB/IMPMethod.cpp) in the reference's order
of operations: the IB_6 kernel with its derivative (:119-171), interpolateVelocity
(:460-536), spreadForce (:848-921), the deformation-gradient steps (:547-716) and the
stress tau = PP FF^T with the law of examples/IMP/explicit/ex0/main.cpp:68-89.

Every float64 operation is one numpy operation in the reference's association, vectorised
over the list entries only, so each entry's value is rounded exactly as the scalar loop
rounds it.  Side arrays are numpy arrays of shape (nz, ny, nx) (2-D: (ny, nx)) over the
ghost box, the face iupper + 1 along the component's own axis included.
"""
from __future__ import annotations

import math

import numpy as np

K = (59.0 / 60.0) * (1.0 - math.sqrt(1.0 - (3220.0 / 3481.0)))
KERNEL_WIDTH = 3


class Geo:
    """One patch: cell box [ilower, ilower + n - 1], ghost width g, spacing dx, corner x_lower."""

    def __init__(self, ilower, n, dx, x_lower, g):
        self.ndim = len(n)
        self.ilower = [int(v) for v in ilower]
        self.n = [int(v) for v in n]
        self.iupper = [lo + m - 1 for lo, m in zip(self.ilower, self.n)]
        self.dx = [float(v) for v in dx]
        self.x_lower = [float(v) for v in x_lower]
        self.g = int(g)

    def ghost_box(self, c):
        lo = [self.ilower[d] - self.g for d in range(self.ndim)]
        hi = [self.iupper[d] + self.g + (1 if d == c else 0) for d in range(self.ndim)]
        return lo, hi

    def patch_side_box(self, c):
        return list(self.ilower), [self.iupper[d] + (1 if d == c else 0) for d in range(self.ndim)]

    def shape(self, c):
        lo, hi = self.ghost_box(c)
        return tuple(hi[d] - lo[d] + 1 for d in reversed(range(self.ndim)))

    def alloc(self, fill=0.0):
        return [np.full(self.shape(c), fill) for c in range(self.ndim)]

    def frame_lower(self, c, d):
        return self.x_lower[d] + (-0.5 * self.dx[d] if d == c else 0.0)

    def coords(self, c, d):
        """Positions of component c's points along dim d, over the ghost box."""
        lo, hi = self.ghost_box(c)
        i = np.arange(lo[d], hi[d] + 1, dtype=np.float64)
        return self.x_lower[d] + (i - self.ilower[d] + (0.0 if d == c else 0.5)) * self.dx[d]


def nint(x):
    """round(): halves away from zero."""
    x = np.asarray(x, dtype=np.float64)
    t = np.trunc(x)  # x - t is exact, where floor(|x| + 0.5) rounds 0.49999999999999994 up
    return (t + np.sign(x) * (np.abs(x - t) >= 0.5)).astype(np.int64)


def kernel(X, patch_x_lower, dx, patch_box_lower):
    """IMPMethod.cpp:119-171 for an array of positions: stencil_box_lower, phi[n][6], dphi[n][6]."""
    X = np.asarray(X, dtype=np.float64)
    X_o_dx = (X - patch_x_lower) / dx
    lower = nint(X_o_dx) + patch_box_lower - KERNEL_WIDTH
    r = 1.0 - X_o_dx + ((lower + KERNEL_WIDTH - 1 - patch_box_lower).astype(np.float64) + 0.5)

    r2 = r * r
    r3 = r * r2
    r4 = r * r3
    r5 = r * r4
    r6 = r * r5

    K2 = K * K
    alpha = 28.0

    beta = (9.0 / 4.0) - (3.0 / 2.0) * (K + r2) + ((22.0 / 3.0) - 7.0 * K) * r - (7.0 / 3.0) * r3
    dbeta = ((22.0 / 3.0) - 7.0 * K) - 3.0 * r - 7.0 * r2

    gamma = (1.0 / 4.0) * (((161.0 / 36.0) - (59.0 / 6.0) * K + 5.0 * K2) * (1.0 / 2.0) * r2 +
                           (-(109.0 / 24.0) + 5.0 * K) * (1.0 / 3.0) * r4 + (5.0 / 18.0) * r6)
    dgamma = (1.0 / 4.0) * (((161.0 / 36.0) - (59.0 / 6.0) * K + 5.0 * K2) * r +
                            (-(109.0 / 24.0) + 5.0 * K) * (4.0 / 3.0) * r3 + (5.0 / 3.0) * r5)

    discr = beta * beta - 4.0 * alpha * gamma

    phi = np.empty(X.shape + (6,))
    dphi = np.empty(X.shape + (6,))
    p0 = (-beta + math.copysign(1.0, (3.0 / 2.0) - K) * np.sqrt(discr)) / (2.0 * alpha)
    phi[..., 0] = p0
    phi[..., 1] = -3.0 * p0 - (1.0 / 16.0) + (1.0 / 8.0) * (K + r2) + (1.0 / 12.0) * (3.0 * K - 1.0) * r + \
        (1.0 / 12.0) * r3
    phi[..., 2] = 2.0 * p0 + (1.0 / 4.0) + (1.0 / 6.0) * (4.0 - 3.0 * K) * r - (1.0 / 6.0) * r3
    phi[..., 3] = 2.0 * p0 + (5.0 / 8.0) - (1.0 / 4.0) * (K + r2)
    phi[..., 4] = -3.0 * p0 + (1.0 / 4.0) - (1.0 / 6.0) * (4.0 - 3.0 * K) * r + (1.0 / 6.0) * r3
    phi[..., 5] = p0 - (1.0 / 16.0) + (1.0 / 8.0) * (K + r2) - (1.0 / 12.0) * (3.0 * K - 1.0) * r - (1.0 / 12.0) * r3

    d0 = -(dbeta * p0 + dgamma) / (2.0 * alpha * p0 + beta)
    dphi[..., 0] = d0
    dphi[..., 1] = -3.0 * d0 + (1.0 / 12.0) * (3.0 * K - 1.0) + (1.0 / 4.0) * r + (1.0 / 4.0) * r2
    dphi[..., 2] = 2.0 * d0 + (1.0 / 6.0) * (4.0 - 3.0 * K) - (1.0 / 2.0) * r2
    dphi[..., 3] = 2.0 * d0 - (1.0 / 2.0) * r
    dphi[..., 4] = -3.0 * d0 - (1.0 / 6.0) * (4.0 - 3.0 * K) + (1.0 / 2.0) * r2
    dphi[..., 5] = d0 - (1.0 / 12.0) * (3.0 * K - 1.0) + (1.0 / 4.0) * r - (1.0 / 4.0) * r2
    return lower, phi, dphi


def list_positions(X, indices=None, xshift=None):
    """The list's marker rows and evaluation positions X(s) + Xshift(l)."""
    X = np.asarray(X, dtype=np.float64)
    idx = np.arange(X.shape[0]) if indices is None else np.asarray(indices, dtype=np.int64)
    Xs = X[idx] if xshift is None else X[idx] + np.asarray(xshift, dtype=np.float64).reshape(len(idx), -1)
    return idx, Xs


def _component_stencils(geo, c, Xs):
    nd = geo.ndim
    lower, phi, a = [], [], []
    for d in range(nd):
        lo, p, dp = kernel(Xs[:, d], geo.frame_lower(c, d), geo.dx[d], geo.ilower[d])
        lower.append(lo)
        phi.append(p)
        a.append(dp / geo.dx[d])
    return lower, phi, a


def _offsets(nd):
    """Stencil offsets in the Box iterator's order: dimension 0 fastest."""
    if nd == 3:
        return [(ix, iy, iz) for iz in range(6) for iy in range(6) for ix in range(6)]
    return [(ix, iy) for iy in range(6) for ix in range(6)]


def _weights(nd, phi, a, off):
    """w and dw_dx_k of one stencil offset: ((1 x0) x1) x2 with x_d = a_d for d == k."""
    w = phi[0][:, off[0]] * phi[1][:, off[1]]
    if nd == 3:
        w = w * phi[2][:, off[2]]
    dw = []
    for k in range(nd):
        t = (a[0] if k == 0 else phi[0])[:, off[0]] * (a[1] if k == 1 else phi[1])[:, off[1]]
        if nd == 3:
            t = t * (a[2] if k == 2 else phi[2])[:, off[2]]
        dw.append(t)
    return w, dw


def _inside(nd, lower, off, lo, hi):
    pos = [lower[d] + off[d] for d in range(nd)]
    ok = np.ones(pos[0].shape, bool)
    for d in range(nd):
        ok &= (pos[d] >= lo[d]) & (pos[d] <= hi[d])
    return pos, ok


def interp(geo, u, X, indices=None, xshift=None, U=None, GradU=None, n_rows=None):
    """IMPMethod::interpolateVelocity: U[s][c] and GradU[s][NDIM c + k], the stencil box
    clipped to the component's ghost box; list entries in order, the last duplicate wins.
    Also returns, per entry, whether a stencil was clipped below / above in each dim."""
    nd = geo.ndim
    idx, Xs = list_positions(X, indices, xshift)
    nrow = (np.asarray(X).shape[0] if n_rows is None else n_rows)
    if U is None:
        U = np.zeros((nrow, nd))
    if GradU is None:
        GradU = np.zeros((nrow, nd * nd))
    ne = len(idx)
    Ue = np.zeros((ne, nd))
    Ge = np.zeros((ne, nd * nd))
    clipped = np.zeros((ne, nd, 2), bool)
    for c in range(nd):
        lower, phi, a = _component_stencils(geo, c, Xs)
        glo, ghi = geo.ghost_box(c)
        for d in range(nd):
            clipped[:, d, 0] |= lower[d] < glo[d]
            clipped[:, d, 1] |= lower[d] + 5 > ghi[d]
        for off in _offsets(nd):
            pos, ok = _inside(nd, lower, off, glo, ghi)
            sel = tuple(np.where(ok, pos[d] - glo[d], 0) for d in reversed(range(nd)))
            v = u[c][sel]
            w, dw = _weights(nd, phi, a, off)
            Ue[:, c] = np.where(ok, Ue[:, c] + v * w, Ue[:, c])
            for k in range(nd):
                Ge[:, nd * c + k] = np.where(ok, Ge[:, nd * c + k] - v * dw[k], Ge[:, nd * c + k])
    for e in range(ne):  # sequential: a later entry of the same marker overwrites
        U[idx[e]] = Ue[e]
        GradU[idx[e]] = Ge[e]
    return U, GradU, clipped


def spread(geo, f, tau, wgt, X, indices=None, xshift=None, clip="patch", stats=False):
    """IMPMethod::spreadForce into f (modified in place): f(i_s) += (sum_k tau(c,k) dw_k) wgt / dV_c.
    With stats, also the number of contributions n_i and S_i = sum |contribution| per point."""
    nd = geo.ndim
    idx, Xs = list_positions(X, indices, xshift)
    tau = np.asarray(tau, dtype=np.float64)
    wg = np.asarray(wgt, dtype=np.float64)[idx]
    dV = 1.0
    for d in range(nd):
        dV = dV * geo.dx[d]
    cnt = [np.zeros(a.shape, np.int64) for a in f] if stats else None
    S = [np.zeros(a.shape) for a in f] if stats else None
    for c in range(nd):
        lower, phi, a = _component_stencils(geo, c, Xs)
        glo, _ = geo.ghost_box(c)
        blo, bhi = geo.patch_side_box(c) if clip == "patch" else geo.ghost_box(c)
        for off in _offsets(nd):
            pos, ok = _inside(nd, lower, off, blo, bhi)
            _, dw = _weights(nd, phi, a, off)
            val = np.zeros(len(idx))
            for k in range(nd):
                val = val + tau[idx, nd * c + k] * dw[k]
            contrib = val * wg / dV
            sel = tuple((pos[d] - glo[d])[ok] for d in reversed(range(nd)))
            np.add.at(f[c], sel, contrib[ok])
            if stats:
                np.add.at(cnt[c], sel, 1)
                np.add.at(S[c], sel, np.abs(contrib[ok]))
    return (f, cnt, S) if stats else f


# ---- pointwise ---------------------------------------------------------------------------

def _pad(rows, nd, z22):
    """[n][NDIM^2] rows as [n][3][3] tensors; in 2-D padded with (2,2) = z22."""
    rows = np.asarray(rows, dtype=np.float64)
    A = np.zeros((rows.shape[0], 3, 3))
    A[:, :nd, :nd] = rows.reshape(-1, nd, nd)
    if nd == 2:
        A[:, 2, 2] = z22
    return A


def det(A):
    """libMesh TypeTensor::det."""
    return (A[:, 0, 0] * (A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1])
            - A[:, 0, 1] * (A[:, 1, 0] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 0])
            + A[:, 0, 2] * (A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]))


def tensor_inverse(A, nd):
    """ibtk/libmesh_utilities.h:310-339."""
    R = np.zeros_like(A)
    det_A = det(A)
    if nd == 2:
        R[:, 0, 0] = +A[:, 1, 1] / det_A
        R[:, 0, 1] = -A[:, 0, 1] / det_A
        R[:, 1, 0] = -A[:, 1, 0] / det_A
        R[:, 1, 1] = +A[:, 0, 0] / det_A
        R[:, 2, 2] = 1.0
    else:
        R[:, 0, 0] = +(A[:, 2, 2] * A[:, 1, 1] - A[:, 2, 1] * A[:, 1, 2]) / det_A
        R[:, 0, 1] = -(A[:, 2, 2] * A[:, 0, 1] - A[:, 2, 1] * A[:, 0, 2]) / det_A
        R[:, 0, 2] = +(A[:, 1, 2] * A[:, 0, 1] - A[:, 1, 1] * A[:, 0, 2]) / det_A
        R[:, 1, 0] = -(A[:, 2, 2] * A[:, 1, 0] - A[:, 2, 0] * A[:, 1, 2]) / det_A
        R[:, 1, 1] = +(A[:, 2, 2] * A[:, 0, 0] - A[:, 2, 0] * A[:, 0, 2]) / det_A
        R[:, 1, 2] = -(A[:, 1, 2] * A[:, 0, 0] - A[:, 1, 0] * A[:, 0, 2]) / det_A
        R[:, 2, 0] = +(A[:, 2, 1] * A[:, 1, 0] - A[:, 2, 0] * A[:, 1, 1]) / det_A
        R[:, 2, 1] = -(A[:, 2, 1] * A[:, 0, 0] - A[:, 2, 0] * A[:, 0, 1]) / det_A
        R[:, 2, 2] = +(A[:, 1, 1] * A[:, 0, 0] - A[:, 1, 0] * A[:, 0, 1]) / det_A
    return R


def matmul(A, B):
    """(A B)(i,j) = sum_k A(i,k) B(k,j), k ascending from 0."""
    R = np.zeros_like(A)
    for i in range(3):
        for j in range(3):
            v = np.zeros(A.shape[0])
            for k in range(3):
                v = v + A[:, i, k] * B[:, k, j]
            R[:, i, j] = v
    return R


def _step(F, Ga, Gb, adt, nd):
    I = np.broadcast_to(np.eye(3), F.shape)
    return matmul(matmul(tensor_inverse(I - adt * Gb, nd), I + adt * Ga), F)


def deformation_update(scheme, dt, F_cur, G0, G1=None):
    """F_new (and F_half for "euler") as rows of NDIM^2: eulerStep :587-588, midpointStep
    :643, trapezoidalStep :703."""
    F_cur = np.asarray(F_cur, dtype=np.float64)
    nd = 2 if F_cur.shape[1] == 4 else 3
    F = _pad(F_cur, nd, 1.0)
    Ga = _pad(G0, nd, 0.0)
    Gb = _pad(G1, nd, 0.0) if scheme == "trapezoidal" else Ga
    out = _step(F, Ga, Gb, 0.5 * dt, nd)[:, :nd, :nd].reshape(-1, nd * nd)
    if scheme == "euler":
        return out, _step(F, Ga, Gb, 0.25 * dt, nd)[:, :nd, :nd].reshape(-1, nd * nd)
    return out, None


def kirchhoff_stress(F, c1, p0=0.0, beta=0.0):
    """tau = PP FF^T, PP = 2 c1 FF [- 2 p0 FF^-T] [+ beta log(det(FF^T FF)) FF^-T]; c1, p0,
    beta scalars or one value per point."""
    F = np.asarray(F, dtype=np.float64)
    nd = 2 if F.shape[1] == 4 else 3
    n = F.shape[0]
    c1, p0, beta = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (c1, p0, beta))
    FF = _pad(F, nd, 1.0)
    FFt = np.transpose(FF, (0, 2, 1)).copy()
    PP = (2.0 * c1)[:, None, None] * FF
    FinvT = np.transpose(tensor_inverse(FF, nd), (0, 2, 1))
    m = p0 != 0.0
    PP[m] = PP[m] - (2.0 * p0[m])[:, None, None] * FinvT[m]
    m = beta != 0.0
    CC = matmul(FFt, FF)
    PP[m] = PP[m] + (beta[m] * np.log(det(CC[m])))[:, None, None] * FinvT[m]
    return matmul(PP, FFt)[:, :nd, :nd].reshape(-1, nd * nd)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)

"""Plain numpy / math restatement of IBMethod's fluid sources and sinks, loop for loop:

* ``locations``  -- IBStandardSourceGen::getSourceLocations (IBStandardSourceGen.cpp:195-250)
* ``spread``     -- IBMethod::spreadFluidSource, the spread (IBMethod.cpp:828-859)
* ``normalize``  -- the consistency check and the boundary offset (:863-941)
* ``pressure``   -- IBMethod::interpolatePressure (:960-1063)

One patch, one rank.  The source loop is the outermost and a box is walked with x fastest, as
SAMRAI's Box iterator walks it; every sum is a serial float64 sum in that order.  A
cell-centred field is a numpy array of the ghost box, shape (n2, n1, n0) [x fastest].  The
tests hold this module to 50-digit known answers (tests/golden/source_kat.npz) and the
device code to this module.
"""
from __future__ import annotations

import math

import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Geo:
    """A patch: box lower corner, cells per dim, spacing, x_lower, ghost width."""

    def __init__(self, ilower, n, dx, x_lower, g):
        self.ndim = len(n)
        self.ilower = tuple(int(v) for v in ilower)
        self.n = tuple(int(v) for v in n)
        self.iupper = tuple(self.ilower[d] + self.n[d] - 1 for d in range(self.ndim))
        self.dx = tuple(float(v) for v in dx)
        self.x_lower = tuple(float(v) for v in x_lower)
        self.x_upper = tuple(self.x_lower[d] + (self.iupper[d] - self.ilower[d] + 1) * self.dx[d]
                             for d in range(self.ndim))
        self.g = int(g)

    def shape(self):
        return tuple(self.n[d] + 2 * self.g for d in reversed(range(self.ndim)))

    def alloc(self):
        return np.zeros(self.shape())

    def at(self, i):
        """The array index of cell i = (i0, i1[, i2])."""
        return tuple(i[d] - self.ilower[d] + self.g for d in reversed(range(self.ndim)))

    def box_slices(self, lo=None, hi=None):
        lo = self.ilower if lo is None else lo
        hi = self.iupper if hi is None else hi
        return tuple(slice(lo[d] - self.ilower[d] + self.g, hi[d] - self.ilower[d] + self.g + 1)
                     for d in reversed(range(self.ndim)))

    def dV(self):
        v = self.dx[0] * self.dx[1]
        return v * self.dx[2] if self.ndim == 3 else v


def cos_kernel(x, eps):
    """IBMethod.cpp:124-134"""
    if abs(x) > eps:
        return 0.0
    return 0.5 * (1.0 + math.cos(math.pi * x / eps)) / eps


def cell_index(X, x_lower, x_upper, dx, ilower, iupper):
    """IndexUtilities::getCellIndex (IndexUtilities-inl.h:66-89), one dimension."""
    dl, du = X - x_lower, X - x_upper
    if abs(dl) <= abs(du):
        return ilower + int(math.floor(dl / dx))
    return iupper + int(math.floor(du / dx)) + 1


def stencil(geo, r_src, X):
    """Per dimension: r, the centre cell, the half width and the box cut to the patch box
    (lo > hi: empty) -- IBMethod.cpp:832-848."""
    out = []
    for d in range(geo.ndim):
        dx = geo.dx[d]
        R = max(math.floor(r_src / dx + 0.5), 2.0)
        r = R * dx
        c = cell_index(X[d], geo.x_lower[d], geo.x_upper[d], dx, geo.ilower[d], geo.iupper[d])
        half = int(r / dx) + 1
        out.append(dict(R=int(R), r=r, centre=c, half=half, lo=max(c - half, geo.ilower[d]), hi=min(c + half, geo.iupper[d])))
    return out


def box_cells(st):
    """The cells of the clipped box, x fastest."""
    nd = len(st)
    if any(s["hi"] < s["lo"] for s in st):
        return
    if nd == 2:
        for j in range(st[1]["lo"], st[1]["hi"] + 1):
            for i in range(st[0]["lo"], st[0]["hi"] + 1):
                yield (i, j)
    else:
        for k in range(st[2]["lo"], st[2]["hi"] + 1):
            for j in range(st[1]["lo"], st[1]["hi"] + 1):
                for i in range(st[0]["lo"], st[0]["hi"] + 1):
                    yield (i, j, k)


def x_center(geo, d, i):
    return geo.x_lower[d] + geo.dx[d] * (float(i - geo.ilower[d]) + 0.5)


def weight_1d(geo, st, X, d, i):
    return cos_kernel(x_center(geo, d, i) - X[d], st[d]["r"])


def locations(X, node, source, n_src):
    """X_src[k][d] = sum X[node][d] / double(count_k) over the local nodes in ascending order,
    from Point::Zero() (IBStandardSourceGen.cpp:213-230)."""
    X = np.asarray(X, dtype=np.float64)
    nd = X.shape[1]
    node, source = np.asarray(node), np.asarray(source)
    count = np.bincount(source, minlength=n_src) if len(source) else np.zeros(n_src, dtype=np.int64)
    X_src = np.zeros((n_src, nd))
    for p in np.argsort(node, kind="stable"):
        k = int(source[p])
        for d in range(nd):
            X_src[k, d] += float(X[node[p], d]) / float(count[k])
    return X_src


def spread(geo, q, X_src, r_src, Q, stats=False):
    """q(i) += Q_n wgt in place (IBMethod.cpp:828-859).  stats: also, per cell, the number of
    sources whose clipped box holds it and the sum of their |Q_n| / (r0 r1 [r2])."""
    nd = geo.ndim
    cnt = np.zeros(geo.shape(), dtype=np.int64)
    S = np.zeros(geo.shape())
    for n in range(len(Q)):
        X = [float(v) for v in X_src[n]]
        st = stencil(geo, float(r_src[n]), X)
        rprod = math.prod(s["r"] for s in st)
        for i in box_cells(st):
            wgt = 1.0
            for d in range(nd):
                wgt *= weight_1d(geo, st, X, d, i[d])
            a = geo.at(i)
            q[a] += float(Q[n]) * wgt
            cnt[a] += 1
            S[a] += abs(float(Q[n])) / rprod
    return (q, cnt, S) if stats else q


def bdry_mask(geo, domain):
    """The cells of domain \\ interior, interior = the domain box shrunk by one cell in every
    dimension but the last (IBMethod.cpp:899-907), as a mask over the ghost-box array."""
    nd = geo.ndim
    lo, hi = domain
    idx = [np.arange(geo.ilower[d] - geo.g, geo.iupper[d] + geo.g + 1) for d in range(nd)]
    grids = np.meshgrid(*[idx[d] for d in reversed(range(nd))], indexing="ij")
    I = [grids[nd - 1 - d] for d in range(nd)]
    inside = np.ones(geo.shape(), dtype=bool)
    for d in range(nd):
        inside &= (I[d] >= lo[d]) & (I[d] <= hi[d])
    edge = np.zeros(geo.shape(), dtype=bool)
    for d in range(nd - 1):
        edge |= (I[d] == lo[d]) | (I[d] == hi[d])
    return inside & edge


def bdry_count(nd, domain):
    lo, hi = domain
    total = math.prod(hi[d] - lo[d] + 1 for d in range(nd))
    inner = math.prod(max(hi[d] - lo[d] + 1 - (2 if d < nd - 1 else 0), 0) for d in range(nd))
    return total - inner


def integral(geo, q):
    """sum q dV over the patch box, serially, x fastest."""
    dV = geo.dV()
    s = 0.0
    for v in q[geo.box_slices()].ravel():
        s += float(v) * dV
    return s


def inconsistent(q_total, Q):
    """The test at IBMethod.cpp:877."""
    Q_sum, Q_max = 0.0, 0.0
    for v in Q:
        Q_sum += float(v)
        Q_max = max(Q_max, abs(float(v)))
    return abs(q_total - Q_sum) > 1.0e-12 and abs(q_total - Q_sum) / max(Q_max, 1.0) > 1.0e-12


def normalize(geo, q, Q, domain=None, do_normalize=True):
    """IBMethod.cpp:863-941 in place.  Returns (totals, flagged): totals = [q_total, Q_sum,
    q_norm, integral_after]; flagged when either TBOX_ERROR would fire."""
    Q_sum = 0.0
    for v in Q:
        Q_sum += float(v)
    q_total = integral(geo, q)
    flagged = inconsistent(q_total, Q)
    if not do_normalize:
        return np.array([q_total, Q_sum, 0.0, q_total]), flagged
    vol = float(bdry_count(geo.ndim, domain))
    for d in range(geo.ndim):
        vol *= geo.dx[d]
    q_norm = -q_total / vol
    box = np.zeros(geo.shape(), dtype=bool)
    box[geo.box_slices()] = True
    q[bdry_mask(geo, domain) & box] += q_norm
    after = integral(geo, q)
    if abs(after) > 1.0e-10 * max(1.0, float(np.abs(q[geo.box_slices()]).max())):
        flagged = True
    return np.array([q_total, Q_sum, q_norm, after]), flagged


def pressure_norm(geo, p, domain):
    """IBMethod.cpp:960-1003: sum p dV / sum dV over the boundary cells in the patch box."""
    box = np.zeros(geo.shape(), dtype=bool)
    box[geo.box_slices()] = True
    dV = geo.dV()
    p_norm, vol = 0.0, 0.0
    for v in p[bdry_mask(geo, domain) & box]:  # boolean indexing walks the array x fastest
        p_norm += float(v) * dV
        vol += dV
    return p_norm / vol


def pressure(geo, p, X_src, r_src, domain=None, stats=False):
    """P_src[n] = sum p(i) wgt - p_norm (IBMethod.cpp:1005-1063).  stats: also, per source,
    the cells of its clipped box and the sum of |p| over them."""
    nd = geo.ndim
    p_norm = 0.0 if domain is None else pressure_norm(geo, p, domain)
    n_src = len(r_src)
    P = np.zeros(n_src)
    m = np.zeros(n_src, dtype=np.int64)
    A = np.zeros(n_src)
    for n in range(n_src):
        X = [float(v) for v in X_src[n]]
        st = stencil(geo, float(r_src[n]), X)
        acc = 0.0
        for i in box_cells(st):
            wgt = 1.0
            for d in range(nd):
                wgt *= weight_1d(geo, st, X, d, i[d]) * geo.dx[d]
            v = float(p[geo.at(i)])
            acc += v * wgt
            m[n] += 1
            A[n] += abs(v)
        P[n] = acc + (-p_norm)
    return (P, p_norm, m, A) if stats else P

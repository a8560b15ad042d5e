"""The levels the level-shape tests share (tests/test_level_cases_cpu.py checks their
preconditions on the CPU, tests/test_gpu_level_shapes.py runs them on the device): patches of
unequal extents at offset and negative indices, non-cubic tilings with tiles missing, a level
one patch thick in a periodic dim, and a level of more patches than the sweeps' LDS patch
table holds.  Host only (numpy and the C oracle); each case is built once per process and
left unchanged.

A case holds the patch boxes, the domain box and its periodic flags, dx and the domain's
x_lower, the markers X and Lagrangian values F, and per patch the interior list (markers
whose cell lies in the patch box, unshifted) and the ghost-box list (markers and periodic
images whose cell lies in the patch box grown by g, Xshift = +-L) -- built here in numpy from
each marker's cell, as test_gpu_level_lists._expected forms them, not with
le.level_index_lists (device code with its own test).  A patch's entries are in marker order,
a marker's images in shift order.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

from imp_cases import DX
from oracle import oracle as ora

NONNEG = ("IB_4", "BSPLINE_4", "PIECEWISE_LINEAR")  # kernels whose weights are >= 0
SPREAD_TOL = 1e-12                                  # the project's, for IB_6
X_LOWER = (0.3, -0.2, 0.1)
MANY_SAMPLE_FIXED = (0, 2047, 2048, 2196)
SHIFTS = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.int64)[:, ::-1]  # x fastest


class Case:
    def __init__(self, name, kernel, lo, n, dom_lo, dom_hi, periodic, X_cells, seed, dx=DX, x_lower=X_LOWER):
        """lo, n: (P, 3) patch lower corners and extents; X_cells: marker positions in cell
        units of the index space (wrapped into the domain in the periodic dims here)."""
        self.name, self.kernel = name, kernel
        self.g = ora.min_ghost_width(kernel)
        self.lo = np.asarray(lo, np.int64)
        self.n = np.asarray(n, np.int64)
        self.hi = self.lo + self.n - 1
        self.npatch = self.lo.shape[0]
        self.dom_lo, self.dom_hi = np.asarray(dom_lo, np.int64), np.asarray(dom_hi, np.int64)
        self.ext = self.dom_hi - self.dom_lo + 1
        self.periodic = np.asarray(periodic, bool)
        self.dx, self.x_lower = np.asarray(dx, np.float64), np.asarray(x_lower, np.float64)
        self.L = self.ext * self.dx
        t = np.asarray(X_cells, np.float64) - self.dom_lo
        t = np.where(self.periodic, t - np.floor(t / self.ext) * self.ext, t)
        self.X = np.ascontiguousarray(self.x_lower + t * self.dx)
        self.M = self.X.shape[0]
        self.cells = self.dom_lo + np.floor((self.X - self.x_lower) / self.dx).astype(np.int64)
        inside = (self.cells >= self.dom_lo) & (self.cells <= self.dom_hi)
        assert np.all(inside | ~self.periodic), "a marker outside the domain in a periodic dim"
        rng = np.random.default_rng(seed)
        self.F = rng.uniform(-1.0, 1.0, (self.M, 3))
        self._build_lists()

    # ---------------------------------------------------------------- lists
    def _members(self, ci, blo, bhi):
        ok = np.ones((self.npatch, ci.shape[0]), bool)
        for d in range(3):
            ok &= (ci[None, :, d] >= blo[:, None, d]) & (ci[None, :, d] <= bhi[:, None, d])
        return ok

    def _build_lists(self):
        c, g = self.cells, self.g
        q, m = np.nonzero(self._members(c, self.lo, self.hi))
        self.int_idx = m.astype(np.int32)
        self.int_off = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=self.npatch))]).astype(np.int64)
        glo, ghi = self.lo - g, self.hi + g
        blo, bhi = glo.min(0), ghi.max(0)
        qs, ms, ks = [], [], []
        for k, s in enumerate(SHIFTS):
            if np.any((s != 0) & ~self.periodic):
                continue
            ci = c + s * self.ext
            sel = np.nonzero(np.all((ci >= blo) & (ci <= bhi), axis=1))[0]  # near the level at all
            if sel.size == 0:
                continue
            q, j = np.nonzero(self._members(ci[sel], glo, ghi))
            qs.append(q)
            ms.append(sel[j])
            ks.append(np.full(q.size, k))
        q, m, k = np.concatenate(qs), np.concatenate(ms), np.concatenate(ks)
        o = np.lexsort((k, m, q))
        self.gh_idx = m[o].astype(np.int32)
        self.gh_shift = SHIFTS[k[o]]
        self.gh_xs = np.ascontiguousarray(self.gh_shift * self.L)
        self.gh_off = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=self.npatch))]).astype(np.int64)

    def interior(self, q):
        return self.int_idx[self.int_off[q]:self.int_off[q + 1]]

    def ghost(self, q):
        a, b = self.gh_off[q], self.gh_off[q + 1]
        return self.gh_idx[a:b], self.gh_xs[a:b]

    # ------------------------------------------------------------- geometry
    def patch_x_lower(self, q):
        return self.x_lower + (self.lo[q] - self.dom_lo) * self.dx

    def geoms(self, le, order=None):
        """the patches as le.Geometry (the GPU tests'), in `order` (default: as listed)"""
        return [le.Geometry([int(v) for v in self.lo[q]], [int(v) for v in self.hi[q]], self.g,
                            [float(v) for v in self.dx], [float(v) for v in self.patch_x_lower(q)])
                for q in (range(self.npatch) if order is None else order)]

    def array_shape(self, q, centering, comp=0, depth=1):
        ext = {"cell": 0, "node": 7, "side": 1 << comp, "edge": 7 & ~(1 << comp)}[centering]
        shp = tuple(int(self.n[q, d] + 2 * self.g + ((ext >> d) & 1)) for d in (2, 1, 0))
        return ((depth,) + shp) if centering in ("cell", "node") else shp

    def alloc(self, q, centering, depth=1):
        ncomp = 3 if centering in ("side", "edge") else 1
        return [np.zeros(self.array_shape(q, centering, a, depth)) for a in range(ncomp)]

    # --------------------------------------------------------------- oracle
    def oracle(self, op, q, centering, u, idx, xs, V, depth=1, kernel=None, X=None):
        """The C oracle on patch q alone -- it knows nothing of levels.  interp writes V's rows
        at idx, spread adds V's rows into u.  u: the patch's component arrays (side / edge:
        three; cell / node: one of `depth` planes); V: (M, 3) or (M, depth)."""
        kernel = kernel or self.kernel
        X = self.X if X is None else X
        idx = np.ascontiguousarray(idx, np.int32)
        if idx.size == 0:
            return
        lo, hi = [int(v) for v in self.lo[q]], [int(v) for v in self.hi[q]]
        dx, xl, gcw = [float(v) for v in self.dx], [float(v) for v in self.patch_x_lower(q)], [self.g] * 3
        xs = np.ascontiguousarray(xs, np.float64)
        if centering == "side":
            f = ora.side_interp if op == "interp" else ora.side_spread
            f(kernel, dx, xl, lo, hi, gcw, u, idx, xs, X, V)
        elif centering == "edge":  # every dim but the axis shifted by dx / 2, toEdgeBox
            for axis in range(3):
                xla = [xl[d] - (0.5 * dx[d] if d != axis else 0.0) for d in range(3)]
                hia = [hi[d] + (1 if d != axis else 0) for d in range(3)]
                Va = np.zeros(int(idx.max()) + 1)
                if op == "interp":
                    ora.interp(kernel, dx, xla, lo, hia, gcw, u[axis], idx, xs, X, Va, depth=1, axis=axis)
                    V[idx, axis] = Va[idx]
                else:
                    Va[idx] = V[idx, axis]
                    ora.spread(kernel, dx, xla, lo, hia, gcw, u[axis], idx, xs, X, Va, depth=1, axis=axis)
        else:
            pair = (ora.cell_interp, ora.cell_spread) if centering == "cell" else (ora.node_interp, ora.node_spread)
            pair[0 if op == "interp" else 1](kernel, dx, xl, lo, hi, gcw, u[0], idx, xs, X, V, depth)

    def spread_ref(self, q, centering, depth=1, kernel=None, F=None, lists=None, X=None):
        """(f_ref, S, n_q): the oracle's spread of F and of |F| on patch q's ghost-box list
        (or `lists` = (idx, xs)) into zeros, and the list's length."""
        F = self.values(centering, depth) if F is None else F
        idx, xs = self.ghost(q) if lists is None else lists
        f, S = self.alloc(q, centering, depth), self.alloc(q, centering, depth)
        self.oracle("spread", q, centering, f, idx, xs, np.ascontiguousarray(F), depth, kernel, X)
        self.oracle("spread", q, centering, S, idx, xs, np.ascontiguousarray(np.abs(F)), depth, kernel, X)
        return f, S, len(idx)

    def values(self, centering, depth=1):
        """the Lagrangian values a centring spreads: (M, 3) or (M, depth) columns of F"""
        return np.ascontiguousarray(self.F if centering in ("side", "edge") else self.F[:, :depth])


def spread_bound(n_q, S):
    """|f_dev - f_ref| <= (n_q + 4) 2^-52 S_i per point: each side sums at most n_q terms, a
    term is formed with at most 4 roundings (weight product, times F, over h^3), so the two
    differ by at most 2 (n_q - 1 + 4) 2^-53 S."""
    return (n_q + 4) * 2.0 ** -52 * S


def spread_ratio(kernel, got, ref, S, n_q):
    """The worst |diff| / bound over the points of one patch's component arrays: against
    spread_bound for the kernels with non-negative weights (a point with bound 0 must be
    equal), against SPREAD_TOL max |f_ref| for IB_6, whose weights change sign.  <= 1 passes."""
    worst = 0.0
    for g, r, s in zip(got, ref, S):
        d = np.abs(np.asarray(g) - r)
        if kernel in NONNEG:
            b = spread_bound(n_q, s)
            if np.any(d[b == 0.0] != 0.0):
                return np.inf
            pos = b > 0.0
            if pos.any():
                worst = max(worst, float((d[pos] / b[pos]).max()))
        else:
            scale = np.abs(r).max()
            if scale == 0.0:
                if d.max() != 0.0:
                    return np.inf
            else:
                worst = max(worst, float(d.max() / (SPREAD_TOL * scale)))
    return worst


# ------------------------------------------------------------------ the cases
RAGGED_LO = ((-45, -30, -40), (-5, -30, -40), (-5, 7, -10), (10, -20, 30), (40, -45, -5), (-43, -30, 30))
RAGGED_N = ((40, 37, 70), (9, 10, 12), (33, 17, 40), (5, 4, 6), (20, 25, 30), (38, 20, 10))
RAGGED_FACE = (0, 1)      # abut face to face (x); so do 0 and 5 (z)
RAGGED_EDGE = (0, 2)      # meet only at an edge
RAGGED_SMALL, RAGGED_FAR = 3, 4
RAGGED_DENSE_CELL = (12, -18, 32)
RAGGED_SHEET = slice(0, 600)   # the sheet's markers, then the dense cell's, then the uniform ones
RAGGED_DENSE = slice(600, 750)


def _ragged(kernel):
    """Six patches of one level: a large one (two z segments, several column rows), a thin one
    against its +x face, one touching it along an edge only, a (5, 4, 6) one, one far from all
    others and one on its +z face that also reaches the domain's periodic upper z face."""
    g = ora.min_ghost_width(kernel)
    lo, n = np.array(RAGGED_LO), np.array(RAGGED_N)
    rng = np.random.default_rng(20)
    # a sheet one cell thick (z cell -35) across the x face between patches 0 and 1
    sheet = np.stack([rng.uniform(-14, 4, 600), rng.uniform(-30, -20, 600), rng.uniform(-35, -34, 600)], axis=1)
    dense = np.array(RAGGED_DENSE_CELL) + rng.uniform(0.02, 0.98, (150, 3))
    vol = np.prod(n + 2 * g, axis=1)
    cnt = 250 + np.round(3500 * vol / vol.sum()).astype(int)
    parts = [sheet, dense] + [rng.uniform(lo[q] - g, lo[q] + n[q] + g, (cnt[q], 3)) for q in range(len(lo))]
    return Case("ragged", kernel, lo, n, (-60, -50, -40), (69, 49, 39), (0, 0, 1), np.concatenate(parts), 21)


TILES_N, TILES_P, TILES_DOM_LO = (40, 24, 10), (2, 3, 4), (-40, 24, 5)
# (0, 0, 0): a corner; (1, 1, 2): interior in y and z (x has two tiles: under a periodic x
# every tile has both x neighbours, under a wall none has)
TILES_MISSING = ((0, 0, 0), (1, 1, 2))
TILES_FLAGS = ((1, 1, 1), (1, 0, 1), (0, 1, 0))


def _tiling(name, kernel, n, P, dom_lo, periodic, missing, M, seed, extra=None):
    n, P, dom_lo = np.array(n), np.array(P), np.array(dom_lo)
    tc = np.array([t[::-1] for t in np.ndindex(*P[::-1]) if t[::-1] not in missing])  # x fastest
    rng = np.random.default_rng(seed)
    Xc = dom_lo + rng.uniform(0.0, 1.0, (M, 3)) * (n * P)
    if extra is not None:
        Xc = np.concatenate([Xc, extra(rng, tc, n, dom_lo)])
    c = Case(name, kernel, dom_lo + tc * n, np.tile(n, (len(tc), 1)), dom_lo, dom_lo + n * P - 1, periodic, Xc,
             seed + 1)
    c.tile_n, c.ntile, c.tc = n, P, tc
    c.present = np.zeros(tuple(P[::-1]), bool)  # [tz, ty, tx]
    c.present[tc[:, 2], tc[:, 1], tc[:, 0]] = True
    return c


def _many_extra(rng, tc, n, dom_lo):
    # five markers inside each of the patches the oracle is always run on
    return np.concatenate([dom_lo + tc[q] * n + rng.uniform(0.0, 1.0, (5, 3)) * n for q in MANY_SAMPLE_FIXED])


@functools.lru_cache(maxsize=None)
def case(name, kernel="IB_4", periodic=None, holes=False):
    """ragged (per kernel); tiles (per kernel, flag set, holes); narrow; many."""
    if name == "ragged":
        return _ragged(kernel)
    if name == "tiles":
        return _tiling("tiles", kernel, TILES_N, TILES_P, TILES_DOM_LO, periodic or (1, 1, 1),
                       TILES_MISSING if holes else (), 6000, 30)
    if name == "narrow":  # one patch across the z period: a marker and its image in one list
        return _tiling("narrow", "IB_4", (24, 20, 12), (2, 3, 1), (-24, 20, 7), (0, 0, 1), (), 3000, 40)
    if name == "many":
        return _tiling("many", "IB_4", (4, 4, 4), (13, 13, 13), (-8, 4, 0), (1, 1, 1), (), 5980, 50, _many_extra)
    raise KeyError(name)


def many_sample(c):
    """64 patches of `many`: the first and last, those either side of the LDS table's end, and
    60 picked at random"""
    rng = np.random.default_rng(51)
    rest = np.setdiff1d(np.arange(c.npatch), MANY_SAMPLE_FIXED)
    return sorted(set(MANY_SAMPLE_FIXED) | set(rng.choice(rest, 60, replace=False).tolist()))


# ------------------------------------------------------------ the level ghost fill
def fill_sources(c, q, centering, comp):
    """Of a tiling's patch q, per point of component comp's array (z, y, x): `ghost` (outside
    the patch's own points: li < g or li >= g + n in some dim, so a side array's upper face
    too), `supplied` (a patch owns the point's wrapped cell and every wrap is across a
    periodic face) and `src`, the np.ix_ index of that cell in a field over the domain."""
    g = c.g
    dr, ok, wt, gi = [], [], [], []
    for d in range(3):
        e = int(c.tile_n[d]) + 2 * g + (1 if centering == "side" and d == comp else 0)
        li = np.arange(e)
        r = np.where(li < g, -1, np.where(li >= g + c.tile_n[d], 1, 0))
        t = c.tc[q, d] + r
        dr.append(r)
        ok.append((r == 0) | ((t >= 0) & (t < c.ntile[d])) | bool(c.periodic[d]))
        wt.append(t % c.ntile[d])
        gi.append(wt[d] * c.tile_n[d] + (li - r * c.tile_n[d] - g))
    ghost = (dr[2][:, None, None] != 0) | (dr[1][None, :, None] != 0) | (dr[0][None, None, :] != 0)
    allowed = ok[2][:, None, None] & ok[1][None, :, None] & ok[0][None, None, :]
    supplied = ghost & allowed & c.present[np.ix_(wt[2], wt[1], wt[0])]
    return ghost, supplied, np.ix_(gi[2], gi[1], gi[0])


def fill_fields(c, centering, depth, seed):
    """One global field per component over the domain, (depth, N2, N1, N0)."""
    rng = np.random.default_rng(seed)
    ncomp = 3 if centering == "side" else 1
    return [rng.uniform(-1.0, 1.0, (depth,) + tuple(int(v) for v in c.ext[::-1])) for _ in range(ncomp)]


def fill_arrays(c, q, centering, depth, G, rng):
    """Patch q's arrays before and after the level ghost fill: its own points hold the global
    field, every other point a value of its own (drawn from rng); after the fill a supplied
    ghost point holds the field at its wrapped index and the others what they held.  Returns
    (before, after, supplied), per component; cell arrays (depth, z, y, x), side (z, y, x)."""
    before, after, sup = [], [], []
    for a in range(len(G)):
        ghost, supplied, src = fill_sources(c, q, centering, a)
        field = G[a][(slice(None),) + src]
        junk = rng.uniform(2.0, 3.0, field.shape)
        b = np.where(ghost, junk, field)
        w = np.where(supplied, field, b)
        if centering == "side":
            b, w = b[0], w[0]
        before.append(np.ascontiguousarray(b))
        after.append(np.ascontiguousarray(w))
        sup.append(supplied)
    return before, after, sup

"""Inputs and scripted call sequences for the handle-reuse tests (helper, not a test file).

tests/test_gpu_reuse.py bins one Markers (or Level) handle again and again -- another list
length, kernel, geometry, dimension, list kind or patch table -- and holds every result to a
fresh Context and a fresh handle that saw only the last binning: history independence, bit
for bit.  tests/test_reuse_cases_cpu.py asserts on these inputs alone, with numpy and the C
oracle, that consecutive states differ enough for a handle that silently kept its previous
state to be seen.  Everything here is host data (seeded numpy, no torch), built once per
process and left unchanged.

One marker array of M = 6000 rows serves every state, so that an index kept from an earlier
state still names a valid row; the positions are per geometry.

A state is what the handle was last binned with: State(geom, kernel, lst, X, F) -- the patch
(`A3`, `B3`, `A2`), the kernel, the list kind (LISTS), the name of the position set and the
seed of the Lagrangian values spread at it (F is rewritten between states).  A sequence is a
list of Step(op, arg, do, extra): op "bin" (arg = (geom, kernel, lst, X)) or "rebin" (arg = X);
`do` says which side-centred calls follow ("both", "interp", "spread"), `extra` the further
centrings ("cell" = cell data of depth 2, "node").
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import cases3d as c3
import level_cases as lc
from cases2d import MIN_GHOST
from oracle import oracle as ora

M = 6000
N_SMALL, N_DUPS, N_DUP_TWICE, N_COUNTED = 700, 3000, 300, 4500
KERNELS = ("IB_4", "IB_6", "PIECEWISE_LINEAR", "IB_3", "BSPLINE_4")
G = max(MIN_GHOST[k] for k in KERNELS)  # one ghost width for every kernel used
SPREAD_TOL = 1e-12                      # tests/test_gpu_spread_fstream.py, test_gpu_spread_ds.py
LISTS = ("big", "small", "dups", "counted", "empty", "counted0")

Patch = namedtuple("Patch", "name ndim N ilower iupper g dx x_lower")
_PATCHES = {  # cells, ilower, dx, x_lower
    "A3": ((40, 24, 20), (-3, 5, 2), (0.11, 0.07, 0.05), (-0.4, 0.3, 1.0)),
    "B3": ((72, 40, 12), (4, -6, -1), (0.06, 0.09, 0.12), (0.5, -1.0, 0.2)),
    "A2": ((40, 24), (-3, 5), (0.11, 0.07), (-0.4, 0.3)),
}


def patch(name):
    N, il, dx, xl = _PATCHES[name]
    return Patch(name, len(N), N, il, tuple(il[d] + N[d] - 1 for d in range(len(N))), G, dx, xl)


def col_geom(name, kernel):
    """the 3-D patch's column grid as make_col_geom lays it out (cases3d.plain_geometry)"""
    p = patch(name)
    return c3.plain_geometry(kernel, p.ilower, p.iupper, p.g, p.dx, p.x_lower, name)


def nbuckets(name, kernel):
    g = col_geom(name, kernel)
    return g.nz * g.ncx * g.ncy * c3.NBAND


def array_shape(p, centering, comp=0, depth=1):
    ext = {"cell": 0, "node": (1 << p.ndim) - 1, "side": 1 << comp}[centering]
    n = [p.N[d] + 2 * p.g + ((ext >> d) & 1) for d in range(p.ndim)]
    shape = tuple(reversed(n))
    return ((depth,) + shape) if centering in ("cell", "node") else shape


def ncomp(p, centering):
    return p.ndim if centering == "side" else 1


def qcols(p, centering, depth):
    return p.ndim if centering == "side" else depth


# ------------------------------------------------------------------ positions
@functools.lru_cache(maxsize=None)
def positions(name):
    """{"X0", "X_moved", "X_within"} of patch `name`, (M, ndim) each.

    X0: uniform over the patch and a margin of 4 % around it; in 3-D z / dz lies in
    k - [0.15, 0.25] for an integer k (test_rebin_within_cells_flips_shifted_anchors'
    construction).  X_moved: every entry moved by up to 0.6 cell per dim.  X_within (3-D): z
    raised by 0.35 dz, to k + [0.1, 0.2] -- the same cell under NINT, the other anchor in the
    frame shifted by -dz/2."""
    p = patch(name)
    rng = np.random.default_rng(zlib.crc32(f"reuse{name}".encode()))
    N, dx, xl = np.array(p.N, np.float64), np.array(p.dx), np.array(p.x_lower)
    t = rng.uniform(-0.04, 1.04, (M, p.ndim)) * N
    if p.ndim == 3:
        t[:, 2] = rng.integers(1, p.N[2] - 1, M) - rng.uniform(0.15, 0.25, M)
    X0 = xl + t * dx
    out = {"X0": X0, "X_moved": X0 + rng.uniform(-0.6, 0.6, (M, p.ndim)) * dx}
    if p.ndim == 3:
        Xw = X0.copy()
        Xw[:, 2] += 0.35 * dx[2]
        out["X_within"] = Xw
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def anchors(kernel, p, X):
    """every marker's key cell per dim by the kernel family's anchor rule (cases3d.FAM), and
    its z anchor in the frame shifted by -dz/2 (3-D)"""
    fam = c3.FAM[kernel]
    xo = (X - np.array(p.x_lower)) / np.array(p.dx)
    if fam == 0:
        a = c3._nint(xo)
    elif fam == 2:
        a = np.trunc(xo) - (xo < 0.0)
    else:
        a = c3._nint(xo - 0.5)
    az = c3._nint(xo[:, -1] - 0.5) if fam == 0 else a[:, -1]
    return a.astype(np.int64), az.astype(np.int64)


# ---------------------------------------------------------------------- lists
@functools.lru_cache(maxsize=None)
def dup_list(name):
    """(idx, Xshift) of `dups` on patch `name`: 3000 entries in random order, N_DUP_TWICE
    markers named twice with different shifts; a fifth of the first namings shifted by -1, 0
    or 1 cell per dim, a second naming by one cell more in x and z and one less in y."""
    p = patch(name)
    rng = np.random.default_rng(7)  # the same entries on every patch
    perm = rng.permutation(M)
    n1 = N_DUPS - N_DUP_TWICE
    cs = np.zeros((N_DUPS, 3))
    pick = rng.random(n1) < 0.2
    cs[:n1][pick] = rng.integers(-1, 2, (int(pick.sum()), 3))
    cs[n1:] = cs[:N_DUP_TWICE] + np.array([1.0, -1.0, 1.0])
    idx = np.concatenate([perm[:n1], perm[:N_DUP_TWICE]])
    o = rng.permutation(N_DUPS)
    return idx[o].astype(np.int32), np.ascontiguousarray(cs[o][:, :p.ndim] * np.array(p.dx))


def entries(geom, lst):
    """the list as the oracle takes it: (idx int32, Xshift (n, ndim))"""
    p = patch(geom)
    if lst == "dups":
        return dup_list(geom)
    n = {"big": M, "small": N_SMALL, "counted": N_COUNTED, "empty": 0, "counted0": 0}[lst]
    return np.arange(n, dtype=np.int32), np.zeros((n, p.ndim))


# --------------------------------------------------------------------- fields
@functools.lru_cache(maxsize=None)
def fields(geom, centering, depth=1):
    """the Eulerian arrays interp reads on patch `geom`: seeded standard normals"""
    p = patch(geom)
    rng = np.random.default_rng(zlib.crc32(f"u{geom}{centering}{depth}".encode()))
    return [rng.standard_normal(array_shape(p, centering, a, depth)) for a in range(ncomp(p, centering))]


@functools.lru_cache(maxsize=None)
def lag_values(seed, cols):
    """F of a state: (M, cols) standard normals"""
    return np.random.default_rng(1000 + seed).standard_normal((M, cols))


# --------------------------------------------------------------------- oracle
State = namedtuple("State", "geom kernel lst X F")


def state_X(st):
    return positions(st.geom)[st.X]


def _args(st):
    p = patch(st.geom)
    return st.kernel, list(p.dx), list(p.x_lower), list(p.ilower), list(p.iupper), [p.g] * p.ndim


@functools.lru_cache(maxsize=None)
def oracle_interp(st, centering="side", depth=1):
    """(Q, named): the oracle's interp on the state's list (a marker named twice takes its
    last entry's value, as the Fortran's sequential loop leaves it); rows no entry names: 0"""
    p = patch(st.geom)
    idx, xs = entries(st.geom, st.lst)
    Q = np.zeros((M, qcols(p, centering, depth)))
    named = np.zeros(M, bool)
    named[idx] = True
    if idx.size:
        u = fields(st.geom, centering, depth)
        if centering == "side":
            ora.side_interp(*_args(st), u, idx, xs, state_X(st), Q)
        else:
            f = ora.cell_interp if centering == "cell" else ora.node_interp
            f(*_args(st), u[0], idx, xs, state_X(st), Q, depth)
    return Q, named


def oracle_spread(st, centering="side", depth=1, order=None):
    """the oracle's spread of the state's F into zeros, the list taken in `order` (positions
    in the list, e.g. Markers.order()) or as it stands"""
    p = patch(st.geom)
    idx, xs = entries(st.geom, st.lst)
    if order is not None:
        idx, xs = idx[order], xs[order]
    f = [np.zeros(array_shape(p, centering, a, depth)) for a in range(ncomp(p, centering))]
    if idx.size:
        F = lag_values(st.F, qcols(p, centering, depth))
        if centering == "side":
            ora.side_spread(*_args(st), f, idx, np.ascontiguousarray(xs), state_X(st), F)
        else:
            g = ora.cell_spread if centering == "cell" else ora.node_spread
            g(*_args(st), f[0], idx, np.ascontiguousarray(xs), state_X(st), F, depth)
    return f


@functools.lru_cache(maxsize=None)
def oracle_spread_listed(st, centering="side", depth=1):
    return oracle_spread(st, centering, depth)


# ------------------------------------------------------------------ sequences
Step = namedtuple("Step", "op arg do extra")
EXTRA = {"cell": ("cell", 2), "node": ("node", 1)}


def B(geom, kernel, lst, X, do="both", extra=()):
    return Step("bin", (geom, kernel, lst, X), do, tuple(extra))


def R(X, do="both", extra=()):
    return Step("rebin", X, do, tuple(extra))


def _grow_shrink():
    s = []
    for lst in ("small", "big", "small"):
        s += [B("A3", "IB_4", lst, "X0"), R("X_moved")]
    return s


def _kernels():
    return [B("A3", k, "big", X, extra=("cell", "node"))
            for k, X in (("IB_4", "X0"), ("PIECEWISE_LINEAR", "X_moved"), ("IB_6", "X0"), ("IB_4", "X_moved"))]


def _geometries():
    s = []
    for geom in ("A3", "B3", "A3"):
        s += [B(geom, "IB_4", "big", "X0"), R("X_moved")]
    return s


def _dimensions(kernel, lst2d):
    return [B("A3", kernel, "big", "X0"), R("X_moved"),
            B("A2", kernel, lst2d, "X0"), R("X_moved"),
            B("A3", kernel, "big", "X0"), R("X_moved")]


def _list_kinds():
    return [B("A3", "IB_4", "big", "X0"), B("A3", "IB_4", "dups", "X_moved"), B("A3", "IB_4", "big", "X0"),
            B("A3", "IB_4", "counted", "X_within"), R("X_moved"), B("A3", "IB_4", "big", "X0")]


def _rebin_states(kernel):
    x = ("node",)
    return [B("A3", kernel, "big", "X0", "spread", x), R("X0", "none"), R("X0", "spread", x),
            R("X_moved", "interp"), R("X_moved", "spread", x),
            R("X_within", "none"), R("X_within", "spread", x),
            R("X0", "spread", x),
            # a stream that stood across a re-binning must not stand across the next binning
            R("X0", "spread", x), B("A3", kernel, "big", "X_moved", "spread", x),
            # nor may the parities of the order before a binning be compared after it: those of
            # X_within recorded, a binning at X0, then X_within again -- nothing moves, and the
            # stream built at X0 is split by other shifted-z anchors
            R("X_within", "spread", x), B("A3", kernel, "big", "X0", "spread", x), R("X_within", "spread", x)]


def _empty():
    return [B("A3", "IB_4", "big", "X0"), B("A3", "IB_4", "empty", "X_moved"), B("A3", "IB_4", "big", "X0"),
            B("A3", "IB_4", "counted0", "X_moved"), R("X0"), B("A3", "IB_4", "big", "X_moved")]


# the sequences one handle runs through tests/test_gpu_reuse.py's interpreter (1-6 and 11 of
# the eleven; 7-10 involve settings, levels or several handles and are written out there)
SEQUENCES = {
    "grow_shrink": _grow_shrink(),
    "kernels": _kernels(),
    "geometries": _geometries(),
    "dimensions-IB_4-big": _dimensions("IB_4", "big"),
    "dimensions-IB_3-big": _dimensions("IB_3", "big"),
    "dimensions-IB_4-dups": _dimensions("IB_4", "dups"),
    "list_kinds": _list_kinds(),
    "rebin_states-IB_4": _rebin_states("IB_4"),
    "rebin_states-BSPLINE_4": _rebin_states("BSPLINE_4"),
    "empty": _empty(),
}


def states(seq):
    """the State after every step of a sequence (F's seed is the step's number)"""
    out, cur = [], None
    for k, s in enumerate(seq):
        if s.op == "bin":
            cur = State(*s.arg, k)
        else:
            cur = State(cur.geom, cur.kernel, cur.lst, s.arg, k)
        out.append(cur)
    return out


# --------------------------------------------------------------------- levels
LEVEL_KERNEL = "IB_4"


def _level_markers(rng, lo, n, g):
    """M markers over the patches' ghost boxes, 250 each and the rest by volume, in cell units"""
    vol = np.prod(n + 2 * g, axis=1).astype(np.float64)
    cnt = 250 + np.floor((M - 250 * len(lo)) * vol / vol.sum()).astype(int)
    cnt[0] += M - cnt.sum()
    return np.concatenate([rng.uniform(lo[q] - g + 0.5, lo[q] + n[q] + g - 0.5, (cnt[q], 3)) for q in range(len(lo))])


@functools.lru_cache(maxsize=None)
def level(name):
    """`LA`: level_cases' tile (40, 24, 10) on a (2, 2, 1) tiling at its dom_lo, periodic --
    four equal patches; `LB`: the first four of level_cases' ragged patches (unequal, offset,
    negative indices), periodic in z only; `LC`: the tile on a (2, 2, 2) tiling -- eight.
    One dx (level_cases' default) and M markers each.  The case carries X_moved: every marker
    moved by up to 0.6 cell (the lists stay those of X)."""
    g = ora.min_ghost_width(LEVEL_KERNEL)
    seed = {"LA": 60, "LB": 70, "LC": 80}[name]
    if name == "LB":
        lo, n = np.array(lc.RAGGED_LO[:4]), np.array(lc.RAGGED_N[:4])
        Xc = _level_markers(np.random.default_rng(seed), lo, n, g)
        c = lc.Case(name, LEVEL_KERNEL, lo, n, (-60, -50, -40), (69, 49, 39), (0, 0, 1), Xc, seed + 1)
    else:
        P = (2, 2, 1) if name == "LA" else (2, 2, 2)
        c = lc._tiling(name, LEVEL_KERNEL, lc.TILES_N, P, lc.TILES_DOM_LO, (1, 1, 1), (), M, seed)
    assert c.M == M
    rng = np.random.default_rng(seed + 2)
    c.X_moved = np.ascontiguousarray(c.X + rng.uniform(-0.6, 0.6, c.X.shape) * c.dx)
    c.u = [[rng.standard_normal(c.array_shape(q, "side", a)) for a in range(3)] for q in range(c.npatch)]
    return c


def level_X(c, X):
    return c.X if X == "X0" else c.X_moved


def level_oracle(c, X, F):
    """(Q, f): the oracle patch by patch at positions `X` ("X0" / "X_moved") -- the interp
    of each patch's interior list from c.u, the spread of F on its ghost-box list into zeros"""
    Xn = level_X(c, X)
    Q = np.zeros((M, 3))
    f = []
    for q in range(c.npatch):
        idx = c.interior(q)
        c.oracle("interp", q, "side", c.u[q], idx, np.zeros((idx.size, 3)), Q, X=Xn)
        f.append(c.spread_ref(q, "side", F=F, X=Xn)[0])
    return Q, f


def relisted(c):
    """other lists with the same offsets length: each patch's ghost-box list without its
    every third entry, and the interior entries (all of them are in the ghost-box list's
    unshifted part) it still holds"""
    gi, gx, go, ii, io = [], [], [0], [], [0]
    for q in range(c.npatch):
        idx, xs = c.ghost(q)
        keep = np.arange(idx.size) % 3 != 2
        idx, xs = idx[keep], xs[keep]
        plain = idx[~xs.any(axis=1)]
        inner = c.interior(q)
        inner = inner[np.isin(inner, plain)]
        gi.append(idx)
        gx.append(xs)
        go.append(go[-1] + idx.size)
        ii.append(inner)
        io.append(io[-1] + inner.size)
    return (np.concatenate(gi).astype(np.int32), np.ascontiguousarray(np.concatenate(gx)), go,
            np.concatenate(ii).astype(np.int32), io)

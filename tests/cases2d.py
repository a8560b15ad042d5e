"""Inputs for the 2-D brick path at sizes where its loops repeat (helper, not a test file).

The 2-D kernels (ibamr_amd/csrc/le_hot.hip) bin into 16^2-cell bricks, numbered in tiles
of 4x4 bricks; the interp takes 2x2 bricks (one brick for the wide kernels) per work item
and the spread one 32^2-cell super-brick, with its candidates listed per class of two
anchor rows.  The builders here return host arrays only, so CPU and GPU tests share them;
`structure` restates in numpy the counts that decide how often the kernels' loops run, so
that a test can assert that its input reaches the code it is meant to reach.

Geometries are non-periodic patches with ilower = (3, -2), dx = (0.1, 0.07) and
x_lower = (-0.3, 0.2), as tests/test_gpu_parity.py's make_case has them.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

ALL = ["PIECEWISE_CONSTANT", "DISCONTINUOUS_LINEAR", "PIECEWISE_LINEAR", "PIECEWISE_CUBIC", "IB_3", "IB_4",
       "IB_4_W8", "IB_6", "BSPLINE_4"]
# W, LO, HI: stencil points per dim; every stencil index lies in [key + LO, key + HI]
# (ibamr_amd/csrc/le_internal.h kKernelInfo)
KINFO = {
    "PIECEWISE_CONSTANT": (1, 0, 1), "DISCONTINUOUS_LINEAR": (2, -1, 2), "PIECEWISE_LINEAR": (2, -1, 2),
    "PIECEWISE_CUBIC": (4, -2, 3), "IB_3": (3, -1, 2), "IB_4": (4, -2, 2), "IB_4_W8": (8, -4, 4),
    "IB_6": (6, -3, 3), "BSPLINE_4": (4, -2, 2),
}
# LEInteractor::getMinimumGhostWidth (oracle.min_ghost_width; IB_3 counts as 4 wide there)
MIN_GHOST = {"PIECEWISE_CONSTANT": 1, "DISCONTINUOUS_LINEAR": 2, "PIECEWISE_LINEAR": 2, "PIECEWISE_CUBIC": 3,
             "IB_3": 3, "IB_4": 3, "IB_4_W8": 5, "IB_6": 4, "BSPLINE_4": 3}

B = 16          # brick edge (cells)
SB = 2 * B      # super-brick edge
TILE = 4        # bricks per tile edge
CW = 2          # anchor rows per candidate class
BLOCK = 256     # interp: markers per pass of a work item
CHUNK = 64      # spread: candidates per chunk of a class
SUBPASS = 1024  # k_cand: neighbourhood entries per sub-pass (KMAX * SBLOCK)

ILOWER = (3, -2)
DX = (0.1, 0.07)
X_LOWER = (-0.3, 0.2)

# name -> (cells, tiles): the tile counts hold for every kernel at its minimum ghost
# width and one more (asserted in geometry())
GEOMS = {
    "wide": ((150, 40), (3, 1)),   # 12 items: G = 8, a second round of 4 with 4 skipped; nt0 != nt1
    "tall": ((40, 150), (1, 3)),   # the transpose: an x/y swap in the tile index
    "big": ((270, 150), (5, 3)),   # 60 items: G = 56, per = 7, a second round of 4
}
# markers of the `uniform` set.  At about five listed, inside entries per cell a class
# (2 rows by 32 + HI - LO columns) holds some 350 of them and a brick some 1 300.  The
# sizes are set by the preconditions of tests/test_cases2d_cpu.py: with 20 000 markers on
# `wide` the longest class has about 180 candidates (under three chunks of 64) and a brick
# about 530 markers; with 40 000 on `big` a neighbourhood has about 1 500 entries (under
# two sub-passes of 1024) and a class about 70.
UNIFORM_M = {"wide": 60_000, "tall": 60_000, "big": 400_000}

# (geometry, marker set, kernel, extra ghost cells) of every case tests/test_gpu_2d_dense.py
# runs; tests/test_cases2d_cpu.py checks each against the preconditions below.
# One kernel of each class-loop period NPH * NQ (8, 12 and 20) and of each family:
FIVE = ["IB_4", "IB_6", "IB_4_W8", "PIECEWISE_CONSTANT", "PIECEWISE_CUBIC"]
CLUSTER_KERNELS = ["IB_4", "IB_6", "IB_3", "PIECEWISE_CONSTANT"]
GPU_CASES = ([("wide", "uniform", k, 0) for k in ALL] +
             [(n, "uniform", k, 1 if (n, k) == ("tall", "IB_4") else 0) for n in ("tall", "big") for k in FIVE] +
             [("wide", "cluster", k, 0) for k in CLUSTER_KERNELS])

Geom = namedtuple("Geom", "name kernel N ilower iupper g dx x_lower L kmin nb nt nbricks")
Case = namedtuple("Case", "geom X idx xshift F")


def geometry(name, kernel, extra_ghost=0):
    """The patch `name` for `kernel`, and its brick grid as make_bin_geom lays it out."""
    N, tiles = GEOMS[name]
    W, LO, HI = KINFO[kernel]
    g = MIN_GHOST[kernel] + extra_ghost
    iupper = tuple(ILOWER[d] + N[d] - 1 for d in range(2))
    kmin, nb, nt = [], [], []
    for d in range(2):
        E = N[d] + 2 * g + 2 + HI - LO          # key cells whose stencil can touch an array
        bricks = -(-E // B)
        nt.append(-(-bricks // TILE))
        nb.append(nt[d] * TILE)
        kmin.append(ILOWER[d] - g - HI)
    assert tuple(nt) == tiles, f"{name} {kernel} g={g}: tiles {nt}, the case is built for {tiles}"
    L = tuple(N[d] * DX[d] for d in range(2))
    return Geom(name, kernel, N, ILOWER, iupper, g, DX, X_LOWER, L, tuple(kmin), tuple(nb), tuple(nt),
                nb[0] * nb[1])


def plain_geometry(kernel, ilower, iupper, g, dx, x_lower):
    """Any non-periodic 2-D patch as a Geom (for `structure`)."""
    W, LO, HI = KINFO[kernel]
    N = tuple(iupper[d] - ilower[d] + 1 for d in range(2))
    kmin, nb, nt = [], [], []
    for d in range(2):
        E = N[d] + 2 * g + 2 + HI - LO
        nt.append(-(-(-(-E // B)) // TILE))
        nb.append(nt[d] * TILE)
        kmin.append(ilower[d] - g - HI)
    L = tuple(N[d] * dx[d] for d in range(2))
    return Geom("plain", kernel, N, tuple(ilower), tuple(iupper), g, tuple(dx), tuple(x_lower), L, tuple(kmin),
                tuple(nb), tuple(nt), nb[0] * nb[1])


def uniform(geom, seed, M=None):
    """Markers uniform over the patch and a margin around it; five far outside, five on
    exact half-cell positions in x; a listed subset in random order, a fifth of it with
    shifts of -L, 0 or L per dim; standard normal F."""
    rng = np.random.default_rng(seed)
    M = UNIFORM_M[geom.name] if M is None else M
    xlo, L = np.array(geom.x_lower), np.array(geom.L)
    X = xlo + rng.uniform(-0.1, 1.1, (M, 2)) * L
    X[:5] = xlo + rng.uniform(-2.0, 3.0, (5, 2)) * L
    X[5:10, 0] = xlo[0] + (np.arange(5) + 2) * geom.dx[0] * 0.5
    idx = rng.permutation(M)[: M - 37].astype(np.int32)
    n = idx.size
    xs = np.zeros((n, 2))
    pick = rng.random(n) < 0.2
    xs[pick] = rng.integers(-1, 2, (int(pick.sum()), 2)) * L
    F = rng.standard_normal((M, 2))
    return Case(geom, X, idx, xs, F)


def cluster_cell(geom):
    """The cluster's cell (absolute index): one cell inside the corner shared by four
    super-bricks that is also a tile corner in x -- key cell rel = (63, 31)."""
    rel = (TILE * B - 1, SB - 1)
    assert geom.nb[0] * B > rel[0] + 1 and geom.nb[1] * B > rel[1] + 1
    return tuple(geom.kmin[d] + rel[d] for d in range(2))


def cluster(geom, seed):
    """8 000 uniform markers, then 2 000 at one point and 2 000 more inside that point's
    cell; the full list, no shifts, F uniform in [0.5, 1.5].

    The sizes are a condition of the spread tolerance, not a measurement: at most about
    4 100 contributions of one sign land on a grid point, so two summation orders differ
    by at most 2 n 2^-53 = 9.1e-13 of the sum, under the project's 1e-12."""
    rng = np.random.default_rng(seed)
    MB, MC = 8000, 2000
    xlo, L, dx = np.array(geom.x_lower), np.array(geom.L), np.array(geom.dx)
    X = np.empty((MB + 2 * MC, 2))
    X[:MB] = xlo + rng.uniform(-0.1, 1.1, (MB, 2)) * L
    cell = np.array(cluster_cell(geom))
    i = cell - np.array(geom.ilower)
    assert (i - 8 >= 0).all() and (i + 8 < np.array(geom.N)).all(), "the cluster's stencils lie inside the patch"
    # a quarter cell above the cell's lower corner: NINT(x), floor(x) and NINT(x - 1/2) all
    # give this cell, so every kernel family keys the point here
    X[MB:MB + MC] = xlo + (i + 0.25) * dx
    X[MB + MC:] = xlo + (i + rng.uniform(0.0, 1.0, (MC, 2))) * dx
    M = X.shape[0]
    idx = np.arange(M, dtype=np.int32)
    F = rng.uniform(0.5, 1.5, (M, 2))
    return Case(geom, X, idx, np.zeros((M, 2)), F)


def one_super_brick(geom, seed, M=10_000):
    """Every marker inside super-brick (1, 1), at least HI + 1 cells from its edge, so no
    stencil leaves it: the other work items have no candidates."""
    rng = np.random.default_rng(seed)
    W, LO, HI = KINFO[geom.kernel]
    xlo, dx = np.array(geom.x_lower), np.array(geom.dx)
    lo = np.array(geom.kmin) + SB + (HI + 1) - np.array(geom.ilower)       # relative cell indices
    hi = np.array(geom.kmin) + 2 * SB - (HI + 1) - np.array(geom.ilower)
    assert (lo >= 0).all() and (hi < np.array(geom.N)).all()
    X = xlo + rng.uniform(lo, hi, (M, 2)) * dx
    idx = np.arange(M, dtype=np.int32)
    F = rng.standard_normal((M, 2))
    return Case(geom, X, idx, np.zeros((M, 2)), F)


@functools.lru_cache(maxsize=4)
def case(name, kind, kernel, extra_ghost=0):
    """The case (geometry, marker set, kernel), built once; callers leave it unchanged."""
    geom = geometry(name, kernel, extra_ghost)
    seed = zlib.crc32(f"{name}{kind}{kernel}".encode())
    return {"uniform": uniform, "cluster": cluster}[kind](geom, seed)


Structure = namedtuple("Structure", "ninside neighbourhood classes interp_items n_spread_items n_interp_items")


def structure(geom, X, idx, xshift):
    """The counts that decide how often the 2-D kernels' loops run, restated in numpy.

    The key cell is taken as floor((X + shift - xlo) / dx) for every kernel, where the
    closed-form kernels round to nearest and the linear ones round x - 1/2: a marker can
    sit one cell off.  The tests compare these counts with thresholds they exceed by a
    good margin, so that is accurate enough.

    neighbourhood[sy, sx]: listed entries k_cand walks for that super-brick (its 4 bricks
        in x; in y the rows whose stencils can reach it).
    classes[sy, sx, k]: entries of class k (anchor rows 2k - HI, 2k - HI + 1 relative to
        the super-brick) that can reach it -- the length of its candidate list.
    interp_items: markers per interp work item (2x2 bricks for W <= 4, else one brick).
    """
    W, LO, HI = KINFO[geom.kernel]
    Xs = X[idx] + xshift
    ok = np.isfinite(Xs).all(axis=1)
    rel = np.zeros((idx.size, 2), dtype=np.int64)
    for d in range(2):
        xo = (Xs[:, d] - geom.x_lower[d]) / geom.dx[d]
        ok &= np.abs(xo) < 1.0e9
        r = np.floor(np.where(ok, xo, 0.0)).astype(np.int64) + geom.ilower[d] - geom.kmin[d]
        ok &= (r >= 0) & (r < geom.nb[d] * B)
        rel[:, d] = r
    rel = rel[ok]
    n0, n1 = geom.nb[0] * B, geom.nb[1] * B
    cells = np.bincount(rel[:, 1] * n0 + rel[:, 0], minlength=n0 * n1).reshape(n1, n0)
    P = np.zeros((n1 + 1, n0 + 1), dtype=np.int64)
    P[1:, 1:] = cells.cumsum(0).cumsum(1)

    def box(x0, x1, y0, y1):  # entries with rel x in [x0, x1), rel y in [y0, y1)
        x0, x1 = max(x0, 0), min(x1, n0)
        y0, y1 = max(y0, 0), min(y1, n1)
        if x0 >= x1 or y0 >= y1:
            return 0
        return int(P[y1, x1] - P[y0, x1] - P[y1, x0] + P[y0, x0])

    ns0, ns1 = geom.nb[0] // 2, geom.nb[1] // 2
    ncls = (SB - 1 + HI - LO) // CW + 1
    nbh = np.zeros((ns1, ns0), dtype=np.int64)
    cls = np.zeros((ns1, ns0, ncls), dtype=np.int64)
    for sy in range(ns1):
        for sx in range(ns0):
            x0, y0 = sx * SB, sy * SB
            nbh[sy, sx] = box(x0 - B, x0 + SB + B, y0 - HI, y0 + SB - LO)
            for k in range(ncls):
                r0 = y0 - HI + k * CW
                cls[sy, sx, k] = box(x0 - HI, x0 + SB - LO, r0, min(r0 + CW, y0 + SB - LO))
    e = SB if W <= 4 else B
    items = cells.reshape(n1 // e, e, n0 // e, e).sum(axis=(1, 3))
    return Structure(int(ok.sum()), nbh, cls, items, geom.nbricks // 4, geom.nbricks // (4 if W <= 4 else 1))

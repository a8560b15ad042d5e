"""Inputs for the 3-D column sweeps at sizes where their loops repeat (helper, not a test file).

The 3-D kernels (ibamr_amd/csrc/le_sweep.hip) bin into columns of 32 x 16 key cells in
(x, y), swept plane by plane in z.  The spread takes the candidates of one (column, anchor
plane) in chunks of 64; the interp pools the markers of 4 anchor planes and deals them to
its 4 waves in chunks of 64.  The builders here return host arrays only, so CPU and GPU
tests share them; `structure` restates in numpy the counts that decide how often those
loops run, so that a test can assert that its input reaches the code it is meant to reach.
`segments` restates how the planes are cut into work items, and `bucket_keys` the bin key
of every list entry exactly -- the GPU test holds the library's order to it, which ties the
column grid restated here to the one on the device.

Geometries are non-periodic patches with ilower = (3, -2, 5), dx = (0.1, 0.07, 0.05) and
x_lower = (-0.3, 0.2, 1.0), as tests/test_gpu_parity.py's make_case has them; `wide_unit`
is `wide` in the frame of Geometry.periodic_unit (ilower 0, the unit box).
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from cases2d import ALL, KINFO, MIN_GHOST  # kKernelInfo and getMinimumGhostWidth, restated there

COLX = 32          # column edge in x (le_internal.h:91)
COLY = 16          # column edge in y (le_internal.h:93, IBTK_LE_COLY)
NBAND = 9          # reach bands of a column (le_internal.h:97)
CHUNK = 64         # spread: candidates per chunk, one per lane (le_sweep.hip:43, SW)
IWAVES = 4         # interp: waves per item = anchor planes per group (le_sweep.hip:790)
MIN_SEG_SMALL = 8  # planes per segment of a patch with few columns (le_sweep.hip:2445)

ILOWER = (3, -2, 5)
DX = (0.1, 0.07, 0.05)
X_LOWER = (-0.3, 0.2, 1.0)

# name -> cells.  No patch is narrower than 62 cells in x: PIECEWISE_CONSTANT (ghost width 1,
# HI - LO = 1) has N + 4 key cells in x and needs more than 64 of them for a third real
# column, without which no column has eight real neighbours.
GEOMS = {
    "wide": (70, 40, 20),   # 3-4 real columns in x and in y, 24-39 anchor planes
    "tall": (62, 70, 20),   # more rows than columns: the x/y swap of the column index
    "deep": (62, 36, 90),   # about a hundred anchor planes, for the segment settings
    "wide_unit": (70, 40, 20),
    "half": (70, 40, 36),   # `wide`, taller: room above lower_half's markers for a segment inside the patch
}
# markers of the `uniform` set: about 0.83 listed markers per cell of the box they are
# drawn from (the patch and a 10 % margin, 1.2^3 of its cells).  With 60 000 on `wide` the
# busiest interior (column, anchor) of PIECEWISE_CONSTANT has under 6 * 64 candidates.
UNIFORM_M = {"wide": 80_000, "tall": 124_000, "deep": 288_000, "wide_unit": 80_000, "half": 145_000}

# one kernel of each code shape of the sweeps and of each family
PATHS = ["IB_4", "IB_6", "IB_4_W8", "PIECEWISE_CUBIC", "IB_3", "PIECEWISE_LINEAR", "PIECEWISE_CONSTANT"]
FILL_KERNELS = ["IB_6", "IB_4_W8", "PIECEWISE_CUBIC", "IB_3", "PIECEWISE_CONSTANT"]
# (geometry, marker set, kernel, extra ghost cells) of every case tests/test_gpu_3d_dense.py
# runs; tests/test_cases3d_cpu.py checks each against its preconditions.
GPU_CASES = ([("wide", "uniform", k, 0) for k in ALL] +
             [("tall", "uniform", k, 1 if k == "IB_4" else 0) for k in PATHS] +
             [("wide", "cluster", k, 0) for k in PATHS] +
             [("deep", "uniform", k, 0) for k in PATHS] +
             [("half", "lower_half", k, 0) for k in PATHS] +
             [("wide_unit", "uniform", k, 0) for k in FILL_KERNELS])

Geom = namedtuple("Geom", "name kernel N ilower iupper g dx x_lower L org ncx ncy nz")
Case = namedtuple("Case", "geom X idx xshift F")


def plain_geometry(kernel, ilower, iupper, g, dx, x_lower, name="plain"):
    """Any 3-D patch and its column grid as make_col_geom lays it out (le_abi.cpp:457-477)."""
    W, LO, HI = KINFO[kernel]
    N = tuple(iupper[d] - ilower[d] + 1 for d in range(3))
    lo = [ilower[d] - g for d in range(3)]
    hi = [iupper[d] + g + 1 for d in range(3)]           # + 1: the extra face / node
    org = [lo[d] - HI for d in range(3)]
    ext = [hi[d] - LO - org[d] + 1 for d in range(3)]    # key cells whose stencil can touch an array
    khi0 = org[0] + ext[0] - 1                           # last key cell in x
    org[0] -= COLX                                       # a guard column, then down to the
    org[0] -= (org[0] - lo[0]) % 16                      # arrays' first index + a multiple of 16
    ncx = (khi0 + 1 - org[0] + COLX - 1) // COLX + 1
    ncy = (ext[1] + COLY - 1) // COLY + 2
    org[1] -= COLY
    L = tuple(N[d] * dx[d] for d in range(3))
    return Geom(name, kernel, N, tuple(ilower), tuple(iupper), g, tuple(dx), tuple(x_lower), L, tuple(org), ncx, ncy,
                ext[2])


def geometry(name, kernel, extra_ghost=0):
    """The patch `name` for `kernel`; columns 0 and ncx-1 and rows 0 and ncy-1 are guards."""
    N = GEOMS[name]
    g = MIN_GHOST[kernel] + extra_ghost
    if name.endswith("_unit"):
        ilower, dx, xlo = (0, 0, 0), tuple(1.0 / n for n in N), (0.0, 0.0, 0.0)
    else:
        ilower, dx, xlo = ILOWER, DX, X_LOWER
    iupper = tuple(ilower[d] + N[d] - 1 for d in range(3))
    return plain_geometry(kernel, ilower, iupper, g, dx, xlo, name)


def segments(geom, seg_items=0):
    """(planes per segment, segments) of a single patch's sweeps, as sweep_segments cuts them
    (le_sweep.hip:2445-2468; seg_items: ctx.tune("seg_items"), 0 = unset)."""
    nz, ncol = geom.nz, geom.ncx * geom.ncy
    want = seg_items if seg_items > 0 else 16384  # IBTK_LE_SEG_ITEMS
    s = -(-nz * ncol // want)
    if s < 64 and seg_items <= 0:  # MIN_SEG
        s = -(-nz // max(nz // 64, 1))
    ncol_real = (geom.ncx - 2) * (geom.ncy - 2)
    if seg_items <= 0 and ncol_real * -(-nz // s) < 1024:  # SMALL_ITEMS
        s = max(-(-nz // -(-1024 // ncol_real)), MIN_SEG_SMALL)
    elif s < 32:
        s = 32
    s = max(min(s, nz), 1)
    s = -(-nz // -(-nz // s))  # equal segments
    return s, -(-nz // s)


def uniform(geom, seed, M=None, zcap=None):
    """Markers uniform over the patch and a margin around it; five far outside, five on
    exact half-cell positions in x; a listed subset in random order, a fifth of it with
    shifts of -L, 0 or L per dim; standard normal F.  zcap: z capped at that fraction of
    the patch height."""
    rng = np.random.default_rng(seed)
    M = UNIFORM_M[geom.name] if M is None else M
    xlo, L = np.array(geom.x_lower), np.array(geom.L)
    X = xlo + rng.uniform(-0.1, 1.1, (M, 3)) * L
    X[:5] = xlo + rng.uniform(-2.0, 3.0, (5, 3)) * L
    X[5:10, 0] = xlo[0] + (np.arange(5) + 2) * geom.dx[0] * 0.5
    if zcap is not None:
        X[:, 2] = np.minimum(X[:, 2], xlo[2] + zcap * L[2])
    idx = rng.permutation(M)[: M - 37].astype(np.int32)
    n = idx.size
    xs = np.zeros((n, 3))
    pick = rng.random(n) < 0.2
    xs[pick] = rng.integers(-1, 2, (int(pick.sum()), 3)) * L
    if zcap is not None:
        xs[:, 2] = 0.0  # no image above the cap
    F = rng.standard_normal((M, 3))
    return Case(geom, X, idx, xs, F)


def lower_half(geom, seed):
    """`uniform` with z capped at 45 % of the patch height and no shift in z: the items
    above own ghost points and have no candidates."""
    return uniform(geom, seed, zcap=0.45)


def cluster_cell(geom):
    """The cluster's cell (absolute index): the last key cell in x and in y of real column
    (1, 1), so band xb = 2, yb = 2 and a candidate of columns (1, 1), (2, 1), (1, 2) and
    (2, 2); in the patch's middle plane."""
    return (geom.org[0] + 2 * COLX - 1, geom.org[1] + 2 * COLY - 1, geom.ilower[2] + geom.N[2] // 2)


def cluster(geom, seed):
    """8 000 uniform markers, then 2 000 at one point and 2 000 more inside that point's
    cell; the full list, no shifts, F uniform in [0.5, 1.5].

    The sizes are a condition of the spread tolerance, not a measurement: at most about
    4 100 contributions of one sign land on a grid point, so two summation orders differ
    by at most 2 n 2^-53 = 9.1e-13 of the sum, under the project's 1e-12."""
    rng = np.random.default_rng(seed)
    MB, MC = 8000, 2000
    xlo, L, dx = np.array(geom.x_lower), np.array(geom.L), np.array(geom.dx)
    X = np.empty((MB + 2 * MC, 3))
    X[:MB] = xlo + rng.uniform(-0.1, 1.1, (MB, 3)) * L
    i = np.array(cluster_cell(geom)) - np.array(geom.ilower)
    W, LO, HI = KINFO[geom.kernel]
    assert (i + LO - 1 >= -geom.g).all() and (i + HI + 1 < np.array(geom.N) + geom.g).all(), \
        "the cluster's stencils lie inside the arrays"
    # a quarter cell above the cell's lower corner: NINT(x), floor(x) and NINT(x - 1/2) all
    # give this cell, so every kernel family keys the point here
    X[MB:MB + MC] = xlo + (i + 0.25) * dx
    X[MB + MC:] = xlo + (i + rng.uniform(0.0, 1.0, (MC, 3))) * dx
    M = X.shape[0]
    idx = np.arange(M, dtype=np.int32)
    F = rng.uniform(0.5, 1.5, (M, 3))
    return Case(geom, X, idx, np.zeros((M, 3)), F)


@functools.lru_cache(maxsize=8)
def case(name, kind, kernel, extra_ghost=0):
    """The case (geometry, marker set, kernel), built once; callers leave it unchanged."""
    geom = geometry(name, kernel, extra_ghost)
    seed = zlib.crc32(f"3d{name}{kind}{kernel}".encode())
    return {"uniform": uniform, "cluster": cluster, "lower_half": lower_half}[kind](geom, seed)


# the families' key anchors (le_stencil.h:93-98): 0 NINT(x), 1 and 3 NINT(x - 1/2), 2 lagrangian_floor(x)
FAM = {"IB_4": 0, "BSPLINE_4": 0, "IB_6": 0, "IB_4_W8": 0, "PIECEWISE_LINEAR": 1, "DISCONTINUOUS_LINEAR": 1,
       "PIECEWISE_CUBIC": 2, "IB_3": 2, "PIECEWISE_CONSTANT": 3}


def _nint(x):  # Fortran NINT / C round: halves away from zero
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def bucket_keys(geom, X, idx, xshift):
    """(key, rel, inside) of every list entry as k_bin_col computes them (le_sweep.hip:107-194):
    the key cell by the family's own anchor rule, relative to the column grid; the bucket
    key ((plane * ncol + column) * 9 + band), or the bucket count for an entry outside the
    grid.  The library's order is the stable sort of the list by this key."""
    W, LO, HI = KINFO[geom.kernel]
    fam = FAM[geom.kernel]
    ext = (geom.ncx * COLX, geom.ncy * COLY, geom.nz)
    Xs = X[idx] + xshift
    inside = np.ones(idx.size, bool)
    rel = np.zeros((idx.size, 3), dtype=np.int64)
    for d in range(3):
        xo = (Xs[:, d] - geom.x_lower[d]) / geom.dx[d]
        fin = np.abs(xo) < 1.0e9  # false for NaN too
        xo = np.where(fin, xo, 0.0)
        if fam == 0:
            a = _nint(xo)
        elif fam == 2:
            a = np.trunc(xo) - (xo < 0.0)  # lagrangian_floor: -2.0 gives -3
        else:
            a = _nint(xo - 0.5)
        r = a.astype(np.int64) + geom.ilower[d] - geom.org[d]
        inside &= fin & (r >= 0) & (r < ext[d])
        rel[:, d] = r
    xl, yl = rel[:, 0] % COLX, rel[:, 1] % COLY
    xb = np.where(xl <= -1 - LO, 0, np.where(xl >= COLX - HI, 2, 1))
    yb = np.where(yl <= -1 - LO, 0, np.where(yl >= COLY - HI, 2, 1))
    col = (rel[:, 1] // COLY) * geom.ncx + rel[:, 0] // COLX
    ncol = geom.ncx * geom.ncy
    key = (rel[:, 2] * ncol + col) * NBAND + 3 * xb + yb
    return np.where(inside, key, geom.nz * ncol * NBAND), rel, inside


Structure = namedtuple("Structure", "ninside own cand from_dir pool real interior inner_column ncand")


def structure(geom, X, idx, xshift):
    """The counts that decide how often the 3-D sweeps' loops run, restated in numpy.

    The key cell is taken as floor((X + shift - xlo) / dx) for every kernel, where the
    closed-form kernels round to nearest and the linear ones round x - 1/2: a marker can
    sit one cell off.  The tests compare these counts with thresholds they exceed by a
    good margin, so that is accurate enough.

    own[a, cy, cx]: listed markers keyed in anchor plane a of column (cx, cy).
    cand[a, cy, cx]: the spread's candidates of that (column, anchor): key cells of plane a
        with kx in [X0 - HI, X0 + 31 - LO] and ky in [Y0 - HI, Y0 + 15 - LO], (X0, Y0) the
        column's first key cell -- every key cell one of whose stencil points the column owns.
    from_dir[cy, cx, j, i]: of those, over all planes, the ones keyed in column
        (cx + i - 1, cy + j - 1); filled for the interior columns only.
    pool[s]: the interp's groups of IWAVES anchor planes starting at planes s, s + 4, ...:
        own summed over each group, [group, cy, cx].
    real: real columns in x and in y;  interior: the (cy, cx) with eight real neighbours;
    inner_column: some real column lies wholly inside the patch box in x and y.
    """
    W, LO, HI = KINFO[geom.kernel]
    ncx, ncy, nz = geom.ncx, geom.ncy, geom.nz
    ext = (ncx * COLX, ncy * COLY, nz)
    Xs = X[idx] + xshift
    ok = np.isfinite(Xs).all(axis=1)
    rel = np.zeros((idx.size, 3), dtype=np.int64)
    for d in range(3):
        xo = (Xs[:, d] - geom.x_lower[d]) / geom.dx[d]
        ok &= np.abs(xo) < 1.0e9
        r = np.floor(np.where(ok, xo, 0.0)).astype(np.int64) + geom.ilower[d] - geom.org[d]
        ok &= (r >= 0) & (r < ext[d])
        rel[:, d] = r
    rel = rel[ok]
    n0, n1 = ext[0], ext[1]
    cells = np.bincount((rel[:, 2] * n1 + rel[:, 1]) * n0 + rel[:, 0], minlength=nz * n1 * n0).reshape(nz, n1, n0)
    own = cells.reshape(nz, ncy, COLY, ncx, COLX).sum(axis=(2, 4))
    P = np.zeros((nz, n1 + 1, n0 + 1), dtype=np.int64)
    P[:, 1:, 1:] = cells.cumsum(1).cumsum(2)

    def box(x0, x1, y0, y1):  # per plane: key cells with x in [x0, x1), y in [y0, y1)
        x0, x1 = max(x0, 0), min(x1, n0)
        y0, y1 = max(y0, 0), min(y1, n1)
        if x0 >= x1 or y0 >= y1:
            return np.zeros(nz, dtype=np.int64)
        return P[:, y1, x1] - P[:, y0, x1] - P[:, y1, x0] + P[:, y0, x0]

    cand = np.zeros((nz, ncy, ncx), dtype=np.int64)
    from_dir = np.zeros((ncy, ncx, 3, 3), dtype=np.int64)
    interior = [(cy, cx) for cy in range(2, ncy - 2) for cx in range(2, ncx - 2)]
    for cy in range(ncy):
        for cx in range(ncx):
            x0, x1 = cx * COLX - HI, cx * COLX + COLX - LO
            y0, y1 = cy * COLY - HI, cy * COLY + COLY - LO
            cand[:, cy, cx] = box(x0, x1, y0, y1)
            if (cy, cx) not in interior:
                continue
            for j in range(3):
                for i in range(3):
                    cx0, cy0 = (cx + i - 1) * COLX, (cy + j - 1) * COLY
                    from_dir[cy, cx, j, i] = box(max(x0, cx0), min(x1, cx0 + COLX), max(y0, cy0),
                                                 min(y1, cy0 + COLY)).sum()
    pool = []
    for s in range(IWAVES):
        ng = (nz - s) // IWAVES
        pool.append(own[s:s + ng * IWAVES].reshape(ng, IWAVES, ncy, ncx).sum(axis=1))
    inner = any(geom.org[0] + cx * COLX >= geom.ilower[0] and geom.org[0] + cx * COLX + COLX - 1 <= geom.iupper[0] and
                geom.org[1] + cy * COLY >= geom.ilower[1] and geom.org[1] + cy * COLY + COLY - 1 <= geom.iupper[1]
                for cy in range(1, ncy - 1) for cx in range(1, ncx - 1))
    real = cand[:, 1:ncy - 1, 1:ncx - 1]
    return Structure(int(ok.sum()), own, cand, from_dir, pool, (ncx - 2, ncy - 2), interior, inner, int(real.sum()))

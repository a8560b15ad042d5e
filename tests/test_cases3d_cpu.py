"""The 3-D dense cases (tests/cases3d.py) reach the code they are built for.

tests/test_gpu_3d_dense.py runs the 3-D column sweeps at sizes where their loops repeat.
Whether they repeat is a property of the input, checked here without a GPU: a column has
real neighbours on every side and candidates from each of them, its busiest anchor plane
takes the spread through several turns of its middle-chunk loops, a group of four anchor
planes gives every wave of the interp several chunks, and a column lies wholly inside the
patch box.  The old 3-D input, make_case's 13x14x15 patch, meets none of these, which is
the gap the dense cases close.
"""
import numpy as np
import pytest

import cases3d as c3
from oracle import oracle as ora

SPREAD_TOL = 1e-12
DIRS = {(0, 0): "SW", (0, 1): "S", (0, 2): "SE", (1, 0): "W", (1, 1): "own", (1, 2): "E", (2, 0): "NW", (2, 1): "N",
        (2, 2): "NE"}


def _id(v):
    return "-".join(str(x) for x in v)


def test_kernel_tables_match_the_oracle():
    for k in c3.ALL:
        assert c3.MIN_GHOST[k] == ora.min_ghost_width(k), k
        assert c3.KINFO[k][0] == ora.STENCIL[k] or k == "IB_3", k


def reachable(kernel):
    """The neighbour directions (j, i) a column can have candidates from: a key cell west
    or south of it reaches it with its upper stencil points (HI > 0), one east or north of
    it with its lower ones (LO < 0).  PIECEWISE_CONSTANT has LO = 0 -- its one point is
    never below the key cell -- so its columns have west, south and south-west neighbours
    only; every other kernel reaches all eight."""
    W, LO, HI = c3.KINFO[kernel]
    ok = [HI > 0, True, LO < 0]
    return [(j, i) for j in range(3) for i in range(3) if ok[j] and ok[i]]


@pytest.mark.parametrize("case", c3.GPU_CASES, ids=_id)
def test_preconditions(case):
    name, kind, kernel, extra = case
    cs = c3.case(name, kind, kernel, extra)
    g = cs.geom
    st = c3.structure(g, cs.X, cs.idx, cs.xshift)
    dirs = reachable(kernel)
    assert len(dirs) == (4 if kernel == "PIECEWISE_CONSTANT" else 9)
    need = (60 if kind == "cluster" else 6) * c3.CHUNK
    assert st.real[0] >= 3 and st.real[1] >= 3, "a column with eight real neighbours"
    assert st.interior
    # the interior column with the busiest anchor among those fed from every reachable side
    fed = [c for c in st.interior if all(st.from_dir[c[0], c[1], j, i] > 0 for j, i in dirs)]
    assert fed, f"no interior column has candidates from all of {[DIRS[d] for d in dirs]}"
    cy, cx = max(fed, key=lambda c: st.cand[:, c[0], c[1]].max())
    busiest = int(st.cand[:, cy, cx].max())
    pools = [int(p.max()) for p in st.pool]
    print(f"{_id(case)}: grid {g.ncx} x {g.ncy} x {g.nz} (real {st.real[0]} x {st.real[1]}), inside {st.ninside} of "
          f"{cs.idx.size}, interior column ({cx}, {cy}): busiest anchor {busiest} candidates, from "
          f"{ {DIRS[d]: int(st.from_dir[cy, cx, d[0], d[1]]) for d in dirs} }, pools {pools}, "
          f"candidates {st.ncand}, inner column {st.inner_column}")
    assert busiest > need, "k_spread_sweep: several turns of the middle-chunk loops in one anchor"
    for s in range(c3.IWAVES):
        assert pools[s] > 16 * c3.CHUNK, f"k_interp_sweep: alignment {s}, every wave at least four chunks"
    assert st.inner_column, "a real column wholly inside the patch box in x and y"
    assert st.ncand <= 4 * cs.idx.size, "the candidate stream's capacity"
    if kind == "cluster":
        # the cluster's cell is the last of real column (1, 1) in x and y: four columns take it
        c = np.array(c3.cluster_cell(g)) - np.array(g.org)
        assert (c[0] % c3.COLX, c[1] % c3.COLY, c[0] // c3.COLX, c[1] // c3.COLY) == (c3.COLX - 1, c3.COLY - 1, 1, 1)
        assert all(st.cand[c[2], y, x] > need for y in (1, 2) for x in (1, 2))
        # its (column, segment) is heavy: more own markers than four times the mean and than 2048
        # (build_items), so the heavy-first item table runs
        assert st.own[c[2], 1, 1] > 2048 >= 4 * (cs.idx.size // (g.ncx * g.ncy))
    if kind == "lower_half":
        W, LO, HI = c3.KINFO[kernel]
        S, nseg = c3.segments(g)
        assert S == c3.MIN_SEG_SMALL
        zlo, zhi = g.ilower[2] - g.org[2], g.iupper[2] - g.org[2]  # the patch box's planes

        def empty(s):  # no candidate reaches segment s (a plane of margin either way)
            return not st.cand[max(s * S - HI - 1, 0):(s + 1) * S - LO + 1].any()

        # the last segment holds ghost planes and no candidates: zero_ghosts_spread zeroes them
        assert (nseg - 1) * S + S - 1 > zhi and empty(nseg - 1)
        # a segment wholly inside the patch box in z has none either: with a column inside
        # the box in x and y (above) that item owns no ghost point and returns at once
        inner = [s for s in range(nseg) if s * S >= zlo and (s + 1) * S - 1 <= zhi and empty(s)]
        print(f"{_id(case)}: {nseg} segments of {S} planes, patch planes {zlo}..{zhi}, inner and empty: {inner}")
        assert inner


def test_segment_settings():
    """What test_deep_segments' settings give on `deep`: segments of 8 planes unset, of at
    most 32 with 100000, three or four with 64, and the whole patch as one with 1."""
    for k in c3.PATHS:
        g = c3.geometry("deep", k)
        assert c3.segments(g) == (c3.MIN_SEG_SMALL, -(-g.nz // c3.MIN_SEG_SMALL)), k
        S, n = c3.segments(g, 100000)
        assert 24 <= S <= 32 and n in (3, 4), k
        S, n = c3.segments(g, 64)
        assert 30 <= S <= 40 and n == 3, k
        assert c3.segments(g, 1) == (g.nz, 1), k
        assert g.nz // (c3.KINFO[k][2] - c3.KINFO[k][1] + 2) >= 10, "the ring wraps ten times and more"


@pytest.mark.parametrize("name", ["wide", "tall", "deep"])
def test_column_grids(name):
    """3-4 real columns each way on `wide`, more rows than columns on `tall`, about a
    hundred anchor planes on `deep`; ncx != ncy for some kernel."""
    grids = {k: c3.geometry(name, k) for k in c3.ALL}
    for k, g in grids.items():
        assert g.ncx - 2 >= 3 and g.ncy - 2 >= 3, k
        assert (g.org[0] - (g.ilower[0] - g.g)) % 16 == 0
        W, LO, HI = c3.KINFO[k]
        # the real columns hold every key cell whose stencil can touch an array
        assert g.org[0] + c3.COLX <= g.ilower[0] - g.g - HI
        assert g.org[0] + (g.ncx - 1) * c3.COLX - 1 >= g.iupper[0] + g.g + 1 - LO
        assert g.org[1] + (g.ncy - 1) * c3.COLY - 1 >= g.iupper[1] + g.g + 1 - LO
        if name == "wide":
            assert g.ncx - 2 <= 4 and g.ncy - 2 <= 4 and 24 <= g.nz <= 40, k
        if name == "tall":
            assert g.ncy > g.ncx, k
        if name == "deep":
            assert g.nz >= 94, k
    assert any(g.ncx != g.ncy for g in grids.values())


@pytest.mark.parametrize("kernel", ["IB_4", "IB_4_W8", "PIECEWISE_CONSTANT"])
@pytest.mark.parametrize("kind", ["uniform", "cluster"])
def test_inputs_leave_the_spread_tolerance_room(kind, kernel):
    """The oracle's side spread in list order and in reversed list order agree within a
    quarter of the spread tolerance, relative to the largest value: the inputs themselves
    leave a kernel's summation order three quarters of its room."""
    ora.lib()
    cs = c3.case("wide", kind, kernel)
    g = cs.geom
    gcw = [g.g] * 3
    out = []
    for sl in (slice(None), slice(None, None, -1)):
        u = [np.zeros(ora.side_ghost_shape(g.ilower, g.iupper, g.g, a)) for a in range(3)]
        ora.side_spread(kernel, g.dx, g.x_lower, g.ilower, g.iupper, gcw, u, cs.idx[sl], cs.xshift[sl], cs.X, cs.F)
        out.append(u)
    for a in range(3):
        scale = np.abs(out[0][a]).max()
        assert scale > 0
        err = np.abs(out[0][a] - out[1][a]).max() / scale
        print(f"wide {kind} {kernel} comp {a}: forward vs reversed {err:.3e}")
        assert err <= 0.25 * SPREAD_TOL


@pytest.mark.parametrize("kernel", c3.ALL)
def test_old_input_repeats_no_loop(kernel):
    """make_case(k, 3, ...), the input of every earlier all-kernel 3-D test: at most two
    real columns in x (none with eight real neighbours), no (column, anchor) beyond one
    chunk of candidates, no group of four planes beyond one chunk per wave."""
    parity = pytest.importorskip("test_gpu_parity")
    geom, X, idx, xs, depth = parity.make_case(kernel, 3, "side", seed=1)
    g = c3.plain_geometry(kernel, geom.ilower, geom.iupper, geom.gcw[0], geom.dx, geom.x_lower)
    st = c3.structure(g, X, idx, xs)
    assert st.real[0] <= 2 and not st.interior
    assert st.cand.max() <= c3.CHUNK
    assert max(p.max() for p in st.pool) <= c3.IWAVES * c3.CHUNK
    assert not st.inner_column


@pytest.mark.parametrize("kernel", c3.ALL)
def test_exact_keys_sit_within_a_cell_of_floor(kernel):
    """bucket_keys takes the key cell by the family's own anchor rule (the GPU test holds the
    library's order to it); structure takes it by floor.  The two differ by at most one
    cell, upwards, and only for the NINT-anchored kernels."""
    cs = c3.case("wide", "uniform", kernel)
    g = cs.geom
    key, rel, inside = c3.bucket_keys(g, cs.X, cs.idx, cs.xshift)
    st = c3.structure(g, cs.X, cs.idx, cs.xshift)
    assert abs(int(inside.sum()) - st.ninside) < 0.02 * st.ninside
    fl = np.floor((cs.X[cs.idx] + cs.xshift - np.array(g.x_lower)) / np.array(g.dx)).astype(np.int64)
    d = rel - (fl + np.array(g.ilower) - np.array(g.org))
    # (not the markers on exact half-cell positions: NINT sends a tie away from zero)
    near = (np.abs(fl) < 10**6).all(axis=1) & ~np.isin(cs.idx, np.arange(5, 10))
    assert set(np.unique(d[near])) <= ({0, 1} if c3.FAM[kernel] == 0 else {0})
    assert (key[inside] < g.nz * g.ncx * g.ncy * c3.NBAND).all() and (key >= 0).all()
    assert np.unique(key[inside] % c3.NBAND).size == (4 if kernel == "PIECEWISE_CONSTANT" else 9)

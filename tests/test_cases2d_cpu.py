"""The 2-D dense cases (tests/cases2d.py) reach the code they are built for.

tests/test_gpu_2d_dense.py runs the 2-D brick kernels at sizes where their loops repeat.
Whether they repeat is a property of the input, checked here without a GPU: the
neighbourhood walk of k_cand takes several sub-passes, a candidate class several chunks,
an interp item several passes of its markers, the items do not fill whole rounds, and the
tile grid is not square.  The old 2-D input, make_case's 29x30 patch, meets none of the
first three, which is the gap the dense cases close.
"""
import numpy as np
import pytest

import cases2d as c2
from oracle import oracle as ora

SPREAD_TOL = 1e-12


def _id(v):
    return "-".join(str(x) for x in v)


def test_kernel_tables_match_the_oracle():
    for k in c2.ALL:
        assert c2.MIN_GHOST[k] == ora.min_ghost_width(k), k


@pytest.mark.parametrize("name", list(c2.GEOMS))
def test_tile_counts_for_every_kernel(name):
    """geometry() asserts the tile counts; at the minimum ghost width and one more."""
    for k in c2.ALL:
        for extra in (0, 1):
            g = c2.geometry(name, k, extra)
            assert g.nt[0] != g.nt[1]
            assert g.nbricks // 4 == {"wide": 12, "tall": 12, "big": 60}[name]


@pytest.mark.parametrize("case", c2.GPU_CASES, ids=_id)
def test_preconditions(case):
    name, kind, kernel, extra = case
    cs = c2.case(name, kind, kernel, extra)
    st = c2.structure(cs.geom, cs.X, cs.idx, cs.xshift)
    W = c2.KINFO[kernel][0]
    nbh, cls, items = int(st.neighbourhood.max()), int(st.classes.max()), int(st.interp_items.max())
    print(f"{_id(case)}: inside {st.ninside} of {cs.idx.size}, neighbourhood max {nbh}, class max {cls}, "
          f"interp item max {items} ({'2x2 bricks' if W <= 4 else 'one brick'}), spread items {st.n_spread_items}, "
          f"interp items {st.n_interp_items}")
    assert nbh > 2 * c2.SUBPASS, "k_cand: a neighbourhood of more than two sub-passes"
    assert cls > (30 if kind == "cluster" else 4) * c2.CHUNK, "k_spread: a class of several chunks"
    assert items > 2 * c2.BLOCK, "k_interp: an item of more than two passes"
    # the spread's items, and the interp's for the kernels that take 2x2 bricks (the wide
    # kernels' one-brick items are four times as many, a multiple of 8)
    assert st.n_spread_items % 8 != 0
    assert W > 4 or st.n_interp_items % 8 != 0
    assert cs.geom.nt[0] != cs.geom.nt[1]
    # several super-bricks hold work, and the candidate lists fit the library's buffer
    assert (st.classes.sum(axis=2) > 0).sum() >= 4
    assert int(st.classes.sum()) <= 4 * cs.idx.size


@pytest.mark.parametrize("kernel", ["IB_4", "PIECEWISE_CONSTANT"])
@pytest.mark.parametrize("kind", ["uniform", "cluster"])
def test_inputs_leave_the_spread_tolerance_room(kind, kernel):
    """The oracle's side spread in list order and in reversed list order agree within a
    quarter of the spread tolerance, relative to the largest value: the inputs themselves
    leave a kernel's summation order three quarters of its room."""
    ora.lib()
    cs = c2.case("wide", kind, kernel)
    g = cs.geom
    gcw = [g.g, g.g]
    out = []
    for sl in (slice(None), slice(None, None, -1)):
        u = [np.zeros(ora.side_ghost_shape(g.ilower, g.iupper, g.g, a)) for a in range(2)]
        ora.side_spread(kernel, g.dx, g.x_lower, g.ilower, g.iupper, gcw, u, cs.idx[sl], cs.xshift[sl], cs.X, cs.F)
        out.append(u)
    for a in range(2):
        scale = np.abs(out[0][a]).max()
        assert scale > 0
        err = np.abs(out[0][a] - out[1][a]).max() / scale
        print(f"wide {kind} {kernel} comp {a}: forward vs reversed {err:.3e}")
        assert err <= 0.25 * SPREAD_TOL


@pytest.mark.parametrize("kernel", c2.ALL)
def test_old_input_repeats_no_loop(kernel):
    """make_case(k, 2, ...), the input of every earlier 2-D test: one tile, no neighbourhood
    beyond one sub-pass, no class beyond one chunk, no interp item beyond one pass."""
    parity = pytest.importorskip("test_gpu_parity")
    geom, X, idx, xs, depth = parity.make_case(kernel, 2, "side", seed=1)
    g = c2.plain_geometry(kernel, geom.ilower, geom.iupper, geom.gcw[0], geom.dx, geom.x_lower)
    st = c2.structure(g, X, idx, xs)
    assert g.nt == (1, 1) and st.n_spread_items == 4
    assert st.neighbourhood.max() <= 2 * c2.SUBPASS and st.neighbourhood.max() <= c2.SUBPASS
    assert st.classes.max() <= 4 * c2.CHUNK
    assert st.interp_items.max() <= 2 * c2.BLOCK

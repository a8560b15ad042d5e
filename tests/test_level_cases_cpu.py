"""CPU: the preconditions of the level-shape cases (tests/level_cases.py), so that no GPU test
of tests/test_gpu_level_shapes.py can pass vacuously: every patch has entries of both kinds,
the periodic dims carry images, `narrow` names markers twice in one list, `many` reaches the
patches either side of the sweeps' LDS patch table, `ragged` has the extents that change the
per-patch tables, the per-patch oracle spreads on the ghost-box lists conserve sum F, the
numpy ghost fill reproduces a periodic field, and the spread bound is smaller than the effect
of one dropped list entry."""
import numpy as np
import pytest

import level_cases as lc

RAGGED_KERNELS = ("IB_4", "IB_6", "PIECEWISE_LINEAR")
TILES = [(k, f, h) for k in ("IB_4", "IB_6") for f in lc.TILES_FLAGS for h in (False, True)]
COLX, COLY, MIN_SEG_LEVEL, CS_PTAB = 32, 16, 32, 2048  # le_sweep.hip


def _both_kinds(c):
    ni, ng = np.diff(c.int_off), np.diff(c.gh_off)
    assert ni.min() >= 20, (c.name, ni)
    assert np.all(ng > ni), (c.name, ni, ng)
    for d in range(3):
        if c.periodic[d]:
            assert np.count_nonzero(c.gh_shift[:, d]) >= 20, f"{c.name}: no images in dim {d}"
        else:
            assert not c.gh_shift[:, d].any()
    # an interior entry is in its patch's ghost-box list, unshifted
    for q in range(0, c.npatch, max(1, c.npatch // 8)):
        idx, xs = c.ghost(q)
        assert np.isin(c.interior(q), idx[~xs.any(axis=1)]).all()


@pytest.mark.parametrize("kernel", RAGGED_KERNELS)
def test_ragged_lists(kernel):
    c = lc.case("ragged", kernel)
    assert 5500 <= c.M <= 6500
    _both_kinds(c)
    small = c.interior(lc.RAGGED_SMALL)
    assert np.count_nonzero(np.all(c.cells[small] == lc.RAGGED_DENSE_CELL, axis=1)) >= 150
    # the sheet crosses the face between patches 0 and 1: some of it interior to each
    sheet = np.arange(c.M)[lc.RAGGED_SHEET]
    for q in lc.RAGGED_FACE:
        assert np.isin(sheet, c.interior(q)).sum() >= 100


def test_ragged_extents():
    c = lc.case("ragged", "IB_6")  # the widest ghost layer
    n, lo, hi, g = c.n, c.lo, c.hi, c.g
    assert c.npatch == 6 and g == 4
    assert len(set(c.dx)) == 3 and all(np.log2(v) % 1 for v in c.dx) and c.x_lower.all()
    assert np.all(lo.min(0) < 0)
    # x extents on both sides of a 32-cell column, y extents over several 16-cell column rows
    assert n[:, 0].min() <= 9 and n[:, 0].max() >= 40
    assert n[:, 1].min() <= 10 and n[:, 1].max() >= 37 and (n[:, 1].max() - n[:, 1].min()) // COLY >= 1
    # z: one segment on some patch, at least two of >= 32 planes on another (the key planes of
    # a patch: its ghost box, a face, the stencil's reach)
    reach = 2 * g + 2 + ora_stencil(c.kernel)
    assert n[:, 2].max() >= 2 * MIN_SEG_LEVEL and n[:, 2].min() + reach < 2 * MIN_SEG_LEVEL
    assert tuple(n[lc.RAGGED_SMALL]) == (5, 4, 6)
    assert all(tuple(n[q]) != tuple(n[0]) for q in range(1, 6))
    assert len({tuple(v) for v in n}) == 6

    def gap(a, b):  # cells between the boxes per dim (negative: they overlap there), period in z
        d = np.maximum(lo[a] - hi[b], lo[b] - hi[a]) - 1
        dz = max(lo[a][2] + c.ext[2] - hi[b][2], lo[b][2] + c.ext[2] - hi[a][2]) - 1
        d[2] = min(d[2], dz) if d[2] >= 0 else d[2]
        return d

    for a in range(6):  # no two patches overlap
        for b in range(a + 1, 6):
            assert gap(a, b).max() >= 0, (a, b)
    f = gap(*lc.RAGGED_FACE)
    assert f[0] == 0 and f[1] < 0 and f[2] < 0, "face to face in x"
    f = gap(0, 5)
    assert f[2] == 0 and f[0] < 0 and f[1] < 0, "face to face in z"
    e = gap(*lc.RAGGED_EDGE)
    assert e[0] == 0 and e[1] == 0 and e[2] < 0, "an edge only"
    assert all(gap(lc.RAGGED_FAR, b).max() > 2 * g for b in range(6) if b != lc.RAGGED_FAR)


def ora_stencil(kernel):
    from oracle import oracle as ora
    return ora.STENCIL[kernel]


@pytest.mark.parametrize("kernel,periodic,holes", TILES)
def test_tiles_lists(kernel, periodic, holes):
    c = lc.case("tiles", kernel, periodic, holes)
    assert c.npatch == (22 if holes else 24)
    assert len(set(c.ntile)) == 3 and len(set(c.tile_n)) == 3
    W = ora_stencil(kernel)
    assert c.tile_n[0] >= COLX + W - 1 and c.tile_n[1] >= COLY + W - 1, "the fused fill_interp's patch size"
    assert tuple(c.dom_lo) == lc.TILES_DOM_LO
    _both_kinds(c)
    if holes:  # the bounding box is still the domain
        assert np.array_equal(c.lo.min(0), c.dom_lo) and np.array_equal(c.hi.max(0), c.dom_hi)


def test_narrow_names_markers_twice():
    c = lc.case("narrow")
    _both_kinds(c)
    assert np.all(c.n[:, 2] == c.ext[2]) and c.ext[2] <= c.n[0, 2] + 2 + 2 * c.g  # select_interior's need_shift
    for q in range(c.npatch):
        idx, xs = c.ghost(q)
        u, cnt = np.unique(idx, return_counts=True)
        twice = u[cnt == 2]
        assert cnt.max() == 2 and twice.size >= 20
        assert np.isin(twice, c.interior(q)).sum() >= 20  # doubled and interior: the unshifted entry is Q's


def test_many_reaches_past_the_lds_table():
    c = lc.case("many")
    assert c.npatch == 2197 > CS_PTAB and c.g == 3 and 5500 <= c.M <= 6500
    for q in lc.MANY_SAMPLE_FIXED:
        assert c.interior(q).size >= 5 and c.ghost(q)[0].size > c.interior(q).size
    assert np.array_equal(np.sort(c.int_idx), np.arange(c.M)), "every marker interior to one patch"
    s = lc.many_sample(c)
    assert len(s) == 64 and set(lc.MANY_SAMPLE_FIXED) <= set(s)
    for d in range(3):
        assert np.count_nonzero(c.gh_shift[:, d]) >= 20


def test_tiles_oracle_spreads_conserve_sum_F():
    """all tiles, fully periodic: the per-patch spreads on the ghost-box lists, summed over the
    patches' own points, are the periodic spread (as test_gpu_level.py)"""
    c = lc.case("tiles", "IB_4", (1, 1, 1), False)
    g, n = c.g, c.tile_n
    tot = np.zeros(3)
    for q in range(c.npatch):
        f, _, _ = c.spread_ref(q, "side")
        for a in range(3):
            tot[a] += f[a][g:g + n[2], g:g + n[1], g:g + n[0]].sum()
    h3 = float(np.prod(c.dx))
    for a in range(3):
        assert abs(tot[a] * h3 - c.F[:, a].sum()) <= 1e-10 * np.abs(c.F[:, a]).sum()


@pytest.mark.parametrize("periodic,holes", [(f, h) for f in lc.TILES_FLAGS for h in (False, True)])
@pytest.mark.parametrize("centering,depth", [("side", 1), ("cell", 2)])
def test_fill_reference(centering, depth, periodic, holes):
    c = lc.case("tiles", "IB_4", periodic, holes)
    G = lc.fill_fields(c, centering, depth, 3)
    rng = np.random.default_rng(4)
    kept = filled = 0
    for q in range(c.npatch):
        before, after, sup = lc.fill_arrays(c, q, centering, depth, G, rng)
        for a in range(len(G)):
            assert after[a].shape == c.array_shape(q, centering, a, depth)
            ghost, supplied, src = lc.fill_sources(c, q, centering, a)
            assert np.array_equal(after[a][..., ~ghost], before[a][..., ~ghost]), "own points unchanged"
            kept += np.count_nonzero(ghost & ~supplied)
            filled += np.count_nonzero(supplied)
            if all(periodic) and not holes:  # the periodic field at every point
                assert supplied[ghost].all()
                N = c.ext
                idx = [(np.arange(after[a].shape[-1 - d]) + c.lo[q, d] - c.g - c.dom_lo[d]) % N[d] for d in range(3)]
                want = G[a][(slice(None),) + np.ix_(idx[2], idx[1], idx[0])]
                assert np.array_equal(after[a], want[0] if centering == "side" else want)
    assert filled > 0 and (kept > 0) == (holes or not all(periodic))


DROPS = [("ragged", "IB_4", None, False), ("ragged", "PIECEWISE_LINEAR", None, False),
         ("tiles", "IB_4", (1, 0, 1), True), ("narrow", "IB_4", None, False), ("many", "IB_4", None, False)]


@pytest.mark.parametrize("name,kernel,periodic,holes", DROPS)
def test_bound_is_below_one_dropped_entry(name, kernel, periodic, holes):
    """Three entries per case, each taken out of its patch's ghost-box list: the oracle's
    spread changes at some point by more than that point's bound."""
    c = lc.case(name, kernel, periodic, holes)
    patches = {"ragged": (0, lc.RAGGED_SMALL, 5), "many": (0, 2048, 2196)}.get(name, (0, c.npatch // 2, c.npatch - 1))
    for q in patches:
        idx, xs = c.ghost(q)
        f, S, n_q = c.spread_ref(q, "side")
        k = {patches[0]: 0, patches[1]: n_q // 2, patches[2]: n_q - 1}[q]
        keep = np.arange(n_q) != k
        f2 = c.alloc(q, "side")
        c.oracle("spread", q, "side", f2, idx[keep], xs[keep], c.F)
        assert lc.spread_ratio(kernel, f2, f, S, n_q) > 1.0, (q, k)
        assert lc.spread_ratio(kernel, f, f, S, n_q) == 0.0

"""The handle-reuse cases (tests/reuse_cases.py) can tell a reused handle from a fresh one.

tests/test_gpu_reuse.py compares a handle that has been binned many times with a fresh one.
That comparison is empty if two consecutive states give the same answer, if the duplicates of
the `dups` list agree, or if the two 3-D patches have the same bucket count: a handle that
silently kept its previous state would pass.  Asserted here on the inputs alone, with numpy
and the C oracle, without a GPU.
"""
import numpy as np
import pytest

import cases3d as c3
import reuse_cases as rc

SEQ_KERNELS = {name: sorted({st.kernel for st in rc.states(seq)}) for name, seq in rc.SEQUENCES.items()}


def test_shapes():
    """A3 has 2 x 2 real columns at least for every kernel, B3 another column, plane and
    bucket count (make_col_geom's, restated by cases3d.plain_geometry); the lists' lengths lie
    outside DevBuf::ensure's 12.5 % slack of one another."""
    for k in rc.KERNELS:
        a, b = rc.col_geom("A3", k), rc.col_geom("B3", k)
        assert a.ncx - 2 >= 2 and a.ncy - 2 >= 2, k
        assert (a.ncx * a.ncy, a.nz) != (b.ncx * b.ncy, b.nz) and a.ncx * a.ncy != b.ncx * b.ncy and a.nz != b.nz, k
        assert rc.nbuckets("A3", k) != rc.nbuckets("B3", k), k
        assert rc.G >= c3.MIN_GHOST[k]
    assert rc.patch("A3").N == (40, 24, 20) and rc.patch("A3").ilower == (-3, 5, 2) and len(set(rc.patch("A3").dx)) == 3
    assert rc.patch("B3").N == (72, 40, 12) and rc.patch("A2").N == (40, 24)
    assert 8 * rc.N_SMALL < rc.M and rc.N_DUPS * 1.125 + 256 < rc.M and rc.N_COUNTED < rc.M
    assert rc.M == 6000 and rc.N_SMALL == 700 and rc.N_DUPS == 3000 and rc.N_COUNTED == 4500


@pytest.mark.parametrize("geom", ["A3", "B3", "A2"])
def test_movers(geom):
    """X_moved changes the anchor cell of 500 entries at least under every kernel's rule;
    X_within changes no cell under NINT (the kernels of the re-binning sequence) and the
    shifted-z anchor of 100 entries at least."""
    p, pos = rc.patch(geom), rc.positions(geom)
    for k in rc.KERNELS:
        a0, z0 = rc.anchors(k, p, pos["X0"])
        a1, _ = rc.anchors(k, p, pos["X_moved"])
        moved = int(np.any(a0 != a1, axis=1).sum())
        assert moved >= 500, (geom, k, moved)
        if p.ndim == 3 and c3.FAM[k] == 0:
            a2, z2 = rc.anchors(k, p, pos["X_within"])
            assert np.array_equal(a0, a2), (geom, k)
            assert int((z0 != z2).sum()) >= 100, (geom, k)
            g = rc.col_geom(geom, k)
            idx, xs = rc.entries(geom, "big")
            k0, k2 = c3.bucket_keys(g, pos["X0"], idx, xs)[0], c3.bucket_keys(g, pos["X_within"], idx, xs)[0]
            assert np.array_equal(k0, k2), "X_within changes a bucket"
            km = c3.bucket_keys(g, pos["X_moved"], idx, xs)[0]
            assert int((k0 != km).sum()) >= 500


@pytest.mark.parametrize("geom", ["A3", "B3", "A2"])
def test_dups(geom):
    """200 markers at least are named twice, with different shifts, and the oracle's interp
    from a marker's last entry differs from the one from its first."""
    p = rc.patch(geom)
    idx, xs = rc.dup_list(geom)
    assert idx.size == rc.N_DUPS and xs.shape == (rc.N_DUPS, p.ndim)
    order = np.argsort(idx, kind="stable")
    s = idx[order]
    twice = np.nonzero(s[1:] == s[:-1])[0]
    assert twice.size >= 200 and np.bincount(idx).max() == 2
    first, last = order[twice], order[twice + 1]
    assert np.all(np.any(xs[first] != xs[last], axis=1))
    st = rc.State(geom, "IB_4", "dups", "X0", 0)
    u, X = rc.fields(geom, "side"), rc.state_X(st)
    Qf, Ql = np.zeros((rc.M, p.ndim)), np.zeros((rc.M, p.ndim))
    from oracle import oracle as ora
    ora.side_interp(*rc._args(st), u, idx[first], xs[first], X, Qf)
    ora.side_interp(*rc._args(st), u, idx[last], xs[last], X, Ql)
    assert np.all(np.any(Qf[s[twice]] != Ql[s[twice]], axis=1))
    Q, named = rc.oracle_interp(st)
    assert np.array_equal(Q[s[twice]], Ql[s[twice]]) and named.sum() == rc.N_DUPS - twice.size


def _differ(a, b):
    """the fraction of the entries nonzero in either list of arrays that differ"""
    if any(x.shape != y.shape for x, y in zip(a, b)):
        return 1.0
    ne = nz = 0
    for x, y in zip(a, b):
        m = (x != 0) | (y != 0)
        nz += int(m.sum())
        ne += int((x != y)[m].sum())
    return ne / nz if nz else 0.0


def _interp_differ(a, b):
    (Qa, na), (Qb, nb) = a, b
    if Qa.shape != Qb.shape:
        return 1.0
    rows = na | nb
    return float((np.any(Qa != Qb, axis=1) | (na != nb))[rows].mean()) if rows.any() else 0.0


@pytest.mark.parametrize("name", list(rc.SEQUENCES), ids=str)
def test_consecutive_states_differ(name):
    """Every pair of consecutive states differs in more than half of the nonzero entries of
    the oracle's spread and of its interp -- where the pair differs in more than F (a repeated
    re-binning at the same positions, there on purpose, differs through F: the spread alone);
    every spread of a non-empty list is nonzero in every component."""
    sts = rc.states(rc.SEQUENCES[name])
    assert len(sts) >= 2
    for prev, cur in zip([None] + sts[:-1], sts):
        f = rc.oracle_spread_listed(cur)
        if rc.entries(cur.geom, cur.lst)[0].size:
            assert all(np.abs(a).max() > 0 for a in f), cur
            assert all(np.abs(c).max() > 0 for c in rc.oracle_interp(cur)[0].T), cur
        if prev is None or not (rc.entries(prev.geom, prev.lst)[0].size or rc.entries(cur.geom, cur.lst)[0].size):
            continue  # (a re-binning of an empty list: nothing before or after it)
        assert _differ(rc.oracle_spread_listed(prev), f) > 0.5, (prev, cur)
        if prev[:4] != cur[:4]:
            assert _interp_differ(rc.oracle_interp(prev), rc.oracle_interp(cur)) > 0.5, (prev, cur)
    for s in rc.SEQUENCES[name]:
        for x in s.extra:
            centering, depth = rc.EXTRA[x]
            st = sts[rc.SEQUENCES[name].index(s)]
            assert all(np.abs(a).max() > 0 for a in rc.oracle_spread_listed(st, centering, depth))


def test_sequences_cover_the_issue():
    s = rc.SEQUENCES
    assert [st.lst for st in rc.states(s["grow_shrink"])[::2]] == ["small", "big", "small"]
    assert [st.kernel for st in rc.states(s["kernels"])] == ["IB_4", "PIECEWISE_LINEAR", "IB_6", "IB_4"]
    assert len({c3.FAM[k] for k in SEQ_KERNELS["kernels"]}) == 2 and \
        len({c3.KINFO[k][1:] for k in SEQ_KERNELS["kernels"]}) == 3
    assert [st.geom for st in rc.states(s["geometries"])[::2]] == ["A3", "B3", "A3"]
    for k in ("dimensions-IB_4-big", "dimensions-IB_3-big", "dimensions-IB_4-dups"):
        assert [st.geom for st in rc.states(s[k])[::2]] == ["A3", "A2", "A3"]
        assert all(step.op == "rebin" for step in s[k][1::2])
    assert [st.lst for st in rc.states(s["list_kinds"])] == ["big", "dups", "big", "counted", "counted", "big"]
    assert [st.lst for st in rc.states(s["empty"])] == ["big", "empty", "big", "counted0", "counted0", "big"]
    for k in ("rebin_states-IB_4", "rebin_states-BSPLINE_4"):
        assert [step.op for step in s[k]] == ["bin"] + ["rebin"] * 8 + ["bin", "rebin", "bin", "rebin"]
        assert [st.X for st in rc.states(s[k])] == (["X0"] * 3 + ["X_moved"] * 2 + ["X_within"] * 2 + ["X0"] * 2 +
                                                     ["X_moved", "X_within", "X0", "X_within"])


def test_levels():
    """LA and LB: four patches each, one dx, other boxes (so the patch table of the one is
    copied into the other's, le_abi.cpp's `prev[q].comp`); LC eight; every level's M markers,
    500 of which change their cell under X_moved; consecutive level states differ."""
    la, lb, lcc = rc.level("LA"), rc.level("LB"), rc.level("LC")
    assert la.npatch == lb.npatch == 4 and lcc.npatch == 8
    assert np.array_equal(la.dx, lb.dx) and np.array_equal(la.dx, lcc.dx)
    assert not np.array_equal(la.lo, lb.lo) and not np.array_equal(la.n, lb.n)
    assert len({tuple(v) for v in la.n}) == 1 and len({tuple(v) for v in lb.n}) == 4
    F0, F1 = rc.lag_values(0, 3), rc.lag_values(1, 3)
    seen = []
    for c in (la, lb, lcc):
        assert c.M == rc.M and c.gh_idx.size > rc.M * 0.9
        assert all(c.interior(q).size > 20 and c.ghost(q)[0].size > c.interior(q).size for q in range(c.npatch))
        cells = np.floor((c.X_moved - c.x_lower) / c.dx)
        assert int(np.any(cells != np.floor((c.X - c.x_lower) / c.dx), axis=1).sum()) >= 500
        (Q0, f0), (Q1, f1) = rc.level_oracle(c, "X0", F0), rc.level_oracle(c, "X_moved", F1)
        for q in range(c.npatch):
            assert all(np.abs(a).max() > 0 for a in f0[q])
            assert _differ(f0[q], f1[q]) > 0.5
        named = np.zeros(rc.M, bool)
        named[c.int_idx] = True
        assert np.any(Q0 != Q1, axis=1)[named].mean() > 0.5
        gi, gx, go, ii, io = rc.relisted(c)
        assert len(go) == c.npatch + 1 and go[-1] < c.gh_idx.size and io[-1] > 100 and gi.size == go[-1]
        seen.append((Q0, f0))
    # LA -> LB -> LA on one handle: the two levels' results are not each other's
    assert np.any(seen[0][0] != seen[1][0], axis=1).mean() > 0.5
    assert any(a.shape != b.shape for a, b in zip(seen[0][1][0], seen[1][1][0]))

"""The plane-window cases (tests/window_cases.py) reach both halves of a windowed call.

tests/test_gpu_plane_window.py holds the inner and outer halves of the 3-D sweeps to their
contract.  That only bites if both halves have work, if a window face falls inside a sweep
segment (so that an uncut item straddles it and a cut one is really cut), and if the heavy
item of the cluster case reaches across the face; all of that is a property of the inputs,
checked here without a GPU.
"""
import numpy as np
import pytest

import cases3d as c3
import window_cases as wc


@pytest.mark.parametrize("kernel", c3.ALL)
def test_both_halves_have_markers(kernel):
    cs = wc.marker_deep(kernel)
    A, inside = wc.entries(cs)
    assert cs.X.shape[0] == wc.DEEP_M and inside.sum() > 0.5 * cs.idx.size and (~inside).sum() > 1000
    for name, win in wc.windows(cs.geom).items():
        inner = wc.inner_anchor(cs.geom, win, A) & inside
        nin, nout = int(inner.sum()), int((inside & ~inner).sum())
        print(f"{kernel} {name} {win}: {nin} inner, {nout} outer anchors, cuts {wc.cuts(cs.geom, win)}")
        if name == "all":
            assert nout == 0
        elif name == "none":
            assert nin == 0 and wc.cuts(cs.geom, win) == []
        else:
            assert nin >= 1000 and nout >= 1000, (name, nin, nout)


@pytest.mark.parametrize("kernel", c3.ALL)
def test_windows_and_cuts(kernel):
    """The windows' planes against the arrays: `low` and `high` reach the arrays' first and
    last plane (their outer cuts clamp away), `thin` is Slab's minimum, and with the default
    segments and with one segment a face of every real window lies strictly inside a segment."""
    g = c3.geometry("deep", kernel)
    W, LO, HI = c3.KINFO[kernel]
    w = wc.windows(g)
    first, last = g.ilower[2] - g.g, g.iupper[2] + g.g + 1  # the z faces' array has the extra plane
    assert g.ilower[2] == 5 and g.N[2] == 90
    assert w["low"][0] == first and w["high"][1] == last
    assert w["all"][0] < first - W and w["all"][1] > last + W and wc.cuts(g, w["all"]) == []
    assert w["thin"][1] - w["thin"][0] + 1 == 2 * g.g + 2 > HI - LO
    assert w["interior"] == (g.ilower[2], g.iupper[2])
    assert g.org[2] + g.nz - 1 + LO == last, "the last anchor plane reaches the last array plane"
    for name in wc.REAL:
        c = wc.cuts(g, w[name])
        assert 2 <= len(c) <= 4, (name, c)
        assert len(c) == 4 or name in ("low", "high") or LO == 0
        lo, hi = wc.plane_slice(g, w[name], last - first + 1)
        assert 0 <= lo < hi <= last - first + 1 and (lo > 0 or hi < last - first + 1)
        for seg_items in (0, 1):
            assert wc.faces_inside_segments(g, w[name], seg_items), (name, seg_items, c3.segments(g, seg_items))
    assert c3.segments(g, 1) == (g.nz, 1)


@pytest.mark.parametrize("kernel", c3.ALL)
def test_shifted_windows_meet_every_segment_position(kernel):
    """Over `middle` and its shifts a default segment boundary falls one anchor short of, at
    and one past each of the four anchors where the `inner` rules switch; each shifted window
    has markers on both sides."""
    cs = wc.marker_deep(kernel)
    g = cs.geom
    S, nseg = c3.segments(g)
    wins = [wc.windows(g)["middle"]] + wc.shifted(g)
    assert len(wins) == S and nseg > 8
    W, LO, HI = c3.KINFO[kernel]
    for bound in range(4):
        for off in (-1, 0, 1):
            at = []
            for zlo, zhi in wins:
                lo, hi = zlo - g.org[2], zhi - g.org[2]
                c = (lo - LO, lo, hi - HI + 1, hi + 1)[bound] + off
                at.append(0 < c < g.nz and c % S == 0)
            assert any(at), (bound, off)
    A, inside = wc.entries(cs)
    for win in wins:
        inner = wc.inner_anchor(g, win, A) & inside
        assert inner.sum() >= 1000 and (inside & ~inner).sum() >= 1000


@pytest.mark.parametrize("kernel", c3.PATHS)
def test_cluster_straddles_the_face(kernel):
    """The cluster's anchor plane is 15 and its stencil planes lie on both sides of plane 16's
    lower face; neither cluster window gives the cluster's anchor to the inner half, and a
    cut of each falls on or next to the cluster's plane inside its segment."""
    cs = c3.case("wide", "cluster", kernel)
    g = cs.geom
    W, LO, HI = c3.KINFO[kernel]
    A, inside = wc.entries(cs)
    cl = np.arange(8000, 12000)  # the cluster's rows (the list is the identity)
    # the 2 000 at one point are anchored in plane 15; of those spread over the cell the
    # kernels that key by NINT(x) anchor the upper half in plane 16
    assert inside[cl].all() and (A[cl[:2000]] == 15).all() and c3.cluster_cell(g)[2] == 15
    assert set(np.unique(A[cl])) <= ({15, 16} if c3.FAM[kernel] == 0 else {15})
    assert 15 + LO <= 15 and 15 + HI >= 16
    S, _ = c3.segments(g)
    a = 15 - g.org[2]
    through = []
    for win in wc.CLUSTER_WINDOWS:
        assert not wc.inner_anchor(g, win, A[cl]).any(), "the whole cluster is the outer half's"
        inner = wc.inner_anchor(g, win, A) & inside
        assert inner.sum() >= 300 and (inside & ~inner).sum() >= 4000, "both halves have markers"
        seg = a // S
        through += [c for c in wc.cuts(g, win) if seg * S < c < (seg + 1) * S]
    # (a face can coincide with a segment boundary: IB_4's plane 16 is one)
    assert through, "a cut of one of the windows goes through the cluster's (column, segment)"

"""GPU: the two halves of a 3-D sweep under a plane window (Context.set_plane_window).

SlabExchange.halo_fill runs the interp's inner items (mode 1) while the neighbours' z planes
are still in flight and ghost_sum the spread's inner items while this rank's ghost planes are
being sent.  That is only correct if a mode-1 interp item reads no plane outside the window,
a mode-1 spread item writes none, and the mode-2 spread alone completes every plane outside
it.  Until now only the end result of one multi-process configuration was compared.  Here
the halves are held to the contract stated in tests/window_cases.py, in one process, bit for
bit against the unrestricted (mode 0) result of the same Markers object, for every kernel
and centering, for item tables cut at the window's faces (window set before Markers.bin) and
uncut (set afterwards), with the default segments and with one segment that all four cuts
fall into; the mode-0 results themselves are held to the oracle.

List entries outside the column grid are not swept by any item: a kernel of their own
writes their 0 in every mode, so the halves partition the entries inside the grid and both
write the others' zeros.

Every function ends with ctx.synchronize(), which raises on the device invariant flags.
"""
import numpy as np
import pytest

import cases3d as c3
import window_cases as wc

torch = pytest.importorskip("torch")

from test_gpu_3d_dense import (DEPTH, DEV, check_interp, dev_geom, gpu_interp, marker_values,  # noqa: E402
                               oracle_interp, q_depth_of, random_arrays)
from test_gpu_fused import _fill  # noqa: E402
from test_gpu_parity import SPREAD_TOL, oracle_call  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -3.0e33  # a finite value no interpolation gives: an entry that still holds it was not written


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


def bits(t):
    return t.contiguous().view(torch.int64)


def same(a, b):
    """Bit for bit (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_where(a, b, mask):
    return bool(((bits(a) == bits(b)) | ~mask).all())


def to_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


class Case:
    """A marker set on the device with the per-marker sets the checks need."""

    def __init__(self, cs):
        self.cs = cs
        self.Xd, self.idd, self.xsd = to_dev(cs.X, cs.idx, cs.xshift)
        self.A, self.inside = wc.entries(cs)
        listed = np.zeros(cs.X.shape[0], bool)
        listed[cs.idx] = True
        self.listed = to_dev(listed)[0]

    def sets(self, win):
        return to_dev(*wc.marker_sets(self.cs, win))


def plane_masks(geom, win, arrays):
    """Per array: a (planes, 1, 1) bool mask of the window's planes."""
    out = []
    for a in arrays:
        nz = a.shape[-3]
        i0, i1 = wc.plane_slice(geom, win, nz)
        mk = torch.zeros(nz, dtype=torch.bool, device=DEV)
        mk[i0:i1] = True
        out.append(mk.view(-1, 1, 1))
    return out


def interp_modes(le, ctx, m, kernel, cen, geom, q, depth, Xd, win, modes=(0, 1, 2), periodic=None):
    """Q, started at SENT, of one interp call per mode; the context is left in mode 0."""
    out = []
    for mode in modes:
        Q = torch.full((Xd.shape[0], q_depth_of(cen, depth)), SENT, dtype=torch.float64, device=DEV)
        ctx.set_plane_window(mode, *win)
        if periodic is None:
            le.interp(ctx, m, kernel, cen, geom, q, Q, Xd, q_depth=depth)
        else:
            le.fill_interp(ctx, m, kernel, cen, geom, q, Q, Xd, q_depth=depth, periodic=periodic)
        out.append(Q)
    ctx.set_plane_window(0, *win)
    return out


def check_partition(case, Q0, Q1, Q2, win, name, cut, what):
    """Property 1: the halves partition the swept entries of mode 0, with its bits."""
    ingrid, inner = case.sets(win)
    listed = case.listed
    sent = bits(torch.tensor([SENT], dtype=torch.float64, device=DEV))[0]
    w = [bits(Q) != sent for Q in (Q0, Q1, Q2)]
    for wk in w:  # all components of a marker come from the same half
        assert torch.equal(wk.all(dim=1), wk.any(dim=1)), f"{what}: a marker's components are split"
    r0, r1, r2 = (wk.all(dim=1) for wk in w)
    assert torch.equal(r0, listed), f"{what}: mode 0 writes the listed markers"
    assert not (r1 & ~listed).any() and not (r2 & ~listed).any(), f"{what}: an unlisted marker was written"
    assert torch.isfinite(Q0).all()
    outside = listed & ~ingrid  # not swept: 0 from every mode
    assert outside.sum() > 1000
    for Q, r in ((Q0, r0), (Q1, r1), (Q2, r2)):
        assert r[outside].all() and (Q[outside] == 0.0).all(), f"{what}: entries outside the grid read 0"
    both, none = r1 & r2 & ingrid, ~r1 & ~r2 & ingrid
    assert not both.any(), f"{what}: {int(both.sum())} entries written by both halves"
    assert not none.any(), f"{what}: {int(none.sum())} entries written by neither half"
    assert torch.equal(bits(Q1)[r1], bits(Q0)[r1]), f"{what}: mode 1 differs from mode 0"
    assert torch.equal(bits(Q2)[r2], bits(Q0)[r2]), f"{what}: mode 2 differs from mode 0"
    got = r1 & ingrid
    if cut:
        bad = got != inner
        assert not bad.any(), f"{what}: {int(bad.sum())} entries on the wrong side of a cut table"
    else:
        assert not (got & ~inner).any(), f"{what}: the inner half took an anchor that reads outside the window"
    if name == "all":
        assert torch.equal(got, ingrid), f"{what}: the outer half must do nothing"
    if name == "none":
        assert not got.any(), f"{what}: the inner half must do nothing"
    if cut and name in wc.REAL:
        assert got.sum() >= 300 and (ingrid & ~got).sum() >= 1000
    return int(got.sum())


def nan_outside(q, masks):
    return [torch.where(mk, a, torch.full_like(a, np.nan)) for a, mk in zip(q, masks)]


def check_interp_window(le, ctx, m, case, kernel, cen, geom, q, depth, win, name, cut, what, Qref=None,
                        periodic=None):
    """Properties 1 and 2 of one window; returns the mode-0 result."""
    Xd = case.Xd
    Q0, Q1, Q2 = interp_modes(le, ctx, m, kernel, cen, geom, q, depth, Xd, win, periodic=periodic)
    if Qref is not None:
        assert same(Q0, Qref), f"{what}: mode 0 differs between item tables"
    check_partition(case, Q0, Q1, Q2, win, name, cut, what)
    # locality: every plane outside the window NaN; the inner half reads none of them
    qn = nan_outside(q, plane_masks(case.cs.geom, win, q))
    (Q1n,) = interp_modes(le, ctx, m, kernel, cen, geom, qn, depth, Xd, win, modes=(1,), periodic=periodic)
    assert not torch.isnan(Q1n).any(), f"{what}: the inner half read a plane outside the window"
    assert same(Q1n, Q1), f"{what}: the inner half depends on planes outside the window"
    return Q0


def spread_modes(le, ctx, m, kernel, cen, geom, f0, Fd, Xd, depth, win, modes, call="spread"):
    f = [a.clone() for a in f0]
    fn = getattr(le, call)
    for mode in modes:
        ctx.set_plane_window(mode, *win)
        fn(ctx, m, kernel, cen, geom, f, Fd, Xd, q_depth=depth)
    ctx.set_plane_window(0, *win)
    return f


def check_spread_window(le, ctx, m, case, kernel, cen, geom, f0, Fd, depth, win, name, cut, what):
    """Property 3 of one window; returns the mode-0 result."""
    args = (le, ctx, m, kernel, cen, geom, f0, Fd, case.Xd, depth, win)
    R21 = spread_modes(*args, (2, 1))  # ghost_sum's order, first on a fresh binning
    R0, R1, R2, R12 = (spread_modes(*args, md) for md in ((0,), (1,), (2,), (1, 2)))
    masks = plane_masks(case.cs.geom, win, f0)
    for c, mk in enumerate(masks):
        w = f"{what} comp {c}"
        out = ~mk
        assert same_where(R1[c], f0[c], out), f"{w}: the inner half wrote a plane outside the window"
        assert same_where(R2[c], R0[c], out), f"{w}: the outer half alone does not complete the planes outside"
        assert same(R21[c], R0[c]), f"{w}: outer then inner differs from one call"
        assert same(R12[c], R0[c]), f"{w}: inner then outer differs from one call"
        if cut:
            assert same_where(R1[c], R0[c], mk), f"{w}: the inner half alone does not complete the window's planes"
            assert same_where(R2[c], f0[c], mk), f"{w}: the outer half wrote a plane inside the window"
        changed = bits(R0[c]) != bits(f0[c])
        if name in wc.REAL or name is None:
            assert (changed & mk).any() and (changed & out).any(), f"{w}: the spread reaches both sides"
        if name == "all":
            assert same(R2[c], f0[c]), f"{w}: the outer half must do nothing"
        if name == "none":
            assert same(R1[c], f0[c]), f"{w}: the inner half must do nothing"
    return R0


def oracle_spread_dev(oracle, order, u0, kernel, cen, geom, cs, Fv, depth):
    """The oracle's spread of Fv into u0 in the binned order, on the device."""
    uo = [a.copy() for a in u0]
    oracle_call(oracle, "spread", kernel, cen, geom, uo, cs.idx[order], cs.xshift[order], cs.X, Fv.copy(), depth)
    return to_dev(*uo)


def rel_err_dev(a, b):
    return float((a - b).abs().max() / b.abs().max())


def window_table(le, ctx, case, kernel, geom, win, cut):
    """A binning whose item table is cut at `win`'s faces, or not; the context in mode 0."""
    if cut:
        ctx.set_plane_window(0, *win)
    else:
        ctx.set_plane_window(0)
    return le.Markers(ctx).bin(geom, kernel, case.Xd, case.idd, case.xsd)


# --------------------------------------------------------------------------
# 1, 2, 3: every kernel and centering, every window, cut and uncut, two segment settings
# --------------------------------------------------------------------------
CASES = [(k, "side") for k in c3.ALL] + [(k, c) for c in ("cell", "node", "edge") for k in c3.PATHS]


@pytest.mark.parametrize("kernel,centering", CASES, ids=lambda v: str(v))
def test_halves(le, oracle, kernel, centering):
    """Interp partition and locality, spread halves (the module docstring's three conditions)
    for the seven windows of window_cases on `deep`; the mode-0 interp is the oracle's bit for
    bit and the cut tables' mode-0 side spread within 1e-12 of the oracle in the binned order.
    On the uncut table with the default segments also `middle` shifted plane by plane through
    a segment's length: a cut table fits its window, so only there does an item end one plane
    short of, at or one past a bound of the rule -- where a bound that is off by one shows."""
    case = Case(wc.marker_deep(kernel))
    cs = case.cs
    geom = dev_geom(le, cs.geom)
    depth = DEPTH[centering]
    wins = wc.windows(cs.geom)
    q, u0 = random_arrays(geom, centering, depth, 21)
    f0, f0n = random_arrays(geom, centering, depth, 22)
    Fv = marker_values(cs.F, centering, depth)
    Fd = to_dev(Fv)[0]
    Qref = order0 = uo = None
    worst = 0.0
    for seg_items in (None, 1):
        ctx = le.Context(0)
        if seg_items is not None:
            ctx.tune("seg_items", seg_items)
        for cut in (True, False):
            m = None
            todo = [(name, wins[name]) for name in wc.NAMES]
            if not cut and seg_items is None:  # every position of a face within the fixed segments
                todo += [(None, win) for win in wc.shifted(cs.geom)]
            for name, win in todo:
                what = f"{kernel} {centering} seg_items={seg_items} {'cut' if cut else 'uncut'} {name}{win}"
                if cut or m is None:
                    m = window_table(le, ctx, case, kernel, geom, win, cut)
                    if order0 is None:
                        order0 = m.order()
                        Qn = gpu_interp(le, ctx, m, kernel, centering, geom, q, depth, case.Xd)
                        ctx.synchronize()
                        check_interp(Qn.cpu().numpy(), oracle_interp(oracle, kernel, centering, geom, u0, cs, depth),
                                     cs, kernel, centering, what)
                        Qref = torch.where(case.listed.view(-1, 1), Qn, torch.full_like(Qn, SENT))
                        if centering == "side":
                            uo = oracle_spread_dev(oracle, order0.cpu().numpy(), f0n, kernel, centering, geom, cs, Fv,
                                                   depth)
                    else:
                        assert torch.equal(m.order(), order0), f"{what}: the order depends on the item table"
                check_interp_window(le, ctx, m, case, kernel, centering, geom, q, depth, win, name, cut, what, Qref)
                R0 = check_spread_window(le, ctx, m, case, kernel, centering, geom, f0, Fd, depth, win, name, cut, what)
                if uo is not None:
                    for c in range(3):
                        err = rel_err_dev(R0[c], uo[c])
                        worst = max(worst, err)
                        assert err <= SPREAD_TOL, f"{what} comp {c}: spread rel err {err:.3e}"
            ctx.synchronize()
    print(f"{kernel} {centering}: worst mode-0 spread rel err against the oracle over the item tables {worst:.2e}")


# --------------------------------------------------------------------------
# 4: the fused calls
# --------------------------------------------------------------------------
@pytest.mark.parametrize("centering", ["side", "cell"])
@pytest.mark.parametrize("kernel", c3.PATHS)
def test_fused_spread_halves(le, kernel, centering):
    """zero_spread from all-NaN arrays: the outer half alone completes the planes outside the
    window (cut table: and leaves the inside NaN), both halves leave no NaN and give mode 0's
    bits.  zero_ghosts_spread from NaN ghosts: the halves in either order give mode 0's bits."""
    case = Case(wc.marker_deep(kernel))
    cs = case.cs
    geom = dev_geom(le, cs.geom)
    depth = DEPTH[centering]
    Fd = to_dev(marker_values(cs.F, centering, depth))[0]
    nan0 = geom.alloc(centering, depth, fill=np.nan)
    g0 = geom.alloc(centering, depth)
    _fill(g0, geom, centering, np.random.default_rng(32))  # random values, NaN ghosts
    ctx = le.Context(0)
    for cut in (True, False):
        m = None
        for name, win in wc.windows(cs.geom).items():
            what = f"{kernel} {centering} {'cut' if cut else 'uncut'} {name}{win}"
            if cut or m is None:
                m = window_table(le, ctx, case, kernel, geom, win, cut)
            args = (le, ctx, m, kernel, centering, geom, nan0, Fd, case.Xd, depth, win)
            Z2 = spread_modes(*args, (2,), call="zero_spread")
            Z0, Z21 = (spread_modes(*args, md, call="zero_spread") for md in ((0,), (2, 1)))
            masks = plane_masks(cs.geom, win, nan0)
            for c, mk in enumerate(masks):
                assert not torch.isnan(Z0[c]).any() and bool((Z0[c] != 0).any())
                assert not (torch.isnan(Z2[c]) & ~mk).any(), f"{what}: a plane outside the window was left"
                assert same_where(Z2[c], Z0[c], ~mk), f"{what}: the outer half alone, outside the window"
                if cut:
                    assert (torch.isnan(Z2[c]) | ~mk).all(), f"{what}: the outer half wrote inside the window"
                assert not torch.isnan(Z21[c]).any(), f"{what}: a point was left unwritten"
                assert same(Z21[c], Z0[c]), f"{what}: zero_spread's halves"
            args = (le, ctx, m, kernel, centering, geom, g0, Fd, case.Xd, depth, win)
            G0, G21, G12 = (spread_modes(*args, md, call="zero_ghosts_spread") for md in ((0,), (2, 1), (1, 2)))
            for c in range(len(g0)):
                assert not torch.isnan(G0[c]).any()
                assert same(G21[c], G0[c]) and same(G12[c], G0[c]), f"{what}: zero_ghosts_spread's halves"
    ctx.synchronize()


@pytest.mark.parametrize("kernel", c3.FILL_KERNELS)
def test_fill_interp_halves(le, kernel):
    """fill_interp(periodic x, y) on the unit box under the slab window (the patch's own
    planes): x/y ghosts NaN and never read, z ghosts real; properties 1 and 2, mode 0 equal
    to a plain interp of arrays whose x/y ghost points hold their periodic images' values,
    and no array point written."""
    case = Case(c3.case("wide_unit", "uniform", kernel))
    cs = case.cs
    geom = dev_geom(le, cs.geom)
    win = wc.windows(cs.geom)["interior"]
    assert win == (0, cs.geom.N[2] - 1)
    A = case.A[case.inside]
    inner = wc.inner_anchor(cs.geom, win, A)
    assert inner.sum() >= 1000 and (~inner).sum() >= 1000
    rng = np.random.default_rng(42)
    qb = geom.alloc("side")
    _fill(qb, geom, "side", rng)  # random values, NaN ghosts
    g = cs.geom.g
    for c, a in enumerate(qb):  # the z ghost planes hold values over the interior x, y
        nx, ny = cs.geom.N[0] + (c == 0), cs.geom.N[1] + (c == 1)
        for sl in (slice(0, g), slice(a.shape[0] - g, a.shape[0])):
            blk = a[sl, g:g + ny, g:g + nx]
            blk.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(blk.shape))))
    before = [b.clone() for b in qb]

    def image(n_array, n):  # array index -> the index of its periodic image in the patch box
        i = np.arange(n_array) - g
        return np.where((i < 0) | (i > n - 1), i % n, i) + g

    # the reference arrays: every x/y ghost point of every plane holds its image's value
    qa = to_dev(*[b.cpu().numpy()[:, image(b.shape[1], cs.geom.N[1])][:, :, image(b.shape[2], cs.geom.N[0])]
                  for b in qb])
    assert all(bool(torch.isfinite(a).all()) for a in qa)
    ctx = le.Context(0)
    Qref = None
    for cut in (True, False):
        what = f"fill_interp {kernel} {'cut' if cut else 'uncut'}"
        m = window_table(le, ctx, case, kernel, geom, win, cut)
        if Qref is None:
            (Qref,) = interp_modes(le, ctx, m, kernel, "side", geom, qa, 1, case.Xd, win, modes=(0,))
        check_interp_window(le, ctx, m, case, kernel, "side", geom, qb, 1, win, "interior", cut, what, Qref,
                            periodic=[1, 1, 0])
    for b0, b1 in zip(before, qb):
        assert same(b0, b1), "fill_interp wrote an array point"
    ctx.synchronize()


# --------------------------------------------------------------------------
# 5: heavy, load-split items that a cut goes through
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", c3.PATHS)
def test_cluster_halves(le, oracle, kernel):
    """4 000 markers in one cell of anchor plane 15, windows with a face between planes 15 and
    16: the heavy (column, segment) is cut by load and by the window, at the default tuning
    and with every item above 300 markers split.  Properties 1 and 3, side data."""
    case = Case(c3.case("wide", "cluster", kernel))
    cs = case.cs
    geom = dev_geom(le, cs.geom)
    q, u0 = random_arrays(geom, "side", 1, 23)
    f0, f0n = random_arrays(geom, "side", 1, 24)
    Fd = to_dev(cs.F)[0]
    Qref = uo = None
    for split in (None, 300):
        ctx = le.Context(0)
        if split is not None:
            ctx.tune("split_target", split)
        for cut in (True, False):
            for win in wc.CLUSTER_WINDOWS:
                what = f"cluster {kernel} split_target={split} {'cut' if cut else 'uncut'} {win}"
                m = window_table(le, ctx, case, kernel, geom, win, cut)
                if Qref is None:
                    Qn = gpu_interp(le, ctx, m, kernel, "side", geom, q, 1, case.Xd)
                    ctx.synchronize()
                    check_interp(Qn.cpu().numpy(), oracle_interp(oracle, kernel, "side", geom, u0, cs, 1), cs, kernel,
                                 "side", what)
                    Qref = Qn
                    uo = oracle_spread_dev(oracle, m.order().cpu().numpy(), f0n, kernel, "side", geom, cs, cs.F, 1)
                Q0, Q1, Q2 = interp_modes(le, ctx, m, kernel, "side", geom, q, 1, case.Xd, win)
                assert same(Q0, Qref), f"{what}: mode 0 differs between item tables"
                ingrid, inner = case.sets(win)
                sent = bits(torch.tensor([SENT], dtype=torch.float64, device=DEV))[0]
                r1, r2 = ((bits(Q) != sent).all(dim=1) for Q in (Q1, Q2))
                assert torch.equal(r1 ^ r2, ingrid) and not (r1 & r2 & ingrid).any(), f"{what}: no partition"
                assert torch.equal(bits(Q1)[r1 & ingrid], bits(Q0)[r1 & ingrid])
                assert torch.equal(bits(Q2)[r2], bits(Q0)[r2])
                assert not (r1[8000:12000]).any(), f"{what}: the cluster reads across the face"
                if cut:
                    assert torch.equal(r1 & ingrid, inner), f"{what}: entries on the wrong side of a cut table"
                else:
                    assert not (r1 & ingrid & ~inner).any(), f"{what}: the inner half reads outside the window"
                R0 = check_spread_window(le, ctx, m, case, kernel, "side", geom, f0, Fd, 1, win, None, cut, what)
                for c in range(3):
                    err = rel_err_dev(R0[c], uo[c])
                    assert err <= SPREAD_TOL, f"{what} comp {c}: spread rel err {err:.3e}"
        ctx.synchronize()


# --------------------------------------------------------------------------
# 6: a re-binning after the window changed
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", c3.PATHS)
def test_rebin_after_window_change(le, kernel):
    """Binned and run with no window, then the window set and the unchanged positions
    re-binned: nothing moved, so the re-binning would keep its item table -- but the cuts
    changed, so it must build the one a fresh binning under the window gets.  The halves of
    both give the same bits, the inner half is exactly the cut table's, the order stands."""
    case = Case(wc.marker_deep(kernel))
    cs = case.cs
    geom = dev_geom(le, cs.geom)
    q, _ = random_arrays(geom, "side", 1, 26)
    f0, _ = random_arrays(geom, "side", 1, 27)
    Fd = to_dev(cs.F)[0]
    wins = wc.windows(cs.geom)
    for name in ("interior", "thin"):
        win = wins[name]
        what = f"rebin {kernel} {name}{win}"
        ctx = le.Context(0)
        m = le.Markers(ctx).bin(geom, kernel, case.Xd, case.idd, case.xsd)
        Qa = interp_modes(le, ctx, m, kernel, "side", geom, q, 1, case.Xd, (0, -1), modes=(0,))[0]
        spread_modes(le, ctx, m, kernel, "side", geom, f0, Fd, case.Xd, 1, (0, -1), (0,))  # the candidate stream exists
        order1 = m.order()
        ctx.set_plane_window(0, *win)
        m.rebin(case.Xd)
        fresh = le.Markers(ctx).bin(geom, kernel, case.Xd, case.idd, case.xsd)
        assert torch.equal(m.order(), order1) and torch.equal(fresh.order(), order1), f"{what}: the order changed"
        Qm = interp_modes(le, ctx, m, kernel, "side", geom, q, 1, case.Xd, win)
        Qf = interp_modes(le, ctx, fresh, kernel, "side", geom, q, 1, case.Xd, win)
        assert same(Qm[0], Qa)
        for a, b in zip(Qm, Qf):
            assert same(a, b), f"{what}: interp halves after rebin differ from a fresh binning's"
        check_partition(case, *Qm, win, name, True, what)
        for modes in ((0,), (1,), (2,)):
            Rm = spread_modes(le, ctx, m, kernel, "side", geom, f0, Fd, case.Xd, 1, win, modes)
            Rf = spread_modes(le, ctx, fresh, kernel, "side", geom, f0, Fd, case.Xd, 1, win, modes)
            for c in range(3):
                assert same(Rm[c], Rf[c]), f"{what}: spread mode {modes[0]} comp {c} after rebin"
        check_spread_window(le, ctx, m, case, kernel, "side", geom, f0, Fd, 1, win, name, True, what)
        ctx.synchronize()

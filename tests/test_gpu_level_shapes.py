"""GPU: the level sweeps (ibtk_le_level_*) on levels that are not P x P x P equal cubes --
tests/level_cases.py: `ragged` (six patches of unequal extents at offset and negative indices,
abutting, touching at an edge, far apart; anisotropic dx; periodic in z only), `tiles` (equal
non-cubic patches on a (2, 3, 4) tiling, with and without two tiles missing, three flag sets),
`narrow` (one patch across the z period: select_interior's need_shift branch) and `many`
(2 197 patches, past the sweeps' LDS patch table).  tests/test_level_cases_cpu.py holds the
cases' preconditions.

The reference throughout is the C oracle run patch by patch on that patch's own list and
geometry; it knows nothing of levels.  Arrays lie in the guard memory of test_gpu_depth's
Eul / Lag (`many`: one allocation per component with guard elements between the patches), so
a write outside an array or a Q row is seen.  Interp: Q equals the oracle bit for bit on every
patch's interior entries and rows no list names keep their NaN.  Spread: for the kernels with
non-negative weights every point is within (n_q + 4) 2^-52 S_i of the oracle, S the oracle's
spread of |F| on the same list and n_q the list's length (level_cases.spread_bound); IB_6
within 1e-12 of max |f_ref|.  Each test prints its worst |diff| / bound.

Edge data goes through the level calls like side data (nothing is refused by design); the
level ghost fill takes side and cell data on equal patches that tile a box, and refuses
unequal patches with "equal patches and ghost widths only".

The spread bound found one thing in the kernels, outside the level code: the spread formed
X_o_dx = (X - x_lower) * (1 / dx) for the closed-form kernels (le_sweep.hip spread_setup,
le_stencil.h stencil1d<K, true>) where the oracle divides -- an ulp of X_o_dx, about 1e-14 in r.
An IB_4 weight at distance e from the end of the support is of order e^2, so it moved by a
fraction 2e-14 / e of itself, and a point that only such weights reach by as much of its S_i:
IB_4 stood at 18 to 513 times the bound here (the single-patch le.spread on ragged's patch 0
at the same 141.5 as the level call; BSPLINE_4 at 55), at 5e-15 of max |f_ref|.  The spread now
corrects the product to the quotient (le_stencil.h quotient_mul) and IB_4 is at 0.006-0.12.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import level_cases as lc  # noqa: E402
from test_gpu_depth import DEV, SENT, Eul, Lag, _bits  # noqa: E402


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def flat_lists(c, which, order=None, empty=()):
    """(indices, Xshift or None, offsets) of the patches in `order`, on the device"""
    order = range(c.npatch) if order is None else order
    idx, xs = [], []
    for q in order:
        i, x = (c.interior(q), None) if which == "interior" else c.ghost(q)
        if q in empty:
            i, x = i[:0], (None if x is None else x[:0])
        idx.append(i)
        xs.append(x)
    off = [0] + [int(v) for v in np.cumsum([len(i) for i in idx])]
    return (dev(np.concatenate(idx).astype(np.int32)),
            None if which == "interior" else dev(np.concatenate(xs).reshape(-1, 3)), off)


def make_level(le, ctx, c, which, Xd, order=None, kernel=None):
    return le.Level.from_flat(ctx, c.geoms(le, order), kernel or c.kernel, Xd, *flat_lists(c, which, order))


def qcols(centering, depth):
    return 3 if centering in ("side", "edge") else depth


def euls(geoms, order, centering, depth, seed=None, fill=0.0):
    """one Eul per patch; random values seeded by the patch's number, not its place"""
    return [Eul(g, centering, depth, None if seed is None else np.random.default_rng(seed + 31 * q), fill)
            for g, q in zip(geoms, order)]


def check_interp(c, centering, depth, ue, Q, order=None, X=None, kernel=None):
    """Q (a Lag) equals the oracle bit for bit on every patch's interior entries; the other
    rows keep their NaN; no array was written"""
    order = range(c.npatch) if order is None else order
    Q.check()
    Qg = Q.v.cpu().numpy()
    named = np.zeros(c.M, bool)
    for e, q in zip(ue, order):
        e.unchanged()
        idx = c.interior(q)
        named[idx] = True
        Qo = np.zeros_like(Qg)
        c.oracle("interp", q, centering, e.numpy(), idx, np.zeros((idx.size, 3)), Qo, depth, kernel, X)
        assert np.array_equal(Qg[idx], Qo[idx]), f"patch {q}: interp is not the oracle's bit for bit"
    assert named.any() and np.isnan(Qg[~named]).all(), "a row no list names was written"
    return Qg


def check_spread(c, centering, depth, fe, order=None, X=None, kernel=None):
    """The worst |diff| / bound of every patch's arrays against the oracle (for `bounded` to
    assert once everything else has been checked); here, the guards and the project's own
    tolerance, 1e-12 of max |f_ref| per array."""
    order = range(c.npatch) if order is None else order
    kernel = kernel or c.kernel
    worst = 0.0
    for e, q in zip(fe, order):
        e.check()
        f, S, n_q = c.spread_ref(q, centering, depth, kernel, X=X)
        assert all(np.abs(a).max() > 0 for a in f), "the reference spread nothing"
        for k, (got, ref) in enumerate(zip(e.numpy(), f)):
            err = np.abs(got - ref).max() / np.abs(ref).max()
            assert err <= lc.SPREAD_TOL, f"patch {q} comp {k}: spread rel err {err:.2e}"
        worst = max(worst, lc.spread_ratio(kernel, e.numpy(), f, S, n_q))
    return worst


def bounded(*cases):
    """print the worst |diff| / bound of each case (what, worst), then hold each to 1"""
    for what, worst in cases:
        print(f"{what}: worst |diff| / bound {worst:.3f}")
    for what, worst in cases:
        assert worst <= 1.0, f"{what}: spread |diff| / bound = {worst:.3g}"


def same_bits(ea, eb, what):
    for q, (a, b) in enumerate(zip(ea, eb)):
        for k, (x, y) in enumerate(zip(a.q, b.q)):
            assert torch.equal(_bits(x), _bits(y)), f"patch {q} comp {k}: {what}"


def run_spreads(lvl, geoms, order, centering, depth, F, Xd):
    """spread into zeros twice and zero_spread into NaN: bit-identical, no NaN left"""
    runs = []
    for fill in (0.0, 0.0, float("nan")):
        fe = euls(geoms, order, centering, depth, fill=fill)
        (lvl.zero_spread if fill != 0.0 else lvl.spread)(centering, [e.q for e in fe], F.v, Xd, q_depth=depth)
        runs.append(fe)
    lvl.ctx.synchronize()
    F.unchanged()
    same_bits(runs[0], runs[1], "two spreads differ")
    for e in runs[2]:
        e.check()
        assert not any(bool(torch.isnan(v).any()) for v in e.q), "zero_spread left a point unwritten"
    same_bits(runs[0], runs[2], "zero_spread is not zero + spread")
    return runs[0]


# --------------------------------------------------------------------------
# 1. ragged against the oracle
# --------------------------------------------------------------------------
CENTERINGS = [("side", 1), ("cell", 2), ("node", 3), ("edge", 1)]


@pytest.mark.parametrize("centering,depth", CENTERINGS, ids=lambda v: str(v))
@pytest.mark.parametrize("kernel", ["IB_4", "IB_6", "PIECEWISE_LINEAR"])
def test_ragged_matches_oracle(le, ctx, kernel, centering, depth):
    """interp on the interior lists, spread / zero_spread on the ghost-box lists, every
    centring (edge data included: the level calls take it like side data).

    Worst |diff| / bound on an MI355X: PIECEWISE_LINEAR side 0.005, cell 0.007, node 0.005, edge
    0.005; IB_6 (against 1e-12 max |f_ref|) 0.004, 0.004, 0.004, 0.006; IB_4 0.008, 0.006, 0.006,
    0.006 (141.5, 17.8, 141.5, 141.5 before the spread's X_o_dx was the quotient)."""
    c = lc.case("ragged", kernel)
    order = range(c.npatch)
    geoms, Xd = c.geoms(le), dev(c.X)
    ue = euls(geoms, order, centering, depth, seed=5)
    Q = Lag(c.M, qcols(centering, depth))
    lvl_i, lvl_s = make_level(le, ctx, c, "interior", Xd), make_level(le, ctx, c, "ghost", Xd)
    lvl_i.interp(centering, [e.q for e in ue], Q.v, Xd, q_depth=depth)
    F = Lag(c.M, qcols(centering, depth), c.values(centering, depth))
    fe = run_spreads(lvl_s, geoms, order, centering, depth, F, Xd)
    ctx.synchronize()
    check_interp(c, centering, depth, ue, Q)
    bounded((f"ragged {kernel} {centering} depth {depth}", check_spread(c, centering, depth, fe)))


# --------------------------------------------------------------------------
# 2. patch order
# --------------------------------------------------------------------------
@pytest.mark.parametrize("centering,depth", [("side", 1), ("cell", 2)], ids=lambda v: str(v))
def test_ragged_patch_order(le, ctx, centering, depth):
    """The same level with its patches listed in reverse: each patch's interp rows are bitwise
    those of the forward level, its spread arrays within the bound of the oracle.

    Worst |diff| / bound 0.008 for side and 0.006 for cell data, forward and reversed alike."""
    c = lc.case("ragged", "IB_4")
    Xd = dev(c.X)
    F = Lag(c.M, qcols(centering, depth), c.values(centering, depth))
    Qs, worst = [], []
    for order in (list(range(c.npatch)), list(range(c.npatch))[::-1]):
        geoms = c.geoms(le, order)
        ue = euls(geoms, order, centering, depth, seed=5)
        Q = Lag(c.M, qcols(centering, depth))
        lvl_i, lvl_s = make_level(le, ctx, c, "interior", Xd, order), make_level(le, ctx, c, "ghost", Xd, order)
        lvl_i.interp(centering, [e.q for e in ue], Q.v, Xd, q_depth=depth)
        fe = euls(geoms, order, centering, depth, fill=0.0)
        lvl_s.spread(centering, [e.q for e in fe], F.v, Xd, q_depth=depth)
        ctx.synchronize()
        check_interp(c, centering, depth, ue, Q, order)
        worst.append(check_spread(c, centering, depth, fe, order))
        Qs.append(Q)
    assert torch.equal(_bits(Qs[0].full), _bits(Qs[1].full)), "interp depends on the patches' order"
    bounded((f"ragged IB_4 {centering}, patches forward", worst[0]),
            (f"ragged IB_4 {centering}, patches reversed", worst[1]))


# --------------------------------------------------------------------------
# 3. re-binning
# --------------------------------------------------------------------------
def _level_results(lvl_i, lvl_s, geoms, order, ue, F, Xd, M):
    Q = Lag(M, 3)
    lvl_i.interp("side", [e.q for e in ue], Q.v, Xd)
    fe = euls(geoms, order, "side", 1, fill=0.0)
    lvl_s.spread("side", [e.q for e in fe], F.v, Xd)
    lvl_s.ctx.synchronize()
    return Q, fe


def test_ragged_rebin(le, ctx):
    """Every marker moved by up to 0.6 cell, the sheet carried across the abutting face and
    200 markers put outside every ghost box, then those brought back: after each move
    rebin(X2) equals a fresh Level at X2 (order, interp and spread bit for bit), and the
    fresh level matches the oracle at X2 on the unchanged lists.

    Worst |diff| / bound 0.006 after either move."""
    c = lc.case("ragged", "IB_4")
    order = list(range(c.npatch))
    geoms = c.geoms(le)
    rng = np.random.default_rng(8)
    X1 = c.X + rng.uniform(-0.6, 0.6, c.X.shape) * c.dx
    X1[lc.RAGGED_SHEET, 0] = c.X[lc.RAGGED_SHEET, 0] + 0.6 * c.dx[0]
    face = c.x_lower[0] + (c.lo[1, 0] - c.dom_lo[0]) * c.dx[0]
    crossed = (c.X[lc.RAGGED_SHEET, 0] < face) & (X1[lc.RAGGED_SHEET, 0] >= face)
    assert crossed.sum() >= 10, "the sheet does not cross the face"
    away = rng.choice(np.arange(750, c.M), 200, replace=False)
    X2 = X1.copy()
    X2[away] = c.x_lower + (c.dom_hi + 40 - c.dom_lo) * c.dx + rng.uniform(0, 1, (200, 3))  # beyond every ghost box
    F = Lag(c.M, 3, c.F)
    ue = euls(geoms, order, "side", 1, seed=6)
    X0d = dev(c.X)
    lvl_i, lvl_s = make_level(le, ctx, c, "interior", X0d), make_level(le, ctx, c, "ghost", X0d)
    worst = []
    for step, Xn in enumerate((X2, X1)):
        Xd = dev(Xn)
        lvl_i.rebin(Xd)
        lvl_s.rebin(Xd)
        fresh_i, fresh_s = make_level(le, ctx, c, "interior", Xd), make_level(le, ctx, c, "ghost", Xd)
        assert torch.equal(lvl_i.markers.order(), fresh_i.markers.order()), f"move {step}: interior order"
        assert torch.equal(lvl_s.markers.order(), fresh_s.markers.order()), f"move {step}: ghost-box order"
        Qa, fa = _level_results(lvl_i, lvl_s, geoms, order, ue, F, Xd, c.M)
        Qb, fb = _level_results(fresh_i, fresh_s, geoms, order, ue, F, Xd, c.M)
        assert torch.equal(_bits(Qa.full), _bits(Qb.full)), f"move {step}: interp after rebin"
        same_bits(fa, fb, f"move {step}: spread after rebin")
        check_interp(c, "side", 1, ue, Qb, X=Xn)
        worst.append(check_spread(c, "side", 1, fb, X=Xn))
    bounded(("ragged IB_4 side, 200 markers outside every ghost box", worst[0]),
            ("ragged IB_4 side, moved by up to 0.6 cell", worst[1]))


# --------------------------------------------------------------------------
# 4. relist
# --------------------------------------------------------------------------
def test_ragged_relist(le, ctx):
    """relist(lists).bin(X) equals Level.from_flat on those lists -- order, interp (through the
    interior selection) and spread bit for bit -- from the interior lists to the ghost-box
    lists, back, and to lists with two patches emptied; a wrong number of offsets raises."""
    c = lc.case("ragged", "IB_4")
    order = list(range(c.npatch))
    geoms, Xd = c.geoms(le), dev(c.X)
    F = Lag(c.M, 3, c.F)
    ue = euls(geoms, order, "side", 1, seed=7)

    def results(lvl, select):
        if select is not None:
            lvl.select_interior(c.M, select[0], select[2])
        Q, fe = _level_results(lvl, lvl, geoms, order, ue, F, Xd, c.M)
        return lvl.markers.order().clone(), Q, fe

    def same(a, b, what):
        assert torch.equal(a[0], b[0]), f"{what}: order"
        assert torch.equal(_bits(a[1].full), _bits(b[1].full)), f"{what}: interp"
        same_bits(a[2], b[2], f"{what}: spread")

    li, lg = flat_lists(c, "interior"), flat_lists(c, "ghost")
    lvl = le.Level.from_flat(ctx, geoms, c.kernel, Xd, *li)
    first = results(lvl, None)
    assert not bool(torch.isnan(first[1].v[li[0].long()]).any())
    lvl.relist(*lg).bin(Xd)
    ghost = results(lvl, li)
    same(ghost, results(le.Level.from_flat(ctx, geoms, c.kernel, Xd, *lg), li), "relist to the ghost-box lists")
    assert torch.equal(_bits(ghost[1].full), _bits(first[1].full)), "the interior selection's interp"
    lvl.relist(*li).bin(Xd)
    same(results(lvl, None), first, "relist back")
    empty = (1, 4)
    ge, ie = flat_lists(c, "ghost", empty=empty), flat_lists(c, "interior", empty=empty)
    assert ge[2][-1] < lg[2][-1] and ge[2][2] == ge[2][1]
    lvl.relist(*ge).bin(Xd)
    got = results(lvl, ie)
    same(got, results(le.Level.from_flat(ctx, geoms, c.kernel, Xd, *ge), ie), "relist with two patches emptied")
    for q in empty:
        assert all(not bool(v.any()) for v in got[2][q].q) and np.isnan(got[1].v.cpu().numpy()[c.interior(q)]).all()
    with pytest.raises(ValueError):
        lvl.relist(lg[0], lg[1], lg[2][:-1])
    with pytest.raises(ValueError):
        lvl.relist(lg[0], lg[1], lg[2] + [lg[2][-1]])
    ctx.synchronize()


# --------------------------------------------------------------------------
# 5. select_interior
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "narrow"])
def test_select_interior(le, ctx, name):
    """The ghost-box binning with the interior lists selected interpolates bit for bit as the
    interior binning and as the oracle -- on `narrow`, where a marker near a z face and its
    image are both in its patch's list, from the unshifted entry (the arrays are random, so
    their z ghosts differ from their periodic images and the shifted entry gives another
    value) -- and again after a rebin that moves markers, the cached selection redone."""
    c = lc.case(name)
    order = list(range(c.npatch))
    geoms = c.geoms(le)
    ue = euls(geoms, order, "side", 1, seed=9)
    li = flat_lists(c, "interior")
    if name == "narrow":  # the image's value differs: the check below can tell the entries apart
        idx, xs = c.ghost(0)
        img = xs.any(axis=1) & np.isin(idx, c.interior(0))
        assert img.sum() >= 20
        Qs, Qu = np.zeros((c.M, 3)), np.zeros((c.M, 3))
        c.oracle("interp", 0, "side", ue[0].numpy(), idx[img], xs[img], Qs)
        c.oracle("interp", 0, "side", ue[0].numpy(), idx[img], 0 * xs[img], Qu)
        assert np.all(np.any(Qs[idx[img]] != Qu[idx[img]], axis=1))
    rng = np.random.default_rng(10)
    X1 = c.X + rng.uniform(-0.3, 0.3, c.X.shape) * c.dx
    lvl_g, seen = None, []
    for step, Xn in enumerate((c.X, X1)):
        Xd = dev(Xn)
        if lvl_g is None:
            lvl_g = make_level(le, ctx, c, "ghost", Xd)
        else:
            lvl_g.rebin(Xd)
        lvl_g.select_interior(c.M, li[0], li[2])
        Qg = Lag(c.M, 3)
        lvl_g.interp("side", [e.q for e in ue], Qg.v, Xd)
        Qi = Lag(c.M, 3)
        lvl_i = make_level(le, ctx, c, "interior", Xd)
        lvl_i.interp("side", [e.q for e in ue], Qi.v, Xd)
        ctx.synchronize()
        assert torch.equal(_bits(Qg.full), _bits(Qi.full)), f"step {step}: selection against the interior binning"
        seen.append(check_interp(c, "side", 1, ue, Qg, X=Xn))
    moved = np.any(seen[0] != seen[1], axis=1)[c.int_idx]
    assert moved.mean() > 0.9, "the move changed nothing: the second selection was not put to the test"


# --------------------------------------------------------------------------
# 6. fill_ghosts on the tilings
# --------------------------------------------------------------------------
FLAGS = [(f, h) for f in lc.TILES_FLAGS for h in (False, True)]


def _fill_case(le, c, centering, depth, seed):
    G = lc.fill_fields(c, centering, depth, seed)
    rng = np.random.default_rng(seed + 1)
    return [lc.fill_arrays(c, q, centering, depth, G, rng) for q in range(c.npatch)]


@pytest.mark.parametrize("centering,depth", [("side", 1), ("cell", 2)], ids=lambda v: str(v))
@pytest.mark.parametrize("periodic,holes", FLAGS, ids=lambda v: str(v))
def test_tiles_fill_ghosts(le, ctx, periodic, holes, centering, depth):
    """Against a numpy fill from one global field: a ghost point takes the value at its wrapped
    global index when a patch owns that cell and the wrap is allowed, otherwise it keeps its
    value bit for bit; the patches' own points are unchanged."""
    c = lc.case("tiles", "IB_4", periodic, holes)
    geoms, Xd = c.geoms(le), dev(c.X)
    host = _fill_case(le, c, centering, depth, 12)
    ue = [Eul(g, centering, depth).set(h[0]) for g, h in zip(geoms, host)]
    lvl = make_level(le, ctx, c, "interior", Xd)
    lvl.fill_ghosts(centering, [e.q for e in ue], q_depth=depth, periodic=list(periodic))
    ctx.synchronize()
    for q, (e, h) in enumerate(zip(ue, host)):
        e.check()
        for a, (got, want) in enumerate(zip(e.numpy(), h[1])):
            assert np.array_equal(got, want), f"patch {q} comp {a}"


def test_fill_ghosts_refuses_unequal_patches(le, ctx):
    from ibamr_amd._lib import IBTKLEError
    c = lc.case("ragged", "IB_4")
    geoms, Xd = c.geoms(le), dev(c.X)
    lvl = make_level(le, ctx, c, "interior", Xd)
    for centering, depth in (("side", 1), ("cell", 2)):
        ue = euls(geoms, range(c.npatch), centering, depth, seed=13)
        Q = Lag(c.M, qcols(centering, depth))
        with pytest.raises(IBTKLEError, match="level_fill_ghosts: equal patches and ghost widths only") as e:
            lvl.fill_ghosts(centering, [x.q for x in ue], q_depth=depth, periodic=[0, 0, 1])
        assert e.value.code == 4
        if depth == 1:  # the fused call refuses them before it reads or writes anything
            with pytest.raises(IBTKLEError, match="level_fill_interp: equal patches and ghost widths only") as e:
                lvl.fill_interp(centering, [x.q for x in ue], Q.v, Xd, q_depth=depth, periodic=[0, 0, 1])
            assert e.value.code == 4
        ctx.synchronize()
        Q.unchanged()
        for x in ue:
            x.unchanged()


# --------------------------------------------------------------------------
# 7. fill_interp on the tilings
# --------------------------------------------------------------------------
def _one_window(ue):
    """ibtk_le_level_fill_interp fuses the fill when each component's arrays of every patch lie
    within 2 GB of each other (where separate allocations land is the allocator's business)"""
    for a in range(len(ue[0].q)):
        lo = min(e.q[a].data_ptr() for e in ue)
        hi = max(e.q[a].data_ptr() + 8 * e.q[a].numel() for e in ue)
        if hi - lo >= 1 << 31:
            return False
    return True


@pytest.mark.parametrize("kernel,centering", [("IB_4", "side"), ("IB_4", "cell"), ("IB_6", "side")])
@pytest.mark.parametrize("periodic,holes", FLAGS, ids=lambda v: str(v))
def test_tiles_fill_interp(le, ctx, periodic, holes, kernel, centering):
    """Q of the fused call equals fill_ghosts + interp bit for bit and the oracle on the
    numpy-filled arrays; the fused call's arrays hold NaN wherever a neighbour supplies the
    ghost, and it writes no array point.  With one allocation per array (in guard memory) and
    with alloc_level's arrays."""
    c = lc.case("tiles", kernel, periodic, holes)
    geoms, Xd = c.geoms(le), dev(c.X)
    D = qcols(centering, 1)
    host = _fill_case(le, c, centering, 1, 14)
    nan = [[np.where(s, np.nan, b) for b, s in zip(h[0], h[2])] for h in host]
    lvl = make_level(le, ctx, c, "interior", Xd)
    # one allocation per array
    ua = [Eul(g, centering, 1).set(h[0]) for g, h in zip(geoms, host)]
    ub = [Eul(g, centering, 1).set(v) for g, v in zip(geoms, nan)]
    Qa, Qb = Lag(c.M, D), Lag(c.M, D)
    lvl.fill_ghosts(centering, [e.q for e in ua], periodic=list(periodic))
    lvl.interp(centering, [e.q for e in ua], Qa.v, Xd)
    lvl.fill_interp(centering, [e.q for e in ub], Qb.v, Xd, periodic=list(periodic))
    ctx.synchronize()
    if _one_window(ub):
        for e in ub:
            e.unchanged()
    else:  # the documented two calls: the fill wrote the ghosts
        for q, (e, h) in enumerate(zip(ub, host)):
            e.check()
            assert all(np.array_equal(got, want) for got, want in zip(e.numpy(), h[1])), f"patch {q}: the fill"
    assert torch.equal(_bits(Qa.full), _bits(Qb.full)), "fill_interp against fill_ghosts + interp"
    uo = [Eul(g, centering, 1).set(h[1]) for g, h in zip(geoms, host)]  # the numpy-filled arrays
    check_interp(c, centering, 1, uo, Qb)
    # alloc_level's arrays: a component's arrays of every patch in one allocation
    va, vb = le.alloc_level(geoms, centering), le.alloc_level(geoms, centering)
    for q in range(c.npatch):
        for a in range(len(va[q])):
            va[q][a].copy_(dev(host[q][0][a]))
            vb[q][a].copy_(dev(nan[q][a]))
    before = [[t.clone() for t in per] for per in vb]
    Qc, Qd = Lag(c.M, D), Lag(c.M, D)
    lvl.fill_ghosts(centering, va, periodic=list(periodic))
    lvl.interp(centering, va, Qc.v, Xd)
    lvl.fill_interp(centering, vb, Qd.v, Xd, periodic=list(periodic))
    ctx.synchronize()
    assert torch.equal(_bits(Qc.full), _bits(Qb.full)) and torch.equal(_bits(Qd.full), _bits(Qb.full))
    for q in range(c.npatch):
        for a in range(len(va[q])):
            assert np.array_equal(va[q][a].cpu().numpy(), host[q][1][a]), f"patch {q} comp {a}: fill_ghosts"
            assert torch.equal(_bits(vb[q][a]), _bits(before[q][a])), "an array point was written"


# --------------------------------------------------------------------------
# 8. more patches than the LDS patch table holds
# --------------------------------------------------------------------------
class Block:
    """The side arrays of every patch of a case carved from one allocation per component, two
    SENT elements before, between and after them (a guard per Eul would be 6 591 allocations)."""

    def __init__(self, c, rng=None):
        self.c = c
        self.buf, self.off, self.q = [], [], [[None] * 3 for _ in range(c.npatch)]
        self.inside = []
        for a in range(3):
            shapes = [c.array_shape(q, "side", a) for q in range(c.npatch)]
            sizes = np.array([int(np.prod(s)) for s in shapes])
            assert not (sizes % 2).any()  # 16-byte aligned arrays
            off = 2 + np.concatenate([[0], np.cumsum(sizes + 2)[:-1]])
            tot = int(off[-1] + sizes[-1] + 2)
            h = np.full(tot, SENT)
            inside = np.zeros(tot, bool)
            for q in range(c.npatch):
                h[off[q]:off[q] + sizes[q]] = rng.uniform(-1, 1, sizes[q]) if rng is not None else 0.0
                inside[off[q]:off[q] + sizes[q]] = True
            buf = dev(h)
            for q in range(c.npatch):
                self.q[q][a] = buf[off[q]:off[q] + sizes[q]].view(shapes[q])
            self.buf.append(buf)
            self.off.append((off, sizes, shapes))
            self.inside.append(inside)
        self.snap = [b.clone() for b in self.buf]

    def host(self):
        """(check the guards and) every array on the host: host()[q] = patch q's three arrays"""
        out = [[None] * 3 for _ in range(self.c.npatch)]
        for a, buf in enumerate(self.buf):
            h = buf.cpu().numpy()
            assert np.all(h[~self.inside[a]] == SENT), "guard memory was written"
            off, sizes, shapes = self.off[a]
            for q in range(self.c.npatch):
                out[q][a] = h[off[q]:off[q] + sizes[q]].reshape(shapes[q])
        return out

    def unchanged(self):
        assert all(torch.equal(_bits(b), _bits(s)) for b, s in zip(self.buf, self.snap)), "an array was written"


def _sub_level(le, ctx, c, which, Xd, geoms, order):
    return le.Level.from_flat(ctx, [geoms[q] for q in order], c.kernel, Xd, *flat_lists(c, which, order))


def test_many_patches(le, ctx):
    """2 197 patches (the sweeps search the patch table in global memory past 2 048): interp and
    spread against the oracle on 64 patches that include 0, 2047, 2048 and 2196, and against the
    same level run as two levels of 1 098 and 1 099 patches, which use the LDS table -- interp
    bit for bit, spread within the bound; one rebin after a move equals a fresh level.

    Worst |diff| / bound 0.111 as one level and as two, 0.120 after the move."""
    c = lc.case("many")
    geoms, Xd = c.geoms(le), dev(c.X)
    sample = lc.many_sample(c)
    u = Block(c, np.random.default_rng(15))
    F = Lag(c.M, 3, c.F)
    halves = (list(range(0, 1098)), list(range(1098, c.npatch)))
    assert len(halves[1]) == 1099

    def run(levels_i, levels_s, orders, X):
        Q, f = Lag(c.M, 3), Block(c)
        for li_, ls_, o in zip(levels_i, levels_s, orders):
            li_.interp("side", [u.q[q] for q in o], Q.v, X)
            ls_.spread("side", [f.q[q] for q in o], F.v, X)
        ctx.synchronize()
        return Q, f

    def against_oracle(Q, f, X, what):
        Q.check()
        u.unchanged()
        F.unchanged()
        Qg, uh, fh = Q.v.cpu().numpy(), u.host(), f.host()
        assert not np.isnan(Qg).any(), "every marker is interior to one patch"
        worst = 0.0
        for q in sample:
            idx = c.interior(q)
            Qo = np.zeros_like(Qg)
            c.oracle("interp", q, "side", uh[q], idx, np.zeros((idx.size, 3)), Qo, X=X)
            assert np.array_equal(Qg[idx], Qo[idx]), f"{what}: patch {q} interp"
            fr, S, n_q = c.spread_ref(q, "side", X=X)
            for k in range(3):
                err = np.abs(fh[q][k] - fr[k]).max() / np.abs(fr[k]).max()
                assert err <= lc.SPREAD_TOL, f"{what}: patch {q} comp {k}: spread rel err {err:.2e}"
            worst = max(worst, lc.spread_ratio(c.kernel, fh[q], fr, S, n_q))
        return worst

    whole = list(range(c.npatch))
    lvl_i, lvl_s = _sub_level(le, ctx, c, "interior", Xd, geoms, whole), _sub_level(le, ctx, c, "ghost", Xd, geoms, whole)
    Q, f = run([lvl_i], [lvl_s], [whole], Xd)
    worst = [against_oracle(Q, f, c.X, "one level")]
    Q2, f2 = run([_sub_level(le, ctx, c, "interior", Xd, geoms, o) for o in halves],
                 [_sub_level(le, ctx, c, "ghost", Xd, geoms, o) for o in halves], halves, Xd)
    worst.append(against_oracle(Q2, f2, c.X, "two levels"))
    assert torch.equal(_bits(Q.full), _bits(Q2.full)), "interp: one level against two"
    # one rebin after a move
    X1 = c.X + np.random.default_rng(16).uniform(-0.6, 0.6, c.X.shape) * c.dx
    X1d = dev(X1)
    lvl_i.rebin(X1d)
    lvl_s.rebin(X1d)
    fresh_i, fresh_s = _sub_level(le, ctx, c, "interior", X1d, geoms, whole), _sub_level(le, ctx, c, "ghost", X1d, geoms, whole)
    assert torch.equal(lvl_i.markers.order(), fresh_i.markers.order())
    assert torch.equal(lvl_s.markers.order(), fresh_s.markers.order())
    Qa, fa = run([lvl_i], [lvl_s], [whole], X1d)
    Qb, fb = run([fresh_i], [fresh_s], [whole], X1d)
    assert torch.equal(_bits(Qa.full), _bits(Qb.full)), "interp after rebin"
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fa.buf, fb.buf)), "spread after rebin"
    worst.append(against_oracle(Qb, fb, X1, "after a move"))
    bounded(*[(f"many IB_4 side, {what}", w)
              for what, w in zip(("one level", "two levels", "one level after a move"), worst)])

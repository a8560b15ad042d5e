"""GPU: the 2-D brick path (le_hot.hip) at sizes where its loops repeat.

Every other 2-D test runs make_case's 29x30 patch (one tile, 4 work items, 263 listed
markers) or cfg1's 304-marker ellipse.  There k_cand's sub-pass carry, the chunk and class
loops of k_spread, the marker loop of k_interp, a second round of work items and a
non-square tile grid never run.  The cases of tests/cases2d.py make them run
(tests/test_cases2d_cpu.py asserts that they do); here the kernels are compared with the
oracle on them: interp bit for bit (the 2-D interp sums in the Fortran order), spread
within the project's 1e-12 both in the library's order and in the caller's.  Every test
ends with ctx.synchronize(), which raises on the device invariant flags.
"""
import numpy as np
import pytest

import cases2d as c2

torch = pytest.importorskip("torch")

from test_gpu_depth import np_ghost_op  # noqa: E402
from test_gpu_parity import INTERP_TOL, SPREAD_TOL, make_case, oracle_call, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEPTH = {"side": 1, "cell": 2, "node": 1}


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def dev_geom(le, g):
    return le.Geometry(list(g.ilower), list(g.iupper), g.g, list(g.dx), list(g.x_lower))


def to_dev(cs):
    return (torch.from_numpy(cs.X).to(DEV), torch.from_numpy(cs.idx).to(DEV), torch.from_numpy(cs.xshift).to(DEV))


def random_arrays(geom, centering, depth, seed):
    rng = np.random.default_rng(seed)
    q = geom.alloc(centering, depth)
    for a in q:
        a.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(a.shape))))
    return q, [a.cpu().numpy().copy() for a in q]


def q_depth_of(centering, depth):
    return 2 if centering == "side" else depth


def marker_values(F, centering, depth):
    return np.ascontiguousarray(F[:, :q_depth_of(centering, depth)])


def gpu_interp(le, ctx, m, kernel, centering, geom, q, depth, Xd):
    Q = torch.full((Xd.shape[0], q_depth_of(centering, depth)), np.nan, dtype=torch.float64, device=DEV)
    le.interp(ctx, m, kernel, centering, geom, q, Q, Xd, q_depth=depth)
    return Q


def oracle_interp(oracle, kernel, centering, geom, u0, cs, depth):
    Qo = np.full((cs.X.shape[0], q_depth_of(centering, depth)), np.nan)
    oracle_call(oracle, "interp", kernel, centering, geom, u0, cs.idx, cs.xshift, cs.X, Qo, depth)
    return Qo


def far_outside(cs):
    """Markers of the list whose shifted position is more than 16 cells from the patch in
    some dim: no stencil of any kernel reaches an array."""
    g = cs.geom
    Xs = cs.X[cs.idx] + cs.xshift
    far = np.zeros(cs.idx.size, bool)
    for d in range(2):
        far |= (Xs[:, d] < g.x_lower[d] - 16 * g.dx[d]) | (Xs[:, d] > g.x_lower[d] + g.L[d] + 16 * g.dx[d])
    return cs.idx[far]


def check_interp(Qg, Qo, cs, what):
    listed = np.zeros(cs.X.shape[0], bool)
    listed[cs.idx] = True
    assert np.isnan(Qg[~listed]).all(), f"{what}: unlisted markers must be untouched"
    assert not np.isnan(Qo[listed]).any()
    err = rel_err(Qg[listed], Qo[listed])
    print(f"{what}: interp rel err {err:.2e}")
    assert err <= INTERP_TOL
    assert np.array_equal(Qg[listed], Qo[listed]), f"{what}: interp is not bitwise the oracle's"
    far = far_outside(cs)
    if cs.xshift.any():
        assert far.size > 100 and (far < 5).any(), "the case has far-outside markers"
    assert (Qg[far] == 0.0).all(), f"{what}: far-outside markers read 0"


def check_spread(oracle, le_order, ug, u0, kernel, centering, geom, cs, Fv, depth, what):
    """ug against the oracle's spread of Fv into u0, in the library's order and the caller's."""
    assert np.array_equal(np.sort(le_order), np.arange(cs.idx.size))
    uo = [a.copy() for a in u0]
    oracle_call(oracle, "spread", kernel, centering, geom, uo, cs.idx[le_order], cs.xshift[le_order], cs.X,
                Fv.copy(), depth)
    uc = [a.copy() for a in u0]
    oracle_call(oracle, "spread", kernel, centering, geom, uc, cs.idx, cs.xshift, cs.X, Fv.copy(), depth)
    for a in range(len(ug)):
        assert not np.array_equal(uo[a], u0[a]), "the spread reaches the array"
        e1, e2 = rel_err(ug[a], uo[a]), rel_err(ug[a], uc[a])
        print(f"{what} comp {a}: spread rel err {e1:.2e} (sorted order), {e2:.2e} (caller's order)")
        assert e1 <= SPREAD_TOL, f"{what}: spread comp {a} rel err {e1:.3e}"
        assert e2 <= SPREAD_TOL, f"{what}: spread comp {a} rel err {e2:.3e} against the caller's order"
    bitwise = all(np.array_equal(ug[a], uo[a]) for a in range(len(ug)))
    print(f"{what}: spread bitwise in sorted order = {bitwise}")
    return uo


def run_parity(le, ctx, oracle, case, centering):
    name, kind, kernel, extra = case
    cs = c2.case(name, kind, kernel, extra)
    geom = dev_geom(le, cs.geom)
    depth = DEPTH[centering]
    what = f"{name} {kind} {kernel} {centering}"
    Xd, idd, xsd = to_dev(cs)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    assert m.count() == cs.idx.size
    # interp
    q, u0 = random_arrays(geom, centering, depth, 11)
    Q = gpu_interp(le, ctx, m, kernel, centering, geom, q, depth, Xd)
    ctx.synchronize()
    check_interp(Q.cpu().numpy(), oracle_interp(oracle, kernel, centering, geom, u0, cs, depth), cs, what)
    # spread into a random, non-zero u
    q, u0 = random_arrays(geom, centering, depth, 12)
    Fv = marker_values(cs.F, centering, depth)
    le.spread(ctx, m, kernel, centering, geom, q, torch.from_numpy(Fv).to(DEV), Xd, q_depth=depth)
    ctx.synchronize()
    check_spread(oracle, m.order().cpu().numpy(), [a.cpu().numpy() for a in q], u0, kernel, centering, geom, cs, Fv,
                 depth, what)
    ctx.synchronize()


@pytest.mark.parametrize("centering", ["side", "cell", "node"])
@pytest.mark.parametrize("kernel", c2.ALL)
def test_wide_uniform(le, ctx, oracle, kernel, centering):
    """12 work items in a 3x1 tile grid: a second round of 4 items with 4 skipped; every
    neighbourhood of several sub-passes, classes of several chunks, items of several passes."""
    run_parity(le, ctx, oracle, ("wide", "uniform", kernel, 0), centering)


@pytest.mark.parametrize("case", [c for c in c2.GPU_CASES if c[0] in ("tall", "big")], ids=_id)
def test_tall_and_big_uniform(le, ctx, oracle, case):
    """The transpose (an x/y swap in the tile index), and 5x3 tiles: 60 items, 56 workgroups
    dealt 7 to an XCD and a second round of 4, neighbourhoods across tiles in both dims."""
    run_parity(le, ctx, oracle, case, "side")


# --------------------------------------------------------------------------
# cluster: thousands of candidates in one class, sent to the same grid points
# --------------------------------------------------------------------------
def _spread_once(le, ctx, geom, kernel, cs, Xd, idd=None, xsd=None, u0=None, F=None):
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    q = geom.alloc("side")
    if u0 is not None:
        for a, b in zip(q, u0):
            a.copy_(torch.from_numpy(b))
    le.spread(ctx, m, kernel, "side", geom, q, torch.from_numpy(cs.F if F is None else F).to(DEV), Xd)
    ctx.synchronize()
    return m, q


@pytest.mark.parametrize("kernel", c2.CLUSTER_KERNELS)
def test_cluster_interp(le, ctx, oracle, kernel):
    cs = c2.case("wide", "cluster", kernel)
    geom = dev_geom(le, cs.geom)
    Xd, idd, xsd = to_dev(cs)
    m = le.Markers(ctx).bin(geom, kernel, Xd)
    q, u0 = random_arrays(geom, "side", 1, 13)
    Q = gpu_interp(le, ctx, m, kernel, "side", geom, q, 1, Xd)
    ctx.synchronize()
    check_interp(Q.cpu().numpy(), oracle_interp(oracle, kernel, "side", geom, u0, cs, 1), cs, f"cluster {kernel}")
    ctx.synchronize()


@pytest.mark.parametrize("kernel", c2.CLUSTER_KERNELS)
def test_cluster_spread(le, ctx, oracle, kernel):
    """4 000 markers in one cell, beside a corner of four super-bricks in two tiles: a class
    of more than 60 chunks.  Within tolerance of the oracle in both orders, and the same
    bits from a second Markers and a second run."""
    cs = c2.case("wide", "cluster", kernel)
    geom = dev_geom(le, cs.geom)
    Xd, _, _ = to_dev(cs)
    _, u0 = random_arrays(geom, "side", 1, 14)
    m, q = _spread_once(le, ctx, geom, kernel, cs, Xd, u0=u0)
    check_spread(oracle, m.order().cpu().numpy(), [a.cpu().numpy() for a in q], u0, kernel, "side", geom, cs, cs.F, 1,
                 f"cluster {kernel}")
    m2, q2 = _spread_once(le, ctx, geom, kernel, cs, Xd, u0=u0)
    assert torch.equal(m.order(), m2.order())
    for a in range(2):
        assert torch.equal(q[a], q2[a]), f"comp {a}: a second Markers and run give other bits"
    ctx.synchronize()


@pytest.mark.parametrize("kernel", c2.CLUSTER_KERNELS)
def test_cluster_conservation(le, ctx, oracle, kernel):
    """sum f dx dy = sum F over the markers whose whole stencil lies inside the arrays.  Those
    are spread alone: the markers whose key cell is more than max(HI, -LO) cells inside every
    array's index range; that none of them is clipped is confirmed by the oracle conserving
    their sum too."""
    cs = c2.case("wide", "cluster", kernel)
    g = cs.geom
    geom = dev_geom(le, g)
    W, LO, HI = c2.KINFO[kernel]
    reach = max(HI, -LO) + 1  # + 1: the key cell is taken by floor here, the kernels may round
    keep = np.ones(cs.X.shape[0], bool)
    for d in range(2):
        cell = np.floor((cs.X[:, d] - g.x_lower[d]) / g.dx[d])
        keep &= (cell - reach >= -g.g) & (cell + reach <= g.N[d] - 1 + g.g)
    idx = np.nonzero(keep)[0].astype(np.int32)
    assert idx.size > 6_000 and keep[8000:].all(), "every cluster marker and many of the others qualify"
    Xd = torch.from_numpy(cs.X).to(DEV)
    idd = torch.from_numpy(idx).to(DEV)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd)
    q = geom.alloc("side")
    le.spread(ctx, m, kernel, "side", geom, q, torch.from_numpy(cs.F).to(DEV), Xd)
    ctx.synchronize()
    uo = [np.zeros(tuple(a.shape)) for a in q]
    oracle.side_spread(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, uo, idx,
                       np.zeros((idx.size, 2)), cs.X, cs.F)
    h2 = g.dx[0] * g.dx[1]
    for a in range(2):
        want = cs.F[idx, a].sum()
        ref = uo[a].sum() * h2
        got = q[a].cpu().numpy().sum() * h2
        print(f"cluster {kernel} comp {a}: sum F {want:.15e}, oracle {ref:.15e}, gpu {got:.15e}")
        assert abs(ref - want) <= 1e-12 * abs(want), "the oracle clips none of the selected markers"
        assert abs(got - want) <= 1e-12 * abs(want)
    ctx.synchronize()


# --------------------------------------------------------------------------
# spread_ds
# --------------------------------------------------------------------------
@pytest.mark.parametrize("centering", ["cell", "side"])
def test_spread_ds(le, ctx, oracle, centering):
    """The density-weighted spread against the oracle given F ds, rounded once."""
    kernel = "IB_4"
    cs = c2.case("wide", "uniform", kernel)
    geom = dev_geom(le, cs.geom)
    depth = DEPTH[centering]
    Xd, idd, xsd = to_dev(cs)
    ds = np.random.default_rng(5).uniform(0.5, 2.0, cs.X.shape[0])
    Fv = marker_values(cs.F, centering, depth)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    q, u0 = random_arrays(geom, centering, depth, 15)
    le.spread(ctx, m, kernel, centering, geom, q, torch.from_numpy(Fv).to(DEV), Xd, q_depth=depth,
              ds=torch.from_numpy(ds).to(DEV))
    ctx.synchronize()
    check_spread(oracle, m.order().cpu().numpy(), [a.cpu().numpy() for a in q], u0, kernel, centering, geom, cs,
                 Fv * ds[:, None], depth, f"spread_ds {centering}")
    ctx.synchronize()


# --------------------------------------------------------------------------
# periodic round trip
# --------------------------------------------------------------------------
class _SideComp:
    """The index ranges of side component `a`, as np_ghost_op reads a geometry."""

    def __init__(self, geom, a):
        self.ndim, self.gcw, self.ilower, self.iupper, self.a = geom.ndim, geom.gcw, geom.ilower, geom.iupper, a

    def ext_mask(self, centering):
        return 1 << self.a


@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
def test_periodic_round_trip(le, ctx, oracle, kernel):
    """A 96x80 periodic box (2x2 tiles, 16 items), 20 000 markers: fill + interp bitwise the
    oracle's on the filled array; zero_spread + fold against the oracle and a numpy fold;
    the fold conserves sum F; <U, F> = <u, f> dx dy."""
    g = oracle.min_ghost_width(kernel)
    N = [96, 80]
    geom = le.Geometry.periodic_unit(N, g)
    rng = np.random.default_rng(31)
    M = 20_000
    Xn = rng.random((M, 2))
    Fn = rng.standard_normal((M, 2)) + 1.0
    idx = np.arange(M, dtype=np.int32)
    xs = np.zeros((M, 2))
    Xd, Fd = torch.from_numpy(Xn).to(DEV), torch.from_numpy(Fn).to(DEV)
    m = le.Markers(ctx).bin(geom, kernel, Xd)
    # interp side
    u = geom.alloc("side")
    for a in u:
        a.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(a.shape)) + 2.0))
    le.fill_periodic_ghosts(ctx, geom, "side", u)
    U = torch.full((M, 2), np.nan, dtype=torch.float64, device=DEV)
    le.interp(ctx, m, kernel, "side", geom, u, U, Xd)
    ctx.synchronize()
    uf = [a.cpu().numpy().copy() for a in u]
    Uo = np.zeros((M, 2))
    oracle.side_interp(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, uf, idx, xs, Xn, Uo)
    Ug = U.cpu().numpy()
    assert np.array_equal(Ug, Uo)
    # spread side
    f = geom.alloc("side", fill=7.0)
    le.zero_spread(ctx, m, kernel, "side", geom, f, Fd, Xd)
    le.fold_periodic_ghosts(ctx, geom, "side", f)
    ctx.synchronize()
    order = m.order().cpu().numpy()
    fo = [np.zeros(tuple(a.shape)) for a in f]
    oracle.side_spread(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, fo, idx[order], xs, Xn, Fn)
    h2 = geom.dx[0] * geom.dx[1]
    lhs = float((Ug * Fn).sum())
    rhs = 0.0
    for a in range(2):
        want = np_ghost_op("fold", fo[a][None], _SideComp(geom, a), "side", [1, 1])[0]
        got = f[a].cpu().numpy()
        err = rel_err(got, want)
        print(f"periodic {kernel} comp {a}: folded spread rel err {err:.2e}")
        assert err <= SPREAD_TOL
        unique = got[g:g + N[1], g:g + N[0]]
        tot, sumF = unique.sum() * h2, Fn[:, a].sum()
        assert abs(tot - sumF) <= 1e-12 * abs(sumF), f"comp {a}: {tot} vs {sumF}"
        rhs += float((uf[a][g:g + N[1], g:g + N[0]] * unique).sum()) * h2
    print(f"periodic {kernel}: <U,F> = {lhs:.15e}, <u,f> dx dy = {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    ctx.synchronize()


# --------------------------------------------------------------------------
# rebin and reuse
# --------------------------------------------------------------------------
def _interp_spread(le, ctx, m, kernel, geom, Xd, F, seed):
    """(Q, arrays after a spread into random values) through the binned list m, side data."""
    q, _ = random_arrays(geom, "side", 1, seed)
    Q = gpu_interp(le, ctx, m, kernel, "side", geom, q, 1, Xd)
    le.spread(ctx, m, kernel, "side", geom, q, F, Xd)
    ctx.synchronize()
    return Q, q


def _same(a, b, what):
    Qa, qa = a
    Qb, qb = b
    assert torch.equal(torch.nan_to_num(Qa, nan=-7.0), torch.nan_to_num(Qb, nan=-7.0)), f"{what}: interp"
    assert bool(torch.isnan(Qa).logical_xor(torch.isnan(Qb)).any()) is False, f"{what}: interp rows written"
    for c in range(len(qa)):
        assert torch.equal(qa[c], qb[c]), f"{what}: spread comp {c}"


@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
def test_rebin_2d(le, ctx, kernel):
    """The 2-D rebin is a fresh binning of the kept list (indices and shifts) at the new
    positions: same order, same interp and spread bits as a new Markers; the count stays,
    and a second rebin at the same positions changes nothing."""
    cs = c2.case("wide", "uniform", kernel)
    geom = dev_geom(le, cs.geom)
    Xd, idd, xsd = to_dev(cs)
    Fd = torch.from_numpy(cs.F).to(DEV)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    _interp_spread(le, ctx, m, kernel, geom, Xd, Fd, 16)  # the candidate lists exist
    order1 = m.order()
    X2n = cs.X + np.random.default_rng(6).uniform(-0.6, 0.6, cs.X.shape) * np.array(cs.geom.dx)
    X2 = torch.from_numpy(X2n).to(DEV)
    m.rebin(X2)
    fresh = le.Markers(ctx).bin(geom, kernel, X2, idd, xsd)
    assert m.count() == fresh.count() == cs.idx.size
    order2 = m.order()
    assert torch.equal(order2, fresh.order())
    assert not torch.equal(order1, order2), "the move changes the order"
    want = _interp_spread(le, ctx, fresh, kernel, geom, X2, Fd, 17)
    got = _interp_spread(le, ctx, m, kernel, geom, X2, Fd, 17)
    _same(got, want, "after rebin")
    m.rebin(X2)
    assert m.count() == cs.idx.size
    assert torch.equal(m.order(), order2)
    _same(_interp_spread(le, ctx, m, kernel, geom, X2, Fd, 17), want, "after a second rebin")
    ctx.synchronize()


def test_reuse_of_one_markers(le, ctx):
    """One Markers through a large binning, a small one with another kernel and geometry,
    then a clustered one: the buffers only grow, and what the larger binning left in them
    (candidate offsets and lists, bucket starts) must not be read.  After each step interp
    and spread equal those of a fresh Markers bit for bit."""
    m = le.Markers(ctx)
    old = make_case("IB_6", 2, "side", seed=3)
    steps = [("big", "uniform", "IB_4"), None, ("wide", "cluster", "PIECEWISE_CONSTANT")]
    for n, step in enumerate(steps):
        if step is None:
            kernel = "IB_6"
            geom, X, idx, xs, _ = old
            F = np.random.default_rng(8).standard_normal((X.shape[0], 2))
        else:
            kernel = step[2]
            cs = c2.case(*step)
            geom, X, idx, xs, F = dev_geom(le, cs.geom), cs.X, cs.idx, cs.xshift, cs.F
        Xd, idd, xsd, Fd = (torch.from_numpy(a).to(DEV) for a in (X, idx, xs, F))
        m.bin(geom, kernel, Xd, idd, xsd)
        fresh = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
        assert torch.equal(m.order(), fresh.order())
        _same(_interp_spread(le, ctx, m, kernel, geom, Xd, Fd, 20 + n),
              _interp_spread(le, ctx, fresh, kernel, geom, Xd, Fd, 20 + n), f"step {n} ({kernel})")
    ctx.synchronize()


# --------------------------------------------------------------------------
# empty regions
# --------------------------------------------------------------------------
def test_empty_regions_stay_untouched(le, ctx, oracle):
    """Every marker inside one super-brick of `big`: the 59 other work items have no
    candidates and write nothing -- each point outside that super-brick keeps its value bit
    for bit -- and the super-brick's points match the oracle."""
    kernel = "IB_4"
    cs = c2.one_super_brick(c2.geometry("big", kernel), 9)
    g = cs.geom
    geom = dev_geom(le, g)
    HI = c2.KINFO[kernel][2]
    Xd = torch.from_numpy(cs.X).to(DEV)
    m = le.Markers(ctx).bin(geom, kernel, Xd)
    const = 1.2345678901234567
    q = geom.alloc("side", fill=const)
    le.spread(ctx, m, kernel, "side", geom, q, torch.from_numpy(cs.F).to(DEV), Xd)
    ctx.synchronize()
    order = m.order().cpu().numpy()
    uo = [np.full(tuple(a.shape), const) for a in q]
    oracle.side_spread(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, uo, cs.idx[order],
                       cs.xshift, cs.X, cs.F)
    # super-brick (1, 1): key cells rel [32, 64), array indices rel - HI (array lower = kmin + HI)
    win = slice(c2.SB - HI, 2 * c2.SB - HI)
    for a in range(2):
        got = q[a].cpu().numpy()
        outside = np.ones(got.shape, bool)
        outside[win, win] = False
        assert (uo[a][outside] == const).all(), "the markers' stencils stay inside the super-brick"
        assert (got[outside] == const).all(), f"comp {a}: a point outside the markers' reach was written"
        assert (uo[a][win, win] != const).sum() > 500
        assert rel_err(got, uo[a]) <= SPREAD_TOL
    ctx.synchronize()

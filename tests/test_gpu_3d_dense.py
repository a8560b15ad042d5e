"""GPU: the 3-D column sweeps (le_sweep.hip) for every kernel at sizes where their loops repeat.

Every other all-kernel 3-D test runs make_case's 13x14x15 patch (2 x 2 real columns, 263
listed markers); the larger 3-D tests that reach the oracle run IB_4, IB_6 or BSPLINE_4 on
a periodic unit box.  There the middle-chunk loops of k_spread_sweep, the dense-group loop
of k_interp_sweep, the candidate ranges of a column with real neighbours on every side and
the early return of a column inside the patch box never run for most kernels.  The cases of
tests/cases3d.py make them run (tests/test_cases3d_cpu.py asserts that they do); here the
kernels are compared with the oracle on them: interp bit for bit (interp_marker sums in the
Fortran order), spread within the project's 1e-12 both in the library's order and in the
caller's.  Every test ends with ctx.synchronize(), which raises on the device invariant
flags.
"""
import functools

import numpy as np
import pytest

import cases3d as c3

torch = pytest.importorskip("torch")

from test_gpu_fused import _fill  # noqa: E402
from test_gpu_parity import INTERP_TOL, SPREAD_TOL, oracle_call, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEPTH = {"side": 1, "cell": 2, "node": 1, "edge": 1}
# (kernel, centering) whose 3-D interp is not bitwise the oracle's on make_case's small
# input either, with the cause; held to INTERP_TOL.  Empty: every one is bitwise there.
NOT_BITWISE = {}


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


def dev_geom(le, g):
    return le.Geometry(list(g.ilower), list(g.iupper), g.g, list(g.dx), list(g.x_lower))


@functools.lru_cache(maxsize=2)
def dev_case(name, kind, kernel, extra=0):
    """The case and its X, list and shifts on the device, built once; left unchanged."""
    cs = c3.case(name, kind, kernel, extra)
    return cs, tuple(torch.from_numpy(a).to(DEV) for a in (cs.X, cs.idx, cs.xshift))


def random_arrays(geom, centering, depth, seed):
    rng = np.random.default_rng(seed)
    q = geom.alloc(centering, depth)
    for a in q:
        a.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(a.shape))))
    return q, [a.cpu().numpy().copy() for a in q]


def set_arrays(geom, centering, depth, u0):
    q = geom.alloc(centering, depth)
    for a, b in zip(q, u0):
        a.copy_(torch.from_numpy(b))
    return q


def q_depth_of(centering, depth):
    return 3 if centering in ("side", "edge") else depth


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
    for d in range(3):
        far |= (Xs[:, d] < g.x_lower[d] - 16 * g.dx[d]) | (Xs[:, d] > g.x_lower[d] + g.L[d] + 16 * g.dx[d])
    return cs.idx[far]


def check_interp(Qg, Qo, cs, kernel, centering, what):
    listed = np.zeros(cs.X.shape[0], bool)
    listed[cs.idx] = True
    assert np.isnan(Qg[~listed]).all(), f"{what}: unlisted markers must be untouched"
    assert not np.isnan(Qo[listed]).any()
    err = rel_err(Qg[listed], Qo[listed])
    bitwise = np.array_equal(Qg[listed], Qo[listed])
    print(f"{what}: interp rel err {err:.2e} bitwise={bitwise}")
    assert err <= INTERP_TOL
    if (kernel, centering) not in NOT_BITWISE:
        assert bitwise, f"{what}: interp is not bitwise the oracle's"
    far = far_outside(cs)
    if cs.xshift.any():
        assert far.size > 100 and (far < 5).any(), "the case has far-outside markers"
    assert (Qg[far] == 0.0).all(), f"{what}: far-outside markers read 0"


def check_spread(oracle, le_order, ug, u0, kernel, centering, geom, cs, Fv, depth, what):
    """ug against the oracle's spread of Fv into u0, in the library's order and the caller's."""
    assert np.array_equal(np.sort(le_order), np.arange(cs.idx.size)), "m.order() is a permutation of the list"
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
    return uo


def run_parity(le, ctx, oracle, case, centering):
    name, kind, kernel, extra = case
    cs, (Xd, idd, xsd) = dev_case(name, kind, kernel, extra)
    geom = dev_geom(le, cs.geom)
    depth = DEPTH[centering]
    what = f"{name} {kind} {kernel} {centering}"
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    assert m.count() == cs.idx.size
    # interp into NaN-filled Q
    q, u0 = random_arrays(geom, centering, depth, 11)
    Q = gpu_interp(le, ctx, m, kernel, centering, geom, q, depth, Xd)
    ctx.synchronize()
    check_interp(Q.cpu().numpy(), oracle_interp(oracle, kernel, centering, geom, u0, cs, depth), cs, kernel, centering,
                 what)
    # spread into a random, non-zero u
    q, u0 = random_arrays(geom, centering, depth, 12)
    Fv = marker_values(cs.F, centering, depth)
    le.spread(ctx, m, kernel, centering, geom, q, torch.from_numpy(Fv).to(DEV), Xd, q_depth=depth)
    ctx.synchronize()
    check_spread(oracle, m.order().cpu().numpy(), [a.cpu().numpy() for a in q], u0, kernel, centering, geom, cs, Fv,
                 depth, what)
    ctx.synchronize()


# --------------------------------------------------------------------------
# 1, 2: uniform, every kernel and centering
# --------------------------------------------------------------------------
@pytest.mark.parametrize("centering", ["side", "cell", "node", "edge"])
@pytest.mark.parametrize("kernel", c3.ALL)
def test_wide_uniform(le, ctx, oracle, kernel, centering):
    """3-4 real columns each way: a column with real neighbours on every side and one inside
    the patch box; (column, anchor)s of more than six chunks of candidates, groups of four
    planes that give every wave of the interp more than four chunks."""
    run_parity(le, ctx, oracle, ("wide", "uniform", kernel, 0), centering)


@pytest.mark.parametrize("case", [c for c in c3.GPU_CASES if c[0] == "tall"], ids=lambda c: c[2])
def test_tall_uniform(le, ctx, oracle, case):
    """More rows than columns: the x/y swap of the column index."""
    run_parity(le, ctx, oracle, case, "side")


# --------------------------------------------------------------------------
# 3: cluster -- thousands of candidates in one (column, anchor), sent to the same points
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", c3.PATHS)
def test_cluster_interp(le, ctx, oracle, kernel):
    cs, (Xd, _, _) = dev_case("wide", "cluster", kernel)
    geom = dev_geom(le, cs.geom)
    m = le.Markers(ctx).bin(geom, kernel, Xd)
    q, u0 = random_arrays(geom, "side", 1, 13)
    Q = gpu_interp(le, ctx, m, kernel, "side", geom, q, 1, Xd)
    ctx.synchronize()
    check_interp(Q.cpu().numpy(), oracle_interp(oracle, kernel, "side", geom, u0, cs, 1), cs, kernel, "side",
                 f"cluster {kernel}")
    ctx.synchronize()


@pytest.mark.parametrize("kernel", c3.PATHS)
def test_cluster_spread(le, ctx, oracle, kernel):
    """4 000 markers in the corner cell of a column, candidates of four columns: an anchor
    of more than 60 chunks in each, and a heavy item.  Within tolerance of the oracle in
    both orders, and the same order and bits from a second Markers and a second run."""
    cs, (Xd, _, _) = dev_case("wide", "cluster", kernel)
    geom = dev_geom(le, cs.geom)
    Fd = torch.from_numpy(cs.F).to(DEV)
    _, u0 = random_arrays(geom, "side", 1, 14)
    runs = []
    for rep in range(2):
        m = le.Markers(ctx).bin(geom, kernel, Xd)
        q = set_arrays(geom, "side", 1, u0)
        le.spread(ctx, m, kernel, "side", geom, q, Fd, Xd)
        ctx.synchronize()
        runs.append((m.order(), q))
    check_spread(oracle, runs[0][0].cpu().numpy(), [a.cpu().numpy() for a in runs[0][1]], u0, kernel, "side", geom, cs,
                 cs.F, 1, f"cluster {kernel}")
    assert torch.equal(runs[0][0], runs[1][0])
    for a in range(3):
        assert torch.equal(runs[0][1][a], runs[1][1][a]), f"comp {a}: a second Markers and run give other bits"
    ctx.synchronize()


# --------------------------------------------------------------------------
# 4: segment settings
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", c3.PATHS)
def test_deep_segments(le, oracle, kernel):
    """About a hundred anchor planes in segments of 8 (the default for so few columns), of
    at most 32 (100000), in three segments (64) and as one segment whose ring wraps ten to
    twenty times (1; cases3d.segments restates the rule): interp bitwise the oracle's under
    each, spread within tolerance under each and bit-stable on a repeat."""
    cs, (Xd, idd, xsd) = dev_case("deep", "uniform", kernel)
    geom = dev_geom(le, cs.geom)
    Fd = torch.from_numpy(cs.F).to(DEV)
    q, u0 = random_arrays(geom, "side", 1, 15)
    Qo = oracle_interp(oracle, kernel, "side", geom, u0, cs, 1)
    order0 = uo = None
    for seg_items in (None, 100000, 64, 1):
        what = f"deep {kernel} seg_items={seg_items}"
        c = le.Context(0)
        if seg_items is not None:
            c.tune("seg_items", seg_items)
        m = le.Markers(c).bin(geom, kernel, Xd, idd, xsd)
        Q = gpu_interp(le, c, m, kernel, "side", geom, q, 1, Xd)
        runs = []
        for rep in range(2):
            f = set_arrays(geom, "side", 1, u0)
            le.spread(c, m, kernel, "side", geom, f, Fd, Xd)
            runs.append(f)
        c.synchronize()
        check_interp(Q.cpu().numpy(), Qo, cs, kernel, "side", what)
        for a in range(3):
            assert torch.equal(runs[0][a], runs[1][a]), f"{what}: comp {a} differs on a repeat"
        order = m.order()
        if uo is None:  # the oracle in the binned order, the same under every setting
            order0 = order
            uo = check_spread(oracle, order.cpu().numpy(), [a.cpu().numpy() for a in runs[0]], u0, kernel, "side", geom,
                              cs, cs.F, 1, what)
        else:
            assert torch.equal(order, order0)
            for a in range(3):
                err = rel_err(runs[0][a].cpu().numpy(), uo[a])
                print(f"{what} comp {a}: spread rel err {err:.2e}")
                assert err <= SPREAD_TOL, f"{what}: spread comp {a} rel err {err:.3e}"
        c.synchronize()


# --------------------------------------------------------------------------
# 5: fused ghost operations at a size with a column inside the patch box
# --------------------------------------------------------------------------
@pytest.mark.parametrize("centering", ["side", "cell"])
@pytest.mark.parametrize("kernel", c3.PATHS)
def test_fused_zero_spread(le, ctx, kernel, centering):
    """zero_ghosts_spread = zero_ghosts + spread and zero_spread = zero + spread, bit for
    bit; the fused calls' arrays start with NaN ghosts, or NaN everywhere.  Markers in the
    lower 45 % of the patch: the last segment owns ghost planes and has no candidates, and a
    segment below it lies inside the patch box in z and has none either -- in a column
    inside the box in x and y that item owns no ghost point and must leave its points."""
    cs, (Xd, idd, xsd) = dev_case("half", "lower_half", kernel)
    geom = dev_geom(le, cs.geom)
    depth = DEPTH[centering]
    F = torch.from_numpy(marker_values(cs.F, centering, depth)).to(DEV)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    rng = np.random.default_rng(31)
    qa = geom.alloc(centering, depth)
    _fill(qa, geom, centering, rng)  # random values, NaN ghosts
    qb = [a.clone() for a in qa]
    le.zero_ghosts(ctx, geom, centering, qa, q_depth=depth)
    le.spread(ctx, m, kernel, centering, geom, qa, F, Xd, q_depth=depth)
    le.zero_ghosts_spread(ctx, m, kernel, centering, geom, qb, F, Xd, q_depth=depth)
    ctx.synchronize()
    for a, b in zip(qa, qb):
        assert not torch.isnan(b).any(), "zero_ghosts_spread: a ghost point was left unwritten"
        assert torch.equal(a, b), "zero_ghosts_spread"
    qa = geom.alloc(centering, depth)
    qb = geom.alloc(centering, depth, fill=np.nan)
    le.spread(ctx, m, kernel, centering, geom, qa, F, Xd, q_depth=depth)
    le.zero_spread(ctx, m, kernel, centering, geom, qb, F, Xd, q_depth=depth)
    ctx.synchronize()
    for a, b in zip(qa, qb):
        assert not torch.isnan(b).any(), "zero_spread: a point was left unwritten"
        assert torch.equal(a, b), "zero_spread"
        assert bool((a != 0).any())
    ctx.synchronize()


@pytest.mark.parametrize("kernel", c3.FILL_KERNELS)
def test_fused_fill_interp(le, ctx, kernel):
    """fill_interp = fill_periodic_ghosts + interp on the periodic unit box: Q bit for bit,
    no ghost value read (they are NaN in the fused call's arrays) and no point written."""
    cs, (Xd, idd, xsd) = dev_case("wide_unit", "uniform", kernel)
    geom = dev_geom(le, cs.geom)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    rng = np.random.default_rng(41)
    qb = geom.alloc("side")
    _fill(qb, geom, "side", rng)  # random values, NaN ghosts
    qa = [torch.nan_to_num(b, nan=0.0) for b in qb]
    q_before = [b.clone() for b in qb]
    Qa = torch.full((cs.X.shape[0], 3), np.nan, dtype=torch.float64, device=DEV)
    Qb = torch.full_like(Qa, np.nan)
    le.fill_periodic_ghosts(ctx, geom, "side", qa, periodic=[1, 1, 1])
    le.interp(ctx, m, kernel, "side", geom, qa, Qa, Xd)
    le.fill_interp(ctx, m, kernel, "side", geom, qb, Qb, Xd, periodic=[1, 1, 1])
    ctx.synchronize()
    listed = np.zeros(cs.X.shape[0], bool)
    listed[cs.idx] = True
    a, b = Qa.cpu().numpy(), Qb.cpu().numpy()
    assert np.isnan(b[~listed]).all() and not np.isnan(a[listed]).any()
    assert np.array_equal(a[listed], b[listed]), f"max diff {np.nanmax(np.abs(a[listed] - b[listed]))}"
    assert np.abs(a[listed]).max() > 0
    for b0, b1 in zip(q_before, qb):  # nothing written
        assert torch.equal(torch.nan_to_num(b0, nan=7.0), torch.nan_to_num(b1, nan=7.0))
        assert torch.equal(torch.isnan(b0), torch.isnan(b1))
    ctx.synchronize()


# --------------------------------------------------------------------------
# 6: rebin
# --------------------------------------------------------------------------
def _interp_spread(le, ctx, m, kernel, geom, Xd, Fd, u0):
    q = set_arrays(geom, "side", 1, u0)
    Q = gpu_interp(le, ctx, m, kernel, "side", geom, q, 1, Xd)
    le.spread(ctx, m, kernel, "side", geom, q, Fd, Xd)
    ctx.synchronize()
    return Q, q


@pytest.mark.parametrize("kernel", c3.ALL)
def test_rebin(le, ctx, oracle, kernel):
    """Every marker moved by up to 0.4 cell per dim: the re-binned list has the order of a
    fresh binning and gives the same interp and spread bits; its spread matches the oracle."""
    cs, (Xd, idd, xsd) = dev_case("wide", "uniform", kernel)
    geom = dev_geom(le, cs.geom)
    Fd = torch.from_numpy(cs.F).to(DEV)
    _, u0 = random_arrays(geom, "side", 1, 16)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    _interp_spread(le, ctx, m, kernel, geom, Xd, Fd, u0)  # the candidate stream exists
    order1 = m.order()
    X2n = cs.X + np.random.default_rng(6).uniform(-0.4, 0.4, cs.X.shape) * np.array(cs.geom.dx)
    X2 = torch.from_numpy(X2n).to(DEV)
    m.rebin(X2)
    fresh = le.Markers(ctx).bin(geom, kernel, X2, idd, xsd)
    assert m.count() == fresh.count() == cs.idx.size
    order2 = m.order()
    assert torch.equal(order2, fresh.order())
    assert not torch.equal(order1, order2), "the move changes the order"
    Qf, qf = _interp_spread(le, ctx, fresh, kernel, geom, X2, Fd, u0)
    Qm, qm = _interp_spread(le, ctx, m, kernel, geom, X2, Fd, u0)
    assert torch.equal(torch.isnan(Qm), torch.isnan(Qf)), "interp rows written"
    assert torch.equal(torch.nan_to_num(Qm, nan=-7.0), torch.nan_to_num(Qf, nan=-7.0)), "interp after rebin"
    for a in range(3):
        assert torch.equal(qm[a], qf[a]), f"spread comp {a} after rebin"
    cs2 = cs._replace(X=X2n)
    check_spread(oracle, order2.cpu().numpy(), [a.cpu().numpy() for a in qm], u0, kernel, "side", geom, cs2, cs.F, 1,
                 f"rebin {kernel}")
    ctx.synchronize()


# --------------------------------------------------------------------------
# 7: the two ways F reaches the spread
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["IB_4_W8", "IB_3", "PIECEWISE_CONSTANT", "DISCONTINUOUS_LINEAR", "BSPLINE_4"])
def test_f_stream_modes(le, kernel):
    """F gathered into sorted order before the sweep (f_stream -1) against F read at its
    marker row through the candidate stream (1): every array bit-equal."""
    cs, (Xd, idd, xsd) = dev_case("wide", "uniform", kernel)
    geom = dev_geom(le, cs.geom)
    Fd = torch.from_numpy(cs.F).to(DEV)
    _, u0 = random_arrays(geom, "side", 1, 17)
    outs = {}
    for mode in (-1, 1):
        c = le.Context(0)
        c.tune("f_stream", mode)
        m = le.Markers(c).bin(geom, kernel, Xd, idd, xsd)
        q = set_arrays(geom, "side", 1, u0)
        le.spread(c, m, kernel, "side", geom, q, Fd, Xd)
        c.synchronize()
        outs[mode] = q
    for a in range(3):
        assert not torch.equal(outs[1][a], torch.from_numpy(u0[a]).to(DEV)), "the spread reaches the array"
        assert torch.equal(outs[-1][a], outs[1][a]), f"comp {a}: the stream's F differs from the gathered F"


# --------------------------------------------------------------------------
# the binning itself
# --------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in c3.GPU_CASES if c[:2] in (("wide", "uniform"), ("tall", "uniform"))],
                         ids=lambda c: f"{c[0]}-{c[2]}")
def test_order_is_the_restated_bucket_order(le, ctx, case):
    """m.order() is the stable sort of the list by cases3d.bucket_keys, entry for entry:
    the key anchor of every family, the column grid (its origin moved to the arrays' first
    x index + a multiple of 16, ncx != ncy) and the bands, and with them the column grid
    that cases3d.structure counts on."""
    name, kind, kernel, extra = case
    cs, (Xd, idd, xsd) = dev_case(name, kind, kernel, extra)
    m = le.Markers(ctx).bin(dev_geom(le, cs.geom), kernel, Xd, idd, xsd)
    key, _, inside = c3.bucket_keys(cs.geom, cs.X, cs.idx, cs.xshift)
    assert inside.sum() > 0.8 * cs.idx.size and (~inside).sum() > 1000
    want = np.argsort(key, kind="stable")
    got = m.order().cpu().numpy()
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} entries differ"
    ctx.synchronize()

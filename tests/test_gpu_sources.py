"""GPU: the fluid-source stages (ibamr_amd.sources) against the numpy restatement
tests/source_ref.py -- which tests/test_sources_cpu.py holds to 50-digit known answers -- on
the cases of tests/source_cases.py: a 24 x 20 x 18 patch with a shifted lower corner, packed
and pitched, and its 2-D twin; radii that clamp to two cells, differ per dimension and hit the
rounding tie; sources on cell centres, on cell faces, overlapping, cut by two patch faces,
seventy at once, none.

Locations: equal to source_ref bit for bit.

Spread: |q_dev - q_ref| <= (3 C_w + 2 (n_i - 1) + 4) 2^-53 S_i per cell, n_i sources covering
the cell, S_i the sum of their |Q_n| / (r0 r1 r2), both from source_ref, and C_w =
8 max(ref_err_w, 1) from the committed known answers (the host cos and the device cos are each
a few ulp from exact; 8 is the margin the IMP update and stress tests give a device function).
Everything outside the patch box -- ghosts, row padding -- and every cell no box covers is
compared bit for bit.

Measured on an MI355X, worst |diff| / bound over all cases: spread 0.0044, pressure 0.00022
(C_w = 69.0 from ref_err_w = 8.63).

Normalize: the integrals within (N_cells + 4) 2^-53 sum |q dV| of source_ref's serial sums, q_norm
within that over vol plus two roundings; the boundary cells move by exactly the q_norm read back.
Pressure: the spread bound's analogue, m cells of the clipped box and sum |p| over them.
"""
import math
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import source_cases as sc  # noqa: E402
import source_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KAT = Path(__file__).resolve().parent / "golden" / "source_kat.npz"
U = 2.0 ** -53


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def sources(le):
    from ibamr_amd import sources as _s
    return _s


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


@pytest.fixture(scope="module")
def C_w():
    return 8.0 * max(float(np.load(KAT)["ref_err_w"]), 1.0)


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to(DEV)  # (a copy: the cases' arrays are read-only)


def make_geom(le, c):
    geo = c["geo"]
    geom = le.Geometry(list(geo.ilower), list(geo.iupper), geo.g, list(geo.dx), list(geo.x_lower))
    return geom.aligned() if c["pitched"] else geom


def span(t):
    """The whole allocation under a (possibly pitched) array, as a flat view."""
    size = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return torch.as_strided(t, (size,), (1,))


def field(geom, geo, values):
    """The cell array of geom: a per-element sentinel over the whole allocation (ghosts and row
    padding included), `values` (a ghost-box array) in the patch box."""
    t = geom.alloc("cell")[0]
    flat = span(t)
    flat.copy_(torch.from_numpy(-(3.0e5 + np.arange(flat.numel(), dtype=np.float64))))
    box = (0,) + geo.box_slices()
    t[box] = dev(values[geo.box_slices()])
    return t


def image(t):
    """(flat copy of the allocation, a view of it shaped as the ghost-box array)."""
    flat = span(t).cpu().numpy().copy()
    return flat, np.lib.stride_tricks.as_strided(flat, tuple(t.shape[1:]), tuple(8 * s for s in t.stride()[1:]))


def plan(sources, ctx, c):
    n = len(c["Q"])
    return sources.Sources(ctx, (c["r_src"], np.zeros(0, np.int32), np.zeros(0, np.int32)), ndim=c["geo"].ndim, n_nodes=0), n


def ratio(diff, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))


# ---- 1. locations ---------------------------------------------------------------------------------

@pytest.mark.parametrize("nd", [3, 2])
def test_locations_bit_for_bit(sources, ctx, nd):
    X, node, source, n_src = sc.node_lists(nd)
    want = sr.locations(X, node, source, n_src)
    s = sources.Sources(ctx, (np.full(n_src, 0.1), node, source), ndim=nd, n_nodes=X.shape[0])
    out = torch.full((n_src, nd), -7.25, dtype=torch.float64, device=DEV)
    got = s.locations(dev(X), out=out).cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert (got[2] == 0.0).all()  # the source without a node
    ctx.synchronize()


# ---- 2., 7. spread ----------------------------------------------------------------------------------

def run_spread(le, sources, ctx, name, start="q0"):
    c = sc.case(name)
    geo = c["geo"]
    geom = make_geom(le, c)
    s, n = plan(sources, ctx, c)
    q = field(geom, geo, c[start] if start else geo.alloc())
    before, _ = image(q)
    s.spread(geom, q, dev(c["X_src"].reshape(n, geo.ndim)), dev(c["Q"]))
    return c, geo, q, before


@pytest.mark.parametrize("name", sc.CASES)
def test_spread(le, sources, ctx, C_w, name):
    c, geo, q, before = run_spread(le, sources, ctx, name)
    flat, view = image(q)
    box = geo.box_slices()
    got = view[box].copy()
    bound = sc.spread_bound(c["cnt"][box], c["S"][box], C_w)
    diff = np.abs(got - c["q"][box])
    r = ratio(diff, bound)
    print(f"{name}: worst |q_dev - q_ref| / bound = {r.max():.4f} (C_w = {C_w:.1f})")
    assert (diff <= bound).all(), f"{name}: worst |diff| / bound = {r.max():.3f}"
    # a cell no clipped box covers is as it was, bit for bit
    free = c["cnt"][box] == 0
    assert np.array_equal(got[free].view(np.int64), c["q0"][box][free].view(np.int64))
    if len(c["Q"]):
        assert (~free).any() and free.any()
    # and so is every element outside the patch box: ghosts, row padding
    view[box] = 0.0
    bview = np.lib.stride_tricks.as_strided(before, view.shape, view.strides)
    bview[box] = 0.0
    assert np.array_equal(flat.view(np.int64), before.view(np.int64)), f"{name}: wrote outside the patch box"
    ctx.synchronize()


# ---- 3. determinism ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["main", "clip", "many_pitched", "many2"])
def test_spread_is_bitwise_repeatable(le, sources, ctx, name):
    a = image(run_spread(le, sources, ctx, name)[2])[0]
    b = image(run_spread(le, sources, ctx, name)[2])[0]
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    ctx.synchronize()


# ---- 4., 7. normalize -------------------------------------------------------------------------------

def check_normalize(le, sources, ctx, name):
    c = sc.case(name)
    geo = c["geo"]
    geom = make_geom(le, c)
    s, n = plan(sources, ctx, c)
    q = field(geom, geo, c["q_zero"])  # the restatement's spread: both sides integrate the same field
    before, bview = image(q)
    totals = s.normalize(geom, q, dev(c["Q"]), c["domain"], normalize=True)
    got = totals.cpu().numpy()  # (a copy on the stream: the call itself has finished without a fault)
    want = c["totals"]
    box = geo.box_slices()
    dV, N = geo.dV(), int(np.prod(geo.n))
    b_int = (N + 4) * U * float(np.abs(c["q_zero"][box] * dV).sum())
    vol = float(sr.bdry_count(geo.ndim, c["domain"])) * float(np.prod(geo.dx))
    print(f"{name}: q_total {got[0]!r} (ref {want[0]!r}, bound {b_int:.2e}), Q_sum {got[1]!r}, q_norm {got[2]!r} "
          f"(ref {want[2]!r}), integral after {got[3]:.3e}")
    assert abs(got[0] - want[0]) <= b_int
    assert abs(got[1] - want[1]) <= (n + 4) * U * float(np.abs(c["Q"]).sum())
    assert abs(got[2] - want[2]) <= b_int / vol + 2 * U * abs(want[2])
    # the boundary cells changed by exactly q_norm as read back; every other element is as it was
    flat, view = image(q)
    mask = np.zeros(geo.shape(), bool)
    mask[box] = True
    mask &= sr.bdry_mask(geo, c["domain"])
    assert mask.any() and not mask[box].all()
    assert np.array_equal(view[mask].view(np.int64), (bview[mask] + got[2]).view(np.int64))
    view[mask] = 0.0
    bview[mask] = 0.0
    assert np.array_equal(flat.view(np.int64), before.view(np.int64))
    nb = int(mask.sum())
    b_after = (N + 4) * U * float(np.abs(c["q_norm"][box] * dV).sum()) + nb * dV * abs(got[2] - want[2])
    assert abs(got[3] - want[3]) <= b_after
    return c, s, geom, q


@pytest.mark.parametrize("name", sc.UNCLIPPED)
def test_normalize_unclipped_leaves_the_flags_clear(le, sources, ctx, name):
    c = sc.case(name)
    geo = c["geo"]
    geom = make_geom(le, c)
    # without the normalisation the field is only read
    s, n = plan(sources, ctx, c)
    q = field(geom, geo, c["q_zero"])
    before = image(q)[0]
    t = s.normalize(geom, q, dev(c["Q"]), None, normalize=False).cpu().numpy()
    assert np.array_equal(image(q)[0].view(np.int64), before.view(np.int64))
    assert t[2] == 0.0 and t[3] == t[0] and t[1] == c["totals"][1] and n > 0
    check_normalize(le, sources, ctx, name)
    assert not c["flagged"]
    ctx.synchronize()  # raises if either call latched a flag


@pytest.mark.parametrize("name", sc.CLIPPED)
def test_normalize_clipped_source_latches_the_flag(le, sources, ctx, name):
    from ibamr_amd._lib import IBTKLEError
    ctx.synchronize()
    c, s, geom, q = check_normalize(le, sources, ctx, name)  # returns: the kernels finished, nothing aborted
    assert c["flagged"]
    with pytest.raises(IBTKLEError) as e:
        ctx.synchronize()
    assert e.value.code == 8 and "(flag 32)" in str(e.value)
    ctx.synchronize()  # reported once, then clear


# ---- 5., 7. pressure --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in sc.CASES if n != "none"])
def test_pressure(le, sources, ctx, C_w, name):
    c = sc.case(name)
    geo = c["geo"]
    geom = make_geom(le, c)
    s, n = plan(sources, ctx, c)
    p = field(geom, geo, c["p"])
    X_src = dev(c["X_src"])
    bound = sc.pressure_bound(c["P_cells"], c["P_abs"], C_w)
    got = s.pressure(geom, p, X_src).cpu().numpy()
    r = ratio(np.abs(got - c["P"]), bound)
    print(f"{name}: worst |P_dev - P_ref| / bound = {r.max():.5f}")
    assert (np.abs(got - c["P"]) <= bound).all()
    out = torch.full((n,), -7.25, dtype=torch.float64, device=DEV)
    gotn = s.pressure(geom, p, X_src, domain=c["domain_big"], out=out).cpu().numpy()
    rn = ratio(np.abs(gotn - c["P_normed"]), bound)
    print(f"{name}: with the normalisation pressure {c['p_norm']!r}: worst ratio {rn.max():.5f}")
    assert (np.abs(gotn - c["P_normed"]) <= bound).all()
    assert abs(c["p_norm"]) > 1e-3 and not np.array_equal(got, gotn)
    ctx.synchronize()


@pytest.mark.parametrize("name", ["main", "main_pitched", "main2"])
def test_pressure_of_a_constant_field(le, sources, ctx, name):
    c = sc.case(name)
    geo = c["geo"]
    geom = make_geom(le, c)
    s, n = plan(sources, ctx, c)
    p = field(geom, geo, np.full(geo.shape(), 3.25))
    got = s.pressure(geom, p, dev(c["X_src"])).cpu().numpy()
    assert np.abs(got - 3.25).max() <= 1e-13 * 3.25
    ctx.synchronize()


# ---- 6. adjointness ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["clip", "many_pitched", "clip2"])
def test_spread_and_pressure_are_adjoint(le, sources, ctx, name):
    c, geo, q, _ = run_spread(le, sources, ctx, name, start=None)
    geom = make_geom(le, c)
    s, n = plan(sources, ctx, c)
    p = field(geom, geo, c["p"])
    P = s.pressure(geom, p, dev(c["X_src"]))
    box = (0,) + geo.box_slices()
    lhs = math.fsum((q[box] * p[box]).cpu().numpy().ravel()) * geo.dV()
    rhs = math.fsum((dev(c["Q"]) * P).cpu().numpy())
    print(f"{name}: sum q p dV = {lhs!r}, sum Q P = {rhs!r}, relative difference {abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs) > 0.0 and abs(lhs - rhs) <= 1e-12 * abs(lhs)
    ctx.synchronize()


# ---- 8. end to end ----------------------------------------------------------------------------------

def test_deck_to_device(le, sources, ctx, tmp_path):
    from ibamr_amd import io
    X, node, source, n_src = sc.node_lists(3)
    nv = X.shape[0]
    radii = np.array([0.03, 0.2, 0.08, 0.12])
    io.write_source(tmp_path / "s.source", [f"source {k}" for k in range(n_src)], radii, node, source)
    specs = sources.SourceSpecs.from_deck(io.read_source(tmp_path / "s.source", nv), num_vertex=nv)
    assert specs.num_source == n_src and specs.names[3] == "source 3"
    plain = sources.Sources(ctx, specs).locations(dev(X)).cpu().numpy()
    assert np.array_equal(plain.view(np.int64), sr.locations(X, node, source, n_src).view(np.int64))
    # a seeded permutation of the nodes that keeps every source's nodes in their relative order
    perm = np.random.default_rng(5).permutation(nv)
    for k in range(n_src):
        mine = specs.node[specs.source == k]
        perm[mine] = np.sort(perm[mine])
    assert not np.array_equal(perm, np.arange(nv))
    Xp = np.empty_like(X)
    Xp[perm] = X
    s = sources.Sources(ctx, specs, perm=perm)
    got = s.locations(dev(Xp)).cpu().numpy()
    assert np.array_equal(got.view(np.int64), plain.view(np.int64))
    # and on through the spread: the located sources land in the 3-D patch, the calls run
    c = sc.case("main")
    geo = c["geo"]
    geom = make_geom(le, c)
    Xin = np.array(geo.x_lower) + (0.3 + 0.4 * (X + 1.0) / 3.0) * np.array(geo.n) * np.array(geo.dx)
    s2 = sources.Sources(ctx, specs)
    X_src = s2.locations(dev(Xin))
    Q = np.array([0.5, -1.0, 0.0, 2.0])
    q = field(geom, geo, geo.alloc())
    s2.spread(geom, q, X_src, dev(Q))
    want = sr.spread(geo, geo.alloc(), X_src.cpu().numpy(), radii, Q)
    got_q = image(q)[1][geo.box_slices()]
    assert np.abs(got_q - want[geo.box_slices()]).max() <= 1e-12 * np.abs(want).max() and np.abs(want).max() > 0
    ctx.synchronize()


# ---- argument errors that need a context ----------------------------------------------------------

def test_argument_errors(le, sources, ctx):
    from ibamr_amd._lib import IBTKLEError
    c = sc.case("main")
    geo = c["geo"]
    geom = make_geom(le, c)
    n = len(c["Q"])
    for bad in ((np.full(1, 0.1), [5], [0]), (np.full(1, 0.1), [0], [1]), (np.full(1, -0.1), [0], [0]),
                (np.full(1, 0.1), [0, 0], [0, 0])):
        with pytest.raises(IBTKLEError) as e:
            sources.Sources(ctx, bad, ndim=3, n_nodes=4)
        assert e.value.code == 4
    with pytest.raises(IBTKLEError):
        sources.Sources(ctx, (np.full(1, 0.1), [], []), ndim=4, n_nodes=0)
    # a radius beyond the tables: IBTK_LE_ERR_ARG, nothing written
    r = c["r_src"].copy()
    r[2] = 17.0 * geo.dx[1]
    s = sources.Sources(ctx, (r, [], []), ndim=3, n_nodes=0)
    q = field(geom, geo, c["q0"])
    before = image(q)[0]
    for call in (lambda: s.spread(geom, q, dev(c["X_src"]), dev(c["Q"])), lambda: s.pressure(geom, q, dev(c["X_src"]))):
        with pytest.raises(IBTKLEError) as e:
            call()
        assert e.value.code == 4 and "radius" in str(e.value)
    assert np.array_equal(image(q)[0].view(np.int64), before.view(np.int64))
    s, _ = plan(sources, ctx, c)
    g2 = make_geom(le, sc.case("main2"))
    with pytest.raises(ValueError):
        s.spread(g2, g2.alloc("cell")[0], dev(c["X_src"]), dev(c["Q"]))
    lib, P = ctx.lib, ctx.lib.ibtk_le_source_pressure
    qp = q.data_ptr()
    import ctypes
    lo_host = np.zeros(3, np.int32)
    lo = lo_host.ctypes.data
    assert lib.ibtk_le_source_spread(ctx.h, s.h, ctypes.byref(g2.c), qp, qp, qp) == 4   # a 2-D geometry, a 3-D plan
    assert P(ctx.h, s.h, ctypes.byref(geom.c), qp, qp, qp, lo, None) == 4               # one of dom_lo / dom_hi
    assert lib.ibtk_le_source_normalize(ctx.h, s.h, ctypes.byref(geom.c), qp, None, lo, qp, 1, qp) == 4
    assert lib.ibtk_le_source_spread(ctx.h, s.h, ctypes.byref(geom.c), None, qp, qp) == 4  # a null array
    bad = le.Geometry(list(geo.ilower), list(geo.iupper), geo.g, [geo.dx[0], float("nan"), geo.dx[2]], list(geo.x_lower))
    assert lib.ibtk_le_source_spread(ctx.h, s.h, ctypes.byref(bad.c), qp, qp, qp) == 4
    empty = le.Geometry(list(geo.ilower), [geo.ilower[0] - 1, geo.iupper[1], geo.iupper[2]], geo.g, list(geo.dx),
                        list(geo.x_lower))
    assert lib.ibtk_le_source_spread(ctx.h, s.h, ctypes.byref(empty.c), qp, qp, qp) == 0   # an empty box: nothing to do
    assert np.array_equal(image(q)[0].view(np.int64), before.view(np.int64))
    other = le.Context(0)
    assert lib.ibtk_le_source_locations(other.h, s.h, qp, qp) == 4  # the plan's own context only
    other.close()
    ctx.synchronize()

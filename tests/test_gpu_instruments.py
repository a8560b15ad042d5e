"""GPU: the flow meters and pressure gauges (ibamr_amd.instruments) against the scalar
restatement tests/instrument_ref.py -- which tests/test_instrument_cpu.py holds to exact known
answers -- on the cases of tests/instrument_cases.py, each packed and pitched with ghost width 1
and 3: meters of 3, 4, 17 and 70 perimeter nodes, planar and slightly non-planar, webs of 2, 4,
8, 14 and 16 nodes a spoke (1120 web patches for the largest), web centroids exactly on cell
faces and cell centres, a meter cut by two patch faces, a centroid outside the box, two meters
sharing cells, eight meters at once, none.

Everything is compared bit for bit: X_centroid, num_web_nodes, X_web, dA_web, cell, counted and
the three values of every meter, with u or p absent too.  A NaN equals a NaN (its sign and
payload are the processor's: 0.0 / 0.0 is a negative NaN on the host and a positive one on the
device); every other value must have the reference's bits.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import instrument_cases as ic  # noqa: E402
import instrument_ref as ir  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 8
SENTINEL = -7.25


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def inst(le):
    from ibamr_amd import instruments as _i
    return _i


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to(DEV)  # (a copy: the cases' arrays are read-only)


def same(got, want):
    """Bit for bit, a NaN equal to a NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)))


def make_geom(le, layout):
    g, pitched = ic.LAYOUTS[layout]
    geo = ic.GEO
    geom = le.Geometry(list(geo.ilower), list(geo.iupper), g, list(geo.dx), list(geo.x_lower))
    return geom.aligned() if pitched else geom


def span(t):
    """The whole allocation under a (possibly pitched) array, as a flat view."""
    size = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return torch.as_strided(t, (size,), (1,))


def load_fields(geom, u, p):
    """The side arrays and the cell array of geom holding u and p (ghost width 1 arrays) in
    their first ghost layer and inside, NaN in every other element of the allocation: the
    further ghost layers and the row padding."""
    k = geom.gcw[0] - 1
    ud = geom.alloc("side")
    pd = geom.alloc("cell")[0]
    for t, a in list(zip(ud, u)) + [(pd[0], p)]:
        span(t).fill_(float("nan"))
        n2, n1, n0 = a.shape
        t[k:k + n2, k:k + n1, k:k + n0] = dev(a)
    return ud, pd


def image(ts):
    return [span(t).cpu().numpy().copy() for t in ts]


def ref_arrays(c):
    """The restatement's webs as arrays, per meter."""
    out = []
    for w in c["webs"]:
        P, nw = w["P"], w["nw"]
        arr = lambda key, dt, width: np.array([w[key][m][n] for m in range(P) for n in range(nw)],  # noqa: E731
                                              dtype=dt).reshape((P, nw, width) if width else (P, nw))
        out.append(dict(X_web=arr("X_web", np.float64, 3), dA_web=arr("dA_web", np.float64, 3),
                        cell=arr("cell", np.int32, 3), counted=arr("counted", np.int32, 0)))
    return out


def run(le, inst, ctx, c, layout, cap=None, u=True, p=True, fields=None, perm=None, domain=None, h_finest=None):
    """Plan, update, read.  Returns (meters, values as a host array)."""
    geom = make_geom(le, layout)
    node, meter, meter_node = c["triples"]
    X, U = c["X"], c["U"]
    n_nodes = X.shape[0]
    if perm is not None:
        node = perm[node]
        Xp, Up = np.empty_like(X), np.empty_like(U)
        Xp[perm], Up[perm] = X, U
        X, U = Xp, Up
    mt = inst.Meters(ctx, (node, meter, meter_node), c["cap"] if cap is None else cap, n_nodes=n_nodes,
                     n_meters=len(c["names"]))
    fu, fp = fields if fields is not None else (c["u"], c["p"])
    ud, pd = load_fields(geom, fu, fp)
    Xd, Ud = dev(X), dev(U)
    before = image(ud + [pd, Xd, Ud])
    L = len(c["names"])
    buf = torch.full((3 * L + 2 * PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    out = buf[PAD:PAD + 3 * L]
    mt.update(geom, Xd, domain=domain, h_finest=h_finest)
    mt.read(geom, ud if u else None, pd if p else None, Ud, out=out)
    host = buf.cpu().numpy()
    # nothing beside values_dev is written; u, p, X and U keep their bits
    assert (host[:PAD] == SENTINEL).all() and (host[PAD + 3 * L:] == SENTINEL).all()
    for a, b in zip(before, image(ud + [pd, Xd, Ud])):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    return mt, host[PAD:PAD + 3 * L].reshape(L, 3).copy()


# ---- 1. against the restatement, bit for bit ------------------------------------------------------

@pytest.mark.parametrize("layout", ic.LAYOUTS)
@pytest.mark.parametrize("name", ic.CASES)
def test_bit_for_bit(le, inst, ctx, name, layout):
    c = ic.case(name)
    mt, values = run(le, inst, ctx, c, layout)
    webs = c["webs"]
    L = len(webs)
    assert same(values, c["values"]), (values, c["values"])
    if L:
        assert same(mt.X_centroid.cpu().numpy(), np.array([w["Xc"] for w in webs]))
        assert mt.num_web_nodes.cpu().numpy().tolist() == [w["nw"] for w in webs]
        cc = mt.centroid_cell.cpu().numpy()
        assert cc[:, :3].tolist() == [list(w["cen_cell"]) for w in webs] and cc[:, 3].tolist() == [int(w["cen_counted"]) for w in webs]
        for got, w in zip(mt.X_perimeter, webs):
            assert same(got.cpu().numpy(), np.array(w["Xp"]))
        want = ref_arrays(c)
        for key in ("X_web", "dA_web"):
            for l, got in enumerate(getattr(mt, key)):
                assert same(got.cpu().numpy(), want[l][key]), (key, c["names"][l])
        for key in ("cell", "counted"):
            for l, got in enumerate(getattr(mt, key)):
                assert np.array_equal(got.cpu().numpy(), want[l][key]), (key, c["names"][l])
    # without u: flow = 0 - correction; without p: NaN and 0
    assert same(run(le, inst, ctx, c, layout, u=False)[1], c["values_no_u"])
    assert same(run(le, inst, ctx, c, layout, p=False)[1], c["values_no_p"])
    ctx.synchronize()  # no flag: every web fits exactly


# ---- 2. determinism -------------------------------------------------------------------------------

@pytest.mark.parametrize("name, layout", [("eight", "pitched_g3"), ("wave", "packed_g1")])
def test_two_runs_are_equal_in_bits(le, inst, ctx, name, layout):
    c = ic.case(name)
    mt, a = run(le, inst, ctx, c, layout)
    Xa = [t.cpu().numpy() for t in mt.X_web]
    mt2, b = run(le, inst, ctx, c, layout)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    for x, t in zip(Xa, mt2.X_web):
        assert np.array_equal(x.view(np.int64), t.cpu().numpy().view(np.int64))
    # and a second update + read on the same plan
    geom = make_geom(le, layout)
    ud, pd = load_fields(geom, c["u"], c["p"])
    mt.update(geom, dev(c["X"]))
    again = mt.read(geom, ud, pd, dev(c["U"])).cpu().numpy()
    assert np.array_equal(a.view(np.int64), again.view(np.int64))
    ctx.synchronize()


# ---- 3. nothing else is read ----------------------------------------------------------------------

@pytest.mark.parametrize("name, layout", [("eight", "pitched_g3"), ("cut", "packed_g3"), ("outside", "packed_g1")])
def test_nan_outside_the_stencils_changes_nothing(le, inst, ctx, name, layout):
    """NaN in every ghost layer beyond the first (load_fields puts it there in every test) and
    in every element no counted web patch's or counted centroid's stencil reaches."""
    c = ic.case(name)
    tu, tp = c["touched"]
    assert all(t.any() and not t.all() for t in tu) and tp.any() and not tp.all()
    u = [np.where(t, a, np.nan) for t, a in zip(tu, c["u"])]
    p = np.where(tp, c["p"], np.nan)
    _, values = run(le, inst, ctx, c, layout, fields=(u, p))
    assert same(values, c["values"]) and not np.isnan(values[:, 0]).any()
    ctx.synchronize()


# ---- 4. capacity ------------------------------------------------------------------------------------

def test_capacity_below_a_web_latches_flag_64_once(le, inst, ctx):
    from ibamr_amd._lib import IBTKLEError
    ctx.synchronize()
    c = ic.case("eight")
    nw = [w["nw"] for w in c["webs"]]
    big = int(np.argmax(nw))
    assert nw[big] == c["cap"] and sorted(nw)[-2] <= c["cap"] - 2  # capacity nw - 2 drops that meter alone
    mt, values = run(le, inst, ctx, c, "pitched_g1", cap=c["cap"] - 2)
    assert np.isnan(values[big]).all()
    others = [l for l in range(len(nw)) if l != big]
    assert same(values[others], c["values"][others])
    assert mt.num_web_nodes.cpu().numpy().tolist() == nw
    webs = mt.X_web
    assert webs[big] is None
    want = ref_arrays(c)
    for l in others:
        assert same(webs[l].cpu().numpy(), want[l]["X_web"])
    with pytest.raises(IBTKLEError) as e:
        ctx.synchronize()
    assert e.value.code == 8 and "(flag 64)" in str(e.value)
    ctx.synchronize()  # reported once, then clear


# ---- 5. a renumbering, another frame, a deck --------------------------------------------------------

def test_renumbered_nodes(le, inst, ctx):
    c = ic.case("eight")
    perm = np.random.default_rng(5).permutation(c["X"].shape[0])
    assert not np.array_equal(perm, np.arange(perm.size))
    _, values = run(le, inst, ctx, c, "packed_g3", perm=perm)
    assert same(values, c["values"])
    ctx.synchronize()


def test_domain_frame_and_h_finest(le, inst, ctx):
    """A domain larger than the patch (getCellIndex measures from its nearer end) and a finer
    h_finest than the patch's own spacing."""
    c = ic.case("cut")
    geo = c["geo"]
    lo = [geo.ilower[0] - 4, geo.ilower[1] - 2, geo.ilower[2]]
    hi = [geo.iupper[0] + 30, geo.iupper[1] + 1, geo.iupper[2] + 7]
    domain = (lo, hi, [geo.x_lower[d] - (geo.ilower[d] - lo[d]) * geo.dx[d] for d in range(3)],
              [geo.x_upper[d] + (hi[d] - geo.iupper[d]) * geo.dx[d] for d in range(3)])
    h = 0.75 * ic.H
    webs = ir.update(geo, c["X"], c["meters"], domain=domain, h_finest=h)
    assert webs[0]["nw"] == 10 != c["webs"][0]["nw"]
    want, _ = ir.read(geo, webs, c["u"], c["p"], c["U"], c["meters"])
    mt, values = run(le, inst, ctx, c, "packed_g1", cap=10, domain=domain, h_finest=h)
    assert same(values, want)
    assert np.array_equal(mt.cell[0].cpu().numpy().reshape(-1, 3), np.array([x for row in webs[0]["cell"] for x in row]))
    assert np.array_equal(mt.counted[0].cpu().numpy().reshape(-1), np.array([int(x) for row in webs[0]["counted"] for x in row]))
    ctx.synchronize()


def test_deck_to_log(le, inst, ctx, tmp_path):
    from ibamr_amd import io
    c = ic.case("small")
    node, meter, meter_node = c["triples"]
    nv = c["X"].shape[0]
    io.write_inst(tmp_path / "m.inst", ["tri", "a quad"], node, meter, meter_node)
    specs = inst.MeterSpecs.from_deck(io.read_inst(tmp_path / "m.inst", nv), num_vertex=nv)
    perm = np.random.default_rng(9).permutation(nv)
    X, U = np.empty_like(c["X"]), np.empty_like(c["U"])
    X[perm], U[perm] = c["X"], c["U"]
    geom = make_geom(le, "pitched_g3")
    ud, pd = load_fields(geom, c["u"], c["p"])
    mt = inst.Meters(ctx, specs, c["cap"], perm=perm)
    mt.update(geom, dev(X))
    values = mt.read(geom, ud, pd, dev(U)).cpu().numpy()
    assert same(values, c["values"])
    Xc = mt.X_centroid.cpu().numpy()
    assert mt.log_lines(0.5, values, Xc) == specs.log_lines(0.5, c["values"], [w["Xc"] for w in c["webs"]])
    assert mt.log_lines(0.5, values, Xc)[1].startswith("a quad  5.00000e-01  ")
    mt.close()
    ctx.synchronize()


def test_zero_radius_meter(le, inst, ctx):
    geo = ic.GEO
    X = np.tile(np.array([[0.25, 1.0, 0.5]]), (4, 1))
    U = np.random.default_rng(3).standard_normal((4, 3))
    meters = [[0, 1, 2, 3]]
    webs = ir.update(geo, X, meters)
    u, p = ic.fields(0)
    want, _ = ir.read(geo, webs, u, p, U, meters)
    assert webs[0]["nw"] == 0 and np.isnan(want[0, 1]) and want[0, 2] != 0.0
    c = dict(triples=(np.arange(4, dtype=np.int32), np.zeros(4, np.int32), np.arange(4, dtype=np.int32)), X=X, U=U, u=u, p=p,
             names=("dot",), cap=2)
    mt, values = run(le, inst, ctx, c, "packed_g1")
    assert same(values, want) and mt.num_web_nodes.cpu().numpy().tolist() == [0]
    ctx.synchronize()


# ---- 6. argument errors: their codes, before anything is launched -------------------------------------

def test_argument_errors(le, inst, ctx):
    from ibamr_amd._lib import IBTKLEError
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    good = (i32(0, 1, 2), i32(0, 0, 0), i32(0, 1, 2))
    for bad, kw in (
        ((i32(0, 1, 5), good[1], good[2]), {}),                   # a node out of range
        ((good[0], i32(0, 0, 1), good[2]), {"n_meters": 1}),      # a meter out of range
        ((good[0], good[1], i32(0, 1, -1)), {}),                  # a negative node index
        ((good[0], good[1], i32(0, 1, 1)), {}),                   # a (meter, node index) pair named twice
        ((good[0], good[1], i32(0, 1, 3)), {}),                   # ... missing
        ((i32(0, 1, 1), good[1], good[2]), {}),                   # a local node named twice
        (good, {"cap": 3}), (good, {"cap": 0}), (good, {"cap": -2}),
        (good, {"cap": 2 * (inst.MAX_WEB // 3 // 2) + 2}),        # P max_web_nodes beyond the limit
        ((i32(), i32(), i32()), {"n_meters": 1}),                 # a meter without a node
    ):
        with pytest.raises(IBTKLEError) as e:
            inst.Meters(ctx, bad, kw.get("cap", 4), n_nodes=4, n_meters=kw.get("n_meters"))
        assert e.value.code == 4, bad
    inst.Meters(ctx, good, 2 * (inst.MAX_WEB // 3 // 2), n_nodes=4).close()  # the limit itself
    c = ic.case("small")
    geom = make_geom(le, "packed_g1")
    ud, pd = load_fields(geom, c["u"], c["p"])
    Xd, Ud = dev(c["X"]), dev(c["U"])
    out = torch.full((6,), SENTINEL, dtype=torch.float64, device=DEV)
    mt = inst.Meters(ctx, c["triples"], c["cap"], n_nodes=c["X"].shape[0])
    lib = ctx.lib
    up = (ctypes.c_void_p * 3)(*[a.data_ptr() for a in ud])
    args = (up, pd.data_ptr(), Ud.data_ptr(), out.data_ptr())
    assert lib.ibtk_le_meters_read(ctx.h, mt.h, ctypes.byref(geom.c), *args) == 4  # no update before it
    I3, D3 = ctypes.c_int * 3, ctypes.c_double * 3
    dom = (I3(*geom.ilower), I3(*geom.iupper), D3(*geom.x_lower), D3(*geom.x_upper))
    g2 = le.Geometry([0, 0], [7, 7], 2, [0.1, 0.1], [0.0, 0.0])
    assert lib.ibtk_le_meters_update(ctx.h, mt.h, ctypes.byref(g2.c), *dom, ic.H, Xd.data_ptr()) == 4   # 2-D
    assert "3-D" in lib.ibtk_le_last_error().decode()
    assert lib.ibtk_le_meters_update(ctx.h, mt.h, ctypes.byref(geom.c), None, dom[1], dom[2], dom[3], ic.H, Xd.data_ptr()) == 4
    assert lib.ibtk_le_meters_update(ctx.h, mt.h, ctypes.byref(geom.c), *dom, 0.0, Xd.data_ptr()) == 4
    assert lib.ibtk_le_meters_update(ctx.h, mt.h, ctypes.byref(geom.c), *dom, ic.H, None) == 4
    with pytest.raises(ValueError):
        mt.update(g2, Xd)
    mt.update(geom, Xd)
    g0 = le.Geometry(list(geom.ilower), list(geom.iupper), [1, 0, 1], list(geom.dx), list(geom.x_lower))
    assert lib.ibtk_le_meters_read(ctx.h, mt.h, ctypes.byref(g0.c), *args) == 2      # IBTK_LE_ERR_GHOST_WIDTH
    other_box = le.Geometry(list(geom.ilower), [v + 1 for v in geom.iupper], 1, list(geom.dx), list(geom.x_lower))
    assert lib.ibtk_le_meters_read(ctx.h, mt.h, ctypes.byref(other_box.c), *args) == 4  # not the update's box
    assert lib.ibtk_le_meters_read(ctx.h, mt.h, ctypes.byref(g2.c), *args) == 4
    assert lib.ibtk_le_meters_read(ctx.h, mt.h, ctypes.byref(geom.c), up, pd.data_ptr(), None, out.data_ptr()) == 4
    assert lib.ibtk_le_meters_read(ctx.h, mt.h, ctypes.byref(geom.c), up, pd.data_ptr(), Ud.data_ptr(), None) == 4
    bad_u = (ctypes.c_void_p * 3)(ud[0].data_ptr(), None, ud[2].data_ptr())
    assert lib.ibtk_le_meters_read(ctx.h, mt.h, ctypes.byref(geom.c), bad_u, *args[1:]) == 4
    assert lib.ibtk_le_meters_workspace(ctx.h, mt.h, 99, out.data_ptr(), 6) == 4
    assert lib.ibtk_le_meters_workspace(ctx.h, mt.h, 0, out.data_ptr(), 5) == 4
    other = le.Context(0)
    assert lib.ibtk_le_meters_read(other.h, mt.h, ctypes.byref(geom.c), *args) == 4  # the plan's own context only
    other.close()
    assert (out.cpu().numpy() == SENTINEL).all()  # nothing was launched
    empty = le.Geometry(list(geom.ilower), [geom.ilower[0] - 1, geom.iupper[1], geom.iupper[2]], 1, list(geom.dx),
                        list(geom.x_lower))
    assert lib.ibtk_le_meters_read(ctx.h, mt.h, ctypes.byref(empty.c), *args) == 0   # an empty box: nothing to do
    assert (out.cpu().numpy() == SENTINEL).all()
    assert same(mt.read(geom, ud, pd, Ud, out=out).cpu().numpy().reshape(2, 3), c["values"])  # and the plan still works
    ctx.synchronize()

"""GPU: the force Jacobian on the device (ibtk_le_forcejac_*, ibtk_le_forcegen_linearized,
ibtk_le_forcegen_jacobian_nnz; ibamr_amd.forcegen.ForceJacobian) against the serial
restatement of IBStandardForceGen::computeLagrangianForceJacobian (tests/forcejac_ref.py).

The pattern is compared exactly, the assembled values bit for bit (int64 views; a NaN equals
a NaN: the sign bit of 0 / 0 differs between an x86 host and the device); the products are
held to the standard bound for any summation order, |Y - J V| <= gamma_m sum |J_ij| |V_j|,
gamma_m = m u / (1 - m u), u = 2^-53, m the row's scalar term count, against a product taken
in numpy.longdouble.
"""
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from forcejac_ref import bsr_arrays, reference_jacobian, reference_nnz  # noqa: E402
from ibamr_amd import io  # noqa: E402
from ibamr_amd.forcegen import ForceSpecs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
U = 2.0 ** -53
X_COEF, U_COEF = 0.5, -0.25 / 3.0e-3  # not powers of two


def gamma(m):
    return m * U / (1.0 - m * U)


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


@pytest.fixture(scope="module")
def fgmod(le):
    from ibamr_amd import forcegen
    return forcegen


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


DECKS = {
    "curve2d_64": (2, {}),
    "sphere3d_32": (3, {"uniform_stiffness": 37.5}),
    "fila_256": (2, {"uniform_stiffness": 1.0e4, "uniform_bend_rigidity": 0.375,
                     "uniform_curvature": [1.0e-5, -2.0e-5], "uniform_target_stiffness": 5.0e3,
                     "uniform_target_damping": 0.75}),
}


def _deck_specs(name):
    ndim, uniform = DECKS[name]
    X0 = io.read_vertex(GOLDEN / "vertex" / f"{name}.vertex", ndim)
    nv = X0.shape[0]
    d = GOLDEN / "ibforce"
    pick = lambda *keys: {k: uniform[k] for k in keys if k in uniform}  # noqa: E731
    springs = beams = targets = None
    if (d / f"{name}.spring").exists():
        springs = io.read_spring(d / f"{name}.spring", nv, **pick("uniform_stiffness", "uniform_rest_length"))
    if (d / f"{name}.beam").exists():
        beams = io.read_beam(d / f"{name}.beam", nv, ndim, **pick("uniform_bend_rigidity", "uniform_curvature"))
    if (d / f"{name}.target").exists():
        targets = io.read_target(d / f"{name}.target", nv,
                                 **pick("uniform_target_stiffness", "uniform_target_damping"))
    return ForceSpecs(ndim, X0, springs, beams, targets)


def _deck_case(name):
    sp = _deck_specs(name)
    a = sp.arrays()
    rng = np.random.default_rng(len(name))
    X = sp.X0 + 1e-3 * rng.standard_normal((sp.num_vertex, sp.ndim))
    return dict(n=sp.num_vertex, nd=sp.ndim, X=X, springs=a["springs"], beams=a["beams"], targets=a["targets"],
                dX=None)


def _synthetic(with_dX=False, coincident=False):
    """1000 nodes; 5000 springs: random ones with 49 repeated edges and a hub (node 7) with 300
    springs, a row longer than a wave; 200 random beams, the first ten on a spring's node pair
    (master, next = that spring's ends), one with next == prev; a target point on every third
    node below 950; nodes 950.. isolated.  coincident: nodes 20 and 21 (joined by the last
    spring of the deck, before its shuffle) share a position."""
    rng = np.random.default_rng(2024)
    n, nd, live = 1000, 3, 950
    X = rng.random((n, nd))
    m = rng.integers(0, live, 4650)
    s = (m + rng.integers(1, live, 4650)) % live
    hub_other = rng.permutation(np.setdiff1d(np.arange(live), [7]))[:300]
    hub_m = np.where(np.arange(300) % 2 == 0, 7, hub_other)
    hub_s = np.where(np.arange(300) % 2 == 0, hub_other, 7)
    mastr = np.concatenate([m, m[:49], hub_m, [20]])
    slave = np.concatenate([s, s[:49], hub_s, [21]])
    o = rng.permutation(mastr.size)
    mastr, slave = mastr[o], slave[o]
    assert mastr.size == 5000 and not (mastr == slave).any()
    springs = (mastr, slave, rng.random(5000) * 100.0, rng.random(5000) * 0.5)
    bm = rng.integers(0, live, 200)
    bn = (bm + rng.integers(1, live, 200)) % live
    bp = (bm + rng.integers(1, live, 200)) % live
    bm[:10], bn[:10] = mastr[:10], slave[:10]  # a beam and a spring between the same two nodes
    bp[:10] = (bm[:10] + 1 + (bn[:10] == (bm[:10] + 1) % live)) % live
    bp[10] = bn[10]  # next == prev
    assert not (bm == bn).any() and not (bm == bp).any()
    beams = (bm, bn, bp, rng.random(200) * 10.0, rng.standard_normal((200, nd)) * 0.1)
    node = np.arange(0, live, 3)
    targets = (node, rng.random(node.size) * 50.0, rng.random(node.size), rng.random((node.size, nd)))
    dX = None
    if with_dX:
        dX = rng.integers(-1, 2, (n, nd)).astype(np.float64)
    if coincident:
        X[21] = X[20]
    return dict(n=n, nd=nd, live=live, X=X, springs=springs, beams=beams, targets=targets, dX=dX)


def _chain(n):
    """A fibre of n nodes in 3-D: springs between neighbours, beams on the interior nodes, a
    target point with damping on node 0."""
    nd = 3
    rng = np.random.default_rng(n)
    X = np.linspace(0.0, 1.0, n)[:, None] * np.ones(nd) + rng.standard_normal((n, nd)) * (0.2 / n)
    i = np.arange(n - 1)
    springs = (i, i + 1, rng.random(n - 1) * 10.0 + 1.0, np.full(n - 1, 0.9 / max(n, 2))) if n > 1 else None
    j = np.arange(1, n - 1)
    beams = (j, j + 1, j - 1, rng.random(j.size) + 0.5, np.zeros((j.size, nd))) if n > 2 else None
    targets = ([0], [3.0], [0.25], rng.random((1, nd)))
    return dict(n=n, nd=nd, X=X, springs=springs, beams=beams, targets=targets, dX=None)


CHAINS = [1, 2, 3, 255, 256, 257, 4099]
CASE_NAMES = list(DECKS) + ["synthetic", "synthetic_dX"] + [f"chain_{n}" for n in CHAINS]


def _make_case(name):
    if name in DECKS:
        return _deck_case(name)
    if name == "synthetic":
        return _synthetic()
    if name == "synthetic_dX":
        return _synthetic(with_dX=True)
    if name == "synthetic_nan":
        return _synthetic(coincident=True)
    return _chain(int(name.split("_")[1]))


_CACHE = {}


def _case(name):
    """The case with its restatement (computed once, then left alone): J as block-CSR arrays,
    the per-block sums of |contributions|, the contribution counts, the longdouble sums of the
    contributions."""
    if name not in _CACHE:
        c = _make_case(name)
        J, A, cnt, E = reference_jacobian(c["n"], c["nd"], c["X"], c["springs"], c["beams"], c["targets"], X_COEF,
                                          U_COEF, dX=c["dX"], exact=True)
        c["rowptr"], c["col"], c["val"] = bsr_arrays(c["n"], c["nd"], J)
        c["absval"] = bsr_arrays(c["n"], c["nd"], A)[2]
        c["count"] = np.array([cnt[k] for k in sorted(cnt)], dtype=np.int64)
        c["exactval"] = np.array([E[k] for k in sorted(E)], dtype=np.longdouble).reshape(-1, c["nd"], c["nd"])
        for a in ("rowptr", "col", "val", "absval", "count", "exactval"):
            c[a].setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def _build(ctx, fgmod, c):
    fg = fgmod.ForceGen(ctx, c["n"], c["nd"], springs=c["springs"], beams=c["beams"], targets=c["targets"])
    return fg, fgmod.ForceJacobian(ctx, fg)


def _assert_bits(got, ref, what):
    assert got.shape == ref.shape, what
    g, r = got.reshape(-1), ref.reshape(-1)
    both_nan = np.isnan(g) & np.isnan(r)
    bad = (g.view(np.int64) != r.view(np.int64)) & ~both_nan
    with np.errstate(invalid="ignore"):
        print(f"{what}: {int(bad.sum())} of {bad.size} words differ, {int(both_nan.sum())} NaN in both")
    assert not bad.any(), what


def _exact_product(c, val, V, absolute=False):
    """sum_j B_ij V_j over the block-CSR arrays in numpy.longdouble, (n, nd)."""
    n, nd = c["n"], c["nd"]
    rows = np.repeat(np.arange(n), np.diff(c["rowptr"]))
    Vl = (np.abs(V) if absolute else V).astype(np.longdouble)
    B = (np.abs(val) if absolute else val).astype(np.longdouble)
    prod = np.einsum("brc,bc->br", B, Vl[c["col"]])
    Y = np.zeros((n, nd), dtype=np.longdouble)
    np.add.at(Y, rows, prod)
    return Y


@pytest.mark.parametrize("name", CASE_NAMES)
def test_pattern_and_values_bitwise(ctx, fgmod, name):
    """rowptr and col equal the restatement's sorted key set; every word of val equals the serial
    assembly's; a second assemble gives the same bits; bsr() views the same memory."""
    c = _case(name)
    fg, J = _build(ctx, fgmod, c)
    X, dX = _dev(c["X"]), _dev(c["dX"])
    J.assemble(X, dX=dX, X_coef=X_COEF, U_coef=U_COEF)
    rowptr, col, val = J.read()
    assert np.array_equal(rowptr, c["rowptr"]) and np.array_equal(col, c["col"])
    assert J.n_blocks == c["col"].size == J.stats()["blocks"]
    _assert_bits(val, c["val"], name)
    assert not np.isnan(val).any()
    J.assemble(X, dX=dX, X_coef=X_COEF, U_coef=U_COEF)
    r2, c2, v2 = J.bsr()
    ctx.synchronize()
    assert r2.dtype == torch.int64 and c2.dtype == torch.int32 and v2.dtype == torch.float64
    assert tuple(v2.shape) == (col.size, c["nd"], c["nd"])
    assert np.array_equal(v2.cpu().numpy().view(np.int64), val.view(np.int64))
    assert np.array_equal(r2.cpu().numpy(), rowptr) and np.array_equal(c2.cpu().numpy(), col)
    # views, not copies: the tensors sit at the library's own device pointers, and a word written
    # through the view is what read() returns
    nb, rp, cl, vl = J._pattern()
    assert (r2.data_ptr(), c2.data_ptr(), v2.data_ptr()) == (rp, cl, vl) and nb == col.size
    v2[0, 0, 0] = 12345.0
    ctx.synchronize()
    assert J.read()[2][0, 0, 0] == 12345.0
    if name.startswith("synthetic"):
        live = c["live"]
        assert np.array_equal(np.diff(rowptr)[live:], np.ones(c["n"] - live))
        assert not val[rowptr[live]:].view(np.int64).any()  # +0.0 in every word of the isolated diagonals
        assert np.diff(rowptr)[7] > 64  # the hub's row is longer than a wave


def test_coincident_pair_gives_nan_in_its_blocks_only(ctx, fgmod):
    c = _case("synthetic_nan")
    fg, J = _build(ctx, fgmod, c)
    J.assemble(_dev(c["X"]), X_coef=X_COEF, U_coef=U_COEF)
    rowptr, col, val = J.read()
    assert np.array_equal(rowptr, c["rowptr"]) and np.array_equal(col, c["col"])
    rows = np.repeat(np.arange(c["n"]), np.diff(rowptr))
    nan_blocks = np.isnan(val).all(axis=(1, 2))
    assert np.array_equal(nan_blocks, np.isnan(val).any(axis=(1, 2)))
    assert sorted(zip(rows[nan_blocks].tolist(), col[nan_blocks].tolist())) == [(20, 20), (20, 21), (21, 20), (21, 21)]
    assert np.array_equal(np.isnan(val), np.isnan(c["val"]))
    _assert_bits(val, c["val"], "synthetic with a coincident pair")


APPLY_CASES = list(DECKS) + ["synthetic"] + [f"chain_{n}" for n in CHAINS]


@pytest.mark.parametrize("name", APPLY_CASES)
def test_apply(ctx, fgmod, name):
    """|Y - J V| <= gamma_m sum_j |J_ij| |V_j| per component, m the scalar terms of the row (ndim
    per block), against the longdouble product of the read-back values; two calls give the same
    bits; accumulate adds onto a random Y; views at an 8-byte offset give the same bits."""
    c = _case(name)
    n, nd = c["n"], c["nd"]
    fg, J = _build(ctx, fgmod, c)
    J.assemble(_dev(c["X"]), dX=_dev(c["dX"]), X_coef=X_COEF, U_coef=U_COEF)
    val = J.read()[2]
    rng = np.random.default_rng(77)
    V = rng.standard_normal((n, nd))
    Y0 = rng.standard_normal((n, nd))
    exact = _exact_product(c, val, V)
    m = (np.diff(c["rowptr"]) * nd)[:, None]
    bound = gamma(m) * np.asarray(_exact_product(c, val, V, absolute=True), dtype=np.float64)
    Vd = _dev(V)
    Y = J.apply(Vd)
    Yb = J.apply(Vd)
    ctx.synchronize()
    Yh = Y.cpu().numpy()
    err = np.abs(np.asarray(Yh.astype(np.longdouble) - exact, dtype=np.float64))
    print(f"{name}: apply max error {err.max():.3e}, max bound {bound.max():.3e}, worst ratio "
          f"{(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(Yh.view(np.int64), Yb.cpu().numpy().view(np.int64))
    # accumulate: one more rounded add onto Y0
    Ya = _dev(Y0)
    assert J.apply(Vd, Y=Ya, accumulate=True) is Ya
    ctx.synchronize()
    assert np.array_equal(Ya.cpu().numpy().view(np.int64), (Y0 + Yh).view(np.int64))
    # 8-byte-offset views of 16-byte-aligned buffers
    vb = torch.zeros(n * nd + 1, dtype=torch.float64, device="cuda")
    yb = torch.full((n * nd + 2,), 7.0, dtype=torch.float64, device="cuda")
    Vv, Yv = vb[1:].view(n, nd), yb[1:n * nd + 1].view(n, nd)
    assert Vv.data_ptr() % 16 == 8 and Yv.data_ptr() % 16 == 8
    Vv.copy_(Vd)
    J.apply(Vv, Y=Yv)
    ctx.synchronize()
    assert yb[0].item() == 7.0 and yb[-1].item() == 7.0  # nothing written around the view
    assert np.array_equal(Yv.cpu().numpy().view(np.int64), Yh.view(np.int64))


LIN_CASES = list(DECKS) + ["synthetic", "synthetic_dX"] + [f"chain_{n}" for n in CHAINS]


@pytest.mark.parametrize("name", LIN_CASES)
def test_linearized(ctx, fgmod, name):
    """Y = J(X + dX) V straight from the plan: within gamma_m sum |contributions| |V| of the
    longdouble product of the longdouble sums of the restated contributions, m = ndim terms
    per contribution of the row (a spring contributes two blocks, a beam entry three, a target
    point one).  Same bits run to run; accumulate; and it agrees with apply within the two
    bounds plus what the assembled blocks' own accumulation differs from the sum of their
    contributions by (gamma_count of the same sums)."""
    c = _case(name)
    n, nd = c["n"], c["nd"]
    fg, J = _build(ctx, fgmod, c)
    rng = np.random.default_rng(78)
    V = rng.standard_normal((n, nd))
    Y0 = rng.standard_normal((n, nd))
    exact = _exact_product(c, c["exactval"], V)
    rows = np.repeat(np.arange(n), np.diff(c["rowptr"]))
    ncontrib = np.zeros(n, dtype=np.int64)
    np.add.at(ncontrib, rows, c["count"])
    absprod = np.asarray(_exact_product(c, c["absval"], V, absolute=True), dtype=np.float64)
    m = (ncontrib * nd)[:, None]
    bound = gamma(m) * absprod
    X, dX, Vd = _dev(c["X"]), _dev(c["dX"]), _dev(V)
    Y = fg.linearized(X, Vd, dX=dX, X_coef=X_COEF, U_coef=U_COEF)
    Yb = fg.linearized(X, Vd, dX=dX, X_coef=X_COEF, U_coef=U_COEF)
    Ya = _dev(Y0)
    assert fg.linearized(X, Vd, Y=Ya, dX=dX, X_coef=X_COEF, U_coef=U_COEF, accumulate=True) is Ya
    J.assemble(X, dX=dX, X_coef=X_COEF, U_coef=U_COEF)
    Yj = J.apply(Vd)
    ctx.synchronize()
    Yh = Y.cpu().numpy()
    err = np.abs(np.asarray(Yh.astype(np.longdouble) - exact, dtype=np.float64))
    print(f"{name}: linearized max error {err.max():.3e}, max bound {bound.max():.3e}, worst ratio "
          f"{(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(Yh.view(np.int64), Yb.cpu().numpy().view(np.int64))
    assert np.array_equal(Ya.cpu().numpy().view(np.int64), (Y0 + Yh).view(np.int64))
    mj = (np.diff(c["rowptr"]) * nd)[:, None]
    assert (np.abs(Yj.cpu().numpy() - Yh) <= bound + (gamma(mj) + gamma(int(c["count"].max()))) * absprod).all()


@pytest.mark.parametrize("name", ["fila_256", "sphere3d_32", "synthetic", "chain_3", "chain_4099"])
def test_jacobian_nnz(ctx, fgmod, name):
    c = _case(name)
    n = c["n"]
    fg = fgmod.ForceGen(ctx, n, c["nd"], springs=c["springs"], beams=c["beams"], targets=c["targets"])
    true = np.diff(c["rowptr"])
    for n_local in (n, max(n - 5, 0), n // 2):
        d, o = fg.jacobian_nnz() if n_local == n else fg.jacobian_nnz(n_local)
        ctx.synchronize()
        assert d.dtype == torch.int32 and o.dtype == torch.int32 and d.numel() == n and o.numel() == n
        dr, orr = reference_nnz(n, n_local, c["springs"], c["beams"])
        assert np.array_equal(d.cpu().numpy(), dr) and np.array_equal(o.cpu().numpy(), orr)
        assert (true <= dr + orr).all()
    with pytest.raises(ValueError):
        fg.jacobian_nnz(n + 1)


def test_renumber_makes_the_pattern_stale_and_rebuild_follows(ctx, fgmod):
    from ibamr_amd._lib import IBTKLEError
    sp = _deck_specs("fila_256")
    n, nd = sp.num_vertex, sp.ndim
    fg = fgmod.ForceGen.from_specs(ctx, sp)
    ds = fgmod.DeviceForceSpecs(ctx, sp)
    J = fgmod.ForceJacobian(ctx, fg)
    rng = np.random.default_rng(5)
    X = _dev(sp.X0 + 1e-3 * rng.standard_normal((n, nd)))
    J.assemble(X, X_coef=X_COEF, U_coef=U_COEF)
    V = torch.ones_like(X)
    J.apply(V)

    def renumber_and_check(order):
        fg.renumber(ds, torch.from_numpy(order.astype(np.int32)).cuda())
        assert not J.stats()["current"]
        for call in (lambda: J.assemble(X, X_coef=X_COEF, U_coef=U_COEF), lambda: J.apply(V)):
            with pytest.raises(IBTKLEError, match="rebuild") as e:
                call()
            assert e.value.code == 4
        st = J.rebuild()
        assert st["current"]
        perm = np.empty(n, dtype=np.int64)
        perm[order] = np.arange(n)
        a = sp.arrays(perm)
        Xn = X.cpu().numpy()
        Jr, _, _ = reference_jacobian(n, nd, Xn, a["springs"], a["beams"], a["targets"], X_COEF, U_COEF)
        rp, cl, vl = bsr_arrays(n, nd, Jr)
        J.assemble(X, X_coef=X_COEF, U_coef=U_COEF)
        rowptr, col, val = J.read()
        assert np.array_equal(rowptr, rp) and np.array_equal(col, cl)
        _assert_bits(val, vl, "renumbered fila_256")
        return st

    st1 = renumber_and_check(rng.permutation(n))
    st2 = renumber_and_check(rng.permutation(n))
    assert st2["allocations"] == st1["allocations"] and st2["bytes"] == st1["bytes"]
    assert st2["builds"] == st1["builds"] + 1 and st2["blocks"] == st1["blocks"]
    # a set_* makes it stale as well
    fg.set_targets([], [], [], np.zeros((0, nd)))
    with pytest.raises(IBTKLEError, match="rebuild"):
        J.assemble(X)
    J.rebuild()
    J.assemble(X)


def test_errors(ctx, le, fgmod):
    from ibamr_amd._lib import IBTKLEError
    c = _case("chain_3")
    n, nd = c["n"], c["nd"]
    fg, J = _build(ctx, fgmod, c)
    X = _dev(c["X"])
    with pytest.raises(IBTKLEError, match="assemble") as e:
        J.apply(X)  # no values yet
    assert e.value.code == 4
    for bad in (X[:2], X.to(torch.float32), torch.zeros((n, nd + 1), dtype=torch.float64, device="cuda"), X.t()):
        with pytest.raises(ValueError):
            J.assemble(bad)
        with pytest.raises(ValueError):
            J.apply(bad)
        with pytest.raises(ValueError):
            fg.linearized(X, bad)
        with pytest.raises(ValueError):
            fg.linearized(bad, X)
    # a force generator of another context
    other = le.Context(0)
    with pytest.raises(IBTKLEError, match="another context") as e:
        fgmod.ForceJacobian(other, fg)
    assert e.value.code == 4
    lib = ctx.lib
    assert lib.ibtk_le_forcejac_assemble(other.h, J.h, None, None, 1.0, 0.0) == 4
    assert b"another context" in lib.ibtk_le_last_error()
    assert lib.ibtk_le_forcejac_assemble(ctx.h, J.h, None, None, 1.0, 0.0) == 4
    assert b"null array" in lib.ibtk_le_last_error()
    # an invalid plan: a failed renumber
    sp = _deck_specs("fila_256")
    fg2 = fgmod.ForceGen.from_specs(ctx, sp)
    J2 = fgmod.ForceJacobian(ctx, fg2)
    ds = fgmod.DeviceForceSpecs(ctx, sp)
    order = np.arange(sp.num_vertex, dtype=np.int32)
    order[4] = order[5]
    with pytest.raises(IBTKLEError):
        fg2.renumber(ds, torch.from_numpy(order).cuda())
    X2 = _dev(sp.X0)
    for call in (J2.rebuild, lambda: J2.assemble(X2), lambda: fgmod.ForceJacobian(ctx, fg2),
                 lambda: fg2.linearized(X2, X2), fg2.jacobian_nnz):
        with pytest.raises(IBTKLEError, match="invalid") as e:
            call()
        assert e.value.code == 4


def test_closed_force_generator(ctx, fgmod):
    """The library reads fg's plan through the Jacobian: once fg is closed every call that would is
    refused in Python, and closing the Jacobian still frees its buffers."""
    c = _case("chain_3")
    fg, J = _build(ctx, fgmod, c)
    X = _dev(c["X"])
    J.assemble(X)
    fg.close()
    for call in (lambda: J.assemble(X), lambda: J.apply(X), J.rebuild, J.stats, J.read, J.bsr):
        with pytest.raises(ValueError, match="closed"):
            call()
    J.close()
    assert J.h is None
    with pytest.raises(ValueError, match="closed"):
        J.stats()


def test_no_host_synchronisation(ctx, fgmod):
    """assemble, apply, linearized, jacobian_nnz and bsr under torch's sync debug mode "error".
    That mode sees only the synchronisations torch itself makes (an allocation that blocks, a
    copy to the host, an .item()): it shows that the Python layer adds none.  A
    hipStreamSynchronize inside the library would pass it; that the four entry points have none
    (no synchronise, no blocking copy, no allocation) rests on reading them in le_abi.cpp."""
    c = _case("sphere3d_32")
    fg, J = _build(ctx, fgmod, c)
    X = _dev(c["X"])
    V = torch.ones_like(X)
    Y = torch.empty_like(X)
    J.assemble(X, X_coef=X_COEF, U_coef=U_COEF)
    J.apply(V, Y=Y)
    ctx.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        J.assemble(X, X_coef=X_COEF, U_coef=U_COEF)
        J.apply(V, Y=Y)
        fg.linearized(X, V, Y=Y, accumulate=True)
        fg.jacobian_nnz(c["n"] - 3)
        J.bsr()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ctx.synchronize()


def test_empty_plan(ctx, fgmod):
    """No springs, beams or target points: the pattern is the +0.0 diagonal."""
    fg = fgmod.ForceGen(ctx, 5, 2)
    J = fgmod.ForceJacobian(ctx, fg)
    X = torch.rand((5, 2), dtype=torch.float64, device="cuda")
    J.assemble(X)
    rowptr, col, val = J.read()
    assert rowptr.tolist() == [0, 1, 2, 3, 4, 5] and col.tolist() == [0, 1, 2, 3, 4]
    assert not val.view(np.int64).any()
    Y = J.apply(X)
    Yl = fg.linearized(X, X)
    ctx.synchronize()
    assert not Y.cpu().numpy().any() and not Yl.cpu().numpy().any()

"""GPU: the side-centred curl (ibtk_le_curl_side, ibamr_amd.gib) against the numpy
restatement tests/curl_ref.py -- which tests/test_curl_cpu.py holds to the compiled
reference Fortran bit for bit -- and the two generalized-IB compositions around it.

Every comparison with curl_ref is bit for bit, as int64.  A w array is compared as its
whole allocation, row padding of a pitched layout included: it starts from a per-point
sentinel pattern, the expected image is that pattern with curl_ref's values in the three
side boxes, and every other bit must survive.

The kernel cuts z into segments of at most CURL_TILE[2] planes and, for the few tiles of
these small boxes, of gib.CURL_MIN_SEGMENT planes: the z extents below cross many segment
boundaries; the segment length enters the kernel only as a loop count.
"""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import curl_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

DX = (0.1, 0.037, 0.2113)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def gib(le):
    from ibamr_amd import gib as _gib
    return _gib


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def make_geom(le, ilower, n, gcw, pitched, dx=DX):
    iupper = [ilower[d] + n[d] - 1 for d in range(3)]
    g = le.Geometry(list(ilower), iupper, gcw, list(dx), [0.0, 0.0, 0.0])
    return g.aligned() if pitched else g


def span(t):
    """The whole allocation under a (possibly pitched) side array, as a flat view."""
    size = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return torch.as_strided(t, (size,), (1,))


def upload(geom, arrays, pattern_base):
    """Device side arrays of geom holding `arrays`, every other element of their
    allocations (row padding) a distinct finite sentinel."""
    ts = geom.alloc("side")
    for c, (t, a) in enumerate(zip(ts, arrays)):
        flat = span(t)
        flat.copy_(torch.from_numpy(-(pattern_base + 1000.0 * c + np.arange(flat.numel(), dtype=np.float64))))
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return ts


def image(t):
    """(flat host copy of the allocation, a strided numpy view of the array in it)."""
    flat = span(t).cpu().numpy().copy()
    view = np.lib.stride_tricks.as_strided(flat, tuple(t.shape), tuple(8 * s for s in t.stride()))
    return flat, view


def ghost_mask(n, g, c, dims):
    """True at the points of side array c outside the cell range in one of `dims` (the
    face iupper + 1 of the array's own axis included): what a periodic fill overwrites."""
    shp = cr.side_shape(n, g, c)
    m = np.zeros(shp, bool)
    gg = [g] * 3 if np.isscalar(g) else list(g)
    for d in dims:
        ax = 2 - d
        idx = np.arange(shp[ax]) - gg[d]
        out = (idx < 0) | (idx >= n[d])
        sl = [None, None, None]
        sl[ax] = slice(None)
        m |= out[tuple(sl)]
    return m


def run_case(le, gib, ctx, ilower, n, ug, wg, pitched, seed, alpha=1.0, accumulate=False, periodic=None,
             dx=DX, u_np=None, against_fill=False):
    """One call on seeded data, checked against curl_ref; returns the side-box values."""
    rng = np.random.default_rng(seed)
    gu, gw = make_geom(le, ilower, n, ug, pitched, dx), make_geom(le, ilower, n, wg, pitched, dx)
    if u_np is None:
        u_np = [rng.standard_normal(cr.side_shape(n, ug, c)) for c in range(3)]
    per_dims = [d for d in range(3) if periodic is not None and periodic[d]]
    if per_dims:  # what the periodic call must not read
        u_np = [a.copy() for a in u_np]
        for c in range(3):
            u_np[c][ghost_mask(n, ug, c, per_dims)] = np.nan
    w_np = []
    for c in range(3):
        a = -(5.0e6 + 1.0e4 * c + np.arange(int(np.prod(cr.side_shape(n, wg, c))), dtype=np.float64))
        a = a.reshape(cr.side_shape(n, wg, c))
        box = cr.side_box(n, wg, c)
        a[box] = rng.standard_normal(a[box].shape) if accumulate else np.nan
        w_np.append(a)
    u_t, w_t = upload(gu, u_np, 1.0e6), upload(gw, w_np, 3.0e6)
    u_before = [image(t)[0] for t in u_t]
    expect = []
    for c in range(3):
        flat, view = image(w_t[c])
        expect.append((flat, view))
    w_host = [np.ascontiguousarray(v) for _, v in expect]
    iupper = [ilower[d] + n[d] - 1 for d in range(3)]
    cr.curl_side_ref(u_np, ilower, iupper, ug, w_host, wg, dx, alpha, accumulate, periodic)
    for c in range(3):
        expect[c][1][...] = w_host[c]
    gib.curl_side(ctx, gu, u_t, gw, w_t, alpha=alpha, accumulate=accumulate, periodic=periodic)
    ctx.synchronize()
    out = []
    for c in range(3):
        got, view = image(w_t[c])
        assert np.array_equal(cr.bits(got), cr.bits(expect[c][0])), \
            f"w{c}: {(cr.bits(got) != cr.bits(expect[c][0])).sum()} of {got.size} elements differ"
        assert np.array_equal(cr.bits(image(u_t[c])[0]), cr.bits(u_before[c])), f"u{c} was written"
        vals = view[cr.side_box(n, wg, c)]
        assert not np.isnan(vals).any(), f"a NaN reached w{c}"
        out.append(vals.copy())
    if against_fill:
        # ibtk_le_fill_periodic_ghosts on a copy, then the plain call
        u2 = upload(gu, u_np, 1.0e6)
        w2 = upload(gw, w_np, 3.0e6)
        le.fill_periodic_ghosts(ctx, gu, "side", u2, periodic=list(periodic))
        gib.curl_side(ctx, gu, u2, gw, w2, alpha=alpha, accumulate=accumulate, periodic=None)
        ctx.synchronize()
        for c in range(3):
            assert np.array_equal(cr.bits(image(w2[c])[0]), cr.bits(image(w_t[c])[0])), f"w{c} against the fill"
    return out


def sweep_cases():
    from ibamr_amd.gib import CURL_TILE
    boxes = []
    for d in range(3):
        T = CURL_TILE[d]
        for e in (1, 2, T - 1, T, T + 1, 2 * T + 3):
            n = [5, 5, 5]
            n[d] = e
            boxes.append(tuple(n))
    TX, TY, TZ = CURL_TILE
    boxes += [(1, 1, 1), (3, 2, 5), (TX + 1, TY + 1, TZ + 1), (2 * TX + 3, TY - 1, 2)]
    cases = []
    for n in boxes:
        for ilower in ((0, 0, 0), (-3, 2, 5)):
            for ug, wg in ((1, 0), (3, 3), (4, 1)):
                for pitched in (False, True):
                    cases.append((n, ilower, ug, wg, pitched))
    return cases


@pytest.mark.parametrize("n,ilower,ug,wg,pitched", sweep_cases(),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_shape_sweep(le, gib, ctx, n, ilower, ug, wg, pitched):
    run_case(le, gib, ctx, ilower, list(n), ug, wg, pitched, seed_of("sweep", n, ilower, ug, wg, pitched))


@pytest.mark.parametrize("alpha", [1.0, 0.5, -3.0])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("pitched", [False, True])
def test_alpha_and_accumulate(le, gib, ctx, alpha, accumulate, pitched):
    from ibamr_amd.gib import CURL_TILE
    n = [CURL_TILE[0] + 3, 7, 6]
    run_case(le, gib, ctx, (-3, 2, 5), n, 2, 3, pitched, seed_of("alpha", alpha, accumulate, pitched), alpha=alpha,
             accumulate=accumulate)


def periodic_boxes():
    from ibamr_amd.gib import CURL_TILE
    TX, TY, TZ = CURL_TILE
    return [(1, 1, 1), (TX + 1, 3, 4), (5, TY + 1, TZ + 1)]


@pytest.mark.parametrize("flags", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
@pytest.mark.parametrize("n", periodic_boxes(), ids=lambda v: "x".join(map(str, v)))
def test_periodic(le, gib, ctx, n, flags):
    """Every subset of periodic dims: u's ghosts are NaN in the flagged dims (never read) and
    random in the others (read as they stand); the result is curl_ref's and, where
    ibtk_le_fill_periodic_ghosts accepts the box (2 gcw + 1 cells in every flagged dim; the
    curl itself has no such limit, box 1x1x1 wraps onto itself), that of the fill on a copy
    followed by the plain call."""
    ug = 1
    fill_ok = any(flags) and all(n[d] >= 2 * ug + 1 for d in range(3) if flags[d])
    for pitched in (False, True):
        run_case(le, gib, ctx, (-3, 2, 5), list(n), ug, 2, pitched, seed_of("per", n, flags, pitched), alpha=0.5,
                 periodic=flags, against_fill=fill_ok)


def test_periodic_needs_no_ghost_layer(le, gib, ctx):
    """A periodic dim of u may have ghost width 0 (the bench path never materialises u's
    periodic ghosts); a non-periodic one still needs 1."""
    run_case(le, gib, ctx, (0, 0, 0), [9, 4, 6], [0, 1, 0], 2, False, 77, alpha=0.5, periodic=(1, 0, 1))
    run_case(le, gib, ctx, (0, 0, 0), [9, 4, 6], 0, 0, True, 78, alpha=1.0, periodic=(1, 1, 1))


@pytest.mark.parametrize("omega", [(1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (1.0, -2.0, 4.0)])
def test_exact_rotation(le, gib, ctx, omega):
    """u = omega x (x - c) on dyadic data: 0.5 curl u == omega in every bit, and a constant
    field gives +0.0."""
    from test_curl_cpu import rotation_field
    n, h = [8, 8, 8], 2.0 ** -4
    u = rotation_field(omega, (0.25, 0.5, 0.125), n, 1, h)
    vals = run_case(le, gib, ctx, (0, 0, 0), n, 1, 0, False, 3, alpha=0.5, dx=(h, h, h), u_np=u)
    for c in range(3):
        assert np.array_equal(cr.bits(vals[c]), cr.bits(np.full(vals[c].shape, omega[c])))
    const = [np.full(cr.side_shape(n, 1, c), v) for c, v in enumerate((1.5, -0.375, 7.0))]
    vals = run_case(le, gib, ctx, (0, 0, 0), n, 1, 0, False, 4, dx=(h, h, h), u_np=const)
    for c in range(3):
        assert not cr.bits(vals[c]).any()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_reference_fixture_on_the_device(le, gib, ctx, k):
    """The compiled reference's own inputs and outputs (tests/golden/curl_side_ref.npz)
    against the kernel, bit for bit, untouched NaNs included."""
    from test_curl_cpu import FIXTURE, fixture_case
    ilo, ihi, ug, wg, dx, u, w_ref = fixture_case(np.load(FIXTURE), k)
    n = cr.box_extent(ilo, ihi)
    for pitched in (False, True):
        gu = make_geom(le, [int(v) for v in ilo], n, ug, pitched, dx)
        gw = make_geom(le, [int(v) for v in ilo], n, wg, pitched, dx)
        u_t = upload(gu, u, 1.0e6)
        w_t = upload(gw, [np.full_like(a, np.nan) for a in w_ref], 3.0e6)
        gib.curl_side(ctx, gu, u_t, gw, w_t)
        ctx.synchronize()
        for c in range(3):
            assert np.array_equal(cr.bits(w_t[c].cpu().numpy()), cr.bits(w_ref[c])), f"case {k} w{c}"


# ---------------------------------------------------------------------------------------
# refusals: argument checks on the host, nothing launched, w untouched
# ---------------------------------------------------------------------------------------
def refusal_setup(le, n=(4, 3, 5), ug=1, wg=1):
    gu, gw = make_geom(le, (0, 0, 0), list(n), ug, False), make_geom(le, (0, 0, 0), list(n), wg, False)
    rng = np.random.default_rng(9)
    u = upload(gu, [rng.standard_normal(cr.side_shape(n, ug, c)) for c in range(3)], 1.0e6)
    w = upload(gw, [np.full(cr.side_shape(n, wg, c), np.nan) for c in range(3)], 3.0e6)
    return gu, u, gw, w


def expect_refusal(le, gib, ctx, code, word, gu, u, gw, w, watch=None, **kw):
    from ibamr_amd._lib import IBTKLEError
    watch = [t for t in (w if watch is None else watch) if t is not None]
    before = [cr.bits(t.cpu().numpy()) for t in watch]
    with pytest.raises(IBTKLEError) as e:
        gib.curl_side(ctx, gu, u, gw, w, **kw)
    assert e.value.code == code, str(e.value)
    assert word in str(e.value), str(e.value)
    ctx.synchronize()
    for t, b in zip(watch, before):
        assert np.array_equal(cr.bits(t.cpu().numpy()), b), "a refused call wrote w"


def test_refusals(le, gib, ctx):
    ARG, GHOST = 4, 2
    gu, u, gw, w = refusal_setup(le)
    n = [4, 3, 5]
    # ndim != 3
    g2 = le.Geometry([0, 0], [3, 2], 1, [0.1, 0.1], [0.0, 0.0])
    expect_refusal(le, gib, ctx, ARG, "ndim", g2, u, gw, w)
    expect_refusal(le, gib, ctx, ARG, "ndim", gu, u, g2, w)
    # boxes and dx that differ
    expect_refusal(le, gib, ctx, ARG, "boxes", make_geom(le, (1, 0, 0), n, 1, False), u, gw, w)
    expect_refusal(le, gib, ctx, ARG, "boxes", gu, u, make_geom(le, (0, 0, 0), [4, 3, 6], 1, False), w)
    expect_refusal(le, gib, ctx, ARG, "dx", gu, u, make_geom(le, (0, 0, 0), n, 1, False, (0.1, 0.037, 0.2)), w)
    # a null pointer
    expect_refusal(le, gib, ctx, ARG, "null", gu, [u[0], None, u[2]], gw, w)
    expect_refusal(le, gib, ctx, ARG, "null", gu, u, gw, [w[0], w[1], None])
    # in place, and a w array inside another u array's range
    expect_refusal(le, gib, ctx, ARG, "overlap", gu, u, gu, u, watch=u)
    expect_refusal(le, gib, ctx, ARG, "overlap", gu, u, gw, [w[0], u[0], w[2]], watch=[w[0], u[0], w[2]])
    # a non-finite or zero dx
    for bad in (0.0, float("nan"), float("inf")):
        gb = make_geom(le, (0, 0, 0), n, 1, False, (0.1, bad, 0.2113))
        expect_refusal(le, gib, ctx, ARG, "dx", gb, u, gb, w)
    # the plain routine reads one ghost point of u in every dim
    g0, u0, _, _ = refusal_setup(le, ug=0)
    expect_refusal(le, gib, ctx, GHOST, "ghost", g0, u0, gw, w)
    expect_refusal(le, gib, ctx, GHOST, "ghost", g0, u0, gw, w, periodic=(1, 0, 1))
    gib.curl_side(ctx, g0, u0, gw, w, periodic=(1, 1, 1))  # every dim periodic: no ghost layer needed
    ctx.synchronize()
    assert not torch.isnan(w[0][cr.side_box(n, 1, 0)]).any()


def test_empty_box_is_ok_and_writes_nothing(le, gib, ctx):
    ge = le.Geometry([0, 0, 0], [-1, 3, 4], 1, list(DX), [0.0, 0.0, 0.0])
    u = ge.alloc("side", fill=1.0)
    w = ge.alloc("side", fill=float("nan"))
    gib.curl_side(ctx, ge, u, ge, w)
    ctx.synchronize()
    assert all(torch.isnan(t).all() for t in w)


# ---------------------------------------------------------------------------------------
# the two compositions
# ---------------------------------------------------------------------------------------
def coupling_markers(rng, M=300):
    X = rng.uniform(0.0, 1.0, (M, 3))
    h = 1.0 / 16
    X[:20, 0] = np.round(X[:20, 0] / h) * h + rng.choice([-1.0e-12, 1.0e-12], 20)   # next to cell faces
    X[20:30, 1] = rng.choice([1.0e-12, 1.0 - 1.0e-12], 10)                          # next to the domain boundary
    X[30:40, 2] = rng.choice([1.0e-12, 1.0 - 1.0e-12], 10)
    return np.ascontiguousarray(np.clip(X, 1.0e-12, 1.0 - 1.0e-12))


@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
def test_interp_angular_velocity(le, gib, ctx, oracle, kernel):
    """W == the oracle's side interp of 0.5 curl_ref(u) with numpy-filled ghosts, bit for
    bit (3-D side interp is bitwise the oracle, tests/test_gpu_parity.py)."""
    g = oracle.min_ghost_width(kernel)
    n = [16, 16, 16]
    rng = np.random.default_rng(seed_of("W", kernel))
    gu, gw = le.Geometry.periodic_unit(n, 1), le.Geometry.periodic_unit(n, g)
    X = coupling_markers(rng)
    u_np = [rng.standard_normal(cr.side_shape(n, 1, c)) for c in range(3)]
    for c in range(3):
        u_np[c][ghost_mask(n, 1, c, (0, 1, 2))] = np.nan  # never read
    u_t = upload(gu, u_np, 1.0e6)
    w_t = gw.alloc("side", fill=float("nan"))
    Xd = torch.from_numpy(X).to(DEV)
    W = torch.full((X.shape[0], 3), np.nan, dtype=torch.float64, device=DEV)
    m = le.Markers(ctx).bin(gw, kernel, Xd)
    gib.interp_angular_velocity(ctx, m, kernel, gu, u_t, gw, w_t, W, Xd, periodic=(1, 1, 1))
    ctx.synchronize()
    w_ref = [np.full(cr.side_shape(n, g, c), np.nan) for c in range(3)]
    cr.curl_side_ref(u_np, (0, 0, 0), (15, 15, 15), 1, w_ref, g, gu.dx, alpha=0.5, periodic=(1, 1, 1))
    for c in range(3):
        box = cr.side_box(n, g, c)
        assert np.array_equal(cr.bits(w_t[c].cpu().numpy()[box]), cr.bits(w_ref[c][box]))
    w_fill = cr.periodic_fill(w_ref, n, g, (1, 1, 1))
    Wo = np.full((X.shape[0], 3), np.nan)
    idx = np.arange(X.shape[0], dtype=np.int32)
    oracle.side_interp(kernel, gw.dx, gw.x_lower, gw.ilower, gw.iupper, gw.gcw, w_fill, idx, np.zeros_like(X), X, Wo)
    assert np.array_equal(cr.bits(W.cpu().numpy()), cr.bits(Wo))


@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
@pytest.mark.parametrize("fold", [True, False])
def test_spread_torque(le, gib, ctx, oracle, kernel, fold):
    """f == 0.5 curl_ref(n_device, periodic) + f0 bit for bit, n_device the scratch read
    back after the call: the curl stage adds no error of its own.  fold=True spreads the
    interior list and folds; fold=False spreads a list that holds the periodic images.
    Two runs give identical bits."""
    g = oracle.min_ghost_width(kernel)
    n = [16, 16, 16]
    rng = np.random.default_rng(seed_of("N", kernel))
    gn, gf = le.Geometry.periodic_unit(n, g), le.Geometry.periodic_unit(n, 0).aligned()
    X = coupling_markers(rng)
    Nn = rng.standard_normal((X.shape[0], 3))
    Xd, Nd = torch.from_numpy(X).to(DEV), torch.from_numpy(Nn).to(DEV)
    if fold:
        m = le.Markers(ctx).bin(gn, kernel, Xd)
    else:
        idx, xs = le.periodic_index_list(ctx, gn, Xd, g, periodic=[1, 1, 1])
        assert idx.numel() > X.shape[0]
        m = le.Markers(ctx).bin(gn, kernel, Xd, idx, xs)
    f0 = [rng.standard_normal(cr.side_shape(n, 0, c)) for c in range(3)]
    results = []
    for run in range(2):
        n_t = gn.alloc("side", fill=float("nan"))
        f_t = upload(gf, f0, 3.0e6)
        f_before = [image(t) for t in f_t]
        gib.spread_torque(ctx, m, kernel, gn, n_t, Nd, Xd, gf, f_t, periodic=(1, 1, 1), fold=fold)
        ctx.synchronize()
        n_dev = [t.cpu().numpy() for t in n_t]
        assert all(np.isfinite(a).all() for a in n_dev) and any(np.abs(a).max() > 0 for a in n_dev)
        f_ref = [a.copy() for a in f0]
        cr.curl_side_ref(n_dev, (0, 0, 0), (15, 15, 15), g, f_ref, 0, gn.dx, alpha=0.5, accumulate=True,
                         periodic=(1, 1, 1))
        for c in range(3):
            flat, view = f_before[c]
            view[...] = f_ref[c]
            got = image(f_t[c])[0]
            assert np.array_equal(cr.bits(got), cr.bits(flat)), f"f{c}"
            assert not np.array_equal(f_ref[c], f0[c])
        results.append([image(t)[0] for t in f_t] + n_dev)
    for a, b in zip(*results):
        assert np.array_equal(cr.bits(a), cr.bits(b)), "two runs differ"


def test_rod_step_plumbing(le, gib, ctx, oracle):
    """One generalized-IB step's Lagrangian-Eulerian plumbing on the ex4 ring, no fluid
    solve: rodgen.compute -> spread_torque, and interp_angular_velocity -> director_update.
    Each stage against the same chain from rod_ref, the oracle and curl_ref under that
    stage's existing standard (tests/test_gpu_rods.py, tests/test_gpu_parity.py); the two
    curl stages bit for bit given their device inputs."""
    from pathlib import Path

    from rod_ref import reference_director_update, reference_rods
    from test_gpu_parity import SPREAD_TOL
    from test_gpu_rods import _check, _scales
    import json

    from ibamr_amd import io, rods
    from ibamr_amd.rods import RodSpecs
    golden = Path(__file__).resolve().parent / "golden"
    kat = json.loads((golden / "rod_kat.json").read_text())
    tol = {q: 8.0 * max(kat["ref_err"][q], 2.0 ** -52) for q in ("F", "N", "D_new")}
    kernel = "IB_4"
    g = oracle.min_ghost_width(kernel)
    X = io.read_vertex(golden / "vertex" / "curve3d_64.vertex", 3)
    sp = RodSpecs.from_files(golden / "ibforce" / "curve3d_64", num_vertex=X.shape[0])
    a = sp.arrays()
    n = [32, 32, 32]
    lo, hi = X.min(0), X.max(0)
    L = 2.0 * float((hi - lo).max())  # the ring's diameter twice over: it sits well inside
    xl = [float(0.5 * (lo[d] + hi[d]) - 0.5 * L) for d in range(3)]
    xu = [v + L for v in xl]
    gn = le.Geometry.periodic_unit(n, g, xl, xu)
    gf = le.Geometry.periodic_unit(n, 1, xl, xu)
    Xd, Dd = torch.from_numpy(X).to(DEV), torch.from_numpy(sp.directors).to(DEV)
    per = (1, 1, 1)
    rng = np.random.default_rng(2024)

    # force and torque at the nodes
    rg = rods.RodForceGen.from_specs(ctx, sp)
    F, N = rg.compute(Xd, Dd)
    ctx.synchronize()
    F_ref, N_ref = reference_rods(X.shape[0], X, sp.directors, a.curr, a.next, a.params)
    N_dev = N.cpu().numpy()
    _check(F.cpu().numpy(), N_dev, F_ref, N_ref, tol, "ex4 step", scales=_scales(X, sp.directors, a.curr, a.next, a.params))

    # torque to the grid: f += 0.5 curl n
    m = le.Markers(ctx).bin(gn, kernel, Xd)
    f0 = [rng.standard_normal(cr.side_shape(n, 1, c)) for c in range(3)]
    f_t = upload(gf, f0, 3.0e6)
    n_t = gn.alloc("side", fill=float("nan"))
    gib.spread_torque(ctx, m, kernel, gn, n_t, N, Xd, gf, f_t, periodic=per)
    ctx.synchronize()
    n_dev = [t.cpu().numpy() for t in n_t]
    idx, xs, _ = oracle.periodic_index_list(X, xl, xu, gn.dx, gn.ilower, gn.iupper, g)
    n_ora = [np.zeros(cr.side_shape(n, g, c)) for c in range(3)]
    oracle.side_spread(kernel, gn.dx, xl, gn.ilower, gn.iupper, gn.gcw, n_ora, idx, xs, X, N_dev)
    for c in range(3):  # the folded interior against the oracle's spread of the list with images
        inner = tuple(slice(g, g + n[d]) for d in (2, 1, 0))
        err = np.abs(n_dev[c][inner] - n_ora[c][inner]).max() / np.abs(n_ora[c]).max()
        print(f"ex4 step: n{c} vs the oracle's spread {err:.3e} (bound {SPREAD_TOL:.1e})")
        assert err <= SPREAD_TOL
    f_ref = [v.copy() for v in f0]
    cr.curl_side_ref(n_dev, gn.ilower, gn.iupper, g, f_ref, 1, gn.dx, alpha=0.5, accumulate=True, periodic=per)
    for c in range(3):
        assert np.array_equal(cr.bits(f_t[c].cpu().numpy()), cr.bits(f_ref[c])), f"f{c}"

    # angular velocity at the nodes and the director update
    u_np = [rng.standard_normal(cr.side_shape(n, 1, c)) for c in range(3)]
    u_t = upload(gf, u_np, 1.0e6)
    w_t = gn.alloc("side", fill=float("nan"))
    W = torch.full((X.shape[0], 3), np.nan, dtype=torch.float64, device=DEV)
    gib.interp_angular_velocity(ctx, m, kernel, gf, u_t, gn, w_t, W, Xd, periodic=per)
    dt = 1.0e-2
    D_new = rods.director_update(ctx, "euler", dt, Dd, W)
    ctx.synchronize()
    w_ref = [np.full(cr.side_shape(n, g, c), np.nan) for c in range(3)]
    cr.curl_side_ref(u_np, gn.ilower, gn.iupper, 1, w_ref, g, gn.dx, alpha=0.5, periodic=per)
    Wo = np.full((X.shape[0], 3), np.nan)
    oracle.side_interp(kernel, gn.dx, xl, gn.ilower, gn.iupper, gn.gcw, cr.periodic_fill(w_ref, n, g, per),
                       np.arange(X.shape[0], dtype=np.int32), np.zeros_like(X), X, Wo)
    W_dev = W.cpu().numpy()
    assert np.array_equal(cr.bits(W_dev), cr.bits(Wo))
    D_ref = reference_director_update("euler", dt, sp.directors, W_dev)
    err = np.abs(D_new.cpu().numpy() - D_ref).max() / np.abs(D_ref).max()
    print(f"ex4 step: D_new vs rod_ref {err:.3e} (bound {2 * tol['D_new']:.3e})")
    assert err <= 2 * tol["D_new"]

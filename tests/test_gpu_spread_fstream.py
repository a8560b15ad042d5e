"""GPU: the 3-D spread reading F at its marker row through the candidate stream's source
rows (ibtk_le_ctx_tune "f_stream" 1) against the gather pass into sorted order (-1).

The stream's entry j carries cs_src[j] = sorted_s[cs_pos[j]] beside the sorted position, so
the sweep loads F(s, c) (times ds(s)) where it loaded sorted_F[c][e]: the same value, the
same add order, so every output array must be equal bit for bit.  Each case spreads once
per mode, each mode in a fresh Context; one case per group also checks the oracle within
the 1e-12 of test_gpu_parity.py.
"""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SPREAD_TOL = 1e-12


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


def _ghost(le, kernel):
    return le._lib.load().ibtk_le_min_ghost_width(le.kernel_id(kernel))


def _both(le, run):
    """run(ctx) -> a list of tensors, once per mode in a fresh Context; asserts them equal
    bit for bit and returns the f_stream = 1 outputs."""
    outs = {}
    for mode in (-1, 1):
        ctx = le.Context(0)
        ctx.tune("f_stream", mode)
        outs[mode] = run(ctx)
        ctx.synchronize()
    assert len(outs[1]) == len(outs[-1]) and len(outs[1]) > 0
    for k, (a, b) in enumerate(zip(outs[-1], outs[1])):
        assert torch.equal(a, b), f"output {k}: the stream's F differs from the gathered F"
    return outs[1]


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


# --- 1. the stream's lifetime -------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
def test_stream_lifetime(le, oracle, kernel):
    """A fresh binning, a re-binning that moved markers (stream and source rows rebuilt from
    the new order) and a standing stream, F rewritten in place between the spreads."""
    geom = le.Geometry.periodic_unit([64, 48, 40], _ghost(le, kernel))
    rng = np.random.default_rng(5)
    M = 40000
    Xn = rng.uniform(0.0, 1.0, (M, 3))
    Fn = rng.standard_normal((M, 3))
    X = torch.from_numpy(Xn).cuda()
    X2 = torch.remainder(X + 0.4 / 64 * (torch.from_numpy(rng.uniform(-0.5, 0.5, (M, 3))).cuda()), 1.0)
    orders = []

    def run(ctx):
        F = torch.from_numpy(Fn).cuda()
        m = le.Markers(ctx).bin(geom, kernel, X)
        res = []
        for step in range(3):
            if step == 1:
                m.rebin(X2)
            if step:
                F.mul_(-0.75).add_(0.125)
            q = geom.alloc("side")
            le.spread(ctx, m, kernel, "side", geom, q, F, X if step == 0 else X2)
            ctx.synchronize()
            res += q
            if step == 1:
                orders.append(m.order().cpu().numpy())
        return res

    out = _both(le, run)
    assert not torch.equal(out[3], out[0]) and not torch.equal(out[6], out[3])  # F's rewrites were seen
    # the spread after the re-binning against the oracle, in the order the GPU sums in
    order = orders[-1]
    F1 = Fn * -0.75 + 0.125
    uo = [np.zeros(tuple(a.shape)) for a in out[:3]]
    oracle.side_spread(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, uo,
                       np.arange(M, dtype=np.int32)[order], np.zeros((M, 3)), X2.cpu().numpy(), F1)
    for a in range(3):
        assert _rel(out[3 + a].cpu().numpy(), uo[a]) <= SPREAD_TOL, f"comp {a}"


# --- 2. the chunk structure ---------------------------------------------------------------

def _chunk_markers(N, g, rng):
    """Dense spots two cells wide in x and y (so all of a spot's markers are candidates of the
    same columns), a thin z layer each:
    357 markers (chunk 1 and four full middle chunks: two turns of the pair loop) with 37 in
    the layer above (the 37 left over carried into that anchor's chunk 1);
    293 + 37 (three middle chunks: the pair loop, then the single loop);
    100 in the topmost anchor plane whose stencil still reaches the array (the last anchor's
    leftovers); and lines of markers along x and y through the layers, which cross every
    column boundary (candidates of the west and south neighbour columns: the band ranges)."""
    h = 1.0 / np.array(N, np.float64)

    def spot(n, cx, cy, cz):
        return np.stack([(cx + rng.uniform(0.0, 2.0, n)) * h[0], (cy + rng.uniform(0.0, 2.0, n)) * h[1],
                         (cz + rng.uniform(0.4, 0.6, n)) * h[2]], axis=1)

    parts = [spot(357, 38, 22, 12), spot(37, 38, 22, 13), spot(293, 10, 6, 20), spot(37, 10, 6, 21),
             spot(100, 38, 22, N[2] + g)]
    t = np.arange(0.125, N[0], 0.25)
    for cz in (12, 13, 20):
        parts.append(np.stack([t * h[0], np.full(t.size, 23.3 * h[1]), np.full(t.size, (cz + 0.45) * h[2])], axis=1))
    t = np.arange(0.125, N[1], 0.25)
    for cz in (12, 21):
        parts.append(np.stack([np.full(t.size, 39.2 * h[0]), t * h[1], np.full(t.size, (cz + 0.55) * h[2])], axis=1))
    X = np.concatenate(parts)
    return X[rng.permutation(X.shape[0])]


@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])  # the pair path, the one-chunk path
def test_chunk_structure(le, oracle, kernel):
    N = [64, 32, 32]
    g = _ghost(le, kernel)
    geom = le.Geometry.periodic_unit(N, g)
    rng = np.random.default_rng(23)
    Xn = _chunk_markers(N, g, rng)
    M = Xn.shape[0]
    Fn = rng.standard_normal((M, 3))
    X, F = torch.from_numpy(Xn).cuda(), torch.from_numpy(Fn).cuda()
    orders = []

    def run(ctx):
        m = le.Markers(ctx).bin(geom, kernel, X)
        q = geom.alloc("side")
        le.spread(ctx, m, kernel, "side", geom, q, F, X)
        ctx.synchronize()
        orders.append(m.order().cpu().numpy())
        return q

    out = _both(le, run)
    uo = [np.zeros(tuple(a.shape)) for a in out]
    oracle.side_spread(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, uo,
                       np.arange(M, dtype=np.int32)[orders[-1]], np.zeros((M, 3)), Xn, Fn)
    for a in range(3):
        assert _rel(out[a].cpu().numpy(), uo[a]) <= SPREAD_TOL, f"comp {a}"


# --- 3. components ------------------------------------------------------------------------

COMPONENTS = [("IB_4", "side", 1, False), ("IB_4", "node", 1, False), ("IB_4", "cell", 2, False),
              ("IB_6", "node", 1, False), ("PIECEWISE_LINEAR", "side", 1, False), ("IB_4", "side", 1, True),
              ("PIECEWISE_CUBIC", "cell", 2, True)]


@pytest.mark.parametrize("kernel,centering,depth,with_ds", COMPONENTS, ids=lambda v: str(v))
def test_components(le, oracle, kernel, centering, depth, with_ds):
    """Side (component 2 on the shifted-z stream), node, cell with q_depth = Q_depth = 2 (not
    a whole 24-byte record), a piecewise kernel on the general ring (which takes its marker
    row from the stream too), and the density-weighted spread."""
    geom = le.Geometry.periodic_unit([40, 36, 44], _ghost(le, kernel))
    rng = np.random.default_rng(31)
    M = 20000
    Qd = 3 if centering == "side" else depth
    Xn = rng.uniform(0.0, 1.0, (M, 3))
    Fn = rng.standard_normal((M, Qd))
    dsn = rng.uniform(1e-4, 1e-3, M)
    X, F, ds = (torch.from_numpy(a).cuda() for a in (Xn, Fn, dsn))
    orders = []

    def run(ctx):
        m = le.Markers(ctx).bin(geom, kernel, X)
        q = geom.alloc(centering, depth=depth)
        le.spread(ctx, m, kernel, centering, geom, q, F, X, q_depth=depth, ds=ds if with_ds else None)
        ctx.synchronize()
        orders.append(m.order().cpu().numpy())
        return q

    out = _both(le, run)
    if (kernel, centering, with_ds) in (("IB_4", "cell", False), ("IB_4", "side", True)):
        idx = np.arange(M, dtype=np.int32)[orders[-1]]
        xs = np.zeros((M, 3))
        Fo = Fn * dsn[:, None] if with_ds else Fn.copy()
        uo = [np.zeros(tuple(a.shape)) for a in out]
        args = (kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw)
        if centering == "side":
            oracle.side_spread(*args, uo, idx, xs, Xn, Fo)
        else:
            oracle.cell_spread(*args, uo[0], idx, xs, Xn, Fo, depth)
        for a in range(len(uo)):
            assert _rel(out[a].cpu().numpy(), uo[a]) <= SPREAD_TOL, f"array {a}"


# --- 4. lists -----------------------------------------------------------------------------

def test_indices_subset(le, oracle):
    kernel = "IB_4"
    geom = le.Geometry.periodic_unit([40, 36, 44], _ghost(le, kernel))
    rng = np.random.default_rng(41)
    M = 12000
    Xn = rng.uniform(0.0, 1.0, (M, 3))
    Fn = rng.standard_normal((M, 3))
    idx = rng.permutation(M)[: M - 3001].astype(np.int32)
    unlisted = np.ones(M, bool)
    unlisted[idx] = False
    Fn[unlisted] = np.nan  # a row the list does not name is never read into a sum
    X, F, I = torch.from_numpy(Xn).cuda(), torch.from_numpy(Fn).cuda(), torch.from_numpy(idx).cuda()
    orders = []

    def run(ctx):
        m = le.Markers(ctx).bin(geom, kernel, X, I)
        q = geom.alloc("side")
        le.spread(ctx, m, kernel, "side", geom, q, F, X)
        ctx.synchronize()
        orders.append(m.order().cpu().numpy())
        return q

    out = _both(le, run)
    uo = [np.zeros(tuple(a.shape)) for a in out]
    oracle.side_spread(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, uo, idx[orders[-1]],
                       np.zeros((idx.size, 3)), Xn, np.nan_to_num(Fn))
    for a in range(3):
        got = out[a].cpu().numpy()
        assert np.isfinite(got).all()
        assert _rel(got, uo[a]) <= SPREAD_TOL, f"comp {a}"


@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
def test_fixed_capacity_list_with_nan_rows(le, kernel):
    """ibtk_le_markers_bin_count: the rows past the device count hold NaN in X and F; no
    stream entry names them, and an idle lane's entry is one of the item's own."""
    geom = le.Geometry.periodic_unit([48, 48, 64], _ghost(le, kernel))
    rng = np.random.default_rng(43)
    cap, M = 12000, 9001
    X = torch.full((cap, 3), float("nan"), dtype=torch.float64, device="cuda")
    F = torch.full((cap, 3), float("nan"), dtype=torch.float64, device="cuda")
    X[:M] = torch.from_numpy(rng.uniform(0.0, 1.0, (M, 3))).cuda()
    F[:M] = torch.from_numpy(rng.standard_normal((M, 3))).cuda()
    n_dev = torch.tensor([M], dtype=torch.int32, device="cuda")

    def run(ctx):
        m = le.Markers(ctx).bin_count(geom, kernel, X, n_dev)
        q = geom.alloc("side")
        le.spread(ctx, m, kernel, "side", geom, q, F, X)
        ctx.synchronize()
        return q

    out = _both(le, run)
    for a in out:
        assert bool(torch.isfinite(a).all())
    # what the first M rows alone spread
    ctx = le.Context(0)
    m = le.Markers(ctx).bin(geom, kernel, X[:M].contiguous())
    q = geom.alloc("side")
    le.spread(ctx, m, kernel, "side", geom, q, F[:M].contiguous(), X[:M].contiguous())
    ctx.synchronize()
    for a, b in zip(out, q):
        assert torch.equal(a, b)


def test_empty_list(le):
    geom = le.Geometry.periodic_unit([16, 16, 16], 3)
    X = torch.zeros((0, 3), dtype=torch.float64, device="cuda")

    def run(ctx):
        m = le.Markers(ctx).bin(geom, "IB_4", X)
        q = geom.alloc("side", fill=1.5)
        le.spread(ctx, m, "IB_4", "side", geom, q, X, X)
        le.zero_ghosts_spread(ctx, m, "IB_4", "side", geom, q, X, X)
        return q

    out = _both(le, run)
    assert all(bool(((a == 1.5) | (a == 0.0)).all()) for a in out)


# --- 5. a level of patches ------------------------------------------------------------------

def _level(le, N, P, g):
    n = N // P
    geoms = []
    for k, j, i in itertools.product(range(P), repeat=3):
        lo = [i * n, j * n, k * n]
        geoms.append(le.Geometry(lo, [v + n - 1 for v in lo], g, [1.0 / N] * 3, [v / N for v in lo]))
    return geoms


def _ghost_box_list(geom, X, N, g):
    """the markers and periodic images whose cell lies in the patch's ghost box"""
    c = np.floor(X * N).astype(np.int64)
    lo, hi = np.array(geom.ilower), np.array(geom.iupper)
    idx, xs = [], []
    for s in itertools.product((-1, 0, 1), repeat=3):
        ci = c + np.array(s) * N
        sel = np.nonzero(np.all((ci >= lo - g) & (ci <= hi + g), axis=1))[0]
        idx.append(sel)
        xs.append(np.tile(np.array(s, np.float64), (sel.size, 1)))
    idx = np.concatenate(idx).astype(np.int32)
    xs = np.concatenate(xs)
    o = np.argsort(idx, kind="stable")
    return idx[o], xs[o]


@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
def test_level(le, oracle, kernel):
    """2 x 2 x 2 patches of 32^3, periodic, ghost-box lists with periodic images:
    zero_spread into junk, then spread on top of it, then both again after a re-binning."""
    N, P = 64, 2
    g = _ghost(le, kernel)
    geoms = _level(le, N, P, g)
    rng = np.random.default_rng(53)
    M = 30000
    Xn = rng.uniform(0.0, 1.0, (M, 3))
    Fn = rng.standard_normal((M, 3))
    X, F = torch.from_numpy(Xn).cuda(), torch.from_numpy(Fn).cuda()
    X2 = torch.remainder(X + 0.4 / N * torch.from_numpy(rng.uniform(-0.5, 0.5, (M, 3))).cuda(), 1.0)
    host = [_ghost_box_list(geom, Xn, N, g) for geom in geoms]
    lists = [(torch.from_numpy(i).cuda(), torch.from_numpy(x).cuda()) for i, x in host]

    def run(ctx):
        lvl = le.Level(ctx, geoms, kernel, X, lists)
        res = []
        for Xc in (X, X2):
            if Xc is X2:
                lvl.rebin(X2)
            f = le.alloc_level(geoms, "side")
            for per in f:
                for a in per:
                    a.fill_(7.0)
            lvl.zero_spread("side", f, F, Xc)
            ctx.synchronize()
            res += [a.clone() for per in f for a in per]
            lvl.spread("side", f, F, Xc)
            ctx.synchronize()
            res += [a for per in f for a in per]
        return res

    out = _both(le, run)
    # patch 5's first zero_spread against the oracle on its ghost-box list
    qp, geom = 5, geoms[5]
    idx, xs = host[qp]
    uo = [np.zeros(tuple(a.shape)) for a in out[3 * qp:3 * qp + 3]]
    oracle.side_spread(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, uo, idx, xs, Xn, Fn)
    for a in range(3):
        assert _rel(out[3 * qp + a].cpu().numpy(), uo[a]) <= SPREAD_TOL, f"patch {qp} comp {a}"

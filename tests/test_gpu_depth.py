"""GPU: cell/node data deeper than 2 and the chunked component launches.

Every interp and spread entry point takes cell- and node-centred data of any depth; the
library cuts the components into launches of MAXC = 4 (le_abi.cpp: interp_impl,
spread_impl, zero_comps), offsets each component's array by ``depth_index * sd`` and
its Q column by ``qcomp`` (make_comps), and the kernels loop or decode over ``ncomp``.
The rest of the suite stops at depth 2; here depths 3 (REC3 gather), 4 (one full launch),
5 (a second launch with first > 0) and 9 (three launches) run through the
single-patch calls, the fused forms, the density-weighted spread, the level calls, the
Fortran shims, the USER_DEFINED path, the ghost operations and mark_stencils.

Every call works inside guard memory: an Eulerian array is the middle of an allocation
two depth planes deeper, Q and F are the middle rows of an array two rows longer, and
the planes, rows (and, for a pitched layout, the row padding) around them must keep
their bits.  A wrong component offset then shows either as a wrong component or as a
touched guard.  Tolerances are the project's (BASELINE.json north_star).
"""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from test_gpu_boundary import KMAP, call_shim  # noqa: E402
from test_gpu_fused import _fill as fill_nan_ghosts  # noqa: E402
from test_gpu_layout import _geoms  # noqa: E402
from test_gpu_level import _lists, _patches  # noqa: E402
from test_gpu_parity import INTERP_TOL, SPREAD_TOL, make_case, oracle_call, rel_err  # noqa: E402
from test_gpu_ref_pin import shim_case  # noqa: E402
from test_gpu_user import KERNELS as USER_KERNELS  # noqa: E402
from test_gpu_user import _use as use_user_kernel  # noqa: E402

SENT = -777.25  # the guards' value
DEV = "cuda:0"
DEPTHS = [3, 4, 5, 9]


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
def lib(le):
    from ibamr_amd import _lib
    return _lib.load()


# --------------------------------------------------------------------------
# guard memory
# --------------------------------------------------------------------------
def _flat(t):
    """every element of t's allocation"""
    return t.as_strided((t.untyped_storage().nbytes() // 8,), (1,), 0)


def _bits(t):
    return t.contiguous().view(torch.int64)


class Eul:
    """The arrays of one centring inside guard memory.  Cell / node: one allocation
    depth + 2 deep (geom's layout, so a pitched one has its row padding too), all SENT,
    the call's array its planes 1 .. depth; side / edge: each component the middle of
    three packed copies.  ``q`` is what the call takes."""

    def __init__(self, geom, centering, depth=1, rng=None, fill=0.0):
        self.depth = depth
        self.full, self.q = [], []
        if centering in ("cell", "node"):
            full = geom.alloc(centering, depth + 2, device=DEV, fill=SENT)[0]
            self.full.append(full)
            self.q.append(full[1:depth + 1])
        else:
            assert not geom.pitched
            for c in range(geom.ncomp(centering)):
                full = torch.full((3,) + tuple(geom.array_shape(centering, c)), SENT, dtype=torch.float64, device=DEV)
                self.full.append(full)
                self.q.append(full[1])
        for v in self.q:
            if rng is not None:
                v.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(v.shape))))
            else:
                v.fill_(fill)
        self.arm()

    def arm(self):
        """take the picture the guards are compared with (after the arrays are set up)"""
        self.snap = [_flat(f).clone() for f in self.full]
        self.q0 = [v.clone() for v in self.q]
        return self

    def set(self, values):
        for v, w in zip(self.q, values):
            v.copy_(w if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w)))
        return self.arm()

    def numpy(self):
        return [v.contiguous().cpu().numpy().copy() for v in self.q]

    def check(self, padding=True):
        """Everything outside the arrays' logical points is as it was, bit for bit.
        padding=False: the row padding between the first and the last point of the
        call's arrays is exempt (ibtk_le_zero_spread zeroes whole spans)."""
        for full, v, snap in zip(self.full, self.q, self.snap):
            flat = _flat(full)
            n = flat.numel()
            inside = torch.zeros(n, dtype=torch.bool, device=flat.device)
            if padding:
                at = torch.as_strided(torch.arange(n, device=flat.device), tuple(v.shape), v.stride(),
                                      v.storage_offset())
                inside[at.reshape(-1)] = True
            else:
                inside[v.storage_offset():v.storage_offset() + v.shape[0] * v.stride(0)] = True
            assert int(inside.sum()) < n
            assert torch.equal(_bits(flat[~inside]), _bits(snap[~inside])), "guard memory was written"

    def unchanged(self):
        self.check()
        for v, w in zip(self.q, self.q0):
            assert torch.equal(_bits(v), _bits(w)), "the array was written"


class Lag:
    """(M, depth) marker data as rows 1 .. M of an (M + 2, depth) array whose first and
    last rows are SENT; NaN rows unless `values`."""

    def __init__(self, M, depth, values=None):
        self.full = torch.full((M + 2, depth), np.nan, dtype=torch.float64, device=DEV)
        self.full[0] = SENT
        self.full[M + 1] = SENT
        self.v = self.full[1:M + 1]
        assert self.v.is_contiguous()
        if values is not None:
            self.v.copy_(values if torch.is_tensor(values) else torch.from_numpy(np.ascontiguousarray(values)))
        self.snap = self.full.clone()

    def check(self):
        assert bool((self.full[0] == SENT).all()) and bool((self.full[-1] == SENT).all()), "a guard row was written"

    def unchanged(self):
        assert torch.equal(_bits(self.full), _bits(self.snap)), "the marker data was written"


def dev_case(kernel, ndim, centering, name, **kw):
    geom, X, idx, xs, _ = make_case(kernel, ndim, centering, seed=zlib.crc32(name.encode()), **kw)
    listed = np.zeros(X.shape[0], bool)
    listed[idx] = True
    return SimpleNamespace(geom=geom, X=X, idx=idx, xs=xs, listed=listed, M=X.shape[0],
                           Xd=torch.from_numpy(X).to(DEV), idd=torch.from_numpy(idx).to(DEV),
                           xsd=torch.from_numpy(xs).to(DEV))


def check_interp(oracle, kernel, centering, c, u_np, Q, depth):
    """Q (a Lag) against the oracle at the listed markers; the others keep their NaN"""
    Q.check()
    Qg = Q.v.cpu().numpy()
    Qo = np.full_like(Qg, np.nan)
    oracle_call(oracle, "interp", kernel, centering, c.geom, u_np, c.idx, c.xs, c.X, Qo, depth)
    assert np.isnan(Qg[~c.listed]).all(), "unlisted markers must be untouched in every column"
    for k in range(depth):
        err = rel_err(Qg[c.listed][:, k], Qo[c.listed][:, k])
        assert err <= INTERP_TOL, f"interp component {k} of {depth}: rel err {err:.3e}"


def check_spread(oracle, kernel, centering, c, u0, ug, F, depth, order, caller_order=True):
    """ug against the oracle started from u0: in the kernel's order and in the caller's"""
    assert sorted(order.tolist()) == list(range(c.idx.size))
    uo = [a.copy() for a in u0]
    oracle_call(oracle, "spread", kernel, centering, c.geom, uo, c.idx[order], c.xs[order], c.X, F.copy(), depth)
    refs = [("the kernel's order", uo)]
    if caller_order:
        uc = [a.copy() for a in u0]
        oracle_call(oracle, "spread", kernel, centering, c.geom, uc, c.idx, c.xs, c.X, F.copy(), depth)
        refs.append(("the caller's order", uc))
    for what, ur in refs:
        for k in range(depth):
            assert not np.array_equal(ur[0][k], u0[0][k]), "the reference spread nothing"
            err = rel_err(ug[0][k], ur[0][k])
            assert err <= SPREAD_TOL, f"spread component {k} of {depth}: rel err {err:.3e} against {what}"


# --------------------------------------------------------------------------
# a. parity against the oracle
# --------------------------------------------------------------------------
PARITY = [(k, nd, c, d) for k in ("IB_4", "IB_6", "BSPLINE_4", "PIECEWISE_LINEAR", "IB_3") for nd in (2, 3)
          for c in ("cell", "node") for d in DEPTHS]


@pytest.mark.parametrize("kernel,ndim,centering,depth", PARITY, ids=lambda v: str(v))
def test_interp_depth_matches_oracle(le, ctx, oracle, kernel, ndim, centering, depth):
    c = dev_case(kernel, ndim, centering, f"di{kernel}{ndim}{centering}{depth}")
    u = Eul(c.geom, centering, depth, np.random.default_rng(11 + depth))
    Q = Lag(c.M, depth)
    m = le.Markers(ctx).bin(c.geom, kernel, c.Xd, c.idd, c.xsd)
    le.interp(ctx, m, kernel, centering, c.geom, u.q, Q.v, c.Xd, q_depth=depth)
    ctx.synchronize()
    u.unchanged()
    check_interp(oracle, kernel, centering, c, u.numpy(), Q, depth)


@pytest.mark.parametrize("kernel,ndim,centering,depth", PARITY, ids=lambda v: str(v))
def test_spread_depth_matches_oracle(le, ctx, oracle, kernel, ndim, centering, depth):
    c = dev_case(kernel, ndim, centering, f"ds{kernel}{ndim}{centering}{depth}")
    rng = np.random.default_rng(12 + depth)
    u = Eul(c.geom, centering, depth, rng)
    u0 = u.numpy()
    Fn = rng.uniform(-1, 1, (c.M, depth))
    F = Lag(c.M, depth, Fn)
    m = le.Markers(ctx).bin(c.geom, kernel, c.Xd, c.idd, c.xsd)
    le.spread(ctx, m, kernel, centering, c.geom, u.q, F.v, c.Xd, q_depth=depth)
    ctx.synchronize()
    u.check()
    F.unchanged()
    check_spread(oracle, kernel, centering, c, u0, u.numpy(), Fn, depth, m.order().cpu().numpy())


# --------------------------------------------------------------------------
# b. depth D = D depth-1 calls, bit for bit
# --------------------------------------------------------------------------
SLICES = [(k, nd, c, d) for k in ("IB_4", "IB_6", "PIECEWISE_LINEAR") for nd in (2, 3) for c in ("cell", "node")
          for d in DEPTHS]


@pytest.mark.parametrize("kernel,ndim,centering,depth", SLICES, ids=lambda v: str(v))
def test_depth_equals_slices(le, ctx, kernel, ndim, centering, depth):
    """One binning, the depth-D call and D depth-1 calls on the slices: the order a point's
    contributions are added in depends on the binning alone, so the results are the same
    bits -- a wrong offset shows even where the values happen to be close."""
    c = dev_case(kernel, ndim, centering, f"sl{kernel}{ndim}{centering}{depth}")
    rng = np.random.default_rng(13 + depth)
    m = le.Markers(ctx).bin(c.geom, kernel, c.Xd, c.idd, c.xsd)
    # interp
    u = Eul(c.geom, centering, depth, rng)
    QD = Lag(c.M, depth)
    le.interp(ctx, m, kernel, centering, c.geom, u.q, QD.v, c.Xd, q_depth=depth)
    Q1 = [Lag(c.M, 1) for _ in range(depth)]
    for k in range(depth):
        le.interp(ctx, m, kernel, centering, c.geom, [u.q[0][k:k + 1]], Q1[k].v, c.Xd, q_depth=1)
    ctx.synchronize()
    u.unchanged()
    QD.check()
    assert not bool(torch.isnan(QD.v[torch.from_numpy(c.listed).to(DEV)]).any())
    for k in range(depth):
        Q1[k].check()
        assert torch.equal(_bits(QD.v[:, k]), _bits(Q1[k].v[:, 0])), f"interp component {k} of {depth}"
    # spread
    F = Lag(c.M, depth, rng.uniform(-1, 1, (c.M, depth)))
    a = Eul(c.geom, centering, depth, rng)
    b = Eul(c.geom, centering, depth).set(a.q)
    le.spread(ctx, m, kernel, centering, c.geom, a.q, F.v, c.Xd, q_depth=depth)
    F1 = [Lag(c.M, 1, F.v[:, k:k + 1].contiguous()) for k in range(depth)]
    for k in range(depth):
        le.spread(ctx, m, kernel, centering, c.geom, [b.q[0][k:k + 1]], F1[k].v, c.Xd, q_depth=1)
    ctx.synchronize()
    a.check()
    b.check()
    F.unchanged()
    for k in range(depth):
        assert not torch.equal(a.q[0][k], a.q0[0][k])
        assert torch.equal(a.q[0][k], b.q[0][k]), f"spread component {k} of {depth}"


# --------------------------------------------------------------------------
# c. more than one column, and full chunks
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
@pytest.mark.parametrize("centering,depth", [("cell", 5), ("node", 4)])
def test_depth_multi_column_packed_and_pitched(le, ctx, oracle, kernel, centering, depth):
    """test_pitched_equals_packed's geometry (several sweep columns, markers to two cells
    outside the box): against the oracle, pitched = packed bit for bit, padding kept."""
    N = (45, 38, 29)
    g = oracle.min_ghost_width(kernel)
    gp, ga = _geoms(le, N, g, ilower=(3, -5, 7))
    assert ga.pitch[0] % 16 == 0 and ga.pitch[0] > N[0] + 2 * g
    rng = np.random.default_rng(11)
    M = 6000
    lo, hi, dx = np.array(gp.x_lower), np.array(gp.x_upper), np.array(gp.dx)
    Xn = rng.uniform(lo - 2 * dx, hi + 2 * dx, (M, 3))
    c = SimpleNamespace(geom=gp, X=Xn, idx=np.arange(M, dtype=np.int32), xs=np.zeros((M, 3)),
                        listed=np.ones(M, bool), M=M, Xd=torch.from_numpy(Xn).to(DEV))
    Fn = rng.standard_normal((M, depth))
    m = le.Markers(ctx).bin(gp, kernel, c.Xd)
    up = Eul(gp, centering, depth, rng)
    ua = Eul(ga, centering, depth).set(up.q)
    Qp, Qa = Lag(M, depth), Lag(M, depth)
    le.interp(ctx, m, kernel, centering, gp, up.q, Qp.v, c.Xd, q_depth=depth)
    le.interp(ctx, m, kernel, centering, ga, ua.q, Qa.v, c.Xd, q_depth=depth)
    fp = Eul(gp, centering, depth, rng)
    fa = Eul(ga, centering, depth).set(fp.q)
    f0 = fp.numpy()
    Fp, Fa = Lag(M, depth, Fn), Lag(M, depth, Fn)
    le.spread(ctx, m, kernel, centering, gp, fp.q, Fp.v, c.Xd, q_depth=depth)
    le.spread(ctx, m, kernel, centering, ga, fa.q, Fa.v, c.Xd, q_depth=depth)
    ctx.synchronize()
    up.unchanged()
    ua.unchanged()  # the row padding among it
    fp.check()
    fa.check()
    Fp.unchanged()
    Fa.unchanged()
    assert torch.equal(_bits(Qp.full), _bits(Qa.full)), "interp: pitched != packed"
    assert torch.equal(fp.q[0], fa.q[0]), "spread: pitched != packed"
    check_interp(oracle, kernel, centering, c, up.numpy(), Qp, depth)
    check_spread(oracle, kernel, centering, c, f0, fp.numpy(), Fn, depth, m.order().cpu().numpy())


def test_depth_dense_bit_stable(le, ctx, oracle):
    """test_spread_bit_stable_dense's markers (many per cell, half of them at one point), cell
    depth 5: two runs alike bit for bit and within tolerance of the oracle in kernel order."""
    kernel, depth = "IB_4", 5
    geom = le.Geometry.periodic_unit([24, 24, 24], oracle.min_ghost_width(kernel) + 1)
    gen = torch.Generator(device=DEV).manual_seed(4)
    M = 30_000
    X = 0.40 + 0.05 * torch.rand((M, 3), dtype=torch.float64, device=DEV, generator=gen)
    X[: M // 2] = X[0]
    Fn = (torch.rand((M, depth), dtype=torch.float64, device=DEV, generator=gen) - 0.5).cpu().numpy()
    outs = []
    for rep in range(2):
        q = Eul(geom, "cell", depth)
        F = Lag(M, depth, Fn)
        m = le.Markers(ctx).bin(geom, kernel, X)
        le.spread(ctx, m, kernel, "cell", geom, q.q, F.v, X, q_depth=depth)
        ctx.synchronize()
        q.check()
        F.unchanged()
        outs.append(q)
    assert torch.equal(outs[0].q[0], outs[1].q[0])
    c = SimpleNamespace(geom=geom, X=X.cpu().numpy(), idx=np.arange(M, dtype=np.int32), xs=np.zeros((M, 3)))
    check_spread(oracle, kernel, "cell", c, [np.zeros(tuple(outs[0].q[0].shape))], outs[0].numpy(), Fn, depth,
                 m.order().cpu().numpy(), caller_order=False)


# --------------------------------------------------------------------------
# d. fused forms = their two calls, bit for bit
# --------------------------------------------------------------------------
FUSED = [(3, c, d, p) for c in ("cell", "node") for d in (5, 9) for p in (False, True)] + [(2, "cell", 5, False)]


def _lower_half(c):
    """markers in the lower half of the slowest dim only: items that own points and no candidate"""
    a = c.geom.ndim - 1
    L = (c.geom.iupper[a] - c.geom.ilower[a] + 1) * c.geom.dx[a]
    c.X[:, a] = np.minimum(c.X[:, a], c.geom.x_lower[a] + 0.45 * L)
    c.Xd = torch.from_numpy(c.X).to(DEV)


@pytest.mark.parametrize("ndim,centering,depth,pitched", FUSED, ids=lambda v: str(v))
def test_zero_spread_depth(le, ctx, ndim, centering, depth, pitched):
    kernel = "IB_4"
    c = dev_case(kernel, ndim, centering, f"zs{ndim}{centering}{depth}", M=400)
    _lower_half(c)
    geom = c.geom.aligned() if pitched else c.geom
    F = Lag(c.M, depth, np.random.default_rng(53).uniform(-1, 1, (c.M, depth)))
    m = le.Markers(ctx).bin(geom, kernel, c.Xd, c.idd, c.xsd)
    a = Eul(geom, centering, depth, fill=0.0)
    b = Eul(geom, centering, depth, fill=float("nan"))
    le.spread(ctx, m, kernel, centering, geom, a.q, F.v, c.Xd, q_depth=depth)
    le.zero_spread(ctx, m, kernel, centering, geom, b.q, F.v, c.Xd, q_depth=depth)
    ctx.synchronize()
    a.check()
    b.check(padding=False)
    F.unchanged()
    assert not bool(torch.isnan(b.q[0]).any()), "a point was left unwritten"
    for k in range(depth):
        assert bool(a.q[0][k].any())
        assert torch.equal(a.q[0][k], b.q[0][k]), f"component {k} of {depth}"


@pytest.mark.parametrize("ndim,centering,depth,pitched", FUSED, ids=lambda v: str(v))
def test_zero_ghosts_spread_depth(le, ctx, ndim, centering, depth, pitched):
    kernel = "IB_4"
    c = dev_case(kernel, ndim, centering, f"zg{ndim}{centering}{depth}", M=400)
    _lower_half(c)
    geom = c.geom.aligned() if pitched else c.geom
    rng = np.random.default_rng(31)
    F = Lag(c.M, depth, rng.uniform(-1, 1, (c.M, depth)))
    m = le.Markers(ctx).bin(geom, kernel, c.Xd, c.idd, c.xsd)
    a = Eul(geom, centering, depth)
    fill_nan_ghosts(a.q, geom, centering, rng)  # random interior (kept, added to), NaN ghosts (all written)
    a.arm()
    b = Eul(geom, centering, depth).set(a.q)
    le.zero_ghosts(ctx, geom, centering, a.q, q_depth=depth)
    le.spread(ctx, m, kernel, centering, geom, a.q, F.v, c.Xd, q_depth=depth)
    le.zero_ghosts_spread(ctx, m, kernel, centering, geom, b.q, F.v, c.Xd, q_depth=depth)
    ctx.synchronize()
    a.check()
    b.check()
    F.unchanged()
    assert not bool(torch.isnan(b.q[0]).any()), "a ghost point was left unwritten"
    for k in range(depth):
        assert torch.equal(a.q[0][k], b.q[0][k]), f"component {k} of {depth}"


@pytest.mark.parametrize("ndim,centering,depth,pitched", FUSED, ids=lambda v: str(v))
@pytest.mark.parametrize("partial", [False, True])
def test_fill_interp_depth(le, ctx, oracle, ndim, centering, depth, pitched, partial):
    """ibtk_le_fill_interp = ibtk_le_fill_periodic_ghosts, then ibtk_le_interp; the fused 3-D
    call reads no ghost of a periodic dim (NaN there when all dims are periodic) and writes
    nothing.  2-D: the two calls."""
    kernel = "IB_4"
    periodic = [1, 1, 0][:ndim] if partial else [1] * ndim
    if ndim == 2 and partial:
        periodic = [1, 0]
    geom = le.Geometry.periodic_unit([16, 20, 24][:ndim], oracle.min_ghost_width(kernel))
    if pitched:
        geom = geom.aligned()
    rng = np.random.default_rng(zlib.crc32(f"fi{ndim}{centering}{depth}".encode()))
    M = 500
    X = rng.uniform(-0.05, 1.05, (M, ndim))
    idx = rng.permutation(M)[: M - 37].astype(np.int32)
    listed = np.zeros(M, bool)
    listed[idx] = True
    Xd, idd = torch.from_numpy(X).to(DEV), torch.from_numpy(idx).to(DEV)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd)
    a = Eul(geom, centering, depth, rng)
    b = Eul(geom, centering, depth).set(a.q)
    fused = ndim == 3
    if fused and not partial:
        fill_nan_ghosts(b.q, geom, centering, rng)  # NaN ghosts, new interior values ...
        keep = ~torch.isnan(b.q[0])
        a.q[0][keep] = b.q[0][keep]                 # ... the same interior in a
        a.arm()
        b.arm()
    Qa, Qb = Lag(M, depth), Lag(M, depth)
    le.fill_periodic_ghosts(ctx, geom, centering, a.q, q_depth=depth, periodic=periodic)
    le.interp(ctx, m, kernel, centering, geom, a.q, Qa.v, Xd, q_depth=depth)
    le.fill_interp(ctx, m, kernel, centering, geom, b.q, Qb.v, Xd, q_depth=depth, periodic=periodic)
    ctx.synchronize()
    a.check()
    if fused:
        b.unchanged()
    else:
        b.check()
        assert torch.equal(a.q[0], b.q[0])
    Qa.check()
    Qb.check()
    lt = torch.from_numpy(listed).to(DEV)
    assert bool(torch.isnan(Qb.v[~lt]).all()), "unlisted markers must be untouched in every column"
    assert not bool(torch.isnan(Qb.v[lt]).any()), "a NaN ghost was read"
    assert torch.equal(_bits(Qa.full), _bits(Qb.full))
    assert len({Qb.v[lt][:, k].cpu().numpy().tobytes() for k in range(depth)}) == depth


# --------------------------------------------------------------------------
# e. density-weighted spread
# --------------------------------------------------------------------------
@pytest.mark.parametrize("ndim,depth", [(3, 3), (3, 5), (2, 5)])
@pytest.mark.parametrize("kernel", ["IB_4", "BSPLINE_4"])
def test_spread_ds_depth(le, ctx, oracle, kernel, ndim, depth):
    """spread(F, ds) on cell data (3-D depth 3: the whole-record gather with ds): the oracle's
    spread of the numpy product F * ds, and bit for bit spread(F * ds) on the same binning."""
    c = dev_case(kernel, ndim, "cell", f"dw{kernel}{ndim}{depth}")
    rng = np.random.default_rng(20 + depth)
    Fn = rng.standard_normal((c.M, depth))
    dsn = rng.random(c.M) * 1e-3 + 1e-4
    FDn = Fn * dsn[:, None]  # rounded once
    F, FD, ds = Lag(c.M, depth, Fn), Lag(c.M, depth, FDn), Lag(c.M, 1, dsn[:, None])
    m = le.Markers(ctx).bin(c.geom, kernel, c.Xd, c.idd, c.xsd)
    a = Eul(c.geom, "cell", depth, rng)
    b = Eul(c.geom, "cell", depth).set(a.q)
    u0 = a.numpy()
    le.spread(ctx, m, kernel, "cell", c.geom, a.q, F.v, c.Xd, q_depth=depth, ds=ds.v)
    le.spread(ctx, m, kernel, "cell", c.geom, b.q, FD.v, c.Xd, q_depth=depth)
    ctx.synchronize()
    a.check()
    b.check()
    for t in (F, FD, ds):
        t.unchanged()
    for k in range(depth):
        assert torch.equal(a.q[0][k], b.q[0][k]), f"component {k} of {depth}"
    check_spread(oracle, kernel, "cell", c, u0, a.numpy(), FDn, depth, m.order().cpu().numpy())


# --------------------------------------------------------------------------
# f. a second launch of three components
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["IB_4", "BSPLINE_4"])
def test_interp_depth7_matches_oracle(le, ctx, oracle, kernel):
    """Cell depth 7 in 3-D: the second launch covers Q columns 4, 5, 6 of 7 -- three components
    with first > 0, which none of DEPTHS gives (5: one, 9: four and one)."""
    depth = 7
    c = dev_case(kernel, 3, "cell", f"d7{kernel}")
    u = Eul(c.geom, "cell", depth, np.random.default_rng(11 + depth))
    Q = Lag(c.M, depth)
    m = le.Markers(ctx).bin(c.geom, kernel, c.Xd, c.idd, c.xsd)
    le.interp(ctx, m, kernel, "cell", c.geom, u.q, Q.v, c.Xd, q_depth=depth)
    ctx.synchronize()
    u.unchanged()
    check_interp(oracle, kernel, "cell", c, u.numpy(), Q, depth)


# --------------------------------------------------------------------------
# g. level
# --------------------------------------------------------------------------
def _level_case(le, N, M, depth, seed):
    kernel, P, g = "IB_4", 2, 3
    geoms = _patches(le, N, P, g)
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (M, 3))
    host = [_lists(geom, X, N, g) for geom in geoms]
    Xd = torch.from_numpy(X).to(DEV)
    lists_i = [(torch.from_numpy(h[0]).to(DEV), None) for h in host]
    lists_s = [(torch.from_numpy(h[1]).to(DEV), torch.from_numpy(h[2]).to(DEV)) for h in host]
    return SimpleNamespace(kernel=kernel, geoms=geoms, rng=rng, X=X, Xd=Xd, host=host, lists_i=lists_i,
                           lists_s=lists_s, M=M)


@pytest.mark.parametrize("centering,depth", [("cell", 4), ("node", 3)])
def test_level_depth(le, ctx, oracle, centering, depth):
    """The level calls on the patches of test_level_matches_patch_by_patch (P = 2 a dim)
    against the single-patch calls patch by patch: interp bit for bit, spread within 1e-12
    (and of the oracle), zero_spread = spread into zeros and fill_interp = fill_ghosts +
    interp bit for bit."""
    from ibamr_amd._lib import IBTKLEError
    L = _level_case(le, 96, 20_000, depth, 5)
    kernel, geoms, rng, M = L.kernel, L.geoms, L.rng, L.M
    Fn = rng.uniform(-1, 1, (M, depth))
    F = Lag(M, depth, Fn)
    ue = [Eul(geom, centering, depth, rng) for geom in geoms]
    u = [e.q for e in ue]
    lvl_i = le.Level(ctx, geoms, kernel, L.Xd, L.lists_i)
    U = Lag(M, depth)
    lvl_i.interp(centering, u, U.v, L.Xd, q_depth=depth)
    lvl_s = le.Level(ctx, geoms, kernel, L.Xd, L.lists_s)
    fe = [Eul(geom, centering, depth, fill=0.0) for geom in geoms]
    f = [e.q for e in fe]
    lvl_s.spread(centering, f, F.v, L.Xd, q_depth=depth)
    ze = [Eul(geom, centering, depth, fill=float("nan")) for geom in geoms]
    z = [e.q for e in ze]
    lvl_s.zero_spread(centering, z, F.v, L.Xd, q_depth=depth)
    ctx.synchronize()
    U.check()
    F.unchanged()
    Ug = U.v.cpu().numpy()
    assert not np.isnan(Ug).any(), "every marker is interior to exactly one patch"
    for q, geom in enumerate(geoms):
        interior, idx, xs = L.host[q]
        ue[q].unchanged()
        fe[q].check()
        ze[q].check()
        assert not bool(torch.isnan(z[q][0]).any()), f"patch {q}: points not written"
        assert torch.equal(z[q][0], f[q][0]), f"patch {q}: zero_spread"
        m = le.Markers(ctx).bin(geom, kernel, L.Xd, L.lists_i[q][0])
        U1 = Lag(M, depth)
        le.interp(ctx, m, kernel, centering, geom, u[q], U1.v, L.Xd, q_depth=depth)
        ms = le.Markers(ctx).bin(geom, kernel, L.Xd, *L.lists_s[q])
        f1 = Eul(geom, centering, depth, fill=0.0)
        le.spread(ctx, ms, kernel, centering, geom, f1.q, F.v, L.Xd, q_depth=depth)
        ctx.synchronize()
        assert np.array_equal(Ug[interior], U1.v.cpu().numpy()[interior]), f"patch {q} interp"
        got, one = f[q][0].cpu().numpy(), f1.q[0].cpu().numpy()
        uo = [np.zeros(got.shape)]
        oracle_call(oracle, "spread", kernel, centering, geom, uo, idx, xs, L.X, Fn.copy(), depth)
        for k in range(depth):
            assert np.abs(one[k]).max() > 0
            err = rel_err(got[k], one[k])
            assert err <= SPREAD_TOL, f"patch {q} comp {k}: rel err {err:.2e} against the single-patch spread"
            err = rel_err(got[k], uo[0][k])
            assert err <= SPREAD_TOL, f"patch {q} comp {k}: rel err {err:.2e} against the oracle"
    # fill_interp
    be = [Eul(geom, centering, depth).set(e.q) for geom, e in zip(geoms, ue)]
    b = [e.q for e in be]
    Qa, Qb = Lag(M, depth), Lag(M, depth)
    if centering == "node":  # the level ghost fill takes side and cell data (ibtk_le.h)
        with pytest.raises(IBTKLEError, match="side or cell data") as e:
            lvl_i.fill_interp(centering, b, Qb.v, L.Xd, q_depth=depth)
        assert e.value.code == 4
        ctx.synchronize()
        Qb.unchanged()
        for x in be:
            x.unchanged()
        return
    lvl_i.fill_ghosts(centering, u, q_depth=depth)
    lvl_i.interp(centering, u, Qa.v, L.Xd, q_depth=depth)
    lvl_i.fill_interp(centering, b, Qb.v, L.Xd, q_depth=depth)
    ctx.synchronize()
    assert not bool(torch.isnan(Qb.v).any())
    assert torch.equal(Qa.full, Qb.full), "fill_interp against fill_ghosts + interp"
    for q, geom in enumerate(geoms):
        ue[q].check()
        be[q].check()
        assert torch.equal(u[q][0], b[q][0]), f"patch {q}: the filled arrays"  # (depth > 1: the two calls)
        interior = L.host[q][0]
        m = le.Markers(ctx).bin(geom, kernel, L.Xd, L.lists_i[q][0])
        U1 = Lag(M, depth)
        le.interp(ctx, m, kernel, centering, geom, u[q], U1.v, L.Xd, q_depth=depth)
        ctx.synchronize()
        assert np.array_equal(Qb.v.cpu().numpy()[interior], U1.v.cpu().numpy()[interior]), f"patch {q} fill_interp"


@pytest.mark.parametrize("centering", ["cell", "node"])
def test_level_refuses_depth_5(le, ctx, centering):
    """A level call takes at most MAXC = 4 components: depth 5 is refused by every call, and
    nothing is written -- no array point, no Q row, no ghost by fill_interp's fill."""
    from ibamr_amd._lib import IBTKLEError
    depth = 5
    L = _level_case(le, 48, 2000, depth, 6)
    geoms, M = L.geoms, L.M
    F = Lag(M, depth, L.rng.uniform(-1, 1, (M, depth)))
    Q = Lag(M, depth)
    ue = [Eul(geom, centering, depth, L.rng) for geom in geoms]
    u = [e.q for e in ue]
    lvl = le.Level(ctx, geoms, L.kernel, L.Xd, L.lists_s)
    for call in (lambda: lvl.interp(centering, u, Q.v, L.Xd, q_depth=depth),
                 lambda: lvl.spread(centering, u, F.v, L.Xd, q_depth=depth),
                 lambda: lvl.zero_spread(centering, u, F.v, L.Xd, q_depth=depth),
                 lambda: lvl.fill_interp(centering, u, Q.v, L.Xd, q_depth=depth)):
        with pytest.raises(IBTKLEError, match="at most 4 components") as e:
            call()
        assert e.value.code == 4
    ctx.synchronize()
    Q.unchanged()
    F.unchanged()
    for x in ue:
        x.unchanged()


# --------------------------------------------------------------------------
# h. Fortran shims
# --------------------------------------------------------------------------
@pytest.mark.parametrize("against", ["oracle", "reference"])
@pytest.mark.parametrize("depth", [5, 9])
@pytest.mark.parametrize("kernel", ["IB_4", "PIECEWISE_CUBIC"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_fortran_shims_depth(lib, oracle, against, ndim, kernel, depth):
    """lagrangian_<k>_{interp,spread}{2,3}d_ of libibtk_le.so (host memory, the Fortran's
    argument tuple) with depth 5 and 9 and a list that names markers twice: interp bit for
    bit, spread within 1e-12, against the oracle and the compiled reference Fortran."""
    if against == "oracle":
        ref_interp, ref_spread = oracle.interp, oracle.spread
    else:
        from oracle import ref
        if not ref.available():
            pytest.skip("oracle/_ref/libleref_{O0,O2}.so absent (built where the reference tree and flang are)")
        ref_interp, ref_spread = ref.interp, ref.spread
    geo, X, idx, xs, rng = shim_case(oracle, kernel, ndim, "box")
    ilo, ihi, g, dx, xlo = geo["ilo"], geo["ihi"], geo["g"], geo["dx"], geo["xlo"]
    M = X.shape[0]
    shape = oracle.ghost_shape(ilo, ihi, g, depth)
    ufull = np.full((depth + 2,) + shape[1:], SENT)
    u = ufull[1:depth + 1]
    u[...] = rng.uniform(-1, 1, shape)
    u0 = u.copy()
    Vfull = np.full((M + 2, depth), SENT)
    V = Vfull[1:M + 1]
    V[...] = 7.0
    call_shim(lib, "interp", KMAP[kernel], ndim, dx, xlo, ilo, ihi, g, u, idx, xs, X, V, depth)
    Vr = np.full((M, depth), 7.0)
    ref_interp(kernel, dx, xlo, ilo, ihi, g, u0, idx, xs, X, Vr, depth=depth)
    assert np.array_equal(V, Vr)
    assert (Vfull[0] == SENT).all() and (Vfull[-1] == SENT).all() and np.array_equal(u, u0)
    assert len({Vr[idx][:, k].tobytes() for k in range(depth)}) == depth
    F = rng.uniform(-1, 1, (M, depth))
    F0 = F.copy()
    call_shim(lib, "spread", KMAP[kernel], ndim, dx, xlo, ilo, ihi, g, u, idx, xs, X, F, depth)
    ur = u0.copy()
    ref_spread(kernel, dx, xlo, ilo, ihi, g, ur, idx, xs, X, F0, depth=depth)
    assert np.array_equal(F, F0)
    assert (ufull[0] == SENT).all() and (ufull[-1] == SENT).all(), "a guard plane was written"
    for k in range(depth):
        assert not np.array_equal(ur[k], u0[k])
        err = rel_err(u[k], ur[k])
        assert err <= 1e-12, f"component {k} of {depth}: rel err {err:.3e}"


# --------------------------------------------------------------------------
# i. USER_DEFINED
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "phi3"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_user_depth(le, ctx, oracle, name, ndim):
    """user_interp / user_spread on cell depth 5 (a make_comps call per component) against the
    oracle's USER_DEFINED: bit for bit, as at depth 2 (tests/test_gpu_user.py)."""
    depth, cent = 5, "cell"
    use_user_kernel(le, oracle, name)
    try:
        assert USER_KERNELS[name][1] in (3, 4)
        c = dev_case("USER_DEFINED", ndim, cent, f"us{name}{ndim}")
        idx = np.concatenate([c.idx, c.idx[:7]]).astype(np.int32)  # markers named twice
        xs = np.concatenate([c.xs, c.xs[:7]])
        idd, xsd = torch.from_numpy(idx).to(DEV), torch.from_numpy(xs).to(DEV)
        rng = np.random.default_rng(3)
        u = Eul(c.geom, cent, depth, rng)
        Q = Lag(c.M, depth)
        le.user_interp(ctx, cent, c.geom, u.q, Q.v, c.Xd, idd, xsd, q_depth=depth)
        ctx.synchronize()
        u.unchanged()
        Q.check()
        Qg = Q.v.cpu().numpy()
        Qo = np.full_like(Qg, np.nan)
        oracle_call(oracle, "interp", "USER_DEFINED", cent, c.geom, u.numpy(), idx, xs, c.X, Qo, depth)
        assert np.isnan(Qg[~c.listed]).all(), "unlisted markers must be untouched in every column"
        assert not np.isnan(Qo[c.listed]).any()
        assert np.array_equal(Qg[c.listed], Qo[c.listed]), f"interp rel err {rel_err(Qg[c.listed], Qo[c.listed]):.3e}"
        Fn = rng.uniform(-1, 1, (c.M, depth))
        F = Lag(c.M, depth, Fn)
        uo = u.numpy()
        le.user_spread(ctx, cent, c.geom, u.q, F.v, c.Xd, idd, xsd, q_depth=depth)
        ctx.synchronize()
        u.check()
        F.unchanged()
        u_before = [a.copy() for a in uo]
        oracle_call(oracle, "spread", "USER_DEFINED", cent, c.geom, uo, idx, xs, c.X, Fn.copy(), depth)
        ug = u.numpy()
        for k in range(depth):
            assert not np.array_equal(uo[0][k], u_before[0][k])
            assert np.array_equal(ug[0][k], uo[0][k]), f"component {k}: rel err {rel_err(ug[0][k], uo[0][k]):.3e}"
    finally:
        le.set_user_kernel(None, 4)
        oracle.set_user_kernel(None, 4)


# --------------------------------------------------------------------------
# j. ghost operations
# --------------------------------------------------------------------------
def np_ghost_op(op, u, geom, centering, per):
    """The periodic ghost fill (wrap-copy), fold (wrap-add, slowest dim first, the dims below
    over the whole ghost box, the periodic dims above over the interior) and ghost zero of a
    (depth, [z,] y, x) array, restated in numpy.  The interior of a dim is its cells'
    index range; a node array's last point is the image of its first."""
    nd = geom.ndim
    ext = geom.ext_mask(centering)
    g = list(geom.gcw)
    N = [geom.iupper[d] - geom.ilower[d] + 1 for d in range(nd)]
    n = [N[d] + 2 * g[d] + ((ext >> d) & 1) for d in range(nd)]
    assert tuple(u.shape[1:]) == tuple(reversed(n))
    A = [np.arange(n[d]) for d in range(nd)]
    I = [np.arange(g[d], g[d] + N[d]) for d in range(nd)]
    G = [np.concatenate([np.arange(g[d]), np.arange(g[d] + N[d], n[d])]) for d in range(nd)]
    K = np.arange(u.shape[0])

    def wrap(j, d):
        return g[d] + (j - g[d]) % N[d]

    def at(sel):  # sel[d]: the indices of dim d (x = dim 0 is the last axis)
        return np.ix_(K, *[sel[d] for d in reversed(range(nd))])

    out = u.copy()
    if op == "zero":
        for d in range(nd):
            sel = list(A)
            sel[d] = G[d]
            out[at(sel)] = 0.0
    elif op == "fill":
        out = u[at([wrap(A[d], d) if per[d] else A[d] for d in range(nd)])]
    else:
        for d in reversed(range(nd)):
            if not per[d]:
                continue
            src, dst = [], []
            for e in range(nd):
                if e == d:
                    src.append(G[d])
                    dst.append(wrap(G[d], d))
                else:
                    r = A[e] if (e < d or not per[e]) else I[e]
                    src.append(r)
                    dst.append(r)
            assert np.unique(dst[d]).size == dst[d].size, "one source per destination"
            out[at(dst)] = out[at(dst)] + out[at(src)]
    return out


GHOST = [(nd, c, d, p) for nd in (2, 3) for (c, d) in (("cell", 5), ("cell", 16), ("node", 5)) for p in (False, True)
         if not (p and (nd == 2 or d == 16))]


@pytest.mark.parametrize("ndim,centering,depth,pitched", GHOST, ids=lambda v: str(v))
@pytest.mark.parametrize("op,partial", [("fill", False), ("fill", True), ("fold", False), ("fold", True),
                                        ("zero", False)])
def test_ghost_ops_depth(le, ctx, op, partial, ndim, centering, depth, pitched):
    """fill / fold / zero of the ghost layers of every depth plane (16: the calls' limit)
    against the numpy restatement, bit for bit: values are multiples of 1/64, so the fold's
    sums of images are exact whatever their order."""
    geom = make_case("IB_4", ndim, centering, seed=1)[0]
    if pitched:
        geom = geom.aligned()
    per = ([1, 0, 1] if partial else [1, 1, 1])[:ndim]
    rng = np.random.default_rng(zlib.crc32(f"gh{op}{ndim}{centering}{depth}".encode()))
    u = Eul(geom, centering, depth)
    v = rng.integers(-512, 513, tuple(u.q[0].shape)).astype(np.float64) / 64.0
    u.set([v])
    if op == "fill":
        le.fill_periodic_ghosts(ctx, geom, centering, u.q, q_depth=depth, periodic=per)
    elif op == "fold":
        le.fold_periodic_ghosts(ctx, geom, centering, u.q, q_depth=depth, periodic=per)
    else:
        le.zero_ghosts(ctx, geom, centering, u.q, q_depth=depth)
    ctx.synchronize()
    u.check()
    want = np_ghost_op(op, v, geom, centering, per)
    assert not np.array_equal(want, v)
    got = u.numpy()[0]
    for k in range(depth):
        assert np.array_equal(got[k], want[k]), f"{op}: depth plane {k} of {depth}"


@pytest.mark.parametrize("centering", ["cell", "node"])
def test_ghost_ops_refuse_depth_17(le, ctx, centering):
    """The ghost operations take at most 16 arrays a call (ibtk_le.h): depth 17 is
    IBTK_LE_ERR_ARG, "too many arrays", and nothing is written."""
    from ibamr_amd._lib import IBTKLEError
    geom = make_case("IB_4", 3, centering, seed=1)[0]
    u = Eul(geom, centering, 17, np.random.default_rng(2))
    for call in (lambda: le.fill_periodic_ghosts(ctx, geom, centering, u.q, q_depth=17),
                 lambda: le.fold_periodic_ghosts(ctx, geom, centering, u.q, q_depth=17),
                 lambda: le.zero_ghosts(ctx, geom, centering, u.q, q_depth=17)):
        with pytest.raises(IBTKLEError, match="too many arrays") as e:
            call()
        assert e.value.code == 4
    ctx.synchronize()
    u.unchanged()


# --------------------------------------------------------------------------
# k. mark_stencils
# --------------------------------------------------------------------------
def mark_reference(oracle, kernel, centering, geom, idx, xs, X, depth):
    """(array != 0) after the oracle spreads F = 1 from every listed entry into zero arrays:
    the points some clipped stencil touches, where the weights are positive throughout."""
    nd = geom.ndim
    Qd = nd if centering in ("side", "edge") else depth
    u = [np.zeros(geom.array_shape(centering, a, depth)) for a in range(geom.ncomp(centering))]
    if idx.size:
        oracle_call(oracle, "spread", kernel, centering, geom, u, idx, xs, X, np.ones((X.shape[0], Qd)), depth)
    return [a != 0 for a in u]


MARK = [("side", 2, 1, False), ("side", 3, 1, False), ("cell", 3, 4, False), ("node", 3, 2, False),
        ("side", 3, 1, True)]


@pytest.mark.parametrize("centering,ndim,depth,pitched", MARK, ids=lambda v: str(v))
@pytest.mark.parametrize("kernel", ["PIECEWISE_LINEAR", "IB_4", "BSPLINE_4"])
def test_mark_stencils(le, ctx, oracle, kernel, centering, ndim, depth, pitched):
    """ibtk_le_mark_stencils (k_mark; bench.py's algorithmic-byte count) against the oracle's
    spread of ones: with make_case's index list, shifts, ghost-layer and far markers the mask
    is exactly the set of points the spread changes.  The five markers on exact cell faces
    have a zero weight at a stencil edge that the mask rightly marks: without them equality,
    with them the spread's points are a subset of the mask."""
    c = dev_case(kernel, ndim, centering, f"mk{kernel}{ndim}{centering}")
    geom = c.geom.aligned() if pitched else c.geom
    for ties in (False, True):
        keep = np.ones(c.idx.size, bool) if ties else ~((c.idx >= 5) & (c.idx < 10))
        idx, xs = np.ascontiguousarray(c.idx[keep]), np.ascontiguousarray(c.xs[keep])
        want = mark_reference(oracle, kernel, centering, c.geom, idx, xs, c.X, depth)
        assert all(int(w.sum()) > 0 for w in want)
        # entries whose (shifted) position is a stencil's reach beyond the ghost box mark nothing
        Xs = c.X[idx] + xs
        lo = np.array(c.geom.x_lower) - (np.array(c.geom.gcw) + 6) * np.array(c.geom.dx)
        hi = np.array(c.geom.x_upper) + (np.array(c.geom.gcw) + 6) * np.array(c.geom.dx)
        far = np.any((Xs < lo) | (Xs > hi), axis=1)
        assert far.sum() >= 3
        none = mark_reference(oracle, kernel, centering, c.geom, idx[far], xs[far], c.X, depth)
        assert all(int(w.sum()) == 0 for w in none), "a far marker's clipped stencil is empty"
        m = le.Markers(ctx).bin(geom, kernel, c.Xd, torch.from_numpy(idx).to(DEV), torch.from_numpy(xs).to(DEV))
        masks = le.mark_stencils(ctx, m, kernel, centering, geom, c.Xd, q_depth=depth)
        ctx.synchronize()
        assert len(masks) == len(want)
        for a, (mk, w) in enumerate(zip(masks, want)):
            got = mk.cpu().numpy()
            assert got.shape == w.shape and set(np.unique(got)) <= {0, 1}
            if ties:
                assert not (w & (got == 0)).any(), f"array {a}: a spread point is not marked"
            else:
                for k in range(w.shape[0] if w.ndim > ndim else 1):
                    gk, wk = (got[k], w[k]) if w.ndim > ndim else (got, w)
                    assert np.array_equal(gk == 1, wk), \
                        f"array {a} depth {k}: {int((gk == 1).sum())} marked, {int(wk.sum())} spread to"


@pytest.mark.parametrize("ndim", [2, 3])
def test_mark_stencils_ib6_one_marker(le, ctx, ndim):
    """One IB_6 marker at a generic position at the box centre: 6**ndim points a component."""
    geom = make_case("IB_6", ndim, "side", seed=1)[0]
    x = [0.5 * (geom.x_lower[d] + geom.x_upper[d]) + 0.2371 * geom.dx[d] for d in range(ndim)]
    X = torch.tensor([x], dtype=torch.float64, device=DEV)
    m = le.Markers(ctx).bin(geom, "IB_6", X)
    for centering, depth in (("side", 1), ("cell", 4), ("node", 3)):
        masks = le.mark_stencils(ctx, m, "IB_6", centering, geom, X, q_depth=depth)
        ctx.synchronize()
        for mk in masks:
            planes = mk.reshape((depth, -1)) if centering in ("cell", "node") else mk.reshape((1, -1))
            assert [int(p.sum()) for p in planes] == [6 ** ndim] * planes.shape[0], centering


def test_mark_stencils_refuses_depth_5(le, ctx):
    from ibamr_amd._lib import IBTKLEError
    c = dev_case("IB_4", 3, "cell", "mk5")
    m = le.Markers(ctx).bin(c.geom, "IB_4", c.Xd, c.idd, c.xsd)
    with pytest.raises(IBTKLEError, match="at most 4 components") as e:
        le.mark_stencils(ctx, m, "IB_4", "cell", c.geom, c.Xd, q_depth=5)
    assert e.value.code == 4


# --------------------------------------------------------------------------
# a context of a test's own (part f) and its markers
# --------------------------------------------------------------------------
def test_context_outlives_its_markers(le):
    """ibtk_le_markers_destroy reads its context, so a Context closed (or finalised by the
    cycle collector, as after a failed test that made its own) before its Markers stays
    open until the last of them is closed."""
    cx = le.Context(0)
    X = torch.rand((50, 3), dtype=torch.float64, device=DEV)
    geom = le.Geometry.periodic_unit([16, 16, 16], 3)
    m1 = le.Markers(cx).bin(geom, "IB_4", X)
    m2 = le.Markers(cx).bin(geom, "IB_4", X)
    cx.close()
    assert cx.h is not None, "the context must stay open while it has markers"
    assert m1.count() == 50
    m1.close()
    assert cx.h is not None
    m2.close()
    assert cx.h is None and m1.h is None and m2.h is None
    m2.close()
    cx.close()

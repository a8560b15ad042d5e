"""GPU: physical-boundary ghost fill and adjoint fold for side data
(ibtk_le_phys_bdry_side) against the oracle, bitwise.

CartSideRobinPhysBdryOp::setPhysicalBoundaryConditions (CartSideRobinPhysBdryOp.cpp:
358-422) and accumulateFromPhysicalBoundaryData (:429-493).  The device runs one
launch per boundary box in the reference's order and gives every target point its
contributions in the Fortran's loop order, so it must equal the serial oracle bit
for bit, for Dirichlet and Robin faces, inhomogeneous data, every face pattern.

The second half of the file walks tests/bdry_cases.py (all 16 / 64 face patterns,
patches narrower than their ghost width, g = 16, b at the Dirichlet threshold, NaN
ghosts) against the oracle and, where oracle/_ref/libbdref_O0.so is present, against
the reference's compiled Fortran directly.
"""
import zlib

import numpy as np
import pytest

import bdry_cases as bc
from oracle import oracle as ora

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


CASES = [
    ([0, 0], [6, 5], 2),
    ([0, 0], [63, 63], 3),
    ([2, -1], [9, 6], 1),
    ([0, 0, 0], [5, 4, 6], 2),
    ([1, 0, -2], [6, 6, 3], 3),
    ([0, 0, 0], [47, 39, 31], 4),
]
PATTERNS = {
    "all": [1, 1, 1, 1, 1, 1],
    "walls_y": [0, 0, 1, 1, 0, 0],
    "mixed": [1, 0, 0, 1, 1, 1],
    "one": [0, 0, 0, 0, 0, 1],
}


def _coefs(rng, nd, kind):
    A = rng.uniform(0.5, 2.0, (nd, 2 * nd))
    B = rng.uniform(0.5, 2.0, (nd, 2 * nd))
    G = rng.uniform(-1.0, 1.0, (nd, 2 * nd))
    if kind == "dirichlet":
        B[:] = 0.0
    elif kind == "mixed":
        B[:, ::2] = 0.0  # lower faces Dirichlet, upper faces Robin
    return A, B, G


@pytest.mark.parametrize("lo,hi,g", CASES)
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("kind", ["robin", "dirichlet", "mixed"])
@pytest.mark.parametrize("adjoint", [True, False])
def test_phys_bdry_bitwise(le, ctx, lo, hi, g, pattern, kind, adjoint):
    nd = len(lo)
    rng = np.random.default_rng(zlib.crc32(repr((lo, hi, g, pattern, kind, adjoint)).encode()))
    phys = PATTERNS[pattern][:2 * nd]
    dx = [0.1, 0.13, 0.07][:nd]
    A, B, G = _coefs(rng, nd, kind)
    host = [rng.standard_normal(ora.side_ghost_shape(lo, hi, g, a)) for a in range(nd)]
    dev = [torch.from_numpy(h.copy()).cuda() for h in host]
    geom = le.Geometry(lo, hi, g, dx, [0.0] * nd)
    le.phys_bdry_side(ctx, geom, dev, phys, A, B, G, adjoint=adjoint)
    ctx.synchronize()
    ora.phys_bdry_side(lo, hi, g, dx, host, phys, A, B, G, adjoint=adjoint)
    for a in range(nd):
        got = dev[a].cpu().numpy()
        bad = np.argwhere(got.view(np.int64) != host[a].view(np.int64))
        assert bad.size == 0, f"comp {a}: {len(bad)} points differ, first {bad[:3].tolist()}"


def test_phys_bdry_rejects_bad_shapes(le, ctx):
    geom = le.Geometry([0, 0, 0], [7, 7, 7], 2, [0.1] * 3, [0.0] * 3)
    u = [torch.zeros(10, dtype=torch.float64, device="cuda") for _ in range(3)]
    with pytest.raises(ValueError):
        le.phys_bdry_side(ctx, geom, u, [1] * 6, 1.0, 1.0, 0.0, adjoint=True)


def test_phys_bdry_nonuniform_ghosts_error(le, ctx):
    geom = le.Geometry([0, 0, 0], [7, 7, 7], [2, 2, 3], [0.1] * 3, [0.0] * 3)
    u = [torch.zeros(geom.array_shape("side", a), dtype=torch.float64, device="cuda") for a in range(3)]
    with pytest.raises(Exception):
        le.phys_bdry_side(ctx, geom, u, [1] * 6, 1.0, 1.0, 0.0, adjoint=True)


@pytest.mark.parametrize("kernel", ["IB_4", "IB_6"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_wall_bounded_spread_and_interp(le, ctx, kernel, ndim):
    """LDataManager::spread in a box with walls (LDataManager.cpp:625-660): spread
    the interior markers over the ghost box, then fold the physical-boundary ghosts
    back (accumulateFromPhysicalBoundaryData); and the interp side: fill the ghosts
    (setPhysicalBoundaryConditions), then interpolate.  Against the oracle running
    the same two steps: interp bitwise, spread within the stated 1e-12."""
    g = ora.min_ghost_width(kernel)
    N = [24, 20, 16][:ndim]
    lo, hi = [0] * ndim, [n - 1 for n in N]
    dx = [1.0 / N[0]] * ndim
    geom = le.Geometry(lo, hi, g, dx, [0.0] * ndim)
    rng = np.random.default_rng(ndim * 10 + g)
    M = 3000
    # markers everywhere in the box, many within a stencil of the walls
    X = rng.uniform(0.0, 1.0, (M, ndim)) * np.array([N[d] * dx[d] for d in range(ndim)])
    X[: M // 3, 0] = rng.uniform(0.0, 2.0 * dx[0], M // 3)
    F = rng.uniform(-1, 1, (M, ndim))
    phys = [1] * (2 * ndim)
    A = np.ones((ndim, 2 * ndim))
    B = np.zeros((ndim, 2 * ndim))
    B[:, 1::2] = 0.5  # lower faces no-slip (Dirichlet), upper faces Robin
    G = np.zeros((ndim, 2 * ndim))
    dev = "cuda:0"
    idx = np.arange(M, dtype=np.int32)
    xs = np.zeros((M, ndim))
    Xd, Fd = torch.from_numpy(X).to(dev), torch.from_numpy(F).to(dev)
    m = le.Markers(ctx).bin(geom, kernel, Xd, torch.from_numpy(idx).to(dev), torch.from_numpy(xs).to(dev))
    # spread + fold
    f = geom.alloc("side")
    le.spread(ctx, m, kernel, "side", geom, f, Fd, Xd)
    le.phys_bdry_side(ctx, geom, f, phys, A, B, G, adjoint=True)
    # fill + interp
    u_host = [rng.uniform(-1, 1, ora.side_ghost_shape(lo, hi, g, a)) for a in range(ndim)]
    u = [torch.from_numpy(h.copy()).to(dev) for h in u_host]
    le.phys_bdry_side(ctx, geom, u, phys, A, B, G, adjoint=False)
    Q = torch.zeros((M, ndim), dtype=torch.float64, device=dev)
    le.interp(ctx, m, kernel, "side", geom, u, Q, Xd)
    ctx.synchronize()
    order = m.order().cpu().numpy()
    fo = [np.zeros(ora.side_ghost_shape(lo, hi, g, a)) for a in range(ndim)]
    ora.side_spread(kernel, dx, [0.0] * ndim, lo, hi, [g] * ndim, fo, idx[order], xs[order], X, F)
    ora.phys_bdry_side(lo, hi, g, dx, fo, phys, A, B, G, adjoint=True)
    for a in range(ndim):
        got = f[a].cpu().numpy()
        assert np.abs(got - fo[a]).max() <= 1e-12 * np.abs(fo[a]).max()
    ora.phys_bdry_side(lo, hi, g, dx, u_host, phys, A, B, G, adjoint=False)
    for a in range(ndim):
        assert np.array_equal(u[a].cpu().numpy(), u_host[a])
    Qo = np.zeros((M, ndim))
    ora.side_interp(kernel, dx, [0.0] * ndim, lo, hi, [g] * ndim, u_host, idx, xs, X, Qo)
    Qg = Q.cpu().numpy()
    assert np.abs(Qg - Qo).max() <= 1e-13 * np.abs(Qo).max()
    if ndim == 3:  # the 3-D sweep interp sums in the Fortran order
        assert np.array_equal(Qg, Qo)


# --------------------------------------------------------------------------
# the shared case list (tests/bdry_cases.py): every face pattern, narrow patches, the
# ghost-width cap, the Dirichlet threshold, NaN ghosts -- against the oracle, which
# tests/test_bdry_ref_pin.py holds to the reference's compiled Fortran, and against that
# library itself
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bdref():
    from oracle import ref as _ref
    if not _ref.bdry_lib_path("O0").is_file():
        pytest.skip("oracle/_ref/libbdref_O0.so absent (built where the reference tree and flang are)")
    return _ref


def _geom(le, patch, pitched=False):
    nd = len(patch["lo"])
    geom = le.Geometry(patch["lo"], patch["hi"], patch["g"], bc.dx_of(patch), [0.0] * nd)
    return geom.aligned(16) if pitched else geom


def _upload(geom, us):
    """The arrays of one case on the device, in the geometry's layout (padding, if any, 7)."""
    dev = geom.alloc("side", fill=7.0)
    for d, u in zip(dev, us):
        d.copy_(torch.from_numpy(u))
    return dev


def _device(le, ctx, geom, patch, case, dev):
    """One call on `dev`, in place."""
    _, _, phys, kind, adjoint = case
    A, B, G = bc.coefs(patch, kind)
    le.phys_bdry_side(ctx, geom, dev, phys, A, B, G, adjoint=adjoint)
    return dev


def _host(fn, patch, case, us):
    _, _, phys, kind, adjoint = case
    A, B, G = bc.coefs(patch, kind)
    out = [u.copy() for u in us]
    fn(patch["lo"], patch["hi"], patch["g"], bc.dx_of(patch), out, phys, A, B, G, adjoint)
    return out


def _sweep(le, ctx, patch, fn, what, pitched):
    """Every case of the patch: the packed device result against `fn`'s, bit for bit (the
    NaN family: NaN where `fn` has NaN, the same bits elsewhere), and -- `pitched` -- the
    pitched layout against the packed one."""
    geom = _geom(le, patch)
    host = {f: bc.inputs(patch, f) for f in ("random", "nan_ghost")}
    base = {f: _upload(geom, us) for f, us in host.items()}
    if pitched:
        pgeom = _geom(le, patch, pitched=True)
        assert pgeom.pitched
    n = 0
    for case in bc.cases(patch):
        fam = case[0]
        dev = _device(le, ctx, geom, patch, case, [b.clone() for b in base[fam]])
        want = _host(fn, patch, case, host[fam])
        diff = bc.same_bits_or_nan if fam == "nan_ghost" else bc.same_bits
        for a in range(len(dev)):
            bad = diff(dev[a].cpu().numpy(), want[a])
            assert bad.size == 0, (f"{bc.label(patch, case)} comp {a}: the device differs from {what} at "
                                   f"{len(bad)} points, first {bad[:3].tolist()}")
        if pitched:
            pdev = _device(le, ctx, pgeom, patch, case, _upload(pgeom, host[fam]))
            for a in range(len(dev)):
                x, y = dev[a], pdev[a]
                if fam == "nan_ghost":  # NaN != NaN: where, then the rest
                    assert torch.equal(x.isnan(), y.isnan()), f"{bc.label(patch, case)} comp {a}: pitched NaN set"
                    x, y = x.nan_to_num(0.0), y.nan_to_num(0.0)
                assert torch.equal(x, y), f"{bc.label(patch, case)} comp {a}: the pitched layout differs from the packed"
                flat = y.as_strided((y.untyped_storage().nbytes() // 8,), (1,), 0)
                pad = torch.ones_like(flat, dtype=torch.bool)
                pad.as_strided(y.shape, y.stride()).fill_(False)
                assert bool((flat[pad] == 7.0).all()), f"{bc.label(patch, case)} comp {a}: padding written"
        n += 1
    assert n == len(bc.cases(patch))


@pytest.mark.parametrize("patch", bc.PATCHES, ids=bc.PATCH_IDS)
def test_case_list_against_oracle(le, ctx, patch):
    """le.phys_bdry_side == le_bdry_oracle.c over tests/bdry_cases.py, packed; on the 3-D
    patches that run every face pattern also pitched == packed (a pitch needs a 3-D patch)."""
    _sweep(le, ctx, patch, ora.phys_bdry_side, "the oracle", pitched=patch["every_pattern"] and len(patch["lo"]) == 3)


@pytest.mark.parametrize("patch", bc.PATCHES, ids=bc.PATCH_IDS)
def test_case_list_against_reference(le, ctx, bdref, patch):
    """The same against oracle/_ref/libbdref_O0.so, the reference's own Fortran, with no
    oracle between."""
    _sweep(le, ctx, patch, bdref.phys_bdry_side, "the -O0 reference library", pitched=False)


@pytest.mark.parametrize("patch", bc.PATCHES, ids=bc.PATCH_IDS)
def test_fill_twice(le, ctx, patch):
    """A second fill changes no bit: the reference's fill reads only the patch's own points
    and ghost points it wrote earlier in the same call (test_bdry_ref_pin.py asserts that of
    the reference).  That needs max(g, 2) cells in every dimension; on a narrow patch a
    mirror point lies in the opposite ghost region and the second fill differs in the
    reference too, so there the device's second fill is held to the oracle's second fill."""
    geom = _geom(le, patch)
    us = bc.inputs(patch, "random")
    base = _upload(geom, us)
    for case in bc.cases(patch):
        if case[0] != "random" or case[4]:
            continue
        once = _device(le, ctx, geom, patch, case, [b.clone() for b in base])
        twice = _device(le, ctx, geom, patch, case, [b.clone() for b in once])
        if bc.is_narrow(patch):
            want = _host(ora.phys_bdry_side, patch, case, _host(ora.phys_bdry_side, patch, case, us))
            for a in range(len(us)):
                bad = bc.same_bits(twice[a].cpu().numpy(), want[a])
                assert bad.size == 0, f"{bc.label(patch, case)} comp {a}: second fill differs from the oracle's"
        else:
            for a in range(len(us)):
                assert torch.equal(once[a], twice[a]), f"{bc.label(patch, case)} comp {a}: a second fill changed it"


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("adjoint", [False, True])
def test_ghost_width_cap_and_zero(le, ctx, ndim, adjoint):
    """g = 17 is refused with IBTK_LE_ERR_GHOST_WIDTH before anything is written (16 is the
    last width taken: the 3x2x2 patch of the case list); g = 0 returns OK and writes nothing."""
    from ibamr_amd._lib import IBTKLEError, STATUS
    lo, hi = [0, -1, 2][:ndim], [2, 0, 3][:ndim]
    A, B, G = bc.coefs(dict(lo=lo, id=f"cap{ndim}"), "mixed")
    rng = np.random.default_rng(ndim)
    for g in (bc.MAX_GHOST + 1, 0):
        geom = le.Geometry(lo, hi, g, bc.DX[:ndim], [0.0] * ndim)
        us = [rng.standard_normal(bc.side_shape(lo, hi, g, a)) for a in range(ndim)]
        dev = [torch.from_numpy(u).cuda() for u in us]
        if g:
            with pytest.raises(IBTKLEError) as e:
                le.phys_bdry_side(ctx, geom, dev, [1] * (2 * ndim), A, B, G, adjoint=adjoint)
            assert STATUS[e.value.code] == "GHOST_WIDTH"
        else:
            le.phys_bdry_side(ctx, geom, dev, [1] * (2 * ndim), A, B, G, adjoint=adjoint)
        ctx.synchronize()
        for a in range(ndim):
            assert bc.same_bits(dev[a].cpu().numpy(), us[a]).size == 0, f"g = {g}: comp {a} was written"

"""GPU kernels against the reference's own compiled Fortran, with no oracle between.

The other GPU tests compare the HIP path with ``oracle/le_oracle.c``, and
``tests/test_ref_pin.py`` compares that file with the reference on the CPU.  Here the
chain is closed directly: the Fortran-symbol shims of ``libibtk_le.so`` and the device
path (``le.interp`` / ``le.spread``) against ``oracle/_ref/libleref_O0.so``, the library
``oracle/build_ref.py`` compiles from the reference's ``.f.m4`` sources.  Only
``oracle/_ref/`` is read, never the reference tree.

Interpolation is asserted bit for bit; spreading within 1e-12 relative of the reference
run in the caller's list order, the Fortran's own summation order.  Kept from the
reference (see tests/test_ref_pin.py): ``DISCONTINUOUS_LINEAR`` 3-D spread, and
``PIECEWISE_CONSTANT`` markers outside the ghost box.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_boundary import KMAP, call_shim  # noqa: E402
from test_gpu_parity import SPREAD_TOL, make_case, rel_err  # noqa: E402
from test_ref_pin import cell_strictly_inside  # noqa: E402


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as _ref
    if not _ref.available():
        pytest.skip("oracle/_ref/libleref_{O0,O2}.so absent (built where the reference tree and flang are)")
    return _ref


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
# same call, two libraries
# --------------------------------------------------------------------------
def shim_case(oracle, kernel, ndim, geometry):
    """The 10-cell box, depth 2, 120 markers and repeating list of
    test_fortran_shims_match_oracle; "ties": a dyadic geometry with every coordinate
    x_lower + j*dx/2 exactly, j from below the ghost layer to above it."""
    rng = np.random.default_rng(17)
    g = oracle.min_ghost_width(kernel)
    ilo = [2, -3, 1][:ndim]
    ihi = [ilo[d] + 9 for d in range(ndim)]
    M = 120
    if geometry == "box":
        dx = [0.1] * ndim
        xlo = [0.2, -0.3, 0.0][:ndim]
        X = np.array(xlo) + rng.uniform(-0.05, 1.05, (M, ndim))
    else:
        dx = [0.125, 0.25, 0.0625][:ndim]
        xlo = [-0.75, -1.5, -0.375][:ndim]
        j = np.arange(-2 * (g + 2), 2 * (10 + g + 2) + 1)
        J = np.stack([rng.permutation(np.concatenate([j, rng.choice(j, M - j.size)])) for _ in range(ndim)], axis=1)
        X = np.array(xlo) + J * (np.array(dx) / 2)
        assert np.array_equal((X - np.array(xlo)) / np.array(dx) * 2, J)
    idx = rng.integers(0, M, 150).astype(np.int32)  # duplicates on purpose
    geo = dict(ndim=ndim, ilo=ilo, ihi=ihi, g=[g] * ndim, dx=dx, xlo=xlo, n=[10] * ndim)
    if kernel == "PIECEWISE_CONSTANT":  # the reference indexes u unchecked: inside the ghost box only
        keep = cell_strictly_inside(geo, idx, np.zeros((idx.size, ndim)), X)
        idx = idx[keep]
        assert idx.size >= 30 and np.unique(idx).size < idx.size
        assert cell_strictly_inside(geo, idx, np.zeros((idx.size, ndim)), X).all()
    xs = np.zeros((idx.size, ndim))
    return geo, np.ascontiguousarray(X), idx, xs, rng


@pytest.mark.parametrize("geometry", ["box", "ties"])
@pytest.mark.parametrize("kernel", list(KMAP))
@pytest.mark.parametrize("ndim", [2, 3])
def test_fortran_shims_match_reference(lib, ref, oracle, kernel, ndim, geometry):
    """One Fortran argument tuple, handed to libibtk_le.so's shim and to the reference's
    symbol of the same name (two CDLL handles)."""
    geo, X, idx, xs, rng = shim_case(oracle, kernel, ndim, geometry)
    rlib = ref.lib("O0")
    assert rlib is not lib and rlib._handle != lib._handle
    ilo, ihi, g, dx, xlo = geo["ilo"], geo["ihi"], geo["g"], geo["dx"], geo["xlo"]
    depth, M = 2, X.shape[0]
    u = rng.uniform(-1, 1, oracle.ghost_shape(ilo, ihi, g, depth))
    V = np.full((M, depth), 7.0)
    call_shim(lib, "interp", KMAP[kernel], ndim, dx, xlo, ilo, ihi, g, u, idx, xs, X, V, depth, axis=1)
    Vr = np.full((M, depth), 7.0)
    ref.interp(kernel, dx, xlo, ilo, ihi, g, u, idx, xs, X, Vr, depth=depth, axis=1)
    assert np.array_equal(V, Vr)
    if (kernel, ndim) == ("DISCONTINUOUS_LINEAR", 3):
        return  # the reference's spread reads an unset index: left to test_fortran_shims_match_oracle
    F = rng.uniform(-1, 1, (M, depth))
    ug = u.copy()
    call_shim(lib, "spread", KMAP[kernel], ndim, dx, xlo, ilo, ihi, g, ug, idx, xs, X, F, depth, axis=1)
    ur = u.copy()
    ref.spread(kernel, dx, xlo, ilo, ihi, g, ur, idx, xs, X, F, depth=depth, axis=1)
    assert not np.array_equal(ur, u)
    err = rel_err(ug, ur)
    print(f"{kernel} {ndim}d {geometry}: shim spread rel err {err:.2e}")
    assert err <= 1e-12


# --------------------------------------------------------------------------
# device path, headline centering
# --------------------------------------------------------------------------
DEVICE_CASES = [("IB_4", 3), ("IB_6", 3), ("PIECEWISE_LINEAR", 3), ("IB_4", 2), ("IB_6", 2)]


@pytest.mark.parametrize("kernel,ndim", DEVICE_CASES, ids=lambda v: str(v))
def test_device_side_against_reference(le, ctx, ref, oracle, kernel, ndim):
    """le.interp / le.spread on side data (3-D, and the 2-D twins of le_hot.hip) against
    the side wrappers run over the reference Fortran: interp bit for bit at the listed
    markers, spread within 1e-12 in the kernel's own order and in the caller's."""
    geom, X, idx, xs, depth = make_case(kernel, ndim, "side", seed=5, M=2000)
    be = ref.backend("O0")
    rng = np.random.default_rng(3)
    dev = "cuda:0"
    q = geom.alloc("side")
    for a in q:
        a.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(a.shape))))
    u0 = [a.cpu().numpy().copy() for a in q]
    F = rng.uniform(-1, 1, (X.shape[0], ndim))
    Xd, Fd = torch.from_numpy(X).to(dev), torch.from_numpy(F).to(dev)
    idd, xsd = torch.from_numpy(idx).to(dev), torch.from_numpy(xs).to(dev)
    m = le.Markers(ctx).bin(geom, kernel, Xd, idd, xsd)
    Q = torch.zeros((X.shape[0], ndim), dtype=torch.float64, device=dev)
    le.interp(ctx, m, kernel, "side", geom, q, Q, Xd)
    le.spread(ctx, m, kernel, "side", geom, q, Fd, Xd)
    ctx.synchronize()
    order = m.order().cpu().numpy()
    head = (kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw)
    Qr = np.zeros((X.shape[0], ndim))
    oracle.side_interp(*head, u0, idx, xs, X, Qr, backend=be)
    assert np.abs(Qr[idx]).max() > 0.1
    assert np.array_equal(Q.cpu().numpy()[idx], Qr[idx])
    uo = [a.copy() for a in u0]
    oracle.side_spread(*head, uo, idx[order], xs[order], X, F, backend=be)
    uc = [a.copy() for a in u0]  # the caller's list order: the Fortran's own summation order
    oracle.side_spread(*head, uc, idx, xs, X, F, backend=be)
    for a in range(ndim):
        ga = q[a].cpu().numpy()
        eo, ec = rel_err(ga, uo[a]), rel_err(ga, uc[a])
        print(f"{kernel} {ndim}d comp {a}: spread rel err {eo:.2e} (kernel order) {ec:.2e} (caller order)")
        assert eo <= SPREAD_TOL, f"comp {a} rel err {eo:.3e}"
        assert ec <= SPREAD_TOL, f"comp {a} rel err {ec:.3e} against the caller's order"


def test_spread_at_rounding_ties_against_reference(le, ctx, ref, oracle):
    """test_spread_at_rounding_ties' inputs (markers where (X - xlo) * (1/dx) and
    (X - xlo) / dx round to different NINT anchors), IB_4, against the reference."""
    from ibamr_amd.le import Geometry
    kernel = "IB_4"
    dx, xlo, N = 0.1, -0.3, 14
    geom = Geometry([0, 0, 0], [N - 1] * 3, oracle.min_ghost_width(kernel), [dx] * 3, [xlo] * 3)
    ties = []
    for k in range(2, N - 2):
        base = xlo + (k + 0.5) * dx
        for j in range(-40, 41):
            X = base + j * np.spacing(base)
            if np.floor((X - xlo) * (1.0 / dx) + 0.5) != np.floor((X - xlo) / dx + 0.5):
                ties.append(X)
    ties = np.array(ties)
    assert ties.size >= 4
    rng = np.random.default_rng(2)
    M = 600
    Xn = rng.choice(ties, size=(M, 3))
    Fn = rng.standard_normal((M, 3))
    X, F = torch.from_numpy(Xn).cuda(), torch.from_numpy(Fn).cuda()
    m = le.Markers(ctx).bin(geom, kernel, X)
    q = geom.alloc("side")
    le.spread(ctx, m, kernel, "side", geom, q, F, X)
    ctx.synchronize()
    order = m.order().cpu().numpy()
    ur = [np.zeros(tuple(a.shape)) for a in q]
    oracle.side_spread(kernel, geom.dx, geom.x_lower, geom.ilower, geom.iupper, geom.gcw, ur,
                       np.arange(M, dtype=np.int32)[order], np.zeros((M, 3)), Xn, Fn, backend=ref.backend("O0"))
    for a in range(3):
        assert rel_err(q[a].cpu().numpy(), ur[a]) <= SPREAD_TOL, f"spread comp {a}"

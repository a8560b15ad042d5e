"""CPU tests of the IMP stages: the numpy restatement (tests/imp_ref.py) against 50-digit
known answers (tests/golden/imp_kat.npz, made by tests/golden/make_imp_kat.py), the
identities the kernel and the two Eulerian operators satisfy, the preconditions of the
cases the GPU tests run, the exports, and the argument checks that need no device.  No GPU.
"""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import imp_cases as ic
import imp_ref as ir

ROOT = Path(__file__).resolve().parents[1]
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def kat():
    return np.load(ROOT / "tests" / "golden" / "imp_kat.npz")


def rel(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


def kat_geo(kat, tag):
    return ir.Geo(kat[f"e{tag}_ilower"], kat[f"e{tag}_n"], kat[f"e{tag}_dx"], kat[f"e{tag}_x_lower"], 4)


# ---- imp_ref against the known answers --------------------------------------------------
# The bounds are fixed from the arithmetic, not from the recorded ref_err: a weight passes
# through about 30 roundings of operands of order 1 (the discriminant's terms reach 9/4 and
# cancel to a phi of order 0.3), so 64 * 2^-52 of the largest value covers the kernel; the
# sums add 6^NDIM products of such weights.  The pointwise stages are a dozen operations on
# well-conditioned 3x3 matrices (|dt G| <= 0.2, det F in [0.5, 2]): 32 * 2^-52.

def test_kernel_and_its_derivative_against_50_digits(kat):
    _, phi, dphi = ir.kernel(kat["k_x"], float(kat["k_xlo"]), kat["k_dx"], int(kat["k_ilo"]))
    e_phi, e_dphi = rel(phi, kat["k_phi"]), rel(dphi, kat["k_dphi"])
    print(f"phi {e_phi:.3e} (recorded {float(kat['ref_err_phi']):.3e}), dphi {e_dphi:.3e}")
    # k_dphi is the derivative of phi itself at 50 digits, not the dphi formulas
    assert e_phi <= 64 * ULP and e_dphi <= 64 * ULP
    assert e_phi == float(kat["ref_err_phi"]) and e_dphi == float(kat["ref_err_dphi"])


@pytest.mark.parametrize("tag", ["3", "2"])
def test_interp_and_spread_against_50_digits(kat, tag):
    geo = kat_geo(kat, tag)
    nd = geo.ndim
    u = [kat[f"e{tag}_u{c}"] for c in range(nd)]
    U, G, clipped = ir.interp(geo, u, kat[f"e{tag}_X"])
    assert clipped.any()
    eU, eG = rel(U, kat[f"e{tag}_U"]), rel(G, kat[f"e{tag}_GradU"])
    print(f"U {eU:.3e}  GradU {eG:.3e}")
    assert eU <= 64 * ULP and eG <= 64 * ULP
    for clip in ("patch", "ghost"):
        f = ir.spread(geo, geo.alloc(), kat[f"e{tag}_tau"], kat[f"e{tag}_wgt"], kat[f"e{tag}_X"], clip=clip)
        ef = max(rel(f[c], kat[f"e{tag}_f_{clip}{c}"]) for c in range(nd))
        print(f"f ({clip}) {ef:.3e}")
        assert ef <= 64 * ULP
        for c in range(nd):  # the same points are touched, and no others
            assert np.array_equal(f[c] != 0.0, kat[f"e{tag}_f_{clip}{c}"] != 0.0)


@pytest.mark.parametrize("nd", [3, 2])
def test_update_and_stress_against_50_digits(kat, nd):
    F, G0, G1, dt = kat[f"p{nd}_F"], kat[f"p{nd}_G0"], kat[f"p{nd}_G1"], float(kat["p_dt"])
    assert np.abs(dt * G0).max() <= 0.2 and np.abs(dt * G1).max() <= 0.2
    d = np.linalg.det(F.reshape(-1, nd, nd))
    assert d.min() >= 0.5 and d.max() <= 2.0
    for scheme in ("euler", "midpoint", "trapezoidal"):
        new, half = ir.deformation_update(scheme, dt, F, G0, G1)
        e = rel(new, kat[f"p{nd}_{scheme}_new"])
        print(f"{scheme} F_new {e:.3e}")
        assert e <= 32 * ULP
        if scheme == "euler":
            assert rel(half, kat[f"p{nd}_euler_half"]) <= 32 * ULP
        else:
            assert half is None
    for k, (c1, p0, beta) in enumerate(kat["p_law"]):
        e = rel(ir.kirchhoff_stress(F, c1, p0, beta), kat[f"p{nd}_tau{k}"])
        print(f"tau law {k} {e:.3e}")
        assert e <= 32 * ULP


def test_update_and_stress_exact_cases():
    for nd in (2, 3):
        w = nd * nd
        F = np.random.default_rng(3).uniform(0.5, 1.5, (7, w))
        new, half = ir.deformation_update("euler", 0.1, F, np.zeros((7, w)))
        assert np.array_equal(ir.bits(new), ir.bits(F)) and np.array_equal(ir.bits(half), ir.bits(F))
        eye = np.tile(np.eye(nd).reshape(1, w), (5, 1))
        assert np.array_equal(ir.bits(ir.kirchhoff_stress(eye, 0.05)), ir.bits(2.0 * 0.05 * eye))


# ---- the kernel's identities --------------------------------------------------------------

def offsets():
    rng = np.random.default_rng(64)
    x = rng.uniform(-6.0, 30.0, 20000)
    ties = np.arange(-6, 30) + 0.5
    return np.concatenate([x, ties, np.nextafter(ties, 99.0), np.nextafter(ties, -99.0)])


def test_kernel_identities():
    """Over 2 10^4 random offsets and the exact ties (frame x_lower = 0, dx = 1, ilower = 0):
    sum phi = 1, sum dphi = 0, sum x_j phi_j = X, -sum x_j dphi_j = 1, x_j = j + 1/2.
    A weight is within 8 * 2^-52 of exact (the known answers), six are summed, and the
    moments multiply each by |x_j| <= 34: bounds 8 * 2^-52 for the plain sums and
    8 * 2^-52 * sum |x_j| for the moments."""
    X = offsets()
    lower, phi, dphi = ir.kernel(X, 0.0, 1.0, 0)
    assert np.array_equal(lower, ir.nint(X) - 3)
    xj = (lower[:, None] + np.arange(6)[None, :]) + 0.5
    s0 = np.abs(phi.sum(axis=1) - 1.0).max()
    s1 = np.abs(dphi.sum(axis=1)).max()
    m0 = np.abs((xj * phi).sum(axis=1) - X)
    m1 = np.abs(-(xj * dphi).sum(axis=1) - 1.0)
    bound_m = 8 * ULP * np.abs(xj).sum(axis=1)
    print(f"sum phi - 1: {s0:.2e}; sum dphi: {s1:.2e}; first moment: {m0.max():.2e}; derivative moment: {m1.max():.2e}")
    assert s0 <= 8 * ULP and s1 <= 8 * ULP
    assert (m0 <= bound_m).all() and (m1 <= bound_m).all()
    # the stencil holds the point: phi vanishes beyond three cells
    assert (np.abs(X[:, None] - xj) <= 3.5).all()


def test_round_is_half_away_from_zero():
    assert ir.nint(np.array([-0.5, 0.5, -1.5, 2.5, -0.49999999999999994])).tolist() == [-1, 1, -2, 3, 0]


# ---- identities of the two operators --------------------------------------------------------

def linear_case(nd):
    geo = ir.Geo((-3, 5, 2)[:nd], (19, 10, 21)[:nd], ic.DX[:nd], (0.3, -0.2, 0.1)[:nd], 4)
    rng = np.random.default_rng(5 + nd)
    xl, dx, n = np.array(geo.x_lower), np.array(geo.dx), np.array(geo.n)
    X = rng.uniform(xl, xl + n * dx, (200, nd))  # interior: no stencil is clipped with ghost width 4
    return geo, X, rng


@pytest.mark.parametrize("nd", [3, 2])
def test_linear_field_is_reproduced(nd):
    """u_c = a_c + b_c . x gives U = u(X) and GradU = b where no stencil is clipped.  Each of
    the 6^NDIM terms is u w with |u| <= umax and sum |w| <= 3 per dim at most, so the sums are
    within 6^NDIM * 2^-52 * umax * 27 (U) and that over dx_k (GradU) of exact."""
    geo, X, rng = linear_case(nd)
    a, b = rng.standard_normal(nd), rng.standard_normal((nd, nd))
    u = []
    for c in range(nd):
        grids = np.meshgrid(*[geo.coords(c, d) for d in reversed(range(nd))], indexing="ij")
        u.append(a[c] + sum(b[c, d] * grids[nd - 1 - d] for d in range(nd)))
    U, G, clipped = ir.interp(geo, u, X)
    assert not clipped.any()
    umax = max(np.abs(v).max() for v in u)
    tol = 6 ** nd * ULP * umax * 27
    eU = np.abs(U - (a[None, :] + X @ b.T)).max()
    print(f"U error {eU:.2e} (bound {tol:.2e})")
    assert eU <= tol
    for c in range(nd):
        for k in range(nd):
            assert np.abs(G[:, nd * c + k] - b[c, k]).max() <= tol / geo.dx[k]


@pytest.mark.parametrize("nd", [3, 2])
def test_power_identity_and_zero_net_force(nd):
    """sum_c sum_i f_c(i) u_c(i) dV = -sum_m wgt_m sum_ck tau_ck GradU_ck with clip="ghost":
    both sides are the same products summed in two orders, each value through at most
    6^NDIM + 8 roundings, so they agree to 2 (6^NDIM + 8) 2^-53 T, T = sum_i S_i |u(i)| dV.
    And sum_i f_c(i) = 0 where no stencil is clipped (sum_j dphi_j = 0 to 8 * 2^-52 per weight
    set): |sum f_c| <= 64 * 2^-52 * sum_i S_i."""
    geo, X, rng = linear_case(nd)
    n = X.shape[0]
    u = [rng.standard_normal(geo.shape(c)) for c in range(nd)]
    tau, wgt = rng.standard_normal((n, nd * nd)), rng.uniform(0.5, 1.5, n)
    dV = float(np.prod(geo.dx))
    f, cnt, S = ir.spread(geo, geo.alloc(), tau, wgt, X, clip="ghost", stats=True)
    _, G, clipped = ir.interp(geo, u, X)
    assert not clipped.any()
    lhs = math.fsum(float(v) for c in range(nd) for v in (f[c] * u[c]).ravel()) * dV
    rhs = -math.fsum(float(v) for v in (wgt[:, None] * tau * G).ravel())
    T = math.fsum(float(v) for c in range(nd) for v in (S[c] * np.abs(u[c])).ravel()) * dV
    print(f"power: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {2 * (6 ** nd + 8) * 2.0 ** -53 * T:.3e}")
    assert abs(lhs) > 0.0
    assert abs(lhs - rhs) <= 2 * (6 ** nd + 8) * 2.0 ** -53 * T
    for c in range(nd):
        tot = math.fsum(float(v) for v in f[c].ravel())
        assert abs(tot) <= 64 * ULP * float(S[c].sum())
    # the reference's clip drops what falls outside the patch's side boxes and nothing else
    fp = ir.spread(geo, geo.alloc(), tau, wgt, X, clip="patch")
    for c in range(nd):
        lo, hi = geo.patch_side_box(c)
        glo, _ = geo.ghost_box(c)
        box = tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in reversed(range(nd)))
        mask = np.ones(fp[c].shape, bool)
        mask[box] = False
        assert not fp[c][mask].any() and np.array_equal(ir.bits(fp[c][box]), ir.bits(f[c][box]))


# ---- the GPU tests' cases -------------------------------------------------------------------

@pytest.mark.parametrize("name", ic.CASES)
def test_case_preconditions(name):
    c = ic.case(name)
    assert 650 <= c["X"].shape[0] <= 800
    ic.check_preconditions(c, ties=name in ("pow2", "2d"))
    # duplicates: the sub-list names ten markers twice, and rows it does not name keep the sentinel
    idx = c["sub_idx"]
    assert len(np.unique(idx)) == len(idx) - 10
    unnamed = np.setdiff1d(np.arange(c["X"].shape[0]), idx)
    assert len(unnamed) > 0 and (c["sub_U"][unnamed] == -7.25).all() and (c["sub_U"][idx] != -7.25).all()


# ---- exports and host-side argument checks ----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ibamr_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ibamr_amd import build
        build.build()
    return _lib.load()


NAMES = ("ibtk_le_imp_interp", "ibtk_le_imp_spread", "ibtk_le_imp_deformation_update", "ibtk_le_imp_stress")


def test_header_declares_and_library_exports_the_imp_calls(lib):
    text = (ROOT / "include" / "ibtk_le.h").read_text()
    from ibamr_amd import _lib
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert re.search(r"int\s+" + name + r"\s*\(\s*ibtk_le_ctx\s+ctx", text), name
        assert any(n == name for n, _, _ in _lib._SIGS) and hasattr(raw, name)
    assert "DEVIATION" in text  # the header says where X + Xshift departs from the reference


def test_imp_module_exports():
    from ibamr_amd import imp
    for name in ("interp_velocity_gradient", "spread_stress", "deformation_update", "kirchhoff_stress"):
        assert callable(getattr(imp, name)) and name in imp.__all__
    text = (ROOT / "ibamr_amd" / "csrc" / "le_imp.h").read_text()
    consts = {k: int(v) for k, v in re.findall(r"\b(IMP_TILE3|IMP_TILE2|IMP_CHUNK|IMP_MIN_GHOST)\s*=\s*(\d+)", text)}
    assert imp.IMP_TILE == (consts["IMP_TILE3"], consts["IMP_TILE2"]) and imp.IMP_CHUNK == consts["IMP_CHUNK"]
    assert imp.MIN_GHOST == consts["IMP_MIN_GHOST"] == 4
    assert imp.CLIP == {"patch": 0, "ghost": 1}
    from ibamr_amd.build import SOURCES
    assert "le_imp.hip" in SOURCES


def test_host_side_argument_errors(lib):
    from ibamr_amd._lib import PatchGeom
    err = lambda: lib.ibtk_le_last_error().decode()  # noqa: E731
    dummy = (ctypes.c_double * 16)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 3)(p, p, p)
    g4 = PatchGeom.make((0, 0, 0), (7, 7, 7), 4, (0.1, 0.1, 0.1), (0.0, 0.0, 0.0))
    g3 = PatchGeom.make((0, 0, 0), (7, 7, 7), 3, (0.1, 0.1, 0.1), (0.0, 0.0, 0.0))
    for call in (lambda g, a: lib.ibtk_le_imp_interp(None, None, g, a, p, p, p),
                 lambda g, a: lib.ibtk_le_imp_spread(None, None, g, a, p, p, p, 0)):
        assert call(ctypes.byref(g3), arr) == 2 and "insufficient ghost cells" in err()  # GHOST_WIDTH
        assert call(None, arr) == 4 and "null geometry" in err()
        bad = PatchGeom.make((0, 0, 0), (7, 7, 7), 4, (0.1, 0.1, 0.1), (0.0, 0.0, 0.0))
        bad.ndim = 4
        assert call(ctypes.byref(bad), arr) == 4 and "ndim" in err()
        assert call(ctypes.byref(g4), None) == 4 and "null array table" in err()
        hole = (ctypes.c_void_p * 3)(p, None, p)
        assert call(ctypes.byref(g4), hole) == 4 and "null side array 1" in err()
        assert call(ctypes.byref(g4), arr) == 4 and "null ctx/markers" in err()
    assert lib.ibtk_le_imp_spread(None, None, ctypes.byref(g4), arr, p, p, p, 2) == 4 and "clip" in err()
    upd = lib.ibtk_le_imp_deformation_update
    assert upd(None, 4, 0, 5, 0.1, p, p, None, p, None) == 4 and "ndim" in err()
    assert upd(None, 3, 3, 5, 0.1, p, p, None, p, None) == 4 and "scheme" in err()
    assert upd(None, 3, 0, -1, 0.1, p, p, None, p, None) == 4 and "negative" in err()
    assert upd(None, 3, 2, 5, 0.1, p, p, None, p, None) == 4 and "TRAPEZOIDAL needs G1" in err()
    assert upd(None, 3, 1, 5, 0.1, p, p, None, p, p) == 4 and "F_half" in err()
    assert upd(None, 3, 0, 5, 0.1, None, p, None, p, None) == 4 and "null array" in err()
    assert upd(None, 3, 0, 5, 0.1, p, p, None, p, p) == 4 and "null context" in err()
    st = lib.ibtk_le_imp_stress
    assert st(None, 1, 5, p, p, 0.05, 0.0, 0.0, None, 0, None) == 4 and "ndim" in err()
    assert st(None, 3, 5, None, p, 0.05, 0.0, 0.0, None, 0, None) == 4 and "null array" in err()
    assert st(None, 3, 5, p, p, 0.05, 0.0, 0.0, p, 2, None) == 4 and "go together" in err()
    assert st(None, 3, 5, p, p, 0.05, 0.0, 0.0, p, 0, p) == 4 and "nsub" in err()
    assert st(None, 3, 5, p, p, 0.05, 0.0, 0.0, None, 0, None) == 4 and "null context" in err()

"""CPU tests of the side-centred curl: the numpy restatement (tests/curl_ref.py) against
the compiled reference's own outputs, the identities the operator satisfies, and the
exports of the C ABI and of ibamr_amd.gib.  No GPU.
"""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import curl_ref as cr

ROOT = Path(__file__).resolve().parents[1]
FIXTURE = ROOT / "tests" / "golden" / "curl_side_ref.npz"
DX = (0.1, 0.037, 0.2113)
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


def fixture_case(z, k):
    u = [z[f"c{k}_u{c}"] for c in range(3)]
    w = [z[f"c{k}_w{c}"] for c in range(3)]
    return (z[f"c{k}_ilower"], z[f"c{k}_iupper"], int(z[f"c{k}_u_gcw"]), int(z[f"c{k}_w_gcw"]), z[f"c{k}_dx"], u, w)


def test_fixture_holds_the_issue_cases(fixture):
    assert int(fixture["ncases"]) == 3
    want = [((-3, 2, 5), (1, 4, 7), 2, 3), ((0, 0, 0), (0, 0, 0), 1, 0), ((4, -7, 1), (20, 3, 9), 4, 4)]
    for k, (lo, hi, ug, wg) in enumerate(want):
        ilo, ihi, g_u, g_w, dx, u, w = fixture_case(fixture, k)
        assert tuple(ilo) == lo and tuple(ihi) == hi and (g_u, g_w) == (ug, wg)
        assert tuple(dx) == DX
        n = cr.box_extent(ilo, ihi)
        for c in range(3):
            assert u[c].shape == cr.side_shape(n, ug, c) and w[c].shape == cr.side_shape(n, wg, c)
            # the routine writes the side box and nothing else: every NaN outside it survived
            mask = np.ones(w[c].shape, bool)
            mask[cr.side_box(n, wg, c)] = False
            assert np.isnan(w[c][mask]).all() and np.isfinite(w[c][~mask]).all()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_restatement_equals_the_reference_bit_for_bit(fixture, k):
    ilo, ihi, ug, wg, dx, u, w_ref = fixture_case(fixture, k)
    w = [np.full_like(a, np.nan) for a in w_ref]
    cr.curl_side_ref(u, ilo, ihi, ug, w, wg, dx)
    for c in range(3):
        assert np.array_equal(cr.bits(w[c]), cr.bits(w_ref[c])), f"case {k} component {c}"


def rotation_field(omega, centre, n, g, h):
    """u = omega x (x - centre) at the side centres of the box 0..n-1 with spacing h."""
    u = []
    for c in range(3):
        ax = []
        for d in range(3):
            i = np.arange(-g, n[d] + g + (1 if d == c else 0), dtype=np.float64)
            ax.append((i + (0.0 if d == c else 0.5)) * h - centre[d])
        Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        r = (X, Y, Z)
        a, b = (c + 1) % 3, (c + 2) % 3
        u.append(omega[a] * r[b] - omega[b] * r[a])
    return u


@pytest.mark.parametrize("omega", [(1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (1.0, -2.0, 4.0)])
def test_exact_rotation(omega):
    """Every operand and partial sum is a small dyadic number: curl u == 2 omega and
    0.5 curl u == omega exactly at every side point, no tolerance."""
    n, g, h = [8, 8, 8], 1, 2.0 ** -4
    u = rotation_field(omega, (0.25, 0.5, 0.125), n, g, h)
    vals = cr.curl_values(u, n, g, (h, h, h))
    for c in range(3):
        assert np.array_equal(cr.bits(vals[c]), cr.bits(np.full(vals[c].shape, 2.0 * omega[c])))
    w = [np.full(cr.side_shape(n, 0, c), np.nan) for c in range(3)]
    cr.curl_side_ref(u, (0, 0, 0), (7, 7, 7), g, w, 0, (h, h, h), alpha=0.5)
    for c in range(3):
        assert np.array_equal(cr.bits(w[c]), cr.bits(np.full(w[c].shape, omega[c])))


def test_constant_field_gives_positive_zero():
    n, g = [8, 8, 8], 1
    u = [np.full(cr.side_shape(n, g, c), v) for c, v in enumerate((1.5, -0.375, 7.0))]
    for vals in (cr.curl_values(u, n, g, DX), cr.curl_values(u, n, g, (2.0 ** -4,) * 3)):
        for c in range(3):
            assert not cr.bits(vals[c]).any()  # +0.0 is all-zero bits


def periodic_case(seed):
    n = [7, 5, 6]
    rng = np.random.default_rng(seed)
    a = [rng.standard_normal(cr.side_shape(n, 0, c)) for c in range(3)]
    b = [rng.standard_normal(cr.side_shape(n, 0, c)) for c in range(3)]
    return n, a, b


def unique(v, n):
    """The unique points of a periodic side-box array: the face iupper + 1 is the image of ilower."""
    return v[:n[2], :n[1], :n[0]]


def test_self_adjoint_on_a_periodic_box():
    """<curl a, b> == <a, curl b> over the unique points to 64 * 2^-52 * S, S = sum |b|
    curl_abs(a) + |a| curl_abs(b): each curl value carries 17 roundings (two sums of 7, two
    scalings, one difference), so the first-order bound is 17 * 2^-53 per value; the
    factor 64 * 2^-52 leaves about 7 over it."""
    n, a, b = periodic_case(11)
    per = (1, 1, 1)
    ca, cb = cr.curl_values(a, n, 0, DX, per), cr.curl_values(b, n, 0, DX, per)
    aa, ab = cr.curl_abs(a, n, 0, DX, per), cr.curl_abs(b, n, 0, DX, per)
    lhs = math.fsum(float(x) for c in range(3) for x in (unique(ca[c], n) * unique(b[c], n)).ravel())
    rhs = math.fsum(float(x) for c in range(3) for x in (unique(a[c], n) * unique(cb[c], n)).ravel())
    S = math.fsum(float(x) for c in range(3)
                  for x in (np.abs(unique(b[c], n)) * unique(aa[c], n) + np.abs(unique(a[c], n)) * unique(ab[c], n)).ravel())
    print(f"self-adjointness: |lhs - rhs| = {abs(lhs - rhs):.3e} = {abs(lhs - rhs) / (2.0 ** -53 * S):.4f} * 2^-53 * S")
    assert abs(lhs - rhs) <= 64 * ULP * S


def test_discrete_divergence_of_the_curl_vanishes():
    """The torque force 0.5 curl n is divergence-free on the grid: the side-to-cell
    divergence of curl a is at most 64 * 2^-52 * max curl_abs(a) * sum_d 1/dx[d]."""
    n, a, _ = periodic_case(12)
    per = (1, 1, 1)
    ca = cr.curl_values(a, n, 0, DX, per)
    div = ((ca[0][:, :, 1:] - ca[0][:, :, :-1]) / DX[0] + (ca[1][:, 1:, :] - ca[1][:, :-1, :]) / DX[1]
           + (ca[2][1:, :, :] - ca[2][:-1, :, :]) / DX[2])
    bound = 64 * ULP * max(float(v.max()) for v in cr.curl_abs(a, n, 0, DX, per)) * sum(1.0 / h for h in DX)
    print(f"divergence: max |div| = {np.abs(div).max():.3e}, bound {bound:.3e}, max |curl| = "
          f"{max(float(np.abs(v).max()) for v in ca):.3g}")
    assert div.shape == (n[2], n[1], n[0])
    assert np.abs(div).max() <= bound


def test_periodic_fill_rule():
    """regrow / periodic_fill: interior kept, ghosts and the face iupper + 1 at their images,
    a non-periodic dim's ghost values kept."""
    n, g = [4, 3, 2], 2
    rng = np.random.default_rng(5)
    u = [rng.standard_normal(cr.side_shape(n, g, c)) for c in range(3)]
    f = cr.periodic_fill(u, n, g, (1, 0, 1))
    for c in range(3):
        assert np.array_equal(f[c][g:g + n[2], :, g:g + n[0]], u[c][g:g + n[2], :, g:g + n[0]])  # y ghosts kept
        assert np.array_equal(f[c][g:g + n[2], :, 0], u[c][g:g + n[2], :, n[0]])  # x = -2 reads x = 2
    assert np.array_equal(f[0][g, g, g + n[0]], u[0][g, g, g])  # the x face iupper + 1 reads ilower
    assert np.array_equal(f[2][g + n[2], g, g], u[2][g, g, g])


def test_header_declares_curl_side_and_library_exports_it():
    text = (ROOT / "include" / "ibtk_le.h").read_text()
    assert re.search(r"int\s+ibtk_le_curl_side\s*\(\s*ibtk_le_ctx\s+ctx", text)
    assert "plain routine" in text.lower()  # the header says what periodic == NULL means
    from ibamr_amd import _lib
    assert any(name == "ibtk_le_curl_side" for name, _, _ in _lib._SIGS)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "ibtk_le_curl_side")


def test_gib_exports():
    from ibamr_amd import gib
    for name in ("curl_side", "interp_angular_velocity", "spread_torque"):
        assert callable(getattr(gib, name))
    tile = gib.CURL_TILE
    assert len(tile) == 3 and all(isinstance(v, int) and v >= 1 for v in tile)
    # the Python constants are those the kernel is compiled with
    text = (ROOT / "ibamr_amd" / "csrc" / "le_curl.h").read_text()
    consts = {k: int(v) for k, v in re.findall(r"\b(CURL_T[XYZ]|CURL_MIN_SEG)\s*=\s*(\d+)", text)}
    assert tile == (consts["CURL_TX"], consts["CURL_TY"], consts["CURL_TZ"])
    assert gib.CURL_MIN_SEGMENT == consts["CURL_MIN_SEG"]

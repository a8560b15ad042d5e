"""CPU tests of the fluid-source stages: the numpy restatement (tests/source_ref.py) against
50-digit known answers (tests/golden/source_kat.npz, made by tests/golden/make_source_kat.py),
the identities of the cosine kernel on whole-cell radii, the preconditions of the cases the
GPU tests run, the exports, and the argument checks that need no device.  No GPU.
"""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import source_cases as sc
import source_ref as sr

ROOT = Path(__file__).resolve().parents[1]
ULP = 2.0 ** -52
STORED = ("main", "clip", "many", "main2", "clip2", "many2")


@pytest.fixture(scope="module")
def kat():
    return np.load(ROOT / "tests" / "golden" / "source_kat.npz")


def rel(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


# ---- source_ref against the known answers ---------------------------------------------------

@pytest.mark.parametrize("name", STORED)
def test_ref_against_50_digits(kat, name):
    c = sc.case(name)
    geo = c["geo"]
    # every 1-D weight: |w - exact| r in units of 2^-53
    k, worst = 0, 0.0
    for n in range(len(c["Q"])):
        X = [float(v) for v in c["X_src"][n]]
        st = sr.stencil(geo, float(c["r_src"][n]), X)
        for d in range(geo.ndim):
            for i in range(st[d]["lo"], st[d]["hi"] + 1):
                worst = max(worst, abs(sr.weight_1d(geo, st, X, d, i) - float(kat[f"{name}_w"][k])) * st[d]["r"] / 2.0 ** -53)
                k += 1
    assert k == kat[f"{name}_w"].size
    tol_P = 8 * max(float(kat["ref_err_P"]), ULP)
    eP, ePn = rel(c["P"], kat[f"{name}_P"]), rel(c["P_normed"], kat[f"{name}_P_normed"])
    print(f"{name}: w {worst:.3f} (recorded {float(kat['ref_err_w']):.3f}), P {eP:.3e}, P - p_norm {ePn:.3e}")
    assert worst <= 8 * max(float(kat["ref_err_w"]), 1.0)
    assert eP <= tol_P and ePn <= tol_P
    assert abs(c["p_norm"] - float(kat[f"{name}_p_norm"])) <= tol_P * np.abs(c["p"]).max()
    if f"{name}_q" in kat:
        eq = rel(c["q"][geo.box_slices()], kat[f"{name}_q"])
        print(f"{name}: q {eq:.3e}")
        assert eq <= 8 * max(float(kat["ref_err_q"]), ULP)


@pytest.mark.parametrize("nd", [3, 2])
def test_locations_against_50_digits(kat, nd):
    X, node, source, n_src = sc.node_lists(nd)
    got = sr.locations(X, node, source, n_src)
    assert rel(got, kat[f"Xsrc{nd}"]) <= 8 * max(float(kat["ref_err_Xsrc"]), ULP)
    assert (got[2] == 0.0).all()  # the source without nodes stays Point::Zero()
    counts = np.bincount(source, minlength=n_src)
    assert counts.tolist() == [1, sc.BIG, 0, 40] and not np.all(np.diff(node) > 0)  # shuffled
    one = int(node[source == 0][0])
    assert np.array_equal(sr.bits(got[0]), sr.bits(X[one] / 1.0))


# ---- the radius, half-width and tie rules ----------------------------------------------------

def test_radius_and_half_width():
    dx = sc.DX
    R = lambda r, h: max(math.floor(r / h + 0.5), 2.0)  # noqa: E731
    assert [R(0.03, h) for h in dx] == [2.0, 2.0, 2.0]                 # clamped
    assert [R(0.2, h) for h in dx] == [4.0, 3.0, 4.0]                  # differs per dimension
    assert 2.5 / 16.0 / dx[1] + 0.5 == 3.0 and R(2.5 / 16.0, dx[1]) == 3.0  # the tie, exactly
    # int((R dx) / dx) + 1 is R for some spacings and R + 1 for others
    assert int((3.0 * dx[0]) / dx[0]) == 2 and int((3.0 * dx[1]) / dx[1]) == 3
    geo = sc.geo_of("g3")
    st = sr.stencil(geo, 0.12, [0.0, 1.0, 0.4])
    assert st[0]["R"] == 3 and st[0]["half"] == 3 and st[1]["R"] == 2 and st[1]["half"] == 3


def test_cell_index_ties_and_kernel_edges():
    geo = sc.geo_of("g3")
    for d in range(3):
        for k in (0, 5, geo.n[d]):   # a face belongs to the cell above it; the upper face to the first cell outside
            X = geo.x_lower[d] + k * geo.dx[d]
            assert sr.cell_index(X, geo.x_lower[d], geo.x_upper[d], geo.dx[d], geo.ilower[d], geo.iupper[d]) == geo.ilower[d] + k
    assert sr.cos_kernel(0.25, 0.25) == 0.0 and sr.cos_kernel(-0.25, 0.25) == 0.0  # exactly |x| = r
    assert sr.cos_kernel(np.nextafter(0.25, 1.0), 0.25) == 0.0
    assert sr.cos_kernel(0.0, 0.25) == 4.0


# ---- identities -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["main", "many", "main2", "many2"])
def test_unclipped_sources_integrate_to_their_strengths(name):
    """Over whole-cell radii the cosine kernel sums to 1 per dimension, so sum q dV = sum Q
    to rounding: 1e-13 relative (to sum |Q|)."""
    c = sc.case(name)
    geo = c["geo"]
    for n in range(len(c["Q"])):
        one = sr.spread(geo, geo.alloc(), c["X_src"][n:n + 1], c["r_src"][n:n + 1], c["Q"][n:n + 1])
        tot = math.fsum(float(v) for v in one[geo.box_slices()].ravel()) * geo.dV()
        assert abs(tot - c["Q"][n]) <= 1e-13 * abs(c["Q"][n])
    assert abs(c["totals"][0] - c["totals"][1]) <= 1e-13 * np.abs(c["Q"]).sum()
    assert not c["flagged"]


@pytest.mark.parametrize("name", list(sc.UNCLIPPED) + list(sc.CLIPPED))
def test_normalized_field_integrates_to_zero(name):
    c = sc.case(name)
    geo = c["geo"]
    after = math.fsum(float(v) for v in c["q_norm"][geo.box_slices()].ravel()) * geo.dV()
    assert abs(after) <= 1e-10 * max(1.0, np.abs(c["q_norm"][geo.box_slices()]).max())
    assert abs(c["totals"][3]) <= 1e-10 * max(1.0, np.abs(c["q_norm"][geo.box_slices()]).max())
    # only the boundary cells moved, each by q_norm; ghosts untouched
    moved = c["q_norm"] != c["q_zero"]
    box = np.zeros(geo.shape(), bool)
    box[geo.box_slices()] = True
    assert np.array_equal(moved, sr.bdry_mask(geo, c["domain"]) & box)
    assert c["flagged"] == (name in sc.CLIPPED)  # a clipped source loses part of its strength


@pytest.mark.parametrize("name", ["main", "main2"])
def test_constant_pressure_is_reproduced(name):
    c = sc.case(name)
    geo = c["geo"]
    P = sr.pressure(geo, np.full(geo.shape(), 3.25), c["X_src"], c["r_src"])
    assert np.abs(P - 3.25).max() <= 1e-13 * 3.25
    # and with the normalisation pressure of a constant field, nothing is left
    Pn = sr.pressure(geo, np.full(geo.shape(), 3.25), c["X_src"], c["r_src"], c["domain_big"])
    assert np.abs(Pn).max() <= 1e-12


@pytest.mark.parametrize("name", ["clip", "many2"])
def test_adjointness(name):
    """sum q p dV = sum Q (P + p_norm): the same products in two orders."""
    c = sc.case(name)
    geo = c["geo"]
    lhs = math.fsum(float(v) for v in (c["q_zero"] * c["p"])[geo.box_slices()].ravel()) * geo.dV()
    rhs = math.fsum(float(a) * float(b) for a, b in zip(c["Q"], c["P"]))
    scale = math.fsum(abs(float(a)) * float(b) for a, b in zip(c["Q"], c["P_abs"]))
    assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-12 * scale


# ---- the GPU tests' cases -------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CASES)
def test_case_preconditions(name):
    c = sc.case(name)
    geo = c["geo"]
    n_src = len(c["Q"])
    if name == "none":
        assert n_src == 0
        return
    smallest = sc.check_weights(geo, c["r_src"], c["X_src"])
    print(f"{name}: smallest non-zero weight times r0 r1 r2 = {smallest:.3e}")
    assert set(np.unique(c["r_src"])) <= set(sc.RADII)
    sts = [sr.stencil(geo, float(c["r_src"][n]), [float(v) for v in c["X_src"][n]]) for n in range(n_src)]
    unclipped = [all(s["lo"] == s["centre"] - s["half"] and s["hi"] == s["centre"] + s["half"] for s in st) for st in sts]
    if name in sc.CLIPPED:
        cut = [d for d, s in enumerate(sts[-1]) if s["lo"] != s["centre"] - s["half"] or s["hi"] != s["centre"] + s["half"]]
        assert cut == [0, 1] and all(unclipped[:-1])  # cut at two patch faces, within R cells of each
        assert sts[-1][0]["centre"] - geo.ilower[0] < sts[-1][0]["R"] and geo.iupper[1] - sts[-1][1]["centre"] < sts[-1][1]["R"]
    else:
        assert all(unclipped)
    tile = 8
    if name.startswith("main") or name.startswith("clip"):
        for d in range(geo.ndim):  # some box is wider than a tile in every dimension: the tile loop repeats
            assert max(st[d]["hi"] - st[d]["lo"] + 1 for st in sts) > tile
        assert c["cnt"].max() >= 2  # overlapping boxes
        Rs = {tuple(s["R"] for s in st) for st in sts}
        assert any(len(set(R)) > 1 for R in Rs) and any(set(R) == {2} for R in Rs)
        # both half-width outcomes
        assert any(s["half"] == s["R"] for st in sts for s in st) and any(s["half"] == s["R"] + 1 for st in sts for s in st)
    if name.startswith("many"):
        assert n_src == sc.MANY > 64 and c["cnt"].max() >= 3
    assert np.abs(c["Q"]).min() >= 0.2  # the bound's scale S_i dwarfs the initial field (|q0| < 6)
    assert np.abs(c["q0"]).max() < 6.0


# ---- exports and host-side argument checks ----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ibamr_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ibamr_amd import build
        build.build()
    return _lib.load()


NAMES = ("ibtk_le_sources_create", "ibtk_le_sources_destroy", "ibtk_le_source_locations", "ibtk_le_source_spread",
         "ibtk_le_source_normalize", "ibtk_le_source_pressure")


def test_header_declares_and_library_exports_the_source_calls(lib):
    text = (ROOT / "include" / "ibtk_le.h").read_text()
    from ibamr_amd import _lib
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert re.search(r"int\s+" + name + r"\s*\(", text), name
        assert any(n == name for n, _, _ in _lib._SIGS) and hasattr(raw, name)
    assert "flag 32" in text  # the new flag is documented beside the others
    from ibamr_amd.build import SOURCES
    assert "le_source.hip" in SOURCES


def test_sources_module_exports():
    from ibamr_amd import io, sources
    for name in ("SourceSpecs", "Sources", "SourceArrays"):
        assert name in sources.__all__ and hasattr(sources, name)
    for name in ("read_source", "write_source", "SourceDeck"):
        assert name in io.__all__
    text = (ROOT / "ibamr_amd" / "csrc" / "le_source.h").read_text()
    consts = {k: int(v) for k, v in re.findall(r"\b(SRC_RMAX|SRC_CHUNK|SRC_FLAG|SRC_TILE3|SRC_TILE2)\s*=\s*(\d+)", text)}
    assert consts["SRC_RMAX"] == sources.R_MAX >= 16 and consts["SRC_FLAG"] == sources.FLAG == 32
    assert consts["SRC_CHUNK"] == 64 < sc.MANY and consts["SRC_TILE3"] == consts["SRC_TILE2"] == 8


def test_null_context_is_an_argument_error(lib):
    """Every entry point returns IBTK_LE_ERR_ARG for a null context and touches nothing else:
    the output handle and the (host) stand-ins for device arrays keep their bytes."""
    from ibamr_amd._lib import PatchGeom
    err = lambda: lib.ibtk_le_last_error().decode()  # noqa: E731
    buf = (ctypes.c_double * 16)(*([7.5] * 16))
    p = ctypes.cast(buf, ctypes.c_void_p)
    ints = (ctypes.c_int * 3)(0, 0, 0)
    ip = ctypes.cast(ints, ctypes.c_void_p)
    g = PatchGeom.make((0, 0, 0), (7, 7, 7), 2, (0.1, 0.1, 0.1), (0.0, 0.0, 0.0))
    h = ctypes.c_void_p(1234)
    assert lib.ibtk_le_sources_create(None, 3, 4, 1, p, 1, ip, ip, ctypes.byref(h)) == 4 and "null context" in err()
    assert h.value == 1234
    fake = ctypes.c_void_p(8)  # never dereferenced: the context is checked first
    assert lib.ibtk_le_source_locations(None, fake, p, p) == 4 and "null context" in err()
    assert lib.ibtk_le_source_spread(None, fake, ctypes.byref(g), p, p, p) == 4 and "null context" in err()
    assert lib.ibtk_le_source_normalize(None, fake, ctypes.byref(g), p, ip, ip, p, 1, p) == 4 and "null context" in err()
    assert lib.ibtk_le_source_pressure(None, fake, ctypes.byref(g), p, p, p, None, None) == 4 and "null context" in err()
    assert list(buf) == [7.5] * 16 and list(ints) == [0, 0, 0]
    assert lib.ibtk_le_sources_destroy(None) == 0

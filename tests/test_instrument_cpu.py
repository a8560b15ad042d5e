"""CPU tests of the flow meters and pressure gauges: the scalar restatement
(tests/instrument_ref.py) against exact known answers (tests/golden/instrument_kat.npz, made by
tests/golden/make_instrument_kat.py with fractions.Fraction, and decimal at 50 digits for |dA|),
two identities of the meter, the preconditions of the cases the GPU tests run, the ``.inst``
deck reader, the exports and the log format.  No GPU.

The restatement is held to 8 times the error the generator measured for it, per quantity, in
units of 2^-53 times the sum of the absolute terms (the margin the source tests give).  Measured
when the answers were made: X_web 8.0, dA_web 9318 (the differences X2 - X0 and X3 - X1 cancel:
the corners are rounded relative to |X|, their differences are half a mesh width), flow 10.6, mean
pressure 29.9, point pressure 99.0 (a weight is a difference of coordinates over dx), correction
8.9.
"""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import instrument_cases as ic
import instrument_ref as ir

ROOT = Path(__file__).resolve().parents[1]
STORED = ("small", "tie", "cut", "outside", "big")
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def kat():
    return np.load(ROOT / "tests" / "golden" / "instrument_kat.npz")


def units(got, exact, scale):
    diff = np.abs(np.asarray(got, dtype=np.float64) - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, diff / (U53 * scale), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def flat_webs(c, key):
    return np.array([w[key][m][n] for w in c["webs"] for m in range(w["P"]) for n in range(w["nw"])]).reshape(-1, 3)


# ---- instrument_ref against the exact answers -------------------------------------------------

@pytest.mark.parametrize("name", STORED)
def test_ref_against_exact_answers(kat, name):
    c = ic.case(name)
    e = dict(Xweb=units(flat_webs(c, "X_web"), kat[f"{name}_Xweb"], kat[f"{name}_S_Xweb"]),
             dA=units(flat_webs(c, "dA_web"), kat[f"{name}_dA"], kat[f"{name}_S_dA"]),
             corr=units([s["corr"] for s in c["stats"]], kat[f"{name}_corr"], kat[f"{name}_S_corr"]))
    for j, k in enumerate(("flow", "mean", "point")):
        e[k] = units(c["values"][:, j], kat[f"{name}_values"][:, j], kat[f"{name}_S_values"][:, j])
    print(name, {k: round(v, 3) for k, v in e.items()}, "recorded", {k: round(float(kat[f"ref_err_{k}"]), 3) for k in e})
    for k, v in e.items():
        assert v <= 8.0 * max(float(kat[f"ref_err_{k}"]), 1.0), (k, v)


# ---- identities ---------------------------------------------------------------------------------

def affine_fields(geo, A, b, q, r):
    """u_a = A[a] . x + b[a] at the side centres, p = q . x + r at the cell centres."""
    def coords(shift):
        return [geo.x_lower[d] + geo.dx[d] * (np.arange(-geo.g, geo.n[d] + geo.g + (1 if shift[d] else 0))
                                              + (0.0 if shift[d] else 0.5)) for d in range(3)]
    u = []
    for a in range(3):
        x, y, z = coords([d == a for d in range(3)])
        Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
        u.append(A[a][0] * X + A[a][1] * Y + A[a][2] * Z + b[a])
    x, y, z = coords([False] * 3)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return u, q[0] * X + q[1] * Y + q[2] * Z + r


def test_affine_fields_are_reproduced(kat):
    """Trilinear interpolation reproduces an affine field, so flow = sum u(X_web) . dA minus the
    correction and mean = p at the area-weighted centroid, to the measured bounds."""
    c = ic.case("big")
    geo, webs = c["geo"], c["webs"]
    A = [[0.3, -0.2, 0.5], [0.1, 0.4, -0.6], [-0.7, 0.2, 0.3]]
    b, q, r = [0.2, -0.1, 0.4], [1.5, -0.5, 0.8], 0.3
    u, p = affine_fields(geo, A, b, q, r)
    values, stats = ir.read(geo, webs, u, p, c["U"], c["meters"])
    for l, w in enumerate(webs):
        flow, area, cen, scale = 0.0, 0.0, [0.0] * 3, 0.0
        for m in range(w["P"]):
            for n in range(w["nw"]):
                X, dA = w["X_web"][m][n], w["dA_web"][m][n]
                ux = [sum(A[a][d] * X[d] for d in range(3)) + b[a] for a in range(3)]
                flow += sum(ux[a] * dA[a] for a in range(3))
                scale += sum(abs(ux[a] * dA[a]) for a in range(3))
                a_ = ir.norm(dA)
                area += a_
                for d in range(3):
                    cen[d] += a_ * X[d]
        cen = [v / area for v in cen]
        want_mean = sum(q[d] * cen[d] for d in range(3)) + r
        tol = 8.0 * max(float(kat["ref_err_flow"]), 1.0) * U53
        assert abs(stats[l]["flow"] - flow) <= tol * 16 * scale  # 8 cells x 3 axes of weights of size <= 1 / dx a term
        assert abs(values[l, 1] - want_mean) <= 8.0 * max(float(kat["ref_err_mean"]), 1.0) * U53 * 16 * (abs(want_mean) + 3.0)
        pc = sum(q[d] * w["Xc"][d] for d in range(3)) + r
        assert abs(values[l, 2] - pc) <= 8.0 * max(float(kat["ref_err_point"]), 1.0) * U53 * (abs(pc) + 3.0)


@pytest.mark.parametrize("name", ["big", "wave"])
def test_a_meter_carried_by_a_uniform_flow_reads_zero(kat, name):
    """u = V everywhere and every marker moving with V: the web and the correction's fan of
    triangles span the same perimeter polygon, so their area vectors are equal (planar or not)
    and the flux through the web and the correction cancel to the measured bound."""
    c = ic.case(name)
    geo, webs = c["geo"], c["webs"]
    V = [0.7, -0.4, 0.9]
    u = [np.full(s, V[a]) for a, s in enumerate(ir.side_shapes(geo))]
    U = np.tile(np.array(V), (c["X"].shape[0], 1))
    values, stats = ir.read(geo, webs, u, None, U, c["meters"])
    for l, w in enumerate(webs):
        scale = sum(abs(V[a] * w["dA_web"][m][n][a]) for m in range(w["P"]) for n in range(w["nw"]) for a in range(3))
        bound = 8.0 * max(float(kat["ref_err_flow"]), float(kat["ref_err_dA"]), 1.0) * U53 * scale
        print(f"flow {stats[l]['flow']!r} correction {stats[l]['corr']!r} difference {values[l, 0]:.3e} bound {bound:.3e}")
        assert stats[l]["flow"] != 0.0 and abs(values[l, 0]) <= bound
        assert math.isnan(values[l, 1]) and values[l, 2] == 0.0  # no p: 0 / 0 and 0


# ---- the GPU tests' cases -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ic.CASES)
def test_case_preconditions(name):
    c = ic.case(name)
    geo, webs = c["geo"], c["webs"]
    if name == "none":
        assert len(webs) == 0 and c["values"].shape == (0, 3)
        return
    plain, _ = ir.read(geo, webs, c["u"], c["p"], c["U"], c["meters"], plain=True)
    # the order is under test: for some meter the reference-order total differs in bits from the (m, n)-order one
    differs = [bool((ir.bits(plain[l, :2]) != ir.bits(c["values"][l, :2])).any()) for l in range(len(webs))]
    print(name, "order matters for meters", [n for n, d in zip(c["names"], differs) if d])
    assert any(differs), f"{name}: redraw FIELD_SEED"
    for w, mname in zip(webs, c["names"]):
        per_cell = {}
        for m in range(w["P"]):
            for n in range(w["nw"]):
                if w["counted"][m][n]:
                    per_cell[w["cell"][m][n]] = per_cell.get(w["cell"][m][n], 0) + 1
        assert w["P"] * w["nw"] > 1 and max(per_cell.values()) >= 2, mname  # a cell holds two of its patches
        assert w["nw"] <= c["cap"]
    assert max(w["nw"] for w in webs) == c["cap"]  # the capacity is exactly the widest web


def test_meter_shapes():
    w = {n: ic.webs_of((n,))[0] for n in ic.METERS}
    assert [w[n]["P"] for n in ("tri", "quad", "ring17", "ring70")] == [3, 4, 17, 70]
    assert w["tri"]["r_max"] <= ic.H and w["quad"]["r_max"] <= ic.H and w["tri"]["nw"] == w["quad"]["nw"] == 2
    assert 6.25 * ic.H < w["ring17"]["r_max"] < 6.35 * ic.H and w["ring17"]["nw"] == 14
    assert w["ring70"]["nw"] == 16 and 70 * 16 > 1024 and 70 > 64
    assert ic.H == ic.DX[0] < min(ic.DX[1:])  # h_finest = min(dx) matters
    # planar and slightly non-planar perimeters
    def off_plane(name):
        X = ic.perimeter(name)
        _, _, vt = np.linalg.svd(X - X.mean(0))
        return np.abs((X - X.mean(0)) @ vt[2]).max()
    assert off_plane("ring70") < 1e-12 and 0.03 * ic.H < off_plane("ring17") < 0.11 * ic.H
    assert off_plane("tri") < 1e-12 and off_plane("quad") > 0.03 * ic.H


def test_tie_case_sits_on_faces_and_centres():
    wz, wy = ic.webs_of(("tie_z", "tie_y"))
    on_face = [X for row in wz["X_web"] for X in row if ic.on_face(X[2], 2)]
    assert len(on_face) >= 10 and len(on_face) == wz["P"] * wz["nw"]
    # getCellIndex's tie: a face belongs to the cell above it
    k = round((on_face[0][2] - ic.X_LOWER[2]) / ic.DX[2])
    assert all(c[2] == ic.ILOWER[2] + k for row in wz["cell"] for c in row)
    on_centre = [X for row in wy["X_web"] for X in row if ic.on_centre(X[1], 1)]
    assert len(on_centre) >= 10  # X < X_cell is false there: the upper neighbours, with weight 0 on the far one
    # in-plane ties too: the corners are multiples of 2^-6 about a centre on the grid's lines
    assert any(ic.on_face(X[0], 0) or ic.on_face(X[1], 1) for row in wz["X_web"] for X in row)


def test_cut_and_outside_cases():
    (w,) = ic.webs_of(("cut",))
    geo = ic.GEO
    counted = np.array(w["counted"])
    cells = np.array(w["cell"])
    assert counted.any() and (~counted).any() and counted.sum() * 4 >= counted.size
    dropped = cells[~counted]
    assert (dropped[:, 0] < geo.ilower[0]).any() and (dropped[:, 1] > geo.iupper[1]).any()  # two patch faces
    assert w["cen_counted"]
    (w,) = ic.webs_of(("outside",))
    assert not w["cen_counted"] and np.array(w["counted"]).any()
    c = ic.case("outside")
    assert c["values"][0, 2] == 0.0 and c["values"][0, 1] != 0.0
    # two meters sharing cells
    a, b = ic.webs_of(("ring17", "ring70"))
    cells_of = lambda w: {w["cell"][m][n] for m in range(w["P"]) for n in range(w["nw"])}  # noqa: E731
    assert len(cells_of(a) & cells_of(b)) >= 10
    z = ic.case("cut_u0")
    assert not z["U"].any() and z["stats"][0]["corr"] == 0.0 and ic.case("cut")["stats"][0]["corr"] != 0.0


def test_zero_radius_meter_and_null_fields():
    """r_max == 0: nw = 0, flow = 0 - correction, mean = 0 / 0."""
    geo = ic.GEO
    X = np.tile(np.array([[0.25, 1.0, 0.5]]), (4, 1))  # (the sum and the product by 1 / 4 are exact)
    webs = ir.update(geo, X, [[0, 1, 2, 3]])
    assert webs[0]["nw"] == 0 and webs[0]["cen_counted"]
    u, p = ic.fields(0)
    values, stats = ir.read(geo, webs, u, p, np.ones((4, 3)), [[0, 1, 2, 3]])
    assert values[0, 0] == 0.0 and math.isnan(values[0, 1]) and values[0, 2] != 0.0
    c = ic.case("small")
    assert np.isnan(c["values_no_p"][:, 1]).all() and (c["values_no_p"][:, 2] == 0.0).all()
    assert np.array_equal(c["values_no_p"][:, 0], c["values"][:, 0])
    assert np.array_equal(c["values_no_u"][:, 1:], c["values"][:, 1:])
    assert np.array_equal(c["values_no_u"][:, 0], np.array([0.0 - s["corr"] for s in c["stats"]]))


# ---- the deck reader ----------------------------------------------------------------------------

GOOD = """2   # two meters
  aortic valve  ! trailing comment
outlet
5
0 1 0
4 0 1
2 1 1   % a node
3 0 0
1 0 2
"""


def write(tmp_path, text, name="m.inst"):
    p = tmp_path / name
    p.write_text(text)
    return p


def test_read_inst_format_and_round_trip(tmp_path):
    from ibamr_amd import io
    d = io.read_inst(write(tmp_path, GOOD), 5)
    assert d.names == ["aortic valve", "outlet"]
    assert d.node.tolist() == [0, 1, 2, 3, 4] and d.meter.tolist() == [1, 0, 1, 0, 0] and d.meter_node.tolist() == [0, 2, 1, 0, 1]
    assert d.node.dtype == d.meter.dtype == d.meter_node.dtype == np.int32
    d = io.read_inst(write(tmp_path, GOOD), 5, vertex_offset=10, instrument_offset=3)
    assert d.node.tolist() == [10, 11, 12, 13, 14] and d.meter.tolist() == [4, 3, 4, 3, 3]
    assert d.meter_node.tolist() == [0, 2, 1, 0, 1]
    c = ic.case("eight")
    node, meter, meter_node = c["triples"]
    p = tmp_path / "rt.inst"
    io.write_inst(p, list(c["names"]), node, meter, meter_node)
    d = io.read_inst(p, c["X"].shape[0])
    o = np.argsort(node)
    assert d.names == list(c["names"]) and np.array_equal(d.node, node[o]) and np.array_equal(d.meter, meter[o])
    assert np.array_equal(d.meter_node, meter_node[o])
    # a vertex listed twice keeps its last entry (the reference stores a map)
    d = io.read_inst(write(tmp_path, "1\na\n3\n1 0 0\n2 0 1\n1 0 1\n"), 4)
    assert d.node.tolist() == [1, 2] and d.meter_node.tolist() == [1, 1]


@pytest.mark.parametrize("text, line, detail", [
    ("", 1, "Premature end"),
    ("x\n", 1, "Invalid entry"),
    ("0\n", 1, "Invalid entry"),
    ("2\na\n", 3, "Premature end"),
    ("2\na\nb\n", 4, "Premature end"),
    ("2\na\nb\nzero\n", 4, "Invalid entry"),
    ("2\na\nb\n0\n", 4, "Invalid entry"),
    ("2\na\nb\n2\n0 0 0\n", 6, "Premature end"),
    ("2\na\nb\n2\n0 0 0\nq 1 0\n", 6, "Invalid entry"),
    ("2\na\nb\n2\n0 0 0\n5 1 0\n", 6, "vertex index 5 is out of range"),
    ("2\na\nb\n2\n0 0 0\n-1 1 0\n", 6, "vertex index -1 is out of range"),
    ("2\na\nb\n2\n0 0 0\n1\n", 6, "Invalid entry"),
    ("2\na\nb\n2\n0 2 0\n1 1 0\n", 5, "meter index 2 is out of range"),
    ("2\na\nb\n2\n0 -1 0\n1 1 0\n", 5, "meter index -1 is out of range"),
    ("2\na\nb\n2\n0 0 0\n1 1\n", 6, "Invalid entry"),
    ("2\na\nb\n2\n0 0 0\n1 1 -1\n", 6, "meter node index is negative"),
])
def test_read_inst_errors_name_the_line(tmp_path, text, line, detail):
    from ibamr_amd import io
    p = write(tmp_path, text)
    with pytest.raises(ValueError) as e:
        io.read_inst(p, 5)
    msg = str(e.value)
    assert detail in msg and f"line {line} of file {p}" in msg, msg


@pytest.mark.parametrize("text, detail", [
    ("2\na\nb\n2\n0 1 0\n1 1 1\n", "Instrument index 0 not found in input file"),
    ("2\na\nb\n2\n0 0 0\n1 0 2\n", "Node index 1 associated with meter index 0 not found in input file"),
    ("2\na\nb\n2\n0 0 0\n1 0 1\n", "Expected to find 2 distinct meter indices in input file"),
])
def test_read_inst_completeness_errors(tmp_path, text, detail):
    from ibamr_amd import io
    p = write(tmp_path, text)
    with pytest.raises(ValueError) as e:
        io.read_inst(p, 5)
    assert detail in str(e.value) and str(p) in str(e.value)


def test_missing_file_writer_arguments_and_specs(tmp_path):
    from ibamr_amd import io
    from ibamr_amd.instruments import MeterSpecs
    with pytest.raises(FileNotFoundError):
        io.read_inst(tmp_path / "none.inst", 3)
    with pytest.raises(ValueError):
        io.write_inst(tmp_path / "w.inst", ["a # b"], [0], [0], [0])
    with pytest.raises(ValueError):
        io.write_inst(tmp_path / "w.inst", ["a"], [0, 1], [0], [0])
    io.write_inst(tmp_path / "a.inst", ["a0", "a1"], [0, 3, 2, 1], [1, 0, 1, 0], [0, 1, 1, 0])
    io.write_inst(tmp_path / "b.inst", ["b0"], [1, 0, 2], [0, 0, 0], [0, 2, 1])
    da = io.read_inst(tmp_path / "a.inst", 4)
    db = io.read_inst(tmp_path / "b.inst", 3, vertex_offset=4, instrument_offset=2)
    s = MeterSpecs.from_deck(da, db, num_vertex=7)
    assert s.names == ["a0", "a1", "b0"] and s.num_meters == 3 and s.num_perimeter_nodes.tolist() == [2, 2, 3]
    assert s.node.tolist() == [0, 1, 2, 3, 4, 5, 6] and s.meter.tolist() == [1, 0, 1, 0, 2, 2, 2]
    assert s.meter_node.tolist() == [0, 0, 1, 1, 2, 0, 1]
    with pytest.raises(ValueError):  # the second deck read without its instrument offset
        MeterSpecs.from_deck(da, io.read_inst(tmp_path / "b.inst", 3, vertex_offset=4), num_vertex=7)
    perm = np.array([6, 5, 4, 3, 2, 1, 0])
    a = s.arrays(perm)
    assert a.node.tolist() == [0, 1, 2, 3, 4, 5, 6] and a.meter.tolist() == [2, 2, 2, 0, 1, 0, 1]
    assert a.meter_node.tolist() == [1, 0, 2, 1, 1, 0, 0] and a.node.dtype == np.int32
    with pytest.raises(ValueError):
        s.arrays(perm[:3])
    with pytest.raises(ValueError):
        MeterSpecs(["a"], [0, 0], [0, 0], [0, 1])  # a node named twice
    with pytest.raises(ValueError):
        MeterSpecs(["a"], [0, 1], [0, 0], [0, 2])  # node index 1 missing
    with pytest.raises(ValueError):
        MeterSpecs(["a"], [0], [1], [0])


# ---- the log format -------------------------------------------------------------------------------

def test_log_lines_format():
    from ibamr_amd.instruments import MeterSpecs, log_lines
    s = MeterSpecs(["aortic valve", "out"], [0, 1, 2, 3], [0, 0, 1, 1], [0, 1, 0, 1])
    values = [[1.5, -2.25e-3, 0.0], [-12345.678, 1.0e100, -0.5]]
    Xc = [[0.5, -1.0, 2.0e-5], [10.0, 0.0, -3.125]]
    lines = s.log_lines(0.125, values, Xc)
    assert lines == [
        "aortic valve  1.25000e-01  5.00000e-01  -1.00000e+00  2.00000e-05  +1.50000e+00  -2.25000e-03  +0.00000e+00",
        "out           1.25000e-01  1.00000e+01  0.00000e+00  -3.12500e+00  -1.23457e+04  +1.00000e+100  -5.00000e-01",
    ]
    assert log_lines(["m"], 2.0, [[1.0, 2.0, 4.0]], [[0.0, 0.0, 0.0]], flow_conv=0.5, pres_conv=0.25) == [
        "m  2.00000e+00  0.00000e+00  0.00000e+00  0.00000e+00  +5.00000e-01  +5.00000e-01  +1.00000e+00"]
    with pytest.raises(ValueError):
        log_lines(["a", "b"], 0.0, [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]])


# ---- exports and host-side argument checks ------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ibamr_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ibamr_amd import build
        build.build()
    return _lib.load()


NAMES = ("ibtk_le_meters_create", "ibtk_le_meters_destroy", "ibtk_le_meters_update", "ibtk_le_meters_read",
         "ibtk_le_meters_workspace")


def test_header_declares_and_library_exports_the_meter_calls(lib):
    text = (ROOT / "include" / "ibtk_le.h").read_text()
    from ibamr_amd import _lib
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert re.search(r"int\s+" + name + r"\s*\(", text), name
        assert any(n == name for n, _, _ in _lib._SIGS) and hasattr(raw, name)
    assert "flag 64" in text  # the new flag is documented beside the others
    from ibamr_amd.build import SOURCES
    assert "le_meter.hip" in SOURCES


def test_instruments_module_exports():
    from ibamr_amd import instruments, io
    for name in ("MeterSpecs", "Meters", "MeterArrays", "log_lines"):
        assert name in instruments.__all__ and hasattr(instruments, name)
    for name in ("read_inst", "write_inst", "InstDeck"):
        assert name in io.__all__
    text = (ROOT / "ibamr_amd" / "csrc" / "le_meter.h").read_text()
    consts = {k: int(v) for k, v in re.findall(r"\b(MTR_MAX_WEB|MTR_FLAG|MTR_WEB_BITS|MTR_BLOCK)\s*=\s*(\d+)", text)}
    assert consts["MTR_MAX_WEB"] == instruments.MAX_WEB == 1 << consts["MTR_WEB_BITS"] and consts["MTR_FLAG"] == instruments.FLAG == 64
    assert 70 * 16 <= instruments.MAX_WEB and consts["MTR_BLOCK"] < 70 * 16  # the largest case repeats a workgroup's loops


def test_null_context_is_an_argument_error(lib):
    """Every entry point returns IBTK_LE_ERR_ARG for a null context and touches nothing else."""
    from ibamr_amd._lib import PatchGeom
    err = lambda: lib.ibtk_le_last_error().decode()  # noqa: E731
    buf = (ctypes.c_double * 16)(*([7.5] * 16))
    p = ctypes.cast(buf, ctypes.c_void_p)
    ints = (ctypes.c_int * 3)(0, 0, 0)
    ip = ctypes.cast(ints, ctypes.c_void_p)
    g = PatchGeom.make((0, 0, 0), (7, 7, 7), 2, (0.1, 0.1, 0.1), (0.0, 0.0, 0.0))
    h = ctypes.c_void_p(1234)
    assert lib.ibtk_le_meters_create(None, 4, 1, 1, ip, ip, ip, 2, ctypes.byref(h)) == 4 and "null context" in err()
    assert h.value == 1234
    fake = ctypes.c_void_p(8)  # never dereferenced: the context is checked first
    assert lib.ibtk_le_meters_update(None, fake, ctypes.byref(g), ip, ip, p, p, 0.1, p) == 4 and "null context" in err()
    assert lib.ibtk_le_meters_read(None, fake, ctypes.byref(g), None, p, p, p) == 4 and "null context" in err()
    assert lib.ibtk_le_meters_workspace(None, fake, 0, p, 3) == 4 and "null context" in err()
    assert list(buf) == [7.5] * 16 and list(ints) == [0, 0, 0]
    assert lib.ibtk_le_meters_destroy(None) == 0

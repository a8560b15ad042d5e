"""CPU: the Kirchhoff rod decks (ibamr_amd.io.read_rod / read_director and their writers),
RodSpecs' flattening into the reference's order, the numpy restatement tests/rod_ref.py
against the 50-digit known answers of tests/golden/rod_kat.json, and the argument checks
of ibtk_le_rodgen_set_rods / ibtk_le_director_update that need no device.
"""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from rod_ref import reference_director_update, reference_rods
from ibamr_amd import io
from ibamr_amd.rods import RodSpecs

GOLDEN = Path(__file__).resolve().parent / "golden"
ROD = GOLDEN / "ibforce" / "curve3d_64.rod"
DIRECTOR = GOLDEN / "ibforce" / "curve3d_64.director"
VERTEX = GOLDEN / "vertex" / "curve3d_64.vertex"


def _tokens(path):
    return [ln.split() for ln in Path(path).read_text().splitlines()]


# ---- the ex4 decks -------------------------------------------------------------------

def test_ex4_rod_deck():
    nv = io.read_vertex(VERTEX, 3).shape[0]
    deck = io.read_rod(ROD, nv)
    assert nv == 200 and deck.curr.size == 200 and deck.params.shape == (200, 10)
    assert np.array_equal(deck.curr, np.arange(200)) and np.array_equal(deck.next, (np.arange(200) + 1) % 200)
    assert (deck.curr[-1], deck.next[-1]) == (199, 0)  # the ring closes, kept as written: next < curr
    tok = _tokens(ROD)
    assert int(tok[0][0]) == 200
    text = np.array([[float(t) for t in row[2:12]] for row in tok[1:201]])
    assert np.array_equal(deck.params, text)  # the parameters are the printed text's doubles


def test_ex4_director_deck_bit_for_bit():
    D = io.read_director(DIRECTOR, 200)
    assert D.shape == (200, 9)
    tok = _tokens(DIRECTOR)
    text = np.array([[float(t) for t in row[:3]] for row in tok[1:601]]).reshape(200, 9)
    # within rounding of unit length: nothing is renormalised, signed zeros included
    assert np.array_equal(D.view(np.int64), text.view(np.int64))
    assert np.abs(np.linalg.norm(D.reshape(-1, 3), axis=1) - 1.0).max() < 1e-15


def test_round_trips_exact(tmp_path):
    rng = np.random.default_rng(3)
    n = 37
    curr, nxt = rng.integers(0, 50, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)
    params = rng.uniform(0.0, 3.0, (n, 10))
    params[:, 7:] -= 1.5  # curvatures of either sign
    io.write_rod(tmp_path / "a.rod", curr, nxt, params)
    deck = io.read_rod(tmp_path / "a.rod", 50)
    assert np.array_equal(deck.curr, curr) and np.array_equal(deck.next, nxt)
    assert np.array_equal(deck.params.view(np.int64), params.view(np.int64))
    D = io.read_director(DIRECTOR, 200)
    io.write_director(tmp_path / "a.director", D)
    assert np.array_equal(io.read_director(tmp_path / "a.director", 200).view(np.int64), D.view(np.int64))
    # the ex4 rod deck through the writer and back
    ex4 = io.read_rod(ROD, 200)
    io.write_rod(tmp_path / "b.rod", *ex4)
    back = io.read_rod(tmp_path / "b.rod", 200)
    assert all(np.array_equal(x, y) for x, y in zip(ex4, back))


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return p


GOOD = "0 1 0.1 1 2 3 4 5 6"


@pytest.mark.parametrize("text, match", [
    ("", "Premature end .* before line 1"),
    ("x\n", "Invalid entry .* line 1"),
    ("0\n", "Invalid entry .* line 1"),
    ("-2\n", "Invalid entry .* line 1"),
    ("2\n" + GOOD + "\n", "Premature end .* before line 3"),
    ("1\nq 1 0.1 1 2 3 4 5 6\n", "Invalid entry .* line 2"),
    ("1\n0 5 0.1 1 2 3 4 5 6\n", "vertex index 5 is out of range"),
    ("1\n-1 1 0.1 1 2 3 4 5 6\n", "vertex index -1 is out of range"),
    ("1\n0 1 -0.1 1 2 3 4 5 6\n", "rod material constant ds is negative"),
    ("1\n0 1 0.1 -1 2 3 4 5 6\n", "rod material constant a1 is negative"),
    ("1\n0 1 0.1 1 -2 3 4 5 6\n", "rod material constant a2 is negative"),
    ("1\n0 1 0.1 1 2 -3 4 5 6\n", "rod material constant a3 is negative"),
    ("1\n0 1 0.1 1 2 3 -4 5 6\n", "rod material constant b1 is negative"),
    ("1\n0 1 0.1 1 2 3 4 -5 6\n", "rod material constant b2 is negative"),
    ("1\n0 1 0.1 1 2 3 4 5 -6\n", "rod material constant b3 is negative"),
    ("1\n0 1 0.1 1 2 3 4 5\n", "Invalid entry .* line 2"),  # b3 missing
    ("1\n0 1 0.1 1 2 zz 4 5 6\n", "Invalid entry .* line 2"),
])
def test_read_rod_errors(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        io.read_rod(_write(tmp_path, "bad.rod", text), 5)


def test_read_rod_missing_file_and_bad_uniform(tmp_path):
    with pytest.raises(FileNotFoundError):
        io.read_rod(tmp_path / "none.rod", 5)
    with pytest.raises(ValueError, match="10 entries"):
        io.read_rod(_write(tmp_path, "a.rod", "1\n" + GOOD + "\n"), 5, uniform_rod_properties=[1.0] * 9)


def test_read_rod_optional_fields_offset_comments_and_uniform(tmp_path):
    text = ("4  # four rods\n" + GOOD + "\n" + "3 2 0.1 1 2 3 4 5 6 -0.5 ! kappa1 alone\n"
            + "1 2 0.2 1 2 3 4 5 6 0.25 -0.75\n" + "2 4 0.0 0 0 0 0 0 0 1 2 3 trailing\n")
    p = _write(tmp_path, "a.rod", text)
    deck = io.read_rod(p, 5, vertex_offset=10)
    assert deck.curr.tolist() == [10, 13, 11, 12] and deck.next.tolist() == [11, 12, 12, 14]  # as written
    assert deck.params[0].tolist() == [0.1, 1, 2, 3, 4, 5, 6, 0, 0, 0]
    assert deck.params[1, 7:].tolist() == [-0.5, 0, 0]
    assert deck.params[2, 7:].tolist() == [0.25, -0.75, 0]
    assert deck.params[3].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 2, 3]  # ds == 0 is read
    uni = np.arange(10.0) + 0.5
    deck = io.read_rod(p, 5, uniform_rod_properties=uni)
    assert np.array_equal(deck.params, np.tile(uni, (4, 1))) and deck.curr.tolist() == [0, 3, 1, 2]


@pytest.mark.parametrize("text, match", [
    ("", "Premature end .* before line 1"),
    ("x\n", "Invalid entry .* line 1"),
    ("3\n", "Invalid entry .* line 1"),  # the count is not num_vertex
    ("2\n1 0 0\n0 1 0\n0 0 1\n1 0 0\n", "Premature end .* before line 6"),
    ("2\n1 0 0\n0 1 0\n0 0 1\n1 0 0\n0 1\n0 0 1\n", "Invalid entry .* line 6"),
    ("2\n1 0 0\n0 q 0\n0 0 1\n1 0 0\n0 1 0\n0 0 1\n", "Invalid entry .* line 3"),
])
def test_read_director_errors(tmp_path, text, match):
    with pytest.raises(ValueError, match=match):
        io.read_director(_write(tmp_path, "bad.director", text), 2)


def test_read_director_normalises_only_when_not_unit(tmp_path):
    tiny = 1.0 + 1e-9   # |norm - 1| below sqrt(DBL_EPSILON): kept as parsed
    off = 1.0 + 1e-7    # above it: divided by the norm
    p = _write(tmp_path, "a.director", f"1\n3 0 4 # norm 5\n0 {tiny!r} 0\n0 0 {off!r}\n")
    D = io.read_director(p, 1)
    assert D[0, 0:3].tolist() == [3 / 5.0, 0.0, 4 / 5.0]
    assert D[0, 3:6].tolist() == [0.0, tiny, 0.0]
    assert D[0, 6:9].tolist() == [0.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        io.write_director(tmp_path / "b.director", np.zeros((0, 9)))


# ---- RodSpecs ------------------------------------------------------------------------

def _specs():
    """7 vertices, 9 rods: a repeated edge (1, 2) with other parameters on its second and
    third line, its reverse (2, 1), which is another edge, next < curr, two masters with
    several rods."""
    curr = [4, 1, 0, 1, 6, 2, 1, 4, 1]
    nxt = [3, 2, 5, 2, 0, 1, 3, 5, 2]
    params = np.arange(90.0).reshape(9, 10) + 1.0
    return RodSpecs(io.RodDeck(np.array(curr), np.array(nxt), params), num_vertex=7), curr, nxt, params


def test_arrays_identity_and_repeated_edge():
    sp, curr, nxt, params = _specs()
    a = sp.arrays()
    # stable by master: deck order within a master
    order = [2, 1, 3, 6, 8, 5, 0, 7, 4]
    assert a.curr.tolist() == [curr[k] for k in order] and a.next.tolist() == [nxt[k] for k in order]
    assert a.curr.dtype == np.int32 and a.next.dtype == np.int32
    want = params[order].copy()
    want[2] = params[1]  # line 3 repeats the edge (1, 2) of line 1: the first line's parameters
    want[4] = params[1]  # and so does line 8
    assert np.array_equal(a.params, want)
    assert np.array_equal(a.params[5], params[5])  # (2, 1) is its own edge
    lag = sp.lagrangian_arrays()
    assert lag.curr.tolist() == curr and np.array_equal(lag.params[[3, 8]], params[[1, 1]])


def test_arrays_random_perm():
    sp, curr, nxt, params = _specs()
    perm = np.random.default_rng(5).permutation(7)
    a = sp.arrays(perm)
    lag = sp.lagrangian_arrays()
    order = sorted(range(9), key=lambda k: (perm[curr[k]], k))
    assert a.curr.tolist() == [int(perm[curr[k]]) for k in order]
    assert a.next.tolist() == [int(perm[nxt[k]]) for k in order]
    assert np.array_equal(a.params, lag.params[order])
    assert np.all(np.diff(a.curr) >= 0)
    with pytest.raises(ValueError, match="perm has"):
        sp.arrays(np.arange(6))


def test_from_files_and_concat(tmp_path):
    ex4 = RodSpecs.from_files(GOLDEN / "ibforce" / "curve3d_64", num_vertex=200)
    assert ex4.num_vertex == 200 and ex4.directors.shape == (200, 9)
    a = ex4.arrays()
    assert np.array_equal(a.curr, np.arange(200)) and a.next[-1] == 0  # next < curr survives
    # a second structure: 3 vertices behind the ring's 200
    io.write_rod(tmp_path / "s.rod", [0, 2], [1, 1], np.ones((2, 10)))
    io.write_director(tmp_path / "s.director", np.tile(np.eye(3).reshape(9), (3, 1)))
    io.write_vertex(tmp_path / "s.vertex", np.zeros((3, 3)))
    second = RodSpecs.from_files(tmp_path / "s", vertex_offset=200)
    assert second.num_vertex == 203 and second.rods.curr.tolist() == [200, 202]
    assert np.all(np.isnan(second.directors[:200]))
    both = RodSpecs.concat([ex4, second])
    assert both.num_vertex == 203 and both.rods.curr.size == 202
    assert np.array_equal(both.directors[:200], ex4.directors) and np.array_equal(both.directors[200:], second.directors[200:])
    perm = np.arange(203)[::-1].copy()
    b = both.arrays(perm)
    assert b.curr[:2].tolist() == [0, 2] and b.next[:2].tolist() == [1, 1]  # vertices 202, 200 come first
    with pytest.raises(ValueError, match="vertex offsets"):
        RodSpecs.concat([second, ex4])


# ---- the host restatement against the 50-digit values -------------------------------

@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "rod_kat.json").read_text())


def _rel(v, ref):
    return float(np.abs(v - ref).max() / np.abs(ref).max())


def test_rod_ref_within_recorded_error(kat):
    r = kat["rods"]
    assert len(r["curr"]) == 64 and np.all(np.array(r["params"])[:, 7:] != 0.0)
    F, N = reference_rods(r["n_nodes"], r["X"], r["D"], r["curr"], r["next"], np.array(r["params"]))
    eF, eN = _rel(F, np.array(r["F"])), _rel(N, np.array(r["N"]))
    d = kat["directors"]
    eD = max(_rel(reference_director_update("euler", d["dt"], d["D"], d["W0"]), np.array(d["D_euler"])),
             _rel(reference_director_update("trapezoidal", d["dt"], d["D"], d["W0"], d["W1"]),
                  np.array(d["D_trapezoidal"])))
    print(f"rod_ref vs 50 digits: F {eF:.3e} N {eN:.3e} D_new {eD:.3e}; recorded {kat['ref_err']}")
    for q, e in (("F", eF), ("N", eN), ("D_new", eD)):
        assert e <= max(kat["ref_err"][q], 2.0 ** -52), q
        assert kat["ref_err"][q] < 1e-14


# ---- argument checks that need no device ---------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ibamr_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ibamr_amd import build
        build.build()
    return _lib.load()


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def test_set_rods_argument_errors_without_a_context(lib):
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    h = ctypes.c_void_p()
    assert lib.ibtk_le_rodgen_create(None, -1, ctypes.byref(h)) == 4
    assert lib.ibtk_le_rodgen_create(None, 5, None) == 4
    assert lib.ibtk_le_rodgen_create(None, 5, ctypes.byref(h)) == 0
    curr, nxt, par = _i([0, 1]), _i([1, 2]), np.ones((2, 10))

    def call(n, c, m, p, handle=h):
        rc = lib.ibtk_le_rodgen_set_rods(handle, n, None if c is None else ptr(c), None if m is None else ptr(m),
                                         None if p is None else ptr(p))
        return rc, lib.ibtk_le_last_error().decode()

    assert call(2, curr, nxt, par, handle=None)[0] == 4
    rc, msg = call(-1, curr, nxt, par)
    assert rc == 4 and "negative" in msg
    for args in ((None, nxt, par), (curr, None, par), (curr, nxt, None)):
        rc, msg = call(2, *args)
        assert rc == 4 and "null array" in msg
    rc, msg = call(2, _i([0, 5]), nxt, par)
    assert rc == 4 and "rod 1" in msg and "out of range" in msg
    rc, msg = call(2, curr, _i([1, -1]), par)
    assert rc == 4 and "next node index -1" in msg
    rc, msg = call(2, curr, _i([1, 1]), par)
    assert rc == 4 and "both node 1" in msg
    for bad in (np.nan, np.inf, -np.inf):
        p = par.copy()
        p[1, 8] = bad
        rc, msg = call(2, curr, nxt, p)
        assert rc == 4 and "kappa2" in msg and "not finite" in msg
    p = par.copy()
    p[0, 0] = 0.0  # ds == 0 passes validation, as the reference accepts it
    rc, msg = call(2, curr, nxt, p)
    assert rc == 4 and "without a context" in msg
    assert call(0, None, None, None)[0] == 0  # clearing needs no device
    ne = ctypes.c_longlong(-1)
    assert lib.ibtk_le_rodgen_plan_size(h, ctypes.byref(ne)) == 0 and ne.value == 0
    assert lib.ibtk_le_rodgen_compute(None, h, None, None, None, None, 1, 0) == 4
    assert lib.ibtk_le_rodgen_destroy(h) == 0


def test_director_update_refuses_midpoint(lib):
    assert lib.ibtk_le_director_update(None, 1, 10, 0.1, None, None, None, None) == 4
    assert "MIDPOINT" in lib.ibtk_le_last_error().decode()
    assert lib.ibtk_le_director_update(None, 7, 10, 0.1, None, None, None, None) == 4
    assert lib.ibtk_le_director_update(None, 0, 10, 0.1, None, None, None, None) == 4  # no context

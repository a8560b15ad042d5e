"""CPU: the .spring / .beam / .target deck readers and writers (ibamr_amd/io.py).

The fixtures under tests/golden/ibforce/ are the decks of IBAMR's explicit IB examples
(ex3/fila_256, ex2/sphere3d_32, ex1/curve2d_64); their .vertex twins sit under
tests/golden/vertex/.  Reader behaviour follows IBStandardInitializer::readSpringFiles,
readBeamFiles and readTargetPointFiles (IBStandardInitializer.cpp:803-1006, 1240-1405,
1740-1870).
"""
from pathlib import Path

import numpy as np
import pytest

from ibamr_amd import io

DECKS = Path(__file__).resolve().parent / "golden" / "ibforce"


def test_fila_spring_fixture():
    s = io.read_spring(DECKS / "fila_256.spring", 201)
    assert s.mastr.size == 200
    assert (s.mastr[0], s.slave[0], s.kappa[0], s.rest[0]) == (0, 1, 0.0, 1.4999999999999999e-02)
    assert (s.mastr[-1], s.slave[-1], s.kappa[-1], s.rest[-1]) == (199, 200, 0.0, 1.4999999999999999e-02)
    assert not s.fcn_idx.any() and all(e.size == 0 for e in s.extra)  # the trailing comment is no parameter
    assert s.mastr.dtype == np.int32 and s.kappa.dtype == np.float64


def test_fila_beam_fixture():
    b = io.read_beam(DECKS / "fila_256.beam", 201, ndim=2)
    assert b.mastr.size == 199
    assert (b.prev[0], b.mastr[0], b.next[0], b.bend[0]) == (0, 1, 2, 0.0)
    assert (b.prev[-1], b.mastr[-1], b.next[-1], b.bend[-1]) == (198, 199, 200, 0.0)
    assert b.curv.shape == (199, 2) and not b.curv.any()  # no curvature columns: the zero vector


def test_fila_target_fixture():
    t = io.read_target(DECKS / "fila_256.target", 201)
    assert t.node.tolist() == [0] and t.kappa.tolist() == [5.0e6] and t.eta.tolist() == [0.0]


def test_sphere_and_curve_spring_fixtures():
    s = io.read_spring(DECKS / "sphere3d_32.spring", 162)
    assert s.mastr.size == 480
    assert (s.mastr[0], s.slave[0], s.kappa[0], s.rest[0]) == (0, 42, 0.0, 1.379522421276337e-01)
    assert (s.mastr[-1], s.slave[-1], s.kappa[-1], s.rest[-1]) == (160, 161, 0.0, 1.624598481164531e-01)
    c = io.read_spring(DECKS / "curve2d_64.spring", 304)
    assert c.mastr.size == 304
    assert (c.mastr[0], c.slave[0], c.kappa[0], c.rest[0]) == (0, 1, 1.9353241079974475e+02, 0.0)
    # the last line reads "303 0": the edge is stored with its smaller index first
    assert (c.mastr[-1], c.slave[-1], c.kappa[-1]) == (0, 303, 1.9353241079974475e+02)


def test_reversed_edge_and_offset(tmp_path):
    p = tmp_path / "a.spring"
    p.write_text("2\n5 2 1.0 0.5  % reversed\n1 3 2.0 0.25 7 0.125 9.5 # fcn idx and two parameters\n")
    s = io.read_spring(p, 6)
    assert (s.mastr[0], s.slave[0]) == (2, 5)
    assert s.fcn_idx.tolist() == [0, 7] and s.extra[1].tolist() == [0.125, 9.5] and s.extra[0].size == 0
    s = io.read_spring(p, 6, vertex_offset=100)
    assert s.mastr.tolist() == [102, 101] and s.slave.tolist() == [105, 103]


def test_spring_overrides_and_length_scale():
    path = DECKS / "sphere3d_32.spring"
    base = io.read_spring(path, 162)
    s = io.read_spring(path, 162, length_scale=3.0)
    assert np.array_equal(s.rest, base.rest * 3.0) and np.array_equal(s.kappa, base.kappa)
    s = io.read_spring(path, 162, length_scale=3.0, uniform_stiffness=7.5, uniform_rest_length=0.125,
                       uniform_force_fcn_idx=2)
    assert np.all(s.kappa == 7.5) and np.all(s.rest == 0.125) and np.all(s.fcn_idx == 2)  # not scaled: :927 then :949


def test_beam_and_target_overrides(tmp_path):
    b = io.read_beam(DECKS / "fila_256.beam", 201, ndim=2, uniform_bend_rigidity=2.5, uniform_curvature=[0.5, -1.0])
    assert np.all(b.bend == 2.5) and np.all(b.curv == [0.5, -1.0])
    # a uniform target override sets every vertex of the structure (:1857-1870)
    t = io.read_target(DECKS / "fila_256.target", 201, uniform_target_damping=0.25)
    assert t.node.tolist() == list(range(201))
    assert t.kappa[0] == 5.0e6 and not t.kappa[1:].any() and np.all(t.eta == 0.25)
    t = io.read_target(DECKS / "fila_256.target", 201, uniform_target_stiffness=3.0)
    assert np.all(t.kappa == 3.0) and not t.eta.any() and t.node.size == 201
    p = tmp_path / "c.beam"
    p.write_text("2\n0 1 2 1.5 0.25 -0.5 3.0\n1 2 3 2.5 ! no curvature\n")
    b = io.read_beam(p, 4, ndim=3)
    assert b.curv.tolist() == [[0.25, -0.5, 3.0], [0.0, 0.0, 0.0]]
    p = tmp_path / "d.target"
    p.write_text("3\n2 4.0 0.5\n0 1.0 # no damping column\n2 8.0\n")
    t = io.read_target(p, 3)
    assert t.node.tolist() == [2, 0] and t.kappa.tolist() == [8.0, 1.0] and t.eta.tolist() == [0.0, 0.0]


def test_write_read_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    n, nv = 37, 50
    a, b = rng.integers(0, nv, n), rng.integers(0, nv, n)
    mastr, slave = np.minimum(a, b), np.maximum(a, b)
    kappa, rest = rng.random(n) * 1e3, rng.random(n) / 3.0
    io.write_spring(tmp_path / "r.spring", mastr, slave, kappa, rest)
    s = io.read_spring(tmp_path / "r.spring", nv)
    assert np.array_equal(s.mastr, mastr) and np.array_equal(s.slave, slave)
    assert np.array_equal(s.kappa, kappa) and np.array_equal(s.rest, rest) and not s.fcn_idx.any()
    fcn = rng.integers(0, 3, n)
    extra = [rng.random(k % 3) for k in range(n)]
    io.write_spring(tmp_path / "r2.spring", mastr, slave, kappa, rest, fcn, extra)
    s = io.read_spring(tmp_path / "r2.spring", nv)
    assert np.array_equal(s.fcn_idx, fcn) and all(np.array_equal(x, y) for x, y in zip(s.extra, extra))
    for ndim in (2, 3):
        m, nx, pv = (rng.integers(0, nv, n) for _ in range(3))
        bend, curv = rng.random(n), rng.standard_normal((n, ndim))
        io.write_beam(tmp_path / "r.beam", m, nx, pv, bend, curv)
        bd = io.read_beam(tmp_path / "r.beam", nv, ndim=ndim)
        assert np.array_equal(bd.mastr, m) and np.array_equal(bd.next, nx) and np.array_equal(bd.prev, pv)
        assert np.array_equal(bd.bend, bend) and np.array_equal(bd.curv, curv)
    node = rng.permutation(nv)[:n]
    tk, te = rng.random(n) * 1e6, rng.random(n)
    io.write_target(tmp_path / "r.target", node, tk, te)
    t = io.read_target(tmp_path / "r.target", nv)
    assert np.array_equal(t.node, node) and np.array_equal(t.kappa, tk) and np.array_equal(t.eta, te)
    io.write_target(tmp_path / "r0.target", node, tk)
    assert not io.read_target(tmp_path / "r0.target", nv).eta.any()


ERRORS = [
    ("spring", "2\n0 1 1.0 0.5\n", "Premature end to input file encountered before line 3"),
    ("spring", "", "Premature end to input file encountered before line 1"),
    ("spring", "x\n0 1 1.0 0.5\n0 1 1.0 0.5\n", "Invalid entry in input file encountered on line 1"),
    ("spring", "0\n0 1 1.0 0.5\n0 1 1.0 0.5\n", "Invalid entry in input file encountered on line 1"),
    ("spring", "2\n0 1 1.0 0.5\n0 1 oops 0.5\n", "Invalid entry in input file encountered on line 3"),
    ("spring", "2\n0 1 1.0 0.5\n0 1 1.0\n", "Invalid entry in input file encountered on line 3"),
    ("spring", "2\n0 1 1.0 0.5\n0 4 1.0 0.5\n", "line 3 of file {name}\n  vertex index 4 is out of range"),
    ("spring", "2\n-1 1 1.0 0.5\n0 1 1.0 0.5\n", "line 2 of file {name}\n  vertex index -1 is out of range"),
    ("spring", "2\n0 1 -1.0 0.5\n0 1 1.0 0.5\n", "line 2 of file {name}\n  spring constant is negative"),
    ("spring", "2\n0 1 1.0 0.5\n0 1 1.0 -0.5\n", "line 3 of file {name}\n  spring resting length is negative"),
    ("beam", "2\n0 1 2 1.0\n", "Premature end to input file encountered before line 3"),
    ("beam", "2\n0 1 2 1.0\n0 1 9 1.0\n", "line 3 of file {name}\n  vertex index 9 is out of range"),
    ("beam", "2\n0 1 2 -1.0\n0 1 2 1.0\n", "line 2 of file {name}\n  beam constant is negative"),
    ("beam", "2\n0 1 2 1.0\n0 1 2 1.0 0.5\n", "line 3 of file {name}\n  incomplete beam curvature specification"),
    ("beam", "2\n0 1 2\n0 1 2 1.0\n", "Invalid entry in input file encountered on line 2"),
    ("target", "2\n0 1.0\n", "Premature end to input file encountered before line 3"),
    ("target", "2\n0 1.0\n4 1.0\n", "line 3 of file {name}\n  vertex index 4 is out of range"),
    ("target", "2\n0 -1.0\n1 1.0\n", "line 2 of file {name}\n  target point spring constant is negative"),
    ("target", "2\n0 1.0\n1 1.0 -0.5\n", "line 3 of file {name}\n  target point damping coefficient is negative"),
    ("target", "2\n0\n1 1.0\n", "Invalid entry in input file encountered on line 2"),
]


@pytest.mark.parametrize("kind,text,message", ERRORS, ids=[f"{k}-{i}" for i, (k, _, _) in enumerate(ERRORS)])
def test_reader_errors(tmp_path, kind, text, message):
    p = tmp_path / f"bad.{kind}"
    p.write_text(text)
    read = {"spring": lambda: io.read_spring(p, 4), "beam": lambda: io.read_beam(p, 4, ndim=2),
            "target": lambda: io.read_target(p, 4)}[kind]
    with pytest.raises(ValueError) as e:
        read()
    assert message.format(name=p) in str(e.value)


def test_missing_file(tmp_path):
    for read in (io.read_spring, io.read_beam, io.read_target):
        with pytest.raises(FileNotFoundError):
            read(tmp_path / "nope", 4)

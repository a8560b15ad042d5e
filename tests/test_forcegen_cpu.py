"""CPU: the force specifications' flat arrays (ForceSpecs.arrays), known answers of the
serial restatement the GPU tests compare against (tests/forcegen_ref.py), and the force
generator ABI's argument errors that need no device."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from forcegen_ref import accumulate_forces, reference_force
from ibamr_amd import io
from ibamr_amd.forcegen import ForceSpecs

GOLDEN = Path(__file__).resolve().parent / "golden"


def _specs(tmp_path, spring_text=None, beam_text=None, target_text=None, nv=6, ndim=2):
    base = tmp_path / "s"
    io.write_vertex(f"{base}.vertex", np.arange(nv * ndim, dtype=np.float64).reshape(nv, ndim))
    for ext, text in (("spring", spring_text), ("beam", beam_text), ("target", target_text)):
        if text is not None:
            Path(f"{base}.{ext}").write_text(text)
    return ForceSpecs.from_files(base, ndim)


def test_arrays_stable_by_master_and_duplicate_edge(tmp_path):
    # deck order: masters 3, 0, 3 (reversed), 0 (a repeat of line 2's edge), 1, 0
    sp = _specs(tmp_path, "6\n3 4 1.0 0.1\n0 2 2.0 0.2\n5 3 3.0 0.3\n2 0 4.0 0.4\n1 2 5.0 0.5\n0 1 6.0 0.6\n")
    s = sp.arrays()["springs"]
    assert s.mastr.tolist() == [0, 0, 0, 1, 3, 3]
    assert s.slave.tolist() == [2, 2, 1, 2, 4, 5]          # deck order within master 0 and master 3
    assert s.kappa.tolist() == [2.0, 2.0, 6.0, 5.0, 1.0, 3.0]  # the repeated edge (0, 2) takes the first line's
    assert s.rest.tolist() == [0.2, 0.2, 0.6, 0.5, 0.1, 0.3]
    assert s.mastr.dtype == np.int32 and not s.fcn_idx.any()


def test_arrays_beams_targets_and_perm(tmp_path):
    sp = _specs(tmp_path, "3\n3 4 1.0 0.1\n0 2 2.0 0.2\n1 0 3.0 0.3\n",
                "3\n2 3 4 1.0\n0 1 2 2.0 0.5 0.25\n1 3 5 3.0\n", "2\n4 7.0 0.5\n1 9.0\n")
    a = sp.arrays()
    b, t = a["beams"], a["targets"]
    assert b.mastr.tolist() == [1, 3, 3] and b.next.tolist() == [2, 4, 5] and b.prev.tolist() == [0, 2, 1]
    assert b.bend.tolist() == [2.0, 1.0, 3.0] and b.curv.tolist() == [[0.5, 0.25], [0.0, 0.0], [0.0, 0.0]]
    assert t.node.tolist() == [1, 4] and t.kappa.tolist() == [9.0, 7.0] and t.eta.tolist() == [0.0, 0.5]
    assert t.X0.tolist() == [[2.0, 3.0], [8.0, 9.0]]  # the vertices' initial positions
    # perm[lagrangian] = local: the arrays follow the masters' local order, indices are local
    perm = np.array([5, 4, 3, 2, 1, 0])
    a = sp.arrays(perm)
    s, b, t = a["springs"], a["beams"], a["targets"]
    assert s.mastr.tolist() == [2, 5, 5] and s.slave.tolist() == [1, 3, 4] and s.kappa.tolist() == [1.0, 2.0, 3.0]
    assert b.mastr.tolist() == [2, 2, 4] and b.next.tolist() == [1, 0, 3] and b.bend.tolist() == [1.0, 3.0, 2.0]
    assert t.node.tolist() == [1, 4] and t.kappa.tolist() == [7.0, 9.0] and t.X0.tolist() == [[8.0, 9.0], [2.0, 3.0]]
    with pytest.raises(ValueError):
        sp.arrays(np.arange(5))


def test_from_files_fixture_and_concat(tmp_path):
    import shutil
    only_vertex = ForceSpecs.from_files(GOLDEN / "vertex" / "fila_256", 2)  # no decks beside this one
    assert only_vertex.num_vertex == 201 and only_vertex.arrays() == {"springs": None, "beams": None, "targets": None}
    for ext in ("spring", "beam", "target"):
        shutil.copy(GOLDEN / "ibforce" / f"fila_256.{ext}", tmp_path)
    shutil.copy(GOLDEN / "vertex" / "fila_256.vertex", tmp_path)
    one = ForceSpecs.from_files(tmp_path / "fila_256", 2, uniform_stiffness=2.0)
    assert one.num_vertex == 201 and one.springs.mastr.size == 200 and one.beams.mastr.size == 199
    assert one.targets.node.tolist() == [0]
    two = ForceSpecs.from_files(tmp_path / "fila_256", 2, vertex_offset=201, uniform_stiffness=3.0)
    both = ForceSpecs.concat([one, two])
    assert both.num_vertex == 402
    s = both.arrays()["springs"]
    assert s.mastr.size == 400 and s.mastr[200] == 201 and s.slave[-1] == 401
    assert np.all(s.kappa[:200] == 2.0) and np.all(s.kappa[200:] == 3.0)
    t = both.arrays()["targets"]
    assert t.node.tolist() == [0, 201] and np.array_equal(t.X0[0], t.X0[1])


def test_spring_known_answers():
    X = np.array([[0.0, 0.0, 1.0], [2.0, 0.0, 1.0]])
    F = accumulate_forces(2, 3, X, springs=([0], [1], [3.0], [1.0]))
    assert F.tolist() == [[3.0, 0.0, 0.0], [-3.0, 0.0, 0.0]]  # stretched by 1: kappa (R - L) = 3 towards each other
    X2 = np.array([[0.0, 3.0], [4.0, 0.0]])
    F = accumulate_forces(2, 2, X2, springs=([0], [1], [2.0], [0.0]))
    assert F.tolist() == [[8.0, -6.0], [-8.0, 6.0]]  # zero rest length: f = kappa D
    # coincident nodes: R < DBL_EPSILON, the spring is skipped (no 0/0)
    Xc = np.array([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0 + 1e-17]])
    F = accumulate_forces(3, 2, Xc, springs=([0, 0], [1, 2], [5.0, 5.0], [1.0, 1.0]))
    assert not F.any() and np.isfinite(F).all()


def test_beam_known_answers():
    X = np.array([[0.0, 0.0], [1.0, 0.5], [2.0, 1.0]])  # collinear, equally spaced
    assert not accumulate_forces(3, 2, X, beams=([1], [2], [0], [4.0], [[0.0, 0.0]])).any()
    # bent: D2X = (0 + 2) - 2*1 = 0 in x, (0 + 0) - 2*1 = -2 in y; f = K D2X = (0, -4)
    X = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 0.0]])
    F = accumulate_forces(3, 2, X, beams=([1], [2], [0], [2.0], [[0.0, 0.0]]))
    assert F.tolist() == [[0.0, 4.0], [0.0, -8.0], [0.0, 4.0]]
    # with curvature C = (0, -2) the bend is the rest shape
    assert not accumulate_forces(3, 2, X, beams=([1], [2], [0], [2.0], [[0.0, -2.0]])).any()


def test_target_known_answers_and_accumulate():
    X = np.array([[1.0, 2.0], [0.0, 0.0]])
    U = np.array([[0.5, -1.0], [9.0, 9.0]])
    tg = ([0], [4.0], [2.0], [[1.5, 1.0]])
    F = accumulate_forces(2, 2, X, targets=tg, U=U)
    assert F.tolist() == [[4.0 * 0.5 - 2.0 * 0.5, 4.0 * -1.0 - 2.0 * -1.0], [0.0, 0.0]]  # (1, -2)
    dX = np.array([[0.5, 0.0], [0.0, 0.0]])  # X + dX sits on the target in x
    assert accumulate_forces(2, 2, X, targets=tg, U=U, dX=dX)[0].tolist() == [-1.0, -2.0]
    F0 = np.array([[10.0, 20.0], [30.0, 40.0]])
    assert reference_force(2, 2, X, targets=tg, U=U, F=F0).tolist() == [[11.0, 18.0], [30.0, 40.0]]
    assert reference_force(2, 2, X, targets=tg, U=U, F=F0, accumulate=False).tolist() == [[1.0, -2.0], [0.0, 0.0]]


def test_forcegen_abi_argument_errors_without_device():
    from ibamr_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.ibtk_le_forcegen_create(None, 3, 10, ctypes.byref(out)) == 4
    assert b"null context" in lib.ibtk_le_last_error()
    idx = (ctypes.c_int * 2)(0, 1)
    val = (ctypes.c_double * 2)(1.0, 1.0)
    assert lib.ibtk_le_forcegen_set_springs(None, 1, idx, idx, val, val, None) == 4
    assert lib.ibtk_le_last_error().decode()
    assert lib.ibtk_le_forcegen_set_beams(None, 1, idx, idx, idx, val, None) == 4
    assert lib.ibtk_le_forcegen_set_targets(None, 1, idx, val, val, val) == 4
    assert lib.ibtk_le_forcegen_compute(None, None, None, None, None, None, 1) == 4
    assert lib.ibtk_le_forcegen_destroy(None) == 0

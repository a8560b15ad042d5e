"""CPU: the host side of the device plan rebuild (ibtk_le_forcespecs, ibtk_le_forcegen_renumber).

* ``ForceSpecs.lagrangian_arrays()`` -- the deck-order, Lagrangian-index arrays the device
  spec store uploads -- carried through a plain numpy restatement of the rebuild's first
  steps (perm = -1, perm[order[i]] = i, key = perm[master], stable sort) reproduces
  ``ForceSpecs.arrays(perm)`` field for field.
* ``ForceSpecs.arrays()`` returns what its formulae before the factoring returned (restated
  here with the per-spring ``dict`` loop).
* ``ibtk_le_forcespecs_set_*`` reject bad arguments with a status and a message before any
  device call (a store created without a context validates on a machine without a GPU).
"""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from ibamr_amd import io
from ibamr_amd.forcegen import ForceSpecs

GOLDEN = Path(__file__).resolve().parent / "golden"

DECKS = {
    "curve2d_64": (2, {}),
    "sphere3d_32": (3, {"uniform_stiffness": 37.5}),
    "fila_256": (2, {"uniform_stiffness": 1.0e4, "uniform_bend_rigidity": 0.375,
                     "uniform_curvature": [1.0e-5, -2.0e-5], "uniform_target_stiffness": 5.0e3,
                     "uniform_target_damping": 0.75}),
}


def _deck_specs(name):
    ndim, uniform = DECKS[name]
    X0 = io.read_vertex(GOLDEN / "vertex" / f"{name}.vertex", ndim)
    nv = X0.shape[0]
    d = GOLDEN / "ibforce"
    pick = lambda *keys: {k: uniform[k] for k in keys if k in uniform}  # noqa: E731
    springs = beams = targets = None
    if (d / f"{name}.spring").exists():
        springs = io.read_spring(d / f"{name}.spring", nv, **pick("uniform_stiffness", "uniform_rest_length"))
    if (d / f"{name}.beam").exists():
        beams = io.read_beam(d / f"{name}.beam", nv, ndim, **pick("uniform_bend_rigidity", "uniform_curvature"))
    if (d / f"{name}.target").exists():
        targets = io.read_target(d / f"{name}.target", nv,
                                 **pick("uniform_target_stiffness", "uniform_target_damping"))
    return ForceSpecs(ndim, X0, springs, beams, targets)


def _synthetic_specs():
    """The synthetic set of tests/test_gpu_forcegen.py as decks in Lagrangian indices: 1000
    vertices, 5000 springs (random ones, 49 repeated edges, a 300-spring hub on vertex 7 as
    master and as slave, a coincident pair), 200 beams, a target point on every third vertex
    below 950."""
    rng = np.random.default_rng(2024)
    n, nd, live = 1000, 3, 950
    X = rng.random((n, nd))
    X[21] = X[20]
    m = rng.integers(0, live, 4650)
    s = (m + rng.integers(1, live, 4650)) % live
    hub_other = rng.permutation(np.setdiff1d(np.arange(live), [7]))[:300]
    hub_m = np.where(np.arange(300) % 2 == 0, 7, hub_other)
    hub_s = np.where(np.arange(300) % 2 == 0, hub_other, 7)
    mastr = np.concatenate([m, m[:49], hub_m, [20]])
    slave = np.concatenate([s, s[:49], hub_s, [21]])
    o = rng.permutation(mastr.size)
    mastr, slave = mastr[o].astype(np.int32), slave[o].astype(np.int32)
    assert mastr.size == 5000 and not (mastr == slave).any()
    springs = io.SpringDeck(mastr, slave, rng.random(5000) * 100.0, rng.random(5000) * 0.5,
                            np.zeros(5000, dtype=np.int32), [np.empty(0)] * 5000)
    bm = rng.integers(0, live, 200)
    bn = (bm + rng.integers(1, live, 200)) % live
    bp = (bm + rng.integers(1, live, 200)) % live
    beams = io.BeamDeck(bm.astype(np.int32), bn.astype(np.int32), bp.astype(np.int32), rng.random(200) * 10.0,
                        rng.standard_normal((200, nd)) * 0.1)
    node = np.arange(0, live, 3, dtype=np.int32)
    targets = io.TargetDeck(node, rng.random(node.size) * 50.0, rng.random(node.size))
    return ForceSpecs(nd, X, springs, beams, targets)


SETS = ["synthetic", *DECKS]


@pytest.fixture(scope="module")
def specs():
    return {"synthetic": _synthetic_specs(), **{name: _deck_specs(name) for name in DECKS}}


def _arrays_before_factoring(sp, perm):
    """ForceSpecs.arrays(perm) as it was written before lagrangian_arrays() was factored out
    of it, the per-spring dict loop included."""
    perm = np.asarray(perm, dtype=np.int64)
    out = {"springs": None, "beams": None, "targets": None}
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    if sp.springs is not None:
        s = sp.springs
        m = np.minimum(s.mastr, s.slave).astype(np.int64)
        v = np.maximum(s.mastr, s.slave).astype(np.int64)
        first = {}
        src = np.empty(m.size, dtype=np.int64)
        for k, e in enumerate(zip(m.tolist(), v.tolist())):
            src[k] = first.setdefault(e, k)
        o = np.argsort(perm[m], kind="stable")
        out["springs"] = (i32(perm[m][o]), i32(perm[v][o]), s.kappa[src][o], s.rest[src][o], i32(s.fcn_idx[src][o]))
    if sp.beams is not None:
        b = sp.beams
        o = np.argsort(perm[b.mastr.astype(np.int64)], kind="stable")
        out["beams"] = (i32(perm[b.mastr][o]), i32(perm[b.next][o]), i32(perm[b.prev][o]), b.bend[o],
                        np.asarray(b.curv[o], dtype=np.float64).reshape(-1, sp.ndim))
    if sp.targets is not None:
        t = sp.targets
        o = np.argsort(perm[t.node.astype(np.int64)], kind="stable")
        out["targets"] = (i32(perm[t.node][o]), t.kappa[o], t.eta[o], sp.X0[t.node[o]].reshape(-1, sp.ndim))
    return out


def _same(got, want, what):
    assert (got is None) == (want is None), what
    if got is None:
        return
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, f)


def _perms(nv, seed):
    yield "identity", np.arange(nv)
    yield "random", np.random.default_rng(seed).permutation(nv)


@pytest.mark.parametrize("name", SETS)
def test_arrays_output_is_unchanged(specs, name):
    sp = specs[name]
    for pname, perm in _perms(sp.num_vertex, 11):
        got, want = sp.arrays(perm), _arrays_before_factoring(sp, perm)
        for c in ("springs", "beams", "targets"):
            _same(got[c], want[c], f"{name} {pname} {c}")
    # arrays() with no perm is the identity
    got, want = sp.arrays(), _arrays_before_factoring(sp, np.arange(sp.num_vertex))
    for c in ("springs", "beams", "targets"):
        _same(got[c], want[c], f"{name} None {c}")
    if name == "synthetic":  # the repeated edges do carry their first line's parameters
        a = sp.arrays()["springs"]
        e = a.mastr.astype(np.int64) * 1000 + a.slave
        _, inv, cnt = np.unique(e, return_inverse=True, return_counts=True)
        rep = cnt[inv] > 1
        assert rep.sum() >= 98
        for key in np.unique(e[rep]):
            assert np.unique(a.kappa[e == key]).size == 1 and np.unique(a.rest[e == key]).size == 1


def _restated_rebuild(lag, order, nv):
    """Steps 1-3 of the device rebuild in numpy, on the deck-order Lagrangian arrays: perm = -1,
    perm[order[i]] = i, the deck sorted stably by perm[master], every index through perm."""
    perm = np.full(nv, -1, dtype=np.int64)
    perm[order] = np.arange(order.size)
    out = {}
    for c, nidx in (("springs", 2), ("beams", 3), ("targets", 1)):
        a = lag[c]
        if a is None:
            out[c] = None
            continue
        key = perm[a[0]]
        o = np.argsort(key, kind="stable")
        out[c] = tuple(np.ascontiguousarray(perm[f][o], dtype=np.int32) if q < nidx else f[o] for q, f in enumerate(a))
    return out


@pytest.mark.parametrize("name", SETS)
def test_lagrangian_arrays_rebuild_matches_arrays(specs, name):
    sp = specs[name]
    nv = sp.num_vertex
    lag = sp.lagrangian_arrays()
    for c, deck in (("springs", sp.springs), ("beams", sp.beams), ("targets", sp.targets)):
        assert (lag[c] is None) == (deck is None)
    if sp.springs is not None:
        s = lag["springs"]
        assert (s.mastr < s.slave).all()  # the master is the smaller Lagrangian index
        assert np.array_equal(s.mastr, np.minimum(sp.springs.mastr, sp.springs.slave))  # deck order
        assert s.mastr.dtype == np.int32 and s.kappa.dtype == np.float64
    if sp.targets is not None:
        assert np.array_equal(lag["targets"].X0, sp.X0[sp.targets.node])
    for seed in (3, 4):
        perm = np.random.default_rng(seed).permutation(nv)
        order = np.argsort(perm)  # order[i] = the Lagrangian index of node i
        got, want = _restated_rebuild(lag, order, nv), sp.arrays(perm)
        for c in ("springs", "beams", "targets"):
            _same(got[c], want[c], f"{name} seed {seed} {c}")


@pytest.fixture(scope="module")
def lib():
    from ibamr_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ibamr_amd import build
        build.build()
    return _lib.load()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_forcespecs_argument_errors_before_any_device_call(lib):
    def err(rc, word):
        assert rc == 4, rc  # IBTK_LE_ERR_ARG
        msg = lib.ibtk_le_last_error().decode()
        assert word in msg, msg

    h = ctypes.c_void_p()
    err(lib.ibtk_le_forcespecs_create(None, 4, 10, ctypes.byref(h)), "ndim")
    err(lib.ibtk_le_forcespecs_create(None, 3, -1, ctypes.byref(h)), "negative")
    err(lib.ibtk_le_forcespecs_create(None, 3, 10, None), "null out")
    # a store without a context: the host checks run, nothing can reach a device
    assert lib.ibtk_le_forcespecs_create(None, 3, 10, ctypes.byref(h)) == 0
    i = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    one, x0 = np.ones(1), np.zeros((1, 3))
    try:
        err(lib.ibtk_le_forcespecs_set_springs(None, 1, _p(i(0)), _p(i(1)), _p(one), _p(one), None), "null spec store")
        err(lib.ibtk_le_forcespecs_set_springs(h, 1, None, _p(i(1)), _p(one), _p(one), None), "null array")
        err(lib.ibtk_le_forcespecs_set_springs(h, 1, _p(i(0)), _p(i(1)), None, _p(one), None), "null array")
        err(lib.ibtk_le_forcespecs_set_beams(h, 1, _p(i(0)), None, _p(i(2)), _p(one), None), "null array")
        err(lib.ibtk_le_forcespecs_set_targets(h, 1, _p(i(0)), _p(one), _p(one), None), "null array")
        err(lib.ibtk_le_forcespecs_set_springs(h, -1, None, None, None, None, None), "negative")
        err(lib.ibtk_le_forcespecs_set_beams(h, -2, None, None, None, None, None), "negative")
        err(lib.ibtk_le_forcespecs_set_targets(h, -3, None, None, None, None), "negative")
        err(lib.ibtk_le_forcespecs_set_springs(h, 1, _p(i(0)), _p(i(10)), _p(one), _p(one), None), "out of range")
        err(lib.ibtk_le_forcespecs_set_springs(h, 1, _p(i(-1)), _p(i(1)), _p(one), _p(one), None), "out of range")
        err(lib.ibtk_le_forcespecs_set_beams(h, 1, _p(i(3)), _p(i(4)), _p(i(10)), _p(one), None), "out of range")
        err(lib.ibtk_le_forcespecs_set_targets(h, 1, _p(i(10)), _p(one), _p(one), _p(x0)), "out of range")
        err(lib.ibtk_le_forcespecs_set_springs(h, 1, _p(i(4)), _p(i(4)), _p(one), _p(one), None), "master and slave")
        err(lib.ibtk_le_forcespecs_set_beams(h, 1, _p(i(3)), _p(i(3)), _p(i(2)), _p(one), None), "master and next")
        err(lib.ibtk_le_forcespecs_set_beams(h, 1, _p(i(3)), _p(i(4)), _p(i(3)), _p(one), None), "master and prev")
        err(lib.ibtk_le_forcespecs_set_springs(h, 1, _p(i(0)), _p(i(1)), _p(one), _p(one), _p(i(1))), "Hookean")
        # the second spring of two is the one named
        err(lib.ibtk_le_forcespecs_set_springs(h, 2, _p(i(0, 5)), _p(i(1, 5)), _p(np.ones(2)), _p(np.ones(2)), None),
            "spring 1")
        # valid arguments: this store has no device to upload to, and says so
        err(lib.ibtk_le_forcespecs_set_springs(h, 1, _p(i(0)), _p(i(1)), _p(one), _p(one), _p(i(0))),
            "without a context")
        assert lib.ibtk_le_forcespecs_set_springs(h, 0, None, None, None, None, None) == 0  # clearing needs none
    finally:
        assert lib.ibtk_le_forcespecs_destroy(h) == 0
    # the plan-side calls reject null handles the same way
    n = ctypes.c_longlong()
    err(lib.ibtk_le_forcegen_renumber(None, None, None, None, 0), "null context")
    err(lib.ibtk_le_forcegen_plan_size(None, 0, ctypes.byref(n)), "null")
    err(lib.ibtk_le_forcegen_plan_read(None, 0, None, None, 0), "null")
    err(lib.ibtk_le_forcegen_renumber_stats(None, None), "null")
    assert lib.ibtk_le_forcespecs_destroy(None) == 0


def test_new_symbols_are_declared():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "ibtk_le.h").read_text()
    for name in ("ibtk_le_forcespecs_create", "ibtk_le_forcespecs_destroy", "ibtk_le_forcespecs_set_springs",
                 "ibtk_le_forcespecs_set_beams", "ibtk_le_forcespecs_set_targets", "ibtk_le_forcegen_renumber",
                 "ibtk_le_forcegen_plan_size", "ibtk_le_forcegen_plan_read"):
        assert name + "(" in hdr, name

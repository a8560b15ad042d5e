"""The numpy restatement of the slab migration kernels (tests/slab_ref.py) and its edge set.

tests/test_gpu_slab_migrate.py compares the kernels with slab_ref bit for bit.  Here, without
a GPU, slab_ref's wrap and owner are held to the torch formula of ibamr_amd.slab.migrate
(remainder, where, clamp) -- the two were written from the same description, torch's is the
one the multi-rank path has always used -- and the edge set is checked to hold what the GPU
test relies on: the edge values themselves, every class in several blocks, waves with
several classes.
"""
import numpy as np
import pytest

import slab_ref as sr

torch = pytest.importorskip("torch")

LS = [(1.0, 1.0, 1.0), (2.0, 0.75, 1.5)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def torch_wrap_owner(X, L, Nz, P):
    """ibamr_amd.slab.migrate's wrap and destination rank, on CPU tensors."""
    Xt = torch.from_numpy(X)
    Lt = torch.tensor(list(L), dtype=torch.float64)
    Xw = torch.remainder(Xt, Lt)
    Xw = torch.where(Xw >= Lt, Xw - Lt, Xw)
    dz = L[2] / Nz
    cell = torch.clamp((Xw[:, 2] / dz).floor().long(), 0, Nz - 1)
    return Xw.numpy(), (cell // (Nz // P)).numpy()


@pytest.mark.parametrize("L", LS, ids=["unit", "box"])
@pytest.mark.parametrize("Nz,P", [(n, p) for n in (48, 64) for p in (1, 2, 3, 4, 8) if n % p == 0])
def test_wrap_and_owner_are_torchs(L, Nz, P):
    X, U0, U1, dt = sr.edge_rows(L, Nz, P, 70001, seed=5)
    for scheme in ("euler", "trapezoidal"):
        Xu = sr.update(scheme, dt, X, U0, U1)
        w = sr.wrap(Xu, np.array(L))
        wt, ot = torch_wrap_owner(Xu, L, Nz, P)
        assert np.array_equal(bits(w), bits(wt)), "the wrap, bit for bit (the sign of zero too)"
        assert np.array_equal(sr.owner(w[:, 2], L[2], Nz, P), ot)
        assert ((w >= 0.0) & (w < np.array(L))).all()
        assert set(np.unique(ot)) == set(range(P))


@pytest.mark.parametrize("L", LS, ids=["unit", "box"])
def test_edge_rows_hold_the_edges(L):
    """The edge rows come through the update unchanged, bit for bit, under both schemes; they
    hold a -0.0, the box length, its neighbours, a subnormal and every slab face per dim."""
    Nz, P = 48, 4
    X, U0, U1, dt = sr.edge_rows(L, Nz, P, 1000, seed=5)
    ne = sr.edge_count(Nz, P)
    at = np.arange(ne) * 3
    La = np.array(L)
    for scheme in ("euler", "trapezoidal"):
        assert np.array_equal(bits(sr.update(scheme, dt, X, U0, U1)[at]), bits(X[at]))
    moved = np.setdiff1d(np.arange(1000), at)
    assert (sr.update("euler", dt, X, U0, U1)[moved] != X[moved]).all()
    for d in range(3):
        col = X[at, d]
        for v in sr.edge_values(La[d]):
            assert (bits(col) == bits(np.array([v]))[0]).any(), (d, v)
    for v in sr.face_values(La[2], Nz, P):
        assert (X[at, 2] == v).any()
    w = sr.wrap(X[at], La)
    assert ((w >= 0.0) & (w < La)).all()
    # the wrap's branches: a result of -0.0, a tiny negative that rounds to L and comes back as 0
    assert np.signbit(w[w == 0.0]).any() and (sr.wrap(np.array([-5e-324]), 1.0) == 0.0).all()
    assert sr.wrap(np.array([np.nextafter(La[2], np.inf)]), La[2])[0] > 0.0
    # a face's lower neighbour belongs to the slab below unless the division rounds it up
    f = sr.face_values(La[2], Nz, P)[1:P]
    assert (sr.owner(f, La[2], Nz, P) == np.arange(1, P)).all()


@pytest.mark.parametrize("M", [1000, 70001])
@pytest.mark.parametrize("scheme", ["euler", "trapezoidal"])
def test_classes_mix_within_blocks_and_waves(M, scheme):
    """P = 4, rank 1: all four classes, each in at least two 256-row blocks, a block with all
    four and a 64-row wave with at least three -- the partition's block offsets and its
    in-wave ranks all do work.  P = 2: the one neighbour is class 1, class 2 is empty."""
    L, Nz = LS[1], 48
    X, U0, U1, dt = sr.edge_rows(L, Nz, 4, M, seed=7)
    Xn, order, counts, cls = sr.update_partition(scheme, dt, X, U0, L, Nz, 4, 1, U1=U1)
    assert (counts > 0).all() and counts.sum() == M
    nb = -(-M // sr.BLOCK)
    per_block = np.zeros((nb, 4), int)
    np.add.at(per_block, (np.arange(M) // sr.BLOCK, cls), 1)
    assert ((per_block > 0).sum(axis=0) >= 2).all()
    assert (per_block > 0).all(axis=1).any()
    per_wave = np.zeros((-(-M // sr.WAVE), 4), int)
    np.add.at(per_wave, (np.arange(M) // sr.WAVE, cls), 1)
    assert ((per_wave > 0).sum(axis=1) >= 3).any()
    # the partition is stable and complete
    assert np.array_equal(np.sort(order), np.arange(M))
    assert (np.diff(cls[order]) >= 0).all()
    for k in range(4):
        assert (np.diff(order[cls[order] == k]) > 0).all()
    _, _, c2, cls2 = sr.update_partition(scheme, dt, X, U0, L, Nz, 2, 1, U1=U1)
    assert c2[2] == 0 and c2[3] == 0 and c2[1] > 0 and c2[0] > 0
    _, o1, c1, _ = sr.update_partition(scheme, dt, X, U0, L, Nz, 1, 0, U1=U1)
    assert c1.tolist() == [M, 0, 0, 0] and np.array_equal(o1, np.arange(M))


def test_pack_and_unpack_restate_the_docstrings():
    rows = np.arange(40.0).reshape(10, 4)
    cls = np.array([0, 1, 2, 0, 1, 1, 0, 2, 0, 0])
    order, counts = sr.partition(cls)
    down, up = sr.pack(rows, order, counts)
    assert down[:, 0].tolist() == [4.0, 16.0, 20.0] and up[:, 0].tolist() == [8.0, 28.0]
    out = sr.unpack(rows, order, counts, up, down)
    assert out[:, 0].tolist() == [0.0, 12.0, 24.0, 32.0, 36.0, 8.0, 28.0, 4.0, 16.0, 20.0]


def test_step_rows_cross_one_face_at_most():
    for P in (2, 3, 4, 8):
        L, Nz = LS[1], 48
        crossed = 0
        for rank in range(P):
            X, U0, dt, F, ids = sr.step_rows(L, Nz, P, rank, 5003, seed=11)
            assert (sr.owner(sr.wrap(X[:, 2], L[2]), L[2], Nz, P) == rank).all()
            _, _, counts, _ = sr.update_partition("euler", dt, X, U0, L, Nz, P, rank)
            assert counts[3] == 0 and counts[1] > 0 and (counts[2] > 0 or P == 2)
            crossed += counts[1] + counts[2]
        assert 0.07 < crossed / (P * 5003) < 0.13

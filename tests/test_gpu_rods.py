"""GPU: Kirchhoff rods on the device (ibtk_le_rodgen_*, ibtk_le_director_update,
ibamr_amd.rods) against the 50-digit known answers of tests/golden/rod_kat.json and the
numpy restatement tests/rod_ref.py.

Tolerances.  tol_q = 8 * max(ref_err_q, 2^-52) per quantity q (F, N, D_new), ref_err_q the
recorded error of rod_ref against the 50-digit values; the factor 8 covers another root
algorithm (Denman-Beavers on the device, Eigen's Schur route in the reference, numpy's eig
in rod_ref) and another product and sum order.  Against the known answers the measure is
the file's own, max|v - v_kat| / max|v_kat| <= tol_q.  Against rod_ref on the larger inputs
(open chains, the hub graph, the director updates) both sides err: max|v - v_ref| /
max|v_ref| <= 2 tol_q.

The two ex4 cases alone take another denominator, max(max|v_ref|, S_q), with S_q the size
of the operands of the rod law's last subtractions,

    S_F = max_k (b1 + b2 + b3) max(|dX| / ds, 1)
    S_N = max_k (a1 + a2 + a3) (max_i |dD_i| / ds + max(|kappa1|, |kappa2|, |tau|)) + |dX| S_F,k / 2

because the ex4 ring sits at rest.  F3 = b3 (D3_half . dX/ds - 1) carries the rounding of
D3_half . dX/ds, eps times a number near 1, whatever is left after the 1 is taken off, and
on the ring what is left is 4e-5: F_half is 1e-3 of b3 and every node's F the difference of
two nearly equal F_half, max|F| = 6.6e-5 against S_F = 162.  Two correctly rounded float64
evaluations of that state (rod_ref with its eig root and with a Denman-Beavers root) differ
by 8e-10 of max|F|: that figure measures the cancellation in the input, not the kernel.
Relative to S_q the same bound 2 tol_q holds, and a swapped parameter, role or director
index is still an error of order S_q.
"""
import json
import math
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from rod_ref import reference_director_update, reference_rods  # noqa: E402
from ibamr_amd import io  # noqa: E402
from ibamr_amd.rods import RodSpecs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
EPS = float(np.finfo(np.float64).eps)


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
def rods(le):
    from ibamr_amd import rods as _rods
    return _rods


@pytest.fixture(scope="module")
def kat():
    return json.loads((GOLDEN / "rod_kat.json").read_text())


@pytest.fixture(scope="module")
def tol(kat):
    return {q: 8.0 * max(kat["ref_err"][q], 2.0 ** -52) for q in ("F", "N", "D_new")}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _view(a):
    """`a` on the device as a view 8 bytes into its buffer."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def _rot(axis, th):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _scales(X, D, curr, nxt, params):
    X, D, p = np.asarray(X), np.asarray(D).reshape(-1, 3, 3), np.asarray(params)
    curr, nxt = np.asarray(curr), np.asarray(nxt)
    if curr.size == 0:
        return 1.0, 1.0
    dX = np.linalg.norm(X[nxt] - X[curr], axis=1)
    ds = p[:, 0]
    sF = p[:, 4:7].sum(1) * np.maximum(dX / ds, 1.0)
    dD = np.linalg.norm(D[nxt] - D[curr], axis=2).max(1)
    sN = p[:, 1:4].sum(1) * (dD / ds + np.abs(p[:, 7:10]).max(1)) + 0.5 * dX * sF
    return float(sF.max()), float(sN.max())


def _check(got_F, got_N, ref_F, ref_N, tol, what, scales=(0.0, 0.0), factor=2.0):
    """Device against rod_ref, max|v - v_ref| / max|v_ref| <= factor tol_q; `scales` (the
    ex4 cases only, see the module's text) widens the denominator to max(max|v_ref|, S_q)."""
    eF = np.abs(got_F - ref_F).max() / max(np.abs(ref_F).max(), scales[0])
    eN = np.abs(got_N - ref_N).max() / max(np.abs(ref_N).max(), scales[1])
    print(f"{what}: device vs rod_ref F {eF:.3e} (bound {factor * tol['F']:.3e}), N {eN:.3e} "
          f"(bound {factor * tol['N']:.3e}); max|F| {np.abs(ref_F).max():.3e} S_F {scales[0]:.3e} "
          f"max|N| {np.abs(ref_N).max():.3e} S_N {scales[1]:.3e}")
    assert eF <= factor * tol["F"], what
    assert eN <= factor * tol["N"], what


def _structure(rng, n_nodes, curr, nxt):
    """Positions on a stretched helix, triads turning 0.1-0.4 rad from node to node and
    drifted by 1e-3, random positive parameters with non-zero curvatures; ds makes every
    rod's stretch |dX| / ds 1.05-1.3."""
    T = np.empty((n_nodes, 3, 3))
    T[0] = _rot(rng.normal(size=3), rng.uniform(0, 3))
    for i in range(1, n_nodes):
        T[i] = T[i - 1] @ _rot(rng.normal(size=3), rng.uniform(0.1, 0.4)).T
    D = (T + 1e-3 * rng.normal(size=T.shape)).reshape(n_nodes, 9)
    s = np.arange(n_nodes) * 0.05
    X = np.stack([np.cos(s), np.sin(s), 0.3 * s], axis=1) + 0.01 * rng.normal(size=(n_nodes, 3))
    curr, nxt = np.asarray(curr, dtype=np.int32), np.asarray(nxt, dtype=np.int32)
    n = curr.size
    params = np.empty((n, 10))
    if n:
        params[:, 0] = np.linalg.norm(X[nxt] - X[curr], axis=1) / rng.uniform(1.05, 1.3, size=n)
        params[:, 1:7] = rng.uniform(0.5, 2.0, size=(n, 6))
        params[:, 7:10] = rng.uniform(0.1, 1.0, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))
    return X, D, curr, nxt, params


def _compute(ctx, rods, n_nodes, X, D, curr, nxt, params, **kw):
    rg = rods.RodForceGen(ctx, n_nodes, (curr, nxt, params))
    F, N = rg.compute(_dev(X), _dev(D), **kw)
    ctx.synchronize()
    rg.close()
    return F.cpu().numpy(), N.cpu().numpy()


# ---- known answers -------------------------------------------------------------------

def test_known_answers_rods(ctx, rods, kat, tol):
    r = kat["rods"]
    F, N = _compute(ctx, rods, r["n_nodes"], r["X"], r["D"], r["curr"], r["next"], np.array(r["params"]))
    Fk, Nk = np.array(r["F"]), np.array(r["N"])
    eF = np.abs(F - Fk).max() / np.abs(Fk).max()
    eN = np.abs(N - Nk).max() / np.abs(Nk).max()
    print(f"device vs 50 digits: F {eF:.3e} (tol {tol['F']:.3e}, rod_ref {kat['ref_err']['F']:.3e}), "
          f"N {eN:.3e} (tol {tol['N']:.3e}, rod_ref {kat['ref_err']['N']:.3e})")
    assert eF <= tol["F"] and eN <= tol["N"]


def test_known_answers_directors(ctx, rods, kat, tol):
    d = kat["directors"]
    D, W0, W1 = _dev(d["D"]), _dev(d["W0"]), _dev(d["W1"])
    for scheme, key in (("euler", "D_euler"), ("trapezoidal", "D_trapezoidal")):
        got = rods.director_update(ctx, scheme, d["dt"], D, W0, W1).cpu().numpy()
        ref = np.array(d[key])
        e = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"director update {scheme}: device vs 50 digits {e:.3e} (tol {tol['D_new']:.3e}, "
              f"rod_ref {kat['ref_err']['D_new']:.3e})")
        assert e <= tol["D_new"], scheme


# ---- exact cases ---------------------------------------------------------------------

def test_straight_untwisted_rod_is_force_free(ctx, rods):
    n = 17
    X = np.zeros((n, 3))
    X[:, 2] = np.arange(n) / 16.0
    D = np.tile(np.eye(3).reshape(9), (n, 1))
    params = np.zeros((n - 1, 10))
    params[:, 0] = 1.0 / 16.0
    params[:, 1:7] = [0.3, 0.4, 0.2, 54.0, 27.0, 13.0]
    F, N = _compute(ctx, rods, n, X, D, np.arange(n - 1), np.arange(1, n), params)
    assert np.all(F == 0.0) and np.all(N == 0.0)  # sqrt(I) is I exactly


def test_one_rod_equal_and_opposite(ctx, rods):
    rng = np.random.default_rng(11)
    X, D, curr, nxt, params = _structure(rng, 2, [1], [0])
    F, N = _compute(ctx, rods, 2, X, D, curr, nxt, params)
    assert np.abs(F[0]).min() > 0.0
    assert np.array_equal(F[0].view(np.int64), (-F[1]).view(np.int64))


def test_pure_twist_closed_form(ctx, rods, tol):
    phi, ds, a3, tau = 0.7, 1.0 / 16.0, 0.2, 0.05
    X = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, ds]])
    D1 = (_rot([0, 0, 1.0], phi) @ np.eye(3).T).T  # rows: the triad turned by phi about D3
    D = np.stack([np.eye(3).reshape(9), D1.reshape(9)])
    params = np.array([[ds, 0.3, 0.4, a3, 54.0, 27.0, 13.0, 0.0, 0.0, tau]])
    F, N = _compute(ctx, rods, 2, X, D, [0], [1], params)
    closed = a3 * (2.0 * np.sin(phi / 2.0) / ds - tau)
    print(f"pure twist: N.D3 {N[0, 2]!r} closed form {closed!r} rel {abs(N[0, 2] - closed) / closed:.3e}")
    assert abs(N[0, 2] - closed) <= tol["N"] * abs(closed)
    assert abs(N[1, 2] + closed) <= tol["N"] * abs(closed)


# ---- sizes where the launch can go wrong -----------------------------------------------

@pytest.mark.parametrize("n_nodes", [2, 255, 256, 257, 1000])
def test_open_chains(ctx, rods, tol, n_nodes):
    rng = np.random.default_rng(n_nodes)
    X, D, curr, nxt, params = _structure(rng, n_nodes, np.arange(n_nodes - 1), np.arange(1, n_nodes))
    ref = reference_rods(n_nodes, X, D, curr, nxt, params)
    got = _compute(ctx, rods, n_nodes, X, D, curr, nxt, params)
    _check(*got, *ref, tol, f"chain of {n_nodes}")


def test_one_node_no_rods(ctx, rods):
    rg = rods.RodForceGen(ctx, 1)
    X, D = _dev(np.ones((1, 3))), _dev(np.eye(3).reshape(1, 9))
    F0 = _dev(np.full((1, 3), 2.5))
    F, N = rg.compute(X, D, F=F0)
    ctx.synchronize()
    assert F is F0 and np.array_equal(F.cpu().numpy(), np.full((1, 3), 2.5)) and np.all(N.cpu().numpy() == 0.0)
    assert rg.plan()[0].tolist() == [0, 0] and rg.plan()[1].size == 0


@pytest.fixture(scope="module")
def ex4():
    X = io.read_vertex(GOLDEN / "vertex" / "curve3d_64.vertex", 3)
    return X, RodSpecs.from_files(GOLDEN / "ibforce" / "curve3d_64", num_vertex=X.shape[0])


def test_ex4_ring_deck_to_device(ctx, rods, tol, ex4):
    """RodForceGen.from_specs on the ex4 decks at the deck's own X and D."""
    X, sp = ex4
    a = sp.arrays()
    assert sp.num_vertex == 200 and a.curr.size == 200
    ref = reference_rods(200, X, sp.directors, a.curr, a.next, a.params)
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[1]).max() > 0
    rg = rods.RodForceGen.from_specs(ctx, sp)
    F, N = rg.compute(_dev(X), _dev(sp.directors))
    ctx.synchronize()
    _check(F.cpu().numpy(), N.cpu().numpy(), *ref, tol, "ex4 ring",
           scales=_scales(X, sp.directors, a.curr, a.next, a.params))


def test_ex4_ring_renumbered(ctx, rods, tol, ex4):
    """The ring in a random numbering: RodSpecs.arrays(perm) + set_rods, the regrid route."""
    X, sp = ex4
    perm = np.random.default_rng(4).permutation(200)
    a = sp.arrays(perm)
    Xp, Dp = np.empty_like(X), np.empty_like(sp.directors)
    Xp[perm], Dp[perm] = X, sp.directors
    ref = reference_rods(200, Xp, Dp, a.curr, a.next, a.params)
    rg = rods.RodForceGen.from_specs(ctx, sp, perm=perm)
    F, N = rg.compute(_dev(Xp), _dev(Dp))
    ctx.synchronize()
    _check(F.cpu().numpy(), N.cpu().numpy(), *ref, tol, "ex4 renumbered",
           scales=_scales(Xp, Dp, a.curr, a.next, a.params))


@pytest.fixture(scope="module")
def graph():
    """300 nodes, 500 rods: node 7 a hub of 40 rods (20 as curr, 20 as next, its partners
    the 12 nodes within 6 of it, so several rods join one pair), 30 further repeated edges,
    both orientations, nodes 280.. rodless.  Rods join nodes at most 6 apart along the
    helix, whose triads are then at most 2.4 rad apart."""
    rng = np.random.default_rng(99)
    n_nodes = 300
    partners = [1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13]
    curr = [7] * 20 + [partners[j % 12] for j in range(20)]
    nxt = [partners[(5 * j) % 12] for j in range(20)] + [7] * 20
    while len(curr) < 470:
        a, b = (int(v) for v in rng.integers(0, 280, size=2))
        if a != b and abs(a - b) <= 6 and 7 not in (a, b):
            curr.append(a)
            nxt.append(b)
    for k in range(440, 470):
        curr.append(curr[k])
        nxt.append(nxt[k])
    order = rng.permutation(500)
    curr, nxt = np.array(curr)[order], np.array(nxt)[order]
    X, D, curr, nxt, params = _structure(rng, n_nodes, curr, nxt)
    assert (curr > nxt).any() and (curr < nxt).any()
    return n_nodes, X, D, curr, nxt, params


def test_graph_with_hub(ctx, rods, tol, graph):
    n_nodes, X, D, curr, nxt, params = graph
    ref = reference_rods(n_nodes, X, D, curr, nxt, params)
    F, N = _compute(ctx, rods, n_nodes, X, D, curr, nxt, params)
    _check(F, N, *ref, tol, "graph")
    assert np.all(F[280:] == 0.0) and np.all(N[280:] == 0.0)
    # the invariants: total force and total torque vanish
    fsum = lambda A: np.array([math.fsum(A[:, d]) for d in range(3)])  # noqa: E731  (exact sums)
    sF = np.abs(fsum(F)).max() / np.abs(F).sum()
    M = N + np.cross(X, F)
    sM = np.abs(fsum(M)).max() / (np.abs(N).sum() + np.abs(np.cross(X, F)).sum())
    print(f"sum F / sum|F| {sF:.3e}, sum (N + X x F) / sum of magnitudes {sM:.3e}")
    assert sF <= tol["F"] and sM <= tol["N"]


def test_plan_read_back(ctx, rods, graph):
    n_nodes, X, D, curr, nxt, params = graph
    rg = rods.RodForceGen(ctx, n_nodes, (curr, nxt, params))
    off, rec = rg.plan()
    assert rec.dtype.itemsize == 88 and rec.size == 2 * curr.size
    want_off, rows = [0], []
    for i in range(n_nodes):
        ks = [k for k in range(curr.size) if curr[k] == i] + [k for k in range(curr.size) if nxt[k] == i]
        rows += ks
        want_off.append(len(rows))
    assert off.tolist() == want_off
    assert np.array_equal(rec["curr"], curr[rows]) and np.array_equal(rec["next"], nxt[rows])
    assert np.array_equal(rec["p"], params[rows])
    assert off[8] - off[7] == 40
    hub = rec[off[7]:off[8]]
    assert np.all(hub["curr"][:20] == 7) and np.all(hub["next"][20:] == 7)  # curr entries, then next entries


# ---- flags, views, determinism, empty and cleared plans ---------------------------------

def test_accumulate_flags_views_and_repeatability(ctx, rods, graph):
    n_nodes, X, D, curr, nxt, params = graph
    rg = rods.RodForceGen(ctx, n_nodes, (curr, nxt, params))
    Xd, Dd = _dev(X), _dev(D)
    F, N = rg.compute(Xd, Dd)
    F, N = F.clone(), N.clone()
    rng = np.random.default_rng(1)
    F0, N0 = rng.normal(size=(n_nodes, 3)), rng.normal(size=(n_nodes, 3))
    for aF in (False, True):
        for aN in (False, True):
            Fo, No = rg.compute(Xd, Dd, F=_dev(F0), N=_dev(N0), accumulate_F=aF, accumulate_N=aN)
            assert torch.equal(Fo, _dev(F0) + F if aF else F), (aF, aN)
            assert torch.equal(No, _dev(N0) + N if aN else N), (aF, aN)
    # the defaults are the reference's: F accumulates, N is overwritten
    Fo, No = rg.compute(Xd, Dd, F=_dev(F0), N=_dev(N0))
    assert torch.equal(Fo, _dev(F0) + F) and torch.equal(No, N)
    # views 8 bytes into their buffers
    Fv, Nv = rg.compute(_view(X), _view(D), F=_view(F0), N=_view(N0), accumulate_F=True, accumulate_N=True)
    assert torch.equal(Fv, _dev(F0) + F) and torch.equal(Nv, _dev(N0) + N)
    # run to run
    F2, N2 = rg.compute(Xd, Dd)
    ctx.synchronize()
    assert torch.equal(F2, F) and torch.equal(N2, N)


def test_empty_and_cleared_plans(ctx, rods, graph):
    n_nodes, X, D, curr, nxt, params = graph
    Xd, Dd = _dev(X), _dev(D)
    F0 = np.random.default_rng(2).normal(size=(n_nodes, 3))
    for rg in (rods.RodForceGen(ctx, n_nodes), rods.RodForceGen(ctx, n_nodes, (curr, nxt, params))):
        rg.set_rods([], [], np.empty((0, 10)))  # the second plan is cleared
        Fo, No = rg.compute(Xd, Dd, F=_dev(F0), N=_dev(F0), accumulate_F=True, accumulate_N=True)
        assert np.array_equal(Fo.cpu().numpy(), F0) and np.array_equal(No.cpu().numpy(), F0)
        Fo, No = rg.compute(Xd, Dd, F=_dev(F0), N=_dev(F0), accumulate_F=False, accumulate_N=False)
        assert np.all(Fo.cpu().numpy() == 0.0) and np.all(No.cpu().numpy() == 0.0)
        off, rec = rg.plan()
        assert off.size == n_nodes + 1 and not off.any() and rec.size == 0


def test_argument_errors(ctx, rods, graph):
    from ibamr_amd._lib import IBTKLEError
    n_nodes, X, D, curr, nxt, params = graph
    rg = rods.RodForceGen(ctx, n_nodes, (curr, nxt, params))
    Xd, Dd = _dev(X), _dev(D)
    with pytest.raises(ValueError, match="X must be"):
        rg.compute(Xd[:-1], Dd)
    with pytest.raises(ValueError, match="D must be"):
        rg.compute(Xd, Dd.view(-1, 3))
    with pytest.raises(ValueError, match="N must be"):
        rg.compute(Xd, Dd, N=torch.zeros((n_nodes, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(IBTKLEError, match="must not overlap"):
        rg.compute(Xd, Dd, F=Xd)
    with pytest.raises(IBTKLEError, match="out of range"):
        rg.set_rods([0], [n_nodes], np.ones((1, 10)))
    assert rg.plan()[1].size == 2 * curr.size  # a failed set_rods leaves the plan as it was
    rg.close()
    with pytest.raises(ValueError, match="closed"):
        rg.compute(Xd, Dd)
    Dd9 = _dev(np.tile(np.eye(3).reshape(9), (4, 1)))
    W = _dev(np.ones((4, 3)))
    with pytest.raises(IBTKLEError, match="MIDPOINT"):
        rods.director_update(ctx, "midpoint", 0.1, Dd9, W)
    with pytest.raises(ValueError):
        rods.director_update(ctx, "trapezoidal", 0.1, Dd9, W)
    with pytest.raises(ValueError):
        rods.director_update(ctx, "euler", 0.1, Dd9, W[:3])
    buf = torch.zeros(4 * 9 + 3, dtype=torch.float64, device="cuda")
    with pytest.raises(IBTKLEError, match="overlaps"):
        rods.director_update(ctx, "euler", 0.1, buf[:36].view(4, 9), W, out=buf[3:39].view(4, 9))


# ---- degenerate triads -----------------------------------------------------------------

def test_half_turn_rod_touches_only_its_nodes(ctx, rods):
    """Rod (5, 20): node 20's triad is node 5's turned by half a turn, so A has the
    eigenvalue -1 twice and no principal root.  The call returns, and every node but 5 and
    20 is bit for bit what it is without that rod."""
    rng = np.random.default_rng(8)
    n = 21
    X, D, curr, nxt, params = _structure(rng, n, np.arange(19), np.arange(1, 20))
    D = np.tile(np.eye(3).reshape(9), (n, 1))  # exact triads: A of the bad rod is diag(-1, -1, 1)
    D[20] = (np.diag([-1.0, -1.0, 1.0]) @ np.eye(3)).reshape(9)
    base = _compute(ctx, rods, n, X, D, curr, nxt, params)
    c2, n2 = np.append(curr, 5).astype(np.int32), np.append(nxt, 20).astype(np.int32)
    p2 = np.vstack([params, params[:1]])
    bad = _compute(ctx, rods, n, X, D, c2, n2, p2)
    keep = np.ones(n, dtype=bool)
    keep[[5, 20]] = False
    for b, g in zip(base, bad):
        assert np.isfinite(b).all()
        assert np.array_equal(b[keep].view(np.int64), g[keep].view(np.int64))


# ---- director update -------------------------------------------------------------------

def _triads(rng, n):
    T = np.stack([_rot(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(n)])
    return (T + 1e-3 * rng.normal(size=T.shape)).reshape(n, 9)


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def test_director_update_threshold(ctx, rods, tol):
    rng = np.random.default_rng(6)
    D = _triads(rng, 3)
    W = np.zeros((3, 3))
    W[1, 1] = EPS        # |W| == DBL_EPSILON exactly: the test is >, so it copies
    W[2, 2] = 2.0 * EPS  # rotates
    dt = 2.0 ** 50       # |W| dt = 0.5 rad where it rotates
    got = rods.director_update(ctx, "euler", dt, _dev(D), _dev(W))
    assert np.array_equal(_bits(got)[:2], D.view(np.int64)[:2])
    ref = reference_director_update("euler", dt, D, W)
    assert np.abs(ref[2] - D[2]).max() > 0.1  # a visible rotation
    assert np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max() <= 2 * tol["D_new"]
    # -0.0 and NaN-free zeros copy bit for bit as well
    Z = np.zeros((3, 9))
    Z[0, 0] = -0.0
    assert np.array_equal(_bits(rods.director_update(ctx, "euler", 1.0, _dev(Z), _dev(np.zeros((3, 3))))), Z.view(np.int64))


@pytest.mark.parametrize("n", [1, 255, 257])
def test_director_update_sizes(ctx, rods, tol, n):
    rng = np.random.default_rng(n)
    D = _triads(rng, n)
    W0 = rng.normal(size=(n, 3)) * rng.uniform(0.1, 10.0, size=(n, 1))
    W1 = W0 + 0.3 * rng.normal(size=(n, 3))
    W0[n // 2] = 0.0
    dt = 0.0625
    Dd, W0d, W1d = _dev(D), _dev(W0), _dev(W1)
    for scheme in ("euler", "trapezoidal"):
        ref = reference_director_update(scheme, dt, D, W0, W1)
        got = rods.director_update(ctx, scheme, dt, Dd, W0d, W1d)
        e = np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max()
        print(f"director update {scheme} n={n}: device vs rod_ref {e:.3e} (bound {2 * tol['D_new']:.3e})")
        assert e <= 2 * tol["D_new"]
        # in place equals out of place, also 8 bytes into a buffer
        inplace = _view(D)
        assert rods.director_update(ctx, scheme, dt, inplace, W0d, W1d, out=inplace) is inplace
        assert torch.equal(inplace, got)
    # trapezoidal is Euler with 0.5 (W0 + W1)
    avg = _dev(0.5 * (W0 + W1))
    assert torch.equal(rods.director_update(ctx, "trapezoidal", dt, Dd, W0d, W1d),
                       rods.director_update(ctx, "euler", dt, Dd, avg))
    assert np.array_equal(_bits(rods.director_update(ctx, "euler", dt, Dd, W0d))[n // 2], D.view(np.int64)[n // 2])


def test_compute_refuses_another_context(le, ctx, rods):
    """set_rods and destroy wait for the plan's own context only, so compute runs on no other."""
    from ibamr_amd.le import _ptr
    other = le.Context(0)
    rg = rods.RodForceGen(ctx, 2, ([0], [1], np.ones((1, 10))))
    X, D = _dev(np.eye(3)[:2]), _dev(np.tile(np.eye(3).reshape(9), (2, 1)))
    F, N = torch.zeros_like(X), torch.zeros_like(X)
    rc = ctx.lib.ibtk_le_rodgen_compute(other.h, rg.h, _ptr(X), _ptr(D), _ptr(F), _ptr(N), 0, 0)
    assert rc == 4 and "another context" in ctx.lib.ibtk_le_last_error().decode()
    assert ctx.lib.ibtk_le_rodgen_compute(ctx.h, rg.h, _ptr(X), _ptr(D), _ptr(F), _ptr(N), 0, 0) == 0
    ctx.synchronize()
    rg.close()

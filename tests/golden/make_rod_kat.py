"""Writes tests/golden/rod_kat.json: known answers for the Kirchhoff rod path, evaluated at
50 digits with mpmath straight from IBKirchhoffRodForceGen.cpp:401-469 (mpmath.sqrtm for
the principal root) and GeneralizedIBMethod.cpp:344-378 / 410-444.  Run by hand
(``python tests/golden/make_rod_kat.py``); no test imports mpmath.

The file holds its own inputs (float64, exact in JSON), the 50-digit results rounded to
float64, and ``ref_err``: the worst error of the float64 host restatement (tests/rod_ref.py)
against those results per quantity, max|v - v_kat| / max|v_kat|.

(a) ``rods``: 64 rods on a branching graph of 50 nodes (a random tree, both orientations,
    plus 15 further rods, two of them repeats of earlier edges), random positive a*, b*,
    non-zero kappa1, kappa2 and tau, stretch |dX|/ds in 1.05-1.3, neighbour triads rotated
    by 0.05-2.5 rad about random axes, every triad perturbed by 1e-3.
(b) ``directors``: 64 director updates for both schemes.
"""
import json
import sys
from pathlib import Path

import mpmath as mp
import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from rod_ref import reference_director_update, reference_rods  # noqa: E402

mp.mp.dps = 50


def rot(axis, th):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def angle_between(Da, Db):
    """The rotation angle taking triad Da (rows) to Db, both orthonormal."""
    R = Db.T @ Da
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


def make_rods(rng):
    n_nodes, n_tree, n_rods = 50, 49, 64
    T = np.empty((n_nodes, 3, 3))  # orthonormal triads, rows D1 D2 D3
    X = np.empty((n_nodes, 3))
    T[0] = rot(rng.normal(size=3), rng.uniform(0, 3))
    X[0] = rng.normal(size=3)
    edges = []
    for i in range(1, n_nodes):
        par = int(rng.integers(0, i))
        R = rot(rng.normal(size=3), rng.uniform(0.05, 2.5))
        T[i] = T[par] @ R.T
        d = rng.normal(size=3)
        X[i] = X[par] + rng.uniform(0.05, 0.2) * d / np.linalg.norm(d)
        edges.append((par, i) if rng.random() < 0.5 else (i, par))
    while len(edges) < n_rods - 2:
        a, b = (int(v) for v in rng.integers(0, n_nodes, size=2))
        if a != b and 0.05 <= angle_between(T[a], T[b]) <= 2.5:
            edges.append((a, b))
    edges += [edges[3], edges[20]]  # repeated edges: two rods between one pair
    order = rng.permutation(len(edges))
    edges = [edges[j] for j in order]
    curr = np.array([e[0] for e in edges], dtype=np.int32)
    nxt = np.array([e[1] for e in edges], dtype=np.int32)
    D = (T + 1e-3 * rng.normal(size=T.shape)).reshape(n_nodes, 9)
    params = np.empty((n_rods, 10))
    for k in range(n_rods):
        params[k, 0] = np.linalg.norm(X[nxt[k]] - X[curr[k]]) / rng.uniform(1.05, 1.3)
        params[k, 1:7] = rng.uniform(0.5, 2.0, size=6)
        params[k, 7:10] = rng.uniform(0.1, 1.0, size=3) * rng.choice([-1.0, 1.0], size=3)
    return n_nodes, X, D, curr, nxt, params


def mpv(v):
    return mp.matrix([mp.mpf(float(x)) for x in v])


def cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def kat_rods(n_nodes, X, D, curr, nxt, params):
    F = [mp.matrix(3, 1) for _ in range(n_nodes)]
    N = [mp.matrix(3, 1) for _ in range(n_nodes)]
    for k in range(len(curr)):
        c, m = int(curr[k]), int(nxt[k])
        Dc = [mpv(D[c, 3 * i:3 * i + 3]) for i in range(3)]
        Dn = [mpv(D[m, 3 * i:3 * i + 3]) for i in range(3)]
        A = mp.matrix(3, 3)
        for i in range(3):
            A += Dn[i] * Dc[i].T
        S = mp.sqrtm(A).apply(mp.re)
        assert mp.mnorm(S * S - A, 1) < mp.mpf(10) ** -40
        Dh = [S * Dc[i] for i in range(3)]
        ds, a1, a2, a3, b1, b2, b3, k1, k2, tau = (mp.mpf(float(v)) for v in params[k])
        dX = mpv(X[m]) - mpv(X[c])
        dX_ds = dX / ds
        Fh = b1 * dot(Dh[0], dX_ds) * Dh[0] + b2 * dot(Dh[1], dX_ds) * Dh[1] + b3 * (dot(Dh[2], dX_ds) - 1) * Dh[2]
        dD = [(Dn[i] - Dc[i]) / ds for i in range(3)]
        Nh = (a1 * (dot(dD[1], Dh[2]) - k1) * Dh[0] + a2 * (dot(dD[2], Dh[0]) - k2) * Dh[1]
              + a3 * (dot(dD[0], Dh[1]) - tau) * Dh[2])
        t = cross(dX / 2, Fh)
        F[c] += Fh
        F[m] -= Fh
        N[c] += Nh + t
        N[m] += -Nh + t
    tof = lambda L: np.array([[float(v[d]) for d in range(3)] for v in L])  # noqa: E731
    return tof(F), tof(N)


def kat_director(trap, dt, D, W0, W1):
    out = np.empty_like(D)
    for l in range(D.shape[0]):
        e = mpv(W0[l])
        if trap:
            e = (e + mpv(W1[l])) / 2
        norm_e = mp.sqrt(dot(e, e))
        theta = norm_e * mp.mpf(float(dt))
        e = e / norm_e
        c, s = mp.cos(theta), mp.sin(theta)
        R = mp.matrix([[c + (1 - c) * e[0] * e[0], (1 - c) * e[0] * e[1] - s * e[2], (1 - c) * e[0] * e[2] + s * e[1]],
                       [(1 - c) * e[1] * e[0] + s * e[2], c + (1 - c) * e[1] * e[1], (1 - c) * e[1] * e[2] - s * e[0]],
                       [(1 - c) * e[2] * e[0] - s * e[1], (1 - c) * e[2] * e[1] + s * e[0], c + (1 - c) * e[2] * e[2]]])
        for a in range(3):
            v = R * mpv(D[l, 3 * a:3 * a + 3])
            out[l, 3 * a:3 * a + 3] = [float(v[d]) for d in range(3)]
    return out


def rel(v, kat):
    return float(np.abs(v - kat).max() / np.abs(kat).max())


def main():
    rng = np.random.default_rng(20240917)
    n_nodes, X, D, curr, nxt, params = make_rods(rng)
    F, N = kat_rods(n_nodes, X, D, curr, nxt, params)
    rF, rN = reference_rods(n_nodes, X, D, curr, nxt, params)

    nd = 64
    Dd = np.stack([rot(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(nd)]).reshape(nd, 9)
    Dd = Dd + 1e-3 * rng.normal(size=Dd.shape)
    W0 = rng.normal(size=(nd, 3)) * rng.uniform(0.1, 10.0, size=(nd, 1))
    W1 = W0 + 0.3 * rng.normal(size=(nd, 3))
    dt = 0.03125
    De = kat_director(False, dt, Dd, W0, W1)
    Dt = kat_director(True, dt, Dd, W0, W1)
    err_D = max(rel(reference_director_update("euler", dt, Dd, W0), De),
                rel(reference_director_update("trapezoidal", dt, Dd, W0, W1), Dt))
    out = {
        "digits": mp.mp.dps,
        "rods": {"n_nodes": n_nodes, "X": X.tolist(), "D": D.tolist(), "curr": curr.tolist(), "next": nxt.tolist(),
                 "params": params.tolist(), "F": F.tolist(), "N": N.tolist()},
        "directors": {"dt": dt, "D": Dd.tolist(), "W0": W0.tolist(), "W1": W1.tolist(), "D_euler": De.tolist(),
                      "D_trapezoidal": Dt.tolist()},
        "ref_err": {"F": rel(rF, F), "N": rel(rN, N), "D_new": err_D},
    }
    (HERE / "rod_kat.json").write_text(json.dumps(out, indent=0) + "\n")
    print("ref_err", out["ref_err"], "max|F|", np.abs(F).max(), "max|N|", np.abs(N).max())


if __name__ == "__main__":
    main()

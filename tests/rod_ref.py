"""A numpy-only restatement of the Kirchhoff rod loops, in the reference's order.

``reference_rods``: IBKirchhoffRodForceGen::computeLagrangianForceAndTorque
(IBKirchhoffRodForceGen.cpp:401-515) -- rod by rod into four scratch arrays, then the
curr contributions added in ascending k and after them the next contributions in ascending
k, as the two VecSetValuesBlocked(ADD_VALUES) calls per vector do.  The principal square
root goes through ``numpy.linalg.eig`` (the reference uses Eigen's Schur route; neither is
the device's Denman-Beavers iteration).

``reference_director_update``: GeneralizedIBMethod::eulerStep / trapezoidalStep
(GeneralizedIBMethod.cpp:344-378, 410-444).

float64 throughout; tests/golden/rod_kat.json records how far these are from the 50-digit
values (``ref_err``).
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def sqrtm3(A):
    """The principal square root of a real 3x3 matrix through its eigen-decomposition."""
    w, V = np.linalg.eig(A.astype(np.complex128))
    return (V @ np.diag(np.sqrt(w)) @ np.linalg.inv(V)).real


def rod_half(X, Xn, D, Dn, p):
    """(F_half, N_half) of one rod: X, Xn (3,), D, Dn (3, 3) rows D1 D2 D3, p (10,)."""
    ds, a1, a2, a3, b1, b2, b3, kappa1, kappa2, tau = (float(v) for v in p)
    A = np.zeros((3, 3))
    for i in range(3):
        A += np.outer(Dn[i], D[i])
    S = sqrtm3(A)
    Dh = [S @ D[i] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        dX_ds = (Xn - X) / ds
        F1 = b1 * Dh[0].dot(dX_ds)
        F2 = b2 * Dh[1].dot(dX_ds)
        F3 = b3 * (Dh[2].dot(dX_ds) - 1.0)
        F_half = F1 * Dh[0] + F2 * Dh[1] + F3 * Dh[2]
        dD = [(Dn[i] - D[i]) / ds for i in range(3)]
        N1 = a1 * (dD[1].dot(Dh[2]) - kappa1)
        N2 = a2 * (dD[2].dot(Dh[0]) - kappa2)
        N3 = a3 * (dD[0].dot(Dh[1]) - tau)
        N_half = N1 * Dh[0] + N2 * Dh[1] + N3 * Dh[2]
    return F_half, N_half


def reference_rods(n_nodes, X, D, curr, nxt, params, F=None, N=None):
    """F (given, or zeros) plus the rods' forces, and N likewise; returns new arrays."""
    X = np.asarray(X, dtype=np.float64).reshape(n_nodes, 3)
    D = np.asarray(D, dtype=np.float64).reshape(n_nodes, 3, 3)
    F = np.zeros((n_nodes, 3)) if F is None else np.array(F, dtype=np.float64).reshape(n_nodes, 3)
    N = np.zeros((n_nodes, 3)) if N is None else np.array(N, dtype=np.float64).reshape(n_nodes, 3)
    n = len(curr)
    Fc, Fn, Nc, Nn = (np.zeros((n, 3)) for _ in range(4))
    for k in range(n):
        c, m = int(curr[k]), int(nxt[k])
        F_half, N_half = rod_half(X[c], X[m], D[c], D[m], params[k])
        with np.errstate(invalid="ignore"):
            t = np.cross(0.5 * (X[m] - X[c]), F_half)
            Fc[k], Fn[k] = F_half, -F_half
            Nc[k], Nn[k] = N_half + t, -N_half + t
    acc_F, acc_N = np.zeros((n_nodes, 3)), np.zeros((n_nodes, 3))
    with np.errstate(invalid="ignore"):
        for k in range(n):
            acc_F[int(curr[k])] += Fc[k]
            acc_N[int(curr[k])] += Nc[k]
        for k in range(n):
            acc_F[int(nxt[k])] += Fn[k]
            acc_N[int(nxt[k])] += Nn[k]
        return F + acc_F, N + acc_N


def reference_director_update(scheme, dt, D, W0, W1=None):
    """scheme "euler" or "trapezoidal"; D (n, 9), W0 / W1 (n, 3).  Returns D_new (n, 9)."""
    D = np.asarray(D, dtype=np.float64).reshape(-1, 9)
    W0 = np.asarray(W0, dtype=np.float64).reshape(-1, 3)
    out = np.empty_like(D)
    for l in range(D.shape[0]):
        e = W0[l].copy() if scheme == "euler" else 0.5 * (W0[l] + np.asarray(W1, dtype=np.float64).reshape(-1, 3)[l])
        norm_e = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        if norm_e > EPS:
            theta = norm_e * dt
            e = e / norm_e
            c_t, s_t = np.cos(theta), np.sin(theta)
            R = np.array([[c_t + (1.0 - c_t) * e[0] * e[0], (1.0 - c_t) * e[0] * e[1] - s_t * e[2],
                           (1.0 - c_t) * e[0] * e[2] + s_t * e[1]],
                          [(1.0 - c_t) * e[1] * e[0] + s_t * e[2], c_t + (1.0 - c_t) * e[1] * e[1],
                           (1.0 - c_t) * e[1] * e[2] - s_t * e[0]],
                          [(1.0 - c_t) * e[2] * e[0] - s_t * e[1], (1.0 - c_t) * e[2] * e[1] + s_t * e[0],
                           c_t + (1.0 - c_t) * e[2] * e[2]]])
            for alpha in range(3):
                out[l, 3 * alpha:3 * alpha + 3] = R @ D[l, 3 * alpha:3 * alpha + 3]
        else:
            out[l] = D[l]
    return out

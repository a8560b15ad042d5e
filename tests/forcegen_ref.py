"""Serial restatement of IBStandardForceGen's three force loops (the tests' yardstick).

computeLagrangianSpringForce / BeamForce / TargetPointForce
(src/IB/IBStandardForceGen.cpp:778-892, 990-1099, 1150-1216) with the default spring law
(include/ibamr/IBSpringForceFunctions.h:117-120), on Python floats: IEEE doubles, one
rounded operation per reference operation, math.sqrt correctly rounded.  The accumulator
starts at zero, takes the springs, then the beams, then the target points, each in a
serial loop over k, and is then added to F (computeLagrangianForce, :265-313).
"""
import math
import sys

import numpy as np

EPS = sys.float_info.epsilon  # std::numeric_limits<double>::epsilon()


def accumulate_forces(n, ndim, X, springs=None, beams=None, targets=None, U=None, dX=None):
    """The reference's F_ghost: (n, ndim) float64.  springs = (mastr, slave, kappa, rest, ...),
    beams = (mastr, next, prev, bend, curv), targets = (node, kappa, eta, X0): flat arrays of
    node indices.  Positions are X + dX (:289)."""
    X = np.asarray(X, dtype=np.float64).reshape(n, ndim)
    x = (X + np.asarray(dX, dtype=np.float64).reshape(n, ndim) if dX is not None else X).tolist()
    u = np.asarray(U, dtype=np.float64).reshape(n, ndim).tolist() if U is not None else None
    acc = [[0.0] * ndim for _ in range(n)]
    R = range(ndim)
    if springs is not None:
        mastr, slave, kappa, rest = (np.asarray(a).tolist() for a in springs[:4])
        for k in range(len(mastr)):
            m, s = mastr[k], slave[k]
            D = [x[s][d] - x[m][d] for d in R]
            r2 = D[0] * D[0] + D[1] * D[1]
            if ndim == 3:
                r2 = r2 + D[2] * D[2]
            r = math.sqrt(r2)
            if r < EPS:
                continue
            t_over_r = (kappa[k] * (r - rest[k])) / r
            for d in R:
                f = t_over_r * D[d]
                acc[m][d] += f
                acc[s][d] -= f
    if beams is not None:
        mastr, nxt, prv, bend = (np.asarray(a).tolist() for a in beams[:4])
        curv = np.asarray(beams[4], dtype=np.float64).reshape(len(mastr), ndim).tolist()
        for k in range(len(mastr)):
            m, a, b = mastr[k], nxt[k], prv[k]
            for d in R:
                f = bend[k] * (x[a][d] + x[b][d] - 2.0 * x[m][d] - curv[k][d])
                acc[m][d] += 2.0 * f
                acc[a][d] -= f
                acc[b][d] -= f
    if targets is not None:
        node, kappa, eta = (np.asarray(a).tolist() for a in targets[:3])
        X0 = np.asarray(targets[3], dtype=np.float64).reshape(len(node), ndim).tolist()
        for k in range(len(node)):
            i = node[k]
            for d in R:
                acc[i][d] += kappa[k] * (X0[k][d] - x[i][d]) - eta[k] * (u[i][d] if u is not None else 0.0)
    return np.array(acc, dtype=np.float64).reshape(n, ndim)


def reference_force(n, ndim, X, springs=None, beams=None, targets=None, U=None, dX=None, F=None, accumulate=True):
    """F + F_ghost (accumulate, the reference's VecAXPY at :311) or F_ghost alone."""
    acc = accumulate_forces(n, ndim, X, springs, beams, targets, U, dX)
    if accumulate and F is not None:
        return np.asarray(F, dtype=np.float64).reshape(n, ndim) + acc
    return acc

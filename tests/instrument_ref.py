"""Plain Python / math scalar restatement of IBInstrumentPanel's flow meters and pressure
gauges, loop for loop (src/IB/IBInstrumentPanel.cpp):

* ``init_meter_elements``  -- init_meter_elements (:133-194)
* ``update``               -- initializeHierarchyDependentData (:698-923), one level, one patch
* ``interp_cell`` / ``interp_side`` -- linear_interp (:315-369, :434-501)
* ``flow_correction``      -- compute_flow_correction (:199-234)
* ``read``                 -- readInstrumentData (:925-1182)

This is a restatement, not the reference's code: the reference needs SAMRAI and PETSc and
cannot be compiled beside these tests.  One patch, one rank.  Every operation is a float64
operation in the reference's order, with the associations of its Eigen 3.2.1 expressions:
a fixed-size reduction is unrolled as halves (Eigen/src/Core/Redux.h:77-106), so
``a.dot(b) = a0 b0 + (a1 b1 + a2 b2)`` and ``norm = sqrt(x^2 + (y^2 + z^2))``; ``cross`` is the
textbook one, ``v / s`` is a division per component, and ``v /= s`` -- the centroid's and
the centroid velocity's (:791, :1149) -- multiplies each component by ``1.0 / s``
(Eigen/src/Core/SelfCwiseBinaryOp.h:181-193).  ``read`` walks the cells of the patch box
with x fastest, as SAMRAI's Box iterator does, and within a cell the web patches in the order
they were inserted (meter, then m, then n: multimap::equal_range keeps it), so the order of a
meter's sums is the reference's by construction, not by a sort.  Python raises where IEEE
arithmetic divides by zero; ``fdiv`` gives the IEEE quotient there.

A cell-centred field is a numpy array of the ghost box, shape (n2, n1, n0) [x fastest]
(source_ref.Geo); the side-centred u is three such arrays, array a one longer along axis a,
element [z][y][x] the lower side of cell (x, y, z) along a.  The tests hold this module to
exact known answers (tests/golden/instrument_kat.npz) and the device code to this module.
"""
from __future__ import annotations

import math

import numpy as np

from source_ref import Geo, bits, cell_index  # noqa: F401  (the patch, and getCellIndex's rule)

NAN = float("nan")


def fdiv(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def dot(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def norm(a):
    return math.sqrt(a[0] * a[0] + (a[1] * a[1] + a[2] * a[2]))


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def init_meter_elements(Xp, Xc, nw):
    """X_web[m][n], dA_web[m][n] (:133-194)."""
    P = len(Xp)
    X_web = [[None] * nw for _ in range(P)]
    dA_web = [[None] * nw for _ in range(P)]
    if nw == 0:  # (dX0 = ... / 0.0 is never used)
        return X_web, dA_web
    R = range(3)
    for m in range(P):
        Xp0 = Xp[m]
        dX0 = [(Xc[d] - Xp0[d]) / float(nw) for d in R]
        Xp1 = Xp[(m + 1) % P]
        dX1 = [(Xc[d] - Xp1[d]) / float(nw) for d in R]
        for n in range(nw):
            X0 = [Xp0[d] + float(n) * dX0[d] for d in R]
            X1 = [Xp1[d] + float(n) * dX1[d] for d in R]
            X2 = [Xp1[d] + float(n + 1) * dX1[d] for d in R]
            X3 = [Xp0[d] + float(n + 1) * dX0[d] for d in R]
            X01 = [0.5 * (X0[d] + X1[d]) for d in R]
            X12 = [0.5 * (X1[d] + X2[d]) for d in R]
            X23 = [0.5 * (X2[d] + X3[d]) for d in R]
            X30 = [0.5 * (X3[d] + X0[d]) for d in R]
            l0 = X01
            d0 = [X23[d] - X01[d] for d in R]
            l1 = X12
            d1 = [X30[d] - X12[d] for d in R]
            d0d0 = dot(d0, d0)
            d0d1 = dot(d0, d1)
            d1d1 = dot(d1, d1)
            d0l0 = dot(d0, l0)
            d0l1 = dot(d0, l1)
            d1l0 = dot(d1, l0)
            d1l1 = dot(d1, l1)
            t = fdiv(-d0l0 * d1d1 + d0l1 * d1d1 + d0d1 * d1l0 - d0d1 * d1l1, -d0d1 * d0d1 + d1d1 * d0d0)
            s = fdiv(d1l0 * d0d0 - d0d1 * d0l0 + d0d1 * d0l1 - d1l1 * d0d0, -d0d1 * d0d1 + d1d1 * d0d0)
            X_web[m][n] = [0.5 * (l0[d] + t * d0[d] + l1[d] + s * d1[d]) for d in R]
            c = cross([X2[d] - X0[d] for d in R], [X3[d] - X1[d] for d in R])
            dA_web[m][n] = [0.5 * c[d] for d in R]
    return X_web, dA_web


def locate(geo, domain, X):
    """The cell of X by getCellIndex in the domain frame with the patch's dx, and whether it
    lies in the patch box (:881-889)."""
    lo, hi, xlo, xup = domain
    i = tuple(cell_index(X[d], xlo[d], xup[d], geo.dx[d], lo[d], hi[d]) for d in range(3))
    return i, all(geo.ilower[d] <= i[d] <= geo.iupper[d] for d in range(3))


def patch_domain(geo):
    return (geo.ilower, geo.iupper, geo.x_lower, geo.x_upper)


def update(geo, X, meters, domain=None, h_finest=None):
    """initializeHierarchyDependentData for one level that is one patch.  ``meters`` is a list,
    per meter, of the local nodes of its perimeter positions 0..P-1.  Returns a list of dicts:
    Xp, Xc, r_max, nw, X_web, dA_web, cell, counted [m][n], cen_cell, cen_counted."""
    if domain is None:
        domain = patch_domain(geo)
    if h_finest is None:
        h_finest = min(geo.dx)
    out = []
    for nodes in meters:
        P = len(nodes)
        Xp = [[float(X[k][d]) for d in range(3)] for k in nodes]
        Xc = [0.0, 0.0, 0.0]
        for n in range(P):
            for d in range(3):
                Xc[d] += Xp[n][d]
        rP = 1.0 / float(P)  # Eigen's v /= s multiplies by Scalar(1) / s (SelfCwiseBinaryOp.h:181-193)
        for d in range(3):
            Xc[d] *= rP
        r_max = 0.0
        for n in range(P):
            r_max = max(r_max, norm([Xp[n][d] - Xc[d] for d in range(3)]))
        nw = 2 * int(math.ceil(r_max / h_finest))
        X_web, dA_web = init_meter_elements(Xp, Xc, nw)
        cell = [[None] * nw for _ in range(P)]
        counted = [[False] * nw for _ in range(P)]
        for m in range(P):
            for n in range(nw):
                cell[m][n], counted[m][n] = locate(geo, domain, X_web[m][n])
        cen_cell, cen_counted = locate(geo, domain, Xc)
        out.append(dict(P=P, Xp=Xp, Xc=Xc, r_max=r_max, nw=nw, X_web=X_web, dA_web=dA_web, cell=cell, counted=counted,
                        cen_cell=cen_cell, cen_counted=cen_counted))
    return out


def x_cell(geo, i):
    """:990-996"""
    return [geo.x_lower[d] + geo.dx[d] * (float(i[d] - geo.ilower[d]) + 0.5) for d in range(3)]


def hat(X, Xc, dx):
    return (X - (Xc - dx) if X < Xc else (Xc + dx) - X) / dx


def interp_cell(geo, v, X, i, X_cell, touched=None):
    """linear_interp of cell-centred data (:315-369)."""
    dx = geo.dx
    lower = [X[d] < X_cell[d] for d in range(3)]
    U = 0.0
    for s2 in range(-1 if lower[2] else 0, (0 if lower[2] else 1) + 1):
        for s1 in range(-1 if lower[1] else 0, (0 if lower[1] else 1) + 1):
            for s0 in range(-1 if lower[0] else 0, (0 if lower[0] else 1) + 1):
                Xc = (X_cell[0] + float(s0) * dx[0], X_cell[1] + float(s1) * dx[1], X_cell[2] + float(s2) * dx[2])
                wgt = (hat(X[0], Xc[0], dx[0]) * hat(X[1], Xc[1], dx[1])) * hat(X[2], Xc[2], dx[2])
                a = geo.at((i[0] + s0, i[1] + s1, i[2] + s2))
                if touched is not None:
                    touched[a] = True
                U += float(v[a]) * wgt
    return U


def interp_side(geo, u, X, i, X_cell, touched=None):
    """linear_interp of side-centred data (:434-501): [U0, U1, U2]."""
    dx = geo.dx
    U = [0.0, 0.0, 0.0]
    for axis in range(3):
        lower = [False if d == axis else X[d] < X_cell[d] for d in range(3)]
        off = [-0.5 if d == axis else 0.0 for d in range(3)]
        for s2 in range(-1 if lower[2] else 0, (0 if lower[2] else 1) + 1):
            for s1 in range(-1 if lower[1] else 0, (0 if lower[1] else 1) + 1):
                for s0 in range(-1 if lower[0] else 0, (0 if lower[0] else 1) + 1):
                    Xs = (X_cell[0] + (float(s0) + off[0]) * dx[0], X_cell[1] + (float(s1) + off[1]) * dx[1],
                          X_cell[2] + (float(s2) + off[2]) * dx[2])
                    wgt = (hat(X[0], Xs[0], dx[0]) * hat(X[1], Xs[1], dx[1])) * hat(X[2], Xs[2], dx[2])
                    a = geo.at((i[0] + s0, i[1] + s1, i[2] + s2))  # the lower side of cell i + shift
                    if touched is not None:
                        touched[axis][a] = True
                    U[axis] += float(u[axis][a]) * wgt
    return U


def flow_correction(Up, Uc, Xp, Xc):
    """compute_flow_correction (:199-234)."""
    P = len(Xp)
    total = 0.0
    for m in range(P):
        m1 = (m + 1) % P
        U = [(Up[m][d] + Up[m1][d] + Uc[d]) / 3.0 for d in range(3)]
        c = cross([Xc[d] - Xp[m][d] for d in range(3)], [Xc[d] - Xp[m1][d] for d in range(3)])
        total += dot(U, [0.5 * c[d] for d in range(3)])
    return total


def centroid_velocity(Up):
    Uc = [0.0, 0.0, 0.0]
    for n in range(len(Up)):
        for d in range(3):
            Uc[d] += Up[n][d]
    rP = 1.0 / float(len(Up))  # v /= s, as for the centroid
    return [Uc[d] * rP for d in range(3)]


def side_shapes(geo):
    return [tuple(geo.n[d] + 2 * geo.g + (1 if d == a else 0) for d in (2, 1, 0)) for a in range(3)]


def read(geo, webs, u, p, U, meters, plain=False, touched=None):
    """readInstrumentData.  Returns (values [L][3] = flow, mean pressure, point pressure; stats):
    stats holds, per meter, the three raw sums, the correction, and the sums of the absolute
    terms.  plain: add each meter's terms in (m, n) order instead of the reference's cell
    order (the tests show the two differ).  touched: (three side masks, a cell mask) that
    receive every element read."""
    L = len(webs)
    flow, mean, A, point = [0.0] * L, [0.0] * L, [0.0] * L, [0.0] * L
    aflow, amean = [0.0] * L, [0.0] * L
    tu = touched[0] if touched else None
    tp = touched[1] if touched else None

    def one(l, m, n, i):
        w = webs[l]
        X, dA = w["X_web"][m][n], w["dA_web"][m][n]
        Xc = x_cell(geo, i)
        if u is not None:
            term = dot(interp_side(geo, u, X, i, Xc, tu), dA)
            flow[l] += term
            aflow[l] += abs(term)
        if p is not None:
            a = norm(dA)
            term = interp_cell(geo, p, X, i, Xc, tp) * a
            mean[l] += term
            amean[l] += abs(term)
            A[l] += a

    if plain:
        for l, w in enumerate(webs):
            for m in range(w["P"]):
                for n in range(w["nw"]):
                    if w["counted"][m][n]:
                        one(l, m, n, w["cell"][m][n])
    else:
        by_cell = {}
        for l, w in enumerate(webs):
            for m in range(w["P"]):
                for n in range(w["nw"]):
                    if w["counted"][m][n]:
                        by_cell.setdefault(w["cell"][m][n], []).append((l, m, n))
        for i2 in range(geo.ilower[2], geo.iupper[2] + 1):
            for i1 in range(geo.ilower[1], geo.iupper[1] + 1):
                for i0 in range(geo.ilower[0], geo.iupper[0] + 1):
                    for l, m, n in by_cell.get((i0, i1, i2), ()):
                        one(l, m, n, (i0, i1, i2))
    values, stats = [], []
    for l, w in enumerate(webs):
        if p is not None and w["cen_counted"]:
            point[l] = interp_cell(geo, p, w["Xc"], w["cen_cell"], x_cell(geo, w["cen_cell"]), tp)
        Up = [[float(U[k][d]) for d in range(3)] for k in meters[l]]
        corr = flow_correction(Up, centroid_velocity(Up), w["Xp"], w["Xc"])
        values.append([flow[l] - corr, fdiv(mean[l], A[l]), point[l]])
        stats.append(dict(flow=flow[l], mean=mean[l], A=A[l], corr=corr, abs_flow=aflow[l], abs_mean=amean[l]))
    return np.array(values, dtype=np.float64).reshape(L, 3), stats

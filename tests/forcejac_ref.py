"""Serial restatement of IBStandardForceGen's force Jacobian (the tests' yardstick).

computeLagrangianForceJacobian (src/IB/IBStandardForceGen.cpp:498-665) and
computeLagrangianForceJacobianNonzeroStructure (:315-496) with the default spring law and
its derivative (include/ibamr/IBSpringForceFunctions.h:117-131), on Python floats: IEEE
doubles, one rounded operation per reference operation, math.sqrt correctly rounded.

The matrix is a dictionary {(block row, block col): block}, a block a row-major list of
ndim * ndim floats as MatSetValuesBlocked reads the values it is handed.  It starts with the
diagonal block of every node at +0.0 (the reference preallocates the diagonal, :351, and
MatZeroEntries leaves +0.0); every other block starts at +0.0 when the first call touches it.
Contributions are added as whole blocks, zeros included, in the order of the calls.
"""
import math

import numpy as np


def eigen_norm(D):
    """Vector::norm() of Eigen 3.2.1 for a fixed size 2 or 3: the reduction is unrolled as
    halves (Redux.h:77-106), x^2 + (y^2 + z^2) in 3-D, not the left-to-right sum."""
    if len(D) == 3:
        return math.sqrt(D[0] * D[0] + (D[1] * D[1] + D[2] * D[2]))
    return math.sqrt(D[0] * D[0] + D[1] * D[1])


def spring_dF(D, kappa, rest, X_coef):
    """The reference's dF_dX(i, j) of one spring, as dF[i][j] (:541-565)."""
    nd = len(D)
    R = eigen_norm(D)
    T = kappa * (R - rest)
    dT_dR = kappa

    def div(a, b):  # IEEE: 0/0 and x/0 do not raise
        return float(np.float64(a) / np.float64(b))

    with np.errstate(all="ignore"):
        T_R = div(T, R)
        return [[X_coef * ((T_R * (1.0 if i == j else 0.0)) + div(((dT_dR - T_R) * D[i]) * D[j], R * R))
                 for j in range(nd)] for i in range(nd)]


def stored_block(dF):
    """What MatSetValuesBlocked stores of dF_dX.data(): Eigen's column-major array read
    row-major, so stored element (r, c) = dF(c, r).  Row-major list."""
    nd = len(dF)
    return [dF[c][r] for r in range(nd) for c in range(nd)]


def reference_jacobian(n, ndim, X, springs=None, beams=None, targets=None, X_coef=1.0, U_coef=0.0, dX=None,
                       exact=False):
    """(J, A, count): J[(row, col)] the block, A[(row, col)] the element-wise sum of the
    absolute values of its contributions, count[(row, col)] the number of contributions.
    exact=True: a fourth dictionary, the sum of each block's contributions in
    numpy.longdouble (what a product formed contribution by contribution is measured by)."""
    X = np.asarray(X, dtype=np.float64).reshape(n, ndim)
    x = (X + np.asarray(dX, dtype=np.float64).reshape(n, ndim) if dX is not None else X).tolist()
    bs = ndim * ndim
    J = {(i, i): [0.0] * bs for i in range(n)}
    A = {(i, i): [0.0] * bs for i in range(n)}
    count = {(i, i): 0 for i in range(n)}
    E = {(i, i): np.zeros(bs, dtype=np.longdouble) for i in range(n)} if exact else None

    def add(row, col, blk):
        key = (row, col)
        if key not in J:
            J[key] = [0.0] * bs
            A[key] = [0.0] * bs
            count[key] = 0
            if exact:
                E[key] = np.zeros(bs, dtype=np.longdouble)
        if exact:
            E[key] = E[key] + np.array(blk, dtype=np.longdouble)
        J[key] = [a + b for a, b in zip(J[key], blk)]
        A[key] = [a + abs(b) for a, b in zip(A[key], blk)]
        count[key] += 1

    def diag(v):
        return [v if e % (ndim + 1) == 0 else 0.0 for e in range(bs)]

    if springs is not None:
        mastr, slave, kappa, rest = (np.asarray(a).tolist() for a in springs[:4])
        for k in range(len(mastr)):
            m, s = mastr[k], slave[k]
            D = [x[s][d] - x[m][d] for d in range(ndim)]
            blk = stored_block(spring_dF(D, kappa[k], rest[k], X_coef))
            add(m, s, blk)
            add(s, m, blk)
            neg = [b * -1.0 for b in blk]
            add(m, m, neg)
            add(s, s, neg)
    if beams is not None:
        mastr, nxt, prv, bend = (np.asarray(a).tolist() for a in beams[:4])
        for k in range(len(mastr)):
            m, a, p = mastr[k], nxt[k], prv[k]
            blk = diag(-1.0 * bend[k] * X_coef)
            add(p, p, blk)
            add(p, a, blk)
            add(a, p, blk)
            add(a, a, blk)
            blk = diag(+2.0 * bend[k] * X_coef)
            add(p, m, blk)
            add(a, m, blk)
            add(m, p, blk)
            add(m, a, blk)
            blk = diag(-4.0 * bend[k] * X_coef)
            add(m, m, blk)
    if targets is not None:
        node, kappa, eta = (np.asarray(a).tolist() for a in targets[:3])
        for k in range(len(node)):
            i = node[k]
            add(i, i, diag(-X_coef * kappa[k] - U_coef * eta[k]))
    if exact:
        return J, A, count, E
    return J, A, count


def bsr_arrays(n, ndim, J):
    """The dictionary as block-CSR: rowptr (n + 1 int64), col (int32, ascending within a
    row), val (blocks, ndim, ndim)."""
    keys = sorted(J)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    for r, _ in keys:
        rowptr[r + 1] += 1
    rowptr = np.cumsum(rowptr)
    col = np.array([c for _, c in keys], dtype=np.int32)
    val = np.array([J[k] for k in keys], dtype=np.float64).reshape(len(keys), ndim, ndim)
    return rowptr, col, val


def reference_nnz(n, n_local, springs=None, beams=None):
    """The per-block-row counts of :351-457, before the expansion to scalar rows; a node is
    local iff its index is < n_local.  Two int arrays over all n nodes."""
    d = [1] * n
    o = [0] * n
    if springs is not None:
        mastr, slave = (np.asarray(a).tolist() for a in springs[:2])
        for k in range(len(mastr)):
            t = d if slave[k] < n_local else o
            t[mastr[k]] += 1
            t[slave[k]] += 1
    if beams is not None:
        mastr, nxt, prv = (np.asarray(a).tolist() for a in beams[:3])
        for k in range(len(mastr)):
            m, a, p = mastr[k], nxt[k], prv[k]
            nl, pl = a < n_local, p < n_local
            if nl and pl:
                for i, v in ((m, 2), (a, 2), (p, 2)):
                    d[i] += v
            elif nl:
                for i, v in ((m, 1), (a, 1)):
                    d[i] += v
                for i, v in ((m, 1), (a, 1), (p, 2)):
                    o[i] += v
            elif pl:
                for i, v in ((m, 1), (p, 1)):
                    d[i] += v
                for i, v in ((m, 1), (a, 2), (p, 1)):
                    o[i] += v
            else:
                for i, v in ((a, 2), (p, 2)):
                    d[i] += v
                for i, v in ((m, 2), (a, 2), (p, 2)):
                    o[i] += v
    return np.array(d, dtype=np.int32), np.array(o, dtype=np.int32)

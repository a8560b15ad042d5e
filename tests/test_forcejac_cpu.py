"""The serial restatement of the force Jacobian (tests/forcejac_ref.py) checked by itself, so
that the bitwise GPU comparison of test_gpu_forcejac.py means something; and the argument
checks of the new entry points that fire before any device call.  No GPU."""
import math

import numpy as np
import pytest

from forcegen_ref import reference_force
from forcejac_ref import bsr_arrays, eigen_norm, reference_jacobian, reference_nnz, spring_dF, stored_block

U = 2.0 ** -53


def gamma(m):
    return m * U / (1.0 - m * U)


def _random_case(ndim, n=40, ns=90, nb=25, with_targets=True, seed=3):
    """Random positions in the unit box; springs with repeats whose rest lengths stay at least
    10 % away from their lengths; beams; a target point on every fourth node."""
    rng = np.random.default_rng(seed + ndim)
    X = rng.random((n, ndim))
    m = rng.integers(0, n, ns)
    s = (m + rng.integers(1, n, ns)) % n
    m[-5:], s[-5:] = m[:5], s[:5]  # repeated edges
    R = np.linalg.norm(X[s] - X[m], axis=1)
    f = np.where(rng.random(ns) < 0.5, rng.uniform(0.3, 0.9, ns), rng.uniform(1.1, 1.7, ns))
    springs = (m, s, rng.uniform(1.0, 100.0, ns), f * R)
    bm = rng.integers(0, n, nb)
    bn = (bm + rng.integers(1, n, nb)) % n
    bp = (bm + rng.integers(1, n, nb)) % n
    bp[0] = bn[0]  # a beam with next == prev
    beams = (bm, bn, bp, rng.uniform(0.5, 10.0, nb), rng.standard_normal((nb, ndim)) * 0.1)
    node = np.arange(0, n, 4)
    targets = (node, rng.uniform(1.0, 50.0, node.size), rng.random(node.size), rng.random((node.size, ndim)))
    return dict(n=n, ndim=ndim, X=X, springs=springs, beams=beams, targets=targets if with_targets else None)


@pytest.mark.parametrize("ndim", [3, 2])
def test_spring_blocks_against_50_digits(ndim):
    """Every element dF(i, j) of every spring of a random case against the analytic

        X_coef ((T / R) delta_ij + (kappa - T / R) D_i D_j / R^2),  T = kappa (R - L),

    evaluated with 50 digits from the same double inputs, within
    c 2^-53 |X_coef| (|T / R| + |kappa - T / R|).

    c: the longest chain of rounded operations that ends in an element is 14 long --
    D = xs - xm; its square; the two adds of the 3-D norm; sqrt; R - L; kappa (.); T / R;
    kappa - T / R; (.) D_i; (.) D_j; (.) / (R R); the add to (T / R) delta_ij; X_coef (.)
    (R R branches off after the sqrt and is shorter; (T / R) delta_ij is exact) -- and every
    operation's relative error reaches the element with a factor of at most 1 in the scale
    |T / R| + |kappa - T / R| = kappa (|1 - L / R| + L / R): the one place where an error is
    amplified relative to its own operand is R - L, and d(T / R) = kappa (L / R) dR / R is
    still within that scale.  Times 2 for the rounding of D and R that feeds R - L and reaches
    an element twice, through T / R and through kappa - T / R: c = 28."""
    import decimal
    dec = decimal.Context(prec=50)  # Decimal(float) is exact; +, -, *, / and sqrt round to 50 digits
    Dc = decimal.Decimal
    c = _random_case(ndim)
    m, s, kappa, rest = c["springs"]
    X_coef = 0.7
    worst = 0.0
    for k in range(m.size):
        xs, xm = c["X"][s[k]].tolist(), c["X"][m[k]].tolist()
        D = [xs[d] - xm[d] for d in range(ndim)]
        R = eigen_norm(D)
        assert abs(R - rest[k]) >= 0.09 * R  # the rest lengths keep their distance
        dF = spring_dF(D, float(kappa[k]), float(rest[k]), X_coef)
        with decimal.localcontext(dec):
            De = [Dc(xs[d]) - Dc(xm[d]) for d in range(ndim)]
            Re = sum(d * d for d in De).sqrt()
            Ke = Dc(float(kappa[k]))
            Te = Ke * (Re - Dc(float(rest[k])))
            scale = Dc(U) * abs(Dc(X_coef)) * (abs(Te / Re) + abs(Ke - Te / Re))
            for i in range(ndim):
                for j in range(ndim):
                    exact = Dc(X_coef) * ((Te / Re) * (1 if i == j else 0) + (Ke - Te / Re) * De[i] * De[j] / (Re * Re))
                    err = abs(Dc(dF[i][j]) - exact)
                    worst = max(worst, float(err / scale))
                    assert err <= 28 * scale, (k, i, j)
    print(f"ndim {ndim}: worst error {worst:.2f} units of 2^-53 scale (bound 28)")
    assert worst > 0.0  # the comparison is not between two copies of one evaluation


@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("with_targets", [False, True])
def test_translation_invariance(ndim, with_targets):
    """A rigid translation changes no spring or beam force: every block row sums to zero.  The
    contributions of a row cancel exactly ((m, s) against (m, m); -b - b + 2 b; 2 b + 2 b - 4 b:
    scalings by powers of two), so what remains is the rounding of the adds inside each block,
    at most gamma_m sum |contributions| with m the row's contributions.  With target points the
    row sum is the node's target diagonal."""
    c = _random_case(ndim, with_targets=with_targets)
    n, X_coef, U_coef = c["n"], 0.5, -0.25 / 3e-3
    J, A, cnt = reference_jacobian(n, ndim, c["X"], c["springs"], c["beams"], c["targets"], X_coef, U_coef)
    tdiag = np.zeros(n)
    if with_targets:
        node, kappa, eta = c["targets"][:3]
        for k in range(node.size):
            tdiag[node[k]] += -X_coef * kappa[k] - U_coef * eta[k]
    bs = ndim * ndim
    for i in range(n):
        keys = [k for k in J if k[0] == i]
        mrow = sum(cnt[k] for k in keys)
        for e in range(bs):
            total = math.fsum(J[k][e] for k in keys)
            want = tdiag[i] if e % (ndim + 1) == 0 else 0.0
            bound = gamma(mrow) * math.fsum(A[k][e] for k in keys)
            assert abs(total - want) <= bound, (i, e, total, want, bound)


def _matvec_longdouble(n, ndim, J, V):
    Y = np.zeros((n, ndim), dtype=np.longdouble)
    Vl = V.astype(np.longdouble)
    for (r, c), blk in J.items():
        Y[r] += np.array(blk, dtype=np.longdouble).reshape(ndim, ndim) @ Vl[c]
    return Y


def _jac_error(n, ndim, A, cnt, V):
    """What the restated blocks' own rounding can move J V by: gamma_count |contributions| |V|."""
    E = np.zeros((n, ndim))
    for (r, c), blk in A.items():
        E[r] += gamma(cnt[(r, c)] + 1) * (np.array(blk).reshape(ndim, ndim) @ np.abs(V[c]))
    return E


def test_finite_difference_linear_classes():
    """Beams and target points are linear in X: the central difference of the restated force,
    (F(X + eps V) - F(X - eps V)) / (2 eps) with X_coef = 1 (U_coef multiplies dF/dU, which a
    difference in X does not see: eta = 0 here), has no truncation term, and the restatement's
    J V must agree within the rounding of the two force evaluations,

        (n_i + 10) 2^-53 S_i / eps.

    S_i bounds the sum of the absolute values of the terms of F_i at |X| + eps |V|; a term
    takes at most 7 rounded operations and the sum n_i adds, so each evaluation is off by at
    most gamma_(n_i + 7) S_i, the rounded X +- eps V (2 operations) moves it by at most
    2 * 2^-53 S_i more, and the two evaluations' errors add and are divided by 2 eps.
    eps = 2^-12 is a power of two: no rounding in the division."""
    c = _random_case(3, with_targets=True)
    n, nd = c["n"], 3
    node, kappa, eta, X0 = c["targets"]
    targets = (node, kappa, np.zeros_like(eta), X0)
    rng = np.random.default_rng(11)
    V = rng.standard_normal((n, nd))
    eps = 2.0 ** -12
    J, A, cnt = reference_jacobian(n, nd, c["X"], None, c["beams"], targets, 1.0, 0.0)
    Y = _matvec_longdouble(n, nd, J, V)
    Fp = reference_force(n, nd, c["X"] + eps * V, None, c["beams"], targets, accumulate=False)
    Fm = reference_force(n, nd, c["X"] - eps * V, None, c["beams"], targets, accumulate=False)
    fd = (Fp.astype(np.longdouble) - Fm.astype(np.longdouble)) / (2 * eps)
    Xa = np.abs(c["X"]) + eps * np.abs(V)
    S = np.zeros((n, nd))
    terms = np.zeros(n)
    bm, bn, bp, bend, curv = c["beams"]
    for k in range(bm.size):
        f = bend[k] * (Xa[bn[k]] + Xa[bp[k]] + 2.0 * Xa[bm[k]] + np.abs(curv[k]))
        for i, w in ((bm[k], 2.0), (bn[k], 1.0), (bp[k], 1.0)):
            S[i] += w * f
            terms[i] += 1
    for k in range(node.size):
        S[node[k]] += kappa[k] * (np.abs(X0[k]) + Xa[node[k]])
        terms[node[k]] += 1
    bound = (terms[:, None] + 10) * U * S / eps + _jac_error(n, nd, A, cnt, V)
    err = np.abs(np.asarray(Y - fd, dtype=np.float64))
    print(f"linear classes: max error {err.max():.3e}, max |J V| {np.abs(np.asarray(Y, dtype=float)).max():.3e}, "
          f"largest bound {bound.max():.3e}")
    assert (err <= bound).all()
    assert np.abs(np.asarray(Y, dtype=float)).max() > 1.0  # not a comparison of zeros


def test_finite_difference_springs():
    """The loose case: springs.  f(D) = kappa D - kappa L D / |D|, and the third directional
    derivative of D / |D| along w is at most 15 |w|^3 / |D|^3 (the derivatives of 1 / R grow as
    1, 1, 3, 15 / R^(k+1), and D / |D| is the gradient of |D|), so the central difference
    truncates by at most eps^2 / 6 * 15 kappa L |w|^3 / Rmin^3 per spring, w = V_s - V_m,
    Rmin = R - eps |w| the shortest length on the segment.  The rounding term is as in the
    linear case with 4 more operations per term for the norm, (n_i + 14) 2^-53 S_i / eps; S_i
    is the sum of the springs' |T| <= kappa (R + L), times 1 + max |X| / Rmin because the
    rounding of X +- eps V is relative to |X| while a spring's force varies on the scale of R.
    The blocks of J themselves are off by at most 28 * 2^-53 kappa (|1 - L / R| + L / R) per
    element (test_spring_blocks_against_50_digits; the force loop's left-to-right norm differs
    from Eigen's by such a rounding too)."""
    c = _random_case(3, with_targets=False)
    n, nd = c["n"], 3
    m, s, kappa, rest = c["springs"]
    rng = np.random.default_rng(12)
    V = rng.standard_normal((n, nd)) * 0.1
    eps = 2.0 ** -17
    J, A, cnt = reference_jacobian(n, nd, c["X"], c["springs"], None, None, 1.0, 0.0)
    Y = _matvec_longdouble(n, nd, J, V)
    Fp = reference_force(n, nd, c["X"] + eps * V, c["springs"], accumulate=False)
    Fm = reference_force(n, nd, c["X"] - eps * V, c["springs"], accumulate=False)
    fd = (Fp.astype(np.longdouble) - Fm.astype(np.longdouble)) / (2 * eps)
    trunc = np.zeros(n)
    S = np.zeros(n)
    terms = np.zeros(n)
    for k in range(m.size):
        w = np.linalg.norm(V[s[k]] - V[m[k]])
        R = np.linalg.norm(c["X"][s[k]] - c["X"][m[k]])
        Rmin = R - eps * w
        t = eps ** 2 / 6.0 * 15.0 * kappa[k] * rest[k] * w ** 3 / Rmin ** 3
        for i in (m[k], s[k]):
            trunc[i] += t
            S[i] += kappa[k] * (R + eps * w + rest[k]) * (1.0 + (np.abs(c["X"]).max() + eps) / Rmin)
            terms[i] += 1
            trunc[i] += 28 * U * kappa[k] * (abs(1.0 - rest[k] / R) + rest[k] / R) * (np.abs(V[s[k]]).sum()
                                                                                     + np.abs(V[m[k]]).sum())
    bound = (trunc + (terms + 14) * U * S / eps)[:, None] + _jac_error(n, nd, A, cnt, V)
    err = np.abs(np.asarray(Y - fd, dtype=np.float64))
    print(f"springs: max error {err.max():.3e}, max |J V| {np.abs(np.asarray(Y, dtype=float)).max():.3e}, "
          f"largest bound {bound.max():.3e}")
    assert (err <= bound).all()
    assert err.max() < 1e-4 * np.abs(np.asarray(Y, dtype=float)).max()  # and the bound means agreement


def test_last_bit_asymmetry_pins_the_transposition():
    """(a D[i]) D[j] does not commute under rounding: for D = (0.1, 0.2, 0.3), kappa = 10,
    L = 0.05 the reference's dF(2, 1) and dF(1, 2) differ in the last bit.  MatSetValuesBlocked
    reads Eigen's column-major dF.data() row-major, so the stored (r, c) is dF(c, r)."""
    dF = spring_dF([0.1, 0.2, 0.3], 10.0, 0.05, 1.0)
    assert dF[2][1] != dF[1][2]
    assert 0.0 < abs(dF[2][1] - dF[1][2]) <= 2.0 * math.ulp(dF[2][1])
    blk = stored_block(dF)
    assert blk[1 * 3 + 2] == dF[2][1] and blk[2 * 3 + 1] == dF[1][2]
    # and through the assembly: block (0, 1) of a single spring holds the transposed storage
    X = np.array([[0.0, 0.0, 0.0], [0.1, 0.2, 0.3]])
    J, _, _ = reference_jacobian(2, 3, X, ([0], [1], [10.0], [0.05]))
    assert J[(0, 1)][1 * 3 + 2] == dF[2][1] and J[(0, 1)][1 * 3 + 2] != J[(0, 1)][2 * 3 + 1]
    assert J[(0, 0)] == [b * -1.0 for b in J[(0, 1)]] and J[(1, 0)] == J[(0, 1)]


def test_eigen_norm_sums_halves_first():
    """(2^27, 1.5, 1.5): x^2 + (y^2 + z^2) = 2^54 + 4.5 rounds to 2^54 + 4, the left-to-right
    sum rounds 2^54 + 2.25 up to 2^54 + 4 and then 2^54 + 6.25 up to 2^54 + 8; the square roots
    differ in the last bit."""
    D = [2.0 ** 27, 1.5, 1.5]
    halves = math.sqrt(D[0] * D[0] + (D[1] * D[1] + D[2] * D[2]))
    left = math.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
    assert halves != left
    assert eigen_norm(D) == halves == 2.0 ** 27
    assert eigen_norm([3.0, 4.0]) == 5.0


def test_preallocation_counts():
    """d_nnz + o_nnz is at least the true block count of every row, whatever the split into
    local and ghost nodes; a 1-D chain's values by hand."""
    for ndim in (2, 3):
        c = _random_case(ndim)
        n = c["n"]
        J, _, _ = reference_jacobian(n, ndim, c["X"], c["springs"], c["beams"], c["targets"])
        rowptr, col, _ = bsr_arrays(n, ndim, J)
        true = np.diff(rowptr)
        for n_local in (n, n - 7, 0):
            d, o = reference_nnz(n, n_local, c["springs"], c["beams"])
            assert ((d + o) >= true).all()
            if n_local == n:
                assert not o.any()
    # a chain 0 - 1 - 2 - 3 - 4: springs (i, i + 1), beams on 1, 2, 3 (next i + 1, prev i - 1)
    i = np.arange(4)
    j = np.arange(1, 4)
    springs, beams = (i, i + 1), (j, j + 1, j - 1)
    d, o = reference_nnz(5, 5, springs, beams)
    # base 1; a spring adds 1 at each end; a beam adds 2 at its three nodes
    assert d.tolist() == [1 + 1 + 2, 1 + 2 + 4, 1 + 2 + 6, 1 + 2 + 4, 1 + 1 + 2] and not o.any()
    d, o = reference_nnz(5, 4, springs, beams)  # node 4 is a ghost
    # spring (3, 4) has a ghost slave: 1 at nodes 3 and 4 of o_nnz.  Beam 3 (next 4 ghost, prev 2
    # local): d_nnz 1 at master 3 and prev 2; o_nnz 1 at master 3, 2 at next 4, 1 at prev 2
    assert d.tolist() == [1 + 1 + 2, 1 + 2 + 4, 1 + 2 + 4 + 1, 1 + 1 + 2 + 1, 1]
    assert o.tolist() == [0, 0, 1, 1 + 1, 1 + 2]
    J, _, _ = reference_jacobian(5, 2, np.arange(10.0).reshape(5, 2) ** 1.5, (i, i + 1, np.ones(4), np.ones(4)),
                                 (j, j + 1, j - 1, np.ones(3), np.zeros((3, 2))))
    assert np.diff(bsr_arrays(5, 2, J)[0]).tolist() == [3, 4, 5, 4, 3]


def test_repeated_entries_merge_and_isolated_nodes_keep_a_zero_diagonal():
    X = np.array([[0.0, 0.0], [1.0, 0.5], [2.0, -0.5], [5.0, 5.0]])
    springs = ([0, 0, 1], [1, 1, 2], [2.0, 2.0, 3.0], [0.5, 0.5, 0.25])  # a repeated edge
    beams = ([1], [2], [0], [0.75], [[0.0, 0.0]])  # shares (1, 2) and (0, 1) with the springs
    J, A, cnt = reference_jacobian(4, 2, X, springs, beams)
    rowptr, col, val = bsr_arrays(4, 2, J)
    assert rowptr.tolist() == [0, 3, 6, 9, 10] and col.tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 3]
    assert cnt[(0, 1)] == 3 and cnt[(0, 0)] == 3 and cnt[(3, 3)] == 0
    assert val[9].view(np.int64).tolist() == [[0, 0], [0, 0]]  # +0.0 in every word
    # a beam with next == prev: four calls of one value on (p, p), two on (p, m) and (m, p)
    J, _, cnt = reference_jacobian(3, 2, X[:3], None, ([1], [2], [2], [0.75], [[0.0, 0.0]]), X_coef=0.3)
    a = -1.0 * 0.75 * 0.3
    assert sorted(J) == [(0, 0), (1, 1), (1, 2), (2, 1), (2, 2)]
    assert cnt[(2, 2)] == 4 and J[(2, 2)][0] == ((a + a) + a) + a and J[(2, 2)][1] == 0.0
    assert cnt[(1, 2)] == 2 and cnt[(2, 1)] == 2 and J[(1, 1)][3] == -4.0 * 0.75 * 0.3


@pytest.fixture(scope="module")
def lib():
    from ibamr_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ibamr_amd import build
        build.build()
    return _lib.load()


def test_argument_errors_before_any_device_call(lib):
    """Null handles and null outputs are refused with IBTK_LE_ERR_ARG (4) and a message before
    anything touches a device."""
    import ctypes
    h = ctypes.c_void_p()
    nb = ctypes.c_longlong()
    out = (ctypes.c_longlong * 6)()
    calls = [
        lambda: lib.ibtk_le_forcejac_create(None, None, ctypes.byref(h)),
        lambda: lib.ibtk_le_forcejac_create(None, None, None),
        lambda: lib.ibtk_le_forcejac_rebuild(None, None),
        lambda: lib.ibtk_le_forcejac_assemble(None, None, None, None, 1.0, 0.0),
        lambda: lib.ibtk_le_forcejac_apply(None, None, None, None, 0),
        lambda: lib.ibtk_le_forcejac_pattern(None, ctypes.byref(nb), None, None, None),
        lambda: lib.ibtk_le_forcejac_read(None, None, None, None, 0),
        lambda: lib.ibtk_le_forcejac_stats(None, out),
        lambda: lib.ibtk_le_forcegen_linearized(None, None, None, None, None, 1.0, 0.0, None, 0),
        lambda: lib.ibtk_le_forcegen_jacobian_nnz(None, None, 0, None, None),
    ]
    for call in calls:
        assert call() == 4
        assert b"null" in lib.ibtk_le_last_error()
    assert lib.ibtk_le_forcejac_destroy(None) == 0


def test_python_argument_errors_without_a_device():
    from ibamr_amd import forcegen
    assert {"ForceJacobian", "ForceGen"} <= set(forcegen.__all__)
    for name in ("rebuild", "assemble", "apply", "bsr", "read", "stats"):
        assert callable(getattr(forcegen.ForceJacobian, name))
    assert callable(forcegen.ForceGen.linearized) and callable(forcegen.ForceGen.jacobian_nnz)

"""The z-slab migration kernels restated in numpy (helper, not a test file; numpy only).

k_slab_update, k_slab_partition, k_mig_pack and k_mig_unpack (ibamr_amd/csrc/le_aux.hip)
update the marker positions, wrap them into the periodic box, class every marker by the
rank that owns its wrapped z cell, partition the rows stably by class and move the leavers
through fixed-size buffers.  Every step is exact arithmetic on doubles and integers, so the
restatement here gives the same bits and the GPU test (tests/test_gpu_slab_migrate.py)
compares with it bit for bit.  `edge_rows` builds the positions at which the wrap and the
owner can go wrong: the box's ends, the slab faces and their neighbours in the doubles.
"""
import numpy as np

BLOCK = 256  # rows per workgroup of the kernels (le_internal.h)
WAVE = 64


def update(scheme, dt, X, U0, U1=None):
    """eulerStep / midpointStep: dt * U0 + X; trapezoidalStep: (h * U0 + X) + h * U1 with
    h = dt / 2; every product and sum rounded (the library is built without contraction)."""
    if scheme == "trapezoidal":
        h = 0.5 * dt
        return (h * U0 + X) + h * U1
    return dt * U0 + X


def wrap(x, L):
    """x into [0, L) as torch.remainder does it: fmod, + L if the result is non-zero and
    negative, then - L if it reached L (a tiny negative x rounds to L)."""
    r = np.fmod(x, L)
    r = np.where((r != 0.0) & (r < 0.0), r + L, r)
    return np.where(r >= L, r - L, r)


def owner(wz, Lz, Nz, P):
    """The rank owning wrapped z: the clamped cell floor(wz / (Lz / Nz)) over Nz / P."""
    dz = Lz / Nz
    cz = np.clip(np.floor(wz / dz).astype(np.int64), 0, Nz - 1)
    return cz // (Nz // P)


def classes(own, P, rank):
    """0 stays, 1 to (rank - 1) % P, 2 to (rank + 1) % P, 3 further -- in that precedence, so
    with P = 2 the one neighbour is class 1 and with P = 1 everything stays."""
    down, up = (rank - 1) % P, (rank + 1) % P
    return np.where(own == rank, 0, np.where(own == down, 1, np.where(own == up, 2, 3)))


def partition(cls):
    """(order, counts): the rows stably partitioned [0 | 1 | 2 | 3], and the class counts."""
    order = np.argsort(cls, kind="stable").astype(np.int32)
    return order, np.bincount(cls, minlength=4).astype(np.int32)


def update_partition(scheme, dt, X, U0, L, Nz, P, rank, U1=None, n=None):
    """slab_update_partition over the first n rows (all by default): (X_new, order, counts, class)."""
    n = X.shape[0] if n is None else n
    L = np.asarray(L, dtype=np.float64)
    Xn = wrap(update(scheme, dt, X[:n], U0[:n], None if U1 is None else U1[:n]), L)
    cls = classes(owner(Xn[:, 2], L[2], Nz, P), P, rank)
    order, counts = partition(cls)
    return Xn, order, counts, cls


def pack(rows, order, counts):
    """(send_down, send_up): the class-1 and class-2 rows in partition order."""
    n0, n1, n2 = (int(c) for c in counts[:3])
    return rows[order[n0:n0 + n1]], rows[order[n0 + n1:n0 + n1 + n2]]


def unpack(rows, order, counts, from_down, from_up):
    """The stayers in partition order, then the arrivals from below, then from above."""
    return np.concatenate([rows[order[:int(counts[0])]], from_down, from_up], axis=0)


def edge_values(L):
    """Positions at which the wrap's branches switch, for a box length L."""
    return np.array([0.0, -0.0, L, -L, 2 * L, np.nextafter(L, 0.0), np.nextafter(L, np.inf), -5e-324, -1e-17 * L,
                     1e6 * L + 0.3 * L, -(1e6 * L + 0.3 * L)])


def face_values(Lz, Nz, P):
    """z at every slab face k (Nz / P) dz, k = 0 .. P, and its two neighbours in the doubles."""
    dz = Lz / Nz
    f = np.arange(P + 1) * (Nz // P) * dz
    return np.concatenate([f, np.nextafter(f, -np.inf), np.nextafter(f, np.inf)])


def edge_rows(L, Nz, P, M, seed, far=True):
    """(X, U0, U1, dt): M rows drawn over the whole box -- every owner, so every class, mixed
    through every 256-row block and 64-row wave -- with real velocities of up to a tenth of
    a slab, with `far` a twentieth of them up to three slabs.  The edge rows (edge_count of
    them, as far as M allows; every third row while M has room) have U0 = U1 = 0, so X_new
    is X exactly, and hold per dim every edge value (z: the slab faces too) beside random
    coordinates in the other dims."""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.float64)
    dz = L[2] / Nz
    dt = 0.37
    slab = (Nz // P) * dz
    X = rng.uniform(0.0, 1.0, (M, 3)) * L  # over the whole box: every owner, so every class
    U0 = rng.uniform(-1.0, 1.0, (M, 3)) * 0.1 * slab / dt
    U1 = rng.uniform(-1.0, 1.0, (M, 3)) * 0.1 * slab / dt
    if far and M >= 20:
        sel = rng.permutation(M)[:max(M // 20, 2)]
        U0[sel, 2] = rng.uniform(-3.0, 3.0, sel.size) * slab / dt
    edges = []
    for d in range(3):
        v = edge_values(L[d])
        if d == 2:
            v = np.concatenate([v, face_values(L[2], Nz, P)])
        e = rng.uniform(0.0, 1.0, (v.size, 3)) * L
        e[:, d] = v
        edges.append(e)
    E = np.concatenate(edges)
    ne = min(E.shape[0], M)
    # the edge rows at a stride through the list (every third row while they last)
    at = (np.arange(ne) * 3) % M if M >= 3 * ne else np.arange(ne)
    X[at] = E[:ne]
    # a zero of X's sign: dt * (-0.0) + (-0.0) keeps the -0.0 that 0.0 + (-0.0) would lose
    U0[at] = np.where(np.signbit(X[at]), -0.0, 0.0)
    U1[at] = U0[at]
    return X, U0, U1, dt


def edge_count(Nz, P):
    """The number of edge rows edge_rows places (fewer when M is smaller)."""
    return 3 * edge_values(1.0).size + 3 * (P + 1)


def step_rows(L, Nz, P, rank, M, seed):
    """(X, U0, dt, F, ids) of rank `rank`: M markers inside its slab, velocities that carry
    about a tenth of them across a slab face (some across the periodic wrap) and none further."""
    rng = np.random.default_rng(seed + rank)
    L = np.asarray(L, dtype=np.float64)
    nz, dz = Nz // P, L[2] / Nz
    X = rng.uniform(0.0, 1.0, (M, 3)) * L
    X[:, 2] = (rank * nz + rng.uniform(0.0, nz, M)) * dz
    dt = 0.2 * nz * dz
    U0 = rng.uniform(-1.0, 1.0, (M, 3))  # |dt U0_z| <= a fifth of a slab: a tenth of the rows cross
    F = rng.standard_normal((M, 3))
    ids = (rank * M + np.arange(M)).astype(np.float64)
    return X, U0, dt, F, ids

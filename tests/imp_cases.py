"""The cases the IMP tests share (tests/test_imp_cpu.py checks their preconditions on the
CPU, tests/test_gpu_imp.py runs them on the device): geometries, list entries, fields and
the numpy restatement's answers, each computed once per process and left unchanged."""
from __future__ import annotations

import functools

import numpy as np

import imp_ref as ir

DX = (0.1, 0.037, 0.2113)
DX_POW2 = (0.125, 0.0625, 0.25)

# name: (ilower, n, dx, x_lower, ghost, pitched)
GEOMS = {
    "g4": ((-3, 5, 2), (19, 10, 21), DX, (0.3, -0.2, 0.1), 4, False),
    "g5p": ((-3, 5, 2), (19, 10, 21), DX, (0.3, -0.2, 0.1), 5, True),
    "pow2": ((-3, 5, 2), (19, 10, 21), DX_POW2, (0.5, -0.25, 1.0), 4, False),
    "2d": ((-3, 5), (23, 17), (0.1, 0.0625), (0.3, -0.25), 4, False),
}
CASES = tuple(GEOMS)
# the dense pair of cells: DENSE[0] points in one cell and DENSE[1] in its x-neighbour, so
# that a workgroup's loop over 64-entry chunks repeats
DENSE = (150, 70)


def geo_of(name):
    ilower, n, dx, xl, g, _ = GEOMS[name]
    return ir.Geo(ilower, n, dx, xl, g)


def entries(name):
    """About 700 positions: interior, ghost layer to its edge, half-cell lattice (exact ties
    in the cell frame and in every side frame where dx is a power of two), a dense pair."""
    geo = geo_of(name)
    nd = geo.ndim
    rng = np.random.default_rng(sum(map(ord, name)))
    xl, dx, n, g = np.array(geo.x_lower), np.array(geo.dx), np.array(geo.n), geo.g
    xu = xl + n * dx
    parts = [rng.uniform(xl, xu, (300, nd))]
    for d in range(nd):  # the outer 2.5 cells of the ghost layer, both sides: really clipped
        for side in (0, 1):
            P = rng.uniform(xl, xu, (30, nd))
            t = rng.uniform(0.0, 2.5, 30)
            t[0] = 1e-9  # (nearly) on the edge of the ghost box
            P[:, d] = xl[d] - (g - t) * dx[d] if side == 0 else xu[d] + (g - t) * dx[d]
            parts.append(P)
    # the half-cell lattice x_lower + (m / 2) dx, m odd: X_o_dx = k + 0.5 in the cell frame;
    # m even: in the side frame; the low ghost layer (k < 0) included
    m = np.stack([rng.integers(-2 * g + 1, 2 * (n[d] + g) - 1, 40) for d in range(nd)], axis=1)
    m[:8] = -1 - (np.arange(8) % 4)[:, None]  # k = -1: round(-0.5) = -1
    parts.append(xl + 0.5 * m * dx)
    cell = np.array([5, 4, 7][:nd])
    for k, cnt in enumerate(DENSE):
        lo = xl + (cell + np.eye(nd, dtype=int)[0] * k) * dx
        parts.append(lo + rng.uniform(0.02, 0.98, (cnt, nd)) * dx)
    return np.ascontiguousarray(np.concatenate(parts))


def sublist(n, seed=7):
    """A permuted sub-list with n_list < n and ten entries named twice."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(n)[:400]
    return np.concatenate([idx, idx[:10]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    geo = geo_of(name)
    nd = geo.ndim
    X = entries(name)
    n = X.shape[0]
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    u = [rng.standard_normal(geo.shape(c)) for c in range(nd)]
    tau = rng.standard_normal((n, nd * nd))
    wgt = rng.uniform(0.5, 1.5, n) * float(np.prod(geo.dx))
    U, G, clipped = ir.interp(geo, u, X)
    out = dict(name=name, geo=geo, X=X, u=u, tau=tau, wgt=wgt, U=U, GradU=G, clipped=clipped)
    for clip in ("patch", "ghost"):
        f, cnt, S = ir.spread(geo, geo.alloc(), tau, wgt, X, clip=clip, stats=True)
        out["f_" + clip], out["cnt_" + clip], out["S_" + clip] = f, cnt, S
    idx = sublist(n)
    Us, Gs, _ = ir.interp(geo, u, X, indices=idx, U=np.full((n, nd), -7.25), GradU=np.full((n, nd * nd), -7.25))
    fs, cs, Ss = ir.spread(geo, geo.alloc(), tau, wgt, X, indices=idx, clip="patch", stats=True)
    out.update(sub_idx=idx, sub_U=Us, sub_GradU=Gs, sub_f=fs, sub_cnt=cs, sub_S=Ss)
    return out


def exact_ties(geo, X):
    """Entries with X_o_dx - floor(X_o_dx) == 0.5 exactly in some dim: in the cell frame, and
    in the side frame of that dim."""
    cell = np.zeros(X.shape[0], bool)
    side = np.zeros(X.shape[0], bool)
    for d in range(geo.ndim):
        for frame, mask in ((geo.x_lower[d], cell), (geo.frame_lower(d, d), side)):
            q = (X[:, d] - frame) / geo.dx[d]
            mask |= (q - np.floor(q)) == 0.5
    return cell, side


def check_preconditions(c, ties):
    """Conditions on imp_ref alone, so that no test of the case passes vacuously."""
    geo = c["geo"]
    for d in range(geo.ndim):
        for side in (0, 1):
            assert c["clipped"][:, d, side].sum() >= 20, (d, side)
    if ties:
        cell, side = exact_ties(geo, c["X"])
        assert cell.sum() >= 10 and side.sum() >= 10
        q = (c["X"] - np.array(geo.x_lower)) / np.array(geo.dx)
        assert ((q == -0.5) & (ir.nint(q) == -1)).sum() >= 1  # round(-0.5) = -1
    for clip in ("patch", "ghost"):
        for a in range(geo.ndim):
            assert np.abs(c["f_" + clip][a]).max() > 0.0
            assert c["cnt_" + clip][a].max() >= DENSE[0]
    assert len(c["sub_idx"]) < c["X"].shape[0]


def spread_bound(cnt, S, q):
    """|f_dev - f_ref| <= (2 (n_i - 1) + q) 2^-53 S_i per point."""
    return (2.0 * np.maximum(cnt - 1, 0) + q) * 2.0 ** -53 * S

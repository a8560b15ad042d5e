"""The cases the fluid-source tests share (tests/test_sources_cpu.py checks their preconditions
on the CPU, tests/test_gpu_sources.py runs them on the device): geometries, sources, node
lists, fields and the numpy restatement's answers, each computed once per process and left
unchanged.  All inputs are seeded."""
from __future__ import annotations

import functools
import math

import numpy as np

import source_ref as sr

DX = (1.0 / 22.0, 1.0 / 16.0, 1.0 / 20.0)
RADII = (0.03, 0.08, 0.12, 0.2, 2.5 / 16.0)

# name: (ilower, n, dx, x_lower, ghost, pitched)
GEOMS = {
    "g3": ((-3, 5, 2), (24, 20, 18), DX, (-0.25, 0.5, 0.0), 2, False),
    "g3p": ((-3, 5, 2), (24, 20, 18), DX, (-0.25, 0.5, 0.0), 2, True),
    "g2": ((-3, 5), (24, 20), DX[:2], (-0.25, 0.5), 2, False),
}
# name: (geometry, what)
CASES = {
    "main": ("g3", "main"), "main_pitched": ("g3p", "main"), "clip": ("g3", "clip"), "many": ("g3", "many"),
    "many_pitched": ("g3p", "many"), "none": ("g3", "none"),
    "main2": ("g2", "main"), "clip2": ("g2", "clip"), "many2": ("g2", "many"),
}
UNCLIPPED = ("main", "main_pitched", "many", "many_pitched", "main2", "many2")
CLIPPED = ("clip", "clip2")
MANY = 70       # sources of the "many" cases: the staging of sources repeats past a chunk of 64
BIG = 257       # nodes of the largest source
MIN_WEIGHT = 1.0e-12  # a non-zero contribution weight times r0 r1 r2 is at least this


def geo_of(name):
    ilower, n, dx, xl, g, _ = GEOMS[name]
    return sr.Geo(ilower, n, dx, xl, g)


def half_widths(geo, r_src):
    return [int((max(math.floor(r_src / dx + 0.5), 2.0) * dx) / dx) + 1 for dx in geo.dx]


def interior_position(geo, rng, r_src):
    """A random position whose stencil box stays inside the patch box."""
    h = half_widths(geo, r_src)
    cell = [rng.integers(geo.ilower[d] + h[d], geo.iupper[d] - h[d] + 1) for d in range(geo.ndim)]
    return [geo.x_lower[d] + (cell[d] - geo.ilower[d] + rng.uniform(0.05, 0.95)) * geo.dx[d] for d in range(geo.ndim)]


def sources(gname, what, seed):
    """(r_src, X_src, Q): the radii, positions and strengths of a case."""
    geo = geo_of(gname)
    nd = geo.ndim
    rng = np.random.default_rng(seed)
    xl, dx = geo.x_lower, geo.dx
    pos = lambda cell, frac: [xl[d] + (cell[d] + frac[d]) * dx[d] for d in range(nd)]  # noqa: E731
    r, X, Q = [], [], []
    if what in ("main", "clip"):
        r.append(0.2)              # every coordinate a cell centre: R differs per dimension
        X.append(pos((9, 8, 7), (0.5, 0.5, 0.5)))
        r.append(2.5 / 16.0)       # every coordinate a cell face (the getCellIndex tie); floor(2.5 + 0.5) in y
        X.append(pos((14, 11, 9), (0.0, 0.0, 0.0)))
        r.append(0.12)             # a centre, a face and a general coordinate
        X.append(pos((8, 12, 8), (0.5, 0.0, 0.37)))
        a = interior_position(geo, rng, 0.2)   # two heavily overlapping boxes, strengths of opposite sign
        r += [0.2, 0.08]
        X += [a, [a[d] + 0.6 * dx[d] for d in range(nd)]]
        r.append(0.03)             # R clamped to 2 in every dimension
        X.append(interior_position(geo, rng, 0.03))
        Q = [1.3, -0.7, 0.45, 2.1, -1.9, 0.8]
        if what == "clip":         # within R cells of the lower x and the upper y face: the box is cut
            r.append(0.2)
            X.append(pos((1, geo.n[1] - 2, 8), (0.3, 0.6, 0.4)))
            Q.append(1.1)
    elif what == "many":
        for _ in range(MANY):
            r.append(float(rng.choice([0.03, 0.08, 0.12])))
            X.append(interior_position(geo, rng, r[-1]))
        Q = list(rng.uniform(0.2, 1.5, MANY) * rng.choice([-1.0, 1.0], MANY))
    n = len(r)
    return np.array(r, dtype=np.float64), np.array(X, dtype=np.float64).reshape(n, nd), np.array(Q, dtype=np.float64)


def domain_of(geo, larger=False):
    """The patch box as the domain; larger: a domain that extends past the patch in the
    upper y (in 2-D: upper x) and both last-dimension directions, so that only some of its
    boundary cells lie in the patch."""
    lo, hi = list(geo.ilower), list(geo.iupper)
    if larger:
        hi[geo.ndim - 2] += 3
        lo[geo.ndim - 1] -= 4
        hi[geo.ndim - 1] += 2
    return tuple(lo), tuple(hi)


def node_lists(nd, seed=11):
    """Nodes for the locations test: X [n_nodes][nd], and (node, source) pairs in a shuffled
    order: source 0 has one node, source 1 has BIG, source 2 none, source 3 forty, and some
    nodes carry no source."""
    rng = np.random.default_rng(seed)
    n_nodes = 1 + BIG + 40 + 25
    X = rng.uniform(-1.0, 2.0, (n_nodes, nd))
    ids = rng.permutation(n_nodes)
    node = np.concatenate([ids[:1], ids[1:1 + BIG], ids[1 + BIG:1 + BIG + 40]]).astype(np.int32)
    source = np.concatenate([np.zeros(1), np.ones(BIG), np.full(40, 3)]).astype(np.int32)
    o = rng.permutation(node.size)
    return X, node[o], source[o], 4


def check_weights(geo, r_src, X_src):
    """The condition the bounds rest on: every (source, cell) weight times r0 r1 r2 is exactly
    0 or at least MIN_WEIGHT.  Returns the smallest non-zero one."""
    smallest = math.inf
    for n in range(len(r_src)):
        X = [float(v) for v in X_src[n]]
        st = sr.stencil(geo, float(r_src[n]), X)
        per_dim = []
        for d in range(geo.ndim):
            w = [sr.weight_1d(geo, st, X, d, i) * st[d]["r"] for i in range(st[d]["lo"], st[d]["hi"] + 1)]
            per_dim.append([v for v in w if v != 0.0])
        if all(per_dim):
            smallest = min(smallest, math.prod(min(w) for w in per_dim))
    assert smallest >= MIN_WEIGHT, f"a non-zero weight of {smallest:.3e}: change the seed"
    return smallest


@functools.lru_cache(maxsize=None)
def case(name):
    gname, what = CASES[name]
    geo = geo_of(gname)
    seed = 100 + sum(map(ord, what)) + geo.ndim
    r_src, X_src, Q = sources(gname, what, seed)
    rng = np.random.default_rng(seed + 1)
    q0 = rng.standard_normal(geo.shape())   # the spread accumulates: a non-zero start
    p = rng.standard_normal(geo.shape())
    out = dict(name=name, geo=geo, pitched=GEOMS[gname][5], r_src=r_src, X_src=X_src, Q=Q, q0=q0, p=p)
    q, cnt, S = sr.spread(geo, q0.copy(), X_src, r_src, Q, stats=True)
    out.update(q=q, cnt=cnt, S=S)
    out["q_zero"] = sr.spread(geo, geo.alloc(), X_src, r_src, Q)  # into a zero field: the identities
    dom = domain_of(geo)
    qn = out["q_zero"].copy()  # the consistency test compares the integral of what was spread with sum Q
    totals, flagged = sr.normalize(geo, qn, Q, dom, True)
    out.update(domain=dom, q_norm=qn, totals=totals, flagged=flagged)
    P, _, m, A = sr.pressure(geo, p, X_src, r_src, None, stats=True)
    big = domain_of(geo, larger=True)
    out.update(P=P, P_cells=m, P_abs=A, domain_big=big, P_normed=sr.pressure(geo, p, X_src, r_src, big),
               p_norm=sr.pressure_norm(geo, p, big))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def spread_bound(cnt, S, C_w):
    """|q_dev - q_ref| <= (3 C_w + 2 (n_i - 1) + 4) 2^-53 S_i: each of the three 1-D weights of
    a contribution is within C_w 2^-53 / r_d of the restatement's; forming the product and
    Q wgt is the same four roundings on both sides, and the n_i - 1 additions (and the one to
    the initial value) each round once on either side."""
    return (3.0 * C_w + 2.0 * np.maximum(cnt - 1, 0) + 4.0) * 2.0 ** -53 * S


def pressure_bound(m, A, C_w):
    """The spread bound's analogue: m cells of the clipped box, A = sum |p| over them, with
    dx_d / r_d <= 1/2 folded in as 1."""
    return (3.0 * C_w + 2.0 * np.maximum(m - 1, 0) + 4.0) * 2.0 ** -53 * A

"""The cases the flow-meter tests share (tests/test_instrument_cpu.py checks their preconditions
on the CPU, tests/test_gpu_instruments.py runs them on the device): the 24 x 20 x 18 patch of
source_cases.py with its shifted lower corner and unequal dx (h_finest = min(dx) = dx[0]), the
meters, the fields and the restatement's answers, each computed once per process and left
unchanged.  All inputs are seeded.

The restatement reads one ghost layer, so its answers are computed on arrays of ghost width 1
and hold for every layout the device tests run (packed and pitched, ghost width 1 and 3): a
wider array carries the same values in its first layer and NaN beyond.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import instrument_ref as ir
from source_cases import DX

ILOWER, N, X_LOWER = (-3, 5, 2), (24, 20, 18), (-0.25, 0.5, 0.0)
H = min(DX)
GEO = ir.Geo(ILOWER, N, DX, X_LOWER, 1)
LAYOUTS = {"packed_g1": (1, False), "pitched_g1": (1, True), "packed_g3": (3, False), "pitched_g3": (3, True)}

# name: (perimeter nodes, centre, radius in units of H, normal, out-of-plane perturbation in units of H)
METERS = {
    # r_max <= h: two web nodes a spoke
    "tri": (3, (0.2, 0.9, 0.3), 0.9, (0.3, 0.2, 1.0), 0.0),
    "quad": (4, (0.5, 1.3, 0.6), 0.8, (1.0, 0.4, 0.2), 0.1),
    # r_max about 6.3 h: 14; slightly non-planar
    "ring17": (17, (0.3, 1.1, 0.45), 6.3, (0.2, 1.0, 0.3), 0.1),
    # more perimeter nodes than a wave, 16 web nodes: 1120 web patches, more than 1024; shares cells with ring17
    "ring70": (70, (0.31, 1.12, 0.46), 7.6, (0.1, 1.0, -0.2), 0.0),
    # a square in the plane of the cell faces z = 7 dz: every web centroid's z is exactly that face
    "tie_z": (4, (0.3, 1.0, 7 * DX[2]), 2.2, (0.0, 0.0, 1.0), 0.0),
    # a square in the plane of the cell centres y = 0.5 + 6.5 dy (dy = 2^-4: exact): the X < X_cell tie
    "tie_y": (4, (0.55, 0.5 + 6.5 * DX[1], 0.5), 1.7, (0.0, 1.0, 0.0), 0.0),
    # cut by the lower x face and the upper y face of the patch
    "cut": (12, (X_LOWER[0] + 1.1 * H, X_LOWER[1] + N[1] * DX[1] - 0.06, 0.5), 3.2, (0.05, 0.05, 1.0), 0.1),
    # the centroid outside the box, half the web inside
    "outside": (8, (X_LOWER[0] - 0.02, 1.0, 0.4), 3.0, (0.0, 1.0, 0.2), 0.0),
}
# name: (meters, U: "random" / "zero")
CASES = {
    "small": (("tri", "quad"), "random"),
    "big": (("ring17",), "random"),
    "wave": (("ring70",), "random"),
    "tie": (("tie_z", "tie_y"), "random"),
    "cut": (("cut",), "random"),
    "cut_u0": (("cut",), "zero"),
    "outside": (("outside",), "random"),
    "shared": (("ring17", "ring70"), "random"),
    "eight": (tuple(METERS), "random"),
    "none": ((), "random"),
}
# the seed of each case's u and p: the first of 0, 1, ... for which the reference-order total of some
# meter differs in bits from its (m, n)-order total (test_instrument_cpu.py checks that it does)
FIELD_SEED = {name: 0 for name in CASES}
SPARE_NODES = 5  # markers that lie on no meter


def perimeter(name):
    """The perimeter nodes of a meter: a regular polygon about `centre` in the plane with
    `normal` (tie_z, tie_y: a square with its corners on exact coordinates), every other node
    moved out of the plane by `bump` h."""
    P, centre, r, normal, bump = METERS[name]
    c = np.array(centre, dtype=np.float64)
    nv = np.array(normal, dtype=np.float64)
    nv /= np.linalg.norm(nv)
    a = np.cross(nv, [1.0, 0.0, 0.0] if abs(nv[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nv, a)
    if name.startswith("tie"):
        # corners c +- s e1 +- s e2 with s a multiple of 2^-6 and the in-plane axes the grid's
        s = math.floor(r * H / math.sqrt(2.0) * 64.0) / 64.0
        e = [d for d in range(3) if normal[d] == 0.0]
        X = np.tile(c, (4, 1))
        for k, (s1, s2) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
            X[k, e[0]] += s1 * s
            X[k, e[1]] += s2 * s
        return X
    th = 2.0 * np.pi * (np.arange(P) + 0.25) / P
    X = c + r * H * (np.cos(th)[:, None] * a + np.sin(th)[:, None] * b)
    X[1::2] += bump * H * nv
    return X


@functools.lru_cache(maxsize=None)
def structure(names):
    """(X [n_nodes][3], meters: the local nodes of each meter's perimeter positions, and the
    (node, meter, meter_node) triples in a shuffled order)."""
    rng = np.random.default_rng(7 + len(names))
    pts = [perimeter(n) for n in names]
    total = sum(len(p) for p in pts) + SPARE_NODES
    ids = rng.permutation(total)
    X = rng.uniform(0.1, 0.8, (total, 3))
    meters, node, meter, meter_node, k = [], [], [], [], 0
    for l, p in enumerate(pts):
        mine = ids[k:k + len(p)]
        k += len(p)
        X[mine] = p
        meters.append([int(v) for v in mine])
        node += list(mine)
        meter += [l] * len(p)
        meter_node += list(range(len(p)))
    o = rng.permutation(len(node))
    as32 = lambda a: np.array(a, dtype=np.int32)[o]  # noqa: E731
    X.setflags(write=False)
    return X, meters, (as32(node), as32(meter), as32(meter_node))


def fields(seed, g=1):
    """(u: three side arrays, p: the cell array) of ghost width g: seeded standard normals in
    the first ghost layer and inside, NaN beyond."""
    rng = np.random.default_rng(1000 + seed)
    geo1 = GEO
    u1 = [rng.standard_normal(s) for s in ir.side_shapes(geo1)]
    p1 = rng.standard_normal(geo1.shape())
    if g == 1:
        return u1, p1
    k = g - 1
    wide = lambda a: np.pad(a, k, constant_values=np.nan)  # noqa: E731
    return [wide(a) for a in u1], wide(p1)


@functools.lru_cache(maxsize=None)
def webs_of(names):
    X, meters, _ = structure(names)
    return ir.update(GEO, X, meters)


@functools.lru_cache(maxsize=None)
def case(name):
    names, Ukind = CASES[name]
    X, meters, triples = structure(names)
    webs = webs_of(names)
    seed = FIELD_SEED[name]
    u, p = fields(seed)
    rng = np.random.default_rng(2000 + seed)
    U = rng.standard_normal(X.shape) if Ukind == "random" else np.zeros(X.shape)
    touched = ([np.zeros(a.shape, bool) for a in u], np.zeros(p.shape, bool))
    values, stats = ir.read(GEO, webs, u, p, U, meters, touched=touched)
    out = dict(name=name, names=names, geo=GEO, X=X, meters=meters, triples=triples, webs=webs, seed=seed, u=u, p=p, U=U,
               values=values, stats=stats, touched=touched,
               values_no_u=ir.read(GEO, webs, None, p, U, meters)[0], values_no_p=ir.read(GEO, webs, u, None, U, meters)[0],
               cap=max([w["nw"] for w in webs] + [2]))
    for v in [X, U, p, values, *u, *touched[0], touched[1]]:
        v.setflags(write=False)
    return out


def on_face(X, d):
    """X is exactly a face coordinate x_lower[d] + k dx[d] of the patch's grid."""
    k = round((X - X_LOWER[d]) / DX[d])
    return X_LOWER[d] + k * DX[d] == X


def on_centre(X, d):
    k = math.floor((X - X_LOWER[d]) / DX[d])
    return X_LOWER[d] + DX[d] * (float(k) + 0.5) == X

"""Cases of the physical-boundary operator on side data, shared by the CPU pin
(test_bdry_ref_pin.py: le_bdry_oracle.c against the compiled reference Fortran) and the
GPU pin (test_gpu_bdry.py: ibtk_le_phys_bdry_side against both).  Plain data and seeded
input makers; nothing here needs a GPU or the reference.

Every case is one tiny patch and one call.  A patch's cases are walked inside one test
function (``cases(patch)``), not parametrised one by one.

Patches ``(lo, hi, g)``:

* the six of test_gpu_bdry.py's ``CASES``;
* narrow ones, fewer cells than ghost cells in some or every dimension: there the
  mirror-image "interior" point of a ghost point lies in the opposite ghost region, and
  both ends of a dimension meet in one row;
* 3 x 2 x 2 cells with g = 16, the largest ghost width ibtk_le_phys_bdry_side takes;
* 48 x 40 x 32 (and 64 x 64), whose faces hold more lines than one block has threads.

Face patterns: every subset of the faces (16 in 2-D, 64 in 3-D) on the narrow and the small
patches, the four named ones of test_gpu_bdry.py on the two large ones.  A subset decides
which edges and corners exist, so "every subset" is also every set of edges and corners.

Coefficients ``A, B, G[component, face]``, G never 0:

* ``robin`` (every b in [0.5, 2]), ``dirichlet`` (every b = 0), ``mixed`` (lower faces
  Dirichlet, upper faces Robin), as test_gpu_bdry.py draws them;
* ``thr0`` .. ``thr7``: a = 1 and b out of ``THRESHOLD_B`` = 0, +-9e-13, +-1e-12,
  +-1.1e-12, -0.7, the values on either side of and exactly at the reference's
  ``abs(b) .lt. 1.d-12``; entry (component c, face loc) of set k takes
  ``THRESHOLD_B[(k + c * 2 ndim + loc) % 8]``, so each set mixes Dirichlet and Robin faces
  and over the eight sets every entry takes every value.  Run with every face physical.

Families: ``random`` (standard normal everywhere; fill and adjoint) and ``nan_ghost`` (fill
only, ``mixed`` coefficients, every pattern): every point outside the patch's own side box
starts NaN, so a ghost point that the fill does not write, or writes from a ghost point not
yet written, shows as NaN.  Compare with ``same_bits_or_nan``.
"""
import itertools
import zlib

import numpy as np

# (lo, hi, g, which patterns)
SMALL = [
    ([0, 0], [6, 5], 2),
    ([2, -1], [9, 6], 1),
    ([0, 0, 0], [5, 4, 6], 2),
    ([1, 0, -2], [6, 6, 3], 3),
]
NARROW = [
    ([0, 0], [0, 0], 3),
    ([2, -1], [3, -1], 4),
    ([0, 0, 0], [0, 1, 2], 4),
    ([3, -1, 0], [3, -1, 0], 2),
]
CAP = [([0, 0, 0], [2, 1, 1], 16)]
LARGE = [
    ([0, 0], [63, 63], 3),
    ([0, 0, 0], [47, 39, 31], 4),
]
MAX_GHOST = 16  # ibtk_le_phys_bdry_side refuses more

NAMED = {
    "all": [1, 1, 1, 1, 1, 1],
    "walls_y": [0, 0, 1, 1, 0, 0],
    "mixed": [1, 0, 0, 1, 1, 1],
    "one": [0, 0, 0, 0, 0, 1],
}
KINDS = ["robin", "dirichlet", "mixed"]
THRESHOLD_B = [0.0, 9e-13, -9e-13, 1e-12, -1e-12, 1.1e-12, -1.1e-12, -0.7]
THRESHOLD_KINDS = [f"thr{k}" for k in range(len(THRESHOLD_B))]
DX = [0.1, 0.13, 0.07]  # anisotropic: dx(location_index/NDIM) picks a different one


def _patch(lo, hi, g, every):
    return dict(lo=lo, hi=hi, g=g, every_pattern=every, id="x".join(str(h - l + 1) for l, h in zip(lo, hi)) +
                f"_lo{'.'.join(map(str, lo))}_g{g}")


PATCHES = [_patch(*p, True) for p in SMALL + NARROW + CAP] + [_patch(*p, False) for p in LARGE]
ALL_PATTERN_PATCHES = [p for p in PATCHES if p["every_pattern"]]
PATCH_IDS = [p["id"] for p in PATCHES]


def dx_of(patch):
    return DX[:len(patch["lo"])]


def patterns(patch):
    """[(name, phys)]: phys[2 d + upper] per face."""
    nd = len(patch["lo"])
    if not patch["every_pattern"]:
        return [(name, p[:2 * nd]) for name, p in NAMED.items()]
    return [("".join(map(str, bits)), list(bits)) for bits in itertools.product((0, 1), repeat=2 * nd)]


def seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def side_shape(lo, hi, g, axis):
    """numpy shape (C order, x last) of the ghosted side array of `axis`."""
    nd = len(lo)
    return tuple(hi[d] - lo[d] + 1 + 2 * g + (1 if d == axis else 0) for d in reversed(range(nd)))


def own_mask(lo, hi, g, axis):
    """True at the patch's own side points of `axis` (both boundary faces of the normal
    direction included): every index within [lo, hi (+1 along axis)]."""
    nd = len(lo)
    shp = side_shape(lo, hi, g, axis)
    m = np.ones(shp, dtype=bool)
    for d in range(nd):
        ax = nd - 1 - d
        n = hi[d] - lo[d] + 1 + (1 if d == axis else 0)
        idx = np.arange(shp[ax])
        sl = [None] * nd
        sl[ax] = slice(None)
        m &= ((idx >= g) & (idx < g + n))[tuple(sl)]
    return m


def coefs(patch, kind):
    """(A, B, G), each (ndim, 2 ndim) = [component, face]; one draw per (patch, kind)."""
    nd = len(patch["lo"])
    rng = np.random.default_rng(seed("coef", patch["id"], kind))
    A = rng.uniform(0.5, 2.0, (nd, 2 * nd))
    B = rng.uniform(0.5, 2.0, (nd, 2 * nd))
    G = rng.uniform(0.25, 1.0, (nd, 2 * nd)) * rng.choice([-1.0, 1.0], (nd, 2 * nd))
    if kind == "dirichlet":
        B[:] = 0.0
    elif kind == "mixed":
        B[:, ::2] = 0.0
    elif kind in THRESHOLD_KINDS:
        k = THRESHOLD_KINDS.index(kind)
        A[:] = 1.0
        for c in range(nd):
            for loc in range(2 * nd):
                B[c, loc] = THRESHOLD_B[(k + c * 2 * nd + loc) % len(THRESHOLD_B)]
    elif kind != "robin":
        raise ValueError(kind)
    assert np.all(G != 0.0)
    return A, B, G


def inputs(patch, family):
    """Fresh side arrays of the patch; one draw per (patch, family)."""
    lo, hi, g = patch["lo"], patch["hi"], patch["g"]
    rng = np.random.default_rng(seed("u", patch["id"], family))
    us = [rng.standard_normal(side_shape(lo, hi, g, a)) for a in range(len(lo))]
    if family == "nan_ghost":
        for a, u in enumerate(us):
            u[~own_mask(lo, hi, g, a)] = np.nan
    elif family != "random":
        raise ValueError(family)
    return us


def cases(patch):
    """[(family, pattern name, phys, kind, adjoint)] of one patch."""
    nd = len(patch["lo"])
    out = []
    for name, phys in patterns(patch):
        for kind in KINDS:
            for adjoint in (False, True):
                out.append(("random", name, phys, kind, adjoint))
    for kind in THRESHOLD_KINDS:
        for adjoint in (False, True):
            out.append(("random", "all", [1] * (2 * nd), kind, adjoint))
    for name, phys in patterns(patch):
        out.append(("nan_ghost", name, phys, "mixed", False))
    return out


def label(patch, case):
    family, name, _, kind, adjoint = case
    return f"patch {patch['id']} pattern {name} kind {kind} mode {'adjoint' if adjoint else 'fill'} family {family}"


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(got, want):
    """Indices where the two arrays differ in any bit (empty: equal)."""
    return np.argwhere(bits(got) != bits(want))


def same_bits_or_nan(got, want):
    """Indices where `want` is NaN and `got` is not, or `want` is a number and `got` has
    other bits.  NaN payloads and signs are not compared."""
    wn = np.isnan(want)
    return np.argwhere(np.where(wn, ~np.isnan(got), bits(got) != bits(want)))


def is_narrow(patch):
    """Some dimension has fewer cells than ghost cells (or fewer than 2)."""
    return any(h - l + 1 < max(patch["g"], 2) for l, h in zip(patch["lo"], patch["hi"]))

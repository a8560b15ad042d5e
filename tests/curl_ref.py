"""A numpy restatement of the side-centred curl, ``PatchMathOps::curl(side, side)``.

``curl_side_ref`` computes what ``ibtk_le_curl_side`` must give bit for bit: per component
two centred differences, each ``fac * (an eight-term sum)`` with ``fac = 0.125 / dx[d]``,
the sum taken left to right in the reference's operand order (``stoscurl3d``,
ibtk/src/math/fortran/curl3d.f.m4:457-559), their difference, then ``alpha * c`` rounded
once and, when accumulating, ``+ w`` rounded once.  numpy evaluates every slice operation
as one IEEE operation per element, so the restatement has the Fortran's roundings;
tests/golden/curl_side_ref.npz holds the compiled Fortran's own outputs to hold it to.

Arrays are the ghosted side arrays in torch / C order, ``a[z, y, x]``: array ``c`` covers
``ilower - g .. iupper + g`` (``+ 1`` along axis ``c``).

The periodic case is defined as "fill the ghosts by ``ibtk_le_fill_periodic_ghosts``' rule,
then run the plain routine": ``periodic_fill`` is that rule -- a point outside the cell
range of a periodic dim takes the value at ``ilower + (i - ilower) mod n``, all periodic
dims wrapped at once, the face ``iupper + 1`` of an array's own axis included.

``curl_abs`` is the same expression with every subtraction replaced by an addition on
``|u|`` and ``|fac|``: the magnitude the rounding-error bounds of the tests are stated in.
"""
import numpy as np

# component -> two terms (source array, dim of the difference, eight (dx, dy, dz) operands
# taken + - + - + - + -); the component is term 0 minus term 1
STENCIL = {
    0: ((2, 1, [(-1, 1, 0), (-1, -1, 0), (0, 1, 0), (0, -1, 0), (-1, 1, 1), (-1, -1, 1), (0, 1, 1), (0, -1, 1)]),
        (1, 2, [(-1, 0, 1), (-1, 0, -1), (0, 0, 1), (0, 0, -1), (-1, 1, 1), (-1, 1, -1), (0, 1, 1), (0, 1, -1)])),
    1: ((0, 2, [(0, -1, 1), (0, -1, -1), (1, -1, 1), (1, -1, -1), (0, 0, 1), (0, 0, -1), (1, 0, 1), (1, 0, -1)]),
        (2, 0, [(1, -1, 0), (-1, -1, 0), (1, 0, 0), (-1, 0, 0), (1, -1, 1), (-1, -1, 1), (1, 0, 1), (-1, 0, 1)])),
    2: ((1, 0, [(1, 0, -1), (-1, 0, -1), (1, 1, -1), (-1, 1, -1), (1, 0, 0), (-1, 0, 0), (1, 1, 0), (-1, 1, 0)]),
        (0, 1, [(0, 1, -1), (0, -1, -1), (1, 1, -1), (1, -1, -1), (0, 1, 0), (0, -1, 0), (1, 1, 0), (1, -1, 0)])),
}


def box_extent(ilower, iupper):
    return [int(iupper[d]) - int(ilower[d]) + 1 for d in range(3)]


def _gcw3(g):
    return [int(g)] * 3 if np.isscalar(g) else [int(v) for v in g]


def side_shape(n, g, c):
    """numpy shape of the ghosted side array of axis c."""
    g = _gcw3(g)
    return tuple(n[d] + 2 * g[d] + (1 if d == c else 0) for d in (2, 1, 0))


def side_box(n, g, c):
    """The slices of the side box (ilower .. iupper, + 1 along c) inside the ghosted array."""
    g = _gcw3(g)
    return tuple(slice(g[d], g[d] + n[d] + (1 if d == c else 0)) for d in (2, 1, 0))


def regrow(u, n, g, periodic=None, g_out=1):
    """The side arrays with ghost width g_out, gathered from arrays of ghost width g: a
    periodic dim reads index i at ``i mod n`` (the fill's rule; the ghost values of u in
    that dim are never looked at), another dim reads i itself and needs g >= g_out."""
    g, go = _gcw3(g), _gcw3(g_out)
    per = [bool(p) for p in periodic] if periodic is not None else [False] * 3
    out = []
    for c in range(3):
        idx = []
        for d in range(3):
            i = np.arange(-go[d], n[d] + go[d] + (1 if d == c else 0))
            if per[d]:
                i = np.mod(i, n[d])
            elif g[d] < go[d]:
                raise ValueError(f"ghost width {g[d]} of dim {d} below {go[d]}")
            idx.append(i + g[d])
        out.append(np.ascontiguousarray(u[c][np.ix_(idx[2], idx[1], idx[0])]))
    return out


def periodic_fill(u, n, g, periodic):
    """ibtk_le_fill_periodic_ghosts on side arrays: new arrays of the same ghost width."""
    return regrow(u, n, g, periodic, g)


def _term(u1, n, c, term, absolute, dx):
    """fac * (eight-term sum) over the side box of component c, from ghost-1 arrays."""
    src, dim, ops = term
    ext = [n[d] + (1 if d == c else 0) for d in range(3)]
    A = np.abs(u1[src]) if absolute else u1[src]

    def at(o):
        return A[1 + o[2]:1 + o[2] + ext[2], 1 + o[1]:1 + o[1] + ext[1], 1 + o[0]:1 + o[0] + ext[0]]

    s = at(ops[0])
    for m, o in enumerate(ops[1:], 1):
        s = s + at(o) if (absolute or m % 2 == 0) else s - at(o)
    fac = np.float64(0.125) / np.float64(dx[dim])
    return (abs(fac) if absolute else fac) * s


def curl_values(u, n, g, dx, periodic=None, absolute=False):
    """The three side-box arrays (no ghosts) of curl u -- or of ``curl_abs`` -- from the
    ghosted arrays u of ghost width g."""
    u1 = regrow(u, n, g, periodic, 1)
    out = []
    with np.errstate(all="ignore"):
        for c in range(3):
            a, b = (_term(u1, n, c, t, absolute, dx) for t in STENCIL[c])
            out.append(a + b if absolute else a - b)
    return out


def curl_abs(u, n, g, dx, periodic=None):
    return curl_values(u, n, g, dx, periodic, absolute=True)


def curl_side_ref(u, ilower, iupper, u_gcw, w, w_gcw, dx, alpha=1.0, accumulate=False, periodic=None):
    """``w = alpha curl u (+ w)`` written into the side boxes of the ghosted arrays w, in
    place; nothing else of w is touched.  Returns w."""
    n = box_extent(ilower, iupper)
    if min(n) <= 0:
        return w
    vals = curl_values(u, n, u_gcw, dx, periodic)
    with np.errstate(all="ignore"):
        for c in range(3):
            t = np.float64(alpha) * vals[c]
            box = side_box(n, w_gcw, c)
            w[c][box] = t + w[c][box] if accumulate else t
    return w


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)

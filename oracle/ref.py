"""ctypes front end of the compiled reference Fortran -- TEST INFRASTRUCTURE ONLY.

Same import rule as ``oracle.py``: only ``tests/`` may import this module; the product
path (``ibamr_amd``), ``smoke()`` and ``bench.py`` never do.  It reads nothing but
``oracle/_ref/libleref_{O0,O2}.so``, which ``oracle/build_ref.py`` compiles from the
reference's own ``lagrangian_interaction{2,3}d.f.m4`` and ``lagrangian_delta.f.m4``
where the reference tree and flang exist; it never looks at the reference tree itself.

``interp`` / ``spread`` have the signatures of ``oracle.interp`` / ``oracle.spread`` and
call ``lagrangian_<kernel>_{interp,spread}{2,3}d_`` of the ``-O0`` library;
``backend(opt)`` gives the same pair over either library, in the form that
``oracle.side_*`` / ``cell_*`` / ``node_*`` take as ``backend=``.

Two calls are kept from the reference (Oracle, deviations table):

* ``DISCONTINUOUS_LINEAR`` 3-D spread reads an unset ``ic_center`` as an array index:
  refused, never called.
* ``PIECEWISE_CONSTANT`` indexes ``u`` unchecked: a listed marker whose cell is not
  strictly inside the ghost box is refused before the call.

``phys_bdry_side`` has the arguments of ``oracle.phys_bdry_side`` and runs over
``oracle/_ref/libbdref_{O0,O2}.so``, the reference's ``cartphysbdryop{2,3}d.f.m4``
(``bdry_available()`` tells whether that pair is there; it is built and found apart from
``libleref_*``).  The Fortran arithmetic and the reading of its arguments are the
reference's; the walk over the boundary boxes around the calls is a restatement of
``CartSideRobinPhysBdryOp.cpp``, see the function.
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
_DIR = _HERE / "_ref"
OPTS = ("O0", "O2")

# the kernels the reference has in Fortran (BSPLINE_4 and USER_DEFINED live in LEInteractor.cpp)
FORTRAN_NAME = {
    "PIECEWISE_CONSTANT": "piecewise_constant",
    "DISCONTINUOUS_LINEAR": "discontinuous_linear",
    "PIECEWISE_LINEAR": "piecewise_linear",
    "PIECEWISE_CUBIC": "piecewise_cubic",
    "IB_3": "ib_3",
    "IB_4": "ib_4",
    "IB_4_W8": "ib_4_w8",
    "IB_6": "ib_6",
}
KERNELS = tuple(FORTRAN_NAME)

_libs = {}


class ReferenceRefused(ValueError):
    """A call the reference cannot be trusted with (see the module docstring)."""


def lib_path(opt="O0"):
    if opt not in OPTS:
        raise ValueError(f"unknown reference build {opt!r} (have {OPTS})")
    return _DIR / f"libleref_{opt}.so"


def available():
    """True when both reference libraries are under oracle/_ref/."""
    return all(lib_path(o).is_file() for o in OPTS)


def lib(opt="O0"):
    """The reference library of one optimisation level, through a handle of its own
    (its symbol names are those of libibtk_le.so's shims, by design)."""
    if opt not in _libs:
        p = lib_path(opt)
        if not p.is_file():
            raise FileNotFoundError(f"{p} is missing: run oracle/build_ref.py where the reference tree is")
        L = ctypes.CDLL(str(p), mode=ctypes.RTLD_LOCAL)
        dref = ctypes.POINTER(ctypes.c_double)
        L.lagrangian_floor_.restype = ctypes.c_int
        L.lagrangian_floor_.argtypes = [dref]
        for name in ("lagrangian_ib_3_delta_", "lagrangian_piecewise_cubic_delta_"):
            f = getattr(L, name)
            f.restype = ctypes.c_double
            f.argtypes = [dref]
        _libs[opt] = L
    return _libs[opt]


# --------------------------------------------------------------------------
# lagrangian_delta.f: arguments by reference, results by value
# --------------------------------------------------------------------------
def _scalar_fn(name, opt, x):
    # the delta functions overwrite their argument with |r|: hand over a copy
    return getattr(lib(opt), name)(ctypes.byref(ctypes.c_double(float(x))))


def lagrangian_floor(x, opt="O0"):
    return int(_scalar_fn("lagrangian_floor_", opt, x))


def ib_3_delta(r, opt="O0"):
    return float(_scalar_fn("lagrangian_ib_3_delta_", opt, r))


def piecewise_cubic_delta(r, opt="O0"):
    return float(_scalar_fn("lagrangian_piecewise_cubic_delta_", opt, r))


# --------------------------------------------------------------------------
# lagrangian_interaction{2,3}d.f
# --------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _i(v):
    return ctypes.byref(ctypes.c_int(int(v)))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def ghost_shape(ilower, iupper, nugc, depth=1):
    n = [iupper[d] - ilower[d] + 1 + 2 * nugc[d] for d in range(len(ilower))]
    return (depth,) + tuple(reversed(n))


def cells_inside_ghost_box(dx, x_lower, ilower, iupper, nugc, indices, Xshift, X):
    """True when NINT((X+Xshift-x_lower)/dx-0.5)+ilower lies in the ghost box for every
    listed entry, whichever way a half is rounded."""
    ndim = len(ilower)
    idx = np.asarray(indices, dtype=np.int64)
    Xs = np.asarray(X, np.float64).reshape(-1, ndim)[idx] + np.asarray(Xshift, np.float64).reshape(-1, ndim)
    for d in range(ndim):
        v = (Xs[:, d] - x_lower[d]) / dx[d] - 0.5
        lo, hi = np.ceil(v - 0.5) + ilower[d], np.floor(v + 0.5) + ilower[d]
        if not (np.all(lo >= ilower[d] - nugc[d]) and np.all(hi <= iupper[d] + nugc[d])):
            return False
    return True


def _call(opt, op, kernel, dx, x_lower, ilower, iupper, nugc, u, idx, xs, X, V, depth, axis):
    """One call with the argument tuple of the Fortran: dx, x_lower, x_upper, depth
    [, axis for DISCONTINUOUS_LINEAR], then box, ghosts, u and the list, X, V in the
    order of the operation."""
    ndim = len(ilower)
    if kernel not in FORTRAN_NAME:
        raise ValueError(f"the reference has no Fortran kernel {kernel}")
    if ndim not in (2, 3):
        raise ValueError("ndim must be 2 or 3")
    if (kernel, ndim, op) == ("DISCONTINUOUS_LINEAR", 3, "spread"):
        raise ReferenceRefused("the reference's DISCONTINUOUS_LINEAR 3-D spread reads an unset ic_center(d) "
                               "for d != axis as an array index; it is never called")
    if u.size != int(np.prod(ghost_shape(ilower, iupper, nugc, depth))):
        raise ValueError("u does not have the ghosted shape")
    if xs.shape != (idx.size, ndim):
        raise ValueError("Xshift must be (nindices, ndim)")
    if idx.size:
        if int(idx.min()) < 0 or (int(idx.max()) + 1) * ndim > X.size or (int(idx.max()) + 1) * depth > V.size:
            raise ValueError("an index of the list lies outside X or V")
    if kernel == "PIECEWISE_CONSTANT" and not cells_inside_ghost_box(dx, x_lower, ilower, iupper, nugc, idx, xs, X):
        raise ReferenceRefused("the reference's PIECEWISE_CONSTANT indexes u unchecked: every listed marker's "
                               "cell must lie inside the ghost box")
    f = getattr(lib(opt), f"lagrangian_{FORTRAN_NAME[kernel]}_{op}{ndim}d_")
    f.restype = None
    dxa, xla = _f64(dx), _f64(x_lower)
    xua = xla + 1.0  # x_upper is passed and unused
    head = [_dp(dxa), _dp(xla), _dp(xua), _i(depth)]
    if kernel == "DISCONTINUOUS_LINEAR":
        head.append(_i(axis))
    box = []
    for d in range(ndim):
        box += [_i(ilower[d]), _i(iupper[d])]
    gc = [_i(nugc[d]) for d in range(ndim)]
    lst = [_ip(idx), _dp(xs), _i(idx.size)]
    if op == "interp":
        f(*head, *box, *gc, _dp(u), *lst, _dp(X), _dp(V))
    else:
        f(*head, *lst, _dp(X), _dp(V), *box, *gc, _dp(u))


def _interp(opt, kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth=1, axis=0):
    assert V.dtype == np.float64 and V.flags.c_contiguous
    _call(opt, "interp", kernel, dx, x_lower, ilower, iupper, nugc, _f64(u), _i32(indices), _f64(Xshift), _f64(X), V,
          int(depth), int(axis))
    return V


def _spread(opt, kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth=1, axis=0):
    assert u.dtype == np.float64 and u.flags.c_contiguous
    _call(opt, "spread", kernel, dx, x_lower, ilower, iupper, nugc, u, _i32(indices), _f64(Xshift), _f64(X), _f64(V),
          int(depth), int(axis))
    return u


def interp(kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth=1, axis=0):
    """lagrangian_<kernel>_interp{2,3}d_ of the -O0 reference (writes V in place)."""
    return _interp("O0", kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth, axis)


def spread(kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth=1, axis=0):
    """lagrangian_<kernel>_spread{2,3}d_ of the -O0 reference (accumulates into u)."""
    return _spread("O0", kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth, axis)


def backend(opt="O0"):
    """(interp, spread) over one reference library, for ``oracle.side_*(..., backend=)``."""
    lib(opt)

    def interp_(kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth=1, axis=0):
        return _interp(opt, kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth, axis)

    def spread_(kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth=1, axis=0):
        return _spread(opt, kernel, dx, x_lower, ilower, iupper, nugc, u, indices, Xshift, X, V, depth, axis)

    return interp_, spread_


# --------------------------------------------------------------------------
# cartphysbdryop{2,3}d.f: the physical-boundary operators on side data
# --------------------------------------------------------------------------
_bdlibs = {}


def bdry_lib_path(opt="O0"):
    if opt not in OPTS:
        raise ValueError(f"unknown reference build {opt!r} (have {OPTS})")
    return _DIR / f"libbdref_{opt}.so"


def bdry_available():
    """True when both boundary-operator libraries are under oracle/_ref/."""
    return all(bdry_lib_path(o).is_file() for o in OPTS)


def bdry_lib(opt="O0"):
    if opt not in _bdlibs:
        p = bdry_lib_path(opt)
        if not p.is_file():
            raise FileNotFoundError(f"{p} is missing: run oracle/build_ref.py where the reference tree is")
        _bdlibs[opt] = ctypes.CDLL(str(p), mode=ctypes.RTLD_LOCAL)
    return _bdlibs[opt]


# Which end of each dimension a codim-2 / codim-3 location index names, copied from the
# comments of the Fortran's own if-chains (cartphysbdryop2d.f.m4:678-706, 3d:1245-1340 and
# 3d:1543-1620): 0 the lower end, 1 the upper end, None the direction the edge runs along.
CORNER_2D = {0: (0, 0), 1: (1, 0), 2: (0, 1), 3: (1, 1)}
EDGE_3D = {0: (None, 0, 0), 1: (None, 1, 0), 2: (None, 0, 1), 3: (None, 1, 1),
           4: (0, None, 0), 5: (0, None, 1), 6: (1, None, 0), 7: (1, None, 1),
           8: (0, 0, None), 9: (1, 0, None), 10: (0, 1, None), 11: (1, 1, None)}
CORNER_3D = {0: (0, 0, 0), 1: (1, 0, 0), 2: (0, 1, 0), 3: (1, 1, 0),
             4: (0, 0, 1), 5: (1, 0, 1), 6: (0, 1, 1), 7: (1, 1, 1)}


def _fill_box(lo, hi, g, ends):
    """PatchGeometry::getBoundaryFillBox of the boundary box at `ends`: g cells deep
    outside the patch in every direction with an end, the patch's cells in the others."""
    flo, fhi = [], []
    for d, e in enumerate(ends):
        if e is None:
            flo.append(lo[d]), fhi.append(hi[d])
        elif e:
            flo.append(hi[d] + 1), fhi.append(hi[d] + g)
        else:
            flo.append(lo[d] - g), fhi.append(lo[d] - 1)
    return flo, fhi


def _pairs(lo, hi, dims=None):
    out = []
    for d in (range(len(lo)) if dims is None else dims):
        out += [_i(lo[d]), _i(hi[d])]
    return out


def phys_bdry_side(box_lo, box_hi, gcw, dx, u_axes, phys, acoef, bcoef, gcoef, adjoint, opt="O0"):
    """CartSideRobinPhysBdryOp on one patch of side data (in place), every number of it
    computed by the reference's compiled {cc,sc}robinphysbdryop* routines.

    What is the reference's: the arithmetic, the loop order and the meaning of every
    argument of the Fortran.  What is restated here, from CartSideRobinPhysBdryOp.cpp, and
    so not pinned by this function: the walk over the boundary boxes --

    * fill (adjoint false, :390-420): codim-1 normal component (:531-629), codim-1
      transverse components through the cell-centred routines over side_box[axis] with the
      coefficient box extended by one along the component (:687-818), codim-2 (:855-952;
      in 3-D the edge-parallel component through ccrobinphysbdryop23d over
      toSideBox(bc_fill_box, axis)), codim-3 (:982-1008);
    * adjoint (:462-492): the same four in reverse;

    the boundary boxes themselves (one per face, edge, corner whose faces are all flagged
    in `phys`, in location-index order, each fill box `gcw` cells deep), and the
    coefficient arrays, which the C++ has a RobinBcCoefStrategy fill and which are filled
    here with one constant per (component, face): acoef/bcoef/gcoef[axis, location]."""
    ndim = len(box_lo)
    if ndim not in (2, 3):
        raise ValueError("ndim must be 2 or 3")
    g = int(gcw)
    if g <= 0:
        return u_axes  # ghost_width_to_fill == 0 (:362, :433)
    L = bdry_lib(opt)
    lo, hi = [int(v) for v in box_lo], [int(v) for v in box_hi]
    for a in range(ndim):
        u = u_axes[a]
        n = [hi[d] - lo[d] + 1 + 2 * g + (1 if d == a else 0) for d in range(ndim)]
        if u.dtype != np.float64 or not u.flags.c_contiguous or u.shape != tuple(reversed(n)):
            raise ValueError(f"u_axes[{a}] is not the ghosted side array of axis {a}")
    A, B, G = (np.broadcast_to(np.asarray(c, np.float64), (ndim, 2 * ndim)) for c in (acoef, bcoef, gcoef))
    dxa = _f64(dx)
    adj = 1 if adjoint else 0
    xyz = "xyz"
    side_lo = [list(lo) for _ in range(ndim)]
    side_hi = [[hi[d] + (1 if d == a else 0) for d in range(ndim)] for a in range(ndim)]
    faces = [loc for loc in range(2 * ndim) if phys[loc]]

    def call(name, *args):
        f = getattr(L, name)
        f.restype = None
        f(*args)

    def codim1(axis, loc):
        """One routine call for component `axis` on face `loc`: sc* when the component is
        the face's normal, else cc* on side_box[axis] with the extended coefficient box."""
        n = loc // 2
        tang = [d for d in range(ndim) if d != n]
        blo, bhi = list(lo), list(hi)  # makeSideBoundaryCodim1Box: tangentially the patch's cells
        if axis != n:
            bhi[axis] += 1  # compute_tangential_extension (:294-299)
        size = 1
        for d in tang:
            size *= bhi[d] - blo[d] + 1
        a, b, gc = (np.full(size, float(C[axis, loc])) for C in (A, B, G))
        if axis == n:
            call(f"scrobinphysbdryop1{xyz[n]}{ndim}d_", _dp(u_axes[axis]), _i(g), _dp(a), _dp(b), _dp(gc), _i(loc),
                 *_pairs(lo, hi), *_pairs(blo, bhi, tang), _dp(dxa), _i(adj))
        else:
            call(f"ccrobinphysbdryop1{xyz[n]}{ndim}d_", _dp(u_axes[axis]), _i(g), _dp(a), _dp(b), _dp(gc), _i(loc),
                 *_pairs(side_lo[axis], side_hi[axis]), *_pairs(blo, bhi, tang), _dp(dxa), _i(adj))

    def codim1_normal():
        for loc in faces:
            codim1(loc // 2, loc)

    def codim1_transverse():
        for loc in faces:
            for axis in range(ndim):
                if axis != loc // 2:
                    codim1(axis, loc)

    def is_physical(ends):
        return all(e is None or phys[2 * d + e] for d, e in enumerate(ends))

    def codim2():
        table = CORNER_2D if ndim == 2 else EDGE_3D
        for loc in sorted(table):
            ends = table[loc]
            if not is_physical(ends):
                continue
            flo, fhi = _fill_box(lo, hi, g, ends)
            call(f"scrobinphysbdryop2{ndim}d_", *[_dp(u) for u in u_axes], _i(g), _i(loc), *_pairs(lo, hi),
                 *_pairs(flo, fhi), _i(adj))
            if ndim == 3:
                axis = loc // 4  # :887-949
                assert ends[axis] is None
                shi = list(fhi)
                shi[axis] += 1  # SideGeometry::toSideBox(bc_fill_box, axis)
                call("ccrobinphysbdryop23d_", _dp(u_axes[axis]), _i(g), _i(loc),
                     *_pairs(side_lo[axis], side_hi[axis]), *_pairs(flo, shi), _i(adj))

    def codim3():
        if ndim != 3:
            return
        for loc in sorted(CORNER_3D):
            ends = CORNER_3D[loc]
            if not is_physical(ends):
                continue
            flo, fhi = _fill_box(lo, hi, g, ends)
            call("scrobinphysbdryop33d_", *[_dp(u) for u in u_axes], _i(g), _i(loc), *_pairs(lo, hi),
                 *_pairs(flo, fhi), _i(adj))

    steps = [codim1_normal, codim1_transverse, codim2, codim3]
    for step in (reversed(steps) if adjoint else steps):
        step()
    return u_axes

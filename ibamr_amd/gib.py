"""The Eulerian side of the generalized IB step: the side-centred curl, the angular
velocity and the torque.

``GeneralizedIBMethod`` couples the rods' director triads to the fluid through the curl of
side-centred data (``src/IB/GeneralizedIBMethod.cpp``):

* ``interpolateVelocity`` (``:292-319``) forms ``w = curl u``, scales it by 0.5, fills its
  ghost cells and interpolates it to the nodes: the angular velocity ``W`` that
  :func:`ibamr_amd.rods.director_update` takes.
* ``spreadForce`` (``:537-577``) zeroes ``n``, spreads the torque ``N`` that
  :meth:`ibamr_amd.rods.RodForceGen.compute` produces into it, fills its ghost cells and adds
  ``f += 0.5 curl n``.

:func:`curl_side` is the operator (``ibtk_le_curl_side``, one HIP launch for the three
components, bit for bit the reference's ``stoscurl3d``); :func:`interp_angular_velocity` and
:func:`spread_torque` are the two compositions for one periodic patch.  Both are sequences
of public calls on the context stream with no host synchronisation.  A caller with
physical walls composes :func:`curl_side` (plain, or periodic in some dims) with
``le.phys_bdry_side`` / ``le.fill_periodic_ghosts`` / ``le.fold_periodic_ghosts`` itself.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

from ._lib import check

__all__ = ["CURL_TILE", "CURL_MIN_SEGMENT", "curl_side", "interp_angular_velocity", "spread_torque"]

# (TX, TY, TZ): the x-y tile a workgroup of the curl kernel owns and the longest z segment
# it marches (CURL_TX, CURL_TY, CURL_TZ of csrc/le_curl.h).  Tiles start at the w arrays'
# first element in x (ilower - gcw) and at ilower in y; a box with few tiles is cut into
# shorter segments, down to CURL_MIN_SEGMENT planes.
CURL_TILE = (32, 16, 32)
CURL_MIN_SEGMENT = 4


def curl_side(ctx, u_geom, u: Sequence, w_geom, w: Sequence, alpha: float = 1.0, accumulate: bool = False,
              periodic=None):
    """``w = alpha curl u`` (``+ w`` with ``accumulate``) over the three side boxes of one
    3-D patch (``ibtk_le_curl_side``; ``PatchMathOps::curl(side, side)``).

    ``u`` and ``w`` are the three ghosted side arrays of ``u_geom`` / ``w_geom``
    (``Geometry.alloc("side")``), which agree in box and ``dx`` and may differ in ghost
    width and pitch; ``w`` must not overlap ``u``.  ``periodic=None`` (or all false) is the
    plain reference routine: it reads ``u``'s ghost layer as it stands and needs a ghost
    width of 1.  Note that None means *no* periodic dim here, unlike
    ``le.fill_periodic_ghosts``.  Where ``periodic[d]`` is set, reads outside the cell
    range of dim ``d`` are taken at their periodic image: the result of
    ``le.fill_periodic_ghosts(u)`` followed by the plain call, bit for bit, with ``u``
    left untouched.  Nothing outside ``w``'s side boxes is written."""
    from .le import _periodic_arg, _ptr_array
    if len(u) != 3 or len(w) != 3:
        raise ValueError("u and w are three side arrays each")
    pa = _periodic_arg(periodic, 3)
    check(ctx.lib.ibtk_le_curl_side(ctx.h, ctypes.byref(u_geom.c), _ptr_array(u, u_geom), ctypes.byref(w_geom.c),
                                    _ptr_array(w, w_geom), float(alpha), int(bool(accumulate)),
                                    pa[0] if pa else None))


def interp_angular_velocity(ctx, markers, kernel: str, u_geom, u: Sequence, w_geom, w: Sequence, W, X,
                            periodic=(True, True, True)):
    """``W = interp(0.5 curl u)``: ``GeneralizedIBMethod::interpolateVelocity``'s angular
    velocity on one periodic patch.

    ``curl_side(u -> w, alpha=0.5, periodic)`` and then
    ``le.fill_interp("side", w_geom, w, W, X, periodic)``, which reads ``w``'s ghost points
    at their periodic images (and falls back to fill plus interp where it cannot fuse).
    ``w`` is caller-owned scratch with the kernel's ghost width; ``markers`` are binned on
    ``w_geom``; ``W`` and ``X`` are ``[n][3]``.  Two calls on the context stream, no host
    synchronisation.  With physical walls use :func:`curl_side` and
    ``le.phys_bdry_side`` / ``le.fill_periodic_ghosts`` / ``le.interp`` directly."""
    from . import le
    curl_side(ctx, u_geom, u, w_geom, w, alpha=0.5, accumulate=False, periodic=periodic)
    le.fill_interp(ctx, markers, kernel, "side", w_geom, w, W, X, periodic=periodic)
    return W


def spread_torque(ctx, markers, kernel: str, n_geom, n: Sequence, N, X, f_geom, f: Sequence,
                  periodic=(True, True, True), fold: bool = True):
    """``f += 0.5 curl(spread N)``: the torque part of ``GeneralizedIBMethod::spreadForce``
    on one periodic patch.

    ``le.zero_spread`` of ``N`` into the caller-owned scratch ``n`` (the kernel's ghost
    width; ``markers`` binned on ``n_geom``), ``le.fold_periodic_ghosts(n)`` when ``fold``
    -- leave it out when the binned list already holds the periodic images
    (``le.periodic_index_list``) --, then ``curl_side(n -> f, alpha=0.5, accumulate=True,
    periodic)``: the curl reads ``n`` at its periodic images, so the reference's ghost fill
    of ``n`` needs no pass and ``n``'s stale ghost values are never read.  Calls on the
    context stream, no host synchronisation.  With physical walls use ``le.zero_spread``,
    ``le.phys_bdry_side(adjoint=True)`` / ``le.fold_periodic_ghosts``, the fills and
    :func:`curl_side` directly."""
    from . import le
    le.zero_spread(ctx, markers, kernel, "side", n_geom, n, N, X)
    if fold:
        le.fold_periodic_ghosts(ctx, n_geom, "side", n, periodic=periodic)
    curl_side(ctx, n_geom, n, f_geom, f, alpha=0.5, accumulate=True, periodic=periodic)
    return f

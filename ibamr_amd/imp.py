"""The immersed material point method on the device: velocity-gradient interpolation, stress
spreading, the deformation-gradient update and the Kirchhoff stress.

``IMPMethod`` (``src/IB/IMPMethod.cpp``) couples material points to the staggered grid
through its own IB_6 kernel *and its derivative* (``:119-171``), not through
``LEInteractor``:

* ``interpolateVelocity`` (``:460-536``) gathers ``U`` and the three columns of ``Grad U``
  at every point -- :func:`interp_velocity_gradient`;
* ``eulerStep`` / ``midpointStep`` / ``trapezoidalStep`` (``:547-716``) advance the
  deformation gradient, ``F_new = inv(I - dt/2 G_b)(I + dt/2 G_a) F`` --
  :func:`deformation_update` (the positions move with ``le.position_update``);
* ``computeLagrangianForce`` (``:718-780``) forms ``tau = PP FF^T`` from a PK1 stress --
  :func:`kirchhoff_stress` computes the law of ``examples/IMP/explicit/ex0``; ``tau`` is a
  plain device array, so any torch expression may fill it instead;
* ``spreadForce`` (``:848-921``) scatters ``f_c += sum_k tau(c,k) d_k delta_h wgt / dV`` --
  :func:`spread_stress`.

All four run on the context stream with no host synchronisation (the first interp after a
binning with an index list builds the duplicate table, as ``le.interp`` does).  ``markers``
is a ``le.Markers`` binned with ``"IB_6"`` on ``geom``: the NINT anchor is the same, so the
IB_6 bins bound this stencil, and the ghost width must be at least :data:`MIN_GHOST`.
Positions are the binned ``X + Xshift``; the reference ignores the periodic offset of an
image node, and with ``Xshift = 0`` the two agree.  One patch; the level and z-slab forms,
``IMPInitializer`` and ``IMPMethod``'s ``LData`` bookkeeping are out of scope.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from ._lib import check

__all__ = ["IMP_TILE", "IMP_CHUNK", "MIN_GHOST", "CLIP", "SCHEMES", "interp_velocity_gradient", "spread_stress",
           "deformation_update", "kirchhoff_stress"]

# (3-D, 2-D) edge of the tile of side points a workgroup of the spread owns, and the entries
# it stages in LDS at a time (IMP_TILE3, IMP_TILE2, IMP_CHUNK of csrc/le_imp.h)
IMP_TILE = (8, 16)
IMP_CHUNK = 64
MIN_GHOST = 4
CLIP = {"patch": 0, "ghost": 1}
SCHEMES = {"euler": 0, "midpoint": 1, "trapezoidal": 2}


def _rows(t: torch.Tensor, n: Optional[int], width: int, name: str):
    if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous float64 device tensor")
    if t.dim() != 2 or t.shape[1] != width or (n is not None and t.shape[0] != n):
        raise ValueError(f"{name}: shape ({'n' if n is None else n}, {width}), got {tuple(t.shape)}")


def interp_velocity_gradient(ctx, markers, geom, u: Sequence, U, GradU, X):
    """``U[s] = u(X_s)`` and ``GradU[s][NDIM*i+j] = d u_i / d x_j`` with IMPMethod's kernel
    (``ibtk_le_imp_interp``), bit for bit the reference's sums.  ``u`` are the ghosted side
    arrays of ``geom``; ``U`` is ``[n][NDIM]``, ``GradU`` ``[n][NDIM*NDIM]``; rows the list
    does not name are not written."""
    from .le import _ptr, _ptr_array
    nd = geom.ndim
    if len(u) != nd:
        raise ValueError("u: NDIM side arrays")
    _rows(U, None, nd, "U")
    _rows(GradU, U.shape[0], nd * nd, "GradU")
    check(ctx.lib.ibtk_le_imp_interp(ctx.h, markers.h, ctypes.byref(geom.c), _ptr_array(u, geom), _ptr(U), _ptr(GradU),
                                     _ptr(X)))
    return U, GradU


def spread_stress(ctx, markers, geom, f: Sequence, tau, wgt, X, clip: str = "patch"):
    """``f_c += sum_k tau(c,k) d_k delta_h wgt / dV`` (``ibtk_le_imp_spread``).

    ``tau`` is ``[n][NDIM*NDIM]``, ``wgt`` ``[n]``.  ``clip="patch"`` is the reference: the
    stencils are cut to the patch's side boxes and periodic images arrive as list entries
    (``le.periodic_index_list``).  ``clip="ghost"`` cuts to the arrays' ghost boxes, for a
    caller who then runs ``le.fold_periodic_ghosts`` or ``le.phys_bdry_side(adjoint=True)``.
    No atomics; the result is bit-identical from run to run."""
    from .le import _ptr, _ptr_array
    nd = geom.ndim
    if clip not in CLIP:
        raise ValueError(f"clip: 'patch' or 'ghost', got {clip!r}")
    if len(f) != nd:
        raise ValueError("f: NDIM side arrays")
    _rows(tau, None, nd * nd, "tau")
    if wgt.dtype != torch.float64 or not wgt.is_cuda or not wgt.is_contiguous() or wgt.numel() != tau.shape[0]:
        raise ValueError("wgt: one float64 per point, contiguous, on the device")
    check(ctx.lib.ibtk_le_imp_spread(ctx.h, markers.h, ctypes.byref(geom.c), _ptr_array(f, geom), _ptr(tau), _ptr(wgt),
                                     _ptr(X), CLIP[clip]))
    return f


def deformation_update(ctx, scheme: str, dt: float, F_cur, G0, G1=None, F_new=None, F_half=None):
    """``F_new = inv(I - dt/2 G_b)(I + dt/2 G0) F_cur`` (``ibtk_le_imp_deformation_update``):
    ``G_b = G0`` for ``"euler"`` (Grad U at the current time) and ``"midpoint"`` (at the half
    time), ``G1`` for ``"trapezoidal"`` (``G0`` current, ``G1`` new).  ``"euler"`` with
    ``F_half`` also writes the half step (``dt/4``).  Rows of 9 (3-D) or 4 (2-D) doubles;
    ``F_new`` is allocated when not given and returned."""
    from .le import _ptr
    if scheme not in SCHEMES:
        raise ValueError(f"scheme: one of {sorted(SCHEMES)}, got {scheme!r}")
    if F_cur.dim() != 2 or F_cur.shape[1] not in (4, 9):
        raise ValueError("F_cur: rows of 4 (2-D) or 9 (3-D) doubles")
    n, w = F_cur.shape
    nd = 2 if w == 4 else 3
    if F_new is None:
        F_new = torch.empty_like(F_cur)
    for name, t in (("F_cur", F_cur), ("G0", G0), ("G1", G1), ("F_new", F_new), ("F_half", F_half)):
        if t is not None:
            _rows(t, n, w, name)
    check(ctx.lib.ibtk_le_imp_deformation_update(ctx.h, nd, SCHEMES[scheme], n, float(dt), _ptr(F_cur), _ptr(G0),
                                                 _ptr(G1), _ptr(F_new), _ptr(F_half)))
    return F_new


def kirchhoff_stress(ctx, F, tau, c1, p0=0.0, beta=0.0, subdomain=None):
    """``tau = PP FF^T`` with ``PP = 2 c1 FF - 2 p0 FF^-T + beta log(det C) FF^-T`` (the
    second and third terms only where ``p0`` / ``beta`` are non-zero), the law of
    ``examples/IMP/explicit/ex0`` (``ibtk_le_imp_stress``).  ``c1``, ``p0``, ``beta`` are
    scalars; or, with ``subdomain`` (int32 per point), ``c1`` is a device ``[nsub][3]``
    table of ``(c1, p0, beta)`` rows.  ``tau`` may be ``F`` itself."""
    from .le import _ptr
    if F.dim() != 2 or F.shape[1] not in (4, 9):
        raise ValueError("F: rows of 4 (2-D) or 9 (3-D) doubles")
    n, w = F.shape
    nd = 2 if w == 4 else 3
    _rows(F, n, w, "F")
    _rows(tau, n, w, "tau")
    if subdomain is None:
        check(ctx.lib.ibtk_le_imp_stress(ctx.h, nd, n, _ptr(F), _ptr(tau), float(c1), float(p0), float(beta), None, 0,
                                         None))
    else:
        table = c1
        if not isinstance(table, torch.Tensor):
            raise ValueError("with subdomain, c1 is the [nsub][3] device table of (c1, p0, beta)")
        _rows(table, None, 3, "parameter table")
        if subdomain.dtype != torch.int32 or not subdomain.is_cuda or not subdomain.is_contiguous() \
                or subdomain.numel() != n:
            raise ValueError("subdomain: one int32 per point, contiguous, on the device")
        check(ctx.lib.ibtk_le_imp_stress(ctx.h, nd, n, _ptr(F), _ptr(tau), 0.0, 0.0, 0.0, _ptr(table),
                                         int(table.shape[0]), _ptr(subdomain)))
    return tau

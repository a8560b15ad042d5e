"""Kirchhoff rods on the device: force, torque and director update.

``IBKirchhoffRodForceGen::computeLagrangianForceAndTorque``
(``src/IB/IBKirchhoffRodForceGen.cpp:326-527``) produces the force ``F`` and the torque
``N`` that ``spread`` consumes from the positions ``X`` and the director triads ``D``, and
``GeneralizedIBMethod::eulerStep`` / ``trapezoidalStep``
(``src/IB/GeneralizedIBMethod.cpp:326-447``) rotate the triads by the interpolated angular
velocity ``W``.  ``W`` and ``N`` themselves are ordinary depth-3 Lagrangian data for
``interpolate`` / ``spread``.  Three pieces live here:

* :class:`RodSpecs` -- the host side.  It holds what :func:`ibamr_amd.io.read_rod` and
  :func:`ibamr_amd.io.read_director` return for one or more structures and flattens the
  rods into the arrays ``IBKirchhoffRodForceGen::initializeLevelData`` caches (``:167-197``),
  in the reference's order: master by master in local node order, deck order within a
  master.

* :class:`RodForceGen` -- the device plan built through the C ABI (``ibtk_le_rodgen_*``)
  and its ``compute``: one gather kernel, a lane per node, no atomics, no host
  synchronisation.

* :func:`director_update` -- ``ibtk_le_director_update``.
"""
from __future__ import annotations

import ctypes
import os
import sys
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import io
from ._lib import check

__all__ = ["RodArrays", "RodSpecs", "RodForceGen", "director_update", "DIRECTOR_SCHEMES"]

DIRECTOR_SCHEMES = {"euler": 0, "midpoint": 1, "trapezoidal": 2}


class RodArrays(NamedTuple):
    curr: np.ndarray    # (n,) int32 node index of the master ("current") end
    next: np.ndarray    # (n,) int32
    params: np.ndarray  # (n, 10) float64: ds a1 a2 a3 b1 b2 b3 kappa1 kappa2 tau


def _i32(a, n=None):
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32)
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} entries, got {a.size}")
    return a


def _f64(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))


class RodSpecs:
    """The rods of one or more structures, in Lagrangian vertex indices.

    ``rods`` is an ``io.RodDeck`` whose indices already include the structure's vertex
    offset; ``directors`` (or None) is the ``(num_vertex, 9)`` array of initial triads,
    indexed by Lagrangian index (rows below a structure's offset are NaN until
    :meth:`concat` joins the structures).  ``num_vertex`` defaults to the directors' rows,
    or else to the largest index named plus one.
    """

    def __init__(self, rods: io.RodDeck, directors: Optional[np.ndarray] = None, num_vertex: Optional[int] = None):
        self.rods = io.RodDeck(_i32(rods.curr), _i32(rods.next, len(rods.curr)),
                               _f64(rods.params, (len(rods.curr), 10)))
        self.directors = None if directors is None else _f64(directors, (-1, 9))
        if num_vertex is None:
            if self.directors is not None:
                num_vertex = self.directors.shape[0]
            else:
                num_vertex = int(max(self.rods.curr.max(initial=-1), self.rods.next.max(initial=-1))) + 1
        self.num_vertex = int(num_vertex)
        if self.directors is not None and self.directors.shape[0] != self.num_vertex:
            raise ValueError(f"directors has {self.directors.shape[0]} rows, the structures {self.num_vertex} vertices")
        for name, v in (("curr", self.rods.curr), ("next", self.rods.next)):
            if v.size and (v.min() < 0 or v.max() >= self.num_vertex):
                raise ValueError(f"{name} index outside [0, {self.num_vertex})")

    @classmethod
    def from_files(cls, base: str | os.PathLike, vertex_offset: int = 0, num_vertex: Optional[int] = None,
                   uniform_rod_properties: Optional[Sequence[float]] = None) -> "RodSpecs":
        """Read ``base.rod`` and, if it exists, ``base.director``.  ``num_vertex`` is the
        structure's vertex count (None: the count line of ``base.vertex``);
        ``vertex_offset`` is the structure's first Lagrangian index."""
        base = os.fspath(base)
        if num_vertex is None:
            num_vertex = io.read_vertex(base + ".vertex", 3).shape[0]
        rods = io.read_rod(base + ".rod", num_vertex, vertex_offset, uniform_rod_properties)
        D = None
        if os.path.isfile(base + ".director"):
            D = io.read_director(base + ".director", num_vertex)
            if vertex_offset:
                D = np.concatenate([np.full((vertex_offset, 9), np.nan), D])
        return cls(rods, D, vertex_offset + num_vertex)

    @classmethod
    def concat(cls, parts: Sequence["RodSpecs"]) -> "RodSpecs":
        """Join structures read with consecutive vertex offsets (part j's offset = the
        vertices of the parts before it)."""
        if not parts:
            raise ValueError("no structures")
        nv = 0
        for p in parts:
            if p.num_vertex < nv:
                raise ValueError("vertex offsets do not follow the structures' vertex counts")
            lo = min(int(p.rods.curr.min(initial=nv)), int(p.rods.next.min(initial=nv)))
            if lo < nv or (p.directors is not None and not np.all(np.isnan(p.directors[:nv]))):
                raise ValueError("vertex offsets do not follow the structures' vertex counts")
            nv = p.num_vertex
        D = None
        if any(p.directors is not None for p in parts):
            D = np.full((nv, 9), np.nan)
            lo = 0
            for p in parts:
                if p.directors is not None:
                    D[lo:p.num_vertex] = p.directors[lo:]
                lo = p.num_vertex
        rods = io.RodDeck(np.concatenate([p.rods.curr for p in parts]), np.concatenate([p.rods.next for p in parts]),
                          np.concatenate([p.rods.params for p in parts]))
        return cls(rods, D, nv)

    def lagrangian_arrays(self) -> RodArrays:
        """The rods in deck order with Lagrangian indices, every line of a repeated
        ``(curr, next)`` edge carrying the parameters of the edge's first line: the edge
        multimap keeps every line, the spec map's ``insert`` only the first
        (``IBStandardInitializer.cpp:1681-1687``), the rule ``ForceSpecs`` documents for
        springs.  ``(a, b)`` and ``(b, a)`` are different edges."""
        r = self.rods
        key = r.curr.astype(np.int64) * max(self.num_vertex, 1) + r.next.astype(np.int64)
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        src = first[inv.reshape(-1)]
        return RodArrays(r.curr.copy(), r.next.copy(), r.params[src].copy())

    def arrays(self, perm: Optional[np.ndarray] = None) -> RodArrays:
        """The flat arrays in the reference's order (``IBKirchhoffRodForceGen.cpp:167-197``
        walks the local nodes in order and each node's rods in deck order):
        ``perm[lagrangian index] = local node index`` (None: the identity); the rods are
        stably sorted by ``perm[curr]`` and every index is taken through ``perm``."""
        nv = self.num_vertex
        if perm is None:
            perm = np.arange(nv, dtype=np.int64)
        else:
            perm = np.asarray(perm, dtype=np.int64).reshape(-1)
            if perm.size != nv:
                raise ValueError(f"perm has {perm.size} entries, the structures {nv} vertices")
        lag = self.lagrangian_arrays()
        o = np.argsort(perm[lag.curr], kind="stable")
        return RodArrays(_i32(perm[lag.curr][o]), _i32(perm[lag.next][o]), _f64(lag.params[o], (-1, 10)))


def _host_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


RECORD_DTYPE = np.dtype([("curr", "<i4"), ("next", "<i4"), ("p", "<f8", (10,))])


class RodForceGen:
    """A device rod plan over ``n_nodes`` nodes (``ibtk_le_rodgen``).

    ``rods = (curr, next, params)`` are host arrays of node indices in ``[0, n_nodes)`` and
    ``[n][10]`` parameters -- :meth:`RodSpecs.arrays` output fits; ``n_nodes`` may include
    trailing ghost nodes.  The plan is built once (host counting sort, one upload);
    :meth:`compute` then runs one kernel on the context stream.  After a regrid, build the
    new numbering's arrays with ``RodSpecs.arrays(perm)`` and call :meth:`set_rods`.
    """

    def __init__(self, ctx, n_nodes: int, rods=None):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n_nodes = int(n_nodes)
        h = ctypes.c_void_p()
        check(self.lib.ibtk_le_rodgen_create(ctx.h, self.n_nodes, ctypes.byref(h)))
        self.h = h
        if rods is not None:
            self.set_rods(*rods)

    @classmethod
    def from_specs(cls, ctx, specs: RodSpecs, perm=None, n_nodes: Optional[int] = None) -> "RodForceGen":
        return cls(ctx, specs.num_vertex if n_nodes is None else n_nodes, specs.arrays(perm))

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the rod force generator is closed")
        return self.h

    def set_rods(self, curr, next, params):
        curr = _i32(curr)
        n = curr.size
        next, params = _i32(next, n), _f64(params, (n, 10))
        check(self.lib.ibtk_le_rodgen_set_rods(self._handle(), n, _host_ptr(curr), _host_ptr(next), _host_ptr(params)))

    def compute(self, X, D, F=None, N=None, accumulate_F: bool = True, accumulate_N: bool = False):
        """``F += f`` (``accumulate_F``) or ``F = f``, likewise ``N``, with ``f`` and ``n`` the
        rods' force and torque at positions ``X`` (``[n_nodes][3]``) and triads ``D``
        (``[n_nodes][9]``, rows D1 D2 D3); float64 device tensors.  ``F=None`` / ``N=None``
        allocate that result.  The defaults are the reference's: it adds to the ``F`` the
        standard generator left and zeroes ``N`` first.  Returns ``(F, N)``.  No host
        synchronisation."""
        import torch

        from .le import _ptr
        h = self._handle()
        s3, s9 = (self.n_nodes, 3), (self.n_nodes, 9)
        if F is None:
            F = torch.empty(s3, dtype=torch.float64, device=X.device)
            accumulate_F = False
        if N is None:
            N = torch.empty(s3, dtype=torch.float64, device=X.device)
            accumulate_N = False
        for name, t, shape in (("X", X, s3), ("D", D, s9), ("F", F, s3), ("N", N, s3)):
            if t.dtype != torch.float64 or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be a float64 tensor of shape {shape}")
        check(self.lib.ibtk_le_rodgen_compute(self.ctx.h, h, _ptr(X), _ptr(D), _ptr(F), _ptr(N),
                                              int(bool(accumulate_F)), int(bool(accumulate_N))))
        return F, N

    def record_dtype(self) -> np.dtype:
        """The structured dtype of the plan's records: 88 bytes, no padding."""
        return RECORD_DTYPE

    def plan(self):
        """The plan read back (blocking; tests and debugging): ``(offsets, records)``,
        ``n_nodes + 1`` int64 row offsets and a structured array of the entries
        (:meth:`record_dtype`) -- per node its curr-role entries in ascending rod number,
        then its next-role entries in ascending rod number."""
        h = self._handle()
        ne = ctypes.c_longlong()
        check(self.lib.ibtk_le_rodgen_plan_size(h, ctypes.byref(ne)))
        off = np.empty(self.n_nodes + 1, dtype=np.int64)
        rec = np.empty(ne.value, dtype=RECORD_DTYPE)
        check(self.lib.ibtk_le_rodgen_plan_read(h, _host_ptr(off), _host_ptr(rec), rec.nbytes))
        return off, rec

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.ibtk_le_rodgen_destroy(self.h)
        self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def director_update(ctx, scheme: str, dt: float, D, W0, W1=None, out=None):
    """``D_new = R(e, |e| dt) D`` row by row on the device, ``e = W0`` (``"euler"``) or
    ``0.5 (W0 + W1)`` (``"trapezoidal"``); where ``|e| <= DBL_EPSILON`` the triad is copied
    bit for bit (``GeneralizedIBMethod::eulerStep`` / ``trapezoidalStep``,
    GeneralizedIBMethod.cpp:326-447).  ``"midpoint"`` raises, as the reference refuses it.
    ``D`` is ``[n][9]``, ``W0`` / ``W1`` ``[n][3]``; ``out`` may be ``D`` itself.  Returns
    ``out``."""
    import torch

    from .le import _ptr
    if scheme not in DIRECTOR_SCHEMES:
        raise ValueError(f"unknown scheme {scheme!r}")
    if scheme == "trapezoidal" and W1 is None:
        raise ValueError("trapezoidal needs W1")
    if D.dim() != 2 or D.shape[1] != 9 or D.dtype != torch.float64:
        raise ValueError("D must be a float64 tensor of shape (n, 9)")
    n = D.shape[0]
    for name, t in (("W0", W0), ("W1", W1 if scheme == "trapezoidal" else None)):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (n, 3)):
            raise ValueError(f"{name} must be a float64 tensor of shape {(n, 3)}")
    if out is None:
        out = torch.empty_like(D)
    elif out.shape != D.shape or out.dtype != torch.float64:
        raise ValueError("out must match D")
    check(ctx.lib.ibtk_le_director_update(ctx.h, DIRECTOR_SCHEMES[scheme], n, float(dt), _ptr(D), _ptr(W0),
                                          _ptr(W1) if scheme == "trapezoidal" else None, _ptr(out)))
    return out

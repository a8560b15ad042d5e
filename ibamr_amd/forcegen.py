"""Lagrangian force generation on the device: springs, beams and target points.

``IBStandardForceGen::computeLagrangianForce`` (``src/IB/IBStandardForceGen.cpp:265-313``)
produces the ``F`` that ``spread`` consumes, from ``X`` and ``U``, every step between the
position update and the spread.  Three pieces live here:

* :class:`ForceSpecs` -- the host side.  It holds what the deck readers of
  :mod:`ibamr_amd.io` return for one or more structures and flattens it into the arrays
  ``IBStandardForceGen::initialize{Spring,Beam,TargetPoint}LevelData`` cache
  (``:700-776``, ``:894-988``, ``:1101-1148``), in the reference's order: master by master
  in local node order, deck order within a master
  (``IBStandardInitializer::initializeSpecs``, ``IBStandardInitializer.cpp:2815-2952``).

* :class:`ForceGen` -- the device plan built through the C ABI
  (``ibtk_le_forcegen_*``) and its ``compute``: one gather kernel, a lane per node,
  the serial loops' result bit for bit, no host synchronisation.

* :class:`DeviceForceSpecs` -- the specs on the device in Lagrangian indices
  (``ibtk_le_forcespecs``), from which :meth:`ForceGen.renumber` rebuilds the plan on the
  device whenever a regrid renumbers the nodes.

* :class:`ForceJacobian` -- the other half of the strategy,
  ``computeLagrangianForceJacobian`` (``:498-665``): ``dF/dX`` in block-CSR on the device
  (``ibtk_le_forcejac``), its pattern built from the plan, its values bit for bit the serial
  assembly, and the product ``J V``; beside it :meth:`ForceGen.linearized` (the product
  without a matrix) and :meth:`ForceGen.jacobian_nnz` (the preallocation counts).
"""
from __future__ import annotations

import ctypes
import os
import sys
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib, io
from ._lib import check

__all__ = ["SpringArrays", "BeamArrays", "TargetArrays", "ForceSpecs", "ForceGen", "ForceJacobian", "DeviceForceSpecs"]


class SpringArrays(NamedTuple):
    mastr: np.ndarray    # (n,) int32 node index of the master
    slave: np.ndarray    # (n,) int32
    kappa: np.ndarray    # (n,) float64
    rest: np.ndarray     # (n,) float64
    fcn_idx: np.ndarray  # (n,) int32; only 0, the default Hookean law, runs on the device


class BeamArrays(NamedTuple):
    mastr: np.ndarray  # (n,) int32
    next: np.ndarray   # (n,) int32
    prev: np.ndarray   # (n,) int32
    bend: np.ndarray   # (n,) float64
    curv: np.ndarray   # (n, ndim) float64


class TargetArrays(NamedTuple):
    node: np.ndarray   # (n,) int32
    kappa: np.ndarray  # (n,) float64
    eta: np.ndarray    # (n,) float64
    X0: np.ndarray     # (n, ndim) float64 the vertex's initial position


def _i32(a, n=None):
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32)
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} entries, got {a.size}")
    return a


def _f64(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
    return a


class ForceSpecs:
    """The force specifications of one or more structures, in Lagrangian vertex indices.

    ``X0`` is the ``(num_vertex, ndim)`` array of initial vertex positions (the target
    points' anchors); ``springs`` / ``beams`` / ``targets`` are an ``io.SpringDeck`` /
    ``io.BeamDeck`` / ``io.TargetDeck`` (or None) whose indices already include the
    structure's vertex offset.  Several structures are joined with :meth:`concat`.
    """

    def __init__(self, ndim: int, X0: np.ndarray, springs: Optional[io.SpringDeck] = None,
                 beams: Optional[io.BeamDeck] = None, targets: Optional[io.TargetDeck] = None):
        if ndim not in (2, 3):
            raise ValueError("ndim must be 2 or 3")
        self.ndim = ndim
        self.X0 = _f64(X0, (-1, ndim))
        self.springs = springs
        self.beams = beams
        self.targets = targets

    @property
    def num_vertex(self) -> int:
        return self.X0.shape[0]

    @classmethod
    def from_files(cls, base: str | os.PathLike, ndim: int, vertex_offset: int = 0, length_scale: float = 1.0,
                   posn_shift: Optional[Sequence[float]] = None, uniform_stiffness: Optional[float] = None,
                   uniform_rest_length: Optional[float] = None, uniform_force_fcn_idx: Optional[int] = None,
                   uniform_bend_rigidity: Optional[float] = None,
                   uniform_curvature: Optional[Sequence[float]] = None,
                   uniform_target_stiffness: Optional[float] = None,
                   uniform_target_damping: Optional[float] = None) -> "ForceSpecs":
        """Read ``base.vertex`` and whichever of ``base.spring``, ``base.beam`` and
        ``base.target`` exist.  ``vertex_offset`` is the structure's first Lagrangian index
        (the vertex counts of the structures before it)."""
        base = os.fspath(base)
        X0 = io.read_vertex(base + ".vertex", ndim, length_scale, posn_shift)
        nv = X0.shape[0]
        springs = beams = targets = None
        if os.path.isfile(base + ".spring"):
            springs = io.read_spring(base + ".spring", nv, vertex_offset, length_scale, uniform_stiffness,
                                     uniform_rest_length, uniform_force_fcn_idx)
        if os.path.isfile(base + ".beam"):
            beams = io.read_beam(base + ".beam", nv, ndim, vertex_offset, uniform_bend_rigidity, uniform_curvature)
        if os.path.isfile(base + ".target"):
            targets = io.read_target(base + ".target", nv, vertex_offset, uniform_target_stiffness,
                                     uniform_target_damping)
        if vertex_offset:
            # X0 is indexed by Lagrangian index: rows below the offset belong to other structures
            X0 = np.concatenate([np.full((vertex_offset, ndim), np.nan), X0])
        return cls(ndim, X0, springs, beams, targets)

    @classmethod
    def concat(cls, parts: Sequence["ForceSpecs"]) -> "ForceSpecs":
        """Join structures read with consecutive vertex offsets (part j's offset = the rows
        of the parts before it)."""
        if not parts:
            raise ValueError("no structures")
        ndim = parts[0].ndim
        X0 = np.empty((0, ndim))
        for p in parts:
            if p.ndim != ndim:
                raise ValueError("structures of different ndim")
            if p.X0.shape[0] < X0.shape[0] or not np.all(np.isnan(p.X0[:X0.shape[0]])):
                raise ValueError("vertex offsets do not follow the structures' vertex counts")
            X0 = np.concatenate([X0, p.X0[X0.shape[0]:]])

        def join(decks, typ):
            decks = [d for d in decks if d is not None]
            if not decks:
                return None
            cols = []
            for f in typ._fields:
                vals = [getattr(d, f) for d in decks]
                cols.append(sum(vals, []) if isinstance(vals[0], list) else np.concatenate(vals))
            return typ(*cols)

        return cls(ndim, X0, join([p.springs for p in parts], io.SpringDeck),
                   join([p.beams for p in parts], io.BeamDeck), join([p.targets for p in parts], io.TargetDeck))

    def arrays(self, perm: Optional[np.ndarray] = None) -> dict:
        """The flat arrays in the reference's order, as ``{"springs": SpringArrays | None,
        "beams": BeamArrays | None, "targets": TargetArrays | None}``.

        ``perm[lagrangian index] = local node index`` (None: the identity).  The order
        ``le.node_distribution`` returns maps the other way (``order[i]`` = the input index of
        node ``i``): its inverse fits here.

        * An edge has its smaller Lagrangian index first: that vertex is the master
          (``IBStandardInitializer.cpp:979-982``).
        * Springs and beams are sorted stably by the master's local index, so deck order
          survives within a master (the multimaps of ``:983``, ``:1401`` walked at ``:2828``,
          ``:2894``).
        * A repeated edge yields one spring per line, every one with the parameters of the
          edge's first line: the edge multimap keeps each entry, the spec map's ``insert``
          only the first (``:983-987``, ``:2848``).
        * Target points are ordered by local node index.
        """
        nv = self.num_vertex
        if perm is None:
            perm = np.arange(nv, dtype=np.int64)
        else:
            perm = np.asarray(perm, dtype=np.int64).reshape(-1)
            if perm.size != nv:
                raise ValueError(f"perm has {perm.size} entries, the structures {nv} vertices")
        lag = self.lagrangian_arrays()
        out = {"springs": None, "beams": None, "targets": None}
        if lag["springs"] is not None:
            s = lag["springs"]
            o = np.argsort(perm[s.mastr], kind="stable")
            out["springs"] = SpringArrays(_i32(perm[s.mastr][o]), _i32(perm[s.slave][o]), s.kappa[o].copy(),
                                          s.rest[o].copy(), _i32(s.fcn_idx[o]))
        if lag["beams"] is not None:
            b = lag["beams"]
            o = np.argsort(perm[b.mastr], kind="stable")
            out["beams"] = BeamArrays(_i32(perm[b.mastr][o]), _i32(perm[b.next][o]), _i32(perm[b.prev][o]),
                                      b.bend[o].copy(), _f64(b.curv[o], (-1, self.ndim)))
        if lag["targets"] is not None:
            t = lag["targets"]
            o = np.argsort(perm[t.node], kind="stable")
            out["targets"] = TargetArrays(_i32(perm[t.node][o]), t.kappa[o].copy(), t.eta[o].copy(),
                                          _f64(t.X0[o], (-1, self.ndim)))
        return out

    def lagrangian_arrays(self) -> dict:
        """What :meth:`arrays` settles before the numbering comes in: the same dictionary of
        ``SpringArrays`` / ``BeamArrays`` / ``TargetArrays`` (or None), in **deck order** with
        **Lagrangian vertex indices**.

        * A spring's master is the smaller Lagrangian index of its edge.
        * Every line of a repeated edge has the parameters of the edge's first line.
        * A target point carries ``X0[node]``.

        This is what the device spec store (:class:`DeviceForceSpecs`) uploads once;
        ``arrays(perm)`` is its stable sort by ``perm[master]`` with every index taken
        through ``perm``.
        """
        out = {"springs": None, "beams": None, "targets": None}
        if self.springs is not None:
            s = self.springs
            m = np.minimum(s.mastr, s.slave).astype(np.int64)
            v = np.maximum(s.mastr, s.slave).astype(np.int64)
            # src[k]: the first line of k's edge (np.unique's index is the first occurrence)
            _, first, inv = np.unique(m * (max(self.num_vertex, int(v.max(initial=0)) + 1)) + v, return_index=True,
                                      return_inverse=True)
            src = first[inv.reshape(-1)]
            out["springs"] = SpringArrays(_i32(m), _i32(v), s.kappa[src].copy(), s.rest[src].copy(),
                                          _i32(s.fcn_idx[src]))
        if self.beams is not None:
            b = self.beams
            out["beams"] = BeamArrays(_i32(b.mastr), _i32(b.next), _i32(b.prev), b.bend.copy(),
                                      _f64(b.curv, (-1, self.ndim)))
        if self.targets is not None:
            t = self.targets
            out["targets"] = TargetArrays(_i32(t.node), t.kappa.copy(), t.eta.copy(),
                                          _f64(self.X0[t.node], (-1, self.ndim)))
        return out


def _host_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class ForceGen:
    """A device force plan over ``n_nodes`` nodes (``ibtk_le_forcegen``).

    ``springs = (mastr, slave, kappa, rest[, fcn_idx])``, ``beams = (mastr, next, prev, bend,
    curv)`` and ``targets = (node, kappa, eta, X0)`` are host arrays of node indices in
    ``[0, n_nodes)`` -- :meth:`ForceSpecs.arrays` output fits; ``n_nodes`` may include
    trailing ghost nodes.  The plan is built once (host counting sort, one upload);
    :meth:`compute` then runs one kernel on the context stream.
    """

    def __init__(self, ctx, n_nodes: int, ndim: int, springs=None, beams=None, targets=None):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n_nodes = int(n_nodes)
        self.ndim = int(ndim)
        h = ctypes.c_void_p()
        check(self.lib.ibtk_le_forcegen_create(ctx.h, self.ndim, self.n_nodes, ctypes.byref(h)))
        self.h = h
        if springs is not None:
            self.set_springs(*springs)
        if beams is not None:
            self.set_beams(*beams)
        if targets is not None:
            self.set_targets(*targets)

    @classmethod
    def from_specs(cls, ctx, specs: ForceSpecs, perm=None, n_nodes: Optional[int] = None) -> "ForceGen":
        a = specs.arrays(perm)
        return cls(ctx, specs.num_vertex if n_nodes is None else n_nodes, specs.ndim, a["springs"], a["beams"],
                   a["targets"])

    def set_springs(self, mastr, slave, kappa, rest, fcn_idx=None):
        mastr = _i32(mastr)
        n = mastr.size
        slave, kappa, rest = _i32(slave, n), _f64(kappa, (n,)), _f64(rest, (n,))
        fcn = None if fcn_idx is None else _i32(fcn_idx, n)
        check(self.lib.ibtk_le_forcegen_set_springs(self.h, n, _host_ptr(mastr), _host_ptr(slave), _host_ptr(kappa),
                                                    _host_ptr(rest), _host_ptr(fcn)))

    def set_beams(self, mastr, next, prev, bend, curv=None):
        mastr = _i32(mastr)
        n = mastr.size
        next, prev, bend = _i32(next, n), _i32(prev, n), _f64(bend, (n,))
        curv = None if curv is None else _f64(curv, (n, self.ndim))
        check(self.lib.ibtk_le_forcegen_set_beams(self.h, n, _host_ptr(mastr), _host_ptr(next), _host_ptr(prev),
                                                  _host_ptr(bend), _host_ptr(curv)))

    def set_targets(self, node, kappa, eta, X0):
        node = _i32(node)
        n = node.size
        kappa, X0 = _f64(kappa, (n,)), _f64(X0, (n, self.ndim))
        eta = None if eta is None else _f64(eta, (n,))
        check(self.lib.ibtk_le_forcegen_set_targets(self.h, n, _host_ptr(node), _host_ptr(kappa), _host_ptr(eta),
                                                    _host_ptr(X0)))

    def compute(self, X, U=None, F=None, dX=None, accumulate: bool = True):
        """``F += acc`` (``accumulate``) or ``F = acc``, with ``acc`` the spring, beam and
        target-point forces at ``X + dX``; ``[n_nodes][ndim]`` float64 device tensors.
        ``F=None`` allocates the result.  ``U`` may be None unless a target point has a
        non-zero damping coefficient.  Returns ``F``.  No host synchronisation."""
        import torch

        from .le import _ptr
        shape = (self.n_nodes, self.ndim)
        if F is None:
            F = torch.empty(shape, dtype=torch.float64, device=X.device)
            accumulate = False
        for name, t in (("X", X), ("U", U), ("F", F), ("dX", dX)):
            if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != shape):
                raise ValueError(f"{name} must be a float64 tensor of shape {shape}")
        check(self.lib.ibtk_le_forcegen_compute(self.ctx.h, self.h, _ptr(X), _ptr(dX), _ptr(U), _ptr(F),
                                                int(bool(accumulate))))
        return F

    def renumber(self, dspecs: "DeviceForceSpecs", order) -> dict:
        """Replace the whole plan with the one of the numbering ``order`` -- an int32 device
        tensor, ``order[i]`` the Lagrangian index of node ``i`` (what ``le.node_distribution``
        returns), at most ``n_nodes`` long -- built on the device from the spec store
        ``dspecs``: byte for byte the plan ``from_specs(ctx, specs, perm=inverse(order))``
        uploads.  A spec whose master is not in ``order`` is dropped; a kept spec with an
        absent endpoint, an ``order`` entry out of range or a repeated one raise
        ``IBTKLEError`` (ARG) and leave the plan invalid (``compute`` raises) until a
        ``renumber`` or a ``set_*`` succeeds.  Blocks for one small read.  Returns
        :meth:`renumber_stats`."""
        import torch

        from .le import _ptr
        if order.dtype != torch.int32 or order.dim() != 1 or not order.is_contiguous():
            raise ValueError("order must be a contiguous 1-D int32 device tensor")
        check(self.lib.ibtk_le_forcegen_renumber(self.ctx.h, self.h, dspecs.h, _ptr(order), int(order.numel())))
        return self.renumber_stats()

    def renumber_stats(self) -> dict:
        """The last :meth:`renumber`: specs ``kept`` and ``dropped`` per class (springs, beams,
        target points), the device ``bytes`` the plan and its scratch hold, and the device
        ``allocations`` the renumber calls have made so far."""
        out = (ctypes.c_longlong * 8)()
        check(self.lib.ibtk_le_forcegen_renumber_stats(self.h, out))
        return {"kept": tuple(out[0:3]), "dropped": tuple(out[3:6]), "bytes": out[6], "allocations": out[7]}

    def linearized(self, X, V, Y=None, dX=None, X_coef: float = 1.0, U_coef: float = 0.0, accumulate: bool = False):
        """``Y += J V`` (``accumulate``) or ``Y = J V`` with ``J`` the force Jacobian at
        ``X + dX`` (:class:`ForceJacobian`'s matrix), formed and applied contribution by
        contribution straight from the plan: the exact product in place of the
        finite-difference ``compute(dX=...)`` route.  ``[n_nodes][ndim]`` float64 device
        tensors; ``Y=None`` allocates the result.  Returns ``Y``.  No host synchronisation."""
        import torch

        from .le import _ptr
        shape = (self.n_nodes, self.ndim)
        if Y is None:
            Y = torch.empty(shape, dtype=torch.float64, device=X.device)
            accumulate = False
        for name, t in (("X", X), ("V", V), ("Y", Y), ("dX", dX)):
            if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape {shape}")
        check(self.lib.ibtk_le_forcegen_linearized(self.ctx.h, self.h, _ptr(X), _ptr(dX), _ptr(V), float(X_coef),
                                                   float(U_coef), _ptr(Y), int(bool(accumulate))))
        return Y

    def jacobian_nnz(self, n_local: Optional[int] = None, device=None):
        """The preallocation counts of ``computeLagrangianForceJacobianNonzeroStructure`` per
        block row: ``(d_nnz, o_nnz)``, two ``n_nodes`` int32 device tensors.  Nodes with an
        index below ``n_local`` (default: all) are local, the others trailing ghost nodes.
        No host synchronisation."""
        import torch

        from .le import _ptr
        n_local = self.n_nodes if n_local is None else int(n_local)
        if not 0 <= n_local <= self.n_nodes:
            raise ValueError(f"n_local {n_local} is outside [0, {self.n_nodes}]")
        dev = torch.device("cuda", self.ctx.device) if device is None else device
        d = torch.empty(self.n_nodes, dtype=torch.int32, device=dev)
        o = torch.empty(self.n_nodes, dtype=torch.int32, device=dev)
        check(self.lib.ibtk_le_forcegen_jacobian_nnz(self.ctx.h, self.h, n_local, _ptr(d), _ptr(o)))
        return d, o

    def record_dtype(self, cls: int) -> np.dtype:
        """The structured dtype of class ``cls``'s plan records (0 springs, 1 beams, 2 target
        points); no padding."""
        nd = self.ndim
        return np.dtype([
            [("m", "<i4"), ("s", "<i4"), ("kappa", "<f8"), ("rest", "<f8")],
            [("m", "<i4"), ("next", "<i4"), ("prev", "<i4"), ("role", "<i4"), ("bend", "<f8"), ("curv", "<f8", (nd,))],
            [("kappa", "<f8"), ("eta", "<f8"), ("X0", "<f8", (nd,))],
        ][cls])

    def plan(self, cls: int):
        """The plan of class ``cls`` read back (blocking; tests and debugging):
        ``(offsets, records)``, ``n_nodes + 1`` int64 row offsets and a structured array of
        the entries (:meth:`record_dtype`)."""
        ne = ctypes.c_longlong()
        check(self.lib.ibtk_le_forcegen_plan_size(self.h, int(cls), ctypes.byref(ne)))
        off = np.empty(self.n_nodes + 1, dtype=np.int64)
        rec = np.empty(ne.value, dtype=self.record_dtype(cls))
        check(self.lib.ibtk_le_forcegen_plan_read(self.h, int(cls), _host_ptr(off), _host_ptr(rec), rec.nbytes))
        return off, rec

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.ibtk_le_forcegen_destroy(self.h)
        self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class _DeviceArray:
    """A device array of the library's as ``__cuda_array_interface__``: what
    ``torch.as_tensor`` wraps without copying.  It keeps its owner alive."""

    def __init__(self, owner, ptr: int, shape, typestr: str):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr or 0), False),
                                         "version": 2, "strides": None}


class ForceJacobian:
    """The force Jacobian ``dF/dX`` of a :class:`ForceGen` on the device, in block-CSR
    (``ibtk_le_forcejac``): what ``IBStandardForceGen::computeLagrangianForceJacobian``
    (``src/IB/IBStandardForceGen.cpp:498-665``) assembles, bit for bit.

    The pattern is built here, on the device, from ``fg``'s current plan; after a ``fg.set_*``
    or ``fg.renumber`` it is stale -- :meth:`assemble` and :meth:`apply` raise ``IBTKLEError``
    -- until :meth:`rebuild`.  ``ctx`` must be the context ``fg`` was created with.  Only the
    (re)build's last step and :meth:`read` synchronise with the host."""

    def __init__(self, ctx, fg: ForceGen):
        self.ctx = ctx
        self.lib = ctx.lib
        self.fg = fg  # the library reads fg's plan on every assemble: keep it alive
        self.n_nodes = fg.n_nodes
        self.ndim = fg.ndim
        h = ctypes.c_void_p()
        check(self.lib.ibtk_le_forcejac_create(ctx.h, fg.h, ctypes.byref(h)))
        self.h = h

    def _live(self):
        """The handle, for a call into the library: the library reads ``fg``'s plan through the
        Jacobian, so neither may have been closed."""
        if getattr(self, "h", None) is None:
            raise ValueError("the ForceJacobian is closed")
        if getattr(self.fg, "h", None) is None:
            raise ValueError("the ForceGen this ForceJacobian was built from is closed")
        return self.h

    def rebuild(self) -> dict:
        """Build the pattern again from ``fg``'s current plan.  Over a plan with the same counts
        nothing is allocated.  Views from an earlier :meth:`bsr` are invalid afterwards.
        Returns :meth:`stats`."""
        check(self.lib.ibtk_le_forcejac_rebuild(self.ctx.h, self._live()))
        return self.stats()

    def _check(self, **tensors):
        import torch
        shape = (self.n_nodes, self.ndim)
        for name, t in tensors.items():
            if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float64 tensor of shape {shape}")

    def assemble(self, X, dX=None, X_coef: float = 1.0, U_coef: float = 0.0) -> "ForceJacobian":
        """The values at ``X + dX``: every block from ``+0.0``, the contributions added as whole
        blocks in the reference's call order.  No host synchronisation."""
        from .le import _ptr
        self._check(X=X, dX=dX)
        check(self.lib.ibtk_le_forcejac_assemble(self.ctx.h, self._live(), _ptr(X), _ptr(dX), float(X_coef), float(U_coef)))
        return self

    def apply(self, V, Y=None, accumulate: bool = False):
        """``Y += J V`` (``accumulate``) or ``Y = J V``; ``Y=None`` allocates the result.  The
        summation order is fixed: identical bits run to run.  Returns ``Y``."""
        import torch

        from .le import _ptr
        if Y is None:
            Y = torch.empty((self.n_nodes, self.ndim), dtype=torch.float64, device=V.device)
            accumulate = False
        self._check(V=V, Y=Y)
        check(self.lib.ibtk_le_forcejac_apply(self.ctx.h, self._live(), _ptr(V), _ptr(Y), int(bool(accumulate))))
        return Y

    def _pattern(self):
        nb = ctypes.c_longlong()
        rp, cl, vl = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(self.lib.ibtk_le_forcejac_pattern(self._live(), ctypes.byref(nb), ctypes.byref(rp), ctypes.byref(cl),
                                                ctypes.byref(vl)))
        return nb.value, rp.value, cl.value, vl.value

    @property
    def n_blocks(self) -> int:
        return self._pattern()[0]

    def bsr(self):
        """``(rowptr, col, val)`` as torch views of the library's device arrays, no copy:
        ``n_nodes + 1`` int64, ``n_blocks`` int32 ascending within a row, ``(n_blocks, ndim,
        ndim)`` float64 row-major blocks.  Valid until the next :meth:`rebuild`; reads are
        ordered after :meth:`assemble` on the context's stream."""
        import torch
        nb, rp, cl, vl = self._pattern()
        dev = torch.device("cuda", self.ctx.device)
        if self.n_nodes == 0 or nb == 0:
            return (torch.zeros(self.n_nodes + 1, dtype=torch.int64, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev),
                    torch.empty((0, self.ndim, self.ndim), dtype=torch.float64, device=dev))
        return (torch.as_tensor(_DeviceArray(self, rp, (self.n_nodes + 1,), "<i8"), device=dev),
                torch.as_tensor(_DeviceArray(self, cl, (nb,), "<i4"), device=dev),
                torch.as_tensor(_DeviceArray(self, vl, (nb, self.ndim, self.ndim), "<f8"), device=dev))

    def read(self, values: bool = True):
        """``(rowptr, col, val)`` as numpy arrays (blocking; tests and debugging);
        ``values=False`` reads the pattern alone and returns ``val = None``."""
        nb = self._pattern()[0]
        rowptr = np.zeros(self.n_nodes + 1, dtype=np.int64)
        col = np.empty(nb, dtype=np.int32)
        val = np.empty((nb, self.ndim, self.ndim), dtype=np.float64) if values else None
        check(self.lib.ibtk_le_forcejac_read(self._live(), _host_ptr(rowptr), _host_ptr(col), _host_ptr(val), nb))
        return rowptr, col, val

    def stats(self) -> dict:
        """``blocks``, ``candidates`` (nodes + 2 springs + 9 beams), the device ``bytes`` held,
        the device ``allocations`` and ``builds`` so far, and whether the pattern is
        ``current``."""
        out = (ctypes.c_longlong * 6)()
        check(self.lib.ibtk_le_forcejac_stats(self._live(), out))
        return {"blocks": out[0], "candidates": out[1], "bytes": out[2], "allocations": out[3], "builds": out[4],
                "current": bool(out[5])}

    def close(self):
        # destroy frees the Jacobian's own buffers and never looks at fg: it runs whether or not
        # fg was closed first
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.ibtk_le_forcejac_destroy(self.h)
        self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class DeviceForceSpecs:
    """The specs of a :class:`ForceSpecs` on the device, in Lagrangian vertex indices and
    deck order (``ibtk_le_forcespecs``): uploaded here, once per structure set, and then the
    source of every :meth:`ForceGen.renumber`.  ``specs.lagrangian_arrays()`` is what goes
    up; the library validates it on the host first."""

    def __init__(self, ctx, specs: ForceSpecs):
        self.ctx = ctx
        self.lib = ctx.lib
        self.ndim = specs.ndim
        self.num_vertex = specs.num_vertex
        h = ctypes.c_void_p()
        check(self.lib.ibtk_le_forcespecs_create(ctx.h, self.ndim, self.num_vertex, ctypes.byref(h)))
        self.h = h
        a = specs.lagrangian_arrays()
        self.counts = tuple(0 if a[c] is None else int(a[c][0].size) for c in ("springs", "beams", "targets"))
        if a["springs"] is not None:
            s = a["springs"]
            check(self.lib.ibtk_le_forcespecs_set_springs(self.h, s.mastr.size, _host_ptr(s.mastr), _host_ptr(s.slave),
                                                          _host_ptr(_f64(s.kappa, (-1,))), _host_ptr(_f64(s.rest, (-1,))),
                                                          _host_ptr(s.fcn_idx)))
        if a["beams"] is not None:
            b = a["beams"]
            check(self.lib.ibtk_le_forcespecs_set_beams(self.h, b.mastr.size, _host_ptr(b.mastr), _host_ptr(b.next),
                                                        _host_ptr(b.prev), _host_ptr(_f64(b.bend, (-1,))),
                                                        _host_ptr(b.curv)))
        if a["targets"] is not None:
            t = a["targets"]
            check(self.lib.ibtk_le_forcespecs_set_targets(self.h, t.node.size, _host_ptr(t.node),
                                                          _host_ptr(_f64(t.kappa, (-1,))), _host_ptr(_f64(t.eta, (-1,))),
                                                          _host_ptr(t.X0)))

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.ibtk_le_forcespecs_destroy(self.h)
        self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

"""Internal fluid sources and sinks on the device: the cosine-kernel spread of ``Q`` and the
pressure interpolation.

``IBMethod::spreadFluidSource`` (``src/IB/IBMethod.cpp:789-943``) and
``IBMethod::interpolatePressure`` (``:945-1069``) are the two ``IBStrategy`` operations that
do not go through ``LEInteractor``: they carry their own kernel, ``cos_kernel(x, r) = 0.5
(1 + cos(pi x / r)) / r`` (``:124-134``), with a radius per source rounded to whole cells,
on cell-centred data, and ``IBStandardSourceGen::getSourceLocations``
(``src/IB/IBStandardSourceGen.cpp:195-250``) puts each source at the mean of the nodes on its
perimeter.  Two pieces live here:

* :class:`SourceSpecs` -- the host side.  It holds what :func:`ibamr_amd.io.read_source`
  returns for one or more structures (names, radii, and the vertex-to-source map in
  Lagrangian indices) and gives the map in a local numbering.

* :class:`Sources` -- the device plan built through the C ABI (``ibtk_le_sources_*``) and
  its four calls, all on the context stream with no host synchronisation and no allocation
  of the library's: :meth:`Sources.locations`, :meth:`Sources.spread`,
  :meth:`Sources.normalize` and :meth:`Sources.pressure`.

``Q`` and ``P`` are plain device arrays of one double per source: the reference's standard
strategy copies constants into ``Q_src`` (``computeSourceStrengths``, ``:262-270``) and
stores ``P_src`` (``setSourcePressures``); any device code may fill or read them.  One patch;
the reference's sums of ``X_src`` and ``P_src`` over ranks and patches are out of scope.
"""
from __future__ import annotations

import ctypes
import sys
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import io
from ._lib import check

__all__ = ["SourceArrays", "SourceSpecs", "Sources", "R_MAX", "FLAG"]

R_MAX = 16  # the largest radius in cells the weight tables hold (SRC_RMAX of csrc/le_source.h)
FLAG = 32   # the context flag an inconsistent integral latches (SRC_FLAG)


class SourceArrays(NamedTuple):
    radii: np.ndarray   # (n_src,) float64
    node: np.ndarray    # (n,) int32 local node indices, ascending
    source: np.ndarray  # (n,) int32


class SourceSpecs:
    """The sources of one or more structures: ``names`` and ``radii`` per source, and the
    map ``node -> source`` over Lagrangian vertex indices (each vertex at most once)."""

    def __init__(self, names: Sequence[str], radii, node, source, num_vertex: Optional[int] = None):
        self.names: List[str] = [str(s) for s in names]
        self.radii = np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1))
        node = np.asarray(node, dtype=np.int64).reshape(-1)
        source = np.asarray(source, dtype=np.int64).reshape(-1)
        if len(self.names) != self.radii.size:
            raise ValueError("one name and one radius per source")
        if node.size != source.size:
            raise ValueError("node and source must have one entry per source point")
        if self.radii.size and not (np.isfinite(self.radii).all() and (self.radii > 0.0).all()):
            raise ValueError("a source radius must be finite and positive")
        if num_vertex is None:
            num_vertex = int(node.max(initial=-1)) + 1
        self.num_vertex = int(num_vertex)
        if node.size and (node.min() < 0 or node.max() >= self.num_vertex):
            raise ValueError(f"node index outside [0, {self.num_vertex})")
        if source.size and (source.min() < 0 or source.max() >= self.radii.size):
            raise ValueError(f"source index outside [0, {self.radii.size})")
        if np.unique(node).size != node.size:
            raise ValueError("a vertex carries one source: a node is named twice")
        o = np.argsort(node, kind="stable")
        self.node = node[o].astype(np.int32)
        self.source = source[o].astype(np.int32)

    @property
    def num_source(self) -> int:
        return int(self.radii.size)

    @classmethod
    def from_deck(cls, *decks: io.SourceDeck, num_vertex: Optional[int] = None) -> "SourceSpecs":
        """The sources of the decks, each read with its structure's ``vertex_offset`` and with
        ``source_offset`` = the sources of the decks before it (the reference's running
        ``source_offset``, ``IBStandardInitializer.cpp:2668-2673``)."""
        names: List[str] = []
        radii, node, source = [], [], []
        for deck in decks:
            if len(deck.source) and (int(np.min(deck.source)) < len(names)
                                     or int(np.max(deck.source)) >= len(names) + len(deck.names)):
                raise ValueError("source offsets do not follow the decks' source counts")
            names += list(deck.names)
            radii.append(np.asarray(deck.radii, dtype=np.float64))
            node.append(np.asarray(deck.node))
            source.append(np.asarray(deck.source))
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
        return cls(names, cat(radii, np.float64), cat(node, np.int64), cat(source, np.int64), num_vertex)

    def arrays(self, perm: Optional[np.ndarray] = None) -> SourceArrays:
        """The map in a local numbering: ``perm[lagrangian index] = local node index`` (None:
        the identity), sorted by local index -- the order ``getSourceLocations`` meets the
        nodes in (``IBStandardSourceGen.cpp:217-230`` walks the local nodes in order)."""
        if perm is None:
            local = self.node.astype(np.int64)
        else:
            perm = np.asarray(perm, dtype=np.int64).reshape(-1)
            if perm.size != self.num_vertex:
                raise ValueError(f"perm has {perm.size} entries, the structures {self.num_vertex} vertices")
            local = perm[self.node]
        o = np.argsort(local, kind="stable")
        return SourceArrays(self.radii.copy(), np.ascontiguousarray(local[o], dtype=np.int32),
                            np.ascontiguousarray(self.source[o], dtype=np.int32))


def _host_ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


class Sources:
    """A device source plan (``ibtk_le_sources``) over ``n_nodes`` local nodes.

    ``specs`` is a :class:`SourceSpecs` (with ``perm``, its map in that local numbering) or a
    ``(radii, node, source)`` triple of host arrays with local node indices.  The plan -- the
    nodes grouped by source, each group in ascending local index -- and every workspace are
    made here; the four calls then only launch.  After a regrid build a new ``Sources`` from
    ``specs`` and the new ``perm``.
    """

    def __init__(self, ctx, specs, ndim: int = 3, n_nodes: Optional[int] = None, perm=None):
        self.ctx = ctx
        self.lib = ctx.lib
        self.ndim = int(ndim)
        if isinstance(specs, SourceSpecs):
            if n_nodes is None:
                n_nodes = specs.num_vertex
            specs = specs.arrays(perm)
        radii, node, source = specs
        radii = np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1))
        node = np.ascontiguousarray(np.asarray(node).reshape(-1), dtype=np.int32)
        source = np.ascontiguousarray(np.asarray(source).reshape(-1), dtype=np.int32)
        if node.size != source.size:
            raise ValueError("node and source must have one entry per source point")
        if n_nodes is None:
            n_nodes = int(node.max(initial=-1)) + 1
        self.n_nodes, self.n_src = int(n_nodes), int(radii.size)
        h = ctypes.c_void_p()
        check(self.lib.ibtk_le_sources_create(ctx.h, self.ndim, self.n_nodes, self.n_src, _host_ptr(radii), int(node.size),
                                              _host_ptr(node), _host_ptr(source), ctypes.byref(h)))
        self.h = h

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the source plan is closed")
        return self.h

    def _vec(self, t, n, name):
        import torch
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"{name}: {n} float64 values, contiguous, on the device")

    def _field(self, geom, t, name):
        import torch
        if geom.ndim != self.ndim:
            raise ValueError(f"a {geom.ndim}-D geometry for a {self.ndim}-D source plan")
        if t.dtype != torch.float64 or not t.is_cuda:
            raise ValueError(f"{name}: a float64 device tensor")
        if tuple(t.shape) != tuple(geom.array_shape("cell", 0, 1)) or not geom.has_layout(t):
            raise ValueError(f"{name}: the cell-centred array of depth 1 of the geometry (shape "
                             f"{tuple(geom.array_shape('cell', 0, 1))}, its pitch), got shape {tuple(t.shape)}, strides "
                             f"{tuple(t.stride())}")

    def _domain(self, domain):
        if domain is None:
            return None, None
        lo, hi = domain
        if len(lo) != self.ndim or len(hi) != self.ndim:
            raise ValueError("domain: (lower, upper) cell indices, NDIM each")
        return (ctypes.c_int * 3)(*[int(v) for v in lo]), (ctypes.c_int * 3)(*[int(v) for v in hi])

    def locations(self, X, out=None):
        """``X_src[k] = sum_i X[node_i] / count_k`` (``ibtk_le_source_locations``), bit for bit
        the reference's sum.  ``X`` is ``[n_nodes][NDIM]``; returns ``[n_src][NDIM]``."""
        import torch

        from .le import _ptr
        if X.dtype != torch.float64 or not X.is_cuda or not X.is_contiguous() or tuple(X.shape) != (self.n_nodes, self.ndim):
            raise ValueError(f"X: a contiguous float64 device tensor of shape {(self.n_nodes, self.ndim)}")
        if out is None:
            out = torch.empty((self.n_src, self.ndim), dtype=torch.float64, device=X.device)
        self._vec(out, self.n_src * self.ndim, "out")
        check(self.lib.ibtk_le_source_locations(self.ctx.h, self._handle(), _ptr(X), _ptr(out)))
        return out

    def spread(self, geom, q, X_src, Q):
        """``q(i) += Q_n wgt`` over every source's stencil box cut to the patch box
        (``ibtk_le_source_spread``).  ``q`` is the cell-centred array of ``geom``
        (``geom.alloc("cell")[0]``).  No atomics; the result is bit-identical from run to run."""
        from .le import _ptr
        self._field(geom, q, "q")
        self._vec(X_src, self.n_src * self.ndim, "X_src")
        self._vec(Q, self.n_src, "Q")
        check(self.lib.ibtk_le_source_spread(self.ctx.h, self._handle(), ctypes.byref(geom.c), ctypes.c_void_p(q.data_ptr()),
                                             _ptr(X_src), _ptr(Q)))
        return q

    def normalize(self, geom, q, Q, domain=None, normalize: bool = True):
        """The consistency check of the spread and, with ``normalize``, the offsetting flow
        through the lateral boundary cells of ``domain = (lower, upper)``
        (``ibtk_le_source_normalize``).  Returns the device tensor ``{q_total, Q_sum, q_norm,
        integral_after}``.  An inconsistent integral latches context flag 32:
        ``ctx.synchronize()`` then raises."""
        import torch

        from .le import _ptr
        self._field(geom, q, "q")
        self._vec(Q, self.n_src, "Q")
        if normalize and domain is None:
            raise ValueError("the normalisation needs the domain box")
        lo, hi = self._domain(domain)
        out = torch.zeros(4, dtype=torch.float64, device=q.device)
        check(self.lib.ibtk_le_source_normalize(self.ctx.h, self._handle(), ctypes.byref(geom.c),
                                                ctypes.c_void_p(q.data_ptr()), lo, hi, _ptr(Q), int(bool(normalize)),
                                                _ptr(out)))
        return out

    def pressure(self, geom, p, X_src, domain=None, out=None):
        """``P_src[n] = sum p(i) wgt - p_norm`` (``ibtk_le_source_pressure``); ``p_norm`` is
        the mean of ``p`` over the lateral boundary cells of ``domain`` in the patch, 0 when
        ``domain`` is None."""
        import torch

        from .le import _ptr
        self._field(geom, p, "p")
        self._vec(X_src, self.n_src * self.ndim, "X_src")
        lo, hi = self._domain(domain)
        if out is None:
            out = torch.zeros(self.n_src, dtype=torch.float64, device=p.device)
        self._vec(out, self.n_src, "out")
        check(self.lib.ibtk_le_source_pressure(self.ctx.h, self._handle(), ctypes.byref(geom.c),
                                               ctypes.c_void_p(p.data_ptr()), _ptr(X_src), _ptr(out), lo, hi))
        return out

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.ibtk_le_sources_destroy(self.h)
        self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

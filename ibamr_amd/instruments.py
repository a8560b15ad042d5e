"""Flow meters and pressure gauges on the device: ``IBInstrumentPanel`` for one 3-D patch.

``IBMethod::postprocessIntegrateData`` (``src/IB/IBMethod.cpp:411-432``) calls
``updateIBInstrumentationData`` (``:1698-1743``) on every step: it rebuilds every meter's web
from the current marker positions (``IBInstrumentPanel::initializeHierarchyDependentData``,
``src/IB/IBInstrumentPanel.cpp:698-923``) and interpolates the side-centred ``u`` and the
cell-centred ``p`` at each web patch (``readInstrumentData``, ``:925-1182``).  Two pieces live
here:

* :class:`MeterSpecs` -- the host side.  It holds what :func:`ibamr_amd.io.read_inst` returns
  for one or more structures (the meters' names and the map vertex -> (meter, node index) in
  Lagrangian indices) and gives the map in a local numbering.

* :class:`Meters` -- the device plan built through the C ABI (``ibtk_le_meters_*``) and its two
  calls, one launch each on the context stream with no host synchronisation and no
  allocation of the library's: :meth:`Meters.update` and :meth:`Meters.read`.

Every value is the reference's one-rank value bit for bit (``include/ibtk_le.h``).
:func:`log_lines` formats them as ``IBInstrumentPanel::outputLogData`` (``:1361-1406``) does.
One patch on one rank; ``d_total_flow_volume`` is ``flow * dt`` added by the caller.
"""
from __future__ import annotations

import ctypes
import sys
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import io
from ._lib import check

__all__ = ["MeterArrays", "MeterSpecs", "Meters", "log_lines", "MAX_WEB", "FLAG"]

MAX_WEB = 4096  # the most web patches of one meter, P_l * max_web_nodes (MTR_MAX_WEB of csrc/le_meter.h)
FLAG = 64       # the context flag a web wider than max_web_nodes latches (MTR_FLAG)

# ibtk_le_meters_workspace's arrays
_X_CENTROID, _NUM_WEB_NODES, _X_WEB, _DA_WEB, _CELL, _COUNTED, _CENTROID_CELL, _X_PERIMETER = range(8)


class MeterArrays(NamedTuple):
    node: np.ndarray        # (n,) int32 local node indices, ascending
    meter: np.ndarray       # (n,) int32
    meter_node: np.ndarray  # (n,) int32 the node's index on its meter's perimeter


class MeterSpecs:
    """The meters of one or more structures: ``names`` per meter and the map ``node -> (meter,
    meter_node)`` over Lagrangian vertex indices (each vertex at most once; every meter's node
    indices are ``0..P-1``, each once)."""

    def __init__(self, names: Sequence[str], node, meter, meter_node, num_vertex: Optional[int] = None):
        self.names: List[str] = [str(s) for s in names]
        node = np.asarray(node, dtype=np.int64).reshape(-1)
        meter = np.asarray(meter, dtype=np.int64).reshape(-1)
        meter_node = np.asarray(meter_node, dtype=np.int64).reshape(-1)
        if not (node.size == meter.size == meter_node.size):
            raise ValueError("node, meter and meter_node must have one entry per instrumented point")
        if num_vertex is None:
            num_vertex = int(node.max(initial=-1)) + 1
        self.num_vertex = int(num_vertex)
        if node.size and (node.min() < 0 or node.max() >= self.num_vertex):
            raise ValueError(f"node index outside [0, {self.num_vertex})")
        if meter.size and (meter.min() < 0 or meter.max() >= len(self.names)):
            raise ValueError(f"meter index outside [0, {len(self.names)})")
        if meter_node.size and meter_node.min() < 0:
            raise ValueError("a meter node index is negative")
        if np.unique(node).size != node.size:
            raise ValueError("a vertex carries one instrument node: a node is named twice")
        for l in range(len(self.names)):
            mine = np.sort(meter_node[meter == l])
            if mine.size == 0 or not np.array_equal(mine, np.arange(mine.size)):
                raise ValueError(f"meter {l}: its node indices must be 0..P-1, each once")
        o = np.argsort(node, kind="stable")
        self.node = node[o].astype(np.int32)
        self.meter = meter[o].astype(np.int32)
        self.meter_node = meter_node[o].astype(np.int32)

    @property
    def num_meters(self) -> int:
        return len(self.names)

    @property
    def num_perimeter_nodes(self) -> np.ndarray:
        """``P_l`` per meter (``IBInstrumentPanel.cpp:589-625``)."""
        return np.bincount(self.meter, minlength=self.num_meters).astype(np.int64)

    @classmethod
    def from_deck(cls, *decks: io.InstDeck, num_vertex: Optional[int] = None) -> "MeterSpecs":
        """The meters of the decks, each read with its structure's ``vertex_offset`` and with
        ``instrument_offset`` = the meters of the decks before it (the reference's running
        ``instrument_offset``, ``IBStandardInitializer.cpp:2434``, ``:2477``)."""
        names: List[str] = []
        node, meter, meter_node = [], [], []
        for deck in decks:
            if len(deck.meter) and (int(np.min(deck.meter)) < len(names)
                                    or int(np.max(deck.meter)) >= len(names) + len(deck.names)):
                raise ValueError("instrument offsets do not follow the decks' meter counts")
            names += list(deck.names)
            node.append(np.asarray(deck.node))
            meter.append(np.asarray(deck.meter))
            meter_node.append(np.asarray(deck.meter_node))
        cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)  # noqa: E731
        return cls(names, cat(node), cat(meter), cat(meter_node), num_vertex)

    def log_lines(self, time: float, values, X_centroid, flow_conv: float = 1.0, pres_conv: float = 1.0) -> List[str]:
        """:func:`log_lines` with these meters' names."""
        return log_lines(self.names, time, values, X_centroid, flow_conv, pres_conv)

    def arrays(self, perm: Optional[np.ndarray] = None) -> MeterArrays:
        """The map in a local numbering: ``perm[lagrangian index] = local node index`` (None:
        the identity), sorted by local index.  A regrid's renumbering takes this host route,
        as the rod plan's does: build a new :class:`Meters` from the same specs."""
        if perm is None:
            local = self.node.astype(np.int64)
        else:
            perm = np.asarray(perm, dtype=np.int64).reshape(-1)
            if perm.size != self.num_vertex:
                raise ValueError(f"perm has {perm.size} entries, the structures {self.num_vertex} vertices")
            local = perm[self.node]
        o = np.argsort(local, kind="stable")
        as32 = lambda a: np.ascontiguousarray(a[o], dtype=np.int32)  # noqa: E731
        return MeterArrays(as32(local), as32(self.meter), as32(self.meter_node))


def _host_ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


class Meters:
    """A device meter plan (``ibtk_le_meters``) over ``n_nodes`` local nodes.

    ``specs`` is a :class:`MeterSpecs` (with ``perm``, its map in that local numbering) or a
    ``(node, meter, meter_node)`` triple of host arrays with local node indices (the meters
    are then named ``meter_0``, ... as the reference names them without a deck).
    ``max_web_nodes`` (even, >= 2) is the capacity of a web in the radial direction,
    ``num_web_nodes = 2 ceil(r_max / h_finest)`` of the widest meter the run will see; the
    workspace holds ``sum_l P_l * max_web_nodes`` web patches, ``P_l * max_web_nodes <=``
    :data:`MAX_WEB` for every meter.  After a regrid build a new ``Meters`` from ``specs``
    and the new ``perm``.
    """

    def __init__(self, ctx, specs, max_web_nodes: int, n_nodes: Optional[int] = None, perm=None,
                 n_meters: Optional[int] = None):
        self.ctx = ctx
        self.lib = ctx.lib
        if isinstance(specs, MeterSpecs):
            if n_nodes is None:
                n_nodes = specs.num_vertex
            self.names = list(specs.names)
            n_meters = specs.num_meters
            specs = specs.arrays(perm)
        else:
            self.names = None
        node, meter, meter_node = (np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32) for a in specs)
        if not (node.size == meter.size == meter_node.size):
            raise ValueError("node, meter and meter_node must have one entry per instrumented point")
        if n_nodes is None:
            n_nodes = int(node.max(initial=-1)) + 1
        self.n_nodes = int(n_nodes)
        self.n_meters = int(meter.max(initial=-1)) + 1 if n_meters is None else int(n_meters)
        if self.names is None:
            self.names = [f"meter_{l}" for l in range(self.n_meters)]  # IBInstrumentPanel.cpp:649-654
        self.max_web_nodes = int(max_web_nodes)
        h = ctypes.c_void_p()
        check(self.lib.ibtk_le_meters_create(ctx.h, self.n_nodes, self.n_meters, int(node.size), _host_ptr(node),
                                             _host_ptr(meter), _host_ptr(meter_node), self.max_web_nodes, ctypes.byref(h)))
        self.h = h
        # P_l and the first web patch of meter l in the workspace
        self.num_perimeter_nodes = np.zeros(self.n_meters, dtype=np.int64)
        if meter.size:
            np.maximum.at(self.num_perimeter_nodes, meter.astype(np.int64), meter_node.astype(np.int64) + 1)
        self.web_offset = self.max_web_nodes * np.concatenate([[0], np.cumsum(self.num_perimeter_nodes)]).astype(np.int64)

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the meter plan is closed")
        return self.h

    # ---- the two device calls -------------------------------------------------------------------

    def update(self, geom, X, domain=None, h_finest: Optional[float] = None):
        """The webs at the marker positions ``X`` (``[n_nodes][3]``):
        ``initializeHierarchyDependentData`` for one level that is one patch
        (``ibtk_le_meters_update``).  ``domain = (lower, upper, x_lower, x_upper)`` is the frame
        ``IndexUtilities::getCellIndex`` works in (None: the patch), ``h_finest`` the finest grid
        spacing (None: ``min(geom.dx)``).  A web wider than ``max_web_nodes`` latches context
        flag 64: ``ctx.synchronize()`` then raises, and that meter reads NaN."""
        import torch

        from .le import _ptr
        if geom.ndim != 3:
            raise ValueError("flow meters need a 3-D patch (the reference has no 2-D flow meters)")
        if X.dtype != torch.float64 or not X.is_cuda or not X.is_contiguous() or tuple(X.shape) != (self.n_nodes, 3):
            raise ValueError(f"X: a contiguous float64 device tensor of shape {(self.n_nodes, 3)}")
        if domain is None:
            domain = (geom.ilower, geom.iupper, geom.x_lower, geom.x_upper)
        lo, hi, xlo, xup = domain
        if not (len(lo) == len(hi) == len(xlo) == len(xup) == 3):
            raise ValueError("domain: (lower, upper, x_lower, x_upper), 3 each")
        if h_finest is None:
            h_finest = min(float(v) for v in geom.dx)
        I3, D3 = ctypes.c_int * 3, ctypes.c_double * 3
        check(self.lib.ibtk_le_meters_update(self.ctx.h, self._handle(), ctypes.byref(geom.c), I3(*[int(v) for v in lo]),
                                             I3(*[int(v) for v in hi]), D3(*[float(v) for v in xlo]),
                                             D3(*[float(v) for v in xup]), float(h_finest), _ptr(X)))

    def read(self, geom, u, p, U, out=None):
        """``{flow, mean pressure, point pressure}`` per meter, shape ``(n_meters, 3)``:
        ``readInstrumentData`` (``ibtk_le_meters_read``).  ``u`` is the side-centred velocity of
        ``geom`` (``geom.alloc("side")``) or None (flow = 0 - correction), ``p`` the cell-centred
        pressure (``geom.alloc("cell")[0]``) or None (NaN and 0), ``U`` the marker velocities
        ``[n_nodes][3]``."""
        import torch

        from .le import _ptr, _ptr_array
        if geom.ndim != 3:
            raise ValueError("flow meters need a 3-D patch (the reference has no 2-D flow meters)")
        if U.dtype != torch.float64 or not U.is_cuda or not U.is_contiguous() or tuple(U.shape) != (self.n_nodes, 3):
            raise ValueError(f"U: a contiguous float64 device tensor of shape {(self.n_nodes, 3)}")
        if u is not None:
            if len(u) != 3 or any(tuple(a.shape) != tuple(geom.array_shape("side", c)) or not geom.has_layout(a)
                                  for c, a in enumerate(u)):
                raise ValueError("u: the three side-centred arrays of the geometry (their shapes, its pitch)")
            u_ptr = _ptr_array(u, geom)
        else:
            u_ptr = None
        if p is not None:
            if p.dtype != torch.float64 or not p.is_cuda or tuple(p.shape) != tuple(geom.array_shape("cell", 0, 1)) \
                    or not geom.has_layout(p):
                raise ValueError("p: the cell-centred array of depth 1 of the geometry (its shape, its pitch)")
        if out is None:
            out = torch.zeros((self.n_meters, 3), dtype=torch.float64, device=U.device)
        if out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or out.numel() != 3 * self.n_meters:
            raise ValueError(f"out: {3 * self.n_meters} float64 values, contiguous, on the device")
        check(self.lib.ibtk_le_meters_read(self.ctx.h, self._handle(), ctypes.byref(geom.c), u_ptr,
                                           ctypes.c_void_p(p.data_ptr()) if p is not None else None, _ptr(U), _ptr(out)))
        return out

    # ---- the plan's workspace, read only --------------------------------------------------------
    # Each is a copy made on the context stream (ibtk_le_meters_workspace): a snapshot that
    # outlives the plan and that nothing written to reaches the plan through.

    def _copy(self, which: int, shape, dtype):
        import torch
        out = torch.empty(shape, dtype=dtype, device=f"cuda:{self.ctx.device}")
        check(self.lib.ibtk_le_meters_workspace(self.ctx.h, self._handle(), which, ctypes.c_void_p(out.data_ptr()),
                                                out.numel()))
        return out

    @property
    def X_centroid(self):
        """``(n_meters, 3)`` float64."""
        import torch
        return self._copy(_X_CENTROID, (self.n_meters, 3), torch.float64)

    @property
    def num_web_nodes(self):
        """``(n_meters,)`` int32: ``2 int(ceil(r_max / h_finest))`` of the last update (-1: no
        int holds it); a value above ``max_web_nodes`` marks a meter that latched flag 64."""
        import torch
        return self._copy(_NUM_WEB_NODES, (self.n_meters,), torch.int32)

    @property
    def centroid_cell(self):
        """``(n_meters, 4)`` int32: the centroid's cell, then whether it is counted."""
        import torch
        return self._copy(_CENTROID_CELL, (self.n_meters, 4), torch.int32)

    @property
    def X_perimeter(self):
        """A list per meter of ``(P_l, 3)`` float64."""
        import torch
        S = int(self.num_perimeter_nodes.sum())
        flat = self._copy(_X_PERIMETER, (S, 3), torch.float64)
        o = np.concatenate([[0], np.cumsum(self.num_perimeter_nodes)]).astype(np.int64)
        return [flat[int(o[l]):int(o[l + 1])] for l in range(self.n_meters)]

    def _webs(self, which: int, width: int, dtype):
        """A list per meter of ``(P_l, nw_l[, width])`` tensors; None for a meter whose web
        does not fit.  Reads ``num_web_nodes`` back: it synchronises the stream."""
        W = int(self.web_offset[-1])
        flat = self._copy(which, (W, width) if width else (W,), dtype)
        nw = self.num_web_nodes.cpu().numpy()
        out = []
        for l in range(self.n_meters):
            P, n = int(self.num_perimeter_nodes[l]), int(nw[l])
            if n < 0 or n > self.max_web_nodes:
                out.append(None)
                continue
            part = flat[int(self.web_offset[l]):int(self.web_offset[l]) + P * n]
            out.append(part.reshape((P, n, width) if width else (P, n)))
        return out

    @property
    def X_web(self):
        import torch
        return self._webs(_X_WEB, 3, torch.float64)

    @property
    def dA_web(self):
        import torch
        return self._webs(_DA_WEB, 3, torch.float64)

    @property
    def cell(self):
        import torch
        return self._webs(_CELL, 3, torch.int32)

    @property
    def counted(self):
        import torch
        return self._webs(_COUNTED, 0, torch.int32)

    def log_lines(self, time: float, values, X_centroid, flow_conv: float = 1.0, pres_conv: float = 1.0) -> List[str]:
        """:func:`log_lines` with the plan's names."""
        return log_lines(self.names, time, values, X_centroid, flow_conv, pres_conv)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.ibtk_le_meters_destroy(self.h)
        self.h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():  # (at interpreter exit the module's globals may be gone)
            return
        try:
            self.close()
        except Exception:
            pass


def log_lines(names: Sequence[str], time: float, values, X_centroid, flow_conv: float = 1.0,
              pres_conv: float = 1.0) -> List[str]:
    """The lines ``IBInstrumentPanel::outputLogData`` (``:1361-1406``) writes, one per meter:
    the name padded to the longest name, the time and the centroid as ``%.5e``, ``flow_conv *
    flow``, ``pres_conv * mean pressure`` and ``pres_conv * point pressure`` as ``%+.5e``, two
    spaces before each field.  ``values`` is ``(n_meters, 3)``, ``X_centroid`` ``(n_meters, 3)``
    (host arrays).  A NaN prints as Python prints it (``+nan``; the C++ stream prints the NaN's own
    sign)."""
    values = np.asarray(values, dtype=np.float64).reshape(-1, 3)
    X_centroid = np.asarray(X_centroid, dtype=np.float64).reshape(-1, 3)
    if not (len(names) == values.shape[0] == X_centroid.shape[0]):
        raise ValueError("one name, one value triple and one centroid per meter")
    width = max((len(s) for s in names), default=0)
    lines = []
    for l, name in enumerate(names):
        fields = [name.ljust(width), "%.5e" % float(time)]
        fields += ["%.5e" % float(v) for v in X_centroid[l]]
        fields += ["%+.5e" % (flow_conv * float(values[l, 0])), "%+.5e" % (pres_conv * float(values[l, 1])),
                   "%+.5e" % (pres_conv * float(values[l, 2]))]
        lines.append("  ".join(fields))
    return lines

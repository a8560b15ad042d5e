"""Wire and disk formats at the edges of the LE path.

These formats let marker data move between this library and an IBAMR run:

* ``.vertex`` files, the input-deck format of ``IBStandardInitializer``
  (reader: ``src/IB/IBStandardInitializer.cpp:725-790``; sample:
  ``examples/IB/explicit/ex1/curve2d_64.vertex``).  Line 1 holds the vertex count.
  Each following line holds one vertex, NDIM coordinates.  Text after ``!``,
  ``#`` or ``%`` on a line is a comment (``discard_comments``, same file
  :101-123).  Extra tokens after the NDIM coordinates are ignored, as
  ``istringstream >>`` ignores them.  The reader applies
  ``X = length_scale * (X + posn_shift)`` per coordinate (:776).  Errors follow the
  reference's messages: premature end of file, invalid entry, count <= 0.

* ``.spring``, ``.beam`` and ``.target`` files, the force-specification decks that sit
  beside a ``.vertex`` file (readers: ``IBStandardInitializer.cpp:803-1006``,
  ``:1240-1405``, ``:1740-1870``; samples: ``examples/IB/explicit/ex3/fila_256.*``).
  Line 1 holds the record count; each following line holds vertex indices and material
  parameters.  ``ibamr_amd.forcegen.ForceSpecs`` turns them into the flat arrays
  ``IBStandardForceGen`` caches.

* ``.rod`` and ``.director`` files, the decks of ``IBKirchhoffRodForceGen`` /
  ``GeneralizedIBMethod`` (readers: ``IBStandardInitializer.cpp:1407-1700``,
  ``:2137-2260``; samples: ``examples/IB/explicit/ex4/curve3d_64.*``).  A ``.rod`` line
  holds an edge ``curr next`` and ten material parameters; a ``.director`` file holds
  three lines per vertex, the triad ``D1 D2 D3``.  ``ibamr_amd.rods.RodSpecs`` turns them
  into the arrays the rod force generator caches.

* ``.source`` files, the deck of internal fluid sources and sinks (reader:
  ``IBStandardInitializer.cpp:2495-2691``): the sources' names and radii, then the
  vertices on each source's perimeter.  ``ibamr_amd.sources.SourceSpecs`` turns them into
  the arrays the source plan takes.

* ``.inst`` files, the deck of flow meters and pressure gauges (reader:
  ``IBStandardInitializer.cpp:2257-2493``): the instruments' names, then the vertices on each
  meter's perimeter with their position on it.  ``ibamr_amd.instruments.MeterSpecs`` turns them
  into the arrays the meter plan takes.

* The ``LNodeIndex`` stream record (``ibtk/include/ibtk/private/LNodeIndex-inl.h:148-172``):
  three ``int`` (Lagrangian index, global PETSc index, local PETSc index), then
  the periodic offset ``int[NDIM]``, then the periodic displacement
  ``double[NDIM]``.  ``LTransaction::packStream``
  (``ibtk/src/lagrangian/LTransaction.cpp:128-140``) frames a batch as an ``int``
  count, then per item its record and its position ``double[NDIM]``.  IBTK's
  ``FixedSizedStream`` packs these with ``memcpy`` into one buffer, so the bytes
  are host order (little-endian here) with no padding between fields.  SAMRAI's
  ``AbstractStream::sizeofInt/sizeofDouble`` may round each ``pack()`` call up to
  an alignment.  SAMRAI is absent from this image, so that rounding cannot be
  checked; ``align`` exposes it and defaults to 1 (parity unpinned for
  ``align > 1``).

These are host-side formats, so they live in numpy.  The structured arrays map
one-to-one onto ``slab.migrate`` fields: ``X`` is the position, and the index
columns travel as payload.
"""
from __future__ import annotations

import os
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

__all__ = [
    "read_vertex", "write_vertex",
    "SpringDeck", "BeamDeck", "TargetDeck",
    "read_spring", "write_spring", "read_beam", "write_beam", "read_target", "write_target",
    "RodDeck", "read_rod", "write_rod", "read_director", "write_director",
    "SourceDeck", "read_source", "write_source",
    "InstDeck", "read_inst", "write_inst",
    "lnode_index_dtype", "lnode_index_stream_size", "pack_lnode_indices", "unpack_lnode_indices",
    "pack_ltransaction", "unpack_ltransaction",
]

_COMMENT_CHARS = "!#%"


def _discard_comments(line: str) -> str:
    """IBStandardInitializer.cpp:101-123: cut at the first '!', then '#', then '%'."""
    for c in _COMMENT_CHARS:
        k = line.find(c)
        if k >= 0:
            line = line[:k]
    return line


def read_vertex(path: str | os.PathLike, ndim: int = 3, length_scale: float = 1.0,
                posn_shift: Optional[Sequence[float]] = None) -> np.ndarray:
    """Read a ``.vertex`` file into an ``(N, ndim)`` float64 array.

    Follows IBStandardInitializer::readVertexFiles (IBStandardInitializer.cpp:725-790).
    Raises ``ValueError`` with the reference's wording on malformed input.
    """
    if ndim not in (2, 3):
        raise ValueError("ndim must be 2 or 3")
    shift = np.zeros(ndim) if posn_shift is None else np.asarray(posn_shift, dtype=np.float64)
    if shift.shape != (ndim,):
        raise ValueError("posn_shift must have ndim entries")
    name = os.fspath(path)
    if not os.path.isfile(name):
        raise FileNotFoundError(f"Cannot find required vertex file: {name}")
    with open(name, "r") as fh:
        first = fh.readline()
        if not first:
            raise ValueError(f"Premature end to input file encountered before line 1 of file {name}")
        tok = _discard_comments(first).split()
        try:
            n = int(tok[0])
        except (IndexError, ValueError):
            raise ValueError(f"Invalid entry in input file encountered on line 1 of file {name}") from None
        if n <= 0:
            raise ValueError(f"Invalid entry in input file encountered on line 1 of file {name}")
        X = np.empty((n, ndim), dtype=np.float64)
        for k in range(n):
            line = fh.readline()
            if not line:
                raise ValueError(f"Premature end to input file encountered before line {k + 2} of file {name}")
            tok = _discard_comments(line).split()
            if len(tok) < ndim:
                raise ValueError(f"Invalid entry in input file encountered on line {k + 2} of file {name}")
            try:
                X[k] = [float(t) for t in tok[:ndim]]
            except ValueError:
                raise ValueError(f"Invalid entry in input file encountered on line {k + 2} of file {name}") from None
    return length_scale * (X + shift)


def write_vertex(path: str | os.PathLike, X: np.ndarray) -> None:
    """Write ``X`` (N, ndim) as a ``.vertex`` file.

    Uses the sample files' style: 17 significant digits in ``%.16e``, so a read
    gives the same doubles back bit for bit.
    """
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] not in (2, 3) or X.shape[0] == 0:
        raise ValueError("X must be (N>0, 2|3)")
    with open(os.fspath(path), "w") as fh:
        fh.write(f"{X.shape[0]}\n")
        np.savetxt(fh, X, fmt="%.16e", delimiter=" ")


class SpringDeck(NamedTuple):
    """A ``.spring`` file in deck order; edges normalised so ``mastr < slave``."""
    mastr: np.ndarray    # (n,) int32
    slave: np.ndarray    # (n,) int32
    kappa: np.ndarray    # (n,) float64 spring constant
    rest: np.ndarray     # (n,) float64 resting length (times length_scale)
    fcn_idx: np.ndarray  # (n,) int32 force function index (0: the default Hookean law)
    extra: List[np.ndarray]  # per line, the parameters after the function index


class BeamDeck(NamedTuple):
    """A ``.beam`` file in deck order (the file's columns are prev, mastr, next)."""
    mastr: np.ndarray  # (n,) int32, the "current" vertex
    next: np.ndarray   # (n,) int32
    prev: np.ndarray   # (n,) int32
    bend: np.ndarray   # (n,) float64 bending rigidity
    curv: np.ndarray   # (n, ndim) float64 mesh-dependent curvature


class TargetDeck(NamedTuple):
    """A ``.target`` file: one entry per vertex named, in order of first appearance."""
    node: np.ndarray   # (n,) int32
    kappa: np.ndarray  # (n,) float64 penalty spring constant
    eta: np.ndarray    # (n,) float64 damping coefficient


class _Deck:
    """Line reader shared by the force-spec decks: the count line, then one record per
    line, comments cut, errors in the reference's wording (IBStandardInitializer.cpp:
    842-862, 871-926)."""

    def __init__(self, path, what: str):
        self.name = os.fspath(path)
        if not os.path.isfile(self.name):
            raise FileNotFoundError(f"Cannot find {what} file: {self.name}")
        self.line = 0

    def __enter__(self):
        self.fh = open(self.name, "r")
        return self

    def __exit__(self, *exc):
        self.fh.close()

    def invalid(self, detail: str = ""):
        msg = f"Invalid entry in input file encountered on line {self.line} of file {self.name}"
        return ValueError(msg + (f"\n  {detail}" if detail else ""))

    def tokens(self) -> List[str]:
        self.line += 1
        line = self.fh.readline()
        if not line:
            raise ValueError(f"Premature end to input file encountered before line {self.line} of file {self.name}")
        return _discard_comments(line).split()

    def count(self) -> int:
        tok = self.tokens()
        try:
            n = int(tok[0])
        except (IndexError, ValueError):
            raise self.invalid() from None
        if n <= 0:
            raise self.invalid()
        return n

    def index(self, tok: List[str], col: int, num_vertex: int) -> int:
        try:
            i = int(tok[col])
        except (IndexError, ValueError):
            raise self.invalid() from None
        if i < 0 or i >= num_vertex:
            raise self.invalid(f"vertex index {i} is out of range")
        return i

    def value(self, tok: List[str], col: int, negative: str) -> float:
        try:
            v = float(tok[col])
        except (IndexError, ValueError):
            raise self.invalid() from None
        if v < 0.0:
            raise self.invalid(negative)
        return v


def read_spring(path: str | os.PathLike, num_vertex: int, vertex_offset: int = 0, length_scale: float = 1.0,
                uniform_stiffness: Optional[float] = None, uniform_rest_length: Optional[float] = None,
                uniform_force_fcn_idx: Optional[int] = None) -> SpringDeck:
    """Read a ``.spring`` file: per line ``idx1 idx2 kappa rest [fcn_idx [params...]]``.

    Follows IBStandardInitializer::readSpringFiles (IBStandardInitializer.cpp:803-1006):
    indices are checked against ``[0, num_vertex)``, the rest length is scaled by
    ``length_scale`` (:927), a missing function index is 0, further parameters are kept,
    the uniform overrides replace the line's values (:943-954), ``vertex_offset`` is
    added, and an edge is stored with its smaller index first (:979-982).
    """
    with _Deck(path, "spring") as deck:
        n = deck.count()
        mastr, slave = np.empty(n, np.int32), np.empty(n, np.int32)
        kappa, rest, fcn = np.empty(n), np.empty(n), np.zeros(n, np.int32)
        extra: List[np.ndarray] = []
        for k in range(n):
            tok = deck.tokens()
            a = deck.index(tok, 0, num_vertex)
            b = deck.index(tok, 1, num_vertex)
            kappa[k] = deck.value(tok, 2, "spring constant is negative")
            rest[k] = deck.value(tok, 3, "spring resting length is negative") * length_scale
            more: List[float] = []
            try:
                fcn[k] = int(tok[4])
                for t in tok[5:]:
                    more.append(float(t))
            except (IndexError, ValueError):
                pass  # as the reference's stream extraction stops at the first token it cannot read
            extra.append(np.asarray(more, dtype=np.float64))
            if uniform_stiffness is not None:
                kappa[k] = uniform_stiffness
            if uniform_rest_length is not None:
                rest[k] = uniform_rest_length
            if uniform_force_fcn_idx is not None:
                fcn[k] = uniform_force_fcn_idx
            mastr[k], slave[k] = min(a, b) + vertex_offset, max(a, b) + vertex_offset
    return SpringDeck(mastr, slave, kappa, rest, fcn, extra)


def read_beam(path: str | os.PathLike, num_vertex: int, ndim: int = 3, vertex_offset: int = 0,
              uniform_bend_rigidity: Optional[float] = None,
              uniform_curvature: Optional[Sequence[float]] = None) -> BeamDeck:
    """Read a ``.beam`` file: per line ``prev curr next bend [curv_0 .. curv_{ndim-1}]``.

    Follows IBStandardInitializer::readBeamFiles (IBStandardInitializer.cpp:1240-1405): a
    missing curvature is the zero vector, a partial one an error (:1339-1359).
    """
    if ndim not in (2, 3):
        raise ValueError("ndim must be 2 or 3")
    ucurv = None if uniform_curvature is None else np.asarray(uniform_curvature, dtype=np.float64)
    if ucurv is not None and ucurv.shape != (ndim,):
        raise ValueError("uniform_curvature must have ndim entries")
    with _Deck(path, "beam") as deck:
        n = deck.count()
        mastr, nxt, prev = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        bend, curv = np.empty(n), np.zeros((n, ndim))
        for k in range(n):
            tok = deck.tokens()
            prev[k] = deck.index(tok, 0, num_vertex) + vertex_offset
            mastr[k] = deck.index(tok, 1, num_vertex) + vertex_offset
            nxt[k] = deck.index(tok, 2, num_vertex) + vertex_offset
            bend[k] = deck.value(tok, 3, "beam constant is negative")
            for d in range(ndim):
                try:
                    curv[k, d] = float(tok[4 + d])
                except (IndexError, ValueError):
                    if d > 0:
                        raise deck.invalid("incomplete beam curvature specification") from None
                    break
            if uniform_bend_rigidity is not None:
                bend[k] = uniform_bend_rigidity
            if ucurv is not None:
                curv[k] = ucurv
    return BeamDeck(mastr, nxt, prev, bend, curv)


def read_target(path: str | os.PathLike, num_vertex: int, vertex_offset: int = 0,
                uniform_target_stiffness: Optional[float] = None,
                uniform_target_damping: Optional[float] = None) -> TargetDeck:
    """Read a ``.target`` file: per line ``idx kappa [eta]``; a missing damping column is 0.

    Follows IBStandardInitializer::readTargetPointFiles (IBStandardInitializer.cpp:
    1740-1870).  The reference keeps one specification per vertex of the structure (zero
    where the file names none; a vertex named twice keeps its last line), and a uniform
    override sets it on every vertex (:1857-1870): with one given, the result covers
    vertices ``0 .. num_vertex-1`` in index order; otherwise the vertices the file names.
    """
    spec: dict = {}
    with _Deck(path, "target point") as deck:
        n = deck.count()
        for _ in range(n):
            tok = deck.tokens()
            i = deck.index(tok, 0, num_vertex)
            k = deck.value(tok, 1, "target point spring constant is negative")
            e = 0.0
            if len(tok) > 2:
                try:
                    e = float(tok[2])
                except ValueError:
                    e = 0.0
                if e < 0.0:
                    raise deck.invalid("target point damping coefficient is negative")
            spec[i] = (k, e)
    if uniform_target_stiffness is not None or uniform_target_damping is not None:
        spec = {i: spec.get(i, (0.0, 0.0)) for i in range(num_vertex)}
    node = np.fromiter(spec.keys(), dtype=np.int32, count=len(spec)) + np.int32(vertex_offset)
    kappa = np.array([v[0] for v in spec.values()], dtype=np.float64)
    eta = np.array([v[1] for v in spec.values()], dtype=np.float64)
    if uniform_target_stiffness is not None:
        kappa[:] = uniform_target_stiffness
    if uniform_target_damping is not None:
        eta[:] = uniform_target_damping
    return TargetDeck(node, kappa, eta)


def _write_deck(path, rows: List[str]) -> None:
    if not rows:
        raise ValueError("a deck holds at least one entry")
    with open(os.fspath(path), "w") as fh:
        fh.write(f"{len(rows)}\n")
        fh.write("\n".join(rows) + "\n")


def write_spring(path: str | os.PathLike, mastr, slave, kappa, rest, fcn_idx=None, extra=None) -> None:
    """Write a ``.spring`` file (``%.16e``: a read gives the same doubles back).  The
    function index column is written when ``fcn_idx`` or ``extra`` is given."""
    n = len(mastr)
    rows = []
    for k in range(n):
        row = f"{int(mastr[k]):6d} {int(slave[k]):6d} {float(kappa[k]):.16e} {float(rest[k]):.16e}"
        if fcn_idx is not None or extra is not None:
            row += f" {int(fcn_idx[k]) if fcn_idx is not None else 0:d}"
            if extra is not None:
                row += "".join(f" {float(v):.16e}" for v in extra[k])
        rows.append(row)
    _write_deck(path, rows)


def write_beam(path: str | os.PathLike, mastr, next, prev, bend, curv=None) -> None:
    """Write a ``.beam`` file (columns prev, mastr, next, bend and, if given, the curvature)."""
    rows = []
    for k in range(len(mastr)):
        row = f"{int(prev[k]):6d} {int(mastr[k]):6d} {int(next[k]):6d} {float(bend[k]):.16e}"
        if curv is not None:
            row += "".join(f" {float(v):.16e}" for v in curv[k])
        rows.append(row)
    _write_deck(path, rows)


def write_target(path: str | os.PathLike, node, kappa, eta=None) -> None:
    """Write a ``.target`` file (``idx kappa`` and, if given, the damping column)."""
    rows = []
    for k in range(len(node)):
        row = f"{int(node[k]):6d} {float(kappa[k]):.16e}"
        if eta is not None:
            row += f" {float(eta[k]):.16e}"
        rows.append(row)
    _write_deck(path, rows)


class RodDeck(NamedTuple):
    """A ``.rod`` file in deck order, edges as written: ``curr`` is the master."""
    curr: np.ndarray    # (n,) int32
    next: np.ndarray    # (n,) int32
    params: np.ndarray  # (n, 10) float64: ds a1 a2 a3 b1 b2 b3 kappa1 kappa2 tau


ROD_PARAMS = ("ds", "a1", "a2", "a3", "b1", "b2", "b3", "kappa1", "kappa2", "tau")


def read_rod(path: str | os.PathLike, num_vertex: int, vertex_offset: int = 0,
             uniform_rod_properties: Optional[Sequence[float]] = None) -> RodDeck:
    """Read a ``.rod`` file: per line ``curr next ds a1 a2 a3 b1 b2 b3 [kappa1 [kappa2 [tau]]]``.

    Follows IBStandardInitializer::readRodFiles (IBStandardInitializer.cpp:1455-1688):
    indices are checked against ``[0, num_vertex)`` before ``vertex_offset`` is added, a
    negative ``ds``, ``a*`` or ``b*`` is an error, missing curvature fields are 0 (the
    reference only warns when some but not all are given), ``uniform_rod_properties`` (10
    values) replaces a line's whole property vector (:1664-1667), and the edge is kept as
    written -- ``curr`` is the master (:1681-1684); unlike a spring's, the smaller index
    does not become the master.
    """
    uni = None if uniform_rod_properties is None else np.asarray(uniform_rod_properties, dtype=np.float64)
    if uni is not None and uni.shape != (10,):
        raise ValueError("uniform_rod_properties must have 10 entries")
    with _Deck(path, "rod") as deck:
        n = deck.count()
        curr, nxt = np.empty(n, np.int32), np.empty(n, np.int32)
        params = np.zeros((n, 10))
        for k in range(n):
            tok = deck.tokens()
            curr[k] = deck.index(tok, 0, num_vertex) + vertex_offset
            nxt[k] = deck.index(tok, 1, num_vertex) + vertex_offset
            for j in range(7):
                params[k, j] = deck.value(tok, 2 + j, f"rod material constant {ROD_PARAMS[j]} is negative")
            for j in range(7, 10):
                try:
                    params[k, j] = float(tok[2 + j])
                except (IndexError, ValueError):
                    break  # the stream extraction fails from here on: the remaining fields stay 0
            if uni is not None:
                params[k] = uni
    return RodDeck(curr, nxt, params)


def write_rod(path: str | os.PathLike, curr, next, params) -> None:
    """Write a ``.rod`` file with all ten parameters (``%.16e``: a read gives the same
    doubles back)."""
    params = np.asarray(params, dtype=np.float64).reshape(-1, 10)
    if params.shape[0] != len(curr) or len(next) != len(curr):
        raise ValueError("curr, next and params must have one entry per rod")
    rows = [f"{int(curr[k]):6d} {int(next[k]):6d}" + "".join(f" {float(v):.16e}" for v in params[k])
            for k in range(len(curr))]
    _write_deck(path, rows)


class SourceDeck(NamedTuple):
    """A ``.source`` file: the sources, and the vertices that carry one."""
    names: List[str]     # per source
    radii: np.ndarray    # (num_source,) float64, each > 0
    node: np.ndarray     # (n,) int32 vertices in ascending order, each once
    source: np.ndarray   # (n,) int32 the source each carries


def read_source(path: str | os.PathLike, num_vertex: int, vertex_offset: int = 0, source_offset: int = 0) -> SourceDeck:
    """Read a ``.source`` file: the number of sources, that many name lines, that many radii,
    the number of source points, then one ``vertex source`` pair per line.

    Follows IBStandardInitializer::readSourceFiles (IBStandardInitializer.cpp:2495-2691): a
    name is its line with the comment cut and the white space trimmed, a radius is ``> 0``,
    a vertex is checked against ``[0, num_vertex)`` and a source index against
    ``[0, num_source)`` before ``vertex_offset`` / ``source_offset`` (the sources of the files
    read before, :2668-2673) are added.  ``d_source_idx[ln][j][n]`` is a map: a vertex listed
    twice keeps its last source, and the deck comes back in ascending vertex order.
    """
    with _Deck(path, "source") as deck:
        num_source = deck.count()
        names = []
        for _ in range(num_source):
            deck.line += 1
            line = deck.fh.readline()
            if not line:
                raise ValueError(f"Premature end to input file encountered before line {deck.line} of file {deck.name}")
            names.append(_discard_comments(line).strip(" \t\n"))
        radii = np.empty(num_source)
        for m in range(num_source):
            tok = deck.tokens()
            try:
                radii[m] = float(tok[0])
            except (IndexError, ValueError):
                raise deck.invalid() from None
            if not radii[m] > 0.0:
                raise deck.invalid("source radius is not positive")
        num_pts = deck.count()
        idx = {}
        for _ in range(num_pts):
            tok = deck.tokens()
            n = deck.index(tok, 0, num_vertex)
            try:
                s = int(tok[1])
            except (IndexError, ValueError):
                raise deck.invalid() from None
            if s < 0 or s >= num_source:
                raise deck.invalid(f"meter index {s} is out of range")
            idx[n] = s
    node = np.array(sorted(idx), dtype=np.int32)
    source = np.array([idx[n] for n in node.tolist()], dtype=np.int32)
    return SourceDeck(names, radii, node + np.int32(vertex_offset), source + np.int32(source_offset))


def write_source(path: str | os.PathLike, names: Sequence[str], radii, node, source) -> None:
    """Write a ``.source`` file (``%.16e`` radii: a read gives the same doubles back).  A
    name may not hold a comment character or a line break, and is written trimmed."""
    radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    if len(names) != radii.size or radii.size == 0:
        raise ValueError("one name and one radius per source, at least one source")
    if len(node) != len(source) or len(node) == 0:
        raise ValueError("node and source must have one entry per source point, at least one")
    for name in names:
        if any(c in name for c in _COMMENT_CHARS + "\n\r"):
            raise ValueError(f"source name {name!r} holds a comment character or a line break")
    with open(os.fspath(path), "w") as fh:
        fh.write(f"{radii.size}\n")
        for name in names:
            fh.write(name.strip(" \t") + "\n")
        for r in radii:
            fh.write(f"{float(r):.16e}\n")
        fh.write(f"{len(node)}\n")
        for n, s in zip(node, source):
            fh.write(f"{int(n):6d} {int(s):6d}\n")


class InstDeck(NamedTuple):
    """An ``.inst`` file: the instruments, and the vertices on their perimeters."""
    names: List[str]        # per instrument
    node: np.ndarray        # (n,) int32 vertices in ascending order, each once
    meter: np.ndarray       # (n,) int32 the meter each lies on
    meter_node: np.ndarray  # (n,) int32 its index on that meter's perimeter


def read_inst(path: str | os.PathLike, num_vertex: int, vertex_offset: int = 0, instrument_offset: int = 0) -> InstDeck:
    """Read an ``.inst`` file: the number of instruments, that many name lines, the number of
    instrumented points, then one ``vertex meter node`` triple per line.

    Follows IBStandardInitializer::readInstrumentationFiles (IBStandardInitializer.cpp:
    2257-2493): a name is its line with the comment cut and the white space trimmed; a vertex is
    checked against ``[0, num_vertex)``, a meter index against ``[0, num_inst)`` and a node
    index against ``>= 0``, in that order on each line; then every meter index and every node
    index ``0..max`` of every meter must have been met, and the meters met must be ``num_inst``
    (:2438-2474).  ``vertex_offset`` and ``instrument_offset`` (the instruments of the files
    read before, :2434, :2477) are added after the checks.  ``d_instrument_idx[ln][j][n]`` is a
    map: a vertex listed twice keeps its last entry (the entries it lost still count as met, as
    in the reference), and the deck comes back in ascending vertex order.
    """
    with _Deck(path, "instrumentation") as deck:
        num_inst = deck.count()
        names = []
        for _ in range(num_inst):
            deck.line += 1
            line = deck.fh.readline()
            if not line:
                raise ValueError(f"Premature end to input file encountered before line {deck.line} of file {deck.name}")
            names.append(_discard_comments(line).strip(" \t\n"))
        num_pts = deck.count()
        idx = {}
        met: List[List[bool]] = []  # encountered_instrument_idx / encountered_node_idx
        for _ in range(num_pts):
            tok = deck.tokens()
            n = deck.index(tok, 0, num_vertex)
            try:
                m = int(tok[1])
            except (IndexError, ValueError):
                raise deck.invalid() from None
            if m < 0 or m >= num_inst:
                raise deck.invalid(f"meter index {m} is out of range")
            while len(met) <= m:
                met.append([])
            try:
                k = int(tok[2])
            except (IndexError, ValueError):
                raise deck.invalid() from None
            if k < 0:
                raise deck.invalid("meter node index is negative")
            met[m] += [False] * (k + 1 - len(met[m]))
            met[m][k] = True
            idx[n] = (m, k)
        for m, nodes in enumerate(met):
            if not nodes:
                raise ValueError(f"Instrument index {m} not found in input file {deck.name}")
            for k, seen in enumerate(nodes):
                if not seen:
                    raise ValueError(f"Node index {k} associated with meter index {m} not found in input file {deck.name}")
        if len(met) != num_inst:
            raise ValueError(f"Not all anticipated instrument indices were found in input file {deck.name}  Expected to find "
                             f"{num_inst} distinct meter indices in input file")
    node = np.array(sorted(idx), dtype=np.int32)
    meter = np.array([idx[n][0] for n in node.tolist()], dtype=np.int32)
    meter_node = np.array([idx[n][1] for n in node.tolist()], dtype=np.int32)
    return InstDeck(names, node + np.int32(vertex_offset), meter + np.int32(instrument_offset), meter_node)


def write_inst(path: str | os.PathLike, names: Sequence[str], node, meter, meter_node) -> None:
    """Write an ``.inst`` file.  A name may not hold a comment character or a line break, and
    is written trimmed."""
    if len(names) == 0:
        raise ValueError("at least one instrument")
    if not (len(node) == len(meter) == len(meter_node)) or len(node) == 0:
        raise ValueError("node, meter and meter_node must have one entry per instrumented point, at least one")
    for name in names:
        if any(c in name for c in _COMMENT_CHARS + "\n\r"):
            raise ValueError(f"instrument name {name!r} holds a comment character or a line break")
    with open(os.fspath(path), "w") as fh:
        fh.write(f"{len(names)}\n")
        for name in names:
            fh.write(name.strip(" \t") + "\n")
        fh.write(f"{len(node)}\n")
        for n, m, k in zip(node, meter, meter_node):
            fh.write(f"{int(n):6d} {int(m):6d} {int(k):6d}\n")


_ROOT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


def _equal_eps(a: float, b: float) -> bool:
    """``|a - b| <= sqrt(DBL_EPSILON) * max(|a|, |b|, 1)``: the rule implemented here for
    SAMRAI's ``MathUtilities<double>::equalEps``, whose text is not in the reference tree
    (parity unpinned)."""
    return abs(a - b) <= _ROOT_EPS * max(abs(a), abs(b), 1.0)


def read_director(path: str | os.PathLike, num_vertex: int) -> np.ndarray:
    """Read a ``.director`` file into a ``(num_vertex, 9)`` float64 array, rows ``D1 D2 D3``.

    Follows IBStandardInitializer::readDirectorFiles (IBStandardInitializer.cpp:2157-2240):
    line 1 holds the count, which must equal ``num_vertex``; then three lines per vertex,
    three components each.  A vector is divided by its norm (``sqrt`` of the squares summed
    in component order) when the norm is not "equal to 1" in the sense of SAMRAI's
    ``MathUtilities<double>::equalEps`` -- implemented here as ``|norm - 1| <=
    sqrt(DBL_EPSILON) * max(norm, 1)``, SAMRAI's own text not being at hand (unpinned,
    DESIGN.md section 2); a vector within that of unit length comes back bit for bit as
    parsed.
    """
    with _Deck(path, "director") as deck:
        tok = deck.tokens()
        try:
            n = int(tok[0])
        except (IndexError, ValueError):
            raise deck.invalid() from None
        if n != num_vertex:
            raise deck.invalid()
        D = np.empty((n, 9), dtype=np.float64)
        for k in range(n):
            for r in range(3):
                tok = deck.tokens()
                norm2 = 0.0
                for d in range(3):
                    try:
                        v = float(tok[d])
                    except (IndexError, ValueError):
                        raise deck.invalid() from None
                    D[k, 3 * r + d] = v
                    norm2 += v * v
                norm = float(np.sqrt(norm2))
                if not _equal_eps(norm, 1.0):
                    D[k, 3 * r:3 * r + 3] /= norm
    return D


def write_director(path: str | os.PathLike, D) -> None:
    """Write ``D`` (N, 9) as a ``.director`` file, three ``%.16e`` lines per vertex."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[1] != 9 or D.shape[0] == 0:
        raise ValueError("D must be (N>0, 9)")
    with open(os.fspath(path), "w") as fh:
        fh.write(f"{D.shape[0]}\n")
        np.savetxt(fh, D.reshape(-1, 3), fmt="%.16e", delimiter=" ")


def _aligned(nbytes: int, align: int) -> int:
    return (nbytes + align - 1) // align * align


def lnode_index_dtype(ndim: int = 3, align: int = 1) -> np.dtype:
    """numpy record dtype of one packed LNodeIndex (LNodeIndex-inl.h:155-163)."""
    if ndim not in (2, 3):
        raise ValueError("ndim must be 2 or 3")
    if align < 1:
        raise ValueError("align must be >= 1")
    names = ["lag", "global_petsc", "local_petsc", "offset", "displacement"]
    formats = ["<i4", "<i4", "<i4", ("<i4", (ndim,)), ("<f8", (ndim,))]
    sizes = [4, 4, 4, 4 * ndim, 8 * ndim]
    offsets, o = [], 0
    for s in sizes:
        offsets.append(o)
        o += _aligned(s, align)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": o})


def lnode_index_stream_size(ndim: int = 3, align: int = 1) -> int:
    """LNodeIndex::getDataStreamSize (LNodeIndex-inl.h:148-151) at the given alignment."""
    return lnode_index_dtype(ndim, align).itemsize


def _records(lag, global_petsc, local_petsc, offset, displacement, ndim, align):
    lag = np.asarray(lag, dtype=np.int64).reshape(-1)
    n = lag.size
    rec = np.zeros(n, dtype=lnode_index_dtype(ndim, align))
    gp = lag if global_petsc is None else global_petsc
    lp = gp if local_petsc is None else local_petsc
    for name, v in (("lag", lag), ("global_petsc", gp), ("local_petsc", lp)):
        v = np.asarray(v, dtype=np.int64).reshape(-1)
        if v.size != n:
            raise ValueError(f"{name} has {v.size} entries, expected {n}")
        if n and (v.min() < -2**31 or v.max() >= 2**31):
            raise ValueError(f"{name} does not fit in int32")
        rec[name] = v
    if offset is not None:
        rec["offset"] = np.asarray(offset, dtype=np.int32).reshape(n, ndim)
    if displacement is not None:
        rec["displacement"] = np.asarray(displacement, dtype=np.float64).reshape(n, ndim)
    return rec


def pack_lnode_indices(lag, global_petsc=None, local_petsc=None, offset=None, displacement=None,
                       ndim: int = 3, align: int = 1) -> bytes:
    """Pack LNodeIndex records back to back, each as LNodeIndex::packStream writes it.

    ``global_petsc``/``local_petsc`` default to the Lagrangian index; ``offset``
    and ``displacement`` default to zero (a marker with no periodic image).
    """
    return _records(lag, global_petsc, local_petsc, offset, displacement, ndim, align).tobytes()


def unpack_lnode_indices(buf: bytes, ndim: int = 3, align: int = 1) -> np.ndarray:
    """Inverse of :func:`pack_lnode_indices`; returns a structured array."""
    dt = lnode_index_dtype(ndim, align)
    if len(buf) % dt.itemsize:
        raise ValueError(f"buffer of {len(buf)} bytes is not a whole number of {dt.itemsize}-byte records")
    return np.frombuffer(buf, dtype=dt).copy()


def _transaction_dtype(ndim: int, align: int) -> np.dtype:
    idx = lnode_index_dtype(ndim, align)
    return np.dtype({"names": ["index", "posn"], "formats": [idx, ("<f8", (ndim,))],
                     "offsets": [0, idx.itemsize], "itemsize": idx.itemsize + _aligned(8 * ndim, align)})


def pack_ltransaction(records: np.ndarray, posn: np.ndarray, ndim: int = 3, align: int = 1) -> bytes:
    """LTransaction<LNodeIndex>::packStream (LTransaction.cpp:128-140): int count, then per item
    its LNodeIndex record and its position double[NDIM]."""
    records = np.asarray(records)
    posn = np.asarray(posn, dtype=np.float64).reshape(-1, ndim)
    if records.dtype != lnode_index_dtype(ndim, align):
        raise ValueError("records must have lnode_index_dtype(ndim, align)")
    if posn.shape[0] != records.size:
        raise ValueError("one position per record")
    body = np.zeros(records.size, dtype=_transaction_dtype(ndim, align))
    body["index"] = records
    body["posn"] = posn
    head = np.zeros(1, dtype=np.dtype({"names": ["n"], "formats": ["<i4"], "itemsize": _aligned(4, align)}))
    head["n"] = records.size
    return head.tobytes() + body.tobytes()


def unpack_ltransaction(buf: bytes, ndim: int = 3, align: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """Inverse of :func:`pack_ltransaction`; returns (records, posn (n, ndim))."""
    h = _aligned(4, align)
    if len(buf) < h:
        raise ValueError("buffer shorter than the item count")
    n = int(np.frombuffer(buf[:4], dtype="<i4")[0])
    dt = _transaction_dtype(ndim, align)
    if n < 0 or len(buf) != h + n * dt.itemsize:
        raise ValueError(f"buffer of {len(buf)} bytes does not hold {n} items of {dt.itemsize} bytes")
    body = np.frombuffer(buf[h:], dtype=dt)
    return body["index"].copy(), body["posn"].copy()

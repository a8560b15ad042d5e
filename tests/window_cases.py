"""Plane windows for the 3-D sweeps' half calls (helper, not a test file; host arrays only).

Context.set_plane_window(mode, zlo, zhi) restricts a 3-D interp or spread to the sweep items
inside (1) or outside (2) the absolute planes [zlo, zhi]; SlabExchange runs the two halves
around its plane exchange.  The rule, as the kernels state it (le_sweep.hip, `inner`), with
LO, HI the kernel's reach (cases2d.KINFO) and array z index = plane - (ilower_z - g):

* an interp item over anchor planes a0 .. a1 - 1 is inner iff a0 + LO >= zlo and
  a1 - 1 + HI <= zhi: it reads no plane outside the window;
* a spread item is inner iff every plane it owns of the component's array lies in the window;
* a window with zlo <= zhi that is set (in mode 0) before Markers.bin cuts the item table at
  the anchors zlo - LO, zlo, zhi - HI + 1 and zhi + 1 (build_items, le_abi.cpp), so that
  every item is wholly inner or wholly not: a marker with anchor plane A is then interpolated
  by the inner half iff zlo - LO <= A <= zhi - HI.

The windows are those of the `deep` patch (cases3d: 62 x 36 x 90 cells, ilower_z = 5).
"""
import functools
import zlib

import numpy as np

import cases3d as c3

DEEP_M = 100_000  # markers of `deep`'s uniform set here (cases3d.uniform's M)
NAMES = ["interior", "middle", "thin", "low", "high", "all", "none"]
REAL = NAMES[:5]  # the windows with items on both sides
# the cluster of cases3d.cluster on `wide` sits in anchor plane 15: each window has a face
# between planes 15 and 16, which the cluster's stencils straddle
CLUSTER_WINDOWS = [(16, 24), (5, 15)]


def windows(geom):
    """name -> (zlo, zhi), absolute planes, for a patch with the z extent of `deep`."""
    g, il, iu = geom.g, geom.ilower[2], geom.iupper[2]
    return {
        "interior": (il, iu),                # a slab's configuration: the patch's own planes
        "middle": (30, 61),
        "thin": (40, 40 + 2 * g + 1),        # Slab's minimum thickness, 2 * ghost + 2 planes
        "low": (il - g, 20),                 # the cuts clamp at the arrays' first plane
        "high": (70, iu + g + 1),            # up to the z faces' last plane
        "all": (il - g - 40, iu + g + 41),   # beyond both ends: the outer half is empty
        "none": (10, 9),                     # empty: the inner half is empty, nothing is cut
    }


def shifted(geom):
    """`middle` moved up by 1 .. S - 1 planes, S the default segment length.  On an uncut
    table the item boundaries stay where they are, so over `middle` and these every face
    meets every position within a segment: some item ends exactly one plane short of, at and
    one past each bound of the `inner` rule, which a cut table (always cut to fit) never shows."""
    S, _ = c3.segments(geom)
    return [(30 + k, 61 + k) for k in range(1, S)]


@functools.lru_cache(maxsize=4)
def marker_deep(kernel):
    """The `deep` uniform case with DEEP_M markers, seeded by the kernel's name; built once,
    callers leave it unchanged."""
    geom = c3.geometry("deep", kernel)
    return c3.uniform(geom, zlib.crc32(f"window{kernel}".encode()), M=DEEP_M)


def cuts(geom, win):
    """The relative anchor planes at which build_items cuts the items under `win`."""
    W, LO, HI = c3.KINFO[geom.kernel]
    zlo, zhi = win
    if zlo > zhi:
        return []
    lo, hi = zlo - geom.org[2], zhi - geom.org[2]
    return sorted({c for c in (lo - LO, lo, hi - HI + 1, hi + 1) if 0 < c < geom.nz})


def inner_anchor(geom, win, A):
    """Absolute anchor planes A -> bool: the anchors a cut item table gives to the inner half."""
    W, LO, HI = c3.KINFO[geom.kernel]
    return (A >= win[0] - LO) & (A <= win[1] - HI)


def entries(cs):
    """(A, inside) of every list entry: its absolute anchor plane (cases3d.bucket_keys) and
    whether it lies in the column grid; the others are not swept, they read 0."""
    _, rel, inside = c3.bucket_keys(cs.geom, cs.X, cs.idx, cs.xshift)
    return rel[:, 2] + cs.geom.org[2], inside


def marker_sets(cs, win):
    """Per marker row: (listed and in the grid, of those the ones with an inner anchor)."""
    A, inside = entries(cs)
    M = cs.X.shape[0]
    ingrid, inner = np.zeros(M, bool), np.zeros(M, bool)
    ingrid[cs.idx[inside]] = True
    inner[cs.idx[inside & inner_anchor(cs.geom, win, A)]] = True
    return ingrid, inner


def plane_slice(geom, win, nz_array):
    """[i0, i1): the array z indices of the window's planes, clipped to an array of nz_array planes."""
    first = geom.ilower[2] - geom.g
    i0, i1 = max(win[0] - first, 0), min(win[1] - first, nz_array - 1) + 1
    return (i0, i1) if i0 < i1 else (0, 0)


def faces_inside_segments(geom, win, seg_items=0):
    """The cuts of `win` that fall strictly inside a segment of cases3d.segments."""
    S, _ = c3.segments(geom, seg_items)
    return [c for c in cuts(geom, win) if c % S]

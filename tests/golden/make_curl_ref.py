"""Generator of tests/golden/curl_side_ref.npz: the reference's own side-centred curl on
seeded inputs.

Runs only where the reference tree and flang are (``IBAMR_REFERENCE_DIR=<tree> python
tests/golden/make_curl_ref.py``).  It reads ``ibtk/src/math/fortran/curl3d.f.m4``, cuts out
the ``stoscurl3d`` subroutine, substitutes what m4 would have (``REAL``, ``INTEGER``,
``NDIM`` and SAMRAI's ``SIDE3d{0,1,2}(lo,hi,g)`` array-dimension macros, a scalar ghost
width), compiles it with flang ``-O0 -ffp-contract=off`` into a temporary directory outside
the repository, runs it and removes the directory.  The fixture holds only the inputs and
the outputs: no reference text and nothing compiled from it is kept.  This file holds the
substitution rules and nothing of the Fortran.

Per case the fixture stores ``ilower``, ``iupper``, ``u_gcw``, ``w_gcw``, ``dx``, the
ghosted inputs ``u0 u1 u2`` and the outputs ``w0 w1 w2`` (pre-filled with NaN: whatever
the routine does not write stays NaN), arrays in C order ``a[z, y, x]``.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OUT = HERE / "curl_side_ref.npz"
TEMPLATE = Path("ibtk") / "src" / "math" / "fortran" / "curl3d.f.m4"
ROUTINE = "stoscurl3d"
FFLAGS = ["-O0", "-ffixed-line-length-132", "-ffp-contract=off", "-fPIC", "-shared"]
DX = (0.1, 0.037, 0.2113)
# (ilower, iupper, u_gcw, w_gcw, scale of u)
CASES = [
    ((-3, 2, 5), (1, 4, 7), 2, 3, 1.0e-3),
    ((0, 0, 0), (0, 0, 0), 1, 0, 1.0),
    ((4, -7, 1), (20, 3, 9), 4, 4, 1.0e3),
]
SEED = 20240611


def side_dims(c, lo, hi, g):
    """SIDE3d<c>(lo,hi,g): the ghost box, + 1 on the upper bound of the array's own axis."""
    return ",".join(f"{lo}{d}-{g}:{hi}{d}+{g}" + ("+1" if d == c else "") for d in range(3))


def cut_routine(text):
    m = re.search(rf"^\s+subroutine {ROUTINE}\(.*?^\s+end\s*$", text, re.S | re.M)
    if not m:
        raise SystemExit(f"{ROUTINE} not found in {TEMPLATE}")
    return m.group(0) + "\n"


def expand(src):
    for c in range(3):
        src = re.sub(rf"SIDE3d{c}\((\w+),(\w+),(\w+)\)", lambda m, c=c: side_dims(c, *m.groups()), src)
    for word, repl in (("REAL", "double precision"), ("INTEGER", "integer"), ("NDIM", "3")):
        src = re.sub(rf"\b{word}\b", repl, src)
    left = re.search(r"\b(define|include|SIDE3d\w*|CELL3d\w*)\b", src)
    if left:
        raise SystemExit(f"m4 text {left.group(0)!r} survives the substitution")
    return src


def find_flang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (Path(rocm) / "lib" / "llvm" / "bin" / "flang", Path(rocm) / "llvm" / "bin" / "flang"):
        if c.is_file():
            return str(c)
    return shutil.which("flang") or shutil.which("flang-new")


def shape(n, g, c):
    return tuple(n[d] + 2 * g + (1 if d == c else 0) for d in (2, 1, 0))


def main():
    ref = os.environ.get("IBAMR_REFERENCE_DIR")
    if not ref or not (Path(ref) / TEMPLATE).is_file():
        raise SystemExit(f"set IBAMR_REFERENCE_DIR to a tree holding {TEMPLATE}")
    flang = find_flang()
    if flang is None:
        raise SystemExit("flang not found")
    tmp = Path(tempfile.mkdtemp(prefix="curl_ref_"))
    if HERE.parents[1] in tmp.resolve().parents:
        raise SystemExit("the temporary directory lies inside the repository")
    out = {}
    try:
        (tmp / "curl.f").write_text(expand(cut_routine((Path(ref) / TEMPLATE).read_text())))
        subprocess.run([flang, *FFLAGS, "-o", str(tmp / "libcurl.so"), str(tmp / "curl.f")], check=True)
        fn = getattr(ctypes.CDLL(str(tmp / "libcurl.so")), ROUTINE + "_")
        fn.restype = None
        rng = np.random.default_rng(SEED)
        dp = ctypes.POINTER(ctypes.c_double)
        for k, (ilo, ihi, ug, wg, scale) in enumerate(CASES):
            n = [ihi[d] - ilo[d] + 1 for d in range(3)]
            u = [scale * rng.standard_normal(shape(n, ug, c)) for c in range(3)]
            w = [np.full(shape(n, wg, c), np.nan) for c in range(3)]
            dx = np.array(DX, dtype=np.float64)
            ints = [ctypes.byref(ctypes.c_int(v)) for v in (ilo[0], ihi[0], ilo[1], ihi[1], ilo[2], ihi[2])]
            fn(*(a.ctypes.data_as(dp) for a in w), ctypes.byref(ctypes.c_int(wg)),
               *(a.ctypes.data_as(dp) for a in u), ctypes.byref(ctypes.c_int(ug)), *ints, dx.ctypes.data_as(dp))
            out[f"c{k}_ilower"], out[f"c{k}_iupper"] = np.array(ilo, np.int32), np.array(ihi, np.int32)
            out[f"c{k}_u_gcw"], out[f"c{k}_w_gcw"] = np.int32(ug), np.int32(wg)
            out[f"c{k}_dx"] = dx
            for c in range(3):
                out[f"c{k}_u{c}"], out[f"c{k}_w{c}"] = u[c], w[c]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out["ncases"] = np.int32(len(CASES))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    sys.exit(main())

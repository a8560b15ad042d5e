"""Build the reference's own Fortran kernels into oracle/_ref/ -- TEST INFRASTRUCTURE ONLY.

The reference keeps its Lagrangian-Eulerian kernels in three m4 templates,
``ibtk/src/lagrangian/fortran/lagrangian_interaction{2,3}d.f.m4`` and
``lagrangian_delta.f.m4``.  They use m4 for ``define(NDIM|REAL|INTEGER, ...)``, one
``include(...)`` of SAMRAI's ``pdat_m4arrdim{2,3}d.i`` and one macro out of that file,
``CELL{2,3}dVECG(lo,hi,g)``.  This recipe holds those substitution rules and nothing of
the reference's text: it expands the templates in memory, writes the result under
``oracle/_ref/src/`` and compiles it with flang into

    oracle/_ref/libleref_O0.so      the pin: le_oracle.c is bitwise equal to it
    oracle/_ref/libleref_O2.so      the same sources, optimised

both with ``-ffp-contract=off`` (no fused multiply-add, as oracle/Makefile and the GPU
kernels).  ``oracle/_ref/`` is ignored by git: neither the expanded Fortran nor the
libraries are ever committed.

The physical-boundary operators, ``ibtk/src/boundary/physical_boundary/fortran/
cartphysbdryop{2,3}d.f.m4``, go the same way into a pair of their own,

    oracle/_ref/libbdref_O0.so      the pin: le_bdry_oracle.c is bitwise equal to it
    oracle/_ref/libbdref_O2.so

so that a tree which holds only ``libleref_*`` skips only the boundary tests.  These two
templates take two more macros out of SAMRAI's file, both with a scalar ghost width:
``CELL{2,3}d(lo,hi,g)`` = ``lo0-g:hi0+g,...`` and ``SIDE{2,3}d{0,1,2}(lo,hi,g)``, the
same with ``+1`` on the upper bound of the side's own dimension.

The reference tree is looked for at ``$IBAMR_REFERENCE_DIR`` (default
``/root/reference``).  Without it, or without flang, ``build()`` says so in one line,
leaves ``oracle/_ref/`` as it is and returns False: the tests that need the libraries
skip.  A library is rebuilt only when a template or this recipe is newer than it.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
OUT = HERE / "_ref"
ENV_REFERENCE = "IBAMR_REFERENCE_DIR"
ENV_FLANG = "FLANG"
DEFAULT_REFERENCE = "/root/reference"
FORTRAN_SUBDIR = Path("ibtk") / "src" / "lagrangian" / "fortran"
TEMPLATES = ("lagrangian_delta.f.m4", "lagrangian_interaction2d.f.m4", "lagrangian_interaction3d.f.m4")
BDRY_SUBDIR = Path("ibtk") / "src" / "boundary" / "physical_boundary" / "fortran"
BDRY_TEMPLATES = ("cartphysbdryop2d.f.m4", "cartphysbdryop3d.f.m4")
OPTS = ("O0", "O2")
# -Bsymbolic: the library's calls to its own delta functions stay inside it, whatever else the
# process has loaded (libibtk_le.so exports the same lagrangian_* names, by design)
FFLAGS = ["-ffixed-line-length-132", "-ffp-contract=off", "-fPIC", "-shared", "-Wl,-Bsymbolic"]

# what m4 would have defined
WORDS = {"REAL": "double precision", "INTEGER": "integer"}
_DEFINE_NDIM = re.compile(r"^define\(NDIM,\s*(\d)\)dnl\s*$")
_DIRECTIVE = re.compile(r"^(define|include)\(.*\)dnl\s*$")
_VECG = re.compile(r"\bCELL(\d)dVECG\(\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*\)")
_CELL = re.compile(r"\bCELL(\d)d\(\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*\)")
_SIDE = re.compile(r"\bSIDE(\d)d(\d)\(\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*\)")
# anything m4-like that survives stops the build: a directive, a quote, an array-dimension
# macro of any centering and any form (CELL3d(, SIDE2d1(, NODE3dVECG(, ...), or one of the
# defined words
_LEFTOVER = re.compile(r"define\(|include\(|\bif(def|else)\(|`|\bdnl\b|\b[A-Z]+\dd\w*\(|"
                       r"\b(NDIM|REAL|INTEGER)\b")


class ExpansionError(RuntimeError):
    pass


def vecg(ndim: int, lo: str, hi: str, g: str) -> str:
    """SAMRAI's ghosted cell-array bounds: lo0-g0:hi0+g0,lo1-g1:hi1+g1[,lo2-g2:hi2+g2]."""
    return ",".join(f"{lo}{d}-{g}{d}:{hi}{d}+{g}{d}" for d in range(ndim))


def celld(ndim: int, lo: str, hi: str, g: str, side: int = -1) -> str:
    """SAMRAI's cell (side = -1) or side-of-dimension-`side` array bounds with one scalar
    ghost width: lo0-g:hi0+g,... and +1 on the upper bound of dimension `side`."""
    if not -1 <= side < ndim:
        raise ExpansionError(f"SIDE{ndim}d{side}: a {ndim}-d array has no side {side}")
    return ",".join(f"{lo}{d}-{g}:{hi}{d}+{g}" + ("+1" if d == side else "") for d in range(ndim))


def expand(text: str, name: str = "<template>") -> str:
    """The template as m4 (with SAMRAI's array-dimension macros) would leave it."""
    words = dict(WORDS)
    out = []
    for line in text.splitlines():
        m = _DEFINE_NDIM.match(line)
        if m:
            words["NDIM"] = m.group(1)
        if _DIRECTIVE.match(line):
            continue  # `define(...)dnl` and `include(...)dnl` expand to nothing
        line = _VECG.sub(lambda v: vecg(int(v.group(1)), v.group(2), v.group(3), v.group(4)), line)
        line = _CELL.sub(lambda v: celld(int(v.group(1)), v.group(2), v.group(3), v.group(4)), line)
        line = _SIDE.sub(lambda v: celld(int(v.group(1)), v.group(3), v.group(4), v.group(5), int(v.group(2))), line)
        for word, repl in words.items():
            line = re.sub(rf"\b{word}\b", repl, line)
        out.append(line)
    expanded = "\n".join(out) + "\n"
    for n, line in enumerate(expanded.splitlines(), 1):
        m = _LEFTOVER.search(line)
        if m:
            raise ExpansionError(f"{name}: line {n} of the expansion still holds m4 text {m.group(0)!r}; "
                                 "the reference uses a macro this recipe does not know")
    return expanded


def reference_dir() -> Path:
    return Path(os.environ.get(ENV_REFERENCE, DEFAULT_REFERENCE)) / FORTRAN_SUBDIR


def bdry_reference_dir() -> Path:
    return Path(os.environ.get(ENV_REFERENCE, DEFAULT_REFERENCE)) / BDRY_SUBDIR


def find_flang():
    cand = os.environ.get(ENV_FLANG)
    if cand:
        return cand if (shutil.which(cand) or Path(cand).is_file()) else None
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (Path(rocm) / "lib" / "llvm" / "bin" / "flang", Path(rocm) / "llvm" / "bin" / "flang"):
        if c.is_file():
            return str(c)
    return shutil.which("flang") or shutil.which("flang-new")


def lib_path(opt: str) -> Path:
    return OUT / f"libleref_{opt}.so"


def bdry_lib_path(opt: str) -> Path:
    return OUT / f"libbdref_{opt}.so"


def _build_set(what, src_dir, names, path_of, say) -> bool:
    """One pair of libraries from one set of templates.  True: both are there and current."""
    templates = [src_dir / t for t in names]
    if not all(t.is_file() for t in templates):
        say(f"no reference Fortran under {src_dir}; {what} in oracle/_ref/ left as they are")
        return False
    flang = find_flang()
    if flang is None:
        say(f"flang not found; {what} are not built")
        return False
    newest = max([t.stat().st_mtime for t in templates] + [Path(__file__).stat().st_mtime])
    libs = [path_of(o) for o in OPTS]
    if all(p.is_file() and p.stat().st_mtime >= newest for p in libs):
        return True
    (OUT / "src").mkdir(parents=True, exist_ok=True)
    sources = []
    for t in templates:
        f = OUT / "src" / t.name[: -len(".m4")]
        f.write_text(expand(t.read_text(), t.name))
        sources.append(str(f))
    for opt, p in zip(OPTS, libs):
        tmp = p.with_suffix(".so.tmp")
        subprocess.run([flang, f"-{opt}", *FFLAGS, "-o", str(tmp), *sources, "-lm"], check=True)
        os.replace(tmp, p)
    say(f"built {', '.join(p.name for p in libs)} with {flang}")
    return True


def build_bdry(verbose: bool = True) -> bool:
    """Bring oracle/_ref/libbdref_{O0,O2}.so up to date.  True: both are there and current."""
    say = (lambda s: print(f"oracle/build_ref: {s}", file=sys.stderr)) if verbose else (lambda s: None)
    return _build_set("the boundary-operator libraries", bdry_reference_dir(), BDRY_TEMPLATES, bdry_lib_path, say)


def build(verbose: bool = True) -> bool:
    """Bring oracle/_ref/ up to date.  True: both libleref libraries are there and current
    (the boundary pair has a result of its own, ``build_bdry``: either pair may be absent
    without the other)."""
    say = (lambda s: print(f"oracle/build_ref: {s}", file=sys.stderr)) if verbose else (lambda s: None)
    ok = _build_set("the Lagrangian-kernel libraries", reference_dir(), TEMPLATES, lib_path, say)
    build_bdry(verbose)
    return ok


if __name__ == "__main__":
    build()

"""The boundary-operator oracle pinned to the reference's own compiled Fortran (CPU only).

``oracle/build_ref.py`` expands the reference's ``cartphysbdryop{2,3}d.f.m4`` and compiles
them with flang into ``oracle/_ref/libbdref_O0.so`` and ``libbdref_O2.so``;
``oracle.ref.phys_bdry_side`` drives their ``{cc,sc}robinphysbdryop*`` routines box by
box.  ``oracle/le_bdry_oracle.c``, which every device test of ``ibtk_le_phys_bdry_side``
compares with, is held to both libraries here, bit for bit, fill and adjoint, over every
case of ``tests/bdry_cases.py``.

What this pins is the Fortran arithmetic and the reading of its arguments (which dx a
face takes, the Dirichlet threshold and its overwrite in the adjoint, f_g with g != 0,
which end of which dimension an edge's location index names, the loop bounds on narrow
patches).  The walk over the boxes in ``ref.phys_bdry_side`` is itself a restatement of
``CartSideRobinPhysBdryOp.cpp``; it is written apart from the oracle's (a table copied
from the Fortran's own comments instead of the cyclic-order formula), but a misreading
of the C++ shared by both is not caught here.
"""
import numpy as np
import pytest

import bdry_cases as bc
from oracle import build_ref
from oracle import oracle as ora
from oracle import ref


@pytest.fixture(scope="module")
def bdref():
    if not ref.bdry_available():
        pytest.skip("oracle/_ref/libbdref_{O0,O2}.so not built (no reference tree or no flang at build time)")
    ora.lib()
    return ref


def run(fn, patch, case, us, **kw):
    _, _, phys, kind, adjoint = case
    A, B, G = bc.coefs(patch, kind)
    out = [u.copy() for u in us]
    fn(patch["lo"], patch["hi"], patch["g"], bc.dx_of(patch), out, phys, A, B, G, adjoint, **kw)
    return out


@pytest.mark.parametrize("patch", bc.PATCHES, ids=bc.PATCH_IDS)
def test_oracle_matches_reference(bdref, patch):
    """le_bdry_oracle.c == the -O0 library == the -O2 library, every bit of every array."""
    base = {f: bc.inputs(patch, f) for f in ("random", "nan_ghost")}
    n = 0
    for case in bc.cases(patch):
        us = base[case[0]]
        got = run(ora.phys_bdry_side, patch, case, us)
        diff = bc.same_bits_or_nan if case[0] == "nan_ghost" else bc.same_bits
        want = {opt: run(bdref.phys_bdry_side, patch, case, us, opt=opt) for opt in ("O0", "O2")}
        if any(case[2]):
            assert any(bc.same_bits_or_nan(w, u).size for w, u in zip(want["O0"], us)), \
                f"{bc.label(patch, case)}: the reference changed nothing"
        for a in range(len(us)):
            if case[0] == "random":
                assert np.isfinite(want["O0"][a]).all(), f"{bc.label(patch, case)}: not finite"
            bad = diff(got[a], want["O0"][a])
            assert bad.size == 0, (f"{bc.label(patch, case)} comp {a}: the oracle differs from the -O0 reference at "
                                   f"{len(bad)} points, first {bad[:3].tolist()}")
            bad = diff(want["O2"][a], want["O0"][a])
            assert bad.size == 0, (f"{bc.label(patch, case)} comp {a}: the -O2 reference differs from the -O0 one at "
                                   f"{len(bad)} points, first {bad[:3].tolist()}")
        n += 1
    assert n == len(bc.cases(patch)) > 0


def test_oracle_backend_argument(bdref):
    """oracle.phys_bdry_side(backend=ref.phys_bdry_side) is the reference call."""
    patch = bc.PATCHES[2]
    case = ("random", "all", [1] * 6, "mixed", True)
    us = bc.inputs(patch, "random")
    a = run(ora.phys_bdry_side, patch, case, us, backend=bdref.phys_bdry_side)
    b = run(bdref.phys_bdry_side, patch, case, us)
    assert all(bc.same_bits(x, y).size == 0 for x, y in zip(a, b))
    assert any(bc.same_bits(x, u).size for x, u in zip(a, us))


@pytest.mark.parametrize("patch", bc.PATCHES, ids=bc.PATCH_IDS)
def test_reference_fill_is_idempotent_unless_narrow(bdref, patch):
    """The premise of the device's idempotence test: with at least max(g, 2) cells in
    every dimension the reference's fill reads only the patch's own points and ghost points
    it wrote earlier in the same call, so a second fill changes no bit.  On a narrow patch
    a mirror point lies in the opposite ghost region, which a later box of the same call
    overwrites: there the second fill differs (checked for the all-faces pattern), and the
    device is held to the oracle's second fill instead."""
    us = bc.inputs(patch, "random")
    for case in bc.cases(patch):
        if case[0] != "random" or case[4]:
            continue
        once = run(bdref.phys_bdry_side, patch, case, us)
        twice = run(bdref.phys_bdry_side, patch, case, once)
        same = all(bc.same_bits(x, y).size == 0 for x, y in zip(once, twice))
        if not bc.is_narrow(patch):
            assert same, f"{bc.label(patch, case)}: a second fill changed the arrays"
        elif case[1] == "1" * (2 * len(patch["lo"])) and case[3] == "robin":
            assert not same, f"{bc.label(patch, case)}: expected the narrow patch's second fill to differ"


# --------------------------------------------------------------------------
# the case list's own preconditions (no reference needed)
# --------------------------------------------------------------------------
def test_case_list_covers_what_it_says():
    assert len(bc.PATCHES) == 11 and len(bc.ALL_PATTERN_PATCHES) == 9
    for p in bc.PATCHES:
        nd = len(p["lo"])
        pats = bc.patterns(p)
        assert len(pats) == ((16 if nd == 2 else 64) if p["every_pattern"] else 4)
        assert len({tuple(ph) for _, ph in pats}) == len(pats)
        assert 1 <= p["g"] <= bc.MAX_GHOST
    ids = [p["id"] for p in bc.PATCHES]
    assert len(set(ids)) == len(ids)
    narrow = [p for p in bc.PATCHES if bc.is_narrow(p)]
    assert len(narrow) == 5 and any(p["g"] == bc.MAX_GHOST for p in narrow)
    # a patch with one cell in every dimension, 2-D and 3-D
    assert sum(all(h == l for l, h in zip(p["lo"], p["hi"])) for p in narrow) == 2
    # a face with more lines than a block of 256 threads, in both dimensions
    assert any(len(p["lo"]) == 3 and (p["hi"][0] + 1) * (p["hi"][1] + 1) > 1024 for p in bc.PATCHES)
    # over the threshold sets every normal-component entry takes every value, on both sides of 1e-12
    for nd in (2, 3):
        p = next(q for q in bc.PATCHES if len(q["lo"]) == nd)
        seen = {}
        for kind in bc.THRESHOLD_KINDS:
            A, B, G = bc.coefs(p, kind)
            assert np.all(A == 1.0)
            for loc in range(2 * nd):
                seen.setdefault(loc, set()).add(B[loc // 2, loc])
        for loc in range(2 * nd):
            assert seen[loc] == set(bc.THRESHOLD_B)
    b = np.array(bc.THRESHOLD_B)
    assert (np.abs(b) < 1e-12).sum() == 3 and (np.abs(b) == 1e-12).sum() == 2 and (np.abs(b) > 1e-12).sum() == 3
    # the NaN family: NaN exactly off the patch's own side points
    p = bc.PATCHES[2]
    for a, u in enumerate(bc.inputs(p, "nan_ghost")):
        own = bc.own_mask(p["lo"], p["hi"], p["g"], a)
        assert own.sum() == np.prod([h - l + 1 + (d == a) for d, (l, h) in enumerate(zip(p["lo"], p["hi"]))])
        assert np.array_equal(np.isnan(u), ~own)
        assert u.shape == ora.side_ghost_shape(p["lo"], p["hi"], p["g"], a)


def test_comparators():
    a = np.array([1.0, np.nan, 0.0, 2.0])
    assert bc.same_bits(a, a.copy()).size == 0
    assert bc.same_bits(a, np.array([1.0, np.nan, -0.0, 2.0])).tolist() == [[2]]
    assert bc.same_bits_or_nan(np.array([1.0, -np.nan, 0.0, 2.0]), a).size == 0
    assert bc.same_bits_or_nan(np.array([1.0, 5.0, 0.0, np.nan]), a).tolist() == [[1], [3]]


# --------------------------------------------------------------------------
# the recipe's expander on the boundary templates' macros (needs neither the reference nor flang)
# --------------------------------------------------------------------------
def test_expander_cell_and_side_bounds():
    assert build_ref.celld(2, "il", "iu", "g") == "il0-g:iu0+g,il1-g:iu1+g"
    assert build_ref.celld(3, "il", "iu", "g", 1) == "il0-g:iu0+g,il1-g:iu1+g+1,il2-g:iu2+g"
    text = "\n".join(["define(NDIM,2)dnl", "define(REAL,`double precision')dnl", "define(INTEGER,`integer')dnl",
                      "include(SOMEWHERE/arrdim2d.i)dnl", "      REAL U(CELL2d(ilower,iupper,U_gcw))",
                      "      REAL u1(SIDE2d1(ilower,iupper,u_gcw))", "      REAL dx(0:NDIM-1)",
                      "         h = dx(location_index/NDIM)"])
    assert build_ref.expand(text) == (
        "      double precision U(ilower0-U_gcw:iupper0+U_gcw,ilower1-U_gcw:iupper1+U_gcw)\n"
        "      double precision u1(ilower0-u_gcw:iupper0+u_gcw,ilower1-u_gcw:iupper1+u_gcw+1)\n"
        "      double precision dx(0:2-1)\n"
        "         h = dx(location_index/2)\n")
    three = build_ref.expand("define(NDIM,3)dnl\n      x(SIDE3d2(a,b,c)) = NDIM")
    assert three == "      x(a0-c:b0+c,a1-c:b1+c,a2-c:b2+c+1) = 3\n"
    for leftover in ("      q(SIDE2d2(lo,hi,g))",        # no side 2 in 2-D
                     "      q(SIDE3d(lo,hi,g))",         # no such macro
                     "      q(CELL3d(lo,hi))",           # two arguments
                     "      q(FACE3d0(lo,hi,g))", "      q(NODE2d(lo,hi,g))", "      q(EDGE3d1(lo,hi,g))",
                     "      q(OUTERSIDE3d0(lo,hi,g))", "      q(CELL2d(lo,hi,g),SIDE2d0VECG(lo,hi,g))"):
        with pytest.raises(build_ref.ExpansionError):
            build_ref.expand(leftover)

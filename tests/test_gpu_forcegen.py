"""GPU: spring, beam and target-point forces on the device (ibtk_le_forcegen_*,
ibamr_amd.forcegen.ForceGen) against the serial restatement of IBStandardForceGen's three
loops (tests/forcegen_ref.py).

The kernel sums every node's contributions in the reference's order from the reference's
operands, one rounded operation per reference operation, so the comparison is bit for bit
(signed zeros included).  Beams and target points need only separately rounded +, - and *;
springs also rest on fp64 sqrt and / being correctly rounded on gfx950.
"""
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from forcegen_ref import reference_force  # noqa: E402
from ibamr_amd import io  # noqa: E402
from ibamr_amd.forcegen import ForceSpecs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


@pytest.fixture(scope="module")
def ForceGen(le):
    from ibamr_amd.forcegen import ForceGen as FG
    return FG


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_bitwise(got, ref, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == ref.shape
    bad = got.view(np.int64) != ref.view(np.int64)
    print(f"{what}: {int(bad.sum())} of {bad.size} words differ, max |diff| {np.abs(got - ref).max():.3e}")
    assert not bad.any(), what


def _deck_specs(name, ndim, **uniform):
    """ForceSpecs of a fixture: the .vertex twin and whichever decks exist."""
    X0 = io.read_vertex(GOLDEN / "vertex" / f"{name}.vertex", ndim)
    nv = X0.shape[0]
    d = GOLDEN / "ibforce"
    pick = lambda *keys: {k: uniform[k] for k in keys if k in uniform}  # noqa: E731
    springs = beams = targets = None
    if (d / f"{name}.spring").exists():
        springs = io.read_spring(d / f"{name}.spring", nv, **pick("uniform_stiffness", "uniform_rest_length"))
    if (d / f"{name}.beam").exists():
        beams = io.read_beam(d / f"{name}.beam", nv, ndim, **pick("uniform_bend_rigidity", "uniform_curvature"))
    if (d / f"{name}.target").exists():
        targets = io.read_target(d / f"{name}.target", nv,
                                 **pick("uniform_target_stiffness", "uniform_target_damping"))
    return ForceSpecs(ndim, X0, springs, beams, targets)


def _run(ctx, ForceGen, n, ndim, X, springs=None, beams=None, targets=None, U=None, dX=None, F0=None,
         accumulate=True):
    fg = ForceGen(ctx, n, ndim, springs=springs, beams=beams, targets=targets)
    F = _dev(F0) if F0 is not None else None
    out = fg.compute(_dev(X), U=_dev(U), F=F, dX=_dev(dX), accumulate=accumulate)
    ctx.synchronize()
    return out


# the decks: (name, ndim, uniform overrides).  sphere3d_32's deck has zero spring constants
# (the example sets them in its input file), so a uniform stiffness stands in for that.
DECKS = {
    "curve2d_64": (2, {}),
    "sphere3d_32": (3, {"uniform_stiffness": 37.5}),
    "fila_256": (2, {"uniform_stiffness": 1.0e4, "uniform_bend_rigidity": 0.375,
                     "uniform_curvature": [1.0e-5, -2.0e-5], "uniform_target_stiffness": 5.0e3,
                     "uniform_target_damping": 0.75}),
}


@pytest.mark.parametrize("name", list(DECKS))
def test_decks_bitwise(ctx, ForceGen, name):
    """curve2d_64 (2-D, 304 springs), sphere3d_32 (3-D, 480 springs, degree 5-6) and fila_256
    (springs, beams and target points with uniform stiffness, rigidity, curvature and damping,
    a random U), at positions a little off the decks', accumulated onto a random F."""
    ndim, uniform = DECKS[name]
    sp = _deck_specs(name, ndim, **uniform)
    a = sp.arrays()
    n = sp.num_vertex
    rng = np.random.default_rng(len(name))
    X = sp.X0 + 1e-3 * rng.standard_normal((n, ndim))
    U = rng.standard_normal((n, ndim))
    F0 = rng.standard_normal((n, ndim))
    assert {"curve2d_64": 304, "sphere3d_32": 480, "fila_256": 200}[name] == a["springs"].mastr.size
    if name == "fila_256":
        assert a["beams"].mastr.size == 199 and a["targets"].node.size == 201
    ref = reference_force(n, ndim, X, a["springs"], a["beams"], a["targets"], U=U, F=F0)
    assert np.abs(ref - F0).max() > 1e-3  # the forces are not trivially zero
    got = _run(ctx, ForceGen, n, ndim, X, a["springs"], a["beams"], a["targets"], U=U, F0=F0)
    _assert_bitwise(got, ref, name)


@pytest.fixture(scope="module")
def synthetic():
    """1000 nodes; 5000 springs: random ones with repeats, a hub (node 7) with 300 springs --
    a list longer than a wave --, one coincident pair (nodes 20, 21); nodes 950.. isolated;
    200 random beams; a target point on every third node below 950."""
    rng = np.random.default_rng(2024)
    n, nd, live = 1000, 3, 950
    X = rng.random((n, nd))
    X[21] = X[20]
    m = rng.integers(0, live, 4650)
    s = (m + rng.integers(1, live, 4650)) % live
    hub_other = rng.permutation(np.setdiff1d(np.arange(live), [7]))[:300]
    hub_m = np.where(np.arange(300) % 2 == 0, 7, hub_other)  # the hub as master and as slave
    hub_s = np.where(np.arange(300) % 2 == 0, hub_other, 7)
    mastr = np.concatenate([m, m[:49], hub_m, [20]])  # 49 repeated edges, the coincident pair last
    slave = np.concatenate([s, s[:49], hub_s, [21]])
    o = rng.permutation(mastr.size)
    mastr, slave = mastr[o], slave[o]
    assert mastr.size == 5000 and not (mastr == slave).any()
    springs = (mastr, slave, rng.random(5000) * 100.0, rng.random(5000) * 0.5)
    bm = rng.integers(0, live, 200)
    bn = (bm + rng.integers(1, live, 200)) % live
    bp = (bm + rng.integers(1, live, 200)) % live
    beams = (bm, bn, bp, rng.random(200) * 10.0, rng.standard_normal((200, nd)) * 0.1)
    node = np.arange(0, live, 3)
    targets = (node, rng.random(node.size) * 50.0, rng.random(node.size), rng.random((node.size, nd)))
    dX = rng.integers(-1, 2, (n, nd)).astype(np.float64)  # periodic displacements of a unit box
    dX[21] = dX[20]
    return dict(n=n, nd=nd, live=live, X=X, springs=springs, beams=beams, targets=targets,
                U=rng.standard_normal((n, nd)), dX=dX, F0=rng.standard_normal((n, nd)))


@pytest.mark.parametrize("with_dX", [False, True])
@pytest.mark.parametrize("accumulate", [True, False])
def test_synthetic_bitwise(ctx, ForceGen, synthetic, with_dX, accumulate):
    c = synthetic
    dX = c["dX"] if with_dX else None
    ref = reference_force(c["n"], c["nd"], c["X"], c["springs"], c["beams"], c["targets"], U=c["U"], dX=dX,
                          F=c["F0"], accumulate=accumulate)
    got = _run(ctx, ForceGen, c["n"], c["nd"], c["X"], c["springs"], c["beams"], c["targets"], U=c["U"], dX=dX,
               F0=c["F0"], accumulate=accumulate)
    _assert_bitwise(got, ref, f"synthetic dX={with_dX} accumulate={accumulate}")
    iso = got.cpu().numpy()[c["live"]:]
    if accumulate:
        assert np.array_equal(iso, c["F0"][c["live"]:])  # the isolated nodes' F is unchanged
    else:
        assert not iso.any()


def _chain(n, nd, rng):
    """A fibre of n nodes: springs between neighbours, beams on the interior nodes, a target
    point without damping on node 0 (so that n = 1 still launches the kernel)."""
    i = np.arange(n - 1)
    springs = (i, i + 1, rng.random(n - 1) * 10.0 + 1.0, np.full(n - 1, 0.9 / max(n, 2))) if n > 1 else None
    j = np.arange(1, n - 1)
    beams = (j, j + 1, j - 1, rng.random(j.size) + 0.5, np.zeros((j.size, nd))) if n > 2 else None
    targets = ([0], [3.0], [0.0], rng.random((1, nd)))
    return springs, beams, targets


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 100_003])
def test_chain_sizes_bitwise(ctx, ForceGen, n):
    """Sizes at wave and block edges, and more than one block."""
    nd = 3
    rng = np.random.default_rng(n)
    X = np.linspace(0.0, 1.0, n)[:, None] * np.ones(nd) + rng.standard_normal((n, nd)) * (0.2 / n)
    springs, beams, targets = _chain(n, nd, rng)
    F0 = rng.standard_normal((n, nd))
    ref = reference_force(n, nd, X, springs, beams, targets, F=F0)
    got = _run(ctx, ForceGen, n, nd, X, springs, beams, targets, F0=F0)  # U=None: no damping
    _assert_bitwise(got, ref, f"chain n={n}")


def test_unaligned_views_and_repeatability(ctx, ForceGen, synthetic):
    """X and F as 8-byte-offset views of 16-byte-aligned allocations; two calls, identical bits."""
    c = synthetic
    n, nd = c["n"], c["nd"]
    fg = ForceGen(ctx, n, nd, springs=c["springs"], beams=c["beams"], targets=c["targets"])
    ref = reference_force(n, nd, c["X"], c["springs"], c["beams"], c["targets"], U=c["U"], F=c["F0"])
    outs = []
    for _ in range(2):
        xb = torch.zeros(n * nd + 1, dtype=torch.float64, device="cuda")
        fb = torch.zeros(n * nd + 1, dtype=torch.float64, device="cuda")
        X, F = xb[1:].view(n, nd), fb[1:].view(n, nd)
        assert X.data_ptr() % 16 == 8 and F.data_ptr() % 16 == 8
        X.copy_(_dev(c["X"]))
        F.copy_(_dev(c["F0"]))
        assert fg.compute(X, U=_dev(c["U"]), F=F) is F
        ctx.synchronize()
        assert fb[0].item() == 0.0  # nothing written in front of the view
        outs.append(F.cpu().numpy())
    _assert_bitwise(outs[0], ref, "unaligned")
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))


def test_empty_plan_and_cleared_classes(ctx, ForceGen, synthetic):
    c = synthetic
    n, nd = c["n"], c["nd"]
    fg = ForceGen(ctx, n, nd)
    F = _dev(c["F0"])
    fg.compute(_dev(c["X"]), F=F)
    ctx.synchronize()
    assert np.array_equal(F.cpu().numpy().view(np.int64), c["F0"].view(np.int64))  # untouched
    fg.compute(_dev(c["X"]), F=F, accumulate=False)
    ctx.synchronize()
    assert not F.cpu().numpy().any()
    # a class set and then cleared (n = 0) is gone from the plan
    fg.set_springs(*c["springs"])
    fg.set_targets(*c["targets"])
    fg.set_springs([], [], [], [])
    ref = reference_force(n, nd, c["X"], targets=c["targets"], U=c["U"], accumulate=False)
    _assert_bitwise(fg.compute(_dev(c["X"]), U=_dev(c["U"])), ref, "targets only")


def test_argument_errors(ctx, ForceGen, le):
    from ibamr_amd._lib import IBTKLEError
    fg = ForceGen(ctx, 10, 3, targets=([2], [1.0], [0.5], [[0.0, 0.0, 0.0]]))
    X = torch.zeros((10, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(IBTKLEError, match="eta"):
        fg.compute(X)  # U=None with a non-zero damping coefficient
    with pytest.raises(ValueError):
        fg.compute(X[:5], U=X)
    one = np.ones(1)
    for call, word in ((lambda: fg.set_springs([0], [10], one, one), "out of range"),
                       (lambda: fg.set_springs([-1], [1], one, one), "out of range"),
                       (lambda: fg.set_springs([4], [4], one, one), "master and slave"),
                       (lambda: fg.set_springs([0], [1], one, one, [1]), "Hookean"),
                       (lambda: fg.set_beams([3], [3], [2], one), "master and next"),
                       (lambda: fg.set_beams([3], [4], [3], one), "master and prev"),
                       (lambda: fg.set_beams([3], [4], [12], one), "out of range"),
                       (lambda: fg.set_targets([10], one, one, np.zeros((1, 3))), "out of range")):
        with pytest.raises(IBTKLEError, match=word) as e:
            call()
        assert e.value.code == 4
    lib = le._lib.load()
    assert lib.ibtk_le_forcegen_set_springs(fg.h, -1, None, None, None, None, None) == 4
    assert b"negative" in lib.ibtk_le_last_error()
    # the failed calls left the plan as it was
    U = torch.ones_like(X)
    F = fg.compute(X, U=U)
    ctx.synchronize()
    ref = reference_force(10, 3, np.zeros((10, 3)), targets=([2], [1.0], [0.5], [[0.0, 0.0, 0.0]]), U=np.ones((10, 3)))
    _assert_bitwise(F, ref, "plan kept")


def test_coupling_step_with_forces_has_no_host_sync(le, ctx, ForceGen):
    """One explicit IB step with the force stage on the device -- ghost fill, interp,
    X += dt U, ForceGen.compute, re-bin, zero ghosts, spread, fold -- on a 48^3 grid with the
    sphere3d_32 deck scaled into the box: silent under torch's sync debug mode "error", and
    equal to the same step run with the mode off."""
    from ibamr_amd.le import Geometry
    N = 48
    geom = Geometry.periodic_unit([N, N, N], 3)
    X0 = 0.5 + 0.5 * io.read_vertex(GOLDEN / "vertex" / "sphere3d_32.vertex", 3)  # radius 0.25 about the centre
    nv = X0.shape[0]
    springs = io.read_spring(GOLDEN / "ibforce" / "sphere3d_32.spring", nv, length_scale=0.5, uniform_stiffness=2.0)
    targets = io.TargetDeck(np.arange(0, nv, 4, dtype=np.int32), np.full((nv + 3) // 4, 10.0),
                            np.full((nv + 3) // 4, 0.5))
    fg = ForceGen.from_specs(ctx, ForceSpecs(3, X0, springs, None, targets))
    g = torch.Generator(device="cuda:0").manual_seed(5)
    u = geom.alloc("side")
    for a in u:
        a.uniform_(-1, 1, generator=g)
    dt = 0.05 / N

    def step(X, U, F, f, bins):
        le.fill_periodic_ghosts(ctx, geom, "side", u)
        le.interp(ctx, bins, "IB_4", "side", geom, u, U, X)
        le.position_update(ctx, "euler", dt, X, U, out=X)
        fg.compute(X, U=U, F=F, accumulate=False)
        bins.bin(geom, "IB_4", X)
        le.zero_ghosts(ctx, geom, "side", f)
        le.spread(ctx, bins, "IB_4", "side", geom, f, F, X)
        le.fold_periodic_ghosts(ctx, geom, "side", f)

    outs = []
    for mode in ("error", None):
        X = _dev(X0)
        U = torch.zeros_like(X)
        F = torch.zeros_like(X)
        f = geom.alloc("side")
        bins = le.Markers(ctx).bin(geom, "IB_4", X)
        step(X, U, F, f, bins)  # first call: the library's buffers are allocated here
        ctx.synchronize()
        if mode:
            torch.cuda.set_sync_debug_mode(mode)
        try:
            step(X, U, F, f, bins)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        ctx.synchronize()
        outs.append((X.clone(), U.clone(), F.clone(), [a.clone() for a in f]))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(outs[0][3], outs[1][3]))
    # the force stage of that step against the restatement, at the step's X and U
    a = ForceSpecs(3, X0, springs, None, targets).arrays()
    Xh, Uh = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
    assert np.abs(outs[0][2].cpu().numpy()).max() > 0
    # F was computed from the X of the update and the U of the interp, both still in place
    _assert_bitwise(outs[0][2], reference_force(nv, 3, Xh, a["springs"], None, a["targets"], U=Uh, accumulate=False),
                    "step F")

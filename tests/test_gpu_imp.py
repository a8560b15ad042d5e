"""GPU: the IMP stages (ibamr_amd.imp) against the numpy restatement tests/imp_ref.py --
which tests/test_imp_cpu.py holds to 50-digit known answers -- on the cases of
tests/imp_cases.py: extents that cross every tile boundary and are multiples of none,
entries in the ghost layer out to its edge, exact NINT ties in the cell frame and in the
side frames, a cell pair dense enough that the spread's 64-entry chunk loop repeats, a
permuted sub-list with duplicates, an empty list.

Interp: U and GradU equal imp_ref bit for bit, as int64.

Spread: the weights are those of the interp's own function and every contribution's sum
over k is formed in the reference's order, so a contribution differs from the reference's
only in f (wgt / dV) for (f wgt) / dV: two roundings here, two there, Q = 4.  For every
point |f_dev - f_ref| <= (2 (n_i - 1) + Q) 2^-53 S_i, n_i contributions, S_i the sum of
their magnitudes, both from imp_ref.  A dropped or doubled entry is about S_i / n_i.

Update and stress: tol_q = 8 max(ref_err_q, 2^-52) against the known answers, 2 tol_q
against imp_ref, errors as max |v - v_ref| / max |v_ref|.
"""
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import imp_cases as ic  # noqa: E402
import imp_ref as ir  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
Q = 4  # roundings that differ in forming one contribution (see above)
SENT = -7.25
KAT = Path(__file__).resolve().parent / "golden" / "imp_kat.npz"


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def imp(le):
    from ibamr_amd import imp as _imp
    return _imp


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


@pytest.fixture(scope="module")
def kat():
    return np.load(KAT)


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def make_geom(le, name):
    ilower, n, dx, xl, g, pitched = ic.GEOMS[name]
    iupper = [ilower[d] + n[d] - 1 for d in range(len(n))]
    geom = le.Geometry(list(ilower), iupper, g, list(dx), list(xl))
    return geom.aligned() if pitched else geom


def span(t):
    """The whole allocation under a (possibly pitched) side array, as a flat view."""
    size = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return torch.as_strided(t, (size,), (1,))


def upload(geom, arrays):
    ts = geom.alloc("side")
    for t, a in zip(ts, arrays):
        span(t).fill_(float("nan"))
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return ts


def clip_slices(geo, c, clip):
    lo, hi = geo.patch_side_box(c) if clip == "patch" else geo.ghost_box(c)
    glo, _ = geo.ghost_box(c)
    return tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in reversed(range(geo.ndim)))


def force_arrays(geom, geo, clip):
    """f arrays whose allocations hold a per-element sentinel pattern, zero in the clip boxes."""
    ts = geom.alloc("side")
    for c, t in enumerate(ts):
        flat = span(t)
        flat.copy_(torch.from_numpy(-(3.0e5 + 1000.0 * c + np.arange(flat.numel(), dtype=np.float64))))
        t[clip_slices(geo, c, clip)] = 0.0
    return ts


def image(t):
    flat = span(t).cpu().numpy().copy()
    return flat, np.lib.stride_tricks.as_strided(flat, tuple(t.shape), tuple(8 * s for s in t.stride()))


def check_spread(geo, ts, before, f_ref, cnt, S, clip, what):
    """Inside the clip boxes the bound; every other bit of the allocations as it was."""
    worst = 0.0
    for c, t in enumerate(ts):
        flat, view = image(t)
        box = clip_slices(geo, c, clip)
        got = view[box].copy()
        bound = ic.spread_bound(cnt[c][box], S[c][box], Q)
        diff = np.abs(got - f_ref[c][box])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max()))
        assert (diff <= bound).all(), f"{what} component {c}: worst |diff| / bound = {ratio.max():.3f}"
        view[box] = 0.0
        bflat, bview = before[c]
        assert np.array_equal(flat.view(np.int64), bflat.view(np.int64)), f"{what} component {c}: wrote outside the clip box"
    print(f"{what}: worst |f_dev - f_ref| / bound = {worst:.3f}")


def host_images(ts):
    out = []
    for t in ts:
        flat, view = image(t)
        out.append((flat, view))
    return out


# ---- interp ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ic.CASES)
def test_interp_bit_for_bit(le, imp, ctx, name):
    c = ic.case(name)
    ic.check_preconditions(c, ties=name in ("pow2", "2d"))
    geo, nd, n = c["geo"], c["geo"].ndim, c["X"].shape[0]
    geom = make_geom(le, name)
    u = upload(geom, c["u"])
    X = dev(c["X"])
    m = le.Markers(ctx).bin(geom, "IB_6", X)
    U = torch.full((n, nd), SENT, dtype=torch.float64, device=DEV)
    G = torch.full((n, nd * nd), SENT, dtype=torch.float64, device=DEV)
    imp.interp_velocity_gradient(ctx, m, geom, u, U, G, X)
    ctx.synchronize()
    Uh, Gh = U.cpu().numpy(), G.cpu().numpy()
    bad_U = int((ir.bits(Uh) != ir.bits(c["U"])).sum())
    bad_G = int((ir.bits(Gh) != ir.bits(c["GradU"])).sum())
    print(f"{name}: U differs in {bad_U} values (max {np.abs(Uh - c['U']).max():.3e}), "
          f"GradU in {bad_G} (max {np.abs(Gh - c['GradU']).max():.3e})")
    assert bad_U == 0 and bad_G == 0
    # the sub-list: permuted, ten markers named twice, rows it does not name keep the sentinel
    idx = c["sub_idx"]
    m2 = le.Markers(ctx).bin(geom, "IB_6", X, indices=dev(idx, torch.int32))
    U.fill_(SENT)
    G.fill_(SENT)
    imp.interp_velocity_gradient(ctx, m2, geom, u, U, G, X)
    ctx.synchronize()
    assert np.array_equal(ir.bits(U.cpu().numpy()), ir.bits(c["sub_U"]))
    assert np.array_equal(ir.bits(G.cpu().numpy()), ir.bits(c["sub_GradU"]))
    unnamed = np.setdiff1d(np.arange(n), idx)
    assert len(unnamed) > 0 and (U.cpu().numpy()[unnamed] == SENT).all()
    # an empty list writes nothing
    m3 = le.Markers(ctx).bin(geom, "IB_6", X, indices=torch.empty(0, dtype=torch.int32, device=DEV))
    U.fill_(SENT)
    imp.interp_velocity_gradient(ctx, m3, geom, u, U, G, X)
    ctx.synchronize()
    assert (U.cpu().numpy() == SENT).all()


# ---- spread ------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip", ["patch", "ghost"])
@pytest.mark.parametrize("name", ic.CASES)
def test_spread_within_the_derived_bound(le, imp, ctx, name, clip):
    c = ic.case(name)
    ic.check_preconditions(c, ties=name in ("pow2", "2d"))
    geo = c["geo"]
    geom = make_geom(le, name)
    X, tau, wgt = dev(c["X"]), dev(c["tau"]), dev(c["wgt"])
    m = le.Markers(ctx).bin(geom, "IB_6", X)
    f = force_arrays(geom, geo, clip)
    before = host_images(f)
    imp.spread_stress(ctx, m, geom, f, tau, wgt, X, clip=clip)
    ctx.synchronize()
    first = [span(t).cpu().numpy().copy() for t in f]
    check_spread(geo, f, before, c["f_" + clip], c["cnt_" + clip], c["S_" + clip], clip, f"{name}/{clip}")
    # a second run from the same start: bit-identical
    f2 = force_arrays(geom, geo, clip)
    imp.spread_stress(ctx, m, geom, f2, tau, wgt, X, clip=clip)
    ctx.synchronize()
    for a, t in zip(first, f2):
        assert np.array_equal(a.view(np.int64), span(t).cpu().numpy().view(np.int64))


@pytest.mark.parametrize("name", ["g4", "2d"])
def test_spread_sublist_and_empty_list(le, imp, ctx, name):
    c = ic.case(name)
    geo = c["geo"]
    geom = make_geom(le, name)
    X, tau, wgt = dev(c["X"]), dev(c["tau"]), dev(c["wgt"])
    m = le.Markers(ctx).bin(geom, "IB_6", X, indices=dev(c["sub_idx"], torch.int32))
    f = force_arrays(geom, geo, "patch")
    before = host_images(f)
    imp.spread_stress(ctx, m, geom, f, tau, wgt, X)
    ctx.synchronize()
    check_spread(geo, f, before, c["sub_f"], c["sub_cnt"], c["sub_S"], "patch", f"{name}/sub-list")
    m0 = le.Markers(ctx).bin(geom, "IB_6", X, indices=torch.empty(0, dtype=torch.int32, device=DEV))
    f = force_arrays(geom, geo, "patch")
    before = host_images(f)
    imp.spread_stress(ctx, m0, geom, f, tau, wgt, X)
    ctx.synchronize()
    for t, (bflat, _) in zip(f, before):
        assert np.array_equal(span(t).cpu().numpy().view(np.int64), bflat.view(np.int64))


@pytest.mark.parametrize("name", ["g4", "2d"])
def test_power_identity_and_zero_net_force_on_device_results(le, imp, ctx, name):
    """The identities of tests/test_imp_cpu.py with the device's f and GradU, same bounds;
    interior points only, so no stencil is clipped."""
    geo = ic.geo_of(name)
    nd = geo.ndim
    geom = make_geom(le, name)
    rng = np.random.default_rng(77)
    xl, dx, nn = np.array(geo.x_lower), np.array(geo.dx), np.array(geo.n)
    Xh = rng.uniform(xl, xl + nn * dx, (300, nd))
    n = Xh.shape[0]
    uh = [rng.standard_normal(geo.shape(a)) for a in range(nd)]
    tauh, wgth = rng.standard_normal((n, nd * nd)), rng.uniform(0.5, 1.5, n)
    _, cnt, S = ir.spread(geo, geo.alloc(), tauh, wgth, Xh, clip="ghost", stats=True)
    assert not ir.interp(geo, uh, Xh)[2].any()
    X, tau, wgt = dev(Xh), dev(tauh), dev(wgth)
    m = le.Markers(ctx).bin(geom, "IB_6", X)
    f = geom.alloc("side")
    imp.spread_stress(ctx, m, geom, f, tau, wgt, X, clip="ghost")
    U = torch.zeros((n, nd), dtype=torch.float64, device=DEV)
    G = torch.zeros((n, nd * nd), dtype=torch.float64, device=DEV)
    imp.interp_velocity_gradient(ctx, m, geom, upload(geom, uh), U, G, X)
    ctx.synchronize()
    import math
    fh = [t.cpu().numpy() for t in f]
    dV = float(np.prod(geo.dx))
    lhs = math.fsum(float(v) for a in range(nd) for v in (fh[a] * uh[a]).ravel()) * dV
    rhs = -math.fsum(float(v) for v in (wgth[:, None] * tauh * G.cpu().numpy()).ravel())
    T = math.fsum(float(v) for a in range(nd) for v in (S[a] * np.abs(uh[a])).ravel()) * dV
    print(f"{name}: power |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {2 * (6 ** nd + 8) * 2.0 ** -53 * T:.3e}")
    assert abs(lhs) > 0.0 and abs(lhs - rhs) <= 2 * (6 ** nd + 8) * 2.0 ** -53 * T
    for a in range(nd):
        assert abs(math.fsum(float(v) for v in fh[a].ravel())) <= 64 * 2.0 ** -52 * float(S[a].sum())


def test_periodic_fold_equals_the_image_list(le, imp, ctx):
    """A periodic unit box: clip="patch" with le.periodic_index_list's images, and
    clip="ghost" followed by le.fold_periodic_ghosts, both against imp_ref on the image list
    and to its bound, over the unique points."""
    N, g = (12, 10, 9), 4
    geom = le.Geometry.periodic_unit(list(N), g)
    geo = ir.Geo((0, 0, 0), N, geom.dx, (0.0, 0.0, 0.0), g)
    rng = np.random.default_rng(12109)
    Xh = rng.uniform(0.0, 1.0, (500, 3))
    tauh, wgth = rng.standard_normal((500, 9)), rng.uniform(0.5, 1.5, 500) * float(np.prod(geom.dx))
    X, tau, wgt = dev(Xh), dev(tauh), dev(wgth)
    idx, xs = le.periodic_index_list(ctx, geom, X, g)
    idx_h, xs_h = idx.cpu().numpy(), xs.cpu().numpy()
    assert len(idx_h) > 500 and np.abs(xs_h).max() == 1.0  # images are in the list
    f_ref, cnt, S = ir.spread(geo, geo.alloc(), tauh, wgth, Xh, indices=idx_h, xshift=xs_h, clip="patch", stats=True)
    m = le.Markers(ctx).bin(geom, "IB_6", X, indices=idx, Xshift=xs)
    fa = geom.alloc("side")
    imp.spread_stress(ctx, m, geom, fa, tau, wgt, X, clip="patch")
    m2 = le.Markers(ctx).bin(geom, "IB_6", X)
    fb = geom.alloc("side")
    imp.spread_stress(ctx, m2, geom, fb, tau, wgt, X, clip="ghost")
    le.fold_periodic_ghosts(ctx, geom, "side", fb)
    ctx.synchronize()
    uniq = tuple(slice(g, g + N[d]) for d in reversed(range(3)))
    for c in range(3):
        bound = ic.spread_bound(cnt[c][uniq], S[c][uniq], Q)
        assert np.abs(f_ref[c][uniq]).max() > 0.0
        for what, t in (("image list", fa), ("ghost + fold", fb)):
            diff = np.abs(t[c].cpu().numpy()[uniq] - f_ref[c][uniq])
            ratio = float((diff / np.where(bound > 0, bound, 1.0)).max())
            print(f"component {c}, {what}: worst |diff| / bound = {ratio:.3f}")
            assert (diff <= bound).all(), (c, what, ratio)


# ---- refusals that need a binned list ------------------------------------------------------------

def test_refuses_other_kernel_geometry_and_ghost_width(le, imp, ctx):
    from ibamr_amd._lib import IBTKLEError
    name = "g4"
    c = ic.case(name)
    geom = make_geom(le, name)
    X = dev(c["X"])
    n = X.shape[0]
    u = geom.alloc("side")
    U = torch.full((n, 3), SENT, dtype=torch.float64, device=DEV)
    G = torch.full((n, 9), SENT, dtype=torch.float64, device=DEV)
    tau, wgt = dev(c["tau"]), dev(c["wgt"])
    m4 = le.Markers(ctx).bin(geom, "IB_4", X)
    other = le.Geometry(geom.ilower, geom.iupper, 5, geom.dx, geom.x_lower)
    m6 = le.Markers(ctx).bin(geom, "IB_6", X)
    thin = le.Geometry(geom.ilower, geom.iupper, 3, geom.dx, geom.x_lower)
    for mk, gm, arrays, code, text in ((m4, geom, u, 4, "not IB_6"), (m6, other, other.alloc("side"), 4, "different patch"),
                                       (m6, thin, thin.alloc("side"), 2, "insufficient ghost")):
        for call in (lambda: imp.interp_velocity_gradient(ctx, mk, gm, arrays, U, G, X),
                     lambda: imp.spread_stress(ctx, mk, gm, arrays, tau, wgt, X)):
            with pytest.raises(IBTKLEError) as e:
                call()
            assert e.value.code == code and text in str(e.value)
    ctx.synchronize()
    assert (U.cpu().numpy() == SENT).all() and all(not t.any() for t in u)
    with pytest.raises(IBTKLEError):
        imp.deformation_update(ctx, "trapezoidal", 0.1, G, G)


# ---- update and stress -----------------------------------------------------------------------------

def tol(kat, q):
    return 8 * max(float(kat["ref_err_" + q]), 2.0 ** -52)


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def deformation_inputs(n, nd, dt, seed):
    """dt |G| <= 0.2 and det F in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    w = nd * nd
    G0 = rng.uniform(-0.2 / dt, 0.2 / dt, (n, w)) / nd
    G1 = rng.uniform(-0.2 / dt, 0.2 / dt, (n, w)) / nd
    F = np.tile(np.eye(nd).reshape(1, w), (n, 1)) + rng.uniform(-0.15, 0.15, (n, w))
    d = np.linalg.det(F.reshape(n, nd, nd))
    assert d.min() >= 0.5 and d.max() <= 2.0 and np.abs(dt * G0).max() <= 0.2 and np.abs(dt * G1).max() <= 0.2
    return F, G0, G1


def run_update(imp, ctx, scheme, dt, F, G0, G1):
    Fd = dev(F)
    half = torch.full_like(Fd, SENT) if scheme == "euler" else None
    new = imp.deformation_update(ctx, scheme, dt, Fd, dev(G0), dev(G1) if scheme == "trapezoidal" else None,
                                 F_half=half)
    ctx.synchronize()
    return new.cpu().numpy(), None if half is None else half.cpu().numpy()


def run_stress(imp, ctx, F, c1, p0, beta):
    Fd = dev(F)
    tau = torch.full_like(Fd, SENT)
    imp.kirchhoff_stress(ctx, Fd, tau, c1, p0, beta)
    ctx.synchronize()
    return tau.cpu().numpy()


@pytest.mark.parametrize("nd", [3, 2])
def test_update_and_stress_against_the_known_answers(imp, ctx, kat, nd):
    F, G0, G1, dt = kat[f"p{nd}_F"], kat[f"p{nd}_G0"], kat[f"p{nd}_G1"], float(kat["p_dt"])
    for scheme in ("euler", "midpoint", "trapezoidal"):
        new, half = run_update(imp, ctx, scheme, dt, F, G0, G1)
        e = rel(new, kat[f"p{nd}_{scheme}_new"])
        print(f"{nd}-D {scheme}: F_new {e:.3e} (tol {tol(kat, f'{scheme}_new{nd}'):.3e})")
        assert e <= tol(kat, f"{scheme}_new{nd}")
        if scheme == "euler":
            assert rel(half, kat[f"p{nd}_euler_half"]) <= tol(kat, f"euler_half{nd}")
    for k, (c1, p0, beta) in enumerate(kat["p_law"]):
        e = rel(run_stress(imp, ctx, F, c1, p0, beta), kat[f"p{nd}_tau{k}"])
        print(f"{nd}-D law {k}: tau {e:.3e} (tol {tol(kat, f'tau{k}_{nd}'):.3e})")
        assert e <= tol(kat, f"tau{k}_{nd}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("nd", [3, 2])
def test_update_and_stress_against_the_restatement(imp, ctx, kat, nd, n):
    dt = float(kat["p_dt"])
    F, G0, G1 = deformation_inputs(n, nd, dt, 100 * n + nd)
    for scheme in ("euler", "midpoint", "trapezoidal"):
        new, half = run_update(imp, ctx, scheme, dt, F, G0, G1)
        rn, rh = ir.deformation_update(scheme, dt, F, G0, G1)
        assert rel(new, rn) <= 2 * tol(kat, f"{scheme}_new{nd}")
        if scheme == "euler":
            assert rel(half, rh) <= 2 * tol(kat, f"euler_half{nd}")
    law = kat["p_law"]
    for k, (c1, p0, beta) in enumerate(law):
        assert rel(run_stress(imp, ctx, F, c1, p0, beta), ir.kirchhoff_stress(F, c1, p0, beta)) <= 2 * tol(kat, f"tau{k}_{nd}")
    # the per-subdomain table gives each point its own row's law
    sub = np.arange(n) % len(law)
    Fd = dev(F)
    tau = torch.full_like(Fd, SENT)
    imp.kirchhoff_stress(ctx, Fd, tau, dev(law), subdomain=dev(sub, torch.int32))
    ctx.synchronize()
    want = ir.kirchhoff_stress(F, law[sub, 0], law[sub, 1], law[sub, 2])
    assert rel(tau.cpu().numpy(), want) <= 2 * max(tol(kat, f"tau{k}_{nd}") for k in range(len(law)))
    # exact cases: G = 0 returns F_cur, F = I gives tau = 2 c1 I
    w = nd * nd
    new, half = run_update(imp, ctx, "euler", dt, F, np.zeros((n, w)), None)
    assert np.array_equal(ir.bits(new), ir.bits(F)) and np.array_equal(ir.bits(half), ir.bits(F))
    eye = np.tile(np.eye(nd).reshape(1, w), (n, 1))
    assert np.array_equal(ir.bits(run_stress(imp, ctx, eye, 0.05, 0.0, 0.0)), ir.bits(2.0 * 0.05 * eye))

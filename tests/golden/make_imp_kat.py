"""Known answers for the IMPMethod stages at 50 digits (mpmath), run by hand:

    python tests/golden/make_imp_kat.py        # writes tests/golden/imp_kat.npz

The inputs are float64 values drawn here; every result is computed from them in exact-real
semantics at 50 digits -- the kernel of IMPMethod.cpp:119-171 as a function of r, its
derivative by differentiation of phi (not from the dphi formulas), the interpolation and
spread sums, the deformation-gradient steps and the stress -- and rounded to float64.
ref_err_<q> = max |imp_ref - answer| / max |answer| records how far the float64 restatement
(tests/imp_ref.py) is from it.  No test imports mpmath.
"""
import sys
from pathlib import Path

import mpmath as mp
import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import imp_ref as ir  # noqa: E402

mp.mp.dps = 50
M = mp.mpf

K = (M(59) / 60) * (1 - mp.sqrt(1 - M(3220) / 3481))


def phi_of_r(r):
    r2, r3, r4, r6 = r ** 2, r ** 3, r ** 4, r ** 6
    alpha = M(28)
    beta = M(9) / 4 - M(3) / 2 * (K + r2) + (M(22) / 3 - 7 * K) * r - M(7) / 3 * r3
    gamma = M(1) / 4 * ((M(161) / 36 - M(59) / 6 * K + 5 * K ** 2) / 2 * r2 + (-M(109) / 24 + 5 * K) / 3 * r4
                        + M(5) / 18 * r6)
    p0 = (-beta + mp.sqrt(beta * beta - 4 * alpha * gamma)) / (2 * alpha)
    return [p0,
            -3 * p0 - M(1) / 16 + (K + r2) / 8 + (3 * K - 1) * r / 12 + r3 / 12,
            2 * p0 + M(1) / 4 + (4 - 3 * K) * r / 6 - r3 / 6,
            2 * p0 + M(5) / 8 - (K + r2) / 4,
            -3 * p0 + M(1) / 4 - (4 - 3 * K) * r / 6 + r3 / 6,
            p0 - M(1) / 16 + (K + r2) / 8 - (3 * K - 1) * r / 12 - r3 / 12]


def mp_nint(x):
    return int(mp.floor(abs(x) + M(1) / 2)) * (1 if x >= 0 else -1)


def kernel(X, xlo, dx, ilo):
    """lower, phi[6], dphi[6] (d phi / d r) at the float64 inputs, exactly."""
    X_o_dx = (M(float(X)) - M(float(xlo))) / M(float(dx))
    lower = mp_nint(X_o_dx) + ilo - 3
    r = 1 - X_o_dx + (lower + 2 - ilo) + M(1) / 2
    phi = phi_of_r(r)
    dphi = [mp.diff(lambda t, j=j: phi_of_r(t)[j], r) for j in range(6)]
    return lower, phi, dphi


def f64(a):
    return np.array([float(v) for v in a], dtype=np.float64)


def rel_err(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


def eulerian(geo, u, X, tau, wgt):
    """U, GradU, and f for both clips, exactly."""
    nd = geo.ndim
    n = X.shape[0]
    U = np.zeros((n, nd))
    G = np.zeros((n, nd * nd))
    f = {clip: [[M(0)] * a.size for a in u] for clip in ("patch", "ghost")}
    dV = M(1)
    for d in range(nd):
        dV *= M(geo.dx[d])
    for c in range(nd):
        glo, ghi = geo.ghost_box(c)
        plo, phi_box = geo.patch_side_box(c)
        shape = u[c].shape
        for s in range(n):
            ker = [kernel(X[s, d], geo.frame_lower(c, d), geo.dx[d], geo.ilower[d]) for d in range(nd)]
            Us, Gs = M(0), [M(0)] * nd
            for off in np.ndindex(*([6] * nd)):
                pos = [ker[d][0] + off[d] for d in range(nd)]
                if any(pos[d] < glo[d] or pos[d] > ghi[d] for d in range(nd)):
                    continue
                sel = tuple(pos[d] - glo[d] for d in reversed(range(nd)))
                w = M(1)
                for d in range(nd):
                    w *= ker[d][1][off[d]]
                dw = []
                for k in range(nd):
                    t = M(1)
                    for d in range(nd):
                        t *= ker[d][2][off[d]] / M(geo.dx[d]) if d == k else ker[d][1][off[d]]
                    dw.append(t)
                v = M(float(u[c][sel]))
                Us += v * w
                for k in range(nd):
                    Gs[k] -= v * dw[k]
                val = sum(M(float(tau[s, nd * c + k])) * dw[k] for k in range(nd)) * M(float(wgt[s])) / dV
                flat = int(np.ravel_multi_index(sel, shape))
                f["ghost"][c][flat] += val
                if all(plo[d] <= pos[d] <= phi_box[d] for d in range(nd)):
                    f["patch"][c][flat] += val
            U[s, c] = float(Us)
            for k in range(nd):
                G[s, nd * c + k] = float(Gs[k])
    fo = {clip: [f64(f[clip][c]).reshape(u[c].shape) for c in range(nd)] for clip in f}
    return U, G, fo


def mp_pad(row, nd, z22):
    A = mp.zeros(3, 3)
    for i in range(nd):
        for j in range(nd):
            A[i, j] = M(float(row[nd * i + j]))
    if nd == 2:
        A[2, 2] = M(z22)
    return A


def mp_rows(A, nd):
    return [float(A[i, j]) for i in range(nd) for j in range(nd)]


def update(scheme, dt, F, G0, G1, nd):
    new, half = [], []
    for s in range(F.shape[0]):
        Fm, Ga = mp_pad(F[s], nd, 1), mp_pad(G0[s], nd, 0)
        Gb = mp_pad(G1[s], nd, 0) if scheme == "trapezoidal" else Ga
        I = mp.eye(3)
        new.append(mp_rows(mp.inverse(I - M(dt) / 2 * Gb) * (I + M(dt) / 2 * Ga) * Fm, nd))
        half.append(mp_rows(mp.inverse(I - M(dt) / 4 * Gb) * (I + M(dt) / 4 * Ga) * Fm, nd))
    return np.array(new), np.array(half)


def stress(F, c1, p0, beta, nd):
    out = []
    for s in range(F.shape[0]):
        FF = mp_pad(F[s], nd, 1)
        PP = 2 * M(c1) * FF
        FinvT = mp.inverse(FF).T
        if p0 != 0.0:
            PP -= 2 * M(p0) * FinvT
        if beta != 0.0:
            PP += M(beta) * mp.log(mp.det(FF.T * FF)) * FinvT
        out.append(mp_rows(PP * FF.T, nd))
    return np.array(out)


def deformation_inputs(rng, n, nd, dt):
    """dt |G| <= 0.2 and det F in [0.5, 2]: the inverse is well conditioned."""
    w = nd * nd
    G0 = rng.uniform(-0.2 / dt, 0.2 / dt, (n, w)) / nd
    G1 = rng.uniform(-0.2 / dt, 0.2 / dt, (n, w)) / nd
    F = np.tile(np.eye(nd).reshape(1, w), (n, 1)) + rng.uniform(-0.15, 0.15, (n, w))
    d = np.linalg.det(F.reshape(n, nd, nd))
    assert d.min() >= 0.5 and d.max() <= 2.0
    return F, G0, G1


def main():
    rng = np.random.default_rng(20261020)
    out = {}
    # ---- the kernel and its derivative: random offsets, and exact ties -----------------
    xlo, dx, ilo = 0.3, 0.1, -1
    kx = np.concatenate([xlo + dx * rng.uniform(-3.0, 9.0, 48), xlo + 0.125 * np.array([0.5, 1.5, -0.5, -1.5])])
    kdx = np.concatenate([np.full(48, dx), np.full(4, 0.125)])
    phi, dphi = np.zeros((len(kx), 6)), np.zeros((len(kx), 6))
    phi_ref, dphi_ref = np.zeros_like(phi), np.zeros_like(dphi)
    for i, (x, h) in enumerate(zip(kx, kdx)):
        _, p, dp = kernel(x, xlo, h, ilo)
        phi[i], dphi[i] = f64(p), f64(dp)
        _, pr, dpr = ir.kernel(np.array([x]), xlo, h, ilo)
        phi_ref[i], dphi_ref[i] = pr[0], dpr[0]
    out.update(k_x=kx, k_dx=kdx, k_xlo=xlo, k_ilo=ilo, k_phi=phi, k_dphi=dphi,
               ref_err_phi=rel_err(phi_ref, phi), ref_err_dphi=rel_err(dphi_ref, dphi))
    # ---- the Eulerian stages on the tiny grids -----------------------------------------
    for tag, ilower, n, h, xl in (("3", (-1, 2, 0), (7, 6, 5), (0.1, 0.037, 0.2113), (0.3, -0.2, 0.1)),
                                  ("2", (2, -3), (7, 6), (0.1, 0.037), (0.3, -0.2))):
        nd = len(n)
        geo = ir.Geo(ilower, n, h, xl, 4)
        npt = 40 if nd == 3 else 24
        lo = np.array([xl[d] - 3.0 * h[d] for d in range(nd)])
        hi = np.array([xl[d] + (n[d] + 3.0) * h[d] for d in range(nd)])
        X = rng.uniform(lo, hi, (npt, nd))
        u = [rng.standard_normal(geo.shape(c)) for c in range(nd)]
        tau = rng.standard_normal((npt, nd * nd))
        wgt = rng.uniform(0.5, 1.5, npt) * float(np.prod(h))
        U, G, f = eulerian(geo, u, X, tau, wgt)
        Ur, Gr, _ = ir.interp(geo, u, X)
        out.update({f"e{tag}_ilower": np.array(ilower), f"e{tag}_n": np.array(n), f"e{tag}_dx": np.array(h),
                    f"e{tag}_x_lower": np.array(xl), f"e{tag}_X": X, f"e{tag}_tau": tau, f"e{tag}_wgt": wgt,
                    f"e{tag}_U": U, f"e{tag}_GradU": G, f"ref_err_U{tag}": rel_err(Ur, U),
                    f"ref_err_GradU{tag}": rel_err(Gr, G)})
        for c in range(nd):
            out[f"e{tag}_u{c}"] = u[c]
        for clip in ("patch", "ghost"):
            fr = ir.spread(geo, geo.alloc(), tau, wgt, X, clip=clip)
            for c in range(nd):
                out[f"e{tag}_f_{clip}{c}"] = f[clip][c]
            out[f"ref_err_f{tag}_{clip}"] = max(rel_err(fr[c], f[clip][c]) for c in range(nd))
    # ---- the pointwise stages ----------------------------------------------------------
    dt = 0.0125
    out["p_dt"] = dt
    out["p_law"] = np.array([[0.05, 0.0, 0.0], [0.7, 0.3, 0.0], [0.05, 0.2, 1.9]])
    for nd in (3, 2):
        F, G0, G1 = deformation_inputs(rng, 40, nd, dt)
        out.update({f"p{nd}_F": F, f"p{nd}_G0": G0, f"p{nd}_G1": G1})
        for scheme in ("euler", "midpoint", "trapezoidal"):
            new, half = update(scheme, dt, F, G0, G1, nd)
            rn, rh = ir.deformation_update(scheme, dt, F, G0, G1)
            out[f"p{nd}_{scheme}_new"] = new
            out[f"ref_err_{scheme}_new{nd}"] = rel_err(rn, new)
            if scheme == "euler":
                out[f"p{nd}_euler_half"] = half
                out[f"ref_err_euler_half{nd}"] = rel_err(rh, half)
        for k, (c1, p0, beta) in enumerate(out["p_law"]):
            t = stress(F, c1, p0, beta, nd)
            out[f"p{nd}_tau{k}"] = t
            out[f"ref_err_tau{k}_{nd}"] = rel_err(ir.kirchhoff_stress(F, c1, p0, beta), t)
    np.savez_compressed(HERE / "imp_kat.npz", **out)
    for k in sorted(out):
        if k.startswith("ref_err"):
            print(f"{k:28s} {float(out[k]):.3e}")


if __name__ == "__main__":
    main()

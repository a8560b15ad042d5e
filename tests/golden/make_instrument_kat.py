"""Known answers for the flow meters and pressure gauges, exact, run by hand:

    python tests/golden/make_instrument_kat.py        # writes tests/golden/instrument_kat.npz

The inputs are the float64 values of tests/instrument_cases.py.  The integer decisions --
num_web_nodes, the cell of a web patch and of a centroid, whether it is counted -- are those
of the float64 restatement (they are part of what is specified).  Every real-valued result is
computed from the inputs with fractions.Fraction: the centroid, t and s, X_web, dA_web, the
two interpolation rules at the exact X_web (lower or upper neighbours by the exact X < X_cell),
the correction.  Everything but |dA| is rational; |dA| = sqrt(dA . dA) is taken with decimal at
50 digits, and so are the two sums it enters and the mean pressure.  Each result is rounded to
float64 once.

Stored beside them, per quantity, the scale S = the sum of the absolute values of the terms that
are added to form it (for the mean pressure: that of its numerator over the exact area), and
how far the float64 restatement (tests/instrument_ref.py) is from exact, in units of 2^-53 S:
ref_err_Xweb, ref_err_dA, ref_err_flow, ref_err_mean, ref_err_point, ref_err_corr = the worst over
every stored case.  t and s cancel near the degenerate centre triangle of a web, so
ref_err_Xweb is what it measures, not an estimate.
"""
import decimal
import sys
from fractions import Fraction as Fr
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import instrument_cases as ic  # noqa: E402

decimal.getcontext().prec = 50
STORED = ("small", "tie", "cut", "outside", "big")
U53 = Fr(1, 2 ** 53)
R3 = range(3)


def F(v):
    return Fr(float(v))


def dec(fr):
    return decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)


def to_float(v):
    return float(v)  # Fraction and Decimal both round to nearest


def dot(a, b):
    return sum(a[d] * b[d] for d in R3)


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def exact_web(Xp, Xc, nw):
    """X_web, dA_web and their scales, exactly."""
    P = len(Xp)
    out = []
    for m in range(P):
        a, b = Xp[m], Xp[(m + 1) % P]
        dX0 = [(Xc[d] - a[d]) / nw for d in R3]
        dX1 = [(Xc[d] - b[d]) / nw for d in R3]
        row = []
        for n in range(nw):
            X0 = [a[d] + n * dX0[d] for d in R3]
            X1 = [b[d] + n * dX1[d] for d in R3]
            X2 = [b[d] + (n + 1) * dX1[d] for d in R3]
            X3 = [a[d] + (n + 1) * dX0[d] for d in R3]
            l0 = [(X0[d] + X1[d]) / 2 for d in R3]
            l1 = [(X1[d] + X2[d]) / 2 for d in R3]
            d0 = [(X2[d] + X3[d]) / 2 - l0[d] for d in R3]
            d1 = [(X3[d] + X0[d]) / 2 - l1[d] for d in R3]
            den = dot(d1, d1) * dot(d0, d0) - dot(d0, d1) ** 2
            t = (-dot(d0, l0) * dot(d1, d1) + dot(d0, l1) * dot(d1, d1) + dot(d0, d1) * dot(d1, l0)
                 - dot(d0, d1) * dot(d1, l1)) / den
            s = (dot(d1, l0) * dot(d0, d0) - dot(d0, d1) * dot(d0, l0) + dot(d0, d1) * dot(d0, l1)
                 - dot(d1, l1) * dot(d0, d0)) / den
            Xw = [(l0[d] + t * d0[d] + l1[d] + s * d1[d]) / 2 for d in R3]
            SX = [(abs(l0[d]) + abs(t * d0[d]) + abs(l1[d]) + abs(s * d1[d])) / 2 for d in R3]
            p, q = [X2[d] - X0[d] for d in R3], [X3[d] - X1[d] for d in R3]
            dA = [c / 2 for c in cross(p, q)]
            SA = [(abs(p[1] * q[2]) + abs(p[2] * q[1])) / 2, (abs(p[2] * q[0]) + abs(p[0] * q[2])) / 2,
                  (abs(p[0] * q[1]) + abs(p[1] * q[0])) / 2]
            row.append((Xw, dA, SX, SA))
        out.append(row)
    return out


def hat(X, Xc, dx):
    return (X - (Xc - dx) if X < Xc else (Xc + dx) - X) / dx


def exact_interp(geo, v, X, i, axis=None):
    """The cell rule (axis None) or one axis of the side rule at X in cell i: (value, sum |terms|)."""
    dx = [F(h) for h in geo.dx]
    Xcell = [F(geo.x_lower[d]) + dx[d] * (Fr(i[d] - geo.ilower[d]) + Fr(1, 2)) for d in R3]
    lo = [-1 if (d != axis and X[d] < Xcell[d]) else 0 for d in R3]
    val, scale = Fr(0), Fr(0)
    for s2 in (lo[2], lo[2] + 1):
        for s1 in (lo[1], lo[1] + 1):
            for s0 in (lo[0], lo[0] + 1):
                sh = (s0, s1, s2)
                Xs = [Xcell[d] + (Fr(sh[d]) - (Fr(1, 2) if d == axis else 0)) * dx[d] for d in R3]
                w = hat(X[0], Xs[0], dx[0]) * hat(X[1], Xs[1], dx[1]) * hat(X[2], Xs[2], dx[2])
                term = F(v[geo.at((i[0] + s0, i[1] + s1, i[2] + s2))]) * w
                val += term
                scale += abs(term)
    return val, scale


def exact_case(c):
    geo = c["geo"]
    out = {k: [] for k in ("Xweb", "dA", "S_Xweb", "S_dA", "values", "S_values", "corr", "S_corr")}
    for l, w in enumerate(c["webs"]):
        P, nw = w["P"], w["nw"]
        Xp = [[F(v) for v in x] for x in w["Xp"]]
        Xc = [sum(Xp[n][d] for n in range(P)) / P for d in R3]
        web = exact_web(Xp, Xc, nw)
        flow, S_flow = Fr(0), Fr(0)
        num, area, S_num = decimal.Decimal(0), decimal.Decimal(0), decimal.Decimal(0)
        for m in range(P):
            for n in range(nw):
                Xw, dA, SX, SA = web[m][n]
                out["Xweb"].append([to_float(v) for v in Xw])
                out["dA"].append([to_float(v) for v in dA])
                out["S_Xweb"].append([to_float(v) for v in SX])
                out["S_dA"].append([to_float(v) for v in SA])
                if not w["counted"][m][n]:
                    continue
                i = w["cell"][m][n]
                for a in R3:
                    val, sc = exact_interp(geo, c["u"][a], Xw, i, axis=a)
                    flow += val * dA[a]
                    S_flow += sc * abs(dA[a])
                val, sc = exact_interp(geo, c["p"], Xw, i)
                nrm = dec(dot(dA, dA)).sqrt()
                num += dec(val) * nrm
                S_num += dec(sc) * nrm
                area += nrm
        Up = [[F(c["U"][k][d]) for d in R3] for k in c["meters"][l]]
        Uc = [sum(Up[n][d] for n in range(P)) / P for d in R3]
        corr, S_corr = Fr(0), Fr(0)
        for m in range(P):
            m1 = (m + 1) % P
            U = [(Up[m][d] + Up[m1][d] + Uc[d]) / 3 for d in R3]
            dA = [v / 2 for v in cross([Xc[d] - Xp[m][d] for d in R3], [Xc[d] - Xp[m1][d] for d in R3])]
            corr += dot(U, dA)
            S_corr += sum(abs(U[d] * dA[d]) for d in R3)
        point, S_point = (exact_interp(geo, c["p"], Xc, w["cen_cell"]) if w["cen_counted"] else (Fr(0), Fr(0)))
        out["values"].append([to_float(flow - corr), to_float(num / area), to_float(point)])
        out["S_values"].append([to_float(S_flow + S_corr), to_float(S_num / area), to_float(S_point)])
        out["corr"].append(to_float(corr))
        out["S_corr"].append(to_float(S_corr))
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}


def restated(c):
    """The restatement's values in the layout of exact_case."""
    Xweb, dA = [], []
    for w in c["webs"]:
        for m in range(w["P"]):
            for n in range(w["nw"]):
                Xweb.append(w["X_web"][m][n])
                dA.append(w["dA_web"][m][n])
    return dict(Xweb=np.array(Xweb).reshape(-1, 3), dA=np.array(dA).reshape(-1, 3), values=c["values"],
                corr=np.array([s["corr"] for s in c["stats"]]))


def units(got, exact, scale):
    """max |got - exact| / (2^-53 scale) (0 / 0 = 0)."""
    diff = np.abs(np.asarray(got, dtype=np.float64) - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, diff / (2.0 ** -53 * scale), np.where(diff > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def main():
    store = {}
    worst = dict(Xweb=0.0, dA=0.0, flow=0.0, mean=0.0, point=0.0, corr=0.0)
    for name in STORED:
        c = ic.case(name)
        ex = exact_case(c)
        got = restated(c)
        for k, v in ex.items():
            store[f"{name}_{k}"] = v
        e = dict(Xweb=units(got["Xweb"], ex["Xweb"], ex["S_Xweb"]), dA=units(got["dA"], ex["dA"], ex["S_dA"]),
                 corr=units(got["corr"], ex["corr"], ex["S_corr"]))
        for j, k in enumerate(("flow", "mean", "point")):
            e[k] = units(got["values"][:, j], ex["values"][:, j], ex["S_values"][:, j])
        print(name, {k: round(v, 3) for k, v in e.items()})
        for k, v in e.items():
            worst[k] = max(worst[k], v)
    for k, v in worst.items():
        store[f"ref_err_{k}"] = np.float64(v)
    print("worst", worst)
    np.savez_compressed(HERE / "instrument_kat.npz", **store)


if __name__ == "__main__":
    main()

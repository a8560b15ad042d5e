"""Known answers for the fluid-source stages at 50 digits (mpmath), run by hand:

    python tests/golden/make_source_kat.py        # writes tests/golden/source_kat.npz

The inputs are the float64 values of tests/source_cases.py.  The integer decisions -- the
radius in cells, the centre cell, the half width, the clipped box -- are those of the float64
arithmetic (they are part of what is specified); every real-valued result is computed from
the inputs in exact-real semantics at 50 digits -- the cell centres, cos_kernel with
|x| <= r decided exactly, the products, the sums, the means -- and rounded to float64.

Recorded beside them, how far the float64 restatement (tests/source_ref.py) is from exact:
ref_err_w = max |w_1D - exact| r / 2^-53 over every 1-D weight of every case, and
ref_err_q, ref_err_P, ref_err_Xsrc = max |v - exact| / max |exact|.  No test imports mpmath.
"""
import sys
from pathlib import Path

import mpmath as mp
import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import source_cases as sc  # noqa: E402
import source_ref as sr  # noqa: E402

mp.mp.dps = 50
M = lambda v: mp.mpf(float(v))  # noqa: E731

STORED = ("main", "clip", "many", "main2", "clip2", "many2")  # the pitched cases share their answers


def exact_weight(geo, st, X, d, i):
    """cos_kernel at cell i of dimension d, exactly, and the radius."""
    r = st[d]["R"] * M(geo.dx[d])  # R dx, exactly
    xc = M(geo.x_lower[d]) + M(geo.dx[d]) * (M(i - geo.ilower[d]) + M(1) / 2)
    x = xc - M(X[d])
    if abs(x) > r:
        return mp.mpf(0), r
    return (1 + mp.cos(mp.pi * x / r)) / (2 * r), r


def exact_case(c):
    geo = c["geo"]
    nd = geo.ndim
    q = {a: M(v) for a, v in np.ndenumerate(c["q0"][geo.box_slices()])}
    off = tuple(s.start for s in geo.box_slices())
    P = []
    w_all, err_w = [], 0.0
    for n in range(len(c["Q"])):
        X = [float(v) for v in c["X_src"][n]]
        st = sr.stencil(geo, float(c["r_src"][n]), X)
        tabs = []
        for d in range(nd):
            tab = {}
            for i in range(st[d]["lo"], st[d]["hi"] + 1):
                w, r = exact_weight(geo, st, X, d, i)
                tab[i] = w
                got = sr.weight_1d(geo, st, X, d, i)
                err_w = max(err_w, float(abs(M(got) - w) * r / mp.mpf(2) ** -53))
                w_all.append(float(w))
            tabs.append(tab)
        acc = mp.mpf(0)
        for i in sr.box_cells(st):
            wgt = mp.mpf(1)
            wdx = mp.mpf(1)
            for d in range(nd):
                wgt *= tabs[d][i[d]]
                wdx *= tabs[d][i[d]] * M(geo.dx[d])
            a = geo.at(i)
            q[tuple(a[k] - off[k] for k in range(nd))] += M(c["Q"][n]) * wgt
            acc += M(c["p"][a]) * wdx
        P.append(acc)
    box = np.zeros(geo.shape(), dtype=bool)
    box[geo.box_slices()] = True
    vals = c["p"][sr.bdry_mask(geo, c["domain_big"]) & box]
    p_norm = sum((M(v) for v in vals), mp.mpf(0)) / len(vals)
    qx = np.zeros(tuple(geo.n[d] for d in reversed(range(nd))))
    for a, v in q.items():
        qx[a] = float(v)
    return dict(q=qx, P=np.array([float(v) for v in P]), P_normed=np.array([float(v - p_norm) for v in P]),
                p_norm=float(p_norm), w=np.array(w_all)), err_w


def exact_locations(nd):
    X, node, source, n_src = sc.node_lists(nd)
    out = np.zeros((n_src, nd))
    for k in range(n_src):
        mine = node[source == k]
        for d in range(nd):
            if len(mine):
                out[k, d] = float(sum((M(X[i, d]) for i in mine), mp.mpf(0)) / len(mine))
    return out, sr.locations(X, node, source, n_src)


def rel_err(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


def main():
    out = {}
    err_w = err_q = err_P = err_X = 0.0
    for name in STORED:
        c = sc.case(name)
        sc.check_weights(c["geo"], c["r_src"], c["X_src"])
        ex, ew = exact_case(c)
        err_w = max(err_w, ew)
        err_q = max(err_q, rel_err(c["q"][c["geo"].box_slices()], ex["q"]))
        err_P = max(err_P, rel_err(c["P"], ex["P"]), rel_err(c["P_normed"], ex["P_normed"]))
        for k in ("P", "P_normed", "p_norm", "w"):
            out[f"{name}_{k}"] = ex[k]
        if not name.startswith("many"):
            out[f"{name}_q"] = ex["q"]
        print(f"{name}: ref_err_w so far {err_w:.3f}, q {err_q:.3e}, P {err_P:.3e}")
    for nd in (3, 2):
        ex, got = exact_locations(nd)
        err_X = max(err_X, rel_err(got, ex))
        out[f"Xsrc{nd}"] = ex
    out.update(ref_err_w=err_w, ref_err_q=err_q, ref_err_P=err_P, ref_err_Xsrc=err_X)
    print(f"ref_err_w {err_w:.3f}  ref_err_q {err_q:.3e}  ref_err_P {err_P:.3e}  ref_err_Xsrc {err_X:.3e}")
    np.savez(HERE / "source_kat.npz", **out)


if __name__ == "__main__":
    main()

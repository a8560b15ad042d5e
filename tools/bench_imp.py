"""Time the four device stages of IMPMethod (ibamr_amd.imp) beside the existing IB_6 interp and
spread on the same markers.

Workload: periodic unit boxes of --sizes cells per dim (default 128 and 256) with ghost width
4 and --density points per cell (default 1e6 / 128^3 = 0.477: 1e6 and 8e6 points), uniform.

For each size, between HIP events on the context stream, after --warmup calls, the median,
min and max over --iters calls of
  * imp.interp_velocity_gradient, imp.spread_stress (clip="ghost"), imp.deformation_update
    ("euler" with F_half) and imp.kirchhoff_stress (c1, p0 and beta all non-zero);
  * le.interp and le.zero_spread with "IB_6", side-centred, on the same binned markers: the
    only yardsticks the library had.  The new interp forms four sums per component where
    le.interp forms one; the new spread scatters three weight tensors where le.zero_spread
    scatters one (and le.zero_spread also zeroes the arrays, which spread_stress does not).
and the bytes each call must move per point, every array read or written once:
  * interp: the sorted position 24, its row 4, U 24, GradU 72 (the grid, 3 * 8 bytes per cell,
    is read through the caches: 6^3 values per component and point);
  * spread: position 24, row 4, tau 72, wgt 8 -- read once per tile that the point reaches --,
    the sort's keys and values 16 (per radix pass), and 3 * 16 bytes per cell of f;
  * update: F_cur 72, G 72, F_new 72, F_half 72; stress: F 72, tau 72.

One JSON line, and --out (default profiles/imp.json).

Usage: python tools/bench_imp.py [--sizes 128 256] [--density D] [--iters K] [--warmup W] [--out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--density", type=float, default=1.0e6 / 128 ** 3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "imp.json"))
    args = ap.parse_args()

    import torch

    from ibamr_amd import build, imp, le

    if not torch.cuda.is_available():
        sys.exit("bench_imp: no GPU (this measurement has no CPU fallback)")
    ctx = le.Context(0)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}  # noqa: E731
    cases = []
    for N in args.sizes:
        n = int(round(args.density * N ** 3))
        geom = le.Geometry.periodic_unit([N, N, N], imp.MIN_GHOST)
        gen = torch.Generator(device="cuda").manual_seed(N)
        X = torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
        u = geom.alloc("side")
        for a in u:
            a.copy_(torch.randn(a.shape, dtype=torch.float64, device="cuda", generator=gen))
        f = geom.alloc("side")
        markers = le.Markers(ctx).bin(geom, "IB_6", X)
        U = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        G = torch.empty((n, 9), dtype=torch.float64, device="cuda")
        wgt = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
        F = torch.eye(3, dtype=torch.float64, device="cuda").reshape(1, 9).repeat(n, 1).contiguous()
        F += 0.1 * (torch.rand((n, 9), dtype=torch.float64, device="cuda", generator=gen) - 0.5)
        Fn, Fh, tau = torch.empty_like(F), torch.empty_like(F), torch.empty_like(F)
        dt = 1.0e-3

        t = {}
        t["imp_interp"] = timed(lambda: imp.interp_velocity_gradient(ctx, markers, geom, u, U, G, X))
        t["le_interp_IB_6"] = timed(lambda: le.interp(ctx, markers, "IB_6", "side", geom, u, U, X))
        t["imp_update"] = timed(lambda: imp.deformation_update(ctx, "euler", dt, F, G, F_new=Fn, F_half=Fh))
        t["imp_stress"] = timed(lambda: imp.kirchhoff_stress(ctx, Fn, tau, 0.05, 0.02, 1.5))
        t["imp_spread"] = timed(lambda: imp.spread_stress(ctx, markers, geom, f, tau, wgt, X, clip="ghost"))
        t["le_zero_spread_IB_6"] = timed(lambda: le.zero_spread(ctx, markers, "IB_6", "side", geom, f, U, X))
        finite = bool(torch.isfinite(G).all() and torch.isfinite(tau).all() and all(torch.isfinite(a).all() for a in f))
        med = {k: statistics.median(v) for k, v in t.items()}
        cases.append({
            "N": N, "points": n, "ghost": imp.MIN_GHOST, "results_finite": finite,
            "ms": {k: stat(v) for k, v in t.items()},
            "imp_interp_over_le_interp": round(med["imp_interp"] / med["le_interp_IB_6"], 3),
            "imp_spread_over_le_zero_spread": round(med["imp_spread"] / med["le_zero_spread_IB_6"], 3),
            "bytes_per_point": {"imp_interp": 124, "imp_spread": 108 + 16, "imp_update": 288, "imp_stress": 144},
            "grid_bytes_per_cell": {"imp_interp": 24, "imp_spread": 48},
            "GB_per_s": {"imp_update": round(288 * n / (med["imp_update"] * 1e-3) / 1e9, 1),
                         "imp_stress": round(144 * n / (med["imp_stress"] * 1e-3) / 1e9, 1)},
        })
        del u, f, markers, X, U, G, F, Fn, Fh, tau, wgt
        torch.cuda.empty_cache()
    res = {"bench": "imp_uniform", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
           "iters": args.iters, "warmup": args.warmup, "density": args.density, "cases": cases}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Time the device force stage (ibtk_le_forcegen_compute) against the copies it replaces.

Workload: a 3-D sheet of N x N nodes (node (i, j) = i N + j), a spring to each of the four
neighbours, a beam through every node along both directions, a target point with damping on
every node -- the incidence mix of an elastic shell.  N defaults to 3162 (about 1e7 nodes).

Reports, on one JSON line (and into --out):
  * kernel_ms: the compute call between HIP events on the context stream, after warm-up
    (median and min over --iters calls; F = acc, so F is written and not read);
  * algorithmic bytes (the plan's offsets and records, X, U and F once each; the
    neighbour gathers of X are taken as cache hits) and bytes per second over the median;
  * copy_ms: a pinned device-to-host copy of X plus a pinned host-to-device copy of F of the
    same size, the least a step pays for this stage when the forces are computed on the host.

--renumber measures the regrid instead: the plan rebuilt for a new numbering of the nodes (a
seeded random permutation), on the device (ForceGen.renumber from a DeviceForceSpecs uploaded
once; HIP events around the call, warm-up calls, then min / median / max) and by the host
route it replaces (ForceSpecs.arrays(perm), then ForceGen(...) through the set_* calls and
their upload; wall clock, --host-iters times).  The two plans are compared byte for byte
unless --no-verify.  Default --out: profiles/forcegen_renumber.json.

--jacobian measures the force Jacobian on the same sheet: the pattern build
(ForceJacobian.rebuild, which ends in one small read), assemble, apply, ForceGen.linearized and,
alternating with them in the same process, compute(dX=...), whose bytes linearized moves; HIP
events, warm-up and --iters as above.  Each time stands next to its algorithmic bytes and the
fraction of 6.29 TB/s (the achievable streaming rate) they amount to.  Default --out:
profiles/forcejac_sheet.json.

Usage: python tools/bench_forcegen.py [--n-side N] [--iters K] [--warmup W] [--out FILE]
       python tools/bench_forcegen.py --renumber [--n-side N] [--iters K] [--warmup W] [--host-iters H]
       python tools/bench_forcegen.py --jacobian [--n-side N] [--iters K] [--warmup W] [--out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def sheet(N: int, rng):
    """Flat plan arrays of the sheet, in the reference's order (master by master)."""
    idx = np.arange(N * N, dtype=np.int64).reshape(N, N)
    # springs: master = the smaller index; per master, the edge along j then the edge along i
    right = np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()])
    down = np.stack([idx[:-1, :].ravel(), idx[1:, :].ravel()])
    e = np.concatenate([right, down], axis=1)
    e = e[:, np.argsort(e[0], kind="stable")]
    ns = e.shape[1]
    springs = (e[0].astype(np.int32), e[1].astype(np.int32), np.full(ns, 50.0), np.full(ns, 1.0 / N))
    # beams: (master, next, prev) along j and along i
    bj = np.stack([idx[:, 1:-1].ravel(), idx[:, 2:].ravel(), idx[:, :-2].ravel()])
    bi = np.stack([idx[1:-1, :].ravel(), idx[2:, :].ravel(), idx[:-2, :].ravel()])
    b = np.concatenate([bj, bi], axis=1)
    b = b[:, np.argsort(b[0], kind="stable")]
    nb = b.shape[1]
    beams = (b[0].astype(np.int32), b[1].astype(np.int32), b[2].astype(np.int32), np.full(nb, 0.25),
             np.zeros((nb, 3)))
    g = np.arange(N) / N
    X0 = np.stack([np.repeat(g, N), np.tile(g, N), np.full(N * N, 0.5)], axis=1)
    targets = (np.arange(N * N, dtype=np.int32), np.full(N * N, 10.0), np.full(N * N, 0.5), X0)
    X = X0 + rng.standard_normal(X0.shape) * (0.05 / N)
    return X, springs, beams, targets


def renumber_bench(args):
    import time

    import torch

    from ibamr_amd import build, io, le
    from ibamr_amd.forcegen import DeviceForceSpecs, ForceGen, ForceSpecs

    if not torch.cuda.is_available():
        sys.exit("bench_forcegen: no GPU (this measurement has no CPU fallback)")
    N, nd = args.n_side, 3
    n = N * N
    rng = np.random.default_rng(0)
    _, springs, beams, targets = sheet(N, rng)
    ns, nb, nt = springs[0].size, beams[0].size, targets[0].size
    sp = ForceSpecs(nd, targets[3], io.SpringDeck(*springs, np.zeros(ns, dtype=np.int32), []), io.BeamDeck(*beams),
                    io.TargetDeck(*targets[:3]))
    perm = rng.permutation(n)            # perm[lagrangian index] = node
    order = np.argsort(perm).astype(np.int32)  # order[node] = lagrangian index
    ctx = le.Context(0)
    t0 = time.perf_counter()
    ds = DeviceForceSpecs(ctx, sp)
    ctx.synchronize()
    store_s = time.perf_counter() - t0
    order_dev = torch.from_numpy(order).cuda()
    fg = ForceGen(ctx, n, nd)
    ms = []
    for it in range(args.warmup + args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fg.renumber(ds, order_dev)
        e1.record()
        e1.synchronize()
        if it >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    stats = fg.renumber_stats()

    host_s, host_arrays_s = [], []
    fh = None
    for _ in range(args.host_iters):
        fh = None  # the earlier host plan's memory goes back first
        t0 = time.perf_counter()
        a = sp.arrays(perm)
        t1 = time.perf_counter()
        fh = ForceGen(ctx, n, nd, a["springs"], a["beams"], a["targets"])
        ctx.synchronize()
        t2 = time.perf_counter()
        host_arrays_s.append(t1 - t0)
        host_s.append(t2 - t0)
    same = None
    if not args.no_verify and fh is not None:
        same = all(np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint8), y[1].view(np.uint8))
                   for x, y in ((fg.plan(c), fh.plan(c)) for c in range(3)))
    rec = {"spring": 24, "beam": 24 + 8 * nd, "target": 16 + 8 * nd}
    plan = 3 * 8 * (n + 1) + 2 * ns * rec["spring"] + 3 * nb * rec["beam"] + nt * rec["target"]
    r3 = lambda v: round(v, 3)  # noqa: E731
    res = {
        "bench": "forcegen_renumber", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
        "n_side": N, "nodes": n, "springs": ns, "beams": nb, "targets": nt, "iters": args.iters,
        "warmup": args.warmup, "host_iters": args.host_iters, "plan_bytes": plan,
        "plan_bytes_per_node": round(plan / n, 1),
        "device_rebuild_ms": {"min": r3(min(ms)), "median": r3(statistics.median(ms)), "max": r3(max(ms))},
        "device_bytes_held": stats["bytes"], "device_allocations": stats["allocations"],
        "spec_store_upload_s": r3(store_s),
        "host_route_s": ({"min": r3(min(host_s)), "median": r3(statistics.median(host_s)), "max": r3(max(host_s)),
                          "arrays_median": r3(statistics.median(host_arrays_s))} if host_s else "not measured"),
        "plans_equal": same,
    }
    if host_s:
        res["host_over_device"] = round(statistics.median(host_s) * 1e3 / statistics.median(ms), 1)
    print(json.dumps(res))
    out = Path(args.out or ROOT / "profiles" / "forcegen_renumber.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    if same is False:
        sys.exit("bench_forcegen: the rebuilt plan differs from the host plan")


HBM_ACHIEVABLE = 6.29e12  # bytes per second: the streaming copy rate the fractions below are of


def jacobian_bench(args):
    import torch

    from ibamr_amd import build, le
    from ibamr_amd.forcegen import ForceGen, ForceJacobian

    if not torch.cuda.is_available():
        sys.exit("bench_forcegen: no GPU (this measurement has no CPU fallback)")
    N, nd = args.n_side, 3
    n = N * N
    rng = np.random.default_rng(0)
    Xh, springs, beams, targets = sheet(N, rng)
    ns, nb, nt = springs[0].size, beams[0].size, targets[0].size
    ctx = le.Context(0)
    fg = ForceGen(ctx, n, nd, springs=springs, beams=beams, targets=targets)
    X = torch.from_numpy(Xh).cuda()
    dX = torch.zeros_like(X)
    U = torch.randn((n, nd), dtype=torch.float64, device="cuda")
    V = torch.randn((n, nd), dtype=torch.float64, device="cuda")
    F = torch.empty_like(X)
    Y = torch.empty_like(X)
    X_coef, U_coef = 0.5, -0.25 / 1.0e-3

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    J = ForceJacobian(ctx, fg)  # the first build allocates
    build_ms = [timed(J.rebuild) for _ in range(args.warmup + args.iters)][args.warmup:]
    stats = J.stats()
    calls = {
        "compute_dX": lambda: fg.compute(X, U=U, F=F, dX=dX, accumulate=False),
        "linearized": lambda: fg.linearized(X, V, Y=Y, dX=dX, X_coef=X_coef, U_coef=U_coef),
        "assemble": lambda: J.assemble(X, dX=dX, X_coef=X_coef, U_coef=U_coef),
        "apply": lambda: J.apply(V, Y=Y),
    }
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    ctx.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.iters):  # the four alternate, so that they share whatever else the device does
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    # the product against the linearized force, once: two summation orders of the same terms
    Ya = J.apply(V)
    Yl = fg.linearized(X, V, dX=dX, X_coef=X_coef, U_coef=U_coef)
    ctx.synchronize()
    scale = float(Yl.abs().max())
    diff = float((Ya - Yl).abs().max())

    rec = {"spring": 24, "beam": 24 + 8 * nd, "target": 16 + 8 * nd}
    plan = 3 * 8 * (n + 1) + 2 * ns * rec["spring"] + 3 * nb * rec["beam"] + nt * rec["target"]
    vec = n * nd * 8
    blocks, cand = stats["blocks"], stats["candidates"]
    bs = nd * nd * 8
    # bytes the algorithm needs, each array once (neighbour gathers taken as cache hits):
    #   compute(dX) / linearized: the plan, X, dX, U or V, F or Y
    #   assemble: the plan, X, dX, the sorted candidates (an int each), a row and a run start
    #     per block, every block written once (a spring's record is read at both its
    #     off-diagonal blocks and at both its diagonal ones: taken as cache hits too)
    #   apply: rowptr, col, val, V, Y
    alg = {"compute_dX": plan + 4 * vec, "linearized": plan + 4 * vec,
           "assemble": plan + 2 * vec + 4 * cand + (8 + bs) * blocks,
           "apply": 8 * (n + 1) + 4 * blocks + bs * blocks + 2 * vec}
    r4 = lambda v: round(v, 4)  # noqa: E731
    res = {
        "bench": "forcejac_sheet", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
        "n_side": N, "nodes": n, "springs": ns, "beams": nb, "targets": nt, "iters": args.iters,
        "warmup": args.warmup, "blocks": blocks, "blocks_per_node": round(blocks / n, 2), "candidates": cand,
        "device_bytes_held": stats["bytes"], "device_allocations": stats["allocations"],
        "pattern_build_ms": {"median": r4(statistics.median(build_ms)), "min": r4(min(build_ms)),
                             "max": r4(max(build_ms))},
    }
    for k in calls:
        med = statistics.median(ms[k])
        rate = alg[k] / (med * 1e-3)
        res[k] = {"ms": {"median": r4(med), "min": r4(min(ms[k])), "max": r4(max(ms[k]))},
                  "algorithmic_bytes": alg[k], "bytes_per_node": round(alg[k] / n, 1),
                  "algorithmic_GB_per_s": round(rate / 1e9, 1),
                  "fraction_of_6.29_TB_per_s": round(rate / HBM_ACHIEVABLE, 3)}
    res["linearized_over_compute_dX"] = round(statistics.median(ms["linearized"])
                                              / statistics.median(ms["compute_dX"]), 3)
    res["apply_minus_linearized_max"] = diff
    res["linearized_max_abs"] = scale
    print(json.dumps(res))
    out = Path(args.out or ROOT / "profiles" / "forcejac_sheet.json")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-side", type=int, default=3162)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--renumber", action="store_true", help="time the plan rebuild at a renumbering instead")
    ap.add_argument("--host-iters", type=int, default=2, help="--renumber: timed runs of the host route")
    ap.add_argument("--no-verify", action="store_true", help="--renumber: skip the byte comparison of the plans")
    ap.add_argument("--jacobian", action="store_true",
                    help="time the force Jacobian (pattern build, assemble, apply, linearized) beside compute(dX)")
    args = ap.parse_args()
    if args.renumber:
        return renumber_bench(args)
    if args.jacobian:
        return jacobian_bench(args)

    import torch

    from ibamr_amd import build, le
    from ibamr_amd.forcegen import ForceGen

    if not torch.cuda.is_available():
        sys.exit("bench_forcegen: no GPU (this measurement has no CPU fallback)")
    N, nd = args.n_side, 3
    n = N * N
    rng = np.random.default_rng(0)
    Xh, springs, beams, targets = sheet(N, rng)
    ctx = le.Context(0)
    fg = ForceGen(ctx, n, nd, springs=springs, beams=beams, targets=targets)
    ns, nb, nt = springs[0].size, beams[0].size, targets[0].size
    X = torch.from_numpy(Xh).cuda()
    U = torch.randn((n, nd), dtype=torch.float64, device="cuda")
    F = torch.empty_like(X)

    def timed(fn, iters):
        ms = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    run = lambda: fg.compute(X, U=U, F=F, accumulate=False)  # noqa: E731
    for _ in range(args.warmup):
        run()
    ctx.synchronize()
    k_ms = timed(run, args.iters)

    xh = torch.empty((n, nd), dtype=torch.float64, pin_memory=True)
    fh = torch.zeros((n, nd), dtype=torch.float64, pin_memory=True)

    def copies():
        xh.copy_(X, non_blocking=True)
        F.copy_(fh, non_blocking=True)

    for _ in range(args.warmup):
        copies()
    torch.cuda.synchronize()
    c_ms = timed(copies, args.iters)

    # bytes the algorithm needs: the plan once (three offset arrays, a record per incidence),
    # X, U and F once each
    rec = {"spring": 24, "beam": 24 + 8 * nd, "target": 16 + 8 * nd}
    plan = 3 * 8 * (n + 1) + 2 * ns * rec["spring"] + 3 * nb * rec["beam"] + nt * rec["target"]
    alg = plan + 3 * n * nd * 8
    k_med, c_med = statistics.median(k_ms), statistics.median(c_ms)
    res = {
        "bench": "forcegen_sheet", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
        "n_side": N, "nodes": n, "springs": ns, "beams": nb, "targets": nt, "iters": args.iters,
        "warmup": args.warmup,
        "kernel_ms": {"median": round(k_med, 4), "min": round(min(k_ms), 4), "max": round(max(k_ms), 4)},
        "algorithmic_bytes": alg, "bytes_per_node": round(alg / n, 1),
        "algorithmic_GB_per_s": round(alg / (k_med * 1e-3) / 1e9, 1),
        "copy_ms": {"median": round(c_med, 4), "min": round(min(c_ms), 4), "max": round(max(c_ms), 4),
                    "bytes_each_way": n * nd * 8},
        "copies_over_kernel": round(c_med / k_med, 2),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

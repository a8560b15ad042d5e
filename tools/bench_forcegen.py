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

Usage: python tools/bench_forcegen.py [--n-side N] [--iters K] [--warmup W] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-side", type=int, default=3162)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

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

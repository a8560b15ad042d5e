"""Time the device rod stage (ibtk_le_rodgen_compute, ibtk_le_director_update) against the
copies the host route pays.

Workload: --nodes nodes (default 1e7) in closed, twisted rings of --ring nodes (default
1000), one rod from every node to the next of its ring: two plan entries per node.

Reports, on one JSON line (and into --out, default profiles/rods.json):
  * compute_ms: RodForceGen.compute between HIP events on the context stream, after warm-up
    (median, min and max over --iters calls; F = f and N = n, so neither is read);
  * director_ms: director_update (trapezoidal, out of place) likewise;
  * algorithmic bytes per node: compute -- the row offset, the node's two 88-byte records,
    its own X and D once, F and N once (the neighbours' X and D are taken as cache hits);
    director update -- D in, W0 and W1 in, D out;
  * copy_ms: pinned device-to-host copies of X and D plus pinned host-to-device copies of F
    and N, the least a step pays for this stage when the rod loop runs on the host (the
    director rotation's D and W copies not counted).

Usage: python tools/bench_rods.py [--nodes N] [--ring M] [--iters K] [--warmup W] [--out FILE]
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def rings(n, m, torch):
    """X [n][3] and D [n][9] on the device: rings of m nodes, radius 1, the triad's D3 along
    the tangent and D1, D2 turning three times about it per ring; the rings on a line."""
    i = torch.arange(n, dtype=torch.float64, device="cuda")
    j = torch.remainder(i, m)
    ring = torch.floor(i / m)
    th = j * (2.0 * math.pi / m)
    c, s, z, o = torch.cos(th), torch.sin(th), torch.zeros_like(th), torch.ones_like(th)
    X = torch.stack([c + 3.0 * ring, s, z], dim=1)
    nrm, bz, tan = torch.stack([c, s, z], 1), torch.stack([z, z, o], 1), torch.stack([-s, c, z], 1)
    ph = 3.0 * th
    D1 = torch.cos(ph)[:, None] * nrm + torch.sin(ph)[:, None] * bz
    D2 = torch.cross(tan, D1, dim=1)
    return X.contiguous(), torch.cat([D1, D2, tan], dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--ring", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rods.json"))
    args = ap.parse_args()

    import torch

    from ibamr_amd import build, le
    from ibamr_amd.rods import RodForceGen, director_update

    if not torch.cuda.is_available():
        sys.exit("bench_rods: no GPU (this measurement has no CPU fallback)")
    m = args.ring
    n = args.nodes // m * m
    curr = np.arange(n, dtype=np.int32)
    nxt = (curr // m * m + (curr % m + 1) % m).astype(np.int32)
    params = np.empty((n, 10))
    params[:] = [2.0 * math.pi / m, 0.3, 0.3, 0.2, 54.0, 54.0, 54.0, 0.0, 0.0, 0.0]
    ctx = le.Context(0)
    rg = RodForceGen(ctx, n, (curr, nxt, params))
    del params
    X, D = rings(n, m, torch)
    F, N = torch.empty_like(X), torch.empty_like(X)
    W0 = torch.randn((n, 3), dtype=torch.float64, device="cuda")
    W1 = W0 + 0.1 * torch.randn((n, 3), dtype=torch.float64, device="cuda")
    Dn = torch.empty_like(D)

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

    k_ms = timed(lambda: rg.compute(X, D, F=F, N=N, accumulate_F=False, accumulate_N=False))
    d_ms = timed(lambda: director_update(ctx, "trapezoidal", 1e-3, D, W0, W1, out=Dn))
    finite = bool(torch.isfinite(F).all() and torch.isfinite(N).all() and torch.isfinite(Dn).all())

    xh = torch.empty((n, 3), dtype=torch.float64, pin_memory=True)
    dh = torch.empty((n, 9), dtype=torch.float64, pin_memory=True)
    fh = torch.zeros((n, 3), dtype=torch.float64, pin_memory=True)
    nh = torch.zeros((n, 3), dtype=torch.float64, pin_memory=True)

    def copies():
        xh.copy_(X, non_blocking=True)
        dh.copy_(D, non_blocking=True)
        F.copy_(fh, non_blocking=True)
        N.copy_(nh, non_blocking=True)

    c_ms = timed(copies)

    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}  # noqa: E731
    compute_bytes = 8 + 2 * 88 + 24 + 72 + 48
    director_bytes = 72 + 24 + 24 + 72
    k_med, d_med, c_med = statistics.median(k_ms), statistics.median(d_ms), statistics.median(c_ms)
    res = {
        "bench": "rods_rings", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
        "nodes": n, "ring": m, "rods": n, "iters": args.iters, "warmup": args.warmup, "results_finite": finite,
        "compute_ms": stat(k_ms), "compute_bytes_per_node": compute_bytes,
        "compute_GB_per_s": round(compute_bytes * n / (k_med * 1e-3) / 1e9, 1),
        "director_ms": stat(d_ms), "director_bytes_per_node": director_bytes,
        "director_GB_per_s": round(director_bytes * n / (d_med * 1e-3) / 1e9, 1),
        "copy_ms": dict(stat(c_ms), bytes_to_host=n * 96, bytes_to_device=n * 48),
        "copies_over_compute": round(c_med / k_med, 2),
    }
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Time the side-centred curl (ibtk_le_curl_side) against the copies it replaces and
against a device copy of the same arrays.

Workload: per size N (default 512 and 1024) a periodic unit cube of N^3 cells, ghost width
3, pitched and aligned side arrays (Geometry.aligned()); ``curl_side(u -> w, alpha=0.5,
periodic)`` -- the call of gib.interp_angular_velocity -- between HIP events, --warmup
calls and then --iters timed ones (median, min, max).

In the same process, per size:
  (a) host_copy_ms: the three u arrays device-to-host and three arrays host-to-device into
      w through pinned memory -- what a step pays for this stage when the curl runs on the
      host.  One pinned buffer of one array's size is reused for the six transfers (the
      bytes and the direction of every transfer are those of the real route; 52 GB of
      pinned memory at 1024^3 are not needed to time it).  --copy-iters timed rounds.
  (b) device_copy_ms: the three u allocations copied into the three w allocations on the
      device: the floor of "every value read once and written once".
and the ratios host_copy / curl and curl / device_copy, next to the tile's halo factor
(TX+2)(TY+2)/(TX TY) from gib.CURL_TILE, which applies to the read half of the traffic:
halo_adjusted_copy = (halo + 1) / 2 device copies.

One JSON line on stdout and --out (default profiles/curl.json).

Usage: python tools/bench_curl.py [--sizes 512,1024] [--iters K] [--warmup W] [--copy-iters C] [--out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def span(torch, t):
    size = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    return torch.as_strided(t, (size,), (1,))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copy-iters", type=int, default=5)
    ap.add_argument("--ghost", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "curl.json"))
    args = ap.parse_args()

    import torch

    from ibamr_amd import build, gib, le

    if not torch.cuda.is_available():
        sys.exit("bench_curl: no GPU (this measurement has no CPU fallback)")
    ctx = le.Context(0)
    TX, TY, TZ = gib.CURL_TILE
    halo = (TX + 2) * (TY + 2) / (TX * TY)
    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}  # noqa: E731

    def timed(fn, warmup, iters):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    sizes = []
    for N in (int(v) for v in args.sizes.split(",")):
        geom = le.Geometry.periodic_unit([N, N, N], args.ghost).aligned()
        u, w = geom.alloc("side"), geom.alloc("side")
        us, ws = [span(torch, t) for t in u], [span(torch, t) for t in w]
        for s in us:
            s.normal_()
        per = (1, 1, 1)
        k_ms = timed(lambda: gib.curl_side(ctx, geom, u, geom, w, alpha=0.5, periodic=per), args.warmup, args.iters)
        inner = tuple(slice(args.ghost, args.ghost + N) for _ in range(3))
        finite = all(bool(torch.isfinite(t[inner]).all()) for t in w)

        def device_copy():
            for a, b in zip(us, ws):
                b.copy_(a)

        d_ms = timed(device_copy, args.warmup, args.iters)
        host = torch.empty(max(s.numel() for s in us), dtype=torch.float64, pin_memory=True)

        def host_copy():
            for s in us:
                host[:s.numel()].copy_(s, non_blocking=True)
            for s in ws:
                s.copy_(host[:s.numel()], non_blocking=True)

        h_ms = timed(host_copy, 1, args.copy_iters)
        k_med, d_med, h_med = (statistics.median(v) for v in (k_ms, d_ms, h_ms))
        points = 3 * N * N * (N + 1)
        alloc_bytes = 8 * sum(s.numel() for s in us)
        sizes.append({
            "N": N, "ghost": args.ghost, "pitch": list(geom.pitch), "results_finite": finite,
            "curl_ms": stat(k_ms), "algorithmic_bytes": 16 * points,
            "curl_GB_per_s": round(16 * points / (k_med * 1e-3) / 1e9, 1),
            "device_copy_ms": dict(stat(d_ms), bytes_read=alloc_bytes, bytes_written=alloc_bytes),
            "host_copy_ms": dict(stat(h_ms), iters=args.copy_iters, bytes_to_host=alloc_bytes, bytes_to_device=alloc_bytes),
            "host_copy_over_curl": round(h_med / k_med, 2),
            "curl_over_device_copy": round(k_med / d_med, 3),
            "halo_adjusted_copy_ms": round(d_med * (halo + 1.0) / 2.0, 4),
            "curl_over_halo_adjusted_copy": round(k_med / (d_med * (halo + 1.0) / 2.0), 3),
            "device_copy_spread_ms": round(max(d_ms) - min(d_ms), 4),
        })
        del u, w, us, ws, host
        torch.cuda.empty_cache()
    res = {"bench": "curl_side", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
           "iters": args.iters, "warmup": args.warmup, "alpha": 0.5, "periodic": [1, 1, 1],
           "curl_tile": [TX, TY, TZ], "halo_factor_reads": round(halo, 4), "sizes": sizes}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Nearest-centre assignment (FlatIndex.assign), cluster sums and one k-means step, timed on one GPU. HIP events around each whole
call (host hand-over included), CUDA inputs and outputs, median of REPS calls after WARM warm-up calls. No pass / fail gate.
  A  1M x 512 random rows, f16 and fp8: assign at C = 16, 64, 256, 1024 with and without distances; the borderline share
     (borderline rows / rows, from guard_stats); membership at P = min(C, 64) in the same process (the parent's code) and that
     time multiplied by the assign call's pass count.
  B  rows and centres at pairwise cosine 0.99 (what an encoder's embeddings look like): C = 16 and 64; most rows are borderline
     and the canonical resolve dominates.
  C  cluster_sums at C = 16 and 256 against one threshold scan over the same rows (query_radius of one query with a radius no
     row reaches).
  D  one k-means step (assign without distances from host centres, cluster_sums, the centre update on the host) at 100k x 512,
     C = 256: wall clock.
Writes the tables to --out (default: stdout only) and prints them."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mmiss_amd  # noqa: F401,E402
from mmiss_amd.index import FlatIndex  # noqa: E402

D = 512
WARM, REPS = 2, 15


def timed(fn, reps=REPS):
    for _ in range(WARM):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def fill(idx, n, make):
    for r0 in range(0, n, 250_000):
        m = min(250_000, n - r0)
        idx.add(make(m), np.arange(r0, r0 + m, dtype=np.int64))


def borderline_rows(idx, c):
    s0 = idx.guard_stats()
    idx.assign(c, want_dist=False)
    s1 = idx.guard_stats()
    return (s1["swept_rows"] - s0["swept_rows"]) / int(c.shape[0]), s1["radius_pages"] - s0["radius_pages"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--parts", default="ABCD")
    args = ap.parse_args()
    n = args.rows
    lines, out = [], []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(4)
    for dtype in ("f16", "f8"):
        if not set("ABC") & set(args.parts):
            break
        idx = FlatIndex(D, dtype, capacity=n)
        fill(idx, n, lambda m: torch.randn(m, D, device="cuda", generator=g))
        if "A" in args.parts:
            say(f"A  assign over {n} x {D} random rows, {dtype}; median of {REPS}")
            say("   C   passes   assign+dist ms   assign ms   borderline share   | membership(P = min(C, 64)) ms   x passes")
            for C in (16, 64, 256, 1024):
                c = torch.randn(C, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
                brows, passes = borderline_rows(idx, c)
                ms_d = timed(lambda: idx.assign(c, want_dist=True))
                ms = timed(lambda: idx.assign(c, want_dist=False))
                P = min(C, 64)
                mem = timed(lambda: idx.membership(c[:P], 0.98))
                out.append({"part": "A", "dtype": dtype, "C": C, "passes": passes, "assign_dist_ms": round(ms_d, 4), "assign_ms": round(ms, 4),
                            "borderline_share": brows / n, "membership_ms": round(mem, 4), "membership_x_passes_ms": round(mem * passes, 4)})
                say(f"{C:5d}   {passes:6d}   {ms_d:14.3f}   {ms:9.3f}   {brows / n:16.5f}   | {mem:29.3f}   {mem * passes:8.3f}")
        if "C" in args.parts:
            say(f"C  cluster_sums over {n} x {D} random rows, {dtype}; median of {REPS}")
            q1 = torch.randn(1, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
            scan = timed(lambda: idx.query_radius(q1, -1.0, 1))
            for C in (16, 256):
                a = torch.randint(0, C, (n,), device="cuda", dtype=torch.int32, generator=torch.Generator(device="cuda").manual_seed(7))
                ms = timed(lambda: idx.cluster_sums(a, C))
                out.append({"part": "C", "dtype": dtype, "C": C, "cluster_sums_ms": round(ms, 4), "threshold_scan_ms": round(scan, 4)})
                say(f"   C = {C:4d}   cluster_sums {ms:8.3f} ms   | one threshold scan {scan:.3f} ms")
        idx.close()
    if "B" in args.parts:
        # pairwise cosine 0.99: u + noise with |noise|^2 = 1 / 99 of |u|^2 per vector
        u = torch.randn(1, D, device="cuda", generator=g)
        u = u / u.norm()
        sigma = float(np.sqrt((1 / 0.99 - 1) / D))
        for dtype in ("f16", "f8"):
            idx = FlatIndex(D, dtype, capacity=n)
            fill(idx, n, lambda m: u + sigma * torch.randn(m, D, device="cuda", generator=g))
            say(f"B  assign over {n} x {D} rows at pairwise cosine 0.99, {dtype}; median of 5")
            for C in (16, 64):
                c = u + sigma * torch.randn(C, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
                brows, passes = borderline_rows(idx, c)
                ms_d = timed(lambda: idx.assign(c, want_dist=True), reps=5)
                out.append({"part": "B", "dtype": dtype, "C": C, "assign_dist_ms": round(ms_d, 4), "borderline_share": brows / n})
                say(f"   C = {C:4d}   assign+dist {ms_d:9.3f} ms   borderline share {brows / n:.5f}")
            idx.close()
    if "D" in args.parts:
        nk, C = 100_000, 256
        for dtype in ("f16", "f8"):
            idx = FlatIndex(D, dtype, capacity=nk)
            fill(idx, nk, lambda m: torch.randn(m, D, device="cuda", generator=g))
            centres = idx.get(np.arange(C, dtype=np.int64) * (nk // C))
            walls = []
            for _ in range(7):
                t0 = time.perf_counter()
                asg, _d, _s = idx.assign(centres, want_dist=False)
                sums, sizes = idx.cluster_sums(asg, C)
                new = (sums.astype(np.float64) * 2.0 ** -32).astype(np.float32)
                keep = (sizes == 0) | ~sums.any(axis=1)
                new[keep] = centres[keep]
                walls.append((time.perf_counter() - t0) * 1e3)
                centres = new
            out.append({"part": "D", "dtype": dtype, "kmeans_step_ms": round(float(np.median(walls[2:])), 4)})
            say(f"D  one k-means step at {nk} x {D}, C = {C}, {dtype}: {np.median(walls[2:]):.3f} ms wall (median of 5 after 2)")
            idx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"assign_bench": out}))


if __name__ == "__main__":
    main()

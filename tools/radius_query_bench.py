#!/usr/bin/env python3
"""Radius queries against the closest existing cost: over 1M x 512 random rows (f16 and fp8 storage) at Q = 1, 16, 64, 256,
HIP events around each whole call (host hand-over included), median of REPS calls after WARM warm-up calls:
  query_radius(r = 0.3, cap = 100)   one threshold pass + re-rank
  query(k = 10), guard_force = 1     first pass + one threshold pass + re-rank: every query widened, the top-k call that does
                                     one pass more (what a top-k query on an index of one encoder's own embeddings costs)
  query(k = 10)                      the ordinary call on these rows (nothing widens), for scale
Then near_duplicates(0.02) over 100 000 x 512 f16 rows that share a direction (pairwise cosine about 0.9, as one encoder's
embeddings do) with PAIRS planted near copies: total time and pairs found. Prints one table row per case and one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mmiss_amd  # noqa: F401,E402
from mmiss_amd import _lib  # noqa: E402
from mmiss_amd.index import FlatIndex  # noqa: E402

N, D = 1_000_000, 512
N_DUP, PAIRS = 100_000, 2000
WARM, REPS = 3, 15


def timed(fn):
    for _ in range(WARM):
        fn()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def main():
    out = []
    for dtype in ("f16", "f8"):
        idx = FlatIndex(D, dtype, capacity=N)
        g = torch.Generator(device="cuda").manual_seed(4)
        for r0 in range(0, N, 250_000):
            idx.add(torch.randn(250_000, D, device="cuda", generator=g), np.arange(r0, r0 + 250_000, dtype=np.int64))
        for Q in (1, 16, 64, 256):
            q = torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
            radius = timed(lambda: idx.query_radius(q, 0.3, 100))
            plain = timed(lambda: idx.query(q, 10))
            _lib.set_option("guard_force", 1)
            try:
                forced = timed(lambda: idx.query(q, 10))
            finally:
                _lib.set_option("guard_force", 0)
            plan = _lib.index_radius_plan(idx._h, Q)["first"]
            row = {"dtype": dtype, "Q": Q, "radius_ms": round(radius, 4), "forced_topk_ms": round(forced, 4), "topk_ms": round(plain, 4),
                   "radius_vs_forced": round(radius / forced, 3), "route": "gemm" if plan["gemm"] else f"scan x{plan['qtiles']}"}
            out.append(row)
            print(f"{dtype:3s} Q={Q:3d}  radius {radius:7.3f} ms  forced top-k {forced:7.3f} ms  x{radius / forced:5.3f}  "
                  f"top-k {plain:7.3f} ms  ({row['route']})", flush=True)
        idx.close()
    # near duplicates
    g = torch.Generator(device="cuda").manual_seed(6)
    common = torch.randn(1, D, device="cuda", generator=g)
    rows = 3.0 * common + torch.randn(N_DUP, D, device="cuda", generator=g)          # pairwise cosine 0.9
    src = torch.randperm(N_DUP, device="cuda", generator=g)[:2 * PAIRS]
    rows[src[PAIRS:]] = rows[src[:PAIRS]] + 0.05 * torch.randn(PAIRS, D, device="cuda", generator=g)
    idx = FlatIndex(D, "f16", capacity=N_DUP)
    idx.add(rows, np.arange(N_DUP, dtype=np.int64))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a, b, d, overflow = idx.near_duplicates(0.02)
    dt = time.perf_counter() - t0
    dup = {"rows": N_DUP, "planted_pairs": PAIRS, "pairs_found": int(a.size), "seconds": round(dt, 3), "overflow_rows": len(overflow),
           "guard": idx.guard_stats()}
    print(f"near_duplicates(0.02) over {N_DUP} x {D} f16: {a.size} pairs in {dt:.3f} s", flush=True)
    idx.close()
    print(json.dumps({"radius_query_bench": out, "near_duplicates": dup}))


if __name__ == "__main__":
    main()

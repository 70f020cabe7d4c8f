#!/usr/bin/env python3
"""Filtered queries on the streaming scan: cosine top-10 over 10M x 512 f16 rows at Q = 1 and Q = 16, HIP events around each
query call (widen pass and host hand-over included), median of REPS calls after WARM warm-up calls:
  unfiltered (mmiss_index_query), and filtered (mmiss_index_query_filtered) with admitted fractions
  1.0 (require = 0), 0.1 and 0.01 of the rows at random, 0.01 as contiguous runs of RUN rows (uploads that share attributes).
Prints one table row per (case, Q): ms per call, the call time relative to the unfiltered one, and the effective bandwidth
over the bytes of the ADMITTED rows (rows x 512 x 2 B). One JSON line at the end holds the same numbers."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mmiss_amd  # noqa: F401,E402
from mmiss_amd.index import FlatIndex  # noqa: E402

N, D, K = 10_000_000, 512, 10
RUN = 4096
WARM, REPS = 3, 15
BIT_R10, BIT_R1, BIT_RUN = 1, 2, 4


def main():
    idx = FlatIndex(D, "f16", capacity=N)
    g = torch.Generator(device="cuda").manual_seed(4)
    for r0 in range(0, N, 1_000_000):
        idx.add(torch.randn(1_000_000, D, device="cuda", generator=g), np.arange(r0, r0 + 1_000_000, dtype=np.int64))
    rng = np.random.Generator(np.random.Philox(11))
    tags = np.zeros(N, np.uint64)
    tags[rng.random(N) < 0.1] |= np.uint64(BIT_R10)
    tags[rng.random(N) < 0.01] |= np.uint64(BIT_R1)
    nruns = N // 100 // RUN                                   # 1 % of the rows in runs of RUN consecutive rows
    starts = rng.choice(N // RUN, size=nruns, replace=False) * RUN
    for s in starts:
        tags[s:s + RUN] |= np.uint64(BIT_RUN)
    idx.set_tags(np.arange(N, dtype=np.int64), tags)
    cases = [("unfiltered", None), ("filtered 1.0", 0), ("filtered 0.1 random", BIT_R10), ("filtered 0.01 random", BIT_R1),
             ("filtered 0.01 contiguous", BIT_RUN)]
    out = []
    for Q in (1, 16):
        q = torch.randn(Q, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        base = None
        for name, req in cases:
            adm = N if not req else int(((tags & np.uint64(req)) != 0).sum())
            kw = {} if req is None else {"require": req}
            for _ in range(WARM):
                idx.query(q, K, **kw)
            times = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                idx.query(q, K, **kw)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            ms = float(np.median(times))
            base = ms if req is None else base
            row = {"case": name, "Q": Q, "admitted": adm, "ms": round(ms, 4), "vs_unfiltered": round(ms / base, 3),
                   "admitted_GBps": round(adm * D * 2 / (ms * 1e-3) / 1e9, 1)}
            out.append(row)
            print(f"{name:26s} Q={Q:2d}  admitted {adm:9d}  {ms:8.3f} ms  x{ms / base:5.3f}  {row['admitted_GBps']:8.1f} GB/s", flush=True)
    print(json.dumps({"filtered_query_bench": out, "guard": idx.guard_stats()}))
    idx.close()


if __name__ == "__main__":
    main()

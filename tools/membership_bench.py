#!/usr/bin/env python3
"""Dense membership (FlatIndex.membership) over 1M x 512 random rows, f16 and fp8 storage, P = 1, 16, 64 probes at a radius that
makes about a third of the rows members (0.98 on these rows: distances are 1 +- 0.044). HIP events around each whole call (host
hand-over included), median of REPS calls after WARM warm-up calls. Per case: ms, the rows' bytes / time, the share of (row,
probe) pairs that were borderline and resolved canonically, the probes that overflowed into the per-probe canonical pass, the
passes over the index. For context, on the same index: a radius call (query_radius) of the same queries with a radius no row
reaches (-1): its one threshold pass collects nothing, so the time is the scan's (its code is not touched by the membership
calls). tag_by_radius at P = 16 shows what the merge into the tags and the copy of the tags to the host mirror add.
There is no pass / fail gate on these times. Writes the table to --out (default profiles/membership.txt) and prints it."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mmiss_amd  # noqa: F401,E402
from mmiss_amd.index import FlatIndex  # noqa: E402

N, D = 1_000_000, 512
RADIUS = 0.98
WARM, REPS = 2, 9


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "membership.txt"))
    ap.add_argument("--rows", type=int, default=N)
    args = ap.parse_args()
    n = args.rows
    lines = [f"membership over {n} x {D} random rows, radius {RADIUS}; median of {REPS} calls (HIP events around the whole call)",
             "dtype   P   member ms   rows GB/s   members/probe   borderline share   overflowed   passes   | radius(-1) scan ms   rows GB/s"]
    out = []
    for dtype, elt in (("f16", 2), ("f8", 1)):
        idx = FlatIndex(D, dtype, capacity=n)
        g = torch.Generator(device="cuda").manual_seed(4)
        for r0 in range(0, n, 250_000):
            m = min(250_000, n - r0)
            idx.add(torch.randn(m, D, device="cuda", generator=g), np.arange(r0, r0 + m, dtype=np.int64))
        gbytes = n * D * elt / 1e9
        for P in (1, 16, 64):
            q = torch.randn(P, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
            s0 = idx.guard_stats()
            words, members = idx.membership(q, RADIUS)
            s1 = idx.guard_stats()
            ms = timed(lambda: idx.membership(q, RADIUS))
            scan_ms = timed(lambda: idx.query_radius(q, -1.0, 1))
            row = {"dtype": dtype, "P": P, "membership_ms": round(ms, 4), "rows_GBps": round(gbytes / (ms * 1e-3), 1),
                   "members_per_probe": float(members.double().mean()), "borderline_share": (s1["swept_rows"] - s0["swept_rows"]) / (n * P),
                   "overflowed_probes": s1["exhaustive"] - s0["exhaustive"], "passes": s1["radius_pages"] - s0["radius_pages"],
                   "radius_unreachable_ms": round(scan_ms, 4), "radius_rows_GBps": round(gbytes / (scan_ms * 1e-3), 1)}
            if P == 16:
                row["tag_by_radius_ms"] = round(timed(lambda: idx.tag_by_radius(q, RADIUS, list(range(16)))), 4)
            out.append(row)
            lines.append(f"{dtype:5s} {P:3d}   {ms:9.3f}   {row['rows_GBps']:9.1f}   {row['members_per_probe']:13.0f}   "
                         f"{row['borderline_share']:16.5f}   {row['overflowed_probes']:10d}   {row['passes']:6d}   | "
                         f"{scan_ms:18.3f}   {row['radius_rows_GBps']:9.1f}" + (f"   (tag_by_radius {row['tag_by_radius_ms']:.3f} ms)" if P == 16 else ""))
            print(lines[-1], flush=True)
        idx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(json.dumps({"membership_bench": out}))


if __name__ == "__main__":
    main()

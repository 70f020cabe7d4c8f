#!/usr/bin/env python3
"""Grouped search (FlatIndex.query_grouped) beside the flat query (FlatIndex.query, the parent commit's code, unchanged) on the same
index in the same process, timed on one GPU. No pass / fail gate.

Corpus: random rows, dim 512; --rows N rows (default: 1M and 10M), f16 and fp8, k = 10, Q = 1 / 16 / 256; HIP events around each
whole call (host hand-over included), CUDA inputs and outputs, median of 15 calls after 2 warm-up calls, the two calls of a pair
alternating. Three tables per index:
  1. the walk route: random group ids below 1000 on every row; beside it the flat query at k = pool (the default pool, 80): the
     grouped call's own list stage. The difference is the walk stage (one launch and the host's look at the flags);
  2. the exhaustive route, forced: one more group owns the nearest 2040 rows of every query of the batch (of the first Q queries,
     when Q of them are timed), so no list of any pool holds a second head; beside it the flat query at k = 10;
  3. per-kernel times from mmiss_prof for one call per route and Q: the list stage's kernels together, grouped_walk, the table
     fill is not a kernel (a memset on the stream) and is not listed, grouped_scan, segment_topk, grouped_resolve.
Writes the tables to --out (default: stdout only) and prints them."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mmiss_amd  # noqa: F401,E402
from mmiss_amd import _lib  # noqa: E402
from mmiss_amd.index import FlatIndex  # noqa: E402

D, K, GROUPS, CROWD = 512, 10, 1000, 2040
WARM, REPS = 2, 15
QS = (1, 16, 256)


def timed_pair(fa, fb, reps=REPS):
    """(median, min, max) in ms of fa and of fb, called alternately"""
    for _ in range(WARM):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        for fn, out in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
    return tuple((float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in (ta, tb))


def kernel_table(fn):
    """{kernel: ms} of one call under mmiss_prof"""
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        recs = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    out = {}
    for r in recs:
        out[r["kernel"]] = out.get(r["kernel"], 0.0) + float(r["ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--dtypes", default="f16,f8")
    args = ap.parse_args()
    sizes = [args.rows] if args.rows else [1_000_000, 10_000_000]
    lines, out = [], []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(6)
    queries = torch.randn(max(QS), D, device="cuda", generator=g)
    rng = np.random.Generator(np.random.Philox(6))
    say(f"corpus: random rows, dim {D}; k = {K}; median (min .. max) of {REPS} after {WARM}, the two calls of a pair alternating; "
        "CUDA inputs and outputs, whole calls")
    for n in sizes:
        labels = np.arange(n, dtype=np.int64)
        for dtype in args.dtypes.split(","):
            idx = FlatIndex(D, dtype, capacity=n)
            for r0 in range(0, n, 250_000):
                m = min(250_000, n - r0)
                idx.add(torch.randn(m, D, device="cuda", generator=g), labels[r0:r0 + m])
            torch.cuda.synchronize()
            say(f"{n} x {D} {dtype}")
            groups = rng.integers(0, GROUPS, n).astype(np.int32)
            idx.set_groups(labels, groups)
            pool = _lib.index_grouped_plan(idx._h, 1, K)["pool"]
            say(f"   1. walk route: {GROUPS} random groups, pool {pool}")
            say("        Q   grouped ms (min .. max)      flat k=pool ms (min .. max)    grouped - flat")
            for Q in QS:
                q = queries[:Q].contiguous()
                route = idx.query_grouped(q, K)[4]
                assert int(route.sum()) == 0, "the walk route was meant"
                (gm, g0, g1), (fm, f0, f1) = timed_pair(lambda: idx.query_grouped(q, K), lambda: idx.query(q, pool))
                out.append({"rows": n, "dtype": dtype, "route": 0, "Q": Q, "grouped_ms": round(gm, 4), "flat_pool_ms": round(fm, 4)})
                say(f"     {Q:4d}   {gm:8.3f} ({g0:.3f} .. {g1:.3f})   {fm:8.3f} ({f0:.3f} .. {f1:.3f})   {gm - fm:10.3f}")
            tabs = {(0, Q): kernel_table(lambda: idx.query_grouped(queries[:Q].contiguous(), K)) for Q in QS}
            # one more group owns the nearest CROWD rows of every query timed so far
            say(f"   2. exhaustive route: group {GROUPS} owns the nearest {CROWD} rows of each of the Q queries")
            say("        Q   grouped ms (min .. max)      flat k=10 ms (min .. max)    grouped / flat   chunks   rows of the group")
            for Q in QS:
                q = queries[:Q].contiguous()
                near = idx.query(q, CROWD)[0].reshape(-1)
                near = torch.unique(near[near >= 0]).cpu().numpy()
                idx.set_groups(near, np.full(near.size, GROUPS, np.int32))
                owned = int((idx.get_groups(labels) == GROUPS).sum())
                route = idx.query_grouped(q, K)[4]
                assert int(route.sum()) == Q, "the exhaustive route was meant"
                plan = _lib.index_grouped_plan(idx._h, Q, K)
                (gm, g0, g1), (fm, f0, f1) = timed_pair(lambda: idx.query_grouped(q, K), lambda: idx.query(q, K))
                out.append({"rows": n, "dtype": dtype, "route": 1, "Q": Q, "grouped_ms": round(gm, 4), "flat_ms": round(fm, 4),
                            "chunks": plan["chunks"], "query_block": plan["first_chunk_block"]})
                say(f"     {Q:4d}   {gm:8.3f} ({g0:.3f} .. {g1:.3f})   {fm:8.3f} ({f0:.3f} .. {f1:.3f})   {gm / fm:14.2f}   {plan['chunks']:6d}   {owned:9d}")
                tabs[(1, Q)] = kernel_table(lambda: idx.query_grouped(q, K))
            say("   3. kernels of one call (mmiss_prof, ms)")
            say("    route      Q   list stage   grouped_walk   grouped_scan   segment_topk   grouped_resolve")
            for (route, Q), tab in sorted(tabs.items()):
                scan = sum(v for name, v in tab.items() if name.startswith("grouped_scan"))
                own = scan + tab.get("grouped_walk", 0.0) + tab.get("grouped_resolve", 0.0) + tab.get("segment_topk", 0.0)
                listed = sum(tab.values()) - own
                out.append({"rows": n, "dtype": dtype, "route": route, "Q": Q, "list_ms": round(listed, 4), "walk_ms": round(tab.get("grouped_walk", 0.0), 4),
                            "scan_ms": round(scan, 4), "select_ms": round(tab.get("segment_topk", 0.0), 4),
                            "resolve_ms": round(tab.get("grouped_resolve", 0.0), 4)})
                say(f"    {route:5d}   {Q:4d}   {listed:10.3f}   {tab.get('grouped_walk', 0.0):12.3f}   {scan:12.3f}   {tab.get('segment_topk', 0.0):12.3f}"
                    f"   {tab.get('grouped_resolve', 0.0):15.3f}")
            idx.close()
            del idx
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"grouped_bench": out}))


if __name__ == "__main__":
    main()

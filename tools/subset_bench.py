#!/usr/bin/env python3
"""Subset search (FlatIndex.query_subset) beside the flat query (FlatIndex.query, the parent commit's code, unchanged) on the same
index in the same process, timed on one GPU. No pass / fail gate; the one expectation the feature came with is printed as a line of
its own: on 10M x 512 f16, a list of 1 % of the rows, Q = 1, the subset call should take less time than the flat one.

Corpus: random rows (the subset call's cost does not depend on where the rows lie); lists: random distinct rows, shuffled, as a CUDA
tensor. --rows N rows (default: 1M and 10M), f16 and fp8, k = 10. Lists of 0.1 % / 1 % / 10 % / 50 % of the rows, Q = 1 / 16 / 256:
HIP events around each whole call (host hand-over included), CUDA inputs and outputs, median of 15 calls after 2 warm-up calls, the
flat query at the same Q timed in the same loop, the two alternating. Per-kernel times from mmiss_prof for one call per list at
Q = 1 and at Q = 16: stages 1 + 2 (subset_mark + subset_compact: the list becomes ascending rows), the scan, the selection — and
the scan's time at Q = 16 over Q = 1: about 1 when the rows are read once per query block, about 16 when once per query.
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

D, K = 512, 10
WARM, REPS = 2, 15
QS, SHARES = (1, 16, 256), (0.001, 0.01, 0.1, 0.5)


def timed_pair(fa, fb, reps=REPS):
    """medians (ms) of fa and fb, called alternately"""
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
    return float(np.median(ta)), float(np.median(tb))


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
    say(f"corpus: random rows, dim {D}; k = {K}; lists: random distinct rows, shuffled, on the device; median of {REPS} after {WARM}, "
        "flat and subset calls alternating")
    for n in sizes:
        for dtype in args.dtypes.split(","):
            idx = FlatIndex(D, dtype, capacity=n)
            for r0 in range(0, n, 250_000):
                m = min(250_000, n - r0)
                idx.add(torch.randn(m, D, device="cuda", generator=g), np.arange(r0, r0 + m, dtype=np.int64))
            torch.cuda.synchronize()
            say(f"{n} x {D} {dtype}")
            say("   list share   list rows      Q   subset ms    flat ms   flat / subset")
            lists = {}
            for share in SHARES:
                m = max(1, int(round(n * share)))
                lists[share] = torch.randperm(n, device="cuda", generator=g)[:m].contiguous()
            for share in SHARES:
                cand = lists[share]
                for Q in QS:
                    q = queries[:Q].contiguous()
                    plan = _lib.index_subset_plan(idx._h, Q, K, int(cand.shape[0]))
                    sub_ms, flat_ms = timed_pair(lambda: idx.query_subset(q, K, cand), lambda: idx.query(q, K))
                    out.append({"rows": n, "dtype": dtype, "share": share, "list": int(cand.shape[0]), "Q": Q, "subset_ms": round(sub_ms, 4),
                                "flat_ms": round(flat_ms, 4), "ratio": round(flat_ms / sub_ms, 3), "chunks": plan["chunks"],
                                "query_block": plan["query_block"]})
                    say(f"   {share:10.3f}   {cand.shape[0]:9d}   {Q:4d}   {sub_ms:9.3f}   {flat_ms:8.3f}   {flat_ms / sub_ms:13.2f}"
                        + (f"   ({plan['chunks']} chunks)" if plan["chunks"] > 1 else ""))
                    if n == 10_000_000 and dtype == "f16" and Q == 1 and share == 0.01:
                        say(f"EXPECTATION (10M x 512 f16, 1 % list, Q = 1): subset {sub_ms:.3f} ms, flat {flat_ms:.3f} ms: "
                            + ("HOLDS" if sub_ms < flat_ms else "DOES NOT HOLD"))
            say("   kernels of one call (mmiss_prof, ms): stages 1 + 2 = subset_mark + subset_compact")
            say("   list share      Q   stages 1+2       scan   selection   prep_queries   scan Q=16 / Q=1")
            for share in SHARES:
                cand = lists[share]
                scan1 = None
                for Q in (1, 16):
                    q = queries[:Q].contiguous()
                    tab = kernel_table(lambda: idx.query_subset(q, K, cand))
                    front = tab.get("subset_mark", 0.0) + tab.get("subset_compact", 0.0)
                    scan = sum(v for k, v in tab.items() if k.startswith("subset_scan"))
                    if Q == 1:
                        scan1 = scan
                    out.append({"rows": n, "dtype": dtype, "share": share, "Q": Q, "front_ms": round(front, 4), "scan_ms": round(scan, 4),
                                "select_ms": round(tab.get("segment_topk", 0.0), 4)})
                    say(f"   {share:10.3f}   {Q:4d}   {front:10.3f}   {scan:8.3f}   {tab.get('segment_topk', 0.0):9.3f}   {tab.get('prep_queries', 0.0):12.3f}"
                        + (f"   {scan / scan1:15.2f}" if Q == 16 and scan1 else ""))
            idx.close()
            del idx
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"subset_bench": out}))


if __name__ == "__main__":
    main()

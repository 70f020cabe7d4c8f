#!/usr/bin/env python3
"""Partitioned search (FlatIndex.build_partition / query_probed) beside the flat query (FlatIndex.query, the parent commit's code,
unchanged) on the same index in the same process, timed on one GPU. No pass / fail gate; the one condition the feature has to meet
is printed as a line of its own: on 10M x 512 f16, C = 1024, nprobe = 32, Q = 1 the probed call must take less time than the flat.

Corpus: BLOBS = 4096 random unit directions u_b; row = u_b + sigma / sqrt(512) * N(0, I) with b uniform: the noise has norm sigma
against the centre's 1, so the pairwise cosine is about 1 / (1 + sigma^2) inside a blob and about 0 across. --sigma 2.0 (default:
cosine 0.2 inside a blob, so a query's ten nearest rows are spread over several cells and recall depends on nprobe) or e.g. 0.6
(cosine 0.74: a blob lies inside one cell and one probe finds everything). Queries are fresh draws of the same law.
--rows N rows (default: 1M and 10M), f16 and fp8. Partition: build_partition(1024) (k-means, 10 iterations at the most), its wall
time. Then query_probed at Q = 1 / 16 / 256 and nprobe = 1 / 8 / 32 / 128 and query at the same Q: HIP events around each whole call
(host hand-over included), CUDA inputs and outputs, median of 15 calls after 2 warm-up calls, k = 10. Scanned share = scanned rows /
rows (mean over the queries); recall@10 = the share of query()'s ten labels that query_probed returns (mean over the 256 queries).
Per-kernel times from mmiss_prof for one call at Q = 1, nprobe = 32 and one at Q = 256, nprobe = 32.
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
from mmiss_amd import _lib  # noqa: E402
from mmiss_amd.index import FlatIndex  # noqa: E402

D, K, CELLS = 512, 10, 1024
BLOBS = 4096
WARM, REPS = 2, 15
QS, NPROBES = (1, 16, 256), (1, 8, 32, 128)


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


def kernel_table(fn):
    """[(kernel, launches, ms)] of one call under mmiss_prof"""
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        recs = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    return [(r["kernel"], int(r["launches"]), float(r["ms"])) for r in recs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--dtypes", default="f16,f8")
    ap.add_argument("--sigma", type=float, default=2.0)
    args = ap.parse_args()
    sizes = [args.rows] if args.rows else [1_000_000, 10_000_000]
    lines, out = [], []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(4)
    u = torch.randn(BLOBS, D, device="cuda", generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    sigma = args.sigma / np.sqrt(D)

    def draw(m):
        b = torch.randint(0, BLOBS, (m,), device="cuda", generator=g)
        return u[b] + sigma * torch.randn(m, D, device="cuda", generator=g)

    queries = draw(max(QS))
    say(f"corpus: {BLOBS} unit directions + {args.sigma} / sqrt({D}) * N(0, I); k = {K}; C = {CELLS}; median of {REPS} after {WARM}")
    for n in sizes:
        for dtype in args.dtypes.split(","):
            idx = FlatIndex(D, dtype, capacity=n)
            for r0 in range(0, n, 250_000):
                m = min(250_000, n - r0)
                idx.add(draw(m), np.arange(r0, r0 + m, dtype=np.int64))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = idx.build_partition(CELLS)
            build_s = time.perf_counter() - t0
            say(f"{n} x {D} {dtype}: build_partition({CELLS}) {build_s:.2f} s wall; largest cell {info['largest_cell']}, "
                f"empty cells {info['empty_cells']}, rows in cells {info['rows_in_cells']}")
            flat_ms, flat_lab = {}, None
            for Q in QS:
                q = queries[:Q].contiguous()
                flat_ms[Q] = timed(lambda: idx.query(q, K))
                if Q == max(QS):
                    flat_lab = idx.query(q, K)[0].cpu().numpy()
            say("     Q   nprobe   probed ms    flat ms   flat / probed   scanned share   recall@10")
            for Q in QS:
                q = queries[:Q].contiguous()
                for nprobe in NPROBES:
                    ms = timed(lambda: idx.query_probed(q, K, nprobe))
                    lab, _d, _c, scanned = idx.query_probed(queries, K, nprobe)
                    lab = lab.cpu().numpy()
                    share = float(scanned.double().mean().item()) / n
                    recall = float(np.mean([len(set(lab[i]) & set(flat_lab[i])) / K for i in range(lab.shape[0])]))
                    out.append({"rows": n, "dtype": dtype, "Q": Q, "nprobe": nprobe, "probed_ms": round(ms, 4), "flat_ms": round(flat_ms[Q], 4),
                                "ratio": round(flat_ms[Q] / ms, 3), "scanned_share": round(share, 5), "recall_at_10": round(recall, 4),
                                "build_s": round(build_s, 2)})
                    say(f"{Q:6d}   {nprobe:6d}   {ms:9.3f}   {flat_ms[Q]:8.3f}   {flat_ms[Q] / ms:13.2f}   {share:13.5f}   {recall:9.4f}")
                    if n == 10_000_000 and dtype == "f16" and Q == 1 and nprobe == 32:
                        say(f"CONDITION (10M x 512 f16, C = 1024, nprobe = 32, Q = 1): probed {ms:.3f} ms, flat {flat_ms[Q]:.3f} ms: "
                            + ("HOLDS" if ms < flat_ms[Q] else "FAILS"))
            for Q in (1, 256):
                q = queries[:Q].contiguous()
                for name, fn in (("query_probed nprobe = 32", lambda: idx.query_probed(q, K, 32)), ("query", lambda: idx.query(q, K))):
                    tab = kernel_table(fn)
                    say(f"   kernels of one {name}, Q = {Q}: " + "; ".join(f"{k} x{c} {ms:.3f} ms" for k, c, ms in tab))
            idx.close()
            del idx
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"partition_bench": out}))


if __name__ == "__main__":
    main()

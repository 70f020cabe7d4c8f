#!/usr/bin/env python3
"""Distinct top-k (FlatIndex.query_distinct) beside the list stage alone (FlatIndex.query(k = pool), the parent commit's call,
unchanged) on the same index in the same process, timed on one GPU. No pass / fail gate.

1M x 512 rows, f16 and fp8; Q = 1 / 16 / 256; k = 10; pool = 80 / 512 / 2040; min_sep = 0.01. HIP events around each whole call (host
hand-over included), CUDA inputs and outputs, median of 15 calls after 2 warm-up calls. Two corpora:
  random:  random unit rows; nothing is suppressed, the suppression stage runs k rounds of one trip list each;
  bursts:  the near-duplicate corpus scaled up: N / 10 random directions, ten rows around each at cosine 0.9995 (pairwise distance
           about 0.001), the queries noisy copies of directions: every kept hit owns its burst.
share = (distinct - list) / distinct: what the suppression stage adds to the call. The stage's own kernel time comes from mmiss_prof
for one call per shape ("kernel ms"); kept = mean out_count, dups = mean entries owned per query.
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

D, K, MIN_SEP = 512, 10, 0.01
WARM, REPS = 2, 15
QS, POOLS = (1, 16, 256), (80, 512, 2040)


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


def kernel_ms(fn, prefix="distinct_"):
    """ms of the kernels whose class starts with `prefix` in one call under mmiss_prof"""
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        recs = _lib.prof_read()
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    return sum(float(r["ms"]) for r in recs if r["kernel"].startswith(prefix))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dtypes", default="f16,f8")
    ap.add_argument("--worst", action="store_true", help="also time the worst case: k = 1000, pool = 2040, nothing suppressed")
    args = ap.parse_args()
    n = args.rows
    lines, out = [], []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(6)

    def unit(m):
        v = torch.randn(m, D, device="cuda", generator=g)
        return v / v.norm(dim=1, keepdim=True)

    say(f"{n} x {D}; k = {K}; min_sep = {MIN_SEP}; median of {REPS} after {WARM}; list = query(k = pool)")
    for corpus in ("random", "bursts"):
        if corpus == "random":
            rows = unit(n)
            queries = unit(max(QS))
        else:
            centres = unit(n // 10)
            rows = (0.9995 * centres[:, None, :] + np.sqrt(1 - 0.9995 ** 2) * unit(n).reshape(n // 10, 10, D)).reshape(n, D)
            pick = torch.randint(0, n // 10, (max(QS),), device="cuda", generator=g)
            queries = centres[pick] + (0.5 / np.sqrt(D)) * torch.randn(max(QS), D, device="cuda", generator=g)
        for dtype in args.dtypes.split(","):
            idx = FlatIndex(D, dtype, capacity=n)
            for r0 in range(0, n, 250_000):
                m = min(250_000, n - r0)
                idx.add(rows[r0:r0 + m].contiguous(), np.arange(r0, r0 + m, dtype=np.int64))
            torch.cuda.synchronize()
            say(f"{corpus}, {dtype}")
            say("     Q    pool   distinct ms    list ms    share   kernel ms    kept     dups")
            for Q in QS:
                q = queries[:Q].contiguous()
                for pool in POOLS:
                    ms = timed(lambda: idx.query_distinct(q, K, MIN_SEP, pool))
                    list_ms = timed(lambda: idx.query(q, pool))
                    kms = kernel_ms(lambda: idx.query_distinct(q, K, MIN_SEP, pool))
                    _l, _d, cnt, dups, _m = idx.query_distinct(q, K, MIN_SEP, pool)
                    kept, owned = float(cnt.double().mean().item()), float(dups.sum(1).double().mean().item())
                    out.append({"corpus": corpus, "dtype": dtype, "Q": Q, "pool": pool, "distinct_ms": round(ms, 4), "list_ms": round(list_ms, 4),
                                "share": round((ms - list_ms) / ms, 3), "kernel_ms": round(kms, 4), "kept": kept, "dups": owned})
                    say(f"{Q:6d}  {pool:6d}   {ms:11.3f}   {list_ms:8.3f}   {(ms - list_ms) / ms:6.2f}   {kms:9.3f}   {kept:5.1f}   {owned:6.1f}")
            if args.worst and corpus == "random":
                for Q in (1, 16):
                    q = queries[:Q].contiguous()
                    ms = timed(lambda: idx.query_distinct(q, 1000, -1.0, 2040), reps=5)
                    list_ms = timed(lambda: idx.query(q, 2040), reps=5)
                    kms = kernel_ms(lambda: idx.query_distinct(q, 1000, -1.0, 2040))
                    out.append({"corpus": "worst", "dtype": dtype, "Q": Q, "pool": 2040, "k": 1000, "distinct_ms": round(ms, 3),
                                "list_ms": round(list_ms, 3), "kernel_ms": round(kms, 3)})
                    say(f"   worst case k = 1000, pool = 2040, min_sep = -1 (1000 rounds over up to 2039 positions), Q = {Q}: "
                        f"distinct {ms:.3f} ms, list {list_ms:.3f} ms, kernel {kms:.3f} ms")
            idx.close()
            del idx
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"distinct_bench": out}))


if __name__ == "__main__":
    main()

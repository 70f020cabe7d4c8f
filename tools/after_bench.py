#!/usr/bin/env python3
"""Search after (FlatIndex.query_after) beside the flat query (FlatIndex.query, the parent commit's code, unchanged) on the same index
in the same process, timed on one GPU. No pass / fail gate.

Corpus: random rows, dim 512; --rows N rows (default: 1M and 10M), f16 and fp8. HIP events around each whole call (host hand-over
included), CUDA inputs and outputs, median of 15 calls after 2 warm-up calls, the two calls alternating.
 (a) depth: the page of 20 entries at positions 1-20, 181-200, 1981-2000 and 100 001-100 020 of one query's ranking, by query_after
     from the cursor of the entry before it, against query(k = the page's last position) where the flat query reaches it (k <= 2040).
     The cursors come from FlatIndex.ranking (pages of 2040 chained), and the page at 1981 is compared with query(k = 2000).
 (b) memory roof: the dense scan's kernel time at Q = 1 (mmiss_prof) against the index bytes, and the key area's share of its traffic.
 (c) batches: Q = 16 and Q = 256 dense from the start of the ranking, beside query at the same Q.
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
from subset_bench import kernel_table, timed_pair  # noqa: E402

D, PAGE = 512, 20
POSITIONS = (0, 180, 1980, 100_000)          # entries of the ranking in front of the page
ELT = {"f16": 2, "f8": 1}


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
    queries = torch.randn(256, D, device="cuda", generator=g)
    say(f"corpus: random rows, dim {D}; page size {PAGE}; device inputs and outputs; median of 15 after 2, query_after and query alternating")
    for n in sizes:
        for dtype in args.dtypes.split(","):
            idx = FlatIndex(D, dtype, capacity=n)
            for r0 in range(0, n, 250_000):
                m = min(250_000, n - r0)
                idx.add(torch.randn(m, D, device="cuda", generator=g), np.arange(r0, r0 + m, dtype=np.int64))
            torch.cuda.synchronize()
            say(f"{n} x {D} {dtype}")
            q1 = queries[:1].contiguous()
            deep = max(POSITIONS)
            rank_l, rank_d = idx.ranking(q1[0], deep, page=2040)
            flat = idx.query(q1, 2000)
            ok = bool((rank_l[:2000] == flat[0][0]).all()) and bool((rank_d[:2000].view(torch.int32) == flat[1][0].view(torch.int32)).all())
            say(f"   ranking() to position {deep} in pages of 2040; its first 2000 entries equal query(k = 2000): {ok}")
            say("(a) position of the page   query_after ms   query(k = position + 20) ms")
            for pos in POSITIONS:
                if pos == 0:
                    ad = torch.full((1,), float("-inf"), device="cuda")
                    al = torch.zeros((1,), dtype=torch.int64, device="cuda")
                else:
                    ad, al = rank_d[pos - 1:pos].contiguous(), rank_l[pos - 1:pos].contiguous()
                k_flat = pos + PAGE
                if k_flat <= 2040:
                    a_ms, f_ms = timed_pair(lambda: idx.query_after(q1, PAGE, ad, al), lambda: idx.query(q1, k_flat))
                    page = idx.query_after(q1, PAGE, ad, al)
                    same = bool((page[0][0] == idx.query(q1, k_flat)[0][0, pos:]).all())
                else:
                    a_ms, _ = timed_pair(lambda: idx.query_after(q1, PAGE, ad, al), lambda: None)
                    f_ms, same = None, None
                out.append({"rows": n, "dtype": dtype, "position": pos + 1, "after_ms": round(a_ms, 4), "flat_ms": None if f_ms is None else round(f_ms, 4)})
                say(f"    {pos + 1:>9d}-{pos + PAGE:<9d}   {a_ms:12.3f}   " + ("      out of reach (k > 2040)" if f_ms is None else f"{f_ms:12.3f}   same labels: {same}"))
            plan = _lib.index_after_plan(idx._h, 1, PAGE)
            tab = kernel_table(lambda: idx.query_after(q1, PAGE, ad, al))
            scan = sum(v for k, v in tab.items() if k.startswith("after_scan"))
            row_bytes = n * (D * ELT[dtype] + 8 + (4 if dtype == "f8" else 0))      # rows, tags, fp8: inverse norms
            key_bytes = n * 8
            say("(b) kernels of one Q = 1 call (mmiss_prof, ms): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(tab.items())))
            say(f"    dense scan {scan:.3f} ms: {row_bytes / 1e9:.3f} GB read = {row_bytes / scan / 1e9:.2f} TB/s; with the {key_bytes / 1e6:.0f} MB of keys it "
                f"writes {(row_bytes + key_bytes) / scan / 1e9:.2f} TB/s (keys: {100.0 * key_bytes / (row_bytes + key_bytes):.1f} % of the traffic); "
                f"share {plan['share']}, splits {plan['splits']}, levels {plan['levels']}")
            out.append({"rows": n, "dtype": dtype, "scan_ms": round(scan, 4), "read_tbs": round(row_bytes / scan / 1e9, 3), "kernels": tab})
            say("(c)    Q   query_after ms   query ms   chunks   block")
            for Q in (16, 256):
                q = queries[:Q].contiguous()
                ad = torch.full((Q,), float("-inf"), device="cuda")
                al = torch.zeros((Q,), dtype=torch.int64, device="cuda")
                plan = _lib.index_after_plan(idx._h, Q, PAGE)
                reps = 15 if Q == 16 or n <= 1_000_000 else 3
                a_ms, f_ms = timed_pair(lambda: idx.query_after(q, PAGE, ad, al), lambda: idx.query(q, PAGE), reps=reps)
                out.append({"rows": n, "dtype": dtype, "Q": Q, "after_ms": round(a_ms, 4), "flat_ms": round(f_ms, 4), "chunks": plan["chunks"]})
                say(f"    {Q:4d}   {a_ms:14.3f}   {f_ms:8.3f}   {plan['chunks']:6d}   {plan['query_block']:5d}" + ("" if reps == 15 else f"   (median of {reps})"))
            idx.close()
            del idx
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"after_bench": out}))


if __name__ == "__main__":
    main()

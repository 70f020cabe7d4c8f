"""Where the index query's kernels sit beside the encoder's in the pipelined bench step, from a rocprofv3 --kernel-trace CSV of
bench.py --steps 20 --warmup 5 --retrieval-rows 0 --no-cpu-baseline --no-kernel-events --no-text.

The headline loop is the first 25 launches of prep_queries_kernel (5 warm-up + 20 timed steps); the window is 16 steady steps of
it, cut at the starts of that kernel. Printed per step: GPU-idle time (gaps in the UNION of the kernel intervals of all streams),
the query stage's kernels and how many of them overlap an encoder kernel, the mean duration of the encoder GEMMs named in
WATCH, and the timeline of the query-stage kernels of one step against the encoder kernels around them.

usage: python tools/query_overlap.py <kernel_trace.csv> [first_step last_step]"""
import csv
import re
import sys

QUERY = re.compile(r"prep_queries_kernel|gemm256s_kernel|select_topk_kernel|merge_lists_kernel|rerank_kernel|gather_rows_kernel|"
                   r"scan_topk_kernel|canonical_scan_kernel")
# (rocprofv3 prints the template arguments that are not defaults; kernels on _Float16 stay mangled: matched by substring)
WATCH = (("gemm256p_kernel<8,3,0,0>", re.compile(r"gemm256p_kernel<8,3[,>]")),
         ("gemm160p_kernel<9,0,48>", re.compile(r"gemm160p_kernel<9,(0,)?48>")))


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)
    return name.replace(" ", "")


def main():
    rows = []
    for r in csv.DictReader(open(sys.argv[1])):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    first, last = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (8, 24)
    preps = [s for s, _, n in rows if "prep_queries_kernel" in n]
    if len(preps) <= last:
        sys.exit("only %d launches of prep_queries_kernel in the trace" % len(preps))
    t0, t1, steps = preps[first], preps[last], last - first
    win = [(s, e, n) for s, e, n in rows if s >= t0 and s < t1]
    # union of the intervals
    busy, cur_s, cur_e = 0, None, None
    gaps = []
    for s, e, n in win:
        if cur_e is None:
            cur_s, cur_e = s, e
        elif s <= cur_e:
            cur_e = max(cur_e, e)
        else:
            busy += cur_e - cur_s
            gaps.append((s - cur_e, n))
            cur_s, cur_e = s, e
    busy += min(cur_e, t1) - cur_s
    span = t1 - t0
    print("window: steps %d..%d of the headline loop, %d kernels, %.1f us per step, busy (union) %.1f us, idle %.1f us per step"
          % (first, last, len(win), span / 1e3 / steps, busy / 1e3 / steps, (span - busy) / 1e3 / steps))
    big = sorted(gaps, reverse=True)[: 2 * steps]
    by = {}
    for g, n in big:
        by.setdefault(n, []).append(g / 1e3)
    for n, g in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        print("  largest gaps: %3d x %6.1f us in front of %s" % (len(g), sum(g) / len(g), n[:70]))
    enc = [(s, e) for s, e, n in win if not QUERY.search(n)]
    qk = [(s, e, n) for s, e, n in win if QUERY.search(n)]

    def overlaps(s, e):
        return sum(max(0, min(e, b) - max(s, a)) for a, b in enc if a < e and b > s)

    n_over = sum(1 for s, e, _ in qk if overlaps(s, e) > 0)
    t_q = sum(e - s for s, e, _ in qk)
    t_over = sum(min(e - s, overlaps(s, e)) for s, e, _ in qk)
    print("query stage: %.1f kernels per step, %.1f us per step; %.1f of them per step overlap an encoder kernel, for %.1f us per step"
          % (len(qk) / steps, t_q / 1e3 / steps, n_over / steps, t_over / 1e3 / steps))
    for w, pat in WATCH:
        d = [(e - s) / 1e3 for s, e, n in win if pat.search(n)]
        if d:
            print("  %-28s n = %4d  mean %7.2f us" % (w, len(d), sum(d) / len(d)))
    # one step's query-stage kernels, and the encoder kernel running when each starts
    mid = preps[first + steps // 2]
    nxt = preps[first + steps // 2 + 1]
    print("one step (offsets from its prep_queries_kernel, us):")
    for s, e, n in qk:
        if mid <= s < nxt:
            beside = [m for a, b, m in win if a < e and b > s and not QUERY.search(m)]
            print("  %8.1f .. %8.1f  %-44s beside %s" % ((s - mid) / 1e3, (e - mid) / 1e3, n[:44], ", ".join(sorted(set(x[:28] for x in beside))) or "-"))
    es = [(s, e) for s, e, n in win if mid <= s < nxt and not QUERY.search(n)]
    if es:
        print("  encoder kernels of that step: %d, first at %.1f, last ends at %.1f" % (len(es), (es[0][0] - mid) / 1e3, (max(e for _, e in es) - mid) / 1e3))


if __name__ == "__main__":
    main()

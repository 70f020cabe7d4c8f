"""plan_after (csrc/index_plans.h) — how a continuation call (mmiss_index_query_after) is laid out — checked on the host: a small
stand-alone C++ program (g++, no HIP, nothing loaded into Python) includes the header api_index.hip plans with and holds every
field to the rule the header and DESIGN §4h state: the bound (count without a list, min(n_cand, count) with one), the selection's
levels and strides, the chunking under the scratch budget, the query block per dim, the scan's share and splits, and the
compaction that only a listed call has."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal-image-similarity-search_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <algorithm>
#include "index_plans.h"

static long g_checked = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s  (count=%lld n_cand=%lld D=%d Q=%d k=%d kb=%d)\n", __LINE__, #c, \
    (long long)count, (long long)n_cand, D, Q, k, o.probe_scratch_kb); return 1; } } while (0)

static int one(int64_t count, int64_t n_cand, int D, int Q, int k, const PlanOptions& o) {
    const AfterPlan p = plan_after(count, n_cand, D, Q, k, o);
    const int64_t SEG = PLAN_PROBE_SEG;
    // the bound: every row without a list, what the list can name at the most with one; the key areas hold it
    CHECK(p.dense == (n_cand < 0));
    CHECK(p.bound == (n_cand < 0 ? count : std::min(count, n_cand)));
    CHECK(p.stride0 == std::max<int64_t>(p.bound, 1));
    // the levels: a level more while a query's keys exceed a segment, each level leaving k keys per segment
    int levels = 1;
    int64_t n = p.bound, first = 0;
    while (n > SEG) { n = (n + SEG - 1) / SEG * k; if (levels == 1) first = n; ++levels; }
    CHECK(p.levels == levels && p.stride1 == first && n <= SEG);
    // the chunks: the key areas of a chunk stay under the budget — one query always runs —, at most 32768 queries (the grid)
    const int64_t per_query = (p.stride0 + p.stride1) * 8, budget = (int64_t)o.probe_scratch_kb * 1024;
    CHECK(p.qchunk >= 1 && p.qchunk <= std::min(Q, 32768));
    CHECK(p.qchunk == 1 || p.qchunk * per_query <= budget);
    CHECK(p.qchunk == std::min(Q, 32768) || (p.qchunk + 1) * per_query > budget);
    CHECK(p.chunks == (Q + p.qchunk - 1) / p.qchunk);
    // the query block: the largest of 16 / 8 / 4 / 2 / 1 whose f32 staging fits 64 KB, whatever the storage dtype
    CHECK(p.qblock == 16 || p.qblock == 8 || p.qblock == 4 || p.qblock == 2 || p.qblock == 1);
    CHECK(p.lds == p.qblock * D * 4 && (p.lds <= 65536 || p.qblock == 1));
    CHECK(p.qblock == 16 || 2 * p.qblock * D * 4 > 65536);
    // the scan: at least 64 positions per workgroup, a multiple of the 16 a workgroup takes per trip, every position covered,
    // and no more workgroups than about 2048 once the share has left its floor
    const int64_t qblocks = (p.qchunk + p.qblock - 1) / p.qblock;
    CHECK(p.share >= 64 && p.share % 16 == 0 && p.splits >= 1);
    CHECK((int64_t)p.splits * p.share >= p.bound && (int64_t)(p.splits - 1) * p.share < std::max<int64_t>(p.bound, 1));
    CHECK(p.share == 64 || (int64_t)p.splits * qblocks <= 2048 + qblocks);
    // the compaction: only with a list — a bit per row, blocks of PLAN_SUBSET_BLOCK_ROWS rows
    if (p.dense) {
        CHECK(p.words == 0 && p.blocks == 0);
    } else {
        CHECK(p.words == (count + 31) / 32 && (int64_t)p.blocks * PLAN_SUBSET_BLOCK_ROWS >= count);
        CHECK(p.blocks == 0 || (int64_t)(p.blocks - 1) * PLAN_SUBSET_BLOCK_ROWS < count);
        // a listed call is planned as the subset call of the same list
        const SubsetPlan s = plan_subset(count, n_cand, D, Q, k, o);
        CHECK(s.bound == p.bound && s.levels == p.levels && s.stride0 == p.stride0 && s.stride1 == p.stride1 && s.qchunk == p.qchunk &&
              s.chunks == p.chunks && s.qblock == p.qblock && s.lds == p.lds && s.share == p.share && s.splits == p.splits &&
              s.words == p.words && s.blocks == p.blocks);
    }
    // the cursor does not enter: there is no argument for it
    ++g_checked;
    return 0;
}

int main() {
    PlanOptions dflt, small;
    small.probe_scratch_kb = 64;
    for (const PlanOptions& o : {dflt, small})
        for (int64_t count : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)4096, (int64_t)4097, (int64_t)17000, (int64_t)140005, (int64_t)1000000,
                              (int64_t)10000000, (int64_t)2147483647})
            for (int64_t n_cand : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)64, (int64_t)65, (int64_t)4096, (int64_t)4097, (int64_t)16385,
                                   (int64_t)100000, (int64_t)2147483647})
                for (int D : {128, 512, 1152, 1920, 3968, 4096})
                    for (int Q : {1, 5, 16, 17, 300, 40000})
                        for (int k : {1, 10, 1000, 2040})
                            if (one(count, n_cand, D, Q, k, o)) return 1;
    // the edges the GPU tests lean on, literally
    {
        const PlanOptions o;
        const int64_t count = 17000, n_cand = -1; const int D = 128, Q = 1, k = 1000;
        CHECK(plan_after(4096, n_cand, D, Q, k, o).levels == 1);             // the dense bound is the row count
        CHECK(plan_after(4097, n_cand, D, Q, k, o).levels == 2);
        CHECK(plan_after(16384, n_cand, D, Q, k, o).levels == 2);
        CHECK(plan_after(count, n_cand, D, Q, k, o).levels == 3 && plan_after(count, n_cand, D, Q, k, o).stride1 == 5000);
        CHECK(plan_after(count, 100000, D, Q, k, o).bound == 17000 && !plan_after(count, 100000, D, Q, k, o).dense);
        CHECK(plan_after(count, 0, D, Q, k, o).bound == 0 && !plan_after(count, 0, D, Q, k, o).dense);   // the empty list is a list
        CHECK(plan_after(4999, n_cand, D, Q, 10, o).share == 64 && plan_after(4999, n_cand, D, Q, 10, o).splits == 79);
        // 140 005 rows, three queries: one narrowed block, 2048 workgroups of 69 (rounded up to 80) positions
        const AfterPlan mid = plan_after(140005, n_cand, D, 3, 10, o);
        CHECK(mid.share == 80 && mid.splits == 1751 && mid.qblock == 16 && subset_block_for(mid.qblock, 3) == 4 && mid.levels == 2);
        // 10M rows, one query: 2048 workgroups of 4883 (rounded up to 4896) rows each
        const AfterPlan big = plan_after(10000000, n_cand, 512, 1, 20, o);
        CHECK(big.share == 4896 && big.splits == 2043 && big.levels == 3 && big.stride1 == 48840 && big.chunks == 1);
        // ... 256 queries: 512 MB / (10 000 000 + 24 420) keys of 8 bytes = 6 queries per chunk
        const AfterPlan wide = plan_after(10000000, n_cand, 512, 256, 10, o);
        CHECK(wide.qchunk == 6 && wide.chunks == 43);
        PlanOptions s; s.probe_scratch_kb = 120;
        CHECK(plan_after(5000, n_cand, D, 8, 10, s).qchunk == 3 && plan_after(5000, n_cand, D, 8, 10, s).chunks == 3);
    }
    std::printf("ok: %ld plans\n", g_checked);
    return 0;
}
"""


def test_plan_after_follows_its_rules(tmp_path):
    src = tmp_path / "after_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "after_plan_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout

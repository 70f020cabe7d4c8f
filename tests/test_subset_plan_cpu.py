"""plan_subset (csrc/index_plans.h) — how a subset call is laid out — checked on the host: a small stand-alone C++ program (g++, no
HIP, nothing loaded into Python) includes the header api_index.hip plans with and holds every field to the rule the header and
DESIGN §4g state: the bound, the selection's levels and strides, the chunking under the scratch budget, the query block per dim,
the scan's share and splits, the compaction's blocks."""
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
    const SubsetPlan p = plan_subset(count, n_cand, D, Q, k, o);
    const int64_t SEG = PLAN_PROBE_SEG;
    // the bound: what the list can name at the most; the key areas hold it
    CHECK(p.bound == std::min(count, n_cand));
    CHECK(p.stride0 == std::max<int64_t>(p.bound, 1));
    // the levels: a level more while a query's keys exceed a segment, each level leaving k keys per segment
    int levels = 1;
    int64_t n = p.bound, first = 0;
    while (n > SEG) { n = (n + SEG - 1) / SEG * k; if (levels == 1) first = n; ++levels; }
    CHECK(p.levels == levels && p.stride1 == first && n <= SEG);
    CHECK((p.levels == 1) == (p.bound <= SEG));
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
    // the scan: at least 64 list positions per workgroup, a multiple of the 16 a workgroup takes per trip, every position covered,
    // and no more workgroups than about 2048 once the share has left its floor
    const int64_t qblocks = (p.qchunk + p.qblock - 1) / p.qblock;
    CHECK(p.share >= 64 && p.share % 16 == 0 && p.splits >= 1);
    CHECK((int64_t)p.splits * p.share >= p.bound && (int64_t)(p.splits - 1) * p.share < std::max<int64_t>(p.bound, 1));
    CHECK(p.share == 64 || (int64_t)p.splits * qblocks <= 2048 + qblocks);
    CHECK(p.share == 64 || (int64_t)p.splits * qblocks > 1024 || qblocks > 2048);
    // the compaction: a bit per row, blocks of PLAN_SUBSET_BLOCK_ROWS rows
    CHECK(p.words == (count + 31) / 32 && (int64_t)p.blocks * PLAN_SUBSET_BLOCK_ROWS >= count);
    CHECK(p.blocks == 0 || (int64_t)(p.blocks - 1) * PLAN_SUBSET_BLOCK_ROWS < count);
    ++g_checked;
    return 0;
}

int main() {
    PlanOptions dflt, small;
    small.probe_scratch_kb = 64;
    for (const PlanOptions& o : {dflt, small})
        for (int64_t count : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)4097, (int64_t)17000, (int64_t)1000000, (int64_t)10000000})
            for (int64_t n_cand : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)4095, (int64_t)4096, (int64_t)4097, (int64_t)16384,
                                   (int64_t)16385, (int64_t)100000, (int64_t)5000000, (int64_t)2147483647})
                for (int D : {128, 512, 768, 1024, 1152, 1920, 2048, 3968, 4096})
                    for (int Q : {1, 5, 16, 17, 64, 300, 40000})
                        for (int k : {1, 10, 1000, 2040})
                            if (one(count, n_cand, D, Q, k, o)) return 1;
    // the edges the GPU tests lean on, literally
    {
        const PlanOptions o;
        const int64_t count = 17000, n_cand = 0; const int D = 128, Q = 1, k = 1000; (void)n_cand;
        CHECK(plan_subset(count, 4096, D, Q, k, o).levels == 1);           // k = 1000 below / above 4096 keys
        CHECK(plan_subset(count, 4097, D, Q, k, o).levels == 2);
        CHECK(plan_subset(count, 16384, D, Q, k, o).levels == 2);          // ... and below / above 16 384 keys
        CHECK(plan_subset(count, 16385, D, Q, k, o).levels == 3);
        CHECK(plan_subset(count, 16385, D, Q, k, o).stride1 == 5000);
        CHECK(plan_subset(count, 100000, D, Q, k, o).bound == 17000);      // a list longer than the index
        CHECK(plan_subset(count, 65, D, Q, 10, o).share == 64 && plan_subset(count, 65, D, Q, 10, o).splits == 2);
        for (int d : {128, 512, 1024}) CHECK(plan_subset(count, 65, d, Q, k, o).qblock == 16);
        CHECK(plan_subset(count, 65, 1152, Q, k, o).qblock == 8 && plan_subset(count, 65, 1920, Q, k, o).qblock == 8);
        CHECK(plan_subset(count, 65, 2048, Q, k, o).qblock == 8 && plan_subset(count, 65, 3968, Q, k, o).qblock == 4);
        CHECK(plan_subset(count, 65, 4096, Q, k, o).qblock == 4);
        // 10M rows, a 1 % list, one query: 2048 workgroups of 49 (rounded up to 64) positions
        const SubsetPlan big = plan_subset(10000000, 100000, 512, 1, 10, o);
        CHECK(big.share == 64 && big.splits == 1563 && big.levels == 2 && big.blocks == 306);
        // ... a 50 % list, 256 queries: 16 query blocks, 128 shares
        const SubsetPlan wide = plan_subset(10000000, 5000000, 512, 256, 10, o);
        CHECK(wide.qchunk == 13 && wide.chunks == 20);                     // 512 MB / (5 000 000 + 12 210) keys of 8 bytes
        // a chunk with fewer queries than the block runs the narrowest instance that holds them
        const int narrowed[][3] = {{16, 1, 1}, {16, 2, 2}, {16, 3, 4}, {16, 5, 8}, {16, 8, 8}, {16, 9, 16}, {16, 300, 16}, {8, 1, 1}, {8, 5, 8},
                                   {4, 3, 4}, {4, 2, 2}, {2, 1, 1}, {1, 1, 1}, {1, 64, 1}};
        for (const auto& t : narrowed) CHECK(subset_block_for(t[0], t[1]) == t[2]);
        PlanOptions s; s.probe_scratch_kb = 120;
        CHECK(plan_subset(count, 5000, D, 8, 10, s).qchunk == 3 && plan_subset(count, 5000, D, 8, 10, s).chunks == 3);
    }
    std::printf("ok: %ld plans\n", g_checked);
    return 0;
}
"""


def test_plan_subset_follows_its_rules(tmp_path):
    src = tmp_path / "subset_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "subset_plan_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout

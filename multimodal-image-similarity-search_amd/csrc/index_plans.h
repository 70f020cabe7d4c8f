// index_plans.h — the launch-shape arithmetic of the index's host layer (api_index.hip): how many queries a scan block stages, how
// the rows are cut into slabs, how a selection or a merge is split, how a probed, a subset or a continuation call is chunked, how the suppression stage of a
// distinct call is laid out, where the arrays of a result block lie. Plain C++, no HIP include, no option lookup: api_index.hip, its debug plan entries (mmiss_dbg_index_*plan) and a
// host-only test program (tests/test_index_plans_cpu.py) all take the rules from here.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <initializer_list>

// the options these rules read, at their defaults; api_index.hip fills one from mmiss_option per call (plan_options)
struct PlanOptions {
    int scan_rounds = 1, scan_max_slabs = 1024;   // plan_scan
    int merge_two_level_min = 64;                 // merge_two_level
    int score_strip_fit = 1, score_strip = 0;     // strip_length
    int probe_scratch_kb = 512 * 1024;            // plan_probed
};

// what the kernel headers fix and these rules repeat (api_index.hip holds them to SELECT_UNIT and PROBE_SEG with a static_assert)
constexpr int PLAN_SELECT_UNIT = 1024;   // group maxima per unit of select_topk_kernel
constexpr int PLAN_PROBE_SEG = 4096;     // keys per segment of segment_topk_kernel

// ------------------------------------------------------------------------------------------------ streaming scan
// a streaming scan launch: 16 * nqt queries per block in list mode (cap entries per query and wave) or, thr, in threshold mode
// (the widen pass: every row reaching its query's threshold is appended to a.glist)
struct ScanPlan {
    int nqt, cap, lds, slabs, qtiles, tiles_per_block;
    bool thr;
};

constexpr int SCAN_LDS_LIMIT = 160 * 1024;
// dynamic LDS of the streaming scan for a block of 16 * nqt queries: the staged query rows (+ 16 B of padding each) and,
// in list mode, four waves' (score, row) lists of `cap` entries per query with their counts and thresholds
inline int scan_lds_bytes(int D, int qelt, int nqt, int cap) {
    const int NQ = 16 * nqt;
    return (((NQ * (D * qelt + 16)) + 15) & ~15) + 2 * 4 * NQ * cap * 4 + 2 * 4 * NQ * 4;
}
// ... in threshold mode (the widen pass, membership, assignment): the query rows only
inline int sweep_scan_lds(int D, int qelt, int nqt) { return ((16 * nqt * (D * qelt + 16)) + 15) & ~15; }

inline ScanPlan plan_scan(int D, int elt, int Q, int kp, int64_t N, const PlanOptions& o) {
    ScanPlan p{};
    const int limit = SCAN_LDS_LIMIT;
    p.nqt = 1; p.cap = 64;
    if (kp <= 16 && Q > 16) {
        for (int nqt : {4, 2})
            if (scan_lds_bytes(D, elt, nqt, 32) <= limit && (Q > 16 * nqt / 2)) { p.nqt = nqt; p.cap = 32; break; }
    }
    const int NQ = 16 * p.nqt;
    p.lds = scan_lds_bytes(D, elt, p.nqt, p.cap);
    p.qtiles = (Q + NQ - 1) / NQ;
    const int64_t ntiles = (N + 15) / 16;
    const int blocks_per_cu = std::max(1, std::min(8, limit / p.lds));
    int64_t target = (int64_t)256 * blocks_per_cu * o.scan_rounds / p.qtiles;
    if (target < 1) target = 1;
    if (target > o.scan_max_slabs) target = o.scan_max_slabs;
    int64_t tpb = (ntiles + target - 1) / target;
    tpb = (tpb + 3) / 4 * 4;  // every wave of a block gets the same number of tiles
    if (tpb < 4) tpb = 4;
    p.tiles_per_block = (int)tpb;
    p.slabs = (int)((ntiles + tpb - 1) / tpb);
    return p;
}

// ------------------------------------------------------------------------------------------------ dense scans
// A scan of EVERY row against n operands whose block stages its operands only: the widen pass's threshold scan (flagged queries),
// the membership scan (probes), the assignment scan (centres). The operand tile is the narrowest of 16 / 32 / 64 that holds all n
// (a wider one would only multiply the MFMA work of a pass that is bound by reading the rows), halved while the staged block does
// not fit the CU's LDS: 64 fit at dim 512 / 768 / 1024 in f16 or fp8 and at dim 512 in f32 (f32 rows at the reference's D = 768:
// 64 x 3088 B = 193 KB do not, 32 do), 16 at dim 3968 (and f32 at 1920). nqt = 1 always fits: mmiss_index_create admits
// only dims whose 16-query block does. Operands beyond one tile are served by further tiles in the grid's y (the widen pass:
// qtiles, and the slab target shrinks with them) or, by_passes, by further launches (membership, assignment: passes).
struct DensePlan {
    int nqt, lds, slabs, tiles_per_block;
    int qtiles, passes;   // one of them is 1
    ScanPlan as_scan() const { return ScanPlan{nqt, 32, lds, slabs, qtiles, tiles_per_block, true}; }   // (the widen pass's launch)
};

inline DensePlan plan_dense(int D, int qelt, int n, int64_t N, bool by_passes) {
    DensePlan p{};
    p.nqt = n > 32 ? 4 : n > 16 ? 2 : 1;
    while (p.nqt > 1 && sweep_scan_lds(D, qelt, p.nqt) > SCAN_LDS_LIMIT) p.nqt >>= 1;
    p.lds = sweep_scan_lds(D, qelt, p.nqt);
    const int tiles = (n + 16 * p.nqt - 1) / (16 * p.nqt);
    p.qtiles = by_passes ? 1 : tiles;
    p.passes = by_passes ? tiles : 1;
    const int64_t ntiles = (N + 15) / 16;
    const int per_cu = std::max(1, std::min(8, SCAN_LDS_LIMIT / p.lds));
    const int64_t target = std::max<int64_t>(1, (int64_t)256 * per_cu / p.qtiles);
    const int64_t tpb = std::max<int64_t>(4, (((ntiles + target - 1) / target) + 3) / 4 * 4);
    p.tiles_per_block = (int)tpb;
    p.slabs = (int)((ntiles + tpb - 1) / tpb);
    return p;
}

// ------------------------------------------------------------------------------------------------ capped grids
// The kernels behind the dense scans walk all N rows (or N list positions) with a grid-stride loop on a capped grid:
// min(cap, ceil(N / per_block)) blocks of 256 threads, a block taking per_block consecutive items per trip — 16 where a group of
// 16 lanes computes one canonical dot product (four rows per wave), 256 where a thread takes one row. The grid covers
// grid * per_block items per trip, so a kernel's second trip starts at N > cap * per_block.
inline int capped_grid(int64_t n, int per_block, int cap) { return (int)std::min<int64_t>(cap, (n + per_block - 1) / per_block); }

constexpr int PLAN_CANON_ROWS_PER_BLOCK = 16;    // canonical_scan_kernel, assign_resolve_kernel
constexpr int PLAN_POINT_ROWS_PER_BLOCK = 256;   // the pointwise kernels
constexpr int PLAN_CANONICAL_SCAN_CAP = 8192;    // canonical_scan_kernel: second trip at N > 131 072
constexpr int PLAN_ASSIGN_RESOLVE_CAP = 4096;    // assign_resolve_kernel: N (or list positions) > 65 536
constexpr int PLAN_COUNT_CAP = 1024;             // member_count_kernel, assign_sizes_kernel: N > 262 144
constexpr int PLAN_ASSIGN_DECIDE_CAP = 2048;     // assign_decide_kernel: N > 524 288
constexpr int PLAN_MEMBER_WORDS_CAP = 4096;      // member_from_dist_kernel, member_merge_tags_kernel: N > 1 048 576

inline int canonical_scan_grid(int64_t N) { return capped_grid(N, PLAN_CANON_ROWS_PER_BLOCK, PLAN_CANONICAL_SCAN_CAP); }
inline int assign_resolve_grid(int64_t N) { return capped_grid(N, PLAN_CANON_ROWS_PER_BLOCK, PLAN_ASSIGN_RESOLVE_CAP); }
inline int member_count_grid(int64_t N) { return capped_grid(N, PLAN_POINT_ROWS_PER_BLOCK, PLAN_COUNT_CAP); }
inline int assign_sizes_grid(int64_t N) { return capped_grid(N, PLAN_POINT_ROWS_PER_BLOCK, PLAN_COUNT_CAP); }
inline int assign_decide_grid(int64_t N) { return capped_grid(N, PLAN_POINT_ROWS_PER_BLOCK, PLAN_ASSIGN_DECIDE_CAP); }
inline int member_from_dist_grid(int64_t N) { return capped_grid(N, PLAN_POINT_ROWS_PER_BLOCK, PLAN_MEMBER_WORDS_CAP); }
inline int member_merge_tags_grid(int64_t N) { return capped_grid(N, PLAN_POINT_ROWS_PER_BLOCK, PLAN_MEMBER_WORDS_CAP); }

// ------------------------------------------------------------------------------------------------ score GEMM, select, merge
// consecutive index tiles per workgroup of the strip score GEMM (Mq queries padded to 256, ncol column tiles of 256 rows):
// long enough to amortise the pipeline fill, short enough to leave >= 8 workgroups per CU for balance; among the strip
// lengths down to half that, the one whose rounds x length (+ a quarter tile of pipeline fill per workgroup and round) is
// smallest (10M rows x 1024 queries: strip 32 gave 4884 workgroups = 19.08 rounds of 256 -> 5 % of the launch spent with 18
// workgroups on the chip).
inline int strip_length(int Mq, int64_t nbn, int64_t ncol, const PlanOptions& o) {
    const int64_t tiles = nbn * (Mq / 256);
    int strip = (int)std::min<int64_t>(32, std::max<int64_t>(1, tiles / 2048));
    if (strip >= 8 && o.score_strip_fit != 0) {
        double best = 1e300;
        int best_s = strip;
        for (int sl = strip; sl >= strip / 2; --sl) {
            const int64_t wgs = (Mq / 256) * ((ncol + sl - 1) / sl);
            const int64_t rounds = (wgs + 255) / 256;
            const double cost = (double)rounds * (sl + 0.25);
            if (cost < best - 1e-9) { best = cost; best_s = sl; }
        }
        strip = best_s;
    }
    if (o.score_strip > 0) strip = o.score_strip;
    return strip;
}

// blocks per query of select_topk over ng group maxima: about 1024 blocks per call, every block at least one unit of
// PLAN_SELECT_UNIT groups, 32 at the most
inline int select_splits(int ng, int Q) {
    const int units = (ng + PLAN_SELECT_UNIT - 1) / PLAN_SELECT_UNIT;
    int splits = (1024 + Q - 1) / Q;
    if (splits > units) splits = units;
    if (splits > 32) splits = 32;
    if (splits < 1) splits = 1;
    return splits;
}

// merge L per-slab lists of every query into its candidate page; above merge_two_level_min lists in two levels so that a single
// query (the API path) is not merged by one lone workgroup
constexpr int MERGE_LISTS_PER_BLOCK = 32;   // lists per first-level merge block
inline bool merge_two_level(int L, const PlanOptions& o) { return L > o.merge_two_level_min; }

// ------------------------------------------------------------------------------------------------ partitioned search
// How a probed call of Q queries runs on a partition of C cells over the first B of `count` rows, `largest` its largest cell and
// top_prefix[j] ([C + 1]) the sum of its j largest. bound: the most keys one query can have (the tail and the NP largest cells):
// it sizes the candidate areas and fixes the selection's levels, so nothing has to come back from the device inside a call.
struct ProbePlan {
    int NP = 0;                 // probe slots: min(nprobe, C)
    int splits = 1, share = 64; // workgroups per list of the scan, rows of a list per workgroup
    int levels = 1;             // segment_topk launches, the FINAL one included
    int qchunk = 1;             // queries per chunk (the scratch budget)
    int64_t bound = 0, stride0 = 1, stride1 = 0;   // keys per query of the two key areas
};

inline ProbePlan plan_probed(int64_t count, int64_t B, int64_t largest, const int64_t* top_prefix, int C, int Q, int k, int nprobe,
                             const PlanOptions& o) {
    ProbePlan p;
    p.NP = std::min(nprobe, C);
    const int64_t tail = count - B;
    p.bound = tail + top_prefix[p.NP];
    p.stride0 = std::max<int64_t>(p.bound, 1);
    for (int64_t n = p.bound; n > PLAN_PROBE_SEG; n = (n + PLAN_PROBE_SEG - 1) / PLAN_PROBE_SEG * k) {
        if (p.levels == 1) p.stride1 = (n + PLAN_PROBE_SEG - 1) / PLAN_PROBE_SEG * k;
        ++p.levels;
    }
    // chunks: the key areas of a chunk's queries stay under the budget (one query always runs, whatever it needs)
    const int64_t budget = (int64_t)o.probe_scratch_kb * 1024;
    const int64_t per_query = (p.stride0 + p.stride1) * 8;
    p.qchunk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(Q, 32768), budget / per_query));
    // the scan: about eight workgroups per CU over (lists x queries of a chunk), 64 rows per workgroup at the least, so that a
    // single query with few probes still fills the chip
    const int64_t maxlist = std::max(tail, largest);
    const int64_t lists = (int64_t)p.qchunk * (p.NP + 1);
    const int64_t want = std::max<int64_t>(1, (2048 + lists - 1) / lists);
    p.share = (int)std::max<int64_t>(64, ((maxlist + want - 1) / want + 15) / 16 * 16);
    p.splits = (int)std::max<int64_t>(1, (maxlist + p.share - 1) / p.share);
    return p;
}

// ------------------------------------------------------------------------------------------------ subset search
// How a subset call of Q queries with a list of n_cand labels runs on `count` rows of dim D (subset_kernels.h). bound: the most
// rows the list can name, min(n_cand, count): it sizes rows[] and the key areas and fixes the selection's levels, as plan_probed's
// bound does, so nothing comes back from the device inside a call. qblock: the queries a scan workgroup stages and scores every
// row of its share against — the largest of 16 / 8 / 4 / 2 / 1 whose f32 staging fits PLAN_SUBSET_LDS (the storage dtype does not
// enter: the staged queries are f32 for every dtype). A chunk with fewer queries than that runs the narrowest instance that holds
// them (subset_block_for): a single query is not scored as sixteen.
constexpr int PLAN_SUBSET_LDS = 64 * 1024;
constexpr int PLAN_SUBSET_BLOCK_ROWS = 32768;   // rows per block of the bitmap's compaction
// blocks of the compaction over `count` rows: block b > 0 writes behind the rows of blocks [0, b) (subset_offsets_kernel's sums)
inline int subset_compact_blocks(int64_t count) { return (int)((count + PLAN_SUBSET_BLOCK_ROWS - 1) / PLAN_SUBSET_BLOCK_ROWS); }
struct SubsetPlan {
    int64_t bound = 0, stride0 = 1, stride1 = 0;   // keys per query of the two key areas
    int levels = 1;                                // segment_topk launches, the FINAL one included
    int qchunk = 1, chunks = 1;                    // queries per chunk (the scratch budget), chunks of the call
    int qblock = 1, lds = 0;                       // queries per scan workgroup, its dynamic LDS
    int share = 64, splits = 1;                    // list positions per scan workgroup, workgroups per query block
    int64_t words = 0;                             // 32-bit words of the bitmap
    int blocks = 0;                                // blocks of the compaction
};

// the query block a chunk of Qc queries runs with: qblock halved while half of it still holds them all
inline int subset_block_for(int qblock, int Qc) {
    while (qblock > 1 && qblock / 2 >= Qc) qblock /= 2;
    return qblock;
}

inline SubsetPlan plan_subset(int64_t count, int64_t n_cand, int D, int Q, int k, const PlanOptions& o) {
    SubsetPlan p;
    p.bound = std::min(n_cand, count);
    p.stride0 = std::max<int64_t>(p.bound, 1);
    for (int64_t n = p.bound; n > PLAN_PROBE_SEG; n = (n + PLAN_PROBE_SEG - 1) / PLAN_PROBE_SEG * k) {
        if (p.levels == 1) p.stride1 = (n + PLAN_PROBE_SEG - 1) / PLAN_PROBE_SEG * k;
        ++p.levels;
    }
    const int64_t budget = (int64_t)o.probe_scratch_kb * 1024;
    const int64_t per_query = (p.stride0 + p.stride1) * 8;
    p.qchunk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(Q, 32768), budget / per_query));
    p.chunks = (Q + p.qchunk - 1) / p.qchunk;
    p.qblock = 1;
    for (int nqb : {16, 8, 4, 2})
        if ((int64_t)nqb * D * 4 <= PLAN_SUBSET_LDS) { p.qblock = nqb; break; }
    p.lds = p.qblock * D * 4;
    // the scan: about 2048 workgroups over (shares x query blocks of a chunk), 64 list positions per workgroup at the least
    const int64_t qblocks = (p.qchunk + p.qblock - 1) / p.qblock;
    const int64_t want = std::max<int64_t>(1, (2048 + qblocks - 1) / qblocks);
    p.share = (int)std::max<int64_t>(64, ((p.bound + want - 1) / want + 15) / 16 * 16);
    p.splits = (int)std::max<int64_t>(1, (p.bound + p.share - 1) / p.share);
    p.words = (count + 31) / 32;
    p.blocks = subset_compact_blocks(count);
    return p;
}

// ------------------------------------------------------------------------------------------------ search after
// How a continuation call (mmiss_index_query_after, after_kernels.h) of Q queries runs on `count` rows of dim D. n_cand < 0: no
// list — the dense scan, whose position i is row i: the bound is count, nothing is marked or compacted (words = blocks = 0).
// n_cand >= 0: a list, and plan_subset's bound min(n_cand, count) with its compaction. Everything else — levels and strides,
// chunks under probe_scratch_kb, the query block from PLAN_SUBSET_LDS narrowed to the chunk (subset_block_for), share and
// splits — is plan_subset's rule applied to that bound: the cursor removes keys on the device, never positions, so the host
// bound does not depend on it.
struct AfterPlan : SubsetPlan {
    bool dense = true;
};

inline AfterPlan plan_after(int64_t count, int64_t n_cand, int D, int Q, int k, const PlanOptions& o) {
    AfterPlan p;
    static_cast<SubsetPlan&>(p) = plan_subset(count, n_cand < 0 ? count : n_cand, D, Q, k, o);
    p.dense = n_cand < 0;
    if (p.dense) { p.words = 0; p.blocks = 0; }
    return p;
}

// ------------------------------------------------------------------------------------------------ distinct results
// The suppression stage of mmiss_index_query_distinct (distinct_kernels.h): one workgroup of PLAN_DISTINCT_THREADS per query, all
// queries of the call in ONE launch; a group of 16 lanes per list position, so a trip covers threads / 16 consecutive positions;
// LDS: the kept row as an f32 query and four int32 arrays of PLAN_DISTINCT_SLOTS list positions (row, owner, kept, owned counts).
constexpr int PLAN_DISTINCT_THREADS = 1024;
constexpr int PLAN_DISTINCT_SLOTS = 2048;
constexpr int PLAN_DISTINCT_MAX_POOL = 2040;   // the list calls' own limit on k
struct DistinctPlan { int rows_per_trip, threads, lds, queries_per_launch, launches; };

inline DistinctPlan plan_distinct(int D, int Q) {
    DistinctPlan p{};
    p.threads = PLAN_DISTINCT_THREADS;
    p.rows_per_trip = p.threads / 16;
    p.lds = D * 4 + 4 * PLAN_DISTINCT_SLOTS * 4;
    p.queries_per_launch = Q;
    p.launches = 1;
    return p;
}

// ------------------------------------------------------------------------------------------------ grouped search
// How a grouped call (mmiss_index_query_grouped, grouped_kernels.h) of Q queries runs on `count` rows of dim D whose group
// high-water mark is G. The list stage is the flat query at k = pool (pool 0: min(2040, max(8 k, 64))); the walk is one workgroup
// of PLAN_GROUPED_THREADS per query, all queries in one launch, with a fixed block of LDS. The exhaustive route — queries whose
// walk is not complete, Qx of them at the most — selects over a table of G + count slots per query: the grouped rows' slots, then
// one per row for the ungrouped. plan_subset's rules applied to that bound give levels and strides, the chunks under
// probe_scratch_kb, the query block from PLAN_SUBSET_LDS (narrowed per chunk by subset_block_for) and the share of ROWS per scan
// workgroup: the scan walks `count` rows, not `table` positions.
constexpr int PLAN_GROUPED_THREADS = 1024;
constexpr int PLAN_GROUPED_SLOTS = 2048;
constexpr int PLAN_GROUPED_MAX_POOL = 2040;            // the list calls' own limit on k
constexpr int PLAN_GROUPED_WALK_LDS = PLAN_GROUPED_SLOTS * 16 + 64;
constexpr int PLAN_GROUPED_MAX_GROUPS = 1 << 24;       // MMISS_MAX_GROUPS
inline int grouped_default_pool(int k) { return std::min(PLAN_GROUPED_MAX_POOL, std::max(8 * k, 64)); }
struct GroupedPlan {
    int pool = 0;
    int walk_threads = PLAN_GROUPED_THREADS, walk_lds = PLAN_GROUPED_WALK_LDS;
    int64_t table = 0, stride0 = 1, stride1 = 0;   // slots per query = keys at level 0; keys per query of the two key areas
    int levels = 1;                                // segment_topk launches, the FINAL one included
    int qchunk = 1, chunks = 1;                    // flagged queries per chunk, chunks when all Qx queries are flagged
    int qblock = 1, lds = 0;                       // queries per scan workgroup, its dynamic LDS (queries and their masks)
    int share = 64, splits = 1;                    // rows per scan workgroup, workgroups per query block
};

inline GroupedPlan plan_grouped(int64_t count, int64_t G, int D, int Qx, int k, int pool, const PlanOptions& o) {
    GroupedPlan p;
    p.pool = pool > 0 ? pool : grouped_default_pool(k);
    p.table = G + count;
    const SubsetPlan s = plan_subset(p.table, p.table, D, Qx, k, o);
    p.stride0 = s.stride0; p.stride1 = s.stride1; p.levels = s.levels;
    p.qchunk = s.qchunk; p.chunks = s.chunks; p.qblock = s.qblock;
    p.lds = p.qblock * D * 4 + p.qblock * 16;
    const int64_t qblocks = (p.qchunk + p.qblock - 1) / p.qblock;
    const int64_t want = std::max<int64_t>(1, (2048 + qblocks - 1) / qblocks);
    p.share = (int)std::max<int64_t>(64, ((count + want - 1) / want + 15) / 16 * 16);
    p.splits = (int)std::max<int64_t>(1, (count + p.share - 1) / p.share);
    return p;
}

// ------------------------------------------------------------------------------------------------ cluster sums
// cluster_sums_kernel over N rows of dim D into C clusters: the widest column chunk (a divisor of dim, a multiple of 16) whose
// [C][cols] table of 64-bit sums fits 128 KiB of LDS — all of dim 512 up to 32 clusters, 16 columns at 1024 clusters —, and the
// rows cut into about 2048 / chunks slabs of 64 rows at the least
struct ClusterSumsPlan { int cols, chunks, rows_per_block, slabs, lds; };

inline ClusterSumsPlan plan_cluster_sums(int D, int C, int64_t N) {
    constexpr int TABLE_LDS = 128 * 1024;
    ClusterSumsPlan p{};
    p.cols = 16;
    for (int k = 1; k <= D / 16; ++k)
        if (D % k == 0 && (D / k) % 16 == 0 && (size_t)C * (D / k) * 8 <= (size_t)TABLE_LDS) { p.cols = D / k; break; }
    p.chunks = D / p.cols;
    const int64_t slab_target = std::max<int64_t>(1, 2048 / p.chunks);
    p.rows_per_block = (int)std::max<int64_t>(64, (N + slab_target - 1) / slab_target);
    p.slabs = (int)((N + p.rows_per_block - 1) / p.rows_per_block);
    p.lds = C * p.cols * 8;
    return p;
}

// ------------------------------------------------------------------------------------------------ result block
// Where the arrays of a call's results lie in the handle's pinned block (api_index.hip ResultBlock), as byte offsets: `slots`
// int64 labels per query at 0, then — if the call has them — an int64 total per query, `slots` float distances per query, an
// int32 count per query and — if the call has them — an int32 flag per query. need: the bytes in all; grow: what a block that is
// too small becomes (a power of two, 4096 at the least). Every array is aligned to its element size: the 8-byte ones come first.
struct ResultLayout { size_t tot, dist, cnt, flags, need, grow; };

inline ResultLayout result_layout(int64_t Q, int64_t slots, bool totals, bool flags) {
    ResultLayout l{};
    l.tot = (size_t)Q * slots * 8;
    l.dist = l.tot + (totals ? (size_t)Q * 8 : 0);
    l.cnt = l.dist + (size_t)Q * slots * 4;
    l.flags = l.cnt + (size_t)Q * 4;
    l.need = l.flags + (flags ? (size_t)Q * 4 : 0);
    l.grow = 4096;
    while (l.grow < l.need) l.grow *= 2;
    return l;
}

// grouped_kernels.h — grouped search over the flat index (mmiss_index_query_grouped; api_index.hip "grouped search"): the exact k
// nearest GROUPS of a query, each by its best row. What Qdrant calls group_by, Milvus grouping search, Elasticsearch collapse.
//
//   R(q)   the complete ranking of the rows q admits and that have a direction, (canonical distance, label) order;
//   group  of a row: its GROUP value (mmiss_index_set_groups), a row with -1 is a group of its own;
//   head   of a group: its first row in R(q);
// and the result is the first k heads in R(q)'s order — whatever the size of a group.
//
// The call's kernels:
//   grouped_walk    ONE launch for all queries, one workgroup of 1024 threads per query, over the query's exact ranked list L (the
//                   flat / filtered query's top-`pool`, on the device): each label becomes its row by distinct_kernel's binary
//                   search, the row's group comes from the group column; the 64-bit keys (group, position) — an ungrouped row:
//                   bit 31 and its own position as the group, which no group id equals — are sorted in LDS (probe_sort_keys);
//                   the first key of a run of equal groups is the group's smallest position, its head; heads are flagged BY
//                   POSITION, an exclusive prefix count in position order ranks them, the first k are written. One flag per
//                   query: complete = k heads found, or the list ended before the pool did (then L is all of R(q)). No atomics.
//   grouped_scan    only for the queries whose walk is not complete (one group owns the pool): subset_scan's structure and
//                   arithmetic (subset_load_piece / subset_accumulate_piece / subset_fold_step, the last three additions,
//                   x (double)inv[row] for fp8 rows, (float)(1.0 - dot): the same bits) over ALL rows, position i = row i. The
//                   final store is a 64-bit atomic minimum of the key (probe_mono(d), row) into table[q][slot], slot = the row's
//                   group, or G + row for an ungrouped row (G: the index's group high-water mark): afterwards slot s holds the
//                   head of group s, or the sentinel it was filled with. A minimum is the same in every order. A row the masks
//                   of no query of the block admit is not read; a refused row or a NaN distance stores nothing;
//   segment_topk    partition_kernels.h's selection as it is over the G + count slots, level by level; FINAL writes labels,
//                   distance bits and counts of the chunk into scratch;
//   grouped_resolve per flagged query: the selected labels back to rows (the same binary search), group[row], and everything to
//                   the query's own place in the outputs (the flagged queries run compacted).
// Plain vector stores and vector atomics only, wave64.
#pragma once
#include "subset_kernels.h"

constexpr int GROUPED_THREADS = 1024;
constexpr int GROUPED_SLOTS = 2048;   // list positions the walk's LDS state holds (pool <= 2040)
// static LDS of the walk: keys (8 B), group and head flag (4 B each) per position, and the prefix's 16 wave sums
constexpr int GROUPED_WALK_LDS = GROUPED_SLOTS * 16 + 16 * 4;

// the row of label `lab` in the strictly increasing label array, -1 if it is not stored
__device__ __forceinline__ int32_t grouped_row_of(const int64_t* __restrict__ labels, int64_t N, int64_t lab) {
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (labels[mid] < lab) lo = mid + 1; else hi = mid;
    }
    return (lo < N && labels[lo] == lab) ? (int32_t)lo : -1;
}

// ------------------------------------------------------------------------------------------------ the walk
struct GroupedWalkArgs {
    const int64_t* labels;       // [N] row -> label, strictly increasing
    int64_t N;
    const int32_t* groups;       // [N] row -> group, -1 = none; null: no row has a group
    const int64_t* list_lab;     // [Q, pool] the list stage's labels, (distance, label) order, -1 behind the count
    const float* list_dist;      // [Q, pool] ... and distance bits
    const int32_t* list_cnt;     // [Q] entries of each list
    int pool, k;
    int64_t* out_labels;         // [Q, k]
    float* out_dist;             // [Q, k]
    int32_t* out_group;          // [Q, k]
    int32_t* out_count;          // [Q]
    int32_t* out_route;          // [Q] or null: 0 here (grouped_resolve writes the 1)
    int32_t* complete;           // [Q] 1: the outputs are the result; 0: the exhaustive route has to answer (host-visible)
};

__global__ __launch_bounds__(GROUPED_THREADS) void grouped_walk_kernel(GroupedWalkArgs a) {
    __shared__ unsigned long long sk[GROUPED_SLOTS];
    __shared__ int32_t s_grp[GROUPED_SLOTS];
    __shared__ int32_t s_head[GROUPED_SLOTS];
    __shared__ int s_sum[16];
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int64_t* const ll = a.list_lab + (size_t)q * a.pool;
    const float* const ld = a.list_dist + (size_t)q * a.pool;
    int m = a.list_cnt[q];
    m = m < 0 ? 0 : (m > a.pool ? a.pool : m);
    int npow = 1;
    while (npow < m) npow <<= 1;

    for (int i = tid; i < GROUPED_SLOTS; i += GROUPED_THREADS) {
        unsigned long long key = PROBE_KEY_NONE;
        int32_t g = -1;
        if (i < m) {
            const int32_t row = grouped_row_of(a.labels, a.N, ll[i]);   // (never -1: the list is the index's own)
            if (row >= 0 && a.groups) g = a.groups[row];
            const uint32_t hi = g >= 0 ? (uint32_t)g : (0x80000000u | (uint32_t)i);
            key = ((unsigned long long)hi << 32) | (uint32_t)i;
        }
        sk[i] = key;
        s_grp[i] = g;
        s_head[i] = 0;
    }
    __syncthreads();
    probe_sort_keys(sk, npow, tid, GROUPED_THREADS);   // (the m real keys are distinct and sort in front of the padding)
    for (int j = tid; j < m; j += GROUPED_THREADS) {
        const unsigned long long key = sk[j];
        if (j == 0 || (uint32_t)(sk[j - 1] >> 32) != (uint32_t)(key >> 32)) s_head[(uint32_t)(key & 0xffffffffull)] = 1;
    }
    __syncthreads();

    // rank the heads in position order: two consecutive positions per thread, an exclusive prefix over the block
    const int i0 = 2 * tid;
    const int h0 = s_head[i0], h1 = s_head[i0 + 1];
    int heads;
    const int before = subset_block_excl(h0 + h1, s_sum, tid, &heads);
    const size_t o = (size_t)q * a.k;
    if (h0 && before < a.k) {
        a.out_labels[o + before] = ll[i0]; a.out_dist[o + before] = ld[i0]; a.out_group[o + before] = s_grp[i0];
    }
    if (h1 && before + h0 < a.k) {
        a.out_labels[o + before + h0] = ll[i0 + 1]; a.out_dist[o + before + h0] = ld[i0 + 1]; a.out_group[o + before + h0] = s_grp[i0 + 1];
    }
    const int nh = heads < a.k ? heads : a.k;
    for (int j = nh + tid; j < a.k; j += GROUPED_THREADS) {
        a.out_labels[o + j] = -1; a.out_dist[o + j] = INFINITY; a.out_group[o + j] = -1;
    }
    if (tid == 0) {
        a.out_count[q] = nh;
        if (a.out_route) a.out_route[q] = 0;
        a.complete[q] = (heads >= a.k || m < a.pool) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ the exhaustive route
struct GroupedScanArgs {
    const void* rows;             // [N, D] storage dtype
    const float* inv;             // fp8 rows: inverse norms
    const uint64_t* tags;         // [N] tag words
    const int32_t* groups;        // [N] row -> group, -1 = none; null: no row has a group
    const float* qn;              // [Q_call, D] the CALL's normalised queries
    const uint64_t* req;          // [Q_call] masks of the call, null = 0
    const uint64_t* exc;
    const int32_t* qmap;          // [Qc] the chunk's flagged queries: their index in the call
    int Qc, D;
    int N;                        // rows
    int G;                        // slots of the grouped rows; an ungrouped row r has slot G + r
    int share;                    // rows per workgroup, a multiple of 16
    unsigned long long* table;    // [Qc][stride], filled with PROBE_KEY_NONE
    int64_t stride;               // >= G + N
};

// dynamic LDS: NQB queries of D floats, then their masks (2 x NQB u64)
__host__ __device__ inline int grouped_scan_lds_bytes(int D, int nqb) { return nqb * D * 4 + nqb * 16; }

// grid = (share of the rows, block of NQB flagged queries), 256 threads: 16 groups of 16 lanes, a row per group and trip. A query
// of the block behind Qc is staged as zeros with masks that admit nothing.
template <typename T, int NQB>
__global__ __launch_bounds__(256) void grouped_scan_kernel(GroupedScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const sq = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x;
    const int p16 = tid & 15, grp = tid >> 4;
    const int D = a.D;
    uint64_t* const sreq = reinterpret_cast<uint64_t*>(smem + (size_t)NQB * D * 4);
    uint64_t* const sexc = sreq + NQB;
    const int q0 = blockIdx.y * NQB;
    const int i_begin = blockIdx.x * a.share;
    if (i_begin >= a.N) return;
    const int i_end = i_begin + a.share < a.N ? i_begin + a.share : a.N;
    for (int e = tid * 4; e < NQB * D; e += 256 * 4) {
        const int qi = e / D;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q0 + qi < a.Qc) v = *reinterpret_cast<const f32x4*>(a.qn + (size_t)a.qmap[q0 + qi] * D + (e - qi * D));
        *reinterpret_cast<f32x4*>(sq + e) = v;
    }
    if (tid < NQB) {
        uint64_t rq = ~0ull, rx = ~0ull;   // (no tag word satisfies both: a query behind Qc admits nothing)
        if (q0 + tid < a.Qc) {
            const int qo = a.qmap[q0 + tid];
            rq = a.req ? a.req[qo] : 0; rx = a.exc ? a.exc[qo] : 0;
        }
        sreq[tid] = rq; sexc[tid] = rx;
    }
    __syncthreads();
    for (int i0 = i_begin; i0 < i_end; i0 += SUBSET_ROWS_PER_TRIP) {
        const int row = i0 + grp;
        const bool in_range = row < i_end;
        uint64_t tag = 0;
        if (in_range) tag = a.tags[row];
        // the queries of the block that admit the row; a row none admits is not read
        unsigned admit = 0;
#pragma unroll
        for (int qi = 0; qi < NQB; ++qi) admit |= (unsigned)tag_admits(tag, sreq[qi], sexc[qi]) << qi;
        const bool live = in_range && admit != 0;
        const T* rv = reinterpret_cast<const T*>(a.rows) + (size_t)(live ? row : 0) * D + 4 * p16;
        double acc[NQB][4];
#pragma unroll
        for (int qi = 0; qi < NQB; ++qi) acc[qi][0] = acc[qi][1] = acc[qi][2] = acc[qi][3] = 0.0;
        for (int d0 = 0; d0 < D; d0 += 512) {
            SubsetPiece<T> piece;
            subset_load_piece<T>(rv, live, d0, D, piece);
#pragma unroll
            for (int qi = 0; qi < NQB; ++qi) subset_accumulate_piece<T>(piece, sq + (size_t)qi * D + 4 * p16, d0, D, acc[qi]);
        }
        double rinv = 1.0;
        int64_t slot = 0;
        if (live) {
            const int32_t g = a.groups ? a.groups[row] : -1;
            slot = g >= 0 ? (int64_t)g : (int64_t)a.G + row;
            if constexpr (sizeof(T) == 1) rinv = (double)a.inv[row];
        }
#pragma unroll
        for (int qi = 0; qi < NQB; ++qi) {
            subset_fold_step<8>(acc[qi]);
            subset_fold_step<4>(acc[qi]);
            subset_fold_step<2>(acc[qi]);
            subset_fold_step<1>(acc[qi]);
            const double t0 = acc[qi][0] + acc[qi][2], t1 = acc[qi][1] + acc[qi][3];
            double dot = t0 + t1;
            if constexpr (sizeof(T) == 1) {
                if (live) dot = dot * rinv;
            }
            const float d = (float)(1.0 - dot);
            if (p16 == 0 && live && ((admit >> qi) & 1u) && d == d && slot < a.stride) {
                const unsigned long long key = ((unsigned long long)probe_mono(d) << 32) | (unsigned)row;
                unsigned long long* const at = a.table + (size_t)(q0 + qi) * a.stride + slot;
                // A slot only ever falls, so a key that does not beat what a plain load sees — however stale — cannot beat the
                // slot: the atomic is skipped. A group of 400 000 rows sends a few dozen atomics to its one address, not 400 000
                // (1M x 512 f16, Q = 1, 40 % of the rows in one group: the scan took 4.65 ms with an atomic per row).
                if (key < __builtin_nontemporal_load(at)) atomicMin(at, key);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ resolve
struct GroupedResolveArgs {
    const int64_t* labels;       // [N]
    int64_t N;
    const int32_t* groups;       // [N] or null
    const int32_t* qmap;         // [Qc]
    const int64_t* sel_labels;   // [Qc, k] segment_topk's FINAL outputs for the chunk
    const float* sel_dist;       // [Qc, k]
    const int32_t* sel_count;    // [Qc]
    int k;
    int64_t* out_labels; float* out_dist; int32_t* out_group; int32_t* out_count; int32_t* out_route;   // the call's
};

// grid = the chunk's flagged queries, 256 threads
__global__ __launch_bounds__(256) void grouped_resolve_kernel(GroupedResolveArgs a) {
    const int qc = blockIdx.x, qo = a.qmap[qc];
    for (int j = threadIdx.x; j < a.k; j += 256) {
        const int64_t lab = a.sel_labels[(size_t)qc * a.k + j];
        int32_t g = -1;
        if (lab >= 0 && a.groups) {
            const int32_t row = grouped_row_of(a.labels, a.N, lab);
            if (row >= 0) g = a.groups[row];
        }
        a.out_labels[(size_t)qo * a.k + j] = lab;
        a.out_dist[(size_t)qo * a.k + j] = a.sel_dist[(size_t)qc * a.k + j];
        a.out_group[(size_t)qo * a.k + j] = g;
    }
    if (threadIdx.x == 0) {
        a.out_count[qo] = a.sel_count[qc];
        if (a.out_route) a.out_route[qo] = 1;
    }
}

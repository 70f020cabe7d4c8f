// partition_kernels.h — partitioned (inverted-file) search over the flat index (mmiss_index_partition_set, mmiss_index_query_probed;
// api_index.hip "partitioned search"): the rows are grouped by the k-means cell mmiss_index_assign gave them, a query reads only
// the rows of the `nprobe` cells whose centres are nearest to it, plus the rows added since the partition was set (the tail).
// What chromadb answers above 100 rows from an approximate HNSW graph (backend/app/utils.py:127-130, backend/app/main.py:761-765).
//
// The approximation is only WHICH rows are looked at, and that set is defined exactly:
//   dc[c]   = the canonical distance of the normalised query to the normalised centre c, the centre treated as an f32 row
//             (canon_partial_dots<float>: the additions of every other distance here, in their order);
//   P(q)    = the min(nprobe, live centres) centres smallest by (dc[c], c) among those whose dc[c] is not NaN;
//   cand(q) = the rows of the cells of P(q), and every tail row.
// Within cand(q) the result is the exact top-k by (canonical distance, row): there is no approximate pass and no guard, every
// candidate gets its canonical distance directly (the candidates are a few percent of the index).
//
// A call's kernels, no host round trip between them:
//   probe_select   one workgroup per query: the C distances dc, a sort of the (dc, c) keys in LDS, the probed cells, each cell's
//                  offset inside the query's candidate area (a prefix sum over the probed sizes) and the query's total;
//   list_scan      grid (share of a list, probe slot, query): four rows per wave, 16 lanes per row as canonical_scan_kernel, but
//                  row = order[i] (a gather of whole rows); the tag word is checked against the query's masks; one 64-bit key
//                  (monotone map of the distance bits, row) per candidate goes to the candidate area — a refused row or a NaN
//                  distance as the sentinel that sorts last. The tail is one more slot whose list is a contiguous range;
//   segment_topk   one workgroup sorts a segment of up to PROBE_SEG keys of one query in LDS and writes its k best; applied
//                  level by level (ping-pong) while a query has more than one segment. The last level (one segment per query)
//                  writes labels, distance bits, counts and the scanned rows itself (FINAL) instead of handing k keys to one
//                  more small kernel: one launch less on the single-query path.
// Row order is label order, so (distance, row) is the (distance, label) order of mmiss_index_query. Keys of real candidates are
// distinct (the row is part of the key), so the sorted order has one value whatever the network does with equal sentinels.
// Every position of a query's candidate area below its total is written by list_scan before segment_topk reads it: nothing of an
// earlier call survives there. Plain vector stores only.
#pragma once
#include "retrieval_kernels.h"

constexpr int PROBE_SEG = 4096;                      // keys per segment: 32 KB of LDS
constexpr int PROBE_MAX_CENTRES = 1024;
#define PROBE_KEY_NONE 0xffffffffffffffffull         // refused row / NaN distance / padding: sorts last, never delivered

// float bits -> unsigned, increasing with the float (NaN never comes here); and back
__device__ __forceinline__ uint32_t probe_mono(float d) {
    const uint32_t b = __float_as_uint(d);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float probe_unmono(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// ascending block bitonic sort of npow (a power of two) 64-bit keys in LDS; ends with the block synchronised
__device__ __forceinline__ void probe_sort_keys(unsigned long long* sk, int npow, int tid, int nthreads) {
    for (int k = 2; k <= npow; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npow; i += nthreads) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long a = sk[i], b = sk[p];
                    const bool up = (i & k) == 0;
                    if (up ? (b < a) : (a < b)) { sk[i] = b; sk[p] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// the canonical distance of one row (16 lanes: p16 = lane & 15) — rerank_kernel's arithmetic: the same shuffles, the same last
// three additions, fp8 rows x (double)inv: the same bits. Valid in every lane of the row's 16.
template <typename T>
__device__ __forceinline__ float probe_canon_distance(const T* rv, bool live, const float* qp, int D, const float* inv, int64_t row) {
    double acc[4];
    canon_partial_dots<T>(rv, live, qp, D, acc);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], o);
    }
    const double t0 = acc[0] + acc[2], t1 = acc[1] + acc[3];
    double dot = t0 + t1;
    if constexpr (sizeof(T) == 1) {
        if (live) dot = dot * (double)inv[row];
    }
    return (float)(1.0 - dot);
}

// ------------------------------------------------------------------------------------------------ building a partition
// live[c] = 1 iff the normalised centre c has a direction (no NaN among its elements: a zero, NaN or infinite centre normalises
// to a row with a NaN, and its distance to any query is NaN). One wave per centre.
__global__ __launch_bounds__(256) void partition_live_kernel(const float* __restrict__ cn, int C, int D, int32_t* __restrict__ live) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    bool nan = false;
    for (int d = lane; d < D; d += 64) {
        const float v = cn[(size_t)c * D + d];
        nan = nan || v != v;
    }
    const uint64_t any = __ballot(nan);
    if (lane == 0) live[c] = any ? 0 : 1;
}

// The scatter of the counting sort: order[off[c] ..) <- the rows r < B with cells[r] == c (entries outside 0 .. C-1: no cell).
// cursor[c] starts at off[c]. A block ranks its PART_FILL_ROWS rows per cell in LDS, reserves every cell's run with one global
// atomic and writes the rows behind it: the order inside a cell is that of the atomics, and no result depends on it.
constexpr int PART_FILL_ITEMS = 8, PART_FILL_ROWS = 256 * PART_FILL_ITEMS;
__global__ __launch_bounds__(256) void partition_fill_kernel(const int32_t* __restrict__ cells, int64_t B, int C, int32_t* __restrict__ cursor,
                                                             int32_t* __restrict__ order) {
    __shared__ int h[PROBE_MAX_CENTRES];
    __shared__ int base[PROBE_MAX_CENTRES];
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) h[c] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * PART_FILL_ROWS;
    int cell[PART_FILL_ITEMS], rank[PART_FILL_ITEMS];
#pragma unroll
    for (int i = 0; i < PART_FILL_ITEMS; ++i) {
        const int64_t r = r0 + i * 256 + tid;
        cell[i] = -1;
        rank[i] = 0;
        if (r < B) {
            const int c = cells[r];
            if (c >= 0 && c < C) { cell[i] = c; rank[i] = atomicAdd(&h[c], 1); }
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) base[c] = h[c] ? atomicAdd(cursor + c, h[c]) : 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PART_FILL_ITEMS; ++i)
        if (cell[i] >= 0) order[base[cell[i]] + rank[i]] = (int32_t)(r0 + i * 256 + tid);
}

// ------------------------------------------------------------------------------------------------ probe selection
struct ProbeSelectArgs {
    const float* qn;        // [Q, D] canonical-normalised queries (prep_queries_kernel), the chunk's first
    const float* cn;        // [C, D] normalised centres
    const int32_t* off;     // [C + 1] cell offsets into order
    int C, D;
    int NP;                 // probe slots of the call: min(nprobe, C)
    int tail;               // rows behind the partition's B
    int32_t* probe_cell;    // [Q, NP] the probed cells, nearest first; -1 behind the live centres
    int32_t* probe_base;    // [Q, NP + 1] where each slot's keys start inside the query's candidate area; slot NP: the tail
    int32_t* total;         // [Q] keys of the query: probed sizes + tail; 0 for a query without a direction
};

// One workgroup of 1024 threads per query (a single query is the case that matters, and 16 waves take 64 centres per trip where 4
// took 16: the trips are dependent memory round trips). The C distances with canon_partial_dots<float> (16 lanes per centre, four
// centres per wave), their keys (monotone distance bits, centre) sorted in LDS — a NaN distance as the sentinel: a centre without a
// direction is never probed, and a query without one has no live centre at all —, then the prefix sum of the probed cells' sizes
// (the first 256 threads).
__global__ __launch_bounds__(1024) void probe_select_kernel(ProbeSelectArgs a) {
    __shared__ unsigned long long sk[PROBE_MAX_CENTRES];
    __shared__ int ssz[PROBE_MAX_CENTRES];
    __shared__ int spart[256];
    __shared__ int s_live;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p16 = lane & 15, sub = lane >> 4;
    const int q = blockIdx.x;
    int npow = 1;
    while (npow < a.C) npow <<= 1;
    for (int i = tid; i < npow; i += 1024) sk[i] = PROBE_KEY_NONE;
    if (tid == 0) s_live = 0;
    __syncthreads();
    const float* qp = a.qn + (size_t)q * a.D + 4 * p16;
    for (int c0 = wave * 4; c0 < a.C; c0 += 64) {
        const int c = c0 + sub;
        const bool live = c < a.C;
        const float* rv = a.cn + (size_t)(live ? c : 0) * a.D + 4 * p16;
        const float d = probe_canon_distance<float>(rv, live, qp, a.D, nullptr, 0);
        if (p16 == 0 && live && d == d) sk[c] = ((unsigned long long)probe_mono(d) << 32) | (unsigned)c;
    }
    __syncthreads();
    probe_sort_keys(sk, npow, tid, 1024);
    int mine = 0;
    for (int i = tid; i < a.C; i += 1024) mine += sk[i] != PROBE_KEY_NONE;
    if (mine) atomicAdd(&s_live, mine);
    __syncthreads();
    const int np = s_live < a.NP ? s_live : a.NP;   // (the live keys are the first s_live of the sorted order)
    for (int i = tid; i < PROBE_MAX_CENTRES; i += 1024) {
        int sz = 0;
        if (i < np) {
            const int c = (int)(sk[i] & 0xffffffffull);
            sz = a.off[c + 1] - a.off[c];
        }
        ssz[i] = sz;
    }
    __syncthreads();
    // exclusive prefix over the (up to 1024) probed sizes: four per thread, then the 256 partial sums
    const bool scans = tid < 256;
    int loc[4] = {0, 0, 0, 0}, s = 0;
    if (scans) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { loc[j] = s; s += ssz[4 * tid + j]; }
        spart[tid] = s;
    }
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = (scans && tid >= o) ? spart[tid - o] : 0;
        __syncthreads();
        if (scans) spart[tid] += v;
        __syncthreads();
    }
    const int excl = scans ? spart[tid] - s : 0, cells_total = spart[255];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = 4 * tid + j;
        if (scans && i < a.NP) {
            a.probe_cell[(size_t)q * a.NP + i] = i < np ? (int)(sk[i] & 0xffffffffull) : -1;
            a.probe_base[(size_t)q * (a.NP + 1) + i] = i < np ? excl + loc[j] : cells_total;
        }
    }
    if (tid == 0) {
        a.probe_base[(size_t)q * (a.NP + 1) + a.NP] = cells_total;
        a.total[q] = np > 0 ? cells_total + a.tail : 0;
    }
}

// ------------------------------------------------------------------------------------------------ list scan
struct ListScanArgs {
    const void* rows;             // [count, D] storage dtype
    const float* inv;             // fp8 rows: inverse norms
    const uint64_t* tags;         // [count] tag words
    const float* qn;              // [Q, D] the chunk's normalised queries
    const uint64_t* req;          // [Q] masks of the chunk, null = 0
    const uint64_t* exc;
    const int32_t* order;         // rows grouped by cell
    const int32_t* off;           // [C + 1]
    const int32_t* probe_cell;    // [Q, NP]
    const int32_t* probe_base;    // [Q, NP + 1]
    const int32_t* total;         // [Q]
    int D, NP;
    int share;                    // rows of a list per workgroup, a multiple of 16
    int64_t B;                    // the partition's rows; the tail is [B, B + tail)
    int tail;
    unsigned long long* keys;     // [Q][stride] candidate areas
    int64_t stride;
};

// grid = (share of a list, probe slot — NP: the tail —, query). A workgroup past its list's end, of an unprobed slot or of a query
// without a direction exits. Every key position of the list's share is written: admitted rows with a distance as (distance, row),
// the others as the sentinel.
template <typename T>
__global__ __launch_bounds__(256) void list_scan_kernel(ListScanArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p16 = lane & 15, sub = lane >> 4;
    const int slot = blockIdx.y, q = blockIdx.z;
    if (a.total[q] == 0) return;
    int n;
    int64_t first = 0;          // tail: its first row; a cell: its offset into order
    const bool is_tail = slot == a.NP;
    if (is_tail) { n = a.tail; first = a.B; }
    else {
        const int c = a.probe_cell[(size_t)q * a.NP + slot];
        if (c < 0) return;
        first = a.off[c];
        n = a.off[c + 1] - (int)first;
    }
    const int i_begin = blockIdx.x * a.share;
    if (i_begin >= n) return;
    const int i_end = i_begin + a.share < n ? i_begin + a.share : n;
    const uint64_t rq = a.req ? a.req[q] : 0, rx = a.exc ? a.exc[q] : 0;
    const float* qp = a.qn + (size_t)q * a.D + 4 * p16;
    unsigned long long* out = a.keys + (size_t)q * a.stride + a.probe_base[(size_t)q * (a.NP + 1) + slot];
    for (int i0 = i_begin + wave * 4; i0 < i_end; i0 += 16) {
        const int i = i0 + sub;
        const bool live = i < i_end;
        int64_t row = 0;
        if (live) row = is_tail ? first + i : (int64_t)a.order[first + i];
        const T* rv = reinterpret_cast<const T*>(a.rows) + (size_t)row * a.D + 4 * p16;
        const float d = probe_canon_distance<T>(rv, live, qp, a.D, a.inv, row);
        if (p16 == 0 && live) {
            const bool ok = d == d && tag_admits(a.tags[row], rq, rx);
            out[i] = ok ? (((unsigned long long)probe_mono(d) << 32) | (unsigned)row) : PROBE_KEY_NONE;
        }
    }
}

// ------------------------------------------------------------------------------------------------ selection
struct SegmentTopkArgs {
    const unsigned long long* in;   // [Q][in_stride]
    unsigned long long* out;        // [Q][out_stride]; segment s writes [s k, s k + k)   (not FINAL)
    int64_t in_stride, out_stride;
    const int32_t* total;           // [Q] keys at level 0
    int level;                      // keys of query q at this level: total[q], `level` times n -> ceil(n / PROBE_SEG) k
    int k;
    // FINAL: the one segment left per query -> the call's outputs (q0 = the chunk's first query)
    const int64_t* labels;
    int64_t* out_labels; float* out_dist; int32_t* out_count; int64_t* out_scanned;
};

// grid = (segments, queries), 1024 threads. A segment past its query's keys exits (FINAL: there is exactly one, and it always
// writes). The segment is padded with the sentinel to the power of two its own count needs, sorted, and its first k entries
// written — sentinels where it has fewer.
template <bool FINAL>
__global__ __launch_bounds__(1024) void segment_topk_kernel(SegmentTopkArgs a) {
    __shared__ unsigned long long sk[PROBE_SEG];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int q = blockIdx.y, s = blockIdx.x;
    int64_t n = a.total[q];
    for (int l = 0; l < a.level; ++l) n = (n + PROBE_SEG - 1) / PROBE_SEG * a.k;
    const int64_t k0 = (int64_t)s * PROBE_SEG;
    if (!FINAL && k0 >= n) return;
    int cnt = (int)(n - k0 < PROBE_SEG ? n - k0 : PROBE_SEG);   // (FINAL: n <= PROBE_SEG by the host's level count)
    if (cnt < 0) cnt = 0;
    int npow = 1;
    while (npow < cnt) npow <<= 1;
    const unsigned long long* src = a.in + (size_t)q * a.in_stride + k0;
    for (int i = tid; i < npow; i += 1024) sk[i] = i < cnt ? src[i] : PROBE_KEY_NONE;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    probe_sort_keys(sk, npow, tid, 1024);
    if constexpr (!FINAL) {
        unsigned long long* dst = a.out + (size_t)q * a.out_stride + (size_t)s * a.k;
        for (int i = tid; i < a.k; i += 1024) dst[i] = i < npow ? sk[i] : PROBE_KEY_NONE;
    } else {
        int mine = 0;
        for (int i = tid; i < a.k; i += 1024) {
            const unsigned long long key = i < npow ? sk[i] : PROBE_KEY_NONE;
            const bool ok = key != PROBE_KEY_NONE;
            a.out_labels[(size_t)q * a.k + i] = ok ? a.labels[(uint32_t)(key & 0xffffffffull)] : -1;
            a.out_dist[(size_t)q * a.k + i] = ok ? probe_unmono((uint32_t)(key >> 32)) : INFINITY;
            mine += ok;
        }
        if (mine) atomicAdd(&s_cnt, mine);
        __syncthreads();
        if (tid == 0) {
            a.out_count[q] = s_cnt;
            if (a.out_scanned) a.out_scanned[q] = a.total[q];
        }
    }
}

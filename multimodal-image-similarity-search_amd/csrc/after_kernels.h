// after_kernels.h — search after (mmiss_index_query_after; api_index.hip "search after"): the exact next k of a query's ranking
// behind a cursor (distance, label), and the number of rows still to come. The ranking is the flat query's: canonical distance
// bits, ties by label; row order is label order, so behind the distance test the label test is a row test.
//
//   A(q) = { r < count : listed (when there is a list), tag_admits, d not NaN, d <= max_dist[q],
//            mono(d) > mono(after_dist[q])  or  mono(d) == mono(after_dist[q]) and r >= first_row[q] }
// with first_row[q] the first row whose label exceeds after_label[q]. The result is the first k of A(q) by (d, row);
// remaining[q] = |A(q)|.
//
// A call's kernels, no host round trip between them; the host sizes everything from count, or min(n_cand, count) with a list:
//   after_resolve   one thread per query: first_row[q] by binary search in the label array, the cursor as the scan reads it
//                   (AfterCursor), remaining[q] = 0, and — dense calls — total[q] = count for the queries of a chunk;
//   subset_mark / _count / _offsets / _scatter   only with a list: subset_kernels.h's stages as they are -> rows[], total = |S|;
//   after_scan      subset_scan's structure and arithmetic (subset_load_piece / subset_accumulate_piece / subset_fold_step: the
//                   same operands, the same additions, the same bits). DENSE: position i is row i, consecutive rows per trip;
//                   otherwise row = list[i]. One key (probe_mono(d), row) per (query, position), the sentinel for a position
//                   that is not in A(q). Every position below the total is written; no row at or past count is read. A
//                   workgroup adds its admitted positions per query to remaining[q]: one atomicAdd per (workgroup, query);
//   segment_topk    partition_kernels.h's selection as it is; FINAL writes labels, distance bits and counts.
// Plain vector stores and vector atomics only, wave64.
#pragma once
#include "subset_kernels.h"

// the cursor of one query as the scan tests it: a key ranks behind it iff
//   m > mono  or  (m == mono and row >= first_row),   and the distance passes  d <= max_dist
// The start of the ranking (after_dist = -inf) is (probe_mono(-inf), 0): every distance passes. A NaN after_dist or max_dist is
// max_dist = NaN: nothing passes.
struct AfterCursor {
    uint32_t mono;
    int32_t first_row;
    float max_dist;
    int32_t pad;
};

// one thread per query. total / nq: the dense call's totals of a chunk (null: a listed call, subset_offsets writes them)
__global__ __launch_bounds__(256) void after_resolve_kernel(const float* __restrict__ after_dist, const int64_t* __restrict__ after_label,
                                                            const float* __restrict__ max_dist, const int64_t* __restrict__ labels, int64_t N,
                                                            int Q, AfterCursor* __restrict__ cur, unsigned long long* __restrict__ remaining,
                                                            int32_t* __restrict__ total, int nq) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const float ad = after_dist[q];
    const int64_t lab = after_label[q];
    int64_t lo = 0, hi = N;   // the first row whose label exceeds lab
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (labels[mid] <= lab) lo = mid + 1; else hi = mid;
    }
    AfterCursor c;
    c.mono = probe_mono(ad);
    c.first_row = (int32_t)lo;
    c.max_dist = max_dist ? max_dist[q] : INFINITY;
    c.pad = 0;
    if (ad == -INFINITY) c.first_row = 0;                      // the start of the ranking, whatever the label
    if (ad != ad) c.max_dist = __uint_as_float(0x7fc00000u);   // a NaN cursor admits nothing
    cur[q] = c;
    remaining[q] = 0ull;
    if (total && q < nq) total[q] = (int32_t)N;
}

struct AfterScanArgs {
    SubsetScanArgs s;                 // list: null for the dense scan
    const AfterCursor* cur;           // [Q] the chunk's cursors
    unsigned long long* remaining;    // [Q] += the positions admitted
};

// grid = (share of the positions, block of NQB queries), 256 threads: 16 groups of 16 lanes, a position per group and trip.
// A workgroup past the total exits. A query of the block behind Q is staged as zeros, writes nothing and counts nothing.
template <typename T, int NQB, bool DENSE>
__global__ __launch_bounds__(256) void after_scan_kernel(AfterScanArgs aa) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const sq = reinterpret_cast<float*>(smem);
    const SubsetScanArgs& a = aa.s;
    const int tid = threadIdx.x;
    const int p16 = tid & 15, grp = tid >> 4;
    const int D = a.D;
    const int q0 = blockIdx.y * NQB;
    const int n = a.total[q0];   // (the positions: the same for every query)
    const int i_begin = blockIdx.x * a.share;
    if (i_begin >= n) return;
    const int i_end = i_begin + a.share < n ? i_begin + a.share : n;
    for (int e = tid * 4; e < NQB * D; e += 256 * 4) {
        const int qi = e / D;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q0 + qi < a.Q) v = *reinterpret_cast<const f32x4*>(a.qn + (size_t)q0 * D + e);
        *reinterpret_cast<f32x4*>(sq + e) = v;
    }
    __syncthreads();
    int admitted[NQB];
#pragma unroll
    for (int qi = 0; qi < NQB; ++qi) admitted[qi] = 0;
    for (int i0 = i_begin; i0 < i_end; i0 += SUBSET_ROWS_PER_TRIP) {
        const int i = i0 + grp;
        const bool live = i < i_end;
        int64_t row = 0;
        if (live) {
            if constexpr (DENSE) row = i; else row = (int64_t)a.list[i];
        }
        const T* rv = reinterpret_cast<const T*>(a.rows) + (size_t)row * D + 4 * p16;
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
        uint64_t tag = 0;
        if (live) {
            tag = a.tags[row];
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
            const int q = q0 + qi;
            if (p16 == 0 && live && q < a.Q) {
                const uint64_t rq = a.req ? a.req[q] : 0, rx = a.exc ? a.exc[q] : 0;
                const AfterCursor c = aa.cur[q];
                const uint32_t m = probe_mono(d);
                const bool behind = m > c.mono || (m == c.mono && (int32_t)row >= c.first_row);
                const bool ok = d == d && tag_admits(tag, rq, rx) && d <= c.max_dist && behind;
                a.keys[(size_t)q * a.stride + i] = ok ? (((unsigned long long)m << 32) | (unsigned)row) : PROBE_KEY_NONE;
                admitted[qi] += ok;
            }
        }
    }
    // the workgroup's admitted positions per query: the groups' counts (lane 0 of each 16) summed over the wave, the four waves'
    // sums through LDS (the staged queries are done with), one atomicAdd per query
    __syncthreads();
    int* const sc = reinterpret_cast<int*>(smem);
#pragma unroll
    for (int qi = 0; qi < NQB; ++qi) {
        int v = admitted[qi];
#pragma unroll
        for (int o = 32; o >= 16; o >>= 1) v += __shfl_xor(v, o);
        if (tid == 0 || tid == 64 || tid == 128 || tid == 192) sc[(tid >> 6) * NQB + qi] = v;
    }
    __syncthreads();
    if (tid < NQB && q0 + tid < a.Q) {
        const int v = sc[tid] + sc[NQB + tid] + sc[2 * NQB + tid] + sc[3 * NQB + tid];
        if (v) atomicAdd(aa.remaining + q0 + tid, (unsigned long long)v);
    }
}

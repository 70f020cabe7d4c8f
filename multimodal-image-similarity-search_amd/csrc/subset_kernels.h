// subset_kernels.h — subset search over the flat index (mmiss_index_query_subset; api_index.hip "subset search"): the exact top-k
// among the rows whose labels a caller lists. What chromadb answers with collection.query(where=..., ids=...).
//
//   S = { r < count : labels[r] is in the caller's list }   (an unknown label is ignored, a repeated one counts once, the order of
//                                                            the list means nothing)
// and the result of query q is the exact top-k by (canonical distance, row) among the rows of S its masks admit: the distance bits
// and the order of mmiss_index_query. One list serves every query of the call.
//
// A call's kernels, no host round trip between them; the host sizes everything from the bound min(n_cand, count), the kernels read
// the real |S| from device memory and workgroups past it exit:
//   subset_mark     one thread per list entry: its row by binary search in the label array (row order is label order:
//                   distinct_kernel's lookup), the row's bit set in a bitmap of one bit per row (cleared on the stream before) by
//                   an atomicOr. A miss sets nothing; duplicates collapse here;
//   subset_count    per block of SUBSET_BLOCK_ROWS rows: the popcount of its bitmap words;
//   subset_offsets  ONE workgroup: the exclusive prefix of the block counts (a serial carry over trips of 1024 blocks), and
//                   total[q] = |S| for every query of a chunk;
//   subset_scatter  per block again: the prefix of its words' popcounts, then rows[] ascending. No workgroup waits on another:
//                   the three launches are the only ordering;
//   subset_scan     grid (share of rows[], block of NQB queries; NQB: the plan's query block, narrowed to the queries a chunk
//                   has): the block's normalised queries staged once in LDS; each group of 16 lanes takes a listed row and
//                   scores it against EVERY query of the block. The row's bytes are loaded
//                   once per 512-element piece into registers (subset_load_piece) and every query accumulates from them
//                   (subset_accumulate_piece): canon_partial_dots cut in its two halves, the additions of each query in
//                   canon_partial_dots' order, then the folds (the lane ^ 8, 4, 2, 1 exchanges as DPP moves), the last three additions, x (double)inv[row] for fp8 rows and
//                   (float)(1.0 - dot) of probe_canon_distance: the same bits. One 64-bit key (probe_mono(d), row) per (query,
//                   position) — the sentinel for a NaN distance or a row tag_admits refuses. Every position below |S| is written;
//   segment_topk    partition_kernels.h's selection as it is, level by level; FINAL writes labels, distance bits, counts and
//                   total[q] = |S| (out_matched).
// Plain vector stores only, wave64.
#pragma once
#include "partition_kernels.h"

constexpr int SUBSET_BLOCK_THREADS = 1024;
constexpr int SUBSET_BLOCK_ROWS = SUBSET_BLOCK_THREADS * 32;   // rows of one block of the compaction: a 32-bit word per thread
constexpr int SUBSET_ROWS_PER_TRIP = 16;                       // rows a scan workgroup of 256 threads takes per trip

// ------------------------------------------------------------------------------------------------ resolve and mark
__global__ __launch_bounds__(256) void subset_mark_kernel(const int64_t* __restrict__ cand, int64_t n_cand, const int64_t* __restrict__ labels,
                                                          int64_t N, uint32_t* __restrict__ bitmap) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cand) return;
    const int64_t lab = cand[i];
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (labels[mid] < lab) lo = mid + 1; else hi = mid;
    }
    if (lo < N && labels[lo] == lab) atomicOr(bitmap + (lo >> 5), 1u << (lo & 31));
}

// ------------------------------------------------------------------------------------------------ compact
// the block's sum of v in every thread; ends with the block synchronised (s: 16 ints of LDS)
__device__ __forceinline__ int subset_block_sum(int v, int* s, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // (s may still be read from an earlier use)
    if ((tid & 63) == 0) s[tid >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < SUBSET_BLOCK_THREADS / 64; ++w) t += s[w];
    return t;
}

// the exclusive prefix of v over the block's threads (s: 16 ints of LDS); *sum: the block's total
__device__ __forceinline__ int subset_block_excl(int v, int* s, int tid, int* sum) {
    const int lane = tid & 63, wave = tid >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) s[wave] = inc;
    __syncthreads();
    int before = 0, t = 0;
#pragma unroll
    for (int w = 0; w < SUBSET_BLOCK_THREADS / 64; ++w) {
        const int c = s[w];
        if (w < wave) before += c;
        t += c;
    }
    *sum = t;
    return before + inc - v;
}

__global__ __launch_bounds__(SUBSET_BLOCK_THREADS) void subset_count_kernel(const uint32_t* __restrict__ bitmap, int64_t nwords,
                                                                            int32_t* __restrict__ block_cnt) {
    __shared__ int s[16];
    const int tid = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * SUBSET_BLOCK_THREADS + tid;
    const int c = w < nwords ? __popc(bitmap[w]) : 0;
    const int t = subset_block_sum(c, s, tid);
    if (tid == 0) block_cnt[blockIdx.x] = t;
}

// one workgroup: block_cnt -> its exclusive prefix in place, total[0 .. nq) = the sum
__global__ __launch_bounds__(SUBSET_BLOCK_THREADS) void subset_offsets_kernel(int32_t* __restrict__ block_cnt, int nblocks, int32_t* __restrict__ total,
                                                                              int nq) {
    __shared__ int s[16];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < nblocks; b0 += SUBSET_BLOCK_THREADS) {
        const int b = b0 + tid;
        const int c = b < nblocks ? block_cnt[b] : 0;
        int sum;
        const int ex = subset_block_excl(c, s, tid, &sum);
        if (b < nblocks) block_cnt[b] = carry + ex;
        carry += sum;
    }
    for (int q = tid; q < nq; q += SUBSET_BLOCK_THREADS) total[q] = carry;
}

// rows[block_off[b] ..) <- the rows of block b whose bit is set, ascending (cap: the entries rows[] holds — |S| never exceeds it)
__global__ __launch_bounds__(SUBSET_BLOCK_THREADS) void subset_scatter_kernel(const uint32_t* __restrict__ bitmap, int64_t nwords,
                                                                              const int32_t* __restrict__ block_off, int32_t* __restrict__ rows,
                                                                              int64_t cap) {
    __shared__ int s[16];
    const int tid = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * SUBSET_BLOCK_THREADS + tid;
    uint32_t bits = w < nwords ? bitmap[w] : 0u;
    int sum;
    int64_t at = (int64_t)block_off[blockIdx.x] + subset_block_excl(__popc(bits), s, tid, &sum);
    while (bits) {
        const int b = __ffs((int)bits) - 1;
        bits &= bits - 1;
        if (at < cap) rows[at] = (int32_t)(w * 32 + b);
        ++at;
    }
}

// ------------------------------------------------------------------------------------------------ scan
// canon_partial_dots in two halves, so that one load of a row's piece serves every query of a block. A piece: the (up to) eight
// 64-element slices of 512 consecutive elements, lane p of a row's 16 holding elements 4p .. 4p + 3 of each slice.
template <typename T> struct SubsetPiece {
    typedef typename std::conditional<sizeof(T) == 1, uint32_t, typename std::conditional<sizeof(T) == 2, u32x2, f32x4>::type>::type piece_t;
    piece_t w[8];
};

// the load half: rv = the lane's first element of the row; a slice past D, or of a row that is not live, is zero
template <typename T>
__device__ __forceinline__ void subset_load_piece(const T* rv, bool live, int d0, int D, SubsetPiece<T>& p) {
    typedef typename SubsetPiece<T>::piece_t piece_t;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        p.w[u] = piece_t{};   // (zero: fp8 code 0 = +0.0)
        if (live && d0 + 64 * u < D) p.w[u] = *reinterpret_cast<const piece_t*>(rv + d0 + 64 * u);
    }
}

// the accumulate half: qp = the lane's first element of the query (LDS); the multiply-adds of canon_partial_dots, in its order
template <typename T>
__device__ __forceinline__ void subset_accumulate_piece(const SubsetPiece<T>& p, const float* qp, int d0, int D, double (&acc)[4]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (d0 + 64 * u < D) {
            const f32x4 qq = *reinterpret_cast<const f32x4*>(qp + d0 + 64 * u);
            float rr[4];
            if constexpr (sizeof(T) == 1) {
                f8x4_values(p.w[u], rr);
            } else if constexpr (sizeof(T) == 2) {
                const _Float16* h = reinterpret_cast<const _Float16*>(&p.w[u]);
#pragma unroll
                for (int j = 0; j < 4; ++j) rr[j] = (float)h[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) rr[j] = p.w[u][j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] + (double)qq[j] * (double)rr[j];
        }
    }
}

// One stage of probe_canon_distance's fold, acc[j] = acc[j] + (acc[j] of lane ^ J), J = 8, 4, 2, 1: the value __shfl_xor(acc[j], J)
// returns, fetched by DPP moves inside the row of 16 lanes (lane_xor: the wave sort's exchange) instead of two ds_bpermute per
// double — with 16 queries a trip has 512 of them, on the LDS pipe the staged queries are read through. Every lane of the wave is
// active here. The same operands, the same additions: the same bits.
template <int J>
__device__ __forceinline__ void subset_fold_step(double (&acc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double other = __hiloint2double(lane_xor<J>(__double2hiint(acc[j])), lane_xor<J>(__double2loint(acc[j])));
        acc[j] = acc[j] + other;
    }
}

struct SubsetScanArgs {
    const void* rows;             // [count, D] storage dtype
    const float* inv;             // fp8 rows: inverse norms
    const uint64_t* tags;         // [count] tag words
    const float* qn;              // [Q, D] the chunk's normalised queries
    const uint64_t* req;          // [Q] masks of the chunk, null = 0
    const uint64_t* exc;
    const int32_t* list;          // [|S|] the listed rows, ascending
    const int32_t* total;         // [Q] |S|
    int Q, D;
    int share;                    // list positions per workgroup, a multiple of 16
    unsigned long long* keys;     // [Q][stride]
    int64_t stride;
};

// dynamic LDS: NQB queries of D floats
__host__ __device__ inline int subset_scan_lds_bytes(int D, int nqb) { return nqb * D * 4; }

// grid = (share of the list, block of NQB queries), 256 threads: 16 groups of 16 lanes, a listed row per group and trip. A
// workgroup past |S| exits. A query of the block behind Q is staged as zeros and writes nothing.
template <typename T, int NQB>
__global__ __launch_bounds__(256) void subset_scan_kernel(SubsetScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const sq = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x;
    const int p16 = tid & 15, grp = tid >> 4;
    const int D = a.D;
    const int q0 = blockIdx.y * NQB;
    const int n = a.total[q0];   // (|S|: the same for every query)
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
    for (int i0 = i_begin; i0 < i_end; i0 += SUBSET_ROWS_PER_TRIP) {
        const int i = i0 + grp;
        const bool live = i < i_end;
        const int64_t row = live ? (int64_t)a.list[i] : 0;
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
                const bool ok = d == d && tag_admits(tag, rq, rx);
                a.keys[(size_t)q * a.stride + i] = ok ? (((unsigned long long)probe_mono(d) << 32) | (unsigned)row) : PROBE_KEY_NONE;
            }
        }
    }
}

// distinct_kernels.h — the suppression stage of mmiss_index_query_distinct (api_index.hip "distinct results"): a greedy walk over
// a query's exact ranked list L (the flat, filtered or probed top-`pool`, already on the device) that keeps an entry unless an
// earlier KEPT entry lies within min_sep of it, and stops after k kept ones.
//
// sep(s, i) is the canonical distance mmiss_index_query_radius_by_label defines with the row of L[s] as the query: the represented
// row (fp8: values x inverse norm, one f32 multiply — rows_as_queries_kernel), normalised as every query is (prep_queries_kernel:
// y = float(double(x) / sqrt(canon_sumsq(x)))), against the stored row of L[i] by canon_partial_dots, the folds and the last three
// additions of rerank_kernel, x (double)inv[row] for fp8 rows, dist = (float)(1.0 - dot). No approximate score, no guard: every
// comparison is `dist <= min_sep` on those bits.
//
// One workgroup of 1024 threads per query, ONE launch for all queries of a call, no host round trip between rounds. A round:
//   the next kept position = the first one without an owner behind the last kept one (every wave finds it by itself from the
//   same LDS state: ballots over 64 positions at a time, no atomic, no extra barrier);
//   its represented row is widened into LDS, every wave computes the canonical norm from there (the same bits in all 16), and
//   the row is normalised in place;
//   the 64 groups of 16 lanes take the positions behind it, DISTINCT_TRIP = 64 consecutive positions per trip; a position that
//   has an owner already is skipped (its group idles for the trip), an ownerless one within min_sep gets this owner. Positions
//   are visited in order and an owned one is never visited again, so the owner is the smallest such kept entry.
// Worst case k rounds x pool dots per query (min_sep below every sep). Wave64; row loads are canon_partial_dots' (16 / 8 / 4
// bytes per lane for f32 / f16 / fp8 rows), the query slice comes from LDS in 16-byte reads.
#pragma once
#include "retrieval_kernels.h"

constexpr int DISTINCT_THREADS = 1024;
constexpr int DISTINCT_TRIP = DISTINCT_THREADS / 16;   // list positions per trip: one per group of 16 lanes
constexpr int DISTINCT_SLOTS = 2048;                   // list positions the LDS state holds (pool <= 2040)

struct DistinctArgs {
    const void* rows; int D;
    const float* inv;            // fp8 rows: inverse norm per row; null otherwise
    const int64_t* labels;       // [N] row -> label, strictly increasing
    int64_t N;
    const int64_t* list_lab;     // [Q, pool] the list stage's labels, (distance, label) order, -1 behind the count
    const float* list_dist;      // [Q, pool] ... and distance bits
    const int32_t* list_cnt;     // [Q] entries of each list
    int pool, k;
    float min_sep;
    int64_t* out_labels;         // [Q, k]
    float* out_dist;             // [Q, k]
    int32_t* out_count;          // [Q]
    int32_t* out_dups;           // [Q, k] or null
    int32_t* out_listed;         // [Q] or null
};

// dynamic LDS: the kept row as a query (f32 [D]) and four int32 arrays of DISTINCT_SLOTS: row and owner (the kept RANK) per list
// position, the kept positions in order, the entries each kept rank owns
__host__ __device__ inline int distinct_lds_bytes(int D) { return D * 4 + 4 * DISTINCT_SLOTS * 4; }

template <typename T>
__global__ __launch_bounds__(DISTINCT_THREADS) void distinct_kernel(DistinctArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int p16 = tid & 15, grp = tid >> 4;
    const int q = blockIdx.x, D = a.D;
    float* const qv = reinterpret_cast<float*>(smem);
    int32_t* const s_row = reinterpret_cast<int32_t*>(smem + (size_t)D * 4);
    int32_t* const s_own = s_row + DISTINCT_SLOTS;
    int32_t* const s_kept = s_own + DISTINCT_SLOTS;
    int32_t* const s_dups = s_kept + DISTINCT_SLOTS;
    const int64_t* const ll = a.list_lab + (size_t)q * a.pool;
    int m = a.list_cnt[q];
    m = m < 0 ? 0 : (m > a.pool ? a.pool : m);

    // rows: row order is label order, so a list label becomes its row by binary search in the label array
    for (int i = tid; i < DISTINCT_SLOTS; i += DISTINCT_THREADS) {
        int32_t row = -1;
        if (i < m) {
            const int64_t lab = ll[i];
            int64_t lo = 0, hi = a.N;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (a.labels[mid] < lab) lo = mid + 1; else hi = mid;
            }
            if (lo < a.N && a.labels[lo] == lab) row = (int32_t)lo;
        }
        s_row[i] = row;
        s_own[i] = -1;
        s_dups[i] = 0;
    }
    __syncthreads();

    const T* const rows = reinterpret_cast<const T*>(a.rows);
    int nk = 0, last = -1;   // kept so far, the last kept position (block-uniform: every wave derives them from the same LDS state)
    while (nk < a.k) {
        int next = m;
        for (int base = last + 1; base < m; base += 64) {
            const int i = base + lane;
            const unsigned long long free = __ballot(i < m && s_own[i] < 0);
            if (free) { next = base + __ffsll((long long)free) - 1; break; }
        }
        if (next >= m) break;
        if (tid == 0) s_kept[nk] = next;
        const int rank = nk;
        ++nk; last = next;
        const int64_t krow = s_row[next];
        if (next == m - 1 || krow < 0) continue;   // nothing behind it (a label that is no row cannot happen: the list is the index's own)
        // the kept row as a query: widened (fp8: x inverse norm), canonical norm, normalised in place
        for (int d = tid; d < D; d += DISTINCT_THREADS) {
            float v = (float)rows[(size_t)krow * D + d];
            if constexpr (sizeof(T) == 1) v = v * a.inv[krow];
            qv[d] = v;
        }
        __syncthreads();
        double ss = 0.0;
        for (int d = lane; d < D; d += 64) {
            const double v = (double)qv[d];
            ss = ss + v * v;
        }
        const double nrm = sqrt(wave_butterfly_sum(ss));
        __syncthreads();
        for (int d = tid; d < D; d += DISTINCT_THREADS) {
            float y = (float)((double)qv[d] / nrm);
            asm volatile("" : "+v"(y));
            qv[d] = y;
        }
        __syncthreads();
        const float* const qp = qv + 4 * p16;
        for (int base = next + 1; base < m; base += DISTINCT_TRIP) {
            const int pos = base + grp;
            int64_t row = -1;
            if (pos < m && s_own[pos] < 0) row = s_row[pos];
            const bool live = row >= 0;
            const T* rv = rows + (size_t)(live ? row : 0) * D + 4 * p16;
            double acc[4];
            canon_partial_dots<T>(rv, live, qp, D, acc);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], o);
            }
            const double t0 = acc[0] + acc[2], t1 = acc[1] + acc[3];
            double dot = t0 + t1;
            if (p16 == 0 && live) {
                if constexpr (sizeof(T) == 1) dot = dot * (double)a.inv[row];
                const float dist = (float)(1.0 - dot);
                if (dist <= a.min_sep) s_own[pos] = rank;
            }
        }
        __syncthreads();
    }
    __syncthreads();

    // write-out: what each kept rank owns, then the kept entries with the list's own distance bits
    for (int i = tid; i < m; i += DISTINCT_THREADS) {
        const int o = s_own[i];
        if (o >= 0) atomicAdd(&s_dups[o], 1);
    }
    __syncthreads();
    const float* const ld = a.list_dist + (size_t)q * a.pool;
    for (int j = tid; j < a.k; j += DISTINCT_THREADS) {
        const bool ok = j < nk;
        const int pos = ok ? s_kept[j] : 0;
        a.out_labels[(size_t)q * a.k + j] = ok ? ll[pos] : -1;
        a.out_dist[(size_t)q * a.k + j] = ok ? ld[pos] : INFINITY;
        if (a.out_dups) a.out_dups[(size_t)q * a.k + j] = ok ? s_dups[j] : 0;
    }
    if (tid == 0) {
        a.out_count[q] = nk;
        if (a.out_listed) a.out_listed[q] = m;
    }
}

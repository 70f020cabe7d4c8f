// assign_kernels.h — nearest-centre assignment of EVERY row and the per-cluster row sums (mmiss_index_assign,
// mmiss_index_cluster_sums; api_index.hip "assignment / clustering"): for C <= 1024 centres the centre of smallest canonical
// distance of every stored row, ties to the smaller centre index — the transposed question of a query (which of these C vectors
// is nearest to row r, for every r): zero-shot classification of the collection against C prompts, and the assignment step of
// spherical k-means, whose other half (the sums of the rows of a cluster) is the second kernel family here.
//
// Routes of an assign call, all exact:
//   scan     assign_scan_kernel: approximate matrix-core scores of every row against 16 NQT centres per pass; per row the
//            largest score s1, its centre i1 and the second-largest score s2 COUNTED WITH MULTIPLICITY (two centres with the
//            same best score give s2 == s1), merged over the passes in a 12-byte state per row;
//   decide   assign_decide_kernel: a row is SURE iff (double)s1 - (double)s2 > 2 E, E = the largest finite eps_q of the call's
//            centres (assign_bound_kernel, on the device); every other row with a finite s1 is BORDERLINE and is listed;
//   resolve  assign_resolve_kernel: the canonical distance of a sure row to i1 (only when distances are wanted), and of a
//            borderline row to every live centre with the minimum by (distance, centre index).
//
// Why a sure row needs no canonical comparison. eps_c = prep_queries_kernel's eps_q of centre c: |s - c| <= eps_c - 2^-21 for
// the approximate score s and the canonical score c of any row (guard_terms; the 2^-21 is slack on top of the arithmetic's
// bound), and eps_c <= E for every live centre. For a sure row and any other live centre j, s_j <= s2, so
//     c_{i1} >= s1 - E + 2^-21   and   c_j <= s2 + E - 2^-21:   c_{i1} - c_j >= (s1 - s2 - 2 E) + 2^-20 > 2^-20.
//   (s1 - s2 is evaluated in fp64 from two floats of magnitude <= 1.1: off by 2^-53 relative at the most, far inside the slack;
//   2 E is exact.) The distance is d = (float)(1 - c): the roundings of 1 - c (fp64, then float) move a value in [0, 2] by at
//   most 2^-24 (+ 2^-53), so d_{i1} <= 1 - c_{i1} + 2^-24 + 2^-53 < 1 - c_j - 2^-20 + 2^-24 + 2^-53 < d_j - 2^-21: d_{i1} < d_j
//   STRICTLY AS FLOATS. i1 is the unique minimum of (distance, index); no tie-break can interfere.
// One live centre only: s2 = -inf, the row is sure.
// Dead centres — without a direction (eps = +inf: their operand is NaN) or behind C in the padded tile — score -inf and are
// never chosen. A row without a direction has a NaN among its stored elements, so EVERY score of it against a live centre
// (finite operand) is NaN, and a row with a direction has none (finite operands, |score| <= 1.1): "some live score is NaN" is
// "the row has no direction". The scan maps such a score to +inf; a row whose s1 is not finite (+inf: no direction; -inf: no
// live centre) gets -1 / +inf.
#pragma once
#include "retrieval_kernels.h"

// E = the largest finite eps_q of centres [0, C) (0 when there is none), nlive = how many centres have one. One wave.
__global__ __launch_bounds__(64) void assign_bound_kernel(const float* __restrict__ eps_q, int C, float* __restrict__ E, int32_t* __restrict__ nlive) {
    const int lane = threadIdx.x;
    float e = 0.f;
    int n = 0;
    for (int c = lane; c < C; c += 64) {
        const float v = eps_q[c];
        if (v < INFINITY) { e = fmaxf(e, v); ++n; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        e = fmaxf(e, __shfl_xor(e, o));
        n += __shfl_xor(n, o);
    }
    if (lane == 0) { *E = e; *nlive = n; }
}

// (a1, ai, a2) <- the two largest, with multiplicity, of the union of (a1, ai, a2) and (o1, oi, o2); equal best scores keep the
// smaller index. No NaN comes here (the scan maps it away).
__device__ __forceinline__ void assign_top2_merge(float& a1, int& ai, float& a2, float o1, int oi, float o2) {
    const float n2 = fmaxf(fminf(a1, o1), fmaxf(a2, o2));
    if (o1 > a1 || (o1 == a1 && oi < ai)) { a1 = o1; ai = oi; }
    a2 = n2;
}

struct AssignScanArgs {
    const void* rows;      // [N, D] storage dtype
    int64_t N;
    int D;
    const void* qs;        // [16 NQT, D] the pass's centre operands (prep_queries_kernel's qs; rows behind C are zero)
    const float* eps_q;    // [C] every centre's bound (indexed by the centre, not by the pass)
    const float* inv;      // fp8 rows: [>= N rounded up to 16] inverse norms
    int tiles_per_block;   // 16-row tiles per slab
    int c0;                // the pass's first centre
    int C;
    int first;             // 1: the pass writes the state; 0: it merges into it
    float* st_s1;          // [N] each: the per-row state (12 bytes per row against >= 128 bytes of row read)
    int32_t* st_i1;
    float* st_s2;
};

// The streaming scan of member_scan_kernel (membership_kernels.h; scan_topk_kernel before it) with a top-2 output: grid = slabs
// of 16-row tiles, 4 waves per block, wave w takes tiles w, w + 4, ...; the 16 NQT centre operands are staged once in LDS with
// the scan's padded row stride (D * QELT + 16 bytes); row fragments go global -> VGPR with 16-byte loads, a group of 8 (then 4)
// loads ahead of the group's MFMAs.
// SAME MFMA instruction and SAME k order per dtype as scan_topk_kernel — f16: 16x16x32_f16 on 64-byte steps; f32: four
// 16x16x4_f32 per 16-byte load; fp8: 16 codes per lane widened to f16, two 16x16x32_f16 per 64-code span, score x SCORE_SCALE x
// inv[row] — so guard_terms / prep_queries_kernel's bound eps_q covers these scores verbatim, as it covers the scan's.
// Accumulator layout D[row = 4 g + reg][col = lane & 15]: a lane owns one centre per centre tile. Per accumulator register the
// lane first folds its NQT centres into (s1, i1, s2), then the 16 lanes of the group fold theirs with four lane ^ J exchanges
// inside the 16-lane row (DPP, no LDS). Lanes with (lane & 15) < 4 then hold row 4 g + (lane & 15) and store (or merge into) its
// state: 16 consecutive rows per tile.
template <typename T, int NQT>
__global__ __launch_bounds__(256) void assign_scan_kernel(AssignScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ELT = ScanTraits<T>::ELT, QELT = ScanTraits<T>::QELT;
    constexpr int NQ = 16 * NQT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int D = a.D;
    const int qstride = D * QELT + 16;
    char* sQ = smem;
    {
        const int chunks_per_row = D * QELT / 16;
        const char* qsrc = reinterpret_cast<const char*>(a.qs);
        for (int i = tid; i < NQ * chunks_per_row; i += 256) {
            const int qr = i / chunks_per_row, c = i - qr * chunks_per_row;
            *reinterpret_cast<u32x4*>(sQ + qr * qstride + c * 16) =
                *reinterpret_cast<const u32x4*>(qsrc + ((size_t)qr * chunks_per_row + c) * 16);
        }
    }
    __syncthreads();

    bool live_r[NQT];   // a dead centre (no direction, or behind C) scores -inf
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        const int c = a.c0 + qt * 16 + fr;
        live_r[qt] = c < a.C && a.eps_q[c < a.C ? c : 0] < INFINITY;
    }

    const int64_t ntiles_total = (a.N + 15) >> 4;
    const int64_t tile0 = (int64_t)blockIdx.x * a.tiles_per_block;
    int64_t tile_end = tile0 + a.tiles_per_block;
    if (tile_end > ntiles_total) tile_end = ntiles_total;

    for (int64_t tile = tile0 + wave; tile < tile_end; tile += 4) {
        const int64_t row0 = tile << 4;
        int64_t rload = row0 + fr;
        if (rload >= a.N) rload = a.N - 1;  // clamp: loads stay in bounds, the rows behind N are not stored below
        const char* rp = reinterpret_cast<const char*>(a.rows) + (size_t)rload * D * ELT + fg * 16;
        const char* qp = sQ + fr * qstride + fg * 16;
        f32x4 acc[NQT];
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) acc[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 rinv = {ScanTraits<T>::SCORE_SCALE, ScanTraits<T>::SCORE_SCALE, ScanTraits<T>::SCORE_SCALE, ScanTraits<T>::SCORE_SCALE};
        if constexpr (ELT == 1) rinv = *reinterpret_cast<const f32x4*>(a.inv + row0 + 4 * fg) * ScanTraits<T>::SCORE_SCALE;
        auto steps = [&](auto nsteps_tag, int byte0) {
            constexpr int NS = decltype(nsteps_tag)::value;
            u32x4 araw[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) araw[s] = *reinterpret_cast<const u32x4*>(rp + byte0 + s * 64);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
#pragma unroll
                for (int qt = 0; qt < NQT; ++qt) {
                    const u32x4 braw = *reinterpret_cast<const u32x4*>(qp + qt * 16 * qstride + byte0 + s * 64);
                    if constexpr (ELT == 2) {
                        acc[qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, araw[s]),
                                                                         __builtin_bit_cast(f16x8, braw), acc[qt], 0, 0, 0);
                    } else {
                        const f32x4 af = __builtin_bit_cast(f32x4, araw[s]), bf = __builtin_bit_cast(f32x4, braw);
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            acc[qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[t], bf[t], acc[qt], 0, 0, 0);
                    }
                }
            }
        };
        auto spans = [&](auto nsp_tag, int span0) {   // fp8 rows: the scan's 64-code spans (its k permutation, on both operands)
            constexpr int NS = decltype(nsp_tag)::value;
            typedef _Float16 h2 __attribute__((ext_vector_type(2)));
            typedef float f2 __attribute__((ext_vector_type(2)));
            const char* rp8 = reinterpret_cast<const char*>(a.rows) + (size_t)rload * D + fg * 16;
            const char* qp8 = sQ + fr * qstride + fg * 32;
            u32x4 araw[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) araw[s] = *reinterpret_cast<const u32x4*>(rp8 + (span0 + s) * 64);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    f16x8 a16;
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        const f2 lo2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)araw[s][2 * h + w], false);
                        const f2 hi2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)araw[s][2 * h + w], true);
                        const h2 l2 = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(lo2[0], lo2[1]));   // (exact: e4m3 fits f16)
                        const h2 g2 = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(hi2[0], hi2[1]));
                        a16[4 * w + 0] = l2[0]; a16[4 * w + 1] = l2[1]; a16[4 * w + 2] = g2[0]; a16[4 * w + 3] = g2[1];
                    }
#pragma unroll
                    for (int qt = 0; qt < NQT; ++qt) {
                        const u32x4 braw = *reinterpret_cast<const u32x4*>(qp8 + qt * 16 * qstride + (span0 + s) * 128 + h * 16);
                        acc[qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16, __builtin_bit_cast(f16x8, braw), acc[qt], 0, 0, 0);
                    }
                }
            }
        };
        if constexpr (ELT == 1) {
            const int nspans = D >> 6;   // D % 128 == 0: even
            int sp = 0;
            for (; sp + 8 <= nspans; sp += 8) spans(std::integral_constant<int, 8>{}, sp);
            if (sp + 4 <= nspans) { spans(std::integral_constant<int, 4>{}, sp); sp += 4; }
            if (sp < nspans) spans(std::integral_constant<int, 2>{}, sp);
        } else {
            const int row_bytes = D * QELT;  // a multiple of 256 (index dim % 128 == 0)
            int byte0 = 0;
            for (; byte0 + 512 <= row_bytes; byte0 += 512) steps(std::integral_constant<int, 8>{}, byte0);
            if (byte0 < row_bytes) steps(std::integral_constant<int, 4>{}, byte0);
        }
        // the two largest scores of every row of the tile over the pass's live centres
        float m1 = -INFINITY, m2 = -INFINITY;   // what this lane stores: row 4 fg + fr of the tile (fr < 4)
        int mi = 0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float b1 = -INFINITY, b2 = -INFINITY;
            int bi = a.c0 + fr;
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                float s = acc[qt][reg] * rinv[reg];   // (f16 / f32 rows: x 1; fp8 rows: x inv[row] / 128, one rounding)
                s = live_r[qt] ? (s != s ? INFINITY : s) : -INFINITY;
                assign_top2_merge(b1, bi, b2, s, a.c0 + qt * 16 + fr, -INFINITY);
            }
            auto fold = [&](auto jt) {
                constexpr int J = decltype(jt)::value;
                const float o1 = __int_as_float(lane_xor<J>(__float_as_int(b1)));
                const int oi = lane_xor<J>(bi);
                const float o2 = __int_as_float(lane_xor<J>(__float_as_int(b2)));
                assign_top2_merge(b1, bi, b2, o1, oi, o2);
            };
            fold(std::integral_constant<int, 1>{});
            fold(std::integral_constant<int, 2>{});
            fold(std::integral_constant<int, 4>{});
            fold(std::integral_constant<int, 8>{});
            if (fr == reg) { m1 = b1; mi = bi; m2 = b2; }
        }
        const int64_t row = row0 + 4 * fg + fr;
        if (fr < 4 && row < a.N) {
            if (!a.first) {   // (the earlier passes' centres have the smaller indices: they go first)
                float p1 = a.st_s1[row], p2 = a.st_s2[row];
                int pi = a.st_i1[row];
                assign_top2_merge(p1, pi, p2, m1, mi, m2);
                m1 = p1; mi = pi; m2 = p2;
            }
            a.st_s1[row] = m1;
            a.st_i1[row] = mi;
            a.st_s2[row] = m2;
        }
    }
}

// Row r: sure -> assign[r] = i1; borderline -> assign[r] = -2 for now and r goes on the list (sized to N: it cannot overflow);
// neither (no direction, or no live centre) -> assign[r] = -1, dist[r] = +inf. One list position per wave and trip is taken
// with one atomic add; the list's order is that of the atomics, and nothing depends on it (a row's result is its own).
__global__ __launch_bounds__(256) void assign_decide_kernel(const float* __restrict__ st_s1, const int32_t* __restrict__ st_i1,
                                                            const float* __restrict__ st_s2, int64_t N, const float* __restrict__ E,
                                                            int32_t* __restrict__ assign, float* __restrict__ dist,
                                                            int32_t* __restrict__ blist, int32_t* __restrict__ bcnt) {
    const int lane = threadIdx.x & 63;
    const double e2 = 2.0 * (double)*E;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); r0 < N; r0 += stride) {
        const int64_t r = r0 + lane;
        bool border = false;
        if (r < N) {
            const float s1 = st_s1[r];
            const bool finite = s1 > -INFINITY && s1 < INFINITY;
            const bool sure = finite && (double)s1 - (double)st_s2[r] > e2;
            border = finite && !sure;
            assign[r] = sure ? st_i1[r] : border ? -2 : -1;
            if (dist && !finite) dist[r] = INFINITY;
        }
        const uint64_t bal = __ballot(border);
        if (bal) {
            int base = 0;
            if (lane == 0) base = atomicAdd(bcnt, __popcll(bal));
            base = __shfl(base, 0);
            if (border) blist[base + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)r;
        }
    }
}

// The canonical arithmetic of rerank_kernel / canonical_scan_kernel (canon_partial_dots, the same shuffles, the same last three
// additions, fp8 rows x (double)inv[row]: the same bits), one 16-lane group per row.
//   blist == null: every row r of [0, N) with assign[r] >= 0 (the sure rows) gets dist[r] = its distance to centre assign[r].
//   blist != null: every listed (borderline) row gets the distance to every live centre, centres ascending; a strictly smaller
//     distance replaces the best, so ties stay with the smaller index and a NaN never wins; assign / dist (dist may be null)
//     get the minimum, -1 / +inf when there is none.
template <typename T>
__global__ __launch_bounds__(256) void assign_resolve_kernel(const void* __restrict__ rows, int D, const float* __restrict__ qn,
                                                             const float* __restrict__ inv, const float* __restrict__ eps_q, int C,
                                                             const int32_t* __restrict__ blist, const int32_t* __restrict__ bcnt,
                                                             int64_t N, int32_t* __restrict__ assign, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p16 = lane & 15, sub = lane >> 4;
    const int64_t n = blist ? (int64_t)*bcnt : N;
    auto distance = [&](const T* rv, bool live, int c, int64_t row) -> float {
        double acc[4];
        canon_partial_dots<T>(rv, live, qn + (size_t)c * D + 4 * p16, D, acc);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] + __shfl_xor(acc[j], o);
        }
        const double t0 = acc[0] + acc[2], t1 = acc[1] + acc[3];
        double dot = t0 + t1;
        if constexpr (sizeof(T) == 1) dot = dot * (double)inv[row];
        return (float)(1.0 - dot);
    };
    for (int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * 4; i0 < n; i0 += (int64_t)gridDim.x * 16) {
        const int64_t i = i0 + sub;
        const bool live = i < n;
        const int64_t row = live ? (blist ? (int64_t)blist[i] : i) : 0;
        const T* rv = reinterpret_cast<const T*>(rows) + (size_t)row * D + 4 * p16;
        if (!blist) {
            const int c = live ? assign[row] : -1;
            const float d = distance(rv, live && c >= 0, c >= 0 ? c : 0, row);
            if (p16 == 0 && c >= 0) dist[row] = d;
        } else {
            float best = INFINITY;
            int bi = -1;
            for (int c = 0; c < C; ++c) {
                if (!(eps_q[c] < INFINITY)) continue;   // (uniform: a centre without a direction is never chosen)
                const float d = distance(rv, live, c, row);
                if (d < best) { best = d; bi = c; }
            }
            if (p16 == 0 && live) {
                assign[row] = bi;
                if (dist) dist[row] = best;
            }
        }
    }
}

// sizes[c] += rows of [0, N) with assign[r] == c, c in [0, C), C <= 1024 (sizes zeroed by the caller; entries outside 0 .. C-1
// are skipped): a block counts in LDS and adds what it found; integer sums, exact in any order.
__global__ __launch_bounds__(256) void assign_sizes_kernel(const int32_t* __restrict__ assign, int64_t N, int C, unsigned long long* __restrict__ sizes) {
    __shared__ int h[1024];
    for (int c = threadIdx.x; c < C; c += 256) h[c] = 0;
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const int a = assign[r];
        if (a >= 0 && a < C) atomicAdd(&h[a], 1);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
        if (h[c]) atomicAdd(sizes + c, (unsigned long long)h[c]);
}

// ------------------------------------------------------------------------------------------------ cluster sums
// sums[c][j] += sum over the rows r with assign[r] == c of (int64) rint((double)x[r][j] * 2^32), x = the float32 value
// mmiss_index_get returns for the element (f16 / f32 rows: the stored value; fp8 rows: value x inv[row], one float multiply, as
// gather_rows_f8_f32_kernel). The product with 2^32 is exact in fp64, rint rounds to nearest even, and 64-bit integer addition
// (two's complement, through the unsigned atomics) is associative and commutative: whatever order the atomics land in, the
// result has one value. |x| <= ~1 and fewer than 2^31 rows: no overflow.
struct ClusterSumsArgs {
    const void* rows;            // [N, D] storage dtype
    const float* inv;            // fp8 rows: [N] inverse norms
    const int32_t* assign;       // [N]; entries outside 0 .. C-1 are skipped
    int64_t N;
    int D, C;
    int rows_per_block;          // rows of a slab (grid.x = slabs)
    int cols;                    // columns of a chunk (grid.y = D / cols), a multiple of 4; C x cols x 8 bytes of LDS
    unsigned long long* sums;    // [C, D], zeroed by the caller
};

// One pass over the rows: a block (1024 threads: the table leaves room for two blocks per CU at the most, and the LDS atomics
// want waves to hide behind) takes a slab of rows and a chunk of columns, a thread four consecutive elements at a time. The
// block adds into a private table [C][cols] of 64-bit sums in LDS (64-bit LDS atomics) and flushes its non-zero entries with one
// 64-bit global atomic add each. The host picks the widest chunk whose table fits (16 columns at C = 1024).
template <typename T>
__global__ __launch_bounds__(1024) void cluster_sums_kernel(ClusterSumsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* tab = reinterpret_cast<unsigned long long*>(smem);
    const int tid = threadIdx.x;
    const int col0 = blockIdx.y * a.cols;
    const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_block;
    const int nrows = (int)(a.N - r0 < a.rows_per_block ? a.N - r0 : a.rows_per_block);
    const int ntab = a.C * a.cols;
    for (int e = tid; e < ntab; e += blockDim.x) tab[e] = 0ull;
    __syncthreads();
    const int q = a.cols >> 2;
    for (int idx = tid; idx < nrows * q; idx += blockDim.x) {
        const int lr = idx / q, g = idx - lr * q;
        const int64_t r = r0 + lr;
        const int c = a.assign[r];
        if (c < 0 || c >= a.C) continue;
        const int col = col0 + 4 * g;
        float x[4];
        if constexpr (sizeof(T) == 1) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(a.rows) + (size_t)r * a.D + col);
            f8x4_values(w, x);
            const float iv = a.inv[r];
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = x[j] * iv;
        } else if constexpr (sizeof(T) == 2) {
            const u32x2 w = *reinterpret_cast<const u32x2*>(reinterpret_cast<const _Float16*>(a.rows) + (size_t)r * a.D + col);
            const _Float16* h = reinterpret_cast<const _Float16*>(&w);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = (float)h[j];
        } else {
            const f32x4 w = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.rows) + (size_t)r * a.D + col);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = w[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long v = (unsigned long long)llrint((double)x[j] * 4294967296.0);
            atomicAdd(tab + c * a.cols + 4 * g + j, v);
        }
    }
    __syncthreads();
    for (int e = tid; e < ntab; e += blockDim.x) {
        const unsigned long long v = tab[e];
        const int c = e / a.cols, j = e - c * a.cols;
        if (v) atomicAdd(a.sums + (size_t)c * a.D + col0 + j, v);
    }
}

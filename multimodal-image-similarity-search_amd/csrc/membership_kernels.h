// membership_kernels.h — dense radius membership (mmiss_index_membership, mmiss_index_tag_by_radius; api_index.hip
// "membership / tagging"): for up to 64 probes (a query vector and a radius each) the exact membership of EVERY row, one bit per
// (row, probe), produced in one streaming pass over the index.
//
// What it replaces: the yes/no pass over every stored image behind the reference's filters (process_filter_on_all_images,
// backend/app/main.py:939-1056), for the one question this library's arithmetic answers itself: "is this row within distance R
// of this embedding?" (the member definition of mmiss_index_query_radius, unchanged).
//
// Three routes, all exact:
//   scan     member_scan_kernel: approximate matrix-core scores against TWO thresholds per probe (below); a pair that clears
//            either is decided, the rest — the borderline pairs — are listed per probe and leave a 0 bit behind;
//   resolve  member_resolve_kernel: the canonical distance of every listed pair, d <= R sets the bit;
//   overflow a probe with more than `bcap` borderline rows (mass duplicates at exactly its radius): canonical_scan_kernel over
//            the whole index and member_from_dist_kernel, which sets or clears the probe's bit on every row.
//
// The two-sided bound. eps_p = prep_queries_kernel's eps_q of probe p: |s - c| <= eps_p - 2^-21 for the approximate score s and
// the canonical score c of any row (guard_terms; the 2^-21 term is slack on top of the arithmetic's bound). d = (float)(1 - c).
//   low side (radius_thr_kernel's derivation): lo_p = (1 - R_p) - eps_p rounded down. s < lo_p gives c < (1 - R_p) - 2^-21, so
//     1 - c > R_p + 2^-21; the roundings of 1 - c (fp64, then float: <= 2^-23 for |1 - c| <= 2) cannot bring it down to R_p:
//     d > R_p, no member.
//   high side: hi_p = (1 - R_p) + eps_p rounded up. s >= hi_p gives c >= s - eps_p >= 1 - R_p, so 1 - c <= R_p in exact
//     arithmetic. R_p is a float and both roundings of 1 - c (to fp64, to float) are monotonic and leave a representable
//     value where it is: fl(1 - c) <= fl(R_p) = R_p. The bound therefore covers the float rounding of the canonical distance:
//     s >= hi_p implies d <= R_p AS FLOATS, a member. (The slack 2^-21 is not needed on this side; it stays in, unused.)
//   1 - R_p is evaluated in fp64: exact unless |R_p| < 2^-53, where it is off by less than 2^-53, far inside the slack.
// A probe without a direction (eps_p = +inf) and a radius of -inf get lo = hi = +inf: no member, nothing listed. R = +inf gives
// -inf twice: every row with a (non-NaN) score is a sure member. A NaN score (a row without a direction: its stored elements
// are NaN) clears neither threshold and is resolved canonically, where its NaN distance is no member — the radius call's rule.
#pragma once
#include "retrieval_kernels.h"

// lo[p], hi[p] for p in [0, Ppad): probes [P, Ppad) are dead (+inf)
__global__ __launch_bounds__(64) void member_thr_kernel(const float* __restrict__ max_dist, const float* __restrict__ eps_q,
                                                        float* __restrict__ lo, float* __restrict__ hi, int P, int Ppad) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= Ppad) return;
    float l = INFINITY, h = INFINITY;
    if (p < P) {
        const float e = eps_q[p];
        if (e < INFINITY) {
            const double mid = 1.0 - (double)max_dist[p];
            const double dl = mid - (double)e, dh = mid + (double)e;
            l = (float)dl;
            if ((double)l > dl) l = nextafterf(l, -INFINITY);
            h = (float)dh;
            if ((double)h < dh) h = nextafterf(h, INFINITY);
        }
    }
    lo[p] = l;
    hi[p] = h;
}

// The borderline counters sit MEMBER_CNT_STRIDE ints (256 bytes) apart: appends of different probes then do not queue up behind
// one another on one cache line (16 counters on one line: 1.07 ms per call of 16 probes at 1M x 512 f16 rows with 0.6 % of the
// pairs borderline, 0.36 ms apart; profiles/membership.txt).
constexpr int MEMBER_CNT_STRIDE = 64;

struct MemberScanArgs {
    const void* rows;      // [N, D] storage dtype
    int64_t N;
    int D;
    const void* qs;        // [16 NQT, D] the pass's probe operands (prep_queries_kernel's qs; rows behind P are zero)
    const float* lo;       // [16 NQT] the pass's thresholds (member_thr_kernel)
    const float* hi;
    const float* inv;      // fp8 rows: [>= N rounded up to 16] inverse norms
    int tiles_per_block;   // 16-row tiles per slab
    uint64_t* words;       // [>= N] one word per row; rows >= N are not touched
    int bit0;              // the pass's first probe is bit bit0 of a word
    int first;             // 1: the pass writes the whole word (its bits, zeros elsewhere); 0: it ORs its bits into the word
    int32_t* bcnt;         // [16 NQT][MEMBER_CNT_STRIDE] borderline rows per probe of the pass, in the first int of each; may run past
                           // bcap (the excess is dropped)
    int32_t* blist;        // [16 NQT][bcap] their rows, any order
    int bcap;
};

// The streaming scan of scan_topk_kernel (retrieval_kernels.h) with a dense output: grid = slabs of 16-row tiles, 4 waves per
// block, wave w takes tiles w, w + 4, ...; the 16 NQT probe operands are staged once in LDS with the scan's padded row stride
// (D * QELT + 16 bytes: the 16 probe rows of a fragment read hit 16 different bank groups); row fragments go global -> VGPR with
// 16-byte loads, a group of 8 (then 4) loads ahead of the group's MFMAs (guide "GEMV / M <= 16": a streamed operand nobody
// shares takes no LDS round trip).
// SAME MFMA instruction and SAME k order per dtype as scan_topk_kernel — f16: 16x16x32_f16 on 64-byte steps; f32: four
// 16x16x4_f32 per 16-byte load; fp8: 16 codes per lane widened to f16, two 16x16x32_f16 per 64-code span, score x SCORE_SCALE x
// inv[row] — so guard_terms / prep_queries_kernel's bound eps_q covers these scores verbatim, as it covers the scan's.
// Accumulator layout D[row = 4 g + reg][col = lane & 15]: a lane owns one probe per probe tile, its two thresholds live in
// registers, and ONE ballot of "sure member" per accumulator register and probe tile holds, in bits [16 g, 16 g + 16), the 16
// probe bits of row 4 g + reg. Lanes 0..15 assemble rows 0..15 of the tile from the 4 NQT ballots and store them with one 8-byte
// vector store each: 128 contiguous bytes per tile.
template <typename T, int NQT>
__global__ __launch_bounds__(256) void member_scan_kernel(MemberScanArgs a) {
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

    float lo_r[NQT], hi_r[NQT];
    bool live_r[NQT];   // a dead probe (no direction, radius -inf, or behind P) lists nothing
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        lo_r[qt] = a.lo[qt * 16 + fr];
        hi_r[qt] = a.hi[qt * 16 + fr];
        live_r[qt] = hi_r[qt] < INFINITY;
    }

    const int64_t ntiles_total = (a.N + 15) >> 4;
    const int64_t tile0 = (int64_t)blockIdx.x * a.tiles_per_block;
    int64_t tile_end = tile0 + a.tiles_per_block;
    if (tile_end > ntiles_total) tile_end = ntiles_total;

    for (int64_t tile = tile0 + wave; tile < tile_end; tile += 4) {
        const int64_t row0 = tile << 4;
        int64_t rload = row0 + fr;
        if (rload >= a.N) rload = a.N - 1;  // clamp: loads stay in bounds, the rows behind N are masked below
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
        // decide: sure members by ballot, borderline pairs to their probe's list
        const int sh = 16 * ((lane >> 2) & 3);   // lanes 0..15 store row `lane` = 4 g + reg with g = lane >> 2, reg = lane & 3
        uint64_t w = 0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = row0 + 4 * fg + reg;
            const bool inb = row < a.N;
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt) {
                const float s = acc[qt][reg] * rinv[reg];   // (f16 / f32 rows: x 1; fp8 rows: x inv[row] / 128, one rounding)
                const bool sure = inb && s >= hi_r[qt];
                const bool border = inb && live_r[qt] && !(s >= hi_r[qt]) && !(s < lo_r[qt]);   // (a NaN score lands here)
                const uint64_t bal = __ballot(sure);
                if ((lane & 3) == reg) w |= ((bal >> sh) & 0xffffull) << (16 * qt);
                if (border) {
                    const int pos = atomicAdd(a.bcnt + (qt * 16 + fr) * MEMBER_CNT_STRIDE, 1);
                    if (pos < a.bcap) a.blist[(size_t)(qt * 16 + fr) * a.bcap + pos] = (int)row;
                }
            }
        }
        if (lane < 16 && row0 + lane < a.N) {
            uint64_t* wp = a.words + row0 + lane;
            uint64_t v = w << a.bit0;
            if (!a.first) v |= *wp;
            *wp = v;
        }
    }
}

// The borderline pairs: one 16-lane group per (row, probe) pair, the canonical dot product of rerank_kernel /
// canonical_scan_kernel (canon_partial_dots, the same shuffles, the same last three additions: the same bits), d <= R sets the
// probe's bit in the row's word with a vector atomic OR (the scan left it 0). Bits are independent and an OR commutes: the
// result does not depend on the order. grid = (blocks, probes); a probe whose list overflowed is skipped (the overflow route
// rewrites its bit on every row).
template <typename T>
__global__ __launch_bounds__(256) void member_resolve_kernel(const void* __restrict__ rows, int D, const float* __restrict__ qn,
                                                             const float* __restrict__ inv, const float* __restrict__ max_dist,
                                                             const int32_t* __restrict__ bcnt, const int32_t* __restrict__ blist,
                                                             int bcap, uint64_t* __restrict__ words) {
    const int probe = blockIdx.y;
    const int n = bcnt[probe * MEMBER_CNT_STRIDE];
    if (n <= 0 || n > bcap) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p16 = lane & 15, sub = lane >> 4;
    const float* qp = qn + (size_t)probe * D + 4 * p16;
    const float rmax = max_dist[probe];
    for (int i0 = (blockIdx.x * 4 + wave) * 4; i0 < n; i0 += gridDim.x * 16) {
        const int i = i0 + sub;
        const bool live = i < n;
        const int64_t row = live ? blist[(size_t)probe * bcap + i] : 0;
        const T* rv = reinterpret_cast<const T*>(rows) + (size_t)row * D + 4 * p16;
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
            if constexpr (sizeof(T) == 1) dot = dot * (double)inv[row];
            const float d = (float)(1.0 - dot);
            if (d <= rmax) atomicOr(reinterpret_cast<unsigned long long*>(words + row), 1ull << probe);
        }
    }
}

// An overflowed probe: dist[r] = canonical_scan_kernel's distance of every row; bit `probe` of every row's word := dist[r] <= R
// (set or cleared; a NaN distance clears it).
__global__ __launch_bounds__(256) void member_from_dist_kernel(const float* __restrict__ dist, int64_t N, const float* __restrict__ max_dist,
                                                               int probe, uint64_t* __restrict__ words) {
    const float rmax = max_dist[probe];
    const uint64_t bit = 1ull << probe;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t w = words[r];
        words[r] = (dist[r] <= rmax) ? (w | bit) : (w & ~bit);
    }
}

// counts[b] += rows of [0, N) whose word has bit b, b = 0..63 (counts zeroed by the caller): a wave takes 64 words at a time,
// lane b keeps the population count of the ballot of bit b; integer sums, exact in any order.
__global__ __launch_bounds__(256) void member_count_kernel(const uint64_t* __restrict__ words, int64_t N, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long mine = 0;
    for (int64_t r0 = wave_id * 64; r0 < N; r0 += nwaves * 64) {
        const int64_t r = r0 + lane;
        const uint64_t w = r < N ? words[r] : 0ull;
#pragma unroll
        for (int b = 0; b < 64; ++b) {
            const int c = __popcll(__ballot((w >> b) & 1ull));
            if (lane == b) mine += (unsigned long long)c;
        }
    }
    if (mine) atomicAdd(counts + lane, mine);
}

// The tag form's merge: tags[r] = (tags[r] & ~mask) | sum over p of bit p of words[r] << bits[p]; rows [0, N). bits: [P] on the
// device, distinct, 0..63; mask = the OR of 1 << bits[p].
__global__ __launch_bounds__(256) void member_merge_tags_kernel(uint64_t* __restrict__ tags, const uint64_t* __restrict__ words, int64_t N,
                                                                const int32_t* __restrict__ bits, int P, uint64_t mask) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t w = words[r];
        uint64_t t = tags[r] & ~mask;
        for (int p = 0; p < P; ++p) t |= ((w >> p) & 1ull) << bits[p];
        tags[r] = t;
    }
}

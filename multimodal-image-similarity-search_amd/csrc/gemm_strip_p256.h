// gemm_strip_p256.h — the retrieval score GEMM (GROUPMAX epilogue, gemm256_strip_kernel's contract: a workgroup walks `strip`
// consecutive 256-row tiles of the index for one 256-query tile as ONE K-tile stream) on the K-tile stream of the persistent
// GEMMs (gemm_p256_stream.h; the why: head of gemm_bf16_p256.h): staggered wave halves, buffer-form LDS-DMA with scalar
// offsets, immediates for every LDS address. The epilogue is registers only (16-row group maxima; dense stores or, FILTER,
// rare threshold-passing appends), so the counted waits never have to allow for it. K = D of the index (a multiple of 128).
// This file holds the kernel's hooks — its fp8 W staging and fragment read, its wait counts, its advance —, its epilogue and
// its launcher.
#pragma once
#include <type_traits>
#include "gemm_bf16_256.h"

// eight e4m3 codes (one lane's 8 consecutive k of an fp8 index row) -> the f16 fragment of the MFMA, exactly (e4m3 fits f16)
__device__ __forceinline__ f16x8 p256_widen_f8(u32x2 w) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    f16x8 r;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
        const f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        const h2 l2 = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(lo[0], lo[1]));
        const h2 g2 = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(hi[0], hi[1]));
        r[4 * i + 0] = l2[0]; r[4 * i + 1] = l2[1]; r[4 * i + 2] = g2[0]; r[4 * i + 3] = g2[1];
    }
    return r;
}

// FILTER: 0 = dense group maxima, 1 = (group maximum, group) appended where the maximum reaches the query's tau, 2 = ROW
// threshold pass of the widen pass (api_index.hip sweep_queries): every index row whose score reaches tau_q is appended to
// the query's list flt.buf_g[m][..] (row ids in any order; flt.cnt[m] may run past cap: the excess is dropped and the
// query goes to the exhaustive pass).
// W8 (round 4): the index rows are fp8 (MMISS_F8: e4m3 codes of 128 x) — half the staged bytes per row. A W slot is then
// 128 rows x 64 bytes: one 16-row LDS-DMA piece per wave (lane = row * 4 + 16-byte unit, unit XOR-swizzled by (row >> 2) & 3
// so that the 8-byte fragment reads of rows r, r + 4, r + 8, r + 12 — one bank window — fall on four different chunks), a
// fragment is one ds_read_b64 widened exactly to f16 in registers (p256_widen_f8), the MFMA stays the f16 one with the f16
// queries; scores come out times 128 (the codes' fixed scale) and are scaled back where they leave the registers.

// ---- this kernel's hooks of the K-tile stream
#define KT_READ_A P256S_READ_A16
#define KT_READ_W(b, nq)                                                                                     \
    if constexpr (W8) {                                                                                     \
        _Pragma("unroll") for (int nf = 0; nf < 2; ++nf) {                                                  \
            wq[nq][nf][0] = __builtin_bit_cast(frag, p256_widen_f8(*reinterpret_cast<const u32x2*>(smem + wb[0] + P256S_SLOT(nq, b) + nf * 1024))); \
            wq[nq][nf][1] = __builtin_bit_cast(frag, p256_widen_f8(*reinterpret_cast<const u32x2*>(smem + wb[1] + P256S_SLOT(nq, b) + nf * 1024))); \
        }                                                                                                   \
    } else {                                                                                                \
        P256S_READ_W16(b, nq)                                                                               \
    }
#define KT_MMA P256S_MMA16
// fp8 index rows: a slot is 128 rows x 64 bytes = ONE 16-row piece per wave (the counted waits know: KT_WAIT)
#define KT_STAGE_W(dst, which, b, oW)                                                                        \
    if constexpr (W8) {                                                                                     \
        char* dst8_ = smem + P256S_SLOT(which, b) + wave * 1024;                                            \
        p256s_blds16(srdW, dst8_, w_vo, (oW) + ((which) & 1) * 4 * w_row8);                                 \
    } else {                                                                                                \
        P256S_STAGE_W(dst, which, oW, w_row8)                                                               \
    }
// counted wait `which` (0, 1: behind the A stagings of phases 0 / 1; 3: behind W n1's in phase 3): the pieces of the five younger
// slot loads stay in flight — 6 + 2w, 6 + 2w, 4 + 3w for w operations per W slot and wave: 10 each for w = 2, 8, 8, 7 for
// an fp8 slot's one; POST: + the piece at the pair's head
#define KT_WAIT(POST, b, which) \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((W8 ? ((which) == 3 ? 7 : 8) : 10) + ((POST) ? EX : 0)) : "memory")
#define KT_PHASE3(FIN)
// position t+1 becomes the old t+2; t+2 moves on one K-tile (into the strip's next index tile, or wraps in the last one)
#define KT_ADVANCE()                                                                                         \
    oA1 = oA2; oW1 = oW2;                                                                                   \
    if (++k2 == nt) {                                                                                       \
        k2 = 0;                                                                                             \
        if (o2 + 1 < mine) ++o2;                                                                            \
        oA2 = 0; oW2 = o2 * 256 * K * WELT;                                                                 \
    } else {                                                                                                \
        oA2 += GEMM_BK * (int)sizeof(IN); oW2 += GEMM_BK * WELT;                                            \
    }

template <typename IN, int FILTER, bool W8 = false>
__global__ __launch_bounds__(512, 2) void gemm256s_kernel(const IN* __restrict__ A, const void* __restrict__ Wv, int M, int N, int K,
                                                          int strip, GemmEpi ep, StripFilter flt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef IN IN_T;
    typedef typename MfmaIn<IN>::frag frag;
    static_assert(!W8 || std::is_same<IN, _Float16>::value, "fp8 rows are widened to f16");
    constexpr int WELT = W8 ? 1 : (int)sizeof(IN);
    constexpr float WSCALE = W8 ? 1.0f / 128.0f : 1.0f;
    // fp8 rows carry one inverse norm each (ep.aux, f8_row_inv_kernel): the 64 of a wave's column quarter arrive by a 4-byte
    // LDS-DMA piece per wave into the wave's private 256 bytes behind the staging slots. The piece is issued at the head of
    // EVERY K-tile pair (the current index tile's values again: 256 bytes per wave), so that the operation counts of the
    // waits are the same in every pair — the four waits behind a piece allow for one more operation in flight (the POST
    // form of the waits, EX = 1), the fifth retires it. (Issued once per tile between the K streams, with plain and POST
    // pairs side by side in the loop as in gemm256p_kernel, this kernel spilled 270 registers.)
    constexpr int EX = W8 ? 1 : 0;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fg = lane >> 4;
    const int nbm = M >> 8, nbn = N >> 8;
    const int nt = K / GEMM_BK;
    const int bn_begin = FILTER != 0 ? flt.bn_begin : 0;
    const int nstrips = (nbn - bn_begin + strip - 1) / strip;
    const int wg = xcd_remap(blockIdx.x, nbm * nstrips);
    const int sidx = wg / nbm, bm = wg - sidx * nbm;   // m fastest: the M-tiles of one strip run side by side
    const int bn0 = bn_begin + sidx * strip;
    const int mine = (nbn - bn0 < strip) ? nbn - bn0 : strip;
    const IN* Ab = A + (size_t)bm * 256 * K;
    const char* Wb = reinterpret_cast<const char*>(Wv) + (size_t)bn0 * 256 * K * WELT;  // offsets inside a strip fit 32 bits (strip <= 32 tiles of <= 1 MB)

    const int r_in = lane >> 3, p = lane & 7;
    const int src_chunk = (p ^ r_in) * 8;
    const int a_vo = (((wave >> 2) * 128 + (wave & 3) * 16 + r_in) * K + src_chunk) * (int)sizeof(IN);
    // W slot row r = weight row (r >> 5) * 64 + nq * 32 + (r & 31); a wave stages slot rows 16 * wave .. + 15: as two 8-row
    // pieces of 128-byte rows (f16), or as ONE piece of sixteen 64-byte rows (fp8: lane = 4 * row + unit)
    const int r8 = lane >> 2;   // fp8: the lane's row of the piece
    const int w_vo = W8 ? (((wave >> 1) * 64 + (wave & 1) * 16 + r8) * K + (((lane & 3) ^ ((r8 >> 2) & 3)) << 4))
                        : (((wave >> 1) * 64 + (wave & 1) * 16 + r_in) * K + src_chunk) * (int)sizeof(IN);
    const __amdgpu_buffer_rsrc_t srdA = __builtin_amdgcn_make_buffer_rsrc(const_cast<IN*>(Ab), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t srdW = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(Wb), 0, 0x7fffffff, 0x00020000);
    const int row8 = 8 * K * (int)sizeof(IN);
    const int w_row8 = 8 * K * WELT;
    const int stage_dst = wave * 2048;
    const int mA1 = 8 * row8;
    uint32_t ab[2], wb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        ab[s] = (wm * 64 + fr) * 128 + (((4 * s + fg) ^ (fr & 7)) << 4);
        wb[s] = W8 ? P256S_SLOT(2, 0) + (wn * 32 + fr) * 64 + (((4 * s + fg) ^ (2 * ((fr >> 2) & 3))) << 3)
                   : P256S_SLOT(2, 0) + (wn * 32 + fr) * 128 + (((4 * s + fg) ^ (fr & 7)) << 4);
    }
    frag am[4][2];
    frag wq[2][2][2];
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float tau_r[8];  // FILTER: thresholds of this lane's 8 queries, complete before the stream starts
#pragma unroll
    for (int j = 0; j < 8; ++j) tau_r[j] = INFINITY;
    if constexpr (FILTER != 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = bm * 256 + wm * 128 + j * 16 + fr;
            if (m < ep.m_valid) tau_r[j] = flt.tau[(size_t)m * flt.tau_stride];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(tau_r[j]));
    }

    int oA1 = 0, oW1 = 0, oA2 = GEMM_BK * (int)sizeof(IN), oW2 = GEMM_BK * WELT;
    int o2 = 0, k2 = 1;
    auto stage_inv = [&](int ti_) {   // the inverse norms of index tile bn0 + ti_, this wave's 64 rows (both halves load their copy)
        if constexpr (W8) {
            const float* src = ep.aux + (size_t)(bn0 + ti_) * 256 + wn * 64 + lane;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(smem + G256_LDS + wave * 256), 4, 0, 0);
        }
    };
    // all but the five youngest slot loads (4 + 3w operations: 10, or 7 with one operation per fp8 W slot)
    P256S_PROLOGUE(true, GEMM_BK * (int)sizeof(IN), GEMM_BK * WELT, W8 ? 7 : 10);

    float* out = reinterpret_cast<float*>(ep.out);
    const int npair = nt >> 1;
    for (int ti = 0; ti < mine; ++ti) {
        for (int kp = 0; kp < npair; ++kp) {
            stage_inv(ti);   // (W8; younger than the slots the next four waits retire, older than what the fifth retires)
            P256S_PAIR(W8, false, false);
        }
        // ---- this index tile is complete: group maxima out (the group numbering of gemm256_kernel), accumulators reset.
        // A few hundred cycles of VALU: it runs without leaving the staggered rhythm (each half does it in front of its next
        // read part, the other half is in its MFMAs), and only the index's last tile pays for masking the pad rows.
        const int bn = bn0 + ti;
        const int g = (bn * 4 + wn) * 4 + fg;
        const int n0 = bn * 256 + wn * 64 + 4 * fg;
        const bool whole = (bn + 1) * 256 <= ep.p0;
        asm volatile("s_nop 11" ::: "memory");   // the asm maxima below read the accumulators of the tile's last MFMAs (mm_mfma_settle)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (W8) {
            // scores of fp8 rows: x inv[row] (this wave's own piece: the one issued at the head of the tile's first pair landed
            // behind that pair's fifth wait, later ones rewrite the same bytes)
            const char* ivp = smem + G256_LDS + wave * 256 + fg * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 iv = *reinterpret_cast<const f32x4*>(ivp + i * 64);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = acc[i][j] * iv;
            }
        }
        // Appending to a query's list is an atomic add WITH return (the slot) followed by the stores into that slot. Round 6: the
        // slots of a tile's eight 16-query blocks are requested FIRST — one atomic per (lane, block) that has something to append,
        // for all of the lane's passing rows at once — and used after the last request: one exposed round trip per tile and wave.
        // Requested where they were used (rounds 3-5) they were up to eight sequential round trips of ~0.4 us per tile with the
        // other waves waiting at the next barrier: the widen pass of the bench step took 78 us with 66 rows per query passing,
        // 117 us with 147, against 43 us with 10 (tools/sweep_probe.py, profiles/sweep_r06.txt).
        if constexpr (FILTER == 2) {
            // ... and a lane keeps WHICH of its 16 rows pass as a bit mask: the slow path is 16 compares into the mask, one popcount, one
            // atomic, and later a loop over the set bits (one or two) — as 16 + 16 branches around a counter and a store per block it
            // was ~2500 vector instructions per wave and tile on an index where most blocks have a passing row, two waves per SIMD.
            uint32_t pmask[8];
            int pos[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int m = bm * 256 + wm * 128 + j * 16 + fr;
                float mx = mm_max3(acc[0][j][0], acc[0][j][1], acc[0][j][2]);   // (mm_max*: no canonicalising v_max per operand)
                mx = mm_max3(mx, acc[0][j][3], acc[1][j][0]);
#pragma unroll
                for (int i = 1; i < 4; ++i) {
                    mx = mm_max3(mx, acc[i][j][1], acc[i][j][2]);
                    mx = i < 3 ? mm_max3(mx, acc[i][j][3], acc[i + 1][j][0]) : mm_max2(mx, acc[i][j][3]);
                }
                mx *= WSCALE;   // (fp8 rows: the codes are 128 x the stored values; a power of two, exact)
                uint32_t pm = 0;
                if (mx >= tau_r[j]) {   // rare: some row of this lane's 16 reaches the query's threshold (tau_r = +inf for pad queries)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            pm |= (acc[i][j][r] * WSCALE >= tau_r[j] && (whole || n0 + i * 16 + r < ep.p0)) ? (1u << (i * 4 + r)) : 0u;
                }
                pmask[j] = pm;
                pos[j] = 0;
                if (pm) pos[j] = atomicAdd(flt.cnt + m, __popc(pm));
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t pm = pmask[j];
                if (pm) {
                    const int m = bm * 256 + wm * 128 + j * 16 + fr;
                    int p = pos[j];
                    while (pm) {
                        const int b = __ffs(pm) - 1;
                        pm &= pm - 1;
                        if (p < flt.cap) flt.buf_g[(size_t)m * flt.cap + p] = n0 + (b >> 2) * 16 + (b & 3);
                        ++p;
                    }
                }
            }
            continue;
        }
        // (FILTER = 1: a block's maximum and its slot wait in two of the block's own — consumed, zeroed — accumulator registers
        // until the second loop: sixteen more live registers were four spilled ones)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float mx = -INFINITY;
            if (whole) {
                // 16 values: 8 three-way maxima without the canonicalising v_max per operand (mm_max3, common.h)
                mx = mm_max3(acc[0][j][0], acc[0][j][1], acc[0][j][2]);
                mx = mm_max3(mx, acc[0][j][3], acc[1][j][0]);
#pragma unroll
                for (int i = 1; i < 4; ++i) {
                    mx = mm_max3(mx, acc[i][j][1], acc[i][j][2]);
                    mx = i < 3 ? mm_max3(mx, acc[i][j][3], acc[i + 1][j][0]) : mm_max2(mx, acc[i][j][3]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = (n0 + i * 16 + r < ep.p0) ? acc[i][j][r] : -INFINITY;
                        mx = fmaxf(mx, v);
                        acc[i][j][r] = 0.f;
                    }
            }
            const int m = bm * 256 + wm * 128 + j * 16 + fr;
            mx *= WSCALE;
            if constexpr (FILTER == 1) {
                int pos_ = -1;
                if (mx >= tau_r[j] && mx > -INFINITY)   // (tau_r = +inf for pad queries; -inf maxima = all-pad groups)
                    pos_ = atomicAdd(flt.cnt + m, 1);
                acc[0][j][0] = mx;
                acc[0][j][1] = __int_as_float(pos_);
            } else {
                if (m < ep.m_valid) out[(size_t)m * ep.ldo + g] = mx;
            }
        }
        if constexpr (FILTER == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int m = bm * 256 + wm * 128 + j * 16 + fr;
                const int pos_ = __float_as_int(acc[0][j][1]);
                if (pos_ >= 0 && pos_ < flt.cap) {
                    flt.buf_s[(size_t)m * flt.cap + pos_] = acc[0][j][0];
                    flt.buf_g[(size_t)m * flt.cap + pos_] = g;
                }
                acc[0][j][0] = 0.f;
                acc[0][j][1] = 0.f;
            }
        }
    }
    if (wm == 0) p256s_barrier();   // (the upper half's last barrier: the lower half is still one behind)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
#undef KT_READ_A
#undef KT_READ_W
#undef KT_MMA
#undef KT_STAGE_W
#undef KT_WAIT
#undef KT_PHASE3
#undef KT_ADVANCE

// the strip score GEMM on the staggered loop (same arguments as launch_gemm256_strip; K % 128 == 0). W8: W = fp8 rows (1 B / elt)
template <typename IN, bool W8 = false>
static int launch_gemm256s(hipStream_t st, const void* A, const void* W, const GemmEpi& ep, int M, int N, int K, int strip,
                           const StripFilter* flt = nullptr) {
    if (M <= 0 || N <= 0 || K < 256 || (M % 256) || (N % 256) || (K % 128) || strip < 1 || strip > 32 ||
        (int64_t)strip * 256 * K * (int64_t)sizeof(IN) >= (1LL << 31) || (int64_t)256 * K * (int64_t)sizeof(IN) >= (1LL << 31))
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "gemm256s: M=%d N=%d K=%d strip=%d", M, N, K, strip);
    const int nbn = N / 256;
    if (W8 && !ep.aux) MM_FAIL(MMISS_ERR_ARG, "gemm256s: fp8 rows need their inverse norms (ep.aux)");
    const int lds = G256_LDS + (W8 ? 2048 : 0);   // + 8 waves x 64 inverse norms
    if (flt && (flt->bn_begin < 0 || flt->bn_begin >= nbn || !flt->tau || !flt->cnt || !flt->buf_g || flt->cap <= 0))
        MM_FAIL(MMISS_ERR_ARG, "gemm256s: bad filter");
    const int nwg = (M / 256) * ((nbn - (flt ? flt->bn_begin : 0) + strip - 1) / strip);
    auto launch = [&](auto filter_c) -> int {
        constexpr int FILTER = decltype(filter_c)::value;
        MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&gemm256s_kernel<IN, FILTER, W8>), lds));
        hipLaunchKernelGGL((gemm256s_kernel<IN, FILTER, W8>), dim3(nwg), dim3(512), lds, st, reinterpret_cast<const IN*>(A),
                           W, M, N, K, strip, ep, flt ? *flt : StripFilter{});
        return MMISS_OK;
    };
    if (!flt) MM_TRY(launch(std::integral_constant<int, 0>{}));
    else if (flt->buf_s) MM_TRY(launch(std::integral_constant<int, 1>{}));
    else MM_TRY(launch(std::integral_constant<int, 2>{}));   // (the row threshold pass keeps no scores)
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// gemm_bf16_p256.h — PERSISTENT 256x256x64 bf16 GEMM for the wide GEMMs of the towers (QKV, FC1: N >= 1536), same
// contract as gemm_bf16.h: C[M,N] = A[M,K] * W[N,K]^T + fused epilogue (bf16 out; bias / bias + QuickGELU, optionally behind
// a LayerNorm folded into W).
//
// Why (measurements of round 3 in profiles/gemm_p256_r03.txt): the one-tile-per-workgroup 256x256 kernel
// (gemm_bf16_256.h) pays per tile a pipeline fill from cold, a drain and an epilogue through the staging LDS, all of it with
// every workgroup of the chip in the same state at the same time; and its K loop spends its time NEXT TO the matrix pipe,
// not in it (PMC: matrix cores busy 45 % of a wave's lifetime; ablations: MFMAs, fragment reads, staging and barriers add
// up instead of overlapping). Here the grid is one workgroup per CU and the workgroup owns its tile schedule:
//   * its tiles form ONE continuous K-tile stream: the loads of the next tile's first two K-tiles are issued by the
//     ordinary t+1 / t+2 prefetch of the current tile's last two K-tiles, the epilogue runs while they fly;
//   * two barriers per phase — [fragment reads + one slot's staging + counted wait] B [16 MFMAs] B — and the waves of the
//     lower tile half (wm = 1: waves 4-7, the SIMD partners of waves 0-3) run ONE barrier behind, so that on every SIMD one
//     wave issues MFMAs while its partner reads fragments and stages (guide: the 256^2 8-phase template's staggered wave
//     groups; MICROARCH "two waves per SIMD", item 9);
//   * the loop is unrolled over the two staging buffers: every LDS address is base register + immediate, every LDS-DMA
//     source a scalar base + a per-lane 32-bit offset computed once, staging is unconditional (past the end of the stream
//     it re-reads the last tile into free slots) and the waits are plain immediates — the first version of this loop spent
//     0.3 us per K-tile on scalar bookkeeping alone (round 3, ablation builds since removed: profiles/gemm_p256_r03.txt);
//   * everything the epilogue needs from memory arrives by LDS-DMA as well — the tile's 256 bias / c values (one 4-byte
//     piece per wave) and, in the folded-LayerNorm mode, the raw (sum, sumsq) partials of its 256 rows (K/256 16-byte
//     pieces per wave), finalised to (mean, rstd) by 256 threads in a wait-free phase of K-tile 2 — because an ordinary
//     load beside LDS-DMA makes hipcc drain the whole pipeline (guide §5, trap (b));
//   * the epilogue's stores and those pieces count in vmcnt (in issue order), so the four counted waits that follow an
//     epilogue allow EX more operations in flight; from the fifth wait on every such operation is older than the slot
//     being waited for and the plain count applies again;
//   * tile order: rounds of 256 tiles of a banded global order, 32 logically consecutive tiles (8 row blocks x 4 column
//     tiles) per XCD; a last round of at most 128 tiles is dealt in half tiles so that every CU takes part in it.
// The stream itself — slots, staging, the four-phase K-tile, prologue, tile driver — is gemm_p256_stream.h (shared with
// gemm256s_kernel and gemm256p8_kernel), the deal p256_deal.h; this file holds the kernel's hooks, its epilogue and launcher.
#pragma once
#include <type_traits>
#include "gemm_bf16_256.h"

#define P256_BC (8 * G256_SLOT)       // 2 x 2 KB: bias [256] f32 + c [256] f32 of the current / next tile
#define P256_TABLE (P256_BC + 4096)   // 256 x (mean, rstd)
#define P256_TILES (P256_TABLE + 2048)  // this workgroup's tile list: p256_table_entries packed tiles, decoded once before the K stream
#define P256_RAW (P256_TILES + 256)    // 256 rows x K/64 x (sum, sumsq) f32, as they lie in memory; the epilogue's patches
#define P256_FTAB (P256_RAW + 16384)   // XP = 1 (finished statistics): 2 x 256 x (mean, rstd) of the current / next tile, behind the patches

// Tried and removed (rounds 3-4; numbers in profiles/gemm_p256_r03.txt, profiles/gemm_p256_r04.txt, DESIGN.md sections 3b, 6):
// compile-time ablations of the loop (no MFMAs / staging / fragment reads / barriers / epilogue) — the parts add up instead
// of overlapping; the loop on v_mfma_f32_32x32x16_bf16 — 5-6 % slower; an epilogue of two v_permlane16_swap per 16 x 32 block
// with 64-byte row segments instead of the LDS transpose patch below — equal or slower.
// XP = statistic pieces per wave and tile in the folded modes: K / 256 16-byte pieces of RAW partials (K = 512, 768: finalised
// in the kernel), or 1 = ONE 4-byte piece of FINISHED (mean, rstd) pairs from ep.ln_final (any K; ln_finalize_kernel ran first);
// 0 otherwise
template <int EPI, int XP>
__global__ __launch_bounds__(512, 2) void gemm256p_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ W, int M,
                                                          int N, int K, GemmEpi ep) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __bf16 IN_T;
    typedef bf16x8 frag;
    constexpr bool FOLD = (EPI == MMISS_EPI_LNFOLD_BF16 || EPI == MMISS_EPI_LNFOLD_QGELU_BF16);
    constexpr bool GELU = (EPI == MMISS_EPI_BIAS_QGELU_BF16 || EPI == MMISS_EPI_LNFOLD_QGELU_BF16);
    static_assert(FOLD == (XP > 0), "statistic pieces exist exactly in the folded modes");
    constexpr bool FINAL = FOLD && XP == 1;
    constexpr int EX = 16 + 1 + XP;  // vector-memory operations of a wave between two tiles' K streams
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fg = lane >> 4;
    const int nbm = M >> 8, nbn = N >> 8;
    const int nt = K / GEMM_BK;  // even (K % 128 == 0)

    // ---- this workgroup's tile list (p256_deal.h)
    P256S_BUILD_TILE_LIST(P256_TILES, nbm, nbn, ep.m_fast)

    // ---- LDS-DMA sources, buffer form (one descriptor per operand; slot map: gemm_p256_stream.h): per-lane byte offset of the
    // lane's row / chunk, XOR swizzle on the source chunk
    const int r_in = lane >> 3, p = lane & 7;
    const int src_chunk = (p ^ r_in) * 8;
    const int a_vo = (((wave >> 2) * 128 + (wave & 3) * 16 + r_in) * K + src_chunk) * 2;
    const int w_vo = (((wave >> 1) * 64 + (wave & 1) * 16 + r_in) * K + src_chunk) * 2;
    const __amdgpu_buffer_rsrc_t srdA = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(A), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t srdW = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(W), 0, 0x7fffffff, 0x00020000);
    const int row8 = 8 * K * 2;  // bytes between a slot's two 8-row pieces
    const int stage_dst = wave * 2048;
    // what the epilogue of tile (bm, bn) reads from memory, by LDS-DMA: 1 + XP pieces per wave
    auto stage_x = [&](int bm, int bn, int par) {
        const float* src = ((FOLD && wave >= 4) ? ep.aux : ep.bias) + bn * 256 + (wave & 3) * 64 + lane;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(smem + P256_BC + par * 2048 + wave * 256), 4, 0, 0);
        if constexpr (FINAL) {
            // the tile's 256 x (mean, rstd) = 512 floats, 64 per wave; two tables (as for bias / c): a wave may be here while
            // another is still in the previous tile's epilogue, reading that tile's table
            const float* fs = ep.ln_final + (size_t)bm * 512 + wave * 64 + lane;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)fs,
                                             (__attribute__((address_space(3))) void*)(smem + P256_FTAB + par * 2048 + wave * 256), 4, 0, 0);
        } else if constexpr (FOLD) {
            const char* st = reinterpret_cast<const char*>(ep.ln_stats) + (size_t)bm * 256 * (size_t)(XP * 32) + lane * 16;
#pragma unroll
            for (int q = 0; q < XP; ++q) glds16(st + (wave * XP + q) * 1024, smem + P256_RAW + (wave * XP + q) * 1024);
        }
    };

    // ---- fragment reads: one base per operand and k step + immediate (slot, 16-row sub-tile)
    uint32_t ab[2], wb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        ab[s] = (wm * 64 + fr) * 128 + (((4 * s + fg) ^ (fr & 7)) << 4);
        wb[s] = P256S_SLOT(2, 0) + (wn * 32 + fr) * 128 + (((4 * s + fg) ^ (fr & 7)) << 4);
    }
    frag am[4][2];
    frag wq[2][2][2];
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

// ---- this kernel's hooks of the K-tile stream (gemm_p256_stream.h)
#define KT_READ_A P256S_READ_A16
#define KT_READ_W P256S_READ_W16
#define KT_MMA P256S_MMA16
#define KT_STAGE_W(dst, which, b, oW) P256S_STAGE_W(dst, which, oW, row8)
// counted wait: P256_INFLIGHT = the pieces of the younger slot loads that stay in flight (five slots of two): behind the A
// stagings of phases 0 / 1 and behind W n1's in phase 3 alike (6 + 2w, 6 + 2w, 4 + 3w for w = 2 operations per W slot);
// POST = the stores and pieces of the previous tile's epilogue are younger than the slot waited for
#define P256_INFLIGHT 10
#define KT_WAIT(POST, b, which) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P256_INFLIGHT + ((POST) ? EX : 0)) : "memory")
// FIN = the pair is not the first behind an epilogue; its buffer-0 K-tile is K-tile 2 of the tile when kp == 1 (the raw
// statistics landed behind the waits of K-tile 1): it makes the (mean, rstd) table of the tile's rows in its last, read-free phase
#define KT_PHASE3(FIN)                                                                                       \
    if constexpr (FOLD && !FINAL && (FIN)) {                                                                \
        if (kp == 1 && tid < 256) finalize_stats();                                                         \
    }
#define KT_PAIR_HEAD(kp)
#define KT_AFTER_EPILOGUE()
// position t+1 becomes the old t+2; t+2 moves on one K-tile (into the next tile, or wraps in the last one)
#define KT_ADVANCE()                                                                                         \
    oA1 = oA2; oW1 = oW2; mA1 = mA2;                                                                        \
    if (++k2 == nt) {                                                                                       \
        k2 = 0;                                                                                             \
        if (o2 + 1 < mine) ++o2;                                                                            \
        int bm_, bn_, hf_;                                                                                  \
        p256s_tile_of(smem + P256_TILES, o2, bm_, bn_, hf_);                                                \
        oA2 = bm_ * 256 * K * 2 + (hf_ == 2 ? 8 * row8 : 0);                                                \
        oW2 = bn_ * 256 * K * 2;                                                                            \
        mA2 = hf_ ? 0 : 8 * row8;                                                                           \
    } else {                                                                                                \
        oA2 += GEMM_BK * 2; oW2 += GEMM_BK * 2;                                                             \
    }

    auto finalize_stats = [&]() {  // thread t: (mean, rstd) of the tile's row t from its K/64 partial (sum, sumsq)
        const f32x4* st = reinterpret_cast<const f32x4*>(smem + P256_RAW + tid * (XP * 32));
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int q = 0; q < XP * 2; ++q) { const f32x4 v = st[q]; s1 += v[0] + v[2]; s2 += v[1] + v[3]; }
        const float kd = (float)K;
        const float mean = s1 / kd;
        const float var = fmaxf(s2 / kd - mean * mean, 0.f);
        float* tb = reinterpret_cast<float*>(smem + P256_TABLE);
        tb[2 * tid] = mean;
        tb[2 * tid + 1] = 1.0f / sqrtf(var + ep.ln_eps);
    };

    // ---- stream state
    int cbm, cbn, chalf;   // the tile being computed; chalf: 0 whole tile, 1 / 2 = its m0 / m1 rows only
    p256s_tile_of(smem + P256_TILES, 0, cbm, cbn, chalf);
    int oA1 = cbm * 256 * K * 2 + (chalf == 2 ? 8 * row8 : 0), oW1 = cbn * 256 * K * 2;  // K-tile 0 of tile 0, then position t+1
    int oA2 = oA1 + GEMM_BK * 2, oW2 = oW1 + GEMM_BK * 2;
    int mA1 = chalf ? 0 : 8 * row8, mA2 = mA1;   // where a position's A m1 slot comes from (a half tile has none: m0 again)
    int o2 = 0, k2 = 1;
    const int dump_row = M - 1;  // rows >= m_valid are stored to the last pad row (the store COUNT must not depend on data)

    // prologue: the first tile's epilogue pieces in front of the slots (a half tile's A m1 slot is its m0 rows again, in full)
    stage_x(cbm, cbn, 0);
    P256S_PROLOGUE(true, GEMM_BK * 2, GEMM_BK * 2, P256_INFLIGHT);

    // ---- epilogue of the tile (cbm, cbn) out of the accumulators, JN = 8 (whole tile) or 4 (half tile: 64 rows per wave,
    // hrow = 0 / 64 for its m0 / m1 rows) 16-row sub-tiles per wave. Runs while the next tile's first K-tiles are in flight.
    auto epilogue = [&](auto jn_c, int hrow, int par) {
        constexpr int JN = decltype(jn_c)::value;
        int lane_e = lane;  // (opaque here: what the epilogue derives from the lane id is not kept live through the K loop)
        asm volatile("" : "+v"(lane_e));
        const int fr = lane_e & 15, fg = lane_e >> 4;
        const char* bc = smem + P256_BC + par * 2048;
        f32x4 bias[4], cvec[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bias[i] = *reinterpret_cast<const f32x4*>(bc + (wn * 64 + i * 16 + 4 * fg) * 4);
            if constexpr (FOLD) cvec[i] = *reinterpret_cast<const f32x4*>(bc + 1024 + (wn * 64 + i * 16 + 4 * fg) * 4);
        }
        float mu[JN], rs[JN];
#pragma unroll
        for (int j = 0; j < JN; ++j) {
            mu[j] = 0.f; rs[j] = 1.f;
            if constexpr (FOLD) {
                const float* tb = reinterpret_cast<const float*>(smem + (FINAL ? P256_FTAB + par * 2048 : P256_TABLE)) +
                                  2 * (wm * 128 + hrow + j * 16 + fr);
                mu[j] = tb[0]; rs[j] = tb[1];
            }
        }
        const __amdgpu_buffer_rsrc_t srdO = __builtin_amdgcn_make_buffer_rsrc(ep.out, 0, 0x7fffffff, 0x00020000);
        const int st_pol = ep.nt_out;  // cache policy of the output stores (launch_gemm256p_inst)
        // Each wave transposes 16 rows x 64 columns at a time through a private 2 KB patch (its own share of the raw
        // statistics area, dead since K-tile 2 and refilled by this wave only after these stores). 8-byte slot s of
        // row r lies at slot s ^ 2 (r & 7).
        char* patch = smem + P256_RAW + wave * (XP >= 2 ? XP * 1024 : 2048);  // = the bytes stage_x() of THIS wave refills
        const int rrow = lane_e >> 3, rchunk = lane_e & 7;
        const int wr_off = fr * 128, wr_sw = 2 * (fr & 7);
        const int col = cbn * 256 + wn * 64 + rchunk * 8;
#pragma unroll
        for (int j = 0; j < JN; ++j) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (FOLD) y[r] = rs[j] * (acc[i][j][r] - mu[j] * cvec[i][r]) + bias[i][r];
                    else y[r] = acc[i][j][r] + bias[i][r];
                    if constexpr (GELU) y[r] = quick_gelu(y[r]);
                }
                u32x2 pk;
                pk[0] = pack_bf16x2(y[0], y[1]);
                pk[1] = pack_bf16x2(y[2], y[3]);
                *reinterpret_cast<u32x2*>(patch + wr_off + (((i * 4 + fg) ^ wr_sw) << 3)) = pk;
                acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                const int row = rh * 8 + rrow;
                const u32x4 v = *reinterpret_cast<const u32x4*>(patch + row * 128 + (((2 * rchunk) ^ (2 * (row & 7))) << 3));
                const int m = cbm * 256 + wm * 128 + hrow + j * 16 + row;
                const int vo = ((m < ep.m_valid ? m : dump_row) * ep.ldo + col) * 2;
                if (st_pol == 16) __builtin_amdgcn_raw_buffer_store_b128(v, srdO, vo, 0, 16);   // sc1: written through, dropped from L2
                else if (st_pol == 2) __builtin_amdgcn_raw_buffer_store_b128(v, srdO, vo, 0, 2);      // nt
                else __builtin_amdgcn_raw_buffer_store_b128(v, srdO, vo, 0, 0);
            }
            __builtin_amdgcn_wave_barrier();  // the patch is rewritten by the next j
        }
    };

    const int npair = nt >> 1;
    // ---- whole tiles, then the half tile of the last round
    P256S_RUN_TILES(P256_TILES)
}
#undef KT_READ_A
#undef KT_READ_W
#undef KT_MMA
#undef KT_STAGE_W
#undef P256_INFLIGHT
#undef KT_WAIT
#undef KT_PHASE3
#undef KT_PAIR_HEAD
#undef KT_AFTER_EPILOGUE
#undef KT_ADVANCE

template <int EPI, int XP>
static int launch_gemm256p_inst(hipStream_t st, const void* A, const void* W, const GemmEpi& ep_in, int M, int N, int K) {
    GemmEpi ep = ep_in;
    if (ep.m_fast == 0) ep.m_fast = mmiss_option("gemm_p256_band", 8);  // row blocks per band of the global tile order
    // Cache policy of the output stores: 0 plain, 2 nt, 16 sc1 (written through, not kept in the XCD's L2). Measured equal in
    // time and in fabric reads (FETCH_SIZE x 2 = 119-126 MB per FC1 launch either way): one round of an XCD's 32 tiles streams
    // 4.6 MB of distinct operand bytes through its 4 MB L2, so nothing survives to the next round whatever the stores do.
    ep.nt_out = mmiss_option("gemm_p256_store", 0);
    const int lds = XP == 1 ? P256_FTAB + 4096 : P256_RAW + (XP >= 2 ? XP * 8192 : 16384);  // (the epilogue's transpose patches live in the raw-statistics area)
    const int grid = p256_grid((M / 256) * (N / 256));
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&gemm256p_kernel<EPI, XP>), lds));
    hipLaunchKernelGGL((gemm256p_kernel<EPI, XP>), dim3(grid), dim3(512), lds, st, reinterpret_cast<const __bf16*>(A),
                       reinterpret_cast<const __bf16*>(W), M, N, K, ep);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// can this GEMM run on the persistent kernel? (bf16 output epilogues; the folded forms need K = 512 or 768: the raw
// statistics of a tile must fit beside the staging buffers)
static inline bool gemm256p_ok(int epi, int M, int N, int K, bool final_stats = false) {
    if (M <= 0 || (M % 256) || N <= 0 || (N % 256) || K < 256 || (K % 256)) return false;
    if ((int64_t)(M / 256) * (N / 256) > p256_max_tiles || M / 256 > 0xffff) return false;  // (the tile table and its entries: p256_deal.h)
    if ((int64_t)M * N * 2 >= (1LL << 31) || (int64_t)M * K * 2 >= (1LL << 31) || (int64_t)N * K * 2 >= (1LL << 31)) return false;  // (32-bit buffer offsets)
    if (epi == MMISS_EPI_LNFOLD_BF16 || epi == MMISS_EPI_LNFOLD_QGELU_BF16) return final_stats || K == 512 || K == 768;
    return epi == MMISS_EPI_BIAS_BF16 || epi == MMISS_EPI_BIAS_QGELU_BF16;
}

// M = rows padded to 256 (the output and, in the folded modes, ep.ln_stats must hold M rows); rows >= ep.m_valid are
// computed but land in row M - 1.
static int launch_gemm256p(hipStream_t st, int epi, const void* A, const void* W, const GemmEpi& ep, int M, int N, int K) {
    const bool fold = epi == MMISS_EPI_LNFOLD_BF16 || epi == MMISS_EPI_LNFOLD_QGELU_BF16;
    const bool fin = fold && ep.ln_final != nullptr;
    if (!gemm256p_ok(epi, M, N, K, fin)) MM_FAIL(MMISS_ERR_UNSUPPORTED, "gemm256p: epi=%d M=%d N=%d K=%d", epi, M, N, K);
    if (!ep.out || !ep.bias || (fold && (!ep.aux || (!fin && (!ep.ln_stats || ep.ln_parts * 64 != K)))))
        MM_FAIL(MMISS_ERR_ARG, "gemm256p: missing operand (fold=%d parts=%d)", (int)fold, ep.ln_parts);
    static const char* names[] = {"", "gemm_bf16_bias_p256", "gemm_bf16_bias_qgelu_p256"};
    const int mv = ep.m_valid < M ? ep.m_valid : M;
    const double bytes = 2.0 * ((double)mv * K + (double)N * K) + 2.0 * (double)mv * N;
    MM_PROF(fold ? (epi == MMISS_EPI_LNFOLD_BF16 ? "gemm_bf16_lnfold_bias_p256" : "gemm_bf16_lnfold_qgelu_p256") : names[epi], st,
            gemm_flops(mv, N, K), bytes);
    switch (epi) {
        case MMISS_EPI_BIAS_BF16: return launch_gemm256p_inst<MMISS_EPI_BIAS_BF16, 0>(st, A, W, ep, M, N, K);
        case MMISS_EPI_BIAS_QGELU_BF16: return launch_gemm256p_inst<MMISS_EPI_BIAS_QGELU_BF16, 0>(st, A, W, ep, M, N, K);
        case MMISS_EPI_LNFOLD_BF16:
            if (fin) return launch_gemm256p_inst<MMISS_EPI_LNFOLD_BF16, 1>(st, A, W, ep, M, N, K);
            return K == 768 ? launch_gemm256p_inst<MMISS_EPI_LNFOLD_BF16, 3>(st, A, W, ep, M, N, K)
                            : launch_gemm256p_inst<MMISS_EPI_LNFOLD_BF16, 2>(st, A, W, ep, M, N, K);
        default:
            if (fin) return launch_gemm256p_inst<MMISS_EPI_LNFOLD_QGELU_BF16, 1>(st, A, W, ep, M, N, K);
            return K == 768 ? launch_gemm256p_inst<MMISS_EPI_LNFOLD_QGELU_BF16, 3>(st, A, W, ep, M, N, K)
                            : launch_gemm256p_inst<MMISS_EPI_LNFOLD_QGELU_BF16, 2>(st, A, W, ep, M, N, K);
    }
}

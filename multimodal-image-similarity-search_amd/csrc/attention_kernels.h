// attention_kernels.h — K4: multi-head attention core, head_dim 64:  ctx = softmax(Q K^T * 64^-0.5 (+causal mask)) V
// (HF:modeling_clip.py:259-277,280-335; text mask :543-548). Softmax statistics in fp32 as HF does.
// The one-pass kernels (T <= 128: attention_kernel, attention_heads_kernel), attention_long_kernel (129..288 keys) and the
// routing between them, attention_stream_kernel (attention_stream.h) and attention_tiled_kernel (attention_tiled.h).
// The shared pieces: attention_common.h. Included by encoder_kernels.h.
#pragma once
#include "attention_common.h"
#include "attention_stream.h"

// ------------------------------------------------------------------------------------------------
// One workgroup per (image/text b, head h), 4 waves, each wave owns 16-query tiles.
// Per wave and query tile everything stays in registers:
//   S^T = K Q^T   (MFMA A = K tile from LDS, B = Q fragment from global)  -> lane holds, for ITS query
//                 (lane & 15), keys 4*(lane>>4)+reg of every 16-key tile: the softmax reduction over
//                 keys is in-lane plus two xor-shuffles (16, 32).
//   O^T = V^T P^T (A = V^T via ds_read_b64_tr_b16 from a row-major V image, B = P^T straight from the
//                 S^T accumulator registers: no LDS round trip, no lane movement — guide §3
//                 "An accumulator tile as the next MFMA's operand", with the k order of both
//                 operands permuted the same way).
// NKP = padded key count / 32.
// ------------------------------------------------------------------------------------------------

// One 16-query tile of the one-pass form (T <= 128 keys: all score tiles live in registers). qf = the tile's Q fragments,
// q = this lane's query row, (b, h) only enter through `orow` = ctx row of q at head h, column 4*fg.
// MXOUT (round 6: the fp8 tower of ViT-B/32 — 50 keys — feeds its out-projection MXFP8 rows, as attention_long_kernel does for
// ViT-L/14): instead of bf16 at `orow`, the tile's rows leave as e4m3 at o8row with the scales at srow (att_store_mx_row).
template <int NKP, bool CAUSAL, bool MXOUT = false>
__device__ __forceinline__ void attention_onepass_tile(const char* sK, const char* sV, const bf16x8 (&qf)[2], int q, int T,
                                                       int fr, int fg, uint16_t* orow, uint8_t* o8row = nullptr, uint8_t* srow = nullptr,
                                                       int h = 0, int only_q = -1) {
    f32x4 sacc[2 * NKP];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2 * NKP; ++kt) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        const int krow = kt * 16 + fr;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int chunk = 4 * s + fg;
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + krow * 128 + ((chunk ^ (krow & 7)) << 4));
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], a, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = kt * 16 + 4 * fg + r;
            const bool ok = (key < T) && (!CAUSAL || key <= q);
            a[r] = ok ? a[r] * 0.125f : -INFINITY;
            mx = fmaxf(mx, a[r]);
        }
        sacc[kt] = a;
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2 * NKP; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pexp = __expf(sacc[kt][r] - mx);
            sacc[kt][r] = pexp;
            l += pexp;
        }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);

    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int tq = fr >> 2, tp = fr & 3;  // tr-read address role inside the 16-lane group
#pragma unroll
    for (int ks = 0; ks < NKP; ++ks) {
        u32x4 praw;
        praw[0] = pack_bf16x2(sacc[2 * ks][0], sacc[2 * ks][1]);
        praw[1] = pack_bf16x2(sacc[2 * ks][2], sacc[2 * ks][3]);
        praw[2] = pack_bf16x2(sacc[2 * ks + 1][0], sacc[2 * ks + 1][1]);
        praw[3] = pack_bf16x2(sacc[2 * ks + 1][2], sacc[2 * ks + 1][3]);
        const bf16x8 pf = __builtin_bit_cast(bf16x8, praw);
        // (att_pv_block and att_store_mx_row restated: through the shared functions the MXOUT forms of this tile took 8 more
        // AGPRs and some of them a wave less per SIMD; the compiler's registers are this kernel's whole margin)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const char* a0 = sV + (32 * ks + 4 * fg + tq) * ATT_VSTRIDE + (dt * 16 + 4 * tp) * 2;
            const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (__attribute__((address_space(3))) bf16x4*)(a0));
            const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (__attribute__((address_space(3))) bf16x4*)(a0 + 16 * ATT_VSTRIDE));
            bf16x8 vf;
            vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
            vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
            oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, oacc[dt], 0, 0, 0);
        }
    }
    const float inv = 1.0f / l;
    if constexpr (MXOUT) {
        // (every lane takes part in the block maxima — the four lane groups of a query hold its 64 columns; only valid queries store)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            float o[2][4];
            float amax = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    o[i][r] = oacc[2 * blk + i][r] * inv;
                    amax = fmaxf(amax, fabsf(o[i][r]));
                }
            amax = att_max_over_lane_groups(amax);
            int e8;
            float sinv;
            mx_scale_of(amax, e8, sinv);
            if (q < T) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    *reinterpret_cast<uint32_t*>(o8row + (2 * blk + i) * 16) = pack_fp8x4(o[i][0] * sinv, o[i][1] * sinv, o[i][2] * sinv, o[i][3] * sinv);
                if (fg == 0) srow[mx_scale_offset(2 * h + blk)] = (uint8_t)e8;
            }
        }
    } else if (q < T && (only_q < 0 || q == only_q)) {   // (only_q: the pooled-query form keeps one row of the tile)
        att_store_bf16_row(oacc, inv, orow);
    }
}

template <int NKP, bool CAUSAL, bool MXOUT = false>
__global__ __launch_bounds__(256) void attention_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ ctx, int T, int H,
                                                        uint8_t* __restrict__ ctx8 = nullptr, uint8_t* __restrict__ ctxs = nullptr, int ld_s = 0) {
    static_assert(NKP <= 4, "sequences over 128 keys: attention_long_kernel");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TP = NKP * 32;
    char* sK = smem;             // [TP][128 B] swizzled
    char* sV = smem + TP * 128;  // [TP][ATT_VSTRIDE B] row-major
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int dmodel = H * 64, ld = 3 * dmodel;
    const uint16_t* base = qkv + (size_t)b * T * ld + h * 64;

    constexpr int NW = 4;
    const int fr = lane & 15, fg = lane >> 4;
    // The Q fragments of this wave's first query tile are fetched BEFORE the K/V image is staged: their global latency then
    // overlaps the staging loads instead of following the barrier (the kernel is a chain of dependent latencies, not
    // bandwidth: 3072 workgroups of ~20 KB each at T = 50).
    const int qt_first = wave + NW * blockIdx.y;
    bf16x8 qf_first[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) qf_first[s] = att_load_q(base, ld, qt_first * 16 + fr, T, s, fg);
    att_stage_kv<TP, NW * 64>(base, ld, dmodel, T, tid, sK);
    __syncthreads();

    const int nqt = (T + 15) >> 4;
    // gridDim.y workgroups share one (b, h): small batches split the query tiles so that the grid still fills the chip
    for (int qt = qt_first; qt < nqt; qt += NW * gridDim.y) {
        const int q = qt * 16 + fr;
        bf16x8 qf[2];
        if (qt == qt_first) {
            qf[0] = qf_first[0];
            qf[1] = qf_first[1];
        } else {
#pragma unroll
            for (int s = 0; s < 2; ++s) qf[s] = att_load_q(base, ld, q, T, s, fg);
        }
        if constexpr (MXOUT) {
            const size_t row = (size_t)b * T + (q < T ? q : 0);
            attention_onepass_tile<NKP, CAUSAL, true>(sK, sV, qf, q, T, fr, fg, nullptr, ctx8 + row * dmodel + h * 64 + 4 * fg, ctxs + row * ld_s, h);
        } else {
            attention_onepass_tile<NKP, CAUSAL>(sK, sV, qf, q, T, fr, fg, ctx + ((size_t)b * T + q) * dmodel + h * 64 + 4 * fg);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K4, long sequences (ViT-L/14: 257 keys, LongCLIP text: 248): 8 waves share one staged K/V image (78 KB for 288 padded keys:
// two workgroups per CU). Holding all score tiles of a query tile costs 288 VGPRs, so the scores are walked 32 keys at a time.
// Round 4 (measured on the round-3 form, 128 images x 16 heads, 97-107 us per layer: its two phases ADD — 27 us of K/V
// staging with nothing computing, 78 us of query tiles with nothing loading — and the query tiles are bound by vector +
// matrix issue together, which the second pass over Q K^T that only found the row maxima fed for nothing):
//   * ONE pass, online softmax (att_key_pair_step): the running offset m of a query is raised — and the output tile and the
//     denominator rescaled by exp2((m_old - m_new) c) — only when a new score exceeds it by more than 8 / c (the probabilities
//     then stay below 2^8: bf16 keeps its 8 bits at any magnitude, the sums are f32). After the first key tiles that is rare;
//     the branch is wave-uniform (any lane). The four lanes that hold one query's keys agree on the maximum through two
//     half-wave / 16-lane-row swaps in the vector unit (v_permlane32_swap, v_permlane16_swap), no LDS round trip.
//   * the softmax denominator comes from the matrix cores: a row tile of ones beside V^T sums the bf16 probabilities — the
//     ones the PV product uses — into every register of lacc (no vector add per score, no shuffle at the end).
//   (NOT kept: a workgroup walking several (item, head) pairs with the next pair's K/V rows in flight in registers — 40 more
//   VGPRs at the 128 that four waves per SIMD allow: 90-95 us against 83 without, the query tiles alone 74 against 64.)
//   * raw scores: the 1/8 scale and log2(e) ride in the ONE fma in front of v_exp_f32; key-validity / causal masks only on
//     boundary tiles; causal key tiles above the diagonal skipped; every LDS address a per-lane constant + a tile multiple.
// MXOUT: INSTEAD of the bf16 rows the kernel writes the output as MXFP8 — e4m3 bytes ctx8 [B*T, H*64] and one E8M0 scale per
// (row, 32 columns) in the permuted layout of gemm_fp8.h (ctxs, ld_s bytes per row): att_store_mx_row.
// ------------------------------------------------------------------------------------------------
template <int NKP, bool CAUSAL, bool MXOUT>
__global__ __launch_bounds__(512) void attention_long_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ ctx, int T,
                                                             int H, uint8_t* __restrict__ ctx8, uint8_t* __restrict__ ctxs, int ld_s) {
    static_assert(NKP > 4 && NKP <= 9, "129..288 keys");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TP = NKP * 32;
    constexpr int NW = 8;
    char* sK = smem;             // [TP][128 B] swizzled
    char* sV = smem + TP * 128;  // [TP][ATT_VSTRIDE B] row-major
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dmodel = H * 64, ld = 3 * dmodel;
    const int fr = lane & 15, fg = lane >> 4;
    const int nqt = (T + 15) >> 4;
    // per-lane constants of the LDS addresses (krow & 7 = fr & 7: a key tile starts at a multiple of 16 rows)
    const char* kbase0 = sK + fr * 128 + ((fg ^ (fr & 7)) << 4);
    const char* kbase1 = sK + fr * 128 + (((4 + fg) ^ (fr & 7)) << 4);
    const int tq = fr >> 2, tp = fr & 3;             // tr-read address role inside the 16-lane group
    const char* vbase = sV + (4 * fg + tq) * ATT_VSTRIDE + 8 * tp;   // + ks * 32 rows + dt * 32 bytes (+ 16 rows)
    u32x4 ones_raw = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
    asm volatile("" : "+v"(ones_raw));   // (opaque: kept in four registers instead of three v_mov per key-pair step)
    const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_raw);

    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const uint16_t* base = qkv + (size_t)b * T * ld + h * 64;
    att_stage_kv<TP, NW * 64>(base, ld, dmodel, T, tid, sK);
    __syncthreads();
    // gridDim.y workgroups share one (b, h): small batches split the query tiles so that the grid still fills the chip
    for (int qt = wave + NW * blockIdx.y; qt < nqt; qt += NW * gridDim.y) {
        const int q = qt * 16 + fr;
        bf16x8 qf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) qf[s] = att_load_q(base, ld, q, T, s, fg);
        const int kt_end = CAUSAL ? (qt + 1 < nqt ? qt + 1 : nqt) : nqt;  // key tiles this query tile needs (nqt = ceil(T/16))
        // tiles [0, kt_clean) hold only valid keys for every query of the tile: no mask
        const int kt_clean = CAUSAL ? (qt < (T >> 4) ? qt : (T >> 4)) : (T >> 4);
        auto score_tile = [&](int kt) -> f32x4 {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            const bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(kbase0 + kt * 2048);
            const bf16x8 kf1 = *reinterpret_cast<const bf16x8*>(kbase1 + kt * 2048);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0, qf[0], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1, qf[1], a, 0, 0, 0);
            if (kt >= kt_clean) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt * 16 + 4 * fg + r;
                    const bool ok = (key < T) && (!CAUSAL || key <= q);
                    a[r] = ok ? a[r] : -INFINITY;
                }
            }
            return a;
        };
        float m = -INFINITY;
        f32x4 lacc = {0.f, 0.f, 0.f, 0.f};
        f32x4 oacc[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int npairs = kt_end >> 1;
#pragma unroll 1
        for (int ks = 0; ks < npairs; ++ks) att_key_pair_step<true>(score_tile, ks, vbase + ks * (32 * ATT_VSTRIDE), ones, m, lacc, oacc);
        if (kt_end & 1) att_key_pair_step<false>(score_tile, npairs, vbase + npairs * (32 * ATT_VSTRIDE), ones, m, lacc, oacc);
        const float inv = 1.0f / lacc[0];
        if constexpr (MXOUT) {
            const size_t row = (size_t)b * T + (q < T ? q : 0);
            att_store_mx_row(oacc, inv, q < T, ctx8 + row * dmodel + h * 64 + 4 * fg, ctxs + row * ld_s, h, fg);
        } else if (q < T) {
            att_store_bf16_row(oacc, inv, ctx + ((size_t)b * T + q) * dmodel + h * 64 + 4 * fg);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K4, short sequences at large batch: one workgroup walks HPB heads of one item. With one (item, head) per workgroup the
// kernel is a chain of dependent latencies (PMC at B = 256, T = 50: 65 % of the wave cycles in s_waitcnt, matrix cores 9 %):
// Q/K/V global loads, LDS writes, barrier, 1 us of arithmetic, store - 3072 workgroups of 20 KB each. Here the K/V image of
// head h+1 (and its Q fragments) is in flight in registers while head h is computed from LDS (two LDS images, one barrier
// per head), so a workgroup pays the load latency once instead of HPB times. Same arithmetic, bit-identical output.
// POOLED (the pruned last layer: one query row per item leaves it): only the 16-query tile that holds row pool_row[b] is
// computed — by the wave that owns it in the full form — from the same K/V images, and only that row is stored, into the
// compact ctx [B, H * 64] at row b. No Q rows of the other tiles are read and no other ctx row is written: half the bytes.
// The tile's arithmetic is the full form's, so the row has the same bits.
// ------------------------------------------------------------------------------------------------
template <int NKP, bool CAUSAL, int HPB, bool MXOUT = false, bool POOLED = false>
__global__ __launch_bounds__(256) void attention_heads_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ ctx,
                                                              int T, int H, uint8_t* __restrict__ ctx8 = nullptr,
                                                              uint8_t* __restrict__ ctxs = nullptr, int ld_s = 0,
                                                              const int32_t* __restrict__ pool_row = nullptr) {
    static_assert(!(POOLED && MXOUT), "the pooled-query form writes bf16");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TP = NKP * 32;
    constexpr int IMG = TP * (128 + ATT_VSTRIDE);  // one K + V image
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int groups = H / HPB;
    const int b = blockIdx.x / groups, h0 = (blockIdx.x - b * groups) * HPB;
    const int dmodel = H * 64, ld = 3 * dmodel;
    const uint16_t* item = qkv + (size_t)b * T * ld;
    const int nqt = (T + 15) >> 4;

    // (att_load_kv_piece / att_store_kv_piece and att_load_q restated in the three lambdas: through the shared functions, by
    // value too, four instantiations of this kernel change their VGPR count and four their number of waits)
    constexpr int NIT = TP * 8 / 256;              // 16-byte chunks per thread and operand (TP % 32 == 0)
    u32x4 kr[NIT], vr[NIT];
    auto load_head = [&](int h) {
        const uint16_t* base = item + h * 64;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int idx = tid + i * 256, row = idx >> 3, c = idx & 7;
            kr[i] = u32x4{0u, 0u, 0u, 0u};
            vr[i] = u32x4{0u, 0u, 0u, 0u};
            if (row < T) {
                kr[i] = *reinterpret_cast<const u32x4*>(base + (size_t)row * ld + dmodel + c * 8);
                vr[i] = *reinterpret_cast<const u32x4*>(base + (size_t)row * ld + 2 * dmodel + c * 8);
            }
        }
    };
    auto store_head = [&](int buf) {
        char* sK = smem + buf * IMG;
        char* sV = sK + TP * 128;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int idx = tid + i * 256, row = idx >> 3, c = idx & 7;
            *reinterpret_cast<u32x4*>(sK + row * 128 + ((c ^ (row & 7)) << 4)) = kr[i];
            *reinterpret_cast<u32x4*>(sV + row * ATT_VSTRIDE + (c << 4)) = vr[i];
        }
    };
    auto load_q = [&](int h, int qt, bf16x8 (&qf)[2]) {
        const int q = qt * 16 + fr;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 raw = {0u, 0u, 0u, 0u};
            if (q < T) raw = *reinterpret_cast<const u32x4*>(item + h * 64 + (size_t)q * ld + s * 32 + fg * 8);
            qf[s] = __builtin_bit_cast(bf16x8, raw);
        }
    };

    bf16x8 qf[2], qn[2];
    int pq = 0, pqt = wave;   // POOLED: the item's pooled query and its tile (every wave stages K/V, one wave computes)
    if constexpr (POOLED) {
        pq = __builtin_amdgcn_readfirstlane(pool_row[b]) - b * T;
        pq = pq < 0 ? 0 : (pq >= T ? T - 1 : pq);
        pqt = pq >> 4;
    }
    const bool my_tile = !POOLED || wave == (pqt & 3);
    if constexpr (POOLED) { if (my_tile) load_q(h0, pqt, qf); }
    else load_q(h0, wave, qf);
    load_head(h0);
    store_head(0);
    __syncthreads();
#pragma unroll 1
    for (int hh = 0; hh < HPB; ++hh) {
        const int h = h0 + hh, cur = hh & 1;
        if (hh + 1 < HPB) {  // next head's operands fly during this head's arithmetic
            if constexpr (POOLED) { if (my_tile) load_q(h + 1, pqt, qn); }
            else load_q(h + 1, wave, qn);
            load_head(h + 1);
        }
        const char* sK = smem + cur * IMG;
        const char* sV = sK + TP * 128;
        if constexpr (POOLED) {
            if (my_tile)
                attention_onepass_tile<NKP, CAUSAL>(sK, sV, qf, pqt * 16 + fr, T, fr, fg, ctx + (size_t)b * dmodel + h * 64 + 4 * fg,
                                                    nullptr, nullptr, 0, pq);
        } else
        for (int qt = wave; qt < nqt; qt += 4) {
            const int q = qt * 16 + fr;
            if (qt != wave) load_q(h, qt, qf);  // (T > 64: a wave's second tile)
            if constexpr (MXOUT) {
                const size_t row = (size_t)b * T + (q < T ? q : 0);
                attention_onepass_tile<NKP, CAUSAL, true>(sK, sV, qf, q, T, fr, fg, nullptr, ctx8 + row * dmodel + h * 64 + 4 * fg, ctxs + row * ld_s, h);
            } else
            attention_onepass_tile<NKP, CAUSAL>(sK, sV, qf, q, T, fr, fg, ctx + ((size_t)b * T + q) * dmodel + h * 64 + 4 * fg);
        }
        if (hh + 1 < HPB) {
            store_head(cur ^ 1);  // image cur^1 was last read before the previous barrier
            qf[0] = qn[0];
            qf[1] = qn[1];
        }
        __syncthreads();
    }
}

// K4 above 288 tokens (up to MMISS_MAX_TOKENS): the keys in chunks through two LDS images, attention_tiled_kernel
#include "attention_tiled.h"

// ------------------------------------------------------------------------------------------------ launchers
// The compile-time choices of a launch reach a generic lambda as integral_constant tags:
// CAUSAL (never true where MAY_CAUSAL is false: the MXFP8 forms exist non-causal only) ...
template <bool MAY_CAUSAL, class F>
static int attention_with_causal(bool causal, F&& f) {
    if constexpr (MAY_CAUSAL)
        if (causal) return f(std::true_type{});
    return f(std::false_type{});
}
// ... NKP = padded keys / 32 in LO..HI (the caller has routed T into that range) together with CAUSAL ...
template <int LO, int HI, bool MAY_CAUSAL, class F>
static int attention_with_nkp(int T, bool causal, F&& f) {
    if constexpr (LO < HI)
        if ((T + 31) / 32 > LO) return attention_with_nkp<LO + 1, HI, MAY_CAUSAL>(T, causal, f);
    return attention_with_causal<MAY_CAUSAL>(causal, [&](auto causal_tag) -> int { return f(std::integral_constant<int, LO>{}, causal_tag); });
}
// ... and HPB, the heads per workgroup of attention_heads_kernel (hpb = attention_pick_hpb's 2, 3, 4 or 6).
template <class F>
static int attention_with_hpb(int hpb, F&& f) {
    switch (hpb) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, 6>{});
    }
}

// query-tile splits per (b, h) of the kernels whose `waves` waves walk the query tiles of one staged image: 1 once B*H covers
// the 256 CUs (one ViT-L/14 image: 16 heads x 17 query tiles -> 3 splits = 48 workgroups instead of 16 walking 3 rounds each)
static int attention_query_splits(int items, int T, int waves) {
    const int rounds = ((T + 15) / 16 + waves - 1) / waves;
    const int qs = 256 / items;
    return qs < 1 ? 1 : (qs > rounds ? rounds : qs);
}

// heads per workgroup of the short-sequence kernel (attention_heads_kernel), 1 = one (item, head) per workgroup (attention_kernel):
// several while >= 512 workgroups remain. Option att_hpb: 0 = automatic, 1 = never, 2/3/4/6 = forced (if it divides H)
static int attention_pick_hpb(int B, int H) {
    int hpb = mmiss_option("att_hpb", 0);
    if (hpb == 0) {
        hpb = 1;
        for (int c : {4, 6, 3, 2})  // B = 256, T = 50, H = 12: 1 head 19.3 us, 2: 17.5, 3: 17.2, 4: 16.2, 6: 16.8 (4.9 TB/s)
            if (H % c == 0 && (int64_t)B * (H / c) >= 512) { hpb = c; break; }
    }
    return ((hpb == 2 || hpb == 3 || hpb == 4 || hpb == 6) && H % hpb == 0) ? hpb : 1;
}

// T <= 128, one-pass kernels: several heads per workgroup (attention_heads_kernel) where attention_pick_hpb says so, else one
// (attention_kernel). bf16 rows at ctx or (mx_tag: non-causal) MXFP8 rows at ctx8 / ctxs.
template <bool MXOUT>
static int launch_attention_short(hipStream_t st, const void* qkv, void* ctx, uint8_t* ctx8, uint8_t* ctxs, int ld_s, int B, int T,
                                  int H, bool causal) {
    const int hpb = attention_pick_hpb(B, H);
    return attention_with_nkp<1, 4, !MXOUT>(T, causal, [&](auto nkp_tag, auto causal_tag) -> int {
        constexpr int NKP = decltype(nkp_tag)::value;
        constexpr bool CAUSAL = decltype(causal_tag)::value;
        constexpr int lds = NKP * 32 * (128 + ATT_VSTRIDE);   // one K + V image
        if (hpb > 1)
            return attention_with_hpb(hpb, [&](auto hpb_tag) -> int {
                constexpr int HPB = decltype(hpb_tag)::value;
                MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&attention_heads_kernel<NKP, CAUSAL, HPB, MXOUT>), 2 * lds));
                hipLaunchKernelGGL((attention_heads_kernel<NKP, CAUSAL, HPB, MXOUT>), dim3(B * (H / HPB)), dim3(256), 2 * lds, st,
                                   (const uint16_t*)qkv, (uint16_t*)ctx, T, H, ctx8, ctxs, ld_s);
                MM_HIP(hipGetLastError());
                return MMISS_OK;
            });
        MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&attention_kernel<NKP, CAUSAL, MXOUT>), lds));
        hipLaunchKernelGGL((attention_kernel<NKP, CAUSAL, MXOUT>), dim3(B * H, attention_query_splits(B * H, T, 4)), dim3(256), lds, st,
                           (const uint16_t*)qkv, (uint16_t*)ctx, T, H, ctx8, ctxs, ld_s);
        MM_HIP(hipGetLastError());
        return MMISS_OK;
    });
}

// 129..288 keys
template <bool MXOUT>
static int launch_attention_long(hipStream_t st, const void* qkv, void* ctx, uint8_t* ctx8, uint8_t* ctxs, int ld_s, int B, int T, int H,
                                 bool causal) {
    // round 5: the ViT-L/14 regime on the persistent streaming kernel (attention_stream.h); option attention_stream = 0: this kernel
    if (!causal)
        if (attention_stream_ok(B, T, H, false) && mmiss_option("attention_stream", 1))
            return launch_attention_stream<MXOUT>(st, qkv, ctx, ctx8, ctxs, ld_s, B, H);
    return attention_with_nkp<5, 9, !MXOUT>(T, causal, [&](auto nkp_tag, auto causal_tag) -> int {
        constexpr int NKP = decltype(nkp_tag)::value;
        constexpr bool CAUSAL = decltype(causal_tag)::value;
        constexpr int lds = NKP * 32 * (128 + ATT_VSTRIDE);
        MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&attention_long_kernel<NKP, CAUSAL, MXOUT>), lds));
        hipLaunchKernelGGL((attention_long_kernel<NKP, CAUSAL, MXOUT>), dim3(B * H, attention_query_splits(B * H, T, 8)), dim3(512), lds,
                           st, (const uint16_t*)qkv, (uint16_t*)ctx, T, H, ctx8, ctxs, ld_s);
        MM_HIP(hipGetLastError());
        return MMISS_OK;
    });
}

// attention writing MXFP8: non-causal only (the vision tower), 1..MMISS_MAX_TOKENS keys (round 6: the one-pass kernels too —
// ViT-B/32's 50 keys; above 288 keys: attention_tiled_kernel)
static bool attention_mx_ok(int T, int H) { return T > 0 && T <= MMISS_MAX_TOKENS && H > 0; }
static int launch_attention_mx(hipStream_t st, const void* qkv, uint8_t* ctx8, uint8_t* ctxs, int ld_s, int B, int T, int H) {
    if (B <= 0) return MMISS_OK;
    if (!attention_mx_ok(T, H) || !ctx8 || !ctxs || ld_s < mx_scale_row_bytes(H * 64))
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "attention (MXFP8 output): T=%d (1..%d), H=%d", T, MMISS_MAX_TOKENS, H);
    MM_PROF("attention_mx", st, 4.0 * B * H * (double)T * T * 64, (double)B * T * H * 64 * (2 * 3 + 1));
    if (T <= 128) return launch_attention_short<true>(st, qkv, nullptr, ctx8, ctxs, ld_s, B, T, H, false);
    if (T > 288) return launch_attention_tiled<false, true>(st, qkv, nullptr, ctx8, ctxs, ld_s, B, T, H);
    return launch_attention_long<true>(st, qkv, nullptr, ctx8, ctxs, ld_s, B, T, H, false);
}

// The pruned last layer's attention: does launch_attention pick attention_heads_kernel at this shape? Then its pooled-query
// form can run instead (launch_attention_pooled: ctxc [B, H * 64] row b = the attention output of query pool_row[b] - b * T);
// every other kernel keeps the full attention and the gather behind it.
static bool attention_pooled_ok(int B, int T, int H) {
    return B > 0 && T > 0 && T <= 128 && H > 0 && attention_pick_hpb(B, H) > 1;
}
static int launch_attention_pooled(hipStream_t st, const void* qkv, void* ctxc, const int32_t* pool_row, int B, int T, int H,
                                   bool causal) {
    if (!attention_pooled_ok(B, T, H) || !pool_row) MM_FAIL(MMISS_ERR_UNSUPPORTED, "attention (pooled query): B=%d T=%d H=%d", B, T, H);
    // one query per (item, head): its scores and its output, and the K/V rows the tile reads
    MM_PROF("attention", st, 4.0 * B * H * (double)T * 64, ((double)B * T * H * 64 * 2 + (double)B * H * 64 * 2) * 2);
    const int hpb = attention_pick_hpb(B, H);
    return attention_with_nkp<1, 4, true>(T, causal, [&](auto nkp_tag, auto causal_tag) -> int {
        return attention_with_hpb(hpb, [&](auto hpb_tag) -> int {
            constexpr int NKP = decltype(nkp_tag)::value, HPB = decltype(hpb_tag)::value;
            constexpr bool CAUSAL = decltype(causal_tag)::value;
            constexpr int lds = 2 * NKP * 32 * (128 + ATT_VSTRIDE);
            MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&attention_heads_kernel<NKP, CAUSAL, HPB, false, true>), lds));
            hipLaunchKernelGGL((attention_heads_kernel<NKP, CAUSAL, HPB, false, true>), dim3(B * (H / HPB)), dim3(256), lds, st,
                               (const uint16_t*)qkv, (uint16_t*)ctxc, T, H, (uint8_t*)nullptr, (uint8_t*)nullptr, 0, pool_row);
            MM_HIP(hipGetLastError());
            return MMISS_OK;
        });
    });
}

static int launch_attention(hipStream_t st, const void* qkv, void* ctx, int B, int T, int H, bool causal) {
    if (B <= 0) return MMISS_OK;
    if (T <= 0 || T > MMISS_MAX_TOKENS || H <= 0)
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "attention: T=%d (1..%d), H=%d", T, MMISS_MAX_TOKENS, H);
    // algorithmic flops: QK^T and PV, unpadded, full (non-causal) count as SURVEY.md §8(d) does
    MM_PROF("attention", st, 4.0 * B * H * (double)T * T * 64, (double)B * T * H * 64 * 2 * 4);
    if (T <= 128) return launch_attention_short<false>(st, qkv, ctx, nullptr, nullptr, 0, B, T, H, causal);
    if (T > 288)   // the K/V image of a head no longer fits in LDS: key chunks (attention_tiled.h)
        return attention_with_causal<true>(causal, [&](auto causal_tag) -> int {
            return launch_attention_tiled<decltype(causal_tag)::value, false>(st, qkv, ctx, nullptr, nullptr, 0, B, T, H);
        });
    return launch_attention_long<false>(st, qkv, ctx, nullptr, nullptr, 0, B, T, H, causal);
}

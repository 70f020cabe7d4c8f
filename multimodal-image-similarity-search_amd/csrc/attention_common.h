// attention_common.h — the pieces every K4 kernel is made of (attention_kernels.h: one-pass and long kernels + routing,
// attention_tiled.h: key chunks above 288 tokens, attention_stream.h: the persistent ViT-L/14 kernel). One copy each of the
// LDS layouts, the global -> LDS staging, the fragment loads, the online-softmax key-pair step and the row epilogues.
//
// Shared layouts: a lane is (fr = lane & 15, fg = lane >> 4); fr is its query inside the 16-query tile, fg the group of four
// keys (S^T) / output columns (O^T) it holds. K image: rows of 128 B, the 16-byte chunks XOR-swizzled by (row & 7). V image:
// rows of ATT_VSTRIDE bytes, row-major, read transposed (ds_read_b64_tr_b16).
//
// Three pieces are NOT shared, on purpose (merging them would change instruction counts or bits):
//   * attention_stream_kernel's key-pair step requests its V fragments ahead of the softmax, uses the packed fma, exchanges
//     lanes only inside the rare rescale and reads a swizzled V image: at 16 waves per CU that order is what hides the LDS latency.
//   * attention_stream_kernel's MXFP8 epilogue takes the block maximum of the unnormalised outputs and folds 1 / l into one
//     multiplier per value: half the multiplies of att_store_mx_row for the same bits.
//   * the one-pass tile's maxima and sums go through __shfl_xor: its softmax is two-pass over registers, the maximum is taken
//     once per tile and the masked scores carry the 1/8 scale, so there is no raw-score offset to agree on per step.
// And the one-pass kernels restate a few of the pieces below because the compiler gave them other registers through the
// shared functions (attention_onepass_tile: the PV block and the MXFP8 epilogue; attention_heads_kernel: its staging and Q
// loads) — the comments there name what changed. tools/codeobj_diff.py against the build before is the check for any edit here.
#pragma once
#include "common.h"
#include "gemm_fp8.h"

#define ATT_VSTRIDE 144  // bytes per V row in LDS (128 + 16 pad: spreads the tr-read's 8 rows over banks)

__device__ __forceinline__ float att_max_over_lane_groups(float v) {   // max over lanes l, l ^ 16, l ^ 32, l ^ 48
    uint32_t u = __float_as_uint(v);
    auto r32 = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    v = mm_max2(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
    u = __float_as_uint(v);
    auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return mm_max2(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
}

// K/V staging, 16 bytes per thread, operand and round. One piece: chunk c (8 columns) of key `row` of the head at `base`
// (= qkv row 0 of the item + h * 64), zeros at or beyond T (never read from memory), and its place in an image: K rows of
// 128 B at sK swizzled, V rows of ATT_VSTRIDE B at sV.
// (The loads return values: filling reference parameters, the compiler meets the memory form of these few lines before it
// inlines them, and the kernels come out with other branches, registers and waits than the text written in place gives.
// The step and the epilogues below take their accumulators by reference and compile to the in-place text.)
struct AttKV { u32x4 k, v; };
__device__ __forceinline__ AttKV att_load_kv_piece(const uint16_t* base, int ld, int dmodel, int row, int c, int T) {
    AttKV t = {u32x4{0u, 0u, 0u, 0u}, u32x4{0u, 0u, 0u, 0u}};
    if (row < T) {
        t.k = *reinterpret_cast<const u32x4*>(base + (size_t)row * ld + dmodel + c * 8);
        t.v = *reinterpret_cast<const u32x4*>(base + (size_t)row * ld + 2 * dmodel + c * 8);
    }
    return t;
}
__device__ __forceinline__ void att_store_kv_piece(char* sK, char* sV, int row, int c, const u32x4 kv, const u32x4 vv) {
    *reinterpret_cast<u32x4*>(sK + row * 128 + ((c ^ (row & 7)) << 4)) = kv;
    *reinterpret_cast<u32x4*>(sV + row * ATT_VSTRIDE + (c << 4)) = vv;
}
// The whole image of a head, ROWS padded keys (V behind the K rows), by a workgroup of NTHR threads: the kernels that stage
// one image up front. (The kernels that fetch the next image under the arithmetic of the current one hold the pieces of a
// round in registers between the two calls above.)
template <int ROWS, int NTHR>
__device__ __forceinline__ void att_stage_kv(const uint16_t* base, int ld, int dmodel, int T, int tid, char* sK) {
    for (int idx = tid; idx < ROWS * 8; idx += NTHR) {
        const int row = idx >> 3, c = idx & 7;
        const AttKV t = att_load_kv_piece(base, ld, dmodel, row, c, T);
        att_store_kv_piece(sK, sK + ROWS * 128, row, c, t.k, t.v);
    }
}

// Q fragment s (0, 1) of query q of the head at `base`: the B operand of S^T = K Q^T; zeros for q >= T
__device__ __forceinline__ bf16x8 att_load_q(const uint16_t* base, int ld, int q, int T, int s, int fg) {
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (q < T) raw = *reinterpret_cast<const u32x4*>(base + (size_t)q * ld + s * 32 + fg * 8);
    return __builtin_bit_cast(bf16x8, raw);
}

// O^T += V^T P^T over the 32 keys of one PV MFMA. vks = this lane's tr-read address in the V row-major image:
// row 32 ks + 4 fg + (fr >> 2), byte 8 (fr & 3); pf = the probabilities, element j < 4 = key 32 ks + 4 fg + j,
// j >= 4 = key 32 ks + 16 + 4 fg + (j - 4).
__device__ __forceinline__ void att_pv_block(const char* vks, const bf16x8& pf, f32x4 (&oacc)[4]) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const char* a0 = vks + dt * 32;
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

// The raw-score scale of the online softmax: exp2((s - m) c) is what enters P, and the offset m may lag the maximum by
// 8 binary orders (deferred rescale: the probabilities stay below 2^8, bf16 keeps its 8 bits at any magnitude).
#define ATT_C_EXP (0.125f * 1.4426950408889634f)
#define ATT_THR_RAW (8.0f / ATT_C_EXP)

// One online-softmax step of attention_long_kernel and attention_tiled_kernel = two key tiles (the 32 keys of one PV MFMA);
// an odd last tile is a step of its own (PAIR = false: second tile -inf). score_tile(t) = the masked raw scores of key
// tile t (f32x4, S^T layout), vks as att_pv_block's, `ones` a bf16 tile of ones (the denominator comes from the matrix cores).
// m = this query's offset (raw score units), lacc = its denominator in every register, oacc = its four output tiles.
template <bool PAIR, class ScoreTile>
__device__ __forceinline__ void att_key_pair_step(ScoreTile&& score_tile, int ks, const char* vks, const bf16x8& ones, float& m,
                                                  f32x4& lacc, f32x4 (&oacc)[4]) {
    const float c_exp = ATT_C_EXP, thr_raw = ATT_THR_RAW;
    f32x4 p0 = score_tile(2 * ks), p1;
    if constexpr (PAIR) p1 = score_tile(2 * ks + 1);
    else p1 = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if constexpr (PAIR) mm_mfma_settle("+v"(p0), "+v"(p1));   // (the asm maxima below read MFMA results: common.h)
    else mm_mfma_settle("+v"(p0));
    float lm = mm_max3(p0[0], p0[1], p0[2]);
    if constexpr (PAIR) lm = mm_max3(mm_max3(lm, p0[3], p1[0]), p1[1], mm_max2(p1[2], p1[3]));
    else lm = mm_max2(lm, p0[3]);
    lm = att_max_over_lane_groups(lm);   // the same value in the four lanes of a query
    if (__any(lm > m + thr_raw)) {       // (m = -inf at the first step: taken, alpha = 0 on zeros)
        const float mn = (lm > m + thr_raw) ? lm : m;
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * c_exp);   // 1 where the offset stays; exp2(-inf) = 0
        m = mn;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[dt][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 4; ++r) lacc[r] *= alpha;
    }
    const float mc = m * c_exp;
#pragma unroll
    for (int r = 0; r < 4; ++r) p0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(p0[r], c_exp, -mc));
#pragma unroll
    for (int r = 0; r < 4; ++r) p1[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(p1[r], c_exp, -mc));
    u32x4 praw;
    praw[0] = pack_bf16x2(p0[0], p0[1]);
    praw[1] = pack_bf16x2(p0[2], p0[3]);
    praw[2] = pack_bf16x2(p1[0], p1[1]);
    praw[3] = pack_bf16x2(p1[2], p1[3]);
    const bf16x8 pf = __builtin_bit_cast(bf16x8, praw);
    lacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, lacc, 0, 0, 0);
    att_pv_block(vks, pf, oacc);
}

// The output tile of one query leaves as a bf16 row: orow = ctx row of the query at head h, column 4 fg (the caller holds
// the store to valid queries).
__device__ __forceinline__ void att_store_bf16_row(const f32x4 (&oacc)[4], float inv, uint16_t* orow) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        u32x2 pk;
        pk[0] = pack_bf16x2(oacc[dt][0] * inv, oacc[dt][1] * inv);
        pk[1] = pack_bf16x2(oacc[dt][2] * inv, oacc[dt][3] * inv);
        *reinterpret_cast<u32x2*>(orow + dt * 16) = pk;
    }
}

// ... or as MXFP8 (the fp8 vision tower's out-projection on the block-scaled fp8 GEMM): e4m3 bytes at o8row (= ctx8 row of the
// query at head h, column 4 fg) and one E8M0 scale per (query, 32 columns) at srow[mx_scale_offset(2 h + block)] (srow = the
// row's scale bytes in the permuted layout of gemm_fp8.h). A (query, head) holds two 32-column blocks (output tiles 0,1 /
// 2,3 of O^T); a lane has 8 values of each, the block maximum is lane-local plus the exchange over the four lane groups —
// so EVERY lane of the wave calls this, and only those with `valid` (q < T) store.
__device__ __forceinline__ void att_store_mx_row(const f32x4 (&oacc)[4], float inv, bool valid, uint8_t* o8row, uint8_t* srow,
                                                 int h, int fg) {
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
        if (valid) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                *reinterpret_cast<uint32_t*>(o8row + (2 * blk + i) * 16) = pack_fp8x4(o[i][0] * sinv, o[i][1] * sinv, o[i][2] * sinv, o[i][3] * sinv);
            if (fg == 0) srow[mx_scale_offset(2 * h + blk)] = (uint8_t)e8;
        }
    }
}

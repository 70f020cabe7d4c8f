// attention_tiled.h — K4 above 288 tokens (ViT-L/14@336 and ViT-B/16@384: 577 tokens, L/14@448: 1025): the keys arrive in
// chunks. Part of the attention header family (attention_kernels.h): the LDS layouts, the staging pieces, the key-pair step
// and the epilogues are attention_common.h's, shared with attention_long_kernel.
//
// attention_long_kernel stages the whole K/V image of an (item, head) in LDS — 272 B per key, 78 KB at 288 padded keys, more
// than a CU has at 577. Here:
//   * a workgroup = 8 waves = one (item, head) x one block of 8 query tiles (128 queries); grid (B * H, ceil(ceil(T / 16) / 8)).
//     A wave owns ONE query tile for the whole launch: its Q fragments, offset m, denominator lacc and the four output tiles
//     stay in registers across all keys.
//   * K/V come in chunks of ATT_TILED_CHUNK = 128 keys into one of two LDS images (2 x 34 KB: two workgroups per CU), in the
//     long kernel's layouts: K rows of 128 B with the 16-byte chunks XOR-swizzled by (row & 7), V rows at ATT_VSTRIDE for the
//     transposing read. The next chunk's rows are fetched global -> registers (4 x 16 B per thread) in front of the current
//     chunk's key steps and written to the other image behind them (the image was last read before the previous barrier);
//     one barrier per chunk. Rows at or beyond T are zero-filled and never read from memory.
//   * per query tile the arithmetic is attention_long_kernel's step, 32 keys at a time with the key tile index offset by the
//     chunk: the chunk is a multiple of 32 keys, so no operation changes its place in the order, and at T <= 288 the output
//     has the long kernel's bits (tests/test_attention_tiled_gpu.py holds it to that).
//   * the chunk count is workgroup-uniform (causal: up to the last chunk the block's highest query tile needs). A wave whose
//     query tile lies beyond ceil(T / 16) stages its share of every chunk and meets every barrier; it only skips the key
//     steps and the store. There is no early return.
#pragma once
#include "attention_common.h"

#define ATT_TILED_CHUNK 128                                        // keys per LDS image (a multiple of 32)
#define ATT_TILED_IMG (ATT_TILED_CHUNK * (128 + ATT_VSTRIDE))      // one K + V image

template <bool CAUSAL, bool MXOUT>
__global__ __launch_bounds__(512) void attention_tiled_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ ctx, int T,
                                                              int H, uint8_t* __restrict__ ctx8, uint8_t* __restrict__ ctxs, int ld_s) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int C = ATT_TILED_CHUNK, IMG = ATT_TILED_IMG;
    constexpr int NW = 8;
    constexpr int CT = C / 16;                       // key tiles per chunk (even: a pair never straddles a chunk seam)
    constexpr int NIT = C * 8 / (NW * 64);           // 16-byte pieces per thread and operand
    static_assert(C % 32 == 0 && (C * 8) % (NW * 64) == 0, "chunk: whole key pairs, whole staging rounds");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dmodel = H * 64, ld = 3 * dmodel;
    const int fr = lane & 15, fg = lane >> 4;
    const int nqt = (T + 15) >> 4;
    // per-lane constants of the LDS addresses inside an image (krow & 7 = fr & 7: a key tile starts at a multiple of 16 rows)
    const int kb0 = fr * 128 + ((fg ^ (fr & 7)) << 4);
    const int kb1 = fr * 128 + (((4 + fg) ^ (fr & 7)) << 4);
    const int tq = fr >> 2, tp = fr & 3;             // tr-read address role inside the 16-lane group
    const int vb = C * 128 + (4 * fg + tq) * ATT_VSTRIDE + 8 * tp;   // + ks * 32 rows + dt * 32 bytes (+ 16 rows)
    u32x4 ones_raw = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
    asm volatile("" : "+v"(ones_raw));
    const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_raw);

    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const uint16_t* base = qkv + (size_t)b * T * ld + h * 64;
    const int qt = wave + NW * blockIdx.y;           // this wave's query tile
    const bool active = qt < nqt;                    // (wave-uniform; the last block of an item may hold idle waves)
    const int q = qt * 16 + fr;

    // workgroup-uniform: the key tiles the block's highest query tile needs, in chunks
    const int qt_hi = (NW * blockIdx.y + NW - 1 < nqt - 1) ? NW * blockIdx.y + NW - 1 : nqt - 1;
    const int kt_block = CAUSAL ? qt_hi + 1 : nqt;
    const int nch = (kt_block + CT - 1) / CT;

    u32x4 kr[NIT], vr[NIT];
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int idx = tid + i * (NW * 64);
            const AttKV t = att_load_kv_piece(base, ld, dmodel, ch * C + (idx >> 3), idx & 7, T);
            kr[i] = t.k;
            vr[i] = t.v;
        }
    };
    auto store_chunk = [&](int buf) {
        char* sK = smem + buf * IMG;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int idx = tid + i * (NW * 64);   // row idx >> 3 < C
            att_store_kv_piece(sK, sK + C * 128, idx >> 3, idx & 7, kr[i], vr[i]);
        }
    };

    bf16x8 qf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) qf[s] = att_load_q(base, ld, q, T, s, fg);
    load_chunk(0);
    store_chunk(0);
    __syncthreads();

    const int kt_end = CAUSAL ? (qt + 1 < nqt ? qt + 1 : nqt) : nqt;  // key tiles this query tile needs (nqt = ceil(T/16))
    // tiles [0, kt_clean) hold only valid keys for every query of the tile: no mask
    const int kt_clean = CAUSAL ? (qt < (T >> 4) ? qt : (T >> 4)) : (T >> 4);
    float m = -INFINITY;   // this query's offset (raw score units): exp2((s - m) c) is what enters P
    f32x4 lacc = {0.f, 0.f, 0.f, 0.f};
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch) {
        const bool more = ch + 1 < nch;              // (workgroup-uniform)
        if (more) load_chunk(ch + 1);                // the next chunk's rows fly during this chunk's key steps
        const char* img = smem + (ch & 1) * IMG;
        const int kt0 = ch * CT;                     // first key tile of the chunk
        // lt = key tile inside the chunk, kt0 + lt = the key tile of the sequence (masks)
        auto score_tile = [&](int lt) -> f32x4 {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            const bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(img + kb0 + lt * 2048);
            const bf16x8 kf1 = *reinterpret_cast<const bf16x8*>(img + kb1 + lt * 2048);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0, qf[0], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1, qf[1], a, 0, 0, 0);
            if (kt0 + lt >= kt_clean) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = (kt0 + lt) * 16 + 4 * fg + r;
                    const bool ok = (key < T) && (!CAUSAL || key <= q);
                    a[r] = ok ? a[r] : -INFINITY;
                }
            }
            return a;
        };
        if (active) {
            // this wave's key tiles inside the chunk: [0, nt), odd only in the wave's last chunk
            int nt = kt_end - kt0;
            nt = nt < 0 ? 0 : (nt > CT ? CT : nt);
            const int npairs = nt >> 1;
#pragma unroll 1
            for (int ks = 0; ks < npairs; ++ks) att_key_pair_step<true>(score_tile, ks, img + vb + ks * (32 * ATT_VSTRIDE), ones, m, lacc, oacc);
            if (nt & 1) att_key_pair_step<false>(score_tile, npairs, img + vb + npairs * (32 * ATT_VSTRIDE), ones, m, lacc, oacc);
        }
        if (more) store_chunk((ch + 1) & 1);         // image (ch + 1) & 1 was last read before the previous barrier
        __syncthreads();
    }

    if (active) {
        const float inv = 1.0f / lacc[0];
        if constexpr (MXOUT) {
            const size_t row = (size_t)b * T + (q < T ? q : 0);
            att_store_mx_row(oacc, inv, q < T, ctx8 + row * dmodel + h * 64 + 4 * fg, ctxs + row * ld_s, h, fg);
        } else if (q < T) {
            att_store_bf16_row(oacc, inv, ctx + ((size_t)b * T + q) * dmodel + h * 64 + 4 * fg);
        }
    }
}

// grid (B * H, blocks of 8 query tiles); option-free: the route is decided by T alone (launch_attention / launch_attention_mx)
template <bool CAUSAL, bool MXOUT>
static int launch_attention_tiled(hipStream_t st, const void* qkv, void* ctx, uint8_t* ctx8, uint8_t* ctxs, int ld_s, int B, int T,
                                  int H) {
    const int lds = 2 * ATT_TILED_IMG;
    const int blocks = ((T + 15) / 16 + 7) / 8;
    MM_TRY(mmiss_ensure_dyn_lds(reinterpret_cast<const void*>(&attention_tiled_kernel<CAUSAL, MXOUT>), lds));
    hipLaunchKernelGGL((attention_tiled_kernel<CAUSAL, MXOUT>), dim3(B * H, blocks), dim3(512), lds, st, (const uint16_t*)qkv,
                       (uint16_t*)ctx, T, H, ctx8, ctxs, ld_s);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

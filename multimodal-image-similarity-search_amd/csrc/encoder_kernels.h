// encoder_kernels.h — the non-GEMM kernels of the CLIP towers (K1 prologue, K2, K4, K8, K9 of
// SURVEY.md §2.2). Each kernel cites the HF arithmetic it restates.
#pragma once
#include "common.h"
#include "attention_stream.h"  // (first: attention_stream_kernel leads the code object, the other attention kernels follow K2)

// ------------------------------------------------------------------------------------------------
// K1 prologue: patchify.  pixels f32 [B,3,S,S] -> patches bf16 [B*G*G, Kp], k = c*P*P + ky*P + kx
// (the flatten order of nn.Conv2d's weight [d,3,P,P], HF:modeling_clip.py:148-154,209-211), zero
// padded from 3*P*P to Kp. One thread produces 8 consecutive k (one 16-byte store).
// SRC_U8: pixels are uint8 [B,S,S,3] HWC and the CLIP rescale+normalise
// ((x/255 - mean)/std, HF:image_processing_clip.py:23-34) is fused in.
// ------------------------------------------------------------------------------------------------
template <bool SRC_U8>
__global__ __launch_bounds__(256) void im2col_kernel(const void* __restrict__ pixels, uint16_t* __restrict__ out,
                                                     int B, int S, int P, int Kp) {
    const int G = S / P;
    const int PP = P * P;
    const int Kreal = 3 * PP;
    const int kgroups = Kp >> 3;
    const int64_t total = (int64_t)B * G * G * kgroups;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float istd[3] = {1.0f / 0.26862954f, 1.0f / 0.26130258f, 1.0f / 0.27577711f};
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int kg = (int)(idx % kgroups);
        const int64_t m = idx / kgroups;
        const int b = (int)(m / (G * G));
        const int pr = (int)(m - (int64_t)b * G * G);
        const int py = pr / G, px = pr - py * G;
        const int k0 = kg << 3;
        float v[8];
        if (!SRC_U8 && (P & 7) == 0 && k0 < Kreal) {
            // 8 consecutive kx of one (c, ky): two float4 loads
            const int c = k0 / PP, rem = k0 - c * PP, ky = rem / P, kx = rem - ky * P;
            const float* src = reinterpret_cast<const float*>(pixels) +
                               (((size_t)b * 3 + c) * S + (size_t)py * P + ky) * S + (size_t)px * P + kx;
            const f32x4 a = *reinterpret_cast<const f32x4*>(src);
            const f32x4 d = *reinterpret_cast<const f32x4*>(src + 4);
            v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
            v[4] = d[0]; v[5] = d[1]; v[6] = d[2]; v[7] = d[3];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = k0 + e;
                float x = 0.f;
                if (k < Kreal) {
                    const int c = k / PP, rem = k - c * PP, ky = rem / P, kx = rem - ky * P;
                    const size_t y = (size_t)py * P + ky, xx = (size_t)px * P + kx;
                    if (SRC_U8) {
                        const uint8_t u = reinterpret_cast<const uint8_t*>(pixels)[(((size_t)b * S + y) * S + xx) * 3 + c];
                        // same op order as the HF processor: rescale (x * 1/255) then (x - mean) / std
                        x = ((float)u * (1.0f / 255.0f) - mean[c]) * istd[c];
                    } else {
                        x = reinterpret_cast<const float*>(pixels)[(((size_t)b * 3 + c) * S + y) * S + xx];
                    }
                }
                v[e] = x;
            }
        }
        u32x4 pk;
        pk[0] = pack_bf16x2(v[0], v[1]);
        pk[1] = pack_bf16x2(v[2], v[3]);
        pk[2] = pack_bf16x2(v[4], v[5]);
        pk[3] = pack_bf16x2(v[6], v[7]);
        *reinterpret_cast<u32x4*>(out + (size_t)m * Kp + k0) = pk;
    }
}

// CLS rows: x[b*T + 0][:] = class_embedding + position_embedding[0]   (HF:modeling_clip.py:213-216)
__global__ void cls_rows_kernel(float* __restrict__ x, const float* __restrict__ cls, const float* __restrict__ pos,
                                int B, int T, int d) {
    const int64_t total = (int64_t)B * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / d), n = (int)(i - (int64_t)b * d);
        x[(size_t)b * T * d + n] = cls[n] + pos[n];
    }
}

// One request at a time (round 5): the vision tower's CLS rows, pre_layrnorm and the entry statistics of the skinny folded mode
// in ONE launch instead of three (cls_rows_kernel, layernorm_kernel in place, skinny_row_stats16_kernel). One wave per token row:
// row t = 0 of an image is class_embedding + position_embedding[0] (HF:modeling_clip.py:213-216) computed here, the others
// were written by the patch GEMM; LayerNorm with layernorm_kernel's arithmetic (two-pass mean / variance, the same lane
// layout and summation order), the result written back as the f32 residual stream, as its bf16 copy, and as the (sum, sumsq)
// of every 16-column slice (four consecutive lanes: skinny_row_stats16_kernel's order) — the same bits as the three kernels.
__global__ __launch_bounds__(256) void prelayernorm_skinny_kernel(float* __restrict__ x, const float* __restrict__ cls,
                                                                  const float* __restrict__ pos, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, uint16_t* __restrict__ xb,
                                                                  float* __restrict__ stats, int M, int T, int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const bool is_cls = (r % T) == 0;
    float* xr = x + (size_t)r * d;
    f32x4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < d) {
            if (is_cls) v[i] = *reinterpret_cast<const f32x4*>(cls + c) + *reinterpret_cast<const f32x4*>(pos + c);
            else v[i] = *reinterpret_cast<const f32x4*>(xr + c);
        }
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < d) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = v[i][e] - mean;
                q += t * t;
            }
        }
    }
    const float var = wave_sum(q) / (float)d;
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;   // (wave-uniform validity per i: d % 256 == 0 is not required, d % 16 == 0 is)
        f32x4 y = {0.f, 0.f, 0.f, 0.f};
        if (c < d) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(beta + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * g[e] + bb[e];
            *reinterpret_cast<f32x4*>(xr + c) = y;
            u32x2 pk;
            pk[0] = pack_bf16x2(y[0], y[1]);
            pk[1] = pack_bf16x2(y[2], y[3]);
            *reinterpret_cast<u32x2*>(xb + (size_t)r * d + c) = pk;
        }
        float ss = (y[0] + y[1]) + (y[2] + y[3]);
        float qq = (y[0] * y[0] + y[1] * y[1]) + (y[2] * y[2] + y[3] * y[3]);
        ss += __shfl_xor(ss, 1); qq += __shfl_xor(qq, 1);
        ss += __shfl_xor(ss, 2); qq += __shfl_xor(qq, 2);
        if (c < d && (lane & 3) == 0) {
            float* o = stats + ((size_t)r * (d >> 4) + (c >> 4)) * 2;
            o[0] = ss;
            o[1] = qq;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K9: text embeddings.  x[b*T+t][:] = token_embedding[ids[b,t]] + position_embedding[t]
// (HF:modeling_clip.py:226-256). Also finds the pooled position per row: first id == eos_id, or
// argmax(ids) when eos_id == 2 (legacy checkpoints) — HF:modeling_clip.py:561-581.
// One block per (b); threads stride over t*d.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                         const float* __restrict__ pos, float* __restrict__ x,
                                                         int32_t* __restrict__ pool_row, int T, int d, int vocab,
                                                         int eos_id) {
    const int b = blockIdx.x;
    const int32_t* row = ids + (size_t)b * T;
    if (threadIdx.x == 0) {
        int pos_eos = 0;
        if (eos_id == 2) {
            int best = row[0];
            for (int t = 1; t < T; ++t)
                if (row[t] > best) { best = row[t]; pos_eos = t; }
        } else {
            // (ids == eos).int().argmax(): first match, 0 when there is none
            for (int t = 0; t < T; ++t)
                if (row[t] == eos_id) { pos_eos = t; break; }
        }
        pool_row[b] = b * T + pos_eos;
    }
    const int dv = d >> 2;
    for (int i = threadIdx.x; i < T * dv; i += blockDim.x) {
        const int t = i / dv, c = (i - t * dv) << 2;
        int id = row[t];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        const f32x4 e = *reinterpret_cast<const f32x4*>(tok + (size_t)id * d + c);
        const f32x4 p = *reinterpret_cast<const f32x4*>(pos + (size_t)t * d + c);
        *reinterpret_cast<f32x4*>(x + ((size_t)b * T + t) * d + c) = e + p;
    }
}

// vision pooled row = token 0 of every image (HF:modeling_clip.py:650-651)
__global__ void vision_pool_rows_kernel(int32_t* pool_row, int B, int T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) pool_row[i] = i * T;
}

// ------------------------------------------------------------------------------------------------
// K2: LayerNorm (eps inside the sqrt, affine; fp32 statistics) — F.layer_norm as used by
// pre_layrnorm / layer_norm1 / layer_norm2 / post_layernorm / final_layer_norm
// (HF:modeling_clip.py:358-360,605-607,504). One wave per row, the row held in registers
// (d <= 1024), two-pass mean / variance. rowmap (optional) gathers input rows: out row r reads
// x row rowmap[r]  (K8's pooling).
// ------------------------------------------------------------------------------------------------
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, void* __restrict__ out,
                                                        const int32_t* __restrict__ rowmap, int M, int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const size_t in_row = rowmap ? (size_t)rowmap[r] : (size_t)r;
    const float* xr = x + in_row * d;
    f32x4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = (c < d) ? *reinterpret_cast<const f32x4*>(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < d) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = v[i][e] - mean;
                q += t * t;
            }
        }
    }
    const float var = wave_sum(q) / (float)d;
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < d) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(beta + c);
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * g[e] + bb[e];
            if constexpr (OUT_BF16) {
                u32x2 pk;
                pk[0] = pack_bf16x2(y[0], y[1]);
                pk[1] = pack_bf16x2(y[2], y[3]);
                *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(out) + (size_t)r * d + c) = pk;
            } else {
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + (size_t)r * d + c) = y;
            }
        }
    }
}

// The same LayerNorm for a bf16 residual stream (bf16 in, bf16 out; d % 8 == 0, d <= 1024): a lane owns 8 consecutive
// elements per 512-column half, one 16-byte load and one 16-byte store each (the 8-byte form of the f32 kernel's layout
// ran at 4.6 TB/s: half the bytes per load instruction in flight). Widening is exact; same two-pass statistics.
// A wave normalises TWO rows, all four of its loads issued before the first use (the kernel is latency-bound: bytes in
// flight per CU, not arithmetic, set its rate).
__global__ __launch_bounds__(256) void layernorm16_kernel(const uint16_t* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, uint16_t* __restrict__ out, int M,
                                                          int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
    if (r0 >= M) return;
    u32x4 w[2][2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int r = (r0 + rr < M) ? r0 + rr : r0;  // (an odd last row is computed twice, stored once)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = (i * 64 + lane) * 8;
            w[rr][i] = u32x4{0u, 0u, 0u, 0u};
            if (c < d) w[rr][i] = *reinterpret_cast<const u32x4*>(x + (size_t)r * d + c);
        }
    }
    f32x4 g[2][2], bb[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < d) {
            g[i][0] = *reinterpret_cast<const f32x4*>(gamma + c); g[i][1] = *reinterpret_cast<const f32x4*>(gamma + c + 4);
            bb[i][0] = *reinterpret_cast<const f32x4*>(beta + c); bb[i][1] = *reinterpret_cast<const f32x4*>(beta + c + 4);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int r = r0 + rr;
        float v[2][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[i][2 * e] = __uint_as_float(w[rr][i][e] << 16);
                v[i][2 * e + 1] = __uint_as_float(w[rr][i][e] & 0xFFFF0000u);
                s += v[i][2 * e] + v[i][2 * e + 1];
            }
        const float mean = wave_sum(s) / (float)d;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if ((i * 64 + lane) * 8 < d) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float t = v[i][e] - mean;
                    q += t * t;
                }
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
        if (r >= M) continue;  // wave-uniform
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = (i * 64 + lane) * 8;
            if (c < d) {
                float y[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    y[e] = (v[i][e] - mean) * rstd * g[i][0][e] + bb[i][0][e];
                    y[4 + e] = (v[i][4 + e] - mean) * rstd * g[i][1][e] + bb[i][1][e];
                }
                u32x4 pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk[e] = pack_bf16x2(y[2 * e], y[2 * e + 1]);
                *reinterpret_cast<u32x4*>(out + (size_t)r * d + c) = pk;
            }
        }
    }
}

// pre_layrnorm for the large calls: LayerNorm in place on the f32 rows AND, in the same pass, what row_stats_kernel would
// produce from the result — the bf16 copy of the new rows (xb) and their (sum, sumsq) in statistics slot 0 of `parts`
// (the others zero). One launch and one 39 MB read less per ViT-B/32 step. d <= 1024, d % 4 == 0.
// LEAN (the bf16 residual stream: the layers read xb and the statistics, nobody reads the f32 rows again): the f32 write-back
// is skipped (39 MB per ViT-B/32 step), and row 0 of every item is class_embedding + position_embedding[0] computed HERE
// (cls_rows_kernel's sum, as prelayernorm_skinny_kernel does), so that launch goes away too. Same arithmetic, same bits.
template <bool LEAN>
__global__ __launch_bounds__(256) void layernorm_stats_kernel(float* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, uint16_t* __restrict__ xb,
                                                              float* __restrict__ stats, int M, int d, int parts, float eps,
                                                              const float* __restrict__ cls = nullptr,
                                                              const float* __restrict__ pos = nullptr, int T = 1) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    float* xr = x + (size_t)r * d;
    const bool is_cls = LEAN && (r % T) == 0;
    f32x4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < d) {
            if (is_cls) v[i] = *reinterpret_cast<const f32x4*>(cls + c) + *reinterpret_cast<const f32x4*>(pos + c);
            else v[i] = *reinterpret_cast<const f32x4*>(xr + c);
        }
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if ((i * 64 + lane) * 4 < d) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = v[i][e] - mean;
                q += t * t;
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
    float ys = 0.f, yq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < d) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(beta + c);
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * g[e] + bb[e];
            if constexpr (!LEAN) *reinterpret_cast<f32x4*>(xr + c) = y;
            u32x2 pk;
            pk[0] = pack_bf16x2(y[0], y[1]);
            pk[1] = pack_bf16x2(y[2], y[3]);
            *reinterpret_cast<u32x2*>(xb + (size_t)r * d + c) = pk;
            ys += (y[0] + y[1]) + (y[2] + y[3]);           // (same per-lane order as row_stats_kernel)
            yq += (y[0] * y[0] + y[1] * y[1]) + (y[2] * y[2] + y[3] * y[3]);
        }
    }
    ys = wave_sum(ys);
    yq = wave_sum(yq);
    float* o = stats + (size_t)r * parts * 2;
    for (int i = lane; i < parts * 2; i += 64) o[i] = (i == 0) ? ys : (i == 1 ? yq : 0.f);
}

// (mean, rstd) of every row from its partial (sum, sumsq) per 64 columns — what the folded GEMM's epilogue applies. The
// persistent kernel finalises a tile's rows itself while K <= 768; for K = 1024 (ViT-L/14) the 32 KB of raw partials of a
// 256-row tile do not fit beside its staging buffers, so this pass runs in front of it: 128 bytes in, 8 out per row, one
// thread per row (4 MB per launch at 32 896 rows: a few us against the 25 us LayerNorm kernel it replaces).
__global__ __launch_bounds__(256) void ln_finalize_kernel(const float* __restrict__ stats, float* __restrict__ out, int M,
                                                          int parts, int d, float eps) {
    // eight lanes per row, one 16-byte load each per 16 partials (consecutive lanes read consecutive bytes), then three
    // xor-shuffles inside the group of eight
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int r = gid >> 3, l8 = gid & 7;
    const int rr = r < M ? r : M - 1;
    const f32x4* st = reinterpret_cast<const f32x4*>(stats + (size_t)rr * parts * 2);
    float s1 = 0.f, s2 = 0.f;
    for (int q = l8; q < parts / 2; q += 8) {
        const f32x4 v = st[q];
        s1 += v[0] + v[2];
        s2 += v[1] + v[3];
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (r < M && l8 == 0) {
        const float kd = (float)d;
        const float mean = s1 / kd;
        const float var = fmaxf(s2 / kd - mean * mean, 0.f);
        *reinterpret_cast<float2*>(out + 2 * (size_t)r) = make_float2(mean, 1.0f / sqrtf(var + eps));
    }
}

// Row statistics for the LayerNorm-fused GEMM (gemm_bf16.h, ALN): stats[r][0] = (sum, sumsq) of row r, the other
// parts zero. Only needed once per forward (the embeddings); afterwards the residual GEMM epilogues produce them.
__global__ __launch_bounds__(256) void row_stats_kernel(const float* __restrict__ x, float* __restrict__ stats,
                                                        uint16_t* __restrict__ xb, int M, int d, int parts) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const float* xr = x + (size_t)r * d;
    float s = 0.f, q = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
        s += (v[0] + v[1]) + (v[2] + v[3]);
        q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        if (xb) {  // bf16 copy of the row: the A operand of the LayerNorm-folded GEMMs
            u32x2 pk;
            pk[0] = pack_bf16x2(v[0], v[1]);
            pk[1] = pack_bf16x2(v[2], v[3]);
            *reinterpret_cast<u32x2*>(xb + (size_t)r * d + c) = pk;
        }
    }
    s = wave_sum(s);
    q = wave_sum(q);
    float* o = stats + (size_t)r * parts * 2;
    for (int i = lane; i < parts * 2; i += 64) o[i] = (i == 0) ? s : (i == 1 ? q : 0.f);
}

// LayerNorm folding (gemm_bf16.h, epilogues 7/8): W'[n,k] = bf16(W[n,k] * gamma[k]), c[n] = sum_k W'[n,k],
// b'[n] = b[n] + sum_k beta[k] * W[n,k]. One wave per output feature n; run once when the weights are finalised.
__global__ __launch_bounds__(256) void fold_ln_weights_kernel(const uint16_t* __restrict__ Wb, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ bias,
                                                              uint16_t* __restrict__ Wf, float* __restrict__ cvec,
                                                              float* __restrict__ bf, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float c = 0.f, bs = 0.f;
    for (int kk = lane; kk < K; kk += 64) {
        const float w = bf16_bits_to_f32(Wb[(size_t)n * K + kk]);
        const bf16_t wf = (bf16_t)(w * gamma[kk]);
        const uint16_t bits = __builtin_bit_cast(uint16_t, wf);
        Wf[(size_t)n * K + kk] = bits;
        c += bf16_bits_to_f32(bits);
        bs += beta[kk] * w;
    }
    c = wave_sum(c);
    bs = wave_sum(bs);
    if (lane == 0) { cvec[n] = c; bf[n] = bias[n] + bs; }
}

// K4 (attention): attention_kernels.h with attention_common.h, attention_stream.h and attention_tiled.h
#include "attention_kernels.h"

// ------------------------------------------------------------------------------------------------
// K8 tail / a7: out[r] = y[r] / ||y[r]||_2, fp32, no epsilon (backend/app/utils.py:78,98).
// One wave per row.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ y, float* __restrict__ out, int B,
                                                          int D, int ldy) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B) return;
    const float* yr = y + (size_t)r * ldy;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += yr[c] * yr[c];
    const float nrm = sqrtf(wave_sum(s));
    for (int c = lane; c < D; c += 64) out[(size_t)r * D + c] = yr[c] / nrm;
}

// f32 -> bf16 conversion (weight upload)
__global__ void f32_to_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        bf16_t v = (bf16_t)src[i];
        dst[i] = __builtin_bit_cast(uint16_t, v);
    }
}
// bf16 -> f32 widening (debug taps)
__global__ void bf16_to_f32_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = bf16_bits_to_f32(src[i]);
}

namespace {   // (the two kernels below keep the internal linkage they had in api_encoder.hip)

// f32 [R,C] -> bf16 rows of stride ldd (dst pre-zeroed where ldd > C)
__global__ void convert_2d_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t R, int C,
                                       int ldd) {
    const int64_t total = R * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / C;
        const int c = (int)(i - r * C);
        bf16_t v = (bf16_t)src[i];
        dst[r * ldd + c] = __builtin_bit_cast(uint16_t, v);
    }
}

// The pruned last layer's two gathers in one launch: ctxc row r = ctx row rowmap[r] (bf16), xc row r = the residual row
// rowmap[r] as f32 — copied from x32, or widened from x16 when the stream is bf16. d % 4 == 0.
__global__ void gather_pooled_kernel(const uint16_t* __restrict__ ctx, uint16_t* __restrict__ ctxc, const float* __restrict__ x32,
                                     const uint16_t* __restrict__ x16, float* __restrict__ xc, const int32_t* __restrict__ rowmap,
                                     int n, int d) {
    const int chunks = d >> 2;
    const int64_t total = (int64_t)n * chunks;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / chunks), c = (int)(i - (int64_t)r * chunks);
        const size_t so = (size_t)rowmap[r] * d + (size_t)c * 4, dofs = (size_t)r * d + (size_t)c * 4;
        *reinterpret_cast<u32x2*>(ctxc + dofs) = *reinterpret_cast<const u32x2*>(ctx + so);
        f32x4 o;
        if (x16) {
            const u32x2 v = *reinterpret_cast<const u32x2*>(x16 + so);
            o[0] = __uint_as_float(v[0] << 16); o[1] = __uint_as_float(v[0] & 0xFFFF0000u);
            o[2] = __uint_as_float(v[1] << 16); o[3] = __uint_as_float(v[1] & 0xFFFF0000u);
        } else {
            o = *reinterpret_cast<const f32x4*>(x32 + so);
        }
        *reinterpret_cast<f32x4*>(xc + dofs) = o;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ launchers
// One per kernel: its preconditions, its profile record (where the encoder has always had one), the launch, the error check.
// The encoder (api_encoder.hip) and the debug ABI (api_encoder_debug.h) launch through these and nowhere else.
static int launch_layernorm(hipStream_t st, const float* x, const float* g, const float* b, void* out, bool out_bf16,
                            const int32_t* rowmap, int M, int d, float eps) {
    if (d % 4 || d > 1024 || d <= 0) MM_FAIL(MMISS_ERR_UNSUPPORTED, "layernorm: d=%d (need d%%4==0, d<=1024)", d);
    if (M <= 0) return MMISS_OK;
    MM_PROF("layernorm", st, 8.0 * M * d, (double)M * d * (4 + (out_bf16 ? 2 : 4)));
    const int grid = (M + 3) / 4;
    if (out_bf16)
        hipLaunchKernelGGL(layernorm_kernel<true>, dim3(grid), dim3(256), 0, st, x, g, b, out, rowmap, M, d, eps);
    else
        hipLaunchKernelGGL(layernorm_kernel<false>, dim3(grid), dim3(256), 0, st, x, g, b, out, rowmap, M, d, eps);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// LayerNorm of a bf16 residual stream -> bf16 GEMM operand
static int launch_layernorm16(hipStream_t st, const uint16_t* x16, const float* g, const float* b, void* out_bf16, int M, int d,
                              float eps) {
    if (d % 8 || d > 1024 || d <= 0) MM_FAIL(MMISS_ERR_UNSUPPORTED, "layernorm16: d=%d (need d%%8==0, d<=1024)", d);
    if (M <= 0) return MMISS_OK;
    MM_PROF("layernorm16", st, 8.0 * M * d, (double)M * d * 4);
    hipLaunchKernelGGL(layernorm16_kernel, dim3((M + 7) / 8), dim3(256), 0, st, x16, g, b, reinterpret_cast<uint16_t*>(out_bf16),
                       M, d, eps);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_im2col(hipStream_t st, const void* pixels, bool src_u8, void* out, int B, int S, int P, int Kp) {
    if (P <= 0 || S % P || Kp % 8 || Kp < 3 * P * P) MM_FAIL(MMISS_ERR_ARG, "im2col: S=%d P=%d Kp=%d", S, P, Kp);
    if (B <= 0) return MMISS_OK;
    const int G = S / P;
    const int64_t total = (int64_t)B * G * G * (Kp / 8);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    MM_PROF("im2col", st, 0.0, (double)B * 3 * S * S * (src_u8 ? 1 : 4) + (double)B * G * G * Kp * 2);
    if (src_u8)
        hipLaunchKernelGGL(im2col_kernel<true>, dim3(grid), dim3(256), 0, st, pixels, (uint16_t*)out, B, S, P, Kp);
    else
        hipLaunchKernelGGL(im2col_kernel<false>, dim3(grid), dim3(256), 0, st, pixels, (uint16_t*)out, B, S, P, Kp);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_cls_rows(hipStream_t st, float* x, const float* cls, const float* pos, int B, int T, int d) {
    MM_PROF("cls_rows", st, (double)B * d, 12.0 * B * d);
    hipLaunchKernelGGL(cls_rows_kernel, dim3((B * d + 255) / 256), dim3(256), 0, st, x, cls, pos, B, T, d);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_prelayernorm_skinny(hipStream_t st, float* x, const float* cls, const float* pos, const float* g, const float* b, uint16_t* xb,
                                      float* stats16, int M, int T, int d, float eps) {
    if (M <= 0 || T < 1 || d <= 0 || d % 16 || d > 1024) MM_FAIL(MMISS_ERR_UNSUPPORTED, "prelayernorm_skinny: M=%d T=%d d=%d (d%%16==0, d<=1024)", M, T, d);
    MM_PROF("layernorm", st, 12.0 * M * d, (double)M * d * 10);
    hipLaunchKernelGGL(prelayernorm_skinny_kernel, dim3((M + 3) / 4), dim3(256), 0, st, x, cls, pos, g, b, xb, stats16, M, T, d, eps);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// lean: x is only read and the CLS rows are made here from cls + pos, one per T rows; otherwise cls, pos and T are not used
static int launch_layernorm_stats(hipStream_t st, float* x, const float* g, const float* b, uint16_t* xb, float* stats, int M, int d, int parts,
                                  float eps, bool lean, const float* cls, const float* pos, int T) {
    if (M <= 0 || d <= 0 || d % 4 || d > 1024 || parts < 1 || (lean && T < 1))
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "prelayernorm_stats: M=%d d=%d (d%%4==0, d<=1024) parts=%d T=%d", M, d, parts, T);
    MM_PROF("layernorm", st, 10.0 * M * d, (double)M * d * (lean ? 6 : 10));
    const dim3 grid((M + 3) / 4), block(256);
    if (lean) hipLaunchKernelGGL(layernorm_stats_kernel<true>, grid, block, 0, st, x, g, b, xb, stats, M, d, parts, eps, cls, pos, T);
    else hipLaunchKernelGGL(layernorm_stats_kernel<false>, grid, block, 0, st, x, g, b, xb, stats, M, d, parts, eps, (const float*)nullptr, (const float*)nullptr, 1);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_ln_finalize(hipStream_t st, const float* stats, float* out, int M, int parts, int d, float eps) {
    // (the kernel reads the partials of a row as 16-byte pairs of (sum, sumsq): an even count, rows 16-byte aligned)
    if (M <= 0 || d <= 0 || parts < 2 || parts % 2 || (reinterpret_cast<uintptr_t>(stats) & 15))
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "ln_finalize: M=%d d=%d parts=%d (even, >= 2; stats 16-byte aligned)", M, d, parts);
    MM_PROF("ln_finalize", st, 4.0 * M * parts, (double)M * (parts * 8 + 8));
    hipLaunchKernelGGL(ln_finalize_kernel, dim3((M * 8 + 255) / 256), dim3(256), 0, st, stats, out, M, parts, d, eps);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// stats_read = false: the separate-LayerNorm mode on a bf16 stream, where only the bf16 copy is used (the byte model leaves the statistics out)
static int launch_row_stats(hipStream_t st, const float* x, float* stats, uint16_t* xb_or_null, int M, int d, int parts, bool stats_read) {
    if (M <= 0 || d <= 0 || d % 4 || parts < 1) MM_FAIL(MMISS_ERR_UNSUPPORTED, "row_stats: M=%d d=%d (d%%4==0) parts=%d", M, d, parts);
    MM_PROF("row_stats", st, 3.0 * M * d, (stats_read ? 6.0 : 4.0) * M * d);
    hipLaunchKernelGGL(row_stats_kernel, dim3((M + 3) / 4), dim3(256), 0, st, x, stats, xb_or_null, M, d, parts);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_fold_ln_weights(hipStream_t st, const uint16_t* w, const float* gamma, const float* beta, const float* bias, uint16_t* wf,
                                  float* c, float* bf, int N, int K) {
    if (N <= 0 || K <= 0) MM_FAIL(MMISS_ERR_UNSUPPORTED, "fold_ln_weights: N=%d K=%d", N, K);
    hipLaunchKernelGGL(fold_ln_weights_kernel, dim3((N + 3) / 4), dim3(256), 0, st, w, gamma, beta, bias, wf, c, bf, N, K);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_text_embed(hipStream_t st, const int32_t* ids, const float* tok, const float* pos, float* x, int32_t* pool_row, int B, int T,
                             int d, int vocab, int eos_id) {
    if (B <= 0 || T < 1 || d <= 0 || d % 4 || vocab < 1) MM_FAIL(MMISS_ERR_UNSUPPORTED, "text_embed: B=%d T=%d d=%d (d%%4==0) vocab=%d", B, T, d, vocab);
    hipLaunchKernelGGL(text_embed_kernel, dim3(B), dim3(256), 0, st, ids, tok, pos, x, pool_row, T, d, vocab, eos_id);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_vision_pool_rows(hipStream_t st, int32_t* pool_row, int B, int T) {
    hipLaunchKernelGGL(vision_pool_rows_kernel, dim3((B + 255) / 256), dim3(256), 0, st, pool_row, B, T);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// pooled rows of the attention output (bf16) and of the residual stream (x32, or x16 widened: exactly one of the two) in ONE launch
static int launch_gather_pooled(hipStream_t st, const uint16_t* ctx, uint16_t* ctxc, const float* x32, const uint16_t* x16, float* xc,
                                const int32_t* rowmap, int n, int d) {
    if (n <= 0 || d <= 0 || d % 4 || !x32 == !x16) MM_FAIL(MMISS_ERR_UNSUPPORTED, "gather_pooled: n=%d d=%d (d%%4==0; one of x32 / x16)", n, d);
    MM_PROF("gather_pooled", st, 0.0, (double)n * d * (x16 ? 10 : 12));
    hipLaunchKernelGGL(gather_pooled_kernel, dim3((n * d / 4 + 255) / 256), dim3(256), 0, st, ctx, ctxc, x32, x16, xc, rowmap, n, d);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_l2norm_rows(hipStream_t st, const float* y, float* out, int B, int D, int ldy) {
    MM_PROF("l2norm_rows", st, 3.0 * B * D, 8.0 * B * D);
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, st, y, out, B, D, ldy);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_convert_2d_bf16(hipStream_t st, const float* src, uint16_t* dst, int64_t R, int C, int ldd) {
    if (R <= 0 || C <= 0 || ldd < C) MM_FAIL(MMISS_ERR_ARG, "convert_2d_bf16: R=%lld C=%d ldd=%d", (long long)R, C, ldd);
    const int64_t blocks = (R * C + 255) / 256;
    hipLaunchKernelGGL(convert_2d_bf16_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, src, dst, R, C, ldd);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_bf16_to_f32(hipStream_t st, const uint16_t* src, float* dst, int64_t n) {
    if (n <= 0) return MMISS_OK;
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(256), dim3(256), 0, st, src, dst, n);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

// calibrate_kernels.h — activation centring for the fp8 vision tower (mmiss_encoder_calibrate; DESIGN.md 3b "Outlier channels").
//
//   LN(x) W^T + b  =  (LN(x) - mu) W^T + (b + W mu)
//
// mu is the constant part of a LayerNorm output, measured once per site on a calibration batch. LN(x) - mu is the same
// LayerNorm with beta' = beta - mu, so the LayerNorm -> MXFP8 kernels and the fp8 GEMMs run unchanged on other pointers; the
// channel that sat at ~24 for every token row no longer multiplies the e4m3 rounding error of the weight column it meets.
// Three kernels, all one-shot (calibration time, never the encode path), all deterministic (no float atomics, fixed orders):
//   ln_colstats_kernel      per-column sum / sum of squares of the LayerNorm OUTPUT over a row block, all in f64, one partial per workgroup
//   colstats_finish_kernel  partials in workgroup order -> mean, variance, the centring rule, mu, beta'
//   bias_fold_kernel        b' = b + W_bf16 mu, one wave per output row
#pragma once
#include "common.h"

#define CAL_MAX_D 1024        // a lane owns 16 columns, as in layernorm_kernel
#define CAL_MAX_PARTIALS 1024 // row blocks per site (the row block grows from 32 rows until they fit)

// Rows [blockIdx.x * rows_per_wg, ...) of x (f32 [M,d], or bf16 when X_BF16): the LayerNorm of each row with layernorm_kernel's
// lane layout, two-pass statistics and eps, but evaluated in f64 — the row (mean, rstd), y = (x - mean) * rstd * gamma + beta
// and, per column, the sums of y and y^2. (fp32 row statistics were measured first: a row mean carries an absolute error
// relative to the row's LARGEST entries, 300 here, which for a single calibration row exceeds 2^-20 of a small column's own
// magnitude; in f64 the statistics are those of the exact LayerNorm and the f32 LayerNorm kernels differ from them by their
// own rounding only, ~1e-7 relative: nothing next to an e4m3 step.) A lane owns columns (i * 64 + lane) * 4 .. + 3, i < 4, so
// the column sums need no cross-lane traffic; a wave takes every fourth row of the block; the four waves' sums are added in
// wave order through LDS. partial: f64 [gridDim.x][2][d]. d % 4 == 0, d <= 1024. Any M >= 1 (a wave without rows adds zeros).
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <bool X_BF16>
__global__ __launch_bounds__(256) void ln_colstats_kernel(const void* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, double* __restrict__ partial, int M,
                                                          int d, float eps, int rows_per_wg) {
    __shared__ double red[2][CAL_MAX_D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = blockIdx.x * rows_per_wg;
    const int row1 = (row0 + rows_per_wg < M) ? row0 + rows_per_wg : M;
    f32x4 g[4], bb[4];
    double s1[4][4], s2[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (i * 64 + lane) * 4;
        g[i] = (c < d) ? *reinterpret_cast<const f32x4*>(gamma + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        bb[i] = (c < d) ? *reinterpret_cast<const f32x4*>(beta + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) s1[i][e] = s2[i][e] = 0.0;
    }
    for (int r = row0 + wave; r < row1; r += 4) {   // (wave-uniform)
        f32x4 v[4];
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = (i * 64 + lane) * 4;
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < d) {
                if constexpr (X_BF16) {
                    const u32x2 w = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(x) + (size_t)r * d + c);
                    v[i][0] = __uint_as_float(w[0] << 16); v[i][1] = __uint_as_float(w[0] & 0xFFFF0000u);
                    v[i][2] = __uint_as_float(w[1] << 16); v[i][3] = __uint_as_float(w[1] & 0xFFFF0000u);
                } else {
                    v[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(x) + (size_t)r * d + c);
                }
            }
            s += ((double)v[i][0] + (double)v[i][1]) + ((double)v[i][2] + (double)v[i][3]);
        }
        const double mean = wave_sum_f64(s) / (double)d;
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if ((i * 64 + lane) * 4 < d) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double t = (double)v[i][e] - mean;
                    q += t * t;
                }
            }
        }
        const double rstd = 1.0 / sqrt(wave_sum_f64(q) / (double)d + (double)eps);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double y = ((double)v[i][e] - mean) * rstd * (double)g[i][e] + (double)bb[i][e];
                s1[i][e] += y;
                s2[i][e] += y * y;
            }
        }
    }
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = (i * 64 + lane) * 4;
                if (c < d) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        red[0][c + e] = (w == 0 ? 0.0 : red[0][c + e]) + s1[i][e];
                        red[1][c + e] = (w == 0 ? 0.0 : red[1][c + e]) + s2[i][e];
                    }
                }
            }
        }
        __syncthreads();
    }
    double* out = partial + (size_t)blockIdx.x * 2 * d;
    for (int c = threadIdx.x; c < d; c += 256) {
        out[c] = red[0][c];
        out[d + c] = red[1][c];
    }
}

// One site: the partials summed in workgroup order, mean = S1 / M, population variance = S2 / M - mean^2 (f64), and the rule
// mu_c = mean_c where mean_c^2 >= var_c, else 0 — a channel is centred only where its constant part is at least as large as its
// varying part over the calibration rows (centring a channel that is large on ONE token row would shift the other rows by
// mean / T each). mu, beta_out = beta - mu: f32 [d]; *centred = channels with mu != 0 chosen by the rule; mean_out / var_out
// (f64 [d], optional) are for the tests. One workgroup.
__global__ __launch_bounds__(256) void colstats_finish_kernel(const double* __restrict__ partial, int nparts, int M, int d,
                                                              const float* __restrict__ beta, float* __restrict__ mu,
                                                              float* __restrict__ beta_out, int32_t* __restrict__ centred,
                                                              double* __restrict__ mean_out, double* __restrict__ var_out) {
    __shared__ int count;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    int mine = 0;
    for (int c = threadIdx.x; c < d; c += 256) {
        double a = 0.0, b = 0.0;
        for (int p = 0; p < nparts; ++p) {
            a += partial[(size_t)p * 2 * d + c];
            b += partial[(size_t)p * 2 * d + d + c];
        }
        const double mean = a / (double)M;
        double var = b / (double)M - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const bool centre = mean * mean >= var;
        const float m = centre ? (float)mean : 0.f;
        mine += centre ? 1 : 0;
        mu[c] = m;
        if (beta_out) beta_out[c] = beta[c] - m;
        if (mean_out) mean_out[c] = mean;
        if (var_out) var_out[c] = var;
    }
    atomicAdd(&count, mine);   // (an integer in LDS: any order gives the same count)
    __syncthreads();
    if (threadIdx.x == 0) *centred = count;
}

// A stored table coming back (mmiss_encoder_calibration_set): beta_out = beta - mu with the same f32 subtraction as above,
// *centred = channels with mu != 0. One workgroup.
__global__ __launch_bounds__(256) void beta_centre_kernel(const float* __restrict__ beta, const float* __restrict__ mu,
                                                          float* __restrict__ beta_out, int32_t* __restrict__ centred, int d) {
    __shared__ int count;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    int mine = 0;
    for (int c = threadIdx.x; c < d; c += 256) {
        const float m = mu[c];
        beta_out[c] = beta[c] - m;
        mine += m != 0.f ? 1 : 0;
    }
    atomicAdd(&count, mine);
    __syncthreads();
    if (threadIdx.x == 0) *centred = count;
}

// out[n] = bias[n] + sum_k W[n,k] mu[k]: W bf16 [N,K] (the UNQUANTISED weights: the point is that this part never passes
// through e4m3), f32 accumulation in the canonical order of the re-rank kernel — lane l sums k = l, l + 64, ..., then the
// fixed xor butterfly. One wave per output row, four rows per workgroup. mu = 0 returns bias.
__global__ __launch_bounds__(256) void bias_fold_kernel(const uint16_t* __restrict__ W, const float* __restrict__ bias,
                                                        const float* __restrict__ mu, float* __restrict__ out, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const uint16_t* w = W + (size_t)n * K;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc += bf16_bits_to_f32(w[k]) * mu[k];
    acc = wave_sum(acc);
    if (lane == 0) out[n] = bias[n] + acc;
}

static int cal_rows_per_wg(int M) {
    int rb = 32;
    while ((M + rb - 1) / rb > CAL_MAX_PARTIALS) rb *= 2;
    return rb;
}
static size_t cal_partial_bytes(int M, int d) {
    const int rb = cal_rows_per_wg(M);
    return (size_t)((M + rb - 1) / rb) * 2 * d * sizeof(double);
}

// one site's statistics: x -> partial (cal_partial_bytes(M, d)) -> mu, beta_out, centred (and mean / var for the tests)
static int launch_ln_colstats(hipStream_t st, const void* x, bool x_bf16, const float* gamma, const float* beta, double* partial,
                              int M, int d, float eps, float* mu, float* beta_out, int32_t* centred, double* mean_out,
                              double* var_out) {
    if (M < 1 || d < 4 || d > CAL_MAX_D || (d % 4)) MM_FAIL(MMISS_ERR_UNSUPPORTED, "ln_colstats: M=%d d=%d (need M >= 1, d <= 1024, d %% 4 == 0)", M, d);
    const int rb = cal_rows_per_wg(M), nparts = (M + rb - 1) / rb;
    {
        MM_PROF("ln_colstats", st, 12.0 * M * d, (double)M * d * (x_bf16 ? 2 : 4));
        if (x_bf16)
            hipLaunchKernelGGL(ln_colstats_kernel<true>, dim3(nparts), dim3(256), 0, st, x, gamma, beta, partial, M, d, eps, rb);
        else
            hipLaunchKernelGGL(ln_colstats_kernel<false>, dim3(nparts), dim3(256), 0, st, x, gamma, beta, partial, M, d, eps, rb);
        MM_HIP(hipGetLastError());
    }
    MM_PROF("colstats_finish", st, 2.0 * nparts * d, 16.0 * nparts * d);
    hipLaunchKernelGGL(colstats_finish_kernel, dim3(1), dim3(256), 0, st, partial, nparts, M, d, beta, mu, beta_out, centred, mean_out,
                       var_out);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_bias_fold(hipStream_t st, const void* w_bf16, const float* bias, const float* mu, float* out, int N, int K) {
    if (N < 1 || K < 1) MM_FAIL(MMISS_ERR_ARG, "bias_fold: N=%d K=%d", N, K);
    MM_PROF("bias_fold", st, 2.0 * N * K, 2.0 * N * K);
    hipLaunchKernelGGL(bias_fold_kernel, dim3((N + 3) / 4), dim3(256), 0, st, reinterpret_cast<const uint16_t*>(w_bf16), bias, mu, out,
                       N, K);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

static int launch_beta_centre(hipStream_t st, const float* beta, const float* mu, float* beta_out, int32_t* centred, int d) {
    hipLaunchKernelGGL(beta_centre_kernel, dim3(1), dim3(256), 0, st, beta, mu, beta_out, centred, d);
    MM_HIP(hipGetLastError());
    return MMISS_OK;
}

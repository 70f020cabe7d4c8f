/*
 * mmiss_debug.h — kernel-level entry points of libmmiss.so used ONLY by tests/ and bench.py to check
 * and time single kernels in isolation. Not part of the drop-in boundary. Same pointer conventions
 * as mmiss.h, except that every pointer here must be a DEVICE pointer of `device` (the tests allocate
 * them with torch) and calls run on `hip_stream` (NULL = default stream) without synchronising.
 */
#ifndef MMISS_DEBUG_H
#define MMISS_DEBUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* epilogues of the bf16 MFMA GEMM  C[M,N] = A[M,K] * W[N,K]^T  (A, W bf16 row-major) */
enum {
    MMISS_EPI_F32 = 0,             /* out f32 [M,N] = acc                                           */
    MMISS_EPI_BIAS_BF16 = 1,       /* out bf16 [M,N] = acc + bias[n]            (K3 QKV)            */
    MMISS_EPI_BIAS_QGELU_BF16 = 2, /* out bf16 [M,N] = quick_gelu(acc + bias)   (K6 FC1)            */
    MMISS_EPI_BIAS_RESID_F32 = 3,  /* out f32 [M,N] += acc + bias[n]            (K5 out-proj, K7 FC2)*/
    MMISS_EPI_PATCH_F32 = 4        /* out f32 row (m/G)*T + 1 + m%G = acc + pos[1 + m%G][n] (K1)    */
};

/* M % 128 == 0, N % 128 == 0, K % 64 == 0. bias f32 [N] (or NULL), aux f32 (pos table for PATCH),
 * p0 = patches per image G, p1 = tokens per image T (PATCH only). variant selects the tile kernel
 * (0 = default). */
int mmiss_dbg_gemm(int device, void* hip_stream, int epi, int variant, const void* A, const void* W,
                   void* out, const float* bias, const float* aux, int32_t M, int32_t N, int32_t K,
                   int32_t p0, int32_t p1);

/* mmiss_dbg_gemm with what the encoder's calls add. m_valid (1 .. M): rows >= m_valid are computed but not stored (under PATCH
 * no output row is written for them). Epilogue 3 only: stats_out (optional) f32 [M][N/64][2] = (sum, sumsq) of the new f32 rows
 * per 64 columns, xb_out (optional) bf16 [M,N] = their bf16 copy; either one keeps the call off the split-K path. Epilogues 7 / 8
 * (LayerNorm folded into W; 8: + QuickGELU): out bf16 [M,N] = rstd_m (A W^T - mean_m c) + b', aux = c f32 [N], bias = b' f32 [N],
 * (mean, rstd) of row m from ln_stats f32 [M][K/64][2] = partial (sum, sumsq) per 64 columns (16-byte aligned) and ln_eps;
 * variant 0 / 128 / 160 / 192: the 128-column tile of that height, always on two staging buffers and 4 waves; 256: the
 * 256 x 256 tile. Refuses what the launchers refuse; no other kernel stands in. */
int mmiss_dbg_gemm_ex(int device, void* hip_stream, int epi, int variant, const void* A, const void* W, void* out,
                      const float* bias, const float* aux, int32_t M, int32_t N, int32_t K, int32_t p0, int32_t p1,
                      int32_t m_valid, float* stats_out, void* xb_out, const float* ln_stats, float ln_eps);
/* which form of the 128-column tile kernel a launch of epilogues 0 .. 4 at tile height bm (0 = 128) over M x N x K in `splits`
 * K slices (1 = no split-K) runs under the current options: 10 * staging buffers (2 | 3) + waves per workgroup (4 | 8), or 0
 * where the shape is no such launch. The launcher's own choice, evaluated on the host: the return value is the answer, not
 * a status; launches nothing, needs no device. */
int mmiss_dbg_gemm_form(int32_t bm, int32_t M, int32_t N, int32_t K, int32_t splits);

/* LayerNorm over the last dim: x f32 [M,d] -> out (bf16 if out_bf16 else f32) [M,d]; may be in place for f32 */
int mmiss_dbg_layernorm(int device, void* hip_stream, const float* x, const float* gamma, const float* beta,
                        void* out, int32_t out_bf16, int32_t M, int32_t d, float eps);

/* The LayerNorm chain around the LayerNorm-folded GEMMs, one kernel per call: each entry calls the launcher the encoder itself
 * calls (the launch_* function beside the kernel), which also makes the checks. Shapes a kernel does not take, M < 1 among them,
 * are refused with MMISS_ERR_UNSUPPORTED.
 * layernorm16: the LayerNorm of a bf16 residual stream, x_bf16 [M,d] -> out_bf16 [M,d]; d % 8 == 0, d <= 1024. */
int mmiss_dbg_layernorm16(int device, void* hip_stream, const void* x_bf16, const float* gamma, const float* beta, void* out_bf16,
                          int32_t M, int32_t d, float eps);
/* mmiss_dbg_layernorm with gathered input rows: out row r = LayerNorm(x row rowmap[r]) (rowmap int32 [M]: the pooling of the head) */
int mmiss_dbg_layernorm_gather(int device, void* hip_stream, const float* x, const float* gamma, const float* beta, void* out,
                               int32_t out_bf16, const int32_t* rowmap, int32_t M, int32_t d, float eps);
/* pre-LayerNorm of the large calls: x f32 [M,d] normalised IN PLACE, xb bf16 [M,d] = its bf16 copy, stats f32 [M][parts][2] = (sum,
 * sumsq) of the new row in slot 0, zeros in the others. lean != 0: x is only read, and row t = 0 of every T rows is taken as
 * cls + pos[0] (cls, pos f32 [d]) instead of x. d % 4 == 0, d <= 1024, parts >= 1. */
int mmiss_dbg_prelayernorm_stats(int device, void* hip_stream, float* x, const float* gamma, const float* beta, void* xb, float* stats,
                                 int32_t M, int32_t d, int32_t parts, float eps, int32_t lean, const float* cls, const float* pos,
                                 int32_t T);
/* pre-LayerNorm of one request: rows t = 0 of every T rows = cls + pos[0], LayerNorm in place on x f32 [M,d], xb bf16 [M,d],
 * stats16 f32 [M][d/16][2] = (sum, sumsq) per 16 columns of the new rows. d % 16 == 0, d <= 1024. */
int mmiss_dbg_prelayernorm_skinny(int device, void* hip_stream, float* x, const float* cls, const float* pos, const float* gamma,
                                  const float* beta, void* xb, float* stats16, int32_t M, int32_t T, int32_t d, float eps);
/* stats f32 [M][parts][2]: slot 0 = (sum, sumsq) of row r of x f32 [M,d], the others zero; xb_or_null: the rows' bf16 copy. d % 4 == 0 */
int mmiss_dbg_row_stats(int device, void* hip_stream, const float* x, float* stats, void* xb_or_null, int32_t M, int32_t d,
                        int32_t parts);
/* The folded chain of one request (M <= 128 rows, <= 320 when N <= 1024; N % 16 == 0, K % 128 == 0), where LayerNorm1 / 2 run inside
 * the skinny GEMM (csrc/gemm_skinny.h). Each entry is the encoder's own launch; where the skinny kernel would not run, it returns
 * MMISS_ERR_UNSUPPORTED, launches nothing and never falls back to a tiled kernel.
 * row_stats16: stats16 f32 [M][d/16][2] = (sum, sumsq) per 16 columns of x f32 [M,d], xb bf16 [M,d] = the rows' bf16 copy. d % 16 == 0 */
int mmiss_dbg_row_stats16(int device, void* hip_stream, const float* x, float* stats16, void* xb, int32_t M, int32_t d);
/* epi 7 / 8 (LayerNorm folded into W; 8: + QuickGELU): out bf16 [M,N] = rstd_m (A Wf^T - mean_m c) + bf, (mean, rstd) of row m from
 * stats16 f32 [M][K/16][2] (16-byte aligned); A bf16 [M,K], Wf bf16 [N,K], c, bf f32 [N] as mmiss_dbg_fold_ln_weights writes them */
int mmiss_dbg_gemm_skinny_fold(int device, void* hip_stream, int epi, const void* A, const void* Wf, void* out, const float* bf,
                               const float* c, const float* stats16, float eps, int32_t M, int32_t N, int32_t K);
/* x f32 [M,N] += A W^T + bias IN PLACE; stats16_out (optional) f32 [M][N/16][2] = (sum, sumsq) of the new rows per 16 columns,
 * xb_out (optional) bf16 [M,N] = their bf16 copy: what the next folded skinny GEMM reads */
int mmiss_dbg_gemm_skinny_resid(int device, void* hip_stream, const void* A, const void* W, float* x, const float* bias,
                                float* stats16_out, void* xb_out, int32_t M, int32_t N, int32_t K);
/* out f32 [M][2] = (mean, rstd) of every row from its `parts` partial (sum, sumsq) (stats f32 [M][parts][2], 16-byte aligned) of
 * d columns in all: var = max(sumsq / d - mean^2, 0), rstd = 1 / sqrt(var + eps). parts even, >= 2. */
int mmiss_dbg_ln_finalize(int device, void* hip_stream, const float* stats, float* out, int32_t M, int32_t parts, int32_t d, float eps);
/* LayerNorm folding: wf bf16 [N,K] = bf16(f32(w) gamma[k]), c f32 [N] = sum_k wf[n,k], bf f32 [N] = bias[n] + sum_k beta[k] w[n,k] */
int mmiss_dbg_fold_ln_weights(int device, void* hip_stream, const void* w_bf16, const float* gamma, const float* beta,
                              const float* bias, void* wf, float* c, float* bf, int32_t N, int32_t K);

/* qkv bf16 [B*T, 3*H*64] -> ctx bf16 [B*T, H*64]; softmax(QK^T/8 (+causal)) V per (b, head); 1 <= T <= MMISS_MAX_TOKENS (1025) */
int mmiss_dbg_attention(int device, void* hip_stream, const void* qkv, void* ctx, int32_t B, int32_t T,
                        int32_t H, int32_t causal);
/* the key-chunked kernel (csrc/attention_tiled.h), which mmiss_dbg_attention / mmiss_dbg_attention_mx run above 288 tokens, at
 * any 1 <= T <= MMISS_MAX_TOKENS. ctx8 == NULL: bf16 rows into ctx [B*T, H*64]. Otherwise MXFP8 into ctx8 / ctx_scale as
 * mmiss_dbg_attention_mx writes them (ctx unused; causal must be 0). At T <= 288 the bits are the long-sequence kernel's. */
int mmiss_dbg_attention_tiled(int device, void* hip_stream, const void* qkv, void* ctx, void* ctx8, void* ctx_scale, int32_t B,
                              int32_t T, int32_t H, int32_t causal);

/* the pooled-query form of the short-sequence attention (the pruned last layer): ctxc bf16 [B, H*64] row b = the attention
 * output of query row pool_row[b] - b*T of item b (pool_row int32 [B]: global token rows). Only where mmiss_dbg_attention runs the
 * several-heads kernel (T <= 128; B * H large enough, or option att_hpb forced): MMISS_ERR_UNSUPPORTED elsewhere. */
int mmiss_dbg_attention_pooled(int device, void* hip_stream, const void* qkv, const int32_t* pool_row, void* ctxc, int32_t B,
                               int32_t T, int32_t H, int32_t causal);

/* the pooled rows' out-projection: out f32 [M,N] = f32(rows_bf16[rowmap[m]]) + A W^T + bias (rows_bf16 bf16 [*, N], rowmap
 * int32 [M]); `out` is only written. M <= 320, N % 16 == 0, K % 128 == 0 (the skinny kernel). */
int mmiss_dbg_gemm_resid_rows(int device, void* hip_stream, const void* A, const void* W, float* out, const float* bias,
                              const void* rows_bf16, const int32_t* rowmap, int32_t M, int32_t N, int32_t K);

/* the patch-embedding GEMM reading the f32 pixels itself (csrc/gemm_bf16_p160.h): pixels f32 [B,3,S,S], W bf16 [d, 3*P*P],
 * pos f32 [G*G+1, d] -> out f32 [B*(G*G+1), d] rows b*(G*G+1) + 1 + patch = patch . W^T + pos[1 + patch]; the CLS rows (token 0)
 * are not written. P = 16 or 32, d % 256 == 0. The same bits as mmiss_dbg_im2col + mmiss_dbg_gemm(MMISS_EPI_PATCH_F32). */
int mmiss_dbg_patch_from_pixels(int device, void* hip_stream, const float* pixels, const void* W, float* out, const float* pos,
                                int32_t B, int32_t S, int32_t P, int32_t d);

/* pixels f32 [B,3,S,S] -> patches bf16 [B*G*G, Kp] (k = c*P*P + ky*P + kx, zero padded to Kp) */
int mmiss_dbg_im2col(int device, void* hip_stream, const float* pixels, void* out, int32_t B, int32_t S,
                     int32_t P, int32_t Kp);

/* HIP-event time of `iters` back-to-back launches of one GEMM (ms per launch) */
int mmiss_dbg_gemm_time(int device, int epi, int variant, const void* A, const void* W, void* out,
                        const float* bias, const float* aux, int32_t M, int32_t N, int32_t K,
                        int32_t p0, int32_t p1, int32_t iters, float* ms_per_launch);

/* the persistent 256 x 256 tile GEMM (csrc/gemm_bf16_p256.h) in isolation: epi 1 / 2 = bias / bias + QuickGELU -> bf16,
 * 7 / 8 = the same behind a LayerNorm folded into W (ln_stats f32 [M][K/64][2] partial (sum, sumsq) per 64 columns,
 * aux = c [N], bias = b' [N]). M % 256 == 0 (rows >= m_valid land in row M - 1), N % 256 == 0, K % 256 == 0.
 * iters > 0 and ms_per_launch != NULL: HIP-event time of `iters` back-to-back launches. */
int mmiss_dbg_gemm_p256(int device, void* hip_stream, int epi, const void* A, const void* W, void* out,
                        const float* bias, const float* aux, const float* ln_stats, float ln_eps, int32_t M, int32_t N,
                        int32_t K, int32_t m_valid, int32_t iters, float* ms_per_launch);

/* the residual GEMM on a bf16 residual stream in isolation: out (bf16 [M,N], IN PLACE) = bf16(f32(out) + A W^T + bias),
 * stats_out (optional) f32 [M][N/64][2] = (sum, sumsq) of the new rows per 64 columns. variant 0 = the 160 x 256 tile on the
 * staggered loop (csrc/gemm_bf16_p160.h: M % 160 == 0, N % 256 == 0, K % 128 == 0), 128 / 160 / 192 = the 128-column kernel of
 * that tile height (M a multiple of it). Rows >= m_valid: untouched, except row M - 1 under variant 0. iters > 0 and
 * ms_per_launch != NULL: HIP-event time of `iters` back-to-back launches (the stream keeps accumulating). */
int mmiss_dbg_gemm_resid16(int device, void* hip_stream, int variant, const void* A, const void* W, void* out,
                           const float* bias, float* stats_out, int32_t M, int32_t N, int32_t K, int32_t m_valid,
                           int32_t iters, float* ms_per_launch);

/* record the residual stream after every layer during encode calls (for mmiss_encoder_tap 0..L) */
struct mmiss_encoder;
int mmiss_dbg_encoder_record_taps(struct mmiss_encoder* enc, int on);
/* how LayerNorm1/2 reach the QKV / FC1 GEMMs: -1 (default) automatic by rows per call, 0 separate LayerNorm kernels,
 * 1 normalised during operand staging, 2 folded algebraically into weights + epilogue (A/B and parity tests) */
int mmiss_dbg_encoder_set_fuse_ln(struct mmiss_encoder* enc, int on);

/* experiment: full GEMM vs two half-M GEMMs (same stream / two streams); ms[3] per GEMM-equivalent */
int mmiss_dbg_gemm_split_time(int device, int epi, int bm, const void* A, const void* W, void* out, const float* bias,
                              int32_t M, int32_t N, int32_t K, int32_t iters, float* ms);

/* fp8 path in isolation (gemm_fp8.h). Scale arrays use the permuted E8M0 layout: 16 * ceil(K / 512) bytes per row, the
 * scale of k-block b = k / 32 at byte (b / 16) * 16 + (b % 4) * 4 + (b / 4) % 4. */
int mmiss_dbg_quantize_weights_fp8(int device, void* hip_stream, const void* w_bf16, void* w8, float* scale, int32_t N,
                                   int32_t K);
int mmiss_dbg_layernorm_mxfp8(int device, void* hip_stream, const float* x, const float* gamma, const float* beta,
                              void* out8, void* out_scale, int32_t M, int32_t d, float eps);
/* the same from bf16 rows (the bf16 residual stream of the large calls) */
int mmiss_dbg_layernorm16_mxfp8(int device, void* hip_stream, const void* x_bf16, const float* gamma, const float* beta,
                                void* out8, void* out_scale, int32_t M, int32_t d, float eps);
/* attention whose output leaves the kernel as MXFP8 (the fp8 out-projection's A operand): qkv bf16 [B*T, 3*H*64] -> ctx8 e4m3
 * [B*T, H*64] + ctx_scale (permuted E8M0, 16 * ceil(H*64 / 512) bytes per row); non-causal, 1 <= T <= MMISS_MAX_TOKENS
 * (1025; round 6: the one-pass kernels for T <= 128 too; above 288: the key-chunked kernel) */
int mmiss_dbg_attention_mx(int device, void* hip_stream, const void* qkv, void* ctx8, void* ctx_scale, int32_t B, int32_t T,
                           int32_t H);
/* epi: 0 out bf16 = acc * wscale[n] + bias[n]; 1 out e4m3 + out_scale = mx(quick_gelu(.)); 2 out f32 += . ; bm = 128 | 160 | 192 */
int mmiss_dbg_gemm8(int device, void* hip_stream, int epi, int bm, const void* A8, const void* As, const void* W8,
                    const float* wscale, const float* bias, void* out, void* out_scale, int32_t M, int32_t N, int32_t K);
int mmiss_dbg_gemm8_time(int device, int epi, int bm, const void* A8, const void* As, const void* W8, const float* wscale,
                         const float* bias, void* out, void* out_scale, int32_t M, int32_t N, int32_t K, int32_t iters,
                         float* ms_per_launch);

/* process-wide integer tuning knob (A/B experiments from tools/): e.g. "scan_group" = 8 | 16 */
int mmiss_dbg_set_option(const char* key, int value);

/* the calibration kernels in isolation (csrc/calibrate_kernels.h). ln_colstats: x f32 [M,d] (bf16 when x_is_bf16) -> column statistics
 * of LayerNorm(x; gamma, beta) over the M rows: mean_out, var_out f64 [d] (population variance), mu_out f32 [d] (the mean where
 * mean^2 >= var, else 0), centred_out int32 [1]; M >= 1, d <= 1024, d % 4 == 0; synchronises the stream (it frees its scratch).
 * bias_fold: out f32 [N] = bias + W mu, W bf16 [N,K], mu f32 [K], f32 accumulation in a fixed order. */
int mmiss_dbg_ln_colstats(int device, void* hip_stream, const void* x, int32_t x_is_bf16, const float* gamma, const float* beta,
                          int32_t M, int32_t d, float eps, double* mean_out, double* var_out, float* mu_out, int32_t* centred_out);
int mmiss_dbg_bias_fold(int device, void* hip_stream, const void* w_bf16, const float* bias, const float* mu, int32_t N, int32_t K,
                        float* out);

/* the resize step's tables in isolation (csrc/preprocess_kernels.h): the host geometry of one H x W image at crop size S, and one
 * resize_coeffs_kernel launch through the encoder's own launcher, with the pool layout of the encoder's own call. geometry: HOST int32 [6] = new_h,
 * new_w, top, left, ksx, ksy. pool int32 [(ksx + ksy) * S] = kx [ksx][S] then ky [S][ksy] (fixed point, 22 bits), bounds int32
 * [4][S] = xmin, xcnt, ymin, ycnt of the crop window's S columns / rows. pool == bounds == NULL: only the geometry, nothing is
 * launched and no device is needed. Refused like an encoder call: edges outside 1..65536, more than 4096 taps (and S outside
 * 1..16384). Synchronises the stream. */
int mmiss_dbg_resize_coeffs(int device, void* hip_stream, int32_t H, int32_t W, int32_t S, int32_t* geometry, int32_t* pool,
                            int32_t* bounds);
/* which resize_crop_kernel<KMAX> a launch over a blob of blob_bytes whose images need at most max_ksx horizontal taps runs:
 * 12 or 24 (taps in registers), 0 (generic). The return value is the answer, not a status. */
int mmiss_dbg_resize_crop_variant(int64_t blob_bytes, int32_t max_ksx);

/* The plan a query call of Q queries and this k (filtered != 0: a filtered one) would follow on the index as it stands, and the
 * plan of the widen pass if `flagged` (0 .. Q) of its queries were flagged: the query path's own planning functions (plan_query,
 * and from csrc/index_plans.h plan_scan, plan_dense, strip_length, select_splits, merge_two_level), evaluated on the host.
 * Launches nothing, changes nothing, needs no device. out is a HOST int32 [24]; fields that do not apply are 0:
 *   [0] dense   [1] dense8   [2] big   [3] strip_v3   [4] sample   [5] kp (k')   [6] pages
 *   dense first pass:  [7] Mq   [8] Npad   [9] ns_tiles (the sample, when [4])   [10] strip (when [2])   [16] splits of select_topk
 *                      [23] groups per split
 *   scan first pass:   [11] nqt   [12] cap   [13] slabs   [14] tiles_per_block   [15] qtiles
 *   [17] the merge that ends the first pass runs in two levels
 *   widen pass:        [18] 1 = strip score GEMM, 0 = scan;  GEMM: [22] strip;  scan: [19] nqt  [20] slabs  [21] tiles_per_block */
struct mmiss_index;
int mmiss_dbg_index_plan(struct mmiss_index* ix, int32_t Q, int32_t k, int32_t filtered, int32_t flagged, int32_t* out);
/* The path a radius call (mmiss_index_query_radius*) of Q queries (filtered != 0: with masks) would take on the index as it
 * stands: its chunks of at most 1024 queries and the threshold pass of the first and of the last chunk (every chunk but the last
 * is a full one; strip_length and plan_dense of csrc/index_plans.h). Launches nothing, changes nothing, needs no device. out is a
 * HOST int32 [16]; fields that do not apply are 0:
 *   [0] chunks
 *   first chunk: [1] queries   [2] 1 = strip score GEMM, 0 = scan;  GEMM: [3] strip;  scan: [4] nqt  [5] slabs  [6] tiles_per_block
 *                [7] qtiles
 *   last chunk:  [8] .. [14] the same seven fields */
int mmiss_dbg_index_radius_plan(struct mmiss_index* ix, int32_t Q, int32_t filtered, int32_t* out);
/* The index's row store as it lies on the device: rows [row0, row0 + n) with 0 <= row0, row0 + n <= capacity (rows behind count
 * included; a range past the capacity is refused with MMISS_ERR_ARG). All outputs are HOST buffers and any may be NULL:
 * rows_out n * dim * (4 | 2 | 1) bytes, the raw f32 / f16 / e4m3 elements; inv_out f32 [n], the inverse norms of fp8 rows (left
 * untouched for f32 / f16 rows); labels_out int64 [n] and tags_out uint64 [n], the DEVICE copies of labels and tags. Reads
 * only: refuses an open query like every other entry, waits for the handle's stream first and returns drained. */
int mmiss_dbg_index_read_rows(struct mmiss_index* ix, int64_t row0, int64_t n, void* rows_out, float* inv_out, int64_t* labels_out,
                              uint64_t* tags_out);
/* The query preparation of a query call, alone: queries f32 [Q, dim] (host or device) go through the call's own upload and
 * prep_queries_kernel launch, and the handle's scratch comes back to HOST buffers (any may be NULL): qn_out f32 [Q, dim] the
 * normalised queries, qs_out [round_up(Q, 256), dim] the first pass's operand (f32 for f32 rows, f16 for f16 / fp8 rows; pad rows
 * included), eps_out f32 [Q] the guard's bound per query. Refuses an open query; returns drained. */
int mmiss_dbg_index_prep_queries(struct mmiss_index* ix, const float* queries, int32_t Q, float* qn_out, void* qs_out, float* eps_out);
/* How a probed call (mmiss_index_query_probed) of Q queries, this k (1 .. 2040) and this nprobe would run on the index's partition
 * as it stands and under the options as they stand (probe_scratch_kb: the scratch budget in KB, default 512 * 1024): the call's own
 * planning function (plan_probed, csrc/index_plans.h), evaluated on the host. Launches nothing, changes nothing. No partition -> MMISS_ERR_STATE. out is a HOST int32 [8]:
 *   [0] splits: workgroups per list of the scan   [1] segment size of the selection (keys)   [2] levels: segment_topk launches
 *   per chunk, the last (the one that writes the results) included   [3] queries per chunk   [4] the bound on one query's
 *   candidates (the tail and the min(nprobe, C) largest cells)   [5] share: rows of a list per scan workgroup   [6] probe slots
 *   min(nprobe, C)   [7] chunks */
int mmiss_dbg_index_probe_plan(struct mmiss_index* ix, int32_t Q, int32_t k, int32_t nprobe, int32_t* out);
/* How the suppression stage of a distinct call (mmiss_index_query_distinct) of Q >= 1 queries is laid out on this index: the call's
 * own planning function (plan_distinct, csrc/index_plans.h), evaluated on the host. Launches nothing, changes nothing. out is a
 * HOST int32 [8]:
 *   [0] rows per trip: consecutive list positions a workgroup takes at a time behind a kept entry (one per group of 16 lanes)
 *   [1] threads per workgroup (one workgroup per query)   [2] dynamic LDS bytes   [3] queries per launch   [4] launches per call
 *   [5] the largest pool   [6], [7] 0 */
int mmiss_dbg_index_distinct_plan(struct mmiss_index* ix, int32_t Q, int32_t* out);
/* How a subset call (mmiss_index_query_subset) of Q >= 1 queries, this k (1 .. 2040) and a list of n_cand >= 0 labels would run on
 * the index as it stands and under the options as they stand (probe_scratch_kb: the scratch budget in KB): the call's own planning
 * function (plan_subset, csrc/index_plans.h), evaluated on the host. Launches nothing, changes nothing. out is a HOST int32 [16]:
 *   [0] bound: min(n_cand, rows), the most rows the list can name   [1] segment size of the selection (keys)   [2] levels:
 *   segment_topk launches per chunk, the last (the one that writes the results) included   [3], [4] keys per query of the two key
 *   areas   [5] queries per chunk   [6] chunks   [7] query block: the queries a scan workgroup stages and scores each of its rows
 *   against   [8] the scan's dynamic LDS bytes   [9] share: list positions per scan workgroup   [10] splits: scan workgroups per
 *   query block   [11] list positions a scan workgroup takes per trip   [12] blocks of the bitmap's compaction   [13] rows per
 *   such block   [14], [15] the query block the first / the last chunk runs with: [7] halved while half of it still holds the
 *   chunk's queries */
int mmiss_dbg_index_subset_plan(struct mmiss_index* ix, int32_t Q, int32_t k, int64_t n_cand, int32_t* out);
/* How a grouped call (mmiss_index_query_grouped) would run on the index as it stands and under the options as they stand
 * (probe_scratch_kb), if Q >= 1 of its queries took the exhaustive route, at this k (1 .. 2040) and pool (0, or k .. 2040):
 * plan_grouped (csrc/index_plans.h), evaluated on the host. Launches nothing, changes nothing. out is a HOST int32 [16]:
 *   [0] the pool of the list stage (pool 0 resolved)   [1] threads of the walk's workgroup (one per query, one launch)   [2] its
 *   LDS bytes   [3] table: slots per query of the exhaustive route, G + rows (G: the largest group id set since the last clear or
 *   load, + 1)   [4] segment size of the selection (keys)   [5] levels: segment_topk launches per chunk, the last included
 *   [6], [7] keys per query of the two key areas   [8] queries per chunk   [9] chunks   [10] query block of the scan   [11] its
 *   dynamic LDS bytes   [12] share: rows per scan workgroup   [13] splits: scan workgroups per query block   [14], [15] the query
 *   block the first / the last chunk runs with */
int mmiss_dbg_index_grouped_plan(struct mmiss_index* ix, int32_t Q, int32_t k, int32_t pool, int32_t* out);
/* How a continuation call (mmiss_index_query_after) of Q >= 1 queries, this k (1 .. 2040) and a list of n_cand labels (n_cand < 0:
 * no list, the dense scan over every row) would run on the index as it stands and under the options as they stand: plan_after
 * (csrc/index_plans.h), evaluated on the host. Launches nothing, changes nothing. out is a HOST int32 [16], laid out as
 * mmiss_dbg_index_subset_plan's except:
 *   [0] bound: rows without a list, min(n_cand, rows) with one   [12] blocks of the bitmap's compaction: 0 without a list
 *   [13] 1: the dense scan (position i is row i), 0: the listed one */
int mmiss_dbg_index_after_plan(struct mmiss_index* ix, int32_t Q, int32_t k, int64_t n_cand, int32_t* out);
/* How the dense scans and the kernels behind them would walk the index as it stands with n_operands (1 .. 1024) probes, centres or
 * clusters: the calls' own planning functions (plan_dense by passes, the capped grids, plan_cluster_sums, subset_compact_blocks;
 * csrc/index_plans.h), evaluated on the host. Launches nothing, changes nothing. out is a HOST int32 [40]; an empty index leaves
 * all but [37] 0:
 *   the scan of membership / assignment: [0] nqt   [1] dynamic LDS bytes   [2] slabs   [3] tiles_per_block   [4] passes
 *     [5] trips of every wave of a full block (tiles_per_block / 4)   [6] rows of a block (16 * tiles_per_block)
 *   grid-stride kernels, three fields each — blocks, rows (or list positions) the grid covers per trip, trips over the rows:
 *     [8] canonical_scan   [11] assign_resolve   [14] member_count   [17] assign_sizes   [20] assign_decide
 *     [23] member_from_dist   [26] member_merge_tags
 *   cluster sums into n_operands clusters: [30] columns per chunk   [31] chunks   [32] rows per block   [33] slabs   [34] LDS bytes
 *   the subset call's compaction: [35] blocks   [36] rows per block
 *   [37] rows of the index */
int mmiss_dbg_index_dense_plan(struct mmiss_index* ix, int32_t n_operands, int32_t* out);


/* The path one chunk of an encode call would take on the handle as it stands and under the options as they stand: B items
 * (1 .. the tower's max_batch) on `tower` (MMISS_TOWER_*), T tokens per item for the text tower (the vision tower's is fixed: pass 0).
 * The encoder's own planning functions, evaluated on the host; no kernel is launched. Like an encode call it allocates the tower's
 * workspaces (zero-filled) if they do not exist yet, because the plan depends on which of them there are. out is a HOST int32 [32]:
 *   [0] fold   [1] fold_final   [2] fp8   [3] out8   [4] resid16   [5] sfold   [6] prune
 *   [7] embed: 0 nothing, 1 xb + 64-column statistics, 2 xb + 16-column statistics (one request)
 *   [8],[9] kernel and tile height of the QKV GEMM   [10],[11] out-projection   [12],[13] FC1   [14],[15] FC2
 *        kernel: 0 BM x 128 tile (the launcher takes the skinny kernel for few rows), 1 256 x 256 tile, 2 persistent 256 x 256,
 *        3 160 x 256 residual, 4 skinny with the LayerNorm folded in, 5 fp8 BM x 128 tile, 6 persistent fp8
 *   [16] the pruned last layer runs the pooled-query tail   [17] FC2 is a split-K candidate   [18] M = B * T
 *   vision only: [19] lean pre-LayerNorm   [20],[21] kernel and tile height of the patch GEMM   [22] it is a split-K candidate
 *   the attention kernel (the token count picks the family: up to 128 one pass, up to 288 long, above it key chunks):
 *   [23] heads per workgroup of the one-pass kernels (attention_pick_hpb; it applies up to 128 tokens)
 *   [24] the shape may run on the streaming kernel (attention_stream_ok; option attention_stream = 0 keeps the long kernel)
 *   [25..31] 0 */
int mmiss_dbg_encoder_plan(struct mmiss_encoder* enc, int32_t tower, int32_t B, int32_t T, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif

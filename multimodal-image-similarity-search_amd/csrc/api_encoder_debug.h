// api_encoder_debug.h — the debug ABI of the encoder (include/mmiss_debug.h): single kernels on caller-owned buffers, for tests/ and
// tools/. Included once, as the last line of api_encoder.hip: the same translation unit, so no kernel is instantiated twice.
// An entry checks its ABI arguments, makes the device current and calls the launcher the encoder itself calls (the launch_*
// functions beside the kernels); it owns no grid formula, no kernel precondition and no profile record of its own.

// the streams and events of a timing entry, destroyed on every path
struct TimingHandles {
    hipStream_t s0 = nullptr, s1 = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, fork = nullptr, join = nullptr;
    ~TimingHandles() {
        for (hipEvent_t e : {e0, e1, fork, join}) if (e) (void)hipEventDestroy(e);
        for (hipStream_t s : {s0, s1}) if (s) (void)hipStreamDestroy(s);
    }
};

// ms per launch of run() on st over `iters` launches, after three warm-up launches
template <typename Run>
static int time_launches(hipStream_t st, int iters, Run&& run, float* ms_per_launch) {
    TimingHandles h;
    MM_HIP(hipEventCreate(&h.e0));
    MM_HIP(hipEventCreate(&h.e1));
    for (int i = 0; i < 3; ++i) MM_TRY(run());
    MM_HIP(hipEventRecord(h.e0, st));
    for (int i = 0; i < iters; ++i) MM_TRY(run());
    MM_HIP(hipEventRecord(h.e1, st));
    MM_HIP(hipEventSynchronize(h.e1));
    float ms = 0.f;
    MM_HIP(hipEventElapsedTime(&ms, h.e0, h.e1));
    *ms_per_launch = ms / iters;
    return MMISS_OK;
}

// debug entries only: scratch so that the split-K path can be exercised (mmiss_dbg_gemm and mmiss_dbg_gemm_ex share it)
static int dbg_splitk_scratch(GemmEpi& ep, int32_t M, int32_t N) {
    static DevBuf dbg_splitk;
    if (M > 0 && N > 0 && (int64_t)M * N <= (1 << 22)) {
        MM_TRY(dbg_splitk.ensure((size_t)8 * M * N * 4));
        ep.splitk_ws = dbg_splitk.as<float>(); ep.splitk_ws_bytes = dbg_splitk.bytes;
    }
    return MMISS_OK;
}

extern "C" int mmiss_dbg_gemm(int device, void* hip_stream, int epi, int variant, const void* A, const void* W,
                              void* out, const float* bias, const float* aux, int32_t M, int32_t N, int32_t K,
                              int32_t p0, int32_t p1) {
    if (!A || !W || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm: null pointer");
    MM_TRY(mmiss_use_device(device));
    GemmEpi ep{};
    ep.out = out; ep.bias = bias; ep.aux = aux; ep.ldo = N; ep.m_valid = M; ep.p0 = p0; ep.p1 = p1;
    MM_TRY(dbg_splitk_scratch(ep, M, N));
    if (variant == 256) return launch_gemm256(reinterpret_cast<hipStream_t>(hip_stream), epi, A, W, ep, M, N, K);
    if (variant > 1000) MM_FAIL(MMISS_ERR_UNSUPPORTED, "GEMM variant %d (ring pipeline / BM x 256 tiles) was removed in round 4: measured slower, profiles/gemm_variants_r01.md", variant);
    return launch_gemm(reinterpret_cast<hipStream_t>(hip_stream), epi, variant, A, W, ep, M, N, K);
}

// mmiss_dbg_gemm with the pad-row mask, the residual epilogue's by-products and the folded epilogues: 0 .. 4 through launch_gemm
// (variant 256: launch_gemm256), 7 / 8 through launch_gemm_fold (variant 256: launch_gemm256). The launchers decide what runs.
extern "C" int mmiss_dbg_gemm_ex(int device, void* hip_stream, int epi, int variant, const void* A, const void* W, void* out,
                                 const float* bias, const float* aux, int32_t M, int32_t N, int32_t K, int32_t p0, int32_t p1,
                                 int32_t m_valid, float* stats_out, void* xb_out, const float* ln_stats, float ln_eps) {
    if (!A || !W || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_ex: null pointer");
    const bool fold = epi == MMISS_EPI_LNFOLD_BF16 || epi == MMISS_EPI_LNFOLD_QGELU_BF16;
    if (!fold && (epi < 0 || epi > 4)) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_ex: epilogue %d", epi);
    if (m_valid < 1 || m_valid > M) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_ex: m_valid=%d outside 1..M=%d", m_valid, M);
    if ((epi >= MMISS_EPI_BIAS_BF16 && epi <= MMISS_EPI_BIAS_RESID_F32 && !bias) || (fold && (!bias || !aux || !ln_stats)) ||
        (epi == MMISS_EPI_PATCH_F32 && (!aux || p0 <= 0 || p1 < p0 + 1)))
        MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_ex: epilogue %d lacks an operand", epi);
    if ((stats_out || xb_out) && epi != MMISS_EPI_BIAS_RESID_F32)
        MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_ex: stats_out / xb_out belong to the f32 residual epilogue, not %d", epi);
    if (ln_stats && !fold) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_ex: ln_stats belong to epilogues 7 / 8, not %d", epi);
    if (variant > 1000) MM_FAIL(MMISS_ERR_UNSUPPORTED, "GEMM variant %d was removed in round 4", variant);
    MM_TRY(mmiss_use_device(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    GemmEpi ep{};
    ep.out = out; ep.bias = bias; ep.aux = aux; ep.ldo = N; ep.m_valid = m_valid; ep.p0 = p0; ep.p1 = p1;
    ep.stats_out = stats_out; ep.xb_out = xb_out;
    if (fold) {
        ep.ln_stats = ln_stats; ep.ln_parts = K / 64; ep.ln_eps = ln_eps;
        if (variant == 256) return launch_gemm256(st, epi, A, W, ep, M, N, K);
        return launch_gemm_fold(st, epi, variant, A, W, ep, M, N, K);
    }
    MM_TRY(dbg_splitk_scratch(ep, M, N));
    if (variant == 256) return launch_gemm256(st, epi, A, W, ep, M, N, K);
    return launch_gemm(st, epi, variant, A, W, ep, M, N, K);
}

// the gemm16_kernel form launch_gemm_stages picks under the current options: 10 * staging buffers + waves (0: no such launch)
extern "C" int mmiss_dbg_gemm_form(int32_t bm, int32_t M, int32_t N, int32_t K, int32_t splits) {
    if (bm == 0) bm = 128;
    if ((bm != 128 && bm != 160 && bm != 192) || M <= 0 || N <= 0 || K <= 0 || splits < 1 || (M % bm) || (N % GEMM_BN) ||
        (K % (splits * GEMM_BK)))
        return 0;
    const Gemm16Form f = gemm16_form(bm, (int64_t)(M / bm) * (N / GEMM_BN) * splits, K, splits);
    return f.bufs * 10 + f.waves;
}

// the persistent 256 x 256 kernel in isolation (gemm_bf16_p256.h): epi 1 / 2 (bias, bias + QuickGELU) or 7 / 8 (the same
// behind a folded LayerNorm: ln_stats [M][K/64][2], aux = c [N], bias = b' [N]); iters > 0 also times it
extern "C" int mmiss_dbg_gemm_p256(int device, void* hip_stream, int epi, const void* A, const void* W, void* out,
                                   const float* bias, const float* aux, const float* ln_stats, float ln_eps, int32_t M,
                                   int32_t N, int32_t K, int32_t m_valid, int32_t iters, float* ms_per_launch) {
    if (!A || !W || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_p256: null pointer");
    MM_TRY(mmiss_use_device(device));
    GemmEpi ep{};
    ep.out = out; ep.bias = bias; ep.aux = aux; ep.ldo = N; ep.m_valid = m_valid;
    ep.ln_stats = ln_stats; ep.ln_parts = K / 64; ep.ln_eps = ln_eps;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    auto run = [&]() -> int { return launch_gemm256p(st, epi, A, W, ep, M, N, K); };
    if (iters <= 0 || !ms_per_launch) return run();
    return time_launches(st, iters, run, ms_per_launch);
}

// the residual GEMM on a bf16 stream (out = bf16(f32(out) + A W^T + bias), in place; stats_out [M][N/64][2] optional) in
// isolation: variant 0 = the 160 x 256 tile on the staggered loop (gemm160p_kernel), 128 / 160 / 192 = the 128-column kernel
// with that tile height; iters > 0 also times it (the stream keeps accumulating: only the time means anything then)
extern "C" int mmiss_dbg_gemm_resid16(int device, void* hip_stream, int variant, const void* A, const void* W, void* out,
                                      const float* bias, float* stats_out, int32_t M, int32_t N, int32_t K, int32_t m_valid,
                                      int32_t iters, float* ms_per_launch) {
    if (!A || !W || !out || !bias) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_resid16: null pointer");
    MM_TRY(mmiss_use_device(device));
    GemmEpi ep{};
    ep.out = out; ep.bias = bias; ep.ldo = N; ep.m_valid = m_valid; ep.stats_out = stats_out;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    auto run = [&]() -> int {
        return variant == 0 ? launch_gemm160p(st, A, W, ep, M, N, K) : launch_gemm_resid16(st, variant, A, W, ep, M, N, K);
    };
    if (iters <= 0 || !ms_per_launch) return run();
    return time_launches(st, iters, run, ms_per_launch);
}

extern "C" int mmiss_dbg_gemm_time(int device, int epi, int variant, const void* A, const void* W, void* out,
                                   const float* bias, const float* aux, int32_t M, int32_t N, int32_t K, int32_t p0,
                                   int32_t p1, int32_t iters, float* ms_per_launch) {
    if (!A || !W || !out || !ms_per_launch || iters <= 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_time: bad argument");
    MM_TRY(mmiss_use_device(device));
    GemmEpi ep{};
    ep.out = out; ep.bias = bias; ep.aux = aux; ep.ldo = N; ep.m_valid = M; ep.p0 = p0; ep.p1 = p1;
    auto run = [&]() -> int {
        if (variant == 256) return launch_gemm256(nullptr, epi, A, W, ep, M, N, K);
        if (variant > 1000) MM_FAIL(MMISS_ERR_UNSUPPORTED, "GEMM variant %d was removed in round 4", variant);
        return launch_gemm(nullptr, epi, variant, A, W, ep, M, N, K);
    };
    return time_launches(nullptr, iters, run, ms_per_launch);
}

extern "C" int mmiss_dbg_layernorm(int device, void* hip_stream, const float* x, const float* gamma, const float* beta,
                                   void* out, int32_t out_bf16, int32_t M, int32_t d, float eps) {
    if (!x || !gamma || !beta || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_layernorm: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_layernorm(reinterpret_cast<hipStream_t>(hip_stream), x, gamma, beta, out, out_bf16 != 0, nullptr, M, d,
                            eps);
}

extern "C" int mmiss_dbg_attention(int device, void* hip_stream, const void* qkv, void* ctx, int32_t B, int32_t T,
                                   int32_t H, int32_t causal) {
    if (!qkv || !ctx) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_attention: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_attention(reinterpret_cast<hipStream_t>(hip_stream), qkv, ctx, B, T, H, causal != 0);
}

extern "C" int mmiss_dbg_attention_pooled(int device, void* hip_stream, const void* qkv, const int32_t* pool_row, void* ctxc,
                                          int32_t B, int32_t T, int32_t H, int32_t causal) {
    if (!qkv || !pool_row || !ctxc) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_attention_pooled: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_attention_pooled(reinterpret_cast<hipStream_t>(hip_stream), qkv, ctxc, pool_row, B, T, H, causal != 0);
}

// attention_tiled_kernel at any 1 <= T <= MMISS_MAX_TOKENS (the product routes T <= 288 to the other kernels): bf16 rows into ctx,
// or with ctx8 != NULL MXFP8 into ctx8 / ctx_scale (non-causal)
extern "C" int mmiss_dbg_attention_tiled(int device, void* hip_stream, const void* qkv, void* ctx, void* ctx8, void* ctx_scale,
                                         int32_t B, int32_t T, int32_t H, int32_t causal) {
    if (!qkv || (!ctx8 && !ctx) || (ctx8 && !ctx_scale)) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_attention_tiled: null pointer");
    if (T <= 0 || T > MMISS_MAX_TOKENS || H <= 0 || B < 0 || (ctx8 && causal))
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "mmiss_dbg_attention_tiled: B=%d T=%d (1..%d) H=%d causal=%d%s", B, T, MMISS_MAX_TOKENS, H, causal,
                ctx8 ? " (MXFP8 output is non-causal)" : "");
    MM_TRY(mmiss_use_device(device));
    if (B == 0) return MMISS_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (ctx8)
        return launch_attention_tiled<false, true>(st, qkv, nullptr, reinterpret_cast<uint8_t*>(ctx8), reinterpret_cast<uint8_t*>(ctx_scale),
                                                   mx_scale_row_bytes(H * 64), B, T, H);
    return causal ? launch_attention_tiled<true, false>(st, qkv, ctx, nullptr, nullptr, 0, B, T, H)
                  : launch_attention_tiled<false, false>(st, qkv, ctx, nullptr, nullptr, 0, B, T, H);
}

// The LayerNorm chain around the folded GEMMs, kernel by kernel: the launchers encode_image_chunk / run_layers / run_wide /
// mmiss_encoder_finalize call, on caller-owned buffers.
extern "C" int mmiss_dbg_layernorm16(int device, void* hip_stream, const void* x_bf16, const float* gamma, const float* beta,
                                     void* out_bf16, int32_t M, int32_t d, float eps) {
    if (!x_bf16 || !gamma || !beta || !out_bf16) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_layernorm16: null pointer");
    if (M <= 0) MM_FAIL(MMISS_ERR_UNSUPPORTED, "layernorm16: M=%d", M);
    MM_TRY(mmiss_use_device(device));
    return launch_layernorm16(reinterpret_cast<hipStream_t>(hip_stream), reinterpret_cast<const uint16_t*>(x_bf16), gamma, beta,
                              out_bf16, M, d, eps);
}

extern "C" int mmiss_dbg_layernorm_gather(int device, void* hip_stream, const float* x, const float* gamma, const float* beta,
                                          void* out, int32_t out_bf16, const int32_t* rowmap, int32_t M, int32_t d, float eps) {
    if (!x || !gamma || !beta || !out || !rowmap) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_layernorm_gather: null pointer");
    if (M <= 0) MM_FAIL(MMISS_ERR_UNSUPPORTED, "layernorm_gather: M=%d", M);
    MM_TRY(mmiss_use_device(device));
    return launch_layernorm(reinterpret_cast<hipStream_t>(hip_stream), x, gamma, beta, out, out_bf16 != 0, rowmap, M, d, eps);
}

extern "C" int mmiss_dbg_prelayernorm_stats(int device, void* hip_stream, float* x, const float* gamma, const float* beta, void* xb,
                                            float* stats, int32_t M, int32_t d, int32_t parts, float eps, int32_t lean,
                                            const float* cls, const float* pos, int32_t T) {
    if (!x || !gamma || !beta || !xb || !stats || (lean && (!cls || !pos)))
        MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_prelayernorm_stats: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_layernorm_stats(reinterpret_cast<hipStream_t>(hip_stream), x, gamma, beta, reinterpret_cast<uint16_t*>(xb), stats, M, d,
                                  parts, eps, lean != 0, cls, pos, T);
}

extern "C" int mmiss_dbg_prelayernorm_skinny(int device, void* hip_stream, float* x, const float* cls, const float* pos,
                                             const float* gamma, const float* beta, void* xb, float* stats16, int32_t M, int32_t T,
                                             int32_t d, float eps) {
    if (!x || !cls || !pos || !gamma || !beta || !xb || !stats16) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_prelayernorm_skinny: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_prelayernorm_skinny(reinterpret_cast<hipStream_t>(hip_stream), x, cls, pos, gamma, beta, reinterpret_cast<uint16_t*>(xb),
                                      stats16, M, T, d, eps);
}

extern "C" int mmiss_dbg_row_stats(int device, void* hip_stream, const float* x, float* stats, void* xb_or_null, int32_t M, int32_t d,
                                   int32_t parts) {
    if (!x || !stats) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_row_stats: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_row_stats(reinterpret_cast<hipStream_t>(hip_stream), x, stats, reinterpret_cast<uint16_t*>(xb_or_null), M, d, parts, true);
}

// The one-request folded chain (P.sfold), kernel by kernel: the launchers run_layers / run_wide / run_resid call, on caller-owned
// buffers. None of the three falls back to a tiled kernel: where the skinny path would not run they refuse.
extern "C" int mmiss_dbg_row_stats16(int device, void* hip_stream, const float* x, float* stats16, void* xb, int32_t M, int32_t d) {
    if (!x || !stats16 || !xb) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_row_stats16: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_row_stats16(reinterpret_cast<hipStream_t>(hip_stream), x, stats16, reinterpret_cast<uint16_t*>(xb), M, d);
}

extern "C" int mmiss_dbg_gemm_skinny_fold(int device, void* hip_stream, int epi, const void* A, const void* Wf, void* out, const float* bf,
                                          const float* c, const float* stats16, float eps, int32_t M, int32_t N, int32_t K) {
    if (!A || !Wf || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_skinny_fold: null pointer");
    // (the kernel reads a row's partials, c and b' as 16-byte vectors)
    if ((reinterpret_cast<uintptr_t>(stats16) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(bf)) & 15)
        MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_skinny_fold: stats16, c and bf must be 16-byte aligned");
    if (epi != MMISS_EPI_LNFOLD_BF16 && epi != MMISS_EPI_LNFOLD_QGELU_BF16)
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "gemm_skinny_fold: epilogue %d (7 or 8)", epi);
    if (M <= 0 || N <= 0 || K <= 0) MM_FAIL(MMISS_ERR_UNSUPPORTED, "gemm_skinny_fold: M=%d N=%d K=%d", M, N, K);
    MM_TRY(mmiss_use_device(device));
    GemmEpi ep{};
    ep.out = out; ep.bias = bf; ep.aux = c; ep.ldo = N; ep.m_valid = M;
    ep.ln_stats = stats16; ep.ln_eps = eps; ep.ln_parts = K / 16; ep.stats16 = 1;
    return launch_gemm_skinny_fold(reinterpret_cast<hipStream_t>(hip_stream), epi, A, Wf, ep, M, N, K);
}

extern "C" int mmiss_dbg_gemm_skinny_resid(int device, void* hip_stream, const void* A, const void* W, float* x, const float* bias,
                                           float* stats16_out, void* xb_out, int32_t M, int32_t N, int32_t K) {
    if (!A || !W || !x || !bias) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_skinny_resid: null pointer");
    GemmEpi ep{};
    ep.out = x; ep.bias = bias; ep.ldo = N; ep.m_valid = M;
    ep.stats_out = stats16_out; ep.xb_out = xb_out; ep.stats16 = 1;
    if (M <= 0 || N <= 0 || K <= 0 || !gemm_skinny_ok(MMISS_EPI_BIAS_RESID_F32, M, N, K, ep))
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "gemm_skinny_resid: M=%d N=%d K=%d is not a skinny GEMM", M, N, K);
    MM_TRY(mmiss_use_device(device));
    return launch_gemm(reinterpret_cast<hipStream_t>(hip_stream), MMISS_EPI_BIAS_RESID_F32, 128, A, W, ep, (int)round_up(M, 128), N, K);
}

extern "C" int mmiss_dbg_ln_finalize(int device, void* hip_stream, const float* stats, float* out, int32_t M, int32_t parts, int32_t d,
                                     float eps) {
    if (!stats || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_ln_finalize: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_ln_finalize(reinterpret_cast<hipStream_t>(hip_stream), stats, out, M, parts, d, eps);
}

extern "C" int mmiss_dbg_fold_ln_weights(int device, void* hip_stream, const void* w_bf16, const float* gamma, const float* beta,
                                         const float* bias, void* wf, float* c, float* bf, int32_t N, int32_t K) {
    if (!w_bf16 || !gamma || !beta || !bias || !wf || !c || !bf) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_fold_ln_weights: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_fold_ln_weights(reinterpret_cast<hipStream_t>(hip_stream), reinterpret_cast<const uint16_t*>(w_bf16), gamma, beta, bias,
                                  reinterpret_cast<uint16_t*>(wf), c, bf, N, K);
}

extern "C" int mmiss_dbg_gemm_resid_rows(int device, void* hip_stream, const void* A, const void* W, float* out, const float* bias,
                                         const void* rows_bf16, const int32_t* rowmap, int32_t M, int32_t N, int32_t K) {
    if (!A || !W || !out || !bias || !rows_bf16 || !rowmap) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_resid_rows: null pointer");
    MM_TRY(mmiss_use_device(device));
    GemmEpi ep{};
    ep.out = out; ep.bias = bias; ep.ldo = N; ep.m_valid = M;
    ep.resid16_rows = reinterpret_cast<const uint16_t*>(rows_bf16); ep.resid_rowmap = rowmap;
    return launch_gemm(reinterpret_cast<hipStream_t>(hip_stream), MMISS_EPI_BIAS_RESID_F32, 128, A, W, ep, (int)round_up(M, 128), N, K);
}

extern "C" int mmiss_dbg_patch_from_pixels(int device, void* hip_stream, const float* pixels, const void* W, float* out,
                                           const float* pos, int32_t B, int32_t S, int32_t P, int32_t d) {
    if (!pixels || !W || !out || !pos) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_patch_from_pixels: null pointer");
    if (P <= 0 || S <= 0 || S % P || B <= 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_patch_from_pixels: B=%d S=%d P=%d", B, S, P);
    MM_TRY(mmiss_use_device(device));
    const int G = S / P;
    GemmEpi ep{};
    ep.out = out; ep.aux = pos; ep.ldo = d; ep.m_valid = B * G * G; ep.p0 = G * G; ep.p1 = G * G + 1;
    return launch_gemm160p_patch_pix(reinterpret_cast<hipStream_t>(hip_stream), pixels, W, ep, B, S, P, (int)round_up(B * G * G, 160), d,
                                     3 * P * P);
}

extern "C" int mmiss_dbg_im2col(int device, void* hip_stream, const float* pixels, void* out, int32_t B, int32_t S,
                                int32_t P, int32_t Kp) {
    if (!pixels || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_im2col: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_im2col(reinterpret_cast<hipStream_t>(hip_stream), pixels, false, out, B, S, P, Kp);
}


// Experiment (tools/gemm_split_test.py): one GEMM over M rows vs two half-M GEMMs back to back vs the two halves on
// two streams joined by events. ms[0..2] = milliseconds per GEMM-equivalent.
extern "C" int mmiss_dbg_gemm_split_time(int device, int epi, int bm, const void* A, const void* W, void* out,
                                         const float* bias, int32_t M, int32_t N, int32_t K, int32_t iters, float* ms) {
    if (!A || !W || !out || !ms || iters <= 0 || (M % (2 * bm))) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm_split_time: bad argument");
    MM_TRY(mmiss_use_device(device));
    TimingHandles h;
    MM_HIP(hipStreamCreateWithFlags(&h.s0, hipStreamNonBlocking));
    MM_HIP(hipStreamCreateWithFlags(&h.s1, hipStreamNonBlocking));
    MM_HIP(hipEventCreate(&h.e0)); MM_HIP(hipEventCreate(&h.e1));
    MM_HIP(hipEventCreateWithFlags(&h.fork, hipEventDisableTiming)); MM_HIP(hipEventCreateWithFlags(&h.join, hipEventDisableTiming));
    const hipStream_t s0 = h.s0, s1 = h.s1;
    const int out_elt = (epi == MMISS_EPI_BIAS_BF16 || epi == MMISS_EPI_BIAS_QGELU_BF16) ? 2 : 4;
    const int Mh = M / 2;
    auto full = [&](hipStream_t s) -> int {
        GemmEpi ep{}; ep.out = out; ep.bias = bias; ep.ldo = N; ep.m_valid = M;
        return launch_gemm(s, epi, bm, A, W, ep, M, N, K);
    };
    auto half = [&](hipStream_t s, int which) -> int {
        GemmEpi ep{}; ep.out = (char*)out + (size_t)which * Mh * N * out_elt; ep.bias = bias; ep.ldo = N; ep.m_valid = Mh;
        return launch_gemm(s, epi, bm, (const char*)A + (size_t)which * Mh * K * 2, W, ep, Mh, N, K);
    };
    for (int mode = 0; mode < 3; ++mode) {
        for (int it = -3; it < iters; ++it) {
            if (it == 0) MM_HIP(hipEventRecord(h.e0, s0));
            if (mode == 0) { MM_TRY(full(s0)); }
            else if (mode == 1) { MM_TRY(half(s0, 0)); MM_TRY(half(s0, 1)); }
            else {
                MM_HIP(hipEventRecord(h.fork, s0));
                MM_HIP(hipStreamWaitEvent(s1, h.fork, 0));
                MM_TRY(half(s0, 0));
                MM_TRY(half(s1, 1));
                MM_HIP(hipEventRecord(h.join, s1));
                MM_HIP(hipStreamWaitEvent(s0, h.join, 0));
            }
        }
        MM_HIP(hipEventRecord(h.e1, s0));
        MM_HIP(hipEventSynchronize(h.e1));
        float t = 0.f;
        MM_HIP(hipEventElapsedTime(&t, h.e0, h.e1));
        ms[mode] = t / iters;
    }
    return MMISS_OK;
}

// ------------------------------------------------------------------------------------------------ calibration kernels in isolation
// x f32 (or bf16 when x_is_bf16) [M,d] -> the column statistics of LayerNorm(x; gamma, beta): mean_out, var_out f64 [d] (population
// variance), mu_out f32 [d] (the mean where mean^2 >= var, else 0), centred_out int32 [1]
extern "C" int mmiss_dbg_ln_colstats(int device, void* hip_stream, const void* x, int32_t x_is_bf16, const float* gamma, const float* beta,
                                     int32_t M, int32_t d, float eps, double* mean_out, double* var_out, float* mu_out, int32_t* centred_out) {
    if (!x || !gamma || !beta || !mean_out || !var_out || !mu_out || !centred_out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_ln_colstats: null pointer");
    if (M < 1) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_ln_colstats: M = %d", M);
    MM_TRY(mmiss_use_device(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    DevBuf part;   // (debug entry only: allocated and freed around the call)
    MM_TRY(part.alloc(cal_partial_bytes(M, d)));
    MM_TRY(launch_ln_colstats(st, x, x_is_bf16 != 0, gamma, beta, part.as<double>(), M, d, eps, mu_out, nullptr, centred_out, mean_out, var_out));
    MM_HIP(hipStreamSynchronize(st));
    return MMISS_OK;
}

extern "C" int mmiss_dbg_bias_fold(int device, void* hip_stream, const void* w_bf16, const float* bias, const float* mu, int32_t N, int32_t K,
                                   float* out) {
    if (!w_bf16 || !bias || !mu || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_bias_fold: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_bias_fold(reinterpret_cast<hipStream_t>(hip_stream), w_bf16, bias, mu, out, N, K);
}

// ------------------------------------------------------------------------------------------------ resize tables in isolation
// resize_geometry + resize_chunk's launcher of resize_coeffs_kernel for a single descriptor, with resize_chunk's pool layout
extern "C" int mmiss_dbg_resize_coeffs(int device, void* hip_stream, int32_t H, int32_t W, int32_t S, int32_t* geometry,
                                       int32_t* pool, int32_t* bounds) {
    if (!geometry) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_resize_coeffs: null geometry");
    if ((pool == nullptr) != (bounds == nullptr)) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_resize_coeffs: pool and bounds go together");
    if (S < 1 || S > (1 << 14)) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_resize_coeffs: S = %d outside 1..16384", S);
    if (H < 1 || W < 1 || H > (1 << 16) || W > (1 << 16))
        MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_resize_coeffs: size %d x %d outside 1..65536", W, H);
    ResizeDesc d;
    resize_geometry(H, W, S, d);
    if (d.ksx > 4096 || d.ksy > 4096)
        MM_FAIL(MMISS_ERR_UNSUPPORTED, "mmiss_dbg_resize_coeffs: %d x %d -> %d needs %d / %d filter taps (limit 4096)", W, H, S, d.ksx,
                d.ksy);
    d.src_off = 0;
    d.kx_off = 0;
    d.ky_off = (int64_t)d.ksx * S;
    const int32_t g[6] = {d.new_h, d.new_w, d.top, d.left, d.ksx, d.ksy};
    memcpy(geometry, g, sizeof(g));
    if (!pool) return MMISS_OK;
    MM_TRY(mmiss_use_device(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    DevBuf dd;   // (debug entry only: allocated and freed around the call)
    MM_TRY(dd.alloc(sizeof(ResizeDesc)));
    MM_HIP(hipMemcpyAsync(dd.p, &d, sizeof(ResizeDesc), hipMemcpyHostToDevice, st));
    MM_TRY(launch_resize_coeffs(st, dd.as<ResizeDesc>(), pool, bounds, S, 1, (int64_t)(d.ksx + d.ksy) * S));
    MM_HIP(hipStreamSynchronize(st));  // the descriptor is freed on return, and is read from this stack frame
    return MMISS_OK;
}

extern "C" int mmiss_dbg_resize_crop_variant(int64_t blob_bytes, int32_t max_ksx) { return resize_crop_variant(blob_bytes, max_ksx); }

// ------------------------------------------------------------------------------------------------ fp8 kernels in isolation
extern "C" int mmiss_dbg_quantize_weights_fp8(int device, void* hip_stream, const void* w_bf16, void* w8, float* scale,
                                              int32_t N, int32_t K) {
    if (!w_bf16 || !w8 || !scale) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_quantize_weights_fp8: bad argument");
    MM_TRY(mmiss_use_device(device));
    return launch_quantize_weights_fp8(reinterpret_cast<hipStream_t>(hip_stream), reinterpret_cast<const uint16_t*>(w_bf16),
                                       reinterpret_cast<uint8_t*>(w8), scale, N, K);
}

// bf16 rows in (the bf16 residual stream): d = 512 / 1024 take the wide kernel of round 4, other d the first form
extern "C" int mmiss_dbg_layernorm16_mxfp8(int device, void* hip_stream, const void* x_bf16, const float* gamma, const float* beta,
                                           void* out8, void* out_scale, int32_t M, int32_t d, float eps) {
    if (!x_bf16 || !gamma || !beta || !out8 || !out_scale) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_layernorm16_mxfp8: null pointer");
    if (M <= 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_layernorm16_mxfp8: M = %d", M);
    MM_TRY(mmiss_use_device(device));
    return launch_layernorm_mxfp8(reinterpret_cast<hipStream_t>(hip_stream), x_bf16, true, gamma, beta,
                                  reinterpret_cast<uint8_t*>(out8), reinterpret_cast<uint8_t*>(out_scale), M, d, eps);
}

// qkv bf16 [B*T, 3*H*64] -> the attention output as MXFP8: ctx8 e4m3 [B*T, H*64] + permuted E8M0 scales [B*T, 16 * ceil(H*64 / 512)]
// (non-causal; T <= 128: the one-pass kernels, 129 <= T <= 288: the long-sequence form, above up to MMISS_MAX_TOKENS: key chunks)
extern "C" int mmiss_dbg_attention_mx(int device, void* hip_stream, const void* qkv, void* ctx8, void* ctx_scale, int32_t B,
                                      int32_t T, int32_t H) {
    if (!qkv || !ctx8 || !ctx_scale) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_attention_mx: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_attention_mx(reinterpret_cast<hipStream_t>(hip_stream), qkv, reinterpret_cast<uint8_t*>(ctx8),
                               reinterpret_cast<uint8_t*>(ctx_scale), mx_scale_row_bytes(H * 64), B, T, H);
}

extern "C" int mmiss_dbg_layernorm_mxfp8(int device, void* hip_stream, const float* x, const float* gamma, const float* beta,
                                         void* out8, void* out_scale, int32_t M, int32_t d, float eps) {
    if (!x || !gamma || !beta || !out8 || !out_scale) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_layernorm_mxfp8: null pointer");
    MM_TRY(mmiss_use_device(device));
    return launch_layernorm_mxfp8(reinterpret_cast<hipStream_t>(hip_stream), x, false, gamma, beta, reinterpret_cast<uint8_t*>(out8),
                                  reinterpret_cast<uint8_t*>(out_scale), M, d, eps);
}

extern "C" int mmiss_dbg_gemm8(int device, void* hip_stream, int epi, int bm, const void* A8, const void* As, const void* W8,
                               const float* wscale, const float* bias, void* out, void* out_scale, int32_t M, int32_t N,
                               int32_t K) {
    MM_TRY(mmiss_use_device(device));
    Gemm8Args g{};
    g.A = reinterpret_cast<const uint8_t*>(A8); g.As = reinterpret_cast<const uint8_t*>(As); g.ld_as = mx_scale_row_bytes(K);
    g.W = reinterpret_cast<const uint8_t*>(W8); g.wscale = wscale; g.bias = bias; g.out = out;
    g.out_scale = reinterpret_cast<uint8_t*>(out_scale); g.ld_os = mx_scale_row_bytes(N);
    g.M = M; g.N = N; g.K = K; g.ldo = N; g.m_valid = M;
    if (bm >= 256) {   // the persistent 256 x 256 kernel (gemm_fp8_p256.h); bm = 256 + v: only the first v rows are valid
        if (bm > 256) g.m_valid = bm - 256 < M ? bm - 256 : M;
        return launch_gemm256p8(reinterpret_cast<hipStream_t>(hip_stream), epi, g);
    }
    return launch_gemm8(reinterpret_cast<hipStream_t>(hip_stream), epi, bm, g);
}

extern "C" int mmiss_dbg_gemm8_time(int device, int epi, int bm, const void* A8, const void* As, const void* W8,
                                    const float* wscale, const float* bias, void* out, void* out_scale, int32_t M, int32_t N,
                                    int32_t K, int32_t iters, float* ms_per_launch) {
    if (!ms_per_launch || iters <= 0) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_gemm8_time: bad argument");
    MM_TRY(mmiss_use_device(device));
    auto run = [&]() -> int { return mmiss_dbg_gemm8(device, nullptr, epi, bm, A8, As, W8, wscale, bias, out, out_scale, M, N, K); };
    return time_launches(nullptr, iters, run, ms_per_launch);
}

// mmiss_debug.h: the path an encode call of this shape would take on the handle as it stands and under the options as they stand.
// Host arithmetic only: plan_layers and the functions run_layers / encode_image_chunk themselves decide by; no kernel is launched.
// Like an encode call it first makes sure the tower's workspaces exist (zero-filled): the plan reads which of them there are.
extern "C" int mmiss_dbg_encoder_plan(mmiss_encoder* enc, int32_t tower, int32_t B, int32_t T, int32_t* out) {
    if (!enc || !out) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_encoder_plan: null argument");
    if (tower != MMISS_TOWER_VISION && tower != MMISS_TOWER_TEXT) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_encoder_plan: unknown tower %d", tower);
    std::lock_guard<std::mutex> lk(enc->mu);
    if (!enc->finalized) MM_FAIL(MMISS_ERR_STATE, "mmiss_dbg_encoder_plan before mmiss_encoder_finalize");
    const bool text = tower == MMISS_TOWER_TEXT;
    Tower& tw = text ? enc->txt : enc->vis;
    const int maxb = text ? enc->cfg.max_batch_text : enc->cfg.max_batch_image;
    if (B < 1 || B > maxb) MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_encoder_plan: B = %d outside 1 .. max_batch = %d (one chunk of a call)", B, maxb);
    if (text ? (T < 1 || T > enc->cfg.t_ctx) : (T != 0 && T != tw.T))
        MM_FAIL(MMISS_ERR_ARG, "mmiss_dbg_encoder_plan: T = %d (text: 1 .. %d; vision: 0 or %d)", T, enc->cfg.t_ctx, enc->vis.T);
    for (int i = 0; i < 32; ++i) out[i] = 0;
    MM_TRY(mmiss_use_device(enc->device));
    MM_TRY(ensure_tower_ws(enc, tw, maxb, enc->cfg.proj_dim));
    const int savedT = tw.T;
    if (text) tw.T = T;   // as encode_text_chunk sets it
    LayerPlan P;
    const int rc = plan_layers(enc, tw, B, text, P);
    if (rc == MMISS_OK) {
        out[0] = P.fold; out[1] = P.fold_final; out[2] = P.fp8; out[3] = P.out8; out[4] = P.resid16;
        out[5] = P.sfold; out[6] = P.prune; out[7] = (int)P.embed;
        const GemmPick picks[4] = {P.qkv, P.out, P.fc1, P.fc2};
        for (int i = 0; i < 4; ++i) { out[8 + 2 * i] = (int)picks[i].kind; out[9 + 2 * i] = picks[i].bm; }
        out[16] = pooled_tail_planned(tw, P);
        out[17] = fc2_splitk_planned(tw, P.M);
        out[18] = P.M;
        out[23] = attention_pick_hpb(B, tw.heads);
        out[24] = attention_stream_ok(B, tw.T, tw.heads, text);
        if (!text) {
            const PatchPlan pp = plan_patch(enc, B);
            out[19] = lean_prelayernorm_planned(P);
            out[20] = (int)(pp.p160 ? GemmKind::P160 : GemmKind::Tile);
            out[21] = pp.p160 ? 160 : pp.bm;
            out[22] = pp.splitk;
        }
    }
    tw.T = savedT;
    return rc;
}

/*
 * mmiss.h — C-ABI of libmmiss.so, the MI355X (gfx950) embed-and-retrieve hot path.
 *
 * This is the drop-in boundary for ONE path of parsakhaz/multimodal-image-similarity-search:
 *   image / text -> CLIP tower -> L2-normalise -> cosine top-k over a flat in-HBM index.
 * The reference has no FFI of its own (it is pure Python over transformers + chromadb); each entry
 * point below names the reference call site whose arithmetic it replaces (paths relative to the
 * reference root; "HF:" = transformers/models/clip/).
 *
 * Conventions
 *   - plain C types only: pointers, sizes, opaque handles. No torch / HIP types in any signature.
 *   - every data pointer may be a HOST pointer or a DEVICE (HBM) pointer of the handle's GPU; the
 *     library detects which (hipPointerGetAttributes) and stages host data itself. Outputs likewise.
 *   - caller allocates every input and output buffer; the library owns only its handles and the HBM
 *     behind them (weights, index rows, workspaces). It never retains caller memory past a call.
 *   - every function returns an int status: 0 = MMISS_OK, <0 = error class; mmiss_last_error() returns
 *     a thread-local message. The Python shim turns non-zero into RuntimeError so the reference's
 *     `except Exception` paths (backend/app/main.py:803-805,825-827,865-867) behave the same.
 *   - a handle is internally serialised (one mutex + one HIP stream per handle); different handles are
 *     independent. Index mutation is safe against a concurrent query on the same handle.
 *   - there is NO CPU fallback anywhere in this library: with no usable gfx950 device every compute
 *     entry point fails with MMISS_ERR_HIP.
 */
#ifndef MMISS_H
#define MMISS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMISS_ABI_VERSION 1

enum {
    MMISS_OK = 0,
    MMISS_ERR_ARG = -1,         /* bad argument (null, shape, range)                 */
    MMISS_ERR_HIP = -2,         /* HIP runtime / device failure                      */
    MMISS_ERR_STATE = -3,       /* call order (e.g. encode before finalize)          */
    MMISS_ERR_NOMEM = -4,       /* host or device allocation failed                  */
    MMISS_ERR_UNSUPPORTED = -5, /* shape/dtype the kernels do not cover              */
    MMISS_ERR_IO = -6           /* file read/write failed (index save/load)          */
};

/* index storage dtypes. MMISS_F8: one byte per element, OCP e4m3 with the fixed scale 2^7 — a code stands for the value
 * decode(byte) / 128; a unit-norm row has |x_i| <= 1, so 128 x_i fits e4m3 and a typical component keeps its 3 mantissa
 * bits — plus ONE float per row, the inverse of the canonical norm of the row's values (+0.8 % bytes at dim 512; derived from
 * the codes, so save files do not hold it). The row the index REPRESENTS is values x inverse norm: a unit vector, so what an
 * fp8 index returns is a cosine distance, 1 - cos(query, represented row) (the reference turns it into
 * similarity = 1 - d / 2, backend/app/main.py:782, on that premise; round 4 returned 1 - |values| cos with |values| within
 * 3 % of 1). Distances are exact (canonical fp64, x the inverse norm) with respect to the represented rows, as for f16; the
 * represented rows themselves are 2^-4-coarse in every component: a row's direction lies within 1 - cos <= 4e-3 of the
 * vector that was added, so an fp8 index ranks like the f32 / f16 index up to that (a row is found first by its own
 * unquantised vector as long as its neighbours are further away than that; mmiss_index_get returns the represented rows).
 * Up to 128 queries per call take the streaming scan (half the bytes of f16 per row), from 129 on the score GEMM with the
 * codes widened to f16 in its operand load; both scale every score by the row's inverse norm. */
enum { MMISS_F32 = 0, MMISS_F16 = 1, MMISS_F8 = 2 };

typedef struct mmiss_encoder mmiss_encoder;
typedef struct mmiss_index mmiss_index;

/* ---------------------------------------------------------------- misc ------------------------- */
int mmiss_abi_version(void);
const char* mmiss_last_error(void);
/* number of visible HIP devices; does not create a context on any of them */
int mmiss_device_count(int* count);

/* ---------------------------------------------------------------- encoder ---------------------- */
/*
 * Shape-parametric CLIP (two towers + projections). Defaults of HF CLIPConfig() are ViT-B/32
 * (HF:configuration_clip.py:47-54,97-105,160). The reference HEAD loads a ViT-L/14 LongCLIP with
 * text_ctx = 248 (backend/app/utils.py:16-17,41-45); both are instances of this struct.
 * head_dim = hidden / heads must be 64; hidden (<= 1024) and mlp must be multiples of 128. A tower has at most
 * MMISS_MAX_TOKENS tokens: (v_image / v_patch)^2 + 1 and t_ctx — a 32 x 32 patch grid plus the class token, e.g. ViT-L/14 at
 * 448 px; ViT-L/14 at 336 px has 577. Up to 288 tokens the attention holds a head's keys in LDS, above it walks them in chunks.
 */
#define MMISS_MAX_TOKENS 1025

typedef struct mmiss_clip_config {
    int32_t struct_size;   /* = sizeof(mmiss_clip_config), ABI guard */
    int32_t v_hidden, v_layers, v_heads, v_mlp, v_patch, v_image; /* 768,12,12,3072,32,224 */
    int32_t t_hidden, t_layers, t_heads, t_mlp, t_vocab, t_ctx;   /* 512,12, 8,2048,49408,77 */
    int32_t proj_dim;      /* 512 */
    int32_t eos_token_id;  /* 49407; the legacy value 2 selects argmax(ids) pooling (HF:modeling_clip.py:561-581) */
    float ln_eps;          /* 1e-5 */
    int32_t max_batch_image; /* workspace sizing; larger batches are processed in chunks of this */
    int32_t max_batch_text;
} mmiss_clip_config;

/* replaces load_clip_model()'s model half — backend/app/utils.py:27-49 */
int mmiss_encoder_create(const mmiss_clip_config* cfg, int device, mmiss_encoder** out);
int mmiss_encoder_destroy(mmiss_encoder* enc);

/*
 * Weights arrive by their HF state_dict key (SURVEY.md §8 a-W), host float32, row-major, e.g.
 *   "vision_model.encoder.layers.3.self_attn.q_proj.weight"  [768,768]
 *   "text_model.embeddings.token_embedding.weight"            [49408,512]
 * Unknown keys ("logit_scale", "*.position_ids") are accepted and ignored (returns MMISS_OK and sets
 * *used = 0 when used != NULL). The library converts GEMM weights to bf16 and fuses q/k/v.
 * replaces CLIPModel.from_pretrained(...)'s tensor load — backend/app/utils.py:44
 */
int mmiss_encoder_set_weight(mmiss_encoder* enc, const char* hf_key, const float* data, int64_t numel, int* used);
/* checks that every tensor of both towers was supplied; must precede encode calls */
int mmiss_encoder_finalize(mmiss_encoder* enc);
/*
 * Arithmetic of the towers' large GEMMs. MMISS_PREC_BF16 (default): bf16 operands, f32 accumulation; in calls of at
 * least ~6000 token rows (hidden <= 768: LayerNorm folded into the GEMMs) the residual stream between the layers is
 * bf16 as well, as in any bf16 deployment of the model (measured 1 - cos vs the fp32 reference arithmetic: 5e-5; with an
 * f32 stream 5e-6). MMISS_PREC_BF16_F32RESID: bf16 operands, the residual stream f32 at every batch size (the round-1
 * behaviour; 4-5 % slower at 256 images). MMISS_PREC_FP8 (BASELINE.json configs[4] "ViT-L/14 fp8 MFMA encode"):
 * the QKV, FC1 and FC2 projections of the VISION tower run on the block-scaled fp8 matrix cores (OCP e4m3 operands, E8M0
 * block scales on the activations, per-output-channel scales on the weights, f32 accumulation) in calls of at least 1024
 * token rows — and, in calls on the bf16 residual stream (>= ~6000 token rows), the out-projection too, its A operand being
 * the attention kernel's MXFP8 output; the attention arithmetic, LayerNorm statistics and the projection head keep their
 * precision, and the residual stream is the same as under MMISS_PREC_BF16: bf16 in calls of at least ~6000 token rows, f32
 * below. Measured 1 - cos vs the fp32 reference arithmetic: 5e-4 at full ViT-L/14 depth, 6e-4 on ViT-B/32 at batch 256
 * (seeded Gaussian weights; asserted at 1e-3). A checkpoint with residual OUTLIER channels needs mmiss_encoder_calibrate (below)
 * to be covered by that bar. An e4m3 weight keeps three mantissa bits at any magnitude, so the weight column that meets a
 * channel of magnitude 300 carries a rounding error comparable to the signal of all ordinary channels: with +300 / -180
 * channels planted, an UNCALIBRATED handle measures 6.7e-4 on ViT-L/14 (width 1024) — inside — but 1.15e-3 on ViT-B/32
 * (width 768) — OUTSIDE the tolerance (tests/test_headline_gpu.py prints both; MMISS_PREC_BF16 holds 5e-5 on the same weights);
 * uncalibrated handles behave exactly as before. After mmiss_encoder_calibrate on a few dozen other images the constant part
 * of every LayerNorm output goes round the fp8 operands and the same ViT-B/32 weights are held to 1e-3
 * (tests/test_fp8_calibration_gpu.py asserts it and prints the figures; the CPU emulation tools/fp8_calib_sim.py gives
 * 1.25e-3 -> 6.2e-4, outliers on the CLS row only 7.8e-4 -> 7.3e-4, no outliers 6.4e-4 -> 6.6e-4; profiles/fp8_calibration.txt).
 * MMISS_PREC_FP8 stays an OPT-IN, to be verified per checkpoint against the default path (bench.py prints that gap); the
 * default is MMISS_PREC_BF16. The TEXT tower stays on the bf16
 * kernels under this setting: its fp8 form measures 3.3-3.9e-3, outside the 1e-3 tolerance (three mantissa bits put ~5 %
 * noise on every GEMM output and the text stream is built almost entirely from GEMM outputs).
 * mmiss_encoder_set_tower_precision switches ONE tower (MMISS_TOWER_VISION / MMISS_TOWER_TEXT) to MMISS_PREC_BF16 or
 * MMISS_PREC_FP8 explicitly; fp8 on the text tower is an opt-in outside the tolerance the other settings are held to.
 * Both may be called before or after finalize. The reference runs fp32 on the CPU (backend/app/utils.py:77,97); every
 * default setting is held to the same bar against it (1 - cos <= 1e-3, asserted in tests/test_fp8_gpu.py).
 */
enum { MMISS_PREC_BF16 = 0, MMISS_PREC_FP8 = 1, MMISS_PREC_BF16_F32RESID = 2 };
enum { MMISS_TOWER_VISION = 0, MMISS_TOWER_TEXT = 1 };
int mmiss_encoder_set_precision(mmiss_encoder* enc, int32_t precision);
int mmiss_encoder_set_tower_precision(mmiss_encoder* enc, int32_t tower, int32_t precision);
/*
 * Calibrated activation centring for MMISS_PREC_FP8 on the VISION tower (the outlier-channel regime above). The constant part
 * of a LayerNorm output does not have to pass through fp8:  LN(x) W^T + b = (LN(x) - mu) W^T + (b + W mu).
 * mmiss_encoder_calibrate runs ONE pass of the vision tower over `pixels` (f32 [B,3,S,S], host or device, as for
 * mmiss_encode_image; 1 <= B <= max_batch_image; after finalize) in the bf16 arithmetic whatever precision is set, on every
 * token row of every layer, and reduces the OUTPUT of each of the 2 * v_layers LayerNorm sites (LN1 -> QKV, LN2 -> FC1) over
 * all B * T rows to a per-channel mean and population variance (f64 sums in a fixed order). mu_c = mean_c where
 * mean_c^2 >= var_c — the channel's constant part is at least as large as its varying part — and 0 elsewhere (centring a channel
 * that is large on one token row only would hurt the other rows). From then on the fp8 QKV / FC1 of this handle run the same
 * LayerNorm -> MXFP8 and GEMM kernels on beta' = beta - mu and b' = b + W_bf16 mu (f32, fixed order): the same launches, no
 * kernel changed. Explicit, one-shot, deterministic: the same weights, pixels and B give the same bits. Use images that look
 * like the ones to be encoded; 16-64 are enough (the statistics are over B * T rows).
 * The stored calibration: cleared by mmiss_encoder_calibration_clear, by any mmiss_encoder_set_weight of a vision-tower tensor
 * and by mmiss_encoder_finalize; no effect on the text tower, on the bf16 settings, or on calls below the fp8 row threshold
 * (they run the bf16 kernels).
 * Errors (MMISS_ERR_ARG, with a message): a call before finalize, B outside 1 .. max_batch_image, a null pointer, a table of
 * the wrong length.
 *   _info   out[0] = sites (2 * v_layers; 0 when uncalibrated), out[1] = v_hidden, out[2] = centred channels over all sites,
 *           out[3] = rows seen (B * T; 0 for a table installed with _set)
 *   _get    the mu table, f32 [2 * v_layers, v_hidden], site order layer 0 LN1, layer 0 LN2, layer 1 LN1, ...; *written = floats
 *           copied (0 when uncalibrated); cap smaller than the table -> MMISS_ERR_ARG
 *   _set    installs a table (n = 2 * v_layers * v_hidden) and derives beta' / b' from it with the same kernels: a server
 *           calibrates once, stores the table and restores it at start — bit-identical embeddings.
 * No reference analogue (the reference runs fp32 on the CPU, backend/app/utils.py:77).
 */
int mmiss_encoder_calibrate(mmiss_encoder* enc, const float* pixels, int32_t B);
int mmiss_encoder_calibration_clear(mmiss_encoder* enc);
int mmiss_encoder_calibration_info(mmiss_encoder* enc, int64_t out[4]);
int mmiss_encoder_calibration_get(mmiss_encoder* enc, float* mu, int64_t cap, int64_t* written);
int mmiss_encoder_calibration_set(mmiss_encoder* enc, const float* mu, int64_t n);
/*
 * use_own != 0 (the default after create): calls run on the handle's private stream and return after the
 * work has finished (host-synchronous). use_own == 0: calls are enqueued on the caller's hipStream_t
 * (passed as void*; NULL = the legacy default stream) and return without synchronising unless an
 * input or output lives in host memory. Changing the stream waits for the work the handle's LAST call left on the
 * stream being left (its workspaces are reused), not for anything else the caller has queued there since.
 * The same rule holds for every call that writes state a queued encode may still read: mmiss_encoder_set_weight,
 * mmiss_encoder_finalize, mmiss_encoder_calibrate, mmiss_encoder_calibration_set / _clear (and the debug tap switch where
 * it forces the workspaces to be reallocated) first wait, on the host, for the handle's last call that returned with work
 * queued on a caller's stream — for that call's work and for nothing else on the caller's stream. A call queued before
 * such a change computes with the state it was queued under. (mmiss_encoder_set_precision / _set_tower_precision drain
 * the handle's current stream.)
 * Threads: every call locks its handle, but the stream is handle state — a thread that sets the stream and then calls
 * must keep other threads off that handle in between (the Python wrappers hold a per-handle lock around the pair);
 * different handles never interact (several batches in flight: one encoder handle per host thread / stream,
 * mmiss_amd/pipeline.py).
 */
int mmiss_encoder_set_stream(mmiss_encoder* enc, void* hip_stream, int32_t use_own);

/*
 * pixels: float32 [B,3,S,S] NCHW, already CLIP-normalised (the output of CLIPImageProcessor,
 *         HF:image_processing_clip.py:23-34). out: float32 [B,proj_dim], rows unit-norm.
 * replaces model.get_image_features(**inputs) + "/ norm" — backend/app/utils.py:77-78
 *          (HF:modeling_clip.py:719-753,613-656)
 */
int mmiss_encode_image(mmiss_encoder* enc, const float* pixels, int32_t B, float* out);

/*
 * pixels_u8: uint8 [B,S,S,3] HWC RGB, already resized+centre-cropped to SxS; the kernel applies
 * x/255, (x-mean)/std (HF:image_processing_clip.py:23-34; mean/std transformers/utils/constants.py:5-6)
 * in the patchify prologue. Same output as mmiss_encode_image.
 */
int mmiss_encode_image_u8(mmiss_encoder* enc, const uint8_t* pixels_u8, int32_t B, float* out);

/*
 * Raw decoded images of ANY size (what PIL hands the processor at backend/app/utils.py:76): B tightly packed RGB8
 * images (row stride 3*W, no padding) laid end to end in `rgb` (host or device, rgb_bytes long); image b starts at
 * byte offsets[b] and is heights[b] x widths[b] (host arrays). The library does the CLIPImageProcessor geometry on
 * the GPU — resize so the shortest edge is S = v_image with PIL's bicubic filter (long edge int(S*long/short)),
 * centre crop S x S (HF:image_processing_clip.py:23-34) — bit-identical to Pillow's 8-bit Image.resize, then
 * rescale/normalise/encode as mmiss_encode_image_u8. JPEG/PNG decoding and convert("RGB") stay with the caller.
 *   mmiss_resize_crop_rgb   out_u8: uint8 [B,S,S,3] (host or device) — the crops themselves;
 *   mmiss_encode_image_rgb  out: float32 [B,proj_dim] unit rows.
 * Errors: sizes outside 1..65536, bytes outside the blob -> MMISS_ERR_ARG; a downscale needing more than 4096 filter
 * taps per output pixel -> MMISS_ERR_UNSUPPORTED.
 */
int mmiss_resize_crop_rgb(mmiss_encoder* enc, const uint8_t* rgb, int64_t rgb_bytes, const int64_t* offsets,
                          const int32_t* heights, const int32_t* widths, int32_t B, uint8_t* out_u8);
int mmiss_encode_image_rgb(mmiss_encoder* enc, const uint8_t* rgb, int64_t rgb_bytes, const int64_t* offsets,
                           const int32_t* heights, const int32_t* widths, int32_t B, float* out);

/*
 * ids: int32 [B,T], T <= t_ctx, rows = BOS ... EOS then padding (CLIPTokenizer output,
 *      backend/app/utils.py:88). out: float32 [B,proj_dim], rows unit-norm. The pooled row is the
 *      first EOS position, so the padding mask cannot change the result (causal attention).
 * replaces model.get_text_features(**inputs) + "/ norm" — backend/app/utils.py:97-98
 *          (HF:modeling_clip.py:683-715,513-586)
 */
int mmiss_encode_text(mmiss_encoder* enc, const int32_t* ids, int32_t B, int32_t T, float* out);

/*
 * Debug tap used by the parity tests to bisect against the oracle's intermediates.
 * tower: 0 = vision, 1 = text. what: 0 = embeddings (after pre-LN for vision), 1..L = residual
 * stream after layer i, 100 = pooled+post-LN row (bf16 widened), 101 = projected (pre-normalise).
 * Copies min(cap, available) floats of the LAST encode call's buffer; *written gets the count.
 */
int mmiss_encoder_tap(mmiss_encoder* enc, int tower, int what, float* out, int64_t cap, int64_t* written);

/* ---------------------------------------------------------------- flat index ------------------- */
/*
 * Flat cosine index resident in HBM: rows are L2-normalised at add time and stored as f32, f16 or fp8 (e4m3).
 * dim: a multiple of 128; f32 rows up to 1920, f16 / fp8 rows up to 3968 (the scan stages a 16-query block beside its
 * lists in one CU's 160 KB of LDS) — anything else is MMISS_ERR_UNSUPPORTED here, not a failed launch at the first query.
 * replaces chromadb's collection with metadata {"hnsw:space":"cosine"} — backend/app/utils.py:104-137
 */
int mmiss_index_create(int32_t dim, int32_t storage_dtype, int device, int64_t capacity_hint, mmiss_index** out);
int mmiss_index_destroy(mmiss_index* idx);
/* same contract as mmiss_encoder_set_stream */
int mmiss_index_set_stream(mmiss_index* idx, void* hip_stream, int32_t use_own);

/*
 * vecs: float32 [n,dim] (any norm > 0). labels: int64 [n], strictly increasing and greater than every
 * label already stored (they are the tie-break order; the Collection shim hands out sequence numbers).
 * replaces collection.add(ids, embeddings, ...) — backend/app/main.py:735-740
 */
int mmiss_index_add(mmiss_index* idx, const float* vecs, const int64_t* labels, int64_t n);
/* overwrite the rows of existing labels (labels: host int64 [n]) — collection.update(..., embeddings=) */
int mmiss_index_update(mmiss_index* idx, const int64_t* labels, const float* vecs, int64_t n);
/* stable removal (row order = label order is preserved). labels: host. — collection.delete(ids), main.py:1069 */
int mmiss_index_remove(mmiss_index* idx, const int64_t* labels, int64_t n, int64_t* removed);
int mmiss_index_clear(mmiss_index* idx);
/* collection.count() — init_db.py:58 */
int mmiss_index_count(mmiss_index* idx, int64_t* count);
/* stored (normalised, storage-rounded) rows widened to f32 [n,dim]; labels: host. Missing label -> MMISS_ERR_ARG */
int mmiss_index_get(mmiss_index* idx, const int64_t* labels, int64_t n, float* out);
/* all labels in row order (host int64 [count]) */
int mmiss_index_labels(mmiss_index* idx, int64_t* out, int64_t cap);

/*
 * queries: float32 [Q,dim] (any norm > 0; normalised internally). k >= 1.
 * out_labels int64 [Q,k], out_dist float32 [Q,k] = cosine distance 1 - cos, ascending; ties by label
 * ascending. out_count int32 [Q] = min(k, count); unused slots hold label -1 / distance +inf.
 * k larger than count is not an error (the UI's "All" sends 1000 — backend/app/main.py:757).
 * A vector without a direction — zero norm, or a NaN / Inf component: 0/0 in the normalisation — has no distance to
 * anything: such a ROW is stored but never returned (out_count then counts the rows that have a distance), such a QUERY has
 * no results (out_count 0). Not an error; the reference never sends one (backend/app/utils.py:88-99 always hands chromadb a
 * CLIP embedding). tests/test_index_gpu.py: test_zero_and_non_finite_vectors_are_never_results, all three storage types.
 * Synchronisation: the exactness guard (below) decides on the host whether any query must be widened (the last kernel
 * leaves one flag per query in a pinned host block; no copy-engine operation), so the call waits for its own work on the
 * stream it runs on — also on a caller's stream with device outputs (mmiss_index_set_stream(.., use_own = 0)), and it
 * cannot be captured into a HIP graph (the encode calls can). mmiss_index_query_begin / _end split that wait off.
 * replaces collection.query(query_embeddings, n_results, include=["metadatas","distances"]) —
 *          backend/app/main.py:761-765
 */
int mmiss_index_query(mmiss_index* idx, const float* queries, int32_t Q, int32_t k,
                      int64_t* out_labels, float* out_dist, int32_t* out_count);
/*
 * The same query in two halves, for a caller that keeps the GPU fed while it waits (a serving loop: queue the NEXT batch's
 * encode between the two calls, bench.py does). _begin queues the first pass on the index's stream and returns without
 * waiting; _end waits for exactly that work (an event, not the stream: whatever the caller queued behind it keeps running),
 * runs the guard's widen pass for the queries that need it, and fills host outputs. mmiss_index_query = _begin + _end.
 * Streams: the first pass is ordered on the index's stream; the widen pass that _end decides on runs on a second stream of
 * the handle's, so it may run BESIDE the work the caller queued on the index's stream between the two calls (the first pass is
 * ahead of that work, by stream order). `queries` may be overwritten by work queued there behind _begin. The results — host
 * or device outputs — are complete when _end returns, for work on any stream queued after that; until then the output buffers
 * hold nothing defined. _end waits for the query's own work only: it does not wait for the caller's stream, and the caller's
 * stream never waits for the widen pass.
 * Between the two calls `queries` and the output buffers must stay valid, and every other call on this index except
 * count / labels / guard_stats fails with MMISS_ERR_STATE (the scratch buffers belong to the open query); _end without
 * _begin -> MMISS_ERR_STATE. No reference analogue: collection.query is synchronous (backend/app/main.py:761-765).
 */
int mmiss_index_query_begin(mmiss_index* idx, const float* queries, int32_t Q, int32_t k,
                            int64_t* out_labels, float* out_dist, int32_t* out_count);
int mmiss_index_query_end(mmiss_index* idx);
/*
 * Give up a query opened with _begin (the caller lost interest: an exception in the serving loop between the two halves):
 * waits for the queued first pass — it still writes the output buffers, which must stay valid until this returns — and
 * re-opens the handle for other calls. No results are delivered. Without an open query: MMISS_OK, nothing happens.
 */
int mmiss_index_query_abort(mmiss_index* idx);
/*
 * Exactness accounting since the index was created ("top-10 recall = 1.0" is proven per query, not assumed): the first
 * pass ranks by approximate matrix-core scores and keeps k' > k rows; a query whose k-th exact score c_k does not clear the
 * best score that pass may have left out by more than the arithmetic's error bound eps_q is widened: ONE threshold pass
 * over the index for all such queries of the call collects every row whose approximate score reaches c_k - eps_q (every
 * row that can still belong to the top-k), and the exact re-rank of those rows is the answer.
 * out[0] = queries served, out[1] = queries widened, out[2] = widen passes run (one per call that had to widen),
 * out[3] = extra passes over the index those cost (1 per widen pass on the score GEMM, one per 64 widened queries on the
 * streaming scan). No reference analogue (chromadb's HNSW is approximate above 100 rows).
 */
int mmiss_index_guard_stats(mmiss_index* idx, int64_t out[4]);
/*
 * The same four counters and: out[4] = the queries whose threshold pass collected more than 8192 rows and went through the
 * exhaustive canonical pass instead (the canonical distance of every row, the k best by (distance, label)) — a plateau of
 * rows within the rounding bound of the k-th score, e.g. > 10^4 copies of one placeholder image; exact for any data, one
 * pass over the index and one host selection per such query. out[5] = rows the threshold passes collected and re-ranked.
 * out[6] = queries served by the radius calls (below), out[7] = passes over the index those cost (1 per chunk on the score GEMM,
 * one per 64 queries of a chunk on the streaming scan). Radius calls leave out[0..3] alone and add to out[4] and out[5].
 * The membership / tagging calls (below) count like radius calls: out[6] += their probes, out[7] += their passes over the index,
 * out[5] += the (row, probe) pairs they resolved canonically, out[4] += the probes that took the per-probe canonical route.
 * mmiss_index_assign counts the same way: out[6] += its centres, out[7] += its passes, out[5] += borderline rows x centres with
 * a direction (the one distance per decided row is not counted); out[0..4] stay untouched.
 */
int mmiss_index_guard_stats_ex(mmiss_index* idx, int64_t out[8]);

/*
 * persistence of rows + labels (replaces chroma_data/, backend/app/utils.py:21,113). The file format (version 1) holds no
 * tags: save does not write them and load resets every row's tag to 0 (a caller that filters re-derives them from its own
 * metadata and sets them again, as the Python collection does).
 */
int mmiss_index_save(mmiss_index* idx, const char* path);
int mmiss_index_load(mmiss_index* idx, const char* path);

/* ---------------------------------------------------------------- filtered queries ------------- */
/*
 * Every row carries a 64-bit TAG word (0 when added; update keeps it; stable removal keeps the survivors'; clear and load
 * reset it). A filtered query gives each query q two masks and admits row r iff
 *     (tags[r] & require[q]) == require[q]  &&  (tags[r] & exclude[q]) == 0
 * and returns the exact top-k AMONG ADMITTED ROWS: ids and distances bit-identical to an unfiltered query of an index that
 * holds only the rows q admits, (distance, label) order, out_count[q] = min(k, admitted rows of q that have a direction),
 * unused slots label -1 / distance +inf. Every pass of a filtered query (first pass, widen pass, exhaustive pass) is the
 * streaming scan, which does not read rows that no query of its block admits; the score GEMM of unfiltered batches is not used.
 * replaces the reference's POST-filter: collection.query(n_results=limit) and then dropping the hits whose
 * filter_results_json answers are not all "yes" (backend/app/main.py:202-222, 258-278, 320-340), which returns fewer than
 * `limit` results whenever the filter rejects some of the nearest rows.
 */
/* labels: int64 [n], tags: uint64 [n] (host or device). A label not in the index -> MMISS_ERR_ARG and nothing is changed. */
int mmiss_index_set_tags(mmiss_index* idx, const int64_t* labels, const uint64_t* tags, int64_t n);
/* out: uint64 [n] (host or device), the tags of `labels`; a label not in the index -> MMISS_ERR_ARG */
int mmiss_index_get_tags(mmiss_index* idx, const int64_t* labels, int64_t n, uint64_t* out);
/*
 * As mmiss_index_query, with require / exclude: uint64 [Q] each, host or device memory, null = 0 for every query. Both
 * null: exactly mmiss_index_query (same path, same results). The exactness guard works on the admitted rows (its bound is
 * the k'-th approximate score among them; the widen pass collects admitted rows only; the exhaustive pass selects among
 * them) and counts in the guard statistics like any query.
 */
int mmiss_index_query_filtered(mmiss_index* idx, const float* queries, int32_t Q, int32_t k,
                               const uint64_t* require, const uint64_t* exclude,
                               int64_t* out_labels, float* out_dist, int32_t* out_count);
/* first half of mmiss_index_query_filtered; ended by mmiss_index_query_end or dropped by mmiss_index_query_abort. The
 * masks are read before it returns. */
int mmiss_index_query_filtered_begin(mmiss_index* idx, const float* queries, int32_t Q, int32_t k,
                                     const uint64_t* require, const uint64_t* exclude,
                                     int64_t* out_labels, float* out_dist, int32_t* out_count);

/* ---------------------------------------------------------------- radius queries --------------- */
/*
 * "Every row at least this similar", exactly. Row r is a MEMBER of query q iff the row has a direction, q admits it (require /
 * exclude as for mmiss_index_query_filtered; null = 0) and d(q, r) <= max_dist[q], compared as floats, d being the canonical
 * distance mmiss_index_query returns: (float)(1.0 - canon_dot(q^, row) [x (double)inv[row] for fp8 rows]). No special radii: a
 * negative one is legal (a distance can be a few ulps below 0), one >= 2 admits every row; a NaN radius is MMISS_ERR_ARG.
 *   out_total[q] (int64 [Q], may be null) = the exact number of members; out_count[q] (int32 [Q]) = min(cap, out_total[q]);
 *   out_labels / out_dist ([Q, cap], 1 <= cap <= 4096) hold the out_count[q] nearest members in (distance, label) order, unused
 *   slots label -1 / distance +inf. A query without a direction: count 0, total 0. An empty index: 0 everywhere.
 * max_dist: float32 [Q], host or device, as the masks. Outputs all host or all device. The call locks the handle, runs on its
 * current stream, returns with its work finished, and fails with MMISS_ERR_STATE while a _begin query is open; it has no
 * _begin / _end form. Any Q: the work is done in chunks of at most 1024 queries.
 * One pass over the index instead of a top-k query's one or two: the exactness guard's threshold pass with the threshold taken
 * from the radius, thr_q = (1 - max_dist[q]) - eps_q (no member's approximate score lies below it), then the canonical re-rank
 * of what it collected, cut at the radius. A query that collects more than 8192 rows goes through the exhaustive canonical pass
 * (one pass over the index and one host selection per such query), as a plateau does under mmiss_index_query.
 * replaces the caller-side "pick a k, hope it is large enough, cut the list": the UI's "All" = 1000
 * (backend/app/main.py:757) and similarity = 1 - d / 2 (main.py:782); the reference's roadmap names the missing piece,
 * "Adjustable similarity thresholds" (CHANGELOG.md:475).
 */
int mmiss_index_query_radius(mmiss_index* idx, const float* queries, int32_t Q, const float* max_dist, int32_t cap,
                             const uint64_t* require, const uint64_t* exclude,
                             int64_t* out_labels, float* out_dist, int32_t* out_count, int64_t* out_total);
/*
 * The same, the queries being the rows the index REPRESENTS under `labels` (host int64 [n]; one radius for all): the stored rows
 * are widened to f32 on the device (fp8 rows x their inverse norm) and handed to the same core — nothing crosses PCIe — which
 * gives exactly what mmiss_index_query_radius returns for the output of mmiss_index_get(labels). later_only != 0 admits only
 * rows whose label is GREATER than the query's own: row order is label order, so the self match is dropped and every pair of a
 * near-duplicate search over all labels is reported once, with the smaller label as the query. A label not in the index ->
 * MMISS_ERR_ARG and nothing is written.
 * replaces nothing the reference can do: its "Duplicate Detection" (README.md:21) is an exact perceptual hash
 * (backend/app/main.py:628-640), so a re-encoded, resized or lightly cropped copy is stored again; its CLIP embedding sits at
 * cosine 0.99 to the original's.
 */
int mmiss_index_query_radius_by_label(mmiss_index* idx, const int64_t* labels, int64_t n, float max_dist, int32_t cap,
                                      int32_t later_only, int64_t* out_labels, float* out_dist, int32_t* out_count,
                                      int64_t* out_total);

/* ---------------------------------------------------------------- membership / tagging --------- */
/*
 * The DENSE form of the radius question: for P probes (1 <= P <= 64; probe p = query vector queries[p] and radius max_dist[p])
 * the exact membership of EVERY row, one bit per (row, probe), in one streaming pass over the index per 16 / 32 / 64 probes
 * (as many as fit the LDS at the index's dim and dtype). Row r is a member of probe p iff the row has a direction, the probe's
 * query has a direction, and d(q_p, r) <= max_dist[p] compared as floats — the member definition of mmiss_index_query_radius
 * (no masks), so for any cap large enough the member set IS the label set that call reports. No special radii: a negative one
 * is legal, one >= 2 admits every row that has a direction; a NaN radius is MMISS_ERR_ARG. There is no cap on the members: the
 * answer is a bit per row, not a list.
 * queries: float32 [P, dim]; max_dist: float32 [P]; out_members: int64 [P], may be null, the exact member count per probe. Each
 * of them host or device memory, independently.
 * Exact: approximate matrix-core scores decide the pairs whose score clears (1 - R_p) + eps_p (member) or stays below
 * (1 - R_p) - eps_p (no member), eps_p being the exactness guard's bound; the borderline pairs in between are re-scored in the
 * canonical arithmetic; a probe with more than 8192 borderline rows (mass duplicates at exactly its radius) gets the canonical
 * distance of every row, on the device.
 * Both calls lock the handle, run on its current stream, return with their work finished, fail with MMISS_ERR_STATE while a
 * _begin query is open, check every argument before they write anything, and on an empty index write nothing but zeros to
 * out_members. Accounting (mmiss_index_guard_stats_ex): out[6] += P, out[7] += passes over the index, out[5] += the (row,
 * probe) pairs resolved canonically (every row of a probe that took the per-probe canonical route), out[4] += the probes that
 * took that route; out[0..3] stay untouched, as for radius calls.
 * replaces the reference's filter pass over the whole collection — add_filter -> process_filter_on_all_images
 * (backend/app/main.py:939-1056) asks a yes/no model about every stored image and stores the answers the searches filter on
 * (main.py:202-222) — for the question CLIP itself answers: "is this image within distance R of this text / image embedding".
 *
 * mmiss_index_membership: out_words uint64 [count] (host or device) in row order — the order of mmiss_index_labels —, bit p of
 * out_words[r] = row r is a member of probe p, bits >= P zero. cap_rows = the rows out_words has room for; cap_rows < count is
 * MMISS_ERR_ARG. Read-only on the index.
 */
int mmiss_index_membership(mmiss_index* idx, const float* queries, int32_t P, const float* max_dist, uint64_t* out_words,
                           int64_t cap_rows, int64_t* out_members);
/*
 * mmiss_index_tag_by_radius: the memberships written straight into the rows' tag words. bits: HOST int32 [P], distinct, each in
 * 0 .. 63 (otherwise MMISS_ERR_ARG); with M = the OR of 1 << bits[p], every row's tag becomes
 *     tags[r] = (tags[r] & ~M) | sum over p of member(r, p) << bits[p]
 * — the named bits are overwritten (set or cleared), every other bit keeps its value. The host copy of the tags that
 * mmiss_index_get_tags, mmiss_index_remove and the exhaustive passes read is up to date when the call returns.
 */
int mmiss_index_tag_by_radius(mmiss_index* idx, const float* queries, int32_t P, const float* max_dist, const int32_t* bits,
                              int64_t* out_members);

/* ---------------------------------------------------------------- assignment / clustering ------ */
/*
 * The TRANSPOSED question of a query: for EVERY stored row, which of C given vectors is nearest? — zero-shot classification of
 * the collection against C prompt embeddings, and the assignment step of spherical k-means.
 * centres: float32 [C, dim], 1 <= C <= 1024, any norm (normalised as queries are). out_assign: int32 [count] in row order — the
 * order of mmiss_index_labels —; out_dist: float32 [count], may be null; out_sizes: int64 [C], may be null. Each of them host or
 * device memory, independently. cap_rows = the rows out_assign (and out_dist) have room for; cap_rows < count is MMISS_ERR_ARG.
 * With Dm[c][r] = the canonical distance of centre c and row r (the bits mmiss_index_query returns for query c and row r):
 *   out_assign[r] = the c that minimises (Dm[c][r], c) over the c whose Dm[c][r] is not NaN — ties in the float distance go to
 *   the smaller centre index —, out_dist[r] = that distance; a row without a direction gets -1 / +inf, as does every row when
 *   no centre has a direction; a centre without a direction is never chosen. out_sizes[c] = the rows assigned to c.
 * Exact: one streaming pass over the index per 16 / 32 / 64 centres (the membership call's tile choice) keeps the two largest
 * approximate matrix-core scores of every row; a row whose best score leads the second by more than twice the exactness
 * guard's bound is decided (its one canonical distance is computed only when out_dist is asked for), every other row gets the
 * canonical distance to every centre. On well-separated centres the second kind is rare; with duplicate centres it is every row.
 * Locks the handle, runs on its current stream, returns with its work finished, fails with MMISS_ERR_STATE while a _begin
 * query is open, checks every argument before it writes anything, and on an empty index writes nothing but zeros to
 * out_sizes. Read-only on the index. Accounting (mmiss_index_guard_stats_ex): out[6] += C, out[7] += passes over the index,
 * out[5] += borderline rows x centres with a direction; out[0..4] stay untouched.
 * (The reference has no counterpart: its collection can only be queried, one embedding at a time — backend/app/main.py:760-867.)
 */
int mmiss_index_assign(mmiss_index* idx, const float* centres, int32_t C, int32_t* out_assign, float* out_dist, int64_t cap_rows,
                       int64_t* out_sizes);
/*
 * The reduction a k-means update needs: per cluster, the sum of its rows — in a fixed-point form that has exactly one value,
 * whatever order the hardware adds in. assign: int32 [n] (host or device), n == count (otherwise MMISS_ERR_ARG), entries outside
 * 0 .. C-1 (mmiss_index_assign's -1) are skipped; 1 <= C <= 1024; out_sums: int64 [C, dim]; out_sizes: int64 [C], may be null,
 * the rows per cluster (host or device each). With x = the float32 value mmiss_index_get returns for an element,
 *   out_sums[c][j] = sum over the rows r with assign[r] == c of (int64) rint((double) x[r][j] * 2^32)
 * (round to nearest even; the product is exact); a cluster's mean direction is (double) out_sums[c] * 2^-32, up to its norm.
 * One pass over the rows. Same locking, stream and state rules as mmiss_index_assign; read-only on the index; no accounting.
 */
int mmiss_index_cluster_sums(mmiss_index* idx, const int32_t* assign, int64_t n, int32_t C, int64_t* out_sums, int64_t* out_sizes);

/* ---------------------------------------------------------------- partitioned search ----------- */
/*
 * An inverted-file search over the centres and cells the assignment calls produce: a query reads only the rows of the few cells
 * whose centres are nearest to it instead of every row. The approximation is ONLY in which rows are looked at, and that set is
 * defined exactly; within it the answer is the exact top-k — the distance bits and the (distance, label) order of
 * mmiss_index_query — so probing every cell returns mmiss_index_query's bits. The reference's own store answers above 100 rows
 * from an approximate HNSW graph (chromadb: backend/app/utils.py:127-130 create, backend/app/main.py:761-765 query).
 *
 * A PARTITION is C centres (1 <= C <= 1024, float32 [C, dim], any norm) and one cell number per row for the B rows the index held
 * when it was set (int32; an entry outside 0 .. C-1, e.g. mmiss_index_assign's -1, puts the row in no cell). Rows added since
 * (r >= B) are the TAIL. For a query q and nprobe >= 1:
 *   dc[c]   = the canonical distance of the normalised query to the normalised centre c treated as an f32 row (the bits
 *             mmiss_index_query reports for q against an f32 row holding the centre);
 *   P(q)    = the min(nprobe, live centres) centres smallest by (dc[c], c) among the c whose dc[c] is not NaN — ties to the
 *             smaller index; a centre without a direction is never probed;
 *   cand(q) = { r < B : cells[r] in P(q) } and every tail row.
 * The result is the exact top-k by (distance, label) over the rows of cand(q) that the masks admit (require / exclude as
 * mmiss_index_query_filtered, null = 0) and that have a distance; out_count = min(k, those rows), unused slots -1 / +inf; a
 * query without a direction gives count 0. out_scanned[q] = the sizes of the cells of P(q) + the tail rows, independent of the
 * masks, 0 for a query without a direction. A row in an unprobed cell is NOT returned however near it is.
 * mmiss_index_add keeps the partition (new rows are tail, candidates of every query); mmiss_index_update, _remove, _clear and
 * _load drop it (rows move or change: a stale cell would silently lose results); mmiss_index_save does not persist it.
 *
 * All five calls lock the handle, run on its current stream, return with their work finished, fail with MMISS_ERR_STATE while
 * a _begin query is open, check every argument before they write anything, and leave the eight guard counters alone.
 *
 * mmiss_index_partition_set: centres and cells each host or device memory; n must equal the row count. n != count, C outside
 * 1 .. 1024, a null pointer or no centre with a direction -> MMISS_ERR_ARG, and the previous partition is kept. Stores the
 * canonically normalised centres, the cells, the row numbers grouped by cell (a counting sort on the device; the order inside a
 * cell is unspecified and no result depends on it), the cell offsets and the sizes.
 */
int mmiss_index_partition_set(mmiss_index* idx, const float* centres, int32_t C, const int32_t* cells, int64_t n);
/* Forget the partition; none set: MMISS_OK, nothing happens. */
int mmiss_index_partition_clear(mmiss_index* idx);
/*
 * out = { C (0 = no partition, and then every other entry is 0), B, tail rows, rows in cells, largest cell, empty cells,
 *         probed queries served since the partition was set, rows scanned since (the sum of their out_scanned) }.
 */
int mmiss_index_partition_info(mmiss_index* idx, int64_t out[8]);
/*
 * The partition as stored: the NORMALISED centres float32 [C, dim], cells int32 [B], sizes int64 [C]; each may be null, each host
 * or device memory. cap_rows = the entries `cells` has room for; cap_rows < B -> MMISS_ERR_ARG. No partition -> MMISS_ERR_STATE.
 */
int mmiss_index_partition_get(mmiss_index* idx, float* centres, int32_t* cells, int64_t cap_rows, int64_t* sizes);
/*
 * The probed query defined above. queries float32 [Q, dim] (host or device), Q >= 1; 1 <= k <= 2040 (above: MMISS_ERR_UNSUPPORTED,
 * the flat query's own limit); nprobe >= 1, values above C are legal (every live centre is probed); require / exclude uint64 [Q],
 * host or device, each may be null; out_labels int64 [Q, k], out_dist float32 [Q, k], out_count int32 [Q], out_scanned int64 [Q]
 * (may be null): all host or all device. No partition -> MMISS_ERR_STATE. On an empty index with a partition: counts 0.
 * Every candidate gets its canonical distance directly (no approximate pass, no guard); the scratch of a call is bounded by the
 * tail and the nprobe largest cells per query, and the queries are taken in chunks that keep it under 512 MB.
 */
int mmiss_index_query_probed(mmiss_index* idx, const float* queries, int32_t Q, int32_t k, int32_t nprobe, const uint64_t* require,
                             const uint64_t* exclude, int64_t* out_labels, float* out_dist, int32_t* out_count, int64_t* out_scanned);

/* ---------------------------------------------------------------- distinct results ------------- */
/*
 * Top-k with near-duplicates of kept hits suppressed, on the device: ten DIFFERENT images instead of ten copies of one (a burst of
 * shots, re-encodes of one picture). The reference has no counterpart: its duplicate check is an exact perceptual hash at upload
 * (backend/app/main.py:628-640) and its searches return collection.query's list as it comes (main.py:761-782).
 *
 * For a query q:
 *   L(q)      = the list mmiss_index_query_filtered(q, k = pool, require, exclude) returns — labels and distance bits in
 *               (distance, label) order, length m = its out_count; with nprobe >= 1 the list of
 *               mmiss_index_query_probed(q, pool, nprobe, ...) instead (no partition: MMISS_ERR_STATE, as there).
 *   sep(s, i) = the float distance mmiss_index_query_radius_by_label defines with label L[s] as the query and the row of L[i]
 *               as the row: the query is the REPRESENTED row of L[s] (fp8 rows: values x inverse norm, one float multiply),
 *               normalised again as every query is. sep is NOT symmetric on f16 and fp8 rows; the direction is "the kept row
 *               is the query". An exact copy sits at whatever distance the flat query reports for it (about 6e-5 on f16 rows),
 *               not at 0.
 *   the walk  = positions 0 .. m-1 in order. Position i is SUPPRESSED when an earlier KEPT position s has sep(s, i) <= min_sep
 *               (compared as floats) and is then OWNED by the smallest such s; otherwise it is kept while fewer than k
 *               positions are kept; positions that are neither, behind the k-th kept one, are left over and ignored. Every kept
 *               position, the k-th included, suppresses over all of L.
 * out_labels / out_dist [Q, k]: the kept entries with L's own distance bits, unused slots -1 / +inf; out_count[q]: the kept
 * entries; out_dups [Q, k] (may be null): the entries of L each kept entry owns ("+12 similar"), unused slots 0; out_listed [Q]
 * (may be null): m. The outputs are all host or all device memory; queries and masks host or device as in the other calls.
 *
 * Consequences:
 *   the walk is prefix-stable: the kept labels for pool p are a prefix of those for any pool > p. So whenever out_count == k the
 *   labels and distances are those of the walk over the ENTIRE ranking, independent of pool; only out_dups depends on pool;
 *   out_count < k && out_listed == pool means the pool ran out and should be raised;
 *   a min_sep below every sep (e.g. -1) gives the first k of L bit for bit with dups 0; min_sep >= 4 keeps only the first entry,
 *   with dups[0] = m - 1.
 *
 * Arguments: 1 <= k <= pool (k > pool, k < 1: MMISS_ERR_ARG), pool <= 2040 (above: MMISS_ERR_UNSUPPORTED, the list calls' own
 * limit); a NaN min_sep is MMISS_ERR_ARG, a negative one is legal; nprobe < 0 is MMISS_ERR_ARG, nprobe == 0 the flat / filtered
 * list. A query without a direction gives count 0 and listed 0; an empty index gives zeros.
 * The call locks the handle, runs on its current stream, returns with its work finished, fails with MMISS_ERR_STATE while a
 * _begin query is open, and checks every argument before it writes anything. The list stage is the restated call's own code and
 * counts in the guard (or partition) counters exactly as that call; the suppression stage — one kernel launch for all queries,
 * every comparison a canonical distance, at worst k rounds of pool distances per query — counts nothing.
 */
int mmiss_index_query_distinct(mmiss_index* idx, const float* queries, int32_t Q, int32_t k, int32_t pool, float min_sep, int32_t nprobe,
                               const uint64_t* require, const uint64_t* exclude, int64_t* out_labels, float* out_dist,
                               int32_t* out_count, int32_t* out_dups, int32_t* out_listed);

/* ---------------------------------------------------------------- subset search ---------------- */
/*
 * The exact top-k within a caller's list of labels: "the nearest rows among THESE images" — an album, a folder, the hits of an
 * earlier search, the rows a metadata predicate admits. The reference's store has it as collection.query(where=..., ids=...).
 *
 *   S = { r < count : labels[r] is in cand_labels }. A label that is not stored is ignored, a label listed several times counts
 *       once, the order of the list means nothing.
 * The result of query q is the exact top-k by (distance, label), with mmiss_index_query's distance bits, over the rows of S that
 * the masks of q admit (require / exclude as mmiss_index_query_filtered, null = 0) and that have a distance; unused slots are
 * -1 / +inf; out_count[q] = min(k, those rows); a query without a direction gives count 0. out_matched[q] = |S| for every q,
 * independent of the masks and of the query; it may be null.
 *
 * Consequences: with every stored label listed, the labels, distance bits and counts are those of mmiss_index_query /
 * mmiss_index_query_filtered; a row outside the list is never returned, however near it is.
 *
 * queries float32 [Q, dim], cand_labels int64 [n_cand], require / exclude uint64 [Q]: each host or device memory; the four outputs
 * (out_labels int64 [Q, k], out_dist float32 [Q, k], out_count int32 [Q], out_matched int64 [Q]) all host or all device memory.
 * n_cand = 0 is legal (cand_labels may then be null): every count is 0. Q >= 1; 1 <= k <= 2040 (above: MMISS_ERR_UNSUPPORTED);
 * k < 1, Q < 1, n_cand < 0 or a null pointer where one is needed: MMISS_ERR_ARG; n_cand above 2^31 - 1: MMISS_ERR_UNSUPPORTED.
 *
 * The call locks the handle, runs on its current stream, returns with its work finished, fails with MMISS_ERR_STATE while a
 * _begin query is open, checks every argument before it writes anything, leaves the eight guard counters and the partition's
 * counters alone, and neither needs nor touches a partition. Every listed row gets its canonical distance directly (no
 * approximate pass, no guard); each listed row is read once per block of up to 16 queries; the queries are taken in chunks that
 * keep the scratch under 512 MB.
 *
 * Not offered: one list per query (a CSR of lists); a subset as the list stage of mmiss_index_query_distinct; ShardedIndex.
 */
int mmiss_index_query_subset(mmiss_index* idx, const float* queries, int32_t Q, int32_t k, const int64_t* cand_labels, int64_t n_cand,
                             const uint64_t* require, const uint64_t* exclude, int64_t* out_labels, float* out_dist,
                             int32_t* out_count, int64_t* out_matched);

/* ---------------------------------------------------------------- search after ----------------- */
/*
 * The exact next k of a ranking behind a cursor (distance, label): "show more". The caller holds the last entry of the page it has
 * and gets the k entries that follow it, at a cost that does not grow with the depth, and the number of rows still to come. The
 * ranking is mmiss_index_query's: canonical distance bits, ties by label. Nothing is kept on the handle between pages.
 *
 * Admitted rows. A(q) is the set of rows r < count for which all of these hold:
 *   - cand_labels is null, or labels[r] is in the list (mmiss_index_query_subset's list: an unknown label is ignored, a repeated
 *     one counts once, the order means nothing);
 *   - the masks of q admit tags[r] (require / exclude as mmiss_index_query_filtered, null = 0);
 *   - the canonical distance d of r to q is not NaN (a query or a row without a direction has none);
 *   - max_dist is null, or d <= max_dist[q] as floats; a NaN max_dist[q] admits nothing;
 *   - r ranks strictly after the cursor: d > after_dist[q], or d == after_dist[q] and labels[r] > after_label[q]. Distances are
 *     compared in the order the ranking itself uses (by their bits: -0.0 before +0.0); labels are compared as values, so the
 *     cursor's label need not be stored — it may have been removed since the last page, and it may be any number. A NaN
 *     after_dist[q] admits nothing; after_dist[q] = -inf is the start of the ranking, whatever the label.
 * Result: the first k of A(q) by (distance, label), -1 / +inf behind the count; out_count[q] = min(k, |A(q)|);
 * out_remaining[q] = |A(q)|, the rows delivered included; it may be null.
 *
 * Consequences:
 *   1. First page. With the cursor -inf, no max_dist and no list, the labels, distance bits and counts are those of
 *      mmiss_index_query / mmiss_index_query_filtered; with a list those of mmiss_index_query_subset; with max_dist those of
 *      mmiss_index_query_radius at cap = k.
 *   2. Pages tile the ranking. Start at -inf and feed each page's last (out_dist, out_labels) back as the next cursor: the chain is
 *      the ranking of A entry for entry, without a repeat or a gap, through runs of equal distances that straddle a page boundary,
 *      past position 2040, at whatever page size 1 <= k <= 2040 each step uses.
 *   3. Remaining. On an unchanged index out_remaining falls by out_count from page to page; the last page has remaining == count;
 *      the page after it has count 0 and remaining 0.
 *   4. Stateless. Rows added, updated or removed between two pages are ranked as they stand at the second call.
 *
 * queries float32 [Q, dim], after_dist float32 [Q], after_label int64 [Q], max_dist float32 [Q], cand_labels int64 [n_cand],
 * require / exclude uint64 [Q]: each host or device memory; the four outputs (out_labels int64 [Q, k], out_dist float32 [Q, k],
 * out_count int32 [Q], out_remaining int64 [Q]) all host or all device memory. Q >= 1; 1 <= k <= 2040 (above:
 * MMISS_ERR_UNSUPPORTED); k < 1, Q < 1, n_cand < 0, a null pointer where one is needed, or cand_labels null with n_cand > 0:
 * MMISS_ERR_ARG; n_cand above 2^31 - 1: MMISS_ERR_UNSUPPORTED. A non-null list with n_cand = 0 is the empty set: counts 0. No
 * cursor value is an error.
 *
 * The call locks the handle, runs on its current stream, returns with its work finished, fails with MMISS_ERR_STATE while a
 * _begin query is open, checks every argument before it writes anything, and leaves the eight guard counters, the partition and
 * its counters alone. Every row (every listed row) is read once per block of up to 16 queries and gets its canonical distance
 * directly; the queries are taken in chunks that keep the scratch under 512 MB. The call is meant for the few queries a scrolling
 * user has open: a large batch over the whole index is bound by the scan's fp64 arithmetic.
 *
 * Not offered: one cursor per shard (ShardedIndex); a cursor into a probed (nprobe) or a distinct ranking; one list per query.
 */
int mmiss_index_query_after(mmiss_index* idx, const float* queries, int32_t Q, int32_t k, const float* after_dist,
                            const int64_t* after_label, const float* max_dist, const int64_t* cand_labels, int64_t n_cand,
                            const uint64_t* require, const uint64_t* exclude, int64_t* out_labels, float* out_dist,
                            int32_t* out_count, int64_t* out_remaining);

/* ---------------------------------------------------------------- grouped search --------------- */
/*
 * The exact k nearest GROUPS of a query, one hit each: one best picture per folder, per upload batch, per k-means cluster. What
 * Qdrant calls group_by, Milvus grouping search and Elasticsearch collapse. The reference ingests whole folders
 * (POST /api/upload-folder, backend/app/main.py:1110) and returns collection.query's list as it comes (main.py:761-782), so a
 * folder of 300 holiday shots fills every slot of a search.
 *
 * Every row carries an int32 GROUP with the lifecycle of the tag word: -1 ("no group: the row is a group of its own") when the
 * row is added; update keeps it; stable removal keeps the survivors'; clear and load reset it. The file format does not hold it.
 * A group id obeys -1 <= group < MMISS_MAX_GROUPS. The table of the exhaustive route (below) has one slot per id below the largest
 * id set since the last clear or load, so ids should be dense.
 */
#define MMISS_MAX_GROUPS (1 << 24)
/* labels: int64 [n], groups: int32 [n] (host or device). A label not in the index, or a group outside -1 .. MMISS_MAX_GROUPS - 1
 * -> MMISS_ERR_ARG and nothing is changed. A label given twice keeps its last value. */
int mmiss_index_set_groups(mmiss_index* idx, const int64_t* labels, const int32_t* groups, int64_t n);
/* out: int32 [n] (host or device), the groups of `labels`; a label not in the index -> MMISS_ERR_ARG */
int mmiss_index_get_groups(mmiss_index* idx, const int64_t* labels, int64_t n, int32_t* out);
/*
 * Contract.
 *   - R(q) is the complete ranking of the rows that q admits (require / exclude as mmiss_index_query_filtered, null = 0) and that
 *     have a direction, in (distance, label) order with mmiss_index_query's distance bits.
 *   - The group of a row is its GROUP value. A row with -1 is a group of its own.
 *   - A group's head is its first row in R(q).
 *   - The result is the first k heads in R(q)'s order. The call never depends on `pool`: it is exact at any group size.
 *   - out_labels / out_dist [Q, k] hold the heads. Slots behind the count hold -1 / +inf.
 *   - out_group [Q, k] holds the head's GROUP. It is -1 for an ungrouped row and behind the count.
 *   - out_count[q] = min(k, number of groups with at least one admitted row that has a direction). It is 0 for a query without a
 *     direction.
 *   - out_route[q] (may be null) is 0 when the list walk answered q, and 1 when q took the exhaustive route.
 * Consequences:
 *   - With every row ungrouped, or every row in a group of its own, the labels, distance bits and counts equal
 *     mmiss_index_query_filtered's.
 *   - With all rows in one group, the result is one entry: the top-1.
 *   - The outputs do not depend on `pool`.
 *
 * How: the flat / filtered query at k = pool gives each query's exact ranked list (pool = 0: min(2040, max(8 k, 64))); one kernel
 * walks all lists and keeps the first entry of every group. A walk that found k heads, or whose list ended before the pool did,
 * has the answer (route 0). Any other query — one group owns the pool: a folder of 5000 near rows in front of a pool of 2040 —
 * takes the exhaustive route in the same call (route 1): every admitted row gets its canonical distance directly, the minimum
 * (distance, row) key per group is kept in a table of one slot per group id and one per ungrouped row, and the k smallest slots
 * are selected. `pool` only moves queries between the routes.
 *
 * 1 <= k <= 2040 (above: MMISS_ERR_UNSUPPORTED). pool = 0, or k <= pool <= 2040: pool < k is MMISS_ERR_ARG, pool > 2040 is
 * MMISS_ERR_UNSUPPORTED. Q >= 1. A missing pointer (out_route excepted) is MMISS_ERR_ARG. queries float32 [Q, dim] and require /
 * exclude uint64 [Q] are each host or device memory; the outputs (out_labels int64 [Q, k], out_dist float32 [Q, k], out_group int32
 * [Q, k], out_count int32 [Q], out_route int32 [Q]) are all host or all device memory.
 *
 * The call locks the handle, runs on its current stream, returns with its work finished, fails with MMISS_ERR_STATE while a
 * _begin query is open, checks every argument before it writes anything, and neither needs nor touches a partition. The list stage
 * counts in the guard counters exactly as mmiss_index_query / _filtered at k = pool do; the walk and the exhaustive route count
 * nothing. The exhaustive route reads each row once per block of up to 16 of its queries and takes its queries in chunks that keep
 * the tables under 512 MB; a large batch on that route is bound by the scan's fp64 arithmetic.
 *
 * Not offered: more than one row per group (expand a group with mmiss_index_query_subset over its labels); nprobe; a list or a
 * cursor combined with grouping; ShardedIndex; an approximate matrix-core first pass for the exhaustive route.
 */
int mmiss_index_query_grouped(mmiss_index* idx, const float* queries, int32_t Q, int32_t k, int32_t pool,
                              const uint64_t* require, const uint64_t* exclude,
                              int64_t* out_labels, float* out_dist, int32_t* out_group, int32_t* out_count,
                              int32_t* out_route /* may be null */);

/* ---------------------------------------------------------------- glue kernels ----------------- */
/*
 * out[q] = normalize(w * normalize(img[q]) + (1-w) * normalize(txt[q])), float32 [Q,dim].
 * w is applied as numpy does for `python_float * float32_array`: (float)w and (float)(1.0 - w).
 * replaces search_multimodal's blend — backend/app/main.py:852-860
 */
int mmiss_blend(int device, void* hip_stream, const float* img, const float* txt, double w,
                int32_t Q, int32_t dim, float* out);

/*
 * Merge S per-shard result lists (as produced by mmiss_index_query on each shard, then all-gathered)
 * into the global top-k: dist float32 [S,Q,k], labels int64 [S,Q,k] -> out [Q,k], ordered by
 * (distance asc, label asc), label -1 entries ignored. Any S >= 1 and k <= 4096: up to 8192 entries per query are
 * merged in one pass (8 shards x the UI's "All" = 1000 hits, backend/app/main.py:757), more in several levels.
 * No reference analogue (the reference is single-process); this is the one exchange step of the row-sharded
 * index.
 */
int mmiss_merge_topk(int device, void* hip_stream, const float* dist, const int64_t* labels,
                     int32_t S, int32_t Q, int32_t k, float* out_dist, int64_t* out_labels, int32_t* out_count);

/* ---------------------------------------------------------------- kernel timing ---------------- */
/*
 * When enabled every kernel launch of this library is bracketed by HIP events on its stream and
 * accumulated per kernel class. mmiss_prof_read drains finished events and writes a JSON array
 *   [{"kernel": "...", "launches": n, "ms": total, "flops": algorithmic, "bytes": algorithmic}, ...]
 * into buf (NUL-terminated, truncated to cap). Used by bench.py for the roofline object.
 */
int mmiss_prof_enable(int on);
/* restrict the bracketing to one kernel class and to every stride-th launch of it (kernel = NULL or "" lifts the
 * restriction). Lets bench.py time the dominant kernel INSIDE its timed region at negligible cost. */
int mmiss_prof_filter(const char* kernel, int stride);
int mmiss_prof_reset(void);
int mmiss_prof_read(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MMISS_H */

"""ctypes binding of libmmiss.so (include/mmiss.h, include/mmiss_debug.h).

The library is the product; this module only loads it and converts its status codes into
exceptions. There is deliberately NO fallback: if libmmiss.so is missing or does not load, importing
the compute path raises (build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C multimodal-image-similarity-search_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmmiss.so")

MMISS_OK = 0
MMISS_F32 = 0
MMISS_F16 = 1
MMISS_F8 = 2
MMISS_PREC_BF16 = 0
MMISS_PREC_FP8 = 1
MMISS_PREC_BF16_F32RESID = 2
MMISS_TOWER_VISION = 0
MMISS_TOWER_TEXT = 1

EPI_F32, EPI_BIAS_BF16, EPI_BIAS_QGELU_BF16, EPI_BIAS_RESID_F32, EPI_PATCH_F32 = range(5)


class MmissError(RuntimeError):
    """Non-zero status from libmmiss (the reference's `except Exception` paths catch it)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"libmmiss error {code}: {msg}")
        self.code = code


class ClipConfigStruct(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("v_hidden", C.c_int32), ("v_layers", C.c_int32), ("v_heads", C.c_int32),
        ("v_mlp", C.c_int32), ("v_patch", C.c_int32), ("v_image", C.c_int32),
        ("t_hidden", C.c_int32), ("t_layers", C.c_int32), ("t_heads", C.c_int32),
        ("t_mlp", C.c_int32), ("t_vocab", C.c_int32), ("t_ctx", C.c_int32),
        ("proj_dim", C.c_int32), ("eos_token_id", C.c_int32), ("ln_eps", C.c_float),
        ("max_batch_image", C.c_int32), ("max_batch_text", C.c_int32),
    ]


_P = C.c_void_p
_I = C.c_int
_I32 = C.c_int32
_I64 = C.c_int64

# name -> (restype, argtypes); every symbol declared in include/mmiss.h and include/mmiss_debug.h
SIGNATURES = {
    # mmiss.h
    "mmiss_abi_version": (_I, []),
    "mmiss_last_error": (C.c_char_p, []),
    "mmiss_device_count": (_I, [C.POINTER(_I)]),
    "mmiss_encoder_create": (_I, [C.POINTER(ClipConfigStruct), _I, C.POINTER(_P)]),
    "mmiss_encoder_destroy": (_I, [_P]),
    "mmiss_encoder_set_weight": (_I, [_P, C.c_char_p, _P, _I64, C.POINTER(_I)]),
    "mmiss_encoder_finalize": (_I, [_P]),
    "mmiss_encoder_set_precision": (_I, [_P, _I32]),
    "mmiss_encoder_set_tower_precision": (_I, [_P, _I32, _I32]),
    "mmiss_encoder_calibrate": (_I, [_P, _P, _I32]),
    "mmiss_encoder_calibration_clear": (_I, [_P]),
    "mmiss_encoder_calibration_info": (_I, [_P, C.POINTER(_I64)]),
    "mmiss_encoder_calibration_get": (_I, [_P, _P, _I64, C.POINTER(_I64)]),
    "mmiss_encoder_calibration_set": (_I, [_P, _P, _I64]),
    "mmiss_encoder_set_stream": (_I, [_P, _P, _I32]),
    "mmiss_encode_image": (_I, [_P, _P, _I32, _P]),
    "mmiss_encode_image_u8": (_I, [_P, _P, _I32, _P]),
    "mmiss_resize_crop_rgb": (_I, [_P, _P, _I64, _P, _P, _P, _I32, _P]),
    "mmiss_encode_image_rgb": (_I, [_P, _P, _I64, _P, _P, _P, _I32, _P]),
    "mmiss_encode_text": (_I, [_P, _P, _I32, _I32, _P]),
    "mmiss_encoder_tap": (_I, [_P, _I, _I, _P, _I64, C.POINTER(_I64)]),
    "mmiss_index_create": (_I, [_I32, _I32, _I, _I64, C.POINTER(_P)]),
    "mmiss_index_destroy": (_I, [_P]),
    "mmiss_index_set_stream": (_I, [_P, _P, _I32]),
    "mmiss_index_add": (_I, [_P, _P, _P, _I64]),
    "mmiss_index_update": (_I, [_P, _P, _P, _I64]),
    "mmiss_index_remove": (_I, [_P, _P, _I64, C.POINTER(_I64)]),
    "mmiss_index_clear": (_I, [_P]),
    "mmiss_index_count": (_I, [_P, C.POINTER(_I64)]),
    "mmiss_index_get": (_I, [_P, _P, _I64, _P]),
    "mmiss_index_labels": (_I, [_P, _P, _I64]),
    "mmiss_index_query": (_I, [_P, _P, _I32, _I32, _P, _P, _P]),
    "mmiss_index_query_begin": (_I, [_P, _P, _I32, _I32, _P, _P, _P]),
    "mmiss_index_query_end": (_I, [_P]),
    "mmiss_index_query_abort": (_I, [_P]),
    "mmiss_index_guard_stats": (_I, [_P, C.POINTER(_I64)]),
    "mmiss_index_guard_stats_ex": (_I, [_P, C.POINTER(_I64)]),
    "mmiss_index_save": (_I, [_P, C.c_char_p]),
    "mmiss_index_load": (_I, [_P, C.c_char_p]),
    "mmiss_index_set_tags": (_I, [_P, _P, _P, _I64]),
    "mmiss_index_get_tags": (_I, [_P, _P, _I64, _P]),
    "mmiss_index_query_filtered": (_I, [_P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "mmiss_index_query_filtered_begin": (_I, [_P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "mmiss_index_query_radius": (_I, [_P, _P, _I32, _P, _I32, _P, _P, _P, _P, _P, _P]),
    "mmiss_index_query_radius_by_label": (_I, [_P, _P, _I64, C.c_float, _I32, _I32, _P, _P, _P, _P]),
    "mmiss_index_membership": (_I, [_P, _P, _I32, _P, _P, _I64, _P]),
    "mmiss_index_tag_by_radius": (_I, [_P, _P, _I32, _P, _P, _P]),
    "mmiss_index_assign": (_I, [_P, _P, _I32, _P, _P, _I64, _P]),
    "mmiss_index_cluster_sums": (_I, [_P, _P, _I64, _I32, _P, _P]),
    "mmiss_index_partition_set": (_I, [_P, _P, _I32, _P, _I64]),
    "mmiss_index_partition_clear": (_I, [_P]),
    "mmiss_index_partition_info": (_I, [_P, C.POINTER(_I64)]),
    "mmiss_index_partition_get": (_I, [_P, _P, _P, _I64, _P]),
    "mmiss_index_query_probed": (_I, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "mmiss_index_query_distinct": (_I, [_P, _P, _I32, _I32, _I32, C.c_float, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "mmiss_index_query_subset": (_I, [_P, _P, _I32, _I32, _P, _I64, _P, _P, _P, _P, _P, _P]),
    "mmiss_index_query_after": (_I, [_P, _P, _I32, _I32, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P]),
    "mmiss_index_set_groups": (_I, [_P, _P, _P, _I64]),
    "mmiss_index_get_groups": (_I, [_P, _P, _I64, _P]),
    "mmiss_index_query_grouped": (_I, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "mmiss_blend": (_I, [_I, _P, _P, _P, C.c_double, _I32, _I32, _P]),
    "mmiss_merge_topk": (_I, [_I, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "mmiss_prof_enable": (_I, [_I]),
    "mmiss_prof_filter": (_I, [C.c_char_p, _I]),
    "mmiss_prof_reset": (_I, []),
    "mmiss_prof_read": (_I, [C.c_char_p, C.c_size_t]),
    # mmiss_debug.h
    "mmiss_dbg_gemm": (_I, [_I, _P, _I, _I, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32]),
    "mmiss_dbg_gemm_ex": (_I, [_I, _P, _I, _I, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, C.c_float]),
    "mmiss_dbg_gemm_form": (_I, [_I32, _I32, _I32, _I32, _I32]),
    "mmiss_dbg_gemm_p256": (_I, [_I, _P, _I, _P, _P, _P, _P, _P, _P, C.c_float, _I32, _I32, _I32, _I32, _I32, _P]),
    "mmiss_dbg_gemm_resid16": (_I, [_I, _P, _I, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "mmiss_dbg_gemm_time": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32,
                                 C.POINTER(C.c_float)]),
    "mmiss_dbg_layernorm": (_I, [_I, _P, _P, _P, _P, _P, _I32, _I32, _I32, C.c_float]),
    "mmiss_dbg_layernorm16": (_I, [_I, _P, _P, _P, _P, _P, _I32, _I32, C.c_float]),
    "mmiss_dbg_layernorm_gather": (_I, [_I, _P, _P, _P, _P, _P, _I32, _P, _I32, _I32, C.c_float]),
    "mmiss_dbg_prelayernorm_stats": (_I, [_I, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, C.c_float, _I32, _P, _P, _I32]),
    "mmiss_dbg_prelayernorm_skinny": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, C.c_float]),
    "mmiss_dbg_row_stats": (_I, [_I, _P, _P, _P, _P, _I32, _I32, _I32]),
    "mmiss_dbg_row_stats16": (_I, [_I, _P, _P, _P, _P, _I32, _I32]),
    "mmiss_dbg_gemm_skinny_fold": (_I, [_I, _P, _I, _P, _P, _P, _P, _P, _P, C.c_float, _I32, _I32, _I32]),
    "mmiss_dbg_gemm_skinny_resid": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32]),
    "mmiss_dbg_ln_finalize": (_I, [_I, _P, _P, _P, _I32, _I32, _I32, C.c_float]),
    "mmiss_dbg_fold_ln_weights": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32]),
    "mmiss_dbg_attention": (_I, [_I, _P, _P, _P, _I32, _I32, _I32, _I32]),
    "mmiss_dbg_attention_tiled": (_I, [_I, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32]),
    "mmiss_dbg_im2col": (_I, [_I, _P, _P, _P, _I32, _I32, _I32, _I32]),
    "mmiss_dbg_patch_from_pixels": (_I, [_I, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32]),
    "mmiss_dbg_attention_pooled": (_I, [_I, _P, _P, _P, _P, _I32, _I32, _I32, _I32]),
    "mmiss_dbg_gemm_resid_rows": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32]),
    "mmiss_dbg_encoder_record_taps": (_I, [_P, _I]),
    "mmiss_dbg_encoder_set_fuse_ln": (_I, [_P, _I]),
    "mmiss_dbg_set_option": (_I, [C.c_char_p, _I]),
    "mmiss_dbg_quantize_weights_fp8": (_I, [_I, _P, _P, _P, _P, _I32, _I32]),
    "mmiss_dbg_layernorm_mxfp8": (_I, [_I, _P, _P, _P, _P, _P, _P, _I32, _I32, C.c_float]),
    "mmiss_dbg_layernorm16_mxfp8": (_I, [_I, _P, _P, _P, _P, _P, _P, _I32, _I32, C.c_float]),
    "mmiss_dbg_attention_mx": (_I, [_I, _P, _P, _P, _P, _I32, _I32, _I32]),
    "mmiss_dbg_gemm8": (_I, [_I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32]),
    "mmiss_dbg_gemm8_time": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, C.POINTER(C.c_float)]),
    "mmiss_dbg_ln_colstats": (_I, [_I, _P, _P, _I32, _P, _P, _I32, _I32, C.c_float, _P, _P, _P, _P]),
    "mmiss_dbg_bias_fold": (_I, [_I, _P, _P, _P, _P, _I32, _I32, _P]),
    "mmiss_dbg_resize_coeffs": (_I, [_I, _P, _I32, _I32, _I32, _P, _P, _P]),
    "mmiss_dbg_resize_crop_variant": (_I, [_I64, _I32]),
    "mmiss_dbg_index_plan": (_I, [_P, _I32, _I32, _I32, _I32, C.POINTER(_I32)]),
    "mmiss_dbg_index_radius_plan": (_I, [_P, _I32, _I32, C.POINTER(_I32)]),
    "mmiss_dbg_index_read_rows": (_I, [_P, _I64, _I64, _P, _P, _P, _P]),
    "mmiss_dbg_index_prep_queries": (_I, [_P, _P, _I32, _P, _P, _P]),
    "mmiss_dbg_index_probe_plan": (_I, [_P, _I32, _I32, _I32, C.POINTER(_I32)]),
    "mmiss_dbg_index_distinct_plan": (_I, [_P, _I32, C.POINTER(_I32)]),
    "mmiss_dbg_index_subset_plan": (_I, [_P, _I32, _I32, _I64, C.POINTER(_I32)]),
    "mmiss_dbg_index_after_plan": (_I, [_P, _I32, _I32, _I64, C.POINTER(_I32)]),
    "mmiss_dbg_index_grouped_plan": (_I, [_P, _I32, _I32, _I32, C.POINTER(_I32)]),
    "mmiss_dbg_index_dense_plan": (_I, [_P, _I32, C.POINTER(_I32)]),
    "mmiss_dbg_encoder_plan": (_I, [_P, _I32, _I32, _I32, C.POINTER(_I32)]),
    "mmiss_dbg_gemm_split_time": (_I, [_I, _I, _I, _P, _P, _P, _P, _I32, _I32, _I32, _I32, C.POINTER(C.c_float)]),
}

_lib = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """Load libmmiss.so once and attach prototypes. Raises if the library is absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: the HIP extension is not built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` at the repo root. "
                "There is no CPU fallback for the mmiss hot path."
            )
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if lib.mmiss_abi_version() != 1:
            raise ImportError("libmmiss.so ABI version mismatch")
        _lib = lib
        # experiment knobs from the environment: MMISS_OPTIONS="gemm_wide=1,scan_rounds=2" (see mmiss_dbg_set_option)
        for kv in filter(None, os.environ.get("MMISS_OPTIONS", "").split(",")):
            k, _, v = kv.partition("=")
            lib.mmiss_dbg_set_option(k.strip().encode(), int(v))
        return lib


def check(status: int) -> None:
    if status != MMISS_OK:
        msg = load().mmiss_last_error()
        raise MmissError(status, msg.decode("utf-8", "replace") if msg else "")


def ptr(x) -> int:
    """Raw address of a torch tensor / numpy array (contiguous) or an int passthrough."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("tensor passed to libmmiss must be contiguous")
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array passed to libmmiss must be C-contiguous")
        return x.ctypes.data
    raise TypeError(f"cannot take the address of {type(x)!r}")


def device_count() -> int:
    n = _I(0)
    check(load().mmiss_device_count(C.byref(n)))
    return n.value


def current_stream_ptr(device=None):
    """hipStream_t of torch's current stream as an integer (0 = default stream)."""
    import torch

    return int(torch.cuda.current_stream(device).cuda_stream)


def set_option(key: str, value: int) -> None:
    check(load().mmiss_dbg_set_option(key.encode(), int(value)))


def prof_enable(on: bool) -> None:
    check(load().mmiss_prof_enable(1 if on else 0))


def prof_filter(kernel=None, stride: int = 1) -> None:
    check(load().mmiss_prof_filter(kernel.encode() if kernel else None, int(stride)))


def prof_reset() -> None:
    check(load().mmiss_prof_reset())


def prof_read() -> list:
    import json

    buf = C.create_string_buffer(1 << 16)
    check(load().mmiss_prof_read(buf, len(buf)))
    return json.loads(buf.value.decode())


def gemm_form(bm: int, M: int, N: int, K: int, splits: int = 1):
    """mmiss_dbg_gemm_form as (staging buffers, waves) of the 128-column tile kernel under the current options; None where the
    shape is no launch of it. Nothing is launched."""
    v = load().mmiss_dbg_gemm_form(int(bm), int(M), int(N), int(K), int(splits))
    return divmod(v, 10) if v else None


INDEX_PLAN_FIELDS = ("dense", "dense8", "big", "strip_v3", "sample", "kp", "pages", "Mq", "Npad", "ns_tiles", "strip", "nqt", "cap",
                     "slabs", "tiles_per_block", "qtiles", "splits", "merge_two_level", "sweep_gemm", "sweep_nqt", "sweep_slabs",
                     "sweep_tiles_per_block", "sweep_strip", "groups_per_split")


def index_plan(handle, Q: int, k: int, filtered: bool = False, flagged: int = 0) -> dict:
    """mmiss_dbg_index_plan as a dict: the path a query call of this shape would take on the index `handle` as it stands (and the
    widen pass's, were `flagged` of its queries flagged). Nothing is launched."""
    out = (_I32 * 24)()
    check(load().mmiss_dbg_index_plan(handle, int(Q), int(k), 1 if filtered else 0, int(flagged), out))
    return dict(zip(INDEX_PLAN_FIELDS, (int(v) for v in out)))


RADIUS_PLAN_FIELDS = ("queries", "gemm", "strip", "nqt", "slabs", "tiles_per_block", "qtiles")


def index_radius_plan(handle, Q: int, filtered: bool = False) -> dict:
    """mmiss_dbg_index_radius_plan as a dict: {"chunks": n, "first": {...}, "last": {...}}, the threshold pass of the first and
    of the last chunk (at most 1024 queries each) of a radius call of Q queries on the index `handle` as it stands. Nothing is
    launched."""
    out = (_I32 * 16)()
    check(load().mmiss_dbg_index_radius_plan(handle, int(Q), 1 if filtered else 0, out))
    v = [int(x) for x in out]
    return {"chunks": v[0], "first": dict(zip(RADIUS_PLAN_FIELDS, v[1:8])), "last": dict(zip(RADIUS_PLAN_FIELDS, v[8:15]))}


PROBE_PLAN_FIELDS = ("splits", "segment", "levels", "queries_per_chunk", "bound", "share", "slots", "chunks")


def index_probe_plan(handle, Q: int, k: int, nprobe: int) -> dict:
    """mmiss_dbg_index_probe_plan as a dict: how a probed call of this shape would run on the partition of the index `handle` as it
    stands (and under the option probe_scratch_kb as it stands). Nothing is launched."""
    out = (_I32 * 8)()
    check(load().mmiss_dbg_index_probe_plan(handle, int(Q), int(k), int(nprobe), out))
    return dict(zip(PROBE_PLAN_FIELDS, (int(v) for v in out)))


DISTINCT_PLAN_FIELDS = ("rows_per_trip", "threads", "lds_bytes", "queries_per_launch", "launches", "max_pool")


def index_distinct_plan(handle, Q: int) -> dict:
    """mmiss_dbg_index_distinct_plan as a dict: how the suppression stage of a distinct call of Q queries is laid out on the index
    `handle`. Nothing is launched."""
    out = (_I32 * 8)()
    check(load().mmiss_dbg_index_distinct_plan(handle, int(Q), out))
    return dict(zip(DISTINCT_PLAN_FIELDS, (int(v) for v in out)))


SUBSET_PLAN_FIELDS = ("bound", "segment", "levels", "stride0", "stride1", "queries_per_chunk", "chunks", "query_block", "lds_bytes",
                      "share", "splits", "rows_per_trip", "compact_blocks", "compact_block_rows", "first_chunk_block",
                      "last_chunk_block")


def index_subset_plan(handle, Q: int, k: int, n_cand: int) -> dict:
    """mmiss_dbg_index_subset_plan as a dict: how a subset call of this shape would run on the index `handle` as it stands (and
    under the option probe_scratch_kb as it stands). Nothing is launched."""
    out = (_I32 * 16)()
    check(load().mmiss_dbg_index_subset_plan(handle, int(Q), int(k), int(n_cand), out))
    return dict(zip(SUBSET_PLAN_FIELDS, (int(v) for v in out)))


GROUPED_PLAN_FIELDS = ("pool", "walk_threads", "walk_lds_bytes", "table", "segment", "levels", "stride0", "stride1",
                       "queries_per_chunk", "chunks", "query_block", "lds_bytes", "share", "splits", "first_chunk_block",
                       "last_chunk_block")


def index_grouped_plan(handle, Q: int, k: int, pool: int = 0) -> dict:
    """mmiss_dbg_index_grouped_plan as a dict: how a grouped call of this k and pool would run on the index `handle` as it stands
    (and under the option probe_scratch_kb as it stands) if Q of its queries took the exhaustive route. Nothing is launched."""
    out = (_I32 * 16)()
    check(load().mmiss_dbg_index_grouped_plan(handle, int(Q), int(k), int(pool), out))
    return dict(zip(GROUPED_PLAN_FIELDS, (int(v) for v in out)))


DENSE_PLAN_KERNELS = ("canonical_scan", "assign_resolve", "member_count", "assign_sizes", "assign_decide", "member_from_dist",
                      "member_merge_tags")


def index_dense_plan(handle, n_operands: int) -> dict:
    """mmiss_dbg_index_dense_plan as a dict: how the dense scans over the index `handle` as it stands would run with n_operands
    probes / centres / clusters — {"scan": {nqt, lds_bytes, slabs, tiles_per_block, passes, wave_trips, block_rows}, one
    {"grid", "rows_per_trip", "trips"} per kernel of DENSE_PLAN_KERNELS, "cluster_sums": {cols, chunks, rows_per_block, slabs,
    lds_bytes}, "compact_blocks", "compact_block_rows", "rows"}. Nothing is launched."""
    out = (_I32 * 40)()
    check(load().mmiss_dbg_index_dense_plan(handle, int(n_operands), out))
    v = [int(x) for x in out]
    d = {"scan": dict(zip(("nqt", "lds_bytes", "slabs", "tiles_per_block", "passes", "wave_trips", "block_rows"), v[0:7]))}
    for i, name in enumerate(DENSE_PLAN_KERNELS):
        d[name] = dict(zip(("grid", "rows_per_trip", "trips"), v[8 + 3 * i:11 + 3 * i]))
    d["cluster_sums"] = dict(zip(("cols", "chunks", "rows_per_block", "slabs", "lds_bytes"), v[30:35]))
    d["compact_blocks"], d["compact_block_rows"], d["rows"] = v[35], v[36], v[37]
    return d


AFTER_PLAN_FIELDS = SUBSET_PLAN_FIELDS[:13] + ("dense",) + SUBSET_PLAN_FIELDS[14:]


def index_after_plan(handle, Q: int, k: int, n_cand=None) -> dict:
    """mmiss_dbg_index_after_plan as a dict: how a continuation call (FlatIndex.query_after) of this shape would run on the index
    `handle` as it stands (and under the option probe_scratch_kb as it stands); n_cand None: no list. Nothing is launched."""
    out = (_I32 * 16)()
    check(load().mmiss_dbg_index_after_plan(handle, int(Q), int(k), -1 if n_cand is None else int(n_cand), out))
    return dict(zip(AFTER_PLAN_FIELDS, (int(v) for v in out)))


_INDEX_ELT = {MMISS_F32: "float32", MMISS_F16: "float16", MMISS_F8: "uint8"}


def index_read_rows(handle, dim: int, dtype: int, row0: int, n: int) -> dict:
    """mmiss_dbg_index_read_rows as numpy arrays: {"rows": [n, dim] float32 / float16 / uint8 (e4m3 codes), "inv": float32 [n] (fp8
    rows; None otherwise), "labels": int64 [n], "tags": uint64 [n]}, the device buffers of rows [row0, row0 + n) as they stand
    (row0 + n <= capacity; rows behind count included)."""
    import numpy as np

    rows = np.empty((n, dim), dtype=_INDEX_ELT[dtype])
    inv = np.empty(n, dtype=np.float32) if dtype == MMISS_F8 else None
    labels = np.empty(n, dtype=np.int64)
    tags = np.empty(n, dtype=np.uint64)
    check(load().mmiss_dbg_index_read_rows(handle, int(row0), int(n), rows.ctypes.data, None if inv is None else inv.ctypes.data,
                                           labels.ctypes.data, tags.ctypes.data))
    return {"rows": rows, "inv": inv, "labels": labels, "tags": tags}


def index_prep_queries(handle, dim: int, dtype: int, queries) -> tuple:
    """mmiss_dbg_index_prep_queries -> (qn float32 [Q, dim], qs [round_up(Q, 256), dim] float32 for f32 rows / float16 otherwise,
    eps_q float32 [Q]): what the query preparation of a query call with these queries (numpy, or a CUDA tensor on the handle's
    current stream) leaves in the handle's scratch."""
    import numpy as np

    Q = int(queries.shape[0])
    qn = np.empty((Q, dim), dtype=np.float32)
    qs = np.empty(((Q + 255) // 256 * 256, dim), dtype=np.float32 if dtype == MMISS_F32 else np.float16)
    eps = np.empty(Q, dtype=np.float32)
    check(load().mmiss_dbg_index_prep_queries(handle, ptr(queries), Q, qn.ctypes.data, qs.ctypes.data, eps.ctypes.data))
    return qn, qs, eps


ENCODER_PLAN_FIELDS = ("fold", "fold_final", "fp8", "out8", "resid16", "sfold", "prune", "embed", "qkv", "qkv_bm", "out", "out_bm",
                       "fc1", "fc1_bm", "fc2", "fc2_bm", "pooled_tail", "fc2_splitk", "M", "lean_pre", "patch", "patch_bm", "patch_splitk",
                       "att_hpb", "att_stream")
GEMM_KINDS = ("Tile", "Tile256", "P256", "P160", "Skinny", "Fp8Tile", "P256Fp8")
EMBED_OUTS = ("Nothing", "Stats64", "Stats16")


def encoder_plan(handle, tower: int, B: int, T: int = 0) -> dict:
    """mmiss_dbg_encoder_plan as a dict: the path one chunk of B items (T tokens each on the text tower) would take on the encoder
    `handle` as it stands, under the options as they stand; GEMM kernels and `embed` by name. No kernel is launched."""
    out = (_I32 * 32)()
    check(load().mmiss_dbg_encoder_plan(handle, int(tower), int(B), int(T), out))
    plan = dict(zip(ENCODER_PLAN_FIELDS, (int(v) for v in out)))
    for k in ("qkv", "out", "fc1", "fc2", "patch"):
        plan[k] = GEMM_KINDS[plan[k]]
    plan["embed"] = EMBED_OUTS[plan["embed"]]
    return plan

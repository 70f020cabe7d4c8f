"""Which calls of tests/encoder_sequence_cases.py (`sc`) run on a caller's stream, shared by test_encoder_stream_cases_cpu.py (which
establishes on the host what the GPU tests rely on) and test_encoder_streams_gpu.py (which runs them). A plain helper module: no
fixtures, numpy only.

With use_own == 0 (mmiss_encoder_set_stream) an encode call is queued on the caller's stream and returns; the kernels, the plan and
the operands are the ones of the same call on the handle's own stream, so the result must be the same BITS. What can go wrong is
order: a launch on another stream, a missing or a needless host wait, a hand-over between streams that does not wait for the
handle's last call (or waits for the caller's whole stream), a state change under a queued call. One victim per plan row of sc.CASES
but (e) (200 MB of pixels, the workload's own size), at the smallest size the table has."""
import dataclasses
import functools

import numpy as np

from oracle import clip_oracle as co
import encoder_sequence_cases as sc

# (a) every route: device in, device out, on torch's default stream and on a side stream
ROUTE_NAMES = (
    "a-sfold-B1", "a-sfold-pooled-B25", "b-plain-B77", "c-fold-bm128-B77", "c-fold-bm160-B113", "d-p256-B205", "d-p256-final-B205",
    "f-splitk-B77", "g-fp8-out8-B77", "g-fp8-calibrated-B77", "h-p256fp8-B205", "i-p256fp8-w1024-ragged-B170", "k-long257-B3",
    "k-stream257-B3", "k-tiled577-B2", "k-fp8-mx-tiled577-B2", "j-a-B7-T16-full", "j-c-B43-T9-full", "j-b-pooled-B29-T9-full",
    "j-g-fp8-B43-T9",
)
LEFT_OUT_PLANS = ("e",)
# the integer input routes (uint8 crops; raw RGB of mixed size in one device blob) on a plain and a folded plan
INT_ROUTES = (("b-plain-B77", "u8"), ("b-plain-B77", "rgb"), ("c-fold-bm128-B77", "u8"), ("c-fold-bm128-B77", "rgb"))
# one call longer than max_batch (sc.CHUNK_CASES): its chunks follow one another on the stream, no host wait in between
CHUNK = ("f32", 160, 77)
assert CHUNK in sc.CHUNK_CASES

# (b) order behind the caller's producer: one case per vision input route, text (the chunked call is CHUNK)
ORDER = (("b-plain-B77", "f32"), ("c-fold-bm128-B77", "u8"), ("b-plain-B77", "rgb"), ("j-c-B43-T9-full", "f32"))
# (c) two calls on one stream with the caller's work between them
NO_DRAIN = ("c-fold-bm128-B77", "j-b-pooled-B29-T9-full")
# (d) host operands on a caller's stream, through the C ABI
HOST_OPERANDS = ("b-plain-B77", "j-c-B43-T9-full")
# (e) hand-over between streams: the skinny chain and a tiled fp8 plan use different workspaces
HANDOVER = ("a-sfold-B25", "g-fp8-out8-B77")
# (f) weights / precision / calibration behind a queued encode: (case whose victim is queued, what changes)
WEIGHTS_CASE = "c-fold-bm128-B77"
PRECISION_CASE = "g-fp8-out8-B77"        # queued on a bf16 handle under the case's options, then set_precision("fp8")
CALIBRATION_CASE = "g-fp8-calibrated-B77"  # queued on an uncalibrated fp8 handle, then set_calibration(table)
W2_SEED = 131


def case(name):
    hits = [c for c in sc.CASES if c.name == name]
    assert len(hits) == 1, name
    return hits[0]


def all_names():
    return (ROUTE_NAMES + tuple(n for n, _ in INT_ROUTES + ORDER) + NO_DRAIN + HOST_OPERANDS + HANDOVER
            + (WEIGHTS_CASE, PRECISION_CASE, CALIBRATION_CASE))


def via_call(c, via):
    """The victim of a vision case through another input route (same B, same plan)."""
    return dataclasses.replace(c.victim, via=via)


def handover_calls(c):
    """(X1, poison, later victim) of a hand-over pair: the case's victim on s1, its NaN poison (another B, another plan) on s2, and
    a second victim of the same shape and plan, other pixels."""
    poison = [p for p in c.poisons if p.kind == "nan"][0]
    return c.victim, poison, dataclasses.replace(c.victim, seed=c.victim.seed + 1000)


def bf16_twin_of(c):
    """PRECISION_CASE before the switch: the same call on a handle still at bf16 (its options leave the folded bf16 plan)."""
    v = dataclasses.replace(c.victim, expect=(("fp8", 0), ("fold", 1), ("resid16", 1)))
    return dataclasses.replace(c, name=c.name + "-at-bf16", victim=v, precision="bf16")


@functools.lru_cache(maxsize=None)
def weights2(shape_key):
    """W2 of (f): co.init_weights under another seed, the NaN token row as in sc.weights."""
    W = co.init_weights(sc.SHAPES[shape_key], seed=W2_SEED)
    tok = W["text_model.embeddings.token_embedding.weight"].copy()
    tok[sc.NAN_ID] = np.nan
    W["text_model.embeddings.token_embedding.weight"] = tok
    return W

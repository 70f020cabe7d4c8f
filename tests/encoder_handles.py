"""Handles, options and plans of the encoder sequence tables (tests/encoder_sequence_cases.py), shared by the GPU tests that run
them: test_encoder_sequence_gpu.py (what a call leaves in the handle) and test_encoder_streams_gpu.py (the same calls on a
caller's stream). A plain helper module: no fixtures, nothing runs at import."""
import contextlib

import numpy as np

import encoder_sequence_cases as sc


def calibration_table(shape):
    """A table as mmiss_encoder_calibrate would leave it: a constant per channel of every LayerNorm output."""
    s = sc.SHAPES[shape]
    g = np.random.Generator(np.random.Philox(key=[20251019, 6]))
    return (0.2 * g.standard_normal((2 * s.v_layers, s.v_hidden))).astype(np.float32)


def new_handle(shape, tower, precision, max_batch, calibrated=False, weights=None):
    import mmiss_amd  # noqa: F401
    from mmiss_amd.encoder import ClipEncoder, ClipShape

    s = sc.SHAPES[shape]
    mi, mt = (max_batch, 8) if tower == "vision" else (8, max_batch)
    enc = ClipEncoder(ClipShape.from_any(s), max_batch_image=mi, max_batch_text=mt)
    if precision == "fp8":
        if tower == "vision":
            enc.set_precision("fp8")
        else:
            enc.set_tower_precision("text", "fp8")
    W = sc.weights(shape) if weights is None else weights
    used, ignored = enc.load_state_dict(W)
    assert ignored == 0 and used == len(W)
    if calibrated:
        enc.set_calibration(calibration_table(shape))
    return enc


@contextlib.contextmanager
def options(opts):
    from mmiss_amd import _lib

    try:
        for k, v in opts:
            _lib.set_option(k, v)
        yield
    finally:
        for k, _ in opts:
            _lib.set_option(k, sc.OPTION_DEFAULTS[k])


def plan(enc, case, call, T=0):
    """The plan of one chunk, with the call's pinned fields asserted (the caller holds the call's options)."""
    from mmiss_amd import _lib

    tower = _lib.MMISS_TOWER_VISION if case.tower == "vision" else _lib.MMISS_TOWER_TEXT
    p = _lib.encoder_plan(enc._h, tower, call.B, T)
    for k, v in call.expect:
        assert p[k] == v, f"{case.name} {call.kind} B={call.B}: plan {k} = {p[k]!r}, the case wants {v!r} ({p})"
    assert p["prune"] == 1, (case.name, p)
    return p


def cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)

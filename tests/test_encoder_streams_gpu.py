"""The encoder on a caller's stream (mmiss_encoder_set_stream(h, stream, 0); every ClipEncoder.encode_* call on a CUDA tensor):
order, hand-over, equal bits. tests/encoder_stream_cases.py selects the calls from the sequence table (encoder_sequence_cases.py).

The reference of a call is the same handle on its OWN stream with numpy in and numpy out (held to the fp32 oracle at sc.COS_TOL
where the case has one). The kernels, the plan and the operands on a caller's stream are the same, only the stream differs: every
comparison is on bits. What the tests look for is order — a stage on another stream, a missing or a needless host wait, a
hand-over that waits for too little or too much, state changed under a queued call — so the caller's stream is kept busy with a
chain of matmuls (>= 100 ms, asserted from event times in every test that relies on it; an encode here takes well under that),
and whether an event behind the chain has been reached when a call returns tells whether the call waited.

Before any assertion about asynchrony the same call runs once on the same stream (first calls allocate: alloc_zero waits on the
null stream, the caching allocator may too), outputs are allocated ahead, and the launch profiler stays off. Every call asserts
its plan from mmiss_dbg_encoder_plan before it runs."""
import contextlib
import functools

import numpy as np
import pytest

import encoder_handles as eh
import encoder_sequence_cases as sc
import encoder_stream_cases as st

pytestmark = pytest.mark.gpu

_HANDLES = {}
_REFS = {}
P = 128      # proj_dim of every shape of the table


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    import torch

    torch.cuda.synchronize()
    for enc in _HANDLES.values():
        enc.close()
    _HANDLES.clear()
    _REFS.clear()


def _handle(case):
    key = (case.shape, case.tower, case.precision, case.max_batch, case.calibrated)
    if key not in _HANDLES:
        _HANDLES[key] = eh.new_handle(*key)
    return _HANDLES[key]


def _chunk_case():
    """sc.CHUNK_CASES' call of max_batch + r images as a case: the first chunk NaN, the victim is the last chunk."""
    via, max_batch, r = st.CHUNK
    plain = (("fold", 0), ("sfold", 0), ("fp8", 0), ("resid16", 0), ("embed", "Nothing"), ("qkv", "Tile"), ("pooled_tail", 0))
    head = sc.Call("nan", max_batch, expect=plain, via=via, seed=3)
    tail = sc.Call("victim", r, expect=plain, via=via, seed=r)
    return sc.Case(f"l-{via}-r{r}", "l", "tiny", "vision", tail, (head,), max_batch)


# ------------------------------------------------------------------------------------------------ one call
def _operands(case, call):
    """numpy operands as the wrapper takes them: (the array that may live on the device, further host arguments)."""
    from mmiss_amd.encoder import ClipEncoder

    if case.plan == "l":
        head = case.poisons[0]
        return np.concatenate([sc.call_input(case, head), sc.call_input(case, call)]), ()
    x = sc.call_input(case, call)
    if case.tower == "vision" and call.via == "rgb":
        blob, off, hs, ws = ClipEncoder._pack_rgb(x)
        return blob, (off, hs, ws)
    return x, ()


def _rows(case, call):
    return call.B + (case.max_batch if case.plan == "l" else 0)


def _assert_plan(enc, case, call, main):
    s = sc.SHAPES[case.shape]
    if case.tower == "text":
        T = int(main.shape[1])
        assert eh.plan(enc, case, call, T)["M"] == call.B * T, case.name
        return
    for c in ((case.poisons[0], call) if case.plan == "l" else (call,)):
        assert eh.plan(enc, case, c)["M"] == c.B * s.v_tokens, case.name


def _run(enc, case, call, main, extra=(), out=None):
    """One call through the Python wrapper under the call's options, its plan asserted before (both chunks' of the long call)."""
    with eh.options(call.opts):
        _assert_plan(enc, case, call, main)
        if case.tower == "text":
            return enc.encode_text(main, out=out, trim_padding=call.trim)
        if call.via == "rgb" and case.plan != "l":
            return enc.encode_image_rgb_packed(main, *extra, out=out)
        return enc.encode_image(main, out=out)


def _reference(case, call, enc=None):
    """The call on the handle's own stream, numpy in and out (float32 [rows, P], read-only); a victim with an oracle is held to it."""
    key = (case.shape, case.tower, case.precision, case.max_batch, case.calibrated, case.plan == "l", call) if enc is None else None
    if key is not None and key in _REFS:
        return _REFS[key]
    main, extra = _operands(case, call)
    ref = _run(_handle(case) if enc is None else enc, case, call, main, extra)
    assert isinstance(ref, np.ndarray) and ref.shape == (_rows(case, call), P)
    tail = ref[-call.B:]
    assert np.isfinite(tail).all(), case.name
    if case.plan == "l":
        assert np.isnan(ref[: case.max_batch]).all()
    if case.oracle and enc is None:
        d = (1 - eh.cos(tail, sc.oracle_embed(case, call))).max()
        assert d < sc.COS_TOL, f"{case.name}: the reference's 1 - cos vs the fp32 oracle {d:.3e}"
    ref.setflags(write=False)
    if key is not None:
        _REFS[key] = ref
    return ref


def _same_bits(got, ref, what):
    """got (CUDA tensor or array) against the reference: the same bits in every finite row, NaN where the reference is NaN (the
    first chunk of the long call)."""
    got = got.cpu().numpy() if hasattr(got, "is_cuda") else np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref).all(axis=1)
    assert np.isnan(got[nan]).all(), what
    bad = np.flatnonzero((eh.bits(got[~nan]) != eh.bits(ref[~nan])).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {int((~nan).sum())} rows differ from the reference bits, first {bad[:8].tolist()}; finite "
                           f"{bool(np.isfinite(got[~nan]).all())}, max |diff| {np.nanmax(np.abs(got[~nan] - ref[~nan])):.3e}")


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _decoy(case, call, main):
    """What the input buffer holds before the caller's producer has run: NaN pixels, a twin batch on the integer routes, prompts
    of the NaN token."""
    if case.tower == "text":
        return np.full_like(main, sc.NAN_ID)
    if main.dtype == np.float32:
        return np.full_like(main, np.nan)
    twin = _operands(case, sc.Call("twin", call.B, via=call.via, seed=3))[0]
    assert twin.shape == main.shape and not np.array_equal(twin, main)
    return twin


# ------------------------------------------------------------------------------------------------ the delay
@functools.lru_cache(maxsize=None)
def _chain_length():
    """how many 4096^3 matmuls run for 200 ms on this GPU (timed with events, after a warm-up)"""
    import torch

    a, out = _chain_operands()
    for _ in range(3):
        torch.mm(a, a, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(8):
        torch.mm(a, a, out=out)
    e1.record()
    e1.synchronize()
    per = e0.elapsed_time(e1) / 8
    return int(np.ceil(200.0 / per))


@functools.lru_cache(maxsize=None)
def _chain_operands():
    import torch

    a = torch.full((4096, 4096), 1.0 / 4096, device="cuda")
    out = torch.empty_like(a)
    torch.cuda.synchronize()
    return a, out


class _Delay:
    """A chain of matmuls on the current stream between two timed events; `end` sits behind it."""

    def __init__(self, part=1.0):
        import torch

        self.n = max(1, int(_chain_length() * part))
        self.begin, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def queue(self):
        import torch

        a, out = _chain_operands()
        self.begin.record()
        for _ in range(self.n):
            torch.mm(a, a, out=out)
        self.end.record()
        return self

    def reached(self):
        return self.end.query()

    def check(self):
        """no test passes because the delay was absent: the chain took at least 100 ms"""
        self.end.synchronize()
        ms = self.begin.elapsed_time(self.end)
        print(f"chain of {self.n} matmuls: {ms:.1f} ms")
        assert ms >= 100.0, ms
        return ms


def _side_stream():
    import torch

    _chain_length()
    torch.cuda.synchronize()
    return torch.cuda.Stream()


def _stream_apart_from_the_own(enc, case, call):
    """A torch stream that shares no hardware queue with the handle's own stream. The runtime deals a process's streams onto a few
    hardware queues and takes the packets of one queue in order (the index's side stream): a synchronous call on the
    own stream returns behind a chain on a stream dealt to the same queue, whatever the handle does. Probed with the call
    itself, numpy in and out, beside a quarter chain."""
    import torch

    main, extra = _operands(case, call)
    tried = []
    for _ in range(8):
        s = torch.cuda.Stream()
        tried.append(s)
        with torch.cuda.stream(s):
            d = _Delay(0.25).queue()
            _run(enc, case, call, main, extra)
            shared = d.reached()
            d.end.synchronize()
        if not shared:
            return s
    pytest.fail(f"{case.name}: a synchronous call on the handle's own stream returned behind the caller's chain on each of 8 streams")


# ------------------------------------------------------------------------------------------------ (a) every route, same bits
def _route(case, call, io):
    import torch

    enc = _handle(case)
    ref = _reference(case, call)
    main, extra = _operands(case, call)
    x = _dev(main)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if io == "stream" else None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        for i in range(2):      # the second call is timed: the first may allocate
            e0.record()
            out = _run(enc, case, call, x, extra)
            e1.record()
            assert out.is_cuda and tuple(out.shape) == ref.shape
            _same_bits(out, ref, f"{case.name} via {call.via} on {io}, call {i}")
        print(f"encode {case.name} via {call.via} on {io}: {e0.elapsed_time(e1):.3f} ms")
    torch.cuda.synchronize()


@pytest.mark.parametrize("io", ("default", "stream"))
@pytest.mark.parametrize("name", st.ROUTE_NAMES)
def test_every_route_returns_the_own_streams_bits(name, io):
    case = st.case(name)
    _route(case, case.victim, io)


@pytest.mark.parametrize("io", ("default", "stream"))
@pytest.mark.parametrize("name,via", st.INT_ROUTES, ids=lambda v: str(v))
def test_integer_input_routes_return_the_own_streams_bits(name, via, io):
    case = st.case(name)
    _route(case, st.via_call(case, via), io)


@pytest.mark.parametrize("io", ("default", "stream"))
def test_a_call_longer_than_max_batch_returns_the_own_streams_bits(io):
    case = _chunk_case()
    _route(case, case.victim, io)


# ------------------------------------------------------------------------------------------------ (b) behind the caller's producer
def _order_cases():
    out = [(st.case(n), st.via_call(st.case(n), via) if st.case(n).tower == "vision" else st.case(n).victim) for n, via in st.ORDER]
    chunk = _chunk_case()
    return out + [(chunk, chunk.victim)]


@pytest.mark.parametrize("case,call", _order_cases(), ids=lambda v: v.name if isinstance(v, sc.Case) else v.via)
def test_the_call_is_ordered_behind_the_callers_producer(case, call):
    """The input buffer holds NaN (a twin batch, NaN-token prompts) until a copy queued on the caller's stream behind the chain fills
    it; the encode is queued behind the copy and a clone of its output behind the encode, the host touches nothing. The call
    returns while the chain runs; the clone holds the reference bits: no stage ran on another stream (it would have read the
    decoy, or been read too early)."""
    import torch

    enc = _handle(case)
    ref = _reference(case, call)
    main, extra = _operands(case, call)
    real, decoy = _dev(main), _dev(_decoy(case, call, main))
    s = _side_stream()
    with torch.cuda.stream(s):
        buf = torch.empty_like(real)
        buf.copy_(decoy)
        # the warm-up call runs on the decoy: every workspace of the handle then holds what the decoy gives, not the answer
        warm = _run(enc, case, call, buf, extra).cpu().numpy()
        assert not np.array_equal(eh.bits(warm[-call.B:]), eh.bits(ref[-call.B:]))
        out = torch.zeros(ref.shape, dtype=torch.float32, device="cuda")
        kept = torch.zeros_like(out)
        s.synchronize()
        delay = _Delay().queue()
        buf.copy_(real)
        got = _run(enc, case, call, buf, extra, out=out)
        waited = delay.reached()
        kept.copy_(got)
        s.synchronize()
    assert got is out
    assert not waited, f"{case.name}: the call returned only after the caller's earlier work had run"
    _same_bits(kept, ref, f"{case.name} via {call.via} behind the producer")
    delay.check()


# ------------------------------------------------------------------------------------------------ (c) no drain
@pytest.mark.parametrize("name", st.NO_DRAIN)
def test_the_callers_stream_is_not_drained(name):
    """Two calls on one stream with the caller's chain and an event E between them: the second call returns before E."""
    import dataclasses

    import torch

    case = st.case(name)
    calls = (case.victim, dataclasses.replace(case.victim, seed=case.victim.seed + 1000))
    enc = _handle(case)
    refs = [_reference(case, c) for c in calls]
    assert not np.array_equal(eh.bits(refs[0]), eh.bits(refs[1]))
    xs = [_dev(_operands(case, c)[0]) for c in calls]
    s = _side_stream()
    with torch.cuda.stream(s):
        _same_bits(_run(enc, case, calls[1], xs[1]), refs[1], name + ": warm-up")      # (the other input: call 0 runs over its state)
        outs = [torch.zeros(refs[0].shape, dtype=torch.float32, device="cuda") for _ in calls]
        s.synchronize()
        _run(enc, case, calls[0], xs[0], out=outs[0])
        delay = _Delay().queue()
        _run(enc, case, calls[1], xs[1], out=outs[1])
        waited = delay.reached()
        s.synchronize()
    assert not waited, f"{name}: the second call waited for what the caller queued behind the first"
    for out, ref, i in zip(outs, refs, range(2)):
        _same_bits(out, ref, f"{name}: call {i}")
    delay.check()


# ------------------------------------------------------------------------------------------------ (d) host operands
def _abi_call(enc, case, call, x, out):
    """mmiss_encode_image / _text through the C ABI on the stream the handle is set to (x, out: tensors or arrays)."""
    from mmiss_amd import _lib

    lib = _lib.load()
    with eh.options(call.opts):
        _assert_plan(enc, case, call, x)
        if case.tower == "text":
            _lib.check(lib.mmiss_encode_text(enc._h, _lib.ptr(x), call.B, int(x.shape[1]), _lib.ptr(out)))
        else:
            _lib.check(lib.mmiss_encode_image(enc._h, _lib.ptr(x), call.B, _lib.ptr(out)))


def _host_array(like, memory):
    """A host array shaped like `like` (a copy of it), pageable or pinned; pinned: (array view, the tensor that owns it). The
    runtime finishes a copy from or to PAGEABLE memory before hipMemcpyAsync returns or behind a wait of its own; only with pinned
    memory is the copy as asynchronous as a kernel, and the call's own host wait the only thing in front of the caller."""
    import torch

    if memory == "pageable":
        return like.copy(), None
    t = torch.from_numpy(like.copy()).pin_memory()
    assert t.is_pinned()
    return t.numpy(), t


@pytest.mark.parametrize("memory", ("pageable", "pinned"))
@pytest.mark.parametrize("name", st.HOST_OPERANDS)
def test_host_operands_on_a_callers_stream(name, memory):
    """use_own == 0 with an operand in host memory (the Python wrapper never does this): the call synchronises. Device in, host
    out: the host buffer holds the reference bits at return, although the chain was queued in front. Host in, device out: the
    output is complete at return (read on a stream that never waited on the caller's) and the host input may be overwritten."""
    import torch

    from mmiss_amd import _lib

    case = st.case(name)
    call = case.victim
    enc = _handle(case)
    ref = _reference(case, call)
    main, _ = _operands(case, call)
    x = _dev(main)
    s = _side_stream()
    lib = _lib.load()
    with enc._call_lock:
        try:
            _lib.check(lib.mmiss_encoder_set_stream(enc._h, s.cuda_stream, 0))
            with torch.cuda.stream(s):
                host, _keep = _host_array(np.zeros(ref.shape, np.float32), memory)
                _abi_call(enc, case, call, x, host)                                  # warm-up
                _same_bits(host, ref, name + ": warm-up")
                host[...] = np.nan
                delay = _Delay().queue()
                _abi_call(enc, case, call, x, host)
                got = host.copy()
                assert delay.reached(), name + ": a host output, and the call returned with the stream still running"
                _same_bits(got, ref, name + ": device in, host out, at return")
                delay.check()

                hx, _keep_in = _host_array(main, memory)
                out = torch.zeros(ref.shape, dtype=torch.float32, device="cuda")
                s.synchronize()
                delay = _Delay().queue()
                _abi_call(enc, case, call, hx, out)
                hx[...] = sc.NAN_ID if case.tower == "text" else np.nan              # the host input is the caller's again
                with torch.cuda.stream(torch.cuda.Stream()):
                    got = out.cpu().numpy()
                _same_bits(got, ref, name + ": host in, device out, at return")
                delay.check()
        finally:
            _lib.check(lib.mmiss_encoder_set_stream(enc._h, None, 1))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (e) hand-over between streams
@pytest.mark.parametrize("second", ("stream", "numpy"))
@pytest.mark.parametrize("name", st.HANDOVER)
def test_handover_waits_for_the_last_call_and_for_nothing_else(name, second):
    """s1: chain, X1 (returns at once), a second chain, E2. Then a NaN poison that covers X1's rows on s2, which waits on nothing
    (or as a numpy call, on the handle's own stream): changing the stream waits for X1 — the first chain has run when the poison
    call returns, X1's output is the reference — and for nothing else: E2 is not reached. A later victim behind the poison
    holds its reference bits too."""
    import torch

    case = st.case(name)
    x1, poison, x2 = st.handover_calls(case)
    enc = _handle(case)
    ref1, ref2 = _reference(case, x1), _reference(case, x2)
    assert not np.array_equal(eh.bits(ref1), eh.bits(ref2))
    h1, hp, h2 = (_operands(case, c)[0] for c in (x1, poison, x2))
    d1, dp, d2 = _dev(h1), _dev(hp), _dev(h2)
    _chain_length()
    s1 = _stream_apart_from_the_own(enc, case, x1) if second == "numpy" else _side_stream()
    s2 = torch.cuda.Stream()
    pshape = (poison.B, P)
    with torch.cuda.stream(s1):                                                        # warm-up of the three calls
        _same_bits(_run(enc, case, x1, d1), ref1, name + ": warm-up")
    with torch.cuda.stream(s2):
        _run(enc, case, poison, dp if second == "stream" else hp)
        _same_bits(_run(enc, case, x2, d2 if second == "stream" else h2), ref2, name + ": warm-up")
    out1 = torch.zeros(ref1.shape, dtype=torch.float32, device="cuda")
    out2 = torch.zeros(ref2.shape, dtype=torch.float32, device="cuda")
    outp = torch.zeros(pshape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        first = _Delay().queue()
        _run(enc, case, x1, d1, out=out1)
        x1_waited = first.reached()
        behind = _Delay().queue()                                                      # E2 = behind.end
    with torch.cuda.stream(s2):
        if second == "stream":
            _run(enc, case, poison, dp, out=outp)
        else:
            _run(enc, case, poison, hp)
        x1_done, e2_reached = first.reached(), behind.reached()
        got2 = _run(enc, case, x2, d2, out=out2) if second == "stream" else _run(enc, case, x2, h2)
    torch.cuda.synchronize()
    assert not x1_waited, name + ": X1 did not return at once"
    assert x1_done, name + ": the hand-over did not wait for X1 (the chain in front of it was still running)"
    assert not e2_reached, name + ": the hand-over waited for what the caller queued behind X1"
    _same_bits(out1, ref1, name + ": X1 under the poison")
    _same_bits(got2, ref2, name + ": the later victim")
    first.check()
    behind.check()


@pytest.mark.parametrize("name", st.HANDOVER)
def test_ping_pong_between_streams(name):
    """Victims alternate s1, s2, s1, s2 with a poison on a third stream between each pair, a short chain in front of every call so
    that its work is still queued when the next call arrives: every call is a hand-over, every victim the reference bits."""
    import torch

    case = st.case(name)
    x1, poison, x2 = st.handover_calls(case)
    enc = _handle(case)
    refs = {x1: _reference(case, x1), x2: _reference(case, x2)}
    dev = {c: _dev(_operands(case, c)[0]) for c in (x1, poison, x2)}
    s1, s2, s3 = _side_stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for s, c in ((s1, x1), (s3, poison), (s2, x2)):                                   # warm-up
        with torch.cuda.stream(s):
            _run(enc, case, c, dev[c])
    outp = torch.zeros((poison.B, P), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    results = []
    for s, c in ((s1, x1), (s3, poison), (s2, x2), (s3, poison), (s1, x2), (s3, poison), (s2, x1)):
        with torch.cuda.stream(s):
            _Delay(0.1).queue()
            if c is poison:
                _run(enc, case, c, dev[c], out=outp)
            else:
                results.append((c, _run(enc, case, c, dev[c], out=torch.zeros(refs[c].shape, dtype=torch.float32, device="cuda"))))
    torch.cuda.synchronize()
    for i, (c, out) in enumerate(results):
        _same_bits(out, refs[c], f"{name}: victim {i}")


# ------------------------------------------------------------------------------------------------ (f) state behind a queued encode
def _queued_then(case_before, case_after, enc, change, ref_before, ref_after):
    """chain, an encode of case_before's victim queued behind it, `change(enc)` on the host without waiting, the same pixels
    again: the queued call's output is what the OLD state gives, the following call's what the new one gives."""
    import torch

    call, after = case_before.victim, case_after.victim
    main, _ = _operands(case_before, call)
    assert main.tobytes() == _operands(case_after, after)[0].tobytes()
    assert not np.array_equal(eh.bits(ref_before), eh.bits(ref_after))
    x = _dev(main)
    s = _side_stream()
    with torch.cuda.stream(s):
        _same_bits(_run(enc, case_before, call, x), ref_before, case_before.name + ": warm-up")
        out1 = torch.zeros(ref_before.shape, dtype=torch.float32, device="cuda")
        out2 = torch.zeros_like(out1)
        s.synchronize()
        delay = _Delay().queue()
        _run(enc, case_before, call, x, out=out1)
        waited = delay.reached()
        change(enc)
        _run(enc, case_after, after, x, out=out2)
        s.synchronize()
    assert not waited
    _same_bits(out1, ref_before, case_before.name + ": the call queued before the change")
    _same_bits(out2, ref_after, case_after.name + ": the call after the change")
    delay.check()


def test_weights_loaded_behind_a_queued_encode():
    """load_state_dict(W2) while an encode under W1 is still queued on the caller's stream: mmiss_encoder_set_weight converts
    into the live weight buffers on the handle's own stream, so it first waits for the handle's last call (and for nothing
    else). The queued call gives W1's bits, the next one W2's (a fresh handle's)."""
    case = st.case(st.WEIGHTS_CASE)
    W2 = st.weights2(case.shape)
    fresh = eh.new_handle(case.shape, case.tower, case.precision, case.max_batch, weights=W2)
    try:
        ref2 = _reference(case, case.victim, enc=fresh)
    finally:
        fresh.close()
    enc = eh.new_handle(case.shape, case.tower, case.precision, case.max_batch)
    try:
        _queued_then(case, case, enc, lambda e: e.load_state_dict(W2), _reference(case, case.victim), ref2)
    finally:
        enc.close()


def test_precision_set_behind_a_queued_encode():
    after = st.case(st.PRECISION_CASE)
    before = st.bf16_twin_of(after)
    enc = eh.new_handle(before.shape, before.tower, "bf16", before.max_batch)
    try:
        _queued_then(before, after, enc, lambda e: e.set_precision("fp8"), _reference(before, before.victim), _reference(after, after.victim))
    finally:
        enc.close()


def test_calibration_set_behind_a_queued_encode():
    after = st.case(st.CALIBRATION_CASE)
    before = st.case(st.PRECISION_CASE)       # the same call, fp8, uncalibrated
    assert before.victim.opts == after.victim.opts and not before.calibrated and after.calibrated
    enc = eh.new_handle(before.shape, before.tower, "fp8", before.max_batch)
    try:
        _queued_then(before, after, enc, lambda e: e.set_calibration(eh.calibration_table(after.shape)), _reference(before, before.victim),
                     _reference(after, after.victim))
    finally:
        enc.close()

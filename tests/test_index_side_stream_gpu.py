"""The split query (mmiss_index_query_begin / _end) with its widen pass on the handle's side stream: option query_side_stream = 1
(the default) and = 0 (everything on the handle's stream, the routing before the side stream existed) must hand back the same
labels, distance bits and counts, equal to the synchronous query() and to the C oracle, with the same guard accounting — on
every route of the widen pass, with work of the caller's queued between the two halves.

The indexes are CLUSTERED (rows unit(c + 0.02 noise), queries rows of the index): the first pass cannot prove any such query,
so every one is widened; each test asserts that from guard_stats(), otherwise the widen pass would not have run at all."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
MODES = (1, 0)
STAT_KEYS = ("queries", "widened", "rounds", "pages", "exhaustive", "swept_rows")


@pytest.fixture(scope="module")
def mods():
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib
    from mmiss_amd.index import FlatIndex
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    return FlatIndex, ro, roc, _lib


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _cluster(N, D, seed):
    """rows unit(c + 0.02 noise) around one centre c ~ N(0, 1)^D; never modified"""
    rng = np.random.Generator(np.random.Philox(seed))
    c = rng.standard_normal((1, D), dtype=np.float32)
    rows = _unit(c + 0.02 * rng.standard_normal((N, D), dtype=np.float32))
    rows.setflags(write=False)
    return rows, c


def _labels(N):
    return np.arange(N, dtype=np.int64) * 3 + 7


_INDEXES = {}


def _index(mods, dtype, D, N):
    """one clustered index per (dtype, D, N) for the whole module -> (handle, rows, stored rows as the oracle reads them, labels)"""
    FlatIndex, ro, _, _ = mods
    key = (dtype, D, N)
    if key not in _INDEXES:
        rows, _ = _cluster(N, D, seed=D + N)
        idx = FlatIndex(D, dtype, capacity=N)
        idx.add(rows, _labels(N))
        _INDEXES[key] = (idx, rows, ro.normalize_rows(rows, dtype), _labels(N))
    return _INDEXES[key]


def _host(res):
    return tuple(a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a) for a in res)


def _same(got, exp, what):
    np.testing.assert_array_equal(got[2], exp[2], err_msg=f"{what}: counts")
    np.testing.assert_array_equal(got[0], exp[0], err_msg=f"{what}: labels")
    np.testing.assert_array_equal(got[1].view(np.uint32), exp[1].view(np.uint32), err_msg=f"{what}: distance bits")


def _delta(idx, before):
    after = idx.guard_stats()
    return {key: after[key] - before[key] for key in STAT_KEYS}


def _busy(n=6, size=1024):
    """the caller's own work between the two halves: a short chain of matmuls on the current torch stream"""
    import torch

    a = torch.full((size, size), 1.0 / size, device="cuda")
    for _ in range(n):
        a = a @ a
    return a


def _split(_lib, idx, make_q, mode, between=None, stream=None, **masks):
    """query_begin, the caller's work, result() under query_side_stream = mode -> (host results, guard_stats delta)"""
    import contextlib

    import torch

    _lib.set_option("query_side_stream", mode)
    try:
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            before = idx.guard_stats()
            qin = make_q()
            h = idx.query_begin(qin, K, **masks)
            keep = between(qin) if between is not None else _busy()
            res = h.result()
            out = _host(res)      # (a device-to-host copy on the caller's stream: behind whatever `between` queued)
            del keep
        return out, _delta(idx, before)
    finally:
        _lib.set_option("query_side_stream", 1)


def _all_routes(mods, idx, q, exp, flagged, io="stream", between=None, masks=None, min_exhaustive=0):
    """The assertions of every case: the split query under modes 1 and 0 and the synchronous query() all equal `exp` (the C
    oracle's answer), `flagged` of the queries were widened on each (at least min_exhaustive of them by the exhaustive pass; 0:
    none), and the guard accounting is the same on all routes.
    io: 'numpy' (host buffers, the handle's own stream), 'default' (CUDA tensors on torch's default stream), 'stream' (CUDA
    tensors on a torch stream of the test's)."""
    import torch

    _, _, _, _lib = mods
    masks = masks or {}
    stream = torch.cuda.Stream() if io == "stream" else None
    make_q = (lambda: q.copy()) if io == "numpy" else (lambda: torch.from_numpy(q.copy()).cuda())
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    deltas = {}
    for mode in MODES:
        got, deltas[mode] = _split(_lib, idx, make_q, mode, between, stream, **masks)
        _same(got, exp, f"query_side_stream = {mode}")
    before = idx.guard_stats()
    got = _host(idx.query(make_q(), K, **masks))
    deltas["query()"] = _delta(idx, before)
    _same(got, exp, "query()")
    torch.cuda.synchronize()
    for route, d in deltas.items():
        assert d["queries"] == q.shape[0] and d["widened"] == flagged, (route, d)
        assert d["exhaustive"] >= min_exhaustive and (min_exhaustive > 0 or d["exhaustive"] == 0), (route, d)
        assert d == deltas[0], (route, d, deltas[0])
    return deltas[0]


@functools.lru_cache(maxsize=None)
def _expected(dtype, D, N, Q):
    """Q queries, every (N // Q)-th row of the clustered index, and the oracle's answer: computed once per shape, never modified"""
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    rows, _ = _cluster(N, D, seed=D + N)
    q = np.ascontiguousarray(rows[:: N // Q][:Q])
    out = roc.query(q, ro.normalize_rows(rows, dtype), _labels(N), K)
    for a in out + (q,):
        a.setflags(write=False)
    return q, out


# the smallest shapes that reach each route of the widen pass: the GEMM threshold pass needs D % 128 == 0, D >= 256 and more
# than 64 flagged queries (f16 and fp8 rows), below that and for f32 rows it is the streaming scan
SHAPES = [("f16", 256, 3000, 65, "sweep_gemm_f16"), ("f16", 256, 3000, 256, "sweep_gemm_f16"),
          ("f16", 256, 3000, 5, "sweep_scan_f16"), ("f16", 256, 3000, 64, "sweep_scan_f16"),
          ("f32", 128, 2000, 20, "sweep_scan_f32"), ("f8", 256, 3000, 65, "sweep_gemm_f8")]


@pytest.mark.parametrize("io", ["numpy", "default", "stream"])
@pytest.mark.parametrize("dtype,D,N,Q,kernel", SHAPES)
def test_every_route_returns_the_same_bits(mods, dtype, D, N, Q, kernel, io):
    """Case 1: host outputs on the handle's own stream, device outputs on torch's default stream and on a stream of the caller's."""
    _, _, _, _lib = mods
    idx = _index(mods, dtype, D, N)[0]
    q, exp = _expected(dtype, D, N, Q)
    _all_routes(mods, idx, q, exp, flagged=Q, io=io)
    # the route itself: which threshold pass ran
    _lib.prof_filter(None, 1); _lib.prof_reset(); _lib.prof_enable(True)
    try:
        idx.query_begin(q.copy(), K).result()
    finally:
        _lib.prof_enable(False)
    kern = {p["kernel"] for p in _lib.prof_read()}
    assert kernel in kern, kern


@functools.lru_cache(maxsize=None)
def _chain_length():
    """how many 4096^3 matmuls run for 200 ms on this GPU (timed with events, after a warm-up)"""
    import torch

    a = torch.full((4096, 4096), 1.0 / 4096, device="cuda")
    out = torch.empty_like(a)
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


@pytest.mark.parametrize("mode", MODES)
def test_query_end_does_not_drain_the_callers_stream(mods, mode):
    """Case 2: behind query_begin the caller queues >= 100 ms of matmuls and an event E on its stream. With the widen pass on the
    side stream result() returns while they run (E not reached); with query_side_stream = 0 the widen pass sits behind them on
    the caller's stream and result() returns only after E — the switch does something. (This is also what holds the side
    stream to a hardware queue that callers' streams do not share: on a shared queue result() waits for the chain.)"""
    import torch

    _, _, _, _lib = mods
    dtype, D, N, Q = "f16", 256, 3000, 256
    idx = _index(mods, dtype, D, N)[0]
    q, exp = _expected(dtype, D, N, Q)
    n = _chain_length()
    a = torch.full((4096, 4096), 1.0 / 4096, device="cuda")
    out = torch.empty_like(a)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    s0, E = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    _lib.set_option("query_side_stream", mode)
    try:
        with torch.cuda.stream(stream):
            before = idx.guard_stats()
            h = idx.query_begin(torch.from_numpy(q.copy()).cuda(), K)
            s0.record()
            for _ in range(n):
                torch.mm(a, a, out=out)
            E.record()
            res = h.result()
            reached = E.query()
            assert _delta(idx, before)["widened"] == Q
            if mode == 0:
                assert reached, "query_side_stream = 0: the widen pass runs behind the caller's work"
            else:
                assert not reached, "query_end waited for the work the caller queued behind query_begin"
            with torch.cuda.stream(torch.cuda.Stream()):      # read the results WITHOUT the caller's stream: they are complete
                got = _host(res)
            _same(got, exp, f"query_side_stream = {mode}")
            E.synchronize()
            assert s0.elapsed_time(E) >= 100.0, s0.elapsed_time(E)
    finally:
        _lib.set_option("query_side_stream", 1)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype,D,N,Q", [("f16", 256, 3000, 256), ("f16", 256, 3000, 5), ("f32", 128, 2000, 20)])
def test_the_query_buffer_may_be_overwritten_behind_begin(mods, dtype, D, N, Q):
    """Case 3: prep_queries_kernel is the only reader of the caller's buffer; what the caller queues behind query_begin may
    overwrite it (the next batch's encode does), and the widen pass on the side stream must not read it again. Here: NaN."""
    idx = _index(mods, dtype, D, N)[0]
    q, exp = _expected(dtype, D, N, Q)

    def poison(qin):
        qin.fill_(float("nan"))
        return _busy()

    for io in ("default", "stream"):
        _all_routes(mods, idx, q, exp, flagged=Q, io=io, between=poison)


@functools.lru_cache(maxsize=None)
def _mixed(D, n_cluster, n_far):
    """a cluster and, on the other side of the origin, n_far scattered rows: cosine -0.3 to the cluster's centre, random among
    themselves, so a query that is one of them is proven by the first pass (its k nearest are spread far wider than eps)"""
    rng = np.random.Generator(np.random.Philox(77))
    rows, c = _cluster(n_cluster, D, seed=78)
    ch = _unit(c)
    g = rng.standard_normal((n_far, D), dtype=np.float32)
    g -= (g @ ch.T) * ch
    far = _unit(_unit(g) * np.float32(np.sqrt(1 - 0.09)) - np.float32(0.3) * ch)
    allr = np.concatenate([rows, far])
    allr.setflags(write=False)
    return allr


@pytest.mark.parametrize("filtered", [False, True])
def test_mixed_batch_compacts_the_flagged_queries(mods, filtered):
    """Case 4: half the queries proven by the first pass, half flagged: the widen pass gathers the flagged ones (65: the GEMM
    threshold pass unfiltered, the scan's filtered form with require / exclude) and writes their rows of the outputs only."""
    FlatIndex, ro, roc, _ = mods
    D, NC, NF, H = 256, 1500, 1500, 65
    rows = _mixed(D, NC, NF)
    N = NC + NF
    labels = _labels(N)
    idx = FlatIndex(D, "f16", capacity=N)
    idx.add(rows, labels)
    tags = (np.arange(N) % 4 == 0).astype(np.uint64) | ((np.arange(N) % 7 == 0).astype(np.uint64) << np.uint64(1))
    idx.set_tags(labels, tags)
    # queries: alternately a cluster row and a far row, all of them admitted by the filter (rows % 28 in {4, 8, ...}: tag 1)
    pick_c = np.arange(4, NC, 4)[np.arange(4, NC, 4) % 7 != 0][:H]
    pick_f = NC + np.arange(0, NF, 4)
    pick_f = pick_f[(pick_f % 4 == 0) & (pick_f % 7 != 0)][:H]
    assert len(pick_c) == H and len(pick_f) == H
    sel = np.stack([pick_c, pick_f], 1).reshape(-1)
    q = np.ascontiguousarray(rows[sel])
    stored = ro.normalize_rows(rows, "f16")
    masks = None
    sub = np.arange(N)
    if filtered:
        masks = {"require": 1, "exclude": 2}
        sub = np.nonzero((tags & np.uint64(1) == 1) & (tags & np.uint64(2) == 0))[0]
    exp = roc.query(q, stored[sub], labels[sub], K)
    assert (exp[0][:, 0] == labels[sel]).all()
    _all_routes(mods, idx, q, exp, flagged=H, masks=masks)
    idx.close()


@pytest.mark.parametrize("D,copies,exhaustive", [(256, 1500, 0), (128, 9000, 1)])
def test_long_lists_take_the_second_rerank_and_the_exhaustive_pass(mods, D, copies, exhaustive):
    """Case 5: a plateau of 1500 copies of one row (more than the first re-rank launch sorts: the second, larger launch) and of
    9000 (more than a list holds: the exhaustive canonical pass), with the caller's work queued between the two halves."""
    FlatIndex, ro, roc, _ = mods
    NC = 600
    crows, _ = _cluster(NC, D, seed=5 + D)
    rows = np.concatenate([crows, np.repeat(crows[:1], copies, 0)])
    N = rows.shape[0]
    labels = _labels(N)
    idx = FlatIndex(D, "f16", capacity=N)
    idx.add(rows, labels)
    q = np.ascontiguousarray(rows[[0, 300, NC + 5]])    # the plateau's row twice over, and a cluster row beside it
    exp = roc.query(q, ro.normalize_rows(rows, "f16"), labels, K)
    # (the two plateau queries for certain; the cluster row too when the plateau reaches its top-k: 9001 ties at one distance)
    d = _all_routes(mods, idx, q, exp, flagged=3, min_exhaustive=2 * exhaustive)
    if not exhaustive:
        assert d["swept_rows"] >= 2 * copies, d      # both plateau queries re-ranked the whole plateau
    idx.close()


def test_abort_and_stream_switch(mods):
    """Case 6: a query given up between the halves leaves nothing behind on the side stream that the next query trips over; a
    handle switched to another torch stream between two split queries answers both."""
    import torch

    _, _, _, _lib = mods
    dtype, D, N = "f16", 256, 3000
    idx = _index(mods, dtype, D, N)[0]
    q, exp = _expected(dtype, D, N, 65)
    q2, exp2 = _expected(dtype, D, N, 64)
    for mode in MODES:
        _lib.set_option("query_side_stream", mode)
        try:
            qt = torch.from_numpy(q2.copy()).cuda()
            h = idx.query_begin(qt, K)
            _busy()
            idx.abort_query()
            with pytest.raises(RuntimeError, match="aborted"):
                h.result()
            _same(_host(idx.query(torch.from_numpy(q.copy()).cuda(), K)), exp, f"query() after an abort, mode {mode}")
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            s1.wait_stream(torch.cuda.current_stream()); s2.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s1):
                h1 = idx.query_begin(torch.from_numpy(q.copy()).cuda(), K)
                _busy()
                r1 = _host(h1.result())
            with torch.cuda.stream(s2):
                h2 = idx.query_begin(torch.from_numpy(q2.copy()).cuda(), K)
                _busy()
                r2 = _host(h2.result())
            _same(r1, exp, f"first stream, mode {mode}")
            _same(r2, exp2, f"second stream, mode {mode}")
        finally:
            _lib.set_option("query_side_stream", 1)
    torch.cuda.synchronize()


def test_two_handles_open_on_one_stream_ended_in_reverse(mods):
    """Case 7: every handle has a side stream of its own; two queries open at once on one caller's stream do not meet."""
    import torch

    _, _, _, _lib = mods
    ia = _index(mods, "f16", 256, 3000)[0]
    ib = _index(mods, "f32", 128, 2000)[0]
    qa, ea = _expected("f16", 256, 3000, 65)
    qb, eb = _expected("f32", 128, 2000, 20)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for mode in MODES:
        _lib.set_option("query_side_stream", mode)
        try:
            with torch.cuda.stream(stream):
                ba, bb = ia.guard_stats(), ib.guard_stats()
                ha = ia.query_begin(torch.from_numpy(qa.copy()).cuda(), K)
                hb = ib.query_begin(torch.from_numpy(qb.copy()).cuda(), K)
                _busy()
                rb = _host(hb.result())
                ra = _host(ha.result())
                assert _delta(ia, ba)["widened"] == 65 and _delta(ib, bb)["widened"] == 20
            _same(ra, ea, f"first handle, mode {mode}")
            _same(rb, eb, f"second handle, mode {mode}")
        finally:
            _lib.set_option("query_side_stream", 1)
    torch.cuda.synchronize()


def test_a_small_query_behind_a_large_one_does_not_see_its_lists(mods):
    """Case 8: the scratch of a Q = 256 split query (lists, counts, maps) is what a Q = 3 split query on the same handle finds."""
    _, _, _, _lib = mods
    dtype, D, N = "f16", 256, 3000
    idx = _index(mods, dtype, D, N)[0]
    q, exp = _expected(dtype, D, N, 256)
    q3 = np.ascontiguousarray(q[[200, 17, 255]])
    e3 = tuple(a[[200, 17, 255]] for a in exp)
    for io in ("numpy", "stream"):
        _all_routes(mods, idx, q, exp, flagged=256, io=io)
        _all_routes(mods, idx, q3, e3, flagged=3, io=io)
        # and back to back under every mode, with nothing else on the handle in between
        for mode in MODES:
            make = (lambda a: (lambda: a.copy())) if io == "numpy" else (lambda a: (lambda: __import__("torch").from_numpy(a.copy()).cuda()))
            got, _ = _split(_lib, idx, make(q), mode)
            _same(got, exp, f"Q = 256, mode {mode}")
            got, d = _split(_lib, idx, make(q3), mode)
            _same(got, e3, f"Q = 3 behind Q = 256, mode {mode}")
            assert d["widened"] == 3, d

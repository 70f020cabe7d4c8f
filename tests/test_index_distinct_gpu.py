"""mmiss_index_query_distinct (and FlatIndex.query_distinct over it) against the restatement in tests/distinct_cases.py: the list
of the flat / filtered / probed query, sep by the oracle with the kept row as the query, the greedy walk. Every comparison is
equality of every element: labels, distance bits, counts, dups and listed. The edges that depend on the kernel's layout — the list
positions a workgroup takes per trip — are read from mmiss_dbg_index_distinct_plan. One test checks the result with calls the library
had before (query, query_radius_by_label) and no oracle at all."""
import numpy as np
import pytest

import distinct_cases as dc
import partition_cases as pc
from index_query_cases import load_mods

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5          # include/mmiss.h
MAX_DIM = {"f32": 1920, "f16": 3968, "f8": 3968}
SEP = dc.MIN_SEP


@pytest.fixture(scope="module")
def mods():
    return load_mods()


_indexes = {}


def index_of(mods, dtype, N=3000, dim=128):
    """the corpus in an index, once per (dtype, N, dim): the tests only read it"""
    key = (dtype, N, dim)
    if key not in _indexes:
        c = dc.corpus(N, dim)
        idx = mods[0](dim, dtype)
        idx.add(c.rows, c.labels)
        idx.set_tags(c.labels, c.tags)
        _indexes[key] = idx
    return _indexes[key]


def plan(mods, idx, Q=1):
    return mods[3].index_distinct_plan(idx._h, Q)


def raw(mods, idx, q, k, pool, min_sep, nprobe, lab, dist, cnt, dups, listed, req=None, exc=None):
    """mmiss_index_query_distinct itself, on the caller's buffers -> status"""
    lib = mods[3]
    q = q if hasattr(q, "data_ptr") else np.ascontiguousarray(q, np.float32)
    return idx._lib.mmiss_index_query_distinct(idx._h, lib.ptr(q), int(q.shape[0]), int(k), int(pool), float(min_sep), int(nprobe), lib.ptr(req),
                                               lib.ptr(exc), lib.ptr(lab), lib.ptr(dist), lib.ptr(cnt), lib.ptr(dups), lib.ptr(listed))


def many_queries(c, Q):
    """Q queries: the corpus's eight in turn, from the ninth on with a little noise (the one without a direction stays so)"""
    rng = np.random.Generator(np.random.Philox(91))
    q = c.queries[np.arange(Q) % dc.NQ].copy()
    q[dc.NQ:] += rng.standard_normal(q[dc.NQ:].shape).astype(np.float32) * np.float32(0.05 / np.sqrt(q.shape[1]))
    q[np.arange(Q) % dc.NQ == dc.Q_NODIR] = 0.0
    return q


def run(idx, q, k, min_sep, pool, device=False, **kw):
    if not device:
        return idx.query_distinct(q, k, min_sep, pool, **kw)
    import torch

    tq = torch.from_numpy(np.array(q)).cuda()
    for name in ("require", "exclude"):
        if kw.get(name) is not None:
            kw[name] = torch.from_numpy(np.asarray(kw[name]).view(np.int64).copy()).cuda()
    got = idx.query_distinct(tq, k, min_sep, pool, **kw)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in got)
    return tuple(t.cpu().numpy() for t in got)


# ================================================================================================ against the restatement
# (Q, k, pool, min_sep, masked, device): k 1 / 10 / 1000 / 2040, pool k / k + 1 / 2040, Q 1 / 5 / 300, the extremes of min_sep
CALLS = [
    (8, 3, 30, SEP, False, False), (8, 10, 10, SEP, False, True), (8, 10, 11, SEP, True, False), (8, 10, 2040, SEP, True, True),
    (1, 1, 1, SEP, False, False), (5, 1, 2, SEP, False, True), (5, 1, 2040, 4.0, False, False), (8, 10, 64, -1.0, False, False),
    (1, 1000, 1000, -1.0, False, True), (1, 1000, 1001, SEP, False, False), (1, 1000, 2040, SEP, True, False),
    (1, 2040, 2040, SEP, False, True), (300, 10, 80, SEP, True, True), (300, 1, 64, SEP, False, False),
]


@pytest.mark.parametrize("dtype", DTYPES)
def test_distinct_equals_the_restatement(mods, dtype):
    c, st, idx = dc.corpus(), dc.stored(dtype), index_of(mods, dtype)
    for Q, k, pool, min_sep, masked, device in CALLS:
        q = many_queries(c, Q) if Q > dc.NQ else c.queries[:Q] if Q > 1 else c.queries[dc.Q_BIG:dc.Q_BIG + 1]
        req, exc = pc.query_masks(Q) if masked else (None, None)
        exp = dc.expected_cached((dtype, Q, k, pool, float(min_sep), masked), q, k, pool, min_sep, st, c.labels, c.tags, req, exc)
        got = run(idx, q, k, min_sep, pool, device, require=req, exclude=exc)
        msg = dc.mismatch(got, exp)
        assert msg is None, (dtype, Q, k, pool, min_sep, masked, device, msg)
        if Q >= dc.NQ:
            assert got[2][dc.Q_NODIR] == 0 and got[4][dc.Q_NODIR] == 0              # the query without a direction


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_cases(mods, dtype):
    c, st, idx = dc.corpus(), dc.stored(dtype), index_of(mods, dtype)
    heads = [c.labels[g] for g in c.bursts]
    lab, _, cnt, dups, listed = idx.query_distinct(c.queries[:1], 3, SEP, 30)
    assert cnt[0] == 3 and listed[0] == 30 and dups[0].tolist() == [9, 9, 9] and all(lab[0, j] in heads[j] for j in range(3))
    a, b, cc = c.chain
    lab, _, cnt, dups, _ = idx.query_distinct(c.queries[dc.Q_CHAIN], 3, SEP, 64)
    assert lab[0, :2].tolist() == c.labels[[a, cc]].tolist() and dups[0].tolist() == [1, 0, 0]     # greedy, not clustering
    # the boundary, at the oracle's own bits of the chain's first pair
    at = np.float32(dc.sep(st, a, [b])[0])
    below = np.nextafter(at, np.float32(-np.inf))
    for min_sep in (at, below):
        exp = dc.expected_distinct(c.queries[dc.Q_CHAIN], 2, 64, min_sep, st, c.labels)
        got = idx.query_distinct(c.queries[dc.Q_CHAIN], 2, min_sep, 64)
        assert dc.mismatch(got, exp) is None, (dtype, min_sep)
        assert (got[0][0, 1] == c.labels[b]) == (min_sep == below)
    # the pool runs out on the big group, and not at 300
    lab, _, cnt, dups, listed = idx.query_distinct(c.queries[dc.Q_BIG], 3, SEP, 64)
    assert cnt[0] == 1 and listed[0] == 64 and dups[0].tolist() == [63, 0, 0] and lab[0, 1:].tolist() == [-1, -1]
    assert idx.query_distinct(c.queries[dc.Q_BIG], 3, SEP, 300)[2][0] == 3
    # prefix stability, on the device's own results
    res = [idx.query_distinct(c.queries[:7], 10, SEP, pool) for pool in (10, 64, 300, 2040)]
    for small, large in zip(res, res[1:]):
        for q in range(7):
            n = small[2][q]
            assert n <= large[2][q] and np.array_equal(small[0][q, :n], large[0][q, :n])
            assert np.array_equal(small[1][q, :n].view(np.uint32), large[1][q, :n].view(np.uint32))
    # the extremes: the first k of the plain query bit for bit; one result owning the rest
    got = idx.query_distinct(c.queries[:7], 10, -1.0, 64)
    assert pc.mismatch(got[:3], idx.query(c.queries[:7], 10)) is None and not got[3].any() and (got[4] == 64).all()
    got = idx.query_distinct(c.queries[:7], 10, 4.0, 64)
    assert (got[2] == 1).all() and (got[3][:, 0] == 63).all() and not got[3][:, 1:].any() and (got[0][:, 1:] == -1).all()
    assert np.isinf(got[1][:, 1:]).all()


@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_direction_the_kept_row_is_the_query(mods, dtype):
    c, st, idx = dc.corpus(), dc.stored(dtype), index_of(mods, dtype)
    told = 0
    for qi, (x, y) in zip(dc.Q_PAIRS, c.pairs):
        top = idx.query(c.queries[qi], 2)[0][0]
        s, i = (x, y) if top[0] == c.labels[x] else (y, x)
        fwd, rev = np.float32(dc.sep(st, s, [i])[0]), np.float32(dc.sep(st, i, [s])[0])
        if fwd.view(np.uint32) == rev.view(np.uint32):
            continue
        told += 1
        got = idx.query_distinct(c.queries[qi], 2, min(fwd, rev), 64)
        assert dc.mismatch(got, dc.expected_distinct(c.queries[qi], 2, 64, min(fwd, rev), st, c.labels)) is None
        assert (got[3][0, 0] == 1) == (fwd <= rev)                                   # suppressed iff sep(kept, later) is the smaller
    assert told >= 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_trip_edges_and_list_positions(mods, dtype):
    c, st, idx = dc.corpus(), dc.stored(dtype), index_of(mods, dtype)
    trip = plan(mods, idx)["rows_per_trip"]
    assert plan(mods, idx)["max_pool"] == dc.MAX_POOL and 1 < trip < c.big.size
    # one below / at / above a trip behind the kept entry at position 0: every position is owned by it (the big group)
    for pool in (trip, trip + 1, trip + 2):
        got = idx.query_distinct(c.queries[dc.Q_BIG], 3, SEP, pool)
        assert got[3][0, 0] == pool - 1 and got[2][0] == 1
        assert dc.mismatch(got, dc.expected_cached((dtype, "big", pool), c.queries[dc.Q_BIG], 3, pool, SEP, st, c.labels)) is None
    # ... and behind the third kept entry (position 20 of the bursts' list), where nothing is owned yet; the list's end: a suppressed
    # entry at the last position (pools 20, 30), a kept one (21), a kept one that owns the last (22)
    for pool in (20, 21, 22, 30, 31, 20 + trip, 21 + trip, 22 + trip):
        got = idx.query_distinct(c.queries[:1], 5, SEP, pool)
        assert dc.mismatch(got, dc.expected_cached((dtype, "bursts", pool), c.queries[:1], 5, pool, SEP, st, c.labels)) is None, pool
        assert got[4][0] == pool
    assert idx.query_distinct(c.queries[:1], 5, SEP, 20)[2][0] == 2 and idx.query_distinct(c.queries[:1], 5, SEP, 21)[2][0] == 3
    assert idx.query_distinct(c.queries[:1], 5, SEP, 22)[3][0].tolist() == [9, 9, 1, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [512, "max"])
def test_other_dims_and_a_pool_above_the_row_count(mods, dtype, dim):
    dim = MAX_DIM[dtype] if dim == "max" else dim
    N = 300
    c, st, idx = dc.corpus(N, dim), dc.stored(dtype, N, dim), index_of(mods, dtype, N, dim)
    assert plan(mods, idx)["lds_bytes"] >= 4 * dim
    for k, pool in ((5, 64), (10, 2040)):
        got = idx.query_distinct(c.queries, k, SEP, pool)
        assert dc.mismatch(got, dc.expected_cached((dtype, dim, k, pool), c.queries, k, pool, SEP, st, c.labels)) is None, (k, pool)
    assert (np.delete(got[4], dc.Q_NODIR) == N - 2).all()                                # listed < pool: every row with a direction
    assert got[3][dc.Q_BURSTS, :3].tolist() == [9, 9, 9] and got[3][dc.Q_BIG, 0] == c.big.size - 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_partition(mods, dtype):
    c, st = dc.corpus(), dc.stored(dtype)
    N, B, C = c.rows.shape[0], 2900, 7
    good = np.setdiff1d(np.arange(N), c.nodir)
    centres = np.array(c.rows[good[np.linspace(0, good.size - 1, C).astype(int)]])
    with np.errstate(all="ignore"):
        cells = np.argmax(np.nan_to_num(c.rows[:B], nan=0.0) @ centres.T, axis=1).astype(np.int32)
    cells[np.isin(np.arange(B), c.nodir)] = -1
    idx = mods[0](128, dtype)
    idx.add(c.rows[:B], c.labels[:B])
    idx.set_tags(c.labels[:B], c.tags[:B])
    idx.set_partition(centres, cells)
    idx.add(c.rows[B:], c.labels[B:])                                                     # the tail (tag 0)
    tags = np.concatenate([c.tags[:B], np.zeros(N - B, np.uint64)])
    q = c.queries
    req, exc = pc.query_masks(q.shape[0])
    for nprobe in (1, C + 5):
        part = dict(nprobe=nprobe, centres=centres, cells=cells, B=B)
        got = idx.query_distinct(q, 5, SEP, 64, nprobe=nprobe)
        assert dc.mismatch(got, dc.expected_distinct(q, 5, 64, SEP, st, c.labels, partition=part)) is None, nprobe
        got = idx.query_distinct(q, 5, SEP, 300, nprobe=nprobe, require=req, exclude=exc)
        assert dc.mismatch(got, dc.expected_distinct(q, 5, 300, SEP, st, c.labels, tags, req, exc, partition=part)) is None, nprobe
    assert dc.mismatch(idx.query_distinct(q, 5, SEP, 64, nprobe=C + 5), idx.query_distinct(q, 5, SEP, 64)) is None   # every cell: the flat result
    # the list stage counts as the probed call does, the guard counters stay
    g0, p0 = idx.guard_stats(), idx.partition_info()
    scanned = idx.query_probed(q, 64, 1)[3]
    p1 = idx.partition_info()
    idx.query_distinct(q, 5, SEP, 64, nprobe=1)
    p2 = idx.partition_info()
    assert idx.guard_stats() == g0
    assert p1["queries"] - p0["queries"] == p2["queries"] - p1["queries"] == q.shape[0]
    assert p1["scanned"] - p0["scanned"] == p2["scanned"] - p1["scanned"] == int(scanned.sum())


# ================================================================================================ buffers, scratch
@pytest.mark.parametrize("dtype", DTYPES)
def test_null_outputs_and_stale_scratch(mods, dtype):
    import torch

    c, st, idx = dc.corpus(), dc.stored(dtype), index_of(mods, dtype)
    Q, k, pool = 8, 3, 30
    exp = dc.expected_cached((dtype, 8, 3, 30, float(SEP), False), c.queries, k, pool, SEP, st, c.labels, c.tags, None, None)
    for with_dups, with_listed in ((False, True), (True, False), (False, False)):
        b = [np.full((Q, k), -77, np.int64), np.full((Q, k), -5.0, np.float32), np.full(Q, -3, np.int32),
             np.full((Q, k), -9, np.int32) if with_dups else None, np.full(Q, -9, np.int32) if with_listed else None]
        assert raw(mods, idx, c.queries, k, pool, SEP, 0, *b) == 0
        assert dc.mismatch(b, exp) is None
        t = [None if x is None else torch.from_numpy(np.full_like(x, -1)).cuda() for x in b]
        tq = torch.from_numpy(np.array(c.queries)).cuda()
        idx._sync_stream(tq)
        assert raw(mods, idx, tq, k, pool, SEP, 0, *t) == 0                               # (returns with its work finished)
        assert dc.mismatch([None if x is None else x.cpu().numpy() for x in t], exp) is None
        idx._sync_stream(None)
    mixed = [np.zeros((Q, k), np.int64), np.zeros((Q, k), np.float32), np.zeros(Q, np.int32), torch.zeros((Q, k), dtype=torch.int32).cuda(), None]
    assert raw(mods, idx, c.queries, k, pool, SEP, 0, *mixed) == ERR_ARG                  # all host or all device
    # a large call, then small ones: nothing of the large call's lists or state is seen
    for Q, k, pool, min_sep in ((8, 1000, 2040, SEP), (2, 3, 30, SEP), (1, 2040, 2040, 4.0), (8, 3, 30, SEP)):
        got = idx.query_distinct(c.queries[:Q], k, min_sep, pool)
        exp = dc.expected_cached((dtype, "stale", Q, k, pool, float(min_sep)), c.queries[:Q], k, pool, min_sep, st, c.labels)
        assert dc.mismatch(got, exp) is None, (Q, k, pool)


# ================================================================================================ without the oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_kept_and_owned_by_calls_the_library_had_before(mods, dtype):
    """For every kept pair (s before t) the radius list of s at min_sep does not hold t; every other entry of the list up to the
    last kept one is held by the radius list of an earlier kept entry, and dups counts them under the FIRST such entry."""
    c, idx = dc.corpus(), index_of(mods, dtype)
    k, pool = 6, 200
    for qi in (dc.Q_BURSTS, dc.Q_CHAIN, dc.Q_BIG):
        q = c.queries[qi:qi + 1]
        L, _, m = idx.query(q, pool)
        lab, dist, cnt, dups, listed = idx.query_distinct(q, k, SEP, pool)
        n = int(cnt[0])
        assert listed[0] == m[0] == pool and n == k
        kept = lab[0, :n].tolist()
        members = [set(x[0][0, :x[2][0]].tolist()) for x in (idx.query_radius_by_label([s], float(SEP), 4096) for s in kept)]
        for j, t in enumerate(kept):
            assert not any(t in members[i] for i in range(j)), (qi, j)
        owned = np.zeros(n, np.int64)
        pos_kept = [int(np.nonzero(L[0] == t)[0][0]) for t in kept]
        assert pos_kept == sorted(pos_kept)
        for p, e in enumerate(L[0].tolist()):
            if e in kept:
                continue
            first = next((j for j in range(n) if pos_kept[j] < p and e in members[j]), None)
            if p < pos_kept[-1]:
                assert first is not None, (qi, p)                                         # passed over: it must have an owner
            if first is not None:
                owned[first] += 1
        assert dups[0, :n].tolist() == owned.tolist(), qi


# ================================================================================================ state, arguments, counters
def test_state_arguments_and_counters(mods):
    c, idx = dc.corpus(), index_of(mods, "f16")
    Q, k = 5, 4
    q = c.queries[:Q]
    bufs = lambda kk=k: [np.full((Q, kk), -77, np.int64), np.full((Q, kk), -5.0, np.float32), np.full(Q, -3, np.int32),  # noqa: E731
                         np.full((Q, kk), -9, np.int32), np.full(Q, -9, np.int32)]
    untouched = lambda b: (b[0] == -77).all() and (b[1] == -5.0).all() and (b[2] == -3).all() and (b[3] == -9).all() and (b[4] == -9).all()  # noqa: E731
    for kk, pool, min_sep, nprobe, status in ((5, 4, 0.01, 0, ERR_ARG), (0, 4, 0.01, 0, ERR_ARG), (4, 2041, 0.01, 0, ERR_UNSUPPORTED),
                                              (2041, 2041, 0.01, 0, ERR_UNSUPPORTED), (4, 64, float("nan"), 0, ERR_ARG),
                                              (4, 64, 0.01, -1, ERR_ARG), (4, 64, 0.01, 2, ERR_STATE)):       # (no partition)
        b = bufs(max(kk, 1))
        assert raw(mods, idx, q, kk, pool, min_sep, nprobe, *b) == status and untouched(b), (kk, pool, min_sep, nprobe)
    b = bufs()
    assert raw(mods, idx, q, k, 64, 0.01, 0, None, b[1], b[2], b[3], b[4]) == ERR_ARG and untouched(b)
    assert raw(mods, idx, q[:0], k, 64, 0.01, 0, *b) == 0 and untouched(b)                # no queries: nothing to do
    assert raw(mods, idx, q, k, 64, -0.5, 0, *b) == 0 and not untouched(b)                # a negative min_sep is legal
    # an open query_begin: refused, nothing written
    pend = idx.query_begin(q, k)
    b = bufs()
    assert raw(mods, idx, q, k, 64, 0.01, 0, *b) == ERR_STATE and untouched(b)
    pend.result()
    # the list stage counts in the guard counters exactly as the query it restates; the suppression stage counts nothing
    req = np.full(Q, 1, np.uint64)
    for masks in ({}, {"require": req}):
        s0 = idx.guard_stats()
        idx.query(q, 64, **masks)
        s1 = idx.guard_stats()
        idx.query_distinct(q, k, SEP, 64, **masks)
        s2 = idx.guard_stats()
        assert {n: s1[n] - s0[n] for n in s0} == {n: s2[n] - s1[n] for n in s0} and s1["queries"] - s0["queries"] == Q
    # an empty index: zeros
    empty = mods[0](128, "f16")
    got = empty.query_distinct(q, k, SEP, 64)
    assert (got[0] == -1).all() and np.isinf(got[1]).all() and not got[2].any() and not got[3].any() and not got[4].any()
    for dt in got:
        assert dt.dtype in (np.int64, np.float32, np.int32)


# ================================================================================================ the collection on the real index
def test_collection_query_on_the_device(mods):
    from mmiss_amd.collection import FlatCollection

    N = 300
    c = dc.corpus(N)
    ids = [f"im{i:03d}" for i in range(N)]
    col = FlatCollection("t", dtype="f16")
    col.add(ids=ids, embeddings=c.rows, metadatas=[{"id": i} for i in ids])          # (labels 0 .. N-1: label == row)
    st, lab = dc.stored("f16", N), np.arange(N, dtype=np.int64)
    q = c.queries[[dc.Q_BURSTS, dc.Q_BIG]]
    got = col.query(query_embeddings=q, n_results=3, distinct_distance=float(SEP))     # the big group exhausts pool 64: repeated at 2040
    exp = dc.expected_distinct(q, 3, 2040, SEP, st, lab)
    assert exp[2].tolist() == [3, 3]
    assert got["ids"] == [[ids[int(l)] for l in exp[0][i]] for i in range(2)]
    assert got["distances"] == [[float(d) for d in exp[1][i]] for i in range(2)]
    assert got["duplicates"] == [[int(u) for u in exp[3][i]] for i in range(2)] and got["duplicates"][0] == [9, 9, 9]
    assert "duplicates" not in col.query(query_embeddings=q, n_results=3)

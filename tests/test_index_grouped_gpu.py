"""Grouped search of the flat index (mmiss_index_set_groups / _get_groups / _query_grouped) against the restatement in
tests/grouped_cases.py: the complete ranking of the admitted rows from ro.query, then the walk that keeps the first row of every
group. Every comparison is equality of every element (distances by their bits, groups, counts and the route included). The edges
of a call's plan — the pool, the table's length against the selection's segment, its levels, the query block, the chunks — are
read from mmiss_dbg_index_grouped_plan, so a test proves it crossed them."""
import numpy as np
import pytest

import grouped_cases as gc
from index_query_cases import load_mods

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
D = gc.D
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5          # include/mmiss.h
SCRATCH_KB = 512 * 1024                                   # the default of the option probe_scratch_kb


@pytest.fixture(scope="module")
def mods():
    return load_mods()


def make_index(mods, x, dtype, groups=None, tags=None, n=None):
    n = x.shape[0] if n is None else n
    lab = gc.labels_of(x.shape[0])[:n]
    idx = mods[0](x.shape[1], dtype)
    idx.add(x[:n], lab)
    if tags is not None:
        idx.set_tags(lab, tags[:n])
    if groups is not None:
        idx.set_groups(lab, groups[:n])
    return idx


def raw_grouped(mods, idx, q, k, pool, lab, dist, grp, cnt, route, req=None, exc=None, Q=None):
    """mmiss_index_query_grouped itself, on the caller's buffers -> status"""
    lib = mods[3]
    q = None if q is None else np.ascontiguousarray(q, np.float32)
    return idx._lib.mmiss_index_query_grouped(idx._h, lib.ptr(q), int(q.shape[0]) if Q is None else Q, int(k), int(pool), lib.ptr(req),
                                              lib.ptr(exc), lib.ptr(lab), lib.ptr(dist), lib.ptr(grp), lib.ptr(cnt), lib.ptr(route))


def on_device(idx, q, k, pool=None, req=None, exc=None):
    """query_grouped with every input a CUDA tensor -> numpy results"""
    import torch

    tq = torch.from_numpy(np.array(q)).cuda()
    tm = [None if m is None else torch.from_numpy(np.asarray(m).view(np.int64).copy()).cuda() for m in (req, exc)]
    got = idx.query_grouped(tq, k, pool, require=tm[0], exclude=tm[1])
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in got)
    return tuple(t.cpu().numpy() for t in got)


def agrees(got, q, k, pool, st, lab, groups, tags=None, req=None, exc=None, ranks=None):
    """None when all five outputs are the restatement's, else what differs; ranks: gc.rankings of q under these masks, if at hand"""
    ranks = gc.rankings(q, st, lab, tags, req, exc) if ranks is None else ranks
    msg = gc.mismatch(got[:4], gc.expected_grouped(q, k, st, lab, groups, tags, req, exc, ranks=ranks))
    if msg is not None:
        return msg
    route = gc.expected_route(q, k, gc.default_pool(k) if not pool else pool, st, lab, groups, tags, req, exc, ranks=ranks)
    got_route = np.asarray(got[4])
    if got_route.dtype != np.int32 or not np.array_equal(got_route, route):
        return f"route: got {got_route.tolist()}, expected {route.tolist()}"
    return None


# ================================================================================================ against the restatement
@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_equals_the_restatement(mods, dtype):
    N = 3001
    p = gc.corpus(61, N, D, 300, n_groups=40)
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(N)
    idx = make_index(mods, p["x"], dtype, p["groups"], p["tags"])
    assert np.array_equal(idx.get_groups(lab), p["groups"])
    plan = mods[3].index_grouped_plan(idx._h, 300, 10)
    qb = plan["query_block"]
    assert qb == 16 and plan["pool"] == 80 and plan["table"] == 41 + N and plan["levels"] == 1
    # flagged queries below / at / above the scan's query block run its narrower instances (1, 2, 4, 8, 16 queries)
    assert [mods[3].index_grouped_plan(idx._h, Q, 10)["first_chunk_block"] for Q in (1, 2, 3, 5, qb, 17, 300)] == [1, 2, 4, 8, 16, 16, 16]
    # Q in {1, 5, 16, 300}, k in {1, 10, 2040}, pool in {k, k + 1, default, 2040}; pool = k sends most queries to the scan,
    # k = 2040 all of them (fewer than 2040 groups exist), the default pool none
    calls = [(1, 10, 10, False, False), (1, 1, 1, True, False), (5, 10, 11, True, True), (5, 1, None, False, False),
             (16, 10, 10, True, False), (16, 10, None, False, True), (17, 10, 10, False, False), (300, 10, 10, True, True),
             (300, 10, None, True, False), (5, 2040, 2040, False, False), (3, 2040, None, True, True), (16, 10, 2040, False, False)]
    routes = set()
    ranks = {False: gc.rankings(p["queries"], st, lab), True: gc.rankings(p["queries"], st, lab, p["tags"], *gc.query_masks(300))}   # once
    for Q, k, pool, masked, device in calls:
        q = p["queries"][:Q]
        req, exc = gc.query_masks(Q) if masked else (None, None)
        got = on_device(idx, q, k, pool, req, exc) if device else idx.query_grouped(q, k, pool, require=req, exclude=exc)
        msg = agrees(got, q, k, pool, st, lab, p["groups"], p["tags"] if masked else None, req, exc, ranks=ranks[masked][:Q])
        assert msg is None, (dtype, Q, k, pool, masked, device, msg)
        routes.add((Q, k, pool, tuple(sorted(set(got[4].tolist())))))
        if Q > 2:
            assert got[3][2] == 0 and got[4][2] == 0                      # the query without a direction: no result, by the walk
    assert (300, 10, 10, (0, 1)) in routes                                # one call in which some queries take each route
    assert (300, 10, None, (0,)) in routes and (5, 2040, 2040, (0, 1)) in routes             # (0: the query without a direction)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [512, "max"])
def test_wider_rows_and_smaller_query_blocks(mods, dtype, dim):
    dim = gc.max_dim(dtype) if dim == "max" else dim
    N, Q, k = (700, 21, 10) if dim == 512 else (300, 11, 10)
    p = gc.corpus(62, N, dim, Q, n_groups=6)
    idx = make_index(mods, p["x"], dtype, p["groups"], p["tags"])
    plan = mods[3].index_grouped_plan(idx._h, Q, k, k)
    # the largest of 16 / 8 / 4 / 2 / 1 queries whose f32 staging fits 64 KB
    assert plan["query_block"] == {512: 16, 1920: 8, 3968: 4}[dim] and plan["lds_bytes"] == plan["query_block"] * (dim * 4 + 16)
    assert Q % plan["query_block"] != 0 and Q > plan["query_block"]
    req, exc = gc.query_masks(Q)
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(N)
    got = idx.query_grouped(p["queries"], k, k)                            # six groups and a few ungrouped rows: the scan answers
    assert agrees(got, p["queries"], k, k, st, lab, p["groups"]) is None and got[4].max() == 1
    got = idx.query_grouped(p["queries"], k, None, require=req, exclude=exc)
    assert agrees(got, p["queries"], k, None, st, lab, p["groups"], p["tags"], req, exc) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_crowd_takes_the_exhaustive_route_and_the_pool_never_shows(mods, dtype):
    p = gc.crowd()
    N = p["x"].shape[0]
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(N)
    idx = make_index(mods, p["x"], dtype, p["groups"])
    k = gc.CROWD_K
    short = idx.query_grouped(p["queries"], k, 16)
    long = idx.query_grouped(p["queries"], k, 2040)
    assert short[4].tolist() == [1] and long[4].tolist() == [0]
    assert gc.mismatch(short[:4], long[:4]) is None                        # the outputs of the two calls are identical
    assert agrees(short, p["queries"], k, 16, st, lab, p["groups"]) is None and short[3][0] == k and short[2][0, 0] == p["big"]
    for pool in (k, gc.CROWD_SIZE + k - 2, gc.CROWD_SIZE + k - 1, None, N, N + 1):     # around the first complete pool, above the rows
        got = idx.query_grouped(p["queries"], k, pool)
        assert agrees(got, p["queries"], k, pool, st, lab, p["groups"]) is None, pool
        assert gc.mismatch(got[:4], long[:4]) is None, pool
    assert idx.query_grouped(p["queries"], k, gc.CROWD_SIZE + k - 2)[4][0] == 1               # 43 entries hold four groups at the most
    # a bigger crowd than any pool: 2100 near rows of one group
    big = gc.crowd(size=2100)
    Nb = big["x"].shape[0]
    idx = make_index(mods, big["x"], dtype, big["groups"])
    got = idx.query_grouped(big["queries"], k, 2040)
    assert got[4].tolist() == [1] and got[3][0] == k
    assert agrees(got, big["queries"], k, 2040, gc.stored_of(big["x"], dtype), gc.labels_of(Nb), big["groups"]) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_heads_ties_masks_and_extreme_ids(mods, dtype):
    for case, k in ((gc.ends(), 4), (gc.ties(), 6), (gc.masked_head(), 8)):
        N = case["x"].shape[0]
        st, lab = gc.stored_of(case["x"], dtype), gc.labels_of(N)
        tags = case.get("tags")
        idx = make_index(mods, case["x"], dtype, case["groups"], tags)
        for pool in (k, None):                                            # by the scan and by the walk
            for req in ((None, np.uint64(1)) if tags is not None else (None,)):
                got = idx.query_grouped(case["queries"], k, pool, require=req)
                assert agrees(got, case["queries"], k, pool, st, lab, case["groups"], tags, req) is None, (N, pool, req)
    p = gc.ends()
    idx = make_index(mods, p["x"], dtype, p["groups"])
    got = idx.query_grouped(p["queries"], 4, 4)
    assert got[0][:, 0].tolist() == gc.labels_of(700)[list(p["planted"])].tolist() and got[2][:, 0].tolist() == [0, 1]
    p = gc.ties()
    got = make_index(mods, p["x"], dtype, p["groups"]).query_grouped(p["queries"], 6, 6)
    assert got[0][0, :3].tolist() == gc.labels_of(60)[list(p["tied"])].tolist() and got[2][0, :3].tolist() == [5, 2, -1]
    p = gc.masked_head()
    got = make_index(mods, p["x"], dtype, p["groups"], p["tags"]).query_grouped(p["queries"], 8, 8, require=np.uint64(1))
    assert got[0][0, 0] == gc.labels_of(80)[p["admitted"]] and got[2][0, 0] == 3


def test_group_ids_at_both_ends_and_three_selection_levels(mods):
    p = gc.extreme_ids()
    N = p["x"].shape[0]
    st, lab = gc.stored_of(p["x"], "f16"), gc.labels_of(N)
    idx = make_index(mods, p["x"], "f16", p["groups"])
    plan = mods[3].index_grouped_plan(idx._h, 3, 5, 5)
    assert plan["table"] == gc.MAX_GROUPS + N and plan["levels"] == 3 and plan["chunks"] == 1, plan
    got = idx.query_grouped(p["queries"], 5, 5)                            # two groups and ungrouped rows; the table has 2^24 + N slots
    assert agrees(got, p["queries"], 5, 5, st, lab, p["groups"]) is None
    assert got[2][:, 0].tolist() == [-1, 0, gc.MAX_GROUPS - 1] and set(got[4].tolist()) <= {0, 1}
    got = idx.query_grouped(p["queries"], 3, 3)
    assert agrees(got, p["queries"], 3, 3, st, lab, p["groups"]) is None and got[4].max() == 1


# ================================================================================================ edges of the plan
@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_edges_segment_levels_and_chunks(mods, dtype):
    lib = mods[3]
    N, k = 4090, 10
    p = gc.corpus(63, N, D, 8)
    rng = np.random.Generator(np.random.Philox(7))
    groups = rng.integers(0, 5, N).astype(np.int32)                       # five big groups: a list of ten never holds ten heads ...
    groups[[0, 1, N - 2, N - 1]] = -1                                      # ... and the first and the last table slot of the ungrouped
    groups[3], groups[N - 3] = 4, 0
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(N)
    idx = make_index(mods, p["x"], dtype, groups)
    q = np.concatenate([p["queries"][:6], p["x"][[0, N - 1]]])             # the last two: bit copies of the ungrouped end rows
    seg = lib.index_grouped_plan(idx._h, 1, k, k)["segment"]
    assert seg == 4096
    # the table one below / at / above a segment: G = 5, 6, 7 over 4090 rows
    for top in (4, 5, 6):
        groups[3] = top
        idx.set_groups(lab[3:4], groups[3:4])
        plan = lib.index_grouped_plan(idx._h, 8, k, k)
        assert plan["table"] == top + 1 + N == seg - 1 + (top - 4) and plan["levels"] == (2 if top == 6 else 1), plan
        got = idx.query_grouped(q, k, k)
        assert agrees(got, q, k, k, st, lab, groups) is None, top
        assert got[4].tolist() == [1, 1, 0, 1, 1, 1, 1, 1] and got[0][6, 0] == lab[0] and got[0][7, 0] == lab[N - 1]
    # two levels with k = 1000 survivors per segment, several queries
    plan = lib.index_grouped_plan(idx._h, 3, 1000, 1000)
    assert plan["levels"] == 2 and plan["stride1"] == 2000, plan
    got = idx.query_grouped(q[:3], 1000, 1000)
    assert agrees(got, q[:3], 1000, 1000, st, lab, groups) is None and 6 <= got[3][0] <= 10   # every group there is
    # several chunks: the scratch budget lowered to three queries' tables (a chunk is then no multiple of the query block)
    one = lib.index_grouped_plan(idx._h, 1, k, k)
    per_query_kb = (one["stride0"] + one["stride1"]) * 8 // 1024 + 1
    lib.set_option("probe_scratch_kb", 3 * per_query_kb)
    try:
        plan = lib.index_grouped_plan(idx._h, 7, k, k)
        assert plan["queries_per_chunk"] == 3 and plan["chunks"] == 3 and (plan["first_chunk_block"], plan["last_chunk_block"]) == (4, 1), plan
        got = idx.query_grouped(q, k, k)                                   # seven of the eight queries are flagged
    finally:
        lib.set_option("probe_scratch_kb", SCRATCH_KB)
    assert agrees(got, q, k, k, st, lab, groups) is None and got[4].sum() == 7


def test_masks_that_admit_nothing_and_an_empty_index(mods):
    N, Q, k = 600, 5, 4
    p = gc.corpus(64, N, D, Q, n_groups=3)
    idx = make_index(mods, p["x"], "f16", p["groups"], p["tags"])         # tags on bits 0 .. 2
    nothing = (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.full((Q, k), -1, np.int32), np.zeros(Q, np.int32))
    for kw in (dict(require=np.uint64(1 << 40)), dict(require=np.uint64(1), exclude=np.uint64(1))):
        got = idx.query_grouped(p["queries"], k, k, **kw)
        assert gc.mismatch(got[:4], nothing) is None and (got[4] == 0).all()                  # the list ends before the pool: the walk
    empty = mods[0](D, "f16")
    got = empty.query_grouped(p["queries"], k)
    assert gc.mismatch(got[:4], nothing) is None and (got[4] == 0).all()
    # one mask per query: query 1 admits nothing, the others go on
    req = np.array([0, 1 << 40, 0, 1, 0], np.uint64)
    st, lab = gc.stored_of(p["x"], "f16"), gc.labels_of(N)
    got = idx.query_grouped(p["queries"], k, k, require=req)
    assert agrees(got, p["queries"], k, k, st, lab, p["groups"], p["tags"], req) is None and got[3][1] == 0 and got[4].max() == 1


# ================================================================================================ state
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_small_call_after_a_large_one_sees_nothing_stale(mods, dtype):
    N = 3001
    p = gc.corpus(65, N, D, 64, n_groups=4)
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(N)
    idx = make_index(mods, p["x"], dtype, p["groups"], p["tags"])
    for Q, k, pool, req in ((64, 1000, 1000, None), (5, 3, 3, None), (1, 2040, 2040, np.uint64(2)), (2, 10, None, None), (3, 5, 5, np.uint64(1))):
        q = p["queries"][:Q]
        got = idx.query_grouped(q, k, pool, require=req)
        assert agrees(got, q, k, pool, st, lab, p["groups"], p["tags"], req) is None, (Q, k, pool)


def test_after_add_update_remove_clear_and_load(mods, tmp_path):
    N, Q, k = 1500, 5, 20
    p = gc.corpus(66, N, D, Q, n_groups=9)
    x, lab, groups = np.array(p["x"]), gc.labels_of(N), np.array(p["groups"])
    idx = make_index(mods, x, "f16", groups, n=1000)
    norm = lambda a: mods[1].normalize_rows(a, "f16")                     # noqa: E731
    q = p["queries"]
    with np.errstate(all="ignore"):
        for pool in (k, None):
            assert agrees(idx.query_grouped(q, k, pool), q, k, pool, norm(x[:1000]), lab[:1000], groups[:1000]) is None
        # added rows are ungrouped until they are given a group
        idx.add(x[1000:], lab[1000:])
        assert (idx.get_groups(lab[1000:]) == -1).all() and np.array_equal(idx.get_groups(lab[:1000]), groups[:1000])
        g2 = groups.copy()
        g2[1000:] = -1
        for pool in (k, None):
            assert agrees(idx.query_grouped(q, k, pool), q, k, pool, norm(x), lab, g2) is None
        idx.set_groups(lab[1000:], groups[1000:])
        assert agrees(idx.query_grouped(q, k, k), q, k, k, norm(x), lab, groups) is None
        # a label given twice keeps its last value; update keeps the group
        idx.set_groups(lab[[7, 8, 7]], np.array([3, 3, 5], np.int32))
        groups[7], groups[8] = 5, 3
        x[[7, 8]] = x[[100, 101]] * 2.0
        idx.update(lab[[7, 8]], x[[7, 8]])
        assert idx.get_groups(lab[[7, 8]]).tolist() == [5, 3]
        for pool in (k, None):
            assert agrees(idx.query_grouped(q, k, pool), q, k, pool, norm(x), lab, groups) is None
        # removal: the survivors keep their groups, on their new rows
        gone = np.concatenate([np.arange(5, 200), [N - 1]])
        assert idx.remove(lab[gone]) == gone.size
        x2, lab2, gr2 = np.delete(x, gone, axis=0), np.delete(lab, gone), np.delete(groups, gone)
        assert np.array_equal(idx.get_groups(lab2), gr2)
        for pool in (k, None):
            got = idx.query_grouped(q, k, pool)
            assert agrees(got, q, k, pool, norm(x2), lab2, gr2) is None and not np.isin(got[0], lab[gone]).any()
        # save and load: the file holds no groups
        path = str(tmp_path / "g.idx")
        idx.save(path)
        idx.load(path)
        assert (idx.get_groups(lab2) == -1).all()
        none = np.full(lab2.size, -1, np.int32)
        got = idx.query_grouped(q, k, k)
        assert agrees(got, q, k, k, norm(x2), lab2, none) is None and (got[2] == -1).all()
        assert gc.pc.mismatch((got[0], got[1], got[3]), idx.query(q, k)) is None
        idx.set_groups(lab2, gr2)
        assert agrees(idx.query_grouped(q, k, k), q, k, k, norm(x2), lab2, gr2) is None
        # clear: no rows, no groups; the same labels come back ungrouped
        idx.clear()
        assert idx.query_grouped(q, k)[3].tolist() == [0] * Q
        idx.add(x2[:300], lab2[:300])
        assert (idx.get_groups(lab2[:300]) == -1).all()
        assert agrees(idx.query_grouped(q, k, k), q, k, k, norm(x2[:300]), lab2[:300], none[:300]) is None


def test_state_arguments_and_counters(mods):
    import partition_cases as pc

    N, C, Q, k = 600, 7, 5, 4
    p = pc.clustered(16, N, D, C, Q)
    groups = (np.arange(N) % 3).astype(np.int32)
    idx = make_index(mods, p["x"], "f16", groups)
    st, lab = gc.stored_of(p["x"], "f16"), gc.labels_of(N)
    bufs = lambda kk=k: (np.full((Q, kk), -77, np.int64), np.full((Q, kk), -5.0, np.float32), np.full((Q, kk), -8, np.int32),  # noqa: E731
                         np.full(Q, -3, np.int32), np.full(Q, -9, np.int32))
    untouched = lambda b: (b[0] == -77).all() and (b[1] == -5.0).all() and (b[2] == -8).all() and (b[3] == -3).all() and (b[4] == -9).all()  # noqa: E731
    # a partition set before the call is still there afterwards, its counters unchanged; the guard counts the list stage exactly as
    # the flat query at k = pool does, whichever route answers
    idx.set_partition(p["centres"], p["cells"])
    idx.query_probed(p["queries"], k, 2)
    info = idx.partition_info()
    delta = lambda a, b: {key: b[key] - a[key] for key in a}              # noqa: E731
    for pool, route in ((k, 1), (2040, 0)):                               # (three groups: four heads never; 2040 is above the rows)
        g0 = idx.guard_stats()
        idx.query(p["queries"], pool)
        g1 = idx.guard_stats()
        got = idx.query_grouped(p["queries"], k, pool)
        g2 = idx.guard_stats()
        assert delta(g0, g1) == delta(g1, g2) and g2["queries"] - g1["queries"] == Q, (pool, g0, g1, g2)
        assert agrees(got, p["queries"], k, pool, st, lab, groups) is None and got[4].max() == route
    assert idx.partition_info() == info and info["cells"] == C
    exp = gc.expected_grouped(p["queries"], k, st, lab, groups)
    # a null out_route; host buffers of the caller's own
    b = bufs()
    assert raw_grouped(mods, idx, p["queries"], k, k, b[0], b[1], b[2], b[3], None) == 0 and (b[4] == -9).all()
    assert gc.mismatch(b[:4], exp) is None
    # every argument error, with the outputs untouched
    q = np.array(p["queries"])
    for kk, pool, kw, status in ((2041, 0, {}, ERR_UNSUPPORTED), (0, 0, {}, ERR_ARG), (-1, 0, {}, ERR_ARG), (k, 0, {"Q": 0}, ERR_ARG),
                                 (k, 0, {"Q": -2}, ERR_ARG), (k, k - 1, {}, ERR_ARG), (k, -1, {}, ERR_ARG), (k, 2041, {}, ERR_UNSUPPORTED)):
        b = bufs(max(kk, 1))
        assert raw_grouped(mods, idx, q, kk, pool, *b, **kw) == status and untouched(b), (kk, pool, kw)
    b = bufs()
    assert raw_grouped(mods, idx, None, k, 0, *b, Q=Q) == ERR_ARG and untouched(b)            # null queries
    for missing in range(4):
        args = list(b)
        args[missing] = None
        assert raw_grouped(mods, idx, q, k, 0, *args) == ERR_ARG and untouched(b), missing
    assert idx._lib.mmiss_index_query_grouped(None, mods[3].ptr(q), Q, k, 0, None, None, mods[3].ptr(b[0]), mods[3].ptr(b[1]), mods[3].ptr(b[2]),
                                              mods[3].ptr(b[3]), mods[3].ptr(b[4])) == ERR_ARG
    import torch

    dev_cnt = torch.full((Q,), -3, dtype=torch.int32, device="cuda")                          # host and device outputs mixed
    assert raw_grouped(mods, idx, q, k, 0, b[0], b[1], b[2], dev_cnt, b[4]) == ERR_ARG and untouched(b) and (dev_cnt.cpu() == -3).all()
    dev_route = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    assert raw_grouped(mods, idx, q, k, 0, b[0], b[1], b[2], b[3], dev_route) == ERR_ARG and untouched(b)
    # set_groups: a label that is not stored or a value outside the range changes nothing
    before = idx.get_groups(lab)
    lib, h = idx._lib, idx._h
    two = np.ascontiguousarray(lab[:2])
    for labels, vals in ((np.array([lab[0], 4], np.int64), [1, 1]), (two, [1, -2]), (two, [gc.MAX_GROUPS, 1])):
        vals = np.array(vals, np.int32)
        assert lib.mmiss_index_set_groups(h, labels.ctypes.data, vals.ctypes.data, 2) == ERR_ARG
    assert lib.mmiss_index_set_groups(h, None, None, 2) == ERR_ARG and lib.mmiss_index_set_groups(h, two.ctypes.data, None, -1) == ERR_ARG
    out = np.full(2, -7, np.int32)
    assert lib.mmiss_index_get_groups(h, np.array([lab[0], 4], np.int64).ctypes.data, 2, out.ctypes.data) == ERR_ARG and (out == -7).all()
    assert np.array_equal(idx.get_groups(lab), before)
    assert mods[3].index_grouped_plan(idx._h, 1, k)["table"] == 3 + N                         # ... and the high-water mark stays
    # device labels and groups
    dl, dg = torch.from_numpy(two.copy()).cuda(), torch.tensor([2, 1], dtype=torch.int32, device="cuda")
    assert lib.mmiss_index_set_groups(h, dl.data_ptr(), dg.data_ptr(), 2) == 0 and idx.get_groups(two).tolist() == [2, 1]
    dout = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    assert lib.mmiss_index_get_groups(h, dl.data_ptr(), 2, dout.data_ptr()) == 0 and dout.cpu().tolist() == [2, 1]
    idx.set_groups(two, before[:2])
    # the wrapper checks before the library call
    for bad in (0, 2041):
        with pytest.raises(ValueError):
            idx.query_grouped(q, bad)
    with pytest.raises(ValueError):
        idx.query_grouped(q, k, k - 1)
    with pytest.raises(ValueError):
        idx.query_grouped(q[:0], k)
    # an open query_begin: the calls refuse and write nothing
    pend = idx.query_begin(p["queries"], k)
    b = bufs()
    assert raw_grouped(mods, idx, q, k, 0, *b) == ERR_STATE and untouched(b)
    vals = np.array([1, 1], np.int32)
    assert lib.mmiss_index_set_groups(h, two.ctypes.data, vals.ctypes.data, 2) == ERR_STATE
    assert lib.mmiss_index_get_groups(h, two.ctypes.data, 2, out.ctypes.data) == ERR_STATE and (out == -7).all()
    pend.result()
    assert np.array_equal(idx.get_groups(lab), before)
    assert gc.mismatch(idx.query_grouped(p["queries"], k, k)[:4], exp) is None
    assert idx.partition_info() == info


# ================================================================================================ without the oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_ungrouped_rows_and_groups_of_one_give_the_filtered_query(mods, dtype):
    N, Q, k = 3001, 64, 50
    p = gc.corpus(67, N, D, Q)
    lab = gc.labels_of(N)
    req, exc = gc.query_masks(Q)
    idx = make_index(mods, p["x"], dtype, None, p["tags"])
    flat, filt = idx.query(p["queries"], k), idx.query(p["queries"], k, require=req, exclude=exc)
    for groups in (None, np.arange(N, dtype=np.int32), np.arange(N, dtype=np.int32)[::-1].copy()):
        if groups is not None:
            idx.set_groups(lab, groups)
        for pool in (k, None, 2040):
            got = idx.query_grouped(p["queries"], k, pool)
            assert gc.pc.mismatch((got[0], got[1], got[3]), flat) is None and (got[4] == 0).all()      # k heads in the first k entries
            got = idx.query_grouped(p["queries"], k, pool, require=req, exclude=exc)
            assert gc.pc.mismatch((got[0], got[1], got[3]), filt) is None
            if groups is not None:
                rows = (got[0] - 5) // 3
                assert np.array_equal(got[2][got[0] >= 0], groups[rows[got[0] >= 0]])
            else:
                assert (got[2] == -1).all()
    # all rows in one group: the top-1
    idx.set_groups(lab, np.zeros(N, np.int32))
    got = idx.query_grouped(p["queries"], k)
    has = flat[2] > 0
    assert np.array_equal(got[3], has.astype(np.int32)) and np.array_equal(got[0][:, 0], flat[0][:, 0]) and (got[0][:, 1:] == -1).all()
    assert np.array_equal(got[1][:, 0].view(np.uint32), flat[1][:, 0].view(np.uint32)) and np.array_equal(got[4], has.astype(np.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_tag_bit_j_on_group_j_gives_the_head_by_the_filtered_query(mods, dtype):
    N, Q, G = 3001, 16, 64
    p = gc.corpus(68, N, D, Q)
    lab = gc.labels_of(N)
    rng = np.random.Generator(np.random.Philox(9))
    groups = rng.integers(0, G, N).astype(np.int32)
    tags = np.uint64(1) << groups.astype(np.uint64)
    idx = make_index(mods, p["x"], dtype, groups, tags)
    heads = {}
    for j in range(G):
        l1, d1, c1 = idx.query(p["queries"], 1, require=np.uint64(1 << j))
        heads[j] = (l1[:, 0], d1[:, 0], c1)
    for pool in (G, None, 2040):                                          # by the scan (64 heads never lie in 64 entries) and by the walk
        got = idx.query_grouped(p["queries"], G, pool)
        for qi in range(Q):
            n = int(got[3][qi])
            assert n == sum(int(heads[j][2][qi]) for j in range(G)) and sorted(got[2][qi, :n].tolist()) == list(range(G))[:n] or n == 0
            for s in range(n):
                j = int(got[2][qi, s])
                assert got[0][qi, s] == heads[j][0][qi] and got[1][qi, s].view(np.uint32) == heads[j][1][qi].view(np.uint32), (pool, qi, s)
            assert (np.diff(got[1][qi, :n]) >= 0).all()

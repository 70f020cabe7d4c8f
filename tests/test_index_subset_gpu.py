"""Subset search of the flat index (mmiss_index_query_subset) against the restatement in tests/subset_cases.py: S by np.isin on
the labels, the masks, ro.query over the admitted rows of S. Every comparison is equality of every element (distances by their
bits, matched included). The edges of a call's plan — the scan's share, its query block, the selection's segment and levels, the
query chunks — are read from mmiss_dbg_index_subset_plan, so a test proves it crossed them."""
import numpy as np
import pytest

import subset_cases as sc
from index_query_cases import load_mods

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
D = sc.D
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5          # include/mmiss.h
SCRATCH_KB = 512 * 1024                                   # the default of the option probe_scratch_kb


@pytest.fixture(scope="module")
def mods():
    return load_mods()


def make_index(mods, x, dtype, tags=None, n=None):
    n = x.shape[0] if n is None else n
    idx = mods[0](x.shape[1], dtype)
    idx.add(x[:n], sc.labels_of(x.shape[0])[:n])
    if tags is not None:
        idx.set_tags(sc.labels_of(x.shape[0])[:n], tags[:n])
    return idx


def raw_subset(mods, idx, q, k, cand, lab, dist, cnt, matched, req=None, exc=None, n_cand=None, Q=None):
    """mmiss_index_query_subset itself, on the caller's buffers -> status"""
    lib = mods[3]
    q = None if q is None else np.ascontiguousarray(q, np.float32)
    cand = None if cand is None else np.ascontiguousarray(cand, np.int64)
    n = (0 if cand is None else int(cand.shape[0])) if n_cand is None else n_cand
    return idx._lib.mmiss_index_query_subset(idx._h, lib.ptr(q), int(q.shape[0]) if Q is None else Q, int(k), lib.ptr(cand), n, lib.ptr(req),
                                             lib.ptr(exc), lib.ptr(lab), lib.ptr(dist), lib.ptr(cnt), lib.ptr(matched))


def on_device(idx, q, k, cand, req=None, exc=None):
    """query_subset with every input a CUDA tensor -> numpy results"""
    import torch

    tq = torch.from_numpy(np.array(q)).cuda()
    tc = torch.from_numpy(np.array(cand, np.int64)).cuda()
    tm = [None if m is None else torch.from_numpy(np.asarray(m).view(np.int64).copy()).cuda() for m in (req, exc)]
    got = idx.query_subset(tq, k, tc, require=tm[0], exclude=tm[1])
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in got)
    return tuple(t.cpu().numpy() for t in got)


# ================================================================================================ against the restatement
@pytest.mark.parametrize("dtype", DTYPES)
def test_subset_equals_the_restatement(mods, dtype):
    N = 4999
    p = sc.corpus(21, N)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    qb = mods[3].index_subset_plan(idx._h, 300, 10, 700)["query_block"]
    assert qb == 16
    mixed, large = sc.mixed_list(N, 700), sc.sized_list(N, 3000)
    longer = np.concatenate([lab, sc.UNKNOWN, lab[::-1]])                # longer than the row count: every label twice
    # Q below / at / a multiple of / above the scan's query block (300 = 18 blocks and 12 queries), k above |S| included; the
    # calls below the block run its narrower instances (1, 2, 4, 8 queries)
    assert [mods[3].index_subset_plan(idx._h, Q, 10, 700)["first_chunk_block"] for Q in (1, 2, 3, 5, qb, 64, 300)] == [1, 2, 4, 8, 16, 16, 16]
    calls = [(1, 10, mixed, False, False), (2, 10, mixed, True, False), (3, 10, large, False, True), (5, 1, mixed, True, True),
             (qb, 10, large, True, False), (64, 1000, mixed, True, False), (300, 2040, large, False, True), (300, 10, longer, True, False)]
    for Q, k, cand, masked, device in calls:
        q = p["queries"][:Q]
        req, exc = sc.query_masks(Q) if masked else (None, None)
        exp = sc.expected_subset(q, k, cand, st, lab, p["tags"], req, exc)
        got = on_device(idx, q, k, cand, req, exc) if device else idx.query_subset(q, k, cand, require=req, exclude=exc)
        msg = sc.mismatch(got, exp)
        assert msg is None, (dtype, Q, k, len(cand), masked, device, msg)
        assert (got[3] == sc.subset_rows(cand, lab).size).all()
        if Q > 2:
            assert got[2][2] == 0 and got[3][2] == got[3][0]            # the query without a direction: no result, matched as ever
    assert exp[3][0] == N and 1000 > sc.subset_rows(mixed, lab).size == 700


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [512, "max"])
def test_wider_rows_and_smaller_query_blocks(mods, dtype, dim):
    dim = sc.max_dim(dtype) if dim == "max" else dim
    N, Q, k = 700, 21, 10
    p = sc.corpus(22, N, dim, Q)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    plan = mods[3].index_subset_plan(idx._h, Q, k, 300)
    # the largest of 16 / 8 / 4 / 2 / 1 queries whose f32 staging fits 64 KB
    assert plan["query_block"] == {512: 16, 1920: 8, 3968: 4}[dim] and plan["lds_bytes"] == plan["query_block"] * dim * 4 <= 65536
    assert Q % plan["query_block"] != 0 and Q > plan["query_block"]
    cand = sc.mixed_list(N, 300)
    req, exc = sc.query_masks(Q)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    assert sc.mismatch(idx.query_subset(p["queries"], k, cand), sc.expected_subset(p["queries"], k, cand, st, lab)) is None
    got = idx.query_subset(p["queries"], k, cand, require=req, exclude=exc)
    assert sc.mismatch(got, sc.expected_subset(p["queries"], k, cand, st, lab, p["tags"], req, exc)) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_label_listed_equals_the_flat_query(mods, dtype):
    N, Q, k = 3001, 64, 10
    p = sc.corpus(23, N, D, Q)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    lab = sc.labels_of(N)
    req, exc = sc.query_masks(Q)
    rng = np.random.Generator(np.random.Philox(5))
    every = lab[rng.permutation(N)]
    got = idx.query_subset(p["queries"], k, every)
    assert sc.mismatch(got[:3], idx.query(p["queries"], k)) is None and (got[3] == N).all()
    assert sc.mismatch(got[:3], sc.expected_flat(p["queries"], k, sc.stored_of(p["x"], dtype), lab)) is None
    got = idx.query_subset(p["queries"], k, every, require=req, exclude=exc)
    assert sc.mismatch(got[:3], idx.query(p["queries"], k, require=req, exclude=exc)) is None and (got[3] == N).all()
    assert sc.mismatch(got[:3], sc.expected_flat(p["queries"], k, sc.stored_of(p["x"], dtype), lab, p["tags"], req, exc)) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_single_and_unknown_lists(mods, dtype):
    N, Q, k = 600, 5, 4
    p = sc.corpus(24, N, D, Q)
    idx = make_index(mods, p["x"], dtype)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    nothing = (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros(Q, np.int32), np.zeros(Q, np.int64))
    assert sc.mismatch(idx.query_subset(p["queries"], k, np.zeros(0, np.int64)), nothing) is None
    assert sc.mismatch(idx.query_subset(p["queries"], k, []), nothing) is None
    assert sc.mismatch(idx.query_subset(p["queries"], k, sc.UNKNOWN), nothing) is None
    assert sc.mismatch(on_device(idx, p["queries"], k, sc.UNKNOWN), nothing) is None
    b = (np.full((Q, k), -77, np.int64), np.full((Q, k), -5.0, np.float32), np.full(Q, -3, np.int32), np.full(Q, -9, np.int64))
    assert raw_subset(mods, idx, p["queries"], k, None, *b) == 0         # n_cand = 0 with a null list
    assert sc.mismatch(b, nothing) is None
    for row in (0, 77, N - 1):
        got = idx.query_subset(p["queries"], k, lab[row:row + 1])
        assert sc.mismatch(got, sc.expected_subset(p["queries"], k, lab[row:row + 1], st, lab)) is None
        assert (got[3] == 1).all() and got[0][0, 0] == lab[row] and got[2][0] == 1 and got[2][2] == 0
    # a listed row without a direction is matched and never returned
    nd = lab[sc.nodir_rows(N)]
    got = idx.query_subset(p["queries"], k, nd)
    assert (got[3] == nd.size).all() and (got[2] == 0).all() and (got[0] == -1).all()
    # an empty index
    empty = mods[0](D, dtype)
    assert sc.mismatch(empty.query_subset(p["queries"], k, lab), nothing) is None


# ================================================================================================ edges of the plan
@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_edges_share_segment_levels_and_chunks(mods, dtype):
    lib = mods[3]
    N = sc.BIG_N
    p = sc.corpus(25, N, D, 8)
    idx = make_index(mods, p["x"], dtype)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    plan = lib.index_subset_plan(idx._h, 1, 10, 65)
    share, seg = plan["share"], plan["segment"]
    assert share >= 64 and share % 16 == 0 and seg == 4096
    q1 = p["queries"][:1]
    # |S| one below / at / above the scan's share and the selection's segment
    for m in (share - 1, share, share + 1, seg - 1, seg, seg + 1):
        plan = lib.index_subset_plan(idx._h, 1, 10, m)
        assert plan["share"] == share and plan["bound"] == m and plan["levels"] == (2 if m > seg else 1), plan
        assert plan["splits"] == -(-m // share)
        cand = sc.sized_list(N, m, seed=m)
        assert sc.mismatch(idx.query_subset(q1, 10, cand), sc.expected_subset(q1, 10, cand, st, lab)) is None, m
    # two and three selection levels (k = 1000: above 4096 and above 16 384 keys), several queries
    q3 = p["queries"][:3]
    for m, levels in ((5000, 2), (16500, 3)):
        plan = lib.index_subset_plan(idx._h, 3, 1000, m)
        assert plan["levels"] == levels and plan["chunks"] == 1, plan
        cand = sc.sized_list(N, m, seed=m)
        assert sc.mismatch(idx.query_subset(q3, 1000, cand), sc.expected_subset(q3, 1000, cand, st, lab)) is None, m
    # several query chunks: the scratch budget lowered to three queries' key areas (a chunk is then no multiple of the query block)
    m, Q = 5000, 8
    cand = sc.sized_list(N, m, seed=m)
    one = lib.index_subset_plan(idx._h, 1, 10, m)
    per_query_kb = (one["stride0"] + one["stride1"]) * 8 // 1024 + 1
    lib.set_option("probe_scratch_kb", 3 * per_query_kb)
    try:
        plan = lib.index_subset_plan(idx._h, Q, 10, m)
        assert plan["queries_per_chunk"] == 3 and plan["chunks"] == 3 and (plan["first_chunk_block"], plan["last_chunk_block"]) == (4, 2), plan
        got = idx.query_subset(p["queries"], 10, cand)
    finally:
        lib.set_option("probe_scratch_kb", SCRATCH_KB)
    assert sc.mismatch(got, sc.expected_subset(p["queries"], 10, cand, st, lab)) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_winners_at_the_ends_of_the_index_and_of_the_list(mods, dtype):
    N = 3001
    p = sc.positions(N)
    idx = make_index(mods, p["x"], dtype)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    for cand in p["lists"]:
        got = idx.query_subset(p["queries"], 3, cand)
        assert sc.mismatch(got, sc.expected_subset(p["queries"], 3, cand, st, lab)) is None
        assert np.array_equal(got[0][:, 0], lab[p["planted"]]) and (got[3] == 302).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_outside_the_list_is_not_returned(mods, dtype):
    p = sc.hidden()
    N = p["x"].shape[0]
    idx = make_index(mods, p["x"], dtype)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    hid = lab[p["hidden"]]
    assert idx.query(p["queries"], 1)[0][0, 0] == hid
    got = idx.query_subset(p["queries"], N, p["cand"])
    assert sc.mismatch(got, sc.expected_subset(p["queries"], N, p["cand"], st, lab)) is None
    assert hid not in got[0] and got[2][0] == N - 1 == got[3][0]
    got = idx.query_subset(p["queries"], 5, np.append(p["cand"], hid))
    assert got[0][0, 0] == hid


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_repeated_label_counts_once(mods, dtype):
    p = sc.crowding()
    idx = make_index(mods, p["x"], dtype)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(200)
    got = idx.query_subset(p["queries"], sc.CROWD_K, p["cand"])
    assert sc.mismatch(got, sc.expected_subset(p["queries"], sc.CROWD_K, p["cand"], st, lab)) is None
    assert got[0][0, 0] == lab[p["crowd"]] and len(set(got[0][0].tolist())) == sc.CROWD_K and got[3][0] == 21


def test_masks_that_admit_nothing(mods):
    N, Q, k = 600, 5, 4
    p = sc.corpus(26, N, D, Q)
    idx = make_index(mods, p["x"], "f16", p["tags"])                      # tags on bits 0 .. 2
    cand = sc.mixed_list(N, 200)
    got = idx.query_subset(p["queries"], k, cand, require=np.uint64(1 << 40))
    assert (got[2] == 0).all() and (got[0] == -1).all() and np.isinf(got[1]).all() and (got[3] == 200).all()
    got = idx.query_subset(p["queries"], k, cand, require=np.uint64(1), exclude=np.uint64(1))
    assert (got[2] == 0).all() and (got[3] == 200).all()


# ================================================================================================ state
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_small_call_after_a_large_one_sees_nothing_stale(mods, dtype):
    N = 4999
    p = sc.corpus(27, N, D, 64)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    idx = make_index(mods, p["x"], dtype)
    big = lab[:4500]                                                      # near rows of the queries (noisy copies of rows 50 ..) included
    small = lab[4600:4640]                                                # disjoint from it
    for cand, k, Q in ((big, 1000, 64), (small, 2040, 5), (lab[4990:4993], 10, 1), (big, 3, 2)):
        got = idx.query_subset(p["queries"][:Q], k, cand)
        assert sc.mismatch(got, sc.expected_subset(p["queries"][:Q], k, cand, st, lab)) is None, (len(cand), k, Q)
        assert np.isin(got[0][got[0] >= 0], cand).all()


def test_after_add_update_and_remove(mods):
    N, Q, k = 1500, 5, 20
    p = sc.corpus(28, N, D, Q)
    x, lab = np.array(p["x"]), sc.labels_of(N)
    idx = make_index(mods, x, "f16", n=1000)
    cand = sc.mixed_list(N, 400)                                          # names rows behind the first 1000 too: unknown for now
    norm = lambda a: mods[1].normalize_rows(a, "f16")                     # noqa: E731
    with np.errstate(all="ignore"):
        assert sc.mismatch(idx.query_subset(p["queries"], k, cand), sc.expected_subset(p["queries"], k, cand, norm(x[:1000]), lab[:1000])) is None
        idx.add(x[1000:], lab[1000:])
        assert sc.mismatch(idx.query_subset(p["queries"], k, cand), sc.expected_subset(p["queries"], k, cand, norm(x), lab)) is None
        listed = sc.subset_rows(cand, lab)
        x[listed[:3]] = x[listed[3:6]] * 2.0
        idx.update(lab[listed[:3]], x[listed[:3]])
        assert sc.mismatch(idx.query_subset(p["queries"], k, cand), sc.expected_subset(p["queries"], k, cand, norm(x), lab)) is None
        # removed labels are unknown, and the dead rows behind count (the old last rows are still there) are never matched
        gone = np.concatenate([listed[5:200], [N - 1]])
        assert idx.remove(lab[gone]) == gone.size
        x2, lab2 = np.delete(x, gone, axis=0), np.delete(lab, gone)
        got = idx.query_subset(p["queries"], k, cand)
        assert sc.mismatch(got, sc.expected_subset(p["queries"], k, cand, norm(x2), lab2)) is None
        assert (got[3] == sc.subset_rows(cand, lab2).size).all() and got[3][0] <= listed.size - 195
        assert not np.isin(got[0], lab[gone]).any()
        got = idx.query_subset(p["queries"], k, lab)                      # every label that ever was
        assert sc.mismatch(got, sc.expected_subset(p["queries"], k, lab, norm(x2), lab2)) is None and (got[3] == lab2.size).all()


def test_state_arguments_and_counters(mods):
    import partition_cases as pc

    N, C, Q, k = 600, 7, 5, 4
    p = pc.clustered(16, N, D, C, Q)
    idx = make_index(mods, p["x"], "f16")
    st, lab = sc.stored_of(p["x"], "f16"), sc.labels_of(N)
    cand = sc.mixed_list(N, 200)
    bufs = lambda kk=k: (np.full((Q, kk), -77, np.int64), np.full((Q, kk), -5.0, np.float32), np.full(Q, -3, np.int32), np.full(Q, -9, np.int64))  # noqa: E731
    untouched = lambda b: (b[0] == -77).all() and (b[1] == -5.0).all() and (b[2] == -3).all() and (b[3] == -9).all()  # noqa: E731
    # a partition set before the call is still there afterwards, its counters and the guard's unchanged
    idx.set_partition(p["centres"], p["cells"])
    idx.query_probed(p["queries"], k, 2)
    idx.query(p["queries"], k)
    info, guard = idx.partition_info(), idx.guard_stats()
    exp = sc.expected_subset(p["queries"], k, cand, st, lab)
    assert sc.mismatch(idx.query_subset(p["queries"], k, cand), exp) is None
    assert idx.partition_info() == info and idx.guard_stats() == guard and info["cells"] == C
    # a null out_matched; host buffers of the caller's own
    b = bufs()
    assert raw_subset(mods, idx, p["queries"], k, cand, b[0], b[1], b[2], None) == 0 and (b[3] == -9).all()
    assert sc.mismatch(b[:3], exp[:3]) is None
    # every argument error, with the outputs untouched
    q = np.array(p["queries"])
    for kk, kw, status in ((2041, {}, ERR_UNSUPPORTED), (0, {}, ERR_ARG), (-1, {}, ERR_ARG), (k, {"Q": 0}, ERR_ARG), (k, {"Q": -2}, ERR_ARG),
                           (k, {"n_cand": -1}, ERR_ARG), (k, {"n_cand": 2 ** 31}, ERR_UNSUPPORTED)):
        b = bufs(max(kk, 1))
        assert raw_subset(mods, idx, q, kk, cand, *b, **kw) == status and untouched(b), (kk, kw)
    b = bufs()
    assert raw_subset(mods, idx, q, k, None, *b, n_cand=5) == ERR_ARG and untouched(b)        # a null list of five labels
    assert raw_subset(mods, idx, None, k, cand, *b, Q=Q) == ERR_ARG and untouched(b)          # null queries
    assert raw_subset(mods, idx, q, k, cand, None, b[1], b[2], b[3]) == ERR_ARG and untouched(b)
    assert raw_subset(mods, idx, q, k, cand, b[0], None, b[2], b[3]) == ERR_ARG and untouched(b)
    assert raw_subset(mods, idx, q, k, cand, b[0], b[1], None, b[3]) == ERR_ARG and untouched(b)
    assert idx._lib.mmiss_index_query_subset(None, mods[3].ptr(q), Q, k, mods[3].ptr(cand.copy()), cand.size, None, None, mods[3].ptr(b[0]),
                                             mods[3].ptr(b[1]), mods[3].ptr(b[2]), mods[3].ptr(b[3])) == ERR_ARG
    import torch

    dev_cnt = torch.full((Q,), -3, dtype=torch.int32, device="cuda")                          # host and device outputs mixed
    assert raw_subset(mods, idx, q, k, cand, b[0], b[1], dev_cnt, b[3]) == ERR_ARG and untouched(b) and (dev_cnt.cpu() == -3).all()
    # the wrapper checks before the library call
    for bad in (0, 2041):
        with pytest.raises(ValueError):
            idx.query_subset(q, bad, cand)
    with pytest.raises(TypeError):
        idx.query_subset(q, k, cand.astype(np.float64))
    with pytest.raises(ValueError):
        idx.query_subset(q[:0], k, cand)
    with pytest.raises(ValueError):
        idx.query_subset(q, k, torch.from_numpy(cand.copy()).cuda())                          # a CUDA list with host queries
    # an open query_begin: the call refuses and writes nothing
    pend = idx.query_begin(p["queries"], k)
    b = bufs()
    assert raw_subset(mods, idx, q, k, cand, *b) == ERR_STATE and untouched(b)
    pend.result()
    assert sc.mismatch(idx.query_subset(p["queries"], k, cand), exp) is None
    assert idx.partition_info() == info


# ================================================================================================ without the oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_tag_bit_63_on_the_listed_rows_gives_the_filtered_query(mods, dtype):
    N, Q, k = 4999, 64, 50
    p = sc.corpus(29, N, D, Q)
    lab = sc.labels_of(N)
    cand = sc.mixed_list(N, 1200)
    listed = np.isin(lab, cand)
    tags = np.array(p["tags"]) | (listed.astype(np.uint64) << np.uint64(63))
    idx = make_index(mods, p["x"], dtype, tags)
    bit = np.uint64(1 << 63)
    got = idx.query_subset(p["queries"], k, cand)
    assert sc.mismatch(got[:3], idx.query(p["queries"], k, require=bit)) is None and (got[3] == listed.sum()).all()
    req, exc = sc.query_masks(Q)
    got = idx.query_subset(p["queries"], k, cand, require=req, exclude=exc)
    assert sc.mismatch(got[:3], idx.query(p["queries"], k, require=req | bit, exclude=exc)) is None

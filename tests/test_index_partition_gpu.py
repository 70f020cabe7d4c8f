"""Partitioned search of the flat index (mmiss_index_partition_set / _query_probed and the calls around them) against the
restatement in tests/partition_cases.py: the probed cells by (canonical centre distance, index), the candidates by the cells as
given, and ro.query over the admitted candidates. Every comparison is equality of every element (distances by their bits,
scanned included). The edges of a call's plan — the scan's share of a list, the selection's segment, its levels, the query
chunks — are read from mmiss_dbg_index_probe_plan, so a test proves it crossed them."""
import numpy as np
import pytest

import partition_cases as pc
from index_query_cases import load_mods

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
D = 128
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5          # include/mmiss.h
SCRATCH_KB = 512 * 1024                                   # the default of the option probe_scratch_kb


@pytest.fixture(scope="module")
def mods():
    return load_mods()


def make_index(mods, x, dtype, tags=None, n=None):
    n = x.shape[0] if n is None else n
    idx = mods[0](x.shape[1], dtype)
    idx.add(x[:n], pc.labels_of(x.shape[0])[:n])
    if tags is not None:
        idx.set_tags(pc.labels_of(x.shape[0])[:n], tags[:n])
    return idx


def raw_probed(mods, idx, q, k, nprobe, lab, dist, cnt, scn, req=None, exc=None):
    """mmiss_index_query_probed itself, on the caller's buffers -> status"""
    lib = mods[3]
    q = np.ascontiguousarray(q, np.float32)
    return idx._lib.mmiss_index_query_probed(idx._h, lib.ptr(q), int(q.shape[0]), int(k), int(nprobe), lib.ptr(req), lib.ptr(exc), lib.ptr(lab),
                                             lib.ptr(dist), lib.ptr(cnt), lib.ptr(scn))


def raw_set(mods, idx, centres, cells, n=None):
    lib = mods[3]
    centres = np.ascontiguousarray(centres, np.float32)
    cells = np.ascontiguousarray(cells, np.int32)
    return idx._lib.mmiss_index_partition_set(idx._h, lib.ptr(centres) if centres.size else None, int(centres.shape[0]), lib.ptr(cells),
                                              int(cells.shape[0] if n is None else n))


# ================================================================================================ against the restatement
# (nprobe, k, Q, masks, device) per C, nprobe as "C" / "C+5" where it depends on C: over the four C every value the contract names
# is met — nprobe 1 / 3 / C / C + 5, k 1 / 10 / 1000 / 2040 (above the candidates included), Q 1 / 5 / 64 / 300
CALLS = {
    1: [(1, 10, 5, False, False), ("C+5", 2040, 1, True, True)],
    7: [(1, 1, 64, False, True), (3, 10, 300, True, False), ("C", 1000, 5, False, False), ("C+5", 2040, 5, True, True)],
    64: [(1, 10, 300, False, True), (3, 1000, 64, True, False), ("C", 10, 5, True, True)],
    1024: [(1, 2040, 5, False, False), (3, 10, 64, True, True), ("C", 1000, 1, False, True), ("C+5", 1, 300, False, False)],
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", sorted(CALLS))
def test_probed_equals_the_restatement(mods, dtype, C):
    import torch

    N = 4999 if C != 64 else 3001
    p = pc.clustered(11, N, D, C, 300)
    st, lab = pc.stored_of(p["x"], dtype), pc.labels_of(N)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    idx.set_partition(p["centres"], p["cells"])
    info = idx.partition_info()
    sizes = pc.cell_sizes(p["cells"], C)
    assert (info["cells"], info["rows"], info["tail"]) == (C, N, 0)
    assert (info["rows_in_cells"], info["largest_cell"], info["empty_cells"]) == (sizes.sum(), sizes.max(), (sizes == 0).sum())
    for nprobe, k, Q, masked, device in CALLS[C]:
        nprobe = {"C": C, "C+5": C + 5}.get(nprobe, nprobe)
        q = p["queries"][:Q]
        req, exc = pc.query_masks(Q) if masked else (None, None)
        exp = pc.expected_probed(q, k, nprobe, p["centres"], p["cells"], N, st, lab, p["tags"], req, exc)
        if device:
            tq = torch.from_numpy(np.array(q)).cuda()
            tm = [None if m is None else torch.from_numpy(m.view(np.int64).copy()).cuda() for m in (req, exc)]
            got = idx.query_probed(tq, k, nprobe, require=tm[0], exclude=tm[1])
            torch.cuda.synchronize()
            assert all(t.is_cuda for t in got)
            got = tuple(t.cpu().numpy() for t in got)
        else:
            got = idx.query_probed(q, k, nprobe, require=req, exclude=exc)
        msg = pc.mismatch(got, exp)
        assert msg is None, (dtype, C, nprobe, k, Q, masked, device, msg)
        if Q > 2:
            assert got[2][2] == 0 and got[3][2] == 0                    # the query without a direction


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [128, 512])
def test_all_cells_probed_equals_the_flat_query(mods, dtype, dim):
    N, C, Q, k = 3001, 7, 64, 10
    p = pc.clustered(12, N, dim, C, Q, complete=True)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    idx.set_partition(p["centres"], p["cells"])
    req, exc = pc.query_masks(Q)
    for nprobe in (C, C + 5):
        assert pc.mismatch(idx.query_probed(p["queries"], k, nprobe)[:3], idx.query(p["queries"], k)) is None
        got = idx.query_probed(p["queries"], k, nprobe, require=req, exclude=exc)
        assert pc.mismatch(got[:3], idx.query(p["queries"], k, require=req, exclude=exc)) is None
        assert (np.delete(got[3], 2) == N - 5).all()                    # every row with a direction was looked at
    # ... and it is the oracle's flat answer
    exp = pc.expected_flat(p["queries"], k, pc.stored_of(p["x"], dtype), pc.labels_of(N))
    assert pc.mismatch(idx.query_probed(p["queries"], k, C)[:3], exp) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_in_an_unprobed_cell_is_not_returned(mods, dtype):
    p = pc.hidden_row(D)
    N = p["x"].shape[0]
    idx = make_index(mods, p["x"], dtype)
    idx.set_partition(p["centres"], p["cells"])
    hidden = pc.labels_of(N)[p["hidden"]]
    st = pc.stored_of(p["x"], dtype)
    for nprobe, first in ((1, False), (2, True)):
        got = idx.query_probed(p["queries"], 5, nprobe)
        assert pc.mismatch(got, pc.expected_probed(p["queries"], 5, nprobe, p["centres"], p["cells"], N, st, pc.labels_of(N))) is None
        assert (hidden in got[0][0]) == first and (got[0][0, 0] == hidden) == first
        assert got[3][0] == (N if first else N // 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["dup", "mirror"])
def test_tied_centres_probe_the_smaller_index_first(mods, dtype, kind):
    p = pc.centre_ties(D, kind)
    N = p["x"].shape[0]
    a, b = p["tied"]
    idx = make_index(mods, p["x"], dtype)
    idx.set_partition(p["centres"], p["cells"])
    st, lab = pc.stored_of(p["x"], dtype), pc.labels_of(N)
    got = idx.query_probed(p["queries"], N, 1)
    assert got[3][0] == p["sizes"][a] and got[2][0] == p["sizes"][a]
    assert set(got[0][0, :got[2][0]].tolist()) == set(lab[p["cells"] == a].tolist())
    assert pc.mismatch(got, pc.expected_probed(p["queries"], N, 1, p["centres"], p["cells"], N, st, lab)) is None
    got = idx.query_probed(p["queries"], N, 2)
    assert got[3][0] == p["sizes"][a] + p["sizes"][b]
    assert pc.mismatch(got, pc.expected_probed(p["queries"], N, 2, p["centres"], p["cells"], N, st, lab)) is None


# ================================================================================================ edges of the plan
@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_edges_share_segment_levels_and_chunks(mods, dtype):
    lib = mods[3]
    p = pc.plan_edges(D)
    B, N, C = p["B"], p["x"].shape[0], len(pc.EDGE_SIZES)
    idx = make_index(mods, p["x"], dtype, n=B)
    idx.set_partition(p["centres"], p["cells"])
    idx.add(p["x"][B:], pc.labels_of(N)[B:])
    st, lab = pc.stored_of(p["x"], dtype), pc.labels_of(N)
    Q = p["queries"].shape[0]
    sizes = set(pc.EDGE_SIZES)
    # every cell probed: the planted winners at the first and the last position of every cell and of the tail are found
    exp = pc.expected_probed(p["queries"], 10, C, p["centres"], p["cells"], B, st, lab)
    got = idx.query_probed(p["queries"], 10, C)
    assert pc.mismatch(got, exp) is None
    assert np.array_equal(got[0][:, 0], lab[p["planted"]]) and (got[3] == N).all()
    # the same one query at a time: the share of a list per workgroup is smallest then, and the lists lie one below / at / above
    # it, as they lie around the selection's segment
    plan = lib.index_probe_plan(idx._h, 1, 10, C)
    assert {plan["share"] - 1, plan["share"], plan["share"] + 1} <= sizes, plan
    assert {plan["segment"] - 1, plan["segment"], plan["segment"] + 1} <= sizes, plan
    assert {0, 1} <= sizes and plan["levels"] >= 2 and plan["bound"] == N and plan["chunks"] == 1 and plan["splits"] > 1
    for q in range(Q):
        one = idx.query_probed(p["queries"][q:q + 1], 10, C)
        assert pc.mismatch(one, tuple(e[q:q + 1] for e in exp)) is None, q
    # one probe: a single list per query (and the tail), every list length of EDGE_SIZES among them
    got = idx.query_probed(p["queries"], 10, 1)
    exp = pc.expected_probed(p["queries"], 10, 1, p["centres"], p["cells"], B, st, lab)
    assert pc.mismatch(got, exp) is None
    assert len(set(exp[3].tolist())) >= 4
    # at least three selection levels
    plan = lib.index_probe_plan(idx._h, 3, 1000, C)
    assert plan["levels"] >= 3, plan
    got = idx.query_probed(p["queries"][:3], 1000, C)
    assert pc.mismatch(got, pc.expected_probed(p["queries"][:3], 1000, C, p["centres"], p["cells"], B, st, lab)) is None
    # several query chunks: the scratch budget lowered to two queries' key areas
    one = lib.index_probe_plan(idx._h, 1, 10, C)
    per_query_kb = (one["bound"] + -(-one["bound"] // one["segment"]) * 10) * 8 // 1024 + 1
    lib.set_option("probe_scratch_kb", 2 * per_query_kb)
    try:
        plan = lib.index_probe_plan(idx._h, Q, 10, C)
        assert plan["queries_per_chunk"] == 2 and plan["chunks"] == -(-Q // 2) >= 3, plan
        got = idx.query_probed(p["queries"], 10, C)
    finally:
        lib.set_option("probe_scratch_kb", SCRATCH_KB)
    assert pc.mismatch(got, pc.expected_probed(p["queries"], 10, C, p["centres"], p["cells"], B, st, lab)) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_rows_are_candidates_of_every_query(mods, dtype):
    N, C, Q = 3001, 7, 5
    p = pc.clustered(13, N + 100, D, C, Q)
    x = np.array(p["x"])
    # a tail row equal to query 0, whose nearest centre's cell does not hold it
    x[N + 50] = p["queries"][0]
    idx = make_index(mods, x, dtype, p["tags"], n=N)
    idx.set_partition(p["centres"], p["cells"][:N])
    idx.add(x[N:], pc.labels_of(N + 100)[N:])
    info = idx.partition_info()
    assert (info["cells"], info["rows"], info["tail"]) == (C, N, 100)
    with np.errstate(all="ignore"):
        st = mods[1].normalize_rows(x, dtype)
    lab = pc.labels_of(N + 100)
    tags = np.concatenate([p["tags"][:N], np.zeros(100, np.uint64)])     # rows are added with tag 0
    got = idx.query_probed(p["queries"], 10, 1)
    assert got[0][0, 0] == lab[N + 50]
    assert pc.mismatch(got, pc.expected_probed(p["queries"], 10, 1, p["centres"], p["cells"][:N], N, st, lab)) is None
    req, exc = pc.query_masks(Q)
    got = idx.query_probed(p["queries"], 10, 3, require=req, exclude=exc)
    assert pc.mismatch(got, pc.expected_probed(p["queries"], 10, 3, p["centres"], p["cells"][:N], N, st, lab, tags, req, exc)) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_small_call_after_a_large_one_sees_no_stale_scratch(mods, dtype):
    N, C = 4999, 64
    p = pc.clustered(14, N, D, C, 64)
    st, lab = pc.stored_of(p["x"], dtype), pc.labels_of(N)
    idx = make_index(mods, p["x"], dtype)
    idx.set_partition(p["centres"], p["cells"])
    for nprobe, k, Q in ((C, 1000, 64), (1, 3, 5), (2, 2040, 1)):
        got = idx.query_probed(p["queries"][:Q], k, nprobe)
        assert pc.mismatch(got, pc.expected_probed(p["queries"][:Q], k, nprobe, p["centres"], p["cells"], N, st, lab)) is None, (nprobe, k, Q)


# ================================================================================================ mutation, state, arguments
@pytest.mark.parametrize("via", ["update", "remove", "clear", "load"])
def test_what_moves_or_changes_rows_drops_the_partition(mods, via, tmp_path):
    N, C = 600, 7
    p = pc.clustered(15, N, D, C, 5, complete=True)
    lab = pc.labels_of(N)
    idx = make_index(mods, p["x"], "f16")
    idx.set_partition(p["centres"], p["cells"])
    idx.add(p["x"][:3], lab[-1] + 1 + np.arange(3))                      # add keeps it
    assert idx.partition_info()["cells"] == C and idx.partition_info()["tail"] == 3
    idx.query_probed(p["queries"], 5, 2)
    path = str(tmp_path / "ix.mmiss")
    idx.save(path)
    assert idx.partition_info()["cells"] == C                            # save neither drops nor persists it
    if via == "update":
        idx.update(lab[:1], p["x"][1:2])
    elif via == "remove":
        assert idx.remove(lab[5:6]) == 1
    elif via == "clear":
        idx.clear()
    else:
        idx.load(path)
    assert idx.partition_info() == dict.fromkeys(idx.PARTITION_INFO_FIELDS, 0)
    with pytest.raises(mods[3].MmissError) as e:
        idx.query_probed(p["queries"], 5, 2)
    assert e.value.code == ERR_STATE
    with pytest.raises(mods[3].MmissError) as e:
        idx.partition()
    assert e.value.code == ERR_STATE
    # the flat query is unaffected: the oracle's answer on the rows as they are now
    x_now, lab_now = np.concatenate([p["x"], p["x"][:3]]), np.concatenate([lab, lab[-1] + 1 + np.arange(3)])
    if via == "update":
        x_now[0] = p["x"][1]
    elif via == "remove":
        x_now, lab_now = np.delete(x_now, 5, axis=0), np.delete(lab_now, 5)
    elif via == "clear":
        x_now, lab_now = x_now[:0], lab_now[:0]
    with np.errstate(all="ignore"):
        exp = mods[1].query(p["queries"], mods[1].normalize_rows(x_now, "f16") if len(lab_now) else x_now.astype(np.float16), lab_now, 5)
    assert pc.mismatch(idx.query(p["queries"], 5), exp) is None
    idx.clear_partition()                                                # none set: nothing happens


def test_state_arguments_and_counters(mods):
    lib = mods[3]
    N, C, Q, k = 600, 7, 5, 4
    p = pc.clustered(16, N, D, C, Q)
    idx = make_index(mods, p["x"], "f16")
    bufs = lambda: (np.full((Q, k), -77, np.int64), np.full((Q, k), -5.0, np.float32), np.full(Q, -3, np.int32), np.full(Q, -9, np.int64))  # noqa: E731
    untouched = lambda b: (b[0] == -77).all() and (b[1] == -5.0).all() and (b[2] == -3).all() and (b[3] == -9).all()  # noqa: E731
    b = bufs()
    assert raw_probed(mods, idx, p["queries"], k, 2, *b) == ERR_STATE and untouched(b)      # no partition yet
    assert idx._lib.mmiss_index_partition_get(idx._h, None, None, 0, None) == ERR_STATE
    idx.set_partition(p["centres"], p["cells"])
    info = idx.partition_info()
    # refused calls keep the previous partition
    dead = np.zeros((3, D), np.float32)
    dead[1, 0] = np.nan
    dead[2, 3] = np.inf
    assert raw_set(mods, idx, p["centres"], p["cells"][:N - 1]) == ERR_ARG                  # n != count
    assert raw_set(mods, idx, np.zeros((0, D), np.float32), p["cells"]) == ERR_ARG          # C = 0
    assert raw_set(mods, idx, np.zeros((1025, D), np.float32) + 1, p["cells"]) == ERR_ARG   # C = 1025
    assert raw_set(mods, idx, dead, np.zeros(N, np.int32)) == ERR_ARG                       # no centre with a direction
    assert idx._lib.mmiss_index_partition_set(idx._h, None, C, lib.ptr(np.array(p["cells"])), N) == ERR_ARG
    assert idx.partition_info() == info
    cn, cells, sizes = idx.partition()
    assert np.array_equal(cells, p["cells"]) and np.array_equal(sizes, pc.cell_sizes(p["cells"], C))
    with np.errstate(all="ignore"):
        exp_cn = mods[1].normalize_rows(p["centres"], "f32")
    assert np.array_equal(cn.view(np.uint32), exp_cn.view(np.uint32))
    assert idx._lib.mmiss_index_partition_get(idx._h, None, lib.ptr(np.zeros(N - 1, np.int32)), N - 1, None) == ERR_ARG
    # argument checks of the probed call come before any write
    for kk, nprobe, status in ((2041, 2, ERR_UNSUPPORTED), (0, 2, ERR_ARG), (k, 0, ERR_ARG)):
        b = (np.full((Q, max(kk, 1)), -77, np.int64), np.full((Q, max(kk, 1)), -5.0, np.float32), np.full(Q, -3, np.int32), np.full(Q, -9, np.int64))
        assert raw_probed(mods, idx, p["queries"], kk, nprobe, *b) == status and untouched(b), (kk, nprobe)
    # an open query_begin: every partition call refuses
    pend = idx.query_begin(p["queries"], k)
    b = bufs()
    assert raw_probed(mods, idx, p["queries"], k, 2, *b) == ERR_STATE and untouched(b)
    assert raw_set(mods, idx, p["centres"], p["cells"]) == ERR_STATE
    assert idx._lib.mmiss_index_partition_clear(idx._h) == ERR_STATE
    pend.result()
    assert idx.partition_info() == info
    # the guard counters stay, the partition's own two advance by Q and by the rows scanned; a null out_scanned is legal
    before = idx.guard_stats()
    got = idx.query_probed(p["queries"], k, 2)
    b = bufs()
    assert raw_probed(mods, idx, p["queries"], k, 3, b[0], b[1], b[2], None) == 0 and (b[3] == -9).all()
    exp3 = pc.expected_probed(p["queries"], k, 3, p["centres"], p["cells"], N, pc.stored_of(p["x"], "f16"), pc.labels_of(N))
    assert pc.mismatch(b[:3], exp3[:3]) is None
    assert idx.guard_stats() == before
    after = idx.partition_info()
    assert after["queries"] - info["queries"] == 2 * Q and after["scanned"] - info["scanned"] == int(got[3].sum() + exp3[3].sum())
    # an empty index with a partition: counts 0
    empty = mods[0](D, "f16")
    empty.set_partition(p["centres"], np.zeros(0, np.int32))
    got = empty.query_probed(p["queries"], k, 2)
    assert (got[2] == 0).all() and (got[3] == 0).all() and (got[0] == -1).all() and np.isinf(got[1]).all()


@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_build_partition_round_trip(mods, dtype):
    import assign_cases as ac

    x = ac.kmeans_corpus()
    idx = make_index(mods, x, dtype)
    info = idx.build_partition(17, iters=5)
    cn, cells, sizes = idx.partition()
    assert info["cells"] == 17 and info["rows"] == x.shape[0] and info["tail"] == 0
    assert np.array_equal(cells, idx.assign(cn, want_dist=False)[0])
    assert np.array_equal(sizes, np.bincount(cells[cells >= 0], minlength=17)) and info["rows_in_cells"] == sizes.sum()
    q = x[:8]
    assert pc.mismatch(idx.query_probed(q, 10, 17)[:3], idx.query(q, 10)) is None
    got = idx.query_probed(q, 10, 2)
    exp = pc.expected_probed(q, 10, 2, cn, cells, x.shape[0], pc.stored_of(x, dtype), pc.labels_of(x.shape[0]))
    assert pc.mismatch(got, exp) is None

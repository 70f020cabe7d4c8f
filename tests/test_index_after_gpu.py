"""Search after on the flat index (mmiss_index_query_after) against the restatement in tests/after_cases.py: A(q) by np.isin, the
masks, ro.distances and the order of the float bits, then ro.query over A(q). Every comparison is equality of every element
(distances by their bits, remaining included). The edges of a call's plan — the scan's share, its query block, the selection's
segment and levels, the query chunks, dense or listed — are read from mmiss_dbg_index_after_plan, so a test proves it crossed
them."""
import numpy as np
import pytest

import after_cases as ac
from index_query_cases import load_mods

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
D = ac.D
N = 4999
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5          # include/mmiss.h
SCRATCH_KB = 512 * 1024                                   # the default of the option probe_scratch_kb
START = ac.START


@pytest.fixture(scope="module")
def mods():
    return load_mods()


def make_index(mods, x, dtype, tags=None, n=None, capacity=None):
    n = x.shape[0] if n is None else n
    idx = mods[0](x.shape[1], dtype) if capacity is None else mods[0](x.shape[1], dtype, capacity=capacity)
    idx.add(x[:n], ac.labels_of(x.shape[0])[:n])
    if tags is not None:
        idx.set_tags(ac.labels_of(x.shape[0])[:n], tags[:n])
    return idx


def raw_after(mods, idx, q, k, ad, al, lab, dist, cnt, rem, md=None, cand=None, n_cand=None, req=None, exc=None, Q=None):
    """mmiss_index_query_after itself, on the caller's buffers -> status"""
    lib = mods[3]
    q = None if q is None else np.ascontiguousarray(q, np.float32)
    ad = None if ad is None else np.ascontiguousarray(ad, np.float32)
    al = None if al is None else np.ascontiguousarray(al, np.int64)
    md = None if md is None else np.ascontiguousarray(md, np.float32)
    cand = None if cand is None else np.ascontiguousarray(cand, np.int64)
    n = (0 if cand is None else int(cand.shape[0])) if n_cand is None else n_cand
    return idx._lib.mmiss_index_query_after(idx._h, lib.ptr(q), int(q.shape[0]) if Q is None else Q, int(k), lib.ptr(ad), lib.ptr(al),
                                            lib.ptr(md), lib.ptr(cand), n, lib.ptr(req), lib.ptr(exc), lib.ptr(lab), lib.ptr(dist),
                                            lib.ptr(cnt), lib.ptr(rem))


def on_device(idx, q, k, ad, al, max_dist=None, labels=None, require=None, exclude=None):
    """query_after with every input a CUDA tensor -> numpy results"""
    import torch

    Q = np.asarray(q).reshape(-1, idx.dim).shape[0]
    cuda = lambda a, dt: torch.from_numpy(np.broadcast_to(np.asarray(a, dt).reshape(-1), (Q,)).copy()).cuda()   # noqa: E731
    kw = {}
    if max_dist is not None:
        kw["max_dist"] = cuda(max_dist, np.float32)
    if labels is not None:
        kw["labels"] = torch.from_numpy(np.array(labels, np.int64)).cuda()
    for name, m in (("require", require), ("exclude", exclude)):
        if m is not None:
            kw[name] = cuda(np.asarray(m).astype(np.uint64).view(np.int64), np.int64)
    got = idx.query_after(torch.from_numpy(np.array(q, np.float32)).cuda(), k, cuda(ad, np.float32), cuda(al, np.int64), **kw)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in got)
    return tuple(t.cpu().numpy() for t in got)


def pager(idx, q, device=False, **kw):
    """after_cases.chain's page function for ONE query on the index"""
    if device:
        return lambda k, ad, al: on_device(idx, q, k, ad, al, **kw)
    return lambda k, ad, al: idx.query_after(q, k, np.float32(ad), np.int64(al), **kw)


def oracle_kw(kw, tags=None):
    """query_after's keywords as after_cases.expected_after's"""
    out = {}
    if "labels" in kw:
        out["cand"] = kw["labels"]
    if "max_dist" in kw:
        out["max_dist"] = kw["max_dist"]
    if "require" in kw or "exclude" in kw:
        out.update(tags=tags, require=kw.get("require"), exclude=kw.get("exclude"))
    return out


# ================================================================================================ the first page
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_page_equals_the_librarys_own_calls(mods, dtype):
    n, Q, k = 3001, 64, 10
    p = ac.corpus(23, n, D, Q)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(n)
    q = p["queries"]
    req, exc = ac.query_masks(Q)
    # query / query_filtered
    got = idx.query_after(q, k, START, 0)
    assert ac.mismatch(got[:3], idx.query(q, k)) is None
    assert ac.mismatch(got, ac.expected_after(q, k, START, 0, st, lab)) is None
    assert got[3][0] == n - 5 and got[3][2] == 0                          # five rows without a direction; query 2 has none
    got = idx.query_after(q, k, START, 77, require=req, exclude=exc)      # (-inf: whatever the label)
    assert ac.mismatch(got[:3], idx.query(q, k, require=req, exclude=exc)) is None
    assert ac.mismatch(got, ac.expected_after(q, k, START, 0, st, lab, p["tags"], req, exc)) is None
    # query_subset
    for cand in (ac.mixed_list(n, 700), lab[::-1].copy()):
        got = on_device(idx, q, k, START, 0, labels=cand, require=req, exclude=exc)
        assert ac.mismatch(got[:3], idx.query_subset(q, k, cand, require=req, exclude=exc)[:3]) is None
        assert ac.mismatch(got, ac.expected_after(q, k, START, 0, st, lab, p["tags"], req, exc, cand=cand)) is None
    # query_radius at cap = k: the members are A, their total is what remains
    radius = np.sort(ac.all_distances(q[:1], st)[0])[40]
    for kw in (dict(), dict(require=req, exclude=exc)):
        got = idx.query_after(q, k, START, 0, max_dist=radius, **kw)
        assert ac.mismatch(got, idx.query_radius(q, radius, k, **kw)) is None
        assert ac.mismatch(got, ac.expected_after(q, k, START, 0, st, lab, max_dist=radius, **oracle_kw(kw, p["tags"]))) is None
    assert idx.query_after(q, k, START, 0, max_dist=radius)[3][0] == 41


# ================================================================================================ pages tile the ranking
@pytest.mark.parametrize("dtype", DTYPES)
def test_pages_tile_the_ranking(mods, dtype):
    p = ac.run_corpus(31, N)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(N)
    req, exc = ac.query_masks(4)
    q0, q3 = p["queries"][:1], p["queries"][3:4]
    assert mods[3].index_after_plan(idx._h, 1, 7)["dense"] == 1 and mods[3].index_after_plan(idx._h, 1, 7, 700)["dense"] == 0
    radius = np.sort(ac.all_distances(q3, st)[0])[900]
    longer = np.concatenate([lab, ac.UNKNOWN, lab[::-1]])                 # longer than the row count: every label twice
    # (query, the call's keywords, page sizes — the last one repeated —, device buffers)
    runs = [(q0, {}, (7,), False),                                        # through the run of 50 copies, page after page of 7
            (q0, {}, (10,), True),
            (q0, {}, (1000,), False),
            (q0, {}, (2040,), True),                                      # past position 2040 in two steps
            (q0, {}, (1, 7, 10, 1000, 2040, 3, 1), False),
            (q0, {"labels": ac.mixed_list(N, 700)}, (1,), False),         # every page a single entry
            (q3, {"require": req[3], "exclude": exc[3]}, (10, 1000, 7), True),
            (q3, {"labels": ac.sized_list(N, 3000)}, (1000,), False),
            (q3, {"labels": lab[::-1].copy()}, (2040, 1, 1000), True),
            (q3, {"labels": longer, "require": req[3]}, (1000, 10), False),
            (q3, {"labels": np.zeros(0, np.int64)}, (10,), False),
            (q3, {"labels": ac.UNKNOWN}, (10,), True),
            (q3, {"max_dist": radius}, (7, 100), False),
            (q3, {"max_dist": radius, "labels": ac.mixed_list(N, 700), "exclude": exc[3]}, (10,), True)]
    for q, kw, sizes, device in runs:
        full_l, full_d = ac.full_ranking(q, st, lab, **oracle_kw(kw, p["tags"]))
        got_l, got_d, pages = ac.chain(pager(idx, q, device, **kw), sizes)
        what = (dtype, sorted(kw), sizes, device)
        assert ac.same_ranking(got_l, got_d, full_l, full_d) is None, what
        assert ac.pages_consistent(pages, full_l.size) is None, what
    # the run: 50 entries at one distance, in label order, across eight page boundaries at k = 7
    got_l, got_d, _ = ac.chain(pager(idx, q0), (7,))
    run = slice(ac.NEARER, ac.NEARER + ac.RUN)
    assert np.array_equal(got_l[run], lab[p["run"]]) and np.unique(got_d[run].view(np.uint32)).size == 1
    assert got_l.size == N - 5 == np.unique(got_l).size > 2040
    assert ac.full_ranking(q3, st, lab, max_dist=radius)[0].size == 901


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_instance_width_and_a_cursor_of_its_own_per_query(mods, dtype):
    p = ac.run_corpus(31, N)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(N)
    lib = mods[3]
    qb = lib.index_after_plan(idx._h, 300, 10)["query_block"]
    assert qb == 16
    widths = (1, 2, 3, 5, qb, 64, 300)                                    # below / at / above the block: 300 = 18 blocks and 12 queries
    assert [lib.index_after_plan(idx._h, Q, 10)["first_chunk_block"] for Q in widths] == [1, 2, 4, 8, 16, 16, 16]
    first = ac.expected_after(p["queries"], 40, START, 0, st, lab)
    cand = ac.mixed_list(N, 700)
    for Q in widths:
        q = p["queries"][:Q]
        j = np.arange(Q)
        # per query in turn: the start, the middle of the ranking, past its end, NaN, the middle of the run (query 0: entry 17)
        ad = np.where(j % 4 == 0, START, np.where(j % 4 == 1, first[1][:Q, 17], np.where(j % 4 == 2, np.float32(np.inf), np.float32(np.nan))))
        ad = ad.astype(np.float32)
        al = np.where(j % 4 == 1, first[0][:Q, 17], 2 ** 62).astype(np.int64)
        if Q >= 5:
            ad[4], al[4] = first[1][0, 17], first[0][0, 17]
            q = q.copy()
            q[4] = q[0]
        req, exc = ac.query_masks(Q)
        for k, kw, device in ((10, {}, False), (7, {"require": req, "exclude": exc}, True), (1000, {"labels": cand}, Q > 5)):
            exp = ac.expected_after(q, k, ad, al, st, lab, **oracle_kw(kw, p["tags"]))
            got = on_device(idx, q, k, ad, al, **kw) if device else idx.query_after(q, k, ad, al, **kw)
            assert ac.mismatch(got, exp) is None, (dtype, Q, k, sorted(kw), ac.mismatch(got, exp))
        got = idx.query_after(q, 10, ad, al)
        assert (got[3][j % 4 >= 2] == 0).all() and (got[2][j % 4 >= 2] == 0).all()
        if Q >= 5:
            assert np.array_equal(got[0][4], first[0][0, 18:28]) and got[3][4] == N - 5 - 18


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [512, "max"])
def test_wider_rows_and_smaller_query_blocks(mods, dtype, dim):
    dim = ac.max_dim(dtype) if dim == "max" else dim
    n, Q, k = 700, 21, 10
    p = ac.corpus(22, n, dim, Q)
    idx = make_index(mods, p["x"], dtype, p["tags"])
    for n_cand in (None, 300):
        plan = mods[3].index_after_plan(idx._h, Q, k, n_cand)
        assert plan["query_block"] == {512: 16, 1920: 8, 3968: 4}[dim] and plan["lds_bytes"] == plan["query_block"] * dim * 4 <= 65536
        assert Q % plan["query_block"] != 0 and Q > plan["query_block"] and plan["dense"] == (n_cand is None)
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(n)
    req, exc = ac.query_masks(Q)
    first = ac.expected_after(p["queries"], k, START, 0, st, lab)
    assert ac.mismatch(idx.query_after(p["queries"], k, START, 0), first) is None
    ad, al = first[1][:, k - 1].copy(), first[0][:, k - 1].copy()        # the second page (query 2: +inf / -1, nothing)
    for kw in ({}, {"require": req, "exclude": exc}, {"labels": ac.mixed_list(n, 300)}):
        exp = ac.expected_after(p["queries"], k, ad, al, st, lab, **oracle_kw(kw, p["tags"]))
        assert ac.mismatch(idx.query_after(p["queries"], k, ad, al, **kw), exp) is None, sorted(kw)
    full_l, full_d = ac.full_ranking(p["queries"][:1], st, lab)
    got_l, got_d, pages = ac.chain(pager(idx, p["queries"][:1]), (300, 7))
    assert ac.same_ranking(got_l, got_d, full_l, full_d) is None and ac.pages_consistent(pages, n - 5) is None


# ================================================================================================ cursors and radii off the ranking
@pytest.mark.parametrize("dtype", DTYPES)
def test_cursors_off_the_ranking_and_radius_values(mods, dtype):
    n, Q, k = 600, 5, 6
    p = ac.corpus(32, n, D, Q)
    idx = make_index(mods, p["x"], dtype)
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(n)
    q = p["queries"]
    first = ac.expected_after(q, 12, START, 0, st, lab)
    d3, d4, l3 = first[1][0, 3], first[1][0, 4], first[0][0, 3]
    assert d3 < d4
    mid = np.float32((np.float64(d3) + np.float64(d4)) / 2)
    below, above = np.nextafter(d3, np.float32(-1)), np.nextafter(d3, np.float32(9))
    cursors = [(mid, -1), (mid, 2 ** 62),                                 # between two entries, any label
               (d3, l3 - 1), (d3, l3), (d3, l3 + 1), (d3, -2 ** 63), (d3, 2 ** 63 - 1),   # at an entry's distance, labels around its own
               (below, 2 ** 62), (above, -1),                             # one float below / above it
               (np.float32(np.inf), 0), (np.float32(np.nan), 0), (np.float32(-0.0), 0), (np.float32(0.0), 0), (np.float32(-3.0), 5)]
    for ad, al in cursors:
        exp = ac.expected_after(q, k, ad, al, st, lab)
        assert ac.mismatch(idx.query_after(q, k, ad, al), exp) is None, (ad, al)
        assert ac.mismatch(on_device(idx, q, k, ad, al), exp) is None, (ad, al)
    assert idx.query_after(q[:1], k, d3, l3 - 1)[0][0, 0] == l3 and idx.query_after(q[:1], k, d3, l3)[0][0, 0] == first[0][0, 4]
    assert idx.query_after(q[:1], k, below, 2 ** 62)[0][0, 0] == l3 and idx.query_after(q[:1], k, above, -1)[0][0, 0] == first[0][0, 4]
    # the label of a removed row: the page continues behind where it was
    assert idx.remove(np.array([l3, first[0][0, 4]])) == 2
    st2, lab2 = st[np.isin(lab, [l3, first[0][0, 4]], invert=True)], lab[np.isin(lab, [l3, first[0][0, 4]], invert=True)]
    for ad, al in ((d3, l3), (d4, first[0][0, 4]), (d3, l3 - 1)):
        got = idx.query_after(q, k, ad, al)
        assert ac.mismatch(got, ac.expected_after(q, k, ad, al, st2, lab2)) is None
        assert got[0][0, 0] == first[0][0, 5] and got[3][0] == n - 5 - 5
    # max_dist: a row's own distance bits (in), one float below (out), NaN, +inf, a value below the cursor
    d7 = first[1][0, 7]
    for md, members in ((d7, 6), (np.nextafter(d7, np.float32(-1)), 5), (np.float32(np.nan), 0), (np.float32(np.inf), n - 7), (np.float32(-1.0), 0)):
        got = idx.query_after(q, k, START, 0, max_dist=md)
        assert ac.mismatch(got, ac.expected_after(q, k, START, 0, st2, lab2, max_dist=md)) is None, md
        assert got[3][0] == members, (md, got[3][0])
        md_q = np.array([md, d7, np.nan, np.inf, -1.0], np.float32)       # one radius per query
        ad_q, al_q = first[1][:, 5].copy(), first[0][:, 5].copy()
        exp = ac.expected_after(q, k, ad_q, al_q, st2, lab2, max_dist=md_q)
        assert ac.mismatch(on_device(idx, q, k, ad_q, al_q, max_dist=md_q), exp) is None
    got = idx.query_after(q[:1], k, first[1][0, 9], first[0][0, 9], max_dist=d7)       # the radius lies below the cursor
    assert got[2][0] == 0 and got[3][0] == 0 and (got[0] == -1).all()


# ================================================================================================ edges of the plan
@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_edges_share_segment_levels_and_chunks(mods, dtype):
    lib = mods[3]
    n = ac.BIG_N
    p = ac.corpus(25, n, D, 8)
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(n)
    q1, q3 = p["queries"][:1], p["queries"][:3]
    # dense: the index grows through the sizes one below / at / above the scan's share and the selection's segment
    idx = mods[0](D, dtype)
    have = 0
    for m in (63, 64, 65, 4095, 4096, 4097):
        idx.add(p["x"][have:m], lab[have:m])
        have = m
        plan = lib.index_after_plan(idx._h, 1, 10)
        assert plan["dense"] == 1 and plan["bound"] == m and plan["share"] == 64 and plan["segment"] == 4096
        assert plan["splits"] == -(-m // 64) and plan["levels"] == (2 if m > 4096 else 1), plan
        first = ac.expected_after(q1, 10, START, 0, st[:m], lab[:m])
        assert ac.mismatch(idx.query_after(q1, 10, START, 0), first) is None, m
        ad, al = first[1][0, 9], first[0][0, 9]
        assert ac.mismatch(idx.query_after(q1, 10, ad, al), ac.expected_after(q1, 10, ad, al, st[:m], lab[:m])) is None, m
    idx.add(p["x"][have:], lab[have:])
    first = ac.expected_after(q3, 1000, START, 0, st, lab)
    ad, al = first[1][:, 499].copy(), first[0][:, 499].copy()            # (query 2: no direction)
    # listed: |S| around the share and the segment, the cursor in the middle of the list's ranking
    share = lib.index_after_plan(idx._h, 1, 10, 65)["share"]
    assert share == 64
    for m in (share - 1, share, share + 1, 4095, 4096, 4097):
        plan = lib.index_after_plan(idx._h, 1, 10, m)
        assert plan["dense"] == 0 and plan["bound"] == m and plan["levels"] == (2 if m > 4096 else 1) and plan["splits"] == -(-m // share)
        cand = ac.sized_list(n, m, seed=m)
        page = ac.expected_after(q1, 10, START, 0, st, lab, cand=cand)
        c_ad, c_al = page[1][0, 4], page[0][0, 4]
        assert ac.mismatch(idx.query_after(q1, 10, c_ad, c_al, labels=cand), ac.expected_after(q1, 10, c_ad, c_al, st, lab, cand=cand)) is None, m
    # two and three selection levels (k = 1000: above 4096 and above 16 384 keys), several queries, dense and listed
    plan = lib.index_after_plan(idx._h, 3, 1000)
    assert plan["levels"] == 3 and plan["chunks"] == 1 and plan["bound"] == n, plan
    assert ac.mismatch(idx.query_after(q3, 1000, START, 0), first) is None
    assert ac.mismatch(idx.query_after(q3, 1000, ad, al), ac.expected_after(q3, 1000, ad, al, st, lab)) is None
    for m, levels in ((5000, 2), (16500, 3)):
        assert lib.index_after_plan(idx._h, 3, 1000, m)["levels"] == levels
        cand = ac.sized_list(n, m, seed=m)
        assert ac.mismatch(idx.query_after(q3, 1000, ad, al, labels=cand), ac.expected_after(q3, 1000, ad, al, st, lab, cand=cand)) is None, m
    # several query chunks: the scratch budget lowered to three queries' key areas (a chunk is then no multiple of the query block)
    Q = 8
    q = p["queries"]
    first = ac.expected_after(q, 10, START, 0, st, lab)
    ad, al = first[1][:, 6].copy(), first[0][:, 6].copy()
    req, exc = ac.query_masks(Q)
    for n_cand, kw in ((None, {}), (5000, {"labels": ac.sized_list(n, 5000, seed=5000)})):
        one = lib.index_after_plan(idx._h, 1, 10, n_cand)
        per_query_kb = (one["stride0"] + one["stride1"]) * 8 // 1024 + 1
        lib.set_option("probe_scratch_kb", 3 * per_query_kb)
        try:
            plan = lib.index_after_plan(idx._h, Q, 10, n_cand)
            assert plan["queries_per_chunk"] == 3 and plan["chunks"] == 3 and (plan["first_chunk_block"], plan["last_chunk_block"]) == (4, 2), plan
            got = idx.query_after(q, 10, ad, al, **kw)
        finally:
            lib.set_option("probe_scratch_kb", SCRATCH_KB)
        assert ac.mismatch(got, ac.expected_after(q, 10, ad, al, st, lab, **oracle_kw(kw))) is None, n_cand


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_dense_scan_past_its_first_trips(mods, dtype):
    n, Q, k = ac.DENSE_N, 3, 10
    p = ac.corpus(26, n, D, Q)
    idx = make_index(mods, p["x"], dtype, capacity=n)
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(n)
    plan = mods[3].index_after_plan(idx._h, Q, k)
    assert plan["dense"] == 1 and plan["share"] > 64 and plan["share"] > plan["rows_per_trip"] * 4 and n % 16 != 0
    assert plan["first_chunk_block"] == 4 and plan["splits"] * plan["share"] > n > (plan["splits"] - 1) * plan["share"]
    q = p["queries"]
    d = ac.all_distances(q, st)
    order = np.lexsort((lab, d[0]))
    mid = order[(n - 5) // 2]                                             # the middle of query 0's ranking
    ad = np.array([d[0, mid], START, START], np.float32)
    al = np.array([lab[mid], 0, 0], np.int64)
    exp = ac.expected_after(q, k, ad, al, st, lab)
    got = idx.query_after(q, k, ad, al)
    assert ac.mismatch(got, exp) is None, ac.mismatch(got, exp)
    assert got[3][0] == (n - 5) - ((n - 5) // 2 + 1) and got[3][1] == n - 5 and got[3][2] == 0


# ================================================================================================ dead rows behind count
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["copies", "nan"])
def test_dead_rows_behind_count_are_never_ranked_or_counted(mods, dtype, kind, tmp_path):
    """The capacity is filled with ghost rows — bit copies of the query directions (the nearest rows there can be), or NaN rows —,
    the index is emptied (by clear; by removing every row; by clear and then a load of a cut-off file of the ghosts, which fails),
    and fewer live rows are added: the ghosts behind count are still in device memory. Dense and listed calls give the oracle's
    bits, no ghost label, and the oracle's remaining."""
    G, n, Q, k = 600, 211, 5, 8
    p = ac.corpus(33, G, D, Q)
    q = p["queries"]
    live_x, live_lab = p["x"][:n], ac.labels_of(G)[:n]
    ghost_lab = ac.labels_of(G) + 1                                       # never a live label
    ghosts = np.ascontiguousarray(q[np.arange(G) % Q]) if kind == "copies" else np.full((G, D), np.nan, np.float32)
    if kind == "copies":
        ghosts[2::Q] = q[0]                                               # (query 2 has no direction)
    st = ac.stored_of(live_x, dtype)
    cand = np.concatenate([live_lab[::2], ghost_lab[:300], live_lab[:10]])
    idx = mods[0](D, dtype, capacity=G)
    path = tmp_path / "ghosts.idx"
    for via in ("clear", "remove_all", "failed_load"):
        idx.add(ghosts, ghost_lab)
        assert idx.count() == G
        if kind == "copies":
            assert idx.query_after(q[:1], k, START, 0)[1][0, 0] < 1e-2    # the ghosts are the nearest rows while they live
        if via == "remove_all":
            assert idx.remove(ghost_lab) == G
        else:
            if via == "failed_load":
                idx.save(str(path))
            idx.clear()
            if via == "failed_load":
                blob = path.read_bytes()
                path.write_bytes(blob[:len(blob) // 2])
                with pytest.raises(RuntimeError):
                    idx.load(str(path))
        assert idx.count() == 0
        nothing = idx.query_after(q, k, START, 0)
        assert (nothing[2] == 0).all() and (nothing[3] == 0).all() and (nothing[0] == -1).all()
        assert (idx.query_after(q, k, START, 0, labels=ghost_lab)[3] == 0).all()
        idx.add(live_x, live_lab)
        first = ac.expected_after(q, k, START, 0, st, live_lab)
        ad, al = first[1][:, 3].copy(), first[0][:, 3].copy()
        for kw in ({}, {"labels": cand}, {"labels": ghost_lab}):
            for a, b in ((START, 0), (ad, al)):
                exp = ac.expected_after(q, k, a, b, st, live_lab, **oracle_kw(kw))
                got = idx.query_after(q, k, a, b, **kw)
                assert ac.mismatch(got, exp) is None, (via, sorted(kw), ac.mismatch(got, exp))
                assert not np.isin(got[0], ghost_lab).any()
        assert idx.query_after(q, k, START, 0)[3][0] == n - 2             # rows 3 and 17 have no direction
        idx.clear()


# ================================================================================================ state
def test_buffers_stale_scratch_and_changes_between_pages(mods):
    n, Q, k = 1500, 5, 20
    p = ac.corpus(28, n, D, Q)
    x, lab = np.array(p["x"]), ac.labels_of(n)
    idx = make_index(mods, x, "f16", n=1000)
    q = p["queries"]
    norm = lambda a: mods[1].normalize_rows(a, "f16")                     # noqa: E731
    with np.errstate(all="ignore"):
        st = norm(x[:1000])
        page1 = idx.query_after(q, k, START, 0)
        assert ac.mismatch(page1, ac.expected_after(q, k, START, 0, st, lab[:1000])) is None
        ad, al = page1[1][:, k - 1].copy(), page1[0][:, k - 1].copy()
        # a small call after a large one (k = 2040 over every row, then one query, k = 3, a short list)
        idx.query_after(q, 2040, START, 0)
        short = lab[990:996]
        assert ac.mismatch(idx.query_after(q[:1], 3, START, 0, labels=short), ac.expected_after(q[:1], 3, START, 0, st, lab[:1000], cand=short)) is None
        assert ac.mismatch(idx.query_after(q, k, ad, al), ac.expected_after(q, k, ad, al, st, lab[:1000])) is None
        # rows added, updated and removed between two pages are ranked as they stand at the second call
        idx.add(x[1000:], lab[1000:])
        assert ac.mismatch(idx.query_after(q, k, ad, al), ac.expected_after(q, k, ad, al, norm(x), lab)) is None
        near = page1[0][0, :3]                                            # three rows of the first page move away,
        rows = (near - 5) // 3
        x[rows] = -x[rows]
        idx.update(near, x[rows])
        far = np.argsort(np.nan_to_num(ac.all_distances(q[:1], norm(x))[0], nan=-1.0))[-2:]
        x[far] = q[0] * np.float32(2.0)                                   # two far rows become copies of the query: they rank BEFORE the cursor
        idx.update(lab[far], x[far])
        got = idx.query_after(q, k, ad, al)
        assert ac.mismatch(got, ac.expected_after(q, k, ad, al, norm(x), lab)) is None
        assert not np.isin(lab[far], got[0][0]).any()
        gone = np.unique(np.concatenate([[al[0]], got[0][0, :5], [lab[n - 1]]]))     # the cursor's own row, the page's first five, the last row
        assert idx.remove(gone) == gone.size
        keep = ~np.isin(lab, gone)
        got = idx.query_after(q, k, ad, al)
        assert ac.mismatch(got, ac.expected_after(q, k, ad, al, norm(x[keep]), lab[keep])) is None
        assert not np.isin(got[0], gone).any()


def test_state_arguments_and_counters(mods):
    import partition_cases as pc
    import torch

    n, C, Q, k = 600, 7, 5, 4
    p = pc.clustered(16, n, D, C, Q)
    idx = make_index(mods, p["x"], "f16")
    st, lab = ac.stored_of(p["x"], "f16"), ac.labels_of(n)
    cand = ac.mixed_list(n, 200)
    q = np.array(p["queries"])
    first = ac.expected_after(q, k, START, 0, st, lab)
    ad, al = first[1][:, 1].copy(), first[0][:, 1].copy()
    exp = ac.expected_after(q, k, ad, al, st, lab)
    bufs = lambda kk=k: (np.full((Q, kk), -77, np.int64), np.full((Q, kk), -5.0, np.float32), np.full(Q, -3, np.int32), np.full(Q, -9, np.int64))  # noqa: E731
    untouched = lambda b: (b[0] == -77).all() and (b[1] == -5.0).all() and (b[2] == -3).all() and (b[3] == -9).all()  # noqa: E731
    # a partition set before the call is still there afterwards, its counters and the guard's unchanged
    idx.set_partition(p["centres"], p["cells"])
    idx.query_probed(p["queries"], k, 2)
    idx.query(p["queries"], k)
    info, guard = idx.partition_info(), idx.guard_stats()
    assert ac.mismatch(idx.query_after(q, k, ad, al), exp) is None
    assert ac.mismatch(idx.query_after(q, k, ad, al, labels=cand, max_dist=0.9), ac.expected_after(q, k, ad, al, st, lab, cand=cand, max_dist=0.9)) is None
    assert idx.partition_info() == info and idx.guard_stats() == guard and info["cells"] == C
    # host buffers of the caller's own; a null out_remaining; a null list with n_cand = 0 is no list
    b = bufs()
    assert raw_after(mods, idx, q, k, ad, al, *b) == 0 and ac.mismatch(b, exp) is None
    b = bufs()
    assert raw_after(mods, idx, q, k, ad, al, b[0], b[1], b[2], None) == 0 and (b[3] == -9).all() and ac.mismatch(b[:3], exp[:3]) is None
    b = bufs()
    assert raw_after(mods, idx, q, k, ad, al, *b, cand=np.zeros(1, np.int64), n_cand=0) == 0           # the empty list: nothing
    assert (b[2] == 0).all() and (b[3] == 0).all() and (b[0] == -1).all() and np.isinf(b[1]).all()
    # device outputs with host inputs, and without out_remaining
    d = (torch.full((Q, k), -77, dtype=torch.int64, device="cuda"), torch.full((Q, k), -5.0, device="cuda"),
         torch.full((Q,), -3, dtype=torch.int32, device="cuda"), torch.full((Q,), -9, dtype=torch.int64, device="cuda"))
    assert raw_after(mods, idx, q, k, ad, al, *d) == 0
    assert ac.mismatch(tuple(t.cpu().numpy() for t in d), exp) is None
    assert raw_after(mods, idx, q, k, START.reshape(1).repeat(Q), al, d[0], d[1], d[2], None) == 0
    assert ac.mismatch(tuple(t.cpu().numpy() for t in d[:3]), first[:3]) is None and ac.mismatch((d[3].cpu().numpy(),), (exp[3],)) is None
    # every argument error, with the outputs untouched
    for kk, kw, status in ((2041, {}, ERR_UNSUPPORTED), (0, {}, ERR_ARG), (-1, {}, ERR_ARG), (k, {"Q": 0}, ERR_ARG), (k, {"Q": -2}, ERR_ARG),
                           (k, {"cand": cand, "n_cand": -1}, ERR_ARG), (k, {"n_cand": 5}, ERR_ARG), (k, {"cand": cand, "n_cand": 2 ** 31}, ERR_UNSUPPORTED)):
        b = bufs(max(kk, 1))
        assert raw_after(mods, idx, q, kk, ad, al, *b, **kw) == status and untouched(b), (kk, kw)
    b = bufs()
    assert raw_after(mods, idx, None, k, ad, al, *b, Q=Q) == ERR_ARG and untouched(b)                  # null queries
    assert raw_after(mods, idx, q, k, None, al, *b) == ERR_ARG and untouched(b)                        # null cursors
    assert raw_after(mods, idx, q, k, ad, None, *b) == ERR_ARG and untouched(b)
    assert raw_after(mods, idx, q, k, ad, al, None, b[1], b[2], b[3]) == ERR_ARG and untouched(b)
    assert raw_after(mods, idx, q, k, ad, al, b[0], None, b[2], b[3]) == ERR_ARG and untouched(b)
    assert raw_after(mods, idx, q, k, ad, al, b[0], b[1], None, b[3]) == ERR_ARG and untouched(b)
    lib = mods[3]
    assert idx._lib.mmiss_index_query_after(None, lib.ptr(q), Q, k, lib.ptr(ad), lib.ptr(al), None, None, 0, None, None, lib.ptr(b[0]),
                                            lib.ptr(b[1]), lib.ptr(b[2]), lib.ptr(b[3])) == ERR_ARG
    dev_cnt = torch.full((Q,), -3, dtype=torch.int32, device="cuda")                                   # host and device outputs mixed
    assert raw_after(mods, idx, q, k, ad, al, b[0], b[1], dev_cnt, b[3]) == ERR_ARG and untouched(b) and (dev_cnt.cpu() == -3).all()
    # the wrapper checks before the library call
    for bad in (0, 2041):
        with pytest.raises(ValueError):
            idx.query_after(q, bad, ad, al)
    with pytest.raises(TypeError):
        idx.query_after(q, k, ad, al, labels=cand.astype(np.float64))
    with pytest.raises(TypeError):
        idx.query_after(q, k, ad, al.astype(np.float64))
    with pytest.raises(ValueError):
        idx.query_after(q, k, ad[:3], al)
    with pytest.raises(ValueError):
        idx.query_after(q[:0], k, ad[:0], al[:0])
    with pytest.raises(ValueError):
        idx.query_after(q, k, torch.from_numpy(ad).cuda(), al)                                         # a CUDA cursor with host queries
    # no cursor value is an error
    weird = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45], np.float32)
    assert ac.mismatch(idx.query_after(q, k, weird, al), ac.expected_after(q, k, weird, al, st, lab)) is None
    # an open query_begin: the call refuses and writes nothing
    pend = idx.query_begin(p["queries"], k)
    b = bufs()
    assert raw_after(mods, idx, q, k, ad, al, *b) == ERR_STATE and untouched(b)
    pend.result()
    assert ac.mismatch(idx.query_after(q, k, ad, al), exp) is None
    assert idx.partition_info() == info


# ================================================================================================ without the oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_pages_of_100_are_the_flat_query_at_2040(mods, dtype):
    n = 3000
    p = ac.run_corpus(34, n, D, 4)
    idx = make_index(mods, p["x"], dtype)
    for qi in (0, 3):
        q = p["queries"][qi:qi + 1]
        flat = idx.query(q, 2040)
        lab, dist = idx.ranking(q[0], n, page=100)
        assert lab.shape == (n - 5,) and dist.shape == (n - 5,) and lab.dtype == np.int64 and dist.dtype == np.float32
        assert ac.same_ranking(lab[:2040], dist[:2040], flat[0][0], flat[1][0]) is None
        assert np.unique(lab).size == n - 5 and (np.diff(ac.mono(dist).astype(np.int64)) >= 0).all()
        same = np.diff(ac.mono(dist).astype(np.int64)) == 0
        assert (np.diff(lab)[same] > 0).all() and (same.sum() >= ac.RUN - 1 or qi != 0)
    # ranking() on the device, a shorter n, a page that does not divide it
    import torch

    lab, dist = idx.ranking(p["queries"][0], 250, page=100)
    tl, td = idx.ranking(torch.from_numpy(np.array(p["queries"][0])).cuda(), 250, page=99)
    assert tl.is_cuda and lab.shape == (250,) and ac.same_ranking(tl.cpu().numpy(), td.cpu().numpy(), lab, dist) is None

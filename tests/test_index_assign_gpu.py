"""Nearest-centre assignment, cluster sums and k-means of the flat index (mmiss_index_assign, mmiss_index_cluster_sums,
FlatIndex.kmeans) against the restatement in tests/assign_cases.py: row r goes to the c that minimises (Dm[c, r], c) over the
non-NaN entries of Dm = oracle.retrieval_oracle.distances(centres, stored). Every comparison is equality of every element
(distances by their bits). Which route decided what is read from the guard statistics: radius_pages (passes over the index),
swept_rows (borderline rows x centres with a direction).

Two things the corpora build in instead of leaving them to chance:
  * the random corpus carries ONE row that is equidistant by construction from two centres (assign_cases.random_corpus, C >= 16),
    so "some row is borderline" does not rest on what the random rows happen to score; the upper bound N C / 2 is untouched;
  * "every row with a direction is borderline" needs EVERY centre duplicated, not one (a row whose best centre is not the
    duplicated one has an ordinary gap): assign_cases.duplicate_corpus has centres[K + i] = centres[i]. The single duplicate and
    the one-ulp centre of the issue are the ties corpus, compared with the oracle like everything else."""
import numpy as np
import pytest

import assign_cases as ac
from index_query_cases import load_mods

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
D = 128
ALL_C = [1, 15, 16, 17, 64, 65, 130]
ERR_ARG, ERR_STATE = -1, -3          # include/mmiss.h


@pytest.fixture(scope="module")
def mods():
    return load_mods()


def labels_of(n):
    return np.arange(n, dtype=np.int64) * 3 + 5


def make_index(mods, x, dtype, dim=D):
    idx = mods[0](dim, dtype)
    idx.add(x, labels_of(x.shape[0]))
    return idx


def delta(idx, before):
    after = idx.guard_stats()
    return {k: after[k] - before[k] for k in after}


def raw_assign(mods, idx, c, out_assign, out_dist, cap, out_sizes):
    """mmiss_index_assign itself, on the caller's buffers -> status"""
    lib = mods[3]
    c = np.ascontiguousarray(c, np.float32)
    return idx._lib.mmiss_index_assign(idx._h, lib.ptr(c) if c.size else None, int(c.shape[0]), lib.ptr(out_assign), lib.ptr(out_dist), int(cap),
                                       lib.ptr(out_sizes))


def check_call(mods, idx, x, c, dtype, dim=D, routes=True):
    """one assign on host buffers against the restatement, with the accounting -> the statistics' delta"""
    N, C = x.shape[0], c.shape[0]
    exp = ac.expected_of(x, c, dtype)[1:]
    before = idx.guard_stats()
    got = idx.assign(c)
    dl = delta(idx, before)
    msg = ac.mismatch(got, exp)
    assert msg is None, (dtype, N, C, msg)
    if routes:
        assert dl["radius_queries"] == C and dl["radius_pages"] == ac.expected_passes(C, dim, dtype), (dtype, C, dl)
        assert all(dl[s] == 0 for s in ("queries", "widened", "rounds", "pages", "exhaustive")), dl
        assert 0 <= dl["swept_rows"] < N * C / 2 or C == 1, (dtype, N, C, dl)
    return dl


# ================================================================================================ 1. oracle equality, 4. routes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", ALL_C)
def test_assign_equals_the_oracle(mods, dtype, C):
    import torch

    N = 4999
    x, c = ac.random_corpus(21, N, D, C)
    a, d, s = ac.expected_of(x, c, dtype)[1:]
    idx = make_index(mods, x, dtype)
    dl = check_call(mods, idx, x, c, dtype)
    live = C - (1 if C > 1 else 0)
    assert dl["swept_rows"] % live == 0
    if C >= 16:
        assert dl["swept_rows"] >= live, dl            # the planted equidistant row is borderline by construction
    if C == 1:
        assert dl["swept_rows"] == 0                   # one live centre: every row is sure
    nd = ac.nodir_rows(N)
    assert (a[nd] == -1).all() and (C == 1 or s[1] == 0)
    # without distances
    ga, gd, gs = idx.assign(c, want_dist=False)
    assert gd is None and ac.mismatch((ga, None, gs), (a, d, s)) is None
    # device inputs and outputs
    ta, td, ts = idx.assign(torch.from_numpy(np.array(c)).cuda())
    assert ta.is_cuda and td.is_cuda and ts.is_cuda and ta.dtype == torch.int32 and ts.dtype == torch.int64
    torch.cuda.synchronize()
    assert ac.mismatch((ta.cpu().numpy(), td.cpu().numpy(), ts.cpu().numpy()), (a, d, s)) is None
    ta, td, ts = idx.assign(torch.from_numpy(np.array(c)).cuda(), want_dist=False)
    assert td is None and ac.mismatch((ta.cpu().numpy(), None, ts.cpu().numpy()), (a, d, s)) is None
    # a larger output buffer: what lies behind count stays untouched
    oa, od, os_ = np.full(N + 9, -77, np.int32), np.full(N + 9, -5.0, np.float32), np.full(C, -3, np.int64)
    assert raw_assign(mods, idx, c, oa, od, N + 9, os_) == 0
    assert ac.mismatch((oa[:N].copy(), od[:N].copy(), os_), (a, d, s)) is None
    assert (oa[N:] == -77).all() and (od[N:] == -5.0).all()
    # null out_dist and null out_sizes
    oa2 = np.full(N, -77, np.int32)
    assert raw_assign(mods, idx, c, oa2, None, N, None) == 0 and np.array_equal(oa2, a)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 15, 16, 17])
def test_small_indexes(mods, dtype, N):
    for C in ALL_C:
        x, c = ac.random_corpus(24, N, D, C)
        idx = make_index(mods, x, dtype)
        check_call(mods, idx, x, c, dtype)


@pytest.mark.parametrize("dtype,dim", [("f16", 1024), ("f8", 1024), ("f32", 1920)])
def test_wide_rows_choose_the_tile_by_the_lds_budget(mods, dtype, dim):
    N, C = 300, 65
    x, c = ac.random_corpus(25, N, dim, C)
    idx = make_index(mods, x, dtype, dim)
    dl = check_call(mods, idx, x, c, dtype, dim)
    assert dl["radius_pages"] == (2 if dim == 1024 else 5)      # 64 centres per pass fit at 1024 x f16; 16 at 1920 x f32


# ================================================================================================ 2. every winner
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", ALL_C)
def test_every_centre_wins_at_every_position(mods, dtype, C):
    x, c = ac.every_winner_corpus(22, D, C)
    idx = make_index(mods, x, dtype)
    check_call(mods, idx, x, c, dtype)
    got = idx.assign(c, want_dist=False)[0]
    missing = [r for r in range(16 * C) if got[r] != ac.winner_of(r, C)]
    assert not missing, (dtype, C, [(r, r % 16, ac.winner_of(r, C) % 16, ac.winner_of(r, C) // 64) for r in missing[:5]])


# ================================================================================================ 3. ties and near-ties
@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_and_near_ties(mods, dtype):
    N = 1000
    x, c = ac.ties_corpus(23, N, D)
    idx = make_index(mods, x, dtype)
    dl = check_call(mods, idx, x, c, dtype)
    a, d, s = ac.expected_of(x, c, dtype)[1:]
    assert s[ac.DUP] == 0 and s[ac.DUP_OF] > 0
    # every row whose winner is the duplicated centre has two equal best scores: borderline at least those
    assert dl["swept_rows"] >= int(s[ac.DUP_OF]) * ac.TIE_C, dl


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicated_centres_make_every_row_borderline(mods, dtype):
    N, K = 1000, 9
    x, c = ac.duplicate_corpus(26, N, D, K)
    idx = make_index(mods, x, dtype)
    exp = ac.expected_of(x, c, dtype)[1:]
    before = idx.guard_stats()
    got = idx.assign(c)
    dl = delta(idx, before)
    assert ac.mismatch(got, exp) is None
    assert not exp[2][K:].any() and exp[2][1] == 0
    assert dl["swept_rows"] == (N - 5) * (2 * K - 2), dl       # (rows with a direction) x (live centres)
    assert dl["radius_pages"] == 1 and dl["radius_queries"] == 2 * K


# ================================================================================================ 5. degenerate calls
@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_calls(mods, dtype):
    N = 500
    x, c = ac.random_corpus(27, N, D, 17)
    idx = make_index(mods, x, dtype)
    # no centre has a direction
    dead = np.zeros((3, D), np.float32)
    dead[1, 4] = np.nan
    dead[2, 0] = np.inf
    a, d, s = idx.assign(dead)
    assert (a == -1).all() and np.isinf(d).all() and (d > 0).all() and not s.any()
    # C = 0, C = 1025, a short buffer: MMISS_ERR_ARG, outputs untouched
    oa, od, os_ = np.full(N, -77, np.int32), np.full(N, -5.0, np.float32), np.full(1025, -3, np.int64)
    big = np.zeros((1025, D), np.float32)
    for status in (raw_assign(mods, idx, big[:0], oa, od, N, os_), raw_assign(mods, idx, big, oa, od, N, os_),
                   raw_assign(mods, idx, c, oa, od, N - 1, os_)):
        assert status == ERR_ARG
        assert (oa == -77).all() and (od == -5.0).all() and (os_ == -3).all()
    sums = np.full((3, D), -9, np.int64)
    lib = mods[3]
    for n, C in ((N - 1, 3), (N, 0), (N, 1025)):
        assert idx._lib.mmiss_index_cluster_sums(idx._h, lib.ptr(np.zeros(N, np.int32)), n, C, lib.ptr(sums), None) == ERR_ARG
        assert (sums == -9).all()
    # an open _begin query: an error, nothing written; afterwards the call works
    pending = idx.query_begin(c[:2], 3)
    assert raw_assign(mods, idx, c, oa, od, N, os_) == ERR_STATE
    assert idx._lib.mmiss_index_cluster_sums(idx._h, lib.ptr(np.zeros(N, np.int32)), N, 3, lib.ptr(sums), None) == ERR_STATE
    assert (oa == -77).all() and (od == -5.0).all() and (os_ == -3).all() and (sums == -9).all()
    pending.result()
    assert ac.mismatch(idx.assign(c), ac.expected_of(x, c, dtype)[1:]) is None
    # an empty index: zeros in the sizes and nothing else
    empty = mods[0](D, dtype)
    os_ = np.full(18, -3, np.int64)
    assert raw_assign(mods, empty, c, oa, od, N, os_) == 0
    assert (oa == -77).all() and (od == -5.0).all() and not os_[:17].any() and os_[17] == -3
    a, d, s = empty.assign(c)
    assert a.shape == (0,) and d.shape == (0,) and s.tolist() == [0] * 17
    su, sz = empty.cluster_sums(np.zeros(0, np.int32), 4)
    assert not su.any() and su.shape == (4, D) and not sz.any()


# ================================================================================================ 6. cluster sums
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,C", [(4999, 130), (4999, 16), (17, 1), (4999, 1), (17, 130)])
def test_cluster_sums_equal_the_definition(mods, dtype, N, C):
    import torch

    x, _ = ac.random_corpus(21 if N == 4999 else 24, N, D, 130)
    idx = make_index(mods, x, dtype)
    rng = np.random.Generator(np.random.Philox(N + C))
    used = np.arange(C)[::3] if C > 3 else np.arange(C)              # the other clusters stay empty
    a = used[rng.integers(0, used.size, N)].astype(np.int32)
    a[rng.random(N) < 0.1] = -1                                       # skipped entries
    if N > 40:
        a[ac.nodir_rows(N)] = -1                                      # rows without a direction are never assigned
        a[100] = C                                                    # ... and an entry behind the clusters is skipped too
    exp = ac.expected_sums(ac.represented(ac.stored_of(x, dtype)), a, C)
    assert np.array_equal(ac.represented(ac.stored_of(x, dtype))[a >= 0], idx.get(labels_of(N)[a >= 0]))   # x IS what get() returns
    got = idx.cluster_sums(a, C)
    assert ac.sums_mismatch(got, exp) is None, (dtype, N, C, ac.sums_mismatch(got, exp))
    again = idx.cluster_sums(a, C)                                    # called twice: the same bits
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    ts, tn = idx.cluster_sums(torch.from_numpy(a).cuda(), C)          # the assignment on the device
    assert ts.is_cuda and tn.is_cuda
    assert ac.sums_mismatch((ts.cpu().numpy(), tn.cpu().numpy()), exp) is None
    if C > 3:
        assert not exp[1][1::3].any() and not got[0][1::3].any()      # empty clusters: zero sums


# ================================================================================================ 7. k-means
@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_kmeans_equals_the_restatement(mods, dtype):
    k = ac.KMEANS
    x = ac.kmeans_corpus()
    idx = make_index(mods, x, dtype)
    exp = ac.expected_kmeans(ac.stored_of(x, dtype), k["C"], k["iters"])
    out = idx.kmeans(k["C"], iters=k["iters"])
    assert out["iterations"] == exp["iterations"] >= 2
    assert np.array_equal(out["centres"].view(np.uint32), exp["centres"].view(np.uint32))
    assert ac.mismatch((out["assign"], out["dist"], out["sizes"]), (exp["assign"], exp["dist"], exp["sizes"])) is None
    # init by labels
    pos = np.arange(k["C"]) * 7 + 1
    exp = ac.expected_kmeans(ac.stored_of(x, dtype), k["C"], 2, init_pos=pos)
    out = idx.kmeans(k["C"], iters=2, init=labels_of(k["N"])[pos])
    assert np.array_equal(out["centres"].view(np.uint32), exp["centres"].view(np.uint32))
    assert ac.mismatch((out["assign"], out["dist"], out["sizes"]), (exp["assign"], exp["dist"], exp["sizes"])) is None


# ================================================================================================ 8. hostile state
@pytest.mark.parametrize("dtype", DTYPES)
def test_stale_state_of_earlier_calls(mods, dtype):
    N = 4999
    x, c = ac.random_corpus(21, N, D, 130)
    idx = make_index(mods, x, dtype)
    check_call(mods, idx, x, c, dtype)                                 # fills the state array and the borderline list for 4999 rows
    xd, cd = ac.duplicate_corpus(26, 1000, D, 9)                       # (its centres only: every row borderline, a long stale list)
    idx.assign(cd)
    # remove rows: the state and the list of the previous calls are stale and larger
    gone = np.arange(1, N, 3)
    assert idx.remove(labels_of(N)[gone]) == gone.size
    keep = np.setdiff1d(np.arange(N), gone)
    st = ac.stored_of(x, dtype)[keep]
    x17, c17 = ac.random_corpus(21, N, D, 17)
    for cc in (c17, c):
        assert ac.mismatch(idx.assign(cc), ac.expected_assign(cc, st)) is None, (dtype, cc.shape)
    # after a membership call and after a query: they share the query scratch (qs, eps_q) with assign
    q = c[40:45]
    idx.membership(q, 0.9)
    assert ac.mismatch(idx.assign(c17), ac.expected_assign(c17, st)) is None
    idx.query(c[:100], 10)
    assert ac.mismatch(idx.assign(c17), ac.expected_assign(c17, st)) is None
    a = ac.expected_assign(c17, st)[0]
    assert ac.sums_mismatch(idx.cluster_sums(a, 17), ac.expected_sums(ac.represented(st), a, 17)) is None

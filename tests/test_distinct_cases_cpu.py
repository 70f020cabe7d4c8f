"""Every planted case of tests/distinct_cases.py held to its claim on the oracle alone, so a failure of test_index_distinct_gpu.py
cannot be the fixture's fault: the bursts, the chain (greedy, not clustering), the boundary at the oracle's own bits, the direction
of sep on f16 / fp8 rows, prefix stability over pools, an exhausted pool, the extremes of min_sep, rows and a query without a
direction, masks."""
import numpy as np
import pytest

import distinct_cases as dc
import partition_cases as pc
from oracle import retrieval_oracle as ro

DTYPES = ["f32", "f16", "f8"]


def _setup(dtype):
    return dc.corpus(), dc.stored(dtype)


def _one(c, st, qi, k, pool, min_sep, **kw):
    return dc.expected_distinct(c.queries[qi:qi + 1], k, pool, min_sep, st, c.labels, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bursts_keep_one_of_each(dtype):
    c, st = _setup(dtype)
    L = ro.query(c.queries[dc.Q_BURSTS:dc.Q_BURSTS + 1], st, c.labels, 31)
    top = L[0][0]
    for j, g in enumerate(c.bursts):                                   # the top 30 are the three bursts, in order
        assert set(top[10 * j:10 * j + 10].tolist()) == set(c.labels[g].tolist())
    assert top[30] not in np.concatenate([c.labels[g] for g in c.bursts])
    lab, dist, cnt, dups, listed = _one(c, st, dc.Q_BURSTS, 3, 30, dc.MIN_SEP)
    assert cnt[0] == 3 and listed[0] == 30 and dups[0].tolist() == [9, 9, 9]
    assert lab[0].tolist() == [top[0], top[10], top[20]]
    assert np.array_equal(dist[0].view(np.uint32), L[1][0, [0, 10, 20]].view(np.uint32))
    # the planted separation: inside a burst <= 0.008, everything else the walk compares >= 0.02
    rows = np.searchsorted(c.labels, top[:30])
    for j in range(3):
        inside = dc.sep(st, rows[10 * j], rows[10 * j + 1:10 * j + 10])
        assert inside.max() <= 0.008, inside.max()
        across = dc.sep(st, rows[10 * j], np.delete(rows, np.s_[10 * j:10 * j + 10]))
        assert across.min() >= 0.02, across.min()


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_is_greedy_not_clustering(dtype):
    c, st = _setup(dtype)
    a, b, cc = c.chain
    ab, ac = dc.sep(st, a, [b, cc])
    bc = dc.sep(st, b, [cc])[0]
    assert ab <= dc.MIN_SEP and bc <= dc.MIN_SEP and ac > dc.MIN_SEP, (ab, bc, ac)
    top = ro.query(c.queries[dc.Q_CHAIN:dc.Q_CHAIN + 1], st, c.labels, 4)[0][0]
    assert top[:3].tolist() == c.labels[[a, b, cc]].tolist()
    lab, _, cnt, dups, _ = _one(c, st, dc.Q_CHAIN, 3, 64, dc.MIN_SEP)
    assert cnt[0] == 3 and lab[0].tolist() == [c.labels[a], c.labels[cc], top[3]]          # a and c kept, b owned by a
    assert dups[0].tolist() == [1, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_at_the_oracles_own_bits(dtype):
    c, st = _setup(dtype)
    a, b, cc = c.chain
    at = np.float32(dc.sep(st, a, [b])[0])
    below = np.nextafter(at, np.float32(-np.inf))
    lab, _, _, dups, _ = _one(c, st, dc.Q_CHAIN, 2, 64, at)
    assert lab[0, 1] != c.labels[b] and dups[0, 0] >= 1                                    # at the value: suppressed
    lab, _, _, dups, _ = _one(c, st, dc.Q_CHAIN, 2, 64, below)
    assert lab[0].tolist() == c.labels[[a, b]].tolist() and dups[0, 0] == 0                # one float below: kept


@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_direction_the_kept_row_is_the_query(dtype):
    c, st = _setup(dtype)
    differing = 0
    for qi, (x, y) in zip(dc.Q_PAIRS, c.pairs):
        top = ro.query(c.queries[qi:qi + 1], st, c.labels, 2)[0][0]
        assert set(top.tolist()) == set(c.labels[[x, y]].tolist())
        s, i = (x, y) if top[0] == c.labels[x] else (y, x)                                 # list order
        fwd, rev = np.float32(dc.sep(st, s, [i])[0]), np.float32(dc.sep(st, i, [s])[0])
        if fwd.view(np.uint32) == rev.view(np.uint32):
            continue
        differing += 1
        between = min(fwd, rev)                                                            # min_sep admits exactly the smaller of the two
        right = _one(c, st, qi, 2, 64, between)
        wrong = _one(c, st, qi, 2, 64, between, transposed=True)
        assert dc.mismatch(right, wrong) is not None
        assert (right[3][0, 0] == 1) == (fwd <= between) and (wrong[3][0, 0] == 1) == (rev <= between)
    assert differing >= 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_stability_over_pools(dtype):
    c, st = _setup(dtype)
    k = 10
    qs = c.queries[[dc.Q_BURSTS, dc.Q_CHAIN, dc.Q_BIG]]
    res = [dc.expected_distinct(qs, k, pool, dc.MIN_SEP, st, c.labels) for pool in (k, 64, 300, dc.MAX_POOL)]
    for small, large in zip(res, res[1:]):
        for q in range(qs.shape[0]):
            n = small[2][q]
            assert n <= large[2][q]
            assert np.array_equal(small[0][q, :n], large[0][q, :n])
            assert np.array_equal(small[1][q, :n].view(np.uint32), large[1][q, :n].view(np.uint32))
            if n == k:                                                                     # complete: independent of the pool
                assert np.array_equal(small[0][q], res[-1][0][q])
            assert (small[3][q, :n] <= large[3][q, :n]).all()                              # only dups depend on the pool


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_exhausted(dtype):
    c, st = _setup(dtype)
    lab, _, cnt, dups, listed = _one(c, st, dc.Q_BIG, 3, 64, dc.MIN_SEP)
    assert cnt[0] == 1 < 3 and listed[0] == 64 and dups[0].tolist() == [63, 0, 0] and lab[0, 1] == -1
    lab, _, cnt, dups, listed = _one(c, st, dc.Q_BIG, 3, 300, dc.MIN_SEP)
    assert cnt[0] == 3 and listed[0] == 300 and dups[0, 0] == c.big.size - 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_extremes_of_min_sep(dtype):
    c, st = _setup(dtype)
    qs = c.queries[:7]
    lab, dist, cnt, dups, listed = dc.expected_distinct(qs, 10, 64, -1.0, st, c.labels)
    ol, od, oc = ro.query(qs, st, c.labels, 10)
    assert pc.mismatch((lab, dist, cnt), (ol, od, oc)) is None and not dups.any() and (listed == 64).all()
    lab, dist, cnt, dups, listed = dc.expected_distinct(qs, 10, 64, 4.0, st, c.labels)
    assert (cnt == 1).all() and (dups[:, 0] == 63).all() and not dups[:, 1:].any()
    assert np.array_equal(lab[:, 0], ol[:, 0]) and (lab[:, 1:] == -1).all() and np.isinf(dist[:, 1:]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_direction(dtype):
    c, st = _setup(dtype)
    out = dc.expected_distinct(c.queries, 5, dc.MAX_POOL, dc.MIN_SEP, st, c.labels)
    assert out[2][dc.Q_NODIR] == 0 and out[4][dc.Q_NODIR] == 0 and (out[0][dc.Q_NODIR] == -1).all()
    lab, _, cnt, _, listed = dc.expected_distinct(c.queries[:1], 1, dc.MAX_POOL, 4.0, st, c.labels)
    assert listed[0] == dc.MAX_POOL
    # a list as long as the index: the rows without a direction are never on it
    sub = np.sort(np.concatenate([np.arange(50), np.asarray(c.nodir)]))
    out = dc.expected_distinct(c.queries[:1], 60, 60, -1.0, st[sub], c.labels[sub])
    assert out[4][0] == sub.size - 2 and not np.isin(c.labels[list(c.nodir)], out[0][0]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_masks(dtype):
    c, st = _setup(dtype)
    qs = c.queries[:7]
    req, exc = pc.query_masks(7)
    out = dc.expected_distinct(qs, 5, 64, dc.MIN_SEP, st, c.labels, c.tags, req, exc)
    tag_of = dict(zip(c.labels.tolist(), c.tags.tolist()))
    for q in range(7):
        for l in out[0][q, :out[2][q]]:
            assert (tag_of[int(l)] & int(req[q])) == int(req[q]) and (tag_of[int(l)] & int(exc[q])) == 0
    # the bursts under a mask: the survivors of each burst still collapse into one
    def admitted(rows):
        return int((((c.tags[rows] & req[0]) == req[0]) & ((c.tags[rows] & exc[0]) == 0)).sum())

    sizes = [admitted(g) for g in c.bursts if admitted(g)]
    assert sizes and out[3][dc.Q_BURSTS, :len(sizes)].tolist() == [n - 1 for n in sizes]
    assert dc.mismatch(out, dc.expected_distinct(qs, 5, 64, dc.MIN_SEP, st, c.labels)) is not None

"""What the grouped-search tests share (test_grouped_cases_cpu.py, test_grouped_layers_cpu.py, test_index_grouped_gpu.py): the numpy
restatement of mmiss_index_query_grouped on the retrieval oracle alone, the planted corpora (cached: the tests share the arrays and
leave them unchanged) and the comparator. Not a test module.

The restatement, for a query q (ro = oracle.retrieval_oracle):
  sub     = the rows the masks of q admit
  R(q)    = ro.query(q, stored[sub], labels[sub], k = |sub|): the COMPLETE ranking, rows without a direction fall away here
  group   = groups[row], a row with -1 a group of its own
  result  = the first k entries of R(q) that are the first of their group, in R(q)'s order; count = how many there are.
`limit` cuts R(q) to its first `limit` entries before the walk: what a walk over a pool of that size would answer on its own."""
import numpy as np

import partition_cases as pc
from assign_cases import nodir_rows
from oracle import retrieval_oracle as ro
from partition_cases import expected_flat, labels_of, query_masks, stored_of  # noqa: F401  (shared with the tests)
from radius_cases import represented  # noqa: F401

_cache = {}
D = 128
MAX_GROUPS = 1 << 24       # MMISS_MAX_GROUPS
MAX_POOL = 2040


def default_pool(k):
    return min(MAX_POOL, max(8 * k, 64))


def _masks(m, Q):
    if m is None:
        return np.zeros(Q, np.uint64)
    return np.broadcast_to(np.asarray(m).astype(np.uint64), (Q,))


def ranking(query, stored, labels, tags=None, require=0, exclude=0):
    """R(q) -> (rows int64 [n], distances float32 [n]) of one query"""
    N = stored.shape[0]
    labels = np.asarray(labels, np.int64)
    tags = np.zeros(N, np.uint64) if tags is None else np.asarray(tags).astype(np.uint64)
    req, exc = np.uint64(require), np.uint64(exclude)
    sub = np.nonzero(((tags & req) == req) & ((tags & exc) == 0))[0]
    if sub.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    with np.errstate(all="ignore"):
        rl, rd, rc = ro.query(np.asarray(query, np.float32).reshape(1, -1), stored[sub], labels[sub], int(sub.size))
    n = int(rc[0])
    return np.searchsorted(labels, rl[0, :n]), rd[0, :n]


def rankings(queries, stored, labels, tags=None, require=None, exclude=None):
    """[R(q) for every query]: computed once, they serve expected_grouped and expected_route of every k and pool (ranks=)"""
    queries = np.asarray(queries, np.float32).reshape(-1, stored.shape[1])
    req, exc = _masks(require, queries.shape[0]), _masks(exclude, queries.shape[0])
    return [ranking(queries[q], stored, labels, tags, req[q], exc[q]) for q in range(queries.shape[0])]


def heads_of(rows, groups):
    """positions in a ranking (its rows given) that are the first of their group, ascending"""
    g = np.asarray(groups, np.int64)[rows]
    key = np.where(g >= 0, g, MAX_GROUPS + rows)
    _, first = np.unique(key, return_index=True)
    return np.sort(first)


def expected_grouped(queries, k, stored, labels, groups, tags=None, require=None, exclude=None, limit=None, ranks=None):
    """-> (labels int64 [Q, k], distances float32 [Q, k], groups int32 [Q, k], counts int32 [Q]); ranks: rankings() of these queries
    and masks, if the caller has them"""
    queries = np.asarray(queries, np.float32).reshape(-1, stored.shape[1])
    Q = queries.shape[0]
    labels = np.asarray(labels, np.int64)
    groups = np.asarray(groups, np.int32)
    ranks = rankings(queries, stored, labels, tags, require, exclude) if ranks is None else ranks
    out = (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.full((Q, k), -1, np.int32), np.zeros(Q, np.int32))
    for q in range(Q):
        rows, dist = ranks[q]
        if limit is not None:
            rows, dist = rows[:limit], dist[:limit]
        h = heads_of(rows, groups)[:k]
        n = h.size
        out[0][q, :n], out[1][q, :n], out[2][q, :n], out[3][q] = labels[rows[h]], dist[h], groups[rows[h]], n
    return out


def expected_route(queries, k, pool, stored, labels, groups, tags=None, require=None, exclude=None, ranks=None):
    """int32 [Q]: 0 where the walk over the first `pool` of R(q) is complete (k heads, or the ranking ends before the pool), else 1"""
    queries = np.asarray(queries, np.float32).reshape(-1, stored.shape[1])
    Q = queries.shape[0]
    ranks = rankings(queries, stored, labels, tags, require, exclude) if ranks is None else ranks
    out = np.zeros(Q, np.int32)
    for q in range(Q):
        rows, _ = ranks[q]
        out[q] = 0 if (rows.size < pool or heads_of(rows[:pool], groups).size >= k) else 1
    return out


def mismatch(got, exp):
    """None when (labels, distances, groups, counts) equals the expected tuple in every element (distances by their bits), else a
    message that names the first difference"""
    names = ("labels", "dist", "group", "count")
    dtypes = (np.int64, np.float32, np.int32, np.int32)
    for name, dt, g, e in zip(names, dtypes, got, exp):
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape or g.dtype != dt:
            return f"{name}: shape / dtype {g.shape} {g.dtype}, expected {e.shape} {np.dtype(dt)}"
        bad = np.argwhere(g.view(np.uint32) != e.view(np.uint32)) if dt == np.float32 else np.argwhere(g != e)
        if bad.size:
            i = tuple(bad[0])
            return f"{name}: {bad.shape[0]} entries differ, first at {i}: got {g[i]!r}, expected {e[i]!r}"
    return None


# ------------------------------------------------------------------------------------------------ corpora
def corpus(seed, N, dim=D, Q=300, n_groups=50):
    """partition_cases.clustered with every cell valid (rows without a direction at assign_cases.nodir_rows(N), query 2 without a
    direction, tags on bits 0 .. 2) and `groups` int32 [N]: random ids below n_groups, every fourth row ungrouped (ungrouped rows
    between grouped ones), and group n_groups holding exactly the first two rows without a direction: a group that never has a head.
    -> dict(x, queries, tags, groups, n_groups)"""
    key = ("corpus", seed, N, dim, Q, n_groups)
    if key not in _cache:
        p = pc.clustered(seed, N, dim, 7, Q, complete=True)
        rng = np.random.Generator(np.random.Philox(3000 + seed))
        g = rng.integers(0, n_groups, N).astype(np.int32)
        g[rng.permutation(N)[:N // 4]] = -1
        nd = nodir_rows(N)
        g[nd[:2]] = n_groups
        _cache[key] = pc._freeze(dict(x=p["x"], queries=p["queries"], tags=p["tags"], groups=g, n_groups=n_groups))
    return _cache[key]


CROWD_SIZE, CROWD_OTHERS, CROWD_K = 40, 12, 5


def crowd(dim=D, size=CROWD_SIZE):
    """One group of `size` rows nearer to the query than everything else, in front of CROWD_OTHERS other groups of five rows each
    and ten ungrouped rows; the rows shuffled over the index. A walk over fewer than size + CROWD_K - 1 entries finds fewer than
    CROWD_K groups. -> dict(x, queries [1, dim], groups, big: the big group's id)"""
    key = ("crowd", dim, size)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(91))
        q = rng.standard_normal(dim, dtype=np.float32)
        near = q + rng.standard_normal((size, dim), dtype=np.float32) * np.float32(0.05)
        far = rng.standard_normal((CROWD_OTHERS * 5 + 10, dim), dtype=np.float32)
        x = np.concatenate([near, far]).astype(np.float32)
        g = np.concatenate([np.full(size, 3), np.repeat(np.arange(CROWD_OTHERS) + 4, 5), np.full(10, -1)]).astype(np.int32)
        perm = rng.permutation(x.shape[0])
        _cache[key] = pc._freeze(dict(x=x[perm], queries=q[None].copy(), groups=g[perm], big=3))
    return _cache[key]


def ends(N=700, dim=D):
    """Heads at the last and the first row of the index: random rows; query 0 is a bit copy of row N - 1, query 1 of row 0. Group 0
    holds row N - 1 and rows 10 .. 19, group 1 holds row 0 and rows 30 .. 39, rows 100 .. 399 lie in groups 2 .. 31, the rest is
    ungrouped. -> dict(x, queries [2, dim], groups, planted: (N - 1, 0))"""
    key = ("ends", N, dim)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(92))
        x = rng.standard_normal((N, dim), dtype=np.float32)
        g = np.full(N, -1, np.int32)
        g[100:400] = 2 + np.arange(300) % 30
        g[10:20] = 0; g[N - 1] = 0
        g[30:40] = 1; g[0] = 1
        _cache[key] = pc._freeze(dict(x=x, queries=x[[N - 1, 0]].copy(), groups=g, planted=(N - 1, 0)))
    return _cache[key]


def ties(dim=D):
    """Heads that tie in distance, so the label decides: 60 random rows; rows 7, 21 and 40 are bit copies of one another and lie in
    group 5, in group 2 and ungrouped; query 0 is a noisy copy of them. Rows 8 (group 5) and 22 (group 2) are bit copies of each
    other and a little farther: never heads. -> dict(x, queries [1, dim], groups, tied: (7, 21, 40))"""
    key = ("ties", dim)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(93))
        x = rng.standard_normal((60, dim), dtype=np.float32)
        x[21] = x[7]; x[40] = x[7]
        q = (x[7] + rng.standard_normal(dim, dtype=np.float32) * np.float32(0.05)).astype(np.float32)
        x[8] = x[7] + rng.standard_normal(dim, dtype=np.float32) * np.float32(0.2)
        x[22] = x[8]
        g = (np.arange(60) % 3 + 10).astype(np.int32)
        g[[7, 8]] = 5; g[[21, 22]] = 2; g[40] = -1
        _cache[key] = pc._freeze(dict(x=x, queries=q[None].copy(), groups=g, tied=(7, 21, 40)))
    return _cache[key]


def masked_head(dim=D):
    """A group whose only admitted row is not its nearest: 80 random rows in groups r % 8; group 3's rows 3 and 11 are noisy copies
    of the query, row 3 the nearer one with tag 0, row 11 with tag 1, every other row of group 3 tag 0, every row of the other
    groups tag 1. Under require = 1 the head of group 3 is row 11. -> dict(x, queries [1, dim], groups, tags, near: 3, admitted: 11)"""
    key = ("masked", dim)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(94))
        x = rng.standard_normal((80, dim), dtype=np.float32)
        q = rng.standard_normal(dim, dtype=np.float32)
        x[3] = q + rng.standard_normal(dim, dtype=np.float32) * np.float32(0.02)
        x[11] = q + rng.standard_normal(dim, dtype=np.float32) * np.float32(0.1)
        g = (np.arange(80) % 8).astype(np.int32)
        tags = np.where(g == 3, 0, 1).astype(np.uint64)
        tags[11] = 1
        _cache[key] = pc._freeze(dict(x=x, queries=q[None].copy(), groups=g, tags=tags, near=3, admitted=11))
    return _cache[key]


def extreme_ids(N=300, dim=D):
    """group ids at both ends of the range: rows r % 3 == 0 in group 0, r % 3 == 1 in group MAX_GROUPS - 1, the rest ungrouped;
    queries: noisy copies of rows 50, 51 and 52 -> dict(x, queries [3, dim], groups)"""
    key = ("extreme", N, dim)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(95))
        x = rng.standard_normal((N, dim), dtype=np.float32)
        g = np.full(N, -1, np.int32)
        g[0::3] = 0
        g[1::3] = MAX_GROUPS - 1
        q = (x[50:53] + rng.standard_normal((3, dim), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
        _cache[key] = pc._freeze(dict(x=x, queries=q, groups=g))
    return _cache[key]


def max_dim(dtype):
    """the largest dim mmiss_index_create admits"""
    return 1920 if dtype == "f32" else 3968

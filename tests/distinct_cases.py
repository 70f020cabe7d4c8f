"""What the distinct-results tests share (test_distinct_cases_cpu.py, test_distinct_layers_cpu.py, test_index_distinct_gpu.py): the
restatement of mmiss_index_query_distinct on the retrieval oracle alone, the planted corpora (cached: the tests share the arrays and
leave them unchanged) and the comparator. Not a test module.

The restatement, for a query q (ro = oracle.retrieval_oracle):
  L        = partition_cases.expected_flat(q, pool, ...) or, with a partition, partition_cases.expected_probed(q, pool, nprobe, ...):
             labels and distance bits in (distance, label) order, m = its count
  sep(s,i) = ro.distances(radius_cases.represented(stored)[row of L[s]][None], stored[[row of L[i]]])[0, 0]
  the walk = positions in order; i is owned by the first (smallest) earlier KEPT s with sep(s, i) <= min_sep (float32 compare),
             else kept while fewer than k are kept; the k-th kept one still owns over all of L."""
import functools
from typing import NamedTuple

import numpy as np

import partition_cases as pc
import radius_cases as rc
from oracle import retrieval_oracle as ro

MAX_POOL = 2040
MIN_SEP = np.float32(0.01)     # between a planted near copy's <= 0.008 and every other pair's >= 0.02 (test_distinct_cases_cpu.py)
NQ = 8                          # queries of a corpus: 0 bursts, 1 chain, 2 .. 5 direction pairs, 6 the big group, 7 no direction
Q_BURSTS, Q_CHAIN, Q_PAIRS, Q_BIG, Q_NODIR = 0, 1, (2, 3, 4, 5), 6, 7
BURSTS, BURST = 3, 10
CHAIN_SEP = 0.006               # a-b and b-c of the chain; a-c is about four times that


def labels_of(n):
    return np.arange(n, dtype=np.int64) * 7 + 2


class Corpus(NamedTuple):
    rows: np.ndarray        # float32 [N, D]
    labels: np.ndarray      # int64 [N]
    tags: np.ndarray        # uint64 [N], values 0 .. 7
    queries: np.ndarray     # float32 [NQ, D]
    bursts: tuple           # three arrays of ten rows
    chain: tuple            # rows (a, b, c)
    pairs: tuple            # four (x, y) row pairs, one per query of Q_PAIRS
    big: np.ndarray         # the rows of the big group
    nodir: tuple            # rows without a direction


@functools.lru_cache(maxsize=None)
def corpus(N=3000, dim=128, seed=5, big=100) -> Corpus:
    """A seeded base of random directions plus planted near copies at chosen cosines (the manner of radius_cases.near_dup_corpus):
    query 0: its 30 nearest rows are three bursts of ten (pairwise distance about 0.001 inside a burst, > 0.2 across);
    query 1: a chain a, b, c in one plane with the query, a nearest: a-b and b-c at CHAIN_SEP, a-c at about 4 CHAIN_SEP;
    queries 2 .. 5: one pair each, y = x + noise of 0.1 sigma: about 0.005 apart;
    query 6: `big` near copies of one centre (pairwise about 0.0001) are its nearest rows;
    query 7 and two rows have no direction."""
    rng = np.random.Generator(np.random.Philox(seed))
    rows = rng.standard_normal((N, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    qs = rng.standard_normal((NQ, dim))
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    slots = rng.permutation(N)
    at = 0

    def take(n):
        nonlocal at
        g = np.sort(slots[at:at + n])
        at += n
        return g

    def near(v, cos, n):
        u = rng.standard_normal((n, dim))
        u -= (u @ v)[:, None] * v[None, :]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        c = np.asarray(cos, np.float64).reshape(-1, 1)
        return c * v[None, :] + np.sqrt(1.0 - c * c) * u

    bursts = []
    for c in (0.9, 0.85, 0.8)[:BURSTS]:
        centre = near(qs[Q_BURSTS], c, 1)[0]
        g = take(BURST)
        rows[g] = near(centre, 0.9995, BURST)
        bursts.append(g)
    u = near(qs[Q_CHAIN], 0.0, 1)[0]                       # a unit vector orthogonal to the query: the chain's plane
    theta, phi = np.arccos(1.0 - CHAIN_SEP), 0.3
    chain = take(3)
    chain = chain[rng.permutation(3)]                      # (row order is not list order)
    for j, r in enumerate(chain):
        rows[r] = np.cos(phi + j * theta) * qs[Q_CHAIN] + np.sin(phi + j * theta) * u
    pairs = []
    for qi in Q_PAIRS:
        g = take(2)
        x = near(qs[qi], 0.95, 1)[0]
        y = x + rng.standard_normal(dim) * (0.1 / np.sqrt(dim))
        rows[g[0]], rows[g[1]] = x, y / np.linalg.norm(y)
        pairs.append((int(g[0]), int(g[1])))
    bg = take(big)
    rows[bg] = near(near(qs[Q_BIG], 0.9, 1)[0], 0.99995, big)
    nodir = take(2)
    rows = (2.0 * rows).astype(np.float32)
    rows[nodir[0]] = 0.0
    rows[nodir[1], 3] = np.nan
    qs = (3.0 * qs).astype(np.float32)
    qs[Q_NODIR] = 0.0
    tags = rng.integers(0, 8, N).astype(np.uint64)
    for a in (rows, qs, tags):
        a.setflags(write=False)
    return Corpus(rows, labels_of(N), tags, qs, tuple(bursts), tuple(int(r) for r in chain), tuple(pairs), bg, tuple(int(r) for r in nodir))


@functools.lru_cache(maxsize=None)
def stored(dtype, N=3000, dim=128, seed=5, big=100):
    with np.errstate(all="ignore"):
        return ro.normalize_rows(corpus(N, dim, seed, big).rows, dtype)


_rep = {}


def represented_of(st):
    """radius_cases.represented(st), once per stored array"""
    if id(st) not in _rep:
        _rep[id(st)] = (st, rc.represented(st))
    return _rep[id(st)][1]


def sep(st, s_rows, i_rows, transposed=False):
    """float32 [len(i_rows)]: sep(s, i) for ONE kept row s against the rows i; transposed: sep(i, s) instead (the wrong direction,
    for the test that tells the two apart)"""
    rep = represented_of(st)
    i_rows = np.asarray(i_rows)
    with np.errstate(all="ignore"):
        if not transposed:
            return ro.distances(rep[s_rows][None], st[i_rows])[0]
        return ro.distances(rep[i_rows], st[[s_rows]])[:, 0]


def ranked_list(queries, pool, st, labels, tags=None, require=None, exclude=None, partition=None):
    """L of every query -> (labels [Q, pool], distances [Q, pool], counts [Q]); partition: dict(nprobe, centres, cells, B) or None"""
    if partition is None:
        return pc.expected_flat(queries, pool, st, labels, tags, require, exclude)
    return pc.expected_probed(queries, pool, partition["nprobe"], partition["centres"], partition["cells"], partition["B"], st, labels, tags,
                              require, exclude)[:3]


def walk(L_lab, L_dist, m, k, min_sep, st, labels, transposed=False):
    """the greedy walk over one list -> (kept positions, owner rank per position (-1: none))"""
    rows = np.searchsorted(labels, L_lab[:m])
    assert (labels[rows] == L_lab[:m]).all()
    own = np.full(m, -1, np.int64)
    kept = []
    for i in range(m):
        if own[i] >= 0:
            continue
        if len(kept) == k:
            break
        kept.append(i)
        behind = np.nonzero(own[i + 1:] < 0)[0] + i + 1
        if behind.size:
            with np.errstate(invalid="ignore"):
                hit = sep(st, rows[i], rows[behind], transposed) <= np.float32(min_sep)
            own[behind[hit]] = len(kept) - 1
    return kept, own


def expected_distinct(queries, k, pool, min_sep, st, labels, tags=None, require=None, exclude=None, partition=None, transposed=False):
    """-> (labels int64 [Q, k], distances float32 [Q, k], counts int32 [Q], dups int32 [Q, k], listed int32 [Q])"""
    queries = np.asarray(queries, np.float32).reshape(-1, st.shape[1])
    labels = np.asarray(labels, np.int64)
    Q = queries.shape[0]
    Ll, Ld, Lc = ranked_list(queries, pool, st, labels, tags, require, exclude, partition)
    out_l = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), np.inf, np.float32)
    out_c = np.zeros(Q, np.int32)
    out_u = np.zeros((Q, k), np.int32)
    out_m = np.asarray(Lc, np.int32).copy()
    for q in range(Q):
        m = int(Lc[q])
        kept, own = walk(Ll[q], Ld[q], m, k, min_sep, st, labels, transposed)
        n = len(kept)
        out_l[q, :n], out_d[q, :n], out_c[q] = Ll[q, kept], Ld[q, kept], n
        out_u[q, :n] = np.bincount(own[own >= 0], minlength=n)[:n] if n else 0
    return out_l, out_d, out_c, out_u, out_m


_exp = {}


def expected_cached(key, *a, **kw):
    """expected_distinct once per `key` (the GPU tests share the results and leave them unchanged)"""
    if key not in _exp:
        out = expected_distinct(*a, **kw)
        for v in out:
            v.setflags(write=False)
        _exp[key] = out
    return _exp[key]


# ------------------------------------------------------------------------------------------------ comparator
def mismatch(got, exp):
    """None when (labels, distances, counts, dups, listed) equals the expected tuple in every element (distances by their bits),
    else a message that names the first difference; None entries of `got` (a null output) are not compared"""
    names = ("labels", "dist", "count", "dups", "listed")
    dtypes = (np.int64, np.float32, np.int32, np.int32, np.int32)
    for name, dt, g, e in zip(names, dtypes, got, exp):
        if g is None:
            continue
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape or g.dtype != dt:
            return f"{name}: shape / dtype {g.shape} {g.dtype}, expected {e.shape} {np.dtype(dt)}"
        bad = np.argwhere(g.view(np.uint32) != e.view(np.uint32)) if dt == np.float32 else np.argwhere(g != e)
        if bad.size:
            i = tuple(bad[0])
            return f"{name}: {bad.shape[0]} entries differ, first at {i}: got {g[i]!r}, expected {e[i]!r}"
    return None

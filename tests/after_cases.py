"""What the search-after tests share (test_after_cases_cpu.py, test_after_layers_cpu.py, test_index_after_gpu.py): the numpy
restatement of mmiss_index_query_after on the retrieval oracle alone, the planted corpora (cached: the tests share the arrays and
leave them unchanged) and the page chain. Not a test module.

The restatement, for a query q with the cursor (ad, al) (ro = oracle.retrieval_oracle):
  d       = ro.distances(q, stored)[0]
  A(q)    = the rows r with  np.isin(labels[r], list)  (when there is a list),  the masks of q admitting tags[r],  d[r] not NaN,
            d[r] <= max_dist[q]  (when there is one; a NaN admits nothing),  and
            mono(d[r]) > mono(ad)  or  mono(d[r]) == mono(ad) and labels[r] > al      (ad NaN: nothing; ad = -inf: every row)
            with mono the order-preserving map of the float bits the ranking sorts by (probe_mono)
  result  = ro.query(q, stored[A], labels[A], k);  remaining = |A(q)|."""
import numpy as np

import partition_cases as pc
import subset_cases as sc
from assign_cases import nodir_rows
from oracle import retrieval_oracle as ro
from partition_cases import expected_flat, labels_of, mismatch, query_masks, stored_of  # noqa: F401  (shared with the tests)
from subset_cases import UNKNOWN, max_dim, mixed_list, sized_list  # noqa: F401

_cache = {}
D = 128
BIG_N = sc.BIG_N        # 17 000 rows: three selection levels at k = 1000
DENSE_N = 140005        # the dense scan past its first trips: a share above 64 positions, no multiple of 16
RUN = 50                # byte-identical copies of one row: an equal-distance run longer than a page
NEARER = 6              # rows nearer to query 0 than the run: at k = 7 the first page ends with the run's first copy
START = np.float32(-np.inf)


def mono(d):
    """probe_mono on numpy float32: uint32 increasing with the float, by its bits (-0.0 before +0.0)"""
    b = np.asarray(d, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000))


def _per_query(v, Q, dtype):
    return np.broadcast_to(np.asarray(v, dtype).reshape(-1), (Q,)) if np.asarray(v).size == 1 else np.asarray(v, dtype).reshape(Q)


def all_distances(queries, stored):
    """ro.distances, once per (queries, stored)"""
    queries = np.asarray(queries, np.float32)
    key = ("dist", id(stored), queries.shape, queries.tobytes())
    if key not in _cache:
        if len(_cache) > 400:
            for old in [k for k in _cache if k[0] == "dist"]:
                del _cache[old]
        with np.errstate(all="ignore"):
            _cache[key] = (stored, ro.distances(queries, stored))
    return _cache[key][1]


def admitted(queries, after_dist, after_label, stored, labels, tags=None, require=None, exclude=None, max_dist=None, cand=None,
             label_test="gt"):
    """A(q) as a bool [Q, N]. label_test: "gt" — the contract; "ge" and "none" are the two broken forms the corpora must tell from
    it ("ge": a tie admits the cursor's own row again; "none": a tie admits nothing, the label is not looked at)."""
    queries = np.asarray(queries, np.float32).reshape(-1, stored.shape[1])
    Q, N = queries.shape[0], stored.shape[0]
    labels = np.asarray(labels, np.int64)
    tags = np.zeros(N, np.uint64) if tags is None else np.asarray(tags).astype(np.uint64)
    req, exc = sc._masks(require, Q), sc._masks(exclude, Q)
    ad, al = _per_query(after_dist, Q, np.float32), _per_query(after_label, Q, np.int64)
    md = None if max_dist is None else _per_query(max_dist, Q, np.float32)
    listed = np.ones(N, bool) if cand is None else np.isin(labels, np.asarray(cand, np.int64).reshape(-1))
    d = all_distances(queries, stored)
    out = np.zeros((Q, N), bool)
    for q in range(Q):
        a = listed & ((tags & req[q]) == req[q]) & ((tags & exc[q]) == 0) & ~np.isnan(d[q])
        with np.errstate(invalid="ignore"):
            if md is not None:
                a &= d[q] <= md[q]                         # (a NaN radius: False everywhere)
        if np.isnan(ad[q]):
            a[:] = False
        elif ad[q] != -np.inf:
            m, cm = mono(d[q]), mono(ad[q])
            tie = {"gt": labels > al[q], "ge": labels >= al[q], "none": np.zeros(N, bool)}[label_test]
            a &= (m > cm) | ((m == cm) & tie)
        out[q] = a
    return out


def expected_after(queries, k, after_dist, after_label, stored, labels, tags=None, require=None, exclude=None, max_dist=None, cand=None,
                   label_test="gt"):
    """-> (labels int64 [Q, k], distances float32 [Q, k], counts int32 [Q], remaining int64 [Q])"""
    queries = np.asarray(queries, np.float32).reshape(-1, stored.shape[1])
    A = admitted(queries, after_dist, after_label, stored, labels, tags, require, exclude, max_dist, cand, label_test)
    rows = [np.nonzero(a)[0] for a in A]
    return sc._query_rows(queries, k, lambda q: rows[q], stored, labels) + (A.sum(1).astype(np.int64),)


def full_ranking(query, stored, labels, **kw):
    """ro.query(..., k = |A|) of ONE query from the start of the ranking -> (labels [n], distances [n])"""
    query = np.asarray(query, np.float32).reshape(1, -1)
    n = int(admitted(query, START, 0, stored, labels, **kw).sum())
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    got = expected_after(query, n, START, 0, stored, labels, **kw)
    assert got[2][0] == n == got[3][0]
    return got[0][0], got[1][0]


def chain(page_fn, sizes, limit=100000):
    """Pages of ONE query chained from the start: page_fn(k, after_dist, after_label) -> (labels [1, k], dist [1, k], count [1],
    remaining [1]); sizes: the page sizes, the last one repeated, until a page comes back EMPTY (the page behind the last one is
    asked for too). -> (labels, distances, [(k, count, remaining) per page])"""
    labs, dists, pages = [], [], []
    ad, al = START, np.int64(0)
    i = 0
    while True:
        k = sizes[min(i, len(sizes) - 1)]
        lab, dist, cnt, rem = (np.asarray(v) for v in page_fn(k, ad, al))
        c = int(cnt[0])
        assert (lab[0, c:] == -1).all() and np.isinf(dist[0, c:]).all() and (dist[0, c:] > 0).all()
        pages.append((k, c, int(rem[0])))
        labs.append(lab[0, :c].copy())
        dists.append(dist[0, :c].copy())
        if c == 0:
            break
        ad, al = dist[0, c - 1], lab[0, c - 1]
        i += 1
        assert i < limit
    return np.concatenate(labs), np.concatenate(dists), pages


def pages_consistent(pages, total):
    """consequence 3: remaining falls by count from page to page; the last non-empty page has remaining == count; the page behind
    it has count 0 and remaining 0"""
    left = total
    for k, c, rem in pages:
        if rem != left or c != min(k, left):
            return f"page (k={k}, count={c}, remaining={rem}): {left} rows were left"
        left -= c
    return None if left == 0 and pages[-1][1:] == (0, 0) else f"{left} rows never delivered, last page {pages[-1]}"


def same_ranking(got_labels, got_dist, exp_labels, exp_dist):
    if got_labels.shape != exp_labels.shape:
        return f"{got_labels.shape[0]} entries, expected {exp_labels.shape[0]}"
    bad = np.nonzero((got_labels != exp_labels) | (got_dist.view(np.uint32) != exp_dist.view(np.uint32)))[0]
    if bad.size:
        i = int(bad[0])
        return f"{bad.size} entries differ, first at {i}: got {got_labels[i]} {got_dist[i]!r}, expected {exp_labels[i]} {exp_dist[i]!r}"
    return None


# ------------------------------------------------------------------------------------------------ corpora
def corpus(seed, N, dim=D, Q=300):
    """subset_cases.corpus: rows without a direction at assign_cases.nodir_rows(N), query 2 without a direction, tags on bits 0 .. 2"""
    return sc.corpus(seed, N, dim, Q)


def run_corpus(seed, N, dim=D, Q=300):
    """corpus(seed, N) with a run planted for query 0: RUN byte-identical copies of one row at scattered rows (`run`, ascending),
    and NEARER rows (`near`) closer to query 0 than the copies — the run holds ranks NEARER .. NEARER + RUN - 1 of query 0, all at
    one distance. -> dict(x, queries, tags, run, near)"""
    key = ("run", seed, N, dim, Q)
    if key not in _cache:
        base = corpus(seed, N, dim, Q)
        rng = np.random.Generator(np.random.Philox(7000 + seed))
        x, queries = np.array(base["x"]), np.array(base["queries"])
        free = np.setdiff1d(np.arange(60, N - 60), nodir_rows(N))
        pick = free[rng.permutation(free.size)[:RUN + NEARER]]
        run, near = np.sort(pick[:RUN]), np.sort(pick[RUN:])
        v = rng.standard_normal(dim, dtype=np.float32)
        x[run] = (v + rng.standard_normal(dim, dtype=np.float32) * np.float32(0.3)).astype(np.float32)[None]
        x[near] = v[None] + rng.standard_normal((NEARER, dim), dtype=np.float32) * np.float32(0.05)
        queries[0] = v
        _cache[key] = pc._freeze(dict(x=x, queries=queries, tags=base["tags"], run=run, near=near))
    return _cache[key]

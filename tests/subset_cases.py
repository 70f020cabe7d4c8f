"""What the subset-search tests share (test_subset_cases_cpu.py, test_subset_layers_cpu.py, test_index_subset_gpu.py): the numpy
restatement of mmiss_index_query_subset on the retrieval oracle alone, the planted corpora (cached: the tests share the arrays and
leave them unchanged) and the lists. Not a test module.

The restatement, for a list of labels and a query q (ro = oracle.retrieval_oracle):
  S       = the rows r with np.isin(labels[r], list)      (unknown labels, repeats and the order of the list fall away here)
  sub     = the rows of S the masks of q admit
  result  = ro.query(q, stored[sub], labels[sub], k);  matched = |S| for every query."""
import numpy as np

import partition_cases as pc
from assign_cases import nodir_rows
from oracle import retrieval_oracle as ro
from partition_cases import expected_flat, labels_of, mismatch, query_masks, stored_of  # noqa: F401  (shared with the tests)

_cache = {}
D = 128
BIG_N = 17000          # rows of the largest corpus: enough for three selection levels at k = 1000 (more than 16 384 keys)
UNKNOWN = np.array([-9, 0, 1, 4, 6, 7, 10 ** 12], np.int64)   # labels_of gives 5, 8, 11, ...: none of these is stored


def _masks(m, Q):
    if m is None:
        return np.zeros(Q, np.uint64)
    return np.broadcast_to(np.asarray(m).astype(np.uint64), (Q,))


def subset_rows(cand_labels, labels):
    """S, ascending"""
    return np.nonzero(np.isin(np.asarray(labels, np.int64), np.asarray(cand_labels, np.int64).reshape(-1)))[0]


def _query_rows(queries, k, rows_per_query, stored, labels):
    Q = queries.shape[0]
    out = (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros(Q, np.int32))
    for q in range(Q):
        sub = rows_per_query(q)
        if sub.size:
            with np.errstate(all="ignore"):
                ol, od, oc = ro.query(queries[q:q + 1], stored[sub], np.asarray(labels, np.int64)[sub], k)
            out[0][q], out[1][q], out[2][q] = ol[0], od[0], oc[0]
    return out


def expected_subset(queries, k, cand_labels, stored, labels, tags=None, require=None, exclude=None):
    """-> (labels int64 [Q, k], distances float32 [Q, k], counts int32 [Q], matched int64 [Q])"""
    queries = np.asarray(queries, np.float32).reshape(-1, stored.shape[1])
    Q, N = queries.shape[0], stored.shape[0]
    tags = np.zeros(N, np.uint64) if tags is None else np.asarray(tags).astype(np.uint64)
    req, exc = _masks(require, Q), _masks(exclude, Q)
    S = subset_rows(cand_labels, labels)
    admit = lambda q: S[((tags[S] & req[q]) == req[q]) & ((tags[S] & exc[q]) == 0)]   # noqa: E731
    return _query_rows(queries, k, admit, stored, labels) + (np.full(Q, S.size, np.int64),)


def expected_without_dedupe(queries, k, cand_labels, stored, labels):
    """The restatement WITHOUT the dedupe: a label listed m times stands for m candidates (and may fill m result slots). What a
    front end that forgot to collapse repeats would answer -> (labels, distances, counts)"""
    queries = np.asarray(queries, np.float32).reshape(-1, stored.shape[1])
    labels = np.asarray(labels, np.int64)
    cand = np.asarray(cand_labels, np.int64).reshape(-1)
    pos = np.searchsorted(labels, cand)
    ok = (pos < labels.size) & (labels[np.minimum(pos, labels.size - 1)] == cand)
    rows = np.sort(pos[ok])
    return _query_rows(queries, k, lambda q: rows, stored, labels)


# ------------------------------------------------------------------------------------------------ corpora and lists
def corpus(seed, N, dim=D, Q=300):
    """partition_cases.clustered with every cell valid: x [N, dim] with rows without a direction at assign_cases.nodir_rows(N),
    queries [Q, dim] (query 2 without a direction), tags uint64 [N] on bits 0 .. 2"""
    return pc.clustered(seed, N, dim, 7, Q, complete=True)


def sized_list(N, m, seed=0):
    """the labels of m distinct rows of an index of N rows, shuffled; rows 0 and N - 1 among them (m >= 2)"""
    key = ("sized", N, m, seed)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(1000 + seed))
        if m >= 2:
            rows = np.concatenate([[0, N - 1], 1 + rng.permutation(N - 2)[:m - 2]])
        else:
            rows = rng.permutation(N)[:m]
        out = labels_of(N)[rows[rng.permutation(rows.size)]]
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def mixed_list(N, m, seed=0):
    """stored + unknown + duplicates, shuffled: the labels of m distinct rows, every third of them once more, and UNKNOWN twice"""
    key = ("mixed", N, m, seed)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(2000 + seed))
        base = sized_list(N, m, seed)
        out = np.concatenate([base, base[::3], UNKNOWN, UNKNOWN])
        out = out[rng.permutation(out.size)]
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def hidden(dim=D):
    """partition_cases.hidden_row: the last row is a bit copy of the query — the nearest row of the whole index — and the list
    names every label but its own -> dict(x, queries [1, dim], hidden: its row, cand: the list)"""
    key = ("hidden", dim)
    if key not in _cache:
        p = pc.hidden_row(dim)
        N = p["x"].shape[0]
        cand = np.delete(labels_of(N), p["hidden"])
        cand.setflags(write=False)
        _cache[key] = dict(x=p["x"], queries=p["queries"], hidden=p["hidden"], cand=cand)
    return _cache[key]


CROWD_K = 5


def crowding(dim=D):
    """One label listed more often than k, both in a run and far apart, and its row the nearest of the list: 200 rows, the query a
    noisy copy of row 100; the list holds the labels of rows 90 .. 110, with row 100's label CROWD_K + 2 times in a run at the
    start, once in the middle and once at the end. A front end that keeps repeats fills all k slots with row 100.
    -> dict(x, queries [1, dim], cand, crowd: the repeated row)"""
    key = ("crowding", dim)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(81))
        x = rng.standard_normal((200, dim), dtype=np.float32)
        q = (x[100] + rng.standard_normal(dim, dtype=np.float32) * np.float32(0.05)).astype(np.float32)
        lab = labels_of(200)
        near = lab[90:111]
        cand = np.concatenate([np.repeat(lab[100], CROWD_K + 2), near[:10], lab[100:101], near[10:], lab[100:101]])
        _cache[key] = pc._freeze(dict(x=x, queries=q[None].copy(), cand=cand, crowd=100))
    return _cache[key]


def positions(N, dim=D):
    """Winners at the first and the last row of the index and at the first and the last list position: random rows, queries = bit
    copies of rows 0, N - 1 and of two rows in between; list A starts with row 0's label and ends with row N - 1's, list B the
    other way round; both hold 300 other rows in between. -> dict(x, queries [4, dim], planted: the rows, lists: (A, B))"""
    key = ("positions", N, dim)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(82))
        x = rng.standard_normal((N, dim), dtype=np.float32)
        lab = labels_of(N)
        mid = 1 + rng.permutation(N - 2)[:300]
        planted = np.array([0, N - 1, int(mid[0]), int(mid[-1])])
        a = np.concatenate([lab[:1], lab[mid], lab[N - 1:]])
        b = np.concatenate([lab[N - 1:], lab[mid[::-1]], lab[:1]])
        _cache[key] = pc._freeze(dict(x=x, queries=x[planted].copy(), planted=planted, lists=(a, b)))
    return _cache[key]


def max_dim(dtype):
    """the largest dim mmiss_index_create admits"""
    return 1920 if dtype == "f32" else 3968

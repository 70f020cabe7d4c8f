"""Planted corpora in which EVERY row position hosts a true top-k row of exactly one query, shared by
test_planted_rows_cpu.py (which pins the properties the design rests on: partition, cosine gap, restricted oracle = full oracle)
and test_index_positions_gpu.py (which runs them through every stage-1 path of the index). Not a test module.

corpus(N, D, k, seed, contiguous): Qt = ceil(N / k) random queries; row perm[i] belongs to query i // k (its owner) with rank
t = i % k and is 3 (a_t q^ + sqrt(1 - a_t^2) u), u a random unit vector orthogonal to q^ = the owner's direction, a_t falling
linearly from 0.95 (rank 0) to 0.80 (rank k - 1). Any other row's cosine to a query is that of two random directions (at D = 128:
sigma 0.09, below 0.5 over 10^8 pairs), so a query's exact top-k is its k planted rows, by a cosine gap of 0.3. perm is the
identity (contiguous: a query's winners fill one or two 16-row tiles — one wave, one group, one list) or a seeded permutation
(scattered over the index). The last query is short when N % k != 0.

filtered_corpus(N, D, k, seed, contiguous, mirrored): 2k rows per query. k DECOYS (a from 0.97 down to 0.90) carry the bit the
query excludes, k WINNERS (a from 0.88 down to 0.75) the bit it requires; query j requires bit j % 62 and excludes bit 63, so
the queries of one call use different masks. Slots 0..k-1 of a query's 2k are the decoys, or, mirrored, the winners: over the
two corpora every position hosts an admitted winner once and a better-scoring excluded row once."""
import functools
from typing import NamedTuple, Optional

import numpy as np

EXCLUDED_BIT = 63
MASK_BITS = 62


class Planted(NamedTuple):
    rows: np.ndarray      # float32 [N, D], norm 3 (the index normalises at add)
    queries: np.ndarray   # float32 [Qt, D]
    owner: np.ndarray     # int64 [N]: the query a row is planted for
    rank: np.ndarray      # int64 [N]: its rank among that query's planted rows (filtered: among the 2k, decoys and winners)
    k: int
    per_query: int        # rows planted per query: k, or 2k in a filtered corpus
    by_owner: tuple       # [Qt] ascending row ids of every query
    tags: Optional[np.ndarray] = None      # filtered: uint64 [N]
    require: Optional[np.ndarray] = None   # filtered: uint64 [Qt]
    exclude: Optional[np.ndarray] = None   # filtered: uint64 [Qt]
    decoy: Optional[np.ndarray] = None     # filtered: bool [N]

    @property
    def n_queries(self) -> int:
        return self.queries.shape[0]

    @property
    def n_full(self) -> int:
        """queries with all their planted rows (the last one is short when N is no multiple of per_query)"""
        return self.rows.shape[0] // self.per_query

    def rows_of(self, j: int) -> np.ndarray:
        """ascending row ids planted for query j (filtered: its decoys and winners)"""
        return self.by_owner[j]


def _by_owner(owner, n_queries):
    order = np.argsort(owner, kind="stable")              # rows ascending inside every owner
    return tuple(np.split(order, np.searchsorted(owner[order], np.arange(1, n_queries))))


def _philox(seed):
    return np.random.Generator(np.random.Philox(seed))


def _plant(N, D, per_query, a_of_slot, seed, contiguous):
    Qt = -(-N // per_query)
    rng = _philox(seed)
    queries = rng.standard_normal((Qt, D), dtype=np.float32)
    perm = np.arange(N, dtype=np.int64) if contiguous else _philox(seed + 1).permutation(N).astype(np.int64)
    i = np.arange(N, dtype=np.int64)
    owner = np.empty(N, np.int64)
    rank = np.empty(N, np.int64)
    owner[perm] = i // per_query
    rank[perm] = i % per_query
    q64 = queries.astype(np.float64)
    qh = (q64 / np.linalg.norm(q64, axis=1, keepdims=True))[owner]            # [N, D]
    u = rng.standard_normal((N, D))
    u -= (u * qh).sum(1, keepdims=True) * qh
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = np.asarray(a_of_slot, np.float64)[rank][:, None]
    rows = (3.0 * (a * qh + np.sqrt(1.0 - a * a) * u)).astype(np.float32)
    return rows, queries, owner, rank


@functools.lru_cache(maxsize=None)
def corpus(N, D, k, seed, contiguous) -> Planted:
    a = np.linspace(0.95, 0.80, k)
    rows, queries, owner, rank = _plant(N, D, k, a, seed, contiguous)
    return Planted(rows, queries, owner, rank, k, k, _by_owner(owner, queries.shape[0]))


@functools.lru_cache(maxsize=None)
def filtered_corpus(N, D, k, seed, contiguous, mirrored) -> Planted:
    decoy_a, winner_a = np.linspace(0.97, 0.90, k), np.linspace(0.88, 0.75, k)
    a = np.concatenate([winner_a, decoy_a] if mirrored else [decoy_a, winner_a])
    rows, queries, owner, rank = _plant(N, D, 2 * k, a, seed, contiguous)
    decoy = (rank >= k) if mirrored else (rank < k)
    bit = np.uint64(1) << (owner % MASK_BITS).astype(np.uint64)
    tags = bit | (decoy.astype(np.uint64) << np.uint64(EXCLUDED_BIT))     # a decoy carries the required bit AND the excluded one
    Qt = queries.shape[0]
    require = np.uint64(1) << (np.arange(Qt) % MASK_BITS).astype(np.uint64)
    exclude = np.full(Qt, np.uint64(1) << np.uint64(EXCLUDED_BIT), np.uint64)
    return Planted(rows, queries, owner, rank, k, 2 * k, _by_owner(owner, Qt), tags, require, exclude, decoy)


def admitted(p: Planted, j: int) -> np.ndarray:
    """ascending row ids query j of a filtered corpus admits"""
    req, exc = p.require[j], p.exclude[j]
    return np.nonzero(((p.tags & req) == req) & ((p.tags & exc) == 0))[0]


def expected(orc, p: Planted, stored, labels, k, full: bool, which=None):
    """The answer the index must give for the queries `which` (all by default): (labels [n, k], distances [n, k], counts [n]) of
    orc.query (oracle/retrieval_oracle or its C twin). full: over the whole index; otherwise over each query's own planted rows
    (test_planted_rows_cpu.py shows the two agree), except the short last query, which always gets the whole index. A filtered
    corpus: over the rows the query admits (a few hundred: always all of them)."""
    which = np.arange(p.n_queries) if which is None else np.asarray(which)
    if p.tags is None and full:
        return orc.query(p.queries[which], stored, labels, k)
    ol = np.empty((which.size, k), np.int64)
    od = np.empty((which.size, k), np.float32)
    oc = np.empty(which.size, np.int32)
    for o, j in enumerate(which):
        if p.tags is not None:
            sub = admitted(p, j)
        elif j >= p.n_full:
            sub = slice(None)
        else:
            sub = p.rows_of(j)
        ol[o], od[o], oc[o] = (x[0] for x in orc.query(p.queries[j:j + 1], stored[sub], labels[sub], k))
    return ol, od, oc


# ---------------------------------------------------------------------------------------------- the corpora the GPU tests use
SEED = 5
D = 128              # the positional structure of the scan and the 128-query score GEMM does not depend on D
D_STRIP = 256        # the staggered strip GEMM (and with it fp8 rows on the score GEMM, and the widen pass's GEMM) starts at dim 256
N_SCAN, N_DENSE, N_SAMPLE = 4099, 20011, 35003     # ragged against 16, 128 and 256
FULL_ORACLE_MAX_N = 4100                           # up to here the expected answer is the oracle over the whole index
LAYOUTS = {"scattered": False, "contiguous": True}
# (N, D, k) of every unfiltered corpus, each in both layouts, and of every filtered pair of corpora
PLAIN = [(N_SCAN, D, 10), (N_SCAN, D, 24), (N_SCAN, D, 100), (N_DENSE, D, 10), (N_DENSE, D_STRIP, 10), (N_SAMPLE, D_STRIP, 10)]
FILTERED = [(N_SCAN, D, 10), (N_SAMPLE, D, 10)]

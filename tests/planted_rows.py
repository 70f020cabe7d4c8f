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
two corpora every position hosts an admitted winner once and a better-scoring excluded row once.

ghosts(p, G, kind), tiny_live and plateau (below) serve test_dead_rows_cpu.py and test_index_dead_rows_gpu.py: the hostile rows
an emptied index keeps behind its count, and the live sets on which such a row would show."""
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


# ---------------------------------------------------------------------------------------------- dead rows behind count
# (test_dead_rows_cpu.py pins what follows, test_index_dead_rows_gpu.py leaves these rows behind the live ones)
GHOST_LABEL0 = 10 ** 12          # ghost row r is added under GHOST_LABEL0 + r: disjoint from (and above) every live label
GHOST_KINDS = ("twin", "nonfinite", "plateau")


def capacity_for(N):
    """the capacity an index created for N rows gets (1024 doubled until it holds them) = the rows a ghost corpus must fill"""
    G = 1024
    while G < N:
        G *= 2
    return G


def ghost_owner(p: Planted, G) -> np.ndarray:
    """int64 [G]: the query whose direction ghost row r copies, (r - N) mod Qt: behind N the queries take turns"""
    return (np.arange(G, dtype=np.int64) - p.rows.shape[0]) % p.n_queries


def ghosts(p: Planted, G, kind) -> np.ndarray:
    """float32 [G, D]: the rows that fill an index of capacity G before it is emptied and the live corpus p is added; rows [N, G)
    stay behind count. twin: row r is 3 q^_j, j = ghost_owner(p, G)[r], cosine 1.0 to query j against its best live row's 0.95
    (a decoy's 0.97). nonfinite: the same, but of every three rows one is all NaN, all +inf or all zero (in turn), stored as
    whatever the normalisation makes of it. plateau: every row is the first row query 0 owns (plateau(): the tied row)."""
    assert kind in GHOST_KINDS and G >= p.rows.shape[0]
    if kind == "plateau":
        return np.repeat(p.rows[p.rows_of(0)[:1]], G, axis=0)
    q64 = p.queries.astype(np.float64)
    qh = q64 / np.linalg.norm(q64, axis=1, keepdims=True)
    rows = (3.0 * qh[ghost_owner(p, G)]).astype(np.float32)
    if kind == "nonfinite":
        r = np.arange(G)
        for i, v in enumerate((np.nan, np.inf, 0.0)):
            rows[(r % 3 == 0) & (r // 3 % 3 == i)] = v
    return rows


def ghost_labels(G) -> np.ndarray:
    return GHOST_LABEL0 + np.arange(G, dtype=np.int64)


TINY_QUERIES = 200


@functools.lru_cache(maxsize=None)
def tiny_live(n_live, D, seed) -> Planted:
    """n_live random rows and TINY_QUERIES random queries: no planted winners (owner 0 holds every row; k = n_live). With
    k >= n_live a query's results are ALL live rows, those of negative cosine included, which a dead row scoring 0 outranks."""
    rng = _philox(seed)
    rows = (3.0 * rng.standard_normal((n_live, D))).astype(np.float32)
    queries = rng.standard_normal((TINY_QUERIES, D), dtype=np.float32)
    every = np.arange(n_live, dtype=np.int64)
    none = np.empty(0, np.int64)
    return Planted(rows, queries, np.zeros(n_live, np.int64), every, n_live, n_live, (every,) + (none,) * (TINY_QUERIES - 1))


PLATEAU_OTHERS = 3


@functools.lru_cache(maxsize=None)
def plateau(N, D, seed) -> Planted:
    """N rows of which N - PLATEAU_OTHERS are byte-identical (query 0 owns them, rank = their order) and three, at the two ends
    and in the middle, are random (query 1 owns them). Queries: the tied row's direction, its opposite plus a little noise (every
    tied row at the same NEGATIVE cosine, below a dead fp8 row's score 0), a random one, and one of the three other rows. For
    each of them the tied rows share one distance, so the answer's order is decided by the labels alone."""
    rng = _philox(seed)
    tied = rng.standard_normal(D)
    rows = np.repeat((3.0 * tied / np.linalg.norm(tied))[None].astype(np.float32), N, axis=0)
    others = np.array([0, N // 2, N - 1])
    rows[others] = (3.0 * rng.standard_normal((PLATEAU_OTHERS, D))).astype(np.float32)
    queries = np.stack([tied, -tied + 0.1 * rng.standard_normal(D), rng.standard_normal(D), rows[others[1]]]).astype(np.float32)
    owner = np.zeros(N, np.int64)
    owner[others] = 1
    rank = np.empty(N, np.int64)
    rank[owner == 0] = np.arange(N - PLATEAU_OTHERS)
    rank[others] = np.arange(PLATEAU_OTHERS)
    return Planted(rows, queries, owner, rank, N - PLATEAU_OTHERS, N - PLATEAU_OTHERS, _by_owner(owner, queries.shape[0]))


def not_excluded(p: Planted) -> np.ndarray:
    """ascending row ids a query of a filtered corpus admits when it only excludes (require = None): every row but the decoys"""
    return np.nonzero((p.tags & p.exclude[0]) == 0)[0]


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
# the dead-row tests: the unfiltered and filtered corpora above that they put ghosts behind (scattered layout), the tiny live
# sets, and the tie plateau of more rows than a widened query may collect (8192)
GHOSTED = [(N_SCAN, D, 10), (N_SCAN, D, 24), (N_SCAN, D, 100), (N_DENSE, D, 10), (N_DENSE, D_STRIP, 10), (N_SAMPLE, D_STRIP, 10)]
GHOSTED_FILTERED = [(N_SCAN, D, 10)]
TINY_LIVE = (1, 3, 19)
N_PLATEAU = 9003

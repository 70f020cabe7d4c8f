"""What the partitioned-search tests share (test_partition_cases_cpu.py, test_partition_layers_cpu.py, test_index_partition_gpu.py):
the numpy restatement of mmiss_index_query_probed on the retrieval oracle alone, the corpora (cached: the tests share the arrays
and leave them unchanged) and the comparator. Not a test module.

The restatement, for a query q and nprobe >= 1 (ro = oracle.retrieval_oracle):
  dc[c]   = ro.distances(q, ro.normalize_rows(centres, "f32"))[0, c]
  P(q)    = the min(nprobe, live) centres smallest by (dc[c], c) among the c with dc[c] not NaN
  cand(q) = { r < B : cells[r] in P(q) } and every r >= B
  result  = ro.query over the rows of cand(q) the masks admit; scanned = the sizes of the cells of P(q) + (N - B), 0 for a
            query without a direction."""
import numpy as np

from assign_cases import mirror, nodir_rows
from oracle import retrieval_oracle as ro

_cache = {}
ALL_BITS = (1 << 64) - 1


def labels_of(n):
    return np.arange(n, dtype=np.int64) * 3 + 5


def centre_distances(queries, centres):
    """dc float32 [Q, C]"""
    with np.errstate(all="ignore"):
        return ro.distances(np.asarray(queries, np.float32).reshape(-1, np.asarray(centres).shape[1]), ro.normalize_rows(centres, "f32"))


def probed_cells(dc_q, nprobe):
    """P(q), nearest first, from one row of centre_distances"""
    live = np.nonzero(~np.isnan(dc_q))[0]
    order = live[np.lexsort((live, dc_q[live]))]
    return order[:min(int(nprobe), live.size)]


def cell_sizes(cells, C):
    cells = np.asarray(cells).astype(np.int64)
    ok = (cells >= 0) & (cells < C)
    return np.bincount(cells[ok], minlength=C).astype(np.int64)


def _masks(m, Q):
    if m is None:
        return np.zeros(Q, np.uint64)
    return np.broadcast_to(np.asarray(m).astype(np.uint64), (Q,))


def expected_probed(queries, k, nprobe, centres, cells, B, stored, labels, tags=None, require=None, exclude=None):
    """-> (labels int64 [Q, k], distances float32 [Q, k], counts int32 [Q], scanned int64 [Q]); cells: int32 [B], B <= N"""
    queries = np.asarray(queries, np.float32).reshape(-1, np.asarray(centres).shape[1])
    Q, N, C = queries.shape[0], stored.shape[0], np.asarray(centres).shape[0]
    cells = np.asarray(cells).astype(np.int64)[:B]
    labels = np.asarray(labels, np.int64)
    tags = np.zeros(N, np.uint64) if tags is None else np.asarray(tags).astype(np.uint64)
    req, exc = _masks(require, Q), _masks(exclude, Q)
    sizes = cell_sizes(cells, C)
    dc = centre_distances(queries, centres)
    out_l = np.full((Q, k), -1, np.int64)
    out_d = np.full((Q, k), np.inf, np.float32)
    out_c = np.zeros(Q, np.int32)
    out_s = np.zeros(Q, np.int64)
    rows = np.arange(N)
    for q in range(Q):
        P = probed_cells(dc[q], nprobe)
        if P.size == 0:
            continue                       # a query without a direction: no live centre, count 0, scanned 0
        out_s[q] = sizes[P].sum() + (N - B)
        cand = rows >= B
        cand[:B] = np.isin(cells, P)
        admit = ((tags & req[q]) == req[q]) & ((tags & exc[q]) == 0)
        sub = np.nonzero(cand & admit)[0]
        if sub.size == 0:
            continue
        with np.errstate(all="ignore"):
            ol, od, oc = ro.query(queries[q:q + 1], stored[sub], labels[sub], k)
        out_l[q], out_d[q], out_c[q] = ol[0], od[0], oc[0]
    return out_l, out_d, out_c, out_s


def expected_flat(queries, k, stored, labels, tags=None, require=None, exclude=None):
    """ro.query over the rows the masks admit -> (labels, distances, counts): mmiss_index_query / _query_filtered"""
    queries = np.asarray(queries, np.float32)
    Q, N = queries.shape[0], stored.shape[0]
    if tags is None and require is None and exclude is None:
        with np.errstate(all="ignore"):
            return ro.query(queries, stored, labels, k)
    tags = np.zeros(N, np.uint64) if tags is None else np.asarray(tags).astype(np.uint64)
    req, exc = _masks(require, Q), _masks(exclude, Q)
    out = (np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros(Q, np.int32))
    for q in range(Q):
        sub = np.nonzero(((tags & req[q]) == req[q]) & ((tags & exc[q]) == 0))[0]
        if sub.size:
            with np.errstate(all="ignore"):
                ol, od, oc = ro.query(queries[q:q + 1], stored[sub], np.asarray(labels)[sub], k)
            out[0][q], out[1][q], out[2][q] = ol[0], od[0], oc[0]
    return out


# ------------------------------------------------------------------------------------------------ corpora
def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def stored_of(x, dtype):
    """oracle.normalize_rows(x, dtype), once per (array, dtype)"""
    key = ("stored", id(x), dtype)
    if key not in _cache:
        with np.errstate(all="ignore"):
            _cache[key] = (x, ro.normalize_rows(x, dtype))
    return _cache[key][1]


def query_masks(Q):
    """(require, exclude) uint64 [Q] on the tag bits of clustered(): bit 0 required by every second query, bit 2 excluded by
    every third"""
    q = np.arange(Q)
    return (q % 2).astype(np.uint64), ((q % 3 == 0) * 4).astype(np.uint64)


def clustered(seed, N, dim, C, Q, complete=False):
    """dict(x [N, dim], centres [C, dim], cells int32 [N], queries [Q, dim], tags uint64 [N]).
    Rows lie around the first min(C, 40) centres (C = 1024: mostly empty cells); cells are the nearest centre in float32
    arithmetic (any assignment is a partition: the contract is about the cells as given). Rows without a direction (zero, NaN,
    +inf) at assign_cases.nodir_rows(N), cell -1. Not `complete`: centre 1 has no direction (C > 1) and rows 30 .. 35 are put
    into its cell by hand — never probed —, rows 40 / 41 carry the cell numbers C + 3 / -7 (no cell). `complete`: every row
    with a direction has a valid cell with a live centre. Queries: noisy copies of rows, random vectors, and (Q > 2) query 2
    without a direction."""
    key = ("clustered", seed, N, dim, C, Q, complete)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(seed))
        c = rng.standard_normal((C, dim), dtype=np.float32)
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        which = rng.integers(0, min(C, 40), N)
        x = (c[which] + rng.standard_normal((N, dim), dtype=np.float32) * np.float32(1.5 / np.sqrt(dim))).astype(np.float32)
        dead = C > 1 and not complete
        if dead:
            c[1] = 0.0
        nd = nodir_rows(N)
        x[nd[0]] = 0.0
        x[nd[1], 5] = np.nan
        x[nd[2], 0] = np.inf
        x[nd[3]] = np.nan
        x[nd[4]] = 0.0
        with np.errstate(all="ignore"):
            score = np.nan_to_num(x, nan=0.0, posinf=0.0) @ c.T
        if dead:
            score[:, 1] = -np.inf
        cells = np.argmax(score, axis=1).astype(np.int32)
        cells[nd] = -1
        if not complete:
            if C > 1:
                cells[30:36] = 1
            cells[40], cells[41] = C + 3, -7
        qs = rng.standard_normal((Q, dim), dtype=np.float32)
        src = rng.integers(50, N - 50, Q)
        near = np.arange(Q) % 3 != 1
        qs[near] = x[src[near]] + rng.standard_normal((int(near.sum()), dim), dtype=np.float32) * np.float32(0.3 / np.sqrt(dim))
        qs = np.nan_to_num(qs, nan=0.5, posinf=1.0).astype(np.float32)
        if Q > 2:
            qs[2] = 0.0
        tags = rng.integers(0, 8, N).astype(np.uint64)
        _cache[key] = _freeze(dict(x=x, centres=c, cells=cells, queries=qs, tags=tags))
    return _cache[key]


def hidden_row(dim, n_per_cell=40):
    """Cells given by hand. Centres [a, b] far apart; rows 0 .. n-1 lie around a in cell 0, rows n .. 2n-1 around b in cell 1, and
    the last row of cell 1 is a bit copy of the query, which lies next to a: the exact nearest row sits in the cell of the far
    centre. -> dict(x, centres, cells, queries [1, dim], hidden: its row)"""
    key = ("hidden", dim, n_per_cell)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(77))
        a = np.zeros(dim, np.float32); a[0] = 1.0
        b = np.zeros(dim, np.float32); b[1] = 1.0
        n = n_per_cell
        noise = rng.standard_normal((2 * n, dim), dtype=np.float32) * np.float32(0.3 / np.sqrt(dim))
        x = np.concatenate([a + noise[:n], b + noise[n:]]).astype(np.float32)
        q = (a + rng.standard_normal(dim, dtype=np.float32) * np.float32(0.1 / np.sqrt(dim))).astype(np.float32)
        x[2 * n - 1] = q
        cells = np.repeat(np.array([0, 1], np.int32), n)
        _cache[key] = _freeze(dict(x=x, centres=np.stack([a, b]), cells=cells, queries=q[None].copy(), hidden=2 * n - 1))
    return _cache[key]


def centre_ties(dim, kind):
    """Two centres at EXACTLY the same canonical distance from the query, in cells of different sizes:
    kind "dup":    centres [a, b, a]; cell 0 holds 11 rows around a, cell 2 holds 23, cell 1 7 rows around b;
    kind "mirror": centres [c, mirror(c)] and a query with q[0] == q[64] (assign_cases.mirror: the same bits by construction);
                   cell 0 holds 11 rows, cell 1 holds 23.
    -> dict(x, centres, cells, queries [1, dim], tied: (first, second) the two tied cells, sizes)"""
    key = ("ties", dim, kind)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(78))
        a = rng.standard_normal(dim, dtype=np.float32)
        noise = lambda n: rng.standard_normal((n, dim), dtype=np.float32) * np.float32(0.5 / np.sqrt(dim))   # noqa: E731
        if kind == "dup":
            b = rng.standard_normal(dim, dtype=np.float32)
            centres = np.stack([a, b, a])
            x = np.concatenate([a + noise(11), b + noise(7), a + noise(23)]).astype(np.float32)
            cells = np.repeat(np.array([0, 1, 2], np.int32), [11, 7, 23])
            q = (a + noise(1)[0]).astype(np.float32)
            tied = (0, 2)
        else:
            centres = np.stack([a, mirror(a)])
            x = np.concatenate([a + noise(11), mirror(a) + noise(23)]).astype(np.float32)
            cells = np.repeat(np.array([0, 1], np.int32), [11, 23])
            q = (a + mirror(a) + noise(1)[0]).astype(np.float32)
            q[64] = q[0]
            tied = (0, 1)
        _cache[key] = _freeze(dict(x=x, centres=centres, cells=cells, queries=q[None].copy(), tied=tied,
                                   sizes=cell_sizes(cells, centres.shape[0])))
    return _cache[key]


EDGE_SIZES = (0, 1, 63, 64, 65, 4095, 4096, 4097, 4200)   # cell c holds EDGE_SIZES[c] rows: around the scan's share and the segment
EDGE_TAIL = 100


def plan_edges(dim):
    """Cells given by hand with the sizes EDGE_SIZES, interleaved over the rows (row r of the partition goes to the cell whose
    running quota is least filled, so the cells are not contiguous row ranges), EDGE_TAIL rows behind them for the tail. Queries:
    bit copies of the rows at the FIRST and the LAST position (by row number) of every non-empty cell and of the tail.
    -> dict(x [B + tail, dim], centres, cells int32 [B], queries, planted: their rows, B)"""
    key = ("edges", dim)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(79))
        C = len(EDGE_SIZES)
        B = sum(EDGE_SIZES)
        cells = np.repeat(np.arange(C, dtype=np.int32), EDGE_SIZES)
        cells = cells[rng.permutation(B)]
        c = rng.standard_normal((C, dim), dtype=np.float32)
        x = rng.standard_normal((B + EDGE_TAIL, dim), dtype=np.float32)
        planted = []
        for cell in range(C):
            r = np.nonzero(cells == cell)[0]
            if r.size:
                planted += [int(r[0]), int(r[-1])]
        planted += [B, B + EDGE_TAIL - 1]
        planted = sorted(set(planted))
        _cache[key] = _freeze(dict(x=x, centres=c, cells=cells, queries=x[planted].copy(), planted=np.asarray(planted), B=B))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ comparator
def mismatch(got, exp):
    """None when (labels, distances, counts[, scanned]) equals the expected tuple in every element (distances by their bits), else
    a message that names the first difference; a tuple of three compares no scanned"""
    names = ("labels", "dist", "count", "scanned")
    dtypes = (np.int64, np.float32, np.int32, np.int64)
    for name, dt, g, e in zip(names, dtypes, got, exp):
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape or g.dtype != dt:
            return f"{name}: shape / dtype {g.shape} {g.dtype}, expected {e.shape} {np.dtype(dt)}"
        bad = np.argwhere(g.view(np.uint32) != e.view(np.uint32)) if dt == np.float32 else np.argwhere(g != e)
        if bad.size:
            i = tuple(bad[0])
            return f"{name}: {bad.shape[0]} entries differ, first at {i}: got {g[i]!r}, expected {e[i]!r}"
    return None

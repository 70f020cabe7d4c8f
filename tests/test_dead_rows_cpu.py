"""What test_index_dead_rows_gpu.py rests on, checked with the oracle alone: the ghost rows of tests/planted_rows.py would change
every query's answer if a kernel let them through (so a passing GPU test means they were masked, not that they were harmless),
they fill every position behind the live rows, and the special corpora have the property their GPU tests name: the tiny live set
returns rows of negative cosine, the exclude-only call admits exactly the non-decoys and its answer is the query's own winners,
the plateau's expected answer is its smallest labels.

The oracle over live rows + twins is the whole one at N = 4099 (every query) and for the tiny sets; at N >= 20011 it is taken
over a query's own planted rows plus every ghost row for all queries, and over the whole index for a seeded sample of 32 (the
same reduction test_planted_rows_cpu.py justifies for the live rows)."""
import numpy as np
import pytest

import planted_rows as pr
from oracle import retrieval_oracle as ro
from oracle import retrieval_oracle_c as roc

DTYPES = ["f32", "f16", "f8"]
LAYOUT = pr.LAYOUTS["scattered"]
GHOST_COUNTS = {pr.N_SCAN: 4093, pr.N_DENSE: 12757, pr.N_SAMPLE: 30533}

PLAIN = [pytest.param(N, D, k, id=f"N{N}-D{D}-k{k}") for N, D, k in pr.GHOSTED]
FILT = [pytest.param(N, D, k, mir, id=f"N{N}-D{D}-k{k}-{'mirrored' if mir else 'plain'}") for N, D, k in pr.GHOSTED_FILTERED
        for mir in (False, True)]


def _labels(N):
    return np.arange(N, dtype=np.int64) * 3 + 5


def _sample(p, n=32):
    must = {0, p.n_full - 1, p.n_queries - 1}
    rest = np.random.Generator(np.random.Philox(99)).choice(p.n_queries, size=min(n, p.n_queries), replace=False).tolist()
    return np.array(sorted(must | set(rest)))


def _positions(p, G):
    """every position behind N holds a ghost, every query owns one, and so do the pad rows of the last 256-row tile"""
    N = p.rows.shape[0]
    assert G == pr.capacity_for(N) and G >= N and G % 1024 == 0 and (G == 1024 or G // 2 < N)
    owner = pr.ghost_owner(p, G)
    dead = owner[N:]
    assert dead.size == G - N
    per_query = np.bincount(dead, minlength=p.n_queries)
    assert per_query.min() >= 1, "a query without a ghost behind count"
    assert -(-N // 256) * 256 <= G                     # the positions N .. round_up(N, 256) - 1 lie inside the ghost rows
    twins = pr.ghosts(p, G, "twin")
    assert twins.shape == (G, p.rows.shape[1]) and twins.dtype == np.float32
    q64 = p.queries.astype(np.float64)
    qh = q64 / np.linalg.norm(q64, axis=1, keepdims=True)
    cos = (twins.astype(np.float64) / 3.0 * qh[owner]).sum(1)
    assert cos.min() > 1 - 1e-6                        # rows [0, N) are twins too: the index is hostile before it is emptied
    labels = pr.ghost_labels(G)
    assert labels.min() > _labels(N).max() and (np.diff(labels) > 0).all()
    return per_query


def _twins_win(p, dtype, k, G, per_query, live_rows_of, tags_ok=None):
    """the oracle over live rows + the twins behind them: every query's first min(k, its ghosts) results are ghost labels"""
    N = p.rows.shape[0]
    stored = ro.concat_rows([ro.normalize_rows(p.rows, dtype), ro.normalize_rows(pr.ghosts(p, G, "twin")[N:], dtype)])
    labels = np.concatenate([_labels(N), pr.ghost_labels(G)[N:]])
    dead = np.arange(N, G)

    def check(j, rows):
        l, d, c = (x[0] for x in roc.query(p.queries[j:j + 1], stored[rows], labels[rows], k))
        n = min(k, int(per_query[j]))
        assert n >= 1 and (l[:n] >= pr.GHOST_LABEL0).all(), (dtype, j, l)
        assert ((l[:n] - pr.GHOST_LABEL0 - N) % p.n_queries == j).all()          # ... its own twins
        return l, d, c

    whole = np.arange(G) if tags_ok is None else None
    if N <= pr.FULL_ORACLE_MAX_N:
        for j in range(p.n_queries):
            check(j, whole if tags_ok is None else np.concatenate([tags_ok(j), dead]))
        return
    for j in range(p.n_queries):
        check(j, np.concatenate([live_rows_of(j), dead[pr.ghost_owner(p, G)[N:] == j]]))
    for j in _sample(p):
        check(j, whole)


@pytest.mark.parametrize("N,D,k", PLAIN)
def test_unmasked_twins_would_change_every_answer(N, D, k):
    p = pr.corpus(N, D, k, pr.SEED, LAYOUT)
    G = pr.capacity_for(N)
    per_query = _positions(p, G)
    assert G - N == GHOST_COUNTS[N]
    print(f"N={N} D={D} k={k}: capacity {G}, {G - N} ghosts behind count, {per_query.min()}..{per_query.max()} per query")
    for dtype in DTYPES:
        _twins_win(p, dtype, k, G, per_query, p.rows_of)


@pytest.mark.parametrize("N,D,k,mirrored", FILT)
def test_unmasked_twins_would_change_every_filtered_answer(N, D, k, mirrored):
    """a ghost's tag is 0 after the clear: the query that only excludes admits it. Over the rows such a query admits plus the
    twins, the twins come first; without them its answer is its own k winners (the decoys, the only better rows, are excluded)."""
    p = pr.filtered_corpus(N, D, k, pr.SEED, LAYOUT, mirrored)
    G = pr.capacity_for(N)
    per_query = _positions(p, G)
    assert G - N == GHOST_COUNTS[N]
    admitted = pr.not_excluded(p)
    np.testing.assert_array_equal(admitted, np.nonzero(~p.decoy)[0])              # exactly the non-decoy rows
    labels = _labels(N)
    for dtype in DTYPES:
        _twins_win(p, dtype, k, G, per_query, None, tags_ok=lambda j: admitted)
        stored = ro.normalize_rows(p.rows, dtype)
        el, ed, ec = roc.query(p.queries, stored[admitted], labels[admitted], k)
        fl, fd, fc = pr.expected(roc, p, stored, labels, k, full=True)             # the require + exclude call
        for j in range(p.n_full):
            own = p.rows_of(j)
            np.testing.assert_array_equal(np.sort((el[j] - 5) // 3), own[~p.decoy[own]])
            assert ec[j] == k
        full = slice(0, p.n_full)                                                  # (the short last query admits other rows)
        np.testing.assert_array_equal(el[full], fl[full])
        np.testing.assert_array_equal(ed[full].view(np.uint32), fd[full].view(np.uint32))


@pytest.mark.parametrize("n_live", pr.TINY_LIVE)
def test_tiny_live_sets(n_live):
    p = pr.tiny_live(n_live, pr.D, pr.SEED)
    assert p.rows.shape == (n_live, pr.D) and p.n_queries == pr.TINY_QUERIES == 200
    G = pr.capacity_for(n_live)
    assert G == 1024
    per_query = _positions(p, G)
    assert per_query.min() >= 5
    labels = _labels(n_live)
    for dtype in DTYPES:
        stored = ro.normalize_rows(p.rows, dtype)
        for k in (10, 24):
            l, d, c = roc.query(p.queries, stored, labels, k)
            assert (c == min(k, n_live)).all()
            nl, nd, nc = ro.query(p.queries[:8], stored, labels, k)               # (the numpy oracle: the C one's own reference)
            np.testing.assert_array_equal(nl, l[:8])
            np.testing.assert_array_equal(nd.view(np.uint32), d[:8].view(np.uint32))
            _twins_win(p, dtype, k, G, per_query, None)
            if n_live == 19 and k == 24:
                # every query's 19 results include a live row of negative cosine (distance above 1): a dead fp8 row, whose
                # inverse norm of zero gives it the score 0, would outrank it
                assert (c == 19).all() and (d[:, :19].max(1) > 1.0).all()


@pytest.mark.parametrize("k", [10, 100])
def test_plateau_answer_is_its_smallest_labels(k):
    N = pr.N_PLATEAU
    p = pr.plateau(N, pr.D, pr.SEED)
    tied = p.rows_of(0)
    assert tied.size == N - pr.PLATEAU_OTHERS == 9000 > 8192 and pr.capacity_for(N) == 16384
    assert (p.rows[tied] == p.rows[tied[0]]).all()
    ghosts = pr.ghosts(p, 16384, "plateau")
    assert ghosts.shape == (16384, pr.D) and (ghosts == p.rows[tied[0]]).all()
    labels = _labels(N)
    for dtype in DTYPES:
        stored = ro.normalize_rows(p.rows, dtype)
        l, d, c = roc.query(p.queries, stored, labels, k)
        assert (c == k).all()
        np.testing.assert_array_equal(l[0], labels[tied[:k]])                      # its own direction: the k smallest labels
        assert (d[0] == d[0, 0]).all() and d[0, 0] < 1e-2
        assert (d[1] == d[1, -1]).sum() >= k - pr.PLATEAU_OTHERS and d[1, -1] > 1.5   # the opposite one: all tied, cosine < 0
        for j in range(p.n_queries):                                               # every query's k-th result lies on the plateau
            assert np.isin(l[j, -1], labels[tied])

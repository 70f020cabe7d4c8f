"""The properties of tests/planted_rows.py that test_index_positions_gpu.py rests on, for every (N, D, k, layout) it uses: owner and
rank partition the rows; in plain fp64 every full query's top-k is its planted set, by a cosine gap of at least 0.25 (the
construction gives 0.31 or more; the guard's eps_q is 2e-3 at most, so stage 1 can never be excused for losing one); and the
oracle restricted to a query's planted rows returns the labels and distance bits of the oracle over the whole index, which is
what lets the GPU tests check 2000 to 3500 queries per sweep."""
import numpy as np
import pytest

import planted_rows as pr
from oracle import retrieval_oracle as ro
from oracle import retrieval_oracle_c as roc

DTYPES = ["f32", "f16", "f8"]
MIN_GAP = 0.25

PLAIN = [pytest.param(N, D, k, lay, id=f"N{N}-D{D}-k{k}-{lay}") for N, D, k in pr.PLAIN for lay in pr.LAYOUTS]
FILT = [pytest.param(N, D, k, lay, mir, id=f"N{N}-D{D}-k{k}-{lay}-{'mirrored' if mir else 'plain'}")
        for N, D, k in pr.FILTERED for lay in pr.LAYOUTS for mir in (False, True)]


def _unit64(x):
    x = x.astype(np.float64)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _cosine_gap(p, rows_ok=None):
    """min over the full queries of (worst planted winner's cosine - best other row's cosine), in plain fp64. rows_ok(j) -> bool [N]
    restricts query j's competition (filtered corpora: the admitted rows); winners = the planted rows among them."""
    r, q = _unit64(p.rows), _unit64(p.queries)
    N = r.shape[0]
    gap = np.inf
    for j0 in range(0, p.n_full, 512):
        j1 = min(j0 + 512, p.n_full)
        cos = q[j0:j1] @ r.T                                        # [b, N]
        own = p.owner[None, :] == np.arange(j0, j1)[:, None]
        if rows_ok is not None:
            ok = np.stack([rows_ok(j) for j in range(j0, j1)])
            cos = np.where(ok, cos, -np.inf)                        # rows the query does not admit do not compete
            own &= ok
        assert (own.sum(1) == p.k).all()
        worst = np.where(own, cos, np.inf).min(1)
        best_other = np.where(own, -np.inf, cos).max(1)
        # the top-k SET is the planted set: exactly k rows reach the worst winner
        assert ((cos >= worst[:, None]).sum(1) == p.k).all()
        gap = min(gap, float((worst - best_other).min()))
    return gap


def _sample(p, n=32):
    """>= n queries: the first, the last full one, the short one (when there is one), and a seeded draw of the others"""
    must = {0, p.n_full - 1, p.n_queries - 1}
    rng = np.random.Generator(np.random.Philox(99))
    rest = rng.choice(p.n_queries, size=min(n, p.n_queries), replace=False).tolist()
    return np.array(sorted(must | set(rest)))


def _same(a, b, what):
    np.testing.assert_array_equal(a[2], b[2], err_msg=what)
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32), err_msg=what)


def _partition(p):
    N = p.rows.shape[0]
    assert p.n_queries == -(-N // p.per_query)
    assert np.concatenate(p.by_owner).size == N and np.unique(np.concatenate(p.by_owner)).size == N
    key = p.owner * p.per_query + p.rank                            # (owner, rank) is a bijection onto 0 .. N - 1
    np.testing.assert_array_equal(np.sort(key), np.arange(N))
    short = N % p.per_query
    assert (N % p.per_query != 0) == (p.n_full < p.n_queries)
    for j in (0, p.n_full - 1):
        assert p.rows_of(j).size == p.per_query and (p.owner[p.rows_of(j)] == j).all()
    if short:
        assert p.rows_of(p.n_queries - 1).size == short
    np.testing.assert_allclose(np.linalg.norm(p.rows.astype(np.float64), axis=1), 3.0, rtol=1e-6)


@pytest.mark.parametrize("N,D,k,layout", PLAIN)
def test_every_row_is_a_winner_of_exactly_one_query(N, D, k, layout):
    p = pr.corpus(N, D, k, pr.SEED, pr.LAYOUTS[layout])
    _partition(p)
    if pr.LAYOUTS[layout]:
        np.testing.assert_array_equal(p.owner, np.arange(N) // k)
    else:
        assert np.unique(p.rows_of(0) // 16).size >= min(k, 8)      # scattered: a query's winners lie in many tiles
    gap = _cosine_gap(p)
    print(f"N={N} D={D} k={k} {layout}: cosine gap {gap:.4f}")
    assert gap >= MIN_GAP, gap
    labels = np.arange(N, dtype=np.int64) * 3 + 5
    which = _sample(p)
    assert which.size >= 32 or which.size == p.n_queries
    for dtype in DTYPES:
        stored = ro.normalize_rows(p.rows, dtype)
        full = roc.query(p.queries[which], stored, labels, k)
        _same(pr.expected(roc, p, stored, labels, k, full=False, which=which), full, f"{dtype} restricted vs full")
        if N <= pr.FULL_ORACLE_MAX_N:                               # (the numpy oracle: the C one's own reference)
            _same(ro.query(p.queries[which[:8]], stored, labels, k), tuple(x[:8] for x in full), f"{dtype} numpy vs C oracle")
        # the oracle's own distance gap between a full query's last winner and the first row behind it
        fullq = which[which < p.n_full]
        l2, d2, _ = roc.query(p.queries[fullq], stored, labels, k + 1)
        np.testing.assert_array_equal(np.sort((l2[:, :k] - 5) // 3, axis=1), np.stack([p.rows_of(j) for j in fullq]))
        assert (d2[:, k] - d2[:, k - 1]).min() >= MIN_GAP, dtype


@pytest.mark.parametrize("N,D,k,layout,mirrored", FILT)
def test_filtered_corpus_decoys_beat_winners_and_are_never_admitted(N, D, k, layout, mirrored):
    p = pr.filtered_corpus(N, D, k, pr.SEED, pr.LAYOUTS[layout], mirrored)
    _partition(p)
    other = pr.filtered_corpus(N, D, k, pr.SEED, pr.LAYOUTS[layout], not mirrored)
    assert (p.decoy != other.decoy).all()                           # over the two corpora every position is a decoy once
    np.testing.assert_array_equal(p.owner, other.owner)
    assert np.unique(p.require[:64]).size == pr.MASK_BITS           # the queries of one call use different masks
    adm = {}

    def rows_ok(j):
        m = np.zeros(N, bool)
        m[pr.admitted(p, j)] = True
        adm[j] = m
        return m

    gap = _cosine_gap(p, rows_ok)
    print(f"N={N} D={D} k={k} {layout} mirrored={mirrored}: cosine gap over the admitted rows {gap:.4f}")
    assert gap >= MIN_GAP, gap
    r, q = _unit64(p.rows), _unit64(p.queries)
    for j in range(p.n_full):
        own = p.rows_of(j)
        dec, win = own[p.decoy[own]], own[~p.decoy[own]]
        assert dec.size == k and win.size == k
        assert not adm[j][dec].any() and adm[j][win].all()
        assert (r[dec] @ q[j]).min() > (r[win] @ q[j]).max()        # every decoy beats every winner of its query
    labels = np.arange(N, dtype=np.int64) * 3 + 5
    which = _sample(p)
    for dtype in DTYPES:
        stored = ro.normalize_rows(p.rows, dtype)
        el, ed, ec = pr.expected(roc, p, stored, labels, k, full=True, which=which)
        for o, j in enumerate(which):
            # the unfiltered oracle puts the query's decoys first: an index that ignored the tags would return them
            ul, _, _ = roc.query(p.queries[j:j + 1], stored, labels, k)
            own = p.rows_of(j)
            ndec = int(p.decoy[own].sum())
            assert set(((ul[0][:min(ndec, k)] - 5) // 3).tolist()) <= set(own[p.decoy[own]].tolist())
            if j < p.n_full:
                np.testing.assert_array_equal(np.sort((el[o] - 5) // 3), own[~p.decoy[own]])
                assert ec[o] == k
            else:                                                   # the short query: the whole admitted set decides
                sub = pr.admitted(p, j)
                _same(tuple(x[o:o + 1] for x in (el, ed, ec)), roc.query(p.queries[j:j + 1], stored[sub], labels[sub], k), dtype)

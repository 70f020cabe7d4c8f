"""Filtered queries (mmiss_index_query_filtered, FlatIndex.query(require=, exclude=)) on the MI355X against the C oracle run
on the ADMITTED subset of the rows: ids, counts and distance bits of every checked query must equal
ro.query(q, stored[admitted], labels[admitted], k) — the exact top-k among the rows the query's predicate admits
((tag & require) == require and (tag & exclude) == 0), where the reference post-filters the k nearest rows
(backend/app/main.py:202-222)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 8   # tags: bits 0..7 uniform random; bit 8 on ~0.1 % of the rows; bit 9 on none


@pytest.fixture(scope="module")
def mods():
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib
    from mmiss_amd.index import FlatIndex
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    return FlatIndex, ro, roc, _lib


def _randn(n, d, seed):
    return np.random.Generator(np.random.Philox(seed)).standard_normal((n, d), dtype=np.float32)


def _tags(n, seed):
    rng = np.random.Generator(np.random.Philox(seed))
    t = rng.integers(0, 256, size=n, dtype=np.uint64)
    t |= (rng.random(n) < 0.001).astype(np.uint64) << np.uint64(BIG)
    return t


# (require, exclude) pairs by admitted fraction
MASKS = {
    "0.5": (1, 0),
    "0.1": (0b111, 0),                       # 1/8
    "0.001": (1 << BIG, 0),
    "0": (1 << (BIG + 1), 0),                # a bit no row has
    "0 (contradiction)": (0b10, 0b10),
    "mixed": (0b1, 0b110),                   # 1/8 with an exclusion
}


def _admitted(tags, req, exc):
    tags = np.asarray(tags, np.uint64)
    req, exc = np.uint64(req), np.uint64(exc)
    return ((tags & req) == req) & ((tags & exc) == 0)


def _check(roc, stored, labels, tags, q, k, req, exc, lab, dist, cnt, which=None):
    """req / exc: [Q] numpy; lab / dist / cnt: the index's answer. Checks the queries in `which` (all by default)."""
    Q = q.shape[0]
    which = range(Q) if which is None else which
    for i in which:
        adm = _admitted(tags, req[i], exc[i])
        sub = np.nonzero(adm)[0]
        if sub.size == 0:
            assert cnt[i] == 0 and (lab[i] == -1).all() and np.isinf(dist[i]).all(), i
            continue
        ol, od, oc = roc.query(q[i:i + 1], stored[sub], labels[sub], k)
        np.testing.assert_array_equal(cnt[i:i + 1], oc, err_msg=f"query {i}")
        np.testing.assert_array_equal(lab[i:i + 1], ol, err_msg=f"query {i}")
        np.testing.assert_array_equal(dist[i:i + 1].view(np.uint32), od.view(np.uint32), err_msg=f"query {i}")


def _build(FlatIndex, ro, dtype, N, D, seed):
    c = _randn(N, D, seed)
    labels = np.arange(N, dtype=np.int64) * 2 + 1
    idx = FlatIndex(D, dtype, capacity=N)
    idx.add(c, labels)
    tags = _tags(N, seed + 1)
    idx.set_tags(labels, tags)
    return idx, ro.normalize_rows(c, dtype), labels, tags


@pytest.mark.parametrize("dtype", ["f32", "f16", "f8"])
@pytest.mark.parametrize("N,D", [(1000, 128), (20011, 768), (70001, 512)])
def test_filtered_query_matches_the_oracle_on_the_admitted_rows(mods, dtype, N, D):
    FlatIndex, ro, roc, _ = mods
    idx, stored, labels, tags = _build(FlatIndex, ro, dtype, N, D, seed=N + D)
    np.testing.assert_array_equal(idx.get_tags(labels[::97]), tags[::97])
    for Q in (1, 3, 17, 70, 300):
        q = _randn(Q, D, seed=Q * 7 + D)
        check = sorted(set(np.linspace(0, Q - 1, min(Q, 5)).astype(int).tolist()))
        for k in (1, 10, 24, 100):
            for name in ("0.5", "0.1", "0.001", "0"):
                req, exc = MASKS[name]
                lab, dist, cnt = idx.query(q, k, require=req, exclude=exc if exc else None)
                assert lab.shape == (Q, k) and dist.shape == (Q, k) and cnt.shape == (Q,)
                rq, rx = np.full(Q, req, np.uint64), np.full(Q, exc, np.uint64)
                # every query: nothing returned that the predicate rejects, counts = min(k, admitted)
                ok = lab >= 0
                assert np.isin(lab[ok], labels[_admitted(tags, req, exc)]).all(), (name, Q, k)
                assert (cnt == np.minimum(k, _admitted(tags, req, exc).sum())).all(), (name, Q, k)
                _check(roc, stored, labels, tags, q, k, rq, rx, lab, dist, cnt, check)
    idx.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "f8"])
def test_different_masks_per_query_host_and_device(mods, dtype):
    import torch

    FlatIndex, ro, roc, _ = mods
    N, D = 30011, 256
    idx, stored, labels, tags = _build(FlatIndex, ro, dtype, N, D, seed=5)
    names = list(MASKS)
    for Q, k in ((5, 10), (40, 24), (130, 100)):
        q = _randn(Q, D, seed=Q + 11)
        pick = [names[i % len(names)] for i in range(Q)]
        req = np.array([MASKS[p][0] for p in pick], np.uint64)
        exc = np.array([MASKS[p][1] for p in pick], np.uint64)
        lab, dist, cnt = idx.query(q, k, require=req, exclude=exc)
        _check(roc, stored, labels, tags, q, k, req, exc, lab, dist, cnt)
        # the same masks as CUDA tensors (int64 bit patterns), with CUDA queries: CUDA outputs, same bits
        qd = torch.from_numpy(q).cuda()
        l2, d2, c2 = idx.query(qd, k, require=torch.from_numpy(req.view(np.int64)).cuda(),
                               exclude=torch.from_numpy(exc.view(np.int64)).cuda())
        assert l2.is_cuda and d2.is_cuda
        np.testing.assert_array_equal(l2.cpu().numpy(), lab)
        np.testing.assert_array_equal(d2.cpu().numpy().view(np.uint32), dist.view(np.uint32))
        np.testing.assert_array_equal(c2.cpu().numpy(), cnt)
        # host queries, device masks
        l3, d3, _ = idx.query(q, k, require=torch.from_numpy(req.view(np.int64)).cuda(), exclude=exc)
        np.testing.assert_array_equal(l3, lab)
        np.testing.assert_array_equal(d3.view(np.uint32), dist.view(np.uint32))
    idx.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "f8"])
def test_zero_masks_equal_the_unfiltered_query(mods, dtype):
    """All masks 0 admit every row: the filtered call (streaming scan, FILT form) returns what the unfiltered one returns, bit
    for bit — also for Q > 16 on f16 / Q > 128 on fp8, where the unfiltered call takes the score GEMM."""
    FlatIndex, ro, roc, _lib = mods
    N, D = 20011, 512
    c = _randn(N, D, seed=77)
    labels = np.arange(N, dtype=np.int64)
    idx = FlatIndex(D, dtype, capacity=N)
    idx.add(c, labels)
    idx.set_tags(labels[::3], np.full(labels[::3].shape, 0xF0F0, np.uint64))
    for Q, k in ((1, 10), (20, 10), (150, 10), (7, 100)):
        q = _randn(Q, D, seed=Q + 3)
        a = idx.query(q, k)
        b = idx.query(q, k, require=0, exclude=0)
        c2 = idx.query(q, k, require=np.zeros(Q, np.uint64))
        for x in (b, c2):
            np.testing.assert_array_equal(x[0], a[0])
            np.testing.assert_array_equal(x[1].view(np.uint32), a[1].view(np.uint32))
            np.testing.assert_array_equal(x[2], a[2])
    # the filtered call never takes the score GEMM
    _lib.prof_enable(True)
    try:
        _lib.prof_reset()
        idx.query(_randn(150, D, seed=1), 10, require=0)
    finally:
        _lib.prof_enable(False)
    kern = {p["kernel"] for p in _lib.prof_read()}
    assert not any(k.startswith("score_gemm") for k in kern) and any(k.startswith("scan_topk") for k in kern), kern
    idx.close()


@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_guard_widens_filtered_queries_on_near_duplicates(mods, dtype):
    """Rows and queries in one narrow cone (pairwise cosine ~0.99, as the encoder's own embeddings): the k-th and k'-th
    approximate scores among the admitted rows sit inside the error bound, so the guard widens; the widen pass collects
    admitted rows only and the answer is still the oracle's on the admitted subset."""
    FlatIndex, ro, roc, _lib = mods
    N, D = 40000, 512
    base = _randn(1, D, seed=3)
    c = base + _randn(N, D, seed=4) * np.float32(np.sqrt(0.002 / D))
    labels = np.arange(N, dtype=np.int64)
    idx = FlatIndex(D, dtype, capacity=N)
    idx.add(c, labels)
    tags = _tags(N, seed=9)
    idx.set_tags(labels, tags)
    stored = ro.normalize_rows(c, dtype)
    Q = 6
    q = base + _randn(Q, D, seed=6) * np.float32(np.sqrt(0.002 / D))
    req = np.array([1, 0b11, 1, 0b111, 1 << BIG, 0], np.uint64)
    exc = np.array([0, 0, 0b100, 0, 0, 0b1000], np.uint64)
    for k in (10, 24):
        before = idx.guard_stats()
        lab, dist, cnt = idx.query(q, k, require=req, exclude=exc)
        after = idx.guard_stats()
        assert after["queries"] - before["queries"] == Q
        assert after["widened"] - before["widened"] >= Q // 2, (before, after)
        _check(roc, stored, labels, tags, q, k, req, exc, lab, dist, cnt)
    _lib.set_option("guard_force", 1)   # every query with a full first-pass list through the widen pass
    try:
        lab, dist, cnt = idx.query(q, 10, require=req, exclude=exc)
    finally:
        _lib.set_option("guard_force", 0)
    _check(roc, stored, labels, tags, q, 10, req, exc, lab, dist, cnt)
    idx.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "f8"])
def test_a_filtered_plateau_goes_to_the_exhaustive_pass(mods, dtype):
    """18 000 identical rows, every other one admitted: the widen pass collects more admitted rows than it holds (8192), the
    query goes to the exhaustive canonical pass, which must select among admitted rows only."""
    FlatIndex, ro, roc, _ = mods
    N, D = 24000, 128
    c = _randn(N, D, seed=21)
    c[:18000] = c[0]
    labels = np.arange(N, dtype=np.int64)
    tags = (labels % 2 == 1).astype(np.uint64) | np.uint64(4)
    idx = FlatIndex(D, dtype, capacity=N)
    idx.add(c, labels)
    idx.set_tags(labels, tags)
    stored = ro.normalize_rows(c, dtype)
    q = np.stack([c[0], _randn(1, D, seed=22)[0]])
    req, exc = np.array([1, 1], np.uint64), np.zeros(2, np.uint64)
    before = idx.guard_stats()["exhaustive"]
    lab, dist, cnt = idx.query(q, 10, require=req)
    assert idx.guard_stats()["exhaustive"] - before >= 1
    assert (lab[0] % 2 == 1).all() and (lab[0] < 18000).all(), lab[0]   # no rejected copy
    _check(roc, stored, labels, tags, q, 10, req, exc, lab, dist, cnt)
    idx.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "f8"])
def test_rows_without_a_direction_are_never_returned_under_a_filter(mods, dtype):
    FlatIndex, ro, roc, _ = mods
    N, D = 300, 128
    c = _randn(N, D, seed=31)
    c[5] = 0.0
    c[17, 3] = np.nan
    c[40, 0] = np.inf
    c[41] = 0.0
    labels = np.arange(N, dtype=np.int64)
    idx = FlatIndex(D, dtype)
    idx.add(c, labels)
    tags = np.zeros(N, np.uint64)
    tags[:60] = 1
    idx.set_tags(labels, tags)
    lab, dist, cnt = idx.query(_randn(2, D, seed=32), 100, require=1)
    assert (cnt == 56).all(), cnt
    got = set(lab[0, :56].tolist())
    assert got == set(range(60)) - {5, 17, 40, 41}
    assert (lab[:, 56:] == -1).all() and np.isinf(dist[:, 56:]).all()
    idx.close()


def test_tags_follow_the_rows_through_mutation_and_persistence(mods, tmp_path):
    FlatIndex, ro, roc, _ = mods
    N, D = 5000, 256
    c = _randn(N, D, seed=41)
    labels = np.arange(N, dtype=np.int64) * 3
    idx = FlatIndex(D, "f16")
    idx.add(c, labels)
    assert (idx.get_tags(labels) == 0).all()
    tags = _tags(N, seed=42)
    idx.set_tags(labels, tags)
    np.testing.assert_array_equal(idx.get_tags(labels), tags)
    with pytest.raises(Exception):
        idx.set_tags(np.array([labels[0], 1]), np.array([7, 7], np.uint64))   # label 1 is not in the index: nothing changes
    assert idx.get_tags(labels[:1])[0] == tags[0]
    # update keeps the tag
    c[10] = _randn(1, D, seed=43)[0]
    idx.update(labels[10:11], c[10:11])
    np.testing.assert_array_equal(idx.get_tags(labels), tags)
    # stable removal keeps the survivors' tags
    gone = np.arange(0, N, 7)
    idx.remove(labels[gone])
    keep = np.setdiff1d(np.arange(N), gone)
    np.testing.assert_array_equal(idx.get_tags(labels[keep]), tags[keep])
    q = _randn(4, D, seed=44)
    stored = ro.normalize_rows(c[keep], "f16")
    req = np.array([1, 0b11, 1 << BIG, 0b101], np.uint64)
    exc = np.array([0b10, 0, 0, 0], np.uint64)
    lab, dist, cnt = idx.query(q, 10, require=req, exclude=exc)
    _check(roc, stored, labels[keep], tags[keep], q, 10, req, exc, lab, dist, cnt)
    # add: new rows get tag 0
    c2 = _randn(100, D, seed=45)
    l2 = np.arange(100, dtype=np.int64) + 3 * N
    idx.add(c2, l2)
    assert (idx.get_tags(l2) == 0).all()
    np.testing.assert_array_equal(idx.get_tags(labels[keep]), tags[keep])
    lab, dist, cnt = idx.query(q, 10, exclude=np.uint64(0xFFFF))   # admits exactly the rows with tag 0 in bits 0..15
    all_lab = np.concatenate([labels[keep], l2])
    all_tags = np.concatenate([tags[keep], np.zeros(100, np.uint64)])
    all_stored = ro.normalize_rows(np.concatenate([c[keep], c2]), "f16")
    _check(roc, all_stored, all_lab, all_tags, q, 10, np.zeros(4, np.uint64), np.full(4, 0xFFFF, np.uint64), lab, dist, cnt)
    # save / load: the file holds no tags, they come back as 0
    path = str(tmp_path / "t.mmiss")
    idx.save(path)
    other = FlatIndex(D, "f16")
    other.load(path)
    assert (other.get_tags(all_lab) == 0).all()
    idx.load(path)
    assert (idx.get_tags(all_lab) == 0).all()
    lab, dist, cnt = idx.query(q, 10, require=1)
    assert (cnt == 0).all() and (lab == -1).all()
    # clear
    idx.set_tags(all_lab[:5], np.full(5, 1, np.uint64))
    idx.clear()
    assert idx.count() == 0
    with pytest.raises(Exception):
        idx.get_tags(all_lab[:1])
    idx.add(c[:20], labels[:20])
    assert (idx.get_tags(labels[:20]) == 0).all()
    idx.close()
    other.close()


def test_filtered_begin_end_and_abort(mods):
    FlatIndex, ro, roc, _ = mods
    N, D = 9000, 256
    idx, stored, labels, tags = _build(FlatIndex, ro, "f16", N, D, seed=51)
    q = _randn(5, D, seed=52)
    req = np.array([1, 2, 4, 8, 1 << BIG], np.uint64)
    exc = np.zeros(5, np.uint64)
    want = idx.query(q, 24, require=req)
    p = idx.query_begin(q, 24, require=req)
    with pytest.raises(Exception):
        idx.set_tags(labels[:1], np.zeros(1, np.uint64))   # the index belongs to the open query
    lab, dist, cnt = p.result()
    np.testing.assert_array_equal(lab, want[0])
    np.testing.assert_array_equal(dist.view(np.uint32), want[1].view(np.uint32))
    _check(roc, stored, labels, tags, q, 24, req, exc, lab, dist, cnt)
    p = idx.query_begin(q, 24, require=req)
    p.abort()
    # query_next: the pending filtered query's results and the next filtered query's handle
    p = idx.query_begin(q, 24, require=req)
    prev, p2 = idx.query_next(p, q[:2], 10, require=np.uint64(1), exclude=np.uint64(2))
    np.testing.assert_array_equal(prev[0], want[0])
    lab2, dist2, cnt2 = p2.result()
    _check(roc, stored, labels, tags, q[:2], 10, np.ones(2, np.uint64), np.full(2, 2, np.uint64), lab2, dist2, cnt2)
    # the unfiltered handle still works after them
    u = idx.query(q, 10)
    ol, od, oc = roc.query(q, stored, labels, 10)
    np.testing.assert_array_equal(u[0], ol)
    idx.close()


def test_scale_1_25m_rows_f16(mods):
    """configs[3]'s per-GPU shard: 1.25M x 512 f16 rows, Q = 4, different masks per query."""
    import torch

    FlatIndex, ro, roc, _ = mods
    N, D = 1_250_000, 512
    c = _randn(N, D, seed=61)
    labels = np.arange(N, dtype=np.int64)
    idx = FlatIndex(D, "f16", capacity=N)
    idx.add(torch.from_numpy(c).cuda(), labels)
    tags = _tags(N, seed=62)
    idx.set_tags(labels, tags)
    q = _randn(4, D, seed=63)
    req = np.array([1, 0b111, 1 << BIG, 0b1], np.uint64)
    exc = np.array([0, 0, 0, 0b1110], np.uint64)
    lab, dist, cnt = idx.query(q, 10, require=req, exclude=exc)
    stored = roc.normalize_rows(c, "f16")
    _check(roc, stored, labels, tags, q, 10, req, exc, lab, dist, cnt)
    idx.close()


def test_collection_prefilter_equals_the_post_filter_of_the_full_ranking(mods):
    import json

    import mmiss_amd  # noqa: F401
    from mmiss_amd.api import apply_filters
    from mmiss_amd.collection import FlatCollection

    N, D = 1800, 256
    rng = np.random.Generator(np.random.Philox(71))
    v = _randn(N, D, seed=72)
    names = ["outdoor", "people", "night", "animal"]
    metas = []
    for i in range(N):
        ans = {n: ("Yes" if rng.random() < p else "no") for n, p in zip(names, (0.5, 0.2, 0.1, 0.02))}
        metas.append({"id": f"img_{i}", "filter_results_json": json.dumps(ans)} if i % 50 else {"id": f"img_{i}"})
    col = FlatCollection("f", dim=D, dtype="f16")
    col.add(ids=[f"img_{i}" for i in range(N)], embeddings=v, metadatas=metas)
    q = _randn(3, D, seed=73)
    for filters in (["outdoor"], ["outdoor", "night"], ["animal", "people"], ["night"]):
        got = col.query(query_embeddings=q, n_results=10, include=["metadatas", "distances"], filters=filters)
        full = col.query(query_embeddings=q, n_results=N, include=["metadatas", "distances"])
        for qi in range(3):
            kept = [(m["id"], d) for m, d in zip(full["metadatas"][qi], full["distances"][qi])
                    if apply_filters([m], filters)][:10]
            assert got["ids"][qi] == [i for i, _ in kept], filters
            assert got["distances"][qi] == [d for _, d in kept]
    # metadata changes reach the next filtered query
    col.update(ids=["img_1"], metadatas=[{"filter_results_json": json.dumps({"animal": "yes", "people": "yes"})}])
    got = col.query(query_embeddings=v[1:2], n_results=1, filters=["animal", "people"])
    assert got["ids"] == [["img_1"]]
    assert col.query(query_embeddings=q, n_results=5, filters=["never-asked"])["ids"] == [[], [], []]

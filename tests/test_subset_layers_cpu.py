"""The host layers of subset search without a GPU, on the oracle-backed stand-in of tests/subset_fakes.py: the `where` evaluator,
FlatCollection.query(ids=, where=) — the intersection, unknown ids, filters as masks, a filter name past the 64th bit folded into
the list, max_distance, n_probe, distinct_distance, the empty set —, FlatCollection.get(where=), the search wrappers and the three
API routes that pass the list through, the argument checks FlatIndex.query_subset makes before it calls the library, and the
recorded proof that a call without the new keywords never reaches query_subset."""
import json
import threading

import numpy as np
import pytest

import subset_cases as sc
from fakes import OracleEncoder
from oracle import clip_oracle as co
from oracle import retrieval_oracle as ro
from subset_fakes import OracleSubsetIndex
from test_partition_layers_cpu import _NoLibrary
from test_radius_layers_cpu import _Proc, _image, _png

N, D = 300, 128
ALBUMS = ("beach", "city", "forest")


@pytest.fixture()
def colmod(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection

    OracleSubsetIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleSubsetIndex)
    return collection


def _ids(n=N):
    return [f"im{i:04d}" for i in range(n)]


def _metas(n=N, filters=1):
    """album: one of three; year: 2000 + r % 25, absent on every seventh row; score: r / n; filter answers f0 .. by parity"""
    out = []
    for r, i in enumerate(_ids(n)):
        m = {"id": i, "album": ALBUMS[r % 3], "score": r / n,
             "filter_results_json": json.dumps({f"f{j}": "yes" if (r + j) % 2 else "no" for j in range(filters)})}
        if r % 7:
            m["year"] = 2000 + r % 25
        out.append(m)
    return out


def _filled(colmod, n=N, filters=1):
    p = sc.corpus(41, n, D, 4)
    col = colmod.FlatCollection("t")
    col.add(ids=_ids(n), embeddings=p["x"], metadatas=_metas(n, filters))     # (labels 0 .. n-1: label == row)
    return col, p, OracleSubsetIndex.instances[-1]


def _as_result(exp, n=N, cut=None):
    cnt = exp[2] if cut is None else cut
    return ([[_ids(n)[int(l)] for l in exp[0][i, :cnt[i]]] for i in range(len(cnt))],
            [[float(d) for d in exp[1][i, :cnt[i]]] for i in range(len(cnt))])


def _rows_where(metas, pred):
    return [r for r, m in enumerate(metas) if pred(m)]


# ================================================================================================ the evaluator
def test_every_where_operator():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.collection import check_where, where_matches

    metas = _metas()
    cases = [
        ({"album": "city"}, lambda m: m["album"] == "city"),
        ({"album": {"$eq": "city"}}, lambda m: m["album"] == "city"),
        ({"album": {"$ne": "city"}}, lambda m: m["album"] != "city"),
        ({"year": {"$gt": 2010}}, lambda m: "year" in m and m["year"] > 2010),
        ({"year": {"$gte": 2010}}, lambda m: "year" in m and m["year"] >= 2010),
        ({"year": {"$lt": 2010}}, lambda m: "year" in m and m["year"] < 2010),
        ({"year": {"$lte": 2010}}, lambda m: "year" in m and m["year"] <= 2010),
        ({"year": {"$in": [2001, 2002, 2024]}}, lambda m: m.get("year") in (2001, 2002, 2024)),
        ({"year": {"$nin": [2001, 2002, 2024]}}, lambda m: m.get("year") not in (2001, 2002, 2024)),
        # a row without the field matches only $ne / $nin
        ({"year": {"$ne": 2001}}, lambda m: m.get("year") != 2001),
        ({"year": {"$eq": 2001}}, lambda m: m.get("year") == 2001),
        ({"nowhere": {"$ne": 1}}, lambda m: True),
        ({"nowhere": {"$nin": [1]}}, lambda m: True),
        ({"nowhere": 1}, lambda m: False),
        ({"nowhere": {"$lt": 1}}, lambda m: False),
        ({"nowhere": {"$in": [None]}}, lambda m: False),
        # two operators on a field, two fields in a dict: all have to hold
        ({"year": {"$gte": 2005, "$lt": 2010}}, lambda m: "year" in m and 2005 <= m["year"] < 2010),
        ({"album": "beach", "score": {"$lt": 0.5}}, lambda m: m["album"] == "beach" and m["score"] < 0.5),
        ({"$and": [{"album": "beach"}, {"score": {"$gte": 0.5}}]}, lambda m: m["album"] == "beach" and m["score"] >= 0.5),
        ({"$or": [{"album": "beach"}, {"year": 2003}]}, lambda m: m["album"] == "beach" or m.get("year") == 2003),
        ({"$and": [{"$or": [{"album": "city"}, {"album": "forest"}]}, {"year": {"$nin": [2000]}}]},
         lambda m: m["album"] in ("city", "forest") and m.get("year") != 2000),
        # values that do not compare do not match
        ({"album": {"$gt": 3}}, lambda m: False),
    ]
    for where, pred in cases:
        check_where(where)
        got = [r for r, m in enumerate(metas) if where_matches(m, where)]
        assert got == _rows_where(metas, pred), where
    assert 0 < len(_rows_where(metas, cases[3][1])) < N and any("year" not in m for m in metas)
    assert where_matches(None, {"a": {"$ne": 1}}) and not where_matches(None, {"a": 1})       # a row without metadata
    for bad in ({}, [], "album", {"album": {"$like": "c%"}}, {"$not": {"album": "city"}}, {"$and": []}, {"$or": {"album": "city"}},
                {"$and": [{"album": {"$regex": "x"}}]}, {"year": {"$in": 2001}}, {"year": {}}, {"year": [2001, 2002]}, {"$eq": 3}):
        with pytest.raises(ValueError):
            check_where(bad)


# ================================================================================================ FlatCollection
def test_ids_where_and_their_intersection(colmod):
    col, p, idx = _filled(colmod)
    q, metas = p["queries"], _metas()
    every = col.query(query_embeddings=q, n_results=5)
    n_other = idx.other_calls()
    # ids alone, shuffled, repeated, with unknown ones
    rows = list(range(10, 200, 3))
    ids = [_ids()[r] for r in rows[::-1]] + ["no-such-id", _ids()[10], "another"]
    got = col.query(query_embeddings=q, n_results=5, ids=ids)
    exp = sc.expected_subset(q, 5, np.asarray(rows), idx.rows, idx.labs)
    assert (got["ids"], got["distances"]) == _as_result(exp)
    assert idx.subset_calls[-1] == (4, 5, tuple(rows), None, None)                       # the list: known labels, once each
    assert got["metadatas"][0][0] == metas[int(exp[0][0, 0])] and got["included"] == ["metadatas", "documents", "distances"]
    # where alone
    where = {"$and": [{"album": "city"}, {"year": {"$gte": 2010}}]}
    wrows = _rows_where(metas, lambda m: m["album"] == "city" and m.get("year", 0) >= 2010)
    got = col.query(query_embeddings=q, n_results=5, where=where)
    assert (got["ids"], got["distances"]) == _as_result(sc.expected_subset(q, 5, np.asarray(wrows), idx.rows, idx.labs))
    assert idx.subset_calls[-1][2] == tuple(wrows)
    # both: the intersection
    both = sorted(set(rows) & set(wrows))
    assert 0 < len(both) < min(len(rows), len(wrows))
    got = col.query(query_embeddings=q, n_results=5, ids=ids, where=where)
    assert (got["ids"], got["distances"]) == _as_result(sc.expected_subset(q, 5, np.asarray(both), idx.rows, idx.labs))
    assert idx.subset_calls[-1][2] == tuple(both)
    # a single id as a string; every id: the flat answer; nothing but the subset call ran
    one = col.query(query_embeddings=q[:1], n_results=5, ids=_ids()[42])
    assert one["ids"] == [[_ids()[42]]]
    assert col.query(query_embeddings=q, n_results=5, ids=_ids()) == every
    assert idx.other_calls() == n_other
    # n_results above the list: what there is
    got = col.query(query_embeddings=q[:1], n_results=50, ids=_ids()[20:27])
    assert sorted(got["ids"][0]) == _ids()[20:27]
    with pytest.raises(ValueError):
        col.query(query_embeddings=q, n_results=5, where={"album": {"$like": "c%"}})
    # get(where=): the same evaluator, before offset and limit
    assert col.get(where=where)["ids"] == [_ids()[r] for r in wrows]
    assert col.get(ids=ids, where=where)["ids"] == [i for i in ids if i in {_ids()[r] for r in both}]
    assert col.get(where=where, offset=1, limit=2)["ids"] == [_ids()[r] for r in wrows[1:3]]
    with pytest.raises(ValueError):
        col.get(where={"$nor": []})


def test_filters_travel_as_masks(colmod):
    col, p, idx = _filled(colmod, filters=3)
    q = p["queries"]
    rows = list(range(0, 250))
    ids = [_ids()[r] for r in rows]
    got = col.query(query_embeddings=q, n_results=5, ids=ids, filters=["f0", "f2"])
    assert idx.subset_calls[-1] == (4, 5, tuple(rows), 0b101, None)
    tags = np.array([idx.tags.get(int(l), 0) for l in idx.labs], np.uint64)
    exp = sc.expected_subset(q, 5, np.asarray(rows), idx.rows, idx.labs, tags, np.uint64(0b101))
    assert (got["ids"], got["distances"]) == _as_result(exp)
    assert all(int(i[2:]) % 2 == 1 and int(i[2:]) < 250 for i in got["ids"][0])           # f0 and f2 say "yes" on odd rows
    # a name no row has ever answered admits nothing, without a call
    n = len(idx.subset_calls)
    assert col.query(query_embeddings=q, n_results=5, ids=ids, filters=["nobody"])["ids"] == [[], [], [], []]
    assert len(idx.subset_calls) == n


def test_a_65th_filter_name_is_folded_into_the_list_exactly(colmod):
    n = 2300                                            # more rows than one flat call ranks (2040): the old post-filter is inexact
    col, p, idx = _filled(colmod, n=n, filters=66)
    q = p["queries"][:1]
    col.query(query_embeddings=q, n_results=1, filters=["f0"])                            # (the tags are pushed: bits are dealt)
    assert "f65" in col._filter_overflow and "f63" in col._filter_bits
    # "yes" under f65 only on the 40 rows FARTHEST from the query: none of them is among the best 2040
    with np.errstate(all="ignore"):
        d = ro.distances(q, idx.rows)[0]
    far = np.argsort(np.nan_to_num(d, nan=-1.0))[-40:]
    for r in range(n):
        answers = json.loads(col._meta[r]["filter_results_json"])
        answers["f65"] = "yes" if r in set(far.tolist()) else "no"
        col._meta[r]["filter_results_json"] = json.dumps(answers)
    old = col.query(query_embeddings=q, n_results=5, filters=["f65"])
    assert old["ids"] == [[]]                                                              # the host post-filter of the best 2040
    got = col.query(query_embeddings=q, n_results=5, filters=["f65"], ids=_ids(n))
    exp = sc.expected_subset(q, 5, np.sort(far), idx.rows, idx.labs)
    assert (got["ids"], got["distances"]) == _as_result(exp, n) and len(got["ids"][0]) == 5
    assert idx.subset_calls[-1] == (1, 5, tuple(np.sort(far).tolist()), None, None)       # folded on the host, no mask
    # a mapped and an unmapped name together: the mapped one as a mask, the other in the list
    got = col.query(query_embeddings=q, n_results=5, filters=["f1", "f65"], where={"album": {"$ne": "nowhere"}})
    assert idx.subset_calls[-1][2:] == (tuple(np.sort(far).tolist()), 1 << col._filter_bits["f1"], None)
    tags = np.array([idx.tags.get(int(l), 0) for l in idx.labs], np.uint64)
    exp = sc.expected_subset(q, 5, np.sort(far), idx.rows, idx.labs, tags, np.uint64(1 << col._filter_bits["f1"]))
    assert (got["ids"], got["distances"]) == _as_result(exp, n) and 0 < len(got["ids"][0])
    # distinct_distance with a name past the 64th bit still raises without ids / where
    with pytest.raises(ValueError):
        col.query(query_embeddings=q, n_results=5, filters=["f65"], distinct_distance=0.01)


def test_max_distance_n_probe_distinct_and_the_empty_set(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"]
    rows = list(range(5, 290))
    ids = [_ids()[r] for r in rows]
    exp = sc.expected_subset(q, 20, np.asarray(rows), idx.rows, idx.labs)
    # max_distance: the sorted result cut at the radius — a prefix
    radius = float(exp[1][0, 7])
    got = col.query(query_embeddings=q, n_results=20, ids=ids, max_distance=radius)
    cut = ((exp[1] <= np.float32(radius)) & (np.arange(20)[None, :] < exp[2][:, None])).sum(1)
    assert (got["ids"], got["distances"]) == _as_result(exp, cut=cut) and 8 <= len(got["ids"][0]) < 20 and got["ids"][2] == []
    assert idx.radius_calls == []
    # n_probe is ignored, with a partition present too: the subset is exact
    plain = col.query(query_embeddings=q, n_results=20, ids=ids)
    assert col.query(query_embeddings=q, n_results=20, ids=ids, n_probe=1) == plain
    col.build_partition(7, iters=2)
    n_probed = len(idx.probed_calls)
    assert col.query(query_embeddings=q, n_results=20, ids=ids, n_probe=1) == plain and len(idx.probed_calls) == n_probed
    assert (plain["ids"], plain["distances"]) == _as_result(exp)
    with pytest.raises(ValueError, match="n_probe"):
        col.query(query_embeddings=q, n_results=20, ids=ids, n_probe=0)
    # distinct_distance together with ids / where raises
    n = len(idx.subset_calls)
    for kw in ({"ids": ids}, {"where": {"album": "city"}}, {"ids": ids, "where": {"album": "city"}}):
        with pytest.raises(ValueError, match="distinct_distance"):
            col.query(query_embeddings=q, n_results=5, distinct_distance=0.01, **kw)
    assert len(idx.subset_calls) == n and idx.distinct_calls == []
    # an empty admitted set gives empty results, without a call
    for kw in ({"ids": []}, {"ids": ["nobody"]}, {"where": {"album": "desert"}}, {"ids": ids, "where": {"score": {"$gt": 2.0}}}):
        got = col.query(query_embeddings=q, n_results=5, **kw)
        assert got["ids"] == [[], [], [], []] and got["distances"] == [[], [], [], []] and got["metadatas"] == [[], [], [], []], kw
    assert len(idx.subset_calls) == n
    # an empty collection
    assert colmod.FlatCollection("empty").query(query_embeddings=q, n_results=5, ids=ids)["ids"] == [[], [], [], []]


# ================================================================================================ search wrappers, routes
def test_search_wrappers_pass_the_list_through(colmod, monkeypatch):
    from mmiss_amd import search, utils

    col, p, idx = _filled(colmod)
    search.set_collection(col)
    monkeypatch.setattr(utils, "load_clip_model", lambda: (None, None))
    monkeypatch.setattr(utils, "generate_clip_embedding",
                        lambda image=None, text=None, model=None, processor=None: {"text": p["queries"][:1], "image": p["queries"][1:2]})
    monkeypatch.setattr(search, "blend", lambda a, b, w: np.asarray(a, np.float32))
    rows = list(range(100, 160))
    ids = [_ids()[r] for r in rows]
    where = {"album": "forest"}
    wrows = [r for r in rows if r % 3 == 2]
    try:
        got = search.search_similar(p["queries"][0], limit=5, within_ids=ids)
        exp = sc.expected_subset(p["queries"][:1], 5, np.asarray(rows), idx.rows, idx.labs)
        assert [r["id"] for r in got] == _as_result(exp)[0][0] and idx.subset_calls[-1] == (1, 5, tuple(rows), None, None)
        assert got[0]["similarity_score"] == 1 - float(exp[1][0, 0]) / 2
        assert len(search.search_similar_batch(p["queries"][:3], limit=4, within_ids=ids, where=where)) == 3
        assert idx.subset_calls[-1] == (3, 4, tuple(wrows), None, None)
        search.search_by_text("a cat", limit=5, where=where, filters=["f0"])
        assert idx.subset_calls[-1] == (1, 5, tuple(r for r in range(N) if r % 3 == 2), 1, None)
        search.search_multimodal(None, "a cat", 0.5, limit=6, within_ids=ids, n_probe=3)
        assert idx.subset_calls[-1] == (1, 6, tuple(rows), None, None)
        search.search_multimodal_batch(p["queries"][:2], p["queries"][:2], 0.5, limit=7, within_ids=ids[:9], min_similarity=0.1)
        assert idx.subset_calls[-1] == (2, 7, tuple(rows[:9]), None, None)
        n = len(idx.subset_calls)
        assert search.search_similar(p["queries"][0], limit=5, within_ids=ids, distinct_similarity=0.99) == []   # (logged, [])
        assert search.search_similar(p["queries"][0], limit=5, where={"album": {"$like": "x"}}) == []
        assert len(idx.subset_calls) == n
    finally:
        search.set_collection(None)


@pytest.fixture()
def tiny(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils

    OracleSubsetIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleSubsetIndex)
    monkeypatch.setattr(search, "blend", lambda i, t, w: ro.blend(i, t, w))
    utils.set_clip_model(OracleEncoder(co.TINY), _Proc(co.TINY))
    search.set_collection(collection.FlatCollection("t"))
    yield search, utils
    utils.set_clip_model(None, None)
    search.set_collection(None)


def test_api_routes_take_the_ids_field(tiny):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from starlette.testclient import TestClient
    from mmiss_amd import api

    search, utils = tiny
    imgs = [_image(i) for i in range(5)]
    emb = [np.asarray(utils.generate_clip_embedding(image=im)["image"][0], np.float32) for im in imgs]
    ids = ["a", "b", "c", "d", "e"]
    search._collection().add(ids=ids, embeddings=np.stack(emb), metadatas=[{"id": i} for i in ids])
    index = OracleSubsetIndex.instances[-1]
    client = TestClient(api.create_app())
    q = {"file": ("q.png", _png(imgs[2]), "image/png")}
    plain = client.post("/api/search/image", files=q, data={"limit": "2"})
    assert plain.status_code == 200 and plain.json()["results"][0]["id"] == "c" and index.subset_calls == []   # absent: today's call
    r = client.post("/api/search/image", files=q, data={"limit": "2", "ids": "a, e,zzz,a"})
    assert r.status_code == 200 and {x["id"] for x in r.json()["results"]} == {"a", "e"}                       # the nearest row is outside
    assert index.subset_calls[-1][:3] == (1, 2, (0, 4))
    t = client.post("/api/search/text", data={"query": "red drill", "limit": "3", "ids": "b,d"})
    assert t.status_code == 200 and {x["id"] for x in t.json()["results"]} == {"b", "d"} and index.subset_calls[-1][2] == (1, 3)
    m = client.post("/api/search/multimodal", files=q, data={"query": "drill", "weight_image": "1.0", "limit": "1", "ids": "c,d",
                                                              "prefilter": "1"})
    assert m.status_code == 200 and [x["id"] for x in m.json()["results"]] == ["c"] and index.subset_calls[-1][2] == (2, 3)
    none = client.post("/api/search/image", files=q, data={"limit": "2", "ids": "zzz"})
    assert none.status_code == 200 and none.json()["results"] == []
    n = len(index.subset_calls)
    for bad in ("", " ", "a,,b", "a,", ",a"):
        for route, kw in (("/api/search/image", dict(files=q, data={"limit": "3", "ids": bad})),
                          ("/api/search/text", dict(data={"query": "x", "limit": "3", "ids": bad})),
                          ("/api/search/multimodal", dict(files=q, data={"query": "x", "limit": "3", "ids": bad}))):
            r = client.post(route, **kw)
            assert r.status_code == 500 and r.json()["success"] is False, (route, bad)
    assert len(index.subset_calls) == n
    # ... as a bad limit is answered
    r = client.post("/api/search/text", data={"query": "x", "limit": "many"})
    assert r.status_code == 500 and r.json()["success"] is False


# ================================================================================================ nothing changes without them
class _RefusingSubsetIndex(OracleSubsetIndex):
    """the stand-in with a query_subset that must not be reached"""
    reached = []

    def query_subset(self, *a, **kw):
        _RefusingSubsetIndex.reached.append((a, kw))
        raise AssertionError("a call without ids / where reached query_subset")


def test_a_call_without_the_new_keywords_never_reaches_query_subset(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils

    _RefusingSubsetIndex.reached = []
    monkeypatch.setattr(collection, "FlatIndex", _RefusingSubsetIndex)
    col, p, idx = _filled(collection, filters=66)
    idx = _RefusingSubsetIndex.instances[-1]
    q = p["queries"]
    col.build_partition(7, iters=2)
    calls = [dict(), dict(filters=["f0"]), dict(filters=["f0", "f65"]), dict(filters=["f65"], max_distance=0.5), dict(max_distance=0.4),
             dict(n_probe=2), dict(n_probe=2, filters=["f1"]), dict(distinct_distance=0.01), dict(distinct_distance=0.01, pool=100, n_probe=1),
             dict(distinct_distance=0.01, filters=["f2"], max_distance=0.9), dict(ids=None, where=None)]
    for kw in calls:
        got = col.query(query_embeddings=q, n_results=5, **kw)
        assert len(got["ids"]) == 4, kw
    kinds = (idx.flat_calls, len(idx.probed_calls), len(idx.distinct_calls), len(idx.radius_calls))
    assert all(kinds), kinds                                              # every older route was taken ...
    search.set_collection(col)
    monkeypatch.setattr(utils, "load_clip_model", lambda: (None, None))
    monkeypatch.setattr(utils, "generate_clip_embedding",
                        lambda image=None, text=None, model=None, processor=None: {"text": q[:1], "image": q[1:2]})
    monkeypatch.setattr(search, "blend", lambda a, b, w: np.asarray(a, np.float32))
    try:
        assert len(search.search_similar(q[0], limit=5)) == 5
        assert len(search.search_similar_batch(q[:2], limit=5, filters=["f0"])) == 2
        assert len(search.search_by_text("a cat", limit=5, n_probe=2)) == 5
        assert len(search.search_multimodal(None, "a cat", 0.5, limit=5, distinct_similarity=0.99)) == 5
        assert len(search.search_multimodal_batch(q[:2], q[:2], 0.5, limit=5, min_similarity=0.1)) == 2
    finally:
        search.set_collection(None)
    col.get(ids=_ids()[:3])
    col.get(limit=2)
    assert _RefusingSubsetIndex.reached == [] and idx.subset_calls == []  # ... and none of them is the new one
    with pytest.raises(AssertionError):                                   # (the stand-in does refuse when it is reached)
        col.query(query_embeddings=q, n_results=5, ids=_ids()[:3])
    assert len(_RefusingSubsetIndex.reached) == 1


# ================================================================================================ FlatIndex.query_subset
def test_wrapper_argument_checks_come_before_the_call():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.index import FlatIndex

    idx = FlatIndex.__new__(FlatIndex)               # no device here: the checks under test run before any library call
    idx.dim, idx.dtype, idx.device, idx._h, idx._lib, idx._call_lock = D, 0, 0, None, _NoLibrary(), threading.RLock()
    q = np.zeros((2, D), np.float32)
    lab = np.arange(5, dtype=np.int64)
    with pytest.raises(ValueError, match="k"):
        idx.query_subset(q, 0, lab)
    with pytest.raises(ValueError, match="k"):
        idx.query_subset(q, 2041, lab)
    with pytest.raises(TypeError, match="labels"):
        idx.query_subset(q, 10, lab.astype(np.float32))
    with pytest.raises(TypeError, match="labels"):
        idx.query_subset(q, 10, ["a", "b"])
    with pytest.raises(ValueError, match="vectors"):
        idx.query_subset(np.zeros((2, D + 1), np.float32), 10, lab)
    with pytest.raises(ValueError, match="query"):
        idx.query_subset(np.zeros((0, D), np.float32), 10, lab)
    with pytest.raises(ValueError, match="require"):
        idx.query_subset(q, 10, lab, require=np.zeros(3, np.uint64))
    with pytest.raises(TypeError, match="exclude"):
        idx.query_subset(q, 10, lab, exclude=1.5)
    idx._h = None                                    # (nothing to destroy)

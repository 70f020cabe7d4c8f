"""The host layers of distinct results without a GPU, on the oracle-backed stand-in of tests/distinct_fakes.py:
FlatCollection.query(distinct_distance=, pool=) — the default pool, the one retry at the largest pool, the radius cut, filters (and
the refusal past 64 names), n_probe, "duplicates" only when asked for —, the search wrappers and the three API routes that pass
distinct_similarity through, and the argument checks FlatIndex.query_distinct makes before it calls the library."""
import json
import threading

import numpy as np
import pytest

import distinct_cases as dc
from distinct_fakes import OracleDistinctIndex
from fakes import OracleEncoder
from oracle import clip_oracle as co
from oracle import retrieval_oracle as ro
from test_partition_layers_cpu import _NoLibrary
from test_radius_layers_cpu import _Proc, _image, _png

N, D = 300, 128


@pytest.fixture()
def colmod(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection

    OracleDistinctIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleDistinctIndex)
    return collection


def _ids(n=N):
    return [f"im{i:03d}" for i in range(n)]


def _filled(colmod, filters=1):
    c = dc.corpus(N)
    col = colmod.FlatCollection("t")
    metas = [{"id": i, "filter_results_json": json.dumps({f"f{j}": "yes" if (r + j) % 2 else "no" for j in range(filters)})}
             for r, i in enumerate(_ids())]
    col.add(ids=_ids(), embeddings=c.rows, metadatas=metas)          # (labels 0 .. N-1: label == row)
    return col, c, OracleDistinctIndex.instances[-1]


def _expect(idx, q, k, pool, min_sep=dc.MIN_SEP, **kw):
    return dc.expected_distinct(q, k, pool, min_sep, idx.rows, idx.labs, **kw)


def _as_result(exp, cut=None):
    cnt = exp[2] if cut is None else cut
    return ([[_ids()[int(l)] for l in exp[0][i, :cnt[i]]] for i in range(len(cnt))],
            [[float(d) for d in exp[1][i, :cnt[i]]] for i in range(len(cnt))],
            [[int(u) for u in exp[3][i, :cnt[i]]] for i in range(len(cnt))])


def test_default_pool_and_the_one_retry(colmod):
    col, c, idx = _filled(colmod)
    sep = float(dc.MIN_SEP)
    q = c.queries[[dc.Q_BURSTS]]
    got = col.query(query_embeddings=q, n_results=3, distinct_distance=sep)
    assert idx.distinct_calls == [(1, 3, sep, 64, 0, False)]                              # min(2040, max(8 k, 64)), no retry
    ids, dist, dups = _as_result(_expect(idx, q, 3, 64))
    assert (got["ids"], got["distances"], got["duplicates"]) == (ids, dist, dups) and dups == [[9, 9, 9]]
    col.query(query_embeddings=q, n_results=40, distinct_distance=sep)
    assert idx.distinct_calls[-1][3] == 320 and len(idx.distinct_calls) == 2
    # the big group exhausts the default pool: repeated once, at 2040
    q = c.queries[[dc.Q_BIG]]
    del idx.distinct_calls[:]
    got = col.query(query_embeddings=q, n_results=3, distinct_distance=sep)
    assert [x[3] for x in idx.distinct_calls] == [64, 2040]
    exp = _expect(idx, q, 3, 2040)
    assert exp[2][0] == 3 and (got["ids"], got["distances"], got["duplicates"]) == _as_result(exp)
    # an explicit pool: taken as given (at least k, at most 2040), retried the same way; a batch is repeated as a whole
    del idx.distinct_calls[:]
    both = c.queries[[dc.Q_BURSTS, dc.Q_BIG]]
    got = col.query(query_embeddings=both, n_results=3, distinct_distance=sep, pool=30)
    assert [(x[0], x[3]) for x in idx.distinct_calls] == [(2, 30), (2, 2040)]
    assert (got["ids"], got["distances"], got["duplicates"]) == _as_result(_expect(idx, both, 3, 2040))
    del idx.distinct_calls[:]
    col.query(query_embeddings=q, n_results=3, distinct_distance=sep, pool=5000)
    col.query(query_embeddings=q, n_results=3, distinct_distance=sep, pool=1)
    assert [x[3] for x in idx.distinct_calls] == [2040, 3, 2040]
    # an exhausted pool that cannot grow is not repeated: fewer than n_results distinct images exist
    del idx.distinct_calls[:]
    got = col.query(query_embeddings=q, n_results=3, distinct_distance=4.0, pool=2040)
    assert len(idx.distinct_calls) == 1 and len(got["ids"][0]) == 1 and got["duplicates"] == [[N - 3]]


def test_radius_cut_is_a_prefix_of_the_kept_list(colmod):
    col, c, idx = _filled(colmod)
    q = c.queries[[dc.Q_BURSTS]]
    full = col.query(query_embeddings=q, n_results=5, distinct_distance=float(dc.MIN_SEP))
    d = full["distances"][0]
    assert d[1] < 0.17 < d[2]
    got = col.query(query_embeddings=q, n_results=5, distinct_distance=float(dc.MIN_SEP), max_distance=0.17)
    assert got["ids"][0] == full["ids"][0][:2] and got["distances"][0] == d[:2] and got["duplicates"][0] == full["duplicates"][0][:2]
    assert idx.radius_calls == []                                                         # the cut is made on the host
    at = col.query(query_embeddings=q, n_results=5, distinct_distance=float(dc.MIN_SEP), max_distance=d[2])
    assert len(at["ids"][0]) == 3                                                          # <= as floats
    assert col.query(query_embeddings=q, n_results=5, distinct_distance=float(dc.MIN_SEP), max_distance=-1.0)["ids"] == [[]]


def test_filters_and_the_refusal_past_64_names(colmod):
    col, c, idx = _filled(colmod, filters=66)
    q = c.queries[[dc.Q_BURSTS]]
    got = col.query(query_embeddings=q, n_results=3, distinct_distance=float(dc.MIN_SEP), filters=["f3"])
    assert idx.distinct_calls[-1][5] is True
    tags = np.array([idx.tags.get(int(l), 0) for l in idx.labs], np.uint64)
    exp = _expect(idx, q, 3, 64, tags=tags, require=np.uint64(1 << 3))
    assert (got["ids"], got["distances"], got["duplicates"]) == _as_result(exp)
    assert all((int(i[2:]) + 3) % 2 for i in got["ids"][0])
    n = len(idx.distinct_calls)
    with pytest.raises(ValueError, match="64"):
        col.query(query_embeddings=q, n_results=3, distinct_distance=float(dc.MIN_SEP), filters=["f65"])
    with pytest.raises(ValueError, match="64"):
        col.query(query_embeddings=q, n_results=3, distinct_distance=float(dc.MIN_SEP), filters=["f3", "f64"])
    assert len(idx.distinct_calls) == n
    assert len(col.query(query_embeddings=q, n_results=3, filters=["f65"])["ids"][0]) == 3        # without it: as before
    got = col.query(query_embeddings=q, n_results=3, distinct_distance=float(dc.MIN_SEP), filters=["no such filter"])
    assert got["ids"] == [[]] and got["duplicates"] == [[]]
    with pytest.raises(ValueError, match="NaN"):
        col.query(query_embeddings=q, n_results=3, distinct_distance=float("nan"))


def test_duplicates_only_when_asked_for_and_nothing_else_changes(colmod):
    col, c, idx = _filled(colmod)
    q = c.queries[:7]
    plain = col.query(query_embeddings=q, n_results=10)
    assert "duplicates" not in plain and idx.distinct_calls == []
    assert "duplicates" not in col.query(query_embeddings=q, n_results=10, pool=100)          # pool alone is ignored
    assert "duplicates" not in col.query(query_embeddings=q, n_results=10, max_distance=0.5, filters=["f0"])
    assert idx.distinct_calls == []
    got = col.query(query_embeddings=q, n_results=10, distinct_distance=-1.0)                 # nothing suppressed: the plain ranking
    dups = got.pop("duplicates")
    assert got == plain and dups == [[0] * 10] * 7
    empty = colmod.FlatCollection("empty").query(query_embeddings=q, n_results=3, distinct_distance=0.01)
    assert empty["ids"] == [[]] * 7 and empty["duplicates"] == [[]] * 7


def test_n_probe_goes_to_the_probed_list(colmod):
    col, c, idx = _filled(colmod)
    q = c.queries[[dc.Q_BURSTS, dc.Q_CHAIN]]
    sep = float(dc.MIN_SEP)
    col.query(query_embeddings=q, n_results=3, distinct_distance=sep, n_probe=2)
    assert idx.distinct_calls[-1][4] == 0                                                 # no partition: the flat list, never an error
    col.build_partition(5, iters=2)
    got = col.query(query_embeddings=q, n_results=3, distinct_distance=sep, n_probe=2)
    assert idx.distinct_calls[-1][4] == 2 and idx.probed_calls == []
    part = dict(nprobe=2, centres=idx.part["centres"], cells=idx.part["cells"], B=N)
    assert (got["ids"], got["distances"], got["duplicates"]) == _as_result(_expect(idx, q, 3, 64, partition=part))
    every = col.query(query_embeddings=q, n_results=3, distinct_distance=sep, n_probe=5)
    assert every == col.query(query_embeddings=q, n_results=3, distinct_distance=sep)       # every cell probed: the flat result


def test_search_wrappers_pass_distinct_similarity_through(colmod, monkeypatch):
    from mmiss_amd import search, utils

    col, c, idx = _filled(colmod)
    search.set_collection(col)
    monkeypatch.setattr(utils, "load_clip_model", lambda: (None, None))
    monkeypatch.setattr(utils, "generate_clip_embedding",
                        lambda image=None, text=None, model=None, processor=None: {"text": c.queries[:1], "image": c.queries[1:2]})
    monkeypatch.setattr(search, "blend", lambda a, b, w: np.asarray(a, np.float32))
    s = 0.995
    sep = float(utils.max_distance_for_similarity(s))
    assert 0.0099 < sep < 0.0101
    try:
        plain = search.search_similar(c.queries[0], limit=3)
        assert idx.distinct_calls == [] and all("duplicates" not in r for r in plain)
        got = search.search_similar(c.queries[0], limit=3, distinct_similarity=s)
        assert idx.distinct_calls[-1] == (1, 3, sep, 64, 0, False)
        assert [r["duplicates"] for r in got] == [9, 9, 9] and [r["id"] for r in got] != [r["id"] for r in plain]
        assert got[0]["id"] == plain[0]["id"] and got[0]["similarity_score"] == plain[0]["similarity_score"]
        batch = search.search_similar_batch(c.queries[:2], limit=4, distinct_similarity=s)
        assert idx.distinct_calls[-1][:4] == (2, 4, sep, 64) and [len(b) for b in batch] == [4, 4] and batch[1][0]["duplicates"] == 1
        search.search_by_text("a cat", limit=5, distinct_similarity=s)
        assert idx.distinct_calls[-1][:3] == (1, 5, sep)
        search.search_multimodal(None, "a cat", 0.5, limit=5, distinct_similarity=s, filters=["f0"])
        assert idx.distinct_calls[-1] == (1, 5, sep, 64, 0, True)
        search.search_multimodal_batch(c.queries[:2], c.queries[:2], 0.5, limit=6, distinct_similarity=s, min_similarity=0.5)
        assert idx.distinct_calls[-1][:3] == (2, 6, sep)
        n = len(idx.distinct_calls)
        assert search.search_similar(c.queries[0], limit=3, distinct_similarity=float("nan")) == []   # (the wrappers log and return [])
        assert len(idx.distinct_calls) == n
    finally:
        search.set_collection(None)


@pytest.fixture()
def tiny(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils

    OracleDistinctIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleDistinctIndex)
    monkeypatch.setattr(search, "blend", lambda i, t, w: ro.blend(i, t, w))
    utils.set_clip_model(OracleEncoder(co.TINY), _Proc(co.TINY))
    search.set_collection(collection.FlatCollection("t"))
    yield search, utils
    utils.set_clip_model(None, None)
    search.set_collection(None)


def test_api_routes_take_the_field(tiny):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from starlette.testclient import TestClient
    from mmiss_amd import api

    search, utils = tiny
    imgs = [_image(i) for i in range(4)]
    emb = [np.asarray(utils.generate_clip_embedding(image=im)["image"][0], np.float32) for im in imgs]
    # image 2 is stored three times (a burst), the others once
    rows = [emb[0], emb[1], emb[2], emb[2], emb[2], emb[3]]
    ids = ["a", "b", "c0", "c1", "c2", "d"]
    search._collection().add(ids=ids, embeddings=np.stack(rows), metadatas=[{"id": i} for i in ids])
    index = OracleDistinctIndex.instances[-1]
    client = TestClient(api.create_app())
    q = {"file": ("q.png", _png(imgs[2]), "image/png")}
    plain = client.post("/api/search/image", files=q, data={"limit": "3"})
    assert plain.status_code == 200 and [r["id"] for r in plain.json()["results"]] == ["c0", "c1", "c2"]
    assert index.distinct_calls == [] and all("duplicates" not in r for r in plain.json()["results"])   # absent: today's call
    r = client.post("/api/search/image", files=q, data={"limit": "3", "distinct_similarity": "0.98"})
    assert r.status_code == 200 and len(index.distinct_calls) == 1
    res = r.json()["results"]
    assert len(res) == 3 and res[0]["id"] == "c0" and res[0]["duplicates"] == 2 and not {"c1", "c2"} & {x["id"] for x in res}
    assert index.distinct_calls[-1][2] == float(utils.max_distance_for_similarity(0.98))
    t = client.post("/api/search/text", data={"query": "red drill", "limit": "2", "distinct_similarity": "0.98"})
    assert t.status_code == 200 and len(index.distinct_calls) == 2 and all("duplicates" in x for x in t.json()["results"])
    m = client.post("/api/search/multimodal", files=q, data={"query": "drill", "weight_image": "1.0", "limit": "2", "distinct_similarity": "0.98",
                                                              "min_similarity": "0.5"})
    assert m.status_code == 200 and len(index.distinct_calls) == 3 and m.json()["results"][0]["id"] == "c0"
    p = client.post("/api/search/image", files=q, data={"limit": "2", "distinct_similarity": "1", "prefilter": "1"})
    assert p.status_code == 200 and len(index.distinct_calls) == 4
    for bad in ("1.5", "-0.1", "nan", "high"):
        for route, kw in (("/api/search/image", dict(files=q, data={"limit": "3", "distinct_similarity": bad})),
                          ("/api/search/text", dict(data={"query": "x", "limit": "3", "distinct_similarity": bad})),
                          ("/api/search/multimodal", dict(files=q, data={"query": "x", "limit": "3", "distinct_similarity": bad}))):
            r = client.post(route, **kw)
            assert r.status_code == 500 and r.json()["success"] is False, (route, bad)
    assert len(index.distinct_calls) == 4


def test_wrapper_argument_checks_come_before_the_call():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.index import FlatIndex, default_distinct_pool

    assert [default_distinct_pool(k) for k in (1, 8, 9, 10, 255, 256, 2040)] == [64, 64, 72, 80, 2040, 2040, 2040]
    idx = FlatIndex.__new__(FlatIndex)               # no device here: the checks under test run before any library call
    idx.dim, idx.dtype, idx.device, idx._h, idx._lib, idx._call_lock = D, 0, 0, None, _NoLibrary(), threading.RLock()
    q = np.zeros((2, D), np.float32)
    with pytest.raises(ValueError, match="k"):
        idx.query_distinct(q, 0, 0.01)
    with pytest.raises(ValueError, match="pool"):
        idx.query_distinct(q, 10, 0.01, pool=9)
    with pytest.raises(ValueError, match="pool"):
        idx.query_distinct(q, 10, 0.01, pool=2041)
    with pytest.raises(ValueError, match="pool"):
        idx.query_distinct(q, 2041, 0.01)
    with pytest.raises(ValueError, match="NaN"):
        idx.query_distinct(q, 10, float("nan"))
    with pytest.raises(ValueError, match="nprobe"):
        idx.query_distinct(q, 10, 0.01, nprobe=-1)
    with pytest.raises(ValueError, match="vectors"):
        idx.query_distinct(np.zeros((2, D + 1), np.float32), 10, 0.01)
    with pytest.raises(ValueError, match="require"):
        idx.query_distinct(q, 10, 0.01, require=np.zeros(3, np.uint64))
    idx._h = None                                    # (nothing to destroy)

"""The host layers of grouped search without a GPU, on the oracle-backed stand-in of tests/grouped_fakes.py:
FlatCollection.query(group_by=) — the field's values mapped to dense ids in order of first appearance by label, pushed lazily,
every refused combination, the radius cut, "groups" / "group_sizes", and the record that a call without group_by never reaches
query_grouped —, the search wrappers and the three API routes that pass group_by through, and the argument checks
FlatIndex.set_groups / query_grouped make before they call the library."""
import json
import threading

import numpy as np
import pytest

import grouped_cases as gc
from fakes import OracleEncoder
from grouped_fakes import OracleGroupedIndex
from oracle import clip_oracle as co
from oracle import retrieval_oracle as ro
from test_partition_layers_cpu import _NoLibrary
from test_radius_layers_cpu import _Proc, _image, _png

N, D, FOLDERS = 300, 128, 7


@pytest.fixture()
def colmod(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection

    OracleGroupedIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleGroupedIndex)
    return collection


def _ids(n=N):
    return [f"im{i:03d}" for i in range(n)]


def _folder(r):
    """every fifth row has no folder"""
    return None if r % 5 == 0 else f"dir{r % FOLDERS}"


def _metas(n=N, filters=1):
    out = []
    for r, i in enumerate(_ids(n)):
        m = {"id": i, "batch": r // 100, "filter_results_json": json.dumps({f"f{j}": "yes" if (r + j) % 2 else "no" for j in range(filters)})}
        if _folder(r) is not None:
            m["folder"] = _folder(r)
        out.append(m)
    return out


def _dense_ids(values):
    """values (None: no field) in label order -> dense ids in order of first appearance, -1 without the field"""
    seen = {}
    return np.array([-1 if v is None else seen.setdefault(v, len(seen)) for v in values], np.int32)


def _filled(colmod, filters=1):
    p = gc.corpus(51, N, D, 6)
    col = colmod.FlatCollection("t")
    col.add(ids=_ids(), embeddings=p["x"], metadatas=_metas(N, filters))      # (labels 0 .. N-1: label == row)
    return col, p, OracleGroupedIndex.instances[-1]


def _as_result(exp, cut=None):
    cnt = exp[3] if cut is None else cut
    return ([[_ids()[int(l)] for l in exp[0][i, :cnt[i]]] for i in range(len(cnt))],
            [[float(d) for d in exp[1][i, :cnt[i]]] for i in range(len(cnt))])


def test_values_become_dense_ids_and_are_pushed_lazily(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"][:4]
    assert idx.group_pushes == []                                                          # nothing before the first grouped query
    col.query(query_embeddings=q, n_results=5, group_by="folder")
    want = _dense_ids([_folder(r) for r in range(N)])
    assert idx.group_pushes == [tuple(range(N))] and np.array_equal(idx.get_groups(np.arange(N)), want)
    assert want[:8].tolist() == [-1, 0, 1, 2, 3, -1, 4, 5] and want.max() == FOLDERS - 1
    col.query(query_embeddings=q, n_results=5, group_by="folder")
    assert len(idx.group_pushes) == 1                                                      # nothing dirty: nothing pushed
    # added rows: only they are pushed, a new value takes the next id, a known one keeps its own
    col.add(ids=["new0", "new1", "new2"], embeddings=p["x"][:3] * 2, metadatas=[{"id": "new0", "folder": "fresh"}, {"id": "new1"}, {"id": "new2", "folder": "dir3"}])
    col.query(query_embeddings=q, n_results=5, group_by="folder")
    assert idx.group_pushes[-1] == (N, N + 1, N + 2) and idx.get_groups([N, N + 1, N + 2]).tolist() == [FOLDERS, -1, 2]
    # a metadata update: that label alone; a document update: nothing
    col.update(ids=["im005"], metadatas=[{"folder": "fresh"}])
    col.update(ids=["im006"], documents=["text"])
    col.query(query_embeddings=q, n_results=5, group_by="folder")
    assert idx.group_pushes[-1] == (5,) and len(idx.group_pushes) == 3 and idx.get_groups([5]).tolist() == [FOLDERS]
    # a deleted row is not pushed again
    col.update(ids=["im007"], metadatas=[{"folder": "dir1"}])
    col.delete(ids=["im007"])
    col.query(query_embeddings=q, n_results=5, group_by="folder")
    assert len(idx.group_pushes) == 3
    # another field: every stored label again, ids afresh
    col.query(query_embeddings=q, n_results=5, group_by="batch")
    stored = [l for l in range(N + 3) if l != 7]
    assert idx.group_pushes[-1] == tuple(stored)
    assert idx.get_groups([0, 99, 100, 299, N, N + 1]).tolist() == [0, 0, 1, 2, -1, -1]
    col.query(query_embeddings=q, n_results=5, group_by="folder")                           # ... and back
    assert idx.group_pushes[-1] == tuple(stored) and idx.get_groups([1, 5, N]).tolist() == [0, 4, 4]   # 'fresh' now first appears at label 5, behind dir1 .. dir4


def test_results_groups_and_group_sizes(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"]
    k = 12
    got = col.query(query_embeddings=q, n_results=k, group_by="folder")
    assert idx.grouped_calls == [(6, k, None, None)]
    groups = _dense_ids([_folder(r) for r in range(N)])
    exp = gc.expected_grouped(q, k, idx.rows, idx.labs, groups)
    assert (got["ids"], got["distances"]) == _as_result(exp) and got["ids"][2] == []         # the query without a direction
    sizes = {}
    for r in range(N):
        sizes[_folder(r)] = sizes.get(_folder(r), 0) + 1
    for qi in (0, 1, 3, 4, 5):
        rows = [int(i[2:]) for i in got["ids"][qi]]
        assert got["groups"][qi] == [_folder(r) for r in rows]
        assert got["group_sizes"][qi] == [1 if _folder(r) is None else sizes[_folder(r)] for r in rows]
        named = [g for g in got["groups"][qi] if g is not None]
        assert len(named) == len(set(named)) >= 3 and None in got["groups"][qi]             # one hit per folder, ungrouped rows between
        assert [m.get("folder") for m in got["metadatas"][qi]] == got["groups"][qi]
    # group sizes follow the collection
    col.delete(ids=[got["ids"][0][0]])
    again = col.query(query_embeddings=q[:1], n_results=k, group_by="folder")
    first = got["groups"][0][0]
    if first is not None:
        every = col.query(query_embeddings=q[:1], n_results=N, group_by="folder")             # every group there is
        assert every["group_sizes"][0][every["groups"][0].index(first)] == sizes[first] - 1
    # pool travels, clamped to k .. 2040, and never changes the result
    for pool, sent in ((30, 30), (1, k), (5000, 2040)):
        g2 = col.query(query_embeddings=q[:1], n_results=k, group_by="folder", pool=pool)
        assert idx.grouped_calls[-1] == (1, k, sent, None) and g2 == again


def test_filters_travel_as_masks_and_the_refusal_past_64_names(colmod):
    col, p, idx = _filled(colmod, filters=66)
    q = p["queries"][:2]
    got = col.query(query_embeddings=q, n_results=4, group_by="folder", filters=["f3"])
    assert idx.grouped_calls[-1] == (2, 4, None, 1 << 3)
    tags = np.array([idx.tags.get(int(l), 0) for l in idx.labs], np.uint64)
    exp = gc.expected_grouped(q, 4, idx.rows, idx.labs, _dense_ids([_folder(r) for r in range(N)]), tags, require=np.uint64(1 << 3))
    assert (got["ids"], got["distances"]) == _as_result(exp) and all((int(i[2:]) + 3) % 2 for i in got["ids"][0])
    n = len(idx.grouped_calls)
    with pytest.raises(ValueError, match="64"):
        col.query(query_embeddings=q, n_results=4, group_by="folder", filters=["f65"])
    with pytest.raises(ValueError, match="64"):
        col.query(query_embeddings=q, n_results=4, group_by="folder", filters=["f3", "f64"])
    assert len(idx.grouped_calls) == n
    got = col.query(query_embeddings=q, n_results=4, group_by="folder", filters=["no such filter"])
    assert got["ids"] == [[], []] and got["groups"] == [[], []] and got["group_sizes"] == [[], []]


def test_every_refused_combination(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"][:1]
    for kw in ({"ids": ["im001"]}, {"where": {"batch": 1}}, {"after": [None]}, {"distinct_distance": 0.01}, {"n_probe": 2}):
        with pytest.raises(ValueError, match="group_by"):
            col.query(query_embeddings=q, n_results=3, group_by="folder", **kw)
    for bad in ("", 7, ["folder"]):
        with pytest.raises(ValueError, match="group_by"):
            col.query(query_embeddings=q, n_results=3, group_by=bad)
    assert idx.grouped_calls == [] and idx.group_pushes == [] and idx.other_calls() == 0


def test_radius_cut_is_a_prefix_of_the_heads(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"][:1]
    full = col.query(query_embeddings=q, n_results=8, group_by="folder")
    d = full["distances"][0]
    cut = (d[2] + d[3]) / 2
    assert d[2] < cut < d[3]
    got = col.query(query_embeddings=q, n_results=8, group_by="folder", max_distance=cut)
    assert got["ids"][0] == full["ids"][0][:3] and got["distances"][0] == d[:3] and got["groups"][0] == full["groups"][0][:3]
    assert got["group_sizes"][0] == full["group_sizes"][0][:3] and idx.radius_calls == []   # the cut is made on the host
    assert len(col.query(query_embeddings=q, n_results=8, group_by="folder", max_distance=d[3])["ids"][0]) == 4   # <= as floats
    assert col.query(query_embeddings=q, n_results=8, group_by="folder", max_distance=-1.0)["ids"] == [[]]


def test_without_group_by_nothing_reaches_the_grouped_call(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"]
    plain = col.query(query_embeddings=q, n_results=10)
    assert "groups" not in plain and "group_sizes" not in plain
    col.query(query_embeddings=q, n_results=10, filters=["f0"], max_distance=0.9)
    col.query(query_embeddings=q, n_results=10, distinct_distance=0.01, pool=100)
    col.query(query_embeddings=q, n_results=10, ids=_ids()[:50])
    col.query(query_embeddings=q, n_results=10, after=[None] * 6)
    assert idx.grouped_calls == [] and idx.group_pushes == [] and idx.groups == {}
    calls = idx.other_calls()
    col.query(query_embeddings=q, n_results=10, group_by="folder")
    assert len(idx.grouped_calls) == 1 and idx.other_calls() == calls                       # ... and the grouped query is ONE index call
    # every row ungrouped (a field no row has): the plain ranking
    none = col.query(query_embeddings=q, n_results=10, group_by="no such field")
    assert none["groups"] == [[None] * len(r) for r in plain["ids"]] and none["group_sizes"] == [[1] * len(r) for r in plain["ids"]]
    del none["groups"], none["group_sizes"]
    assert none == plain
    empty = colmod.FlatCollection("empty").query(query_embeddings=q, n_results=3, group_by="folder")
    assert empty["ids"] == [[]] * 6 and empty["groups"] == [[]] * 6 and empty["group_sizes"] == [[]] * 6


def test_search_wrappers_pass_group_by_through(colmod, monkeypatch):
    from mmiss_amd import search, utils

    col, p, idx = _filled(colmod)
    search.set_collection(col)
    monkeypatch.setattr(utils, "load_clip_model", lambda: (None, None))
    monkeypatch.setattr(utils, "generate_clip_embedding",
                        lambda image=None, text=None, model=None, processor=None: {"text": p["queries"][:1], "image": p["queries"][1:2]})
    monkeypatch.setattr(search, "blend", lambda a, b, w: np.asarray(a, np.float32))
    try:
        plain = search.search_similar(p["queries"][0], limit=5)
        assert idx.grouped_calls == [] and all("group" not in r and "group_size" not in r for r in plain)
        got = search.search_similar(p["queries"][0], limit=5, group_by="folder")
        assert idx.grouped_calls[-1] == (1, 5, None, None) and len(got) == 5
        assert [r["group"] for r in got] == [r.get("folder") for r in got] and all(r["group_size"] >= 1 for r in got)
        assert got[0]["id"] == plain[0]["id"] and got[0]["similarity_score"] == plain[0]["similarity_score"]
        named = [r["group"] for r in got if r["group"] is not None]
        assert len(named) == len(set(named))
        batch = search.search_similar_batch(p["queries"][:2], limit=4, group_by="folder")
        assert idx.grouped_calls[-1][:2] == (2, 4) and [len(b) for b in batch] == [4, 4] and "group" in batch[1][0]
        search.search_by_text("a cat", limit=3, group_by="folder")
        assert idx.grouped_calls[-1][:2] == (1, 3)
        search.search_multimodal(None, "a cat", 0.5, limit=3, group_by="folder", filters=["f0"])
        assert idx.grouped_calls[-1] == (1, 3, None, 1)
        search.search_multimodal_batch(p["queries"][:2], p["queries"][:2], 0.5, limit=6, group_by="batch", min_similarity=0.5)
        assert idx.grouped_calls[-1][:2] == (2, 6)
        n = len(idx.grouped_calls)
        assert search.search_similar(p["queries"][0], limit=3, group_by="folder", n_probe=2) == []        # (the wrappers log and return [])
        assert search.search_similar(p["queries"][0], limit=3, group_by="folder", after="") == {"results": [], "next": None, "remaining": 0}
        assert len(idx.grouped_calls) == n
    finally:
        search.set_collection(None)


@pytest.fixture()
def tiny(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils

    OracleGroupedIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleGroupedIndex)
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
    # image 2 is stored three times in one folder, the others once: two in another folder, one in none
    rows = [emb[0], emb[1], emb[2], emb[2], emb[2], emb[3]]
    ids = ["a", "b", "c0", "c1", "c2", "d"]
    folders = ["x", "x", "y", "y", "y", None]
    metas = [{"id": i} if f is None else {"id": i, "folder": f} for i, f in zip(ids, folders)]
    search._collection().add(ids=ids, embeddings=np.stack(rows), metadatas=metas)
    index = OracleGroupedIndex.instances[-1]
    client = TestClient(api.create_app())
    q = {"file": ("q.png", _png(imgs[2]), "image/png")}
    plain = client.post("/api/search/image", files=q, data={"limit": "3"})
    assert plain.status_code == 200 and [r["id"] for r in plain.json()["results"]] == ["c0", "c1", "c2"]   # the folder fills every slot
    assert index.grouped_calls == [] and all("group" not in r for r in plain.json()["results"])           # absent: today's call
    r = client.post("/api/search/image", files=q, data={"limit": "3", "group_by": "folder"})
    assert r.status_code == 200 and len(index.grouped_calls) == 1
    res = r.json()["results"]
    assert len(res) == 3 and res[0]["id"] == "c0" and (res[0]["group"], res[0]["group_size"]) == ("y", 3)
    assert sorted((x["group"] or "", x["group_size"]) for x in res) == [("", 1), ("x", 2), ("y", 3)]
    t = client.post("/api/search/text", data={"query": "red drill", "limit": "2", "group_by": "folder"})
    assert t.status_code == 200 and len(index.grouped_calls) == 2 and all("group" in x for x in t.json()["results"])
    m = client.post("/api/search/multimodal", files=q, data={"query": "drill", "weight_image": "1.0", "limit": "2", "group_by": "folder",
                                                              "min_similarity": "0.5"})
    assert m.status_code == 200 and len(index.grouped_calls) == 3 and m.json()["results"][0]["id"] == "c0"
    p = client.post("/api/search/image", files=q, data={"limit": "2", "group_by": "folder", "prefilter": "1"})
    assert p.status_code == 200 and len(index.grouped_calls) == 4
    for route, kw in (("/api/search/image", dict(files=q, data={"limit": "3", "group_by": " "})),
                      ("/api/search/text", dict(data={"query": "x", "limit": "3", "group_by": ""})),
                      ("/api/search/multimodal", dict(files=q, data={"query": "x", "limit": "3", "group_by": " "}))):
        bad = client.post(route, **kw)
        assert bad.status_code == 500 and bad.json()["success"] is False, route
    assert len(index.grouped_calls) == 4


def test_wrapper_argument_checks_come_before_the_call():
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib
    from mmiss_amd.index import MAX_GROUPS, FlatIndex

    assert MAX_GROUPS == gc.MAX_GROUPS == 1 << 24
    assert len(_lib.GROUPED_PLAN_FIELDS) == 16 and len(set(_lib.GROUPED_PLAN_FIELDS)) == 16
    idx = FlatIndex.__new__(FlatIndex)               # no device here: the checks under test run before any library call
    idx.dim, idx.dtype, idx.device, idx._h, idx._lib, idx._call_lock = D, 0, 0, None, _NoLibrary(), threading.RLock()
    q = np.zeros((2, D), np.float32)
    for k in (0, -1, 2041):
        with pytest.raises(ValueError, match="k"):
            idx.query_grouped(q, k)
    for pool in (9, 2041, -1):
        with pytest.raises(ValueError, match="pool"):
            idx.query_grouped(q, 10, pool=pool)
    with pytest.raises(ValueError, match="vectors"):
        idx.query_grouped(np.zeros((2, D + 1), np.float32), 10)
    with pytest.raises(ValueError, match="query"):
        idx.query_grouped(np.zeros((0, D), np.float32), 10)
    with pytest.raises(ValueError, match="require"):
        idx.query_grouped(q, 10, require=np.zeros(3, np.uint64))
    with pytest.raises(ValueError, match="groups"):
        idx.set_groups([1, 2], [0])
    with pytest.raises(ValueError, match="groups"):
        idx.set_groups([1, 2], [0, -2])
    with pytest.raises(ValueError, match="groups"):
        idx.set_groups([1, 2], [MAX_GROUPS, 0])
    with pytest.raises(TypeError, match="groups"):
        idx.set_groups([1, 2], [0.5, 1.0])
    idx._h = None                                    # (nothing to destroy)

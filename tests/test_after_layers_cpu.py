"""The host layers of search after without a GPU, on the oracle-backed stand-in of tests/after_fakes.py: the continuation token,
FlatIndex.ranking, FlatCollection.query(after=) — filters as masks, a filter name past the 64th bit folded into the list, ids /
where as the list, max_distance as the radius, a cursor whose row was deleted between pages, `next` and `remaining` on the last
page, every forbidden combination —, the search wrappers and the three API routes that pass the token through, the argument checks
FlatIndex.query_after makes before it calls the library, and the recorded proof that a call without `after` never reaches
query_after."""
import json
import threading

import numpy as np
import pytest

import after_cases as ac
from after_fakes import OracleAfterIndex
from fakes import OracleEncoder
from oracle import clip_oracle as co
from oracle import retrieval_oracle as ro
from test_partition_layers_cpu import _NoLibrary
from test_radius_layers_cpu import _Proc, _image, _png
from test_subset_layers_cpu import _as_result, _ids, _metas

N, D = 300, 128


@pytest.fixture()
def colmod(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection

    OracleAfterIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleAfterIndex)
    return collection


def _filled(colmod, n=N, filters=1):
    p = ac.corpus(41, n, D, 4)
    col = colmod.FlatCollection("t")
    col.add(ids=_ids(n), embeddings=p["x"], metadatas=_metas(n, filters))     # (labels 0 .. n-1: label == row)
    return col, p, OracleAfterIndex.instances[-1]


def _bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


# ================================================================================================ the token
def test_token_round_trip_for_every_class_of_float_bits():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.collection import make_token, parse_token

    patterns = [0x00000000, 0x80000000,                 # +0.0, -0.0
                0x00000001, 0x807fffff,                 # subnormals of both signs
                0x3f800000, 0xbf800000, 0x3e99999a,     # 1.0, -1.0, 0.3
                0x7f7fffff, 0x00800000,                 # the largest and the smallest normal
                0x7f800000, 0xff800000,                 # +inf, -inf
                0x7fc00000, 0xffc00001]                 # NaNs keep their bits too
    for b in patterns:
        d = np.array([b], np.uint32).view(np.float32)[0]
        for label in (0, 5, -1, 2 ** 62, -2 ** 63, 2 ** 63 - 1):
            token = make_token(d, label)
            assert token == "%08x.%d" % (b, label)
            back = parse_token(token)
            assert _bits(back[0]) == b and back[1] == label and isinstance(back[1], int)
    for bad in ("", " ", "3e99999a", "3e99999a.", ".5", "3e99999a.5.1", "3E99999A.5", "3e99999.5", "03e99999a.5", "3e99999a.+5", "3e99999a.5 ",
                "3e99999a.0x5", "3e99999a.1e3", "zzzzzzzz.5", "3e99999a.%d" % 2 ** 63, "3e99999a.%d" % (-2 ** 63 - 1), None, 5, 0.3, b"3e99999a.5",
                ["3e99999a.5"]):
        with pytest.raises(ValueError):
            parse_token(bad)


# ================================================================================================ FlatIndex.ranking
def test_ranking_chains_pages_to_any_length():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.index import FlatIndex

    n = 700
    p = ac.run_corpus(42, n, D, 4)
    idx = OracleAfterIndex(D, "f16")
    idx.add(p["x"], np.arange(n, dtype=np.int64))
    full_l, full_d = ac.full_ranking(p["queries"][0], idx.rows, idx.labs)
    assert full_l.size == n - 5
    for want, page in ((n + 50, 100), (n - 5, 139), (333, 50), (50, 1000), (7, 7), (1, 1), (0, 10)):
        idx.after_calls.clear()
        lab, dist = FlatIndex.ranking(idx, p["queries"][0], want, page=page)
        m = min(want, n - 5)
        assert lab.shape == dist.shape == (m,) and lab.dtype == np.int64 and dist.dtype == np.float32
        assert ac.same_ranking(lab, dist, full_l[:m], full_d[:m]) is None, (want, page)
        # a full page asks for another one; a short one ends the chain; no page is larger than what is still wanted
        assert len(idx.after_calls) == (-(-want // page) if want <= n - 5 else (n - 5) // page + 1)
        assert all(c[1] <= page for c in idx.after_calls) and sum(c[1] for c in idx.after_calls) <= max(want, 0) + page
    # the same keywords on every page
    cand = np.arange(0, n, 3)
    idx.after_calls.clear()
    lab, dist = FlatIndex.ranking(idx, p["queries"][0], 1000, page=60, labels=cand, max_dist=np.float32(1.2), require=np.uint64(0))
    exp_l, exp_d = ac.full_ranking(p["queries"][0], idx.rows, idx.labs, cand=cand, max_dist=np.float32(1.2))
    assert ac.same_ranking(lab, dist, exp_l, exp_d) is None and 60 < lab.size < cand.size
    assert all(c[3] == float(np.float32(1.2)) and c[4] == tuple(cand.tolist()) and c[5] == 0 for c in idx.after_calls)
    for bad in (dict(n=-1), dict(n=5, page=0), dict(n=5, page=2041)):
        with pytest.raises(ValueError):
            FlatIndex.ranking(idx, p["queries"][0], **bad)


# ================================================================================================ FlatCollection
def test_pages_through_the_collection_and_the_last_page(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"]
    every = col.query(query_embeddings=q, n_results=N)                    # the whole ranking in one call (N < 2040)
    assert "next" not in every and "remaining" not in every
    n_other = idx.other_calls()
    pages = [col.query(query_embeddings=q, n_results=40, after=[None] * 4)]
    assert idx.after_calls[-1] == (4, 40, ((_bits(-np.inf), 0),) * 4, None, None, None, None)
    while any(t is not None for t in pages[-1]["next"]):
        assert len(pages) < 20
        pages.append(col.query(query_embeddings=q, n_results=40, after=pages[-1]["next"]))
    for qi in (0, 1, 3):
        assert sum((pg["ids"][qi] for pg in pages), []) == every["ids"][qi]
        assert sum((pg["distances"][qi] for pg in pages), []) == every["distances"][qi]
        left = N - 5
        for pg in pages:
            assert pg["remaining"][qi] == left
            left -= len(pg["ids"][qi])
            # `next` is the last entry's token until the page that delivers the last row
            last = None if left == 0 else "%08x.%d" % (_bits(pg["distances"][qi][-1]), int(pg["ids"][qi][-1][2:]))
            assert pg["next"][qi] == last
        assert left == 0 and len(pages) == -(-(N - 5) // 40)
    assert all(pg["ids"][2] == [] and pg["next"][2] is None and pg["remaining"][2] == 0 for pg in pages)   # no direction
    assert pages[0]["metadatas"][0][0] == _metas()[int(pages[0]["ids"][0][0][2:])] and pages[0]["included"] == every["included"]
    assert idx.other_calls() == n_other                                   # nothing but query_after ran
    # the page behind the last one, and a mixed batch: one query at the start, one in the middle, one at its end
    end = "%08x.%d" % (_bits(every["distances"][0][-1]), int(every["ids"][0][-1][2:]))
    got = col.query(query_embeddings=q, n_results=10, after=[end, None, None, pages[0]["next"][3]])
    assert got["ids"][0] == [] and got["remaining"][0] == 0 and got["next"][0] is None
    assert got["ids"][1] == every["ids"][1][:10] and got["ids"][3] == every["ids"][3][40:50] and got["remaining"][3] == N - 5 - 40
    # n_results above 2040 asks for 2040 at the most, without the clamp's warning; above the count: the count
    col.query(query_embeddings=q[:1], n_results=5000, after=[None])
    assert idx.after_calls[-1][1] == N


def test_a_cursor_whose_row_was_deleted_between_pages(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"][:1]
    every = col.query(query_embeddings=q, n_results=N)["ids"][0]
    page1 = col.query(query_embeddings=q, n_results=10, after=[None])
    assert page1["ids"][0] == every[:10]
    col.delete(ids=[every[9], every[10], every[3]])                       # the cursor's own row, the next one, an earlier one
    page2 = col.query(query_embeddings=q, n_results=10, after=page1["next"])
    assert page2["ids"][0] == every[11:21] and page2["remaining"][0] == N - 5 - 3 - 8       # (eight live rows lie before the cursor)
    # a row added between pages is ranked as it stands: a copy of the query lies BEFORE the cursor and is not delivered
    col.add(ids=["late"], embeddings=np.asarray(q) * 3.0, metadatas=[{"id": "late"}])
    page3 = col.query(query_embeddings=q, n_results=10, after=page2["next"])
    assert page3["ids"][0] == every[21:31] and col.query(query_embeddings=q, n_results=1, after=[None])["ids"][0] == ["late"]


def test_filters_ids_where_and_max_distance_travel(colmod):
    col, p, idx = _filled(colmod, filters=3)
    q = p["queries"]
    tags = lambda: np.array([idx.tags.get(int(l), 0) for l in idx.labs], np.uint64)   # noqa: E731
    # filters as masks
    page1 = col.query(query_embeddings=q, n_results=7, filters=["f0", "f2"], after=[None] * 4)
    assert idx.after_calls[-1][3:] == (None, None, 0b101, None)
    exp = ac.expected_after(q, 7, ac.START, 0, idx.rows, idx.labs, tags(), np.uint64(0b101))
    assert (page1["ids"], page1["distances"]) == _as_result(exp) and page1["remaining"] == [int(r) for r in exp[3]]
    assert all(int(i[2:]) % 2 == 1 for i in page1["ids"][0])              # f0 and f2 say "yes" on odd rows
    page2 = col.query(query_embeddings=q, n_results=7, filters=["f0", "f2"], after=page1["next"])
    exp2 = ac.expected_after(q, 7, exp[1][:, 6], exp[0][:, 6], idx.rows, idx.labs, tags(), np.uint64(0b101))
    assert (page2["ids"][0], page2["distances"][0]) == (_as_result(exp2)[0][0], _as_result(exp2)[1][0]) and page2["remaining"][0] == exp[3][0] - 7
    # a name no row has ever answered admits nothing, without a call
    n = len(idx.after_calls)
    got = col.query(query_embeddings=q, n_results=5, filters=["nobody"], after=[None] * 4)
    assert got["ids"] == [[], [], [], []] and got["next"] == [None] * 4 and got["remaining"] == [0] * 4 and len(idx.after_calls) == n
    # ids / where become the list, max_distance the radius — inside the call, not a cut of its result
    rows = list(range(10, 200, 3))
    ids = [_ids()[r] for r in rows[::-1]] + ["no-such-id", _ids()[10]]
    where = {"album": "city"}
    both = [r for r in rows if r % 3 == 1]
    first = ac.expected_after(q, 30, ac.START, 0, idx.rows, idx.labs, cand=np.asarray(both))
    radius = float(first[1][0, 12])
    got = col.query(query_embeddings=q, n_results=5, ids=ids, where=where, max_distance=radius, n_probe=3, after=[None] * 4)
    assert idx.after_calls[-1][3:] == (float(np.float32(radius)), tuple(both), None, None) and idx.radius_calls == [] and idx.probed_calls == []
    exp = ac.expected_after(q, 5, ac.START, 0, idx.rows, idx.labs, cand=np.asarray(both), max_dist=np.float32(radius))
    assert (got["ids"], got["distances"]) == _as_result(exp) and got["remaining"][0] == 13 and got["next"][0] is not None
    got = col.query(query_embeddings=q, n_results=5, ids=["no-such-id"], after=[None] * 4)
    assert got["ids"] == [[], [], [], []] and got["remaining"] == [0] * 4
    with pytest.raises(ValueError):
        col.query(query_embeddings=q, n_results=5, where={"album": {"$like": "c%"}}, after=[None] * 4)
    # an empty collection
    got = colmod.FlatCollection("empty").query(query_embeddings=q, n_results=5, after=[None] * 4)
    assert got["ids"] == [[], [], [], []] and got["next"] == [None] * 4 and got["remaining"] == [0] * 4


def test_a_65th_filter_name_is_folded_into_the_list(colmod):
    n = 400
    col, p, idx = _filled(colmod, n=n, filters=66)
    q = p["queries"][:1]
    col.query(query_embeddings=q, n_results=1, filters=["f0"])            # (the tags are pushed: bits are dealt)
    assert "f65" in col._filter_overflow and "f63" in col._filter_bits
    yes65 = [r for r in range(n) if (r + 65) % 2]
    got = col.query(query_embeddings=q, n_results=5, filters=["f65"], after=[None])
    assert idx.after_calls[-1][3:] == (None, tuple(yes65), None, None)    # folded on the host, no mask
    exp = ac.expected_after(q, 5, ac.START, 0, idx.rows, idx.labs, cand=np.asarray(yes65))
    assert (got["ids"], got["distances"]) == _as_result(exp, n) and got["remaining"][0] == exp[3][0]
    # a mapped and an unmapped name together, within ids: the mapped one as a mask, the other narrows the list
    bit = 1 << col._filter_bits["f1"]
    got = col.query(query_embeddings=q, n_results=5, filters=["f1", "f65"], ids=_ids(n)[:100], after=got["next"])
    assert idx.after_calls[-1][3:] == (None, tuple(r for r in yes65 if r < 100), bit, None)
    assert idx.after_calls[-1][2] == ((_bits(exp[1][0, 4]), int(exp[0][0, 4])),)


def test_forbidden_combinations_and_malformed_tokens(colmod):
    col, p, idx = _filled(colmod)
    q = p["queries"]
    n = len(idx.after_calls)
    with pytest.raises(ValueError, match="distinct_distance"):
        col.query(query_embeddings=q, n_results=5, distinct_distance=0.01, after=[None] * 4)
    for bad in ([None] * 3, [None] * 5, [], "3e99999a.5", [None, "x", None, None], [None, "3e99999a", None, None], [5, None, None, None],
                [None, None, None, "3e99999a.5.5"]):
        with pytest.raises(ValueError, match="after"):
            col.query(query_embeddings=q, n_results=5, after=bad)
    with pytest.raises(ValueError, match="n_probe"):
        col.query(query_embeddings=q, n_results=5, n_probe=0, after=[None] * 4)
    assert len(idx.after_calls) == n and idx.distinct_calls == []
    # n_probe is ignored, with a partition present too: the continuation is exact
    plain = col.query(query_embeddings=q, n_results=5, after=[None] * 4)
    col.build_partition(7, iters=2)
    n_probed = len(idx.probed_calls)
    assert col.query(query_embeddings=q, n_results=5, n_probe=1, after=[None] * 4) == plain and len(idx.probed_calls) == n_probed


# ================================================================================================ search wrappers, routes
def test_search_wrappers_return_pages(colmod, monkeypatch):
    from mmiss_amd import search, utils

    col, p, idx = _filled(colmod)
    search.set_collection(col)
    monkeypatch.setattr(utils, "load_clip_model", lambda: (None, None))
    monkeypatch.setattr(utils, "generate_clip_embedding",
                        lambda image=None, text=None, model=None, processor=None: {"text": p["queries"][:1], "image": p["queries"][1:2]})
    monkeypatch.setattr(search, "blend", lambda a, b, w: np.asarray(a, np.float32))
    q = p["queries"]
    try:
        plain = search.search_similar(q[0], limit=25)
        assert isinstance(plain, list) and len(plain) == 25
        page1 = search.search_similar(q[0], limit=10, after="")
        assert sorted(page1) == ["next", "remaining", "results"] and page1["remaining"] == N - 5
        page2 = search.search_similar(q[0], limit=10, after=page1["next"])
        page3 = search.search_similar(q[0], limit=5, after=page2["next"], n_probe=2)
        assert page1["results"] + page2["results"] + page3["results"] == plain and page3["remaining"] == N - 5 - 20
        # limit <= 0: pages of 1000 — here the whole ranking, and the last page
        rest = search.search_similar(q[0], limit=0, after=page3["next"])
        assert len(rest["results"]) == N - 5 - 25 == rest["remaining"] and rest["next"] is None and idx.after_calls[-1][1] == N
        # the other arguments travel
        got = search.search_by_text("a cat", limit=5, after="", filters=["f0"], within_ids=_ids()[:100], min_similarity=0.1)
        assert idx.after_calls[-1][1:] == (5, ((_bits(-np.inf), 0),), float(np.float32(utils.max_distance_for_similarity(0.1))),
                                           tuple(range(100)), 1, None)
        assert len(got["results"]) == 5 and got["next"] is not None
        got = search.search_multimodal(None, "a cat", 0.5, limit=6, after=got["next"], where={"album": "forest"})
        assert idx.after_calls[-1][1] == 6 and idx.after_calls[-1][4] == tuple(r for r in range(N) if r % 3 == 2)
        batch = search.search_similar_batch(np.stack([q[0], q[0], q[2]]), limit=4, after=["", page1["next"], None])   # (query 2: no direction)
        assert [sorted(b) for b in batch] == [["next", "remaining", "results"]] * 3
        assert batch[1]["results"] == plain[10:14] and batch[0]["results"] == plain[:4] and batch[2] == {"results": [], "next": None, "remaining": 0}
        batch = search.search_multimodal_batch(q[:2], q[:2], 0.5, limit=3, after=[page2["next"], ""])
        assert batch[0]["results"] == plain[20:23] and len(batch[1]["results"]) == 3
        # refused: logged, an empty page (the list forms answer [])
        n = len(idx.after_calls)
        empty = {"results": [], "next": None, "remaining": 0}
        assert search.search_similar(q[0], limit=5, after="not-a-token") == empty
        assert search.search_similar(q[0], limit=5, after="", distinct_similarity=0.99) == empty
        assert search.search_by_text("a cat", limit=5, after="3e99999a") == empty
        assert search.search_multimodal(None, "a cat", 0.5, limit=5, after="x.y") == empty
        assert search.search_similar_batch(q[:3], limit=4, after=[""]) == []
        assert len(idx.after_calls) == n
    finally:
        search.set_collection(None)


@pytest.fixture()
def tiny(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils

    OracleAfterIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleAfterIndex)
    monkeypatch.setattr(search, "blend", lambda i, t, w: ro.blend(i, t, w))
    utils.set_clip_model(OracleEncoder(co.TINY), _Proc(co.TINY))
    search.set_collection(collection.FlatCollection("t"))
    yield search, utils
    utils.set_clip_model(None, None)
    search.set_collection(None)


def test_api_routes_take_the_after_field(tiny):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from starlette.testclient import TestClient
    from mmiss_amd import api

    search, utils = tiny
    imgs = [_image(i) for i in range(7)]
    emb = [np.asarray(utils.generate_clip_embedding(image=im)["image"][0], np.float32) for im in imgs]
    ids = ["a", "b", "c", "d", "e", "f", "g"]
    yes = lambda i: json.dumps({"keep": "yes" if i != "b" else "no"})     # noqa: E731
    search._collection().add(ids=ids, embeddings=np.stack(emb), metadatas=[{"id": i, "filter_results_json": yes(i)} for i in ids])
    index = OracleAfterIndex.instances[-1]
    client = TestClient(api.create_app())
    q = {"file": ("q.png", _png(imgs[2]), "image/png")}
    plain = client.post("/api/search/image", files=q, data={"limit": "7"})
    assert plain.status_code == 200 and sorted(plain.json()) == ["results"] and index.after_calls == []          # absent: today's call
    order = [x["id"] for x in plain.json()["results"]]
    assert order[0] == "c" and len(order) == 7
    # an empty field is the first page; `next` continues; the last page has next null
    r1 = client.post("/api/search/image", files=q, data={"limit": "3", "after": ""}).json()
    assert sorted(r1) == ["next", "remaining", "results"] and [x["id"] for x in r1["results"]] == order[:3] and r1["remaining"] == 7
    r2 = client.post("/api/search/image", files=q, data={"limit": "3", "after": r1["next"]}).json()
    r3 = client.post("/api/search/image", files=q, data={"limit": "3", "after": r2["next"]}).json()
    assert [x["id"] for x in r2["results"] + r3["results"]] == order[3:] and r2["remaining"] == 4 and r3["remaining"] == 1 and r3["next"] is None
    # limit <= 0 with the field present: pages of 1000
    r = client.post("/api/search/image", files=q, data={"limit": "0", "after": r1["next"]}).json()
    assert [x["id"] for x in r["results"]] == order[3:] and r["next"] is None and index.after_calls[-1][1] == 7
    # filters are applied before the search; ids travel
    r = client.post("/api/search/image", files=q, data={"limit": "2", "after": "", "filters": "keep", "ids": "a,b,c,d"}).json()
    assert [x["id"] for x in r["results"]] == [i for i in order if i in "acd"][:2] and r["remaining"] == 3
    assert index.after_calls[-1][4] == (0, 1, 2, 3) and index.after_calls[-1][5] == 1
    t1 = client.post("/api/search/text", data={"query": "red drill", "limit": "4", "after": ""})
    assert t1.status_code == 200 and t1.json()["remaining"] == 7 and len(t1.json()["results"]) == 4
    t2 = client.post("/api/search/text", data={"query": "red drill", "limit": "4", "after": t1.json()["next"]}).json()
    assert len(t2["results"]) == 3 and t2["next"] is None and not {x["id"] for x in t2["results"]} & {x["id"] for x in t1.json()["results"]}
    m = client.post("/api/search/multimodal", files=q, data={"query": "drill", "weight_image": "1.0", "limit": "2", "after": r1["next"]}).json()
    assert [x["id"] for x in m["results"]] == order[3:5] and m["remaining"] == 4 and m["next"] is not None
    n = len(index.after_calls)
    for bad in ("x", "3e99999a", "3e99999a.5.5", "3E99999A.5"):
        for route, kw in (("/api/search/image", dict(files=q, data={"limit": "3", "after": bad})),
                          ("/api/search/text", dict(data={"query": "x", "limit": "3", "after": bad})),
                          ("/api/search/multimodal", dict(files=q, data={"query": "x", "limit": "3", "after": bad}))):
            r = client.post(route, **kw)
            assert r.status_code == 500 and r.json()["success"] is False, (route, bad)
    assert len(index.after_calls) == n
    # ... as a bad limit is answered
    r = client.post("/api/search/text", data={"query": "x", "limit": "many"})
    assert r.status_code == 500 and r.json()["success"] is False


# ================================================================================================ nothing changes without it
class _RefusingAfterIndex(OracleAfterIndex):
    """the stand-in with a query_after that must not be reached"""
    reached = []

    def query_after(self, *a, **kw):
        _RefusingAfterIndex.reached.append((a, kw))
        raise AssertionError("a call without after reached query_after")


def test_a_call_without_after_never_reaches_query_after(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils

    _RefusingAfterIndex.reached = []
    monkeypatch.setattr(collection, "FlatIndex", _RefusingAfterIndex)
    col, p, _ = _filled(collection, filters=66)
    idx = _RefusingAfterIndex.instances[-1]
    q = p["queries"]
    col.build_partition(7, iters=2)
    calls = [dict(), dict(filters=["f0"]), dict(filters=["f0", "f65"]), dict(filters=["f65"], max_distance=0.5), dict(max_distance=0.4),
             dict(n_probe=2), dict(n_probe=2, filters=["f1"]), dict(distinct_distance=0.01), dict(distinct_distance=0.01, pool=100, n_probe=1),
             dict(ids=_ids()[:50]), dict(where={"album": "city"}, filters=["f0"]), dict(after=None), dict(ids=None, where=None, after=None)]
    for kw in calls:
        got = col.query(query_embeddings=q, n_results=5, **kw)
        assert len(got["ids"]) == 4 and "next" not in got and "remaining" not in got, kw
    kinds = (idx.flat_calls, len(idx.probed_calls), len(idx.distinct_calls), len(idx.radius_calls), len(idx.subset_calls))
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
        assert len(search.search_multimodal_batch(q[:2], q[:2], 0.5, limit=5, min_similarity=0.1, within_ids=_ids()[:40])) == 2
    finally:
        search.set_collection(None)
    assert _RefusingAfterIndex.reached == [] and idx.after_calls == []    # ... and none of them is the new one
    with pytest.raises(AssertionError):                                   # (the stand-in does refuse when it is reached)
        col.query(query_embeddings=q, n_results=5, after=[None] * 4)
    assert len(_RefusingAfterIndex.reached) == 1


def test_the_clamp_warns_only_without_after(colmod):
    n = 2100
    col, p, idx = _filled(colmod, n=n)
    q = p["queries"][:1]
    import logging

    records = []
    handler = logging.Handler()
    handler.emit = records.append
    colmod.logger.addHandler(handler)
    try:
        got = col.query(query_embeddings=q, n_results=n)
        assert len(got["ids"][0]) == 2040 and any("clamped" in r.getMessage() for r in records)
        records.clear()
        got = col.query(query_embeddings=q, n_results=n, after=[None])
        assert len(got["ids"][0]) == 2040 and got["remaining"][0] == n - 5 and got["next"][0] is not None and records == []
        rest = col.query(query_embeddings=q, n_results=n, after=got["next"])
        assert len(rest["ids"][0]) == n - 5 - 2040 and rest["next"][0] is None   # past position 2040: what the clamp cuts off
    finally:
        colmod.logger.removeHandler(handler)


# ================================================================================================ FlatIndex.query_after
def test_wrapper_argument_checks_come_before_the_call():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.index import FlatIndex

    idx = FlatIndex.__new__(FlatIndex)               # no device here: the checks under test run before any library call
    idx.dim, idx.dtype, idx.device, idx._h, idx._lib, idx._call_lock = D, 0, 0, None, _NoLibrary(), threading.RLock()
    q = np.zeros((2, D), np.float32)
    ad, al = np.zeros(2, np.float32), np.zeros(2, np.int64)
    with pytest.raises(ValueError, match="k"):
        idx.query_after(q, 0, ad, al)
    with pytest.raises(ValueError, match="k"):
        idx.query_after(q, 2041, ad, al)
    with pytest.raises(TypeError, match="labels"):
        idx.query_after(q, 10, ad, al, labels=np.arange(5, dtype=np.float32))
    with pytest.raises(TypeError, match="labels"):
        idx.query_after(q, 10, ad, al, labels=["a", "b"])
    with pytest.raises(TypeError, match="after_label"):
        idx.query_after(q, 10, ad, al.astype(np.float32))
    with pytest.raises(ValueError, match="after_dist"):
        idx.query_after(q, 10, np.zeros(3, np.float32), al)
    with pytest.raises(ValueError, match="after_label"):
        idx.query_after(q, 10, ad, np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="max_dist"):
        idx.query_after(q, 10, ad, al, max_dist=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="vectors"):
        idx.query_after(np.zeros((2, D + 1), np.float32), 10, ad, al)
    with pytest.raises(ValueError, match="query"):
        idx.query_after(np.zeros((0, D), np.float32), 10, ad[:0], al[:0])
    with pytest.raises(ValueError, match="require"):
        idx.query_after(q, 10, ad, al, require=np.zeros(3, np.uint64))
    with pytest.raises(TypeError, match="exclude"):
        idx.query_after(q, 10, ad, al, exclude=1.5)
    with pytest.raises(ValueError, match="page"):
        idx.ranking(q[0], 5, page=0)
    idx._h = None                                    # (nothing to destroy)

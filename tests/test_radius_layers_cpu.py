"""The host layers of radius queries without a GPU, on the oracle-backed stand-in of tests/radius_fakes.py:
FlatCollection.query(max_distance=) with and without filters, the search functions' min_similarity, find_near_duplicates,
process_image(near_duplicate_similarity=) and the API's form fields (absent, valid, bad)."""
import io
import json

import numpy as np
import pytest

from fakes import OracleEncoder
from oracle import clip_oracle as co
from oracle import retrieval_oracle as ro
from radius_fakes import OracleRadiusIndex

D = 128


def _rows(n=40, seed=2):
    """n random rows; rows 5 / 6 and 20 / 21 / 22 are near copies (cosine about 0.999)"""
    rng = np.random.Generator(np.random.Philox(seed))
    v = rng.standard_normal((n, D)).astype(np.float32)
    for a, bs in ((5, (6,)), (20, (21, 22))):
        for b in bs:
            v[b] = v[a] + 0.04 * np.linalg.norm(v[a]) / np.sqrt(D) * rng.standard_normal(D).astype(np.float32)
    return v


def _meta(i, answers=None):
    return {"id": f"im{i:02d}", "filter_results_json": json.dumps(answers or {})}


@pytest.fixture()
def mods(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils

    monkeypatch.setattr(collection, "FlatIndex", OracleRadiusIndex)
    col = collection.FlatCollection("t")
    v = _rows()
    col.add(ids=[f"im{i:02d}" for i in range(v.shape[0])], embeddings=v,
            metadatas=[_meta(i, {"even": "yes" if i % 2 == 0 else "no"}) for i in range(v.shape[0])])
    search.set_collection(col)
    yield collection, search, utils, col, v
    search.set_collection(None)


def test_collection_query_with_max_distance(mods):
    collection, search, utils, col, v = mods
    q = v[20:21]
    wide = col.query(query_embeddings=q, n_results=40, include=["distances"])
    got = col.query(query_embeddings=q, n_results=40, include=["distances"], max_distance=0.01)
    n = sum(d <= np.float32(0.01) for d in wide["distances"][0])
    assert n == 3 and got["ids"][0] == wide["ids"][0][:3] and sorted(got["ids"][0]) == ["im20", "im21", "im22"]
    assert got["distances"][0] == wide["distances"][0][:3]
    assert col.query(query_embeddings=q, n_results=2, max_distance=0.01)["ids"][0] == wide["ids"][0][:2]      # n_results is the cap
    assert col.query(query_embeddings=q, n_results=5, max_distance=-1.0)["ids"] == [[]]
    # with a filter: the members among the admitted rows
    got = col.query(query_embeddings=q, n_results=40, max_distance=0.01, filters=["even"])
    assert got["ids"][0] == [i for i in wide["ids"][0][:3] if int(i[2:]) % 2 == 0] and len(got["ids"][0]) == 2
    assert col.query(query_embeddings=q, n_results=40, max_distance=0.01, filters=["no such filter"])["ids"] == [[]]


def test_search_min_similarity_is_the_cut_of_the_ranking(mods, monkeypatch):
    collection, search, utils, col, v = mods
    for s in (0.0, 0.5, 0.52, 0.995, 1.0):
        full = search.search_similar(v[5], limit=0)
        got = search.search_similar(v[5], limit=0, min_similarity=s)
        assert got == [r for r in full if r["similarity_score"] >= s], s
    assert [r["id"] for r in search.search_similar(v[5], limit=0, min_similarity=0.995)] == ["im05", "im06"]
    assert len(search.search_similar(v[5], limit=1, min_similarity=0.995)) == 1
    batch = search.search_similar_batch(v[[5, 20]], limit=0, min_similarity=0.995)
    assert [[r["id"] for r in b] for b in batch] == [["im05", "im06"], ["im20", "im21", "im22"]]
    monkeypatch.setattr(search, "blend", lambda i, t, w: ro.blend(i, t, w))
    got = search.search_multimodal_batch(v[[5]], v[[5]], 0.5, limit=0, min_similarity=0.995)
    assert [r["id"] for r in got[0]] == ["im05", "im06"]
    got = search.search_similar(v[20], limit=0, min_similarity=0.995, filters=["even"])
    assert [r["id"] for r in got] == ["im20", "im22"]


def test_find_near_duplicates(mods):
    collection, search, utils, col, v = mods
    pairs = search.find_near_duplicates(min_similarity=0.995)
    assert [(a, b) for a, b, _ in pairs] in ([("im05", "im06"), ("im20", "im21"), ("im20", "im22"), ("im21", "im22")],
                                              [("im05", "im06"), ("im20", "im22"), ("im20", "im21"), ("im21", "im22")])
    assert all(0.995 <= s <= 1.0 for _, _, s in pairs)
    assert pairs[1][2] >= pairs[2][2]                       # a row's partners: nearest first
    assert search.find_near_duplicates(min_similarity=0.995, limit=2) == pairs[:2]
    assert search.find_near_duplicates(min_similarity=1.0) == []
    assert col._index.radius_calls[0][0] == "by_label"


class _Proc:
    def __init__(self, shape):
        self.shape = shape

    def rgb_arrays(self, images):
        return [np.asarray(im.convert("RGB") if hasattr(im, "convert") else im, dtype=np.uint8) for im in images]

    def tokenize(self, texts):
        s = self.shape
        return np.stack([co.synthetic_text_ids(1, s.t_ctx, s.t_vocab, s.eos_token_id, seed=sum(map(ord, t)) % 9973)[0] for t in texts])


def _image(seed, touch=False, size=(90, 70)):
    from PIL import Image

    a = np.random.Generator(np.random.Philox(seed)).integers(0, 256, size=(size[1], size[0], 3), dtype=np.uint8)
    if touch:
        a[3, 4, 1] ^= 1                                     # one pixel, one bit
    return Image.fromarray(a)


def _png(image):
    buf = io.BytesIO()
    image.save(buf, format="PNG")
    return buf.getvalue()


@pytest.fixture()
def tiny(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection, search, utils

    monkeypatch.setattr(collection, "FlatIndex", OracleRadiusIndex)
    monkeypatch.setattr(search, "blend", lambda i, t, w: ro.blend(i, t, w))
    utils.set_clip_model(OracleEncoder(co.TINY), _Proc(co.TINY))
    search.set_collection(collection.FlatCollection("t"))
    yield search
    utils.set_clip_model(None, None)
    search.set_collection(None)


def test_process_image_refuses_a_near_duplicate(tiny):
    search = tiny
    meta, stored = search.process_image(_image(1), "first", {"id": "first", "note": "original"}, near_duplicate_similarity=0.98)
    assert stored and meta["note"] == "original"
    meta, stored = search.process_image(_image(1, touch=True), "second", {"id": "second"}, near_duplicate_similarity=0.98)
    assert not stored and meta["id"] == "first" and meta["note"] == "original"
    assert search._collection().count() == 1
    meta, stored = search.process_image(_image(1, touch=True), "second", {"id": "second"})          # without the field: stored
    assert stored and search._collection().count() == 2
    meta, stored = search.process_image(_image(2), "third", {"id": "third"}, near_duplicate_similarity=0.98)
    assert stored
    assert search.process_images([_image(2, touch=True), _image(3)], ["fourth", "fifth"], near_duplicate_similarity=0.98) == 1
    assert search._collection().get(ids=["fourth", "fifth"], include=[])["ids"] == ["fifth"]


def test_api_fields(tiny):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from starlette.testclient import TestClient
    from mmiss_amd import api

    search = tiny
    client = TestClient(api.create_app())
    imgs = [_image(i) for i in range(4)]
    ids = [client.post("/api/upload", files={"file": (f"{i}.png", _png(im), "image/png")}).json()["metadata"]["id"] for i, im in enumerate(imgs)]
    q = {"file": ("q.png", _png(imgs[2]), "image/png")}
    plain = client.post("/api/search/image", files=q, data={"limit": "0"})
    assert plain.status_code == 200 and len(plain.json()["results"]) == 4
    index = search._collection()._index
    assert index.radius_calls == []                                       # an absent field: the top-k query, as before
    for s in ("0", "0.6", "0.999", "1"):
        r = client.post("/api/search/image", files=q, data={"limit": "0", "min_similarity": s})
        assert r.status_code == 200
        assert r.json()["results"] == [x for x in plain.json()["results"] if x["similarity_score"] >= float(s)], s
    assert [x["id"] for x in client.post("/api/search/image", files=q, data={"limit": "0", "min_similarity": "0.999"}).json()["results"]] == [ids[2]]
    assert len(index.radius_calls) == 5
    t_plain = client.post("/api/search/text", data={"query": "red drill", "limit": "0"}).json()["results"]
    t = client.post("/api/search/text", data={"query": "red drill", "limit": "0", "min_similarity": "0.5"})
    assert t.status_code == 200 and t.json()["results"] == [x for x in t_plain if x["similarity_score"] >= 0.5]
    m = client.post("/api/search/multimodal", files=q, data={"query": "drill", "weight_image": "1.0", "limit": "0", "min_similarity": "0.999"})
    assert m.status_code == 200 and [x["id"] for x in m.json()["results"]] == [ids[2]]
    bad_limit = client.post("/api/search/image", files=q, data={"limit": "many"})
    for bad in ("1.5", "-0.1", "nan", "high"):
        r = client.post("/api/search/image", files=q, data={"limit": "3", "min_similarity": bad})
        assert r.status_code == bad_limit.status_code == 500 and r.json()["success"] is False, bad
        r = client.post("/api/upload", files={"file": ("n.png", _png(_image(9)), "image/png")}, data={"near_duplicate_similarity": bad})
        assert r.status_code == 500, bad
    # a one-pixel change gets a new hash id... or the same: either way the upload is answered 409 with the stored image's metadata
    r = client.post("/api/upload", files={"file": ("again.png", _png(_image(1, touch=True)), "image/png")},
                    data={"near_duplicate_similarity": "0.98"})
    assert r.status_code == 409 and r.json()["metadata"]["id"] == ids[1]
    assert search._collection().count() == 4

"""Filtered search without a GPU: the new C entry points refuse to run without a device, FlatIndex validates the query
masks, FlatCollection derives, tracks and pushes the rows' tag words (on a test-local stand-in whose filtered query is the
oracle on the admitted subset), and the API's `prefilter` field returns `limit` filtered results where the reference's
post-filter (backend/app/main.py:202-222) returns fewer."""
import io
import json

import numpy as np
import pytest

from fakes import OracleEncoder, OracleIndex
from oracle import retrieval_oracle as ro


class TaggedOracleIndex(OracleIndex):
    """OracleIndex with per-row tag words and the filtered query of FlatIndex, answered by the oracle on the admitted rows.
    Records every set_tags call."""

    instances = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.tags = {}
        self.pushes = []
        TaggedOracleIndex.instances.append(self)

    def set_tags(self, labels, tags):
        labels = [int(x) for x in np.asarray(labels).reshape(-1)]
        tags = [int(x) for x in np.asarray(tags, np.uint64).reshape(-1)]
        have = set(self.labs.tolist())
        if any(l not in have for l in labels):
            raise RuntimeError("label not in the index")
        self.pushes.append(dict(zip(labels, tags)))
        self.tags.update(zip(labels, tags))

    def get_tags(self, labels):
        return np.array([self.tags.get(int(l), 0) for l in np.asarray(labels).reshape(-1)], np.uint64)

    def load(self, path):
        super().load(path)
        self.tags = {}   # as mmiss_index_load: the file holds no tags

    def query(self, q, k, require=None, exclude=None):
        if require is None and exclude is None:
            return super().query(q, k)
        q = np.asarray(q, np.float32)
        if q.ndim == 1:
            q = q[None]
        Q = q.shape[0]
        req = np.broadcast_to(np.asarray(0 if require is None else require, np.uint64), (Q,))
        exc = np.broadcast_to(np.asarray(0 if exclude is None else exclude, np.uint64), (Q,))
        tags = np.array([self.tags.get(int(l), 0) for l in self.labs], np.uint64)
        out = [np.full((Q, k), -1, np.int64), np.full((Q, k), np.inf, np.float32), np.zeros(Q, np.int32)]
        for i in range(Q):
            sub = np.nonzero(((tags & req[i]) == req[i]) & ((tags & exc[i]) == 0))[0]
            if sub.size:
                ol, od, oc = ro.query(q[i:i + 1], self.rows[sub], self.labs[sub], k)
                out[0][i], out[1][i], out[2][i] = ol[0], od[0], oc[0]
        return tuple(out)


def _vecs(n, d=128, seed=0):
    return np.random.Generator(np.random.Philox(seed)).standard_normal((n, d), dtype=np.float32)


def _meta(answers):
    return {"filter_results_json": json.dumps(answers)}


@pytest.fixture()
def colmod(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection

    TaggedOracleIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", TaggedOracleIndex)
    return collection


# ---------------------------------------------------------------------------------------------------- C-ABI and FlatIndex
def test_filtered_entry_points_exist_and_fail_loudly_without_a_device():
    import torch

    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib
    from mmiss_amd.index import FlatIndex

    lib = _lib.load()
    for name in ("mmiss_index_set_tags", "mmiss_index_get_tags", "mmiss_index_query_filtered", "mmiss_index_query_filtered_begin"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    q = np.zeros((1, 128), np.float32)
    lab, dist = np.zeros((1, 1), np.int64), np.zeros((1, 1), np.float32)
    req = np.zeros(1, np.uint64)
    assert lib.mmiss_index_query_filtered(None, q.ctypes.data, 1, 1, req.ctypes.data, None, lab.ctypes.data, dist.ctypes.data, None) != 0
    assert lib.mmiss_index_query_filtered_begin(None, q.ctypes.data, 1, 1, None, None, lab.ctypes.data, dist.ctypes.data, None) != 0
    labels = np.zeros(1, np.int64)
    assert lib.mmiss_index_set_tags(None, labels.ctypes.data, req.ctypes.data, 1) != 0
    assert lib.mmiss_index_get_tags(None, labels.ctypes.data, 1, req.ctypes.data) != 0
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            FlatIndex(128, "f16")


def test_mask_shapes_and_dtypes_are_validated():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.index import FlatIndex

    m = FlatIndex._mask
    q = np.zeros((3, 128), np.float32)
    assert m(None, 3, q, "require") is None
    np.testing.assert_array_equal(m(5, 3, q, "require"), np.full(3, 5, np.uint64))
    np.testing.assert_array_equal(m(np.uint64(1 << 63), 3, q, "require"), np.full(3, 1 << 63, np.uint64))
    np.testing.assert_array_equal(m((1 << 64) - 1, 3, q, "require"), np.full(3, (1 << 64) - 1, np.uint64))
    np.testing.assert_array_equal(m(-1, 3, q, "require"), np.full(3, (1 << 64) - 1, np.uint64))   # an int64 bit pattern
    got = m(np.array([1, -1, 2], np.int64), 3, q, "require")
    assert got.dtype == np.uint64 and got.tolist() == [1, (1 << 64) - 1, 2]
    assert m(np.array([1, 2, 3], np.uint32), 3, q, "exclude").tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="require"):
        m(np.zeros(2, np.uint64), 3, q, "require")            # not [Q]
    with pytest.raises(ValueError):
        m(np.zeros((3, 1), np.uint64), 3, q, "require")
    with pytest.raises(ValueError):
        m(1 << 64, 3, q, "require")                           # does not fit 64 bits
    with pytest.raises(TypeError):
        m(np.zeros(3, np.float32), 3, q, "exclude")
    with pytest.raises(TypeError):
        m(1.0, 3, q, "exclude")
    with pytest.raises(TypeError):
        m(True, 3, q, "exclude")
    import torch

    t = m(torch.tensor([1, 2, 3]), 3, q, "require")             # CPU tensor -> numpy
    assert isinstance(t, np.ndarray) and t.tolist() == [1, 2, 3]
    with pytest.raises(TypeError):
        m(torch.zeros(3), 3, q, "require")
    with pytest.raises(ValueError):
        m(torch.zeros(4, dtype=torch.int64), 3, q, "require")


def test_sharded_index_passes_masks_to_its_shard():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.sharded import ShardedIndex

    seen = {}

    class Local:
        def query(self, q, k, **kw):
            seen.update(kw)
            return "r"

    s = ShardedIndex.__new__(ShardedIndex)
    s.local, s.group, s.rank, s.world = Local(), None, 0, 1
    assert s.query(np.zeros((1, 4)), 3, require=5) == "r" and seen == {"require": 5}
    seen.clear()
    s.query(np.zeros((1, 4)), 3)
    assert seen == {}


# ---------------------------------------------------------------------------------------------------- collection
def _post_filter(col, q, n, filters):
    """The reference's answer with n_results = count: the full ranking, post-filtered, truncated to n."""
    from mmiss_amd.api import apply_filters

    full = col.query(query_embeddings=q, n_results=col.count(), include=["metadatas", "distances"])
    out = []
    for qi in range(q.shape[0]):
        kept = [(i, d) for i, m, d in zip(full["ids"][qi], full["metadatas"][qi], full["distances"][qi])
                if apply_filters([dict(m or {})], filters)][:n]
        out.append(kept)
    return out


def test_filtered_query_equals_the_post_filter_of_the_full_ranking(colmod):
    rng = np.random.Generator(np.random.Philox(3))
    col = colmod.FlatCollection("t")
    n = 300
    v = _vecs(n, seed=1)
    metas = []
    for i in range(n):
        if i % 37 == 0:
            metas.append({"filter_results_json": "not json"})
        elif i % 41 == 0:
            metas.append(None)
        else:
            metas.append(_meta({"outdoor": rng.choice(["Yes", " yes ", "no", "YES"]), "night": rng.choice(["yes", "no", "no"])}))
    col.add(ids=[f"i{i}" for i in range(n)], embeddings=v, metadatas=metas)
    assert TaggedOracleIndex.instances[0].pushes == []          # nothing is pushed at add time
    q = _vecs(4, seed=2)
    for filters in (["outdoor"], ["night"], ["outdoor", "night"], ["night", "night"]):
        got = col.query(query_embeddings=q, n_results=10, include=["metadatas", "distances"], filters=filters)
        want = _post_filter(col, q, 10, filters)
        for qi in range(4):
            assert got["ids"][qi] == [i for i, _ in want[qi]]
            assert got["distances"][qi] == [d for _, d in want[qi]]
            assert len(got["ids"][qi]) == 10                      # the post-filter of the 10 nearest has fewer
    idx = TaggedOracleIndex.instances[0]
    assert len(idx.pushes) == 1 and len(idx.pushes[0]) == n      # one push of every row, at the first filtered query
    # filters=None / [] are the unfiltered query
    assert col.query(query_embeddings=q, n_results=5, filters=[])["ids"] == col.query(query_embeddings=q, n_results=5)["ids"]


def test_bits_follow_first_appearance_in_label_order(colmod):
    col = colmod.FlatCollection("t")
    col.add(ids=["a", "b", "c"], embeddings=_vecs(3),
            metadatas=[_meta({"zeta": "no"}), _meta({"alpha": "yes", "zeta": "yes"}), _meta({"mid": "yes", "alpha": "no"})])
    col.query(query_embeddings=_vecs(1), n_results=1, filters=["alpha"])
    assert col._filter_bits == {"zeta": 0, "alpha": 1, "mid": 2}
    idx = TaggedOracleIndex.instances[0]
    assert idx.get_tags([0, 1, 2]).tolist() == [0, 0b11, 0b100]


def test_dirty_tags_are_pushed_at_the_next_filtered_query_only(colmod, tmp_path):
    d = str(tmp_path)
    col = colmod.FlatCollection("t", persist_dir=d)
    col.add(ids=["a", "b", "c", "d"], embeddings=_vecs(4), metadatas=[_meta({"x": "yes"}), _meta({"x": "no"}), None, _meta({"x": "yes"})])
    idx = TaggedOracleIndex.instances[-1]
    assert col.query(query_embeddings=_vecs(1, seed=5), n_results=4, filters=["x"])["ids"][0] and len(idx.pushes) == 1
    assert sorted(col.query(query_embeddings=_vecs(1, seed=5), n_results=4, filters=["x"])["ids"][0]) == ["a", "d"]
    assert len(idx.pushes) == 1                                    # nothing changed, nothing pushed
    col.update(ids=["b"], metadatas=[_meta({"x": "yes"})])         # metadata change: dirty
    col.update(ids=["a"], documents=["doc"])                       # no metadata change: not dirty
    col.add(ids=["e"], embeddings=_vecs(1, seed=9), metadatas=[_meta({"x": "Yes"})])
    col.delete(ids=["d"])
    assert len(idx.pushes) == 1                                    # mutations never push
    got = col.query(query_embeddings=_vecs(1, seed=5), n_results=10, filters=["x"])["ids"][0]
    assert sorted(got) == ["a", "b", "e"]
    assert idx.pushes[-1] == {col._by_id["b"]: 1, col._by_id["e"]: 1}
    # unfiltered queries never push either
    col.update(ids=["c"], metadatas=[_meta({"x": "yes"})])
    col.query(query_embeddings=_vecs(1, seed=5), n_results=10)
    assert len(idx.pushes) == 2
    col.persist()
    # reload: snapshot + journal; the index comes back with tags 0 and every row is pushed at the first filtered query
    col.update(ids=["a"], metadatas=[_meta({"x": "no", "y": "yes"})])
    col2 = colmod.FlatCollection("t", persist_dir=d)
    idx2 = TaggedOracleIndex.instances[-1]
    assert idx2 is not idx and idx2.pushes == []
    got = col2.query(query_embeddings=_vecs(1, seed=5), n_results=10, filters=["x"])["ids"][0]
    assert sorted(got) == ["b", "c", "e"]
    assert len(idx2.pushes) == 1 and len(idx2.pushes[0]) == col2.count()
    assert col2.query(query_embeddings=_vecs(1, seed=5), n_results=10, filters=["y"])["ids"][0] == ["a"]


def test_unknown_filter_names_admit_nothing(colmod):
    col = colmod.FlatCollection("t")
    col.add(ids=["a", "b"], embeddings=_vecs(2), metadatas=[_meta({"x": "yes"}), _meta({"y": "no"})])
    out = col.query(query_embeddings=_vecs(2, seed=3), n_results=5, filters=["x", "never"], include=["distances", "metadatas"])
    assert out["ids"] == [[], []] and out["distances"] == [[], []] and out["metadatas"] == [[], []]
    assert col.query(query_embeddings=_vecs(1, seed=3), n_results=5, filters=["y"])["ids"] == [[]]   # answered, never "yes"
    assert col.query(query_embeddings=_vecs(1, seed=3), n_results=5, filters=["x"])["ids"] == [["a"]]


def test_more_than_64_filter_names_fall_back_to_an_exact_host_path(colmod):
    rng = np.random.Generator(np.random.Philox(8))
    col = colmod.FlatCollection("t")
    n = 160
    metas = []
    for i in range(n):
        ans = {f"f{j}": "yes" for j in range(70) if (i + j) % 3 == 0}
        ans["common"] = "yes" if rng.random() < 0.7 else "no"
        metas.append(_meta(ans))
    col.add(ids=[f"i{i}" for i in range(n)], embeddings=_vecs(n, seed=4), metadatas=metas)
    q = _vecs(3, seed=6)
    for filters in (["f69"], ["f69", "common"], ["f1", "common"], ["f68", "f67"]):
        got = col.query(query_embeddings=q, n_results=7, include=["metadatas", "distances"], filters=filters)
        assert len(col._filter_bits) == 64 and col._filter_overflow
        want = _post_filter(col, q, 7, filters)
        for qi in range(3):
            assert got["ids"][qi] == [i for i, _ in want[qi]], filters
            assert got["distances"][qi] == [d for _, d in want[qi]]


# ---------------------------------------------------------------------------------------------------- API

def _png(seed, size=(90, 70)):
    from PIL import Image

    rng = np.random.Generator(np.random.Philox(seed))
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, size=(size[1], size[0], 3), dtype=np.uint8)).save(buf, format="PNG")
    return buf.getvalue()


class _Proc:
    def __init__(self, shape):
        self.shape = shape

    def preprocess_images(self, images):
        from oracle import clip_oracle as co

        return np.stack([co.preprocess_image(im, self.shape.v_image) for im in images])

    def rgb_arrays(self, images):
        return [np.asarray(im.convert("RGB") if hasattr(im, "convert") else im, dtype=np.uint8) for im in images]

    def tokenize(self, texts):
        from oracle import clip_oracle as co

        s = self.shape
        return np.stack([co.synthetic_text_ids(1, s.t_ctx, s.t_vocab, s.eos_token_id, seed=sum(map(ord, t)) % 9973)[0] for t in texts])


@pytest.fixture()
def client(monkeypatch):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from starlette.testclient import TestClient

    import mmiss_amd  # noqa: F401
    from mmiss_amd import api, collection, search, utils
    from oracle import clip_oracle as co

    monkeypatch.setattr(collection, "FlatIndex", TaggedOracleIndex)
    monkeypatch.setattr(search, "blend", lambda i, t, w: ro.blend(i, t, w))
    utils.set_clip_model(OracleEncoder(co.TINY), _Proc(co.TINY))
    search.set_collection(collection.FlatCollection("t"))
    yield TestClient(api.create_app())
    utils.set_clip_model(None, None)
    search.set_collection(None)


def test_prefilter_returns_limit_results_where_the_post_filter_returns_fewer(client):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import search

    imgs = [_png(200 + i) for i in range(12)]
    ids = [client.post("/api/upload", files={"file": (f"{i}.png", d, "image/png")}).json()["metadata"]["id"] for i, d in enumerate(imgs)]
    col = search._collection()
    q = {"file": ("q.png", imgs[0], "image/png")}
    for route, data, files in (("/api/search/image", {}, q), ("/api/search/text", {"query": "drill"}, None),
                               ("/api/search/multimodal", {"query": "drill", "weight_image": "0.5"}, q)):
        # the 5 images this route ranks last answer "yes", the others "no"
        full = [r["id"] for r in client.post(route, data=dict(data, limit="12"), files=files).json()["results"]]
        assert sorted(full) == sorted(ids)
        yes = set(full[-5:])
        for iid in ids:
            col.update(ids=[iid], metadatas=[_meta({"is red": "yes" if iid in yes else "no"})])
        base = dict(data, limit="3", filters=["is red"])
        post = client.post(route, data=base, files=files).json()["results"]
        pre = client.post(route, data=dict(base, prefilter="true"), files=files).json()["results"]
        assert post == []                                                  # the reference's post-filter of the 3 nearest
        assert [r["id"] for r in pre] == full[-5:-2], route                # the 3 nearest among the images that pass
        assert client.post(route, data=dict(base, prefilter="1"), files=files).json()["results"] == pre
        assert client.post(route, data=dict(base, prefilter="0"), files=files).json()["results"] == post

"""The host layers of assignment and clustering without a GPU, on an oracle-backed stand-in for FlatIndex.assign / cluster_sums:
FlatIndex.kmeans (the product's own loop, over the stand-in's calls) against assign_cases.expected_kmeans, FlatCollection.assign /
cluster, search.classify_collection / cluster_collection, and the argument checks FlatIndex makes before it calls the library."""
import threading

import numpy as np
import pytest

import assign_cases as ac
from radius_fakes import OracleRadiusIndex

D = 128


class OracleAssignIndex(OracleRadiusIndex):
    """OracleRadiusIndex with the two assignment calls, answered by the restatement, and FlatIndex's own kmeans on top of them"""
    instances = []
    MAX_CENTRES = 1024

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._call_lock = threading.RLock()
        self.assign_calls = []           # (C, want_dist) of every assign call
        self.sum_calls = 0
        OracleAssignIndex.instances.append(self)

    def assign(self, centres, want_dist=True):
        c = np.asarray(centres, np.float32).reshape(-1, self.dim)
        if not 1 <= c.shape[0] <= 1024:
            raise RuntimeError("1 .. 1024 centres")
        self.assign_calls.append((c.shape[0], bool(want_dist)))
        if self.labs.size == 0:
            return np.zeros(0, np.int32), (np.zeros(0, np.float32) if want_dist else None), np.zeros(c.shape[0], np.int64)
        a, d, s = ac.expected_assign(c, self.rows)
        return a, (d if want_dist else None), s

    def cluster_sums(self, assign, n_clusters):
        self.sum_calls += 1
        assert np.asarray(assign).shape == self.labs.shape
        return ac.expected_sums(ac.represented(self.rows), assign, int(n_clusters))

    def kmeans(self, n_clusters, iters=10, init=None):
        from mmiss_amd.index import FlatIndex

        return FlatIndex.kmeans(self, n_clusters, iters, init)


def _index(dtype, x):
    import mmiss_amd  # noqa: F401

    idx = OracleAssignIndex(x.shape[1], dtype)
    idx.add(x, np.arange(x.shape[0], dtype=np.int64) * 3 + 5)
    return idx


def _same(out, exp):
    assert out["iterations"] == exp["iterations"]
    assert np.array_equal(out["centres"].view(np.uint32), exp["centres"].view(np.uint32))
    assert ac.mismatch((out["assign"], out["dist"], out["sizes"]), (exp["assign"], exp["dist"], exp["sizes"])) is None


@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_kmeans_default_init_equals_the_restatement(dtype):
    k = ac.KMEANS
    x = ac.kmeans_corpus()
    idx = _index(dtype, x)
    out = idx.kmeans(k["C"], iters=k["iters"])
    exp = ac.expected_kmeans(ac.stored_of(x, dtype), k["C"], k["iters"])
    _same(out, exp)
    assert exp["iterations"] >= 2
    # every loop assign runs without distances, the last one with: the returned assignment belongs to the returned centres
    assert [w for _, w in idx.assign_calls[:-1]] == [False] * (len(idx.assign_calls) - 1) and idx.assign_calls[-1] == (k["C"], True)
    assert ac.mismatch((out["assign"], out["dist"], out["sizes"]), ac.expected_assign(out["centres"], ac.stored_of(x, dtype))) is None


def test_kmeans_init_by_labels_early_stop_and_empty_clusters():
    k = ac.KMEANS
    x = ac.kmeans_corpus()
    idx = _index("f16", x)
    st = ac.stored_of(x, "f16")
    # init by labels, with one label twice: cluster 1 starts empty and keeps its centre through the first update
    pos = np.array([0, 0] + list(range(100, 100 + k["C"] - 2)))
    out = idx.kmeans(k["C"], iters=1, init=pos * 3 + 5)
    exp = ac.expected_kmeans(st, k["C"], 1, init_pos=pos)
    _same(out, exp)
    assert np.array_equal(out["centres"][1], ac.represented(st)[0]) and (exp["history"][0] != 1).all()
    # early stop: with room for 40 iterations the loop ends by itself, one assign after the last update sees no change
    n0, s0 = len(idx.assign_calls), idx.sum_calls
    out = idx.kmeans(k["C"], iters=40)
    exp = ac.expected_kmeans(st, k["C"], 40)
    _same(out, exp)
    assert out["iterations"] < 40
    assert idx.sum_calls - s0 == out["iterations"] and len(idx.assign_calls) - n0 == out["iterations"] + 2
    # iters = 0: the initial centres, assigned once
    out = idx.kmeans(3, iters=0)
    _same(out, ac.expected_kmeans(st, 3, 0))
    assert out["iterations"] == 0
    with pytest.raises(ValueError, match="init"):
        idx.kmeans(3, init=[5, 8])
    with pytest.raises(ValueError, match="n_clusters"):
        idx.kmeans(0)
    with pytest.raises(ValueError, match="n_clusters"):
        idx.kmeans(1025)


@pytest.fixture()
def colmod(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection

    OracleAssignIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleAssignIndex)
    return collection


def _ids(n):
    return [f"im{i:03d}" for i in range(n)]


def test_collection_assign_and_cluster_map_rows_to_ids(colmod, tmp_path):
    x, c = ac.random_corpus(21, 60, D, 5)
    col = colmod.FlatCollection("t", persist_dir=str(tmp_path))
    col.persist()
    ids0, a0, d0, s0 = col.assign(c)                                    # an empty collection: nothing to assign
    assert ids0 == [] and a0.shape == (0,) and s0.tolist() == [0] * 5
    col.add(ids=_ids(60), embeddings=x, metadatas=[{"id": i} for i in _ids(60)])
    col.delete(ids=["im010"])                                           # row positions shift: ids follow the rows
    keep = [i for i in range(60) if i != 10]
    journal = open(col._journal_paths(col._index_gen)[0]).read()
    ids, a, d, s = col.assign(c)
    exp = ac.expected_assign(c, ac.stored_of(x, "f32")[keep])
    assert ids == [_ids(60)[i] for i in keep]
    assert ac.mismatch((a, d, s), exp) is None
    assert (a[[ids.index("im003"), ids.index("im017")]] == -1).all()    # rows without a direction
    out = col.cluster(4, iters=3, init_ids=["im000", "im020", "im040", "im059"])
    pos = [keep.index(i) for i in (0, 20, 40, 59)]
    expk = ac.expected_kmeans(ac.stored_of(x, "f32")[keep], 4, 3, init_pos=pos)
    assert out["ids"] == ids
    _same(out, expk)
    # neither call writes anything: the journal and the metadata are what they were
    assert open(col._journal_paths(col._index_gen)[0]).read() == journal
    assert col.get(ids=["im000"])["metadatas"][0] == {"id": "im000"}
    with pytest.raises(ValueError):
        col.assign(np.zeros((2, 64), np.float32))
    with pytest.raises(ValueError):
        colmod.FlatCollection("empty").cluster(3)


def test_classify_and_cluster_collection(colmod, monkeypatch):
    from mmiss_amd import search, utils

    x, c = ac.random_corpus(21, 60, D, 5)
    col = colmod.FlatCollection("t")
    col.add(ids=_ids(60), embeddings=x, metadatas=[{"id": i} for i in _ids(60)])
    search.set_collection(col)
    prompts = [f"a photo of thing {i}" for i in range(5)]
    monkeypatch.setattr(utils, "load_clip_model", lambda: (None, None))
    monkeypatch.setattr(utils, "generate_clip_embedding",
                        lambda image=None, text=None, model=None, processor=None: {"text": c[prompts.index(text)][None]})
    try:
        idx = OracleAssignIndex.instances[-1]
        res = search.classify_collection(prompts)
        assert idx.assign_calls == [(5, True)]                          # ONE assign decides every image
        a, d, s = ac.expected_assign(c, ac.stored_of(x, "f32"))
        assert [r[0] for r in res] == _ids(60) and [r[1] for r in res] == a.tolist()
        for r, ai, di in zip(res, a.tolist(), d.tolist()):
            assert r[2] == (1 - float(di) / 2 if ai >= 0 else None)     # similarity = 1 - d / 2 in Python floats on the float32 distance
        assert res[3][1:] == (-1, None) and all(r[1] != 1 for r in res)   # no direction: -1 / None; the empty prompt's centre is never chosen
        with pytest.raises(ValueError):
            search.classify_collection([])
        mapping, sizes = search.cluster_collection(4, iters=3)
        expk = ac.expected_kmeans(ac.stored_of(x, "f32"), 4, 3)
        assert mapping == dict(zip(_ids(60), expk["assign"].tolist())) and sizes == expk["sizes"].tolist()
        assert mapping["im003"] == -1 and sum(sizes) == 55
    finally:
        search.set_collection(None)


class _NoLibrary:
    """what FlatIndex needs of the library before it calls it: nothing — every call here is a bug of the wrapper"""
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} with arguments it should have refused")


def test_wrapper_argument_checks_come_before_the_call():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.index import FlatIndex

    idx = FlatIndex.__new__(FlatIndex)               # no device here: the checks under test run before any library call
    idx.dim, idx.dtype, idx.device, idx._h, idx._lib, idx._call_lock = D, 0, 0, None, _NoLibrary(), threading.RLock()
    idx.count = lambda: 10
    with pytest.raises(ValueError, match="centres"):
        idx.assign(np.zeros((0, D), np.float32))
    with pytest.raises(ValueError, match="centres"):
        idx.assign(np.zeros((1025, D), np.float32))
    with pytest.raises(ValueError, match="vectors"):
        idx.assign(np.zeros((3, D + 1), np.float32))
    with pytest.raises(ValueError, match="assign"):
        idx.cluster_sums(np.zeros(9, np.int32), 3)   # the wrong length
    with pytest.raises(ValueError, match="assign"):
        idx.cluster_sums(np.zeros((10, 1), np.int32), 3)
    with pytest.raises(TypeError, match="assign"):
        idx.cluster_sums(np.zeros(10, np.float32), 3)
    with pytest.raises(ValueError, match="n_clusters"):
        idx.cluster_sums(np.zeros(10, np.int32), 0)
    with pytest.raises(ValueError, match="n_clusters"):
        idx.cluster_sums(np.zeros(10, np.int32), 1025)
    with pytest.raises(ValueError, match="n_clusters"):
        idx.kmeans(1025)
    idx._h = None                                    # (nothing to destroy)

"""The host layers of partitioned search without a GPU, on an oracle-backed stand-in for FlatIndex's partition calls: the product's
own FlatIndex.build_partition (kmeans then set_partition, over the stand-in's calls), FlatCollection.query(n_probe=) with its
routing — the probed query with a partition, the silent exact answer without one, with max_distance= or with more than 64 filter
names —, FlatCollection.build_partition / partition_info, the search wrappers that pass n_probe through, and the argument checks
FlatIndex makes before it calls the library. Nothing of it is journaled."""
import threading

import numpy as np
import pytest

import assign_cases as ac
import partition_cases as pc
from test_assign_layers_cpu import OracleAssignIndex

D = 128


class OraclePartitionIndex(OracleAssignIndex):
    """OracleAssignIndex with the partition calls answered by the restatement, and FlatIndex's own build_partition on top"""
    instances = []
    PARTITION_INFO_FIELDS = ("cells", "rows", "tail", "rows_in_cells", "largest_cell", "empty_cells", "queries", "scanned")

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.part = None
        self.probed_calls = []           # (Q, k, nprobe, masked) of every probed call
        self.flat_calls = 0
        OraclePartitionIndex.instances.append(self)

    def set_partition(self, centres, cells):
        c = np.asarray(centres, np.float32).reshape(-1, self.dim)
        cells = np.asarray(cells, np.int32)
        if cells.shape != self.labs.shape:
            raise RuntimeError("one cell per row")
        self.part = dict(centres=c.copy(), cells=cells.copy(), B=int(self.labs.size), queries=0, scanned=0)

    def clear_partition(self):
        self.part = None

    def partition_info(self):
        if self.part is None:
            return dict.fromkeys(self.PARTITION_INFO_FIELDS, 0)
        s = pc.cell_sizes(self.part["cells"], self.part["centres"].shape[0])
        return dict(zip(self.PARTITION_INFO_FIELDS, (int(s.shape[0]), self.part["B"], int(self.labs.size) - self.part["B"], int(s.sum()), int(s.max()),
                                                     int((s == 0).sum()), self.part["queries"], self.part["scanned"])))

    def build_partition(self, n_cells, iters=10, init=None):
        from mmiss_amd.index import FlatIndex

        return FlatIndex.build_partition(self, n_cells, iters, init)

    def query_probed(self, queries, k, nprobe, require=None, exclude=None):
        if self.part is None:
            raise RuntimeError("no partition")
        q = np.asarray(queries, np.float32).reshape(-1, self.dim)
        self.probed_calls.append((q.shape[0], k, nprobe, require is not None or exclude is not None))
        tags = np.array([self.tags.get(int(l), 0) for l in self.labs], np.uint64)
        out = pc.expected_probed(q, k, nprobe, self.part["centres"], self.part["cells"], self.part["B"], self.rows, self.labs, tags, require, exclude)
        self.part["queries"] += q.shape[0]
        self.part["scanned"] += int(out[3].sum())
        return out

    def query(self, q, k, require=None, exclude=None):
        self.flat_calls += 1
        return super().query(q, k, require, exclude)

    def update(self, labels, vecs):
        self.part = None
        return super().update(labels, vecs)

    def remove(self, labels):
        self.part = None
        return super().remove(labels)


def _index(dtype, x):
    import mmiss_amd  # noqa: F401

    idx = OraclePartitionIndex(x.shape[1], dtype)
    idx.add(x, pc.labels_of(x.shape[0]))
    return idx


def test_build_partition_is_kmeans_then_set_partition_under_one_lock():
    k = ac.KMEANS
    x = ac.kmeans_corpus()
    idx = _index("f16", x)
    seen = []
    lock = idx._call_lock

    class Spy:
        """the handle's lock, recording how deep it is held when a call on the index starts"""
        depth = 0

        def __enter__(self):
            lock.acquire()
            Spy.depth += 1

        def __exit__(self, *exc):
            Spy.depth -= 1
            lock.release()

    idx._call_lock = Spy()
    real_set = idx.set_partition
    idx.set_partition = lambda c, a: (seen.append(("set", Spy.depth)), real_set(c, a))[1]
    real_assign = idx.assign
    idx.assign = lambda c, want_dist=True: (seen.append(("assign", Spy.depth)), real_assign(c, want_dist))[1]
    info = idx.build_partition(k["C"], iters=k["iters"])
    exp = ac.expected_kmeans(ac.stored_of(x, "f16"), k["C"], k["iters"])
    assert np.array_equal(idx.part["centres"].view(np.uint32), exp["centres"].view(np.uint32))
    assert np.array_equal(idx.part["cells"], exp["assign"])
    assert info == idx.partition_info() and info["cells"] == k["C"] and info["rows"] == x.shape[0] and info["tail"] == 0
    assert info["rows_in_cells"] == int(exp["sizes"].sum())
    assert seen[-1][0] == "set" and all(depth >= 1 for _, depth in seen)     # every call of the unit ran with the handle's lock held
    with pytest.raises(ValueError, match="n_clusters"):
        idx.build_partition(1025)


@pytest.fixture()
def colmod(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection

    OraclePartitionIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OraclePartitionIndex)
    return collection


def _ids(n):
    return [f"im{i:03d}" for i in range(n)]


def _filled(colmod, tmp_path=None, n=300, filters=1):
    p = pc.clustered(31, n, D, 7, 4, complete=True)
    col = colmod.FlatCollection("t", persist_dir=str(tmp_path) if tmp_path else None)
    if tmp_path:
        col.persist()
    import json

    metas = [{"id": i, "filter_results_json": json.dumps({f"f{j}": "yes" if (r + j) % 2 else "no" for j in range(filters)})}
             for r, i in enumerate(_ids(n))]
    col.add(ids=_ids(n), embeddings=p["x"], metadatas=metas)
    return col, p


def test_collection_query_routes_n_probe(colmod, tmp_path):
    col, p = _filled(colmod, tmp_path)
    idx = OraclePartitionIndex.instances[-1]
    q = p["queries"][:2]
    flat = col.query(query_embeddings=q, n_results=5)
    # no partition: n_probe is ignored, the exact answer, never an error
    assert col.partition_info()["cells"] == 0
    assert col.query(query_embeddings=q, n_results=5, n_probe=1) == flat and idx.probed_calls == []
    journal = open(col._journal_paths(col._index_gen)[0]).read()
    info = col.build_partition(7, iters=3)
    assert info["cells"] == 7 and col.partition_info() == info
    # with a partition: the probed query, the ids of the restatement's labels
    n0 = idx.flat_calls
    got = col.query(query_embeddings=q, n_results=5, n_probe=1)
    assert idx.probed_calls == [(2, 5, 1, False)] and idx.flat_calls == n0
    exp = pc.expected_probed(q, 5, 1, idx.part["centres"], idx.part["cells"], 300, idx.rows, idx.labs)
    assert got["ids"] == [[_ids(300)[int(l)] for l in exp[0][i, :exp[2][i]]] for i in range(2)]
    assert got["distances"] == [[float(d) for d in exp[1][i, :exp[2][i]]] for i in range(2)]
    assert col.query(query_embeddings=q, n_results=5, n_probe=7) == flat            # every cell probed: the flat answer
    # without n_probe, and with max_distance: the flat / radius path as before
    n_probed = len(idx.probed_calls)
    assert col.query(query_embeddings=q, n_results=5) == flat
    col.query(query_embeddings=q, n_results=5, max_distance=0.5, n_probe=1)
    assert len(idx.probed_calls) == n_probed and idx.radius_calls[-1][0] == "query"
    # filters: the probed query with the filter's bit required
    got = col.query(query_embeddings=q, n_results=5, filters=["f0"], n_probe=2)
    assert idx.probed_calls[-1] == (2, 5, 2, True)
    tags = np.array([idx.tags.get(int(l), 0) for l in idx.labs], np.uint64)
    exp = pc.expected_probed(q, 5, 2, idx.part["centres"], idx.part["cells"], 300, idx.rows, idx.labs, tags, np.uint64(1))
    assert got["ids"] == [[_ids(300)[int(l)] for l in exp[0][i, :exp[2][i]]] for i in range(2)]
    with pytest.raises(ValueError, match="n_probe"):
        col.query(query_embeddings=q, n_results=5, n_probe=0)
    # nothing of all this was journaled or written to the metadata
    assert open(col._journal_paths(col._index_gen)[0]).read() == journal
    assert col.get(ids=["im000"])["metadatas"][0]["id"] == "im000"
    # rows added afterwards are tail; an update drops the partition and the queries run flat again
    col.add(ids=["new"], embeddings=p["x"][7:8], metadatas=[{"id": "new"}])
    assert col.partition_info()["tail"] == 1 and col.partition_info()["cells"] == 7
    col.update(ids=["im001"], embeddings=p["x"][2:3])
    assert col.partition_info()["cells"] == 0
    n_probed = len(idx.probed_calls)
    col.query(query_embeddings=q, n_results=5, n_probe=1)
    assert len(idx.probed_calls) == n_probed
    with pytest.raises(ValueError):
        colmod.FlatCollection("empty").build_partition(3)
    assert colmod.FlatCollection("empty").partition_info()["cells"] == 0


def test_more_than_64_filter_names_run_exactly(colmod):
    col, p = _filled(colmod, filters=66)
    idx = OraclePartitionIndex.instances[-1]
    col.build_partition(7, iters=2)
    q = p["queries"][:1]
    exact = col.query(query_embeddings=q, n_results=5, filters=["f65"])
    n_probed = len(idx.probed_calls)
    assert col.query(query_embeddings=q, n_results=5, filters=["f65"], n_probe=1) == exact      # a name past the 64th bit: exact
    assert len(idx.probed_calls) == n_probed
    col.query(query_embeddings=q, n_results=5, filters=["f3"], n_probe=1)                       # a mapped name: probed
    assert len(idx.probed_calls) == n_probed + 1


def test_search_wrappers_pass_n_probe_through(colmod, monkeypatch):
    from mmiss_amd import search, utils

    col, p = _filled(colmod)
    idx = OraclePartitionIndex.instances[-1]
    search.set_collection(col)
    monkeypatch.setattr(utils, "load_clip_model", lambda: (None, None))
    monkeypatch.setattr(utils, "generate_clip_embedding",
                        lambda image=None, text=None, model=None, processor=None: {"text": p["queries"][:1], "image": p["queries"][1:2]})
    monkeypatch.setattr(search, "blend", lambda a, b, w: np.asarray(a, np.float32))
    try:
        info = search.build_search_partition(7, iters=2)
        assert info["cells"] == 7 and idx.part is not None
        exact = search.search_similar(p["queries"][0], limit=5)
        assert len(exact) == 5 and idx.probed_calls == []
        assert len(search.search_similar(p["queries"][0], limit=5, n_probe=2)) == 5 and idx.probed_calls[-1] == (1, 5, 2, False)
        assert search.search_similar(p["queries"][0], limit=5, n_probe=7) == exact
        assert len(search.search_similar_batch(p["queries"][:3], limit=4, n_probe=3)) == 3 and idx.probed_calls[-1] == (3, 4, 3, False)
        search.search_by_text("a cat", limit=5, n_probe=1)
        assert idx.probed_calls[-1] == (1, 5, 1, False)
        search.search_multimodal(None, "a cat", 0.5, limit=5, n_probe=4)
        assert idx.probed_calls[-1] == (1, 5, 4, False)
        search.search_multimodal_batch(p["queries"][:2], p["queries"][:2], 0.5, limit=5, n_probe=5, filters=["f0"])
        assert idx.probed_calls[-1] == (2, 5, 5, True)
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
    q = np.zeros((2, D), np.float32)
    with pytest.raises(ValueError, match="k"):
        idx.query_probed(q, 0, 1)
    with pytest.raises(ValueError, match="k"):
        idx.query_probed(q, 2041, 1)
    with pytest.raises(ValueError, match="nprobe"):
        idx.query_probed(q, 10, 0)
    with pytest.raises(ValueError, match="vectors"):
        idx.query_probed(np.zeros((2, D + 1), np.float32), 10, 1)
    with pytest.raises(ValueError, match="query"):
        idx.query_probed(np.zeros((0, D), np.float32), 10, 1)
    with pytest.raises(ValueError, match="require"):
        idx.query_probed(q, 10, 1, require=np.zeros(3, np.uint64))
    with pytest.raises(ValueError, match="centres"):
        idx.set_partition(np.zeros((0, D), np.float32), np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="centres"):
        idx.set_partition(np.zeros((1025, D), np.float32), np.zeros(5, np.int32))
    with pytest.raises(TypeError, match="cells"):
        idx.set_partition(np.zeros((3, D), np.float32), np.zeros(5, np.float32))
    with pytest.raises(ValueError, match="cells"):
        idx.set_partition(np.zeros((3, D), np.float32), np.zeros((5, 1), np.int32))
    idx._h = None                                    # (nothing to destroy)

"""The host layers of similarity filters without a GPU, on an oracle-backed stand-in for FlatIndex.membership / tag_by_radius:
FlatCollection.add_similarity_filter (every row answered, journaled, reloaded, feeding query(filters=), beside other answers),
search.apply_text_filter / apply_image_filter (the similarity -> distance conversion), and the argument checks FlatIndex makes
before it calls the library."""
import json

import numpy as np
import pytest

from oracle import retrieval_oracle as ro
from radius_fakes import OracleRadiusIndex

D = 128


class OracleMembershipIndex(OracleRadiusIndex):
    """OracleRadiusIndex with the two membership calls, answered by the oracle's distances"""
    instances = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.membership_calls = []
        OracleMembershipIndex.instances.append(self)

    def _members(self, queries, max_dist):
        q = np.asarray(queries, np.float32).reshape(-1, self.dim)
        R = np.broadcast_to(np.asarray(max_dist, np.float32), (q.shape[0],))
        if np.isnan(R).any():
            raise RuntimeError("max_dist is NaN")
        if not 1 <= q.shape[0] <= 64:
            raise RuntimeError("1 .. 64 probes")
        if self.labs.size == 0:
            return np.zeros((q.shape[0], 0), bool)
        with np.errstate(all="ignore"):
            return ro.distances(q, self.rows) <= R[:, None]

    def membership(self, queries, max_dist):
        mem = self._members(queries, max_dist)
        self.membership_calls.append((mem.shape[0], np.asarray(max_dist, np.float32).copy()))
        words = np.zeros(mem.shape[1], np.uint64)
        for p in range(mem.shape[0]):
            words |= mem[p].astype(np.uint64) << np.uint64(p)
        return words, mem.sum(1).astype(np.int64)

    def tag_by_radius(self, queries, max_dist, bits):
        mem = self._members(queries, max_dist)
        for r, lab in enumerate(self.labs.tolist()):
            t = self.tags.get(lab, 0)
            for p, b in enumerate(bits):
                t = (t & ~(1 << int(b))) | (int(mem[p, r]) << int(b))
            self.tags[lab] = t
        return mem.sum(1).astype(np.int64)


def _rows(n=30, seed=3):
    return np.random.Generator(np.random.Philox(seed)).standard_normal((n, D)).astype(np.float32)


def _ids(n):
    return [f"im{i:02d}" for i in range(n)]


@pytest.fixture()
def colmod(monkeypatch):
    import mmiss_amd  # noqa: F401
    from mmiss_amd import collection

    OracleMembershipIndex.instances = []
    monkeypatch.setattr(collection, "FlatIndex", OracleMembershipIndex)
    return collection


def _expected_yes(v, probe, R, dtype="f32"):
    return (ro.distances(probe[None], ro.normalize_rows(v, dtype))[0] <= np.float32(R)).tolist()


def test_add_similarity_filter_answers_every_row(colmod):
    v = _rows()
    col = colmod.FlatCollection("t")
    assert col.add_similarity_filter("dog", v[0], 0.9) == 0                     # an empty collection: nothing to answer
    metas = [{"id": i, "filter_results_json": json.dumps({"even": "yes" if k % 2 == 0 else "no"})} for k, i in enumerate(_ids(30))]
    metas[7] = None                                                              # a row without metadata
    metas[8] = {"id": "im08", "filter_results_json": "not json"}                # ... and one with unparseable answers
    col.add(ids=_ids(30), embeddings=v, metadatas=metas)
    probe = v[4] + 0.5 * v[9]
    R = 0.95
    yes = _expected_yes(v, probe, R)
    assert 2 < sum(yes) < 28
    idx = OracleMembershipIndex.instances[-1]
    assert col.add_similarity_filter("dog", probe, R) == sum(yes)
    assert len(idx.membership_calls) == 1 and idx.membership_calls[0][0] == 1   # ONE call decides every row
    got = col.get(include=["metadatas"])
    for k, m in enumerate(got["metadatas"]):
        answers = json.loads(m["filter_results_json"])
        assert answers["dog"] == ("yes" if yes[k] else "no"), k
        if k not in (7, 8):
            assert answers["even"] == ("yes" if k % 2 == 0 else "no") and m["id"] == f"im{k:02d}"      # what was there stays
    # it feeds the filtered query: exact top-k among the "yes" rows, alone and combined with a stored answer
    q = v[11:12]
    want = [i for i in col.query(query_embeddings=q, n_results=30)["ids"][0] if yes[int(i[2:])]]
    assert col.query(query_embeddings=q, n_results=30, filters=["dog"])["ids"][0] == want
    both = col.query(query_embeddings=q, n_results=30, filters=["dog", "even"])["ids"][0]
    assert both == [i for i in want if int(i[2:]) % 2 == 0 and int(i[2:]) not in (7, 8)] and both
    # api.apply_filters reads the same answers
    from mmiss_amd import api

    kept = api.apply_filters([dict(m) for m in got["metadatas"]], ["dog"])
    assert [m.get("id") for m in kept if m.get("id")] == [f"im{k:02d}" for k in range(30) if yes[k] and k not in (7, 8)]
    # running it again refreshes: another radius, rows added in between get their answer
    col.add(ids=["late"], embeddings=probe[None], metadatas=[{"id": "late"}])
    assert "filter_results_json" not in col.get(ids=["late"])["metadatas"][0]
    assert col.query(query_embeddings=q, n_results=31, filters=["dog"])["ids"][0] == want          # no answer yet: not admitted
    n2 = col.add_similarity_filter("dog", probe, 0.5)
    yes2 = _expected_yes(np.concatenate([v, probe[None]]), probe, 0.5)
    assert n2 == sum(yes2) and yes2[-1] and n2 < sum(yes)
    assert sorted(col.query(query_embeddings=q, n_results=31, filters=["dog"])["ids"][0]) == sorted(
        (_ids(30) + ["late"])[k] for k in range(31) if yes2[k])
    with pytest.raises(ValueError):
        col.add_similarity_filter("dog", v[:2], 0.5)
    with pytest.raises(ValueError):
        col.add_similarity_filter("dog", np.zeros(64, np.float32), 0.5)


def test_similarity_filter_is_journaled_and_survives_a_reopen(colmod, tmp_path):
    d = str(tmp_path)
    v = _rows(12, seed=4)
    col = colmod.FlatCollection("t", persist_dir=d)
    col.persist()
    col.add(ids=_ids(12), embeddings=v, metadatas=[{"id": i} for i in _ids(12)])
    probe = v[2] + v[3]
    yes = _expected_yes(v, probe, 0.9)
    assert 0 < sum(yes) < 12
    assert col.add_similarity_filter("pair", probe, 0.9) == sum(yes)
    jl = col._journal_paths(col._index_gen)[0]
    last = json.loads(open(jl).read().splitlines()[-1])
    assert last["op"] == "update" and last["ids"] == _ids(12)                   # one journal record, through update()
    assert [json.loads(m["filter_results_json"])["pair"] for m in last["metadatas"]] == ["yes" if y else "no" for y in yes]
    col2 = colmod.FlatCollection("t", persist_dir=d)                            # snapshot + journal replay
    assert col2.count() == 12
    got = col2.query(query_embeddings=v[5:6], n_results=12, filters=["pair"])["ids"][0]
    assert sorted(got) == [i for i, y in zip(_ids(12), yes) if y]
    col2.persist()                                                              # ... and a full snapshot
    col3 = colmod.FlatCollection("t", persist_dir=d)
    assert sorted(col3.query(query_embeddings=v[5:6], n_results=12, filters=["pair"])["ids"][0]) == sorted(got)


def test_similarity_filter_past_64_names(colmod):
    v = _rows(10, seed=5)
    col = colmod.FlatCollection("t")
    many = {f"f{j:02d}": "yes" for j in range(64)}
    col.add(ids=_ids(10), embeddings=v, metadatas=[{"id": i, "filter_results_json": json.dumps(many)} for i in _ids(10)])
    yes = _expected_yes(v, v[1], 0.9)
    assert col.add_similarity_filter("the 65th", v[1], 0.9) == sum(yes) and 0 < sum(yes) < 10
    got = col.query(query_embeddings=v[6:7], n_results=10, filters=["the 65th", "f03"])["ids"][0]
    assert "the 65th" in col._filter_overflow and sorted(got) == [i for i, y in zip(_ids(10), yes) if y]


def test_apply_filters_convert_similarity_to_distance(colmod, monkeypatch):
    from mmiss_amd import search, utils

    v = _rows(20, seed=6)
    col = colmod.FlatCollection("t")
    col.add(ids=_ids(20), embeddings=v, metadatas=[{"id": i} for i in _ids(20)])
    search.set_collection(col)
    text_vec, image_vec = (v[3] + v[4]).astype(np.float32), (v[5] - v[6]).astype(np.float32)
    monkeypatch.setattr(utils, "load_clip_model", lambda: (None, None))
    monkeypatch.setattr(utils, "generate_clip_embedding",
                        lambda image=None, text=None, model=None, processor=None: {"text": text_vec[None]} if text is not None else {"image": image_vec[None]})
    try:
        idx = OracleMembershipIndex.instances[-1]
        for s in (0.55, 0.5, 0.0, 1.0):
            n = search.apply_text_filter("a photo of a dog", s)
            R = idx.membership_calls[-1][1]
            assert R.dtype == np.float32 and float(R) == float(utils.max_distance_for_similarity(s))
            # similarity = 1 - d / 2 in Python floats on the float32 distance (main.py:782): "yes" exactly where it reaches s
            d = ro.distances(text_vec[None], ro.normalize_rows(v, "f32"))[0]
            yes = [1 - float(x) / 2 >= s for x in d]
            assert n == sum(yes)
            metas = col.get(include=["metadatas"])["metadatas"]
            assert [json.loads(m["filter_results_json"])["a photo of a dog"] == "yes" for m in metas] == yes
        assert 0 < search.apply_text_filter("a photo of a dog", 0.5) < 20
        n = search.apply_image_filter(object(), "like this one", 0.52)
        d = ro.distances(image_vec[None], ro.normalize_rows(v, "f32"))[0]
        assert n == sum(1 - float(x) / 2 >= 0.52 for x in d) and 0 < n < 20
        answers = json.loads(col.get(ids=["im00"])["metadatas"][0]["filter_results_json"])
        assert set(answers) == {"a photo of a dog", "like this one"}
        res = search.search_similar(v[0], limit=20, filters=["like this one"])
        assert len(res) == n
        with pytest.raises(ValueError):
            search.apply_text_filter("x", float("nan"))
    finally:
        search.set_collection(None)


class _NoLibrary:
    """what FlatIndex needs of the library before it calls it: nothing — every call here is a bug of the wrapper"""
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} with arguments it should have refused")


def test_wrapper_argument_checks_come_before_the_call():
    import threading

    import mmiss_amd  # noqa: F401
    from mmiss_amd.index import FlatIndex

    idx = FlatIndex.__new__(FlatIndex)               # no device here: the checks under test run before any library call
    idx.dim, idx.dtype, idx.device, idx._h, idx._lib, idx._call_lock = D, 0, 0, None, _NoLibrary(), threading.RLock()
    q = np.zeros((3, D), np.float32)
    with pytest.raises(ValueError, match="max_dist"):
        idx.membership(q, np.ones(2, np.float32))
    with pytest.raises(ValueError, match="max_dist"):
        idx.membership(q, np.ones((3, 1), np.float32))
    with pytest.raises(ValueError, match="vectors"):
        idx.membership(np.zeros((3, D + 1), np.float32), 1.0)
    with pytest.raises(ValueError, match="max_dist"):
        idx.tag_by_radius(q, np.ones(4, np.float32), [1, 2, 3])
    with pytest.raises(TypeError, match="bits"):
        idx.tag_by_radius(q, 1.0, [1.0, 2.0, 3.0])
    with pytest.raises(TypeError, match="bits"):
        idx.tag_by_radius(q, 1.0, ["a", "b", "c"])
    with pytest.raises(TypeError, match="bits"):
        idx.tag_by_radius(q, 1.0, [True, False, True])
    with pytest.raises(ValueError, match="bits"):
        idx.tag_by_radius(q, 1.0, [1, 2])
    idx._h = None                                    # (nothing to destroy)

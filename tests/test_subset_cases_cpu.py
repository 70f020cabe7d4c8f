"""The planted corpora of tests/subset_cases.py held to their claims on the CPU, with the oracle alone: a case that does not plant
what it says would let the GPU tests pass for the wrong reason."""
import numpy as np
import pytest

import subset_cases as sc
from oracle import retrieval_oracle as ro

DTYPES = ["f32", "f16", "f8"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_hidden_row_is_the_nearest_of_the_index_and_outside_the_list(dtype):
    p = sc.hidden()
    N = p["x"].shape[0]
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    hid = lab[p["hidden"]]
    flat = sc.expected_flat(p["queries"], 3, st, lab)
    assert flat[0][0, 0] == hid and flat[1][0, 0] < flat[1][0, 1]             # strictly the nearest row of the whole index
    assert hid not in p["cand"] and p["cand"].size == N - 1
    got = sc.expected_subset(p["queries"], N, p["cand"], st, lab)
    assert hid not in got[0] and got[2][0] == N - 1 == got[3][0]
    assert np.array_equal(got[0][0, :2], flat[0][0, 1:3])                     # the list's best is the index's second


@pytest.mark.parametrize("dtype", DTYPES)
def test_crowding_needs_the_dedupe(dtype):
    p = sc.crowding()
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(200)
    crowd = lab[p["crowd"]]
    cand = p["cand"]
    at = np.nonzero(cand == crowd)[0]
    assert at.size > sc.CROWD_K                                               # listed more often than k,
    assert (np.diff(at) == 1).sum() >= sc.CROWD_K and (np.diff(at) > 5).sum() >= 2   # in a run and far apart
    got = sc.expected_subset(p["queries"], sc.CROWD_K, cand, st, lab)
    naive = sc.expected_without_dedupe(p["queries"], sc.CROWD_K, cand, st, lab)
    assert got[0][0, 0] == crowd and (naive[0][0] == crowd).all()             # the repeats would fill every slot
    assert sc.mismatch(got[:3], naive) is not None
    assert len(set(got[0][0].tolist())) == sc.CROWD_K and got[3][0] == np.unique(cand).size == 21
    # without repeats the two restatements agree
    once = np.unique(cand)
    assert sc.mismatch(sc.expected_subset(p["queries"], sc.CROWD_K, once, st, lab)[:3],
                       sc.expected_without_dedupe(p["queries"], sc.CROWD_K, once, st, lab)) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_label_listed_is_the_flat_answer(dtype):
    N, Q, k = 3001, 64, 10
    p = sc.corpus(23, N, sc.D, Q)
    st, lab = sc.stored_of(p["x"], dtype), sc.labels_of(N)
    req, exc = sc.query_masks(Q)
    rng = np.random.Generator(np.random.Philox(5))
    every = np.concatenate([lab[rng.permutation(N)], sc.UNKNOWN, lab[:50]])
    got = sc.expected_subset(p["queries"], k, every, st, lab)
    assert sc.mismatch(got[:3], sc.expected_flat(p["queries"], k, st, lab)) is None and (got[3] == N).all()
    got = sc.expected_subset(p["queries"], k, every, st, lab, p["tags"], req, exc)
    assert sc.mismatch(got[:3], sc.expected_flat(p["queries"], k, st, lab, p["tags"], req, exc)) is None
    assert got[2][2] == 0 and (got[2][[0, 1, 3]] == k).all()                  # query 2 has no direction


def test_lists_and_positions():
    N = 4999
    lab = sc.labels_of(N)
    assert not np.isin(sc.UNKNOWN, sc.labels_of(sc.BIG_N)).any()
    for m in (2, 63, 64, 65, 700, 3000):
        s = sc.sized_list(N, m, seed=m)
        assert s.size == m == np.unique(s).size and np.isin(s, lab).all() and lab[0] in s and lab[N - 1] in s
        assert not np.array_equal(s, np.sort(s)) or m == 2                    # shuffled
    mixed = sc.mixed_list(N, 700)
    assert sc.subset_rows(mixed, lab).size == 700 and mixed.size > 700 + 2 * sc.UNKNOWN.size and np.isin(sc.UNKNOWN, mixed).all()
    assert np.unique(mixed).size < mixed.size
    p = sc.positions(3001)
    lab = sc.labels_of(3001)
    a, b = p["lists"]
    assert a[0] == lab[0] == b[-1] and a[-1] == lab[3000] == b[0] and a.size == b.size == 302
    assert p["planted"][0] == 0 and p["planted"][1] == 3000 and set(lab[p["planted"]].tolist()) <= set(a.tolist())
    st = sc.stored_of(p["x"], "f16")
    for cand in (a, b):
        got = sc.expected_subset(p["queries"], 3, cand, st, lab)
        assert np.array_equal(got[0][:, 0], lab[p["planted"]])                # each planted row wins its query
    with np.errstate(all="ignore"):
        nodir = np.isnan(ro.distances(sc.corpus(21, N)["queries"][:1], sc.stored_of(sc.corpus(21, N)["x"], "f32"))[0])
    assert set(np.nonzero(nodir)[0].tolist()) == set(sc.nodir_rows(N))        # the rows without a direction are where the tests say
    assert sc.max_dim("f32") == 1920 and sc.max_dim("f16") == sc.max_dim("f8") == 3968

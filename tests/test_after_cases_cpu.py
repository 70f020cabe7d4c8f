"""The planted corpora and the restatement of tests/after_cases.py held to their claims on the CPU, with the oracle alone: a case
that does not plant what it says, or a restatement that cannot tell the contract from its two nearest mistakes, would let the GPU
tests pass for the wrong reason."""
import numpy as np
import pytest

import after_cases as ac
from oracle import retrieval_oracle as ro

DTYPES = ["f32", "f16", "f8"]
N = 4999


def _pager(q, st, lab, label_test="gt", **kw):
    return lambda k, ad, al: ac.expected_after(q, k, ad, al, st, lab, label_test=label_test, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_run_is_where_the_corpus_says(dtype):
    p = ac.run_corpus(31, N)
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(N)
    assert p["run"].size == ac.RUN and p["near"].size == ac.NEARER and (np.diff(p["run"]) > 0).all()
    assert (np.diff(p["run"]) > 1).sum() > ac.RUN // 2                        # scattered, not one block of rows
    assert (p["x"][p["run"]].view(np.uint32) == p["x"][p["run"][0]].view(np.uint32)).all()
    full_l, full_d = ac.full_ranking(p["queries"][0], st, lab)
    assert full_l.size == N - 5                                               # every row but the five without a direction
    assert set(full_l[:ac.NEARER].tolist()) == set(lab[p["near"]].tolist())
    run = slice(ac.NEARER, ac.NEARER + ac.RUN)
    assert np.array_equal(full_l[run], lab[p["run"]])                         # the run, by label
    assert np.unique(full_d[run].view(np.uint32)).size == 1                   # ... at one distance,
    assert full_d[ac.NEARER - 1] < full_d[ac.NEARER] and full_d[ac.NEARER + ac.RUN - 1] < full_d[ac.NEARER + ac.RUN]   # alone at it


@pytest.mark.parametrize("dtype", DTYPES)
def test_pages_of_seven_through_the_run_and_the_two_broken_forms(dtype):
    p = ac.run_corpus(31, N)
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(N)
    q = p["queries"][:1]
    full_l, full_d = ac.full_ranking(q, st, lab)
    head = 12 * 7                                                             # twelve pages: the run and what follows it
    pager = _pager(q, st, lab)
    labs, dists, pages = [], [], []
    ad, al = ac.START, 0
    for _ in range(12):
        got = pager(7, ad, al)
        labs.append(got[0][0]), dists.append(got[1][0]), pages.append((7, int(got[2][0]), int(got[3][0])))
        ad, al = got[1][0, -1], got[0][0, -1]
    assert ac.same_ranking(np.concatenate(labs), np.concatenate(dists), full_l[:head], full_d[:head]) is None
    assert [r for _, _, r in pages] == [full_l.size - 7 * i for i in range(12)]
    assert labs[0][-1] == ac.labels_of(N)[p["run"][0]]                        # the first page ends with the run's first copy
    # ">=" on the label: the second page starts with the entry the first one ended with
    second = ac.expected_after(q, 7, dists[0][-1], labs[0][-1], st, lab, label_test="ge")
    assert second[0][0, 0] == labs[0][-1] and second[3][0] == pages[1][2] + 1
    assert ac.mismatch(second, pager(7, dists[0][-1], labs[0][-1])) is not None
    # no label test: the second page starts behind the run — 49 entries are lost
    second = ac.expected_after(q, 7, dists[0][-1], labs[0][-1], st, lab, label_test="none")
    assert second[0][0, 0] == full_l[ac.NEARER + ac.RUN] and second[3][0] == pages[1][2] - (ac.RUN - 1)
    assert ac.mismatch(second, pager(7, dists[0][-1], labs[0][-1])) is not None


@pytest.mark.parametrize("dtype", DTYPES)
def test_chains_tile_the_ranking_with_masks_list_and_radius(dtype):
    p = ac.run_corpus(31, N)
    st, lab = ac.stored_of(p["x"], dtype), ac.labels_of(N)
    req, exc = ac.query_masks(4)
    q = p["queries"][3:4]
    d = ac.all_distances(q, st)[0]
    radius = np.sort(d[~np.isnan(d)])[900]
    for kw in (dict(), dict(tags=p["tags"], require=req[3], exclude=exc[3]), dict(cand=ac.mixed_list(N, 700)), dict(max_dist=radius),
               dict(cand=ac.UNKNOWN), dict(cand=np.zeros(0, np.int64))):
        full_l, full_d = ac.full_ranking(q, st, lab, **kw)
        for sizes in ((1000,), (2040,), (7, 1, 10, 1000)):
            got_l, got_d, pages = ac.chain(_pager(q, st, lab, **kw), sizes)
            assert ac.same_ranking(got_l, got_d, full_l, full_d) is None, (kw.keys(), sizes)
            assert ac.pages_consistent(pages, full_l.size) is None
            assert np.unique(got_l).size == got_l.size
    assert ac.full_ranking(q, st, lab, max_dist=radius)[0].size == 901


def test_cursor_values():
    p = ac.corpus(32, 600, ac.D, 5)
    st, lab = ac.stored_of(p["x"], "f16"), ac.labels_of(600)
    q = p["queries"]
    first = ac.expected_after(q, 10, ac.START, 0, st, lab)
    assert ac.mismatch(first[:3], ac.expected_flat(q, 10, st, lab)) is None and first[3][0] == 595 and first[3][2] == 0
    assert ac.mismatch(first, ac.expected_after(q, 10, ac.START, 2 ** 62, st, lab)) is None       # -inf: whatever the label
    nan = ac.expected_after(q, 10, np.float32(np.nan), 0, st, lab)
    assert (nan[2] == 0).all() and (nan[3] == 0).all()
    assert (ac.expected_after(q, 10, ac.START, 0, st, lab, max_dist=np.float32(np.nan))[3] == 0).all()
    # a cursor off the ranking: between two entries, any label; at an entry's distance with the labels around its own
    d3, d4, l3 = first[1][0, 3], first[1][0, 4], first[0][0, 3]
    assert d3 < d4
    mid = np.float32((np.float64(d3) + np.float64(d4)) / 2)
    for al in (-1, 2 ** 62):
        got = ac.expected_after(q[:1], 3, mid, al, st, lab)
        assert np.array_equal(got[0][0], first[0][0, 4:7]) and got[3][0] == 595 - 4
    assert ac.expected_after(q[:1], 3, d3, l3 - 1, st, lab)[0][0, 0] == l3                       # a removed label below it
    assert ac.expected_after(q[:1], 3, d3, l3, st, lab)[0][0, 0] == first[0][0, 4]
    assert ac.expected_after(q[:1], 3, np.nextafter(d3, np.float32(-1)), 2 ** 62, st, lab)[0][0, 0] == l3
    assert ac.expected_after(q[:1], 3, np.nextafter(d3, np.float32(9)), -1, st, lab)[0][0, 0] == first[0][0, 4]
    # the order of the bits: -0.0 ranks before +0.0
    assert ac.mono(np.float32(-0.0)) < ac.mono(np.float32(0.0)) and ac.mono(np.float32(-1e-30)) < ac.mono(np.float32(-0.0))
    v = np.array([-np.inf, -2.5, -1e-40, -0.0, 0.0, 1e-40, 1.0, np.inf], np.float32)
    assert (np.diff(ac.mono(v).astype(np.int64)) > 0).all()
    with np.errstate(all="ignore"):
        nodir = np.isnan(ro.distances(q[:1], st)[0])
    assert set(np.nonzero(nodir)[0].tolist()) == set(ac.nodir_rows(600))

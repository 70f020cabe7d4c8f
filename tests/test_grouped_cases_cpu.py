"""The planted corpora of tests/grouped_cases.py held to their claims on the CPU, with the oracle alone: a case that does not plant
what it says would let the GPU tests pass for the wrong reason."""
import numpy as np
import pytest

import grouped_cases as gc

DTYPES = ["f32", "f16", "f8"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_crowd_hides_the_other_groups_from_a_short_walk(dtype):
    p = gc.crowd()
    N = p["x"].shape[0]
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(N)
    rows, dist = gc.ranking(p["queries"][0], st, lab)
    assert rows.size == N and (p["groups"][rows[:gc.CROWD_SIZE]] == p["big"]).all()           # nearer than everything else
    assert dist[gc.CROWD_SIZE - 1] < dist[gc.CROWD_SIZE]
    k = gc.CROWD_K
    full = gc.expected_grouped(p["queries"], k, st, lab, p["groups"])
    short = gc.expected_grouped(p["queries"], k, st, lab, p["groups"], limit=16)
    assert full[3][0] == k and short[3][0] == 1 < k                                           # what the exhaustive route exists for
    assert full[0][0, 0] == short[0][0, 0] == lab[rows[0]] and full[2][0, 0] == p["big"]
    assert (full[2][0, 1:] != p["big"]).all() and len(set(full[0][0].tolist())) == k
    assert gc.expected_route(p["queries"], k, 16, st, lab, p["groups"])[0] == 1
    assert gc.expected_route(p["queries"], k, gc.CROWD_SIZE + k - 2, st, lab, p["groups"])[0] == 1
    assert gc.expected_route(p["queries"], k, 2040, st, lab, p["groups"])[0] == 0              # the list ends before the pool
    # all CROWD_OTHERS + 1 groups and the ten ungrouped rows: the count of a k above them
    big = gc.expected_grouped(p["queries"], 100, st, lab, p["groups"])
    assert big[3][0] == gc.CROWD_OTHERS + 1 + 10 and (big[0][0, big[3][0]:] == -1).all() and np.isinf(big[1][0, big[3][0]:]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_heads_at_the_last_and_the_first_row(dtype):
    p = gc.ends()
    N = p["x"].shape[0]
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(N)
    got = gc.expected_grouped(p["queries"], 4, st, lab, p["groups"])
    assert got[0][0, 0] == lab[N - 1] and got[2][0, 0] == 0 and got[0][1, 0] == lab[0] and got[2][1, 0] == 1
    for q in range(2):                                                                       # one hit per group
        g = got[2][q][got[2][q] >= 0]
        assert len(set(g.tolist())) == g.size


@pytest.mark.parametrize("dtype", DTYPES)
def test_tied_heads_are_ordered_by_label(dtype):
    p = gc.ties()
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(60)
    got = gc.expected_grouped(p["queries"], 6, st, lab, p["groups"])
    a, b, c = p["tied"]
    assert got[0][0, :3].tolist() == [lab[a], lab[b], lab[c]] and got[2][0, :3].tolist() == [5, 2, -1]
    assert len(set(got[1][0, :3].view(np.uint32).tolist())) == 1                              # the same distance bits
    assert lab[8] not in got[0][0] and lab[22] not in got[0][0]                               # second rows of their groups


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_mask_moves_the_head_of_a_group(dtype):
    p = gc.masked_head()
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(80)
    free = gc.expected_grouped(p["queries"], 8, st, lab, p["groups"], p["tags"])
    held = gc.expected_grouped(p["queries"], 8, st, lab, p["groups"], p["tags"], require=1)
    assert free[0][0, 0] == lab[p["near"]] and held[0][0, 0] == lab[p["admitted"]] and free[2][0, 0] == held[2][0, 0] == 3
    assert free[1][0, 0] < held[1][0, 0] and free[3][0] == held[3][0] == 8


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_and_queries_without_a_direction_and_ungrouped_rows(dtype):
    N, Q, k = 900, 6, 30
    p = gc.corpus(41, N, gc.D, Q, n_groups=12)
    st, lab = gc.stored_of(p["x"], dtype), gc.labels_of(N)
    g = p["groups"]
    assert (g == -1).sum() >= N // 4 - 5 and (g == p["n_groups"]).sum() == 2                  # the group without a direction
    got = gc.expected_grouped(p["queries"], k, st, lab, g)
    assert got[3][2] == 0 and (got[0][2] == -1).all()                                         # the query without a direction
    assert p["n_groups"] not in got[2] and not np.isin(got[0], lab[gc.nodir_rows(N)]).any()
    for q in (0, 1, 3):
        assert got[3][q] == k
        grouped = got[2][q][got[2][q] >= 0]
        assert len(set(grouped.tolist())) == grouped.size <= 12 and (got[2][q] == -1).any()   # ungrouped rows between grouped ones
        assert (np.diff(got[1][q]) >= 0).all()
    # every row ungrouped, or every row in a group of its own: the flat query
    flat = gc.expected_flat(p["queries"], k, st, lab)
    for groups in (np.full(N, -1, np.int32), np.arange(N, dtype=np.int32)):
        e = gc.expected_grouped(p["queries"], k, st, lab, groups)
        assert gc.pc.mismatch((e[0], e[1], e[3]), flat) is None
    # all rows in one group: the top-1
    one = gc.expected_grouped(p["queries"], k, st, lab, np.zeros(N, np.int32))
    assert (one[3] == [1, 1, 0, 1, 1, 1]).all() and np.array_equal(one[0][:, 0], flat[0][:, 0]) and (one[0][:, 1:] == -1).all()


def test_group_ids_at_both_ends_of_the_range():
    p = gc.extreme_ids()
    st, lab = gc.stored_of(p["x"], "f16"), gc.labels_of(300)
    got = gc.expected_grouped(p["queries"], 5, st, lab, p["groups"])
    assert got[2][:, 0].tolist() == [-1, 0, gc.MAX_GROUPS - 1] and (got[3] == 5).all()
    for q in range(3):
        assert (got[2][q] == 0).sum() == 1 and (got[2][q] == gc.MAX_GROUPS - 1).sum() == 1

"""The corpora of tests/assign_cases.py are what they claim to be, and its comparators reject the defects the GPU tests exist to
catch. No GPU: everything here is the oracle's arithmetic."""
import numpy as np
import pytest

import assign_cases as ac

D = 128
DTYPES = ["f32", "f16", "f8"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_ties_are_equal_float_distances_and_near_ties_differ(dtype):
    x, c = ac.ties_corpus(23, 1000, D)
    Dm, a, d, s = ac.expected_of(x, c, dtype)
    has_dir = ~np.isnan(Dm).all(axis=0)
    assert has_dir.sum() == 1000 - 5 and not has_dir[ac.nodir_rows(1000)].any()
    # the duplicate centre: the same bits against every row, and the smaller index takes all of them
    assert np.array_equal(Dm[ac.DUP].view(np.uint32), Dm[ac.DUP_OF].view(np.uint32))
    assert s[ac.DUP] == 0 and s[ac.DUP_OF] > 0 and (a != ac.DUP).all()
    # the one-ulp centre: a different vector, different distances on some rows, and it wins some and loses some
    differ = Dm[ac.NEAR][has_dir] != Dm[ac.NEAR_OF][has_dir]
    assert differ.any()
    lo, hi = Dm[ac.NEAR][has_dir] < Dm[ac.NEAR_OF][has_dir], Dm[ac.NEAR][has_dir] > Dm[ac.NEAR_OF][has_dir]
    assert lo.any() and hi.any(), (dtype, int(lo.sum()), int(hi.sum()))
    # the rows that are copies of a centre go to it (to the smaller index of a tied pair)
    copies = a[20:20 + ac.TIE_C]
    want = np.arange(ac.TIE_C)
    want[ac.DUP] = ac.DUP_OF
    free = [i for i in range(ac.TIE_C) if i not in (ac.NEAR, ac.NEAR_OF)]
    assert np.array_equal(copies[free], want[free]) and set(copies[[ac.NEAR, ac.NEAR_OF]]) <= {ac.NEAR, ac.NEAR_OF}
    # the sums of two centres are decided between exactly those two
    for i in range(ac.TIE_C):
        pair = {want[i], want[(i + 1) % ac.TIE_C]} | ({ac.NEAR, ac.NEAR_OF} if {i, (i + 1) % ac.TIE_C} & {ac.NEAR, ac.NEAR_OF} else set())
        assert a[40 + i] in pair, (i, a[40 + i])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_planted_row_of_the_random_corpus_is_equidistant(dtype):
    for C in (16, 17, 64, 65, 130):
        x, c = ac.random_corpus(21, 4999, D, C)
        Dm, a, d, s = ac.expected_of(x, c, dtype)
        r = ac.PLANTED_ROW
        assert Dm[0, r].view(np.uint32) == Dm[C - 1, r].view(np.uint32), (dtype, C)
        assert a[r] == 0 and d[r] == Dm[0, r] and (Dm[2:C - 1, r] > Dm[0, r]).all()


@pytest.mark.parametrize("C", [1, 15, 16, 17, 64, 65, 130])
def test_every_centre_wins_at_every_row_position(C):
    x, c = ac.every_winner_corpus(22, D, C)
    planted = np.array([ac.winner_of(r, C) for r in range(16 * C)])
    for dtype in DTYPES:
        a, d, s = ac.expected_of(x, c, dtype)[1:]
        assert np.array_equal(a, planted), (dtype, C)
        assert (s == 16).all()
    for cc in range(C):
        assert sorted(np.nonzero(planted == cc)[0] % 16) == list(range(16))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_and_centres_without_a_direction(dtype):
    N, C = 4999, 17
    x, c = ac.random_corpus(21, N, D, C)
    Dm, a, d, s = ac.expected_of(x, c, dtype)
    nd = ac.nodir_rows(N)
    assert np.isnan(Dm[:, nd]).all()                       # all-NaN columns
    assert (a[nd] == -1).all() and np.isinf(d[nd]).all()
    assert np.isnan(Dm[1]).all() and s[1] == 0 and (a != 1).all()      # the centre without a direction is never chosen
    assert (a >= 0).sum() == N - len(nd) and s.sum() == N - len(nd)
    # no centre has a direction: every row -1 / +inf
    a0, d0, s0 = ac.expected_assign(np.zeros((3, D), np.float32), ac.stored_of(x, dtype))
    assert (a0 == -1).all() and np.isinf(d0).all() and not s0.any()


@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_expected_kmeans_moves_rows_and_then_converges(dtype):
    k = ac.KMEANS
    st = ac.stored_of(ac.kmeans_corpus(), dtype)
    out = ac.expected_kmeans(st, k["C"], k["iters"])
    h = out["history"]
    assert len(h) >= 2 and not np.array_equal(h[0], h[1])              # the assignment changed at least once
    assert out["iterations"] == len(h) <= k["iters"]
    long = ac.expected_kmeans(st, k["C"], 40)
    assert long["iterations"] < 40                                      # ... and the loop stops by itself
    a, d, s = ac.expected_assign(out["centres"], st)
    assert np.array_equal(a, out["assign"]) and np.array_equal(s, out["sizes"])     # the assignment belongs to the centres
    # an empty cluster keeps its centre: two identical initial rows, the later one gets nothing
    pos = np.array([0, 0] + list(range(100, 100 + k["C"] - 2)))
    dup = ac.expected_kmeans(st, k["C"], 1, init_pos=pos)
    assert (dup["history"][0] != 1).all() and (dup["history"][0] == 0).any()
    assert np.array_equal(dup["centres"][1], ac.represented(st)[0]) and not np.array_equal(dup["centres"][0], ac.represented(st)[0])


def test_expected_sums_is_the_definition():
    x = ac.represented(ac.stored_of(ac.random_corpus(21, 17, D, 1)[0], "f16"))
    a = np.array([0, 1, -1, 1, 2, 5, 0] + [1] * 10, np.int32)
    sums, sizes = ac.expected_sums(x, a, 3)
    assert sizes.tolist() == [2, 12, 1]
    for cc in range(3):
        want = sum(int(round(float(v) * 2 ** 32)) for v in x[a == cc][:, 9].astype(np.float64))
        assert int(sums[cc, 9]) == want


def test_comparators_reject_each_defect():
    N, C = 1000, ac.TIE_C
    x, c = ac.ties_corpus(23, N, D)
    Dm, a, d, s = ac.expected_of(x, c, "f16")
    assert ac.mismatch((a.copy(), d.copy(), s.copy()), (a, d, s)) is None
    assert ac.mismatch((a.copy(), None, s.copy()), (a, d, s)) is None
    # a wrong tie-break: the rows of the duplicated centre given to the larger index
    wrong = a.copy()
    wrong[a == ac.DUP_OF] = ac.DUP
    ws = np.bincount(wrong[wrong >= 0], minlength=C).astype(np.int64)
    assert "assign" in ac.mismatch((wrong, d.copy(), ws), (a, d, s))
    # a row without a direction given 0 instead of -1
    wrong = a.copy()
    wrong[3] = 0
    assert "assign" in ac.mismatch((wrong, d.copy(), s.copy()), (a, d, s))
    # a dead centre chosen
    x2, c2 = ac.random_corpus(21, 4999, D, 17)
    e2 = ac.expected_of(x2, c2, "f16")[1:]
    wrong = e2[0].copy()
    wrong[100] = 1
    assert "assign" in ac.mismatch((wrong, e2[1].copy(), e2[2].copy()), e2)
    # one bit of a distance, a size
    wd = d.copy()
    wd[50] = np.nextafter(wd[50], np.float32(2))
    assert "dist" in ac.mismatch((a.copy(), wd, s.copy()), (a, d, s))
    wsz = s.copy()
    wsz[0] += 1
    assert "sizes" in ac.mismatch((a.copy(), d.copy(), wsz), (a, d, s))
    # a sum off by one unit
    xr = ac.represented(ac.stored_of(x, "f16"))
    es = ac.expected_sums(xr, a, C)
    assert ac.sums_mismatch((es[0].copy(), es[1].copy()), es) is None
    off = es[0].copy()
    off[5, 77] += 1
    assert "sums" in ac.sums_mismatch((off, es[1].copy()), es)

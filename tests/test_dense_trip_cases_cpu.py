"""The corpora and expected answers of tests/dense_trip_cases.py, checked on the reference alone, before any kernel runs: (a) every
kernel a case names makes at least two trips at that size (figures from the host-only plans program), (b) the margin rule hands at
most 1 % of a case's pairs to the canonical oracle (the share is printed), (c) a probe with a median radius has between 25 % and
75 % members in every trip's rows, (d) every centre wins rows in every trip's rows — so a kernel that skips or repeats a trip
cannot pass —, (e) the comparison rejects the edits a broken row loop would make. Also: the pairwise canonical distance has the
bits of retrieval_oracle.distances, and the margin rule's answers equal the full canonical oracle's on a sample."""
import numpy as np
import pytest

import dense_trip_cases as dt
import subset_cases as sc
from oracle import retrieval_oracle as ro

MID = ("f32", "f16", "f8")


def fig(name, dtype, n):
    N, dim = dt.SIZES[name]
    return dt.host_figures(dim, dtype, n, N)


def rows_of_dense_trip(N, tpb, trip, wave=None):
    _s, w, t = dt.dense_position(np.arange(N), tpb)
    return np.nonzero((t == trip) & ((w == wave) if wave is not None else True))[0]


def row_sets(N, f, kernels):
    """{name: [row index arrays]}: the rows of every trip of the dense scan and of the named grid-stride kernels"""
    tpb = f["scan"]["tiles_per_block"]
    out = {"dense": [rows_of_dense_trip(N, tpb, t) for t in range(tpb // 4)]}
    for k in kernels:
        out[k] = [np.arange(a, b) for a, b in dt.trip_ranges(N, f[k]["rows_per_trip"])]
        assert len(out[k]) == f[k]["trips"] >= 2, (k, f[k])
    return out


# ================================================================================================ (a) trips
def test_a_every_named_kernel_makes_a_second_trip():
    two, three = [], []
    for dtype in MID:
        for n in (1, 8, 17, 64, 16, 130):
            f = fig("mid", dtype, n)
            assert f["scan"]["wave_trips"] >= 2 and f["scan"]["tiles_per_block"] == 4 * f["scan"]["wave_trips"], (dtype, n, f["scan"])
            (two if f["scan"]["wave_trips"] == 2 else three).append((dtype, n))
            # the last slab is ragged: some wave makes fewer trips than its neighbours
            tpb, slabs = f["scan"]["tiles_per_block"], f["scan"]["slabs"]
            left = -(-dt.MID_N // 16) - (slabs - 1) * tpb
            trips = [len(range(w, left, 4)) for w in range(4)]
            assert 0 < left <= tpb and len(set(trips)) > 1, (dtype, n, left, trips)
        f = fig("mid", dtype, 130)
        assert f["scan"]["passes"] == 3, f["scan"]
        assert f["canonical_scan"]["trips"] >= 2 and f["assign_resolve"]["trips"] >= 3 and f["compact_blocks"] == 5, f
        assert fig("mid", dtype, 16)["cluster_sums"]["rows_per_block"] > 64
        cs = fig("mid", dtype, 1024)["cluster_sums"]
        assert cs["rows_per_block"] > 64 and cs["chunks"] == 8, cs
    assert ("f16", 64) in two and ("f8", 17) in two and ("f32", 64) in three and ("f32", 130) in three, (two, three)
    f = fig("top", "f16", 16)
    for k in ("member_count", "assign_sizes", "assign_decide", "member_from_dist", "member_merge_tags", "canonical_scan", "assign_resolve"):
        assert f[k]["trips"] >= 2, (k, f[k])
    assert f["scan"]["wave_trips"] >= 2
    f = fig("wide", "f32", dt.WIDE["P"])
    assert f["scan"]["passes"] == 2 and f["scan"]["nqt"] == 2 and f["scan"]["wave_trips"] >= 2, f["scan"]
    # the border plants need one probe per (wave 0 | 3, trip): 8 probes run two trips in every dtype
    assert all(fig("mid", dtype, 8)["scan"]["tiles_per_block"] == 8 for dtype in MID)


def test_planted_rows_do_not_collide():
    for name in ("mid", "top"):
        N = dt.SIZES[name][0]
        special = set(dt.nodir_rows(N)) | set(dt.tie_rows(N)) | set(range(N - dt.TAIL, N)) | {dt.copy_of(name)}
        assert not special & set(dt.copy_rows(N).tolist())
        assert len(set(dt.nodir_rows(N)) | set(dt.tie_rows(N))) == 5 + len(dt.tie_rows(N))
        assert dt.copy_rows(N)[-1] < N - dt.TAIL and np.unique(dt.copy_rows(N)).size == dt.NCOPY
    _s, w, t = dt.dense_position(np.array(dt.nodir_rows(dt.MID_N)), 8)
    assert (int(w[2]), int(t[2])) == (1, 1) and dt.dense_position(np.array([83]), 36)[2][0] == 1   # a tile of a later trip


# ================================================================================================ the oracle's two forms
@pytest.mark.parametrize("dtype", MID)
def test_pairwise_canonical_distances_have_the_oracles_bits_and_the_margin_rule_its_answers(dtype):
    st = dt.stored("mid", dtype)
    pick = np.unique(np.concatenate([np.arange(0, 300), np.arange(dt.MID_N - 300, dt.MID_N), np.array(dt.tie_rows(dt.MID_N)),
                                     np.random.Generator(np.random.Philox(3)).integers(0, dt.MID_N, 3000)]))
    q = dt.probes("mid")[:8]
    with np.errstate(all="ignore"):
        full = ro.distances(q, st[pick])
    pp, rr = np.meshgrid(np.arange(8), np.arange(pick.size), indexing="ij")
    got = dt.canon_pair_distances(q, st, pick[rr.ravel()], pp.ravel()).reshape(8, pick.size)
    assert np.array_equal(got.view(np.uint32), full.view(np.uint32))
    # the exact distances stay within the bound the margin was derived from
    ex = dt.exact_distances(q, st[pick])
    ok = ~np.isnan(full)
    assert np.array_equal(np.isnan(ex), ~ok) and np.abs(ex[ok] - full[ok].astype(np.float64)).max() < 2.0 ** -22
    # membership and assignment by the margin rule == by the canonical oracle alone
    R = dt.mixed_radii(ex)
    R[3] = full[3, 40]                     # one radius AT a distance
    words, counts, mem, _n = dt.expected_membership(q, st[pick], R)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(mem, full <= R[:, None]) and np.array_equal(counts, (full <= R[:, None]).sum(1))
    from assign_cases import expected_assign as canonical_assign
    for c in (dt.centres(16), dt.duplicated_centres()):
        a, d, s, _n = dt.expected_assign(c, st[pick])
        ea, ed, es = canonical_assign(c, st[pick])
        assert np.array_equal(a, ea) and np.array_equal(d.view(np.uint32), ed.view(np.uint32)) and np.array_equal(s, es)


# ================================================================================================ (b), (c): membership
def in_band(mem_row, sets, what):
    for k, trips in sets.items():
        for t, r in enumerate(trips):
            share = mem_row[r].mean()
            assert 0.25 <= share <= 0.75, (what, k, t, r.size, share)


@pytest.mark.parametrize("dtype", MID)
def test_bc_membership_at_mid_size(dtype):
    N = dt.MID_N
    for P in (1, 17, 64):
        q, R, (words, counts, mem, ncanon) = dt.mixed_call("mid", dtype, P)
        share = ncanon / (P * N)
        print(f"membership mid {dtype} P={P}: canonical pairs {ncanon} = {100 * share:.4f} % of the case")
        assert share <= dt.MAX_CANONICAL_SHARE
        sets = row_sets(N, fig("mid", dtype, P), ())
        for p in dt.median_probes(P):
            in_band(mem[p], sets, (dtype, P, p))
        assert not words[dt.nodir_rows(N)].any() and (P == 1 or counts[1] == 0)
    # the overflow call: every copy is an undecided pair, and the probe has both kinds of rows in both trips of the canonical pass
    q, R, (words, counts, mem, ncanon), below = dt.overflow_call("mid", dtype)
    share = ncanon / (8 * N)
    print(f"membership mid {dtype} overflow: canonical pairs {ncanon} = {100 * share:.4f} % of the case")
    assert dt.NCOPY <= ncanon and share <= dt.MAX_CANONICAL_SHARE
    in_band(mem[2], row_sets(N, fig("mid", dtype, 8), ("canonical_scan",)), (dtype, "overflow"))
    copies = dt.copy_rows(N)
    assert mem[2][copies].all() and not below[2][2][copies].any() and counts[2] - below[1][2] >= dt.NCOPY
    # no other probe of the call has the copies anywhere near its radius: they overflow probe 2's list alone
    d = dt.distances_of("mid", dtype, "probes", True)[:8, dt.copy_of("mid")]
    assert all(abs(d[p] - R[p]) > 0.02 for p in (0, 4, 6)), (d, R)
    # the border call: planted pairs flip with one ulp
    f = fig("mid", dtype, 8)
    q, R, planted, e0, Rb, e1 = dt.border_call("mid", dtype, f["scan"]["tiles_per_block"], f["scan"]["slabs"] // 2)
    assert sorted((int(w), int(t)) for _s, w, t in (dt.dense_position(r, 8) for r in planted.values())) == [(0, 0), (0, 1), (3, 0), (3, 1)]
    for p, r in planted.items():
        assert e0[2][p, r] and not e1[2][p, r]


def test_bc_membership_wide_and_top():
    W = dt.WIDE
    q, R, (words, counts, mem, ncanon) = dt.mixed_call("wide", "f32", W["P"])
    print(f"membership wide f32 P=64: canonical pairs {ncanon} = {100 * ncanon / (W['P'] * W['N']):.4f} % of the case")
    assert ncanon / (W["P"] * W["N"]) <= dt.MAX_CANONICAL_SHARE
    sets = row_sets(W["N"], fig("wide", "f32", W["P"]), ())
    for p in dt.median_probes(W["P"]):
        in_band(mem[p], sets, ("wide", p))
    assert any(p >= 32 for p in dt.median_probes(W["P"]))          # the second pass has a median probe too
    N = dt.TOP_N
    q, R, (words, counts, mem, ncanon), below = dt.overflow_call("top", "f16")
    print(f"membership top f16 P=3: canonical pairs {ncanon} = {100 * ncanon / (3 * N):.4f} % of the case")
    assert dt.NCOPY <= ncanon and ncanon / (3 * N) <= dt.MAX_CANONICAL_SHARE
    sets = row_sets(N, fig("top", "f16", 3), ("member_count", "member_from_dist", "member_merge_tags", "canonical_scan"))
    in_band(mem[0], sets, ("top", "median"))
    in_band(mem[2], sets, ("top", "overflow"))
    assert counts[1] == N - 5 and np.isinf(R[1])
    d = dt.distances_of("top", "f16", "probes", True)[0, dt.copy_of("top")]
    assert abs(d - R[0]) > 0.02


# ================================================================================================ (b), (d): assignment
@pytest.mark.parametrize("dtype", MID)
def test_bd_assignment_at_mid_size(dtype):
    N = dt.MID_N
    for C in (16, 130):
        c, (a, dist, sizes, ncanon) = dt.assign_call("mid", dtype, C)
        print(f"assignment mid {dtype} C={C}: canonical pairs {ncanon} = {100 * ncanon / (C * N):.4f} % of the case")
        assert ncanon / (C * N) <= dt.MAX_CANONICAL_SHARE
        for k, trips in row_sets(N, fig("mid", dtype, C), ("assign_resolve",)).items():
            for t, r in enumerate(trips):
                won = np.bincount(a[r][a[r] >= 0], minlength=C)
                assert (won > 0).all(), (dtype, C, k, t, np.nonzero(won == 0)[0])
        assert (a[dt.nodir_rows(N)] == -1).all() and np.isinf(dist[dt.nodir_rows(N)]).all() and (a >= 0).sum() == N - 5
        assert (a[dt.tie_rows(N)] == 0).all()                       # the planted ties: centre 0, not C - 1


def test_bd_assignment_duplicates_and_top():
    N = dt.MID_N
    c, (a, dist, sizes, ncanon) = dt.assign_call("mid", "f16", "dup")
    assert ncanon == 4 * N and sizes[2] == 0 and sizes[3] == 0        # every row is the canonical oracle's, by construction
    f = fig("mid", "f16", 4)
    assert (a >= 0).sum() > 2 * f["assign_resolve"]["rows_per_trip"]  # the list form runs past two reaches of its grid
    for t, r in enumerate(row_sets(N, f, ("assign_resolve",))["assign_resolve"]):
        assert (np.bincount(a[r][a[r] >= 0], minlength=4)[:2] > 0).all()
    N = dt.TOP_N
    c, (a, dist, sizes, ncanon) = dt.assign_call("top", "f16", 16)
    print(f"assignment top f16 C=16: canonical pairs {ncanon} = {100 * ncanon / (16 * N):.4f} % of the case")
    assert ncanon / (16 * N) <= dt.MAX_CANONICAL_SHARE
    for k, trips in row_sets(N, fig("top", "f16", 16), ("assign_decide", "assign_sizes", "assign_resolve")).items():
        for t, r in enumerate(trips):
            won = np.bincount(a[r][a[r] >= 0], minlength=16)
            assert (won > 0).all(), (k, t, r.size, won)


# ================================================================================================ (e) power
def test_e_the_comparison_rejects_what_a_broken_row_loop_would_write():
    N = dt.MID_N
    f = fig("mid", "f16", 64)
    tpb = f["scan"]["tiles_per_block"]
    q, R, (words, counts, mem, _n) = dt.mixed_call("mid", "f16", 64)
    c, (a, dist, sizes, _n) = dt.assign_call("mid", "f16", 16)
    assert dt.words_mismatch(words.copy(), words) is None and dt.ints_mismatch(a.copy(), a, "assign") is None
    assert dt.bits_mismatch(dist.copy(), dist) is None
    # all rows of the second trip of one wave cleared (or left as the 0xA5 fill)
    second = rows_of_dense_trip(N, tpb, 1, wave=2)
    for fill_w, fill_a in ((0, -1), (0xA5A5A5A5A5A5A5A5, np.int32(-1515870811))):
        w2, a2, d2 = words.copy(), a.copy(), dist.copy()
        w2[second] = np.uint64(fill_w); a2[second] = fill_a; d2[second] = np.float32(np.inf)
        assert dt.words_mismatch(w2, words) and dt.ints_mismatch(a2, a, "assign") and dt.bits_mismatch(d2, dist)
    # one trip's rows shifted by 16: wave 1's second trip reads the tile behind its own
    trip = rows_of_dense_trip(N, tpb, 1, wave=1)
    src = np.minimum(trip + 16, N - 1)
    w2, a2, d2 = words.copy(), a.copy(), dist.copy()
    w2[trip], a2[trip], d2[trip] = words[src], a[src], dist[src]
    assert dt.words_mismatch(w2, words) and dt.ints_mismatch(a2, a, "assign") and dt.bits_mismatch(d2, dist)
    # ... and the same for one trip of a grid-stride kernel
    r0, r1 = dt.trip_ranges(N, f["assign_resolve"]["rows_per_trip"])[1]
    d2 = dist.copy()
    d2[r0:r1] = dist[r0 + 16:r1 + 16]
    assert dt.bits_mismatch(d2, dist)
    # the last ragged tile dropped
    assert N % 16
    w2, a2 = words.copy(), a.copy()
    w2[N - N % 16:] = 0; a2[N - N % 16:] = -1
    assert dt.words_mismatch(w2, words) and dt.ints_mismatch(a2, a, "assign")
    # counts and sizes move with any of it
    assert counts[0] != (w2 & np.uint64(1)).sum() and not np.array_equal(np.bincount(a2[a2 >= 0], minlength=16), sizes)
    # block_off of subset block 1 set to 0: the list's head is overwritten, row 0 (query 0's nearest row) is gone
    listed = dt.subset_list_rows(N)
    broken = dt.block_off_zeroed(listed)
    assert listed[0] == 0 and 0 not in broken and broken.size == listed.size
    st, labels, qs = dt.stored("mid", "f16"), dt.labels_of(N), dt.subset_queries("mid")
    good = sc.expected_subset(qs[:1], 10, labels[listed], st, labels)
    bad = sc.expected_subset(qs[:1], 10, labels[np.unique(broken)], st, labels)
    assert good[0][0, 0] == labels[0] and sc.mismatch(bad[:3], good[:3]) is not None


def test_the_subset_list_covers_the_blocks_as_described():
    N = dt.MID_N
    listed = dt.subset_list_rows(N)
    per = np.bincount(listed // dt.BLOCK, minlength=5)
    assert per[2] == 0 and per[3] == dt.BLOCK and all(per[b] > 500 for b in (0, 1, 4)), per
    for b in (0, 1, 3, 4):
        assert b * dt.BLOCK in listed and min(N, (b + 1) * dt.BLOCK) - 1 in listed
    assert fig("mid", "f16", 1)["compact_block_rows"] == dt.BLOCK


def test_the_fast_cluster_sums_are_the_definition():
    import assign_cases as ac

    x = ac.represented(dt.stored("mid", "f8")[:6000])
    for C in (16, 1024):
        a = dt.synthetic_assign(6000, C)
        assert set(np.unique(a).tolist()) == set(range(-1, C + 1)) and (a[[3, 5, 83, 84]] == -1).all()
        with np.errstate(all="ignore"):
            assert ac.sums_mismatch(dt.expected_sums(x, a, C), ac.expected_sums(x, a, C)) is None

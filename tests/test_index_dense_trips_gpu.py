"""The index scans PAST THEIR FIRST TRIP (membership / tagging, assignment, cluster sums, k-means, radius, probed and subset search)
against the oracle, at the sizes where the row loops of their kernels make a second trip: corpora, expected answers and the trip
geometry are tests/dense_trip_cases.py's, checked on the reference alone by test_dense_trip_cases_cpu.py. Every test reads the trip
counts of the kernels it names from mmiss_dbg_index_dense_plan and asserts them BEFORE the call; every raw call gets device output
buffers pre-filled with 0xA5 bytes, so a row the kernels never wrote shows as that pattern and not as a plausible zero; after the
call the guard statistics say which route decided (radius_pages: passes, swept_rows: pairs resolved canonically, exhaustive: probes
on the per-probe canonical route). One index per corpus and dtype, built once."""
import time

import numpy as np
import pytest

import assign_cases as ac
import dense_trip_cases as dt
import partition_cases as pc
import subset_cases as sc
from index_query_cases import load_mods

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
FILL = 0xA5
FILL64 = np.uint64(0xA5A5A5A5A5A5A5A5)
FILL32 = np.uint32(0xA5A5A5A5)
PAD = 64
_indexes = {}


@pytest.fixture(scope="module")
def mods():
    m = load_mods()
    yield m
    for idx in _indexes.values():
        idx.close()
    _indexes.clear()


def index_of(mods, name, dtype, copies=None):
    """the one index of a corpus and dtype; the tests leave its rows as they are (tags are rewritten by the tests that use them)"""
    copies = (name == "top") if copies is None else copies
    key = (name, dtype, copies)
    if key not in _indexes:
        x = dt.rows(name, copies)
        idx = mods[0](x.shape[1], dtype, capacity=x.shape[0])
        idx.add(x, dt.labels_of(x.shape[0]))
        _indexes[key] = idx
    return _indexes[key]


def plan_of(mods, idx, n):
    return mods[3].index_dense_plan(idx._h, n)


def delta(idx, before):
    after = idx.guard_stats()
    return {k: after[k] - before[k] for k in after}


def quiet(dl):
    return all(dl[s] == 0 for s in ("queries", "widened", "rounds", "pages"))


def filled(nbytes):
    import torch

    return torch.full((int(nbytes),), FILL, dtype=torch.uint8, device="cuda")


def host(buf, dtype):
    return buf.cpu().numpy().view(dtype)


def sync():
    import torch

    torch.cuda.synchronize()


def raw_membership(mods, idx, q, R):
    """mmiss_index_membership into 0xA5-filled device buffers with PAD spare rows -> (words [count], members [P]); nothing is
    written behind count or behind P"""
    lib, P, n = mods[3], int(q.shape[0]), idx.count()
    q, R = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(R, np.float32)
    words, members = filled((n + PAD) * 8), filled((P + 2) * 8)
    sync()
    lib.check(idx._lib.mmiss_index_membership(idx._h, q.ctypes.data, P, R.ctypes.data, words.data_ptr(), n + PAD, members.data_ptr()))
    w, m = host(words, np.uint64), host(members, np.uint64)
    assert (w[n:] == FILL64).all() and (m[P:] == FILL64).all()
    return w[:n], m[:P].view(np.int64)


def raw_assign(mods, idx, c, want_dist=True):
    lib, C, n = mods[3], int(c.shape[0]), idx.count()
    c = np.ascontiguousarray(c, np.float32)
    asg, dist, sizes = filled((n + PAD) * 4), filled((n + PAD) * 4), filled((C + 2) * 8)
    sync()
    lib.check(idx._lib.mmiss_index_assign(idx._h, c.ctypes.data, C, asg.data_ptr(), dist.data_ptr() if want_dist else None, n + PAD,
                                          sizes.data_ptr()))
    a, d, s = host(asg, np.uint32), host(dist, np.uint32), host(sizes, np.uint64)
    assert (a[n:] == FILL32).all() and (d[n if want_dist else 0:] == FILL32).all() and (s[C:] == FILL64).all()
    return a[:n].view(np.int32), d[:n].view(np.float32), s[:C].view(np.int64)


def raw_cluster_sums(mods, idx, a, C):
    import torch

    lib, n, dim = mods[3], idx.count(), idx.dim
    da = torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    sums, sizes = filled((C * dim + 2) * 8), filled((C + 2) * 8)
    sync()
    lib.check(idx._lib.mmiss_index_cluster_sums(idx._h, da.data_ptr(), n, C, sums.data_ptr(), sizes.data_ptr()))
    s, z = host(sums, np.uint64), host(sizes, np.uint64)
    assert (s[C * dim:] == FILL64).all() and (z[C:] == FILL64).all()
    return s[:C * dim].view(np.int64).reshape(C, dim), z[:C].view(np.int64)


def raw_subset(mods, idx, q, k, cand, require=None, exclude=None):
    import torch

    lib, Q = mods[3], int(q.shape[0])
    dq = torch.from_numpy(np.array(q, np.float32)).cuda()
    cand = np.ascontiguousarray(cand, np.int64)
    masks = [None if m is None else np.ascontiguousarray(np.broadcast_to(np.asarray(m).astype(np.uint64), (Q,))) for m in (require, exclude)]
    lab, dist, cnt, matched = filled((Q * k + 2) * 8), filled((Q * k + 2) * 4), filled((Q + 2) * 4), filled((Q + 2) * 8)
    sync()
    lib.check(idx._lib.mmiss_index_query_subset(idx._h, dq.data_ptr(), Q, k, cand.ctypes.data, int(cand.shape[0]), lib.ptr(masks[0]),
                                                lib.ptr(masks[1]), lab.data_ptr(), dist.data_ptr(), cnt.data_ptr(), matched.data_ptr()))
    l, d, c, m = host(lab, np.uint64), host(dist, np.uint32), host(cnt, np.uint32), host(matched, np.uint64)
    assert (l[Q * k:] == FILL64).all() and (d[Q * k:] == FILL32).all() and (c[Q:] == FILL32).all() and (m[Q:] == FILL64).all()
    return l[:Q * k].view(np.int64).reshape(Q, k), d[:Q * k].view(np.float32).reshape(Q, k), c[:Q].view(np.int32), m[:Q].view(np.int64)


def raw_radius(mods, idx, cap, q=None, R=None, by_label=None, max_dist=None, later_only=False):
    """mmiss_index_query_radius (q, R) or mmiss_index_query_radius_by_label (by_label, max_dist) into 0xA5-filled device buffers"""
    import torch

    lib = mods[3]
    Q = int(q.shape[0]) if by_label is None else int(by_label.shape[0])
    lab, dist, cnt, tot = filled((Q * cap + 2) * 8), filled((Q * cap + 2) * 4), filled((Q + 2) * 4), filled((Q + 2) * 8)
    outs = (lab.data_ptr(), dist.data_ptr(), cnt.data_ptr(), tot.data_ptr())
    if by_label is None:
        dq = torch.from_numpy(np.array(q, np.float32)).cuda()
        R = np.ascontiguousarray(np.broadcast_to(np.asarray(R, np.float32), (Q,)))
        sync()
        lib.check(idx._lib.mmiss_index_query_radius(idx._h, dq.data_ptr(), Q, R.ctypes.data, cap, None, None, *outs))
    else:
        by_label = np.ascontiguousarray(by_label, np.int64)
        sync()
        lib.check(idx._lib.mmiss_index_query_radius_by_label(idx._h, by_label.ctypes.data, Q, float(max_dist), cap, 1 if later_only else 0, *outs))
    l, d, c, t = host(lab, np.uint64), host(dist, np.uint32), host(cnt, np.uint32), host(tot, np.uint64)
    assert (l[Q * cap:] == FILL64).all() and (d[Q * cap:] == FILL32).all() and (c[Q:] == FILL32).all() and (t[Q:] == FILL64).all()
    return (l[:Q * cap].view(np.int64).reshape(Q, cap), d[:Q * cap].view(np.float32).reshape(Q, cap), c[:Q].view(np.int32),
            t[:Q].view(np.int64))


def check_membership(got, exp, P, what):
    words, members = got
    assert dt.words_mismatch(words, exp[0], P) is None, (what, dt.words_mismatch(words, exp[0], P))
    assert np.array_equal(members, exp[1]), (what, members, exp[1])


def check_assign(got, exp, what, at=None):
    a, d, s = got
    assert dt.ints_mismatch(a, exp[0], "assign") is None, (what, dt.ints_mismatch(a, exp[0], "assign"))
    assert dt.bits_mismatch(d, exp[1], at) is None, (what, dt.bits_mismatch(d, exp[1], at))
    assert np.array_equal(s, exp[2]), (what, s, exp[2])


# ================================================================================================ membership, mid size
@pytest.mark.parametrize("dtype", DTYPES)
def test_membership_words_and_counts_on_every_trip(mods, dtype):
    t0 = time.time()
    idx = index_of(mods, "mid", dtype)
    N = dt.MID_N
    trips = set()
    for P in (1, 17, 64):
        plan = plan_of(mods, idx, P)
        assert plan["rows"] == N and plan["scan"]["wave_trips"] >= 2 and plan["scan"]["passes"] == 1, plan["scan"]
        trips.add(plan["scan"]["wave_trips"])
        q, R, exp = dt.mixed_call("mid", dtype, P)
        before = idx.guard_stats()
        got = raw_membership(mods, idx, q, R)
        check_membership(got, exp, P, (dtype, P))
        assert not got[0][dt.nodir_rows(N)].any()
        dl = delta(idx, before)
        assert dl["radius_queries"] == P and dl["radius_pages"] == 1 and dl["exhaustive"] == 0 and quiet(dl), dl
        assert dl["swept_rows"] <= dt.MAX_CANONICAL_SHARE * P * N, dl
    assert trips == ({2, 3} if dtype == "f32" else {2}), trips
    print(f"membership mid {dtype}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("dtype", DTYPES)
def test_membership_borderline_pairs_on_every_trip_of_waves_0_and_3(mods, dtype):
    idx = index_of(mods, "mid", dtype)
    scan = plan_of(mods, idx, 8)["scan"]
    assert scan["wave_trips"] == 2 and scan["tiles_per_block"] == 8, scan
    q, R, planted, e0, Rb, e1 = dt.border_call("mid", dtype, scan["tiles_per_block"], scan["slabs"] // 2)
    spots = sorted(tuple(int(v) for v in dt.dense_position(r, scan["tiles_per_block"])[1:]) for r in planted.values())
    assert spots == [(0, 0), (0, 1), (3, 0), (3, 1)], spots
    for step, (Rs, exp) in enumerate(((R, e0), (Rb, e1))):
        before = idx.guard_stats()
        got = raw_membership(mods, idx, q, Rs)
        check_membership(got, exp, 8, (dtype, step))
        for p, r in planted.items():
            assert int(got[0][r] >> np.uint64(p)) & 1 == (1 if step == 0 else 0), (dtype, step, p, r)
        dl = delta(idx, before)
        assert dl["swept_rows"] >= len(planted) and dl["exhaustive"] == 0 and dl["radius_pages"] == 1 and quiet(dl), dl


@pytest.mark.parametrize("dtype", DTYPES)
def test_membership_mass_duplicates_take_the_canonical_pass_over_two_trips(mods, dtype):
    idx = index_of(mods, "mid", dtype, copies=True)
    N = dt.MID_N
    plan = plan_of(mods, idx, 8)
    assert plan["canonical_scan"]["trips"] >= 2 and plan["scan"]["wave_trips"] >= 2, plan
    q, R, e0, e1 = dt.overflow_call("mid", dtype)
    copies = dt.copy_rows(N)
    for step, exp in enumerate((e0, e1)):
        Rs = np.array(R)
        if step:
            Rs[2] = np.nextafter(R[2], np.float32(-np.inf))
        before = idx.guard_stats()
        got = raw_membership(mods, idx, q, Rs)
        check_membership(got, exp, 8, (dtype, step))
        is_member = ((got[0][copies] >> np.uint64(2)) & np.uint64(1)).astype(bool)
        assert is_member.all() if step == 0 else not is_member.any()
        dl = delta(idx, before)
        assert dl["exhaustive"] == 1 and dl["radius_pages"] == 1 and dl["swept_rows"] >= N and quiet(dl), dl


def test_membership_two_passes_of_two_trips_at_dim_768(mods):
    W = dt.WIDE
    idx = index_of(mods, "wide", "f32")
    scan = plan_of(mods, idx, W["P"])["scan"]
    assert scan["passes"] == 2 and scan["wave_trips"] >= 2, scan
    q, R, exp = dt.mixed_call("wide", "f32", W["P"])
    before = idx.guard_stats()
    got = raw_membership(mods, idx, q, R)
    check_membership(got, exp, W["P"], "wide")
    dl = delta(idx, before)
    assert dl["radius_pages"] == 2 and dl["radius_queries"] == W["P"] and dl["exhaustive"] == 0 and quiet(dl), dl


# ================================================================================================ assignment, mid size
@pytest.mark.parametrize("dtype", DTYPES)
def test_assignment_of_every_row_on_every_trip_and_pass(mods, dtype):
    t0 = time.time()
    idx = index_of(mods, "mid", dtype)
    N = dt.MID_N
    for C in (16, 130):
        plan = plan_of(mods, idx, C)
        assert plan["scan"]["wave_trips"] >= 2 and plan["scan"]["passes"] == (1 if C == 16 else 3), plan["scan"]
        assert plan["assign_resolve"]["trips"] >= 3, plan["assign_resolve"]
        c, exp = dt.assign_call("mid", dtype, C)
        before = idx.guard_stats()
        got = raw_assign(mods, idx, c)
        check_assign(got, exp, (dtype, C))
        assert (got[0][dt.tie_rows(N)] == 0).all() and (got[0][dt.nodir_rows(N)] == -1).all()
        dl = delta(idx, before)
        assert dl["radius_queries"] == C and dl["radius_pages"] == plan["scan"]["passes"] and dl["exhaustive"] == 0 and quiet(dl), dl
        assert dl["swept_rows"] % C == 0 and len(dt.tie_rows(N)) * C <= dl["swept_rows"] < N * C / 2, dl   # (borderline rows x live centres)
        # without distances: the same assignment, nothing written to a distance buffer
        got = raw_assign(mods, idx, c, want_dist=False)
        assert dt.ints_mismatch(got[0], exp[0], "assign") is None and np.array_equal(got[2], exp[2])
    print(f"assignment mid {dtype}: {time.time() - t0:.2f} s")


def test_assignment_with_duplicated_centres_lists_every_row(mods):
    idx = index_of(mods, "mid", "f16")
    N = dt.MID_N
    plan = plan_of(mods, idx, 4)
    c, exp = dt.assign_call("mid", "f16", "dup")
    assert plan["assign_resolve"]["trips"] >= 3 and N - 5 > 2 * plan["assign_resolve"]["rows_per_trip"], plan["assign_resolve"]
    before = idx.guard_stats()
    got = raw_assign(mods, idx, c)
    check_assign(got, exp, "dup")
    dl = delta(idx, before)
    assert dl["swept_rows"] == (N - 5) * 4 and dl["radius_pages"] == 1 and quiet(dl), dl   # (rows with a direction) x (live centres)


# ================================================================================================ cluster sums, k-means
@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_sums_with_more_than_64_rows_per_block(mods, dtype):
    idx = index_of(mods, "mid", dtype)
    N = dt.MID_N
    x = ac.represented(dt.stored("mid", dtype))
    for C, a in ((16, dt.assign_call("mid", dtype, 16)[1][0]), (1024, dt.synthetic_assign(N, 1024))):
        cs = plan_of(mods, idx, C)["cluster_sums"]
        assert cs["rows_per_block"] > 64 and cs["chunks"] == (8 if C == 1024 else 1), cs
        with np.errstate(all="ignore"):
            exp = dt.expected_sums(x, a, C)
        got = raw_cluster_sums(mods, idx, a, C)
        assert ac.sums_mismatch(got, exp) is None, (dtype, C, ac.sums_mismatch(got, exp))


def test_kmeans_three_iterations(mods):
    t0 = time.time()
    idx = index_of(mods, "mid", "f16")
    st, C = dt.stored("mid", "f16"), 5
    assert plan_of(mods, idx, C)["scan"]["wave_trips"] >= 2
    with np.errstate(all="ignore"):
        exp = ac.expected_kmeans(st, C, 3, assign=lambda c, s: dt.expected_assign(c, s)[:3], sums=dt.expected_sums)
    out = idx.kmeans(C, iters=3)
    assert out["iterations"] == exp["iterations"] == 3
    assert np.array_equal(out["centres"].view(np.uint32), exp["centres"].view(np.uint32))
    assert ac.mismatch((out["assign"], out["dist"], out["sizes"]), (exp["assign"], exp["dist"], exp["sizes"])) is None
    print(f"kmeans mid f16: {time.time() - t0:.2f} s")


# ================================================================================================ radius, mid size
def radius_expected(q, st, labels, R, cap, row_min=-1):
    """radius_cases.members by the margin rule: the canonical distance of every row whose exact distance is within MARGIN of the
    radius or below it"""
    d = dt.exact_distances(q[None], st)[0]
    with np.errstate(invalid="ignore"):
        near = np.nonzero(~(d > float(R) + dt.MARGIN))[0]
    near = near[near > row_min]
    cd = dt.canon_pair_distances(q[None], st, near, np.zeros(near.size, np.int64))
    with np.errstate(invalid="ignore"):
        keep = cd <= np.float32(R)
    idx, cd = near[keep], cd[keep]
    order = np.lexsort((labels[idx], cd))
    out_l, out_d = np.full(cap, -1, np.int64), np.full(cap, np.inf, np.float32)
    n = min(cap, idx.size)
    out_l[:n], out_d[:n] = labels[idx[order[:n]]], cd[order[:n]]
    return out_l, out_d, np.int32(n), np.int64(idx.size)


def test_radius_calls_past_the_cap_through_the_exhaustive_pass_and_by_label(mods):
    import radius_cases as rc

    t0 = time.time()
    idx = index_of(mods, "mid", "f16", copies=True)
    N, st, labels = dt.MID_N, dt.stored("mid", "f16", True), dt.labels_of(dt.MID_N)
    assert mods[3].index_radius_plan(idx._h, 1)["first"]["tiles_per_block"] > 4
    assert plan_of(mods, idx, 1)["canonical_scan"]["trips"] >= 2
    # more members than cap: the 1000 nearest of about 2 % of the rows
    q = dt.probes("mid")[7]
    R = np.float32(np.nanquantile(dt.distances_of("mid", "f16", "probes", True)[7], 0.02))
    exp = radius_expected(q, st, labels, R, 1000)
    assert 2000 < exp[3] < 8000 and abs(dt.distances_of("mid", "f16", "probes", True)[7, dt.copy_of("mid")] - R) > 0.01
    before = idx.guard_stats()
    got = raw_radius(mods, idx, 1000, q[None], R)
    rc.same(got, tuple(np.asarray(e)[None] for e in exp), "more members than cap")
    dl = delta(idx, before)
    assert dl["exhaustive"] == 0 and dl["radius_queries"] == 1, dl
    # the radius AT the copies' distance: more borderline rows than the sweep lists, the exhaustive pass decides
    q, R, e0, _e1 = dt.overflow_call("mid", "f16")
    exp = radius_expected(q[2], st, labels, R[2], 1000)
    assert exp[3] == e0[1][2]
    before = idx.guard_stats()
    got = raw_radius(mods, idx, 1000, q[2:3], R[2])
    rc.same(got, tuple(np.asarray(e)[None] for e in exp), "exhaustive")
    dl = delta(idx, before)
    assert dl["exhaustive"] == 1 and dl["radius_queries"] == 1 and quiet(dl), dl
    # by label, later_only: a copy near the end has the later copies as its only partners, all of them in the last trips
    copies = dt.copy_rows(N)
    rows = np.array([copies[-10], copies[-1], copies[dt.NCOPY // 2]])
    cap = 64
    exp = [radius_expected(ac.represented(st[r:r + 1])[0], st, labels, rc.ND_RADIUS, cap, row_min=int(r)) for r in rows]
    assert [int(e[3]) for e in exp] == [9, 0, dt.NCOPY - 1 - dt.NCOPY // 2]
    got = raw_radius(mods, idx, cap, by_label=labels[rows], max_dist=rc.ND_RADIUS, later_only=True)
    rc.same(got, tuple(np.stack([np.asarray(e[i]) for e in exp]) for i in range(4)), "later_only")
    assert set(got[0][0, :9].tolist()) == set(labels[copies[-9:]].tolist())
    print(f"radius mid f16: {time.time() - t0:.2f} s")


# ================================================================================================ subset search, mid size
@pytest.mark.parametrize("dtype", DTYPES)
def test_subset_search_over_five_compaction_blocks(mods, dtype):
    idx = index_of(mods, "mid", dtype)
    N, k = dt.MID_N, 50
    labels, st, q = dt.labels_of(N), dt.stored("mid", dtype), dt.subset_queries("mid")
    listed = dt.subset_list_rows(N)
    rng = np.random.Generator(np.random.Philox(17))
    cand = np.concatenate([labels[listed], labels[listed[::5]], sc.UNKNOWN])[rng.permutation(listed.size + listed[::5].size + sc.UNKNOWN.size)]
    plan = plan_of(mods, idx, 1)
    assert plan["compact_blocks"] == 5 and plan["compact_block_rows"] == dt.BLOCK, plan
    assert mods[3].index_subset_plan(idx._h, q.shape[0], k, cand.size)["compact_blocks"] == 5
    per_block = np.bincount(listed // plan["compact_block_rows"], minlength=5)
    assert per_block[2] == 0 and per_block[3] == plan["compact_block_rows"] and (per_block[[0, 1, 4]] > 0).all()
    idx.set_tags(labels, np.zeros(N, np.uint64))
    exp = sc.expected_subset(q, k, cand, st, labels)
    before = idx.guard_stats()
    got = raw_subset(mods, idx, q, k, cand)
    assert sc.mismatch(got[:3], exp[:3]) is None, (dtype, sc.mismatch(got[:3], exp[:3]))
    assert (got[3] == listed.size).all() and got[0][0, 0] == labels[0] and got[2][2] == 0
    assert all(v == 0 for v in delta(idx, before).values())
    # the bit-63 tag form: the filtered query over the rows that carry the bit is the same question
    bit = np.uint64(1 << 63)
    tags = np.zeros(N, np.uint64)
    tags[listed] = bit
    tags[::3] |= np.uint64(1)
    idx.set_tags(labels, tags)
    flat = idx.query(q, k, require=bit)
    assert sc.mismatch(got[:3], flat) is None
    got1 = raw_subset(mods, idx, q, k, cand, require=np.uint64(1))
    assert sc.mismatch(got1[:3], idx.query(q, k, require=bit | np.uint64(1))) is None and (got1[3] == listed.size).all()
    exp1 = sc.expected_subset(q[:2], k, cand, st, labels, tags, require=np.uint64(1))
    assert sc.mismatch(tuple(g[:2] for g in got1[:3]), exp1[:3]) is None
    idx.set_tags(labels, np.zeros(N, np.uint64))


# ================================================================================================ probed search, mid size
def test_probed_search_in_a_cell_of_more_than_65536_rows(mods):
    t0 = time.time()
    idx = index_of(mods, "mid", "f16")
    N, k = dt.MID_N, 20
    labels, st = dt.labels_of(N), dt.stored("mid", "f16")
    info = idx.build_partition(2, iters=3)
    try:
        assert info["largest_cell"] > 65536 and info["cells"] == 2 and info["rows"] == N, info
        centres, cells, sizes = idx.partition()
        with np.errstate(all="ignore"):
            km = ac.expected_kmeans(st, 2, 3, assign=lambda c, s: dt.expected_assign(c, s)[:3], sums=dt.expected_sums)
        assert np.array_equal(cells, km["assign"]) and np.array_equal(sizes, km["sizes"])
        q = np.array(dt.probes("mid")[20:24])
        q[1] = dt.rows("mid", False)[int(np.nonzero(cells == 1)[0][-1])]      # the last row of cell 1 is query 1's nearest row
        for nprobe in (1, 2):
            plan = mods[3].index_probe_plan(idx._h, q.shape[0], k, nprobe)
            assert plan["bound"] > 65536, plan
            exp = pc.expected_probed(q, k, nprobe, km["centres"], cells, N, st, labels)
            got = idx.query_probed(q, k, nprobe)
            assert pc.mismatch(got, exp) is None, (nprobe, pc.mismatch(got, exp))
        assert pc.mismatch(idx.query_probed(q, k, 2)[:3], idx.query(q, k)) is None
    finally:
        idx.clear_partition()
    print(f"probed mid f16: {time.time() - t0:.2f} s")


# ================================================================================================ top size
def test_top_size_membership_tagging_and_assignment(mods):
    t0 = time.time()
    idx = index_of(mods, "top", "f16")
    N = dt.TOP_N
    labels = dt.labels_of(N)
    plan = plan_of(mods, idx, 3)
    for kern in ("member_from_dist", "member_count", "member_merge_tags", "canonical_scan"):
        assert plan[kern]["trips"] >= 2, (kern, plan[kern])
    assert plan["rows"] == N and plan["scan"]["wave_trips"] >= 2
    q, R, e0, _e1 = dt.overflow_call("top", "f16")
    before = idx.guard_stats()
    got = raw_membership(mods, idx, q, R)
    check_membership(got, e0[:2], 3, "top")
    dl = delta(idx, before)
    assert dl["exhaustive"] == 1 and dl["radius_pages"] == 1 and N <= dl["swept_rows"] <= N + dt.MAX_CANONICAL_SHARE * 3 * N and quiet(dl), dl
    print(f"top membership: {time.time() - t0:.2f} s")
    # tag_by_radius into bits 63, 0, 17 over pre-set tags: the named bits are rewritten, every other bit is kept on every row
    t1 = time.time()
    bits = [63, 0, 17]
    old = np.random.Generator(np.random.Philox(99)).integers(0, 1 << 63, N, dtype=np.int64).view(np.uint64) * np.uint64(2) + np.uint64(1)
    idx.set_tags(labels, old)
    members = idx.tag_by_radius(q, R, bits)
    assert np.array_equal(members, e0[1])
    want = old & ~np.uint64(sum(1 << b for b in bits))
    for p, b in enumerate(bits):
        want |= e0[2][p].astype(np.uint64) << np.uint64(b)
    tags = idx.get_tags(labels)
    bad = np.nonzero(tags != want)[0]
    assert bad.size == 0, (bad[:5], [hex(int(v)) for v in tags[bad[:5]]], [hex(int(v)) for v in want[bad[:5]]])
    tail = mods[3].index_read_rows(idx._h, dt.D, idx.dtype, N - 4096, 4096)["tags"]      # the device copy, across the last trip's start
    assert np.array_equal(tail, want[N - 4096:])
    idx.set_tags(labels, np.zeros(N, np.uint64))
    print(f"top tagging: {time.time() - t1:.2f} s")
    # assignment with sizes
    t1 = time.time()
    plan = plan_of(mods, idx, 16)
    for kern in ("assign_decide", "assign_sizes", "assign_resolve"):
        assert plan[kern]["trips"] >= 2, (kern, plan[kern])
    at = dt.boundary_rows(N, plan)
    c, exp = dt.assign_call("top", "f16", 16, at)
    before = idx.guard_stats()
    got = raw_assign(mods, idx, c)
    check_assign(got, exp, "top", at)
    dl = delta(idx, before)
    assert dl["radius_pages"] == 1 and dl["swept_rows"] % 16 == 0 and 16 * len(dt.tie_rows(N)) <= dl["swept_rows"] < 16 * N / 2 and quiet(dl), dl
    print(f"top assignment: {time.time() - t1:.2f} s; top size in all {time.time() - t0:.2f} s")


# ================================================================================================ after a remove
def test_dead_copies_of_the_operands_stay_out_before_and_after_a_remove(mods):
    """The index is filled with the N rows and, behind them, 1000 copies of the probes and centres, cleared, and the N rows are
    added again: rows N .. N + 999 of the store, behind count, still hold the copies — dead rows that would be members of
    everything and the nearest row of every centre. Then 1000 rows spread over all trips are removed and the calls are repeated
    on the rows that closed up. (A remove compacts into a fresh allocation, so what lies behind count AFTER it is not the test's to
    choose: the hostile rows are planted before it, the way test_index_dead_rows_gpu.py plants its ghosts.)"""
    FlatIndex, ro, _roc, lib = mods
    N = dt.MID_N
    x, labels = dt.rows("mid", False), dt.labels_of(dt.MID_N + 1000)
    ops = np.concatenate([dt.probes("mid")[:17], dt.centres(16)])
    extra = ops[np.arange(1000) % ops.shape[0]]
    idx = FlatIndex(dt.D, "f16", capacity=N + 1000)
    try:
        idx.add(x, labels[:N])
        idx.add(extra, labels[N:])
        idx.clear()
        idx.add(x, labels[:N])
        assert idx.count() == N
        dead = lib.index_read_rows(idx._h, dt.D, idx.dtype, N, 1000)["rows"]
        with np.errstate(all="ignore"):
            assert np.array_equal(dead.astype(np.float32), ro.normalize_rows(extra, "f16").astype(np.float32), equal_nan=True)
        plan = plan_of(mods, idx, 17)
        assert plan["rows"] == N and plan["scan"]["wave_trips"] == 2 and plan["assign_resolve"]["trips"] >= 3, plan
        q, R, exp = dt.mixed_call("mid", "f16", 17)
        check_membership(raw_membership(mods, idx, q, R), exp, 17, "dead rows")
        c, exp = dt.assign_call("mid", "f16", 16)
        check_assign(raw_assign(mods, idx, c), exp, "dead rows")
        after = lib.index_read_rows(idx._h, dt.D, idx.dtype, N, 1000)["rows"]
        assert np.array_equal(after.view(np.uint16), dead.view(np.uint16))          # nothing written behind count
        # the remove: rows of both trips of every wave, and of the last reach of every grid
        gone = 70 + 139 * np.arange(1000)
        keep = np.setdiff1d(np.arange(N), gone)
        _s, w, t = dt.dense_position(gone, plan["scan"]["tiles_per_block"])
        assert {(int(a), int(b)) for a, b in zip(w, t)} == {(a, b) for a in range(4) for b in range(2)} and gone[-1] > 131072
        assert idx.remove(labels[gone]) == 1000 and idx.count() == N - 1000
        st = dt.stored("mid", "f16", False)[keep]
        plan = plan_of(mods, idx, 17)
        assert plan["rows"] == N - 1000 and plan["scan"]["wave_trips"] == 2 and plan["assign_resolve"]["trips"] >= 3, plan
        d = dt.exact_distances(q, st)
        R = dt.mixed_radii(d)
        exp = dt.expected_membership(q, st, R, d)
        check_membership(raw_membership(mods, idx, q, R), exp, 17, "after remove")
        exp = dt.expected_assign(c, st)
        check_assign(raw_assign(mods, idx, c), exp[:3], "after remove")
    finally:
        idx.close()

"""Dense radius membership and tagging of the flat index (mmiss_index_membership, mmiss_index_tag_by_radius) against the oracle:
the expected bit of (row r, probe p) is `oracle.retrieval_oracle.distances(q, stored)[p, r] <= R[p]` as floats (a NaN distance is
no member), stored = oracle.normalize_rows(x, dtype). Words and counts are compared for equality. Which route decided what is
read from the guard statistics: radius_pages (passes over the index), swept_rows ((row, probe) pairs resolved canonically),
exhaustive (probes that took the per-probe canonical route)."""
import warnings

import numpy as np
import pytest

from index_query_cases import load_mods
from oracle import retrieval_oracle as ro

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
D = 128
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
_cache = {}


@pytest.fixture(scope="module")
def mods():
    return load_mods()


def labels_of(n):
    return np.arange(n, dtype=np.int64) * 3 + 5


def corpus(seed, N, dim, P, nodir=True):
    """rows [N, dim], probes [P, dim]; nodir: rows without a direction (zero, NaN, +inf) at fixed places, and probe 1 (when there
    is one) without a direction. Cached: the tests share the arrays and leave them unchanged."""
    key = (seed, N, dim, P, nodir)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(seed))
        x = rng.standard_normal((N, dim), dtype=np.float32)
        q = rng.standard_normal((P, dim), dtype=np.float32)
        if nodir and N > 40:
            x[3] = 0.0
            x[17, 5] = np.nan
            x[N - 2, 0] = np.inf
            x[N // 2] = np.nan
            x[N // 2 + 1] = 0.0
            if P > 1:
                q[1] = 0.0
        x.setflags(write=False)
        q.setflags(write=False)
        _cache[key] = (x, q)
    return _cache[key]


def oracle_dist(key, q, x, dtype):
    """float32 [P, N] oracle distances, computed once per (corpus, dtype)"""
    k = ("dist", key, dtype)
    if k not in _cache:
        with np.errstate(all="ignore"):
            _cache[k] = ro.distances(q, ro.normalize_rows(x, dtype))
        _cache[k].setflags(write=False)
    return _cache[k]


def words_of(dist, R):
    """uint64 [N] expected words and int64 [P] expected counts"""
    with np.errstate(invalid="ignore"):
        mem = dist <= np.asarray(R, np.float32)[:, None]
    w = np.zeros(dist.shape[1], np.uint64)
    for p in range(dist.shape[0]):
        w |= mem[p].astype(np.uint64) << np.uint64(p)
    return w, mem.sum(1).astype(np.int64)


def mixed_radii(dist):
    """one radius per probe, the kinds in turn: negative, 0, the probe's median distance, >= 2, 0.9, +inf"""
    P = dist.shape[0]
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (the probe without a direction: an all-NaN row of distances)
        med = np.nanmedian(dist, axis=1).astype(np.float32)
    med = np.where(np.isnan(med), np.float32(1.0), med)
    kinds = [lambda p: -0.5, lambda p: 0.0, lambda p: med[p], lambda p: 2.5, lambda p: 0.9, lambda p: np.inf]
    order = [2, 0, 1, 3, 4, 5]   # probe 0 gets a median radius: a call of one probe has members and non-members
    return np.array([kinds[order[p % 6]](p) for p in range(P)], np.float32)


def make_index(mods, x, dtype, dim=D):
    idx = mods[0](dim, dtype)
    idx.add(x, labels_of(x.shape[0]))
    return idx


def delta(idx, before):
    after = idx.guard_stats()
    return {k: after[k] - before[k] for k in after}


# ================================================================================================ 1. oracle equality
@pytest.mark.parametrize("dtype", DTYPES)
def test_words_and_counts_equal_the_oracle(mods, dtype):
    N = 4999
    idx = None
    for P in (1, 16, 17, 64):
        x, q = corpus(11, N, D, 64)
        q = q[:P]
        dist = oracle_dist((11, N, D, 64), corpus(11, N, D, 64)[1], x, dtype)[:P]
        R = mixed_radii(dist)
        exp_w, exp_c = words_of(dist, R)
        if idx is None:
            idx = make_index(mods, x, dtype)
        before = idx.guard_stats()
        words, members = idx.membership(q, R)
        assert words.dtype == np.uint64 and words.shape == (N,) and members.dtype == np.int64 and members.shape == (P,)
        bad = np.nonzero(words != exp_w)[0]
        assert bad.size == 0, (dtype, P, bad[:5], [hex(int(v)) for v in words[bad[:5]]], [hex(int(v)) for v in exp_w[bad[:5]]])
        assert np.array_equal(members, exp_c), (dtype, P, members, exp_c)
        if P < 64:
            assert not (words >> np.uint64(P)).any()
        assert 0 < exp_c[0] < N                      # (the median radius: members and non-members)
        if P > 1:
            assert exp_c[1] == 0                     # the probe without a direction
        dl = delta(idx, before)
        assert dl["radius_queries"] == P and dl["radius_pages"] == 1, dl
        assert all(dl[s] == 0 for s in ("queries", "widened", "rounds", "pages")), dl
        # the rows without a direction are no member of anything, not even of a radius of +inf
        assert not words[[3, 17, N - 2, N // 2, N // 2 + 1]].any()


# ================================================================================================ 2. one-ulp borders
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_ulp_below_the_distance_is_no_member(mods, dtype):
    N, P = 4999, 8
    x, q = corpus(12, N, D, P, nodir=False)
    dist = oracle_dist((12, N, D, P, False), q, x, dtype)
    idx = make_index(mods, x, dtype)
    eps = mods[3].index_prep_queries(idx._h, D, idx.dtype, q)[2].astype(np.float64)
    rows = np.empty(P, np.int64)      # the planted row of probe p
    order = np.argsort(dist, axis=1)
    # the planted row of probe p is given the rank 10 + 300 p of that probe's distances: radii from tight to half the rows
    R = np.empty(P, np.float32)
    for p in range(P):
        rows[p] = order[p, 10 + 300 * p]
        R[p] = dist[p, rows[p]]
    for step, Rs in enumerate((R, np.nextafter(R, np.float32(-np.inf)))):
        exp_w, exp_c = words_of(dist, Rs)
        before = idx.guard_stats()
        words, members = idx.membership(q, Rs)
        assert np.array_equal(words, exp_w) and np.array_equal(members, exp_c), (dtype, step)
        got = (words[rows] >> np.arange(P, dtype=np.uint64)) & np.uint64(1)
        assert (got == (1 if step == 0 else 0)).all(), (dtype, step, got)
        dl = delta(idx, before)
        # the canonical route ran for the planted pairs at least, and only for pairs the guard's own inequality leaves open:
        # |approximate - canonical| <= eps_q on both sides of the threshold
        near = (np.abs((1.0 - dist.astype(np.float64)) - (1.0 - Rs.astype(np.float64))[:, None]) <= 2.0 * eps[:, None]).sum()
        print(dtype, "step", step, "swept", dl["swept_rows"], "bound", int(near), "eps", eps.max())
        assert P <= dl["swept_rows"] <= near, (dtype, step, dl, near)
        assert dl["exhaustive"] == 0 and dl["radius_pages"] == 1, dl


# ================================================================================================ 3. overflow route
@pytest.mark.parametrize("dtype", DTYPES)
def test_mass_duplicates_at_the_radius_take_the_canonical_pass(mods, dtype):
    N, NCOPY, P = 20000, 9000, 4
    key = ("dup", N, dtype)
    x, q = corpus(13, N, D, P, nodir=False)
    x = x.copy()
    copies = np.arange(N)[1::2][:NCOPY]
    x[copies] = x[1]
    dist = oracle_dist(key, q, x, dtype)
    assert (dist[2, copies].view(np.uint32) == dist[2, 1].view(np.uint32)).all()
    # probes 0, 1, 3 are ordinary (a fixed radius each: the copies sit on nobody else's threshold), probe 2's radius is exactly
    # its distance to the copies
    R = np.array([0.95, -0.5, dist[2, 1], 2.5], np.float32)
    assert np.abs(dist[0, 1] - R[0]) > 1e-3
    idx = make_index(mods, x, dtype)
    for step, Rs in enumerate((R, np.where(np.arange(P) == 2, np.nextafter(R, np.float32(-np.inf)), R).astype(np.float32))):
        exp_w, exp_c = words_of(dist, Rs)
        before = idx.guard_stats()
        words, members = idx.membership(q, Rs)
        assert np.array_equal(words, exp_w) and np.array_equal(members, exp_c), (dtype, step)
        is_member = ((words[copies] >> np.uint64(2)) & np.uint64(1)).astype(bool)
        assert is_member.all() if step == 0 else not is_member.any()
        dl = delta(idx, before)
        assert dl["exhaustive"] == 1 and dl["radius_pages"] == 1, dl


# ================================================================================================ 4. more probes than slots
def test_more_probes_than_slots_make_several_passes(mods):
    N, dim, P = 600, 1920, 40
    x, q = corpus(14, N, dim, P)
    dist = oracle_dist((14, N, dim, P), q, x, "f32")
    R = mixed_radii(dist)
    exp_w, exp_c = words_of(dist, R)
    idx = make_index(mods, x, "f32", dim)
    before = idx.guard_stats()
    words, members = idx.membership(q, R)
    assert np.array_equal(words, exp_w) and np.array_equal(members, exp_c)
    dl = delta(idx, before)
    assert dl["radius_pages"] > 1 and dl["radius_queries"] == P, dl


# ================================================================================================ 5. row-count edges
@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 257])
def test_row_count_edges_and_nothing_written_past_count(mods, N):
    P = 3
    lib = mods[3].load()
    for dtype in DTYPES:
        x, q = corpus(15, 257, D, P, nodir=False)
        x = x[:N]
        dist = oracle_dist((15, 257, D, P, False), q, corpus(15, 257, D, P, nodir=False)[0], dtype)[:, :N]
        R = np.array([np.median(dist[0]), 2.5, np.median(dist[2])], np.float32)
        exp_w, exp_c = words_of(dist, R)
        idx = make_index(mods, x, dtype)
        out = np.full(N + 64, SENTINEL, np.uint64)
        members = np.full(P + 2, -7, np.int64)
        mods[3].check(lib.mmiss_index_membership(idx._h, q.ctypes.data, P, R.ctypes.data, out.ctypes.data, N + 64, members.ctypes.data))
        assert np.array_equal(out[:N], exp_w), (dtype, N)
        assert (out[N:] == SENTINEL).all(), (dtype, N)
        assert np.array_equal(members[:P], exp_c) and (members[P:] == -7).all(), (dtype, N, members)
        assert exp_c[1] == N


# ================================================================================================ 6. tag_by_radius
@pytest.mark.parametrize("dtype", DTYPES)
def test_tag_by_radius_overwrites_the_named_bits_only(mods, dtype):
    N, P, k = 2000, 3, 10
    bits = [63, 0, 17]
    x, q = corpus(16, N, D, P)
    dist = oracle_dist((16, N, D, P), q, x, dtype)
    labels = labels_of(N)
    with np.errstate(all="ignore"):
        R = np.array([np.nanmedian(dist[0]), 0.9, np.nanquantile(dist[2], 0.25)], np.float32)   # probe 1 has no direction
        mem = dist <= R[:, None]
    expected = np.zeros(N, np.uint64)
    for p, b in enumerate(bits):
        expected |= mem[p].astype(np.uint64) << np.uint64(b)
    M = np.uint64(sum(1 << b for b in bits))
    idx = make_index(mods, x, dtype)
    rng = np.random.Generator(np.random.Philox(99))
    for old in (np.full(N, ~np.uint64(0), np.uint64), rng.integers(0, 1 << 63, N, dtype=np.int64).view(np.uint64) * np.uint64(2) + np.uint64(1)):
        idx.set_tags(labels, old)
        members = idx.tag_by_radius(q, R, bits)
        assert np.array_equal(members, mem.sum(1)), (dtype, members)
        want = (old & ~M) | expected
        assert np.array_equal(idx.get_tags(labels), want), dtype
        assert np.array_equal(mods[3].index_read_rows(idx._h, D, idx.dtype, 0, N)["tags"], want), dtype   # device copy and mirror agree
    # the tag feeds the filtered query: the exact top-k among the members of probe 2
    sub = np.nonzero(mem[2])[0]
    with np.errstate(all="ignore"):
        stored = ro.normalize_rows(x, dtype)
        ol, od, oc = ro.query(q[2:3], stored[sub], labels[sub], k)
    lab, dd, cnt = idx.query(q[2:3], k, require=np.uint64(1 << 17))
    assert np.array_equal(lab, ol) and np.array_equal(dd.view(np.uint32), od.view(np.uint32)) and np.array_equal(cnt, oc)
    # a stale host mirror would lose the tags here: remove() rebuilds the device tags from it
    gone = np.arange(N)[::10]
    keep = np.setdiff1d(np.arange(N), gone)
    assert idx.remove(labels[gone]) == gone.size
    assert np.array_equal(idx.get_tags(labels[keep]), want[keep])
    assert np.array_equal(mods[3].index_read_rows(idx._h, D, idx.dtype, 0, keep.size)["tags"], want[keep])
    new = np.arange(4, dtype=np.int64) + labels[-1] + 1
    idx.add(x[:4], new)
    assert not idx.get_tags(new).any()
    assert np.array_equal(idx.get_tags(labels[keep]), want[keep])


# ================================================================================================ 7. device in / out
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_inputs_and_outputs_give_the_same_bits(mods, dtype):
    import torch

    N, P = 4999, 17
    x, q = corpus(11, N, D, 64)
    q = q[:P]
    dist = oracle_dist((11, N, D, 64), corpus(11, N, D, 64)[1], x, dtype)[:P]
    R = mixed_radii(dist)
    idx = make_index(mods, x, dtype)
    hw, hm = idx.membership(q, R)
    dw, dm = idx.membership(torch.from_numpy(np.array(q)).cuda(), torch.from_numpy(R).cuda())
    assert dw.is_cuda and dm.is_cuda and dw.dtype == torch.int64 and dm.dtype == torch.int64
    assert np.array_equal(dw.cpu().numpy().view(np.uint64), hw) and np.array_equal(dm.cpu().numpy(), hm)
    assert np.array_equal(hw, words_of(dist, R)[0])
    # mixed: device queries, host radii
    dw2, dm2 = idx.membership(torch.from_numpy(np.array(q)).cuda(), R)
    assert np.array_equal(dw2.cpu().numpy().view(np.uint64), hw) and np.array_equal(dm2.cpu().numpy(), hm)
    tm = idx.tag_by_radius(torch.from_numpy(np.array(q[:3])).cuda(), torch.from_numpy(R[:3]).cuda(), [5, 6, 7])
    assert tm.is_cuda and np.array_equal(tm.cpu().numpy(), hm[:3])
    assert np.array_equal(idx.get_tags(labels_of(N)), (hw & np.uint64(7)) << np.uint64(5))


# ================================================================================================ 8. errors change nothing
def test_errors_change_nothing(mods):
    FlatIndex, _, _, _lib = mods
    lib = _lib.load()
    N, P = 300, 3
    x, q = corpus(17, N, D, P, nodir=False)
    labels = labels_of(N)
    idx = make_index(mods, x, "f16")
    tags = np.random.Generator(np.random.Philox(5)).integers(0, 1 << 62, N, dtype=np.int64).view(np.uint64)
    idx.set_tags(labels, tags)
    R = np.full(P, 1.0, np.float32)
    out = np.full(N, SENTINEL, np.uint64)
    members = np.full(P, -7, np.int64)

    def unchanged():
        assert np.array_equal(idx.get_tags(labels), tags)
        assert np.array_equal(_lib.index_read_rows(idx._h, D, idx.dtype, 0, N)["tags"], tags)
        assert (out == SENTINEL).all() and (members == -7).all()

    def refused(status, code=-1):
        assert status == code, status
        unchanged()

    h = idx._h
    b3 = np.array([1, 2, 3], np.int32)
    q65 = np.zeros((65, D), np.float32)
    r65 = np.ones(65, np.float32)
    b65 = np.arange(65, dtype=np.int32)
    refused(lib.mmiss_index_membership(h, q.ctypes.data, 0, R.ctypes.data, out.ctypes.data, N, members.ctypes.data))
    refused(lib.mmiss_index_tag_by_radius(h, q.ctypes.data, 0, R.ctypes.data, b3.ctypes.data, members.ctypes.data))
    refused(lib.mmiss_index_membership(h, q65.ctypes.data, 65, r65.ctypes.data, out.ctypes.data, N, None))
    refused(lib.mmiss_index_tag_by_radius(h, q65.ctypes.data, 65, r65.ctypes.data, b65.ctypes.data, None))
    rn = np.array([1.0, np.nan, 1.0], np.float32)
    refused(lib.mmiss_index_membership(h, q.ctypes.data, P, rn.ctypes.data, out.ctypes.data, N, members.ctypes.data))
    refused(lib.mmiss_index_tag_by_radius(h, q.ctypes.data, P, rn.ctypes.data, b3.ctypes.data, members.ctypes.data))
    for bad in ([1, 2, 1], [1, 64, 3], [-1, 2, 3]):
        bb = np.array(bad, np.int32)
        refused(lib.mmiss_index_tag_by_radius(h, q.ctypes.data, P, R.ctypes.data, bb.ctypes.data, members.ctypes.data))
        with pytest.raises(_lib.MmissError):
            idx.tag_by_radius(q, R, bad)
        unchanged()
    refused(lib.mmiss_index_membership(h, q.ctypes.data, P, R.ctypes.data, out.ctypes.data, N - 1, members.ctypes.data))
    refused(lib.mmiss_index_membership(h, None, P, R.ctypes.data, out.ctypes.data, N, members.ctypes.data))
    refused(lib.mmiss_index_membership(h, q.ctypes.data, P, None, out.ctypes.data, N, members.ctypes.data))
    refused(lib.mmiss_index_membership(h, q.ctypes.data, P, R.ctypes.data, None, N, members.ctypes.data))
    refused(lib.mmiss_index_tag_by_radius(h, q.ctypes.data, P, R.ctypes.data, None, members.ctypes.data))
    with pytest.raises(_lib.MmissError):
        idx.membership(q, rn)
    with pytest.raises(_lib.MmissError):
        idx.membership(np.zeros((0, D), np.float32), np.zeros(0, np.float32))
    unchanged()
    # while a query is open the handle's scratch belongs to it
    pending = idx.query_begin(q, 5)
    assert lib.mmiss_index_membership(h, q.ctypes.data, P, R.ctypes.data, out.ctypes.data, N, members.ctypes.data) == -3
    assert lib.mmiss_index_tag_by_radius(h, q.ctypes.data, P, R.ctypes.data, b3.ctypes.data, members.ctypes.data) == -3
    first = pending.result()
    unchanged()                                   # (get_tags itself is refused while the query is open)
    again = idx.query(q, 5)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # the calls still work after all of that
    words, mem = idx.membership(q, R)
    assert words.shape == (N,) and mem.sum() == sum(bin(int(v)).count("1") for v in words)
    unchanged()
    # an empty index: nothing is written but zeros to the counts
    empty = FlatIndex(D, "f16")
    w0, m0 = empty.membership(q, R)
    assert w0.shape == (0,) and np.array_equal(m0, np.zeros(P, np.int64))
    m1 = np.full(P, -7, np.int64)
    _lib.check(lib.mmiss_index_membership(empty._h, q.ctypes.data, P, R.ctypes.data, out.ctypes.data, N, m1.ctypes.data))
    assert (out == SENTINEL).all() and not m1.any()
    m1[:] = -7
    _lib.check(lib.mmiss_index_tag_by_radius(empty._h, q.ctypes.data, P, R.ctypes.data, b3.ctypes.data, m1.ctypes.data))
    assert not m1.any() and empty.count() == 0

"""Radius queries and near-duplicate pairs of the flat index (mmiss_index_query_radius, _by_label) against the oracle: labels,
counts and totals for equality, distances as bits. The expected answers and the properties of the corpora they rest on are in
tests/radius_cases.py and test_radius_cases_cpu.py. The path of every call is read from mmiss_dbg_index_radius_plan and asserted
before it runs; the kernels that ran are read from mmiss_prof_read after it."""
import numpy as np
import pytest

import planted_rows as pr
import radius_cases as rc
from index_query_cases import ALL_DTYPES, VIAS, Case, fill_with_ghosts, labels_of, load_mods
from oracle import retrieval_oracle as ro

pytestmark = pytest.mark.gpu

CORPORA = [(pr.N_SCAN, pr.D, 10), (pr.N_DENSE, pr.D_STRIP, 10), (pr.N_SAMPLE, pr.D_STRIP, 10)]
SCAN_QS = [(1, 1), (17, 2), (40, 4), (64, 4)]     # (queries per call, query tiles of 16 per block)


@pytest.fixture(scope="module")
def mods():
    return load_mods()


def _index(mods, case, dtype, ghosts=None, tmp_path=None):
    FlatIndex = mods[0]
    p = case.corpus()
    idx = FlatIndex(case.D, dtype, capacity=case.N)
    if not (ghosts and fill_with_ghosts(mods, idx, p, dtype, ghosts, tmp_path)):
        idx.add(p.rows, labels_of(case.N))
    if case.filtered:
        idx.set_tags(labels_of(case.N), p.tags)
    return idx, p


def _gemm_route(dtype, D, Q, filtered=False):
    return (not filtered) and dtype in ("f16", "f8") and D >= 256 and Q > 64


def _sweep(mods, idx, p, dtype, D, Q, exp, cap, radius=rc.RADIUS, filtered=False, which=None, what=""):
    """all queries `which` of p, Q per call, at one radius; the plan asserted before, the kernels after; -> the stacked answer"""
    _lib = mods[3]
    which = np.arange(p.n_queries) if which is None else np.asarray(which)
    plan = _lib.index_radius_plan(idx._h, Q, filtered)
    gemm = _gemm_route(dtype, D, Q, filtered)
    assert plan["chunks"] == 1 and plan["first"]["queries"] == Q and plan["first"]["gemm"] == int(gemm), plan
    if gemm:
        assert plan["first"]["strip"] >= 1 and plan["first"]["nqt"] == 0
    else:
        assert plan["first"]["nqt"] == (4 if Q > 32 else 2 if Q > 16 else 1) and plan["first"]["qtiles"] == -(-Q // (16 * plan["first"]["nqt"]))
        assert plan["first"]["slabs"] >= 1 and plan["first"]["tiles_per_block"] >= 4
    out = [[], [], [], []]
    _lib.prof_reset()
    _lib.prof_enable(True)
    before = idx.guard_stats()
    try:
        for j0 in range(0, which.size, Q):
            sl = which[j0:j0 + Q]
            kw = {"require": p.require[sl], "exclude": p.exclude[sl]} if filtered else {}
            for o, g in zip(out, idx.query_radius(p.queries[sl], radius, cap, **kw)):
                o.append(g)
    finally:
        _lib.prof_enable(False)
    after = idx.guard_stats()
    ran = {r["kernel"] for r in _lib.prof_read()}
    sweep = ("sweep_gemm_" if gemm else "sweep_scan_") + dtype
    assert {sweep, "radius_thr", "rerank", "prep_queries"} <= ran and not ran & {"canonical_scan", "rows_as_queries"}, ran
    assert not any(k.startswith(("scan_topk", "score_gemm", "merge", "select")) for k in ran), ran
    got = tuple(np.concatenate(o) for o in out)
    rc.same(got, tuple(e[which] for e in exp), what)
    delta = {s: after[s] - before[s] for s in after}
    assert delta["radius_queries"] == which.size and delta["exhaustive"] == 0, delta
    assert all(delta[s] == 0 for s in ("queries", "widened", "rounds", "pages")), delta
    calls = -(-which.size // Q)
    if gemm:
        assert delta["radius_pages"] == calls, delta
    assert not (got[0] >= pr.GHOST_LABEL0).any()
    return got


# ================================================================================================ positions
@pytest.mark.parametrize("layout", list(pr.LAYOUTS))
@pytest.mark.parametrize("N,D,k", CORPORA)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_every_row_position_is_a_member_exactly_once(mods, dtype, N, D, k, layout):
    case = Case(N, D, k, layout)
    cap = k + 6
    exp = rc.planted_expected(case, dtype, cap)
    idx, p = _index(mods, case, dtype)
    try:
        for Q, nqt in SCAN_QS + [(70, 4), (300, 4)]:
            got = _sweep(mods, idx, p, dtype, D, Q, exp, cap, what=f"{dtype} N={N} {layout} Q={Q}")
            lab = got[0][got[0] >= 0]
            np.testing.assert_array_equal(np.sort(lab), labels_of(N))       # every row of the index, exactly once
            assert (got[3][:p.n_full] == k).all() and (got[2][:p.n_full] == k).all()
    finally:
        idx.close()


# ================================================================================================ boundaries
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_radii_at_a_members_own_distance_mixed_in_one_call(mods, dtype):
    import torch

    case = Case(pr.N_SCAN, pr.D, 10, "scattered")
    idx, p = _index(mods, case, dtype)
    try:
        stored = ro.normalize_rows(p.rows, dtype)
        labels = labels_of(case.N)
        qs, radii = [], []
        for j in (0, 7, p.n_full - 1):
            d = np.sort(ro.distances(p.queries[j:j + 1], stored)[0][p.rows_of(j)])
            for t in range(case.k):
                for r in rc.boundary_radii(d, t):
                    qs.append(j), radii.append(r)
        qs, radii = np.array(qs), np.array(radii, np.float32)
        exp = rc.expected(p.queries[qs], stored, labels, radii, 16)
        np.testing.assert_array_equal(exp[3], np.tile(np.repeat(np.arange(case.k), 2) + np.tile([1, 0], case.k), 3))
        rc.same(idx.query_radius(p.queries[qs], radii, 16), exp, "host radii")
        dev = torch.device("cuda")
        got = idx.query_radius(torch.from_numpy(p.queries[qs]).to(dev), torch.from_numpy(radii).to(dev), 16)
        assert all(g.is_cuda for g in got)
        rc.same(tuple(g.cpu().numpy() for g in got), exp, "device radii, queries and outputs")
        got = idx.query_radius(torch.from_numpy(p.queries[qs]).to(dev), radii, 16)
        rc.same(tuple(g.cpu().numpy() for g in got), exp, "host radii, device queries")
    finally:
        idx.close()


# ================================================================================================ cap below total, extremes
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_cap_below_total_and_extreme_radii(mods, dtype):
    case = Case(pr.N_SCAN, pr.D, 10, "scattered")
    idx, p = _index(mods, case, dtype)
    try:
        which = np.arange(20)
        full = rc.planted_expected(case, dtype, 16)
        lab, dist, cnt, tot = idx.query_radius(p.queries[which], rc.RADIUS, 3)
        np.testing.assert_array_equal(lab, full[0][which, :3])
        np.testing.assert_array_equal(dist.view(np.uint32), full[1][which, :3].view(np.uint32))
        assert (cnt == 3).all() and (tot == 10).all()
        lab, dist, cnt, tot = idx.query_radius(p.queries[which], -1.0, 8)
        assert (lab == -1).all() and np.isinf(dist).all() and (cnt == 0).all() and (tot == 0).all()
    finally:
        idx.close()
    # radius 2.5 over 1000 rows (two of them without a direction), cap 4096: every row with a direction, in oracle order
    FlatIndex = mods[0]
    rows = p.rows[:1000].copy()
    rows[17] = 0.0
    rows[500] = np.nan
    labels = labels_of(1000)
    idx = FlatIndex(case.D, dtype, capacity=1000)
    try:
        idx.add(rows, labels)
        stored = ro.normalize_rows(rows, dtype)
        exp = rc.expected(p.queries[:3], stored, labels, 2.5, 4096)
        assert (exp[3] == 998).all()
        rc.same(idx.query_radius(p.queries[:3], 2.5, 4096), exp, "radius 2.5")
        rc.same(idx.query_radius(p.queries[:3], np.float32(np.inf), 4096), exp, "radius +inf")
    finally:
        idx.close()


# ================================================================================================ long lists
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_list_longer_than_the_first_rerank_launch(mods, dtype):
    FlatIndex = mods[0]
    nd, stored = rc.near_dup_corpus(), rc.near_dup_stored(dtype)
    idx = FlatIndex(rc.ND_D, dtype, capacity=rc.ND_N)
    try:
        idx.add(nd.rows, nd.labels)
        q = rc.represented(stored)[nd.big[[0, 5]]]
        q = np.concatenate([q, nd.rows[nd.groups[2][:1]]])       # ... and a short list in the same call
        exp = rc.expected(q, stored, nd.labels, rc.ND_RADIUS, 2048)
        assert (exp[3][:2] > rc.SWEEP_FAST).all() and exp[3][2] == 17
        before = idx.guard_stats()
        rc.same(idx.query_radius(q, rc.ND_RADIUS, 2048), exp, "second re-rank launch")
        after = idx.guard_stats()
        assert after["exhaustive"] == before["exhaustive"] and after["swept_rows"] - before["swept_rows"] >= int(exp[3].sum())
    finally:
        idx.close()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_plateau_goes_through_the_exhaustive_pass(mods, dtype):
    import torch

    FlatIndex, _, _, _lib = mods
    p = pr.plateau(pr.N_PLATEAU, pr.D, pr.SEED)
    labels = labels_of(pr.N_PLATEAU)
    stored = ro.normalize_rows(p.rows, dtype)
    idx = FlatIndex(pr.D, dtype, capacity=pr.N_PLATEAU)
    try:
        idx.add(p.rows, labels)
        tied = float(ro.distances(p.queries[:1], stored)[0][p.rows_of(0)[0]])
        q = p.queries[[0, 2]]
        radii = np.array([tied, 0.0], np.float32)                # the tied distance; a random query with no member
        exp = rc.expected(q, stored, labels, radii, 50)
        assert exp[3][0] == pr.N_PLATEAU - pr.PLATEAU_OTHERS == 9000 and exp[3][1] == 0
        np.testing.assert_array_equal(exp[0][0], labels[p.rows_of(0)[:50]])     # the cap smallest labels
        before = idx.guard_stats()
        _lib.prof_reset()
        _lib.prof_enable(True)
        try:
            got = idx.query_radius(q, radii, 50)
        finally:
            _lib.prof_enable(False)
        assert "canonical_scan" in {r["kernel"] for r in _lib.prof_read()}
        rc.same(got, exp, "exhaustive, host outputs")
        assert idx.guard_stats()["exhaustive"] - before["exhaustive"] == 1
        got = idx.query_radius(torch.from_numpy(q).cuda(), radii, 50)
        rc.same(tuple(g.cpu().numpy() for g in got), exp, "exhaustive, device outputs")
    finally:
        idx.close()


# ================================================================================================ filtered
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_filtered_members_only_admitted_winners(mods, dtype, mirrored):
    import torch

    case = Case(pr.N_SCAN, pr.D, 10, "scattered", True, mirrored)
    idx, p = _index(mods, case, dtype)
    try:
        labels = labels_of(case.N)
        exp = rc.planted_expected(case, dtype, 16)       # the cached filtered top-k: the admitted winners (0.12 .. 0.25)
        assert (exp[3][:p.n_full] == case.k).all()
        for Q in (16, 70):
            got = _sweep(mods, idx, p, dtype, case.D, Q, exp, 16, filtered=True, what=f"filtered {dtype} Q={Q}")
            assert not np.isin(got[0], labels[p.decoy]).any()
        # masks as CUDA tensors
        sl = np.arange(40)
        dev = torch.device("cuda")
        as_i64 = lambda m: torch.from_numpy(m.view(np.int64)).to(dev)
        got = idx.query_radius(torch.from_numpy(p.queries[sl]).to(dev), float(rc.RADIUS), 16, require=as_i64(p.require[sl]),
                               exclude=as_i64(p.exclude[sl]))
        rc.same(tuple(g.cpu().numpy() for g in got), tuple(e[sl] for e in exp), "CUDA masks")
        # exclude only: a query's winners and nothing of its decoys
        stored = ro.normalize_rows(p.rows, dtype)
        ok = np.zeros(case.N, bool)
        ok[pr.not_excluded(p)] = True
        exp_x = rc.expected(p.queries[:5], stored, labels, rc.RADIUS, 16, admit=lambda j: ok)
        rc.same(idx.query_radius(p.queries[:5], rc.RADIUS, 16, exclude=p.exclude[:5]), exp_x, "exclude only")
        # a predicate nothing satisfies
        lab, dist, cnt, tot = idx.query_radius(p.queries[:5], rc.RADIUS, 16, require=np.uint64(1) << np.uint64(62), exclude=p.exclude[:5])
        assert (lab == -1).all() and (cnt == 0).all() and (tot == 0).all()
    finally:
        idx.close()


# ================================================================================================ dead rows behind count
@pytest.mark.parametrize("kind", ["twin", "nonfinite"])
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_dead_rows_behind_count_are_never_members(mods, dtype, via, kind, tmp_path):
    """the ghosts copy the query directions (cosine 1.0): one that leaked would be a member at any radius"""
    case = Case(pr.N_DENSE, pr.D_STRIP, 10, "scattered")
    exp = rc.planted_expected(case, dtype, 16)
    idx, p = _index(mods, case, dtype, ghosts=(kind, via), tmp_path=tmp_path)
    try:
        which = np.arange(p.n_queries - 600, p.n_queries)       # (behind count the ghosts copy the queries in turn: each has twins)
        for Q in (64, 300):                                     # the scan; the strip GEMM on f16 / fp8 rows
            _sweep(mods, idx, p, dtype, case.D, Q, exp, 16, which=np.concatenate([np.arange(300), which]), what=f"ghosts {kind} {via} Q={Q}")
    finally:
        idx.close()


# ================================================================================================ no direction, errors
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_no_direction_nan_radius_and_open_query(mods, dtype):
    case = Case(pr.N_SCAN, pr.D, 10, "scattered")
    FlatIndex = mods[0]
    p = case.corpus()
    rows = p.rows.copy()
    bad_rows = p.rows_of(3)[:3]
    rows[bad_rows[0]], rows[bad_rows[1]], rows[bad_rows[2]] = 0.0, np.nan, np.inf
    labels = labels_of(case.N)
    idx = FlatIndex(case.D, dtype, capacity=case.N)
    try:
        idx.add(rows, labels)
        q = p.queries[:6].copy()
        q[0], q[1], q[2, 5] = 0.0, np.nan, np.inf
        lab, dist, cnt, tot = idx.query_radius(q, 2.5, 32)
        assert (cnt[:3] == 0).all() and (tot[:3] == 0).all() and (lab[:3] == -1).all()
        assert tot[4] == case.N - 3 and not np.isin(lab, labels[bad_rows]).any()
        exp = rc.expected(q[3:], ro.normalize_rows(rows, dtype), labels, rc.RADIUS, 32)
        assert exp[3][0] == case.k - 3
        rc.same(idx.query_radius(q[3:], rc.RADIUS, 32), exp, "rows without a direction")
        with pytest.raises(RuntimeError):
            idx.query_radius(q[3:], np.array([0.3, np.nan, 0.3], np.float32), 32)
        with pytest.raises(RuntimeError):
            idx.query_radius(q[3:], 0.3, 4097)
        ref = idx.query(p.queries[:8], 10)
        pending = idx.query_begin(p.queries[:8], 10)
        with pytest.raises(RuntimeError):
            idx.query_radius(q[3:], 0.3, 32)
        with pytest.raises(RuntimeError):
            idx.query_radius_by_label(labels[:2], 0.3, 32)
        for a, b in zip(pending.result(), ref):                 # the open query still delivers
            np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
        empty = FlatIndex(case.D, dtype)
        try:
            lab, dist, cnt, tot = empty.query_radius(p.queries[:3], 2.5, 4)
            assert (lab == -1).all() and np.isinf(dist).all() and (cnt == 0).all() and (tot == 0).all()
        finally:
            empty.close()
    finally:
        idx.close()


# ================================================================================================ _by_label, near_duplicates
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_by_label_and_near_duplicates(mods, dtype):
    import torch

    FlatIndex, _, _, _lib = mods
    nd = rc.near_dup_corpus()
    idx = FlatIndex(rc.ND_D, dtype, capacity=rc.ND_N)
    try:
        idx.add(nd.rows, nd.labels)
        cap = 1200
        some = np.concatenate([g[:2] for g in nd.groups] + [np.arange(0, rc.ND_N, 97)])
        lab = nd.labels[some]
        host = idx.query_radius_by_label(lab, rc.ND_RADIUS, cap)
        rc.same(host, idx.query_radius(idx.get(lab), rc.ND_RADIUS, cap), "by label = query_radius(get(labels))")
        dev = idx.query_radius_by_label(lab, rc.ND_RADIUS, cap, device="cuda")
        assert all(g.is_cuda for g in dev)
        rc.same(tuple(g.cpu().numpy() for g in dev), host, "device outputs")
        assert (host[3] >= 1).all()                                  # the self match
        # a label that is not stored: raises, writes nothing
        with pytest.raises(RuntimeError):
            idx.query_radius_by_label(np.array([lab[0], 4], np.int64), rc.ND_RADIUS, 4)
        # later_only over every label: the oracle's pair set, each pair once, never (a, a), ordered (a, dist, b)
        (ea, eb, ed), _ = rc.near_dup_pairs(dtype)
        before = idx.guard_stats()
        _lib.prof_reset()
        _lib.prof_enable(True)
        try:
            a, b, d, overflow = idx.near_duplicates(rc.ND_RADIUS, cap_per_row=cap)
        finally:
            _lib.prof_enable(False)
        ran = {r["kernel"] for r in _lib.prof_read()}
        assert "rows_as_queries" in ran and "radius_thr" in ran, ran
        after = idx.guard_stats()
        assert after["radius_queries"] - before["radius_queries"] == rc.ND_N and overflow == {}
        np.testing.assert_array_equal(a, ea)
        np.testing.assert_array_equal(b, eb)
        np.testing.assert_array_equal(d.view(np.uint32), ed.view(np.uint32))
        assert (a < b).all()
        # a small cap: the nearest partners and the totals of the rows that have more
        a2, b2, d2, overflow = idx.near_duplicates(rc.ND_RADIUS, cap_per_row=64)
        counts = {int(x): int(n) for x, n in zip(*np.unique(ea, return_counts=True))}
        assert overflow == {x: n for x, n in counts.items() if n > 64}
        keep = np.concatenate([np.nonzero(ea == x)[0][:64] for x in np.unique(ea)])
        np.testing.assert_array_equal(a2, ea[keep])
        np.testing.assert_array_equal(b2, eb[keep])
        # n = 2500 labels in one call (three chunks) = three separate calls
        many = nd.labels[:2500]
        plan = _lib.index_radius_plan(idx._h, 2500)
        assert plan["chunks"] == 3 and plan["first"]["queries"] == 1024 and plan["last"]["queries"] == 452, plan
        one = idx.query_radius_by_label(many, rc.ND_RADIUS, 32, later_only=True)
        parts = [idx.query_radius_by_label(many[i:i + 1024], rc.ND_RADIUS, 32, later_only=True) for i in (0, 1024, 2048)]
        rc.same(one, tuple(np.concatenate([x[i] for x in parts]) for i in range(4)), "three chunks")
    finally:
        idx.close()


# ================================================================================================ statistics
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_statistics_and_topk_unchanged_by_radius_calls(mods, dtype):
    case = Case(pr.N_DENSE, pr.D_STRIP, 10, "scattered")
    idx, p = _index(mods, case, dtype)
    try:
        ref = idx.query(p.queries[:70], 10)
        before = idx.guard_stats()
        idx.query_radius(p.queries[:100], rc.RADIUS, 16)            # 100 queries: the GEMM (1 pass) or the scan (2 query tiles of 64)
        idx.query_radius(p.queries[:5], rc.RADIUS, 16)
        after = idx.guard_stats()
        delta = {s: after[s] - before[s] for s in after}
        gemm = _gemm_route(dtype, case.D, 100)
        assert delta["radius_queries"] == 105 and delta["radius_pages"] == (1 if gemm else 2) + 1, delta
        assert all(delta[s] == 0 for s in ("queries", "widened", "rounds", "pages", "exhaustive")) and delta["swept_rows"] >= 1050, delta
        again = idx.query(p.queries[:70], 10)
        for a, b in zip(again, ref):
            np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    finally:
        idx.close()

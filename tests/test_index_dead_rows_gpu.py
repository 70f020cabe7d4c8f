"""The other half of the index's row contract: nothing behind `count` may become a result, take a slot in a candidate list, raise
a group maximum or cause a widen pass. test_index_positions_gpu.py queries fresh indexes, whose rows behind count are whatever
the allocator returned; here every path of it runs on an index whose capacity was first filled with hostile rows
(planted_rows.ghosts: exact copies of the query directions, cosine 1.0 against the best live row's 0.95; or NaN / inf / zero
rows) and then emptied by clear(), by a remove of every row, or by a load of a smaller file over it. All of these keep the row
bytes and the device labels behind count; inverse norms (fp8 rows) and tags are zeroed. The kernels read behind count on purpose
(the scan its whole last 16-row tile, the score GEMMs up to a multiple of 128 or 256 rows), so the masks `row < N` of the scans,
`n < p0` of the GROUPMAX and threshold-append epilogues and `row >= nrows` of the re-rank are the whole defence: a twin that
leaks comes back under a ghost label (>= planted_rows.GHOST_LABEL0), one that only enters a stage-1 list displaces a winner or
makes the guard flag its query. Either fails here: ids, distance bits and counts of every query are compared with the oracle
over the live rows, first-pass tests require that no query widened and no widen kernel ran, forced-widen tests that every query
widened and none ended in the exhaustive pass. The path is read from mmiss_dbg_index_plan and asserted before the run.

fp8 rows have a second defence, the zero inverse norm (a dead row scores 0): a lost mask shows on them only where a score of 0
competes: the tiny live sets (k >= live rows, live rows of negative cosine) and the plateau's query of negative cosine.

Behind a partial remove and a growth of the capacity lie fresh buffers, so nothing can be planted there; what can go wrong is a
live row lost or shifted: the compaction, growth and update tests at the end compare every query again."""
import functools

import numpy as np
import pytest

import planted_rows as pr
from index_query_cases import (ALL_DTYPES, Case, check_queries, dense_names, expected, fill_with_ghosts, labels_of, load_mods,
                               options_set, run, scan_names)

pytestmark = pytest.mark.gpu

TWIN = ("twin", "clear")
LAYOUT = "scattered"         # the ghosts' positions matter here, not the live layout
SCAN_CASE = Case(pr.N_SCAN, pr.D, 10, LAYOUT)
FILT_CASES = [Case(pr.N_SCAN, pr.D, 10, LAYOUT, True, mirrored) for mirrored in (False, True)]
DENSE_CASE = Case(pr.N_DENSE, pr.D_STRIP, 10, LAYOUT)


@pytest.fixture(scope="module")
def mods():
    return load_mods()


def _scan16_check(pl):
    assert not pl["dense"] and pl["nqt"] == 1 and pl["cap"] == 64 and pl["kp"] == 16 and pl["pages"] == 1


def _scan_or_gemm128(dtype, Q, pl, nqt):
    """Q > 16 on f16 rows is the 128-query score GEMM; f32 and fp8 rows stay on the scan with nqt query tiles"""
    if dtype == "f16" and Q > 16:
        assert pl["dense"] and not pl["big"] and pl["Mq"] == 128 and pl["Npad"] - pr.N_SCAN == 125
        return dense_names("f16")
    assert not pl["dense"] and pl["nqt"] == nqt
    return scan_names(dtype)


# ================================================================================================ first pass: streaming scan
@pytest.mark.parametrize("k", [10, 24])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_scan_16_query_tile(mods, dtype, k):
    """the last 16-row tile holds 3 live rows and 13 twins"""
    assert pr.N_SCAN % 16 == 3

    def check(pl):
        assert not pl["dense"] and pl["nqt"] == 1 and pl["cap"] == 64 and pl["kp"] == (16 if k == 10 else 32) and pl["pages"] == 1
        assert pl["slabs"] > 64 and pl["merge_two_level"] == 1 and pl["tiles_per_block"] == 4

    run(mods, Case(pr.N_SCAN, pr.D, k, LAYOUT), dtype, 16, plan_check=check, kernels=scan_names(dtype), ghosts=TWIN,
        what=f"ghosts scan16 {dtype}")


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_scan_deep_slabs(mods, dtype):
    def check(pl):
        assert not pl["dense"] and pl["nqt"] == 1 and pl["slabs"] == 2 and pl["merge_two_level"] == 0
        assert pl["tiles_per_block"] >= 4 * 32 and pl["tiles_per_block"] * 16 < pr.N_SCAN

    run(mods, SCAN_CASE, dtype, 16, options={"scan_max_slabs": 2}, plan_check=check, kernels=scan_names(dtype), ghosts=TWIN,
        what=f"ghosts deep slabs {dtype}")


def test_scan_group_of_16(mods):
    def check(pl):
        assert not pl["dense"] and pl["nqt"] == 1 and pl["cap"] == 64

    run(mods, SCAN_CASE, "f16", 16, options={"scan_group": 16}, plan_check=check, kernels=scan_names("f16"), ghosts=TWIN,
        what="ghosts group 16")


@pytest.mark.parametrize("Q,nqt", [(32, 2), (64, 4)])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_scan_2_and_4_query_tiles(mods, dtype, Q, nqt):
    """f32 and fp8 rows: 2 / 4 query tiles per block; f16 rows at these call sizes are the 128-query score GEMM"""
    run(mods, SCAN_CASE, dtype, Q, plan_check=lambda pl: _scan_or_gemm128(dtype, Q, pl, nqt), ghosts=TWIN,
        extra_calls=[(100, 33)] if nqt == 4 else [], kernels=dense_names("f16") if dtype == "f16" else scan_names(dtype),
        what=f"ghosts scan nqt={nqt} {dtype}")


@pytest.mark.parametrize("Q", [3, 16])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_paged_scan(mods, dtype, Q):
    def check(pl):
        assert not pl["dense"] and pl["pages"] == 4 and pl["kp"] == 32 and pl["nqt"] == 1 and pl["cap"] == 64

    run(mods, Case(pr.N_SCAN, pr.D, 100, LAYOUT), dtype, Q, plan_check=check, kernels=scan_names(dtype), ghosts=TWIN,
        what=f"ghosts paged {dtype}")


@pytest.mark.parametrize("exclude_only", [False, True], ids=["require+exclude", "exclude-only"])
@pytest.mark.parametrize("Q,nqt", [(16, 1), (64, 4)])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_filtered_scan(mods, dtype, Q, nqt, exclude_only):
    """The FILT form. Every ghost's tag is 0 after the clear: with a require mask the predicate refuses it as well, a query that
    only excludes admits tag 0, so there `row < N` alone stands between the twins and the lists."""

    def check(pl):
        assert not pl["dense"] and pl["nqt"] == nqt and pl["cap"] == (64 if nqt == 1 else 32) and pl["kp"] == 16
        assert pl["slabs"] > 64 and pl["tiles_per_block"] == 4

    for case in FILT_CASES:
        run(mods, case, dtype, Q, plan_check=check, kernels=scan_names(dtype), ghosts=TWIN, exclude_only=exclude_only,
            what=f"ghosts filtered {dtype} mirrored={case.mirrored} exclude_only={exclude_only}")


# ================================================================================================ first pass: score GEMM
@pytest.mark.parametrize("Q", [40, 128])
def test_score_gemm_128_query_tile(mods, Q):
    """f16 rows: the last 128-row tile holds 3 live rows and 125 twins, which share GROUPMAX groups with them"""

    def check(pl):
        assert pl["dense"] and not pl["big"] and not pl["dense8"] and not pl["sample"] and pl["kp"] == 16
        assert pl["Mq"] == 128 and pl["Npad"] % 128 == 0 and pl["Npad"] - pr.N_SCAN == 125

    run(mods, SCAN_CASE, "f16", Q, plan_check=check, kernels=dense_names("f16"), ghosts=TWIN, what=f"ghosts score gemm Q={Q}")


CONCENTRATED = [
    pytest.param(SCAN_CASE, 40, {}, id="gemm128"),
    pytest.param(DENSE_CASE, 256, {}, id="strip-v3"),
    pytest.param(DENSE_CASE, 256, {"score_strip_v3": 0}, id="strip-v3-off"),
    pytest.param(Case(pr.N_DENSE, pr.D, 10, LAYOUT), 256, {}, id="strip-dim128"),
]


@pytest.mark.parametrize("case,Q,options", CONCENTRATED)
def test_score_gemm_twins_in_every_group_of_the_last_tile(mods, case, Q, options):
    """With one twin per query in the last tile an unmasked group maximum costs one of the k' = 16 group slots and displaces
    nobody. Here the ghosts are the twins of SEVEN queries only, in turn, so each of them has a twin in every group of the last
    tile (8 or 16 groups): with its winners' 10 groups that is more than 16, and a group maximum formed over dead rows pushes a
    winner's group out. The first Q queries are issued in one call (f16 rows)."""
    FlatIndex, ro, roc, _lib = mods
    p, N = case.corpus(), case.N
    few = p._replace(queries=p.queries[:7])
    tile = 256 if Q > 128 else 128
    dead = np.arange(N, -(-N // tile) * tile)
    for j in range(7):
        r = dead[pr.ghost_owner(few, pr.capacity_for(N))[dead] == j]
        assert np.unique(r // 64 * 4 + r % 16 // 4).size >= 7, j        # (groupmax_row: 4 rows of each 16-row quarter of 64)
    exp = tuple(a[:Q] for a in expected(case, "f16"))

    def check(pl):
        assert pl["dense"] and pl["kp"] == 16 and pl["big"] == (Q > 128) and pl["Npad"] == dead[-1] + 1

    idx = FlatIndex(case.D, "f16", capacity=N)
    try:
        with options_set(_lib, options):
            fill_with_ghosts(mods, idx, few, "f16", TWIN)
            idx.add(p.rows, labels_of(N))
            check_queries(mods, idx, p, case.k, Q, exp, which=np.arange(Q), plan_check=check,
                          kernels=dense_names("f16"), what=f"concentrated twins {case.N} Q={Q}")
    finally:
        idx.close()


STRIP_CASES = [
    pytest.param({"score_strip": 1}, 1, 1, id="v3-strip1"),
    pytest.param({"score_strip": 3}, 1, 3, id="v3-strip3"),
    pytest.param({}, 1, None, id="v3-default"),
    pytest.param({"score_strip_v3": 0}, 0, None, id="v3-off"),
    pytest.param({"score_strip_v3": 0, "score_strip": 3}, 0, 3, id="v3-off-strip3"),
    pytest.param({}, 0, None, id="dim128"),   # (below dim 256 the strip kernel of the 256 x 256 tile GEMM serves)
]


def _strip_check(N, v3, strip, dense8=False):
    def check(pl):
        assert pl["dense"] and pl["big"] and pl["dense8"] == dense8 and not pl["sample"] and pl["strip_v3"] == v3
        assert pl["Mq"] == 256 and pl["Npad"] > N and pl["Npad"] % 256 == 0 and pl["Npad"] - N < 256
        assert pl["strip"] == (strip if strip else pl["strip"]) and pl["strip"] >= 1 and pl["splits"] >= 2

    return check


@pytest.mark.parametrize("options,v3,strip", STRIP_CASES)
def test_strip_gemm_256(mods, request, options, v3, strip):
    """f16 rows, 256 x 256 tiles: 213 twins behind N in the last row tile, on the staggered loop and the strip kernel"""
    case = Case(pr.N_DENSE, pr.D, 10, LAYOUT) if request.node.callspec.id == "dim128" else DENSE_CASE
    run(mods, case, "f16", 256, options=options, plan_check=_strip_check(pr.N_DENSE, v3, strip), kernels=dense_names("f16"),
        ghosts=TWIN, what=f"ghosts strip gemm {options} D={case.D}")


@pytest.mark.parametrize("strip", [0, 3])
def test_strip_gemm_fp8_rows(mods, strip):
    run(mods, DENSE_CASE, "f8", 256, options={"score_strip": strip}, plan_check=_strip_check(pr.N_DENSE, 1, strip, dense8=True),
        kernels=dense_names("f8"), ghosts=TWIN, what="ghosts strip gemm fp8")


@pytest.mark.parametrize("dtype,v3", [("f16", 1), ("f16", 0), ("f8", 1)])
def test_sample_form(mods, dtype, v3):
    """score_filter = 2: the twins lie behind the sample, in the last of the tiles whose groups the strip kernel appends"""
    N = pr.N_SAMPLE

    def check(pl):
        assert pl["dense"] and pl["big"] and pl["sample"] and pl["ns_tiles"] == 16 and pl["strip_v3"] == v3
        assert pl["dense8"] == (dtype == "f8") and pl["Npad"] > N and pl["Npad"] // 256 >= 128

    run(mods, Case(N, pr.D_STRIP, 10, LAYOUT), dtype, 256, options={"score_filter": 2, "score_strip_v3": v3}, plan_check=check,
        kernels=dense_names(dtype, sample=True) + ("score_gemm_" + dtype,), ghosts=TWIN, what=f"ghosts sample form {dtype}")


# ================================================================================================ widen pass
@pytest.mark.parametrize("Q,nqt", [(16, 1), (32, 2), (64, 4)])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_widen_threshold_scan(mods, dtype, Q, nqt):
    """guard_force: every answer comes from the threshold scan's list, which every twin's score would enter"""

    def check(pl):
        assert pl["sweep_gemm"] == 0 and pl["sweep_nqt"] == nqt and pl["sweep_slabs"] > 1 and pl["sweep_tiles_per_block"] >= 4

    run(mods, SCAN_CASE, dtype, Q, widen=True, plan_check=check, kernels=("sweep_scan_" + dtype, "rerank"), ghosts=TWIN,
        extra_calls=[(100, 33)] if nqt == 4 else [], what=f"ghosts widen scan {dtype}")


@pytest.mark.parametrize("exclude_only", [False, True], ids=["require+exclude", "exclude-only"])
@pytest.mark.parametrize("Q,nqt", [(16, 1), (32, 2), (64, 4)])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_widen_threshold_scan_filtered(mods, dtype, Q, nqt, exclude_only):
    def check(pl):
        assert not pl["dense"] and pl["sweep_gemm"] == 0 and pl["sweep_nqt"] == nqt

    for case in FILT_CASES:
        run(mods, case, dtype, Q, widen=True, plan_check=check, kernels=("sweep_scan_" + dtype, "rerank"), ghosts=TWIN,
            exclude_only=exclude_only, what=f"ghosts widen filtered {dtype} mirrored={case.mirrored} exclude_only={exclude_only}")


@pytest.mark.parametrize("strip", [0, 3])
@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_widen_threshold_gemm(mods, dtype, strip):
    """guard_force, Q = 256: the threshold pass is the strip GEMM appending rows; with one strip it takes every tile as whole"""

    def check(pl):
        assert pl["sweep_gemm"] == 1 and pl["sweep_strip"] >= 1 and (strip == 0 or pl["sweep_strip"] == strip)
        assert pl["dense"] and pl["big"]

    run(mods, DENSE_CASE, dtype, 256, widen=True, options={"score_strip": strip}, plan_check=check,
        kernels=("sweep_gemm_" + dtype, "rerank"), ghosts=TWIN, what=f"ghosts widen gemm {dtype}")


# ================================================================================================ fewer live rows than k
@functools.lru_cache(maxsize=None)
def _tiny_expected(n_live, dtype, k):
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    p = pr.tiny_live(n_live, pr.D, pr.SEED)
    out = roc.query(p.queries, ro.normalize_rows(p.rows, dtype), labels_of(n_live), k)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("k", [10, 24])
@pytest.mark.parametrize("n_live", pr.TINY_LIVE)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_tiny_live_index(mods, dtype, n_live, k):
    """1, 3 and 19 random live rows under 1024 twins, 200 random queries in calls of 1, 16, 40 and 200: k >= n_live returns every
    live row, those of negative cosine too, which a dead fp8 row's score of 0 would outrank. Whatever the guard does on so small
    an index, it does the same on a fresh one: the ghosts cause no widen pass."""
    FlatIndex, ro, roc, _lib = mods
    p = pr.tiny_live(n_live, pr.D, pr.SEED)
    exp = _tiny_expected(n_live, dtype, k)
    assert (exp[2] == min(k, n_live)).all()
    for Q in (1, 16, 40, 200):
        deltas, dense = [], dtype == "f16" and Q > 16      # (the score GEMM: one tile of 128 or 256 rows, all but n_live of them dead)

        def check(pl):
            assert pl["dense"] == dense and pl["kp"] == (16 if min(k, n_live) <= 10 else 32) and pl["pages"] == 1
            assert (pl["big"] == (Q > 128) and pl["Npad"] == (256 if Q > 128 else 128)) if dense else pl["nqt"] >= 1

        for ghosts in (None, TWIN):
            idx = FlatIndex(pr.D, dtype, capacity=n_live)
            try:
                if ghosts:
                    fill_with_ghosts(mods, idx, p, dtype, ghosts)
                idx.add(p.rows, labels_of(n_live))
                *_, delta, ran = check_queries(mods, idx, p, k, Q, exp, mode=None, plan_check=check,
                                               kernels=(("score_gemm_" if dense else "scan_topk_") + dtype, "rerank"),
                                               what=f"tiny {n_live} {dtype} Q={Q} {ghosts}")
            finally:
                idx.close()
            deltas.append((delta, ran))
        assert deltas[0] == deltas[1], deltas


# ================================================================================================ exhaustive pass
PLATEAU_LABEL0 = 3 << 20     # the plateau's live labels start here (3 r + 5 above it); its ghosts' labels 3 r all lie below


def _plateau_labels():
    return labels_of(pr.N_PLATEAU) + PLATEAU_LABEL0


@functools.lru_cache(maxsize=None)
def _plateau_expected(dtype, k):
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    p = pr.plateau(pr.N_PLATEAU, pr.D, pr.SEED)
    out = roc.query(p.queries, ro.normalize_rows(p.rows, dtype), _plateau_labels(), k)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_exhaustive_pass(mods, dtype, k):
    """9000 byte-identical rows among 9003, more than a widened query may collect, under 16384 copies of the same row: the
    canonical pass decides by label. A dead copy ties with the live ones on distance, so here the ghosts carry the SMALLER
    labels (3 r, below every live label and disjoint from them): one that got through `row < N` would lead the answer."""
    FlatIndex, ro, roc, _lib = mods
    N = pr.N_PLATEAU
    p = pr.plateau(N, pr.D, pr.SEED)
    G = pr.capacity_for(N)
    labels, dead_labels = _plateau_labels(), 3 * np.arange(G, dtype=np.int64)
    assert dead_labels.max() < labels.min()
    exp = _plateau_expected(dtype, k)
    np.testing.assert_array_equal(exp[0][0], labels[p.rows_of(0)][:k])   # its own direction: the k smallest plateau labels
    idx = FlatIndex(pr.D, dtype, capacity=N)
    try:
        fill_with_ghosts(mods, idx, p, dtype, ("plateau", "clear"), labels=dead_labels)
        idx.add(p.rows, labels)

        def check(pl):
            assert not pl["dense"] and pl["nqt"] == 1 and pl["pages"] == (1 if k == 10 else 4)

        gl, *_ = check_queries(mods, idx, p, k, 4, exp, mode="exhaustive", plan_check=check, kernels=("canonical_scan",),
                               what=f"plateau {dtype} k={k}", row_of_label=lambda lab: (lab - PLATEAU_LABEL0 - 5) // 3)
        assert (gl >= PLATEAU_LABEL0).all()      # no dead row in any answer
    finally:
        idx.close()


# ================================================================================================ other ghosts, other ways to empty
@pytest.mark.parametrize("path,dtype", [("scan", "f16"), ("scan", "f8"), ("gemm128", "f16"), ("strip", "f16"), ("strip", "f8")])
def test_nonfinite_ghosts(mods, path, dtype):
    """of every three dead rows one is NaN, +inf or zero input, as the normalisation stored it (fp8 rows reach the score GEMM
    from 129 queries on: their GEMM case is the strip one)"""
    if path == "scan":
        run(mods, SCAN_CASE, dtype, 16, plan_check=_scan16_check, kernels=scan_names(dtype), ghosts=("nonfinite", "clear"),
            what=f"nonfinite scan {dtype}")
    elif path == "gemm128":
        run(mods, SCAN_CASE, dtype, 128, plan_check=lambda pl: _scan_or_gemm128(dtype, 128, pl, 0), kernels=dense_names(dtype),
            ghosts=("nonfinite", "clear"), what="nonfinite score gemm")
    else:
        run(mods, DENSE_CASE, dtype, 256, plan_check=_strip_check(pr.N_DENSE, 1, None, dense8=dtype == "f8"),
            kernels=dense_names(dtype), ghosts=("nonfinite", "clear"), what=f"nonfinite strip gemm {dtype}")


@pytest.mark.parametrize("via", ["remove_all", "load"])
@pytest.mark.parametrize("dtype", ["f16", "f8"])
@pytest.mark.parametrize("path", ["scan", "strip"])
def test_emptied_by_remove_and_by_load(mods, path, dtype, via, tmp_path):
    """the twins left by a remove of every row, and by a load of the live corpus's file over the full ghost index"""
    if path == "scan":
        run(mods, SCAN_CASE, dtype, 16, plan_check=_scan16_check, kernels=scan_names(dtype), ghosts=("twin", via), tmp_path=tmp_path,
            what=f"{via} scan {dtype}")
    else:
        run(mods, DENSE_CASE, dtype, 256, plan_check=_strip_check(pr.N_DENSE, 1, None, dense8=dtype == "f8"),
            kernels=dense_names(dtype), ghosts=("twin", via), tmp_path=tmp_path, what=f"{via} strip gemm {dtype}")


def test_filtered_after_load_sets_tags_again(mods, tmp_path):
    """a load resets every tag: the filtered corpus sets them after it, and the exclude-only queries still meet tag-0 twins"""
    for exclude_only in (False, True):
        run(mods, FILT_CASES[0], "f16", 16, plan_check=_scan16_check, kernels=scan_names("f16"), ghosts=("twin", "load"),
            exclude_only=exclude_only, tmp_path=tmp_path, what=f"load filtered exclude_only={exclude_only}")


def test_pipelined_chain(mods):
    """one query_begin / query_next chain over the whole corpus, 64 queries a step (f16 rows: the 128-query score GEMM)"""
    run(mods, SCAN_CASE, "f16", 64, plan_check=lambda pl: _scan_or_gemm128("f16", 64, pl, 0), kernels=dense_names("f16"),
        ghosts=TWIN, pipelined=True, what="ghosts pipelined")


# ================================================================================================ compaction, growth, update
def _oracle(case, dtype, labels, which, stored=None):
    """expected answers of the queries `which` over the rows whose label is >= 0 (the others are not in the index)"""
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    p = case.corpus()
    stored = ro.normalize_rows(p.rows, dtype) if stored is None else stored
    if case.N <= pr.FULL_ORACLE_MAX_N and not case.filtered:
        live = np.nonzero(labels >= 0)[0]
        return roc.query(p.queries[which], stored[live], labels[live], case.k)
    # a large or filtered corpus: over each query's own (admitted) rows, all of which must be in the index
    assert case.filtered or (which < p.n_full).all() or (labels >= 0).all()   # (the short last query: the whole index)
    for j in which:
        assert (labels[pr.admitted(p, j) if case.filtered else p.rows_of(j)] >= 0).all()
    return pr.expected(roc, p, stored, labels, case.k, full=False, which=which)


COMPACTION = [
    pytest.param(SCAN_CASE, "f32", 16, id="scan-f32"),
    pytest.param(SCAN_CASE, "f16", 16, id="scan-f16"),
    pytest.param(SCAN_CASE, "f8", 16, id="scan-f8"),
    pytest.param(FILT_CASES[0], "f16", 16, id="filtered-scan-f16"),
    pytest.param(FILT_CASES[1], "f8", 16, id="filtered-mirrored-scan-f8"),
    pytest.param(SCAN_CASE, "f16", 128, id="gemm128-f16"),
    pytest.param(DENSE_CASE, "f16", 256, id="strip-f16"),
    pytest.param(DENSE_CASE, "f8", 256, id="strip-f8"),
]


@pytest.mark.parametrize("case,dtype,Q", COMPACTION)
def test_compaction_keeps_every_winner(mods, case, dtype, Q):
    """Remove every row of the queries j % 3 == 0 (scattered: holes through every tile, group and slab), issue the others; add
    the removed rows back under new, larger labels and issue all. No query widens; labels and tags follow the rows."""
    FlatIndex, ro, roc, _lib = mods
    p, N, k = case.corpus(), case.N, case.k
    labels = labels_of(N)
    drop = p.owner % 3 == 0
    if case.filtered:       # (a filtered query admits the rows that carry its bit: those of the queries j + 62 i, removed or kept with it)
        drop = (p.owner % pr.MASK_BITS) % 3 == 0
        others = np.nonzero(np.arange(p.n_queries) % pr.MASK_BITS % 3 != 0)[0]
    else:
        others = np.nonzero(np.arange(p.n_queries) % 3 != 0)[0]
    kept = labels[~drop]
    names = dense_names(dtype) if (dtype == "f16" and Q > 16) or Q > 128 else scan_names(dtype)
    idx = FlatIndex(case.D, dtype, capacity=N)
    try:
        idx.add(p.rows, labels)
        if case.filtered:
            idx.set_tags(labels, p.tags)
        assert idx.remove(labels[drop]) == int(drop.sum())
        np.testing.assert_array_equal(idx.labels(), kept)
        if case.filtered:
            np.testing.assert_array_equal(idx.get_tags(kept), p.tags[~drop])
        holes = np.where(drop, -1, labels)
        common = dict(filtered=case.filtered, kernels=names, decoy_labels=labels[p.decoy] if case.filtered else None)
        check_queries(mods, idx, p, k, Q, _oracle(case, dtype, holes, others), which=others, what=f"compacted {dtype}",
                      row_of_label=lambda lab: int(np.searchsorted(kept, lab)), **common)
        back = labels[-1] + 1 + np.arange(int(drop.sum()), dtype=np.int64)
        idx.add(p.rows[drop], back)
        again = labels.copy()
        again[drop] = back
        now = np.concatenate([kept, back])
        np.testing.assert_array_equal(idx.labels(), now)
        if case.filtered:
            np.testing.assert_array_equal(idx.get_tags(back), np.zeros(back.size, np.uint64))   # added rows: tag 0
            idx.set_tags(back, p.tags[drop])
            np.testing.assert_array_equal(idx.get_tags(now), np.concatenate([p.tags[~drop], p.tags[drop]]))
            common["decoy_labels"] = again[p.decoy]
        check_queries(mods, idx, p, k, Q, _oracle(case, dtype, again, np.arange(p.n_queries)), what=f"refilled {dtype}",
                      row_of_label=lambda lab: int(np.searchsorted(now, lab)), **common)
    finally:
        idx.close()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_growth_keeps_every_row(mods, dtype):
    """no capacity hint, the corpus in pieces of 1000: the capacity doubles from 1024 to 8192, three copies into fresh buffers.
    Every query after every piece (the guard may widen: most winners are not there yet), on the scan and, f16, the score GEMM."""
    FlatIndex, ro, roc, _lib = mods
    case = SCAN_CASE
    p, N = case.corpus(), case.N
    labels = labels_of(N)
    stored = ro.normalize_rows(p.rows, dtype)
    idx = FlatIndex(case.D, dtype)
    try:
        for n0 in range(0, N, 1000):
            n1 = min(n0 + 1000, N)
            idx.add(p.rows[n0:n1], labels[n0:n1])
            np.testing.assert_array_equal(idx.labels(), labels[:n1])
            exp = roc.query(p.queries, stored[:n1], labels[:n1], case.k)
            for Q in (16, 128) if dtype == "f16" else (16,):
                check_queries(mods, idx, p, case.k, Q, exp, mode="first" if n1 == N else None,
                              kernels=dense_names(dtype) if Q > 16 else scan_names(dtype), what=f"grown to {n1} {dtype} Q={Q}")
    finally:
        idx.close()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_update_exchanges_winners(mods, dtype):
    """update() exchanges the vectors of 50 pairs of winners of different queries, spread over the index: every row is still
    some query's winner, at another position (fp8 rows: the inverse norms follow the codes)"""
    FlatIndex, ro, roc, _lib = mods
    case = SCAN_CASE
    p, N = case.corpus(), case.N
    labels = labels_of(N)
    step = N // 100
    a, b = np.arange(50) * 2 * step, (np.arange(50) * 2 + 1) * step + 7
    b += p.owner[a] == p.owner[b]          # (a pair of one query's winners: its neighbour instead)
    assert b.max() < N and (p.owner[a] != p.owner[b]).all() and np.unique(np.concatenate([a, b])).size == 100
    rows = p.rows.copy()
    rows[a], rows[b] = p.rows[b], p.rows[a]
    exp = roc.query(p.queries, ro.normalize_rows(rows, dtype), labels, case.k)
    idx = FlatIndex(case.D, dtype, capacity=N)
    try:
        idx.add(p.rows, labels)
        idx.update(labels[np.concatenate([a, b])], p.rows[np.concatenate([b, a])])
        for Q in (16, 128) if dtype == "f16" else (16,):
            check_queries(mods, idx, p, case.k, Q, exp, kernels=dense_names(dtype) if Q > 16 else scan_names(dtype),
                          what=f"updated {dtype} Q={Q}")
    finally:
        idx.close()

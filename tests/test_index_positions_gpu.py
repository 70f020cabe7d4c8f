"""Stage 1 of the index query, position by position: on the corpora of tests/planted_rows.py EVERY row of the index is a true
top-k row of exactly one query, and every query is issued, so a kernel that loses the row at one structural position — the last
tile of a slab, row 15 of the ragged last tile, the first tile behind a tag batch, the group just behind a select_topk split,
the first tile behind the sample — loses somebody's winner and fails the bit-exact comparison. The exactness guard cannot hide
it: the first-pass tests require that NO query was widened (and that no widen-pass kernel ran), the widen-pass tests force
every query through the threshold pass and require that none ended in the exhaustive pass.

Every test reads the path it means to reach from the product (mmiss_dbg_index_plan) and asserts it before it runs: the kernel
form, its tile / slab / split / strip arithmetic and the boundaries printed for a missing winner come from the planning
functions the query path itself calls, not from formulas restated here.

Expected answers: the oracle over the whole index at N = 4099 and for every filtered query (over its admitted rows), the oracle
restricted to a query's own planted rows at N >= 20011 (equal to the full one: test_planted_rows_cpu.py). Ids, distance bits
and counts of every query are compared; no case is left out."""
import numpy as np
import pytest

import planted_rows as pr
from index_query_cases import ALL_DTYPES, Case, load_mods
from index_query_cases import dense_names as _dense_names, run as _run, scan_names as _scan_names

pytestmark = pytest.mark.gpu

LAYOUT_IDS = list(pr.LAYOUTS)


@pytest.fixture(scope="module")
def mods():
    return load_mods()


# ================================================================================================ first pass: streaming scan
@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("k", [10, 24])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_scan_16_query_tile(mods, dtype, k, layout):
    """Q = 16 per call: the 16-query tile with 64-entry lists; 257 tiles in slabs of 4 (one tile per wave), more than 64 slabs so the
    merge runs in two levels of 32 lists; the last tile holds 3 rows."""
    N = pr.N_SCAN
    assert N % 16 == 3

    def check(pl):
        assert not pl["dense"] and pl["nqt"] == 1 and pl["cap"] == 64 and pl["kp"] == (16 if k == 10 else 32) and pl["pages"] == 1
        assert pl["slabs"] > 64 and pl["merge_two_level"] == 1 and pl["tiles_per_block"] == 4

    _run(mods, Case(N, pr.D, k, layout), dtype, 16, plan_check=check, kernels=_scan_names(dtype), what=f"scan16 {dtype}")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_scan_deep_slabs(mods, dtype, layout):
    """scan_max_slabs = 2: two slabs of 132 tiles, 33 tiles per wave — the lists fill and are compacted inside the loop, and the
    slab boundary lies in the middle of the index; one-level merge."""

    def check(pl):
        assert not pl["dense"] and pl["nqt"] == 1 and pl["slabs"] == 2 and pl["merge_two_level"] == 0
        assert pl["tiles_per_block"] >= 4 * 32 and pl["tiles_per_block"] * 16 < pr.N_SCAN

    _run(mods, Case(pr.N_SCAN, pr.D, 10, layout), dtype, 16, options={"scan_max_slabs": 2}, plan_check=check,
         kernels=_scan_names(dtype), what=f"deep slabs {dtype}")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("slabs", [1024, 2])
def test_scan_group_of_16(mods, slabs, layout):
    """scan_group = 16 (f16 lists of a 16-query tile, rows in groups of 16): the oracle's answer, hence the bits of the group-of-8 run"""
    case = Case(pr.N_SCAN, pr.D, 10, layout)

    def check(pl):
        assert not pl["dense"] and pl["nqt"] == 1 and pl["cap"] == 64

    g8 = _run(mods, case, "f16", 16, options={"scan_max_slabs": slabs}, plan_check=check, kernels=_scan_names("f16"), what="group 8")
    g16 = _run(mods, case, "f16", 16, options={"scan_max_slabs": slabs, "scan_group": 16}, plan_check=check,
               kernels=_scan_names("f16"), what="group 16")
    np.testing.assert_array_equal(g16[0], g8[0])
    np.testing.assert_array_equal(g16[1].view(np.uint32), g8[1].view(np.uint32))
    np.testing.assert_array_equal(g16[2], g8[2])


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("Q,nqt", [(32, 2), (64, 4)])
@pytest.mark.parametrize("dtype", ["f32", "f8"])
def test_scan_2_and_4_query_tiles(mods, dtype, Q, nqt, layout):
    """Q = 32 / 64 per call (f32 and fp8 rows; f16 rows go to the score GEMM): 2 / 4 query tiles per block, 32-entry lists. One more
    call of 33 queries: four query tiles of which the last three hold one query and 31 padding queries."""
    FlatIndex, ro, roc, _lib = mods

    def check(pl):
        assert not pl["dense"] and pl["nqt"] == nqt and pl["cap"] == 32 and pl["kp"] == 16 and pl["qtiles"] == 1
        assert pl["slabs"] > 64 and pl["merge_two_level"] == 1 and pl["tiles_per_block"] == 4

    _run(mods, Case(pr.N_SCAN, pr.D, 10, layout), dtype, Q, plan_check=check, kernels=_scan_names(dtype),
         extra_calls=[(100, 33)] if nqt == 4 else [], what=f"scan nqt={nqt} {dtype}")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("Q", [3, 16])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_paged_scan(mods, dtype, Q, layout):
    """k = 100, 100 winners planted per query: four pages of 32 candidates; every page cursor lies between two planted rows"""

    def check(pl):
        assert not pl["dense"] and pl["pages"] == 4 and pl["kp"] == 32 and pl["nqt"] == 1 and pl["cap"] == 64

    _run(mods, Case(pr.N_SCAN, pr.D, 100, layout), dtype, Q, plan_check=check, kernels=_scan_names(dtype),
         what=f"paged {dtype}")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("slabs", [1024, 2])
@pytest.mark.parametrize("Q,nqt", [(16, 1), (32, 2), (64, 4)])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_filtered_scan(mods, dtype, Q, nqt, slabs, layout):
    """The FILT form on the decoy corpora, both of them: at every position an admitted winner once and an excluded, better-scoring
    decoy once; a different mask per query of a call. Default slabs (one tile per wave) and two deep slabs (the tag words are
    fetched four tiles at a time, one batch ahead: 33 tiles per wave cross eight batch swaps)."""

    def check(pl):
        assert not pl["dense"] and pl["nqt"] == nqt and pl["cap"] == (64 if nqt == 1 else 32) and pl["kp"] == 16
        if slabs == 2:
            assert pl["slabs"] == 2 and pl["tiles_per_block"] >= 4 * 32
        else:
            assert pl["slabs"] > 64 and pl["tiles_per_block"] == 4

    for mirrored in (False, True):
        _run(mods, Case(pr.N_SCAN, pr.D, 10, layout, True, mirrored), dtype, Q, options={"scan_max_slabs": slabs}, plan_check=check,
             kernels=_scan_names(dtype), what=f"filtered {dtype} mirrored={mirrored}")


# ================================================================================================ first pass: score GEMM
@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("Q", [40, 128])
def test_score_gemm_128_query_tile(mods, Q, layout):
    """f16 rows, Q = 40 and 128 per call: the 128-row tile GEMM to group maxima, select_topk in two splits (1256 groups: the
    second split starts at group 1024), pad rows behind N in the last tile"""
    N = pr.N_DENSE

    def check(pl):
        assert pl["dense"] and not pl["big"] and not pl["dense8"] and not pl["sample"] and pl["kp"] == 16
        assert pl["Mq"] == 128 and pl["Npad"] > N and pl["Npad"] % 128 == 0 and pl["Npad"] - N < 128
        assert pl["splits"] >= 2 and pl["groups_per_split"] * (pl["splits"] - 1) < N // 16

    _run(mods, Case(N, pr.D, 10, layout), "f16", Q, plan_check=check, kernels=_dense_names("f16"), what=f"score gemm Q={Q}")


STRIP_CASES = [
    pytest.param(pr.D_STRIP, {"score_strip": 1}, 1, 1, id="v3-strip1"),
    pytest.param(pr.D_STRIP, {"score_strip": 3}, 1, 3, id="v3-strip3"),
    pytest.param(pr.D_STRIP, {}, 1, None, id="v3-default"),
    pytest.param(pr.D_STRIP, {"score_strip_v3": 0}, 0, None, id="v3-off"),
    pytest.param(pr.D_STRIP, {"score_strip_v3": 0, "score_strip": 3}, 0, 3, id="v3-off-strip3"),
    pytest.param(pr.D, {}, 0, None, id="dim128"),   # (below dim 256 the strip kernel of the 256 x 256 tile GEMM serves)
]


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("D,options,v3,strip", STRIP_CASES)
def test_strip_gemm_256(mods, D, options, v3, strip, layout):
    """f16 rows, Q = 256 per call: 256 x 256 tiles walked in strips of 1, 3 and the default length, on the staggered loop and on
    the strip kernel it replaced; 79 row tiles, so strips of 3 end in a strip of one; pad rows behind N in the last tile"""
    N = pr.N_DENSE

    def check(pl):
        assert pl["dense"] and pl["big"] and not pl["dense8"] and not pl["sample"] and pl["strip_v3"] == v3
        assert pl["Mq"] == 256 and pl["Npad"] > N and pl["Npad"] % 256 == 0 and pl["Npad"] - N < 256
        assert pl["strip"] == (strip if strip else pl["strip"]) and pl["strip"] >= 1
        if strip and strip > 1:
            assert (pl["Npad"] // 256) % strip != 0          # the last strip is a short one
        assert pl["splits"] >= 2

    _run(mods, Case(N, D, 10, layout), "f16", 256, options=options, plan_check=check, kernels=_dense_names("f16"),
         what=f"strip gemm {options}")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("strip", [0, 3])
def test_strip_gemm_fp8_rows(mods, strip, layout):
    """fp8 rows, Q = 256 per call: the strip GEMM that widens the codes in its operand load, scores x inverse norms"""
    N = pr.N_DENSE

    def check(pl):
        assert pl["dense"] and pl["dense8"] and pl["big"] and pl["strip_v3"] and not pl["sample"]
        assert pl["Npad"] > N and pl["splits"] >= 2 and (strip == 0 or pl["strip"] == strip)

    _run(mods, Case(N, pr.D_STRIP, 10, layout), "f8", 256, options={"score_strip": strip}, plan_check=check,
         kernels=_dense_names("f8"), what="strip gemm fp8")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("dtype,v3", [("f16", 1), ("f16", 0), ("f8", 1)])   # (fp8 rows reach the score GEMM on the staggered loop only)
def test_sample_form(mods, dtype, v3, layout):
    """score_filter = 2, Q = 256 per call, N = 35003: the first 16 row tiles (4096 rows) go through group maxima, select and merge;
    the strip kernel appends the groups of the other 121 tiles that reach the sample's k'-th score. Every row is some query's
    winner, so are the last rows before row 4096 and the first behind it, the first tile the appending kernel visits."""
    N = pr.N_SAMPLE

    def check(pl):
        assert pl["dense"] and pl["big"] and pl["sample"] and pl["ns_tiles"] == 16 and pl["strip_v3"] == v3
        assert pl["dense8"] == (dtype == "f8") and pl["Npad"] > N and pl["Npad"] // 256 >= 128
        assert pl["merge_two_level"] == 0

    _run(mods, Case(N, pr.D_STRIP, 10, layout), dtype, 256, options={"score_filter": 2, "score_strip_v3": v3}, plan_check=check,
         kernels=_dense_names(dtype, sample=True) + ("score_gemm_" + dtype,), what=f"sample form {dtype}")


# ================================================================================================ widen pass
@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("Q,nqt", [(16, 1), (32, 2), (64, 4)])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_widen_threshold_scan(mods, dtype, Q, nqt, layout):
    """guard_force: every query's answer comes from the threshold scan's list alone (1, 2 and 4 query tiles)"""

    def check(pl):
        assert pl["sweep_gemm"] == 0 and pl["sweep_nqt"] == nqt and pl["sweep_slabs"] > 1 and pl["sweep_tiles_per_block"] >= 4

    _run(mods, Case(pr.N_SCAN, pr.D, 10, layout), dtype, Q, widen=True, plan_check=check,
         kernels=("sweep_scan_" + dtype, "rerank"), extra_calls=[(100, 33)] if nqt == 4 else [], what=f"widen scan {dtype}")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("Q,nqt", [(16, 1), (32, 2), (64, 4)])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_widen_threshold_scan_filtered(mods, dtype, Q, nqt, layout):
    """... in its FILT form on the decoy corpora: every decoy reaches its query's threshold and must not be collected"""

    def check(pl):
        assert not pl["dense"] and pl["sweep_gemm"] == 0 and pl["sweep_nqt"] == nqt

    for mirrored in (False, True):
        _run(mods, Case(pr.N_SCAN, pr.D, 10, layout, True, mirrored), dtype, Q, widen=True, plan_check=check,
             kernels=("sweep_scan_" + dtype, "rerank"), what=f"widen filtered {dtype} mirrored={mirrored}")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_widen_threshold_scan_filtered_deep_slabs(mods, dtype, layout):
    """The threshold scan's slabs grow only with the number of query tiles: 1024 filtered queries per call (16 query tiles) at
    N = 35003 give every wave five tiles or more, so its FILT form crosses a swap of the tag batch, which the sizes above do
    not reach (one tile per wave). The first pass of these calls is the FILT list scan at 16 query tiles, 35 tiles per wave."""

    def check(pl):
        assert not pl["dense"] and pl["nqt"] == 4 and pl["qtiles"] == 16 and pl["tiles_per_block"] >= 4 * 32
        assert pl["sweep_gemm"] == 0 and pl["sweep_nqt"] == 4 and pl["sweep_tiles_per_block"] > 4 * 4 and pl["sweep_slabs"] > 1

    for mirrored in (False, True):
        _run(mods, Case(pr.N_SAMPLE, pr.D, 10, layout, True, mirrored), dtype, 1024, widen=True, plan_check=check,
             kernels=("sweep_scan_" + dtype, "rerank"), what=f"widen filtered deep {dtype} mirrored={mirrored}")


@pytest.mark.parametrize("layout", LAYOUT_IDS)
@pytest.mark.parametrize("strip", [0, 3])
@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_widen_threshold_gemm(mods, dtype, strip, layout):
    """guard_force, Q = 256 per call, N = 35003: the threshold pass is the strip score GEMM appending rows (f16 and fp8 rows)"""

    def check(pl):
        assert pl["sweep_gemm"] == 1 and pl["sweep_strip"] >= 1 and (strip == 0 or pl["sweep_strip"] == strip)
        assert pl["dense"] and pl["big"]

    _run(mods, Case(pr.N_SAMPLE, pr.D_STRIP, 10, layout), dtype, 256, widen=True, options={"score_strip": strip},
         plan_check=check, kernels=("sweep_gemm_" + dtype, "rerank"), what=f"widen gemm {dtype}")

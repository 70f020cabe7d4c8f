"""Holds tests/partition_cases.py to what it claims, on the CPU: the restatement with every cell probed is ro.query, and the planted
cases really have their property — the tie is a tie in float bits, the hidden row is the exact nearest, and at nprobe = 1 some
query's expected result differs from the flat one (a test that cannot tell probed from flat shows nothing)."""
import numpy as np
import pytest

import partition_cases as pc
from oracle import retrieval_oracle as ro

D = 128


@pytest.mark.parametrize("dtype", ["f32", "f16", "f8"])
def test_every_cell_probed_is_the_flat_query(dtype):
    p = pc.clustered(5, 900, D, 7, 6, complete=True)
    st, lab = pc.stored_of(p["x"], dtype), pc.labels_of(900)
    req, exc = pc.query_masks(6)
    for masks in (dict(), dict(tags=p["tags"], require=req, exclude=exc)):
        got = pc.expected_probed(p["queries"], 10, 7, p["centres"], p["cells"], 900, st, lab, **masks)
        assert pc.mismatch(got[:3], pc.expected_flat(p["queries"], 10, st, lab, **masks)) is None
        assert got[3].tolist() == [895, 895, 0, 895, 895, 895]          # every row with a direction; query 2 has none
    with np.errstate(all="ignore"):
        flat = ro.query(p["queries"], st, lab, 10)
    assert pc.mismatch(pc.expected_probed(p["queries"], 10, 12, p["centres"], p["cells"], 900, st, lab)[:3], flat) is None
    assert flat[2].tolist() == [10, 10, 0, 10, 10, 10]


def test_nprobe_one_differs_from_flat_and_unprobed_cells_hide_rows():
    p = pc.clustered(5, 900, D, 7, 6)
    st, lab = pc.stored_of(p["x"], "f16"), pc.labels_of(900)
    with np.errstate(all="ignore"):
        flat = ro.query(p["queries"], st, lab, 10)
    one = pc.expected_probed(p["queries"], 10, 1, p["centres"], p["cells"], 900, st, lab)
    assert any(not np.array_equal(one[0][q], flat[0][q]) for q in range(6))
    # all live cells probed still is not the flat result here: rows 30 .. 35 sit in the cell of the centre without a direction,
    # rows 40 / 41 in no cell
    every = pc.expected_probed(p["queries"], 2040, 7, p["centres"], p["cells"], 900, st, lab)
    hidden = set(lab[[30, 31, 32, 33, 34, 35, 40, 41]].tolist())
    assert not hidden & set(every[0][0].tolist()) and hidden <= set(ro.query(p["queries"][:1], st, lab, 2040)[0][0].tolist())
    assert every[3][0] == pc.cell_sizes(p["cells"], 7)[[0, 2, 3, 4, 5, 6]].sum() and pc.cell_sizes(p["cells"], 7)[1] == 6
    # the tail: rows behind B are candidates of every query
    tail = pc.expected_probed(p["queries"], 10, 1, p["centres"], p["cells"], 800, st, lab)
    assert (tail[3][[0, 1, 3]] >= 100).all() and tail[3][2] == 0


def test_the_hidden_row_is_the_exact_nearest_and_sits_behind_the_far_centre():
    p = pc.hidden_row(D)
    st, lab = pc.stored_of(p["x"], "f32"), pc.labels_of(p["x"].shape[0])
    flat = ro.query(p["queries"], st, lab, 5)
    assert flat[0][0, 0] == lab[p["hidden"]] and flat[1][0, 0] < flat[1][0, 1]
    dc = pc.centre_distances(p["queries"], p["centres"])[0]
    assert dc[0] < dc[1] and p["cells"][p["hidden"]] == 1
    one = pc.expected_probed(p["queries"], 5, 1, p["centres"], p["cells"], 80, st, lab)
    assert lab[p["hidden"]] not in one[0][0] and one[3][0] == 40
    assert pc.expected_probed(p["queries"], 5, 2, p["centres"], p["cells"], 80, st, lab)[0][0, 0] == lab[p["hidden"]]


@pytest.mark.parametrize("kind", ["dup", "mirror"])
def test_the_centre_tie_is_a_tie_in_float_bits(kind):
    p = pc.centre_ties(D, kind)
    dc = pc.centre_distances(p["queries"], p["centres"])[0]
    a, b = p["tied"]
    assert dc[a:a + 1].view(np.uint32)[0] == dc[b:b + 1].view(np.uint32)[0] and a < b
    assert all(dc[a] < dc[c] for c in range(dc.shape[0]) if c not in (a, b))
    assert pc.probed_cells(dc, 1).tolist() == [a] and pc.probed_cells(dc, 2).tolist() == [a, b]
    assert p["sizes"][a] != p["sizes"][b]                               # scanned tells which of the two was probed
    if kind == "mirror":
        assert not np.array_equal(p["centres"][0], p["centres"][1])     # two different vectors, one distance


def test_plan_edges_have_their_sizes_and_planted_rows():
    p = pc.plan_edges(D)
    assert pc.cell_sizes(p["cells"], len(pc.EDGE_SIZES)).tolist() == list(pc.EDGE_SIZES)
    assert p["B"] == sum(pc.EDGE_SIZES) and p["x"].shape[0] == p["B"] + pc.EDGE_TAIL
    assert {p["B"], p["B"] + pc.EDGE_TAIL - 1} <= set(p["planted"].tolist())
    for cell in range(1, len(pc.EDGE_SIZES)):
        r = np.nonzero(p["cells"] == cell)[0]
        assert {int(r[0]), int(r[-1])} <= set(p["planted"].tolist())

"""What test_index_positions_gpu.py and test_index_dead_rows_gpu.py share: a corpus of planted_rows as a Case, its expected answer
(computed once), the run of all its queries through one planned path of the index with the bit-exact comparison and the guard
accounting, and the message that names the structural position of a missing winner. Not a test module.

An index is prepared by run(): the live corpus under labels 3 r + 5 and, with ghosts=(kind, via), behind it the hostile rows
of planted_rows.ghosts: they are added first (they fill the capacity), the index is emptied by `via`, and the live corpus goes
into the same handle, so the rows [N, capacity) and their labels are still the ghosts'."""
import functools
from typing import NamedTuple

import numpy as np
import pytest

import planted_rows as pr

DEFAULTS = {"scan_max_slabs": 1024, "scan_group": 8, "score_strip": 0, "score_strip_v3": 1, "score_filter": 1, "guard_force": 0}
WIDEN_KERNELS = {"sweep_scan_f32", "sweep_scan_f16", "sweep_scan_f8", "sweep_gemm_f16", "sweep_gemm_f8", "canonical_scan"}
ALL_DTYPES = ["f32", "f16", "f8"]
VIAS = ("clear", "remove_all", "load")


def load_mods():
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib
    from mmiss_amd.index import FlatIndex
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    return FlatIndex, ro, roc, _lib


def labels_of(N):
    return np.arange(N, dtype=np.int64) * 3 + 5


class Case(NamedTuple):
    """one corpus of planted_rows (they are cached there: every test on a case shares the arrays)"""
    N: int
    D: int
    k: int
    layout: str
    filtered: bool = False
    mirrored: bool = False

    def corpus(self):
        if self.filtered:
            return pr.filtered_corpus(self.N, self.D, self.k, pr.SEED, pr.LAYOUTS[self.layout], self.mirrored)
        return pr.corpus(self.N, self.D, self.k, pr.SEED, pr.LAYOUTS[self.layout])


def _frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(case, dtype):
    """computed once per corpus and storage dtype, shared by every test on it, never modified"""
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    p = case.corpus()
    stored = ro.normalize_rows(p.rows, dtype)
    return _frozen(pr.expected(roc, p, stored, labels_of(case.N), case.k, full=case.N <= pr.FULL_ORACLE_MAX_N))


@functools.lru_cache(maxsize=None)
def expected_exclude_only(case, dtype):
    """a filtered corpus queried with require = None: the oracle over every row that is no decoy, for every query"""
    from oracle import retrieval_oracle as ro
    from oracle import retrieval_oracle_c as roc

    p = case.corpus()
    sub = pr.not_excluded(p)
    return _frozen(roc.query(p.queries, ro.normalize_rows(p.rows, dtype)[sub], labels_of(case.N)[sub], case.k))


def where(row, plan):
    """the structural position of a row, from the plan of the call that should have found it"""
    tile, s = row // 16, [f"row {row}", f"row%16 {row % 16}", f"tile%4 {row // 16 % 4}"]
    if plan["tiles_per_block"]:
        s.append(f"slab {tile // plan['tiles_per_block']} (tile {tile % plan['tiles_per_block']} of {plan['tiles_per_block']})")
    if plan["sweep_tiles_per_block"]:
        s.append(f"sweep slab {tile // plan['sweep_tiles_per_block']}")
    if plan["groups_per_split"]:
        # a group of the score GEMM's maxima is 4 rows of each 16-row quarter of a 64-row block (groupmax_row, csrc/gemm_bf16.h)
        group = row // 64 * 4 + row % 16 // 4
        s.append(f"group {group}, split {group // plan['groups_per_split']} (group {group % plan['groups_per_split']} of it)")
    if plan["dense"] and plan["big"]:
        t256, first = row // 256, plan["ns_tiles"] if plan["sample"] else 0     # (the appending launch starts behind the sample)
        if t256 >= first:
            s.append(f"256-row tile {t256}, strip {(t256 - first) // max(1, plan['strip'])} (tile {(t256 - first) % max(1, plan['strip'])} of it)")
        if plan["sample"]:
            s.append(f"{'behind' if t256 >= first else 'in'} the sample of {first} tiles")
    elif plan["dense"]:
        s.append(f"128-row tile {row // 128}")
    if plan["sweep_gemm"]:
        s.append(f"sweep strip {row // 256 // max(1, plan['sweep_strip'])}")
    return ", ".join(s)


def compare(got, exp, plan, what, row_of_label=lambda lab: (lab - 5) // 3):
    gl, gd, gc = got
    el, ed, ec = exp
    bad = np.nonzero((gl != el).any(1) | (gd.view(np.uint32) != ed.view(np.uint32)).any(1) | (gc != ec))[0]
    if bad.size == 0:
        return
    lines = [f"{what}: {bad.size} of {gl.shape[0]} queries differ from the oracle; the winners that are missing:"]
    for j in bad[:24]:
        missing = sorted(set(el[j][el[j] >= 0].tolist()) - set(gl[j].tolist()))
        for lab in missing:
            lines.append(f"  query {j}: {where(row_of_label(lab), plan)}")
        ghosts = gl[j][gl[j] >= pr.GHOST_LABEL0] - pr.GHOST_LABEL0
        if ghosts.size:
            lines.append(f"  query {j}: dead rows {ghosts.tolist()} among its results")
        if not missing:
            lines.append(f"  query {j}: same ids; counts {gc[j]} / {ec[j]}, order or distance bits differ")
    print("\n".join(lines))
    pytest.fail("\n".join(lines[:12]))


def fill_with_ghosts(mods, idx, p, dtype, ghosts, tmp_path=None, labels=None):
    """Steps 1 and 2 of a ghost run (step 3, the live rows, is the caller's add): fill the capacity with ghost rows (under
    planted_rows.ghost_labels, or `labels`), empty the index by `via`. Returns True when the live corpus is in the index
    already (via = load)."""
    FlatIndex, ro, roc, _lib = mods
    kind, via = ghosts
    assert via in VIAS
    N, D = p.rows.shape
    G = pr.capacity_for(N)
    labels = pr.ghost_labels(G) if labels is None else labels
    idx.add(pr.ghosts(p, G, kind), labels)
    assert idx.count() == G
    if via == "clear":
        idx.clear()
    elif via == "remove_all":
        assert idx.remove(labels) == G
    else:
        path = str(tmp_path / "live.idx")
        other = FlatIndex(D, dtype, capacity=N)
        try:
            other.add(p.rows, labels_of(N))
            other.save(path)
        finally:
            other.close()
        idx.load(path)             # over the full ghost index: no clear in between
        assert idx.count() == N
        return True
    assert idx.count() == 0
    return False


def check_queries(mods, idx, p, k, Q, exp, *, filtered=False, exclude_only=False, which=None, mode="first", plan_check=None,
                  kernels=(), extra_calls=(), what="", decoy_labels=None, row_of_label=None, pipelined=False):
    """Issue the queries `which` of p (all by default) Q per call (the last call is short; extra_calls: further (first, Q) calls
    into `which`) on the index as it stands, compare every answer with exp (labels, distances, counts of those queries, in that
    order), and hold the guard's accounting to `mode`: first (nothing widened, no widen kernel ran), widen (guard_force is set:
    every query widened, none exhaustively), exhaustive (at least one query ended in the canonical pass) or None (the caller
    looks at the returned delta itself). pipelined: one query_begin / query_next chain instead of query calls.
    Returns (labels, distances, counts, plan, delta of guard_stats, kernels that ran)."""
    FlatIndex, ro, roc, _lib = mods
    which = np.arange(p.n_queries) if which is None else np.asarray(which)
    queries = p.queries[which]
    Qt = which.size
    plan = _lib.index_plan(idx._h, Q, k, filtered, Q if mode == "widen" else 0)
    print(f"{what} plan(Q={Q}, k={k}): " + ", ".join(f"{f}={v}" for f, v in plan.items() if v))
    if plan_check:
        plan_check(plan)
    gl = np.empty((Qt, k), np.int64)
    gd = np.empty((Qt, k), np.float32)
    gc = np.empty(Qt, np.int32)

    def masks(sl):
        if not filtered:
            return {}
        return {"require": None if exclude_only else p.require[which[sl]], "exclude": p.exclude[which[sl]]}

    def call(j0, n):
        sl = slice(j0, min(j0 + n, Qt))
        return idx.query(queries[sl], k, **masks(sl))

    _lib.prof_reset()
    _lib.prof_enable(True)
    before = idx.guard_stats()
    try:
        if pipelined:
            slices = [slice(j0, min(j0 + Q, Qt)) for j0 in range(0, Qt, Q)]
            pending = idx.query_begin(queries[slices[0]], k, **masks(slices[0]))
            for prev, sl in zip(slices, slices[1:]):
                (gl[prev], gd[prev], gc[prev]), pending = idx.query_next(pending, queries[sl], k, **masks(sl))
            gl[slices[-1]], gd[slices[-1]], gc[slices[-1]] = pending.result()
        else:
            for j0 in range(0, Qt, Q):
                gl[j0:j0 + Q], gd[j0:j0 + Q], gc[j0:j0 + Q] = call(j0, Q)
        extras = [(j0, n, call(j0, n)) for j0, n in extra_calls]
    finally:
        _lib.prof_enable(False)
    after = idx.guard_stats()
    ran = {r["kernel"] for r in _lib.prof_read()}
    kw = {"row_of_label": row_of_label} if row_of_label else {}
    compare((gl, gd, gc), exp, plan, what, **kw)
    for j0, n, got in extras:
        compare(got, tuple(a[j0:j0 + n] for a in exp), plan, f"{what} extra call of {n} from query {j0}", **kw)
    nq = Qt + sum(min(j0 + n, Qt) - j0 for j0, n in extra_calls)
    delta = {s: after[s] - before[s] for s in after}
    assert delta["queries"] == nq, delta
    assert not (gl >= pr.GHOST_LABEL0).any()         # no dead row in any answer
    if decoy_labels is not None:                     # no decoy in any answer
        assert not np.isin(gl, decoy_labels).any()
    if mode == "widen":
        assert delta["widened"] == nq and delta["exhaustive"] == 0, delta
    elif mode == "exhaustive":
        assert delta["exhaustive"] >= 1 and "canonical_scan" in ran, (delta, ran)
    elif mode == "first":
        assert delta["widened"] == 0 and delta["rounds"] == 0 and delta["exhaustive"] == 0, delta
        assert not (ran & WIDEN_KERNELS), ran
    else:
        assert mode is None
    for name in kernels:
        assert name in ran, (name, ran)
    return gl, gd, gc, plan, delta, ran


class options_set:
    """the debug options of a test, set on entry and back at their defaults on exit"""

    def __init__(self, _lib, options):
        self._lib, self.options = _lib, dict(options or {})

    def __enter__(self):
        for o, v in self.options.items():
            self._lib.set_option(o, v)

    def __exit__(self, *exc):
        for o in self.options:
            self._lib.set_option(o, DEFAULTS[o])
        return False


def run(mods, case, dtype, Q, *, options=None, widen=False, plan_check=None, kernels=(), extra_calls=(), what="", ghosts=None,
        exclude_only=False, pipelined=False, tmp_path=None):
    """Add the corpus (labels 3 r + 5; ghosts=(kind, via): behind the dead rows of fill_with_ghosts), issue its queries Q per call
    (the last call is short; extra_calls: further (first, Q) calls), compare every answer with the oracle's. exclude_only: the
    queries of a filtered corpus pass no require mask. Returns (labels, distances, counts, plan)."""
    FlatIndex, ro, roc, _lib = mods
    p, N, D, k, filtered = case.corpus(), case.N, case.D, case.k, case.filtered
    options = dict(options or {})
    if widen:
        options["guard_force"] = 1
    labels = labels_of(N)
    idx = FlatIndex(D, dtype, capacity=N)
    try:
        with options_set(_lib, options):
            if not (ghosts and fill_with_ghosts(mods, idx, p, dtype, ghosts, tmp_path)):
                idx.add(p.rows, labels)
            if filtered:
                idx.set_tags(labels, p.tags)
            exp = expected_exclude_only(case, dtype) if exclude_only else expected(case, dtype)
            return check_queries(mods, idx, p, k, Q, exp, filtered=filtered, exclude_only=exclude_only,
                                 mode="widen" if widen else "first", plan_check=plan_check, kernels=kernels, extra_calls=extra_calls,
                                 what=what, decoy_labels=labels[p.decoy] if filtered else None, pipelined=pipelined)[:4]
    finally:
        idx.close()


def scan_names(dtype):
    return ("scan_topk_" + dtype, "merge_lists", "rerank")


def dense_names(dtype, sample=False):
    return ("score_gemm_" + dtype + ("_sample" if sample else ""), "select_topk", "merge_lists", "rerank")

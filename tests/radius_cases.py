"""What test_radius_cases_cpu.py (which pins these properties on the oracle alone) and test_index_radius_gpu.py (which runs the
index against them) share: the expected answer of a radius query, the radii at a planted row's own distance, the restated
threshold bound, and the near-duplicate corpus. Not a test module.

The expected answer of query q at radius R is the oracle's: the rows with retrieval_oracle.distances(q, stored)[r] <= R (a
float32 compare; a NaN distance is no member), admitted, sorted by (distance, label); total counts them all, the first
min(cap, total) fill the slots, unused slots are -1 / +inf. The canonical sum of a row does not depend on the other rows, so the
oracle over a subset of the rows gives the subset's bits of the oracle over all of them."""
import functools
from typing import NamedTuple

import numpy as np

import index_query_cases as iqc
import planted_rows as pr
from oracle import retrieval_oracle as ro

RADIUS = np.float32(0.35)      # between a planted row's 0.05 .. 0.20 and every other row's > 0.5
GAP = (0.25, 0.45)             # no distance of a planted corpus lies in here (test_radius_cases_cpu.py)
CHUNK = 1024                   # queries per chunk of a radius call (csrc/api_index.hip RADIUS_CHUNK)
SWEEP_FAST, SWEEP_CAP = 1024, 8192


def represented(stored) -> np.ndarray:
    """float32 [N, D]: the rows an index represents (what FlatIndex.get returns)"""
    return stored.represented() if hasattr(stored, "represented") else np.asarray(stored).astype(np.float32)


def members(q_raw, stored, labels, radius, cap, admit=None, row_min=-1):
    """one query against `stored` -> (labels [cap], distances [cap], count, total). admit: bool [N] or None; row_min: only rows
    above this row position (later_only)."""
    d = ro.distances(np.asarray(q_raw, np.float32).reshape(1, -1), stored)[0]
    with np.errstate(invalid="ignore"):
        ok = d <= np.float32(radius)
    if admit is not None:
        ok &= admit
    ok[:max(row_min + 1, 0)] = False
    idx = np.nonzero(ok)[0]
    idx = idx[np.lexsort((labels[idx], d[idx]))]
    out_l = np.full(cap, -1, np.int64)
    out_d = np.full(cap, np.inf, np.float32)
    n = min(cap, idx.size)
    out_l[:n], out_d[:n] = labels[idx[:n]], d[idx[:n]]
    return out_l, out_d, np.int32(n), np.int64(idx.size)


def expected(queries, stored, labels, radii, cap, admit=None, row_min=None):
    """`members` for every query -> (labels [Q, cap], distances [Q, cap], counts int32 [Q], totals int64 [Q]); radii a scalar or
    [Q], admit(j) -> bool [N], row_min [Q]"""
    Q = queries.shape[0]
    radii = np.broadcast_to(np.asarray(radii, np.float32), (Q,))
    out = [members(queries[j], stored, labels, radii[j], cap, admit(j) if admit else None, -1 if row_min is None else int(row_min[j]))
           for j in range(Q)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], np.int64))


def same(got, exp, what=""):
    gl, gd, gc, gt = (np.asarray(x) for x in got)
    el, ed, ec, et = exp
    np.testing.assert_array_equal(gt, et, err_msg=f"{what}: totals")
    np.testing.assert_array_equal(gc, ec, err_msg=f"{what}: counts")
    np.testing.assert_array_equal(gl, el, err_msg=f"{what}: labels")
    np.testing.assert_array_equal(gd.view(np.uint32), ed.view(np.uint32), err_msg=f"{what}: distance bits")


@functools.lru_cache(maxsize=None)
def planted_expected(case, dtype, cap):
    """The radius answer of EVERY query of a planted corpus at RADIUS, from the corpus's cached top-k (index_query_cases.expected:
    the C oracle, once per corpus and dtype): no row lies between 0.25 and 0.45 and a full query's (k + 1)-th row is further
    than 0.45 (test_radius_cases_cpu.py), so the members are the top-k entries within RADIUS."""
    el, ed, ec = iqc.expected(case, dtype)
    k = el.shape[1]
    assert cap >= k
    with np.errstate(invalid="ignore"):
        ok = (ed <= RADIUS) & (el >= 0)
    assert (ok[:, :-1] >= ok[:, 1:]).all()     # a prefix
    out_l = np.full((el.shape[0], cap), -1, np.int64)
    out_d = np.full((el.shape[0], cap), np.inf, np.float32)
    out_l[:, :k] = np.where(ok, el, -1)
    out_d[:, :k] = np.where(ok, ed, np.float32(np.inf))
    tot = ok.sum(1)
    return iqc._frozen((out_l, out_d, tot.astype(np.int32), tot.astype(np.int64)))


# ---------------------------------------------------------------------------------------------- boundary radii
def boundary_radii(d_sorted, t):
    """the two radii at planted rank t of a query whose sorted member distances are d_sorted: its own distance (t + 1 members)
    and the float below it (t members, the distances being strictly increasing up to t)"""
    r = np.float32(d_sorted[t])
    return r, np.nextafter(r, np.float32(-np.inf))


# ---------------------------------------------------------------------------------------------- the threshold's bound
def guard_terms(D, dtype):
    """(fixed, cnorm) of csrc/api_index.hip guard_terms, restated"""
    f8, f32 = dtype == "f8", dtype == "f32"
    cn = 1.07 if f8 else 1.0 + 2.0 ** -9
    e = 4.0 * D * 2.0 ** -24 * cn * (1.0 + 2.0 ** -9)
    if not f32:
        e += D * 2.0 ** -25 * cn
    if f8:
        e += 2.0 ** -23
    return e * 1.003 + 2.0 ** -21, (0.0 if f32 else cn * 1.003)


def query_operand(q_raw, dtype):
    """(qn float32 [D], qs: the scan's operand — qn itself for f32 rows, float16(qn) for f16 / fp8 rows)"""
    qn = ro.normalize_rows(np.asarray(q_raw, np.float32).reshape(1, -1), "f32")[0]
    return qn, (qn if dtype == "f32" else qn.astype(np.float16))


def eps_q(q_raw, D, dtype):
    """csrc/retrieval_kernels.h prep_queries_kernel: (fixed + cnorm |qs - qn|_2) x 1.0001, rounded up to float32"""
    fixed, cnorm = guard_terms(D, dtype)
    qn, qs = query_operand(q_raw, dtype)
    dq = float(np.sqrt(((qs.astype(np.float64) - qn.astype(np.float64)) ** 2).sum()))
    e = (fixed + cnorm * dq) * 1.0001
    ef = np.float32(e)
    return np.nextafter(ef, np.float32(np.inf)) if float(ef) < e else ef


def approx_score(q_raw, stored, rows, dtype):
    """an f32-accumulated dot product of the scan's query operand with stored rows `rows` (x inv for fp8 rows)"""
    _, qs = query_operand(q_raw, dtype)
    vals = np.asarray(stored)[rows].astype(np.float32)
    s = (vals * qs.astype(np.float32)[None, :]).sum(1, dtype=np.float32)
    return s * stored.inv[rows] if getattr(stored, "inv", None) is not None else s


# ---------------------------------------------------------------------------------------------- near-duplicate corpus
ND_N, ND_D, ND_SEED = 4099, 128, 11
ND_RADIUS = np.float32(0.01)
ND_COPY_GROUPS = (2, 3, 17)
ND_PERTURBED = 12
ND_BIG = 1100


class NearDup(NamedTuple):
    rows: np.ndarray       # float32 [N, D]
    labels: np.ndarray     # int64 [N], 7 r + 2
    groups: tuple          # ascending row ids of every planted group (copies, perturbed pairs, the big group last)
    big: np.ndarray        # the big group's rows


@functools.lru_cache(maxsize=None)
def near_dup_corpus() -> NearDup:
    rng = np.random.Generator(np.random.Philox(ND_SEED))
    rows = rng.standard_normal((ND_N, ND_D))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    slots = rng.permutation(ND_N)
    groups, at = [], 0

    def take(n):
        nonlocal at
        g = np.sort(slots[at:at + n])
        at += n
        return g

    def near(v, cos, n):
        u = rng.standard_normal((n, ND_D))
        u -= (u @ v)[:, None] * v[None, :]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        c = np.asarray(cos, np.float64).reshape(-1, 1)
        return c * v[None, :] + np.sqrt(1.0 - c * c) * u

    for n in ND_COPY_GROUPS:                       # exact byte copies
        g = take(n)
        rows[g] = rows[g[0]]
        groups.append(g)
    for c in np.linspace(0.999, 0.9995, ND_PERTURBED):   # one perturbed copy each
        g = take(2)
        rows[g[1]] = near(rows[g[0]], c, 1)[0]
        groups.append(g)
    big = take(ND_BIG)                             # near-copies of one centre: pairwise cosine 0.99995^2
    rows[big] = near(rows[big[0]], 0.99995, ND_BIG)
    groups.append(big)
    rows = (2.0 * rows).astype(np.float32)
    rows.setflags(write=False)
    return NearDup(rows, np.arange(ND_N, dtype=np.int64) * 7 + 2, tuple(groups), big)


@functools.lru_cache(maxsize=None)
def near_dup_stored(dtype):
    return ro.normalize_rows(near_dup_corpus().rows, dtype)


@functools.lru_cache(maxsize=None)
def near_dup_pairs(dtype):
    """The oracle's pair set at ND_RADIUS, queries = the represented rows: (a, b, dist) with row a < row b, ordered by (a, dist, b),
    as labels; and the smallest distance of any pair outside the planted groups. Candidates by a float64 product (cosine > 0.9),
    their distances by the oracle."""
    nd, stored = near_dup_corpus(), near_dup_stored(dtype)
    rep = represented(stored)
    r64 = rep.astype(np.float64)
    r64 = r64 / np.linalg.norm(r64, axis=1, keepdims=True)
    cos = r64 @ r64.T
    np.fill_diagonal(cos, -1.0)
    group_of = np.full(ND_N, -1)
    for i, g in enumerate(nd.groups):
        group_of[g] = i
    other = cos.copy()
    other[(group_of[:, None] == group_of[None, :]) & (group_of[:, None] >= 0)] = -1.0
    pa, pb, pd = [], [], []
    for a in np.nonzero((cos > 0.9).any(1))[0]:
        cand = np.nonzero(cos[a] > 0.9)[0]
        cand = cand[cand > a]
        if cand.size == 0:
            continue
        d = ro.distances(rep[a:a + 1], stored[cand])[0]
        keep = d <= ND_RADIUS
        cand, d = cand[keep], d[keep]
        order = np.lexsort((cand, d))
        pa.append(np.full(order.size, a)), pb.append(cand[order]), pd.append(d[order])
    a, b, d = np.concatenate(pa), np.concatenate(pb), np.concatenate(pd).astype(np.float32)
    return iqc._frozen((nd.labels[a], nd.labels[b], d)), float(1.0 - other.max())

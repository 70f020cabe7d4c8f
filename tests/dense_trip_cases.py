"""What the tests of the index scans PAST THEIR FIRST TRIP share (test_dense_trip_cases_cpu.py, test_index_dense_trips_gpu.py): the
corpora at the sizes where the row loops of the membership, assignment, cluster-sum and compaction kernels make a second trip, the
expected answers, the geometry of the trips and the comparators. Not a test module.

Sizes (all trip counts are READ from the plan — mmiss_dbg_index_dense_plan on the GPU, the host-only plans program of
test_index_plans_cpu.py without one — and asserted by the tests; nothing here repeats a grid constant):
  mid   N = 140 005 (N % 16 = 5), dim 128: past every threshold up to 131 072 — the dense scans run 8 tiles per block (two trips per
        wave; 12, three trips, for f32 rows against more than 32 operands), canonical_scan and assign_resolve make 2 and 3 trips,
        cluster_sums takes more than 64 rows per block, the subset compaction has 5 blocks.
  top   N = 1 048 629 (2^20 + 53), dim 128, f16: the pointwise kernels (member_count, assign_sizes, assign_decide, member_from_dist,
        member_merge_tags) make 5, 5, 3, 2 and 2 trips.
  wide  N = 20 005, dim 768, f32, 64 probes: the probe tile is 32 wide, so membership makes two passes, two trips each.

Expected answers. The definition is the canonical oracle's (oracle/retrieval_oracle.py): bit p of row r = distances(q, stored)[p, r]
<= R[p] as floats; row r goes to the centre minimising (distances(c, stored)[c, r], c). Evaluating it for every pair of the top
size takes minutes in numpy, so a pair is decided by the plain float64 product (exact_distances: BLAS order) when that distance is
farther than MARGIN = 2^-16 from the radius — for assignment: when the best and the second-best centre are farther apart than that —
and by the canonical oracle otherwise. MARGIN is derived, not fitted: the canonical dot product and the plain one each differ from
the real-number value by fewer than 200 fp64 additions of terms below 1 (< 2 * 10^-13 together, the fp8 rows' multiplication by
inv included), and the canonical distance then takes one float32 rounding of a value below 2 (<= 2^-23): a distance farther than
2^-16 from a float32 radius, or two distances farther apart than that, compare the same way in both arithmetics. Distance BITS
always come from the canonical arithmetic (canon_pair_distances, the element-wise form of retrieval_oracle.distances; the CPU test
holds the two to equal bits)."""
import tempfile

import numpy as np

from assign_cases import assign_from_distances, mirror
from oracle import retrieval_oracle as ro

D = 128
MID_N = 140005         # > 131 072 = 8192 x 16, the one-trip reach of canonical_scan_kernel: the largest threshold below 262 144
TOP_N = 1048629        # 2^20 + 53 > 1 048 576 = 4096 x 256, the one-trip reach of member_from_dist / member_merge_tags
WIDE = dict(N=20005, dim=768, P=64)
SIZES = {"mid": (MID_N, D), "top": (TOP_N, D), "wide": (WIDE["N"], WIDE["dim"])}
MARGIN = 2.0 ** -16
MAX_CANONICAL_SHARE = 0.01
NCOPY = 9000           # copies of row copy_of(name), all at one distance from every probe: more than the borderline list holds
OVERFLOW_PROBE = 2     # the probe whose radius the overflow tests set to exactly its distance to the copies
TAIL = 64              # the last TAIL rows lie near centres(16)[0 .. 15] in turn: every centre wins rows in a last trip of 53 rows
N_CENTRES = 130
_cache = {}
BLOCK = 32768


def labels_of(n):
    return np.arange(n, dtype=np.int64) * 3 + 5


def _freeze(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs[0] if len(arrs) == 1 else arrs


# ------------------------------------------------------------------------------------------------ corpora
def nodir_rows(N):
    """rows without a direction: zero and NaN in the first tile, NaN and zero in tile 5 (wave 1's second trip of the first slab,
    whatever the tiles per block), +inf in the last tile"""
    return [3, 5, 83, 84, N - 2]


def centres_base(dim=D):
    key = ("centres", dim)
    if key not in _cache:
        _cache[key] = _freeze(np.random.Generator(np.random.Philox(71)).standard_normal((N_CENTRES, dim), dtype=np.float32))
    return _cache[key]


def centres(C):
    """C of the base centres (every one with a direction), the last one replaced by mirror(centre 0): TIE_ROW below is at the SAME
    canonical distance from centres 0 and C - 1 (assign_cases.mirror) — a borderline row by construction, owed to centre 0"""
    key = ("centres", D, C)
    if key not in _cache:
        c = np.array(centres_base()[:C])
        c[C - 1] = mirror(c[0])
        _cache[key] = _freeze(c)
    return _cache[key]


def duplicated_centres():
    """[4, D]: centres 2, 3 are bit copies of centres 0, 1: every row's two best scores are equal, so every row with a direction is
    borderline and the resolve kernel's list holds all of them; no centre >= 2 wins a row"""
    key = ("dupcentres",)
    if key not in _cache:
        c = np.array(centres_base()[:2])
        _cache[key] = _freeze(np.concatenate([c, c]))
    return _cache[key]


def tie_value():
    c0 = centres_base()[0]
    return (c0 + mirror(c0)).astype(np.float32)


def tie_rows(N):
    """where tie_value() is planted: the second tile of wave 3's second trip of slab 7 at 8 tiles per block (tile 63), a row of
    the second and one of the third reach of a 65 536-row grid, one of the last full tile"""
    return [63 * 16 + 8, 65536 + 4097, 131072 + 1234, (N // 16 - 1) * 16 + 2] if N > 132400 else [63 * 16 + 8, N // 2 + 3]


def copy_rows(N):
    """the NCOPY rows that are copies of row copy_of(name): evenly spread, so every trip of every kernel has some"""
    step = (N - TAIL - 200) // NCOPY
    return 200 + 7 + step * np.arange(NCOPY, dtype=np.int64)


def copy_of(name):
    """the row the copies are copies of: among rows 100 .. 199 the one whose distance to probe OVERFLOW_PROBE is nearest to 1, the
    median distance of Gaussian rows — with its radius AT that distance the probe has members and non-members in every trip"""
    key = ("copy_of", name)
    if key not in _cache:
        if ("head", name) not in _cache:
            rows(name)
        x = _cache[("head", name)].astype(np.float64)
        q = probes(name)[:8].astype(np.float64)
        with np.errstate(all="ignore"):
            cos = (x @ q.T) / (np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(q, axis=1)[None, :])
        # ... and which stays 0.03 away from the radii of the other probes of an overflow call (the medians, about 1, of probes 0
        # and 6; probe 4's 0.9), hundreds of times the guard's eps: the copies fill the borderline list of the overflow probe alone
        clear = (np.abs(cos[:, 0]) > 0.03) & (np.abs(cos[:, 6]) > 0.03) & (np.abs(cos[:, 4] - 0.1) > 0.03)
        _cache[key] = 100 + int(np.argmin(np.where(clear, np.abs(cos[:, OVERFLOW_PROBE]), np.inf)))
    return _cache[key]


def _plain_rows(name):
    N, dim = SIZES[name]
    x = np.random.Generator(np.random.Philox({"mid": 61, "top": 62, "wide": 63}[name])).standard_normal((N, dim), dtype=np.float32)
    if dim == D:
        c = centres(16)
        for i in range(TAIL):
            if i % 16 in (0, 15):          # centre 15 is mirror(centre 0): without noise on the two components they differ in,
                x[N - TAIL + i, [0, 64]] = 0.0   # the row is nearer to its own by (c[0] - c[64])^2 / |row|
            x[N - TAIL + i] = c[i % 16] + np.float32(0.5) * x[N - TAIL + i]
        x[tie_rows(N)] = tie_value()
    x[3] = 0.0
    x[5, 5] = np.nan
    x[83] = np.nan
    x[84] = 0.0
    x[N - 2, 0] = np.inf
    _cache[("head", name)] = np.array(x[100:200])
    return x


def rows(name, copies=None):
    """float32 [N, dim] Philox Gaussian rows with rows without a direction at nodir_rows(N); at dim 128 also tie_value() at
    tie_rows(N) and the last TAIL rows near centres 0 .. 15 in turn. copies (default: the top corpus only): NCOPY copies of row
    copy_of(name) at copy_rows(N). Cached, read-only."""
    copies = (name == "top") if copies is None else copies
    key = ("rows", name, copies)
    if key not in _cache:
        x = np.array(_cache[("rows", name, False)]) if ("rows", name, False) in _cache else _plain_rows(name)
        if copies:
            x[copy_rows(x.shape[0])] = x[copy_of(name)]
        _cache[key] = _freeze(x)
    return _cache[key]


def probes(name):
    """float32 [64, dim]; probe 1 has no direction"""
    key = ("probes", name)
    if key not in _cache:
        q = np.random.Generator(np.random.Philox(81)).standard_normal((64, SIZES[name][1]), dtype=np.float32)
        q[1] = 0.0
        _cache[key] = _freeze(q)
    return _cache[key]


def stored(name, dtype, copies=None):
    """oracle.normalize_rows(rows(name), dtype), in blocks (rows are independent), once per corpus and dtype"""
    copies = (name == "top") if copies is None else copies
    key = ("stored", name, dtype, copies)
    if key not in _cache:
        if copies and ("stored", name, dtype, False) in _cache:      # (a copy of a row is a copy of its stored form)
            base = _cache[("stored", name, dtype, False)]
            vals = np.array(np.asarray(base))
            vals[copy_rows(vals.shape[0])] = vals[copy_of(name)]
            if getattr(base, "inv", None) is not None:
                inv = np.array(base.inv)
                inv[copy_rows(vals.shape[0])] = inv[copy_of(name)]
                out = ro.F8Rows(vals, inv)
            else:
                out = vals
        else:
            x = rows(name, copies)
            with np.errstate(all="ignore"):
                out = ro.concat_rows([ro.normalize_rows(x[r0:r0 + 65536], dtype) for r0 in range(0, x.shape[0], 65536)])
        _cache[key] = out
    return _cache[key]


def normalized(q):
    """float64 [n, dim]: the operands as the index normalises them (NaN rows for operands without a direction)"""
    with np.errstate(all="ignore"):
        return ro.normalize_rows(np.asarray(q, np.float32), "f32").astype(np.float64)


# ------------------------------------------------------------------------------------------------ distances
def exact_distances(q, st, block=65536):
    """float64 [n, N]: 1 - <q^, row> by plain float64 products in BLAS order (fp8 rows: x inv). NaN where the canonical distance
    is NaN: an operand or a row without a direction."""
    qn = normalized(q)
    vals, inv = np.asarray(st), getattr(st, "inv", None)
    out = np.empty((qn.shape[0], vals.shape[0]), np.float64)
    with np.errstate(all="ignore"):
        for r0 in range(0, vals.shape[0], block):
            dot = qn @ vals[r0:r0 + block].astype(np.float64).T
            if inv is not None:
                dot = dot * inv[r0:r0 + block].astype(np.float64)
            out[:, r0:r0 + block] = 1.0 - dot
    return out


def canon_pair_distances(q, st, row_idx, op_idx, block=32768):
    """float32 [M]: retrieval_oracle.distances(q, st)[op_idx[i], row_idx[i]] for M (row, operand) pairs, without the rest of the
    matrix: the same products, the same canon_sum, the same two roundings, element by element"""
    qn = normalized(q)
    vals, inv = np.asarray(st), getattr(st, "inv", None)
    row_idx, op_idx = np.asarray(row_idx, np.int64), np.asarray(op_idx, np.int64)
    out = np.empty(row_idx.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for i0 in range(0, row_idx.shape[0], block):
            r, o = row_idx[i0:i0 + block], op_idx[i0:i0 + block]
            dot = ro.canon_sum(vals[r].astype(np.float32).astype(np.float64) * qn[o])
            if inv is not None:
                dot = dot * inv[r].astype(np.float64)
            out[i0:i0 + block] = (1.0 - dot).astype(np.float32)
    return out


def distances_of(name, dtype, what, copies=None):
    """exact_distances of the corpus to its 64 probes (what = "probes") or to centres(C) (what = C), cached, read-only"""
    copies = (name == "top") if copies is None else copies
    key = ("exact", name, dtype, what, copies)
    if key not in _cache:
        ops = probes(name) if what == "probes" else centres(what)
        _cache[key] = _freeze(exact_distances(ops, stored(name, dtype, copies)))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ membership
def mixed_radii(d):
    """one radius per probe from its exact distances d [P, N], the kinds in turn: the probe's median distance, negative, 0, >= 2,
    0.9, +inf (probe 0 gets a median: a call of one probe has members and non-members)"""
    import warnings

    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        med = np.nanmedian(d, axis=1).astype(np.float32)
    med = np.where(np.isnan(med), np.float32(1.0), med)
    kinds = [lambda p: med[p], lambda p: -0.5, lambda p: 0.0, lambda p: 2.5, lambda p: 0.9, lambda p: np.inf]
    return np.array([kinds[p % 6](p) for p in range(d.shape[0])], np.float32)


def median_probes(P):
    return [p for p in range(P) if p % 6 == 0]


def expected_membership(q, st, R, d=None):
    """-> (words uint64 [N], counts int64 [P], member bool [P, N], canonical: the pairs the margin rule handed to the canonical
    oracle). d: exact_distances(q, st) if the caller has them. A probe without a direction has no member (every product with its
    NaN operand is NaN, and a NaN distance is no member): its pairs are not counted as canonical ones."""
    q = np.asarray(q, np.float32)
    R = np.asarray(R, np.float32)
    d = exact_distances(q, st) if d is None else d
    P, N = d.shape
    R64 = R.astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        mem = d <= R64
        undecided = ~(np.abs(d - R64) > MARGIN)        # (a NaN distance, and +inf - +inf, land here)
    dead = ~np.isfinite(normalized(q)).all(axis=1)
    undecided[dead] = False
    mem[dead] = False
    p_idx, r_idx = np.nonzero(undecided)
    if p_idx.size:
        cd = canon_pair_distances(q, st, r_idx, p_idx)
        with np.errstate(invalid="ignore"):
            mem[p_idx, r_idx] = cd <= R[p_idx]
    words = np.zeros(N, np.uint64)
    for p in range(P):
        words |= mem[p].astype(np.uint64) << np.uint64(p)
    return words, mem.sum(axis=1).astype(np.int64), mem, int(p_idx.size)


def mixed_call(name, dtype, P, copies=None):
    """the first P probes with mixed radii -> (q, R, expected_membership(...))"""
    key = ("mixed", name, dtype, P, copies)
    if key not in _cache:
        d = distances_of(name, dtype, "probes", copies)[:P]
        q, R = probes(name)[:P], mixed_radii(d)
        _cache[key] = (q, _freeze(R), expected_membership(q, stored(name, dtype, copies), R, d))
    return _cache[key]


def overflow_call(name, dtype):
    """a call on the corpus WITH copies whose probe at slot 2 has its radius at exactly its canonical distance to the copies:
    mid: the first 8 probes, mixed radii elsewhere; top: probes 0 (its median radius), 4 (+inf) and OVERFLOW_PROBE.
    -> (q, R, step 0: expected_membership with R, step 1: with the overflow radius one float below)"""
    key = ("overflow", name, dtype)
    if key not in _cache:
        which = np.arange(8) if name == "mid" else np.array([0, 4, OVERFLOW_PROBE])
        st = stored(name, dtype, True)
        d = distances_of(name, dtype, "probes", True)[which]
        q = probes(name)[which]
        R = mixed_radii(d)
        if name != "mid":
            R[1] = np.inf
        R[2] = canon_pair_distances(q, st, [copy_of(name)], [2])[0]
        below = R.copy()
        below[2] = np.nextafter(R[2], np.float32(-np.inf))
        _cache[key] = (_freeze(np.array(q)), _freeze(R), expected_membership(q, st, R, d), expected_membership(q, st, below, d))
    return _cache[key]


def border_call(name, dtype, tiles_per_block, slab):
    """8 probes; probe p of BORDER_PROBES[i] has its radius at exactly its canonical distance to one row of slab `slab`: the row at
    position 5 + wave of the tile wave `wave` takes on its trip `trip`, for wave 0 and wave 3 and every trip.
    -> (q, R, planted rows per probe {p: row}, step 0 expected, step 1 expected: the planted radii one float below)"""
    key = ("border", name, dtype, tiles_per_block, slab)
    if key not in _cache:
        st = stored(name, dtype, False)
        q = probes(name)[:8]
        d = distances_of(name, dtype, "probes", False)[:8]
        spots = [(w, t) for w in (0, 3) for t in range(tiles_per_block // 4)]
        live = [p for p in range(8) if p != 1]
        assert len(spots) <= len(live), (tiles_per_block, "more trips than probes to plant with")
        R = np.full(8, 0.9, np.float32)
        planted = {}
        for p, (w, t) in zip(live, spots):
            planted[p] = dense_row(slab, w, t, tiles_per_block, 5 + w)
            R[p] = canon_pair_distances(q, st, [planted[p]], [p])[0]
        below = R.copy()
        for p in planted:
            below[p] = np.nextafter(R[p], np.float32(-np.inf))
        _cache[key] = (q, _freeze(R), planted, expected_membership(q, st, R, d), _freeze(below), expected_membership(q, st, below, d))
    return _cache[key]


def assign_call(name, dtype, C, dist_rows=None):
    """centres(C) (C = "dup": duplicated_centres()) -> (centres, expected_assign(...)); dist_rows as expected_assign's"""
    key = ("assign", name, dtype, C, None if dist_rows is None else dist_rows.tobytes())
    if key not in _cache:
        c = duplicated_centres() if C == "dup" else centres(C)
        d = exact_distances(c, stored(name, dtype)) if C == "dup" else distances_of(name, dtype, C)
        _cache[key] = (c, expected_assign(c, stored(name, dtype), d, dist_rows))
    return _cache[key]


def expected_sums(represented_rows, assign, C):
    """assign_cases.expected_sums (the definition: the sum over a cluster's rows of rint(float64(x) * 2^32), entries of assign
    outside 0 .. C-1 skipped), by a sort and one reduceat instead of np.add.at -> (sums int64 [C, D], sizes int64 [C])"""
    x = np.asarray(represented_rows, np.float32)
    a = np.asarray(assign).astype(np.int64)
    ok = np.nonzero((a >= 0) & (a < C))[0]
    order = ok[np.argsort(a[ok], kind="stable")]
    sizes = np.bincount(a[ok], minlength=C).astype(np.int64)
    sums = np.zeros((C, x.shape[1]), np.int64)
    if order.size:
        fx = np.rint(x[order].astype(np.float64) * 2.0 ** 32).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        has = sizes > 0
        sums[has] = np.add.reduceat(fx, starts[has], axis=0)
    return sums, sizes


def synthetic_assign(N, C):
    """int32 [N]: every cluster of C (a power of two up to 1024) in every 1024 consecutive rows (7 r mod 1024 is a permutation of
    them), row 11 of every 97 in no cluster (-1), row 13 in cluster C (out of range: skipped)"""
    r = np.arange(N, dtype=np.int64)
    a = ((r * 7 + r // 1024) % C).astype(np.int32)
    a[r % 97 == 11] = -1
    a[r % 97 == 13] = C
    a[nodir_rows(N)] = -1          # (their elements are NaN: no fixed-point value)
    return a


# ------------------------------------------------------------------------------------------------ assignment
def expected_assign(c, st, d=None, dist_rows=None):
    """-> (assign int32 [N], dist float32 [N], sizes int64 [C], canonical: the (row, centre) pairs handed to the canonical oracle).
    dist_rows: the rows whose distance bits are wanted (default: all); the others' dist is NaN."""
    c = np.asarray(c, np.float32)
    d = exact_distances(c, st) if d is None else d
    C, N = d.shape
    key = np.where(np.isnan(d), np.inf, d)
    a = np.argmin(key, axis=0).astype(np.int32)
    if C > 1:
        two = np.partition(key, 1, axis=0)[:2]
        with np.errstate(invalid="ignore"):
            undecided = ~((two[1] - two[0]) > MARGIN)   # (inf - inf: a row without a direction, or one live centre)
    else:
        undecided = ~np.isfinite(key[0])
    r_idx = np.nonzero(undecided)[0]
    if r_idx.size:
        with np.errstate(all="ignore"):
            a[r_idx] = assign_from_distances(ro.distances(c, st[r_idx]))[0]
    dist = np.full(N, np.inf if dist_rows is None else np.nan, np.float32)
    want = np.arange(N) if dist_rows is None else np.asarray(dist_rows, np.int64)
    dist[want] = np.inf
    live = want[a[want] >= 0]
    dist[live] = canon_pair_distances(c, st, live, a[live])
    sizes = np.bincount(a[a >= 0], minlength=C).astype(np.int64)
    return a, dist, sizes, int(r_idx.size) * C


# ------------------------------------------------------------------------------------------------ trips
def dense_position(r, tiles_per_block):
    """(slab, wave, trip) of the dense scan that handles row r (numpy arrays in, arrays out): tile = r // 16 belongs to slab
    tile // tiles_per_block, and within it wave j % 4 takes tile j on its trip j // 4"""
    tile = np.asarray(r, np.int64) // 16
    j = tile % tiles_per_block
    return tile // tiles_per_block, j % 4, j // 4


def dense_row(slab, wave, trip, tiles_per_block, pos=0):
    return ((slab * tiles_per_block + wave + 4 * trip) * 16) + pos


def trip_ranges(N, rows_per_trip):
    """[(first, behind)] row ranges of the trips of a grid-stride kernel whose grid covers rows_per_trip rows at a time"""
    return [(r0, min(N, r0 + rows_per_trip)) for r0 in range(0, N, rows_per_trip)]


def boundary_rows(N, plan, around=64, extra=20000, seed=5):
    """rows within `around` of every trip boundary of every grid-stride kernel of `plan` (the dict of mmiss_dbg_index_dense_plan),
    the first and last `around` rows, and `extra` further seeded rows; ascending"""
    pick = [np.arange(0, min(N, around)), np.arange(max(0, N - around), N)]
    for k, v in plan.items():
        if isinstance(v, dict) and "rows_per_trip" in v:
            for b in range(v["rows_per_trip"], N, v["rows_per_trip"]):
                pick.append(np.arange(max(0, b - around), min(N, b + around)))
    pick.append(np.random.Generator(np.random.Philox(seed)).integers(0, N, extra))
    return np.unique(np.concatenate(pick))


# ------------------------------------------------------------------------------------------------ subset lists
def subset_list_rows(N, block_rows=BLOCK):
    """the rows the subset tests name, ascending: in every compaction block but block 2 the first and the last row; every seventh
    row of block 0, 2000 seeded rows of block 1, none of block 2, EVERY row of block 3, 1000 seeded rows of the last block"""
    nb = -(-N // block_rows)
    assert nb == 5, nb
    rng = np.random.Generator(np.random.Philox(91))
    span = lambda b: (b * block_rows, min(N, (b + 1) * block_rows))   # noqa: E731
    pick = []
    for b in (0, 1, 3, 4):
        pick.append(np.array([span(b)[0], span(b)[1] - 1]))
    pick.append(np.arange(*span(0), 7))
    pick.append(span(1)[0] + rng.integers(0, block_rows, 2000))
    pick.append(np.arange(*span(3)))
    pick.append(span(4)[0] + rng.integers(0, span(4)[1] - span(4)[0], 1000))
    return np.unique(np.concatenate(pick))


def block_off_zeroed(listed, block=1, block_rows=BLOCK):
    """what the scan would read as the row list had block_off[block] been 0: the block's rows written over the head of the list,
    and the places they belong to never written (the rows of the blocks behind them follow at their own offsets)"""
    listed = np.asarray(listed)
    mine = listed[(listed // block_rows) == block]
    out = np.array(listed)
    out[:mine.size] = mine
    return out


def subset_queries(name):
    """float32 [6, dim]: query 0 is row 0 itself (named by every list: the first row of block 0, and the nearest row there is),
    query 2 has no direction, the others are probes"""
    key = ("subq", name)
    if key not in _cache:
        q = np.array(probes(name)[10:16])
        q[0] = rows(name, False)[0]
        q[2] = 0.0
        _cache[key] = _freeze(q)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ comparators
def words_mismatch(got, exp, P=64):
    """None when the words are equal on every row, else a message that names the first rows"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != np.uint64:
        return f"words: shape / dtype {got.shape} {got.dtype}, expected {exp.shape} uint64"
    bad = np.nonzero(got != exp)[0]
    if bad.size:
        return (f"words: {bad.size} rows differ, first {bad[:5].tolist()}: got {[hex(int(v)) for v in got[bad[:5]]]}, "
                f"expected {[hex(int(v)) for v in exp[bad[:5]]]}")
    if P < 64 and (got >> np.uint64(P)).any():
        return f"words: bits >= {P} set"
    return None


def bits_mismatch(got, exp, at=None, what="dist"):
    """None when the float32 arrays have equal bits (on the rows `at`), else a message"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != np.float32:
        return f"{what}: shape / dtype {got.shape} {got.dtype}, expected {exp.shape} float32"
    g, e = (got, exp) if at is None else (got[at], exp[at])
    bad = np.nonzero(g.view(np.uint32) != e.view(np.uint32))[0]
    if bad.size:
        where = bad[:5] if at is None else np.asarray(at)[bad[:5]]
        return f"{what}: {bad.size} rows differ in bits, first {where.tolist()}: got {g[bad[:5]].tolist()}, expected {e[bad[:5]].tolist()}"
    return None


def ints_mismatch(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return f"{what}: shape / dtype {got.shape} {got.dtype}, expected {exp.shape} {exp.dtype}"
    bad = np.nonzero(got != exp)[0]
    if bad.size:
        return f"{what}: {bad.size} differ, first {bad[:5].tolist()}: got {got[bad[:5]].tolist()}, expected {exp[bad[:5]].tolist()}"
    return None


# ------------------------------------------------------------------------------------------------ plan figures without a GPU
def host_figures(dim, dtype, n_operands, N):
    """what mmiss_dbg_index_dense_plan reports for such an index, from the host-only plans program (test_index_plans_cpu.py)"""
    import test_index_plans_cpu as plans

    if "exe" not in _cache:
        _cache["tmp"] = tempfile.TemporaryDirectory()
        _cache["exe"] = plans.build_program(_cache["tmp"].name)
    key = ("figures", dim, dtype, n_operands, N)
    if key not in _cache:
        _cache[key] = plans.dense_figures(_cache["exe"], dim, 4 if dtype == "f32" else 2, n_operands, N)
    return _cache[key]

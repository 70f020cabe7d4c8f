"""What the assignment / clustering tests share (test_assign_cases_cpu.py, test_assign_layers_cpu.py, test_index_assign_gpu.py):
the numpy restatement of mmiss_index_assign, mmiss_index_cluster_sums and FlatIndex.kmeans on the retrieval oracle, the corpora
(cached: the tests share the arrays and leave them unchanged) and the comparator. Not a test module.

The restatement: with Dm = oracle.retrieval_oracle.distances(centres, stored) ([C, N] float32 canonical distances), row r goes to
the c that minimises (Dm[c, r], c) over the c whose Dm[c, r] is not NaN; no such c: -1 / +inf."""
import numpy as np

from oracle import retrieval_oracle as ro

_cache = {}
NODIR_MIN_N = 41          # corpora of more rows than this carry rows without a direction at NODIR_ROWS(N)


def nodir_rows(N):
    return [3, 17, N - 2, N // 2, N // 2 + 1]


def represented(stored):
    """float32 [N, D]: what mmiss_index_get returns for the stored rows"""
    return stored.represented() if hasattr(stored, "represented") else np.asarray(stored).astype(np.float32)


def oracle_distances(centres, stored):
    with np.errstate(all="ignore"):
        return ro.distances(np.asarray(centres, np.float32), stored)


def assign_from_distances(Dm):
    """(assign int32 [N], dist float32 [N], sizes int64 [C]) from Dm [C, N]"""
    C, N = Dm.shape
    nan = np.isnan(Dm)
    key = np.where(nan, np.float32(np.inf), Dm)
    a = np.argmin(key, axis=0) if N else np.zeros(0, np.int64)       # (the first minimum: ties go to the smaller index)
    d = key[a, np.arange(N)]
    none = nan.all(axis=0)
    a = np.where(none, -1, a).astype(np.int32)
    d = np.where(none, np.float32(np.inf), d).astype(np.float32)
    sizes = np.bincount(a[a >= 0], minlength=C).astype(np.int64)
    return a, d, sizes


def expected_assign(centres, stored):
    return assign_from_distances(oracle_distances(centres, stored))


def expected_sums(represented_rows, assign, C):
    """(sums int64 [C, D], sizes int64 [C]); entries of assign outside 0 .. C-1 are skipped"""
    x = np.asarray(represented_rows, np.float32)
    a = np.asarray(assign).astype(np.int64)
    ok = (a >= 0) & (a < C)
    fx = np.rint(x[ok].astype(np.float64) * 2.0 ** 32).astype(np.int64)
    sums = np.zeros((C, x.shape[1]), np.int64)
    np.add.at(sums, a[ok], fx)
    return sums, np.bincount(a[ok], minlength=C).astype(np.int64)


def expected_kmeans(stored, C, iters, init_pos=None, assign=None, sums=None):
    """FlatIndex.kmeans on row POSITIONS (init_pos None: floor(i n / C)) -> its dict plus `history`, the assignment of every
    update step. assign / sums: other evaluations of the same definitions than expected_assign / expected_sums (the large corpora
    of dense_trip_cases.py)"""
    expected_assign, expected_sums = assign or globals()["expected_assign"], sums or globals()["expected_sums"]
    x = represented(stored)
    n = x.shape[0]
    pos = (np.arange(C, dtype=np.int64) * n) // C if init_pos is None else np.asarray(init_pos, np.int64)
    centres = x[pos].copy()
    prev, done, history = None, 0, []
    for _ in range(iters):
        a = expected_assign(centres, stored)[0]
        if prev is not None and np.array_equal(a, prev):
            break
        prev = a
        history.append(a)
        sums, sizes = expected_sums(x, a, C)
        new = (sums.astype(np.float64) * 2.0 ** -32).astype(np.float32)
        keep = (sizes == 0) | ~sums.any(axis=1)
        new[keep] = centres[keep]
        centres = new
        done += 1
    a, d, s = expected_assign(centres, stored)
    return {"centres": centres, "assign": a, "dist": d, "sizes": s, "iterations": done, "history": history}


# ------------------------------------------------------------------------------------------------ corpora
def _freeze(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


def mirror(v):
    """v with components 0 and 64 exchanged: against a row x with x[0] == x[64] the canonical dot product adds the same two
    products first, in the other order (a + b == b + a), and then the same terms — the same bits; the same holds for the norm"""
    w = np.array(v, np.float32, copy=True)
    w[..., 0], w[..., 64] = v[..., 64], v[..., 0]
    return w


PLANTED_ROW = 7            # random_corpus: the row equidistant BY CONSTRUCTION from centres 0 and C - 1 (C >= 16)


def random_corpus(seed, N, dim, C):
    """rows [N, dim], centres [C, dim]. N > 40: rows without a direction (zero, NaN, +inf) at nodir_rows(N); C > 1: centre 1 has
    no direction. C >= 16 and N > 40: centre C - 1 is mirror(centre 0) and row PLANTED_ROW = centre 0 + centre C - 1, whose
    components 0 and 64 are equal: its two nearest centres are at the SAME canonical distance, a borderline row whatever the
    approximate scores are."""
    key = ("random", seed, N, dim, C)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(seed))
        x = rng.standard_normal((N, dim), dtype=np.float32)
        c = rng.standard_normal((C, dim), dtype=np.float32)
        if N >= NODIR_MIN_N:
            x[3] = 0.0
            x[17, 5] = np.nan
            x[N - 2, 0] = np.inf
            x[N // 2] = np.nan
            x[N // 2 + 1] = 0.0
            if C >= 16:
                c[C - 1] = mirror(c[0])
                x[PLANTED_ROW] = c[0] + c[C - 1]
        if C > 1:
            c[1] = 0.0
        _cache[key] = _freeze(x, c)
    return _cache[key]


def winner_of(r, C):
    """every_winner_corpus: the centre planted as the winner of row r — tile t = r // 16, position p = r % 16: (t + p) % C"""
    return (r // 16 + r % 16) % C


def every_winner_corpus(seed, dim, C):
    """N = 16 C rows: row r is centre winner_of(r, C) plus small noise. Over the C tiles every centre is the winner at every row
    position mod 16, and (C >= 16) the 16 rows of a tile have 16 different winners: every column of a centre tile, every pass."""
    key = ("winner", seed, dim, C)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(seed))
        c = rng.standard_normal((C, dim), dtype=np.float32)
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        N = 16 * C
        noise = rng.standard_normal((N, dim), dtype=np.float32) * np.float32(0.1 / np.sqrt(dim))
        x = (c[[winner_of(r, C) for r in range(N)]] + noise).astype(np.float32)
        _cache[key] = _freeze(x, c)
    return _cache[key]


TIE_C = 17
DUP, DUP_OF = 7, 2         # centre 7 is a bit copy of centre 2
NEAR, NEAR_OF = 9, 4       # centre 9 is centre 4 with its largest component moved by one float ulp


def ties_corpus(seed, N, dim):
    """rows [N, dim], centres [TIE_C, dim]: the duplicate and the one-ulp centre above; rows 20 .. 20 + TIE_C - 1 are exact copies
    of the centres, rows 40 .. 40 + 2 TIE_C - 1 are c_a + c_b of neighbouring (and the special) centres; rows without a direction
    at nodir_rows(N); the rest random."""
    key = ("ties", seed, N, dim)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(seed))
        x = rng.standard_normal((N, dim), dtype=np.float32)
        c = rng.standard_normal((TIE_C, dim), dtype=np.float32)
        c[DUP] = c[DUP_OF]
        c[NEAR] = c[NEAR_OF]
        j = int(np.argmax(np.abs(c[NEAR_OF])))
        c[NEAR, j] = np.nextafter(c[NEAR_OF, j], np.float32(np.inf))
        x[20:20 + TIE_C] = c
        for i in range(TIE_C):
            x[40 + i] = c[i] + c[(i + 1) % TIE_C]
        pairs = [(DUP_OF, DUP), (NEAR_OF, NEAR), (DUP_OF, NEAR_OF), (DUP, NEAR)]
        for i in range(TIE_C):
            a, b = pairs[i % len(pairs)]
            x[40 + TIE_C + i] = c[a] * np.float32(1.0 + i / 8.0) + c[b]
        x[3] = 0.0
        x[17, 5] = np.nan
        x[N - 2, 0] = np.inf
        x[N // 2] = np.nan
        x[N // 2 + 1] = 0.0
        _cache[key] = _freeze(x, c)
    return _cache[key]


def duplicate_corpus(seed, N, dim, K):
    """rows [N, dim], centres [2 K, dim] with centres[K + i] a bit copy of centres[i]: EVERY row's two best scores belong to a
    pair of identical operands and are equal, so every row with a direction is borderline, and no centre >= K wins a row.
    Centres 1 and K + 1 have no direction; rows without a direction at nodir_rows(N)."""
    key = ("dup", seed, N, dim, K)
    if key not in _cache:
        rng = np.random.Generator(np.random.Philox(seed))
        x = rng.standard_normal((N, dim), dtype=np.float32)
        c = rng.standard_normal((K, dim), dtype=np.float32)
        c[1] = 0.0
        c = np.concatenate([c, c])
        x[3] = 0.0
        x[17, 5] = np.nan
        x[N - 2, 0] = np.inf
        x[N // 2] = np.nan
        x[N // 2 + 1] = 0.0
        _cache[key] = _freeze(x, c)
    return _cache[key]


def expected_passes(C, dim, dtype):
    """passes over the index of an assign call: the centre tile is the narrowest of 16 / 32 / 64 that holds C, halved while its
    staged operands (16 nqt rows of dim elements + 16 bytes each; f16 operands for f16 and fp8 rows) exceed 160 KiB of LDS"""
    qelt = 4 if dtype == "f32" else 2
    nqt = 4 if C > 32 else 2 if C > 16 else 1
    while nqt > 1 and 16 * nqt * (dim * qelt + 16) > 160 * 1024:
        nqt //= 2
    return -(-C // (16 * nqt))


KMEANS = dict(seed=31, N=2000, dim=128, C=17, iters=5, blobs=12)


def kmeans_corpus():
    """N rows around `blobs` random directions (fewer than C: the default initial centres split blobs and the first updates move
    rows between clusters)"""
    key = ("kmeans",)
    if key not in _cache:
        k = KMEANS
        rng = np.random.Generator(np.random.Philox(k["seed"]))
        b = rng.standard_normal((k["blobs"], k["dim"]), dtype=np.float32)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        which = rng.integers(0, k["blobs"], k["N"])
        x = (b[which] + rng.standard_normal((k["N"], k["dim"]), dtype=np.float32) * np.float32(1.0 / np.sqrt(k["dim"]))).astype(np.float32)
        _cache[key] = _freeze(x)
    return _cache[key][0]


def stored_of(x, dtype):
    """oracle.normalize_rows(x, dtype), once per (array, dtype)"""
    key = ("stored", id(x), dtype)
    if key not in _cache:
        with np.errstate(all="ignore"):
            _cache[key] = (x, ro.normalize_rows(x, dtype))     # (x kept: its id stays taken)
    return _cache[key][1]


def expected_of(x, c, dtype):
    """expected_assign(c, stored_of(x, dtype)) and the distance matrix, once per (arrays, dtype), read-only"""
    key = ("expected", id(x), id(c), dtype)
    if key not in _cache:
        Dm = oracle_distances(c, stored_of(x, dtype))
        a, d, s = assign_from_distances(Dm)
        _cache[key] = (x, c) + _freeze(Dm, a, d, s)
    return _cache[key][2:]


# ------------------------------------------------------------------------------------------------ comparator
def mismatch(got, exp):
    """None when (assign, dist | None, sizes) equals the expected triple in every element (distances by their bits), else a
    message that names the first difference"""
    ga, gd, gs = got
    ea, ed, es = exp
    ga, gs = np.asarray(ga), np.asarray(gs)
    if ga.shape != ea.shape or ga.dtype != np.int32:
        return f"assign: shape / dtype {ga.shape} {ga.dtype}, expected {ea.shape} int32"
    bad = np.nonzero(ga != ea)[0]
    if bad.size:
        return f"assign: {bad.size} rows differ, first {bad[:5].tolist()}: got {ga[bad[:5]].tolist()}, expected {ea[bad[:5]].tolist()}"
    if gd is not None:
        gd = np.asarray(gd)
        if gd.shape != ed.shape or gd.dtype != np.float32:
            return f"dist: shape / dtype {gd.shape} {gd.dtype}"
        bad = np.nonzero(gd.view(np.uint32) != ed.view(np.uint32))[0]
        if bad.size:
            return f"dist: {bad.size} rows differ in bits, first {bad[:5].tolist()}: got {gd[bad[:5]].tolist()}, expected {ed[bad[:5]].tolist()}"
    if gs.shape != es.shape or gs.dtype != np.int64 or not np.array_equal(gs, es):
        return f"sizes: got {gs.tolist()}, expected {es.tolist()}"
    return None


def sums_mismatch(got, exp):
    """None when (sums, sizes) equal the expected pair in every element"""
    gs, gn = np.asarray(got[0]), np.asarray(got[1])
    if gs.shape != exp[0].shape or gs.dtype != np.int64:
        return f"sums: shape / dtype {gs.shape} {gs.dtype}, expected {exp[0].shape} int64"
    bad = np.argwhere(gs != exp[0])
    if bad.size:
        c, j = bad[0]
        return f"sums: {bad.shape[0]} elements differ, first [{c}, {j}]: got {gs[c, j]}, expected {exp[0][c, j]}"
    if gn.dtype != np.int64 or not np.array_equal(gn, exp[1]):
        return f"sizes: got {gn.tolist()}, expected {exp[1].tolist()}"
    return None

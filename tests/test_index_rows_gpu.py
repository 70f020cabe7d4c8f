"""The index's row store on the MI355X, byte for byte: every writer (normalize_rows_kernel, f8_row_inv_kernel; add, update, load),
mover (gather_rows_kernel, the copies of a growing capacity) and reader (gather_rows_f32_kernel, gather_rows_f8_f32_kernel) and the
query preparation (prep_queries_kernel), read back raw through mmiss_dbg_index_read_rows / mmiss_dbg_index_prep_queries and
compared with bytes index_row_cases.py derives itself (exact rows, scaled twins, double-rounding witnesses) or takes from
oracle/retrieval_oracle.py (general rows). Every row and every element is compared; the one exception is an fp8 zero code, whose
sign is free (index_row_cases.check_rows). test_index_row_cases_cpu.py shows that the comparator fails on the defects it is for."""
import struct

import numpy as np
import pytest

import index_row_cases as rc

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "f8"]
MAX_DIM = {"f32": 1920, "f16": 3968, "f8": 3968}


@pytest.fixture(scope="module")
def mods(mm):
    import torch

    from mmiss_amd import _lib
    from mmiss_amd.index import FlatIndex

    return FlatIndex, _lib, torch


def _capacity(most_rows: int) -> int:
    cap = 1024
    while cap < most_rows:
        cap *= 2
    return cap


def _read(mods, idx, most_rows: int) -> rc.Store:
    """The whole row store of `idx`, whose capacity follows from the most rows it ever held (1024 doubled until it fits): one row
    more is refused."""
    _, _lib, _ = mods
    cap = _capacity(most_rows)
    with pytest.raises(_lib.MmissError):
        _lib.index_read_rows(idx._h, idx.dim, idx.dtype, 0, cap + 1)
    with pytest.raises(_lib.MmissError):
        _lib.index_read_rows(idx._h, idx.dim, idx.dtype, cap, 1)
    d = _lib.index_read_rows(idx._h, idx.dim, idx.dtype, 0, cap)
    return rc.Store(rc.to_codes(d["rows"]), d["inv"], d["labels"], d["tags"])


def _src(mods, x, device: bool):
    return mods[2].from_numpy(x).cuda() if device else x


_CACHE = {}


def _gauss(n, D, seed):
    """Gaussian rows at log-uniform scales (distinct norms, distinct fp8 inverse norms)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D)) * 10.0 ** rng.uniform(-6, 6, size=(n, 1))).astype(np.float32)


def _mixed(n, D, dtype, seed):
    """(x [n, D], codes, inv): the writer corpus of dimension D (known and general rows, the ones without a direction among them)
    followed by Gaussian rows up to n, with their reference bytes. Computed once per shape and dtype."""
    key = (n, D, dtype, seed)
    if key not in _CACHE:
        xw, _ = rc.writer_corpus(D)
        cw, iw = rc.writer_reference(D, dtype)
        g = _gauss(n - xw.shape[0], D, seed)
        cg, ig = rc.oracle_store(g, dtype)
        _CACHE[key] = (np.concatenate([xw, g]), np.concatenate([cw, cg]), None if iw is None else np.concatenate([iw, ig]))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ writers
@pytest.mark.parametrize("device_src", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dim", [128, 384, 1024, "max"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_stores_the_reference_bytes(mods, dtype, dim, device_src):
    """normalize_rows_kernel<float / _Float16 / F8> and f8_row_inv_kernel through add: calls of 1, 2, 3, 4, 5 rows and of the rest of
    the corpus (one wave per row, four rows per block: every remainder, a full grid), exact rows, scaled twins, witnesses and general
    rows, from the host and from the device."""
    FlatIndex, _, _ = mods
    D = MAX_DIM[dtype] if dim == "max" else dim
    x, _ = rc.writer_corpus(D)
    codes, inv = rc.writer_reference(D, dtype)
    N = x.shape[0]
    labels = np.arange(N, dtype=np.int64) * 3 + 7
    idx = FlatIndex(D, dtype)
    r0 = 0
    for n in (1, 2, 3, 4, 5, N - 15):
        idx.add(_src(mods, np.ascontiguousarray(x[r0:r0 + n]), device_src), labels[r0:r0 + n])
        r0 += n
    assert r0 == N == idx.count()
    rc.check_store(_read(mods, idx, N), rc.Store(codes, inv, labels, np.zeros(N, np.uint64)), dtype, N)
    idx.close()


@pytest.mark.parametrize("device_src", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_across_the_chunk_boundary(mods, dtype, device_src):
    """One add of 65 536 + 5 rows behind 3 rows: two chunks, the staging buffer used twice (host source), the second chunk's rows and
    inverse norms at count + 65 536 with count no multiple of 4."""
    FlatIndex, _, _ = mods
    D, n = 128, 3 + 65536 + 5
    x, codes, inv = _mixed(n, D, dtype, seed=11)
    # (the corpus rows sit at the front; the chunk boundary, three rows before the end of the first 65 536, gets known rows of its own)
    k, at = 64, n - 64
    x, codes = x.copy(), codes.copy()
    x[at:], codes[at:] = x[:k], codes[:k]
    if inv is not None:
        inv = inv.copy()
        inv[at:] = inv[:k]
    labels = np.arange(n, dtype=np.int64) * 2 + 1
    idx = FlatIndex(D, dtype)
    idx.add(_src(mods, np.ascontiguousarray(x[:3]), device_src), labels[:3])
    idx.add(_src(mods, np.ascontiguousarray(x[3:]), device_src), labels[3:])
    rc.check_store(_read(mods, idx, n), rc.Store(codes, inv, labels, np.zeros(n, np.uint64)), dtype, n)
    idx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_growth_keeps_rows_inverse_norms_labels_and_tags(mods, dtype):
    """index_reserve's copies: 1024 -> 2048 -> 4096 with tags set before each growth."""
    FlatIndex, _, _ = mods
    D, n = 128, 2100
    x, codes, inv = _mixed(n, D, dtype, seed=12)
    labels = np.arange(n, dtype=np.int64) + 5
    tags = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    idx = FlatIndex(D, dtype)
    done = 0
    for upto in (1000, 1100, 2100):
        idx.add(x[done:upto], labels[done:upto])
        idx.set_tags(labels[done:upto], tags[done:upto])
        done = upto
        rc.check_store(_read(mods, idx, done), rc.Store(codes[:done], None if inv is None else inv[:done], labels[:done], tags[:done]),
                       dtype, done)
    assert _capacity(1000) == 1024 and _capacity(1100) == 2048 and _capacity(2100) == 4096
    idx.close()


@pytest.mark.parametrize("device_src", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_rewrites_exactly_its_rows(mods, dtype, device_src):
    """update: one launch per label at that label's row (rows and inverse norms), the first and the last row among them, a label
    given twice (the later vector stays); every other row, every label and every tag as before."""
    FlatIndex, _, _ = mods
    D, n = 384, 301
    x, codes, inv = _mixed(800, D, dtype, seed=13)
    nk = rc.known_rows(D).x.shape[0]
    base = slice(nk, nk + n)                       # general rows first ...
    labels = np.arange(n, dtype=np.int64) * 5
    tags = np.arange(1, n + 1, dtype=np.uint64) << np.uint64(33)
    idx = FlatIndex(D, dtype)
    idx.add(x[base], labels)
    idx.set_tags(labels, tags)
    rows = np.array([0, n - 1, 17, 150, 17, 151, 2, 150, 299])      # ... then known rows over them; 17 and 150 twice
    src = np.linspace(0, nk - 1, rows.size).astype(np.int64)         # exact rows, twins, witnesses
    idx.update(labels[rows], _src(mods, np.ascontiguousarray(x[src]), device_src))
    want, winv = codes[base].copy(), None if inv is None else inv[base].copy()
    for r, s in zip(rows, src):                                      # (in call order)
        want[r] = codes[s]
        if winv is not None:
            winv[r] = inv[s]
    assert not np.array_equal(codes[src[2]], codes[src[4]])
    rc.check_store(_read(mods, idx, n), rc.Store(want, winv, labels, tags), dtype, n)
    idx.close()


BIG_N, BIG_D = 4200, 256   # more than 2^20 elements: the gathers' grid (4096 blocks of 256) strides


def _big(mods, dtype):
    FlatIndex, _, _ = mods
    x, codes, inv = _mixed(BIG_N, BIG_D, dtype, seed=14)
    labels = np.arange(BIG_N, dtype=np.int64) * 7 + 3
    tags = np.arange(1, BIG_N + 1, dtype=np.uint64) * np.uint64(0x0101010101010101)
    idx = FlatIndex(BIG_D, dtype)
    idx.add(x, labels)
    idx.set_tags(labels, tags)
    return idx, rc.Store(codes, inv, labels, tags)


@pytest.mark.parametrize("dtype", DTYPES)
def test_remove_compacts_every_kept_row(mods, dtype):
    """gather_rows_kernel<Bits> (and <float> on inv) past 4096 x 256 elements: row 0, the last row, a run of consecutive rows and
    scattered ones leave; rows, inverse norms, labels and tags of every kept row move up in order."""
    idx, ref = _big(mods, dtype)
    drop = np.unique(np.concatenate([[0, BIG_N - 1], np.arange(100, 141), np.arange(50, BIG_N, 211), [BIG_N - 2]]))
    keep = np.setdiff1d(np.arange(BIG_N), drop)
    assert keep.size * BIG_D > (1 << 20) + BIG_D
    assert idx.remove(np.concatenate([ref.labels[drop], [1, 2]])) == drop.size     # (two labels that are not stored)
    want = rc.Store(ref.rows[keep], None if ref.inv is None else ref.inv[keep], ref.labels[keep], ref.tags[keep])
    rc.check_store(_read(mods, idx, BIG_N), want, dtype, keep.size)
    assert np.array_equal(idx.labels(), ref.labels[keep])
    idx.close()


@pytest.mark.parametrize("device_out", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_get_returns_the_stored_rows_widened(mods, dtype, device_out):
    """gather_rows_f32_kernel<T> / gather_rows_f8_f32_kernel past 4096 x 256 elements, all rows in reversed and in repeated label
    order: the stored values widened (f32, f16), float32(values * inv) (fp8), bit for bit, the rows without a direction included."""
    _, _lib, torch = mods
    idx, ref = _big(mods, dtype)
    full = rc.get_reference(ref.rows, ref.inv, dtype)
    rng = np.random.default_rng(15)
    for order in (np.arange(BIG_N)[::-1].copy(), rng.integers(0, BIG_N, size=BIG_N + 77)):
        lab = np.ascontiguousarray(ref.labels[order])
        if device_out:
            out = torch.full((lab.size, BIG_D), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            _lib.check(idx._lib.mmiss_index_get(idx._h, lab.ctypes.data, int(lab.size), out.data_ptr()))
            got = out.cpu().numpy()
        else:
            got = idx.get(lab)
        rc.check_rows(got, full[order], "f32", what="get", f8_nan=dtype == "f8")
    idx.close()


def _file_rows(path, D, elt):
    """(count, labels, raw row bytes) of an index file."""
    raw = open(path, "rb").read()
    magic, version, dim, dtype, _, count = struct.unpack("<8siiiiq", raw[:32])
    assert magic == b"MMISSIDX" and version == 1 and dim == D
    labels = np.frombuffer(raw, dtype=np.int64, count=count, offset=32)
    body = raw[32 + 8 * count:]
    assert len(body) == count * D * elt
    return count, labels, body


@pytest.mark.parametrize("dtype", DTYPES)
def test_save_then_load_into_a_fuller_handle(mods, dtype, tmp_path):
    """save writes the stored bytes; load into a handle that held more rows (and tags) leaves exactly the file's rows, the inverse
    norms recomputed from the codes, and zero inverse norms and tags behind count and zero tags below it."""
    FlatIndex, _, _ = mods
    D = 128
    xw, _ = rc.writer_corpus(D)
    cw, iw = rc.writer_reference(D, dtype)
    sel = np.linspace(0, xw.shape[0] - 1, 150).astype(np.int64)
    sel[-4:] = np.arange(xw.shape[0] - 4, xw.shape[0])                 # (the rows without a direction)
    sel = np.unique(sel)
    n = sel.size
    labels = np.arange(n, dtype=np.int64) * 11
    a = FlatIndex(D, dtype)
    a.add(xw[sel], labels)
    a.set_tags(labels, np.full(n, 5, np.uint64))
    path = str(tmp_path / "rows.idx")
    a.save(path)
    got_a = _read(mods, a, n)
    count, flab, body = _file_rows(path, D, got_a.rows.dtype.itemsize)
    assert count == n and np.array_equal(flab, labels) and body == got_a.rows[:n].tobytes()
    b = FlatIndex(D, dtype)
    b.add(_gauss(300, D, 16), np.arange(300, dtype=np.int64))
    b.set_tags(np.arange(300, dtype=np.int64), np.full(300, 0xFFFF, np.uint64))
    b.load(path)
    want = rc.Store(cw[sel], None if iw is None else iw[sel], labels, np.zeros(n, np.uint64))
    got_b = _read(mods, b, 300)
    rc.check_store(got_b, want, dtype, n)
    assert got_b.rows[:n].tobytes() == body                           # (the bytes themselves, zero codes' signs included)
    if dtype == "f8":
        assert np.array_equal(rc.to_codes(got_b.inv[:n]), rc.to_codes(got_a.inv[:n]))    # (the same kernel on the same codes: NaNs too)
    a.close(); b.close()


def test_load_recomputes_power_of_two_inverse_norms(mods, tmp_path):
    """f8_row_inv_kernel through load_rows on a written file of exact codes whose values have norm 2^-j: inv = 2^j exactly."""
    FlatIndex, _, _ = mods
    D = 1024
    codes, inv = rc.pow2_file_rows(D)
    n = codes.shape[0]
    labels = np.arange(n, dtype=np.int64) + 100
    path = str(tmp_path / "pow2.idx")
    with open(path, "wb") as f:
        f.write(struct.pack("<8siiiiq", b"MMISSIDX", 1, D, 2, 0, n) + labels.tobytes() + codes.tobytes())
    b = FlatIndex(D, "f8")
    b.add(_gauss(40, D, 17), np.arange(40, dtype=np.int64))
    b.load(path)
    got = _read(mods, b, 40)
    rc.check_store(got, rc.Store(codes, inv, labels, np.zeros(n, np.uint64)), "f8", n)
    assert got.rows[:n].tobytes() == codes.tobytes()
    b.close()


# ------------------------------------------------------------------------------------------------ query preparation
def _no_direction(x):
    with np.errstate(all="ignore"):
        s = (x.astype(np.float64) ** 2).sum(axis=1)
    return ~(np.isfinite(s) & (s > 0))


@pytest.mark.parametrize("dim", [128, 1024])
@pytest.mark.parametrize("dtype", DTYPES)
def test_prep_queries(mods, dtype, dim):
    """prep_queries_kernel<float / _Float16>: qn bit for bit, qs = qn (f32 rows) or RNE_f16(qn), zero pad rows up to the next
    multiple of 256 (after a larger call too), eps_q rounded up from the guard's bound and never more than one float32 above it, +inf
    for the queries without a direction, one value for every query of an f32 index."""
    FlatIndex, _lib, torch = mods
    D = dim
    xw, known = rc.writer_corpus(D)
    qn_ref, _ = rc.writer_reference(D, "f32")
    qs_ref = qn_ref if dtype == "f32" else rc.writer_reference(D, "f16")[0]
    # the rows without a direction first (behind one ordinary row), so that the short calls hold them too
    N = xw.shape[0]
    order = np.concatenate([[0], np.arange(N - rc.NON_FINITE_ROWS, N), np.arange(1, N - rc.NON_FINITE_ROWS)])
    nodir = _no_direction(xw)
    assert nodir.sum() == rc.NON_FINITE_ROWS and nodir[N - rc.NON_FINITE_ROWS:].all()
    idx = FlatIndex(D, dtype)
    idx.add(_gauss(8, D, 18), np.arange(8, dtype=np.int64))
    h = idx._h
    e_all = rc.eps_reference(qn_ref, qs_ref, D, dtype)
    fixed, cnorm = rc.guard_terms(D, dtype)
    plan = [(256, 5, False), (3, 0, False), (1, 0, False), (4, 0, False), (255, 120, False), (257, 0, False), (256, N - 256, True),
            (3, 1, True)]
    for Q, start, dev in plan:
        sel = order[start:start + Q]
        assert sel.size == Q
        if Q == 256:
            assert not nodir[sel].all()
        q = np.ascontiguousarray(xw[sel])
        if dev:
            qd = torch.from_numpy(q).cuda()
            idx._sync_stream(qd)
            qn, qs, eps = _lib.index_prep_queries(h, D, idx.dtype, qd)
        else:
            idx._sync_stream(q)
            qn, qs, eps = _lib.index_prep_queries(h, D, idx.dtype, q)
        Qpad = (Q + 255) // 256 * 256
        assert qs.shape == (Qpad, D)
        rc.check_rows(qn, qn_ref[sel], "f32", what=f"qn Q={Q}")
        rc.check_rows(qs[:Q], qs_ref[sel], "f32" if dtype == "f32" else "f16", what=f"qs Q={Q}")
        assert not rc.to_codes(qs[Q:]).any(), f"pad rows of qs are not zero (Q={Q})"
        rc.check_eps(eps, e_all[sel], ~nodir[sel])
        if dtype == "f32":
            fin = eps[~nodir[sel]]
            assert cnorm == 0.0 and np.unique(fin).size <= 1
            assert (fin.astype(np.float64) >= fixed * 1.0001).all()
    # the exact rows: |qs - qn|_2 is known exactly from the catalogue (qn = x, qs = RNE_f16(x)), and e with it
    if dtype != "f32":
        from fractions import Fraction
        import math

        for r in (0, 1, 7, 20):
            assert known.norms[r] == 1
            dq = Fraction(0)
            for d in np.nonzero(known.x[r])[0]:
                a = abs(rc.frac(known.x[r, d]))
                dq += (rc.value(rc.store_code(a, "f16"), rc.F16) - a) ** 2
            e_exact = (fixed + cnorm * math.sqrt(dq)) * 1.0001
            assert abs(e_exact - e_all[r]) <= 1e-12 * e_exact
            q = np.ascontiguousarray(known.x[r:r + 1])
            idx._sync_stream(q)
            eps = _lib.index_prep_queries(h, D, idx.dtype, q)[2]
            assert e_exact * (1 - 1e-12) <= float(eps[0]) <= float(np.nextafter(np.float32(e_exact * (1 + 1e-12)), np.float32(np.inf)))
    idx.close()


def test_debug_entries_refuse_an_open_query_and_leave_the_index_as_it_was(mods):
    FlatIndex, _lib, _ = mods
    D = 128
    x = _gauss(50, D, 19)
    labels = np.arange(50, dtype=np.int64)
    idx = FlatIndex(D, "f8")
    idx.add(x, labels)
    before = idx.query(x[:5], 3)
    pend = idx.query_begin(x[:5], 3)
    with pytest.raises(_lib.MmissError):
        _lib.index_read_rows(idx._h, D, idx.dtype, 0, 10)
    with pytest.raises(_lib.MmissError):
        _lib.index_prep_queries(idx._h, D, idx.dtype, x[:2])
    pend.result()
    s1 = _read(mods, idx, 50)
    _lib.index_prep_queries(idx._h, D, idx.dtype, x[:7])
    _lib.check(idx._lib.mmiss_dbg_index_read_rows(idx._h, 0, 10, None, None, None, None))      # (every output may be null)
    _lib.check(idx._lib.mmiss_dbg_index_read_rows(idx._h, 1024, 0, None, None, None, None))
    s2 = _read(mods, idx, 50)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(s1, s2))
    after = idx.query(x[:5], 3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    assert idx.guard_stats()["queries"] == 15
    idx.close()

"""What test_index_rows_gpu.py relies on, established on the host (index_row_cases.py): every exact row meets the conditions under
which its stored bytes are known without the oracle, the integer rounding functions agree with numpy's float16 and the fp8 oracle on
the whole catalogue, the double-rounding witnesses are witnesses, and the comparator rejects every wrong result it exists for."""
from fractions import Fraction

import numpy as np
import pytest

import index_row_cases as rc
from oracle import fp8_oracle as fo
from oracle import retrieval_oracle as ro

D = 128


def _bits(a):
    return rc.to_codes(a)


def test_exact_rows_meet_their_conditions():
    rows = rc.exact_rows() + rc.pow2_rows(1024)
    assert sum(r.grid for r in rows) >= 40 and any(not r.grid for r in rows)
    for r in rows:
        assert all(rc.is_f32(v) for v in r.vals)
        S = sum(v * v for v in r.vals)
        if r.grid:
            n = [v * (1 << 24) for v in r.vals]
            assert all(k.denominator == 1 and abs(k) <= 1 << 24 for k in n)
            assert sum(int(k) ** 2 for k in n) == 1 << 48 and S == 1
        else:
            assert abs(S - 1) < Fraction(1, 1 << 48)
        assert r.norm == 1


def test_catalogue_holds_every_edge():
    """Every e4m3 code of 128 y up to 128 and every midpoint of two adjacent ones, the f16 subnormal edges, both signs."""
    vals = {v for r in rc.exact_rows() for v in r.vals}
    top = rc.rne(Fraction(128), rc.E4M3)
    assert top == 0x70
    for c in range(top):
        mid = (rc.value(c, rc.E4M3) + rc.value(c + 1, rc.E4M3)) / 256
        lo, hi = rc.f32_neighbours(mid)
        for v in (mid, lo, hi, rc.value(c + 1, rc.E4M3) / 128):
            assert v in vals and -v in vals, (c, v)
        # the midpoint goes to the even code, its neighbours to the nearer one
        even = c if c % 2 == 0 else c + 1
        assert rc.store_code(mid, "f8") == even and rc.store_code(lo, "f8") == c and rc.store_code(hi, "f8") == c + 1
    assert rc.store_code(rc.two(-17), "f8") == 0          # 128 y = 2^-10: between zero and the smallest code, to zero
    for v, code in ((rc.two(-25), 0), (rc.f32_neighbours(rc.two(-25))[1], 1), (3 * rc.two(-25), 2), (1023 * rc.two(-24), 0x3FF),
                    (rc.two(-14), 0x400), (2047 * rc.two(-25), 0x400), (rc.two(-24), 1)):
        assert v in vals and -v in vals
        assert rc.store_code(v, "f16") == code, (v, code)
    assert Fraction(1) in vals and Fraction(-1) in vals
    assert rc.store_code(Fraction(1), "f8") == 0x70 and rc.store_code(Fraction(1), "f16") == 0x3C00


@pytest.mark.parametrize("dim", [128, 1024])
def test_known_rows_against_the_oracle(dim):
    """normalize_rows(x, "f32") == x for every exact row (== the unscaled row for its scaled twins), and this module's bytes equal the
    oracle's for every known row and every dtype; the twins include float32 subnormal inputs, the f32 rows subnormal results."""
    k = rc.known_rows(dim)
    y = ro.normalize_rows(k.x, "f32")
    base, _ = rc.place(tuple(r for r in rc.exact_rows() + rc.pow2_rows(dim)), dim, seed=1000)
    assert np.array_equal(_bits(y[:base.shape[0]]), _bits(k.x[:base.shape[0]])) and np.array_equal(_bits(base), _bits(k.x[:base.shape[0]]))
    n0 = 0
    for s in rc.SCALES:
        rows = [r for r in rc.exact_rows() + rc.pow2_rows(dim) if (s > -120 or r.grid) and (s == 0 or r.kind != "f32-subnormal")]
        x0, _ = rc.place(tuple(rows), dim, seed=1000 + abs(s))
        assert np.array_equal(_bits(y[n0:n0 + len(rows)]), _bits(x0)), s
        n0 += len(rows)
    sub = (k.x != 0) & (np.abs(k.x) < np.float32(2.0 ** -126))
    assert sub.sum() >= 100, "the 2^-120 twins must hold float32 subnormal inputs"
    assert ((y != 0) & (np.abs(y) < np.float32(2.0 ** -126))).sum() >= 5
    for dt in ("f32", "f16", "f8"):
        ref = rc.reference_codes(k.x, k.norms, dt)
        orc, oinv = rc.oracle_store(k.x, dt)
        rc.check_rows(ref, orc, "f32" if dt == "f32" else dt)
        assert np.array_equal(ref, orc)    # (zero codes included: the oracle keeps the sign)
        if dt == "f8":
            assert np.array_equal(_bits(rc.f8_inv(ref)), _bits(oinv))


def test_rounding_functions_agree_with_numpy_and_the_fp8_oracle():
    vals = sorted({abs(v) for r in rc.exact_rows() for v in r.vals} | {Fraction(k, rc.WITNESS_DEN) for k in rc.witnesses()[:200]})
    f = np.array([float(rc.value(rc.rne(v, rc.F32), rc.F32)) for v in vals], dtype=np.float64)
    f32 = f.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), f)
    assert np.array_equal(f32.view(np.uint32), np.array([rc.rne(v, rc.F32) for v in vals], dtype=np.uint32))
    h = np.array([rc.rne(rc.frac(x), rc.F16) for x in f32], dtype=np.uint16)
    assert np.array_equal(h, f32.astype(np.float16).view(np.uint16))
    c = np.array([rc.rne(128 * rc.frac(x), rc.E4M3) for x in f32], dtype=np.uint8)
    assert np.array_equal(c, fo.e4m3_encode(f32 * np.float32(128.0)))
    assert np.array_equal(_bits(rc.f8_values(np.arange(256, dtype=np.uint8))[:127]), _bits((fo.e4m3_decode(np.arange(127, dtype=np.uint8)) / 128).astype(np.float32)))
    for code in range(0x7F):
        assert rc.rne(rc.value(code, rc.E4M3), rc.E4M3) == code
    for code in (0, 1, 0x3FF, 0x400, 0x7BFF):
        assert rc.rne(rc.value(code, rc.F16), rc.F16) == code


def test_witnesses_are_witnesses():
    w = rc.witnesses()
    assert len(w) >= 8
    rows = rc.witness_rows()
    held = 0
    for r in rows:
        assert sum(v * v for v in r.vals) == rc.WITNESS_DEN ** 2 and r.norm == rc.WITNESS_DEN
        assert all(v.denominator == 1 and abs(v) < 1 << 24 for v in r.vals)
        held += sum(1 for v in r.vals if abs(int(v)) in w)
    assert held >= 8
    x, norms = rc.place(rows, D, seed=77)
    assert np.array_equal(ro.canon_norm(x), np.full(len(rows), float(rc.WITNESS_DEN)))
    y32 = ro.normalize_rows(x, "f32")
    two_step = y32.astype(np.float16)
    one_step = (x.astype(np.float64) / float(rc.WITNESS_DEN)).astype(np.float16)    # (float64 -> float16: one rounding of RNE_f64(v))
    assert (two_step.view(np.uint16) != one_step.view(np.uint16)).sum() >= 8
    for k in w[:50]:
        v = Fraction(k, rc.WITNESS_DEN)
        assert rc.store_code(v, "f16") != rc.rne(v, rc.F16)
        assert abs(rc.store_code(v, "f16") - rc.rne(v, rc.F16)) == 1


def test_general_rows_reference_is_the_oracles():
    """oracle_store's fp8 codes and inverse norms are those of normalize_rows(x, "f8"), the rows without a direction included."""
    import warnings

    x = rc.general_rows(D)
    codes, inv = rc.oracle_store(x, "f8")
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        st = ro.normalize_rows(x, "f8")
    assert np.array_equal(_bits(rc.f8_values(codes)) << 1, _bits(np.asarray(st)) << 1)      # (a NaN's sign is not part of a value)
    assert np.array_equal(_bits(inv) << 1, _bits(st.inv) << 1)
    fin = ~np.isnan(np.asarray(st)).any(axis=1)
    assert fin.sum() == x.shape[0] - rc.NON_FINITE_ROWS and np.array_equal(_bits(rc.f8_values(codes))[fin], _bits(np.asarray(st))[fin])
    assert np.array_equal(_bits(inv)[fin], _bits(st.inv)[fin])
    # what the rows without a direction hold
    zero, nan, pinf, ninf = (x.shape[0] - 4 + i for i in range(4))
    assert ((codes[[zero, nan]] & 0x7F) == 0x7F).all() and np.isnan(inv[[zero, nan, pinf, ninf]]).all()
    for r in (pinf, ninf):
        assert ((codes[r] & 0x7F) == 0x7F).sum() == 1 and ((codes[r] & 0x7F) == 0).sum() == D - 1
        z = (codes[r] & 0x7F) == 0
        assert np.array_equal((codes[r] >> 7 == 1)[z], np.signbit(x[r])[z])      # (zeros of the component's own sign: nrm = +inf)


def test_pow2_file_rows_have_power_of_two_inverse_norms():
    codes, inv = rc.pow2_file_rows(1024)
    assert np.array_equal(_bits(rc.f8_inv(codes)), _bits(inv)) and set(inv.tolist()) == {1.0, 2.0, 4.0}
    x, norms = rc.place(rc.pow2_rows(1024), 1024, seed=3)
    assert np.array_equal(_bits(rc.f8_inv(rc.reference_codes(x, norms, "f8"))), _bits(np.ones(x.shape[0], np.float32)))


def test_guard_terms_restate_the_bound():
    fixed, cnorm = rc.guard_terms(128, "f32")
    assert cnorm == 0.0 and fixed == (4.0 * 128 * 2.0 ** -24 * (1 + 2.0 ** -9) ** 2) * 1.003 + 2.0 ** -21
    f16 = rc.guard_terms(1024, "f16")
    f8 = rc.guard_terms(1024, "f8")
    assert f8[0] > f16[0] > rc.guard_terms(1024, "f32")[0] and f8[1] == 1.07 * 1.003 and f16[1] == (1 + 2.0 ** -9) * 1.003


# ------------------------------------------------------------------------------------------------ the comparator rejects what it exists for
def _store(codes, inv, count, cap, tags=None):
    D_ = codes.shape[1]
    rows = np.zeros((cap, D_), dtype=codes.dtype)
    rows[:count] = codes
    iv = None
    if inv is not None:
        iv = np.zeros(cap, dtype=np.float32)
        iv[:count] = inv
    lab = np.zeros(cap, dtype=np.int64)
    lab[:count] = np.arange(10, 10 + count)
    tg = np.zeros(cap, dtype=np.uint64)
    tg[:count] = np.arange(1, count + 1, dtype=np.uint64) if tags is None else tags
    return rc.Store(rows, iv, lab, tg)


def _ref(st, count):
    return rc.Store(st.rows[:count], None if st.inv is None else st.inv[:count], st.labels[:count], st.tags[:count])


def _rejects(got, ref, dtype, count):
    with pytest.raises(AssertionError):
        rc.check_store(got, ref, dtype, count)


@pytest.fixture(scope="module")
def known():
    return rc.known_rows(D)


@pytest.mark.parametrize("dtype", ["f32", "f16", "f8"])
def test_comparator_accepts_the_reference(known, dtype):
    codes = rc.reference_codes(known.x, known.norms, dtype)
    inv = rc.f8_inv(codes) if dtype == "f8" else None
    st = _store(codes, inv, codes.shape[0], 1024)
    rc.check_store(st, _ref(st, codes.shape[0]), dtype, codes.shape[0])
    if dtype == "f8":   # the one exception: a zero of the other sign
        flipped = st.rows.copy()
        z = (flipped & 0x7F) == 0
        flipped[z] ^= 0x80
        rc.check_store(st._replace(rows=flipped), _ref(st, codes.shape[0]), dtype, codes.shape[0])
    else:
        flipped = st.rows.copy()
        z = np.argwhere((flipped[:codes.shape[0]] << 1) == 0)[0]
        flipped[tuple(z)] ^= flipped.dtype.type(1 << (8 * flipped.dtype.itemsize - 1))
        _rejects(st._replace(rows=flipped), _ref(st, codes.shape[0]), dtype, codes.shape[0])


@pytest.mark.parametrize("dtype,wrong", [("f8", {"tie": "away"}), ("f16", {"tie": "away"}), ("f32", {"flush_in": True}),
                                         ("f16", {"flush_in": True}), ("f8", {"flush_in": True}), ("f32", {"flush_out": True}),
                                         ("f16", {"flush_out": True}), ("f8", {"flush_out": True}), ("f16", {"single": True})])
def test_comparator_rejects_wrong_roundings(known, dtype, wrong):
    """Ties rounded half away, subnormal inputs flushed, subnormal outputs flushed, a single rounding to f16: each changes bytes of the
    catalogue, and the comparator sees it. (An fp8 zero of the other sign does not count: the wrong bytes differ elsewhere too.)"""
    n = known.x.shape[0]
    good = rc.reference_codes(known.x, known.norms, dtype)
    bad = rc.reference_codes(known.x, known.norms, dtype, **wrong)
    st = _store(good, rc.f8_inv(good) if dtype == "f8" else None, n, 1024)
    with pytest.raises(AssertionError):
        rc.check_rows(bad, good, dtype)
    _rejects(st._replace(rows=_store(bad, None, n, 1024).rows), _ref(st, n), dtype, n)
    if "single" in wrong:
        assert (bad != good).sum() >= 8


def test_comparator_takes_either_encoding_of_the_fp8_nan_and_nothing_else():
    x = rc.general_rows(D)
    codes, inv = rc.oracle_store(x, "f8")
    nan = (codes & 0x7F) == 0x7F
    assert nan.sum() == 2 * D + 2
    other = np.where(nan, codes ^ 0x80, codes).astype(np.uint8)
    rc.check_rows(other, codes, "f8")
    for wrong in (np.where(nan, 0x7E, codes), np.where(nan, 0, codes)):
        with pytest.raises(AssertionError):
            rc.check_rows(wrong.astype(np.uint8), codes, "f8")
    number = np.argwhere(~nan & ((codes & 0x7F) != 0))[0]
    wrong = codes.copy()
    wrong[tuple(number)] = 0x7F
    with pytest.raises(AssertionError):
        rc.check_rows(wrong, codes, "f8")
    # what is computed from the codes (inv, get): a NaN for a NaN, whatever its sign; never a NaN for a number or the reverse
    flip = inv.copy().view(np.uint32)
    flip[np.isnan(inv)] ^= 0x80000000
    rc.check_rows(flip.view(np.float32), inv, "f32", f8_nan=True)
    with pytest.raises(AssertionError):
        rc.check_rows(flip.view(np.float32), inv, "f32")
    for wrong in (np.where(np.isnan(inv), np.float32(1), inv), np.where(np.arange(inv.size) == 0, np.float32(np.nan), inv)):
        with pytest.raises(AssertionError):
            rc.check_rows(wrong.astype(np.float32), inv, "f32", f8_nan=True)
    # f32 / f16: a NaN of other bits is a difference
    c32, _ = rc.oracle_store(x, "f32")
    wrong = c32.copy()
    wrong[-4, 0] ^= 0x80000000
    with pytest.raises(AssertionError):
        rc.check_rows(wrong, c32, "f32")


def _general_store(n, dtype, cap, seed=3):
    x = rc.general_rows(D, n=n, seed=seed)[:n]
    codes, inv = rc.oracle_store(x, dtype)
    return _store(codes, inv, n, cap)


def test_comparator_rejects_misplaced_inverse_norms():
    n = 300
    st = _general_store(n, "f8", 1024)
    ref = _ref(st, n)
    rc.check_store(st, ref, "f8", n)
    _rejects(st._replace(inv=np.roll(st.inv, 1)), ref, "f8", n)                     # shifted by one row
    inv = st.inv.copy()
    inv[n] = 1.0
    _rejects(st._replace(inv=inv), ref, "f8", n)                                     # not zero behind count
    # two chunks of an add (rows [3, 3 + c) and [3 + c, n)): the second chunk's inv written at the first chunk's offset
    c = 256
    inv = st.inv.copy()
    inv[3:3 + (n - 3 - c)] = st.inv[3 + c:n]
    inv[3 + c:n] = 0
    _rejects(st._replace(inv=inv), ref, "f8", n)
    tags = st.tags.copy()
    tags[n + 5] = 1
    _rejects(st._replace(tags=tags), ref, "f8", n)
    lab = st.labels.copy()
    lab[7] += 1
    _rejects(st._replace(labels=lab), ref, "f8", n)


@pytest.mark.parametrize("dtype", ["f16", "f8"])
def test_comparator_rejects_wrong_compactions_and_short_gathers(dtype):
    n = 64
    st = _general_store(n, dtype, 1024)
    keep = np.setdiff1d(np.arange(n), [0, 20, 21, 22, n - 1])
    ref = rc.Store(st.rows[keep], None if st.inv is None else st.inv[keep], st.labels[keep], st.tags[keep])

    def compacted(order):
        out = _store(st.rows[order], None if st.inv is None else st.inv[order], len(order), 1024, tags=st.tags[order])
        return out._replace(labels=np.concatenate([st.labels[order], np.zeros(1024 - len(order), np.int64)]))

    rc.check_store(compacted(keep), ref, dtype, keep.size)
    dropped = np.concatenate([keep[:30], keep[31:], keep[-1:]])       # one row dropped, the tail moves up
    repeated = np.concatenate([keep[:31], keep[30:-1]])               # one row twice
    for order in (dropped, repeated):
        got = compacted(keep)._replace(rows=compacted(order).rows)
        _rejects(got, ref, dtype, keep.size)
        if dtype == "f8":
            _rejects(compacted(keep)._replace(inv=compacted(order).inv), ref, dtype, keep.size)
    # a gather whose grid-stride loop stops after its first 4096 x 256 elements (here: after the first 40 rows' worth)
    for fill in (0, 0xFF):
        short = compacted(keep).rows.copy()
        short.reshape(-1)[40 * D + 17:keep.size * D] = fill
        _rejects(compacted(keep)._replace(rows=short), ref, dtype, keep.size)
    g = rc.get_reference(ref.rows, ref.inv, dtype)
    short = g.copy()
    short.reshape(-1)[40 * D + 17:] = 0
    with pytest.raises(AssertionError):
        rc.check_rows(short, g, "f32")


def test_eps_check_rejects_a_bound_that_is_too_small_or_too_large():
    e = np.array([1e-4, 2.5e-4, np.nan])
    finite = np.array([True, True, False])
    up = np.nextafter(e[:2].astype(np.float32), np.float32(np.inf))
    up = np.where(e[:2].astype(np.float32).astype(np.float64) >= e[:2], e[:2].astype(np.float32), up)
    rc.check_eps(np.concatenate([up, [np.float32(np.inf)]]), e, finite)
    for bad in (np.concatenate([np.nextafter(up, np.float32(0))[:1], up[1:], [np.inf]]),
                np.concatenate([np.nextafter(np.nextafter(up, np.float32(1)), np.float32(1))[:1], up[1:], [np.inf]]),
                np.concatenate([up, [1.0]]), np.concatenate([[np.inf], up[1:], [np.inf]])):
        with pytest.raises(AssertionError):
            rc.check_eps(bad.astype(np.float32), e, finite)

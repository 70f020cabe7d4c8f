"""Inputs of the flat index whose STORED BYTES are known without the oracle, the reference of every other row, and the comparator of
tests/test_index_rows_gpu.py (tests/test_index_row_cases_cpu.py establishes all of it on the host).

The contract of the row store (csrc/retrieval_kernels.h normalize_rows_kernel, oracle/retrieval_oracle.py normalize_rows):
    nrm = sqrt(canonical float64 sum of squares)        y64 = RNE_f64(x / nrm)        y32 = RNE_f32(y64)
    f32 rows: y32        f16 rows: RNE_f16(y32)        fp8 rows: the e4m3 code of RNE_e4m3(128 * y32)
Every rounding is to nearest, ties to even, subnormals kept (inputs, y32, f16 and e4m3 results alike); a zero keeps its sign.

Exact rows. Components x_i = n_i 2^-24 with integers |n_i| <= 2^24 and sum n_i^2 = 2^48: every square and every partial sum is an
integer below 2^53 (in units of 2^-48), so the sum of squares is exactly 1 in float64 IN ANY ORDER, nrm = 1 and y32 = x bit for bit;
the canonical summation order does not enter. Edge values that are not on the 2^-24 grid (a midpoint plus or minus one float32
ulp) ride in rows whose exact sum of squares is within 2^-48 of 1: the float64 sum, in any order, is then within 2^-45 of 1, nrm
within 2^-46, and RNE_f32(x / nrm) = x for every float32 x (a relative change of 2^-46 against half an ulp of 2^-25 at least).
What the storage rounding makes of y32 = x comes from `rne` below: integer / Fraction arithmetic with the format's parameters, no
numpy conversion and no table of the fp8 oracle. A row times 2^s is the same row (nrm = 2^s, every quotient the same rational) as
long as no product leaves float32's grid; at 2^-120 the small components are float32 SUBNORMALS on input and must be kept.

Witness rows. Integers n_i < 2^24 with sum n_i^2 = c^2 for the odd c = 3 * 2^23 + 1 (c^2 < 2^53: the sum is exact in any order,
nrm = c exactly) and x_i / nrm = n_i / c, a known rational that is no binary fraction. They carry the components at which
RNE_f16(RNE_f32(v)) != RNE_f16(v). (A norm of the form 3 * 2^k cannot have any: v = n / (3 * 2^k) and an f16 midpoint m / 2^t differ by
a multiple of 1 / (3 * 2^max(t, k)), never within half a float32 ulp of the midpoint without being equal; an odd c of 25 bits can.)
"""
from __future__ import annotations

import functools
from fractions import Fraction
from math import isqrt
from typing import NamedTuple

import numpy as np

HALF = Fraction(1, 2)


class Fmt(NamedTuple):
    name: str
    ebits: int
    mbits: int
    bias: int
    max_finite: int   # largest finite magnitude code


F64 = Fmt("f64", 11, 52, 1023, 0x7FEFFFFFFFFFFFFF)
F32 = Fmt("f32", 8, 23, 127, 0x7F7FFFFF)
F16 = Fmt("f16", 5, 10, 15, 0x7BFF)
E4M3 = Fmt("e4m3", 4, 3, 7, 0x7E)   # OCP e4m3fn: no infinity, 0x7F is the NaN
STORE_FMT = {"f32": F32, "f16": F16, "f8": E4M3}
CODE_DTYPE = {"f32": np.uint32, "f16": np.uint16, "f8": np.uint8}
F8_SCALE = 128


def two(e: int) -> Fraction:
    return Fraction(2) ** e


def rne(a: Fraction, fmt: Fmt, tie: str = "even", flush: bool = False) -> int:
    """Magnitude code (exponent and mantissa fields, no sign) of a >= 0 rounded to nearest in `fmt`. tie: "even" (the contract) or
    "away" (a wrong rule, for the comparator's own test); flush: a subnormal result becomes zero (wrong, likewise)."""
    assert a >= 0
    if a == 0:
        return 0
    emin = 1 - fmt.bias
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if two(e) > a:
        e -= 1
    assert two(e) <= a < two(e + 1)
    e = max(e, emin)
    q = a / two(e - fmt.mbits)           # in units of the last place: [2^mbits, 2^(mbits+1)) for a normal number, below for a subnormal
    n = q.numerator // q.denominator
    r = q - n
    if r > HALF or (r == HALF and (tie == "away" or (n & 1))):
        n += 1
    code = ((e - emin) << fmt.mbits) + n  # (a carry out of the mantissa lands in the exponent field by itself)
    assert code <= fmt.max_finite, (a, fmt.name)
    if flush and code < (1 << fmt.mbits):
        code = 0
    return code


def value(code: int, fmt: Fmt) -> Fraction:
    """The magnitude a magnitude code stands for."""
    code = int(code)
    assert 0 <= code <= fmt.max_finite
    exp, man = code >> fmt.mbits, code & ((1 << fmt.mbits) - 1)
    emin = 1 - fmt.bias
    if exp == 0:
        return man * two(emin - fmt.mbits)
    return ((1 << fmt.mbits) + man) * two(exp - 1 + emin - fmt.mbits)


def frac(x) -> Fraction:
    """A float's exact value."""
    return Fraction(float(x))


def is_f32(fr: Fraction) -> bool:
    return fr == 0 or value(rne(abs(fr), F32), F32) == abs(fr)


def f32_neighbours(fr: Fraction):
    """(the float32 below, the float32 above) a positive float32 value."""
    c = rne(fr, F32)
    assert value(c, F32) == fr and c > 0
    return value(c - 1, F32), value(c + 1, F32)


# ------------------------------------------------------------------------------------------------ the storage rounding of one component
@functools.lru_cache(maxsize=None)
def store_code(a: Fraction, dtype: str, tie: str = "even", flush_out: bool = False, single: bool = False) -> int:
    """Magnitude code stored for the exact quotient a = |x| / nrm. tie / flush_out / single: wrong rules (ties away from zero in the
    storage rounding, subnormal results flushed, f16 rounded once from the exact quotient) for the comparator's own test."""
    y64 = value(rne(a, F64), F64)
    c32 = rne(y64, F32, flush=flush_out)
    if dtype == "f32":
        return c32
    y32 = value(c32, F32)
    if dtype == "f16":
        return rne(a if single else y32, F16, tie, flush_out)
    return rne(F8_SCALE * y32, E4M3, tie, flush_out)


def reference_codes(x: np.ndarray, norms, dtype: str, flush_in: bool = False, **wrong) -> np.ndarray:
    """Stored codes [n, D] (uint32 / uint16 / uint8, sign included) of float32 rows x whose norms are known exactly (`norms`: one
    Fraction per row). flush_in: float32 subnormal inputs read as zero (wrong; for the comparator's own test)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    fmt = STORE_FMT[dtype]
    sign_shift = fmt.ebits + fmt.mbits
    out = (np.signbit(x).astype(np.uint64) << np.uint64(sign_shift))
    bits = x.view(np.uint32)
    rr, dd = np.nonzero(bits & np.uint32(0x7FFFFFFF))
    for r, d in zip(rr.tolist(), dd.tolist()):
        a = abs(frac(x[r, d]))
        if flush_in and a < two(-126):
            continue
        out[r, d] |= np.uint64(store_code(a / norms[r], dtype, **wrong))
    return out.astype(CODE_DTYPE[dtype])


E4M3_VALUES = np.array([float(value(c, E4M3) / F8_SCALE) if c <= E4M3.max_finite else np.nan for c in range(128)], dtype=np.float32)


def f8_values(codes: np.ndarray) -> np.ndarray:
    """float32 values decode(code) / 128 of e4m3 codes (this module's own table)."""
    codes = np.asarray(codes, dtype=np.uint8)
    v = E4M3_VALUES[codes & 0x7F]
    return np.where(codes & 0x80, -v, v).astype(np.float32)


def f8_inv(codes: np.ndarray) -> np.ndarray:
    """float32 [n]: the inverse of the canonical norm of the values the codes stand for (f8_row_inv_kernel)."""
    from oracle import retrieval_oracle as ro

    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / ro.canon_norm(f8_values(codes))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ edge catalogue
def e4m3_edges():
    """y > 0 at which 128 y is an e4m3 code (every one up to 128, subnormal codes included), the midpoint of two adjacent codes
    (2^-10, between zero and the smallest code, included) and each midpoint's two float32 neighbours."""
    out = []
    top = rne(Fraction(F8_SCALE), E4M3)          # the code of 128 (y = 1)
    for c in range(1, top):                      # (y = 1 itself: the one-hot row)
        out.append(value(c, E4M3) / F8_SCALE)
    for c in range(0, top):
        mid = (value(c, E4M3) + value(c + 1, E4M3)) / 2 / F8_SCALE
        out += [mid, *f32_neighbours(mid)]
    return out


def f16_edges():
    """y > 0 at f16 midpoints of the normal range (low, middle and high mantissas of every binade below 1, even and odd lower
    neighbours) with their float32 neighbours, and the subnormal edges: 2^-25 (to zero) and the float32 above it, 3 * 2^-25, more
    subnormal midpoints, the largest subnormal, the smallest normal number and the midpoint between the two."""
    out = []
    for e in range(-14, 0):
        for j in (0, 1, 2, 511, 512, 1022, 1023):
            mid = (2 * (1024 + j) + 1) * two(e - 11)
            out += [mid, *f32_neighbours(mid)]
    sub = [two(-25), f32_neighbours(two(-25))[1], f32_neighbours(two(-25))[0], 3 * two(-25), 5 * two(-25), 7 * two(-25),
           1021 * two(-25), 1023 * two(-25), 2045 * two(-25), 2047 * two(-25), *f32_neighbours(2047 * two(-25)),
           1023 * two(-24), 1022 * two(-24), two(-14), two(-24), two(-23)]
    return out + sub


class Row(NamedTuple):
    vals: tuple      # float32-exact Fractions, signed
    negz: int        # number of -0.0 components behind the values (the rest of the row is +0.0)
    norm: Fraction   # the row's norm as the kernel computes it (exact)
    grid: bool       # every component n 2^-24, sum n^2 = 2^48 exactly
    kind: str


def ballast(R: int, cap: int = (1 << 24) - 1):
    """Integers whose squares sum to R, greedily the largest first (the last ones are 1s)."""
    out = []
    while R > 0:
        k = min(isqrt(R), cap)
        out.append(k)
        R -= k * k
    return out


def _close_row(edges, kind):
    S = sum(e * e for e in edges)
    assert S <= 1
    grid = all((e * (1 << 24)).denominator == 1 for e in edges)
    R = (1 - S) * (1 << 48)
    R = R.numerator // R.denominator
    bal = [Fraction(k if i % 2 == 0 else -k, 1 << 24) for i, k in enumerate(ballast(R))]
    vals = tuple(edges) + tuple(bal)
    assert len(vals) <= 126, len(vals)
    assert abs(sum(v * v for v in vals) - 1) < two(-48) and (not grid or sum(v * v for v in vals) == 1)
    return Row(vals, 2, Fraction(1), grid, kind)


@functools.lru_cache(maxsize=None)
def exact_rows():
    """The edge catalogue packed into unit rows: edges first (both signs), then the ballast that completes the sum of squares."""
    rows = []
    for kind, edges in (("e4m3", e4m3_edges()), ("f16", f16_edges())):
        signed = []
        for i, e in enumerate(edges):
            assert is_f32(e)
            signed += [e, -e] if i % 2 == 0 else [-e, e]
        cur, S = [], Fraction(0)
        for e in signed:
            if cur and (S + e * e > 1 or len(cur) >= 96):
                rows.append(_close_row(cur, kind))
                cur, S = [], Fraction(0)
            cur.append(e)
            S += e * e
        rows.append(_close_row(cur, kind))
    rows.append(Row((Fraction(1),), 3, Fraction(1), True, "one-hot"))
    rows.append(Row((Fraction(-1),), 0, Fraction(1), True, "one-hot"))
    # components that are float32 subnormals AFTER normalisation (f32 rows keep them; f16 / fp8 rows hold signed zeros)
    tiny = (Fraction(1), two(-130), -two(-149), 3 * two(-140), -(two(-126) - two(-149)), two(-126), -two(-127))
    rows.append(Row(tiny, 1, Fraction(1), False, "f32-subnormal"))
    return tuple(rows)


def equal_row(m: int, v: Fraction):
    """A unit row of m components v (m v^2 = 1)."""
    assert m * v * v == 1
    return Row((v,) * m, 0, Fraction(1), (v * (1 << 24)).denominator == 1, "pow2")


@functools.lru_cache(maxsize=None)
def pow2_rows(D: int):
    """Rows of m equal components 1 / sqrt(m) whose fp8 codes are exact: the values' norm is exactly 1 and inv = 1.0. (The same codes
    with a norm of 2^-j, inv = 2^j, are reached through a crafted file: pow2_file_rows.)"""
    rows = [equal_row(4, Fraction(1, 2)), equal_row(16, Fraction(-1, 4)), equal_row(1, Fraction(1)), equal_row(64, Fraction(1, 8))]
    if D >= 256:
        rows.append(equal_row(256, Fraction(1, 16)))
    if D >= 1024:
        rows.append(equal_row(1024, Fraction(-1, 32)))
    return tuple(rows)


def pow2_file_rows(D: int):
    """(codes uint8 [n, D], inv float32 [n]) for a crafted fp8 index file: m components of value v whose norm is 2^-j exactly, so the
    inverse norm load recomputes is the power of two 2^j: (4, 1/4) -> 2, (16, 1/16) -> 4, (1, 1/2) -> 2, (4, 1/2) -> 1,
    (16, 1/4) -> 1, (1, 1) -> 1, and with D >= 256 (256, 1/32) -> 2 and (256, 1/16) -> 1, with D >= 1024 (1024, 1/64) -> 2 and
    (1024, 1/32) -> 1."""
    spec = [(4, Fraction(1, 4), 2.0), (16, Fraction(1, 16), 4.0), (1, Fraction(1, 2), 2.0), (4, Fraction(1, 2), 1.0),
            (16, Fraction(1, 4), 1.0), (1, Fraction(1), 1.0)]
    if D >= 256:
        spec += [(256, Fraction(1, 32), 2.0), (256, Fraction(1, 16), 1.0)]
    if D >= 1024:
        spec += [(1024, Fraction(1, 64), 2.0), (1024, Fraction(1, 32), 1.0)]
    codes = np.zeros((len(spec), D), dtype=np.uint8)
    for i, (m, v, _) in enumerate(spec):
        c = rne(F8_SCALE * v, E4M3)
        assert value(c, E4M3) == F8_SCALE * v
        pos = np.random.default_rng(900 + i).permutation(D)[:m]
        codes[i, pos] = c | (0x80 if i % 2 else 0)
    return codes, np.array([s[2] for s in spec], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ double-rounding witnesses (f16)
WITNESS_DEN = (3 << 23) + 1   # nrm of a witness row (odd)


@functools.lru_cache(maxsize=None)
def witnesses():
    """Integers n < 2^24 (n / WITNESS_DEN in [1/4, 2/3)) with RNE_f16(RNE_f32(RNE_f64(v))) != RNE_f16(v) for v = n / WITNESS_DEN:
    RNE_f32 lands exactly on an f16 midpoint that v itself is not, and ties-to-even then goes the other way."""
    n = np.arange(WITNESS_DEN // 4, 1 << 24, dtype=np.int64)
    y32 = (n.astype(np.float64) / float(WITNESS_DEN)).astype(np.float32)
    cand = n[(y32.view(np.uint32) & 0x1FFF) == 0x1000]      # the 13 bits below an f16 mantissa: exactly one half
    out = []
    for k in cand.tolist():
        v = Fraction(k, WITNESS_DEN)
        if store_code(v, "f16") != rne(v, F16):
            out.append(k)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def witness_rows(count: int = 24):
    """Rows of integers with sum of squares WITNESS_DEN^2 that hold `count` witnesses, spread over both binades and both signs."""
    w = witnesses()
    pick = [w[i * (len(w) - 1) // (count - 1)] for i in range(count)]
    assert len(set(pick)) == count
    total = WITNESS_DEN * WITNESS_DEN
    rows, cur, S = [], [], 0
    for i, k in enumerate(pick + [None]):
        if k is None or S + k * k > total:
            bal = ballast(total - S)
            vals = tuple(Fraction(v) for v in cur) + tuple(Fraction(b if j % 2 else -b) for j, b in enumerate(bal))
            assert sum(v * v for v in vals) == total and all(abs(v) < (1 << 24) for v in vals)
            rows.append(Row(vals, 1, Fraction(WITNESS_DEN), False, "witness"))
            cur, S = [], 0
        if k is not None:
            cur.append(k if i % 2 == 0 else -k)
            S += k * k
    return tuple(rows)


# ------------------------------------------------------------------------------------------------ rows as float32 matrices
def place(rows, D: int, seed: int, scale: int = 0):
    """float32 [n, D] of `rows` times 2^scale: a row's values and its -0.0 components at seeded pseudo-random positions (every lane
    and every 64-column block gets its share), +0.0 elsewhere; with the rows' exact norms."""
    x = np.zeros((len(rows), D), dtype=np.float32)
    rng = np.random.default_rng(seed)
    norms = []
    for r, row in enumerate(rows):
        m = len(row.vals)
        assert m + row.negz <= D
        pos = rng.permutation(D)[:m + row.negz]
        vals = [v * two(scale) for v in row.vals]
        assert all(is_f32(v) for v in vals), (row.kind, scale)
        x[r, pos[:m]] = np.array([float(v) for v in vals], dtype=np.float64).astype(np.float32)
        x[r, pos[m:]] = np.float32(-0.0)
        norms.append(row.norm * two(scale))
    return x, norms


SCALES = (0, -100, 90, -120)   # (-120: grid rows only; their small components become float32 subnormals)


class Known(NamedTuple):
    x: np.ndarray     # float32 [n, D]
    norms: list       # exact norm per row
    kinds: list


@functools.lru_cache(maxsize=None)
def known_rows(D: int) -> Known:
    """Every row whose stored bytes this module derives itself: the exact rows and their scaled twins, the power-of-two rows and the
    witness rows."""
    xs, norms, kinds = [], [], []
    for s in SCALES:
        # (the rows with components that are float32 subnormals already have no smaller twin)
        rows = tuple(r for r in exact_rows() + pow2_rows(D) if (s > -120 or r.grid) and (s == 0 or r.kind != "f32-subnormal"))
        x, nr = place(rows, D, seed=1000 + abs(s), scale=s)
        xs.append(x); norms += nr; kinds += [f"{r.kind}*2^{s}" for r in rows]
    x, nr = place(witness_rows(), D, seed=77)
    xs.append(x); norms += nr; kinds += ["witness"] * len(nr)
    return Known(np.concatenate(xs), norms, kinds)


def general_rows(D: int, n: int = 40, seed: int = 5) -> np.ndarray:
    """Rows compared with the oracle in every byte: Gaussian rows at log-uniform scales from 1e-30 to 1e30, rows with one dominant
    component and the others 2^-20 below it, and the rows without a direction (zero, NaN, +inf, -inf: NON_FINITE_ROWS)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, D)).astype(np.float32)
    g *= (10.0 ** rng.uniform(-30, 30, size=(n, 1))).astype(np.float32)
    mixed = (rng.standard_normal((8, D)) * 2.0 ** -20).astype(np.float32)
    mixed[np.arange(8), rng.integers(0, D, size=8)] = np.array([1, -1, 3, -7, 1e10, -1e-10, 0.37, -5], dtype=np.float32)
    bad = rng.standard_normal((4, D)).astype(np.float32)
    bad[0] = 0.0
    bad[1, 3] = np.nan
    bad[2, 9] = np.inf
    bad[3, 9] = -np.inf
    return np.concatenate([g, mixed, bad])


NON_FINITE_ROWS = 4   # the last rows of general_rows


def writer_corpus(D: int):
    """(x float32 [N, D], known): the rows of the writer tests — known_rows(D) first, general_rows(D) behind them."""
    k = known_rows(D)
    return np.concatenate([k.x, general_rows(D)]), k


def to_codes(a: np.ndarray) -> np.ndarray:
    """float32 / float16 / uint8 array -> its bits as uint32 / uint16 / uint8."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def oracle_store(x: np.ndarray, dtype: str):
    """(codes, inv or None) of rows x as oracle/retrieval_oracle.py stores them. What the rows without a direction hold follows from
    the same arithmetic: a zero row is 0/0 in every component — every f32 / f16 element a NaN, every fp8 code the format's NaN
    (0x7F or 0xFF: one NaN, two encodings; check_rows takes either), inv = NaN; a row with a NaN likewise; a row with an infinity has nrm = inf, so every finite component
    becomes a zero of its own sign (f32, f16 and fp8 alike) and the infinite one inf/inf = NaN, and its inv is NaN as well."""
    import warnings

    from oracle import fp8_oracle as fo
    from oracle import retrieval_oracle as ro

    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        if dtype == "f8":
            # normalize_rows(x, "f8") step by step (the same calls; test_index_row_cases_cpu.py holds the two to each other), to have
            # the codes themselves and not only the values they stand for
            codes = fo.e4m3_encode(ro.normalize_rows(x, "f32") * np.float32(128.0))
            return codes, f8_inv(codes)
        return to_codes(ro.normalize_rows(x, dtype)), None


@functools.lru_cache(maxsize=None)
def writer_reference(D: int, dtype: str):
    """(codes [N, D], inv float32 [N] or None) of writer_corpus(D): this module's own bytes for the known rows, the oracle's for the
    general ones."""
    x, k = writer_corpus(D)
    nk = k.x.shape[0]
    known = reference_codes(k.x, k.norms, dtype)
    gen, ginv = oracle_store(x[nk:], dtype)
    codes = np.concatenate([known, gen])
    inv = np.concatenate([f8_inv(known), ginv]) if dtype == "f8" else None
    return codes, inv


def get_reference(codes: np.ndarray, inv, dtype: str) -> np.ndarray:
    """uint32 bits of what mmiss_index_get returns for stored codes: the stored values widened (f32, f16), float32(values * inv)
    (fp8: one float32 multiply)."""
    with np.errstate(all="ignore"):
        if dtype == "f32":
            return codes.view(np.uint32)
        if dtype == "f16":
            return to_codes(codes.view(np.float16).astype(np.float32))
        return to_codes((f8_values(codes) * inv[:, None]).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the comparator
class Store(NamedTuple):
    """The four per-row buffers of an index over [0, capacity): rows as codes, inv (fp8 rows) as float32, labels, tags."""
    rows: np.ndarray
    inv: object
    labels: np.ndarray
    tags: np.ndarray


def check_rows(got: np.ndarray, ref: np.ndarray, dtype: str, what: str = "rows", f8_nan: bool = False) -> None:
    """Every element of `got` equals `ref` as bits. fp8 rows: where the reference code is a zero of either sign, either zero code
    passes (the one exception among numbers), and where it is the format's NaN — e4m3 has ONE NaN with two encodings, 0x7F and 0xFF,
    and no operation tells them apart: rows without a direction only — either encoding of it passes. (f32 / f16 NaNs are compared
    as bits like every other element.) f8_nan: `got` / `ref` are float32 results computed FROM fp8 codes (inv, what get returns): a
    NaN among them descends from a NaN code, takes its sign from the encoding that happened to be written, and is compared as "a NaN"."""
    got, ref = to_codes(got), to_codes(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = got != ref
    if f8_nan:
        assert got.dtype == np.uint32
        bad &= ~(((ref & 0x7FFFFFFF) > 0x7F800000) & ((got & 0x7FFFFFFF) > 0x7F800000))
    if dtype == "f8":
        bad &= ~(((ref & 0x7F) == 0) & ((got & 0x7F) == 0))
        bad &= ~(((ref & 0x7F) == 0x7F) & ((got & 0x7F) == 0x7F))
    if bad.any():
        idx = np.argwhere(bad)
        first = tuple(idx[0])
        raise AssertionError(f"{what}: {idx.shape[0]} of {got.size} elements differ, first at {first}: got {int(got[first]):#x}, "
                             f"expected {int(ref[first]):#x}; rows {sorted(set(idx[:, 0].tolist()))[:8]}")


def check_store(got: Store, ref: Store, dtype: str, count: int) -> None:
    """`got`, read over the whole capacity, holds `ref`'s `count` rows: every element of every row, inv bit for bit, device labels
    and tags; behind count inv and tags are zero."""
    cap = got.tags.shape[0]
    assert 0 <= count <= cap and got.rows.shape[0] == cap and ref.rows.shape[0] == count
    check_rows(got.rows[:count], ref.rows, dtype)
    assert np.array_equal(got.labels[:count], ref.labels), "device labels differ from the host labels"
    assert np.array_equal(got.tags[:count], ref.tags), "device tags differ"
    assert not got.tags[count:].any(), "tags behind count are not zero"
    if dtype == "f8":
        check_rows(got.inv[:count], ref.inv, "f32", what="inv", f8_nan=True)
        assert not to_codes(got.inv)[count:].any(), "inv behind count is not zero"


# ------------------------------------------------------------------------------------------------ query preparation
def guard_terms(D: int, dtype: str):
    """(fixed, cnorm) of the exactness guard's bound in float64, operation for operation as guard_terms of csrc/api_index.hip
    (DESIGN.md section 4): eps_q = (fixed + cnorm * |qs - qn|_2) * 1.0001, rounded up to float32."""
    cn = 1.07 if dtype == "f8" else 1.0 + 2.0 ** -9
    e = 4.0 * float(D) * 2.0 ** -24 * cn * (1.0 + 2.0 ** -9)
    if dtype != "f32":
        e += float(D) * 2.0 ** -25 * cn
    if dtype == "f8":
        e += 2.0 ** -23
    return e * 1.003 + 2.0 ** -21, (0.0 if dtype == "f32" else cn * 1.003)


def eps_reference(qn_codes: np.ndarray, qs_codes: np.ndarray, D: int, dtype: str) -> np.ndarray:
    """float64 [Q]: e of prep_queries_kernel from the reference qn (uint32 bits) and qs (bits in the query dtype): the canonical
    float64 sum of (float32(qs) - qn)^2, its square root, then (fixed + cnorm * that) * 1.0001. NaN where the query has no direction."""
    from oracle import retrieval_oracle as ro

    fixed, cnorm = guard_terms(D, dtype)
    with np.errstate(all="ignore"):
        qn = qn_codes.view(np.float32).astype(np.float64)
        qs = (qs_codes.view(np.float32) if dtype == "f32" else qs_codes.view(np.float16).astype(np.float32)).astype(np.float64)
        d = qs - qn
        dq = ro.canon_sum(d * d)
        return (fixed + cnorm * np.sqrt(dq)) * 1.0001


def check_eps(eps: np.ndarray, e: np.ndarray, finite: np.ndarray) -> None:
    """eps_q (float32 from the device) against e (float64): never below e, at most one float32 above RNE_f32(e); +inf exactly where
    the query has no direction."""
    eps = np.asarray(eps, dtype=np.float32)
    assert np.array_equal(np.isposinf(eps), ~finite), "eps_q must be +inf exactly for the zero / NaN / inf queries"
    assert np.isfinite(eps[finite]).all() and np.isfinite(e[finite]).all()
    g, w = eps[finite], e[finite]
    assert (g.astype(np.float64) >= w).all(), "eps_q below the bound"
    assert (g <= np.nextafter(w.astype(np.float32), np.float32(np.inf))).all(), "eps_q more than one float32 above the bound"

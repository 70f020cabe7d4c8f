"""What test_gemm_exact_gpu.py relies on, established on the host (gemm_exact_cases.py): every case it builds meets the
conditions under which the float64 reference IS the only correct output — (a) exact fp32 accumulation, (b) exact statistics,
(c) / (d) enough rounding ties and inexact elements, the cap on undecided elements of the inexact epilogues — and the comparison
rejects each wrong result it is there to catch, simulated here on the reference."""
import pytest
import torch

import gemm_exact_cases as gx


def _whats(M, N, K, kind, patch):
    if kind == "stats":
        return ("resid", "resid16")
    if kind == "fold":
        return ("fold", "fold_qgelu")
    return ("f32", "bf16", "qgelu", "resid") + (("patch",) if patch is not None else ())


@pytest.mark.parametrize("spec", gx.tile_cases(), ids=lambda s: "%dx%dx%d-%s" % s[:4])
def test_conditions_hold_for_every_gpu_case(spec):
    M, N, K, kind, patch = spec
    c = gx.case(M, N, K, kind, patch)
    for what in _whats(*spec):
        fig = c.check(what)
        print(spec[:4], what, {k: round(v, 4) for k, v in fig.items()})
    assert c.A.to(torch.bfloat16).double().equal(c.A) and c.W.to(torch.bfloat16).double().equal(c.W)
    if kind == "stats":
        assert c.x0.to(torch.bfloat16).double().equal(c.x0)          # the bf16 residual stream holds it


@pytest.mark.parametrize("B,S,P,d", gx.PIX_SHAPES)
def test_pixel_cases_are_exact(B, S, P, d):
    px, W, pos, rows = gx.pixel_case(B, S, P, d)
    assert px.to(torch.bfloat16).double().equal(px) and (px != 0).all()
    assert rows.float().double().equal(rows)


def test_bf16_round_is_the_one_correct_rounding():
    """against torch's own f32 -> bf16 (nearest even) on f32 inputs, ties and binade edges included"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1 << 16, generator=g) * 8
    edge = torch.tensor([1.0, 2.0, 1.00390625, 1.01171875, 255.5 / 128, 3.99, 127.5 * 2.0 ** -7, -1.00390625, -2.5, 0.0078125])
    x = torch.cat([x, edge])
    r = gx.bf16_round(x.double())
    assert r.value.equal(x.to(torch.bfloat16).double())
    assert r.bits.equal(gx.bits_of(x.to(torch.bfloat16)))
    assert r.tie_down[-10 + 2] and r.tie_up[-10 + 3]     # 1 + 2^-8 -> 1 (down to even), 1 + 3 * 2^-8 -> 1 + 2^-6 (up to even)
    # below a power of two the grid halves: 2 - 2^-9 is decided by 2^-10, not undecided at 2^-8
    v = torch.tensor([2.0 - 2.0 ** -9], dtype=torch.float64)
    assert gx.bf16_round(v, torch.tensor([2.0 ** -10], dtype=torch.float64)).decided.all()
    assert not gx.bf16_round(v, torch.tensor([2.0 ** -8], dtype=torch.float64)).decided.any()


# ------------------------------------------------------------------------------------------------ the power of the comparison
M, N, K = 320, 256, 128


def _rejects(fn):
    with pytest.raises(AssertionError, match="elements differ"):
        fn()


def _trunc(v):
    """f64 -> bf16 by truncation of the f32 pattern"""
    return ((v.float().view(torch.int32) >> 16) << 16).view(torch.float32).to(torch.bfloat16)


def test_comparison_rejects_wrong_roundings():
    c = gx.case(M, N, K)
    v = c.ref_bias()
    good = gx.bf16_round(v).value.to(torch.bfloat16)
    gx.assert_bf16_rounded(good, v, tile_h=160)
    _rejects(lambda: gx.assert_bf16_rounded(_trunc(v), v))
    r = gx.bf16_round(v)
    away = torch.where(r.tie_down, r.hi, r.value).to(torch.bfloat16)              # round half away from zero
    _rejects(lambda: gx.assert_bf16_rounded(away, v))
    # double rounding through a coarser intermediate: first to 9 significant bits (nearest even), then to 8
    mant, expo = torch.frexp(v)
    coarse = torch.ldexp(torch.round(mant * 512.0), expo - 9)
    x = c.x0 * 0.5 + v                                                            # (a reference on the 2^-8 grid, so that 9 bits round)
    mant, expo = torch.frexp(x)
    coarse = torch.ldexp(torch.round(mant * 512.0), expo - 9)
    assert (coarse != x).any()
    _rejects(lambda: gx.assert_bf16_rounded(gx.bf16_round(coarse).value.to(torch.bfloat16), x))
    gx.assert_bf16_rounded(gx.bf16_round(x).value.to(torch.bfloat16), x)


def test_comparison_rejects_wrong_sums_and_places():
    c = gx.case(M, N, K)
    v = c.ref_f32()
    gx.assert_f32_exact(v.float(), v)
    drop = v - c.A[:, 77:78] @ c.W[:, 77:78].T                                    # one k dropped
    twice = v + c.A[:, 5:6] @ c.W[:, 5:6].T                                       # one k counted twice
    for wrong in (drop, twice):
        _rejects(lambda: gx.assert_f32_exact(wrong.float(), v))
        _rejects(lambda: gx.assert_bf16_rounded(gx.bf16_round(wrong + c.bias).value.to(torch.bfloat16), c.ref_bias()))
        assert (wrong != v).all()                                                 # no zero operand: every element moves
    rows = v.clone()
    rows[[3, 200]] = rows[[200, 3]]
    _rejects(lambda: gx.assert_f32_exact(rows.float(), v))
    cols = v.clone()
    cols[:, 16:32], cols[:, 144:160] = v[:, 144:160], v[:, 16:32]
    _rejects(lambda: gx.assert_f32_exact(cols.float(), v))
    shifted = c.acc + torch.roll(c.bias, 1)
    _rejects(lambda: gx.assert_bf16_rounded(gx.bf16_round(shifted).value.to(torch.bfloat16), c.ref_bias()))
    # the report names the fragment: two swapped 16-column groups show as n % 64 in 16..31 only
    with pytest.raises(AssertionError) as e:
        gx.assert_f32_exact(cols.float(), v)
    assert "n % 64: [16, 17" in str(e.value) and "31]" in str(e.value)


def test_comparison_rejects_statistics_of_the_unrounded_rows_and_a_stored_pad_row():
    c = gx.case(M, N, K, "stats")
    v = c.ref_resid()
    stored = gx.bf16_round(v).value
    want = c.stats64(stored)
    gx.assert_f32_exact(want.float().view(M, -1), want.view(M, -1))
    before = c.stats64(v)                                                         # taken before the rounding (bf16 stream)
    _rejects(lambda: gx.assert_f32_exact(before.float().view(M, -1), want.view(M, -1)))
    # a pad row stored: over the old row of an in-place epilogue, and over the NaN of a pure-write one
    mv = gx.ragged(M, 160)
    old = c.x0.to(torch.bfloat16)
    got = old.clone()
    got[:mv + 1] = stored[:mv + 1].to(torch.bfloat16)
    gx.assert_untouched(got[mv + 1:], old[mv + 1:])
    with pytest.raises(AssertionError, match=r"in rows \[0\]"):
        gx.assert_untouched(got[mv:], old[mv:])
    nan = torch.full((M, N), float("nan"))
    out = nan.clone()
    out[:mv] = c.ref_f32().float()[:mv]
    gx.assert_untouched(out[mv:], nan[mv:])
    out[M - 1, 64:128] = c.ref_f32().float()[M - 1, 64:128]
    with pytest.raises(AssertionError, match=r"64 elements differ"):
        gx.assert_untouched(out[mv:], nan[mv:])


def test_margins_decide_most_elements_and_only_near_boundaries():
    c = gx.case(M, N, K)
    v, margin = c.ref_qgelu()
    r = gx.bf16_round(v, margin)
    assert (~r.decided).double().mean().item() <= gx.UNDECIDED_CAP
    # an undecided element accepts both neighbours and nothing else; a decided one only its rounding
    good = r.value.to(torch.bfloat16)
    gx.assert_bf16_rounded(good, v, margin)
    other = torch.where(r.decided, r.value, torch.where(r.value == r.lo, r.hi, r.lo)).to(torch.bfloat16)
    gx.assert_bf16_rounded(other, v, margin)
    flipped = torch.where(r.value == r.lo, r.hi, r.lo).to(torch.bfloat16)
    _rejects(lambda: gx.assert_bf16_rounded(flipped, v, margin))
    # cancellation: a value far below its own T (margin of several bf16 steps) admits the roundings of [v - margin, v + margin] only
    tiny = torch.tensor([[3.1e-8]], dtype=torch.float64)
    wide = torch.tensor([[4e-9]], dtype=torch.float64)
    assert not gx.bf16_round(tiny, wide).decided.any()
    gx.assert_bf16_rounded(torch.tensor([[3.3e-8]]).to(torch.bfloat16), tiny, wide)
    _rejects(lambda: gx.assert_bf16_rounded(torch.tensor([[3.6e-8]]).to(torch.bfloat16), tiny, wide))
    _rejects(lambda: gx.assert_bf16_rounded(torch.tensor([[-3.1e-8]]).to(torch.bfloat16), tiny, wide))
    assert gx.observed_ratio(good, v, margin) == 0.0 and 0.0 < gx.observed_ratio(other, v, margin) <= 1.0

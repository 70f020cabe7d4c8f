"""What tests/test_skinny_chain_gpu.py relies on, established on the host (numpy float64, no GPU): the helpers of
skinny_chain_cases.py restate the device formats bit for bit, and the EXACT folded form rstd (xb W'^T - mean c) + b' — float64 on the
rounded W', c, b' and the f32 partials per 16 columns the kernel reads — lies within half of the project's bf16 tolerance (rtol 2^-7,
atol 4e-3) of the semantic form LayerNorm(xb) W^T + b for every (shape, stage, profile) the GPU chain test holds the kernel to the
semantic form on. The other half is the kernel's: the bf16 rounding of the output (2^-9 |y|) and its f32 accumulation.

Weight scale: as in test_chain_prelayernorm_fold_and_folded_gemm, W ~ 0.25 K^-1/2 N(0,1) for the semantic comparison. The rounding
of W' (2^-9 relative per weight) and the statistics being those of the f32 rows while A = bf16(rows) both move an output in
proportion to the weight scale; at unit scale NO profile meets half of tol at d = 128 (ratios 1.1 - 8.1 of tol, printed below), at
0.25 the profiles of SEMANTIC_CLEARED do, each with a margin (at most 0.44 of tol). The profiles left out (at d = 128 rowwise,
outlier and, at 0.49 too close to call, offset: rows near 38 with a standard deviation of 1 sit on a bf16 grid of 0.25, so the
mean of xb is not the mean of x) are still compared with the exact folded form on the GPU, at both scales."""
import numpy as np
import pytest

import skinny_chain_cases as sc


def test_bf16_helpers_match_torch_bit_for_bit():
    import torch

    g = sc.rng_of(1)
    x = np.concatenate([g.standard_normal(4096) * 10.0 ** g.integers(-6, 6, 4096),
                        [0.0, -0.0, 1.00390625, 1.01171875, 3.3895314e38, 1e-40]]).astype(np.float32)   # ties to even, near-max, subnormal
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(sc.bf16_bits(x), want)
    assert np.array_equal(sc.bf16_round(x).view(np.uint32), want.astype(np.uint32) << 16)


def test_rows_have_the_profiles_the_tests_rely_on():
    x = sc.rows(128, 1024, "rowwise", 3).astype(np.float64)
    m = np.arange(128)
    assert np.allclose(x.mean(1), 0.5 * m, atol=0.8) and np.allclose(x.std(1), 1 + m % 5, rtol=0.15)
    # neighbouring 16-row tiles: the same row of the next tile is 8 away in the mean (>= 1.6 standard deviations of ANY row)
    assert np.all(np.abs(x.mean(1)[16:] - x.mean(1)[:-16]) > 6.0)
    o = sc.rows(77, 128, "offset", 3).astype(np.float64)
    assert np.allclose(o.mean(1) / o.std(1), 10, rtol=0.25)
    t = sc.rows(77, 128, "outlier", 3).astype(np.float64)
    assert (t * t)[:, [3, 65, 126]].sum() > 0.98 * (t * t).sum()
    assert np.array_equal(sc.rows(5, 64, "plain", 3), sc.rows(5, 64, "plain", 3))
    W, _, _, _ = sc.weights(128, 2048, 4)
    assert np.array_equal(sc.bf16_round(W), W) and abs(W.astype(np.float64).std() * 2048 ** 0.5 - 1) < 0.02


@pytest.mark.parametrize("profile", sc.PROFILES)
def test_host_partials_are_within_the_summation_bound(profile):
    x = sc.rows(77, 768, profile, 5)
    st = sc.stats16_host(x).astype(np.float64)
    v = x.astype(np.float64).reshape(77, 48, 16)
    assert (np.abs(st[..., 0] - v.sum(-1)) <= 16 * sc.U * np.abs(v).sum(-1)).all()
    assert (np.abs(st[..., 1] - (v * v).sum(-1)) <= 16 * sc.U * (v * v).sum(-1)).all()


def _ratio(case, stage):
    x, W, gam, bet, bias, gelu = case.stage(stage)
    xb = sc.bf16_round(x)
    wf, c, bf = sc.fold_host(W, gam, bet, bias)
    exact = sc.exact_folded(xb, wf, c, bf, sc.stats16_host(x), gelu)
    ref = sc.semantic(xb, W, gam, bet, bias, gelu)
    return float((np.abs(exact - ref) / sc.tol(ref)).max())


@pytest.mark.parametrize("profile", sc.PROFILES)
@pytest.mark.parametrize("stage", ["qkv", "fc1"])
@pytest.mark.parametrize("shape", sc.CHAIN_SHAPES, ids=lambda s: f"d{s[0]}")
def test_exact_folded_form_is_within_half_the_tolerance_of_the_semantic_form(shape, stage, profile):
    d, Nq, mlp = shape
    r = _ratio(sc.ChainCase(d, Nq, mlp, profile, sc.SEMANTIC_W_SCALE), stage)
    r1 = _ratio(sc.ChainCase(d, Nq, mlp, profile, 1.0), stage)
    print(f"d={d} {stage} {profile}: max |exact - semantic| / tol = {r:.3f} at scale {sc.SEMANTIC_W_SCALE}, {r1:.3f} at unit scale")
    if profile in sc.SEMANTIC_CLEARED[(d, stage)]:
        assert r <= 0.5, r


def test_unit_scale_cannot_meet_half_the_tolerance_at_d128():
    """why the semantic comparison runs at 0.25: at unit scale even the plain profile exceeds the WHOLE tolerance at d = 128"""
    d, Nq, mlp = sc.CHAIN_SHAPES[0]
    for stage in ("qkv", "fc1"):
        assert _ratio(sc.ChainCase(d, Nq, mlp, "plain", 1.0), stage) > 1.0

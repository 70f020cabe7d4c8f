"""Calibrated activation centring for the fp8 vision tower (mmiss_encoder_calibrate, csrc/calibrate_kernels.h):

    LN(x) W^T + b  =  (LN(x) - mu) W^T + (b + W mu)

The three one-shot kernels against float64 restatements, the parity gap of the outlier-channel regime closing below the
project's 1e-3 (tests/test_headline_gpu.py pins the UNCALIBRATED handle at 1.15e-3; that test stays as it is), and bit
equality of everything the calibration must not touch."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COS_TOL = 1e-3  # BASELINE.json north_star: "within 1e-3 cosine of the reference CPU path"
EPS = 1e-5


def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _kernels_of(fn):
    """Run fn() with every libmmiss launch bracketed; returns (result, {kernel class: launches})."""
    from mmiss_amd import _lib

    _lib.prof_filter(None, 1)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        out = fn()
    finally:
        _lib.prof_enable(False)
    return out, {p["kernel"]: p["launches"] for p in _lib.prof_read()}


def _sim():
    spec = importlib.util.spec_from_file_location("fp8_calib_sim", os.path.join(ROOT, "tools", "fp8_calib_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    return sim


# ------------------------------------------------------------------------------------------------ 1. ln_colstats
def _colstats_case(M, d, bf16_in):
    import torch

    rng = np.random.Generator(np.random.Philox(1000 * M + d + (7 if bf16_in else 0)))
    x = rng.standard_normal((M, d), dtype=np.float32)
    x[:, 31] += 300.0       # planted on every row
    x[:, d - 268] -= 180.0  # (500 at d = 768)
    x[0, 100] += 250.0      # large in row 0 only
    gam = (1.0 + 0.1 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
    bet = (0.02 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    if bf16_in:
        xd = xd.to(torch.bfloat16)
        x = xd.float().cpu().numpy()   # the same input bytes, widened
    return x, gam, bet, xd


def _run_colstats(xd, gam, bet, M, d, bf16_in):
    import torch
    from mmiss_amd import _lib

    lib = _lib.load()
    gd, bd = torch.from_numpy(gam).cuda(), torch.from_numpy(bet).cuda()
    mean = torch.full((d,), np.nan, dtype=torch.float64, device="cuda")
    var = torch.full((d,), np.nan, dtype=torch.float64, device="cuda")
    mu = torch.full((d,), np.nan, dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.mmiss_dbg_ln_colstats(0, None, xd.data_ptr(), 1 if bf16_in else 0, gd.data_ptr(), bd.data_ptr(), M, d, EPS,
                                         mean.data_ptr(), var.data_ptr(), mu.data_ptr(), cnt.data_ptr()))
    torch.cuda.synchronize()
    return mean.cpu().numpy(), var.cpu().numpy(), mu.cpu().numpy(), int(cnt.item())


@pytest.mark.parametrize("M,d,bf16_in", [(M, d, False) for M in (1, 50, 257, 1203) for d in (768, 1024)] + [(257, 768, True), (257, 1024, True)])
def test_ln_colstats_against_float64(M, d, bf16_in):
    """Column mean / population variance of LayerNorm(x) over M rows (ragged row blocks of 32, one row, several workgroups)
    against float64 on the same input bytes. Accumulation is f64, so what remains is the f32 evaluation of y (about 8 roundings
    of 2^-24 and the hardware rsqrt); the bounds are ~16 x that:
      mean      |err_c| <= 2^-20 (|beta_c| + |gamma_c| max_r |xhat_rc|)
      variance  |err_c| <= 2^-18 var_c + (the mean's bound)^2
    The centring decision equals the float64 one for every channel whose mean^2 / var is outside [0.99, 1.01]."""
    x, gam, bet, xd = _colstats_case(M, d, bf16_in)
    mean, var, mu, cnt = _run_colstats(xd, gam, bet, M, d, bf16_in)
    x64 = x.astype(np.float64)
    rm = x64.mean(1, keepdims=True)
    rv = ((x64 - rm) ** 2).mean(1, keepdims=True)
    xhat = (x64 - rm) / np.sqrt(rv + EPS)
    y = xhat * gam.astype(np.float64) + bet.astype(np.float64)
    mean_ref = y.mean(0)
    var_ref = ((y - mean_ref) ** 2).mean(0)
    a = 2.0 ** -20 * (np.abs(bet) + np.abs(gam) * np.abs(xhat).max(0))
    e_mean = np.abs(mean - mean_ref)
    e_var = np.abs(var - var_ref)
    b_var = 2.0 ** -18 * var_ref + a * a
    print("ln_colstats M=%d d=%d %s: max |mean err| / bound %.3f, max |var err| / bound %.3f (worst column %d)"
          % (M, d, "bf16" if bf16_in else "f32", (e_mean / a).max(), (e_var / np.maximum(b_var, 1e-300)).max(),
             int((e_var / np.maximum(b_var, 1e-300)).argmax())))
    assert (e_mean <= a).all(), (e_mean / a).max()
    assert (e_var <= b_var).all(), (e_var / b_var).max()
    # the decision
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(var_ref > 0, mean_ref ** 2 / var_ref, np.inf)
    clear = (ratio < 0.99) | (ratio > 1.01)
    centred = mu != 0
    np.testing.assert_array_equal(centred[clear], (ratio >= 1.0)[clear])
    np.testing.assert_array_equal(mu[centred], mean.astype(np.float32)[centred])
    assert cnt == int(centred.sum())
    if M > 1:
        assert centred[31] and centred[d - 268]            # planted on every row: constant part >> varying part
        assert not centred[100]                            # large in row 0 only: mean^2 / var ~ 1 / M
        assert centred.sum() < d // 2, centred.sum()       # most ordinary columns vary more than they sit
    else:
        assert centred.all()                               # one row: no varying part at all
    # two calls, equal bytes
    mean2, var2, mu2, cnt2 = _run_colstats(xd, gam, bet, M, d, bf16_in)
    assert mean.tobytes() == mean2.tobytes() and var.tobytes() == var2.tobytes() and mu.tobytes() == mu2.tobytes() and cnt == cnt2


# ------------------------------------------------------------------------------------------------ 2. bias_fold
@pytest.mark.parametrize("N", [2304, 3072, 64])
@pytest.mark.parametrize("K", [768, 1024])
def test_bias_fold_against_float64(N, K):
    """b' = b + W_bf16 mu, one wave per row, f32 accumulation in a fixed order: |err_n| <= 4 K 2^-24 sum_k |w_nk mu_k| against
    float64 on the bf16-rounded weights (the project's form of the f32-accumulation bound); mu = 0 returns the bias bit for bit."""
    import torch
    from mmiss_amd import _lib

    lib = _lib.load()
    rng = np.random.Generator(np.random.Philox(N * 7 + K))
    w = torch.from_numpy(rng.standard_normal((N, K), dtype=np.float32) * np.float32(0.03)).to(torch.bfloat16).cuda()
    bias = (0.02 * rng.standard_normal(N, dtype=np.float32)).astype(np.float32)
    mu = (0.1 * rng.standard_normal(K, dtype=np.float32)).astype(np.float32)
    mu[31], mu[500] = 24.0, -24.0
    bd, md = torch.from_numpy(bias).cuda(), torch.from_numpy(mu).cuda()
    out = torch.full((N + 3,), np.nan, dtype=torch.float32, device="cuda")
    _lib.check(lib.mmiss_dbg_bias_fold(0, None, w.data_ptr(), bd.data_ptr(), md.data_ptr(), N, K, out.data_ptr()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[N:]).all())   # nothing behind row N - 1 is written
    w64 = w.float().cpu().numpy().astype(np.float64)
    ref = bias.astype(np.float64) + w64 @ mu.astype(np.float64)
    bound = 4.0 * K * 2.0 ** -24 * (np.abs(w64) * np.abs(mu.astype(np.float64))).sum(1)
    err = np.abs(out[:N].cpu().numpy().astype(np.float64) - ref)
    print("bias_fold N=%d K=%d: max |err| / bound %.4f" % (N, K, (err / bound).max()))
    assert (err <= bound).all(), (err / bound).max()
    zero = torch.zeros((K,), dtype=torch.float32, device="cuda")
    _lib.check(lib.mmiss_dbg_bias_fold(0, None, w.data_ptr(), bd.data_ptr(), zero.data_ptr(), N, K, out.data_ptr()))
    torch.cuda.synchronize()
    assert out[:N].cpu().numpy().tobytes() == bias.tobytes()


# ------------------------------------------------------------------------------------------------ the tower
@pytest.fixture(scope="module")
def b32():
    """Seeded ViT-B/32 weights, the 256 evaluated images and the subset of tests/test_headline_gpu.py's outlier test, and 64
    OTHER images to calibrate on; oracle embeddings are computed once per weight set."""
    import mmiss_amd  # noqa: F401
    from oracle import clip_oracle as co

    sim = _sim()
    W0 = co.init_weights(co.VIT_B32, seed=0)
    px = np.random.Generator(np.random.Philox(4321)).standard_normal((256, 3, 224, 224), dtype=np.float32)
    cpx = (np.random.Generator(np.random.Philox(99)).standard_normal((64, 3, 224, 224), dtype=np.float32) * np.float32(0.7)
           + np.float32(0.3)).astype(np.float32)
    sub = np.arange(3, 256, 32)
    cache = {}

    def weights_and_ref(how):
        if how not in cache:
            W = sim.outlier_weights(W0, how)
            cache[how] = (W, co.embed_images(px[sub], W, co.VIT_B32))
        return cache[how]

    return co, sim, px, cpx, sub, weights_and_ref


def _fp8_encoder(co, W, **kw):
    from mmiss_amd.encoder import ClipEncoder, ClipShape

    enc = ClipEncoder(ClipShape.from_any(co.VIT_B32), max_batch_image=256, max_batch_text=8, precision="fp8", **kw)
    enc.load_state_dict(W)
    return enc


def test_b32_bs256_fp8_outlier_channels_calibrated_hold_the_tolerance(b32):
    """3. The +300 / -180 residual channels of test_b32_bs256_fp8_setting_with_outlier_hidden_channels_is_outside_the_tolerance
    (1.15e-3 uncalibrated) after calibrate() on 64 other images: inside 1e-3 (simulated 1.25e-3 -> 6.2e-4), with exactly the
    launches of the uncalibrated encode."""
    co, _, px, cpx, sub, weights_and_ref = b32
    W, ref = weights_and_ref("all")
    enc = _fp8_encoder(co, W)
    try:
        out0, kern0 = _kernels_of(lambda: enc.encode_image(px))
        info = enc.calibrate(cpx)
        out1, kern1 = _kernels_of(lambda: enc.encode_image(px))
    finally:
        enc.close()
    d0 = (1 - _cos(out0[sub], ref)).max()
    d1 = (1 - _cos(out1[sub], ref)).max()
    print("ViT-B/32 bs 256, outlier channels +300 / -180, fp8: 1 - cos vs fp32 oracle  uncalibrated %.2e, calibrated %.2e  (%s)"
          % (d0, d1, info))
    assert info["sites"] == 24 and info["hidden"] == 768 and info["rows"] == 64 * 50 and info["centred"] >= 48, info
    assert kern1 == kern0, (kern0, kern1)
    assert kern1.get("gemm_fp8_bias_p256", 0) == 12, kern1
    assert d1 < COS_TOL, (d0, d1)
    assert np.abs(np.linalg.norm(out1, axis=1) - 1).max() < 1e-5


def test_b32_bs256_fp8_cls_row_outliers_calibrated(b32):
    """4. The same channels on the CLS row only: centring them would put 24 / 50 on the 49 ordinary rows, so the rule
    (mean^2 >= var) must leave them alone wherever the float64 statistics of that site say so — and the result stays inside
    1e-3 (simulated 7.3e-4; uncalibrated 7.8e-4)."""
    import torch

    co, sim, px, cpx, sub, weights_and_ref = b32
    W, ref = weights_and_ref("cls")
    enc = _fp8_encoder(co, W)
    try:
        out0 = enc.encode_image(px)
        enc.calibrate(cpx)
        mu = enc.get_calibration()
        out1 = enc.encode_image(px)
    finally:
        enc.close()
    d0 = (1 - _cos(out0[sub], ref)).max()
    d1 = (1 - _cos(out1[sub], ref)).max()
    print("ViT-B/32 bs 256, +300 / -180 on the CLS row only, fp8: 1 - cos vs fp32 oracle  uncalibrated %.2e, calibrated %.2e" % (d0, d1))
    assert mu.shape == (24, 768)
    stats = []
    with torch.no_grad():
        sim.tower(cpx, W, co.VIT_B32, "collect", stats, device="cuda")   # float64 (mean, variance) of every site
    ratio = np.stack([(m * m / v)[[31, 500]].cpu().numpy() for m, v in stats])
    print("mean^2 / var of channels 31, 500 per site: min %.3g max %.3g; mu there: %s" % (ratio.min(), ratio.max(), np.abs(mu[:, [31, 500]]).max()))
    assert (ratio[0] < 0.99).all()                       # site 0 by construction: one row of 50 carries the channel
    assert (mu[:, [31, 500]][ratio < 0.99] == 0).all()
    assert d1 < COS_TOL, (d0, d1)


def test_b32_bs256_fp8_without_outliers_calibrated(b32):
    """5. Seeded Gaussian weights: calibration neither helps nor hurts much (simulated 6.4e-4 -> 6.6e-4); inside 1e-3 against the
    oracle and against the bf16 path."""
    co, _, px, cpx, sub, weights_and_ref = b32
    W, ref = weights_and_ref(None)
    enc = _fp8_encoder(co, W)
    try:
        out0 = enc.encode_image(px)
        info = enc.calibrate(cpx)
        out1 = enc.encode_image(px)
        enc.set_precision("bf16")
        out16 = enc.encode_image(px)
    finally:
        enc.close()
    d0 = (1 - _cos(out0[sub], ref)).max()
    d1 = (1 - _cos(out1[sub], ref)).max()
    d16 = (1 - _cos(out1, out16)).max()
    print("ViT-B/32 bs 256, no outliers, fp8: 1 - cos vs fp32 oracle  uncalibrated %.2e, calibrated %.2e; calibrated vs bf16 path %.2e  (%s)"
          % (d0, d1, d16, info))
    assert d1 < COS_TOL, (d0, d1)
    assert d16 < COS_TOL, d16


def test_calibration_moves_nothing_else(b32):
    """6. Bit equality of everything the calibration must not touch, and of everything it promises to reproduce."""
    co, _, px, cpx, _, weights_and_ref = b32
    W, _ = weights_and_ref("all")
    s = co.VIT_B32
    ids = co.synthetic_text_ids(4, s.t_ctx, s.t_vocab, s.eos_token_id, seed=8)
    enc = _fp8_encoder(co, W)
    fresh = None
    try:
        fp8_before = enc.encode_image(px)
        small_before = enc.encode_image(px[:16])     # 800 rows < fp8_min_rows: the bf16 kernels
        txt_before = enc.encode_text(ids)
        enc.set_precision("bf16")
        bf16_before = enc.encode_image(px)
        enc.set_precision("fp8")

        enc.calibrate(cpx)
        mu1 = enc.get_calibration()
        fp8_cal = enc.encode_image(px)
        assert not np.array_equal(fp8_cal, fp8_before)   # (it does do something on these weights)
        np.testing.assert_array_equal(enc.encode_image(px[:16]), small_before)
        np.testing.assert_array_equal(enc.encode_text(ids), txt_before)
        enc.set_precision("bf16")
        np.testing.assert_array_equal(enc.encode_image(px), bf16_before)
        enc.set_precision("fp8")
        np.testing.assert_array_equal(enc.encode_image(px), fp8_cal)   # the calibration survives the precision switch

        enc.calibrate(cpx)                               # twice on the same pixels
        np.testing.assert_array_equal(enc.get_calibration(), mu1)
        np.testing.assert_array_equal(enc.encode_image(px), fp8_cal)

        fresh = _fp8_encoder(co, W)                      # a stored table on a fresh handle with the same weights
        fresh.set_calibration(mu1)
        assert fresh.calibration_info()["sites"] == 24 and fresh.calibration_info()["centred"] == enc.calibration_info()["centred"]
        np.testing.assert_array_equal(fresh.encode_image(px), fp8_cal)

        enc.clear_calibration()
        assert enc.calibration_info()["sites"] == 0 and enc.get_calibration().shape == (0, 768)
        np.testing.assert_array_equal(enc.encode_image(px), fp8_before)
    finally:
        enc.close()
        if fresh is not None:
            fresh.close()


def test_calibration_errors_name_the_argument():
    """7. MMISS_ERR_ARG with a message that names the argument; a cleared handle reports no sites."""
    import mmiss_amd  # noqa: F401
    from mmiss_amd.encoder import ClipEncoder, ClipShape
    from oracle import clip_oracle as co

    s = co.TINY
    W = co.init_weights(s, seed=0)
    S = s.v_image
    px = np.random.Generator(np.random.Philox(5)).standard_normal((5, 3, S, S), dtype=np.float32)
    raw = ClipEncoder(ClipShape.from_any(s), max_batch_image=4, max_batch_text=4)
    enc = ClipEncoder(ClipShape.from_any(s), max_batch_image=4, max_batch_text=4)
    try:
        with pytest.raises(RuntimeError, match="enc is not finalized"):
            raw.calibrate(px[:2])
        with pytest.raises(RuntimeError, match="enc is not finalized"):
            raw.set_calibration(np.zeros((2 * s.v_layers, s.v_hidden), np.float32))
        enc.load_state_dict(W)
        with pytest.raises(RuntimeError, match=r"B = 0 outside 1 \.\. max_batch_image = 4"):
            enc.calibrate(px[:0])
        with pytest.raises(RuntimeError, match=r"B = 5 outside 1 \.\. max_batch_image = 4"):
            enc.calibrate(px)
        with pytest.raises(RuntimeError, match=r"n = %d, the table holds" % (2 * s.v_layers * s.v_hidden - 1)):
            enc.set_calibration(np.zeros(2 * s.v_layers * s.v_hidden - 1, np.float32))
        assert enc.calibration_info()["sites"] == 0
        info = enc.calibrate(px[:4])
        assert (info["sites"], info["hidden"], info["rows"]) == (2 * s.v_layers, s.v_hidden, 4 * ((S // s.v_patch) ** 2 + 1)), info
        assert enc.get_calibration().shape == (2 * s.v_layers, s.v_hidden)
        enc.clear_calibration()
        assert enc.calibration_info()["sites"] == 0
        # a weight of the vision tower changes: the calibration goes with it
        enc.calibrate(px[:4])
        enc.load_state_dict({"vision_model.pre_layrnorm.bias": W["vision_model.pre_layrnorm.bias"]})
        assert enc.calibration_info()["sites"] == 0
    finally:
        raw.close()
        enc.close()


def test_l14_width_fp8_outlier_channels_calibrated():
    """8. Width 1024: the 6-layer tower of the ViT-L/14 geometry with the +300 / -180 channels of
    test_l14_width_fp8_outlier_hidden_channels (8.3e-4 uncalibrated), 128 images per call, calibrated on 16 other images — the
    d = 1024 LayerNorm -> MXFP8 kernels and the persistent fp8 GEMM at K = 1024 on beta' / b'."""
    import mmiss_amd  # noqa: F401
    from mmiss_amd.encoder import ClipEncoder, ClipShape
    from oracle import clip_oracle as co

    s = dataclasses.replace(co.LONGCLIP_L14, v_layers=6, t_layers=1, t_vocab=1000, eos_token_id=999)
    W = co.init_weights(s, seed=61)
    pos = W["vision_model.embeddings.position_embedding.weight"].copy()
    pos[:, 31] += 300.0
    pos[:, 700] -= 180.0
    W["vision_model.embeddings.position_embedding.weight"] = pos
    px = np.random.Generator(np.random.Philox(62)).standard_normal((128, 3, 224, 224), dtype=np.float32)
    cpx = (np.random.Generator(np.random.Philox(99)).standard_normal((16, 3, 224, 224), dtype=np.float32) * np.float32(0.7)
           + np.float32(0.3)).astype(np.float32)
    sub = [0, 5, 15, 64, 127]
    ref = co.embed_images(px[sub], W, s)
    enc = ClipEncoder(ClipShape.from_any(s), max_batch_image=128, max_batch_text=2, precision="fp8")
    enc.load_state_dict(W)
    try:
        out0, kern0 = _kernels_of(lambda: enc.encode_image(px))
        info = enc.calibrate(cpx)
        out1, kern1 = _kernels_of(lambda: enc.encode_image(px))
    finally:
        enc.close()
    d0 = (1 - _cos(out0[sub], ref)).max()
    d1 = (1 - _cos(out1[sub], ref)).max()
    print("L/14 width, 6 layers, outlier channels +300 / -180, fp8, 128 per call: 1 - cos vs fp32 oracle  uncalibrated %.2e, calibrated %.2e  (%s)"
          % (d0, d1, info))
    assert info["sites"] == 12 and info["hidden"] == 1024 and info["rows"] == 16 * 257, info
    assert kern1 == kern0 and any(k.startswith("gemm_fp8") and k.endswith("p256") for k in kern1), (kern0, kern1)
    assert d1 < COS_TOL, (d0, d1)

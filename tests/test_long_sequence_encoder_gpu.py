"""Towers above 288 tokens end to end: the ViT-L/14 geometry at 336 px (24 x 24 + 1 = 577 vision tokens, the shape of
openai/clip-vit-large-patch14-336) two layers deep, and a causal text tower of 300 tokens, through ClipEncoder against
oracle/clip_oracle.py at the project's bar. Above 288 tokens the attention is attention_tiled_kernel (csrc/attention_tiled.h,
held kernel-level in tests/test_attention_tiled_gpu.py); everything else works on token rows and is the code the shorter
towers run — what these tests prove is that nothing on the way silently assumed fewer rows per item."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3  # BASELINE.json north_star: "within 1e-3 cosine of the reference CPU path"
N_IMAGES = 11   # 11 x 577 = 6347 rows: above ln_fold_min_rows (6000)


def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@pytest.fixture(scope="module")
def l336():
    """(shape, weights, pixels [11], oracle embeddings [11], oracle taps of the first two images) — the oracle runs ONCE."""
    from oracle import clip_oracle as co

    s = dataclasses.replace(co.LONGCLIP_L14, v_image=336, v_layers=2, t_layers=2, t_ctx=77, t_vocab=2000, eos_token_id=1999)
    assert s.v_tokens == 577
    W = co.init_weights(s, seed=336)
    rng = np.random.Generator(np.random.Philox(337))
    px = rng.standard_normal((N_IMAGES, 3, 336, 336), dtype=np.float32)
    taps = {}
    ref = co.l2_normalize(co.image_features(px, W, s, taps))
    return s, W, px, ref, {l: t[:2].copy() for l, t in taps.items()}


def _encoder(s, W, batch, precision="bf16"):
    from mmiss_amd.encoder import ClipEncoder, ClipShape

    enc = ClipEncoder(ClipShape.from_any(s), max_batch_image=batch, max_batch_text=2, precision=precision)
    enc.load_state_dict(W)
    return enc


def _with_kernels(fn):
    from mmiss_amd import _lib

    _lib.prof_reset(); _lib.prof_enable(True)
    try:
        out = fn()
    finally:
        _lib.prof_enable(False)
    return out, {p["kernel"]: p["launches"] for p in _lib.prof_read()}


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_two_images_small_call_path(l336, precision):
    """B = 2: 1154 rows — the f32 residual stream, separate LayerNorm kernels; under "fp8" above fp8_min_rows (1024), so QKV /
    FC1 / FC2 run on the fp8 GEMMs while the attention still writes bf16 rows (no bf16 residual stream: no fp8 out-projection)."""
    s, W, px, ref, _ = l336
    enc = _encoder(s, W, 2, precision)
    out, kern = _with_kernels(lambda: enc.encode_image(px[:2]))
    enc.close()
    assert out.shape == (2, 768) and np.abs(np.linalg.norm(out, axis=1) - 1).max() < 1e-5
    assert kern.get("attention", 0) == 2 and "attention_mx" not in kern, kern
    assert any(k.startswith("gemm_fp8") for k in kern) == (precision == "fp8"), kern
    assert (1 - _cos(out, ref[:2])).max() < COS_TOL


def test_eleven_images_bf16_residual_stream(l336):
    """B = 11: 6347 rows >= ln_fold_min_rows — the bf16 residual stream with the LayerNorm folded into the QKV / FC1 GEMMs
    (hidden 1024: finished row statistics, ln_finalize_kernel), the last layer pruned to the class rows: both layers' attention
    is the full 577-token one (the pooled-query form stops at 128 tokens) with the gather behind the second."""
    s, W, px, ref, _ = l336
    enc = _encoder(s, W, N_IMAGES)
    out, kern = _with_kernels(lambda: enc.encode_image(px))
    enc.close()
    assert kern.get("attention", 0) == 2 and kern.get("ln_finalize", 0) > 0, kern
    assert (1 - _cos(out, ref)).max() < COS_TOL


def test_eleven_images_fp8_attention_writes_mxfp8(l336):
    """B = 11 under "fp8": the first layer's out-projection is the fp8 GEMM, fed by the attention's MXFP8 output — one
    attention_mx launch, which at 577 tokens can only be attention_tiled_kernel<false, true> (launch_attention_mx routes by T
    alone); the pruned last layer keeps the bf16 attention."""
    s, W, px, ref, _ = l336
    enc = _encoder(s, W, N_IMAGES, "fp8")
    out, kern = _with_kernels(lambda: enc.encode_image(px))
    enc.close()
    assert kern.get("attention_mx", 0) == 1 and kern.get("attention", 0) == 1, kern
    assert any(k.startswith("gemm_fp8_bias_resid16") for k in kern), kern   # the residual GEMMs on the bf16 stream, in fp8
    assert (1 - _cos(out, ref)).max() < COS_TOL


def test_residual_stream_after_the_first_layer(l336):
    """The residual stream after layer 1 of the B = 2 call, every token row, at test_tiny_image_tower_layer_by_layer's tolerance."""
    s, W, px, ref, taps = l336
    enc = _encoder(s, W, 2)
    enc.record_taps(True)
    out = enc.encode_image(px[:2])
    T, d = s.v_tokens, s.v_hidden
    got = enc.tap(0, 1, 2 * T * d).reshape(2, T, d)
    enc.close()
    err, scale = np.abs(got - taps[1]).max(), np.abs(taps[1]).max()
    assert err < 0.03 * scale, (err, scale)
    assert (1 - _cos(out, ref[:2])).max() < COS_TOL


def test_resize_and_crop_to_336(l336):
    """CLIPImageProcessor's resize + centre crop at S = 336 (no encoder of that image size could be created before), bit for bit."""
    from mmiss_amd.encoder import ClipEncoder, ClipShape
    from oracle import resize_oracle as ro

    s = l336[0]
    enc = ClipEncoder(ClipShape.from_any(s), max_batch_image=2, max_batch_text=2)   # no weights: the resize needs none
    rng = np.random.default_rng(336)
    imgs = [rng.integers(0, 256, (500, 400, 3), dtype=np.uint8), rng.integers(0, 256, (336, 700, 3), dtype=np.uint8)]
    got = enc.resize_crop_rgb(imgs)
    enc.close()
    assert got.shape == (2, 336, 336, 3) and got.dtype == np.uint8
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i], ro.resize_crop_u8(im, 336)), i


def test_causal_text_tower_of_300_tokens():
    """TINY widths, t_ctx = 300: the causal form of the tiled kernel inside a tower. Three rows with the EOS (the pooled row) at
    positions 5, 150 and 299 — the first chunk, the second, and the last key of the odd 19th key tile."""
    from mmiss_amd.encoder import ClipEncoder, ClipShape
    from oracle import clip_oracle as co

    s = dataclasses.replace(co.TINY, t_ctx=300)
    W = co.init_weights(s, seed=300)
    rng = np.random.Generator(np.random.Philox(301))
    ids = np.full((3, 300), s.eos_token_id, dtype=np.int64)
    for r, eos in enumerate((5, 150, 299)):
        ids[r, :eos] = rng.integers(1, s.eos_token_id - 1, eos)
    enc = ClipEncoder(ClipShape.from_any(s), max_batch_image=2, max_batch_text=4)
    enc.load_state_dict(W)
    out, kern = _with_kernels(lambda: enc.encode_text(ids))
    enc.close()
    assert kern.get("attention", 0) == s.t_layers, kern
    assert (1 - _cos(out, co.embed_texts(ids, W, s))).max() < COS_TOL

"""attention_tiled_kernel (csrc/attention_tiled.h): attention above 288 tokens, the keys walked in chunks of 128 through two
LDS images. Through the C-ABI (mmiss_dbg_attention_tiled runs the kernel at any 1 <= T <= 1025; the product routes T <= 288
elsewhere), against the fp32 softmax of torch within the per-element bound every attention kernel of the project is held to,
and — where both run — against attention_long_kernel bit for bit: the chunk is a multiple of the 32 keys of one step, so
chunking changes the order of no operation, and a difference is a bug in the chunk seams.

Every output buffer carries one sentinel row behind row B * T, which must come back untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch, _lib, lib


def _attn_ref(torch, qkv, B, T, H, causal, with_bound=False):
    """fp32 softmax attention of torch. with_bound: also the per-element bound the kernels are held to: 2.5e-3 + 2^-8 |out|
    (the output's bf16 rounding, half an ulp) + 4 x 2^-9 sqrt(sum_i p_i^2 v_i^2) (P is rounded to bf16, 2^-9 relative per
    probability, independent roundings: four standard deviations of their sum)."""
    d = H * 64
    x = qkv.float().reshape(B, T, 3, H, 64)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s + torch.triu(torch.full((T, T), float("-inf"), device=qkv.device), diagonal=1)
    p = torch.softmax(s, dim=-1)
    out = (p @ v).transpose(1, 2).reshape(B * T, d)
    if not with_bound:
        return out
    spread = ((p * p) @ (v * v)).sqrt().transpose(1, 2).reshape(B * T, d)
    return out, 2.5e-3 + out.abs() * 2.0 ** -8 + spread * (4 * 2.0 ** -9)


def _assert_attention_close(torch, ctx, ref, bound):
    assert torch.isfinite(ctx.float()).all()
    err = (ctx.float() - ref).abs()
    assert (err <= bound).all(), (err.max().item(), (err - bound).max().item())


def _tiled(env, qkv, B, T, H, causal):
    """attention_tiled_kernel, bf16 rows."""
    torch, _lib, lib = env
    ctx = torch.full((B * T + 1, H * 64), -7.0, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mmiss_dbg_attention_tiled(0, None, qkv.data_ptr(), ctx.data_ptr(), None, None, B, T, H, causal))
    torch.cuda.synchronize()
    assert (ctx[B * T] == -7.0).all(), "the row behind the last item was written"
    return ctx[:B * T]


def _tiled_mx(env, qkv, B, T, H):
    """attention_tiled_kernel, MXFP8 rows: (e4m3 bytes, permuted E8M0 scale bytes)."""
    from oracle import fp8_oracle as fo

    torch, _lib, lib = env
    c8 = torch.full((B * T + 1, H * 64), 0x5A, device="cuda", dtype=torch.uint8)
    cs = torch.full((B * T + 1, fo.scale_row_bytes(H * 64)), 0x5A, device="cuda", dtype=torch.uint8)
    _lib.check(lib.mmiss_dbg_attention_tiled(0, None, qkv.data_ptr(), None, c8.data_ptr(), cs.data_ptr(), B, T, H, 0))
    torch.cuda.synchronize()
    assert (c8[B * T] == 0x5A).all() and (cs[B * T] == 0x5A).all(), "the row behind the last item was written"
    return c8[:B * T], cs[:B * T]


def _randn_qkv(torch, B, T, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B * T, 3 * H * 64, device="cuda", generator=g).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- (a) against fp32 torch
# For a chunk of 128, 256 or 288 keys alike: whole chunks (512, 576, 1024 + 1), one key in the last chunk (289, 385, 513,
# 577, 1025), an odd last key tile (289, 385, 513, 577, 1025), the smallest new T; more than one query block and, at 577 =
# 4 blocks + 5 tiles, idle waves in the last block; the last case fills the chip (384 pairs x 5 blocks).
@pytest.mark.parametrize("B,T,H,causal", [(1, 289, 2, 0), (2, 289, 2, 1), (1, 385, 2, 0), (2, 512, 2, 0), (1, 513, 3, 1), (1, 576, 2, 0),
                                          (2, 577, 4, 0), (1, 577, 2, 1), (1, 1025, 2, 0), (1, 1025, 1, 1), (24, 577, 16, 0)])
def test_tiled_attention_against_fp32_softmax(env, B, T, H, causal):
    torch, _lib, lib = env
    qkv = _randn_qkv(torch, B, T, H, B * 1000 + T + causal)
    ctx = _tiled(env, qkv, B, T, H, causal)
    ref, bound = _attn_ref(torch, qkv, B, T, H, bool(causal), with_bound=True)
    _assert_attention_close(torch, ctx, ref, bound)
    for _ in range(3):   # repeatable bits
        assert torch.equal(ctx, _tiled(env, qkv, B, T, H, causal))
    # the product's route above 288 tokens is this kernel
    via = torch.full((B * T + 1, H * 64), -7.0, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mmiss_dbg_attention(0, None, qkv.data_ptr(), via.data_ptr(), B, T, H, causal))
    torch.cuda.synchronize()
    assert (via[B * T] == -7.0).all() and torch.equal(via[:B * T], ctx)


def test_token_limit(env):
    torch, _lib, lib = env
    UNSUPPORTED = -5   # MMISS_ERR_UNSUPPORTED (include/mmiss.h)
    qkv = torch.zeros(1026, 3 * 64, device="cuda", dtype=torch.bfloat16)
    ctx = torch.zeros(1026, 64, device="cuda", dtype=torch.bfloat16)
    assert lib.mmiss_dbg_attention(0, None, qkv.data_ptr(), ctx.data_ptr(), 1, 1026, 1, 0) == UNSUPPORTED
    assert b"1025" in lib.mmiss_last_error()
    assert lib.mmiss_dbg_attention_tiled(0, None, qkv.data_ptr(), ctx.data_ptr(), None, None, 1, 1026, 1, 0) == UNSUPPORTED
    c8 = torch.zeros(300, 64, device="cuda", dtype=torch.uint8)   # MXFP8 output is non-causal only
    assert lib.mmiss_dbg_attention_tiled(0, None, qkv.data_ptr(), None, c8.data_ptr(), c8.data_ptr(), 1, 289, 1, 1) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------- (b) the long kernel's bytes
@pytest.mark.parametrize("B,T,H,causal", [(2, 257, 3, 0), (1, 288, 2, 0), (2, 129, 2, 0), (2, 150, 2, 1), (1, 248, 3, 1)])
def test_equal_bytes_with_the_long_kernel(env, B, T, H, causal):
    """B * H < 256: mmiss_dbg_attention runs attention_long_kernel here, not the streaming kernel."""
    torch, _lib, lib = env
    qkv = _randn_qkv(torch, B, T, H, 31 * T + B + causal)
    long_ = torch.full((B * T + 1, H * 64), -7.0, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mmiss_dbg_attention(0, None, qkv.data_ptr(), long_.data_ptr(), B, T, H, causal))
    torch.cuda.synchronize()
    assert torch.equal(_tiled(env, qkv, B, T, H, causal), long_[:B * T])


# ---------------------------------------------------------------------------------------------- (c) rescale across seams
@pytest.mark.parametrize("causal", [0, 1])
def test_rescale_branch_across_chunk_seams(env, causal):
    """The offset of the online softmax is raised — and the output tile and the denominator rescaled — only when a score exceeds
    it by more than 2^8: a rare, data-dependent branch that needs an input that forces it. Every query's component 0 is 4; keys
    7, 40, 133, 300 and 520 carry spikes of 6, 24, 80, 180 and 400 there (logits +3, +12, +40, +90, +200): each of the four
    larger ones raises the maximum past the threshold, three of them in later chunks (keys 133, 300, 520: chunks 1, 2, 4), so
    the state rescaled is the one carried across the seams; key 7 must NOT rescale. Queries 400..419 have a second direction
    that only key 570 answers. Against the fp32 softmax of torch on the whole tensor."""
    torch, _lib, lib = env
    B, T, H = 2, 577, 3
    g = torch.Generator(device="cuda").manual_seed(577)
    qkv = torch.randn(B * T, 3 * H * 64, device="cuda", generator=g) * 0.5
    x = qkv.view(B, T, 3, H, 64)
    x[:, :, 0, :, 0] = 4.0
    for key, val in ((7, 6.0), (40, 24.0), (133, 80.0), (300, 180.0), (520, 400.0)):
        x[:, key, 1, :, 0] = val                 # logit += 4 * val / 8
    x[:, 400:420, 0, :, 1] = 8.0
    x[:, 570, 1, :, 1] = 600.0                   # +600 for queries 400..419 (past key 520's +200), ~0 for the others
    qkv = qkv.to(torch.bfloat16)
    ctx = _tiled(env, qkv, B, T, H, causal)
    ref, bound = _attn_ref(torch, qkv, B, T, H, bool(causal), with_bound=True)
    _assert_attention_close(torch, ctx, ref, bound)


# ---------------------------------------------------------------------------------------------- (d) every key counts
def test_577_keys_every_key_counts(env):
    """q, k ~ 0.3 N(0, 1), V = +-8 in every component: the scores are mild, so losing any single key moves every output by about
    8 / 577 = 1.4e-2, above the bound (at most 9e-3 here). The test checks that of its own reference first — the reference
    with ONE key removed (the first, the last of chunk 1, the first and another of chunk 2, the lone key of chunk 4) must be
    outside the bound nearly everywhere — then compares the last query (the odd last tile, one valid row) alone, then all."""
    torch, _lib, lib = env
    B, T, H = 2, 577, 3
    g = torch.Generator(device="cuda").manual_seed(577 + B)
    qkv = torch.randn(B * T, 3 * H * 64, device="cuda", generator=g) * 0.3
    x = qkv.view(B, T, 3, H, 64)
    x[:, :, 2] = torch.where(torch.rand(B, T, H, 64, device="cuda", generator=g) < 0.5, -8.0, 8.0)
    qkv = qkv.to(torch.bfloat16)
    ref, bound = _attn_ref(torch, qkv, B, T, H, False, with_bound=True)
    last = torch.arange(B, device="cuda") * T + (T - 1)
    xf = qkv.float().reshape(B, T, 3, H, 64)
    q = xf[:, :, 0].transpose(1, 2)
    for drop in (0, 256, 288, 300, 576):
        keep = [j for j in range(T) if j != drop]
        k, v = xf[:, keep, 1].transpose(1, 2), xf[:, keep, 2].transpose(1, 2)
        p = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, dim=-1)
        wrong = (p @ v).transpose(1, 2).reshape(B * T, H * 64)
        outside = (wrong - ref).abs() > bound
        assert outside.float().mean().item() > 0.9 and outside[last].float().mean().item() > 0.9, drop
    ctx = _tiled(env, qkv, B, T, H, 0)
    _assert_attention_close(torch, ctx[last], ref[last], bound[last])
    _assert_attention_close(torch, ctx, ref, bound)


# ---------------------------------------------------------------------------------------------- (e) MXFP8 output
@pytest.mark.parametrize("B,T,H", [(2, 577, 4), (1, 289, 2), (24, 577, 16)])
def test_tiled_attention_with_mxfp8_output(env, B, T, H):
    """The dequantised bytes against the SAME kernel's bf16 rows (held against torch above) up to the e4m3 rounding of a block —
    2^-4 of the block's largest magnitude — plus the bf16 rounding of the rows compared with."""
    from oracle import fp8_oracle as fo

    torch, _lib, lib = env
    qkv = _randn_qkv(torch, B, T, H, B * 1000 + T)
    ref = _tiled(env, qkv, B, T, H, 0).float().cpu().numpy()
    c8, cs = _tiled_mx(env, qkv, B, T, H)
    back = fo.mx_dequantize(c8.cpu().numpy(), fo.unpermute_scales(cs.cpu().numpy(), H * 64))
    gmax = np.abs(ref).reshape(B * T, -1, 32).max(axis=2).repeat(32, axis=1)
    assert np.isfinite(back).all()
    assert (np.abs(back - ref) <= gmax * (2.0 ** -4 * 1.01 + 2.0 ** -8) + 1e-6).all()
    # the product's MXFP8 route above 288 tokens is this kernel
    v8, vs = torch.full_like(c8, 0x5A), torch.full_like(cs, 0x5A)   # (the same fill: a row's unused scale bytes are not written)
    _lib.check(lib.mmiss_dbg_attention_mx(0, None, qkv.data_ptr(), v8.data_ptr(), vs.data_ptr(), B, T, H))
    torch.cuda.synchronize()
    assert torch.equal(v8, c8) and torch.equal(vs, cs)


def test_mxfp8_bytes_equal_the_long_kernels(env):
    """(2, 257, 4): 8 pairs, so mmiss_dbg_attention_mx runs attention_long_kernel's MXFP8 form."""
    from oracle import fp8_oracle as fo

    torch, _lib, lib = env
    B, T, H = 2, 257, 4
    qkv = _randn_qkv(torch, B, T, H, 2574)
    c8, cs = _tiled_mx(env, qkv, B, T, H)
    l8 = torch.full((B * T + 1, H * 64), 0x5A, device="cuda", dtype=torch.uint8)
    ls = torch.full((B * T + 1, fo.scale_row_bytes(H * 64)), 0x5A, device="cuda", dtype=torch.uint8)
    _lib.check(lib.mmiss_dbg_attention_mx(0, None, qkv.data_ptr(), l8.data_ptr(), ls.data_ptr(), B, T, H))
    torch.cuda.synchronize()
    assert torch.equal(c8, l8[:B * T]) and torch.equal(cs, ls[:B * T])

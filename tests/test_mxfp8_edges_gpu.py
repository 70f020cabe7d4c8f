"""Byte-exact edge tests of every MXFP8 producer and of the fp8 GEMMs' operand decode, on the MI355X.

The other fp8 tests feed Gaussian inputs and pass on statistics (> 99.9 % of scale bytes equal; within 2^-4 of the block maximum).
Here every producer gets inputs that make its pre-quantisation value known bit for bit, built from ONE catalogue of 32-value edge
blocks (tests/mx_edge_blocks.py: zeros and -0, the block maximum at each of the 32 positions, maxima at 446 / 448 / 450 * 2^k
where the scale byte steps, every e4m3 tie, blocks under the 1e-30 clamp, 3e38, both signs). tests/test_mxfp8_edges_cpu.py shows
that the reference stands on its own and that a skipped lane, a tie rule that is not to-even and an off-by-one scale each fail.

Comparison rule (_assert_mx_bytes): scale bytes (through unpermute_scales) and codes EQUAL oracle/fp8_oracle.py::mx_quantize of
the known rows, no element excluded; where the reference code is 0x00 / 0x80, either zero code passes. Rows behind the last row
and scale bytes no block owns keep their fill.

  producer                                   test                                       shapes                  how the launch takes it
  layernorm_mxfp8_kernel<false>              test_layernorm_f32_rows                    d 96 768 1024, M 19     dedicated entry point (f32 rows)
  layernorm_mxfp8_kernel<true>               test_layernorm_bf16_rows[96]               d 96, M 19              shape rule: d not in {512, 768, 1024}
  layernorm16_mxfp8_wide_kernel<1>           test_layernorm_bf16_rows[512]              d 512, M 19             shape rule
  layernorm16_mxfp8_wide_kernel<2, 768>      test_layernorm_bf16_rows[768]              d 768, M 19             shape rule
  layernorm16_mxfp8_1024_kernel              test_layernorm_bf16_rows[1024]             d 1024, M 19            shape rule
  attention_kernel<NKP, false, true>         test_attention_one_head_kernel             T 1 17 50 77 128, B 2, H 2   shape rule, proved: the pooled form is refused
  attention_heads_kernel<NKP, false, 2, true> test_attention_heads_kernel               the same                option att_hpb = 2, proved: the pooled form is accepted
  attention_long_kernel<NKP, false, true>    test_attention_long_kernel                 T 130 257 288, B 2, H 2 shape rule: 128 < T <= 288, B H = 4 < 256 pairs
  attention_stream_kernel<true>              test_attention_stream_kernel               T 257, B 3, H 2         option attention_stream_min_pairs = 1 (attention_stream_ok)
  attention_tiled_kernel<false, true>        test_attention_tiled_kernel                T 289 577, B 2, H 2     dedicated entry point
  gemm8_kernel<BM, QGELU_MXFP8>              test_qgelu_epilogue_tile_kernel            M bm and 2 bm, N 256, K 512   bm argument 128 / 160 / 192
  gemm256p8_kernel<QGELU_MXFP8> + ragged     test_qgelu_epilogue_persistent_kernel[512]   M 512 (300 valid), N 512, K 512   bm argument 256 + m_valid
  ... two scale groups of four K-tiles       test_qgelu_epilogue_persistent_kernel[1024]  the same, K 1024        bm argument 256 + m_valid
  operand decode, gemm8_kernel               test_operand_edges_tile_kernel             M 640 / 640 / 576, N 256, K 512   bm argument
  operand decode, gemm256p8_kernel           test_operand_edges_persistent_kernel       M 768 (768 and 556 valid)        bm argument 256 + m_valid

Shapes the issue names that an entry point does not admit: none.
"""
import contextlib

import numpy as np
import pytest

import mx_edge_blocks as mxb

pytestmark = pytest.mark.gpu

FILL = 0x5A


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib
    from oracle import fp8_oracle as fo

    lib = _lib.load()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch, _lib, lib, fo


@pytest.fixture(scope="module")
def cat():
    c = mxb.catalogue()
    return [n for n, _, _ in c], [v for _, _, v in c]


@contextlib.contextmanager
def _option(_lib, key, value, default):
    """The C API can set an option but not read one (include/mmiss_debug.h), so what is restored is the default the launcher itself
    names: att_hpb 0 (attention_kernels.h: attention_pick_hpb), attention_stream_min_pairs 256 (attention_stream.h:
    attention_stream_ok) — as tests/test_attention_heads_gpu.py::_forced does. tests/test_mxfp8_edges_cpu.py holds
    these two numbers against the sources, so a changed default in csrc/ fails here instead of leaking into later tests."""
    _lib.set_option(key, value)
    try:
        yield
    finally:
        _lib.set_option(key, default)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_mx_bytes(fo, got_q, got_e, y, what, name_of=None):
    """got_q uint8 [R, K] codes, got_e uint8 [R, K/32] scale bytes in natural order, y float32 [R, K] the known rows."""
    q, e = fo.mx_quantize(y, 32)
    bad_e = got_e != e
    zero = (q & 0x7F) == 0
    bad_q = (got_q != q) & ~(zero & ((got_q & 0x7F) == 0))
    if bad_e.any() or bad_q.any():
        lines = []
        for r, j in np.argwhere(bad_e | bad_q.reshape(q.shape[0], -1, 32).any(axis=2))[:6]:
            sl = slice(32 * j, 32 * j + 32)
            lines.append("row %d block %d%s: scale got %d want %d; codes differ at %s\n  y    %s\n  got  %s\n  want %s" % (
                r, j, " (%s)" % name_of(r, j) if name_of else "", got_e[r, j], e[r, j], np.nonzero(bad_q[r, sl])[0].tolist(),
                y[r, sl].tolist(), got_q[r, sl].tolist(), q[r, sl].tolist()))
        raise AssertionError("%s: %d scale bytes and %d codes differ from mx_quantize\n%s" % (what, int(bad_e.sum()), int(bad_q.sum()),
                                                                                            "\n".join(lines)))


# ================================================================================================ LayerNorm -> MXFP8, gamma = 0
def _layernorm_case(env, cat, bf16_rows, d):
    """gamma = 0, beta = one row of the catalogue layout: y = (x - mean) rstd 0 + beta = beta exactly for every finite x (a zero of
    either sign where beta is a zero). One launch per rotation r of the catalogue (beta = layout row r: block j holds case r + j),
    C launches of M = 19 rows (five workgroups of the four-rows form, two of the wide forms): every block index sees every case."""
    torch, _lib, lib, fo = env
    names, blocks = cat
    C, M, PAD = len(blocks), 19, 3
    beta = mxb.layout_rows(blocks, d)
    rng = np.random.default_rng(d)
    x = _dev(torch, (rng.standard_normal((M, d)) * 2 + 0.5).astype(np.float32))
    if bf16_rows:
        x = x.to(torch.bfloat16)
    assert float(x.float().var(dim=1).min()) > 1.0
    gam, bet = torch.zeros(d, device="cuda"), _dev(torch, beta)
    srb = fo.scale_row_bytes(d)
    out = torch.full((C, M + PAD, d), FILL, dtype=torch.uint8, device="cuda")
    osc = torch.full((C, M + PAD, srb), FILL, dtype=torch.uint8, device="cuda")
    fn = lib.mmiss_dbg_layernorm16_mxfp8 if bf16_rows else lib.mmiss_dbg_layernorm_mxfp8
    for r in range(C):
        _lib.check(fn(0, None, x.data_ptr(), gam.data_ptr(), bet[r].data_ptr(), out[r].data_ptr(), osc[r].data_ptr(), M, d, 1e-5))
    torch.cuda.synchronize()
    got, gs = out.cpu().numpy(), osc.cpu().numpy()
    assert (got[:, M:] == FILL).all() and (gs[:, M:] == FILL).all(), "rows behind row M - 1 were written"
    used = fo.scale_offset(np.arange(d // 32))
    pad = np.setdiff1d(np.arange(srb), used)
    assert (gs[:, :M][:, :, pad] == FILL).all(), "scale bytes no block owns were written"
    y = np.repeat(beta[:, None, :], M, axis=1).reshape(C * M, d)
    _assert_mx_bytes(fo, got[:, :M].reshape(C * M, d), gs[:, :M].reshape(C * M, srb)[:, used], y, "layernorm d=%d" % d,
                     lambda r, j: "%s, launch %d row %d" % (names[(r // M + j) % C], r // M, r % M))


@pytest.mark.parametrize("d", [96, 768, 1024])
def test_layernorm_f32_rows(env, cat, d):
    """layernorm_mxfp8_kernel<false>: eight lanes per block (xor 1 / 2 / 4); d = 96 leaves three of its four passes idle."""
    _layernorm_case(env, cat, False, d)


@pytest.mark.parametrize("d", [96, 512, 768, 1024])
def test_layernorm_bf16_rows(env, cat, d):
    """launch_layernorm_mxfp8 picks by shape: d = 96 the first form on bf16 rows, 512 / 768 the eight-columns form
    (four lanes per block; at 768 half of the second step's lanes idle), 1024 the sixteen-columns form (two lanes per block)."""
    _layernorm_case(env, cat, True, d)


# ================================================================================================ attention, one-hot softmax
def _chosen_keys(T):
    """key 0, key T - 1 (the odd last tile), one key in every 32-key step, one on each side of every 128-key chunk seam"""
    ks = {0, T - 1} | {32 * s + (11 * s + 5) % 32 for s in range((T + 31) // 32)} | {127, 128, 255, 256, 383, 384, 511, 512}
    return sorted(k for k in ks if k < T)


def _one_hot_input(torch, blocks, B, T, H, launch):
    """q = 4 in all 64 components; the chosen key of each (item, head) = 6 in all 64, every other key 0: the chosen raw score is
    1536 (192 after the 1/8), the others 0, so every other probability is exp(-192) = 0 in f32 and the chosen one is 1. V of the
    chosen key = catalogue blocks i and i + 1 for pair number i (counted over all launches): over 2 C pairs every block passes
    through both 32-column halves of a head (two lane groups each) and, C being odd and B H even, through an even and an odd head.
    Every other V value is +-(4 .. 12): a leak shows. -> qkv, y float32 [B, H * 64]"""
    C = len(blocks)
    rng = np.random.default_rng(1000 * T + launch)
    x = np.zeros((B, T, 3, H, 64), np.float32)
    x[:, :, 0] = 4.0
    x[:, :, 2] = rng.integers(32, 97, (B, T, H, 64)) / 8.0 * rng.choice([-1.0, 1.0], (B, T, H, 64))
    keys = _chosen_keys(T)
    y = np.empty((B, H * 64), np.float32)
    what = []
    for b in range(B):
        for h in range(H):
            i = launch * B * H + b * H + h
            key = keys[i % len(keys)]
            x[b, key, 1, h] = 6.0
            x[b, key, 2, h] = np.concatenate([blocks[i % C], blocks[(i + 1) % C]])
            y[b, h * 64:(h + 1) * 64] = x[b, key, 2, h]
            what.append((key, i % C))
    qkv = _dev(torch, x.reshape(B * T, 3 * H * 64)).to(torch.bfloat16)
    return qkv, y, what


def _one_hot_attention(env, cat, B, T, H, tiled=False, last_query_alone=False):
    """Over ceil(2 C / (B H)) launches (51 at B H = 4) every catalogue block passes through both halves of an even and of an odd
    head, and the chosen key cycles through _chosen_keys(T). Per launch: first the PRECONDITION — the bf16-output form of the same kernel returns exactly the chosen V row
    for every query (a known answer, not the kernel under test) — then ctx8 / ctx_scale of every query row equal mx_quantize of it."""
    torch, _lib, lib, fo = env
    names, blocks = cat
    C, d = len(blocks), H * 64
    srb = fo.scale_row_bytes(d)
    used = fo.scale_offset(np.arange(d // 32))
    pad = np.setdiff1d(np.arange(srb), used)
    assert C % 2 == 1 and (B * H) % 2 == 0 and H % 2 == 0
    for launch in range(-(-2 * C // (B * H))):
        qkv, y, what = _one_hot_input(torch, blocks, B, T, H, launch)
        ctx = torch.full((B * T + 1, d), -7.0, device="cuda", dtype=torch.bfloat16)
        c8 = torch.full((B * T + 1, d), FILL, device="cuda", dtype=torch.uint8)
        cs = torch.full((B * T + 1, srb), FILL, device="cuda", dtype=torch.uint8)
        if tiled:
            _lib.check(lib.mmiss_dbg_attention_tiled(0, None, qkv.data_ptr(), ctx.data_ptr(), None, None, B, T, H, 0))
            _lib.check(lib.mmiss_dbg_attention_tiled(0, None, qkv.data_ptr(), None, c8.data_ptr(), cs.data_ptr(), B, T, H, 0))
        else:
            _lib.check(lib.mmiss_dbg_attention(0, None, qkv.data_ptr(), ctx.data_ptr(), B, T, H, 0))
            _lib.check(lib.mmiss_dbg_attention_mx(0, None, qkv.data_ptr(), c8.data_ptr(), cs.data_ptr(), B, T, H))
        torch.cuda.synchronize()
        assert (ctx[B * T] == -7.0).all() and (c8[B * T] == FILL).all() and (cs[B * T] == FILL).all(), "the row behind the last item was written"
        want = _dev(torch, y)[:, None, :].expand(B, T, d)
        got16 = ctx[:B * T].float().reshape(B, T, d)
        assert torch.equal(got16, want), ("PRECONDITION: the bf16 rows are not the chosen V row", T, launch, what,
                                          (got16 != want).nonzero()[:6].tolist())
        gq = c8[:B * T].cpu().numpy()
        gs = cs[:B * T].cpu().numpy()
        assert (gs[:, pad] == FILL).all(), "scale bytes no block owns were written"
        yy = np.repeat(y[:, None, :], T, axis=1).reshape(B * T, d)
        name_of = lambda r, j: "%s, launch %d item %d query %d key %d" % (names[(what[(r // T) * H + j // 2][1] + j % 2) % C], launch, r // T,
                                                                         r % T, what[(r // T) * H + j // 2][0])
        if last_query_alone:
            last = np.arange(B) * T + T - 1
            _assert_mx_bytes(fo, gq[last], gs[last][:, used], yy[last], "attention T=%d, the last query" % T,
                             lambda r, j: name_of(last[r], j))
        _assert_mx_bytes(fo, gq, gs[:, used], yy, "attention T=%d" % T, name_of)


def _pooled_form_accepted(env, B, T, H):
    """mmiss_dbg_attention_pooled accepts a shape exactly where mmiss_dbg_attention / _mx run attention_heads_kernel there
    (attention_pick_hpb > 1; tests/test_attention_heads_gpu.py::_forced)."""
    torch, _lib, lib, fo = env
    qkv = torch.zeros(B * T, 3 * H * 64, device="cuda", dtype=torch.bfloat16)
    rows = torch.arange(B, device="cuda", dtype=torch.int32) * T
    out = torch.zeros(B, H * 64, device="cuda", dtype=torch.bfloat16)
    status = lib.mmiss_dbg_attention_pooled(0, None, qkv.data_ptr(), rows.data_ptr(), out.data_ptr(), B, T, H, 0)
    torch.cuda.synchronize()
    return status == 0


T_SHORT = [1, 17, 50, 77, 128]


@pytest.mark.parametrize("T", T_SHORT)
def test_attention_one_head_kernel(env, cat, T):
    """attention_kernel<ceil(T / 32), false, true>: B H = 4 pairs are far below the 512 workgroups of the several-heads form."""
    assert not _pooled_form_accepted(env, 2, T, 2)
    _one_hot_attention(env, cat, 2, T, 2)


@pytest.mark.parametrize("T", T_SHORT)
def test_attention_heads_kernel(env, cat, T):
    """attention_heads_kernel<ceil(T / 32), false, 2, true>, forced with option att_hpb = 2."""
    torch, _lib, lib, fo = env
    with _option(_lib, "att_hpb", 2, 0):
        assert _pooled_form_accepted(env, 2, T, 2)
        _one_hot_attention(env, cat, 2, T, 2)


@pytest.mark.parametrize("T", [130, 257, 288])
def test_attention_long_kernel(env, cat, T):
    """attention_long_kernel<5 / 9 / 9, false, true>: the online softmax raises its offset to the chosen key's score (more than 2^8
    above), which clears what came before (alpha = 0); l = 1."""
    _one_hot_attention(env, cat, 2, T, 2)


def test_attention_stream_kernel(env, cat):
    """attention_stream_kernel<true> at B H = 6 pairs: attention_stream_ok is T == 257, non-causal and B H >= option
    attention_stream_min_pairs (default 256), lowered to 1 here for the bf16 precondition and the MXFP8 launch alike. The 257th
    query is merged from nine partial softmaxes in a separate epilogue: compared on its own first."""
    torch, _lib, lib, fo = env
    with _option(_lib, "attention_stream_min_pairs", 1, 256):
        _one_hot_attention(env, cat, 3, 257, 2, last_query_alone=True)


@pytest.mark.parametrize("T", [289, 577])
def test_attention_tiled_kernel(env, cat, T):
    """attention_tiled_kernel<false, true> through its own entry point: chosen keys in every 128-key chunk and on both sides of
    every chunk seam (127 | 128, 255 | 256, ...), the lone key of the last chunk among them (288, 576)."""
    _one_hot_attention(env, cat, 2, T, 2, tiled=True)


# ================================================================================================ one-hot fp8 GEMMs
# ------------------------------------------------------------------------------------------------ QuickGELU -> MXFP8 (64-column scales)
def _assert_qgelu_bytes(fo, got_q, got_e, pre, what):
    """The banded rule. Reference: float64 QuickGELU of the exactly known pre-activation, then mx_quantize(., 64). Scale bytes equal
    (the cases keep every block maximum 2^-10 away from 448 * 2^k: tests/test_mxfp8_edges_cpu.py), both bytes of a 64-column group
    equal; codes equal, except where the exact scaled value lies within relative 2^-16 (128 f32 ulps: a fast exp2 and a reciprocal
    are a few) of a code midpoint: one code step there. That share is capped at 1 %. Either zero code passes for a zero.
    For the inputs of mx_edge_blocks.qgelu_case the band is EMPTY (share 0.0, printed here and asserted on the CPU): every code of
    these tests is held to equality, and the one-step branch is there for a case whose values change."""
    y = mxb.qgelu_reference(pre)
    q, e = fo.mx_quantize(y.astype(np.float32), 64)
    assert (got_e[:, ::2] == got_e[:, 1::2]).all(), what
    assert (got_e == e).all(), (what, "scale bytes", np.argwhere(got_e != e)[:6].tolist())
    near = mxb.near_midpoint(y, e)
    print(what, "share of elements within 2^-16 of a code midpoint: %.5f" % near.mean())
    assert near.mean() <= mxb.QGELU_CAP
    gm, qm = (got_q & 0x7F).astype(int), (q & 0x7F).astype(int)
    zero = (gm == 0) & (qm == 0)
    equal = (got_q == q) | zero
    assert equal[~near].all(), (what, "codes", int((~equal & ~near).sum()), np.argwhere(~equal & ~near)[:6].tolist())
    step = (np.abs(gm - qm) <= 1) & ((((got_q ^ q) & 0x80) == 0) | (np.minimum(gm, qm) == 0))
    assert step[near].all(), (what, "codes next to a midpoint", np.argwhere(~step & near)[:6].tolist())


@pytest.mark.parametrize("bm,blocks_m", [(128, 1), (128, 2), (160, 1), (160, 2), (192, 1), (192, 2)])
def test_qgelu_epilogue_tile_kernel(env, bm, blocks_m):
    """gemm8_kernel<bm, QGELU_MXFP8>, M = bm and 2 bm, N = 256, K = 512: one-hot A rows select column m of W8 (mx_edge_blocks.qgelu_case),
    so the 64-column maximum of row m sits at column m % 64 — lanes fr, fr + 16, fr + 32, fr + 48 and each of a lane's 16 values."""
    torch, _lib, lib, fo = env
    M, N, K = bm * blocks_m, 256, 512
    A8, As, W8, bias, pre = mxb.qgelu_case(M, N, K)
    srb = fo.scale_row_bytes(N)
    out = torch.full((M + 1, N), FILL, dtype=torch.uint8, device="cuda")
    osc = torch.full((M + 1, srb), FILL, dtype=torch.uint8, device="cuda")
    A8d, Asd, W8d, bd = _dev(torch, A8), _dev(torch, fo.permute_scales(As)), _dev(torch, W8), _dev(torch, bias)
    ws = torch.ones(N, device="cuda")
    _lib.check(lib.mmiss_dbg_gemm8(0, None, 1, bm, A8d.data_ptr(), Asd.data_ptr(), W8d.data_ptr(), ws.data_ptr(), bd.data_ptr(),
                                   out.data_ptr(), osc.data_ptr(), M, N, K))
    torch.cuda.synchronize()
    gs = osc.cpu().numpy()
    used = fo.scale_offset(np.arange(N // 32))
    assert (out[M] == FILL).all() and (gs[M] == FILL).all() and (gs[:M, np.setdiff1d(np.arange(srb), used)] == FILL).all()
    _assert_qgelu_bytes(fo, out[:M].cpu().numpy(), gs[:M][:, used], pre, "gemm8 bm=%d M=%d" % (bm, M))


@pytest.mark.parametrize("K", [512, 1024])
def test_qgelu_epilogue_persistent_kernel(env, K):
    """gemm256p8_kernel<QGELU_MXFP8>, M = 512 with 300 valid rows, N = 512: rows 0 .. 255 leave through the tile epilogue, rows
    256 .. 299 through the ragged pass (its own maxima over lane groups), rows 300 .. 510 are padding and keep their fill (row
    M - 1 is the dump row). K = 512 is one scale group of four K-tiles, K = 1024 two: the scale ring changes parity inside the
    tile, and the ragged pass reads a second scale dword per row."""
    torch, _lib, lib, fo = env
    M, mv, N = 512, 300, 512
    A8, As, W8, bias, pre = mxb.qgelu_case(M, N, K)
    srb = fo.scale_row_bytes(N)
    out = torch.full((M, N), FILL, dtype=torch.uint8, device="cuda")
    osc = torch.full((M, srb), FILL, dtype=torch.uint8, device="cuda")
    A8d, Asd, W8d, bd = _dev(torch, A8), _dev(torch, fo.permute_scales(As)), _dev(torch, W8), _dev(torch, bias)
    ws = torch.ones(N, device="cuda")
    _lib.check(lib.mmiss_dbg_gemm8(0, None, 1, 256 + mv, A8d.data_ptr(), Asd.data_ptr(), W8d.data_ptr(), ws.data_ptr(), bd.data_ptr(),
                                   out.data_ptr(), osc.data_ptr(), M, N, K))
    torch.cuda.synchronize()
    assert (out[mv:M - 1] == FILL).all() and (osc[mv:M - 1] == FILL).all(), "padding rows were written"
    used = fo.scale_offset(np.arange(N // 32))
    assert srb == used.size                                                     # (N = 512: every scale byte of a row is owned)
    for lo, hi, part in ((0, 256, "tile rows"), (256, mv, "ragged rows")):
        _assert_qgelu_bytes(fo, out[lo:hi].cpu().numpy(), osc[lo:hi].cpu().numpy()[:, used], pre[lo:hi], "gemm256p8 K=%d %s" % (K, part))


# ------------------------------------------------------------------------------------------------ operand edges, exact
SCALES = (1, 20, 100, 127, 150, 200, 250)


def _operand_case(fo, M, N, K, s, zero_rows=8):
    """Row m: ONE non-zero activation code at column k_m = m % K — the codes cycle through all 126 finite magnitudes with both signs,
    subnormals and +-448 included — in a block of scale byte s; every other block of the row holds zero codes (0x00 and 0x80) under
    arbitrary scale bytes 0 .. 254. The last `zero_rows` rows are EXTRA rows (M - zero_rows >= K, so they displace no one-hot row
    and every k position is hit) of all zero codes under scale byte 0: the state of zero-allocated padding rows. W8: every finite
    code. -> A8, As (natural), W8, want float64 [M, N] = decode(a) decode(W8[n, k_m]), ok bool [M, N]: the f32 accumulator
    a w 2^(s - 127) is zero or normal and finite (only there is the result exactly a w), km int [M] (-1 for the zero rows)."""
    assert M - zero_rows >= K
    rng = np.random.default_rng(10 * K + s)
    finite = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    nonzero = np.array([c for c in range(256) if c & 0x7F not in (0, 0x7F)], np.uint8)
    assert nonzero.size == 252
    W8 = rng.choice(finite, size=(N, K))
    A8 = rng.choice(np.array([0x00, 0x80], np.uint8), size=(M, K))
    As = rng.integers(0, 255, size=(M, K // 32)).astype(np.uint8)
    m = np.arange(M)
    km = m % K
    code = nonzero[(m + 37 * s) % 252]
    A8[m, km] = code
    As[m, km // 32] = s
    A8[M - zero_rows:] = rng.choice(np.array([0x00, 0x80], np.uint8), size=(zero_rows, K))
    As[M - zero_rows:] = 0
    a = fo.e4m3_decode(code).astype(np.float64)
    a[M - zero_rows:] = 0.0
    want = a[:, None] * fo.e4m3_decode(W8).astype(np.float64).T[km]
    acc = np.abs(want) * 2.0 ** (s - 127)
    ok = (acc == 0) | ((acc >= 2.0 ** -126) & (acc < 2.0 ** 128))
    assert (np.count_nonzero(A8 & 0x7F, axis=1) == (m < M - zero_rows)).all()
    return A8, As, W8, want, ok, np.where(m < M - zero_rows, km, -1)


def _run_operand_case(env, epi, bm, M, N, K, mv):
    """out = acc * wscale + 0 with wscale = 2^(127 - s): a product of two 4-bit significands, exact in bf16 (8 bits) and in f32, and
    the ONE non-zero product of an MFMA row loses nothing to alignment — so the output equals a w exactly (a zero of either sign
    where a w = 0). Excluded: accumulators that would be f32 subnormals (s = 1 and |a w| < 1: 38 % of that slice) or beyond the f32
    range (s = 250 and |a w| >= 32: 32 % of that slice); counted and printed; the other five slices are compared whole."""
    torch, _lib, lib, fo = env
    for s in SCALES:
        A8, As, W8, want, ok, km = _operand_case(fo, M, N, K, s)
        assert set(km[:mv].tolist()) - {-1} == set(range(K)), "a k position never carries the non-zero code"
        A8d, Asd, W8d = _dev(torch, A8), _dev(torch, fo.permute_scales(As)), _dev(torch, W8)
        ws = torch.full((N,), 2.0 ** (127 - s), device="cuda")
        bias = torch.zeros(N, device="cuda")
        out = torch.zeros((M, N), dtype=torch.float32 if epi == 2 else torch.bfloat16, device="cuda")
        dummy = torch.zeros((M, fo.scale_row_bytes(N)), dtype=torch.uint8, device="cuda")
        _lib.check(lib.mmiss_dbg_gemm8(0, None, epi, bm, A8d.data_ptr(), Asd.data_ptr(), W8d.data_ptr(), ws.data_ptr(), bias.data_ptr(),
                                       out.data_ptr(), dummy.data_ptr(), M, N, K))
        torch.cuda.synchronize()
        got = out.float().cpu().numpy().astype(np.float64)[:mv]
        ok, want = ok[:mv], want[:mv]
        print("epi %d bm %d scale byte %d: %.1f %% of the elements compared" % (epi, bm, s, 100 * ok.mean()))
        assert ok.all() or s in (1, 250)
        assert ok.mean() > 0.6
        bad = (got != want) & ok
        assert not bad.any(), ("epi %d bm %d scale byte %d" % (epi, bm, s), int(bad.sum()),
                               [(int(r), int(c), got[r, c], want[r, c]) for r, c in np.argwhere(bad)[:6]])


@pytest.mark.parametrize("epi", [0, 2])
@pytest.mark.parametrize("bm", [128, 160, 192])
def test_operand_edges_tile_kernel(env, epi, bm):
    """gemm8_kernel<bm, BIAS_BF16 / BIAS_RESID_F32 on old = 0>: the smallest multiple of bm with M >= K + 8 = 520 (640 / 640 / 576:
    a one-hot row for every k position and eight zero rows behind them), N = 256."""
    M = -(-520 // bm) * bm
    _run_operand_case(env, epi, bm, M, 256, 512, M)


@pytest.mark.parametrize("epi", [0, 3])
@pytest.mark.parametrize("mv", [768, 556])
def test_operand_edges_persistent_kernel(env, epi, mv):
    """gemm256p8_kernel<BIAS_BF16 / BIAS_RESID_BF16 on old = 0> (it has no f32 residual form): M = 768 whole (rows 0 .. 511 carry the
    non-zero code at every k position, the last K-tile and scale group included; the eight zero rows are rows 760 .. 767), and with
    556 valid rows (rows 0 .. 511 through the tile stream, rows 512 .. 555 through the ragged pass, whose K-tiles are dealt over
    eight waves: seven exact zeros added to the one product). The scale ring of the tile stream sees scale bytes 0 .. 254 beside
    the one that counts."""
    _run_operand_case(env, epi, 256 + mv, 768, 256, 512, mv)

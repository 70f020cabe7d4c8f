"""The pruned last layer without its gather (api_encoder.hip run_layers): the several-heads attention kernel computes only the
16-query tile that holds an item's pooled row and stores that row into the compact buffer; the skinny out-projection reads its
old residual row through the row map. Both against the launches they replace, bit for bit, and the whole tail inside a tiny
encoder against the unpruned computation. The pre-LayerNorm that makes the CLS rows itself and keeps its f32 rows to itself
(layernorm_stats_kernel<true>) against the three-launch form."""
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


@pytest.fixture()
def heads_kernel(env):
    """Force the several-heads attention kernel (two heads per workgroup) whatever the batch: the pooled-query form exists for
    that kernel only, and the small batches of these tests would otherwise run one (item, head) per workgroup."""
    _, _lib, _ = env
    _lib.set_option("att_hpb", 2)
    yield
    _lib.set_option("att_hpb", 0)


def _pool_rows(torch, B, T, causal):
    """Global token row of every item's pooled query. The vision tower pools row 0; the text tower any row: first tile, second
    tile (where T has one), the last row."""
    if not causal:
        return torch.arange(B, device="cuda", dtype=torch.int32) * T
    picks = [0, 5, min(16, T - 1), T - 1, min(31, T - 1), T // 2]
    return torch.tensor([b * T + picks[b % len(picks)] for b in range(B)], device="cuda", dtype=torch.int32)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("B", [3, 37])
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("T", [17, 50, 64])
def test_pooled_query_attention_equals_full_attention_and_gather(env, heads_kernel, T, H, B, causal):
    torch, _lib, lib = env
    g = torch.Generator(device="cuda").manual_seed(1000 * T + 10 * H + B + causal)
    qkv = torch.randn(B * T, 3 * H * 64, device="cuda", generator=g).to(torch.bfloat16)
    rows = _pool_rows(torch, B, T, causal)
    full = torch.zeros(B * T, H * 64, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mmiss_dbg_attention(0, None, qkv.data_ptr(), full.data_ptr(), B, T, H, causal))
    got = torch.full((B + 1, H * 64), -7.0, device="cuda", dtype=torch.bfloat16)   # one sentinel row behind the B rows
    _lib.check(lib.mmiss_dbg_attention_pooled(0, None, qkv.data_ptr(), rows.data_ptr(), got.data_ptr(), B, T, H, causal))
    torch.cuda.synchronize()
    want = full[rows.long()]
    diff = got[:B].view(torch.int16) != want.view(torch.int16)
    assert not diff.any(), (int(diff.sum()), diff.nonzero()[:8].tolist())
    assert (got[B] == -7.0).all()


def test_pooled_query_attention_is_refused_where_the_heads_kernel_does_not_run(env):
    torch, _lib, lib = env
    qkv = torch.zeros(3 * 50, 3 * 2 * 64, device="cuda", dtype=torch.bfloat16)
    rows = torch.arange(3, device="cuda", dtype=torch.int32) * 50
    out = torch.zeros(3, 2 * 64, device="cuda", dtype=torch.bfloat16)
    assert lib.mmiss_dbg_attention_pooled(0, None, qkv.data_ptr(), rows.data_ptr(), out.data_ptr(), 3, 50, 2, 0) != 0


@pytest.mark.parametrize("N,K", [(768, 768), (128, 128)])
@pytest.mark.parametrize("B", [1, 7, 130])
def test_row_mapped_out_projection_equals_gather_then_gemm(env, B, N, K):
    """out = f32(xb[rowmap[m]]) + A W^T + bias against the gathered, widened rows as the in-place residual of launch_gemm."""
    torch, _lib, lib = env
    T = 50
    g = torch.Generator(device="cuda").manual_seed(7 * B + N)
    A = torch.randn(B, K, device="cuda", generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g)
    xb = torch.randn(B * T, N, device="cuda", generator=g).to(torch.bfloat16)
    rowmap = (torch.arange(B, device="cuda", dtype=torch.int32) * T + torch.arange(B, device="cuda", dtype=torch.int32) % T)
    want = xb[rowmap.long()].float().contiguous()
    _lib.check(lib.mmiss_dbg_gemm(0, None, _lib.EPI_BIAS_RESID_F32, 128, A.data_ptr(), W.data_ptr(), want.data_ptr(),
                                  bias.data_ptr(), None, B, N, K, 0, 0))
    got = torch.full((B + 1, N), float("nan"), device="cuda")
    _lib.check(lib.mmiss_dbg_gemm_resid_rows(0, None, A.data_ptr(), W.data_ptr(), got.data_ptr(), bias.data_ptr(), xb.data_ptr(),
                                             rowmap.data_ptr(), B, N, K))
    torch.cuda.synchronize()
    assert torch.equal(got[:B].view(torch.int32), want.view(torch.int32))
    assert torch.isnan(got[B]).all()


def _kernels_of(_lib, fn):
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        out = fn()
    finally:
        _lib.prof_enable(False)
    return out, {p["kernel"]: p["launches"] for p in _lib.prof_read()}


@pytest.fixture(scope="module")
def tiny_pair():
    import mmiss_amd  # noqa: F401
    from mmiss_amd.encoder import ClipEncoder, ClipShape
    from oracle import clip_oracle as co

    W = co.init_weights(co.TINY, seed=0)
    full = ClipEncoder(ClipShape.from_any(co.TINY), max_batch_image=130, max_batch_text=130)
    full.record_taps(True)   # taps = every row of every layer: nothing pruned
    full.load_state_dict(W)
    pruned = ClipEncoder(ClipShape.from_any(co.TINY), max_batch_image=130, max_batch_text=130)
    pruned.load_state_dict(W)
    yield full, pruned, co
    full.close()
    pruned.close()


@pytest.mark.parametrize("B", [7, 130])
def test_tiny_encoder_pooled_tail_matches_the_unpruned_computation(env, heads_kernel, tiny_pair, B):
    """As test_last_layer_pruning_matches_full_computation: identical arithmetic on both sides (separate LayerNorm kernels), so
    the pruned tail — now the pooled-query attention and the row-mapped out-projection — reproduces the full computation to
    atol 1e-6; the gather launch is gone from the call, and comes back under option pooled_tail = 0 with the same bits."""
    torch, _lib, lib = env
    full, pruned, co = tiny_pair
    s = co.TINY
    rng = np.random.Generator(np.random.Philox(770 + B))
    px = rng.standard_normal((B, 3, s.v_image, s.v_image), dtype=np.float32)
    ids = co.synthetic_text_ids(B, s.t_ctx, s.t_vocab, s.eos_token_id, seed=78 + B)
    _lib.set_option("skinny_fold", 0)
    try:
        img, kern_i = _kernels_of(_lib, lambda: pruned.encode_image(px))
        txt, kern_t = _kernels_of(_lib, lambda: pruned.encode_text(ids))
        for kern, layers in ((kern_i, s.v_layers), (kern_t, s.t_layers)):
            assert "gather_pooled" not in kern and kern.get("attention", 0) == layers, kern
            assert kern.get("gemm_skinny_bias_resid", 0) >= 2, kern   # the pooled rows' out-projection and FC2
        ref_i, ref_t = full.encode_image(px), full.encode_text(ids)
        print("pooled tail vs unpruned, B =", B, "max |d| image", np.abs(img - ref_i).max(), "text", np.abs(txt - ref_t).max())
        np.testing.assert_allclose(img, ref_i, atol=1e-6)
        np.testing.assert_allclose(txt, ref_t, atol=1e-6)
        _lib.set_option("pooled_tail", 0)
        try:
            img0, kern0 = _kernels_of(_lib, lambda: pruned.encode_image(px))
            txt0 = pruned.encode_text(ids)
        finally:
            _lib.set_option("pooled_tail", 1)
        assert kern0.get("gather_pooled", 0) == 1, kern0
        np.testing.assert_array_equal(img.view(np.uint32), img0.view(np.uint32))
        np.testing.assert_array_equal(txt.view(np.uint32), txt0.view(np.uint32))
    finally:
        _lib.set_option("skinny_fold", 1)


def test_lean_prelayernorm_equals_the_three_launch_form(env, heads_kernel, tiny_pair):
    """The bf16 residual stream forced onto a tiny call (folded LayerNorm from 0 rows): the pre-LayerNorm makes the CLS rows itself
    and writes no f32 rows; option prelayernorm_lean = 0 brings cls_rows_kernel and the write-back back. Same embeddings, bit for bit."""
    torch, _lib, lib = env
    _, pruned, co = tiny_pair
    s = co.TINY
    rng = np.random.Generator(np.random.Philox(4242))
    px = rng.standard_normal((9, 3, s.v_image, s.v_image), dtype=np.float32) * 2 + 0.5
    _lib.set_option("ln_fold_min_rows", 0)
    try:
        lean, kern = _kernels_of(_lib, lambda: pruned.encode_image(px))
        _lib.set_option("prelayernorm_lean", 0)
        try:
            ref, kern0 = _kernels_of(_lib, lambda: pruned.encode_image(px))
        finally:
            _lib.set_option("prelayernorm_lean", 1)
    finally:
        _lib.set_option("ln_fold_min_rows", 6000)
    assert "cls_rows" not in kern and kern0.get("cls_rows", 0) == 1, (kern, kern0)
    assert "gather_pooled" not in kern, kern
    np.testing.assert_array_equal(lean.view(np.uint32), ref.view(np.uint32))
    ref32 = co.embed_images(px, co.init_weights(s, seed=0), s)
    assert (1 - (lean * ref32).sum(1)).max() < 1e-3

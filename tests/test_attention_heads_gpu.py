"""attention_heads_kernel (attention_kernels.h: several heads of one item per workgroup, T <= 128 — the kernel every layer of both
towers runs at batch 256) against torch's fp32 softmax on the whole tensor, under the per-element bound of
tests/test_kernels_gpu.py::_attn_ref. Every instantiation <NKP, CAUSAL, HPB, MXOUT, POOLED> the launchers can pick:

  NKP      = ceil(T / 32): 1 (T = 1, 15, 16, 17, 32), 2 (33, 50, 64), 3 (65, 77, 96), 4 (97, 128)
  HPB      = 2, 3, 4, 6 forced through option att_hpb (H = 12: several groups per item; H = HPB: one), or picked by the batch
  CAUSAL   = both
  MXOUT    = test_mxfp8_output_is_bit_identical_to_the_one_head_kernel (non-causal only: the launcher has no causal MXFP8 form)
  POOLED   = test_pooled_query_* (bf16 only: the kernel static_asserts !(POOLED && MXOUT))

The small batches of these tests would otherwise run attention_kernel (one head per workgroup), which is what the shapes of
test_kernels_gpu.py::test_attention reach."""
import contextlib

import pytest

from test_kernels_gpu import _attn_ref   # the reference and its bound, unchanged

pytestmark = pytest.mark.gpu

T_ALL = [1, 15, 16, 17, 32, 33, 50, 64, 65, 77, 96, 97, 128]   # all four NKP, the 16-query and 32-key edges, second query tiles from 65
HPBS = [2, 3, 4, 6]
B_SMALL = 3


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch, _lib, lib


@contextlib.contextmanager
def _forced(env, hpb, B, T, H):
    """Option att_hpb for the launches inside: 1 = attention_kernel, 2/3/4/6 = attention_heads_kernel<.., HPB, ..>; 0 (automatic)
    after. That the forcing took at (B, T, H) is proved on the spot: mmiss_dbg_attention_pooled accepts the shape exactly where
    attention_pick_hpb returns more than 1, i.e. where mmiss_dbg_attention runs attention_heads_kernel."""
    torch, _lib, lib = env
    _lib.set_option("att_hpb", hpb)
    try:
        qkv = torch.zeros(B * T, 3 * H * 64, device="cuda", dtype=torch.bfloat16)
        rows = torch.arange(B, device="cuda", dtype=torch.int32) * T
        out = torch.zeros(B, H * 64, device="cuda", dtype=torch.bfloat16)
        status = lib.mmiss_dbg_attention_pooled(0, None, qkv.data_ptr(), rows.data_ptr(), out.data_ptr(), B, T, H, 0)
        torch.cuda.synchronize()
        assert (status == 0) == (hpb > 1), (hpb, B, T, H, status)
        yield
    finally:
        _lib.set_option("att_hpb", 0)


def _qkv(torch, B, T, H, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B * T, 3 * H * 64, device="cuda", generator=g) * scale).to(torch.bfloat16)


def _attend(env, qkv, B, T, H, causal):
    """mmiss_dbg_attention into a buffer with one sentinel row behind the B * T rows, which must come back untouched."""
    torch, _lib, lib = env
    ctx = torch.full((B * T + 1, H * 64), -7.0, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mmiss_dbg_attention(0, None, qkv.data_ptr(), ctx.data_ptr(), B, T, H, causal))
    torch.cuda.synchronize()
    assert (ctx[B * T] == -7.0).all(), "the row behind the last item was written"
    return ctx[:B * T]


def _attend_mx(env, qkv, B, T, H):
    from oracle import fp8_oracle as fo

    torch, _lib, lib = env
    c8 = torch.full((B * T + 1, H * 64), 0x5A, device="cuda", dtype=torch.uint8)
    cs = torch.full((B * T + 1, fo.scale_row_bytes(H * 64)), 0x5A, device="cuda", dtype=torch.uint8)
    _lib.check(lib.mmiss_dbg_attention_mx(0, None, qkv.data_ptr(), c8.data_ptr(), cs.data_ptr(), B, T, H))
    torch.cuda.synchronize()
    assert (c8[B * T] == 0x5A).all() and (cs[B * T] == 0x5A).all(), "the row behind the last item was written"
    return c8[:B * T], cs[:B * T]


def _heads_outside(torch, ctx, ref, bound, H):
    """{head: (elements outside the bound, largest excess)} — a K/V image swapped between the heads of a group names itself."""
    assert torch.isfinite(ctx.float()).all()
    excess = ((ctx.float() - ref).abs() - bound).reshape(-1, H, 64)
    bad = (excess > 0).sum(dim=(0, 2))
    return {h: (int(bad[h]), float(excess[:, h].max())) for h in range(H) if bad[h] > 0}


def _h_of(hpb):
    return (12, hpb)   # several groups per item; one group


# ---------------------------------------------------------------------------------------------- (a) every instantiation
@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("hpb", HPBS)
def test_every_instantiation_against_fp32_softmax(env, hpb, causal, T):
    """attention_heads_kernel<ceil(T / 32), causal, hpb, false, false> at B = 3."""
    torch, _lib, lib = env
    for H in _h_of(hpb):
        qkv = _qkv(torch, B_SMALL, T, H, 10000 * hpb + 100 * T + 10 * causal + H)
        with _forced(env, hpb, B_SMALL, T, H):
            ctx = _attend(env, qkv, B_SMALL, T, H, causal)
        ref, bound = _attn_ref(torch, qkv, B_SMALL, T, H, bool(causal), with_bound=True)
        bad = _heads_outside(torch, ctx, ref, bound, H)
        assert not bad, (H, bad)


# ---------------------------------------------------------------------------------------------- (b) automatic choice
@pytest.mark.parametrize("B,T,H,causal", [(256, 50, 12, 0), (256, 77, 8, 1),     # the product shapes: <2, false, 4>, <3, true, 4>
                                          (512, 17, 2, 0), (512, 17, 2, 1),      # B * (H / c) >= 512 at the smallest B: HPB = 2
                                          (512, 17, 3, 0), (512, 17, 3, 1),      # 3
                                          (512, 17, 4, 0), (512, 17, 4, 1),      # 4
                                          (512, 17, 6, 0), (512, 17, 6, 1)])     # 6
def test_automatic_choice_runs_the_heads_kernel_and_matches_fp32_softmax(env, B, T, H, causal):
    """No option set. That attention_pick_hpb returns more than 1 here — so mmiss_dbg_attention ran attention_heads_kernel —
    shows in mmiss_dbg_attention_pooled accepting the shape: it refuses wherever the choice is 1."""
    torch, _lib, lib = env
    qkv = _qkv(torch, B, T, H, 1000 * B + 10 * T + H + causal)
    rows = torch.arange(B, device="cuda", dtype=torch.int32) * T + (T - 1)
    pooled = torch.full((B + 1, H * 64), -7.0, device="cuda", dtype=torch.bfloat16)
    assert lib.mmiss_dbg_attention_pooled(0, None, qkv.data_ptr(), rows.data_ptr(), pooled.data_ptr(), B, T, H, causal) == 0
    ctx = _attend(env, qkv, B, T, H, causal)
    ref, bound = _attn_ref(torch, qkv, B, T, H, bool(causal), with_bound=True)
    bad = _heads_outside(torch, ctx, ref, bound, H)
    assert not bad, bad
    assert torch.equal(pooled[:B].view(torch.int16), ctx[rows.long()].view(torch.int16))
    assert (pooled[B] == -7.0).all()


def test_automatic_choice_is_one_head_below_512_workgroups(env):
    """The other side of the threshold, so that the acceptance above means something: one item fewer, and the pooled form is refused."""
    torch, _lib, lib = env
    B, T, H = 511, 17, 2
    qkv = torch.zeros(B * T, 3 * H * 64, device="cuda", dtype=torch.bfloat16)
    rows = torch.arange(B, device="cuda", dtype=torch.int32) * T
    out = torch.zeros(B, H * 64, device="cuda", dtype=torch.bfloat16)
    assert lib.mmiss_dbg_attention_pooled(0, None, qkv.data_ptr(), rows.data_ptr(), out.data_ptr(), B, T, H, 0) != 0


# ---------------------------------------------------------------------------------------------- (c) bit identity
@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("hpb", HPBS)
def test_output_is_bit_identical_to_the_one_head_kernel(env, hpb, T):
    """The kernel's comment: 'Same arithmetic, bit-identical output' — attention_kernel (att_hpb = 1) on the same input."""
    torch, _lib, lib = env
    for causal in (0, 1):
        for H in _h_of(hpb):
            qkv = _qkv(torch, B_SMALL, T, H, 20000 * hpb + 100 * T + 10 * causal + H)
            with _forced(env, 1, B_SMALL, T, H):
                one = _attend(env, qkv, B_SMALL, T, H, causal)
            with _forced(env, hpb, B_SMALL, T, H):
                got = _attend(env, qkv, B_SMALL, T, H, causal)
            diff = got.view(torch.int16) != one.view(torch.int16)
            assert not diff.any(), (causal, H, int(diff.sum()), diff.nonzero()[:8].tolist())


@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("hpb", HPBS)
def test_mxfp8_output_is_bit_identical_to_the_one_head_kernel(env, hpb, T):
    """attention_heads_kernel<ceil(T / 32), false, hpb, true, false> against attention_kernel<.., false, true>: e4m3 codes and
    E8M0 scale bytes both equal (the scale bytes no block owns keep their fill on both sides)."""
    torch, _lib, lib = env
    for H in _h_of(hpb):
        qkv = _qkv(torch, B_SMALL, T, H, 30000 * hpb + 100 * T + H)
        with _forced(env, 1, B_SMALL, T, H):
            c1, s1 = _attend_mx(env, qkv, B_SMALL, T, H)
        with _forced(env, hpb, B_SMALL, T, H):
            c2, s2 = _attend_mx(env, qkv, B_SMALL, T, H)
        assert torch.equal(c1, c2), (H, int((c1 != c2).sum()), (c1 != c2).nonzero()[:8].tolist())
        assert torch.equal(s1, s2), (H, int((s1 != s2).sum()), (s1 != s2).nonzero()[:8].tolist())
        assert (s1 != 0x5A).any()   # (the kernel did write scales)


# ---------------------------------------------------------------------------------------------- (d) every key counts
def _without_key(torch, qkv, B, T, H, drop):
    """The non-causal fp32 reference with key `drop` removed for every query."""
    x = qkv.float().reshape(B, T, 3, H, 64)
    keep = [j for j in range(T) if j != drop]
    q = x[:, :, 0].transpose(1, 2)
    k, v = x[:, keep, 1].transpose(1, 2), x[:, keep, 2].transpose(1, 2)
    p = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, dim=-1)
    return (p @ v).transpose(1, 2).reshape(B * T, H * 64)


def _every_key_counts_input(torch, B, T, H, device="cuda"):
    """V = +-8 in every component, Q and K from 0.3 N(0,1): mild scores, so every key carries ~1/T of every output."""
    g = torch.Generator(device=device).manual_seed(4000 + T)
    qkv = torch.randn(B * T, 3 * H * 64, device=device, generator=g) * 0.3
    x = qkv.view(B, T, 3, H, 64)
    x[:, :, 2] = torch.where(torch.rand(B, T, H, 64, device=device, generator=g) < 0.5, -8.0, 8.0)
    return qkv.to(torch.bfloat16)


def _dropped_keys(T):
    return sorted({0, T - 1, T // 2, 15, 16} & set(range(T)))


@pytest.mark.parametrize("T", [17, 50, 77, 128])
def test_every_key_counts_in_every_head_of_a_group(env, T):
    """As test_attention_257_keys_last_query_every_key_counts. First the power of the bound, on the reference alone: with ONE key
    removed (first, last, T // 2, 15, 16) the reference lies outside its own bound in more than 0.9 of the elements (1.0 for all
    four T on the CPU). Then the kernel, four and six heads per workgroup, inside the bound in every head."""
    torch, _lib, lib = env
    B, H = B_SMALL, 12
    qkv = _every_key_counts_input(torch, B, T, H)
    ref, bound = _attn_ref(torch, qkv, B, T, H, False, with_bound=True)
    for drop in _dropped_keys(T):
        wrong = _without_key(torch, qkv, B, T, H, drop)
        assert ((wrong - ref).abs() > bound).float().mean().item() > 0.9, drop
    for hpb in (4, 6):
        with _forced(env, hpb, B, T, H):
            ctx = _attend(env, qkv, B, T, H, 0)
        bad = _heads_outside(torch, ctx, ref, bound, H)
        assert not bad, (hpb, bad)


# ---------------------------------------------------------------------------------------------- (e) items stay apart
@pytest.mark.parametrize("T", [17, 50])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("hpb", HPBS)
def test_items_do_not_see_each_other(env, hpb, causal, T):
    """The odd items' qkv rows are NaN: a row guard that reads past T into the next item poisons the even items' softmax."""
    torch, _lib, lib = env
    B, H = 4, 12
    qkv = _qkv(torch, B, T, H, 50000 + 100 * T + hpb)
    ref, bound = _attn_ref(torch, qkv, B, T, H, bool(causal), with_bound=True)   # (of the clean input: items are independent)
    poisoned = qkv.clone()
    poisoned.view(B, T, -1)[1::2] = float("nan")
    with _forced(env, hpb, B, T, H):
        ctx = _attend(env, poisoned, B, T, H, causal)
    even = (torch.arange(B * T, device="cuda") // T) % 2 == 0
    bad = _heads_outside(torch, ctx[even], ref[even], bound[even], H)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- (f) pooled-query form
def _pooled_positions(T):
    """Tiles 0..7 of the pooled query (the kernel picks the computing wave as tile & 3: it wraps from position 64 on), both
    ends of a tile, the text tower's last EOS position 76, and the last row."""
    return [p for p in (0, 15, 16, 40, 63, 64, 76, 90, 100, 127) if p < T - 1] + [T - 1]


@pytest.mark.parametrize("T", [50, 77, 128])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("hpb", HPBS)
def test_pooled_query_form_equals_the_full_form_and_fp32_softmax(env, hpb, causal, T):
    """attention_heads_kernel<ceil(T / 32), causal, hpb, false, true>: item b pools position _pooled_positions(T)[b]."""
    torch, _lib, lib = env
    H = 12
    pos = _pooled_positions(T)
    B = len(pos)
    qkv = _qkv(torch, B, T, H, 60000 + 100 * T + 10 * hpb + causal)
    rows = torch.tensor([b * T + p for b, p in enumerate(pos)], device="cuda", dtype=torch.int32)
    got = torch.full((B + 1, H * 64), -7.0, device="cuda", dtype=torch.bfloat16)
    with _forced(env, hpb, B, T, H):
        full = _attend(env, qkv, B, T, H, causal)
        _lib.check(lib.mmiss_dbg_attention_pooled(0, None, qkv.data_ptr(), rows.data_ptr(), got.data_ptr(), B, T, H, causal))
        torch.cuda.synchronize()
    assert (got[B] == -7.0).all(), "the row behind the last item was written"
    ref, bound = _attn_ref(torch, qkv, B, T, H, bool(causal), with_bound=True)
    idx = rows.long()
    bad = _heads_outside(torch, got[:B], ref[idx], bound[idx], H)
    assert not bad, bad
    diff = (got[:B].view(torch.int16) != full[idx].view(torch.int16)).any(dim=1)
    assert not diff.any(), [pos[b] for b in diff.nonzero().flatten().tolist()]   # (the pooled positions that differ)

"""The patch-embedding GEMM that reads the f32 pixels itself (gemm160p_kernel<MMISS_EPI_PATCH_PIX_F32>, gemm_bf16_p160.h) against
the two launches it replaces — im2col (f32 -> bf16 patches) and the 128-column patch GEMM — bit for bit: the same f32 -> bf16
conversion, the same K order inside every accumulator, the same epilogue. The shapes cover one and two row blocks (the second
almost all pad rows), one and three column tiles, 48 and 12 K-tiles (two and four pixel rows per K-tile), and a grid of nine
patches per image, where the row -> (image, py, px) division is a real one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (S, P, d, B): rows = B * (S / P)^2
SHAPES = [(64, 32, 256, 40), (64, 32, 768, 41), (32, 16, 256, 45), (96, 32, 256, 18)]
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch, _lib, lib


def _pixels(torch, B, S, seed):
    """Gaussian pixels with the f32 -> bf16 edge cases planted all over: exact rounding ties (to even, both ways), values one
    f32 ulp on either side of a tie, +-0, f32 denormals, the largest bf16 denormal's neighbourhood and +-3e38 (rounds to a
    finite bf16 just below the overflow to infinity)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    px = torch.randn(B, 3, S, S, device="cuda", generator=g)
    special = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,   # ties, near-ties
                        0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000,   # +-0, denormals (tie among them)
                        0x7F61B1E6, 0xFF61B1E6, 0x7F7F0000, 0x3F800000], dtype=np.uint32).view(np.float32)   # +-3e38, 3.39e38
    flat = px.view(-1)
    idx = torch.randperm(flat.numel(), device="cuda", generator=g)[: 64 * len(special)]
    flat[idx] = torch.from_numpy(np.tile(special, 64)).cuda()
    flat[:len(special)] = torch.from_numpy(special).cuda()          # the first patch row's first K-tile
    flat[-len(special):] = torch.from_numpy(special).cuda()         # the last valid row's last pixels
    return px


@pytest.mark.parametrize("S,P,d,B", SHAPES)
def test_patch_gemm_from_pixels_is_bit_identical_to_im2col_plus_gemm(env, S, P, d, B):
    torch, _lib, lib = env
    G = S // P
    GG, T, K = G * G, G * G + 1, 3 * P * P
    M = B * GG
    g = torch.Generator(device="cuda").manual_seed(S + P + d + B)
    px = _pixels(torch, B, S, 17 * S + B)
    W = (torch.randn(d, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    pos = torch.randn(T, d, device="cuda", generator=g)

    # reference: im2col into a buffer padded to the 128-row tile, then the 128-column kernel (epilogue 4, tile height 128) —
    # gemm16_kernel itself: at these row counts mmiss_dbg_gemm would otherwise hand the GEMM to the skinny kernel or split K,
    # which sum K in another order
    Mp = (M + 127) // 128 * 128
    patches = torch.zeros(Mp, K, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.mmiss_dbg_im2col(0, None, px.data_ptr(), patches.data_ptr(), B, S, P, K))
    # (mmiss_dbg_gemm stores all Mp rows: its pad rows land in the token rows of images B, B + 1, ... — room for them)
    rows_alloc = ((Mp + GG - 1) // GG + 1) * T
    want = torch.full((rows_alloc, d), SENTINEL, device="cuda")
    _lib.set_option("gemm_skinny", 0)
    _lib.set_option("gemm_splitk", 0)
    try:
        _lib.check(lib.mmiss_dbg_gemm(0, None, _lib.EPI_PATCH_F32, 128, patches.data_ptr(), W.data_ptr(), want.data_ptr(), None,
                                      pos.data_ptr(), Mp, d, K, GG, T))
    finally:
        _lib.set_option("gemm_skinny", 1)
        _lib.set_option("gemm_splitk", 1)
    got = torch.full((rows_alloc, d), SENTINEL, device="cuda")
    _lib.check(lib.mmiss_dbg_patch_from_pixels(0, None, px.data_ptr(), W.data_ptr(), got.data_ptr(), pos.data_ptr(), B, S, P, d))
    torch.cuda.synchronize()

    rows = torch.arange(B * T, device="cuda")
    is_patch = (rows % T) != 0
    diff = got[:B * T][is_patch].view(torch.int32) != want[:B * T][is_patch].view(torch.int32)
    assert not diff.any(), (int(diff.sum()), diff.nonzero()[:8].tolist())
    assert torch.isfinite(got[:B * T][is_patch]).all()
    # the CLS rows and everything past the valid rows still hold the sentinel
    assert (got[:B * T][~is_patch] == SENTINEL).all()
    assert (got[B * T:] == SENTINEL).all()

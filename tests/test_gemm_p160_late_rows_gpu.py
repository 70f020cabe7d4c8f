"""gemm160p_kernel (gemm_bf16_p160.h) fetches the bf16 rows it adds to — its own old output rows — with the two stagings that
have no K-tile left to fetch, into the LDS slots those fill, and its epilogue reads them from there. Which slots depends on
nt % 3 (nt = K / 64 K-tiles, three staging buffers), the row stride of the output replaces K in the per-lane offset, and the
K-tile count is a run-time value or a compile-time tag depending on K. The 128-column kernel of the same epilogue (variant 160
of mmiss_dbg_gemm_resid16) is the bit reference: same k order in the MFMA chain, same rounding point, same statistics."""
import pytest

pytestmark = pytest.mark.gpu

# (M, N, K, m_valid): nt = 4, 6 (run-time K-tile count), 8, 12, 48 (compile-time) — nt % 3 = 1, 0, 2, 0, 0; row stride == K and
# != K; one and three column tiles; (320, 768, 768, 170): the lower wave half of the second row block is all pad rows
SHAPES = [(320, 256, 256, 301), (320, 768, 384, 320), (480, 512, 512, 333), (320, 768, 768, 170), (160, 768, 3072, 97)]


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch, _lib, lib


def _resid16(env, variant, A, W, out, bias, stats, m_valid):
    torch, _lib, lib = env
    M, K = A.shape
    N = W.shape[0]
    _lib.check(lib.mmiss_dbg_gemm_resid16(0, None, variant, A.data_ptr(), W.data_ptr(), out.data_ptr(), bias.data_ptr(),
                                          stats.data_ptr(), M, N, K, m_valid, 0, None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K,mv", SHAPES)
def test_late_rows_bit_equal_to_the_128_column_kernel(env, M, N, K, mv):
    """Output and statistics of the valid rows equal the reference's bits; pad rows other than the dump row M - 1 keep their
    bytes and their statistics stay NaN. Three repetitions with fresh inputs: a slot read before its piece landed, or a
    transpose patch written over a piece, would show as a stale value."""
    torch, _lib, lib = env
    g = torch.Generator(device="cuda").manual_seed(11 * M + 5 * N + K)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g)
    for rep in range(3):
        A = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
        x0 = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
        want = x0.clone()
        st_want = torch.zeros(M, N // 64, 2, device="cuda")
        _resid16(env, 160, A, W, want, bias, st_want, M)
        out = x0.clone()
        st = torch.full((M, N // 64, 2), float("nan"), device="cuda")
        _resid16(env, 0, A, W, out, bias, st, mv)
        diff = out[:mv].view(torch.int16) != want[:mv].view(torch.int16)
        assert not diff.any(), (rep, int(diff.sum()), diff.nonzero()[:8].tolist())
        assert torch.equal(st[:mv].view(torch.int32), st_want[:mv].view(torch.int32)), rep
        if mv < M:
            assert torch.equal(out[mv:M - 1].view(torch.int16), x0[mv:M - 1].view(torch.int16)), rep
            assert torch.isnan(st[mv:]).all(), rep


def test_late_rows_come_back_unchanged_under_a_zero_product(env):
    """A = 0 and bias = 0: the kernel must return the old rows bit for bit (f32(x) + 0 rounds back to x), so a piece that
    landed in, or was read from, the wrong slot shows up as itself and not as GEMM noise. nt = 4: both fetches wrap into
    buffers 1 and 2 and the patches move to buffer 0; the row stride (768) is not K (256); three column tiles."""
    torch, _lib, lib = env
    M, N, K = 320, 768, 256
    g = torch.Generator(device="cuda").manual_seed(99)
    A = torch.zeros(M, K, device="cuda", dtype=torch.bfloat16)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.zeros(N, device="cuda")
    x0 = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
    assert not (x0.view(torch.int16) == -32768).any()   # (-0.0 + 0.0 would come back as +0.0)
    out = x0.clone()
    st = torch.zeros(M, N // 64, 2, device="cuda")
    _resid16(env, 0, A, W, out, bias, st, M)
    diff = out.view(torch.int16) != x0.view(torch.int16)
    assert not diff.any(), (int(diff.sum()), diff.nonzero()[:8].tolist())

"""The tile epilogue of gemm160p_kernel's residual form (gemm_bf16_p160.h): old rows out of the late stagings' LDS slots, blocks
0..2 started before the second staging has landed, two alternating transpose patches per wave, row statistics added up by DPP,
output rows and statistics stored through buffer descriptors with per-tile offsets. All of it must give the bits of the
128-column kernel of the same epilogue (variant 160 of mmiss_dbg_gemm_resid16), rows and statistics, and must leave every pad
row but the dump row M - 1 alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (M, N, K): nt = K / 64 = 4, 6 (run-time K-tile count), 8, 12, 48 (compile-time): nt % 3 = 1, 0, 2, 0, 0 decides the old rows' slots
# and the buffer the patches lie over; one, two and three column tiles
SHAPES = [(160, 256, 256), (320, 768, 384), (480, 512, 512), (320, 768, 768), (160, 768, 3072)]
# m_valid: inside and at the two 8-row halves of a 16-row block (1, 8, 9, 16), the wave-half boundary (80, 81), M - 1, M
CASES = [(160, 256, 256, mv) for mv in (1, 8, 9, 16, 80, 81, 159, 160)]
CASES += [(M, N, K, mv) for (M, N, K) in SHAPES[1:] for mv in (M - 1, M)]
# the second row block's lower wave half (rows 240..319) is all pad rows; and a first valid row there
CASES += [(320, 768, 768, 200), (320, 768, 384, 241), (480, 512, 512, 333), (160, 768, 3072, 81)]


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
                                          stats.data_ptr() if stats is not None else None, M, N, K, m_valid, 0, None))
    torch.cuda.synchronize()


def _operands(torch, g, M, N, K):
    A = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    x0 = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
    return A, x0


@pytest.mark.parametrize("M,N,K,mv", CASES)
def test_epilogue_bit_equal_to_the_128_column_kernel(env, M, N, K, mv):
    """Rows and statistics of the valid rows carry the reference's bits; pad rows other than the dump row M - 1 keep their
    bytes and their statistics stay NaN. Three repetitions with fresh inputs: a patch read before it was written, or written
    over before it was read, shows as a value of the repetition before."""
    torch, _lib, lib = env
    g = torch.Generator(device="cuda").manual_seed(13 * M + 7 * N + K + mv)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g)
    for rep in range(3):
        A, x0 = _operands(torch, g, M, N, K)
        want = x0.clone()
        st_want = torch.zeros(M, N // 64, 2, device="cuda")
        _resid16(env, 160, A, W, want, bias, st_want, M)
        out = x0.clone()
        st = torch.full((M, N // 64, 2), float("nan"), device="cuda")
        _resid16(env, 0, A, W, out, bias, st, mv)
        diff = out[:mv].view(torch.int16) != want[:mv].view(torch.int16)
        assert not diff.any(), (rep, int(diff.sum()), diff.nonzero()[:8].tolist())
        sdiff = st[:mv].view(torch.int32) != st_want[:mv].view(torch.int32)
        assert not sdiff.any(), (rep, int(sdiff.sum()), sdiff.nonzero()[:8].tolist())
        if mv < M:
            assert torch.equal(out[mv:M - 1].view(torch.int16), x0[mv:M - 1].view(torch.int16)), rep
            assert torch.isnan(st[mv:]).all(), rep


@pytest.mark.parametrize("M,N,K,mv", [(320, 768, 768, 320), (320, 768, 384, 241), (160, 256, 256, 9)])
def test_epilogue_without_statistics(env, M, N, K, mv):
    """stats_out == NULL: the rows are still the reference's, the pad rows still their own."""
    torch, _lib, lib = env
    g = torch.Generator(device="cuda").manual_seed(3 * M + N + K + mv)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g)
    for rep in range(3):
        A, x0 = _operands(torch, g, M, N, K)
        want = x0.clone()
        _resid16(env, 160, A, W, want, bias, torch.zeros(M, N // 64, 2, device="cuda"), M)
        out = x0.clone()
        _resid16(env, 0, A, W, out, bias, None, mv)
        assert torch.equal(out[:mv].view(torch.int16), want[:mv].view(torch.int16)), rep
        if mv < M:
            assert torch.equal(out[mv:M - 1].view(torch.int16), x0[mv:M - 1].view(torch.int16)), rep


def _kernel_order_sums(y):
    """(sum, sum of squares) per 64 columns of f32 rows y [M, N] in the epilogue's association, every operation rounded to f32:
    a lane adds its 8 columns pair by pair (0 + (a0 + b0)) + (a1 + b1) ..., the eight lanes of a row then add up as a
    butterfly over lane xor 1, 2, 4 (read in lane 0)."""
    M, N = y.shape
    v = y.reshape(M, N // 64, 8, 4, 2).astype(np.float32)
    a, b = v[..., 0], v[..., 1]
    rs = np.zeros(v.shape[:3], np.float32)
    rq = np.zeros(v.shape[:3], np.float32)
    for e in range(4):
        rs = rs + (a[..., e] + b[..., e])
        rq = rq + (a[..., e] * a[..., e] + b[..., e] * b[..., e])
    out = []
    for r in (rs, rq):
        t = r[..., 0::2] + r[..., 1::2]           # lanes 0, 2, 4, 6 after xor 1
        u = t[..., 0::2] + t[..., 1::2]           # lanes 0, 4 after xor 2
        out.append(u[..., 0] + u[..., 1])         # lane 0 after xor 4
    return out


def test_statistics_keep_their_order_of_addition(env):
    """Old rows and products mix magnitudes 2^-12 .. 2^12, so that an f32 sum over a row's 64 columns depends on the order it
    is taken in (asserted on this very data, on the host: the plain left-to-right sum of the same 64 stored values differs in
    bits somewhere). The statistics must still be the reference kernel's bits, and the epilogue's order restated in numpy."""
    torch, _lib, lib = env
    M, N, K = 320, 768, 768
    g = torch.Generator(device="cuda").manual_seed(4242)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.zeros(N, device="cuda")
    for rep in range(3):
        # per element: a power of two between 2^-12 and 2^12 times a unit normal, on the old rows; per row on A (its products)
        ex = torch.randint(-12, 13, (M, N), device="cuda", generator=g).float()
        x0 = (torch.randn(M, N, device="cuda", generator=g) * torch.exp2(ex)).to(torch.bfloat16)
        ea = torch.randint(-12, 13, (M, 1), device="cuda", generator=g).float()
        A = (torch.randn(M, K, device="cuda", generator=g) * torch.exp2(ea)).to(torch.bfloat16)
        want = x0.clone()
        st_want = torch.zeros(M, N // 64, 2, device="cuda")
        _resid16(env, 160, A, W, want, bias, st_want, M)
        out = x0.clone()
        st = torch.full((M, N // 64, 2), float("nan"), device="cuda")
        _resid16(env, 0, A, W, out, bias, st, M)
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), rep
        y = out.float().cpu().numpy()
        # another association of the same values: left to right over the 64 columns
        seq = np.zeros((M, N // 64), np.float32)
        cols = y.reshape(M, N // 64, 64)
        for c in range(64):
            seq = seq + cols[..., c]
        ks, kq = _kernel_order_sums(y)
        assert (seq.view(np.uint32) != ks.view(np.uint32)).any(), "the data does not tell two orders of addition apart"
        got = st.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), st_want.cpu().numpy().view(np.uint32)), rep
        assert np.array_equal(got[..., 0].view(np.uint32), ks.view(np.uint32)), rep
        assert np.array_equal(got[..., 1].view(np.uint32), kq.view(np.uint32)), rep

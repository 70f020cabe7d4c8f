"""Operands and float64 references of the one-request folded skinny GEMM chain, shared by test_skinny_chain_cpu.py (which
establishes on the host what the GPU tests rely on) and test_skinny_chain_gpu.py (which runs them through gemm_skinny_kernel and
skinny_row_stats16_kernel). A plain helper module: no fixtures, numpy only, Philox seeds; every call with the same arguments
returns the same bits.

Row profiles (rows(M, d, profile, seed), f32 [M, d]):
  rowwise  row m = 0.5 m + (1 + m mod 5) N(0,1): every row has its own mean and scale, neighbouring 16-row tiles differ by 8 in
           the mean. A kernel that applies another row's (mean, rstd), another tile's old residual or another slice's sums misses
           by orders of magnitude more than any tolerance here.
  plain    3 N(0,1) + 0.5 (test_kernels_gpu.py::test_layernorm)
  offset   3 N(0,1) + 30: mean = 10 std, E[x^2] - mean^2 cancels two decimal digits (test_layernorm_chain_gpu.py)
  outlier  N(0,1) with columns 3, d / 2 + 1 and d - 2 at 100 x: three slices carry nearly all of the sum of squares
Weights: W = bf16(scale K^-1/2 N(0,1)), gamma, beta, bias ~ N(0,1) (test_layernorm_chain_gpu.py::_fold_inputs).

The folded algebra (csrc/gemm_bf16.h, epilogues 7 / 8): with A = xb = bf16(x), W' = bf16(f32(W) gamma), c_n = sum_k W'[n,k],
b'_n = b_n + sum_k beta_k W[n,k] and (mean_m, rstd_m) from the (sum, sumsq) partials per 16 columns OF THE f32 ROWS x,
    y = rstd_m (xb W'^T - mean_m c) + b'      ("exact folded form": float64 on the rounded operands the kernel reads)
stands for LayerNorm(xb; gamma, beta) W^T + b ("semantic form"). The two differ by the rounding of W' (2^-9 relative per weight),
by the f32 rounding of c, b' and the partials, and by the statistics being those of x, not of xb = bf16(x).
"""
import numpy as np

U = 2.0 ** -24
EPS = 1e-5
RTOL, ATOL = 2.0 ** -7, 4e-3          # the project's bf16 tolerance (test_chain_prelayernorm_fold_and_folded_gemm)
PROFILES = ("rowwise", "plain", "offset", "outlier")
# the chain of test_skinny_chain_gpu.py::test_chain: (d, N of the QKV stand-in, mlp), M rows
CHAIN_SHAPES = ((128, 384, 512), (768, 128, 256))
CHAIN_M = 77
SEMANTIC_W_SCALE = 0.25
# (d, stage) -> the profiles whose exact folded form lies within HALF of tol of the semantic form at SEMANTIC_W_SCALE
# (test_skinny_chain_cpu.py asserts it): only these are held to the semantic form on the GPU. Listed are the profiles that clear
# half of tol with a margin (ratio <= 0.45 here; the highest listed is 0.44), so that another numpy / BLAS build does not flip
# one: d = 128 fc1 offset (0.49) and rowwise (0.50) are left out with the ones that clearly miss (0.59 - 2.1).
SEMANTIC_CLEARED = {
    (128, "qkv"): ("plain",),
    (128, "fc1"): ("plain",),
    (768, "qkv"): ("plain", "offset"),
    (768, "fc1"): ("rowwise", "plain", "offset", "outlier"),
}


def rng_of(*seed):
    return np.random.Generator(np.random.Philox(key=[20250601, sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed))]))


def bf16_bits(x):
    """f32 -> the bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(x):
    """f32 -> the nearest bf16 value, as f32."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def rows(M, d, profile, seed):
    g = rng_of(seed, M, d, PROFILES.index(profile))
    z = g.standard_normal((M, d))
    m = np.arange(M, dtype=np.float64)[:, None]
    if profile == "rowwise":
        x = 0.5 * m + (1.0 + (m % 5)) * z
    elif profile == "plain":
        x = 3.0 * z + 0.5
    elif profile == "offset":
        x = 3.0 * z + 30.0
    elif profile == "outlier":
        x = z.copy()
        x[:, [3, d // 2 + 1, d - 2]] *= 100.0
    else:
        raise ValueError(profile)
    return x.astype(np.float32)


def weights(N, K, seed, scale=1.0):
    """W f32 [N, K] on the bf16 grid, gamma, beta f32 [K], bias f32 [N]"""
    g = rng_of(seed, N, K)
    W = bf16_round((g.standard_normal((N, K)) * (scale * K ** -0.5)).astype(np.float32))
    gam = g.standard_normal(K).astype(np.float32)
    bet = g.standard_normal(K).astype(np.float32)
    bias = g.standard_normal(N).astype(np.float32)
    return W, gam, bet, bias


def fold_host(W, gam, bet, bias):
    """What fold_ln_weights_kernel writes, restated: W' bit for bit, c and b' as correctly rounded f32 of the f64 sums (the
    kernel's f32 sums lie within K u sum|.| of them: test_fold_ln_weights)."""
    wf = bf16_round(W.astype(np.float32) * gam.astype(np.float32))
    c = wf.astype(np.float64).sum(1).astype(np.float32)
    bf = (bias.astype(np.float64) + (W.astype(np.float64) * bet.astype(np.float64)).sum(1)).astype(np.float32)
    return wf, c, bf


def stats16_host(x):
    """f32 [M][d/16][2]: (sum, sumsq) per 16 columns, summed in f32 in skinny_row_stats16_kernel's order (4 values per lane,
    then lanes l ^ 1, l ^ 2)."""
    x = np.ascontiguousarray(x, np.float32)
    M, d = x.shape
    v = x.reshape(M, d // 16, 4, 4)
    sq = v * v
    s = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
    q = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
    s = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
    q = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    return np.stack([s, q], -1).astype(np.float32)


def mean_rstd64(stats, K, eps=EPS):
    """(mean, rstd) f64 [M, 1] from the f32 partials [M][K/16][2]: the kernel's formula, sums and root in float64"""
    s = stats.astype(np.float64).sum(1)
    mean = s[:, :1] / K
    var = np.maximum(s[:, 1:] / K - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + eps)


def quick_gelu64(y):
    return y / (1.0 + np.exp(-1.702 * y))


def exact_folded(xb, wf, c, bf, stats, gelu, eps=EPS):
    """float64 rstd (xb W'^T - mean c) + b' on the rounded operands and the f32 partials the kernel reads"""
    K = xb.shape[1]
    mean, rstd = mean_rstd64(stats, K, eps)
    y = rstd * (xb.astype(np.float64) @ wf.astype(np.float64).T - mean * c.astype(np.float64)) + bf.astype(np.float64)
    return quick_gelu64(y) if gelu else y


def semantic(xb, W, gam, bet, bias, gelu, eps=EPS):
    """float64 LayerNorm(xb; gamma, beta) W^T + b (then QuickGELU)"""
    x = xb.astype(np.float64)
    mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)
    h = (x - mean) / np.sqrt(var + eps) * gam.astype(np.float64) + bet.astype(np.float64)
    y = h @ W.astype(np.float64).T + bias.astype(np.float64)
    return quick_gelu64(y) if gelu else y


def tol(ref):
    return ATOL + RTOL * np.abs(ref)


def resid_rows64(x0, A, W, bias):
    """float64 x0 + A W^T + bias and the sum of magnitudes |x0| + |bias| + sum_k |a w| that bounds its f32 evaluation"""
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    ref = x0.astype(np.float64) + A64 @ W64.T + bias.astype(np.float64)
    mag = np.abs(x0).astype(np.float64) + np.abs(A64) @ np.abs(W64).T + np.abs(bias).astype(np.float64)
    return ref, mag


def resid_terms64(x0, A, W, bias):
    """t = |x0| + |A W^T| + |bias| per element (float64): the size of the terms the residual epilogue adds"""
    acc = A.astype(np.float64) @ W.astype(np.float64).T
    return np.abs(x0).astype(np.float64) + np.abs(acc) + np.abs(bias).astype(np.float64)


class ChainCase:
    """The operands of one chain run (d, Nq, mlp) x profile x weight scale; the stages that follow the device are restated on
    the host in float64 -> f32 so that the CPU test sees (to the last few ulp) the rows the GPU test normalises."""

    def __init__(self, d, Nq, mlp, profile, w_scale, M=CHAIN_M):
        self.d, self.Nq, self.mlp, self.M, self.profile, self.w_scale = d, Nq, mlp, M, profile, w_scale
        self.x0 = rows(M, d, profile, 501)
        self.Wq, self.g1, self.b1, self.bq = weights(Nq, d, 502, w_scale)          # LayerNorm1 + QKV stand-in
        self.ctx = bf16_round(rng_of(503, M, d).standard_normal((M, d)).astype(np.float32))
        self.Wo, _, _, self.bo = weights(d, d, 504)                                # out-projection
        self.W1, self.g2, self.b2, self.bf1 = weights(mlp, d, 505, w_scale)        # LayerNorm2 + FC1

    def new_rows_host(self):
        ref, _ = resid_rows64(self.x0, self.ctx, self.Wo, self.bo)
        return ref.astype(np.float32)

    def stage(self, name, x=None):
        """(x f32 rows, W, gamma, beta, bias, gelu) of the folded GEMM 'qkv' (on x0) or 'fc1' (on the new rows: x, or the host's)"""
        if name == "qkv":
            return self.x0, self.Wq, self.g1, self.b1, self.bq, False
        return (self.new_rows_host() if x is None else x), self.W1, self.g2, self.b2, self.bf1, True

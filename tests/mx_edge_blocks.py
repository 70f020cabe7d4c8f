"""One catalogue of 32-value edge blocks for every MXFP8 producer (tests/test_mxfp8_edges_cpu.py, tests/test_mxfp8_edges_gpu.py).
A plain helper module: no fixtures, numpy only.

Every value is bf16-representable (at most 8 significant bits, exponent inside the f32 / bf16 range), so the same list serves a
kernel that reads f32 and one that reads bf16. The groups, and what each is there to catch:

  zeros     all +0, all -0, alternating: the amax = 0 path through the 1e-30 clamp, codes 0x00 / 0x80
  maxpos    300.0 at position p, the other 31 values in +-[1, 2): a block maximum that misses position p takes a scale 8
            steps too small, 300 * inv leaves the e4m3 range and the bytes differ (32 blocks, one per position)
  boundary  amax in {446, 448, 450} * 2^k, k in {-20, -8, -1, 0, 1, 8, 20}: 446 and 448 are the last two bf16 values whose scale
            byte is 127 + k, 450 the first with 128 + k
  ties      amax = 448 (scale 1) and +- every midpoint of two neighbouring e4m3 codes (5 significant bits each), the subnormal
            ties (2 j + 1) 2^-10 among them: all must go to the even code
  clamp     amax 2^-120 (under the 1e-30 clamp, every code zero), amax 2^-116 (under the clamp, codes NOT zero: the scale byte is
            the clamp's, not the block's) and amax 1.765625 * 2^127 = 3.0e38
  sign      the maxpos blocks negated; +448 and -448 in one block
"""
import numpy as np

GROUPS = ("zeros", "maxpos", "boundary", "ties", "clamp", "sign")
BOUNDARY_K = (-20, -8, -1, 0, 1, 8, 20)


def _e4m3_positive():
    """the 127 non-negative finite e4m3 values, ascending (OCP FP8 E4M3: bias 7, subnormals m / 8 * 2^-6, largest 448)"""
    v = []
    for code in range(127):
        e, m = code >> 3, code & 7
        v.append((m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7))
    return np.array(v, np.float64)


E4M3_POS = _e4m3_positive()
E4M3_MIDPOINTS = (E4M3_POS[:-1] + E4M3_POS[1:]) / 2.0     # 126 ties; entry i lies between codes i and i + 1


def is_bf16(x) -> bool:
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return bool(((u & 0xFFFF) == 0).all())


def _small(rng, n):
    """n values +-(1 + j / 128), j = 0..127: +-[1, 2) on the bf16 grid"""
    return ((1.0 + rng.integers(0, 128, n) / 128.0) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def catalogue():
    """[(name, group, float32 [32])]; fixed seed, the same list on every call."""
    rng = np.random.default_rng(20240607)
    out = []

    def add(name, group, v):
        v = np.asarray(v, np.float32)
        assert v.shape == (32,) and np.isfinite(v).all() and is_bf16(v), name
        out.append((name, group, v))

    add("zeros+", "zeros", np.zeros(32))
    add("zeros-", "zeros", -np.zeros(32))
    add("zeros+-", "zeros", np.where(np.arange(32) % 2 == 0, 0.0, -0.0))
    sweep = []
    for p in range(32):
        v = _small(rng, 32)
        v[p] = 300.0
        sweep.append(v)
        add("maxpos%02d" % p, "maxpos", v)
    for i, k in enumerate(BOUNDARY_K):
        for j, a in enumerate((446.0, 448.0, 450.0)):
            v = _small(rng, 32) * np.float32(4.0 * 2.0 ** k)            # 4 .. 8 times 2^k: codes of their own, far under the maximum
            v[(5 * (3 * i + j) + 3) % 32] = a * 2.0 ** k * (-1.0 if (i + j) % 2 else 1.0)
            add("boundary%d*2^%d" % (int(a), k), "boundary", v)
    ties = np.concatenate([E4M3_MIDPOINTS, -E4M3_MIDPOINTS])              # 252 values, 31 to a block beside the 448
    ties = ties[rng.permutation(ties.size)]
    for b in range(-(-ties.size // 31)):
        t = ties[31 * b:31 * b + 31]
        t = np.concatenate([t, np.zeros(31 - t.size)])
        p = (7 * b + 2) % 32
        add("ties%d" % b, "ties", np.concatenate([t[:p], [448.0], t[p:]]))
    v = _small(rng, 32) * np.float32(2.0 ** -122)
    v[11] = 2.0 ** -120
    add("clamp_all_zero", "clamp", v)
    v = _small(rng, 32) * np.float32(2.0 ** -118)
    v[29] = -(2.0 ** -116)
    add("clamp_codes", "clamp", v)
    v = _small(rng, 32) * np.exp2(rng.integers(100, 111, 32)).astype(np.float32)
    v[6] = 1.765625 * 2.0 ** 127
    add("huge", "clamp", v)
    for p in range(32):
        add("maxpos%02d-" % p, "sign", -sweep[p])
    v = _small(rng, 32)
    v[3], v[20] = 448.0, -448.0
    add("+448-448", "sign", v)
    return out


def layout_rows(blocks, d):
    """float32 [C, d]: row r, block j holds blocks[(r + j) % C] — every block index of a row (every lane group of a producer)
    sees every case. `blocks`: a list of 32-value arrays."""
    C = len(blocks)
    assert d % 32 == 0
    stack = np.stack([np.asarray(b, np.float32) for b in blocks])
    idx = (np.arange(C)[:, None] + np.arange(d // 32)[None, :]) % C
    return np.ascontiguousarray(stack[idx].reshape(C, d))


# ------------------------------------------------------------------------------------------------ QuickGELU -> MXFP8 cases
QGELU_BAND = 2.0 ** -16     # relative distance of the exact scaled value to a code midpoint inside which one code step passes
QGELU_CAP = 0.01            # largest share of elements the band may take


def qgelu_case(M, N, K):
    """The operands of one QuickGELU -> MXFP8 case. A rows are one-hot (code 1.0 at column k_m = m % K, every scale byte 127),
    so acc[m, n] = W[n, m % K] exactly and the pre-activation is float32(W[n, k_m] + bias[n]), one rounding however the
    epilogue multiplies by wscale = 1 and adds. W8: bands of 64 output columns, band b = (n // 64) % 4:
      0  240 where n % 64 == k % 64, else 1 .. 1.75; bias 0       the 64-column maximum of row m sits at column m % 64
      1  1 .. 1.75 only; bias -50                                 QuickGELU ~ -7e-35: under the 1e-30 clamp, codes not zero
      2  zero codes (both signs); bias 0                          exact zeros
      3  as band 0 with random signs; bias j / 16 in [-2, 2)       the sweep on other values (a -240 gives -0: the maximum is elsewhere)
    -> (A8, As natural [M, K/32], W8, bias f32 [N], pre f32 [M, N])"""
    rng = np.random.default_rng(1000 + N + K)
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    band = (n // 64) % 4
    mag = 0x38 + rng.integers(0, 7, (N, K))                                  # codes of 1, 1.125 .. 1.75
    W8 = np.where((n % 64 == k % 64) & ((band == 0) | (band == 3)), 0x77, mag)   # 0x77 = 240
    W8 = np.where((band == 3) & (rng.random((N, K)) < 0.5), W8 | 0x80, W8)
    W8 = np.where(band == 2, np.where(rng.random((N, K)) < 0.5, 0x80, 0x00), W8).astype(np.uint8)
    b1 = (n[:, 0] // 64) % 4
    bias = np.where(b1 == 1, -50.0, np.where(b1 == 3, rng.integers(-32, 32, N) / 16.0, 0.0)).astype(np.float32)
    A8 = np.zeros((M, K), np.uint8)
    A8[np.arange(M), np.arange(M) % K] = 0x38
    As = np.full((M, K // 32), 127, np.uint8)
    e, m = (W8 >> 3) & 0xF, W8 & 7
    Wf = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * np.exp2(e.astype(np.float64) - 7)) * np.where(W8 & 0x80, -1.0, 1.0)
    pre = (Wf.astype(np.float32).T[np.arange(M) % K] + bias[None, :]).astype(np.float32)
    return A8, As, W8, bias, pre


def qgelu_reference(pre):
    """float64 QuickGELU x sigmoid(1.702 x) of the float32 pre-activations (HF activations.py: QuickGELUActivation)"""
    x = np.asarray(pre, np.float64)
    return x / (1.0 + np.exp(-1.702 * x))


def near_midpoint(y64, e64, band=QGELU_BAND):
    """y64 float64 [M, N], e64 uint8 [M, N/32] scale bytes -> bool [M, N]: the exact scaled value |y| 2^(127 - e) lies within
    relative `band` of a midpoint of two neighbouring e4m3 codes."""
    v = np.abs(y64) * np.exp2(127.0 - e64.astype(np.float64)).repeat(32, axis=1)
    i = np.clip(np.searchsorted(E4M3_MIDPOINTS, v), 0, E4M3_MIDPOINTS.size - 1)
    lo = E4M3_MIDPOINTS[np.clip(i - 1, 0, None)]
    hi = E4M3_MIDPOINTS[i]
    return (np.abs(v - lo) <= band * lo) | (np.abs(v - hi) <= band * hi)

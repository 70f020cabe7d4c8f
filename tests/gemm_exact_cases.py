"""Exactly representable operands, float64 references and the comparison of the tiled bf16 GEMM tests, shared by
test_gemm_exact_cpu.py (which establishes on the host what the GPU tests rely on: the conditions below, and that the comparison
rejects the wrong results it is there to catch) and test_gemm_exact_gpu.py (which runs the cases through every instance of
gemm16_kernel, gemm256_kernel, the persistent kernels, the skinny kernel and splitk_reduce_kernel). A plain helper module: no
fixtures; torch only, on whatever device it is handed; the operands come from an integer hash of (row, column, seed), so the
host and the device see the same bits.

The method. A[m,k] are nonzero integers, W[n,k] nonzero integers times 2^-s, bias / x0 / pos multiples of Q = 2^-7. Every
product and every partial sum, in any order, is then a multiple of the common quantum below 2^24 of them (condition a): exact in
fp32. The accumulator of every kernel, split-K and the K slices of the skinny kernel included, must equal the float64 product bit
for bit, acc + bias (+ old row) is exact too, and a bf16 output has exactly one correct bit pattern: the epilogue's one documented
rounding, to nearest even. No operand is zero, so one lost or doubled product changes the element.

Kinds of operands (Case.kind):
  wide   A in +-1..+-4, W in +-1..+-4 times 2^-s with s = ceil(log2(K) / 2 + 1/2): |acc| has standard deviation 2.7-5.3. Used for the
         plain epilogues.
  fold   the same with s + 1, for the folded epilogues: y = rstd (acc - mean c) + b' then has standard deviation 0.5-0.7, which
         keeps the undecided share of epilogue 8 (whose margin carries both factors) under the cap. The rows' mean is ~0:
         |mean| <= sigma; offset-dominated rows belong to test_layernorm_chain_gpu.py.
  stats  A in +-1, W in +-1 times 2^-7, |x0| in [2.25, 2.75) on the 2^-6 grid (exact in bf16: the bf16 residual stream too):
         every value stays below 4 = 2^9 Q, so that (sum, sumsq) over 64 columns is exact in any order (condition b), and most
         values sit in [2, 4), where the bf16 grid is 2^-6 and every odd multiple of Q is a rounding tie.

Conditions, asserted by Case.check on the reference alone:
  (a) (K max|a| max|w| + max|bias| + max|x0|) / quantum < 2^24
  (b) statistics: 64 max(v^2) / Q^2 < 2^24 for the values v the statistics are taken of
  (c) at least 5 % of the elements of a bf16 output are ties that round up (in magnitude) to even, 5 % ties that round down
  (d) at least 25 % of them are inexact in bf16 (ties included)

Inexact epilogues (QuickGELU: v_exp_f32 and v_rcp_f32; folded LayerNorm: rstd). The float64 value is the true value of what the
kernel computes up to a few f32 roundings, so the reference comes with a margin
    margin = 2^-18 T,   T (QuickGELU) = |y| (1 + |2.4555 x|),   T (folded) = rstd (|acc| + |mean c|) + |b'|
                                                                 (times the QuickGELU factor of its own x for epilogue 8)
2^-18 = 32 unit roundoffs of fp32: fewer than ten operations of at most 1 ulp each, and the (1 + |arg|) factor carries the
relative error of the exponent's argument into the exponential. A derivation, not a fit. An element is DECIDED when its float64
value lies farther than the margin from the nearest bf16 rounding boundary: it must match the correctly rounded bf16 bit for bit.
An undecided element must be the correct rounding of some value within the margin of the reference: the bf16 neighbour across
the boundary (where cancellation leaves |y| below 2^-9 T, so that the margin spans several bf16 steps: any of them). At most UNDECIDED_CAP of a case may be undecided (asserted on the reference).
"""
import math

import torch

Q = 2.0 ** -7
U18 = 2.0 ** -18
UNDECIDED_CAP = 0.05
LN_EPS = 1e-5
GELU_LOG2 = 2.4554669595930157      # 1.702 log2(e): the constant of quick_gelu (csrc/gemm_bf16.h)

EPI_F32, EPI_BIAS, EPI_QGELU, EPI_RESID, EPI_PATCH, EPI_FOLD, EPI_FOLD_QGELU = 0, 1, 2, 3, 4, 7, 8


# ------------------------------------------------------------------------------------------------ operands
def _mix(x):
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def hash2(rows, cols, seed, device):
    """int64 [rows, cols] in 0 .. 2^32 - 1: the same on every device"""
    i = torch.arange(rows, device=device, dtype=torch.int64)[:, None]
    j = torch.arange(cols, device=device, dtype=torch.int64)[None, :]
    return _mix(_mix((i * 0x9E3779B1 + seed * 0x632BE5AB) & 0xFFFFFFFF) ^ ((j * 0x85EBCA77 + 0x27D4EB2F) & 0xFFFFFFFF))


def signed_ints(rows, cols, seed, device, top=4):
    """float64 [rows, cols]: nonzero integers in +-1 .. +-top (top a power of two)"""
    h = hash2(rows, cols, seed, device)
    return (((h & (top - 1)) + 1) * (1 - 2 * ((h >> 8) & 1))).double()


def weight_shift(K):
    """s with 2 sqrt(K) / 2^s in (0.7, 1.42]: |acc| then has standard deviation 7.5 sqrt(K) 2^-s = 2.7 .. 5.3"""
    return math.ceil(math.log2(K) / 2 + 0.5 - 1e-9)


class Case:
    """The operands of one GEMM shape, as float64 tensors on `device` (every one exactly representable in the type the kernel
    reads it in), and the float64 references of the epilogues."""

    def __init__(self, M, N, K, kind="wide", seed=1, device="cpu", patch=None):
        assert kind in ("wide", "fold", "stats")
        self.M, self.N, self.K, self.kind, self.seed, self.device, self.patch = M, N, K, kind, seed, device, patch
        s0 = seed * 16
        if kind != "stats":
            self.s = weight_shift(K) + (kind == "fold")
            self.A = signed_ints(M, K, s0 + 1, device)
            self.W = signed_ints(N, K, s0 + 2, device) * 2.0 ** -self.s
            self.bias = signed_ints(1, N, s0 + 3, device, top=8)[0] * Q
            self.x0 = signed_ints(M, N, s0 + 4, device, top=32) * Q
        else:
            self.s = 7
            self.A = signed_ints(M, K, s0 + 1, device, top=1)
            self.W = signed_ints(N, K, s0 + 2, device, top=1) * 2.0 ** -7
            self.bias = signed_ints(1, N, s0 + 3, device, top=4)[0] * Q
            h = hash2(M, N, s0 + 4, device)
            self.x0 = (2.25 + (h & 31).double() * 2.0 ** -6) * (1 - 2 * ((h >> 8) & 1)).double()
        self.quantum = min(Q, 2.0 ** -self.s)
        self.acc = self.A @ self.W.T
        if patch is not None:       # (G patches, T tokens per image): the position table [T, N]
            self.pos = signed_ints(patch[1], N, s0 + 5, device, top=32) * Q
        self._fold = None

    # -------------------------------------------------------------------------------------------- references (float64)
    def ref_f32(self):
        return self.acc

    def ref_bias(self):
        return self.acc + self.bias

    def ref_qgelu(self):
        return quick_gelu_margin(self.acc + self.bias)

    def ref_resid(self):
        return self.x0 + self.acc + self.bias

    def ref_patch_rows(self):
        """(the output row of GEMM row m, its float64 value): row (m / G) T + 1 + m % G = acc + pos[1 + m % G]"""
        G, T = self.patch
        m = torch.arange(self.M, device=self.device)
        return (m // G) * T + 1 + m % G, self.acc + self.pos[1 + m % G]

    def fold_operands(self):
        """ln_stats f64 [M][K/64][2] = (sum, sumsq) per 64 columns of A (small integers: exact in f32), c = row sums of W,
        b' = bias, and the rows' (mean, rstd) in float64"""
        if self._fold is None:
            p = self.A.view(self.M, self.K // 64, 64)
            stats = torch.stack([p.sum(-1), (p * p).sum(-1)], -1).contiguous()
            c = self.W.sum(1)
            mean = self.A.mean(1, keepdim=True)
            var = (self.A * self.A).mean(1, keepdim=True) - mean * mean
            self._fold = stats, c, mean, 1.0 / torch.sqrt(var + LN_EPS)
        return self._fold

    def ref_fold(self, gelu):
        """(value, margin) of rstd (acc - mean c) + b' (then QuickGELU)"""
        _, c, mean, rstd = self.fold_operands()
        y = rstd * (self.acc - mean * c) + self.bias
        T = rstd * (self.acc.abs() + (mean * c).abs()) + self.bias.abs()
        if not gelu:
            return y, U18 * T
        return quick_gelu(y), U18 * T * (1.0 + (GELU_LOG2 * y).abs())

    def stats64(self, v):
        """f64 [M][N/64][2]: (sum, sumsq) per 64 columns of v"""
        p = v.view(v.shape[0], v.shape[1] // 64, 64)
        return torch.stack([p.sum(-1), (p * p).sum(-1)], -1).contiguous()

    # -------------------------------------------------------------------------------------------- conditions
    def check(self, what):
        """Assert on the reference alone what the comparison of `what` relies on. what: 'f32' (a), 'bf16' (a, c, d on acc + bias),
        'resid' (a; kind stats: b, and c, d on the rows' bf16 copy), 'resid16' (kind stats: a, b of the STORED rows, c, d),
        'qgelu' / 'fold' / 'fold_qgelu' (a and the undecided cap). Returns the figures."""
        fig = {}
        amax, wmax = self.A.abs().max().item(), self.W.abs().max().item()
        extra = self.bias.abs().max().item() + (self.x0.abs().max().item() if what in ("resid", "resid16") else 0.0)
        if what == "patch":
            extra = self.pos.abs().max().item()
        fig["a"] = (self.K * amax * wmax + extra) / self.quantum
        assert fig["a"] < 2 ** 24, fig
        assert (self.A != 0).all() and (self.W != 0).all() and (self.bias != 0).all()
        if what in ("f32", "patch"):
            return fig
        if what in ("qgelu", "fold", "fold_qgelu"):
            if what != "qgelu":
                _, _, mean, rstd = self.fold_operands()
                assert (mean.abs() * rstd <= 1.0).all()           # |mean| <= sigma
            v, margin = self.ref_qgelu() if what == "qgelu" else self.ref_fold(what == "fold_qgelu")
            fig["undecided"] = (~bf16_round(v, margin).decided).double().mean().item()
            assert fig["undecided"] <= UNDECIDED_CAP, fig
            return fig
        v = self.ref_bias() if what == "bf16" else self.ref_resid()
        if what in ("resid", "resid16"):
            if self.kind != "stats":
                return fig
            stored = bf16_round(v).value if what == "resid16" else v
            fig["b"] = 64 * (stored * stored).max().item() / Q ** 2
            assert fig["b"] < 2 ** 24, fig
            assert (torch.remainder(stored, Q) == 0).all()
        r = bf16_round(v)
        fig["ties_up"], fig["ties_down"] = r.tie_up.double().mean().item(), r.tie_down.double().mean().item()
        fig["inexact"] = (r.value != v).double().mean().item()
        assert fig["ties_up"] >= 0.05 and fig["ties_down"] >= 0.05 and fig["inexact"] >= 0.25, fig
        return fig


def quick_gelu(x):
    return x / (1.0 + torch.exp(-1.702 * x))


def quick_gelu_margin(x):
    y = quick_gelu(x)
    return y, U18 * y.abs() * (1.0 + (GELU_LOG2 * x).abs())


# ------------------------------------------------------------------------------------------------ bf16 rounding in float64
class Bf16Round:
    pass


def bf16_round(v, margin=None):
    """The correct (one rounding, nearest even) bf16 of float64 values, worked in float64 (normal range only):
    .value f64, .bits int32 (the 16-bit pattern), .lo / .hi f64 (the bf16 neighbours below / above in magnitude; lo = hi = v
    where v is a bf16 number), .tie_up / .tie_down (exact ties, rounding up / down in magnitude), .decided (farther than
    `margin` from the nearest rounding boundary; all True without a margin)."""
    r = Bf16Round()
    mant, expo = torch.frexp(v)                       # v = mant 2^expo, |mant| in [0.5, 1)
    q = ((expo.to(torch.int64) - 8 + 1023) << 52).view(torch.float64)     # 2^(expo - 8), from its bits: the bf16 grid of v's binade
    t = (mant * 256.0).abs()
    fl = torch.floor(t)
    rt = torch.round(t)                               # half to even: the integer's parity is the mantissa's last bit
    sign = torch.where(v < 0, -1.0, 1.0).to(v.dtype)
    r.value = sign * rt * q
    r.lo, r.hi = sign * fl * q, sign * torch.ceil(t) * q
    frac = t - fl
    r.tie_up = (frac == 0.5) & (rt > t)
    r.tie_down = (frac == 0.5) & (rt < t)
    f = r.value.float()
    assert (f.double() == r.value).all()
    r.bits = (f.view(torch.int32) >> 16) & 0xFFFF
    if margin is None:
        r.decided = torch.ones_like(v, dtype=torch.bool)
    else:
        # the boundaries of the interval that rounds to rt: rt +- 0.5, except below a power of two (rt = 128), where the grid
        # halves: 127.75
        lower = torch.where(rt == 128.0, torch.full_like(t, 127.75), rt - 0.5)
        dist = torch.minimum(rt + 0.5 - t, t - lower) * q
        r.decided = (dist > margin) | (v == 0)
    return r


def bits_of(x_bf16):
    """the 16-bit patterns of a bf16 tensor as int32"""
    return x_bf16.view(torch.int16).to(torch.int32) & 0xFFFF


def bf16_tensor(v):
    """float64 values that ARE bf16 numbers -> a bf16 tensor (asserted exact)"""
    b = v.to(torch.bfloat16)
    assert (b.double() == v).all()
    return b


def f32_tensor(v):
    f = v.float()
    assert (f.double() == v).all()
    return f


# ------------------------------------------------------------------------------------------------ comparison
def _report(bad, got, want, tile_h, what):
    idx = bad.nonzero()
    first = [(int(m), int(n), got[m, n].item(), want[m, n].item()) for m, n in idx[:6].tolist()]
    ms, ns = idx[:, 0], idx[:, 1]
    return ("%s: %d of %d elements differ; first (m, n, got, want): %s; distinct m %% %d: %s; n %% 128: %s; n %% 64: %s"
            % (what, idx.shape[0], bad.numel(), first, tile_h, torch.unique(ms % tile_h).tolist()[:48],
               torch.unique(ns % 128).tolist()[:48], torch.unique(ns % 64).tolist()[:48]))


def assert_f32_exact(got, v, tile_h=128, what="f32 output"):
    """got f32 [M, N] equals the float64 value v (which must be an f32 number) bit for bit"""
    want = f32_tensor(v)
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bad.any(), _report(bad, got, want, tile_h, what)


def assert_untouched(got, prefill, what="pad / sentinel rows"):
    """got (any 2- or 4-byte type) holds the bit patterns of `prefill` (NaN patterns included)"""
    it = torch.int16 if got.element_size() == 2 else torch.int32
    bad = got.contiguous().view(it) != prefill.contiguous().view(it)
    if bad.any():
        idx = bad.reshape(bad.shape[0], -1).any(1).nonzero().flatten().tolist()
        raise AssertionError("%s: %d elements differ from what was there before the call, in rows %s (of this slice)"
                             % (what, int(bad.sum()), idx[:16]))


def assert_bf16_rounded(got, v, margin=None, tile_h=128, what="bf16 output"):
    """got bf16 [M, N] is the one correct rounding of v where that is decided, and the rounding of a value within the margin of v
    elsewhere. Returns observed_ratio (None without a margin)."""
    r = bf16_round(v, margin)
    gb = bits_of(got)
    g64 = got.double()
    if margin is None:
        bad = gb != r.bits
    else:
        # undecided: the correct rounding of SOME value within the margin of v — the neighbour across the boundary, or, where
        # cancellation leaves |v| so far below T that the margin spans several bf16 steps, any bf16 number of that span
        bad = torch.where(r.decided, gb != r.bits, (g64 < bf16_round(v - margin).value) | (g64 > bf16_round(v + margin).value))
    assert not bad.any(), _report(bad, g64, r.value, tile_h, what)
    if margin is None:
        return None
    return observed_ratio(got, v, margin)


def observed_ratio(got, v, margin):
    """The largest |f32 value before the rounding - v| / margin the bf16 output proves: an element that differs from the correct
    rounding of v shows that the kernel's value lay on the other side of the boundary between the two, at least
    |boundary - v| away. 0 where every element is the correct rounding. Recorded, not asserted."""
    r = bf16_round(v)
    g64 = got.double()
    off = (g64 != r.value) & (margin > 0)
    if not off.any():
        return 0.0
    boundary = (g64 + r.value) / 2
    return ((boundary - v).abs()[off] / margin[off]).max().item()


# ------------------------------------------------------------------------------------------------ the GPU file's cases
# gemm16_kernel: (buffers, waves) -> the options that force the form at a small grid (defaults: gemm_s3 1, gemm_w8 1,
# gemm_w8_max_wgs 512), the tile heights that have it, and the K-tile counts it can run (three buffers need K >= 256)
OPTION_DEFAULTS = {"gemm_s3": 1, "gemm_w8": 1, "gemm_w8_max_wgs": 512, "gemm_skinny": 1, "gemm_splitk": 1}
FORMS = {
    (3, 8): ({}, (128,), (4, 12)),
    (3, 4): ({"gemm_w8": 0}, (128, 160, 192), (4, 12)),
    (2, 8): ({"gemm_s3": 0}, (128,), (1, 2, 3, 4, 12)),
    (2, 4): ({"gemm_s3": 0, "gemm_w8_max_wgs": 0}, (128, 160, 192), (1, 2, 3, 4, 12)),
}
TILE_N = 256                       # two column tiles; M = two row tiles
FOLD_KTILES = (2, 4, 12, 16)       # the folded epilogues read K / 64 partials in pairs, 16 at the most
BAND_SHAPE = (7 * 128, 1024, 64)   # 8 column tiles: the banded order, 7 row tiles against bands of 5
G256_SHAPE = (512, 512)
G256_KTILES = (1, 2, 3, 12)
G256_FOLD_KTILES = (2, 12)
SPLITK_K = 1536                    # 2 x 2 tiles: 4 slices of 6 K-tiles, the fewest gemm_splitk_splits accepts
SKINNY_MS = (1, 17, 77, 128)
SKINNY_N, SKINNY_KS = 1040, (768, 2048)     # 4 K-quarters of 192; 8 slices of 256
P256_SHAPES = ((512, 512, 512, 512), (512, 512, 512, 300), (19 * 256, 14 * 256, 512, 19 * 256 - 100), (512, 768, 768, 257))
P160_SHAPES = ((320, 512, 256, 320), (320, 512, 768, 170), (320, 256, 384, 319))
RESID16_KTILES = (1, 2, 3, 12)
PIX_SHAPES = ((3, 64, 16, 256), (11, 64, 16, 512), (2, 64, 32, 256))     # (B, S, P, d)
PATCH_G, PATCH_T = 12, 13          # 128-, 160- and 192-row tiles all cut images


def ragged(M, bm):
    """an m_valid inside the last tile, off every 16-row sub-tile edge"""
    return M - bm + 21


def tile_cases():
    """every (M, N, K, kind, patch) the gemm16 / gemm256 / split-K / skinny tests build"""
    out = set()
    for (_, heights, ktiles) in FORMS.values():
        for bm in heights:
            for kt in ktiles:
                out.add((2 * bm, TILE_N, 64 * kt, "wide", (PATCH_G, PATCH_T)))
                out.add((2 * bm, TILE_N, 64 * kt, "stats", None))
    for bm in (128, 160, 192):
        for kt in FOLD_KTILES:
            out.add((2 * bm, TILE_N, 64 * kt, "fold", None))
        out.add((2 * bm, TILE_N, SPLITK_K, "wide", (PATCH_G, PATCH_T)))
        for kt in RESID16_KTILES:
            out.add((2 * bm, TILE_N, 64 * kt, "stats", None))
    out.add(BAND_SHAPE + ("wide", (PATCH_G, PATCH_T)))
    for kt in G256_FOLD_KTILES:
        out.add(G256_SHAPE + (64 * kt, "fold", None))
    for kt in G256_KTILES:
        out.add(G256_SHAPE + (64 * kt, "wide", None))
        out.add(G256_SHAPE + (64 * kt, "stats", None))
    for M in SKINNY_MS:
        for K in SKINNY_KS:
            out.add((M, SKINNY_N, K, "wide", (PATCH_G, PATCH_T)))
    for (M, N, K, _) in P256_SHAPES:
        out.add((M, N, K, "wide", None))
        out.add((M, N, K, "fold", None))
    for (M, N, K, _) in P160_SHAPES:
        out.add((M, N, K, "stats", None))
    return sorted(out, key=str)


_cache = {}


def case(M, N, K, kind="wide", patch=None, device="cpu"):
    """the shared, unchanged Case of a shape (built once per device)"""
    key = (M, N, K, kind, patch, str(device))
    if key not in _cache:
        if len(_cache) > 24:
            _cache.clear()
        _cache[key] = Case(M, N, K, kind, seed=1 + (M * 31 + N * 7 + K) % 1000, device=device, patch=patch)
    return _cache[key]


def pixel_case(B, S, P, d, device="cpu"):
    """pixels f64 [B,3,S,S] (integers +-1..+-4: exact in bf16), W f64 [d, 3 P^2], pos f64 [G^2 + 1, d], and the float64 patch rows
    [B G^2, d] = patch . W^T + pos[1 + patch]"""
    G, K = S // P, 3 * P * P
    px = signed_ints(B * 3 * S, S, 900 + B + P, device).view(B, 3, S, S)
    W = signed_ints(d, K, 901 + B + P, device) * 2.0 ** -weight_shift(K)
    pos = signed_ints(G * G + 1, d, 902 + B + P, device, top=32) * Q
    patches = px.reshape(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, K)
    rows = patches @ W.T + pos[1:].repeat(B, 1)
    assert (K * 16 * 2.0 ** -weight_shift(K) + pos.abs().max().item()) / Q < 2 ** 24
    return px, W, pos, rows

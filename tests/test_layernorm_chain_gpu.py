"""The LayerNorm chain around the LayerNorm-folded GEMMs, kernel by kernel (include/mmiss_debug.h), against float64 on the host:
layernorm16_kernel, the rowmap path of layernorm_kernel, layernorm_stats_kernel<false / true>, prelayernorm_skinny_kernel,
row_stats_kernel, ln_finalize_kernel, fold_ln_weights_kernel — the producers of the statistics the folded epilogues consume —
then the chain end to end into the persistent GEMM's folded epilogue, and the statistics the residual GEMMs leave behind.

Inputs follow test_kernels_gpu.py::test_layernorm (3 N(0,1) + 0.5); `offset` rows sit at 3 N(0,1) + 30, mean = 10 std, where
E[x^2] - mean^2 cancels two decimal digits. Every output buffer has one sentinel row behind its M rows that must stay untouched.

Summation bounds: an f32 sum of n terms in ANY order is within (n - 1) u sum|x_i| of the exact sum (u = 2^-24), a sum of n rounded
products within n u sum|x_i y_i|. The tests use n u for both: no tuned number."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DS = [64, 128, 320, 512, 768, 1024]      # (all multiples of 8: layernorm16 takes every one; 320 = a partly filled 256-column pass)
MS = [1, 2, 7, 8, 9, 333]                # an odd last row of a two-row wave, partly filled workgroups of 4 / 8 rows
KINDS = ["plain", "offset"]
EPS = 1e-5
SENT = -7.0


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch, _lib, lib


def _p(t):
    return None if t is None else t.data_ptr()


def _rows(torch, M, d, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, d, device="cuda", generator=g) * 3 + (30.0 if kind == "offset" else 0.5)
    gam = torch.randn(d, device="cuda", generator=g)
    bet = torch.randn(d, device="cuda", generator=g)
    return x, gam, bet


def _with_sentinel(torch, t):
    """t with one more row of SENT behind it (a fresh buffer)."""
    return torch.cat([t, torch.full((1,) + tuple(t.shape[1:]), SENT, device=t.device, dtype=t.dtype)]).contiguous()


def _sentinel_buf(torch, shape, dtype):
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), SENT, device="cuda", dtype=dtype)


def _untouched(t, M):
    return bool((t[M] == SENT).all())


def _f64(t):
    return t.detach().double().cpu()


def _ln64(torch, x, gam, bet, eps=EPS):
    x, gam, bet = _f64(x), _f64(gam), _f64(bet)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gam + bet


def _bits(t):
    import torch

    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_sums(torch, got_sum, got_sq, y, n, what):
    """got_sum / got_sq f32 [...] against the f64 sums over the last axis of y (n terms each), bound n u sum|y| and n u sum y^2."""
    y = _f64(y)
    s, a, q = y.sum(-1), y.abs().sum(-1), (y * y).sum(-1)
    es, eq = (_f64(got_sum) - s).abs(), (_f64(got_sq) - q).abs()
    print(what, "sum err / bound max", float((es / (n * U * a).clamp_min(1e-300)).max()), "sumsq err / bound max",
          float((eq / (n * U * q).clamp_min(1e-300)).max()))
    assert (es <= n * U * a).all(), (what, "sum", float(es.max()))
    assert (eq <= n * U * q).all(), (what, "sumsq", float(eq.max()))


# ------------------------------------------------------------------------------------------------ callers
def _layernorm(env, x, gam, bet, out, out_bf16, M, d):
    torch, _lib, lib = env
    _lib.check(lib.mmiss_dbg_layernorm(0, None, _p(x), _p(gam), _p(bet), _p(out), out_bf16, M, d, EPS))
    torch.cuda.synchronize()


def _prestats(env, x, gam, bet, xb, stats, M, d, parts, lean=0, cls=None, pos=None, T=1):
    torch, _lib, lib = env
    _lib.check(lib.mmiss_dbg_prelayernorm_stats(0, None, _p(x), _p(gam), _p(bet), _p(xb), _p(stats), M, d, parts, EPS, lean,
                                                _p(cls), _p(pos), T))
    torch.cuda.synchronize()


def _row_stats(env, x, stats, xb, M, d, parts):
    torch, _lib, lib = env
    _lib.check(lib.mmiss_dbg_row_stats(0, None, _p(x), _p(stats), _p(xb), M, d, parts))
    torch.cuda.synchronize()


def _fold(env, W, gam, bet, bias, N, K):
    torch, _lib, lib = env
    wf = _sentinel_buf(torch, (N, K), torch.bfloat16)
    c = _sentinel_buf(torch, (N,), torch.float32)
    bf = _sentinel_buf(torch, (N,), torch.float32)
    _lib.check(lib.mmiss_dbg_fold_ln_weights(0, None, _p(W), _p(gam), _p(bet), _p(bias), _p(wf), _p(c), _p(bf), N, K))
    torch.cuda.synchronize()
    assert _untouched(wf, N) and _untouched(c, N) and _untouched(bf, N)
    return wf[:N], c[:N], bf[:N]


# ------------------------------------------------------------------------------------------------ layernorm16
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
def test_layernorm16(env, d, kind):
    """bf16 rows -> bf16 rows against the f64 LayerNorm of the widened rows; tolerance of test_layernorm's bf16 branch. A wave
    takes two rows: every M runs on a prefix of the same rows, and a row must not depend on M — for M = 7 row 6 is the odd last
    row ('computed twice, stored once'), for M = 8 it has a neighbour."""
    torch, _lib, lib = env
    x, gam, bet = _rows(torch, max(MS), d, kind, 16 * d + len(kind))
    x16 = x.to(torch.bfloat16)
    ref = _ln64(torch, x16.float(), gam, bet)
    outs = {}
    for M in MS:
        out = _sentinel_buf(torch, (M, d), torch.bfloat16)
        _lib.check(lib.mmiss_dbg_layernorm16(0, None, _p(x16), _p(gam), _p(bet), _p(out), M, d, EPS))
        torch.cuda.synchronize()
        assert _untouched(out, M), M
        assert torch.allclose(_f64(out[:M].float()), ref[:M], rtol=2 ** -8, atol=1e-3), (M, float((_f64(out[:M].float()) - ref[:M]).abs().max()))
        outs[M] = out[:M]
    assert torch.equal(_bits(outs[7][6]), _bits(outs[8][6]))
    for M in MS:
        assert torch.equal(_bits(outs[M]), _bits(outs[max(MS)][:M])), M


def test_entry_points_refuse_shapes_the_kernels_do_not_take(env):
    torch, _lib, lib = env
    x = torch.zeros(4, 1032, device="cuda", dtype=torch.bfloat16)
    g = torch.zeros(1032, device="cuda")
    UNSUPPORTED = -5   # MMISS_ERR_UNSUPPORTED (include/mmiss.h)
    for M, d in ((2, 12), (2, 1032), (2, 0), (0, 64)):
        assert lib.mmiss_dbg_layernorm16(0, None, _p(x), _p(g), _p(g), _p(x), M, d, EPS) == UNSUPPORTED, (M, d)
    s = torch.zeros(64, device="cuda")
    i = torch.zeros(4, device="cuda", dtype=torch.int32)
    for M, d in ((0, 64), (1, 6), (1, 1028)):
        assert lib.mmiss_dbg_layernorm_gather(0, None, _p(x), _p(g), _p(g), _p(x), 0, _p(i), M, d, EPS) == UNSUPPORTED, (M, d)
    assert lib.mmiss_dbg_ln_finalize(0, None, _p(s), _p(s), 2, 3, 192, EPS) == UNSUPPORTED       # an odd number of partials
    assert lib.mmiss_dbg_ln_finalize(0, None, _p(s), _p(s), 0, 2, 128, EPS) == UNSUPPORTED
    assert lib.mmiss_dbg_prelayernorm_skinny(0, None, _p(s), _p(s), _p(s), _p(s), _p(s), _p(s), _p(s), 1, 1, 24, EPS) == UNSUPPORTED
    assert lib.mmiss_dbg_prelayernorm_stats(0, None, _p(s), _p(s), _p(s), _p(s), _p(s), 1, 1028, 1, EPS, 0, None, None, 1) == UNSUPPORTED
    assert lib.mmiss_dbg_prelayernorm_stats(0, None, _p(s), _p(s), _p(s), _p(s), _p(s), 0, 64, 1, EPS, 0, None, None, 1) == UNSUPPORTED
    assert lib.mmiss_dbg_row_stats(0, None, _p(s), _p(s), None, 1, 6, 1) == UNSUPPORTED
    assert lib.mmiss_dbg_fold_ln_weights(0, None, _p(s), _p(s), _p(s), _p(s), _p(s), _p(s), _p(s), 0, 64) == UNSUPPORTED


# ------------------------------------------------------------------------------------------------ rowmap path of layernorm_kernel
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
def test_layernorm_gather(env, d, kind):
    """Out row r = LayerNorm(x row rowmap[r]): the same bits as mmiss_dbg_layernorm on the gathered rows. rowmap: a permutation
    of 13 source rows, cut or repeated to M entries."""
    torch, _lib, lib = env
    R = 13
    x, gam, bet = _rows(torch, R, d, kind, 17 * d + len(kind))
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(d)).tolist()
    for M in MS:
        rowmap = torch.tensor([perm[(5 * i) % R] if i % 3 else perm[i % 4] for i in range(M)], device="cuda", dtype=torch.int32)
        gathered = x[rowmap.long()].contiguous()
        for out_bf16, dtype in ((0, torch.float32), (1, torch.bfloat16)):
            want = torch.zeros(M, d, device="cuda", dtype=dtype)
            _layernorm(env, gathered, gam, bet, want, out_bf16, M, d)
            got = _sentinel_buf(torch, (M, d), dtype)
            _lib.check(lib.mmiss_dbg_layernorm_gather(0, None, _p(x), _p(gam), _p(bet), _p(got), out_bf16, _p(rowmap), M, d, EPS))
            torch.cuda.synchronize()
            assert _untouched(got, M), (M, out_bf16)
            assert torch.equal(_bits(got[:M]), _bits(want)), (M, out_bf16)


# ------------------------------------------------------------------------------------------------ layernorm_stats_kernel
def _parts_of(d):
    return max(1, d // 64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
def test_prelayernorm_stats(env, d, kind):
    """layernorm_stats_kernel<false>: LayerNorm in place, the bf16 copy, (sum, sumsq) of the new rows in statistics slot 0."""
    torch, _lib, lib = env
    parts = _parts_of(d)
    for M in MS:
        x, gam, bet = _rows(torch, M, d, kind, 18 * d + M)
        ref = _ln64(torch, x, gam, bet)
        xbuf = _with_sentinel(torch, x)
        xb = _sentinel_buf(torch, (M, d), torch.bfloat16)
        st = _sentinel_buf(torch, (M, parts, 2), torch.float32)
        _prestats(env, xbuf, gam, bet, xb, st, M, d, parts)
        assert _untouched(xbuf, M) and _untouched(xb, M) and _untouched(st, M), M
        y = xbuf[:M]
        assert torch.allclose(_f64(y), ref, rtol=1e-5, atol=1e-5), (M, float((_f64(y) - ref).abs().max()))
        assert torch.equal(_bits(xb[:M]), _bits(y.to(torch.bfloat16))), M
        _assert_sums(torch, st[:M, 0, 0], st[:M, 0, 1], y, d, f"prelayernorm_stats d={d} {kind} M={M}")
        assert (st[:M, 1:] == 0).all(), M


@pytest.mark.parametrize("T", [5, 50])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
def test_prelayernorm_stats_lean(env, d, kind, T):
    """layernorm_stats_kernel<true>: the same bits as the non-lean run on rows whose token-0 rows were first set to cls + pos[0];
    the f32 rows are only read. The token-0 rows of the input hold 1e3: a row that was not replaced shows."""
    torch, _lib, lib = env
    parts = _parts_of(d)
    g = torch.Generator(device="cuda").manual_seed(19 * d + T)
    cls = torch.randn(d, device="cuda", generator=g)
    pos = torch.randn(T, d, device="cuda", generator=g)
    for M in MS:
        x, gam, bet = _rows(torch, M, d, kind, 19 * d + M)
        x[0::T] = 1e3
        filled = x.clone()
        filled[0::T] = cls + pos[0]
        xb_want = torch.zeros(M, d, device="cuda", dtype=torch.bfloat16)
        st_want = torch.zeros(M, parts, 2, device="cuda")
        _prestats(env, filled, gam, bet, xb_want, st_want, M, d, parts)
        xbuf = _with_sentinel(torch, x)
        xb = _sentinel_buf(torch, (M, d), torch.bfloat16)
        st = _sentinel_buf(torch, (M, parts, 2), torch.float32)
        _prestats(env, xbuf, gam, bet, xb, st, M, d, parts, lean=1, cls=cls, pos=pos, T=T)
        assert _untouched(xbuf, M) and _untouched(xb, M) and _untouched(st, M), M
        assert torch.equal(_bits(xbuf[:M]), _bits(x)), M
        assert torch.equal(_bits(xb[:M]), _bits(xb_want)), M
        assert torch.equal(_bits(st[:M]), _bits(st_want)), M


# ------------------------------------------------------------------------------------------------ prelayernorm_skinny_kernel
@pytest.mark.parametrize("T", [5, 50])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
def test_prelayernorm_skinny(env, d, kind, T):
    """CLS rows, LayerNorm in place, bf16 copy and (sum, sumsq) per 16 columns in one launch: against f64, and the rows bit-equal
    to mmiss_dbg_layernorm in place on the same input with the CLS rows pre-filled."""
    torch, _lib, lib = env
    g = torch.Generator(device="cuda").manual_seed(20 * d + T)
    cls = torch.randn(d, device="cuda", generator=g)
    pos = torch.randn(T, d, device="cuda", generator=g)
    for M in MS:
        x, gam, bet = _rows(torch, M, d, kind, 20 * d + M)
        x[0::T] = 1e3
        filled = x.clone()
        filled[0::T] = cls + pos[0]
        ref = _ln64(torch, filled, gam, bet)
        xbuf = _with_sentinel(torch, x)
        xb = _sentinel_buf(torch, (M, d), torch.bfloat16)
        st = _sentinel_buf(torch, (M, d // 16, 2), torch.float32)
        _lib.check(lib.mmiss_dbg_prelayernorm_skinny(0, None, _p(xbuf), _p(cls), _p(pos), _p(gam), _p(bet), _p(xb), _p(st), M, T, d, EPS))
        torch.cuda.synchronize()
        assert _untouched(xbuf, M) and _untouched(xb, M) and _untouched(st, M), M
        y = xbuf[:M]
        assert torch.allclose(_f64(y), ref, rtol=1e-5, atol=1e-5), (M, float((_f64(y) - ref).abs().max()))
        assert torch.equal(_bits(xb[:M]), _bits(y.to(torch.bfloat16))), M
        _assert_sums(torch, st[:M, :, 0], st[:M, :, 1], y.view(M, d // 16, 16), 16, f"prelayernorm_skinny d={d} {kind} M={M}")
        _layernorm(env, filled, gam, bet, filled, 0, M, d)
        assert torch.equal(_bits(y), _bits(filled)), M


# ------------------------------------------------------------------------------------------------ row_stats_kernel
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
def test_row_stats(env, d, kind):
    torch, _lib, lib = env
    parts = _parts_of(d)
    for M in MS:
        x, _, _ = _rows(torch, M, d, kind, 21 * d + M)
        st = _sentinel_buf(torch, (M, parts, 2), torch.float32)
        xb = _sentinel_buf(torch, (M, d), torch.bfloat16)
        _row_stats(env, x, st, xb, M, d, parts)
        assert _untouched(st, M) and _untouched(xb, M), M
        _assert_sums(torch, st[:M, 0, 0], st[:M, 0, 1], x, d, f"row_stats d={d} {kind} M={M}")
        assert (st[:M, 1:] == 0).all(), M
        assert torch.equal(_bits(xb[:M]), _bits(x.to(torch.bfloat16))), M
        st2 = _sentinel_buf(torch, (M, parts, 2), torch.float32)
        _row_stats(env, x, st2, None, M, d, parts)     # no bf16 copy asked for
        assert torch.equal(_bits(st2), _bits(st)), M


# ------------------------------------------------------------------------------------------------ ln_finalize_kernel
def _finalize_ref(stats, d, eps=EPS):
    """(mean, rstd) in f64 from the f32 partials [M][parts][2], and the tolerances of an f32 evaluation of the same formula."""
    s, q = stats[..., 0].astype(np.float64), stats[..., 1].astype(np.float64)
    parts = s.shape[1]
    mean, a1, e2 = s.sum(1) / d, np.abs(s).sum(1) / d, q.sum(1) / d
    var = np.maximum(e2 - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    tol_mean = parts * U * a1
    dvar = U * (parts * e2 + 2 * parts * np.abs(mean) * a1 + mean * mean + var)
    tol_rstd = rstd * (0.5 * dvar / (var + eps) + 8 * U)
    return mean, rstd, tol_mean, tol_rstd


def _finalize_f32(stats, d, eps=EPS, pairwise=False):
    """The formula in f32 numpy (sequential or pairwise sums of the partials): what the tolerance was confirmed on."""
    s, q = stats[..., 0], stats[..., 1]
    if pairwise:
        while s.shape[1] > 1:
            if s.shape[1] % 2:
                s, q = np.pad(s, ((0, 0), (0, 1))), np.pad(q, ((0, 0), (0, 1)))
            s, q = s[:, 0::2] + s[:, 1::2], q[:, 0::2] + q[:, 1::2]
        s1, s2 = s[:, 0], q[:, 0]
    else:
        s1, s2 = np.zeros(len(s), np.float32), np.zeros(len(s), np.float32)
        for i in range(s.shape[1]):
            s1, s2 = s1 + s[:, i], s2 + q[:, i]
    mean = s1 / np.float32(d)
    var = np.maximum(s2 / np.float32(d) - mean * mean, np.float32(0))
    return mean, np.float32(1) / np.sqrt(var + np.float32(eps))


def _random_partials(rng, M, parts, offset):
    """Partials no row produced: per 64 columns a sum around 64 * offset and a sum of squares above sum^2 / 64 (a variance > 0);
    row 0 all zeros (rstd = eps^-1/2: the epsilon is inside the root), row 1 a constant row (variance 0 up to cancellation)."""
    sd = 3.0
    s = 64 * (offset + 0.3 * sd * rng.standard_normal((M, parts)))
    q = s * s / 64 + 64 * sd * sd * rng.uniform(0.5, 1.5, (M, parts))
    st = np.stack([s, q], -1).astype(np.float32)
    st[0] = 0
    if M > 1:
        st[1, :, 0], st[1, :, 1] = 64 * 0.5, 64 * 0.25
    return st


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("parts", [2, 8, 12, 16])
def test_ln_finalize(env, parts, kind):
    """(mean, rstd) = (S1 / d, 1 / sqrt(max(S2 / d - mean^2, 0) + eps)) from `parts` partial (sum, sumsq) per row, against f64 on
    the same partials. Tolerance, for an f32 evaluation in any summation order (u = 2^-24, P = parts, A1 = sum|s_i| / d,
    E2 = S2 / d = var + mean^2):
      mean:  P - 1 additions and one division                      |d mean|  <= P u A1
      E2:    the same on non-negative terms                        |d E2|    <= P u E2
      mean^2: 2 |mean| |d mean| + one rounding                     |d mean^2| <= 2 P u |mean| A1 + u mean^2
      var = E2 - mean^2 and one rounding                           |d var|   <= u (P E2 + 2 P |mean| A1 + mean^2 + var)
      rstd = (var + eps)^-1/2: half the relative error of var + eps, and the add, the root and the reciprocal (<= 8 u in all)
                                                                   |d rstd| / rstd <= |d var| / (2 (var + eps)) + 8 u
    On rows with one sign this is u ((P + 1) + (3 P + 1) mean^2 / var) / 2: the cancellation of the offset rows (mean^2 / var =
    100) costs 1.5e-4 at P = 16. The first-order figure 2^-23 (1 + mean^2 / var) — four roundings, not 3 P — is NOT a bound: f32
    numpy restatements of the formula exceed it themselves (20 000 rows: up to 1.7 x on plain rows, 2.3 x on offset rows with
    sequential sums, 1.5 x with pairwise sums), and stay within half of the bound above (asserted below for both orders). The
    partials come from row_stats on every 64-column slice of real rows, and from _random_partials."""
    torch, _lib, lib = env
    d = 64 * parts
    rng = np.random.default_rng(parts + len(kind))
    for M in MS:
        x, _, _ = _rows(torch, M, d, kind, 22 * d + M)
        from_rows = torch.zeros(M * parts, 1, 2, device="cuda")
        _row_stats(env, x.view(M * parts, 64), from_rows, None, M * parts, 64, 1)     # [M * parts][1][2] = [M][parts][2]
        for name, st in (("row_stats", from_rows.view(M, parts, 2)),
                         ("random", torch.from_numpy(_random_partials(rng, M, parts, 30.0 if kind == "offset" else 0.5)).cuda())):
            out = _sentinel_buf(torch, (M, 2), torch.float32)
            _lib.check(lib.mmiss_dbg_ln_finalize(0, None, _p(st), _p(out), M, parts, d, EPS))
            torch.cuda.synchronize()
            assert _untouched(out, M), (name, M)
            host = st.cpu().numpy()
            mean, rstd, tol_mean, tol_rstd = _finalize_ref(host, d)
            got = out[:M].cpu().numpy().astype(np.float64)
            em, er = np.abs(got[:, 0] - mean), np.abs(got[:, 1] - rstd)
            print(f"ln_finalize parts={parts} {kind} {name} M={M}: mean err / tol max", float((em / np.maximum(tol_mean, 1e-300)).max()),
                  "rstd err / tol max", float((er / tol_rstd).max()), "rstd rel err max", float((er / rstd).max()))
            assert (em <= tol_mean).all(), (name, M, float(em.max()))
            assert (er <= tol_rstd).all(), (name, M, float((er / rstd).max()))
            for pairwise in (False, True):   # the tolerance holds for the f32 restatements too: it is the formula's, not the kernel's
                m32, r32 = _finalize_f32(host, d, pairwise=pairwise)
                assert (np.abs(m32 - mean) <= tol_mean).all() and (np.abs(r32 - rstd) <= tol_rstd).all(), (name, M, pairwise)
            if name == "row_stats":   # and the partials were the rows': the f64 statistics of x itself, to the partials' own rounding
                x64 = _f64(x)
                assert np.allclose(mean, x64.mean(1).numpy(), rtol=1e-5, atol=1e-6)
                assert np.allclose(rstd, 1 / np.sqrt(x64.var(1, unbiased=False).numpy() + EPS), rtol=1e-3 if kind == "offset" else 1e-4)


# ------------------------------------------------------------------------------------------------ fold_ln_weights_kernel
def _fold_inputs(torch, N, K, seed, w_scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = (torch.randn(N, K, device="cuda", generator=g) * (w_scale * K ** -0.5)).to(torch.bfloat16)
    gam = torch.randn(K, device="cuda", generator=g)
    bet = torch.randn(K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    return W, gam, bet, bias


@pytest.mark.parametrize("N,K", [(128, 128), (384, 768), (256, 1024)])
def test_fold_ln_weights(env, N, K):
    """W' = bf16(f32(W) gamma) bit for bit; c = row sums of the dequantised W' (K terms); b' = bias + sum beta W (K rounded
    products and the bias: K + 1 terms)."""
    torch, _lib, lib = env
    W, gam, bet, bias = _fold_inputs(torch, N, K, N + K)
    wf, c, bf = _fold(env, W, gam, bet, bias, N, K)
    assert torch.equal(_bits(wf), _bits((W.float() * gam).to(torch.bfloat16)))
    wf64 = _f64(wf.float())
    ec = (_f64(c) - wf64.sum(1)).abs()
    assert (ec <= K * U * wf64.abs().sum(1)).all(), float(ec.max())
    prod = _f64(W.float()) * _f64(bet)
    eb = (_f64(bf) - (_f64(bias) + prod.sum(1))).abs()
    assert (eb <= (K + 1) * U * (_f64(bias).abs() + prod.abs().sum(1))).all(), float(eb.max())
    print(f"fold_ln_weights {N}x{K}: c err / bound max", float((ec / (K * U * wf64.abs().sum(1))).max()), "b' err / bound max",
          float((eb / ((K + 1) * U * (_f64(bias).abs() + prod.abs().sum(1)))).max()))


# ------------------------------------------------------------------------------------------------ the chain
def test_chain_prelayernorm_fold_and_folded_gemm(env):
    """What the product does between the embeddings and the first QKV GEMM of a large call: prelayernorm_stats writes xb and its
    statistics, fold_ln_weights the folded weights; the persistent GEMM's folded epilogue (7) consumes both. Against torch's fp32
    layer_norm(xb) @ W^T + b with test_gemm_p256_persistent's tolerances (rtol 2^-7, atol 4e-3).
    The scale of W: the folded form multiplies by W' = bf16(W gamma), the reference by the unrounded W gamma (in
    test_gemm_p256_persistent both sides use the same rounded weights). That rounding — up to 2^-9 relative per weight, uniform —
    moves an output by sigma = 2^-9 / sqrt(3) |xhat . W gamma|_2 = 1.1e-3 at unit output scale: over 65 536 outputs the EXACT
    folded form (f64, below) then misses atol 4e-3 on outputs near zero (max excess 1.3e-3 on the CPU). With W ~ 0.25 K^-1/2
    N(0,1) sigma is 2.8e-4 and the tolerance is 14 sigma; that the exact folded form of these very operands lies inside half
    the tolerance is asserted first, so the kernel is not held to a bound its own algebra cannot meet. At BOTH scales, unit scale
    included, the kernel is also held to that f64 folded form itself — the same rounded W', c, b' and statistics, as
    test_gemm_p256_persistent does — under the same rtol 2^-7, atol 4e-3."""
    torch, _lib, lib = env
    M, K, N = 256, 768, 256
    x, g0, b0 = _rows(torch, M, K, "plain", 99)
    xb = torch.zeros(M, K, device="cuda", dtype=torch.bfloat16)
    st = torch.zeros(M, K // 64, 2, device="cuda")
    _prestats(env, x, g0, b0, xb, st, M, K, K // 64)
    s64 = _f64(st).sum(1)
    mean = s64[:, :1] / K
    rstd = 1 / torch.sqrt(s64[:, 1:] / K - mean * mean + EPS)
    for w_scale in (0.25, 1.0):
        W, gam, bet, bias = _fold_inputs(torch, N, K, 100, w_scale=w_scale)
        wf, c, bf = _fold(env, W, gam, bet, bias, N, K)
        wf, c, bf = wf.contiguous(), c.contiguous(), bf.contiguous()
        out = _sentinel_buf(torch, (M, N), torch.bfloat16)
        _lib.check(lib.mmiss_dbg_gemm_p256(0, None, 7, _p(xb), _p(wf), _p(out), _p(bf), _p(c), _p(st), EPS, M, N, K, M, 0, None))
        torch.cuda.synchronize()
        assert _untouched(out, M)
        got = _f64(out[:M].float())
        exact = rstd * (_f64(xb.float()) @ _f64(wf.float()).T - mean * _f64(c)) + _f64(bf)
        # at either scale: the f64 folded form of the SAME rounded W', c, b' and statistics, under the same tolerance
        e1 = (got - exact).abs()
        print(f"chain w_scale={w_scale}: kernel vs exact folded form, max |d| / tol", float((e1 / (4e-3 + 2 ** -7 * exact.abs())).max()))
        assert torch.allclose(got, exact, rtol=2 ** -7, atol=4e-3), (w_scale, float(e1.max()))
        if w_scale == 1.0:
            continue
        ref = torch.nn.functional.layer_norm(xb.float(), (K,), gam, bet, EPS) @ W.float().T + bias
        tol = 4e-3 + 2 ** -7 * ref.abs()
        e0 = (exact - _f64(ref)).abs()
        print("chain: exact folded form vs reference, max |d| / tol", float((e0 / _f64(tol)).max()))
        assert (e0 <= 0.5 * _f64(tol)).all()       # (the other half: the output's bf16 rounding, 2^-9 |out|, and the f32 accumulation)
        err = (out[:M].float() - ref).abs()
        print("chain: max |d|", float(err.max()), "max |d| / tol", float((err / tol).max()))
        assert torch.allclose(out[:M].float(), ref, rtol=2 ** -7, atol=4e-3), float(err.max())


# ------------------------------------------------------------------------------------------------ residual GEMM statistics
@pytest.mark.parametrize("variant", [0, 160])
def test_residual_gemm_statistics_are_those_of_the_stored_rows(env, variant):
    """stats_out of the residual GEMMs on the bf16 stream (what the NEXT folded GEMM normalises with) against f64 sums over the
    stored bf16 rows per 64 columns — test_gemm_p160_resid16 compares it only between the two kernels."""
    torch, _lib, lib = env
    M, N, K = 160, 256, 256
    g = torch.Generator(device="cuda").manual_seed(160 + variant)
    A = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g)
    x0 = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
    out = _with_sentinel(torch, x0)
    st = _sentinel_buf(torch, (M, N // 64, 2), torch.float32)
    _lib.check(lib.mmiss_dbg_gemm_resid16(0, None, variant, _p(A), _p(W), _p(out), _p(bias), _p(st), M, N, K, M, 0, None))
    torch.cuda.synchronize()
    assert _untouched(out, M) and _untouched(st, M)
    ref = x0.float() + (A.float() @ W.float().T + bias)
    assert torch.allclose(out[:M].float(), ref, rtol=2 ** -7, atol=4e-3)      # (the rows themselves: as test_gemm_p160_resid16)
    _assert_sums(torch, st[:M, :, 0], st[:M, :, 1], out[:M].float().view(M, N // 64, 64), 64, f"resid16 variant {variant}")

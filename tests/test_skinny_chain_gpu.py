"""The one-request folded chain (M <= 128 rows: plan_layers sets P.sfold) at kernel level, against float64 on the host:
skinny_row_stats16_kernel, the folded epilogues 7 / 8 of gemm_skinny_kernel with its row_mean_rstd, and the statistics / bf16-copy
part of its residual epilogue, through mmiss_dbg_row_stats16 / _gemm_skinny_fold / _gemm_skinny_resid (include/mmiss_debug.h) —
each with the m-tiles per workgroup (option gemm_skinny_mt) forced to every instance, so that the LATE path (m-tile t != wave: MT = 8
and 16 at four waves, MT = 16 at K = 2048; the old residual and the row statistics loaded in the epilogue) runs deliberately.

Operands come from tests/skinny_chain_cases.py (numpy, Philox), the same the CPU test test_skinny_chain_cpu.py sees; rows follow
its `rowwise` profile (row m = 0.5 m + (1 + m mod 5) N(0,1)) wherever a row, tile or slice mix-up must not hide. Every output
buffer has one sentinel row behind its M rows that must stay untouched; every option a test sets is restored in `finally`.

Waves per workgroup (launch_gemm_skinny_inst): NW = 8 when K >= 2048 and MT <= 8, else 4. The k order of an output element and the
fixed-order sum of the NW K-slices do not depend on MT, and the prefetched and the late row_mean_rstd sum in the same order: outputs
of instances with the same NW are compared BIT FOR BIT. MT = 16 at K = 2048 cuts K four ways, not eight — other partial sums,
other roundings — so against the other instances it is held to the float64 reference only. gemm_skinny_mt = 0 leaves the choice to the cost
model: at N <= 256 every candidate grid is one round of workgroups and MT = 1 is the cheapest.

Tolerances. bf16 outputs: the project's rtol 2^-7, atol 4e-3. f32 residual rows at K = 128: the project's rtol 1e-5, atol 2e-4
(test_gemm_skinny_all_epilogues). At K = 2048 no project number exists; as in test_layernorm_chain_gpu.py, an f32 sum of n terms in
ANY order is within n u sum|terms| of the exact sum (u = 2^-24; the bf16 x bf16 products are exact in f32): an output is the sum of
K products, the bias and the old value, so |out - ref| <= (K + 2) u (|x0| + |bias| + sum_k |a w|) per element. Statistics: n = 16
terms per slice, n u sum|x| and n u sum x^2 (_assert_sums). The residual epilogue sums the terms s = (old + acc) + bias while it
stores x = old + (acc + bias). With e = old + acc + bias exact and t = |old| + |acc| + |bias| (>= |e|), to first order in u:
|x - e| <= u (|acc| + |bias|) + u t and |s - e| <= u (|old| + |acc|) + u t, so |s - x| <= 4 u t and |s^2 - x^2| <= 8 u |x| t.
Against the f64 sums over the STORED rows the statistics of that epilogue are therefore held to
    n u sum|x| + 4 u sum t    and    n u sum x^2 + 8 u sum |x| t
(t from the float64 product: its f32 rounding is second order). Under strong cancellation inside a slice (t >> |x|) the second
term is the larger one; the measured ratios are printed."""
import collections
import contextlib

import numpy as np
import pytest

import skinny_chain_cases as sc

pytestmark = pytest.mark.gpu

U = sc.U
EPS = sc.EPS
SENT = -7.0
UNSUPPORTED = -5   # MMISS_ERR_UNSUPPORTED (include/mmiss.h)
EPI_LNFOLD, EPI_LNFOLD_QGELU = 7, 8
MS = [1, 16, 17, 50, 77, 128]          # one partly filled tile, one full, 2 / 4 / 5 (13 valid rows in the last) / 8 m-tiles
MTS = [0, 1, 2, 4, 8, 16]
LAUNCHED = collections.Counter()       # (entry, epilogue, forced MT, NW by the launcher's rule): printed when the module is done


def _nw(K, mt):
    return 8 if (K >= 2048 and K % 256 == 0 and (mt or 1) <= 8) else 4


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    yield torch, _lib, lib
    for key in sorted(LAUNCHED, key=str):
        print("launched", key, LAUNCHED[key])


@contextlib.contextmanager
def _option(_lib, key, value, restore):
    _lib.set_option(key, value)
    try:
        yield
    finally:
        _lib.set_option(key, restore)


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(torch, a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(torch.bfloat16) if bf16 else t      # (exact: the values of a bf16 operand are on the bf16 grid already)


def _host(t):
    """device f32 / bf16 tensor -> numpy f32"""
    return t.detach().float().cpu().numpy()


def _sentinel_buf(torch, shape, dtype):
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), SENT, device="cuda", dtype=dtype)


def _with_sentinel(torch, t):
    return torch.cat([t, torch.full((1,) + tuple(t.shape[1:]), SENT, device=t.device, dtype=t.dtype)]).contiguous()


def _untouched(t, M):
    return bool((t[M:] == SENT).all())


def _bits(t):
    import torch

    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_sums(got, y, n, what, t=None):
    """got f32 [M][parts][2] against the f64 (sum, sumsq) over the last axis of y [M][parts][n]: bound n u sum|y|, n u sum y^2;
    t (the residual epilogue, see the docstring above): + 4 u sum t and + 8 u sum |y| t. -> the two max error / bound ratios"""
    y = y.astype(np.float64)
    s, a, q = y.sum(-1), np.abs(y).sum(-1), (y * y).sum(-1)
    bs, bq = n * U * a, n * U * q
    if t is not None:
        t = t.reshape(y.shape)
        bs, bq = bs + 4 * U * t.sum(-1), bq + 8 * U * (np.abs(y) * t).sum(-1)
    es, eq = np.abs(got[..., 0].astype(np.float64) - s), np.abs(got[..., 1].astype(np.float64) - q)
    rs, rq = float((es / np.maximum(bs, 1e-300)).max()), float((eq / np.maximum(bq, 1e-300)).max())
    print(what, "sum err / bound max", rs, "sumsq err / bound max", rq)
    assert (es <= bs).all(), (what, "sum", float(es.max()))
    assert (eq <= bq).all(), (what, "sumsq", float(eq.max()))
    return rs, rq


# ------------------------------------------------------------------------------------------------ callers
def _row_stats16(env, x, M, d):
    """-> (stats f32 [M][d/16][2], xb bf16 [M, d]) of the device rows x, sentinel rows checked"""
    torch, _lib, lib = env
    st = _sentinel_buf(torch, (M, d // 16, 2), torch.float32)
    xb = _sentinel_buf(torch, (M, d), torch.bfloat16)
    _lib.check(lib.mmiss_dbg_row_stats16(0, None, _p(x), _p(st), _p(xb), M, d))
    torch.cuda.synchronize()
    assert _untouched(st, M) and _untouched(xb, M), (M, d)
    return st[:M], xb[:M]


def _fold_weights(env, W, gam, bet, bias):
    """fold_ln_weights_kernel on the device (tested in test_layernorm_chain_gpu.py): W' bf16, c, b' f32"""
    torch, _lib, lib = env
    N, K = W.shape
    Wd, gd, bd, biasd = _dev(torch, W, True), _dev(torch, gam), _dev(torch, bet), _dev(torch, bias)
    wf = torch.zeros(N, K, device="cuda", dtype=torch.bfloat16)
    c = torch.zeros(N, device="cuda")
    bf = torch.zeros(N, device="cuda")
    _lib.check(lib.mmiss_dbg_fold_ln_weights(0, None, _p(Wd), _p(gd), _p(bd), _p(biasd), _p(wf), _p(c), _p(bf), N, K))
    torch.cuda.synchronize()
    return wf, c, bf


def _fold_gemm(env, epi, xb, wf, c, bf, st, M, N, K, mt):
    torch, _lib, lib = env
    out = _sentinel_buf(torch, (M, N), torch.bfloat16)
    with _option(_lib, "gemm_skinny_mt", mt, 0):
        _lib.check(lib.mmiss_dbg_gemm_skinny_fold(0, None, epi, _p(xb), _p(wf), _p(out), _p(bf), _p(c), _p(st), EPS, M, N, K))
        torch.cuda.synchronize()
    LAUNCHED[("gemm_skinny_fold", epi, mt, _nw(K, mt))] += 1
    assert _untouched(out, M), (M, N, K, mt)
    return out[:M]


def _resid_gemm(env, A, W, x0, bias, M, N, K, mt, stats=True, xb=True):
    """-> (new rows f32 [M, N], stats or None, xb or None), sentinel rows checked"""
    torch, _lib, lib = env
    x = _with_sentinel(torch, x0)
    st = _sentinel_buf(torch, (M, N // 16, 2), torch.float32) if stats else None
    xo = _sentinel_buf(torch, (M, N), torch.bfloat16) if xb else None
    with _option(_lib, "gemm_skinny_mt", mt, 0):
        _lib.check(lib.mmiss_dbg_gemm_skinny_resid(0, None, _p(A), _p(W), _p(x), _p(bias), _p(st), _p(xo), M, N, K))
        torch.cuda.synchronize()
    LAUNCHED[("gemm_skinny_resid", 3, mt, _nw(K, mt))] += 1
    assert _untouched(x, M) and (st is None or _untouched(st, M)) and (xo is None or _untouched(xo, M)), (M, N, K, mt)
    return x[:M], None if st is None else st[:M], None if xo is None else xo[:M]


def _plain_gemm(env, epi, A, W, out, bias, aux, M, N, K, mt, p0=0, p1=0):
    torch, _lib, lib = env
    with _option(_lib, "gemm_skinny_mt", mt, 0):
        _lib.check(lib.mmiss_dbg_gemm(0, None, epi, 0, _p(A), _p(W), _p(out), _p(bias), _p(aux), M, N, K, p0, p1))
        torch.cuda.synchronize()
    LAUNCHED[("gemm", epi, mt, _nw(K, mt))] += 1


# ------------------------------------------------------------------------------------------------ skinny_row_stats16_kernel
@pytest.mark.parametrize("kind", ["plain", "offset"])
@pytest.mark.parametrize("d", [64, 128, 320, 768, 1024])
def test_row_stats16(env, d, kind):
    """xb = bf16(x) bit for bit; (sum, sumsq) per 16 columns within n u of the f64 sums; and on rows prelayernorm_skinny has
    normalised, the very statistics and bf16 rows that kernel left (encoder_kernels.h promises the same bits). M = 1, 3, 4, 5:
    a workgroup of four waves partly filled, full, and one row into the next; d = 320: a second, partly filled pass of the
    wave (columns 256 .. 319 on 16 of its lanes); d = 64: 16 lanes of the only pass."""
    torch, _lib, lib = env
    for M in [1, 3, 4, 5, 77]:
        xh = sc.rows(M, d, kind, 11)
        x = _dev(torch, xh)
        st, xb = _row_stats16(env, x, M, d)
        assert np.array_equal(_bits(xb).cpu().numpy().view(np.uint16), sc.bf16_bits(xh)), M
        _assert_sums(st.cpu().numpy(), xh.reshape(M, d // 16, 16), 16, f"row_stats16 d={d} {kind} M={M}")
        # the producer of the vision tower: CLS row, LayerNorm in place, bf16 copy and statistics in one launch
        g = sc.rng_of(12, d)
        cls, pos, gam, bet = (_dev(torch, g.standard_normal(d).astype(np.float32)) for _ in range(4))
        y = x.clone()
        xb_pre = torch.zeros(M, d, device="cuda", dtype=torch.bfloat16)
        st_pre = torch.zeros(M, d // 16, 2, device="cuda")
        _lib.check(lib.mmiss_dbg_prelayernorm_skinny(0, None, _p(y), _p(cls), _p(pos), _p(gam), _p(bet), _p(xb_pre), _p(st_pre), M, M, d, EPS))
        torch.cuda.synchronize()
        st2, xb2 = _row_stats16(env, y, M, d)
        assert torch.equal(_bits(st2), _bits(st_pre)) and torch.equal(_bits(xb2), _bits(xb_pre)), M


# ------------------------------------------------------------------------------------------------ folded epilogues 7 / 8
@pytest.mark.parametrize("epi", [EPI_LNFOLD, EPI_LNFOLD_QGELU])
@pytest.mark.parametrize("K", [128, 768, 1024])
def test_folded_epilogues_every_instance(env, K, epi):
    """rstd (acc - mean c) + b' (8: then QuickGELU) against the float64 exact folded form of the same xb, W', c, b' and the same
    f32 statistics buffer, under rtol 2^-7, atol 4e-3, for every MT instance; all instances bit-identical (K < 2048: four waves
    each). K = 128: 4 quads of partials, K = 768: exactly one trip of 24 quads, K = 1024: a second trip of 8 with 16 masked.
    Rows: the rowwise profile — the late tiles of MT = 8 / 16 (m-tiles 4.. of a workgroup) get their own (mean, rstd) or miss by
    a mean that is 8 or more away."""
    torch, _lib, lib = env
    N = 128
    W, gam, bet, bias = sc.weights(N, K, 21)
    wf, c, bf = _fold_weights(env, W, gam, bet, bias)
    wf_h, c_h, bf_h = _host(wf), _host(c), _host(bf)
    worst = 0.0
    for M in MS:
        x = _dev(torch, sc.rows(M, K, "rowwise", 22))
        st, xb = _row_stats16(env, x, M, K)
        exact = sc.exact_folded(_host(xb), wf_h, c_h, bf_h, _host(st), epi == EPI_LNFOLD_QGELU)
        first = None
        for mt in MTS:
            out = _fold_gemm(env, epi, xb, wf, c, bf, st, M, N, K, mt)
            r = float((np.abs(_host(out).astype(np.float64) - exact) / sc.tol(exact)).max())
            worst = max(worst, r)
            assert r <= 1.0, (M, mt, r)
            if first is None:
                first = out
            assert torch.equal(_bits(out), _bits(first)), (M, mt)
    print(f"fold epi={epi} K={K}: max |kernel - exact folded form| / tol over M, MT = {worst:.4f}")


# ------------------------------------------------------------------------------------------------ residual epilogue + statistics
@pytest.mark.parametrize("K", [128, 2048])
@pytest.mark.parametrize("N", [128, 256])
def test_residual_epilogue_with_statistics_every_instance(env, N, K):
    """x += A W^T + bias with stats_out [M][N/16][2] and xb_out: the rows against float64, bit-identical to mmiss_dbg_gemm's
    (statistics must not change the stream) and across instances of the same NW; xb_out = bf16(stored rows) bit for bit;
    stats_out = the sums over the stored rows' 16-column slices within n u plus the epilogue's own term (module docstring); either of the two outputs may be null. K = 2048: eight
    waves for MT <= 8 (MT = 8: one m-tile per wave, none late), four for MT = 16 (twelve late tiles). x0 and A: rowwise rows."""
    torch, _lib, lib = env
    W, _, _, bias = sc.weights(N, K, 31)
    Wd, biasd = _dev(torch, W, True), _dev(torch, bias)
    worst = 0.0
    for M in MS:
        Ah = sc.bf16_round(sc.rows(M, K, "rowwise", 32))
        x0h = sc.rows(M, N, "rowwise", 33)
        A, x0 = _dev(torch, Ah, True), _dev(torch, x0h)
        ref, mag = sc.resid_rows64(x0h, Ah, W, bias)
        t = sc.resid_terms64(x0h, Ah, W, bias)
        first = {}
        for mt in MTS:
            x, st, xb = _resid_gemm(env, A, Wd, x0, biasd, M, N, K, mt)
            xh = x.cpu().numpy()
            err = np.abs(xh.astype(np.float64) - ref)
            if K == 128:
                bound = 2e-4 + 1e-5 * np.abs(ref)
            else:
                bound = (K + 2) * U * mag
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (M, mt, float((err / bound).max()))
            plain = _with_sentinel(torch, x0)
            _plain_gemm(env, 3, A, Wd, plain, biasd, None, M, N, K, mt)
            assert _untouched(plain, M) and torch.equal(_bits(plain[:M]), _bits(x)), (M, mt)
            assert torch.equal(_bits(xb), _bits(x.to(torch.bfloat16))), (M, mt)
            _assert_sums(st.cpu().numpy(), xh.reshape(M, N // 16, 16), 16, f"resid N={N} K={K} M={M} MT={mt}", t)
            x1, st1, _ = _resid_gemm(env, A, Wd, x0, biasd, M, N, K, mt, xb=False)
            x2, _, xb2 = _resid_gemm(env, A, Wd, x0, biasd, M, N, K, mt, stats=False)
            assert torch.equal(_bits(x1), _bits(x)) and torch.equal(_bits(x2), _bits(x)), (M, mt)
            assert torch.equal(_bits(st1), _bits(st)) and torch.equal(_bits(xb2), _bits(xb)), (M, mt)
            nw = _nw(K, mt)
            if nw not in first:
                first[nw] = (x, st, xb)
            for a, b in zip(first[nw], (x, st, xb)):     # (across NW: both are within the bound of the float64 rows, no more)
                assert torch.equal(_bits(a), _bits(b)), (M, mt)
    print(f"resid N={N} K={K}: max |rows - float64| / bound over M, MT = {worst:.4f}")


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("profile", sc.PROFILES)
@pytest.mark.parametrize("shape", sc.CHAIN_SHAPES, ids=lambda s: f"d{s[0]}")
def test_chain(env, shape, profile):
    """What the product does on a 77-row request: row_stats16 -> fold_ln_weights -> folded QKV (7) -> residual GEMM on a random bf16
    `ctx` with statistics and bf16 copy -> folded FC1 (8) from THOSE statistics. Every folded output against the exact folded form
    of the device's own operands at both weight scales and on every profile; against the semantic form
    QuickGELU(LayerNorm(new rows) W^T + b) at scale 0.25 on the profiles test_skinny_chain_cpu.py cleared. MT is left to the cost
    model and forced to 8 (the text tower's QKV: m-tile 4 of 5 is a late tile of wave 0); the two runs are bit-identical."""
    torch, _lib, lib = env
    d, Nq, mlp = shape
    M = sc.CHAIN_M
    for w_scale in (sc.SEMANTIC_W_SCALE, 1.0):
        case = sc.ChainCase(d, Nq, mlp, profile, w_scale)
        x0 = _dev(torch, case.x0)
        st1, xb1 = _row_stats16(env, x0, M, d)
        ctx, Wo, bo = _dev(torch, case.ctx, True), _dev(torch, case.Wo, True), _dev(torch, case.bo)
        ref_rows, mag = sc.resid_rows64(case.x0, case.ctx, case.Wo, case.bo)
        t = sc.resid_terms64(case.x0, case.ctx, case.Wo, case.bo)
        wfq, cq, bfq = _fold_weights(env, case.Wq, case.g1, case.b1, case.bq)
        wf1, c1, bf1 = _fold_weights(env, case.W1, case.g2, case.b2, case.bf1)
        outs = {}
        for mt in (0, 8):
            qkv = _fold_gemm(env, EPI_LNFOLD, xb1, wfq, cq, bfq, st1, M, Nq, d, mt)
            x, st2, xb2 = _resid_gemm(env, ctx, Wo, x0, bo, M, d, d, mt)
            fc1 = _fold_gemm(env, EPI_LNFOLD_QGELU, xb2, wf1, c1, bf1, st2, M, mlp, d, mt)
            outs[mt] = (qkv, x, st2, xb2, fc1)
            xh = x.cpu().numpy()
            assert (np.abs(xh.astype(np.float64) - ref_rows) <= (d + 2) * U * mag).all(), mt
            assert torch.equal(_bits(xb2), _bits(x.to(torch.bfloat16))), mt
            _assert_sums(st2.cpu().numpy(), xh.reshape(M, d // 16, 16), 16, f"chain d={d} {profile} scale={w_scale} MT={mt}", t)
            for stage, got, xb, st, (wf, c, bf) in (("qkv", qkv, xb1, st1, (wfq, cq, bfq)), ("fc1", fc1, xb2, st2, (wf1, c1, bf1))):
                _, Wh, gam, bet, bias, gelu = case.stage(stage, xh)
                got = _host(got).astype(np.float64)
                exact = sc.exact_folded(_host(xb), _host(wf), _host(c), _host(bf), _host(st), gelu)
                r = float((np.abs(got - exact) / sc.tol(exact)).max())
                print(f"chain d={d} {profile} scale={w_scale} MT={mt} {stage}: max |kernel - exact folded form| / tol = {r:.4f}")
                assert r <= 1.0, (stage, mt, r)
                if w_scale == sc.SEMANTIC_W_SCALE and profile in sc.SEMANTIC_CLEARED[(d, stage)]:
                    ref = sc.semantic(_host(xb), Wh, gam, bet, bias, gelu)
                    r = float((np.abs(got - ref) / sc.tol(ref)).max())
                    print(f"chain d={d} {profile} MT={mt} {stage}: max |kernel - semantic form| / tol = {r:.4f}")
                    assert r <= 1.0, (stage, mt, r)
        for a, b in zip(outs[0], outs[8]):
            assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ launch counters
def test_launch_counters_name_the_skinny_classes(env):
    """The project's own launch counters (mmiss_prof_read) over one pass of the three entries at every forced MT: the skinny
    classes, each the expected number of times, and no tiled or persistent GEMM class. The counters name the kernel class only;
    WHICH instance ran follows from the forced gemm_skinny_mt (launch_gemm_skinny_mt's switch) and from K (NW = 8 when K >= 2048 and
    MT <= 8, launch_gemm_skinny_inst) — and a wrong instance choice would not change the bits the other tests compare."""
    torch, _lib, lib = env
    M, N, K = 77, 128, 128
    W, gam, bet, bias = sc.weights(N, K, 51)
    wf, c, bf = _fold_weights(env, W, gam, bet, bias)
    x0 = _dev(torch, sc.rows(M, K, "rowwise", 52))
    Wd, biasd = _dev(torch, W, True), _dev(torch, bias)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        st, xb = _row_stats16(env, x0, M, K)
        for mt in MTS:
            _fold_gemm(env, EPI_LNFOLD, xb, wf, c, bf, st, M, N, K, mt)
            _fold_gemm(env, EPI_LNFOLD_QGELU, xb, wf, c, bf, st, M, N, K, mt)
            _resid_gemm(env, xb, Wd, x0, biasd, M, N, K, mt)
        counts = {r["kernel"]: r["launches"] for r in _lib.prof_read()}
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    print("prof_read", counts)
    assert counts == {"row_stats": 1, "gemm_skinny_lnfold_bias": len(MTS), "gemm_skinny_lnfold_qgelu": len(MTS),
                      "gemm_skinny_bias_resid": len(MTS)}, counts


# ------------------------------------------------------------------------------------------------ refusals
def test_entries_refuse_what_the_skinny_path_does_not_take(env):
    """Non-zero status and untouched outputs for: 129 rows at N = 2048 (the dispatch stops at 128 rows above N = 1024), K = 192
    (no multiple of 128), N no multiple of 16, null statistics, a wrong epilogue, d no multiple of 16, M = 0 — and, with the
    skinny kernel switched off, shapes the TILED kernels would take (M = N = K = 128): no entry falls back to them. Every buffer
    is as large as the refused launch would need."""
    torch, _lib, lib = env

    def bufs(M, N, K):
        A = torch.zeros(M, K, device="cuda", dtype=torch.bfloat16)
        W = torch.zeros(max(N, 16), K, device="cuda", dtype=torch.bfloat16)
        v = torch.zeros(max(N, 16) + 16, device="cuda")
        st_in = torch.zeros(M, max(K // 16, 2), 2, device="cuda")
        out16 = _sentinel_buf(torch, (M, N + 16), torch.bfloat16)
        x = _sentinel_buf(torch, (M, N + 16), torch.float32)
        st = _sentinel_buf(torch, (M, N // 16 + 1, 2), torch.float32)
        return A, W, v, st_in, out16, x, st

    def fold(epi, M, N, K, stats=True):
        A, W, v, st_in, out16, _, _ = bufs(max(M, 1), N, K)
        rc = lib.mmiss_dbg_gemm_skinny_fold(0, None, epi, _p(A), _p(W), _p(out16), _p(v), _p(v), _p(st_in) if stats else None, EPS, M, N, K)
        torch.cuda.synchronize()
        return rc, bool((out16 == SENT).all())

    def resid(M, N, K):
        A, W, v, _, out16, x, st = bufs(max(M, 1), N, K)
        rc = lib.mmiss_dbg_gemm_skinny_resid(0, None, _p(A), _p(W), _p(x), _p(v), _p(st), _p(out16), M, N, K)
        torch.cuda.synchronize()
        return rc, bool((out16 == SENT).all() and (x == SENT).all() and (st == SENT).all())

    for M, N, K in ((129, 2048, 128), (16, 128, 192), (16, 120, 128), (0, 128, 128)):
        for epi in (EPI_LNFOLD, EPI_LNFOLD_QGELU):
            rc, clean = fold(epi, M, N, K)
            assert rc == UNSUPPORTED and clean, ("fold", epi, M, N, K, rc)
        rc, clean = resid(M, N, K)
        assert rc == UNSUPPORTED and clean, ("resid", M, N, K, rc)
    rc, clean = fold(EPI_LNFOLD, 16, 128, 128, stats=False)
    assert rc != 0 and clean, ("fold without statistics", rc)
    A, W, v, st_in, out16, _, _ = bufs(16, 128, 128)        # statistics, c or b' off the 16-byte grid the kernel loads them on
    for off_st, off_c, off_b in ((4, 0, 0), (0, 4, 0), (0, 0, 8)):
        rc = lib.mmiss_dbg_gemm_skinny_fold(0, None, EPI_LNFOLD, _p(A), _p(W), _p(out16), _p(v) + off_b, _p(v) + off_c, _p(st_in) + off_st, EPS,
                                            16, 128, 128)
        torch.cuda.synchronize()
        assert rc != 0 and bool((out16 == SENT).all()), ("fold with misaligned operands", off_st, off_c, off_b, rc)
    for epi in (0, 1, 2, 3, 4, 9):
        rc, clean = fold(epi, 16, 128, 128)
        assert rc == UNSUPPORTED and clean, ("fold", epi, rc)
    with _option(_lib, "gemm_skinny", 0, 1):
        for epi in (EPI_LNFOLD, EPI_LNFOLD_QGELU):
            rc, clean = fold(epi, 128, 128, 128)
            assert rc == UNSUPPORTED and clean, ("fold with the skinny kernel off", epi, rc)
        rc, clean = resid(128, 128, 128)
        assert rc == UNSUPPORTED and clean, ("resid with the skinny kernel off", rc)
    # row_stats16
    x = torch.zeros(4, 64, device="cuda")
    st = _sentinel_buf(torch, (4, 4, 2), torch.float32)
    xb = _sentinel_buf(torch, (4, 64), torch.bfloat16)
    for M, d in ((4, 24), (4, 8), (0, 64), (-1, 64), (4, 0)):
        assert lib.mmiss_dbg_row_stats16(0, None, _p(x), _p(st), _p(xb), M, d) == UNSUPPORTED, (M, d)
    for args in ((None, _p(st), _p(xb)), (_p(x), None, _p(xb)), (_p(x), _p(st), None)):
        assert lib.mmiss_dbg_row_stats16(0, None, *args, 4, 64) != 0
    torch.cuda.synchronize()
    assert bool((st == SENT).all() and (xb == SENT).all())


# ------------------------------------------------------------------------------------------------ plain epilogues, MT = 4 / 8 / 16
@pytest.mark.parametrize("K", [128, 2048])
def test_plain_epilogues_at_forced_instances(env, K):
    """The five plain epilogues of test_gemm_skinny_all_epilogues / test_gemm_skinny_patch_epilogue_and_determinism at M = 77 (five
    m-tiles, 13 valid rows in the last), N = 128 with MT forced to 4, 8 and 16 — instances the cost model never picks at those
    tests' shapes — under the same tolerances, against float64."""
    torch, _lib, lib = env
    M, N = 77, 128
    G, imgs, T = 7, 11, 8            # patch epilogue: row m = img * 7 + patch lands at img * 8 + 1 + patch
    g = sc.rng_of(41, K)
    Ah = sc.bf16_round(g.standard_normal((M, K)).astype(np.float32))
    W, _, _, bias = sc.weights(N, K, 42)
    x0h = g.standard_normal((M, N)).astype(np.float32)
    posh = g.standard_normal((T, N)).astype(np.float32)
    A, Wd, biasd, pos = _dev(torch, Ah, True), _dev(torch, W, True), _dev(torch, bias), _dev(torch, posh)
    acc = Ah.astype(np.float64) @ W.astype(np.float64).T
    yb = acc + bias
    for mt in (4, 8, 16):
        out = _sentinel_buf(torch, (M, N), torch.float32)
        _plain_gemm(env, 0, A, Wd, out, None, None, M, N, K, mt)
        assert _untouched(out, M) and np.abs(_host(out[:M]) - acc).max() <= 2e-4 * max(1.0, np.abs(acc).max()), mt
        ob = _sentinel_buf(torch, (M, N), torch.bfloat16)
        _plain_gemm(env, 1, A, Wd, ob, biasd, None, M, N, K, mt)
        assert _untouched(ob, M) and np.allclose(_host(ob[:M]), yb, rtol=2 ** -8, atol=1e-3), mt
        og = _sentinel_buf(torch, (M, N), torch.bfloat16)
        _plain_gemm(env, 2, A, Wd, og, biasd, None, M, N, K, mt)
        assert _untouched(og, M) and np.allclose(_host(og[:M]), sc.quick_gelu64(yb), rtol=2 ** -7, atol=2e-3), mt
        x = _with_sentinel(torch, _dev(torch, x0h))
        _plain_gemm(env, 3, A, Wd, x, biasd, None, M, N, K, mt)
        assert _untouched(x, M) and np.allclose(_host(x[:M]), x0h + yb, rtol=1e-5, atol=2e-4), mt
        op = torch.zeros(imgs * T + 1, N, device="cuda")
        op[imgs * T] = SENT
        _plain_gemm(env, 4, A, Wd, op, None, pos, M, N, K, mt, p0=G, p1=T)
        got = _host(op[:imgs * T]).reshape(imgs, T, N)
        assert _untouched(op, imgs * T) and (got[:, 0] == 0).all(), mt
        assert np.allclose(got[:, 1:], acc.reshape(imgs, G, N) + posh[1:][None], rtol=1e-5, atol=3e-4), mt

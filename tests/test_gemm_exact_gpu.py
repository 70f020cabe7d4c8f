"""Every instance of the tiled bf16 GEMM family on the MI355X against exact arithmetic (gemm_exact_cases.py): operands whose
products and partial sums are exact in fp32 in any order, so that the accumulator of every kernel must equal the float64 product
bit for bit, f32 outputs and statistics have one correct value, and bf16 outputs one correct bit pattern (QuickGELU and the folded
epilogues: wherever the float64 value lies farther than its derived margin from a rounding boundary). test_gemm_exact_cpu.py
asserts on the host that every case here meets the conditions for that, and that the comparison rejects the wrong results it is
there to catch.

Calls go through the C ABI (include/mmiss_debug.h). Pure-write outputs start as NaN, in-place ones as the old rows; every output,
statistics and bf16-copy buffer carries SENT sentinel rows behind it (no entry takes an output row stride, so there are no
sentinel columns), and rows from m_valid on must keep what they held. Options are restored in `finally`. The largest
|got - ref| / margin a run proves for the inexact epilogues is printed (run with -s), not asserted: DESIGN.md records it."""
import contextlib

import pytest

import gemm_exact_cases as gx

pytestmark = pytest.mark.gpu
SENT = 3
MMISS_ERR_UNSUPPORTED = -5
RATIOS = {}


@pytest.fixture(scope="module")
def env():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch, _lib, lib


@contextlib.contextmanager
def options(_lib, **forced):
    """the tiled kernels in charge (no skinny kernel, no split-K unless asked for), the forced options on top; defaults after"""
    want = dict(gemm_skinny=0, gemm_splitk=0)
    want.update(forced)
    try:
        for k, v in want.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k in want:
            _lib.set_option(k, gx.OPTION_DEFAULTS[k])


@contextlib.contextmanager
def launches(_lib, counts):
    """the launch counters (mmiss_prof_read) of the calls inside, into `counts`"""
    _lib.prof_filter(None, 1)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        yield
        counts.update({r["kernel"]: r["launches"] for r in _lib.prof_read()})
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()


def _dev(torch, c):
    """the device operands of a Case in the types the kernels read (exactness asserted), built once"""
    if getattr(c, "_dev", None) is None:
        d = dict(A=gx.bf16_tensor(c.A), W=gx.bf16_tensor(c.W), bias=gx.f32_tensor(c.bias))
        if c.kind == "fold":
            stats, cv, _, _ = c.fold_operands()
            d["ln"], d["c"] = gx.f32_tensor(stats), gx.f32_tensor(cv)
        else:
            d["x0"] = gx.f32_tensor(c.x0)
        if c.patch is not None:
            d["pos"] = gx.f32_tensor(c.pos)
        c._dev = d
    return c._dev


def _filled(torch, rows, cols, dtype, head=None):
    """[rows + SENT, *cols] of NaN, the first rows = head (the old rows of an in-place epilogue)"""
    shape = (rows + SENT,) + (cols if isinstance(cols, tuple) else (cols,))
    t = torch.full(shape, float("nan"), device="cuda", dtype=dtype)
    if head is not None:
        t[:rows] = head
    return t


def _note(key, ratio):
    if ratio is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def _gemm_ex(env, epi, variant, d, out, M, N, K, mv, aux=None, p0=0, p1=0, stats=None, xb=None, ln=None):
    torch, _lib, lib = env
    p = _lib.ptr
    _lib.check(lib.mmiss_dbg_gemm_ex(0, None, epi, variant, p(d["A"]), p(d["W"]), p(out), p(d["bias"]), p(aux), M, N, K, p0, p1, mv,
                                     p(stats), p(xb), p(ln), gx.LN_EPS))
    torch.cuda.synchronize()


def run_epilogues(env, c, variant, epis, mvs, tile_h, kernel, keep=None):
    """Case c through mmiss_dbg_gemm_ex for every epilogue of `epis` (3 on a case of kind 'stats': with stats_out and xb_out) and
    every m_valid of `mvs`, each output held to the float64 reference, pad and sentinel rows to what they held."""
    torch, _lib, lib = env
    M, N, K = c.M, c.N, c.K
    d = _dev(torch, c)
    for epi in epis:
        for mv in mvs:
            what = "%s epi %d %dx%dx%d m_valid %d" % (kernel, epi, M, N, K, mv)
            if epi == gx.EPI_F32:
                out = _filled(torch, M, N, torch.float32)
                _gemm_ex(env, epi, variant, d, out, M, N, K, mv)
                gx.assert_f32_exact(out[:mv], c.ref_f32()[:mv], tile_h, what)
                gx.assert_untouched(out[mv:], _filled(torch, M, N, torch.float32)[mv:], what)
            elif epi in (gx.EPI_BIAS, gx.EPI_QGELU, gx.EPI_FOLD, gx.EPI_FOLD_QGELU):
                out = _filled(torch, M, N, torch.bfloat16)
                if epi in (gx.EPI_FOLD, gx.EPI_FOLD_QGELU):
                    _gemm_ex(env, epi, variant, d, out, M, N, K, mv, aux=d["c"], ln=d["ln"])
                    v, margin = c.ref_fold(epi == gx.EPI_FOLD_QGELU)
                else:
                    _gemm_ex(env, epi, variant, d, out, M, N, K, mv)
                    v, margin = (c.ref_bias(), None) if epi == gx.EPI_BIAS else c.ref_qgelu()
                _note((kernel, epi), gx.assert_bf16_rounded(out[:mv], v[:mv], None if margin is None else margin[:mv], tile_h, what))
                gx.assert_untouched(out[mv:], _filled(torch, M, N, torch.bfloat16)[mv:], what)
            elif epi == gx.EPI_RESID:
                before = _filled(torch, M, N, torch.float32, d["x0"])
                out = before.clone()
                if c.kind == "stats":
                    stats = _filled(torch, M, (N // 64, 2), torch.float32)
                    xb = _filled(torch, M, N, torch.bfloat16)
                    _gemm_ex(env, epi, variant, d, out, M, N, K, mv, stats=stats, xb=xb)
                    v = c.ref_resid()
                    gx.assert_f32_exact(stats[:mv].view(mv, -1), c.stats64(v)[:mv].view(mv, -1), tile_h, what + " stats_out")
                    gx.assert_untouched(stats[mv:], _filled(torch, M, (N // 64, 2), torch.float32)[mv:], what + " stats_out")
                    gx.assert_bf16_rounded(xb[:mv], v[:mv], None, tile_h, what + " xb_out")
                    gx.assert_untouched(xb[mv:], _filled(torch, M, N, torch.bfloat16)[mv:], what + " xb_out")
                else:
                    _gemm_ex(env, epi, variant, d, out, M, N, K, mv)
                gx.assert_f32_exact(out[:mv], c.ref_resid()[:mv], tile_h, what)
                gx.assert_untouched(out[mv:], before[mv:], what)
            else:
                G, T = c.patch
                rows_out = (M + G - 1) // G * T
                out = _filled(torch, rows_out, N, torch.float32)
                _gemm_ex(env, epi, variant, d, out, M, N, K, mv, aux=d["pos"], p0=G, p1=T)
                idx, v = c.ref_patch_rows()
                gx.assert_f32_exact(out[idx[:mv]], v[:mv], tile_h, what)
                if keep is not None:
                    keep[(epi, mv)] = out.clone()
                out[idx[:mv]] = float("nan")      # everything else — CLS rows, pad rows, the rows behind the last image — untouched
                gx.assert_untouched(out, _filled(torch, rows_out, N, torch.float32), what)
            if keep is not None and epi != gx.EPI_PATCH:
                keep[(epi, mv)] = out.clone()


PLAIN = (gx.EPI_F32, gx.EPI_BIAS, gx.EPI_QGELU, gx.EPI_RESID, gx.EPI_PATCH)
FOLDED = (gx.EPI_FOLD, gx.EPI_FOLD_QGELU)


# ------------------------------------------------------------------------------------------------ gemm16_kernel
@pytest.mark.parametrize("form,bm", [(f, bm) for f, (_, heights, _) in gx.FORMS.items() for bm in heights],
                         ids=lambda v: str(v).replace(" ", ""))
def test_gemm16_every_form_every_epilogue(env, form, bm):
    """The four forms of gemm16_kernel (two / three staging buffers x 4 / 8 waves) at every tile height that has them, forced at a
    2 x 2 grid of tiles and confirmed by the launcher's own choice (mmiss_dbg_gemm_form) before anything is compared: K-tile
    counts 1, 2, 3, 4, 12 (three buffers: from 4 on), the five plain epilogues, the residual one again with stats_out and xb_out,
    each with m_valid = M and with m_valid inside the last tile."""
    torch, _lib, lib = env
    forced, _, ktiles = gx.FORMS[form]
    M, N = 2 * bm, gx.TILE_N
    with options(_lib, **forced):
        for kt in ktiles:
            K = 64 * kt
            assert _lib.gemm_form(bm, M, N, K) == form, (_lib.gemm_form(bm, M, N, K), form, K)
            kernel = "gemm16 bm %d %d buffers %d waves" % ((bm,) + form)
            mvs = (M, gx.ragged(M, bm))
            run_epilogues(env, gx.case(M, N, K, "wide", (gx.PATCH_G, gx.PATCH_T), "cuda"), bm, PLAIN, mvs, bm, kernel)
            run_epilogues(env, gx.case(M, N, K, "stats", None, "cuda"), bm, (gx.EPI_RESID,), mvs, bm, kernel)
    print("margin ratios", {k: round(v, 3) for k, v in RATIOS.items() if k[0].startswith("gemm16 bm %d %d buffers %d" % ((bm,) + form))})


@pytest.mark.parametrize("bm", [128, 160, 192])
def test_gemm16_folded_epilogues(env, bm):
    """launch_gemm_fold in isolation: epilogues 7 / 8 on the 128-column tile of every height (always two buffers, 4 waves), K of 2,
    4, 12 and 16 K-tiles (the rows' partials are read in pairs, 16 at the most), full and ragged m_valid."""
    torch, _lib, lib = env
    M, N = 2 * bm, gx.TILE_N
    with options(_lib):
        for kt in gx.FOLD_KTILES:
            run_epilogues(env, gx.case(M, N, 64 * kt, "fold", None, "cuda"), bm, FOLDED, (M, gx.ragged(M, bm)), bm, "gemm16 fold bm %d" % bm)
    print("margin ratios", {k: round(v, 3) for k, v in RATIOS.items() if k[0] == "gemm16 fold bm %d" % bm})


def test_gemm16_banded_tile_order(env):
    """8 column tiles: the banded tile order (gemm_band = 5 row tiles per band) with 7 row tiles, so that the last band is short;
    every output tile must still be computed exactly once, by the right (bm, bn)."""
    torch, _lib, lib = env
    M, N, K = gx.BAND_SHAPE
    assert N // 128 >= 8 and (M // 128) % 5 != 0
    with options(_lib):
        assert _lib.gemm_form(128, M, N, K) == (2, 8)
        run_epilogues(env, gx.case(M, N, K, "wide", (gx.PATCH_G, gx.PATCH_T), "cuda"), 128, PLAIN, (M, gx.ragged(M, 128)), 128,
                      "gemm16 banded")


def test_folded_launchers_refuse_the_K_their_statistics_loop_does_not_cover(env):
    """ln_row_stats sums a row's partials in pairs, 8 pairs at the most: K = 64 and 192 (odd counts) and K = 2048 (32 partials) used
    to run with silently wrong (mean, rstd); the launchers refuse them now, and nothing is written."""
    torch, _lib, lib = env
    for variant, M in ((128, 256), (256, 512)):
        for K in (64, 192, 2048):
            N = 256
            A = torch.ones(M, K, device="cuda", dtype=torch.bfloat16)
            W = torch.ones(N, K, device="cuda", dtype=torch.bfloat16)
            d = dict(A=A, W=W, bias=torch.ones(N, device="cuda"))
            out = _filled(torch, M, N, torch.bfloat16)
            with pytest.raises(_lib.MmissError) as e:
                _gemm_ex(env, gx.EPI_FOLD, variant, d, out, M, N, K, M, aux=torch.ones(N, device="cuda"),
                         ln=torch.ones(M, K // 64, 2, device="cuda"))
            assert e.value.code == MMISS_ERR_UNSUPPORTED, (variant, K, e.value)
            torch.cuda.synchronize()
            gx.assert_untouched(out, _filled(torch, M, N, torch.bfloat16))


# ------------------------------------------------------------------------------------------------ gemm256_kernel
def test_gemm256_every_epilogue(env):
    """launch_gemm256 (the 256 x 256 phase-pipelined tile) at 2 x 2 tiles: K-tile counts 1, 2, 3, 12 cover prologue, tail and
    steady state; epilogues 0 .. 3, the residual one with stats_out / xb_out, and the folded 7 / 8 (K of 2 and 12 K-tiles)."""
    torch, _lib, lib = env
    M, N = gx.G256_SHAPE
    mvs = (M, gx.ragged(M, 256))
    with options(_lib):
        for kt in gx.G256_KTILES:
            run_epilogues(env, gx.case(M, N, 64 * kt, "wide", None, "cuda"), 256, PLAIN[:4], mvs, 256, "gemm256")
            run_epilogues(env, gx.case(M, N, 64 * kt, "stats", None, "cuda"), 256, (gx.EPI_RESID,), mvs, 256, "gemm256")
        for kt in gx.G256_FOLD_KTILES:
            run_epilogues(env, gx.case(M, N, 64 * kt, "fold", None, "cuda"), 256, FOLDED, mvs, 256, "gemm256")
    print("margin ratios", {k: round(v, 3) for k, v in RATIOS.items() if k[0] == "gemm256"})


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("bm", [128, 160, 192])
def test_split_k_is_exact_and_equals_the_unsplit_bits(env, bm):
    """The smallest shape gemm_splitk_splits accepts (2 x 2 tiles, K = 1536: 4 slices of 6 K-tiles): the slices sum exactly, so
    every epilogue of splitk_reduce_kernel equals the float64 reference, and the unsplit kernel's output, bit for bit. The launch
    counters name the split classes: the split path really ran."""
    torch, _lib, lib = env
    M, N, K = 2 * bm, gx.TILE_N, gx.SPLITK_K
    c = gx.case(M, N, K, "wide", (gx.PATCH_G, gx.PATCH_T), "cuda")
    mvs = (M, gx.ragged(M, bm))
    split, whole, counts = {}, {}, {}
    with options(_lib, gemm_splitk=1):
        assert _lib.gemm_form(bm, M, N, K, 4) == (3, 8 if bm == 128 else 4)
        with launches(_lib, counts):
            run_epilogues(env, c, bm, PLAIN, mvs, bm, "split-K bm %d" % bm, keep=split)
    assert counts == {"gemm_splitk_" + n: 2 for n in ("f32", "bias", "bias_qgelu", "bias_resid", "patch")}, counts
    with options(_lib):
        run_epilogues(env, c, bm, PLAIN, mvs, bm, "unsplit bm %d" % bm, keep=whole)
    for key in split:
        gx.assert_untouched(split[key], whole[key], "split-K against the unsplit kernel, (epi, m_valid) = %s" % (key,))
    print("margin ratios", {k: round(v, 3) for k, v in RATIOS.items() if k[0] == "split-K bm %d" % bm})


# ------------------------------------------------------------------------------------------------ skinny kernel, plain epilogues
@pytest.mark.parametrize("M", gx.SKINNY_MS)
def test_skinny_plain_epilogues(env, M):
    """gemm_skinny_kernel through launch_gemm's own dispatch (default options; the counters name the skinny classes): M = 1, 17,
    77, 128 rows (clamped loads, a ragged last 16-row tile), N = 65 x 16 columns, K = 768 (4 K-quarters of 6 steps) and 2048
    (8 slices): the slices are summed through LDS, exactly."""
    torch, _lib, lib = env
    counts = {}
    with launches(_lib, counts):
        for K in gx.SKINNY_KS:
            run_epilogues(env, gx.case(M, gx.SKINNY_N, K, "wide", (gx.PATCH_G, gx.PATCH_T), "cuda"), 0, PLAIN, (M,), 16, "skinny")
    n = len(gx.SKINNY_KS)
    assert counts == {"gemm_skinny_" + k: n for k in ("f32", "bias", "bias_qgelu", "bias_resid", "patch")}, counts
    print("margin ratios", {k: round(v, 3) for k, v in RATIOS.items() if k[0] == "skinny"})


# ------------------------------------------------------------------------------------------------ persistent 256 x 256
@pytest.mark.parametrize("M,N,K,mv", gx.P256_SHAPES)
def test_p256_persistent(env, M, N, K, mv):
    """gemm256p_kernel: 4 tiles (fewer tiles than workgroups), 6 tiles at K = 768, and 266 tiles (1-2 tiles per workgroup as one K
    stream); epilogues 1 / 2 and the folded 7 / 8 (raw statistics beside the staging buffers: K = 512 and 768); full and ragged
    m_valid. Rows from m_valid on land in the dump row M - 1: the rows between stay NaN, row M - 1 is not specified."""
    torch, _lib, lib = env
    p = _lib.ptr
    for kind, epis in (("wide", (gx.EPI_BIAS, gx.EPI_QGELU)), ("fold", FOLDED)):
        c = gx.case(M, N, K, kind, None, "cuda")
        d = _dev(torch, c)
        for epi in epis:
            what = "p256 epi %d %dx%dx%d m_valid %d" % (epi, M, N, K, mv)
            out = _filled(torch, M, N, torch.bfloat16)
            _lib.check(lib.mmiss_dbg_gemm_p256(0, None, epi, p(d["A"]), p(d["W"]), p(out), p(d["bias"]), p(d.get("c")), p(d.get("ln")),
                                               gx.LN_EPS, M, N, K, mv, 0, None))
            torch.cuda.synchronize()
            if epi == gx.EPI_BIAS:
                v, margin = c.ref_bias(), None
            else:
                v, margin = c.ref_qgelu() if epi == gx.EPI_QGELU else c.ref_fold(epi == gx.EPI_FOLD_QGELU)
            _note(("p256", epi), gx.assert_bf16_rounded(out[:mv], v[:mv], None if margin is None else margin[:mv], 256, what))
            clean = _filled(torch, M, N, torch.bfloat16)
            if mv < M:
                gx.assert_untouched(out[mv:M - 1], clean[mv:M - 1], what)
            gx.assert_untouched(out[M:], clean[M:], what + " sentinel rows")
            del out, clean
    print("margin ratios", {k: round(v, 3) for k, v in RATIOS.items() if k[0] == "p256"})


# ------------------------------------------------------------------------------------------------ bf16 residual stream
def _resid16(env, variant, c, mv, tile_h, dump_row):
    torch, _lib, lib = env
    p = _lib.ptr
    M, N, K = c.M, c.N, c.K
    d = _dev(torch, c)
    what = "resid16 variant %d %dx%dx%d m_valid %d" % (variant, M, N, K, mv)
    before = _filled(torch, M, N, torch.bfloat16, gx.bf16_tensor(c.x0))
    out = before.clone()
    stats = _filled(torch, M, (N // 64, 2), torch.float32)
    _lib.check(lib.mmiss_dbg_gemm_resid16(0, None, variant, p(d["A"]), p(d["W"]), p(out), p(d["bias"]), p(stats), M, N, K, mv, 0, None))
    torch.cuda.synchronize()
    v = c.ref_resid()
    gx.assert_bf16_rounded(out[:mv], v[:mv], None, tile_h, what)
    stored = gx.bf16_round(v).value                  # the statistics are those of the STORED rows
    gx.assert_f32_exact(stats[:mv].view(mv, -1), c.stats64(stored)[:mv].view(mv, -1), tile_h, what + " stats_out")
    gx.assert_untouched(stats[mv:], _filled(torch, M, (N // 64, 2), torch.float32)[mv:], what + " stats_out")
    end = M - 1 if (dump_row and mv < M) else M
    gx.assert_untouched(out[mv:end], before[mv:end], what)
    gx.assert_untouched(out[M:], before[M:], what + " sentinel rows")


@pytest.mark.parametrize("M,N,K,mv", gx.P160_SHAPES)
def test_p160_residual_stream(env, M, N, K, mv):
    """gemm160p_kernel (160 x 256 tile, staggered loop): the K = 768 specialisation and the generic K loop, full and ragged m_valid
    (rows from m_valid on land in the dump row M - 1). Exact bf16 rows, exact statistics of the stored rows."""
    _resid16(env, 0, gx.case(M, N, K, "stats", None, "cuda"), mv, 160, True)


@pytest.mark.parametrize("bm", [128, 160, 192])
def test_resid16_tile_kernels(env, bm):
    """the bf16-stream epilogue of gemm16_kernel (launch_gemm_resid16) at every tile height: K-tile counts 1, 2, 3, 12, full and
    ragged m_valid; pad rows keep the old stream, their statistics stay unwritten."""
    M, N = 2 * bm, gx.TILE_N
    for kt in gx.RESID16_KTILES:
        for mv in (M, gx.ragged(M, bm)):
            _resid16(env, bm, gx.case(M, N, 64 * kt, "stats", None, "cuda"), mv, bm, False)


# ------------------------------------------------------------------------------------------------ patch GEMM from the pixels
@pytest.mark.parametrize("B,S,P,d", gx.PIX_SHAPES)
def test_patch_from_pixels_exact(env, B, S, P, d):
    """mmiss_dbg_patch_from_pixels on bf16-exact pixels: the patch rows are exact f32; the CLS rows, and the sentinel rows behind
    the last image, are untouched. 48 rows (one tile, 112 pad rows), 176 rows (two tiles), and P = 32 (K = 3072)."""
    torch, _lib, lib = env
    p = _lib.ptr
    px, W, pos, rows = gx.pixel_case(B, S, P, d, "cuda")
    G2 = (S // P) ** 2
    T = G2 + 1
    out = _filled(torch, B * T, d, torch.float32)
    px32, W16, pos32 = gx.f32_tensor(px).contiguous(), gx.bf16_tensor(W), gx.f32_tensor(pos)
    _lib.check(lib.mmiss_dbg_patch_from_pixels(0, None, p(px32), p(W16), p(out), p(pos32), B, S, P, d))
    torch.cuda.synchronize()
    m = torch.arange(B * G2, device="cuda")
    idx = (m // G2) * T + 1 + m % G2
    gx.assert_f32_exact(out[idx], rows, 160, "patch_from_pixels B %d S %d P %d d %d" % (B, S, P, d))
    out[idx] = float("nan")
    gx.assert_untouched(out, _filled(torch, B * T, d, torch.float32), "CLS and sentinel rows")

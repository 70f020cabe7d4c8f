"""Is an encode call's result independent of everything earlier calls left in the handle? (tests/encoder_sequence_cases.py)

A victim call runs on a fresh handle A (every workspace = the zeros of alloc_zero) and on a long-lived handle B of the same shape,
weights, precision and max_batch after a NaN poison call and again after a twin poison call: the three results must be the same
bits, and finite; where the fp32 oracle is cheap they are also held to it at COS_TOL, so that A and B cannot be wrong together.
Every call asserts the path it means to take from the product (mmiss_dbg_encoder_plan) BEFORE it runs, and the kernel names
mmiss_prof_read recorded after it where the names tell the paths apart. The handles B live at module scope and go through every
case of their shape in turn, so each case also runs over whatever the cases before it left.

tests/golden/encoder_sequence_parent.json holds, per case, what the commit BEFORE mmiss_dbg_encoder_plan and its shared predicates
gave for the first poison call and the victim call after it: the profile (kernel, launches) and the sha256 of the victim's output
bytes. The entry and the refactoring that came with it must change neither (cases added later have no record there).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import encoder_sequence_cases as sc
from encoder_handles import bits as _bits, cos as _cos, new_handle as _new_handle, options as _options, plan as _plan

pytestmark = pytest.mark.gpu

_HANDLES = {}
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_sequence_parent.json")) as _f:
    _PARENT = json.load(_f)


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for enc in _HANDLES.values():
        enc.close()
    _HANDLES.clear()


def _shared_handle(case):
    key = (case.shape, case.tower, case.precision, case.max_batch, case.calibrated)
    if key not in _HANDLES:
        _HANDLES[key] = _new_handle(*key)
    return _HANDLES[key]


def _expected_kernels(plan, s, tower, rows):
    """(names that must be in the profile, names that must not) of a two-layer call on this plan: layer 0 runs the four planned
    GEMMs, layer 1 the QKV GEMM and the pruned tail."""
    fold, r16 = plan["fold"], plan["resid16"]
    d, mlp = (s.v_hidden, s.v_mlp) if tower == "vision" else (s.t_hidden, s.t_mlp)
    skinny_rows = 320 if 3 * d <= 1024 else 128      # gemm_skinny_ok: the launcher of the BM x 128 tile takes the skinny kernel up to here
    must, never = set(), set()
    must.add({"Skinny": "gemm_skinny_lnfold_bias", "P256": "gemm_bf16_lnfold_bias_p256" if fold else "gemm_bf16_bias_p256",
              "Tile256": "gemm_bf16_lnfold_bias" if fold else "gemm_bf16_bias", "Fp8Tile": "gemm_fp8_bias", "P256Fp8": "gemm_fp8_bias_p256",
              "Tile": "gemm_bf16_lnfold_bias" if fold else ("gemm_bf16_bias" if rows > skinny_rows else "gemm_skinny_bias")}[plan["qkv"]])
    fc2 = {"P160": f"gemm_bf16_bias_resid16_p160_k{mlp}", "Fp8Tile": "gemm_fp8_bias_resid16" if r16 else "gemm_fp8_bias_resid",
           "P256Fp8": "gemm_fp8_bias_resid16_p256",
           "Tile": f"gemm_bf16_bias_resid16_k{mlp}" if r16 else None}[plan["fc2"]]
    if fc2:
        must.add(fc2)
    if plan["fc2"] == "Tile" and plan["fc2_splitk"] and not (fold or plan["sfold"] or r16) and rows > 320:
        must.add("gemm_splitk_bias_resid")
    (must if plan["out8"] else never).add("attention_mx")
    (never if plan["pooled_tail"] else must).add("gather_pooled")
    for name in ("gemm_skinny_lnfold_bias", "gemm_skinny_lnfold_qgelu"):
        (must if plan["sfold"] else never).add(name)
    if not plan["fp8"]:
        never.update(("gemm_fp8_bias", "gemm_fp8_bias_p256", "layernorm_mxfp8", "layernorm16_mxfp8"))
    if not fold:
        never.update(("gemm_bf16_lnfold_bias", "gemm_bf16_lnfold_bias_p256"))
    if tower == "vision":
        if plan["embed"] == "Stats16":
            never.update(("row_stats", "cls_rows"))
        elif plan["lean_pre"]:
            never.add("cls_rows")
        else:
            must.add("cls_rows")
        if plan["sfold"] and plan["embed"] == "Nothing":
            must.add("row_stats")
        patch_rows = rows // s.v_tokens * (s.v_tokens - 1)
        if plan["patch"] == "P160":
            must.add("gemm_bf16_patch_p160")
        elif plan["patch_splitk"] and patch_rows > 320:
            must.add("gemm_splitk_patch")
    return must, never


def _profiled(fn):
    """fn() under the profiler: its result and the records of mmiss_prof_read."""
    from mmiss_amd import _lib

    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        out = fn()
    finally:
        _lib.prof_enable(False)
    return out, _lib.prof_read()


def _check_names(what, prof, expected):
    """Every (must, never) pair of `expected` (one per chunk of the call) against the profile's kernel names."""
    names = {p["kernel"] for p in prof}
    must = set().union(*(m for m, _ in expected))
    never = set.intersection(*(set(n) for _, n in expected))
    assert must <= names and not (never & names), f"{what}: missing {sorted(must - names)}, unexpected {sorted(never & names)} in {sorted(names)}"


def _run(enc, case, call, x):
    """One call of the case on `enc`: the plan asserted before, the kernel names after. Returns the embeddings, the plan and the
    profile. Text: encode_text trims the matrix itself (trim_padding = call.trim); the plan is asked for the trimmed length."""
    s = sc.SHAPES[case.shape]
    with _options(call.opts):
        if case.tower == "vision":
            plan = _plan(enc, case, call)
            rows = call.B * s.v_tokens
        else:
            T = sc.trimmed(case.shape, x, call.trim).shape[1]
            plan = _plan(enc, case, call, T)
            rows = call.B * T
        assert plan["M"] == rows, (case.name, plan)
        out, prof = _profiled(lambda: enc.encode_image(x) if case.tower == "vision" else enc.encode_text(x, trim_padding=call.trim))
    _check_names(f"{case.name} {call.kind}", prof, [_expected_kernels(plan, s, case.tower, rows)])
    return out, plan, prof


def _launches(prof):
    return sorted([p["kernel"], p["launches"]] for p in prof)


@pytest.mark.parametrize("case", sc.CASES, ids=[c.name for c in sc.CASES])
def test_victim_after_poison_is_the_fresh_handles_result(case):
    x = sc.call_input(case, case.victim)
    fresh = _new_handle(case.shape, case.tower, case.precision, case.max_batch, case.calibrated)
    try:
        want, _, _ = _run(fresh, case, case.victim, x)
    finally:
        fresh.close()
    assert np.isfinite(want).all(), case.name
    enc = _shared_handle(case)
    parent = _PARENT.get(case.name)
    for i, poison in enumerate(case.poisons):
        got_p, plan_p, prof_p = _run(enc, case, poison, sc.call_input(case, poison))
        if poison.kind == "twin":
            assert np.isfinite(got_p).all()
        elif not plan_p["fp8"]:     # (the MXFP8 producers take a block's amax with a NaN-ignoring max: what leaves an fp8 call is not pinned)
            assert np.isnan(got_p).all(), f"{case.name}: the NaN poison left finite output rows"
        got, _, prof = _run(enc, case, case.victim, x)
        bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1))
        assert bad.size == 0, (f"{case.name}: after the {poison.kind} poison {bad.size} of {len(got)} rows differ from the fresh handle's, first "
                               f"{bad[:8].tolist()}; finite {bool(np.isfinite(got).all())}, max |diff| {np.nanmax(np.abs(got - want)):.3e}")
        if parent and i == 0:
            assert _launches(prof_p) == parent["poison_kernels"], f"{case.name}: the poison call's launches changed"
            assert _launches(prof) == parent["victim_kernels"], f"{case.name}: the victim call's launches changed"
            assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == parent["victim_sha256"], f"{case.name}: output bytes changed"
    if case.oracle:
        d = (1 - _cos(want, sc.oracle_embed(case, case.victim))).max()
        assert d < sc.COS_TOL, f"{case.name}: 1 - cos vs the fp32 oracle {d:.3e}"


def test_the_parent_record_covers_the_cases_it_was_taken_on():
    assert len(set(_PARENT) & {c.name for c in sc.CASES}) >= 60


@pytest.mark.parametrize("via,max_batch,r", sc.CHUNK_CASES + sc.CHUNK_INT_CASES, ids=lambda v: str(v))
def test_last_chunk_of_a_long_call_after_a_hostile_chunk(via, max_batch, r):
    """(l) One call of max_batch + r images: the first chunk is NaN (f32 pixels) or a twin batch (u8 crops, raw RGB of mixed size: the
    integer routes hold no NaN), the last chunk of r images runs over everything it left, staging and crop buffers included. The
    first rows are NaN (or the twin's own embeddings), the last r are the fresh handle's bytes. Both chunks' plans are asserted on
    each handle before its calls, the kernel names of both after."""
    s = sc.SHAPES["tiny"]
    plain = (("fold", 0), ("sfold", 0), ("fp8", 0), ("resid16", 0), ("embed", "Nothing"), ("qkv", "Tile"), ("pooled_tail", 0))
    one = (("fold", 0), ("sfold", 1), ("embed", "Stats16"), ("qkv", "Skinny"), ("pooled_tail", 0))
    head_call = sc.Call("nan" if via == "f32" else "twin", max_batch, expect=plain, via=via, seed=3)
    tail_call = sc.Call("victim", r, expect=one if r == 1 else plain, via=via, seed=r)
    case = sc.Case(f"l-{via}-r{r}", "l", "tiny", "vision", tail_call, (), max_batch)
    tail, head = sc.call_input(case, tail_call), sc.call_input(case, head_call)
    encode = (lambda e, x: e.encode_image_rgb(x)) if via == "rgb" else (lambda e, x: e.encode_image(x))

    def expected(enc, calls):
        plans = [_plan(enc, case, c) for c in calls]
        assert [p["M"] for p in plans] == [c.B * s.v_tokens for c in calls]
        return [_expected_kernels(p, s, "vision", p["M"]) for p in plans]

    fresh = _new_handle("tiny", "vision", "bf16", max_batch)
    try:
        exp = expected(fresh, [tail_call])
        want, prof = _profiled(lambda: encode(fresh, tail))
        _check_names(case.name + " fresh tail", prof, exp)
        want_head = None if via == "f32" else encode(fresh, head)
    finally:
        fresh.close()
    enc = _shared_handle(case)
    both = head + tail if via == "rgb" else np.concatenate([head, tail])
    for _ in range(2):       # the second call runs over the first call's last chunk as well
        exp = expected(enc, [head_call, tail_call])
        got, prof = _profiled(lambda: encode(enc, both))
        _check_names(case.name, prof, exp)
        assert got.shape == (max_batch + r, 128)
        if via == "f32":
            assert np.isnan(got[:max_batch]).all()
        else:
            assert np.array_equal(_bits(got[:max_batch]), _bits(want_head))
        assert np.isfinite(got[max_batch:]).all() and np.array_equal(_bits(got[max_batch:]), _bits(want)), (via, r)
    ref = sc.oracle_embed(case, tail_call)
    assert (1 - _cos(want, ref)).max() < sc.COS_TOL


@pytest.mark.parametrize("hpb", (0, 2), ids=("gather", "pooled-tail"))
@pytest.mark.parametrize("trim", (False, True), ids=("full", "trim"))
@pytest.mark.parametrize("pc", sc.pooled_position_cases(), ids=lambda pc: pc[0])
def test_pooled_text_position(pc, trim, hpb):
    """text_embed_kernel picks the pooled row on the GPU and leaves it in pool_row, which the handle carries: every case of
    HF's rule through encode_text against the oracle, after a call whose pooled positions were all different. Both consumers of
    pool_row: gather_pooled (and the head's LayerNorm), and with att_hpb = 2 the causal pooled-query attention with the
    out-projection's row map. Plan before, kernel names after, like every sequence."""
    from oracle import clip_oracle as co

    name, shape, ids, want = pc
    s, W = sc.SHAPES[shape], sc.weights(shape)
    opts = (("att_hpb", hpb),) if hpb else ()
    expect = (("sfold", 1), ("fold", 0), ("fp8", 0), ("embed", "Nothing"), ("pooled_tail", 1 if hpb else 0))
    call = sc.Call("victim", len(ids), 16, opts, expect, trim)
    pre = sc.pooled_position_prelude(shape, want)
    pre_call = sc.Call("twin", len(pre), 16, opts, expect, trim)
    case = sc.Case(f"pool-{name}", "4", shape, "text", call, (), 8)
    fresh = _new_handle(shape, "text", "bf16", 8)
    try:
        alone, _, _ = _run(fresh, case, call, ids)
    finally:
        fresh.close()
    enc = _shared_handle(case)
    assert np.isfinite(_run(enc, case, pre_call, pre)[0]).all()
    got = _run(enc, case, call, ids)[0]
    ref = co.embed_texts(ids, W, s)
    assert np.isfinite(got).all() and (1 - _cos(got, ref)).max() < sc.COS_TOL, name
    assert np.array_equal(_bits(got), _bits(alone)), name
    # the oracle itself tells the pooled column from its neighbours: pooling another row would miss by more than the bound
    assert np.array_equal(co.eos_positions(ids, s.eos_token_id), want)

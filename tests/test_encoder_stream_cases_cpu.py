"""What test_encoder_streams_gpu.py relies on, established on the host (tests/encoder_stream_cases.py): the selection resolves in
the sequence table and leaves out plan (e) only, every hand-over poison covers its victim's rows, and the results the GPU tests
tell apart by their bits are far apart in the fp32 oracle, so that "equal bits" cannot hold by accident."""
import numpy as np

from oracle import clip_oracle as co
from oracle import fp8_oracle as fo
import encoder_handles as eh
import encoder_sequence_cases as sc
import encoder_stream_cases as st

# A GPU result lies within sc.COS_TOL = 1e-3 of the oracle's; two oracle rows more than 1e-2 apart (1 - cos) cannot both be
# within 1e-3 of one GPU row
APART = 1e-2


def test_every_name_resolves_in_the_sequence_table():
    names = {c.name for c in sc.CASES}
    assert set(st.all_names()) <= names, set(st.all_names()) - names
    assert len(set(st.ROUTE_NAMES)) == len(st.ROUTE_NAMES) == 20
    for n in st.all_names():
        c = st.case(n)
        if c.tower == "text":      # device input_ids are never trimmed: the reference is taken with trim_padding=False
            assert c.victim.trim is False, n
    for n, via in st.INT_ROUTES + st.ORDER:
        assert st.case(n).tower == "vision" or via == "f32", n
    assert {via for _, via in st.ORDER if st.case(_).tower == "vision"} == {"f32", "u8", "rgb"}
    assert any(st.case(n).tower == "text" for n, _ in st.ORDER)


def test_every_plan_row_but_e_is_present():
    rows = {st.case(n).plan for n in st.ROUTE_NAMES}
    assert rows == {c.plan for c in sc.CASES} - set(st.LEFT_OUT_PLANS), rows
    assert all(c.plan != "e" for c in map(st.case, st.all_names()))


def test_handover_poisons_cover_their_victims_rows():
    """sc's rule: poison rows >= round_up(victim rows, 256) + 192, in one chunk; and another B, another plan's workspace use."""
    for n in st.HANDOVER:
        c = st.case(n)
        x1, poison, x2 = st.handover_calls(c)
        M = sc.call_rows(c, x1)
        assert poison.kind == "nan" and poison.covers and poison.B <= c.max_batch and poison.B != x1.B, n
        assert sc.call_rows(c, poison) >= sc.round_up(M, 256) + 192, (n, M)
        assert (x2.B, x2.opts, x2.expect) == (x1.B, x1.opts, x1.expect) and x2.seed != x1.seed, n
    plans = [dict(st.case(n).victim.expect) for n in st.HANDOVER]
    assert plans[0].get("sfold") == 1 and plans[1].get("fp8") == 1 and plans[1].get("out8") == 1


def test_handover_results_are_pairwise_apart_in_the_oracle():
    for n in st.HANDOVER:
        c = st.case(n)
        assert c.oracle, n
        x1, poison, x2 = st.handover_calls(c)
        a, p, b = (sc.oracle_embed(c, call) for call in (x1, poison, x2))
        assert np.isnan(p).all(), n                      # the poison's own result: NaN in every row
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert (1 - eh.cos(a, b)).min() > APART, (n, (1 - eh.cos(a, b)).min())
        assert (a @ b.T).max() < 1 - APART, n            # no row of one is a row of the other either


def test_the_two_weight_sets_are_apart_in_the_oracle():
    c = st.case(st.WEIGHTS_CASE)
    s, x = sc.SHAPES[c.shape], sc.call_input(c, c.victim)
    W1, W2 = sc.weights(c.shape), st.weights2(c.shape)
    assert set(W1) == set(W2) and all(W1[k].shape == W2[k].shape for k in W1)
    a, b = co.embed_images(x, W1, s), co.embed_images(x, W2, s)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert (1 - eh.cos(a, b)).min() > APART, (1 - eh.cos(a, b)).min()


def test_calibrated_and_uncalibrated_fp8_operands_differ():
    """The fp8 QKV GEMM of layer 0 reads MXFP8(LayerNorm1(x)) uncalibrated and MXFP8(LayerNorm1(x) - mu) calibrated (mu folded back
    through the bias): simulated with oracle/fp8_oracle.py on the case's own input, the two operands differ in every row, and so do
    the settings before and after set_precision("fp8") (the bf16 operand is not on the e4m3 grid)."""
    c = st.case(st.CALIBRATION_CASE)
    assert c.calibrated and c.precision == "fp8" and not st.case(st.PRECISION_CASE).calibrated
    assert sc.call_input(c, c.victim).tobytes() == sc.call_input(st.case(st.PRECISION_CASE), st.case(st.PRECISION_CASE).victim).tobytes()
    s, W = sc.SHAPES[c.shape], sc.weights(c.shape)
    taps = {}
    co.image_features(sc.call_input(c, c.victim), W, s, taps=taps)
    p = "vision_model.encoder.layers.0.layer_norm1."
    h = co.layer_norm(taps[0], W[p + "weight"], W[p + "bias"], s.ln_eps).reshape(-1, s.v_hidden).astype(np.float32)
    mu = eh.calibration_table(c.shape)[0]
    assert mu.shape == (s.v_hidden,) and np.abs(mu).min() > 0
    plain = fo.mx_dequantize(*fo.mx_quantize(h))
    centred = fo.mx_dequantize(*fo.mx_quantize(h - mu)) + mu
    assert (plain != centred).any(axis=1).all()
    assert (plain != h).any(axis=1).all()
    b = st.bf16_twin_of(st.case(st.PRECISION_CASE))
    assert b.precision == "bf16" and dict(b.victim.expect)["fp8"] == 0 and b.victim.opts == st.case(st.PRECISION_CASE).victim.opts

"""Call sequences on ONE encoder handle, shared by test_encoder_sequence_cpu.py (which establishes on the host what the GPU tests
rely on) and test_encoder_sequence_gpu.py (which runs them). A plain helper module: no fixtures, numpy only, Philox seeds; every
call with the same arguments returns the same bits.

The question: is a call's result independent of everything earlier calls left in the handle? A case names a VICTIM call and two
POISON calls. The victim runs on a fresh handle (workspaces = the zeros of alloc_zero) and, on a second handle of the same shape,
weights, precision and max_batch, after each poison; the three results must be the same bits.

Poisons:
  nan    vision: every pixel NaN (encode_image accepts them). Text: prompts made of NAN_ID only, a reserved token whose embedding
         row is NaN in the state dict both handles load. Every buffer a kernel of the call writes then holds NaN in every row it
         covers (the fp32 oracle returns NaN in every output row: test_encoder_sequence_cpu.py).
  twin   another valid batch, finite, other seeds, scaled and shifted. It catches what a NaN-ignoring max swallows (the amax of an
         MX block, a softmax maximum, v_max_f32 returns the other operand).
A poison covers the rows a victim's tiles can read: poison rows >= round_up(victim rows, 256) + 192 (the CPU test asserts it for
every pair of the tables).

Victim row counts: for a tile height bm, M = B T with M % bm == 1, M % bm == bm - 1 and one exact multiple. The vision tower of
TINY has T = 5, so every residue is reachable for bm = 128, 192, 256 (gcd(5, bm) = 1): B = 77 (385 = 3 * 128 + 1 = 2 * 192 + 1),
205 (1025 = 4 * 256 + 1), 307 (1535 = 6 * 256 - 1). For bm = 160 only multiples of 5 are: the shape "tiny17" (patch 16: T = 17) gives
B = 113 (1921 = 12 * 160 + 1) and B = 47 (799 = 5 * 160 - 1).
"""
import dataclasses
import functools

import numpy as np

from oracle import clip_oracle as co

COS_TOL = 1e-3   # BASELINE.json north_star: "within 1e-3 cosine of the reference CPU path"

_T = dict(t_hidden=128, t_layers=2, t_heads=2, t_mlp=256, t_vocab=1000, t_ctx=16, proj_dim=128, eos_token_id=999)
SHAPES = {
    "tiny": co.TINY,                                                    # vision d = 128, T = 5, two layers; text ctx 16
    "tiny17": dataclasses.replace(co.TINY, v_patch=16),                 # T = 17
    # d = 512 / 1024 for the K and N rules of the 256-wide kernels (gemm256p_ok, gemm256p8_ok, gemm160p_ok), TINY-sized images
    "w512": co.ClipShape(v_hidden=512, v_layers=2, v_heads=8, v_mlp=2048, v_patch=32, v_image=64, **_T),
    "w1024": co.ClipShape(v_hidden=1024, v_layers=2, v_heads=16, v_mlp=4096, v_patch=32, v_image=64, **_T),
    # patch 14: 257 tokens (long / stream attention kernels) and 577 (tiled), narrow towers
    "t257": co.ClipShape(v_hidden=128, v_layers=2, v_heads=2, v_mlp=256, v_patch=14, v_image=224, **_T),
    "t577": co.ClipShape(v_hidden=128, v_layers=2, v_heads=2, v_mlp=256, v_patch=14, v_image=336, **_T),
    # legacy checkpoints: eos_token_id == 2, the pooled row is argmax(ids)
    "legacy": dataclasses.replace(co.TINY, eos_token_id=2),
}
NAN_ID = 997     # reserved: its token-embedding row is NaN; no victim prompt holds it (bos = 998, eos = 999 in every shape but legacy)

# option -> the default its call site passes (what a test restores)
OPTION_DEFAULTS = {
    "ln_fold_min_rows": 6000, "fp8_min_rows": 1024, "embed_fused": 1, "pooled_tail": 1, "skinny_fold": 1, "att_hpb": 0,
    "gemm_bm_qkv": 0, "gemm_bm_d": 0, "gemm_bm_mlp": 0, "prelayernorm_lean": 1, "resid16": -1, "gemm_256_fold": -1,
    "gemm_256_fold_mlp": 0, "gemm_p256": 1, "gemm_p256_fp8": 1, "attention_stream_min_pairs": 256,
    "gemm_splitk_target": 384,
}


def round_up(a, b):
    return (a + b - 1) // b * b


@dataclasses.dataclass(frozen=True)
class Call:
    kind: str                 # "victim" | "nan" | "twin"
    B: int
    T: int = 0                # text: columns of the id matrix handed over; vision: 0 (the shape's token count)
    opts: tuple = ()          # ((option, value), ...) in force during this call; OPTION_DEFAULTS otherwise
    expect: tuple = ()        # ((plan field, value), ...) asserted from mmiss_dbg_encoder_plan BEFORE the call
    trim: bool = True         # text: encode_text(trim_padding=...)
    via: str = "f32"          # vision input route: "f32" pixels, "u8" crops, "rgb" raw images of mixed size
    seed: int = 0
    covers: bool = True       # a poison: it writes every row the victim's tiles can read (else it is there for the LAYOUT it leaves)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    plan: str                 # the row of the issue's plan table (DESIGN.md "the encoder's state between calls")
    shape: str
    tower: str                # "vision" | "text"
    victim: Call
    poisons: tuple            # two Calls, run in this order, the victim after each
    max_batch: int = 256
    precision: str = "bf16"   # "bf16" | "fp8" (text: set_tower_precision)
    oracle: bool = True       # also held to the fp32 oracle at COS_TOL
    calibrated: bool = False  # fp8: a calibration table installed on both handles


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def weights(shape_key):
    s = SHAPES[shape_key]
    W = co.init_weights(s, seed=97)
    tok = W["text_model.embeddings.token_embedding.weight"].copy()
    tok[NAN_ID] = np.nan
    W["text_model.embeddings.token_embedding.weight"] = tok
    return W


def images(shape_key, kind, B, seed, via="f32"):
    """f32 [B,3,S,S] (via f32), uint8 [B,S,S,3] (u8) or a list of raw uint8 [H,W,3] images of mixed size (rgb)."""
    s = SHAPES[shape_key]
    S = s.v_image
    g = np.random.Generator(np.random.Philox(key=[20251019, 1000 * seed + {"victim": 1, "twin": 2, "nan": 3}[kind]]))
    if via == "f32":
        if kind == "nan":
            return np.full((B, 3, S, S), np.nan, np.float32)
        px = g.standard_normal((B, 3, S, S), dtype=np.float32)
        return px * np.float32(1.7) + np.float32(0.3) if kind == "twin" else px
    assert kind != "nan", "integer pixels hold no NaN"
    if via == "u8":
        return g.integers(0, 256, size=(B, S, S, 3), dtype=np.uint8)
    sizes = [(S, S), (S + 13, 2 * S), (3 * S, S + 5), (S + 1, S + 1)]
    return [g.integers(0, 256, size=sizes[i % 4] + (3,), dtype=np.uint8) for i in range(B)]


def text_ids(shape_key, kind, B, T, seed):
    """int32 [B,T]. victim / twin: BOS, body, the first EOS at a random position in [2, T-1], EOS padding; no NAN_ID."""
    s = SHAPES[shape_key]
    if kind == "nan":
        return np.full((B, T), NAN_ID, np.int32)
    if s.eos_token_id == 2:      # legacy: the pooled row is the argmax; ids below NAN_ID, one maximum per row
        g = np.random.Generator(np.random.Philox(key=[20251019, 7000 + seed + (500 if kind == "twin" else 0)]))
        ids = g.integers(3, 900, size=(B, T), dtype=np.int32)
        ids[np.arange(B), g.integers(0, T, size=B)] = 950
        return ids
    ids = co.synthetic_text_ids(B, T, s.t_vocab, s.eos_token_id, seed=seed + (500 if kind == "twin" else 0))
    body = (ids != s.eos_token_id) & (ids != s.eos_token_id - 1)
    # victims speak in even ids, twins in odd ones below NAN_ID: no twin prompt is a victim prompt, and none holds NAN_ID
    ids[body] = ids[body] % 498 * 2 + (1 if kind == "twin" else 0)
    return ids


def trimmed(shape_key, ids, trim):
    """The matrix ClipEncoder.encode_text hands to the library (host arrays): columns after the last row's EOS dropped."""
    s = SHAPES[shape_key]
    if not trim:
        return ids
    eos = s.eos_token_id
    pos = ids.argmax(axis=1) if eos == 2 else (ids == eos).argmax(axis=1)
    has = np.ones(ids.shape[0], bool) if eos == 2 else (ids == eos).any(axis=1)
    return np.ascontiguousarray(ids[:, : int(pos.max()) + 1]) if has.all() else ids


def call_input(case, call):
    if case.tower == "vision":
        return images(case.shape, call.kind, call.B, call.seed, call.via)
    return text_ids(case.shape, call.kind, call.B, call.T, call.seed)


def call_rows(case, call):
    """Token rows the call's chunk runs on (text: after trimming)."""
    if case.tower == "vision":
        return call.B * SHAPES[case.shape].v_tokens
    return call.B * trimmed(case.shape, call_input(case, call), call.trim).shape[1]


def oracle_embed(case, call):
    """The fp32 oracle on the call's input (u8 / rgb: on the normalised crops the oracle's own preprocessing makes)."""
    s, W = SHAPES[case.shape], weights(case.shape)
    x = call_input(case, call)
    with np.errstate(all="ignore"):
        if case.tower == "text":
            return co.embed_texts(x, W, s)
        if call.via == "u8":
            x = co.normalize_u8(x)
        elif call.via == "rgb":
            from PIL import Image

            x = np.stack([co.preprocess_image(Image.fromarray(a), s.v_image) for a in x])
        return co.embed_images(x, W, s)


# ------------------------------------------------------------------------------------------------ the tables
def _o(**kw):
    return tuple(sorted(kw.items()))


def _vision_cases():
    C = []
    big = 256                                   # TINY: 1280 rows, covers victims up to 1025 rows + 192

    def add(name, plan, B, opts, expect, shape="tiny", max_batch=big, poisons=None, precision="bf16", oracle=True, calibrated=False,
            via="f32"):
        v = Call("victim", B, opts=opts, expect=expect, seed=B, via=via)
        if poisons is None:
            poisons = (Call("nan", max_batch, opts=opts), Call("twin", max_batch, opts=opts, seed=3))
        C.append(Case(name, plan, shape, "vision", v, tuple(poisons), max_batch, precision, oracle, calibrated))

    # (a) one request, skinny folded chain; poisoned by calls of plan (c), whose statistics in tw.stats are per 64 columns
    fold_lo = _o(ln_fold_min_rows=129)
    pa = (Call("nan", big, opts=fold_lo, expect=_o(fold=1, sfold=0, embed="Stats64")),
          Call("twin", big, opts=fold_lo, seed=3, expect=_o(fold=1, sfold=0, embed="Stats64")))
    for B in (1, 25):                           # M = 1 T, 125
        add(f"a-sfold-B{B}", "a", B, fold_lo, _o(sfold=1, embed="Stats16", qkv="Skinny", fc1="Skinny", pooled_tail=0, att_hpb=1), poisons=pa)
        add(f"a-sfold-pooled-B{B}", "a", B, fold_lo + _o(att_hpb=2), _o(sfold=1, embed="Stats16", pooled_tail=1),
            poisons=tuple(dataclasses.replace(p, opts=p.opts + _o(att_hpb=2)) for p in pa))
    add("a-sfold-unfused-B25", "a", 25, _o(embed_fused=0, ln_fold_min_rows=129), _o(sfold=1, embed="Nothing"), poisons=pa)
    add("a-sfold-fulltail-B25", "a", 25, _o(att_hpb=2, pooled_tail=0, ln_fold_min_rows=129), _o(sfold=1, pooled_tail=0),
        poisons=tuple(dataclasses.replace(p, opts=p.opts + _o(att_hpb=2)) for p in pa))
    add("a-plain-skinny-B25", "a", 25, _o(skinny_fold=0, ln_fold_min_rows=129), _o(sfold=0, fold=0, qkv="Tile"), poisons=pa)
    # M = 128 needs T | 128: the text tower (case j-a-128)

    # (b) small plain call: f32 stream, separate LayerNorm, pruned tail through gather_pooled. Up to 320 rows the launcher takes
    # the skinny kernel for every GEMM this narrow (130, 255 rows), above it the BM x 128 tile: M % 128 == 1, 127, 0 (385, 895, 640)
    for B in (26, 51, 77, 179, 128):
        add(f"b-plain-B{B}", "b", B, (), _o(fold=0, sfold=0, fp8=0, resid16=0, prune=1, embed="Nothing", qkv="Tile", pooled_tail=0))
    # ... poisoned by one request (16-column statistics, xb written) and the reverse of (a): (c) after (a)
    add("c-after-a-B77", "c", 77, fold_lo, _o(fold=1, resid16=1, embed="Stats64"), poisons=(
        Call("twin", 25, opts=fold_lo, seed=3, expect=_o(sfold=1, embed="Stats16"), covers=False),
        Call("nan", 1, opts=fold_lo, seed=4, expect=_o(sfold=1, embed="Stats16"), covers=False)))

    # (c) folded LayerNorm on the BM x 128 tile, bf16 residual stream: every height through the three option keys
    def fold(bm, lean=1, r16=-1):
        return _o(ln_fold_min_rows=129, gemm_bm_qkv=bm, gemm_bm_d=bm, gemm_bm_mlp=bm, prelayernorm_lean=lean, resid16=r16)

    for bm, Bs in ((128, (77, 51, 128)), (192, (77, 115, 192))):      # 5 B % bm == 1, bm - 5 + ... : 385, 255 | 575 = 3 * 192 - 1, 960
        for B in Bs:
            add(f"c-fold-bm{bm}-B{B}", "c", B, fold(bm), _o(fold=1, resid16=1, embed="Stats64", lean_pre=1, qkv="Tile", qkv_bm=bm, out_bm=bm,
                                                          fc1_bm=bm, fc2_bm=bm))
    for B in (113, 47, 160):                                          # 17 B = 1921 = 12 * 160 + 1, 799 = 5 * 160 - 1, 2720 = 17 * 160
        add(f"c-fold-bm160-B{B}", "c", B, fold(160), _o(fold=1, resid16=1, qkv_bm=160, out_bm=160, fc1_bm=160, fc2_bm=160), shape="tiny17",
            max_batch=192)
    add("c-fold-fat-pre-B77", "c", 77, fold(128, lean=0), _o(fold=1, resid16=1, embed="Stats64", lean_pre=0))
    add("c-fold-f32resid-B77", "c", 77, fold(128, r16=0), _o(fold=1, resid16=0, embed="Stats64", lean_pre=0))
    add("c-fold-f32resid-bm192-B115", "c", 115, fold(192, r16=0), _o(fold=1, resid16=0, qkv_bm=192))

    # (d) folded on the 256 x 256 tile and on its persistent form; d = 512 (K rule of gemm256p_ok), d = 1024 (ln_finalize)
    t256 = _o(ln_fold_min_rows=129, gemm_256_fold=256, gemm_256_fold_mlp=1, gemm_p256=0)
    p256 = _o(ln_fold_min_rows=129, gemm_p256=2)
    for B in (205, 307, 256):                                         # 1025 = 4 * 256 + 1, 1535 = 6 * 256 - 1, 1280
        add(f"d-tile256-B{B}", "d", B, t256, _o(fold=1, qkv="Tile256", fc1="Tile256"), shape="w512", max_batch=384)
        add(f"d-p256-B{B}", "d", B, p256, _o(fold=1, qkv="P256", fc1="P256"), shape="w512", max_batch=384)
    for B in (205, 307):
        add(f"d-p256-final-B{B}", "d", B, p256, _o(fold=1, fold_final=1, qkv="P256", fc1="P256"), shape="w1024", max_batch=384)

    # (e) P160 residual GEMMs and the patch GEMM on the same kernel: 200 .. 256 tiles of 160 x 256 at d = 512
    pe = _o(ln_fold_min_rows=129)
    for B in (4001, 4096):                                            # 20005 rows (% 160 == 5), 20480 = 128 * 160; 16004 / 16384 patch rows
        add(f"e-p160-B{B}", "e", B, pe, _o(fold=1, resid16=1, out="P160", fc2="P160", patch="P160"), shape="w512", max_batch=4160,
            oracle=False)

    # (f) split-K FC2 and split-K patch GEMM (f32 stream, K >= 1536, few tiles); poisoned by a call whose split count differs
    fk = (Call("nan", 384, expect=_o(fc2_splitk=1)), Call("twin", 384, seed=3, opts=_o(gemm_splitk_target=128)))
    for B in (77, 179, 128, 205):                                     # above the skinny kernel's 320 rows: 385, 895, 640, 1025
        add(f"f-splitk-B{B}", "f", B, (), _o(fold=0, resid16=0, fc2="Tile", fc2_splitk=1, patch="Tile", patch_splitk=1), shape="w512",
            max_batch=384, poisons=fk)

    # (g) fp8 on gemm8_kernel; out8 (MXFP8 attention output) where the bf16 stream is on; below fp8_min_rows: bf16 kernels over
    # buffers the fp8 calls wrote, and the reverse
    g8 = _o(fp8_min_rows=129, ln_fold_min_rows=129)
    for B in (77, 51, 128):
        add(f"g-fp8-out8-B{B}", "g", B, g8, _o(fp8=1, out8=1, resid16=1, qkv="Fp8Tile", out="Fp8Tile", fc2="Fp8Tile"), precision="fp8")
    add("g-fp8-f32resid-B77", "g", 77, _o(fp8_min_rows=129), _o(fp8=1, out8=0, resid16=0, qkv="Fp8Tile", out="Tile"), precision="fp8")
    add("g-fp8-calibrated-B77", "g", 77, g8, _o(fp8=1, out8=1), precision="fp8", calibrated=True)
    lo = _o(fp8_min_rows=400, ln_fold_min_rows=129)                   # 385 rows: bf16 folded; the poisons (1280 rows): fp8
    add("g-bf16-after-fp8-B77", "g", 77, lo, _o(fp8=0, fold=1), precision="fp8",
        poisons=(Call("nan", big, opts=lo, expect=_o(fp8=1, out8=1)), Call("twin", big, opts=lo, seed=3, expect=_o(fp8=1))))
    add("g-bf16-small-after-fp8-B25", "g", 25, lo, _o(fp8=0, sfold=1), precision="fp8",
        poisons=(Call("nan", big, opts=lo, expect=_o(fp8=1, out8=1)), Call("twin", big, opts=lo, seed=3, expect=_o(fp8=1))))
    hi = _o(fp8_min_rows=129, ln_fold_min_rows=129)
    add("g-fp8-after-bf16-B77", "g", 77, hi, _o(fp8=1, out8=1), precision="fp8",
        poisons=(Call("nan", big, opts=_o(fp8_min_rows=5000, ln_fold_min_rows=129), expect=_o(fp8=0, fold=1)),
                 Call("twin", 25, opts=_o(fp8_min_rows=5000), seed=3, expect=_o(fp8=0, sfold=1), covers=False)))

    # (h) fp8 on the persistent 256 x 256 kernel (d >= 512, K % 256 == 0), also calibrated
    h8 = _o(fp8_min_rows=129, ln_fold_min_rows=129, gemm_p256_fp8=2)
    for B in (205, 307, 256):
        add(f"h-p256fp8-B{B}", "h", B, h8, _o(fp8=1, out8=1, qkv="P256Fp8", out="P256Fp8", fc1="P256Fp8", fc2="P256Fp8"), shape="w512",
            max_batch=384, precision="fp8")
    add("h-p256fp8-calibrated-B205", "h", 205, h8, _o(fp8=1, qkv="P256Fp8"), shape="w512", max_batch=384, precision="fp8", calibrated=True)

    # (i) the same kernel at d = 1024 (two scale groups per tile at K = 1024): a ragged last block, M in (Mpad - 256, Mpad - 128], and one without
    i8 = _o(fp8_min_rows=129, ln_fold_min_rows=129, gemm_p256_fp8=2)
    for B in (180, 205, 307, 256):                                    # 900 (not ragged: above Mpad - 128), 1025, 1535, 1280
        add(f"i-p256fp8-w1024-B{B}", "i", B, i8, _o(fp8=1, out8=1, qkv="P256Fp8", out="P256Fp8", fc1="P256Fp8", fc2="P256Fp8"), shape="w1024",
            max_batch=384, precision="fp8")
    add("i-p256fp8-w1024-ragged-B170", "i", 170, i8, _o(fp8=1, out8=1, qkv="P256Fp8"), shape="w1024", max_batch=384, precision="fp8")  # 850 in (768, 896]

    # (k) the attention kernel by token count, inside an encode (T <= 128: every case above; one head per workgroup unless att_hpb)
    add("k-heads-B77", "k", 77, _o(att_hpb=2), _o(sfold=0, pooled_tail=1, att_hpb=2), max_batch=big)
    add("k-long257-B3", "k", 3, (), _o(M=771, pooled_tail=0, att_stream=0), shape="t257", max_batch=8)
    add("k-stream257-B3", "k", 3, _o(attention_stream_min_pairs=4), _o(M=771, pooled_tail=0, att_stream=1), shape="t257", max_batch=8)
    add("k-tiled577-B2", "k", 2, (), _o(M=1154, pooled_tail=0), shape="t577", max_batch=5)
    add("k-fp8-mx-long257-B3", "k", 3, g8, _o(fp8=1, out8=1), shape="t257", max_batch=8, precision="fp8")
    add("k-fp8-mx-stream257-B3", "k", 3, g8 + _o(attention_stream_min_pairs=4), _o(fp8=1, out8=1, att_stream=1), shape="t257", max_batch=8, precision="fp8")
    add("k-fp8-mx-tiled577-B2", "k", 2, g8, _o(fp8=1, out8=1), shape="t577", max_batch=5, precision="fp8")
    return C


def _text_cases():
    C = []

    def add(name, B, T, opts, expect, pT, trim=True, precision="bf16", max_batch=256, pB=None, oracle=True):
        pB = pB or max_batch
        v = Call("victim", B, T, opts, expect, trim, seed=B + T)
        ps = (Call("nan", pB, pT[0], opts, trim=trim), Call("twin", pB, pT[1], opts, trim=trim, seed=3))
        C.append(Case(name, "j", "tiny", "text", v, ps, max_batch, precision, oracle))

    fold_lo = _o(ln_fold_min_rows=129)
    # victim T smaller and larger than the poison's T: rows land at other offsets; trimmed and untrimmed
    for trim in (True, False):
        t = "trim" if trim else "full"
        add(f"j-a-B7-T16-{t}", 7, 16, (), _o(sfold=1, embed="Nothing"), (9, 16), trim)
        add(f"j-a-128-B8-T16-{t}", 8, 16, (), _o(sfold=1, fold=0), (9, 16), trim)      # untrimmed: M = 128
        add(f"j-b-B29-T9-{t}", 29, 9, (), _o(fold=0, sfold=0, resid16=0), (16, 5), trim)
        add(f"j-c-B43-T9-{t}", 43, 9, fold_lo, _o(fold=1, resid16=1, embed="Nothing"), (16, 5), trim)
        add(f"j-c-B24-T16-{t}", 24, 16, fold_lo, _o(fold=1, resid16=1), (7, 11), trim)
        # the causal pooled-query tail: pool_row (per-row EOS positions) feeds launch_attention_pooled and the out-projection's rowmap
        add(f"j-a-pooled-B7-T16-{t}", 7, 16, _o(att_hpb=2), _o(sfold=1, pooled_tail=1, att_hpb=2), (9, 16), trim)
        add(f"j-b-pooled-B29-T9-{t}", 29, 9, _o(att_hpb=2), _o(fold=0, sfold=0, pooled_tail=1), (16, 5), trim)
        add(f"j-c-pooled-B43-T9-{t}", 43, 9, fold_lo + _o(att_hpb=2), _o(fold=1, resid16=1, pooled_tail=1), (16, 5), trim)
    g8 = _o(fp8_min_rows=129, ln_fold_min_rows=129)
    add("j-g-fp8-B43-T9", 43, 9, g8, _o(fp8=1, out8=0, qkv="Fp8Tile"), (16, 5), False, precision="fp8", oracle=False)
    return C


VISION_CASES = tuple(_vision_cases())
TEXT_CASES = tuple(_text_cases())
CASES = VISION_CASES + TEXT_CASES


# (l) one call longer than max_batch: B = max_batch + r, the first max_batch images NaN. (route, max_batch, r): r = 1 and r leaving
# M % 128 == 1 (5 * 77 = 385) on the plain path of TINY
CHUNK_CASES = (("f32", 160, 1), ("f32", 160, 77))
# the integer routes hold no NaN: the first chunk is a twin batch, and the staging / crop buffers it filled are reused by the tail
CHUNK_INT_CASES = (("u8", 160, 1), ("u8", 160, 77), ("rgb", 160, 1), ("rgb", 160, 77))


# ------------------------------------------------------------------------------------------------ pooled text position (section 4)
def pooled_position_cases():
    """(name, shape key, ids int32 [B, 16], the pooled column of every row): test_encoder_sequence_cpu.py holds the table to
    co.eos_positions. Each is run after a call whose pooled positions all differ from these (`pooled_position_prelude`)."""
    T, eos, bos = 16, 999, 998
    g = np.random.Generator(np.random.Philox(key=[20251019, 4]))

    def body(B):
        ids = g.integers(0, NAN_ID, size=(B, T), dtype=np.int32)
        ids[:, 0] = bos
        return ids

    out = []
    a = body(4); a[:, 0] = eos
    out.append(("eos-at-0", "tiny", a, np.zeros(4, np.int64)))
    a = body(4); a[:, T - 1] = eos
    out.append(("eos-at-T-1", "tiny", a, np.full(4, T - 1, np.int64)))
    a = body(5); pos = np.array([3, 7, 1, 12, 5])
    for r, p in enumerate(pos):
        a[r, p] = eos; a[r, min(p + 2, T - 1)] = eos; a[r, T - 1] = eos
    out.append(("several-eos-first-counts", "tiny", a, pos.astype(np.int64)))
    a = body(6); pos = np.array([4, 0, 9, 0, 15, 0])
    for r in (0, 2, 4):
        a[r, pos[r]:] = eos
    out.append(("rows-without-eos-pool-row-0", "tiny", a, pos.astype(np.int64)))
    # legacy argmax: a tied maximum (the first counts), the maximum at 0 and at T - 1
    a = g.integers(3, 900, size=(6, T), dtype=np.int32)
    pos = np.array([5, 2, 0, T - 1, 0, T - 1])
    a[0, 5] = a[0, 11] = 950
    a[1, 2] = a[1, 3] = a[1, 15] = 960
    a[2, 0] = 970
    a[3, T - 1] = 970
    a[4, 0] = a[4, T - 1] = 980
    a[5, T - 1] = 990
    out.append(("legacy-argmax-ties-and-ends", "legacy", a, pos.astype(np.int64)))
    return out


def pooled_position_prelude(shape_key, want):
    """ids int32 [max(len(want), 8), 16] whose pooled column differs from `want` in every row want has (a stale pool_row entry shows)."""
    s = SHAPES[shape_key]
    B, T = max(len(want), 8), 16
    g = np.random.Generator(np.random.Philox(key=[20251019, 5]))
    ids = g.integers(3, 900, size=(B, T), dtype=np.int32)
    for r in range(B):
        p = (int(want[r]) + 6) % T if r < len(want) else 6
        ids[r, p] = s.eos_token_id if s.eos_token_id != 2 else 995
    return ids

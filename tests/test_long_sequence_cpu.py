"""Towers above 288 tokens, the part that needs no GPU: mmiss_encoder_create's shape check (it runs before the device is
touched), the exported debug entry of the key-chunked attention kernel, and the compiler's resource report for that kernel."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_HIP, ERR_UNSUPPORTED = 0, -2, -5   # include/mmiss.h


def _create(shape):
    """(status, last error) of mmiss_encoder_create for `shape`; an encoder that was created (a GPU is present) is destroyed."""
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    s = shape
    cfg = _lib.ClipConfigStruct(
        C.sizeof(_lib.ClipConfigStruct), s.v_hidden, s.v_layers, s.v_heads, s.v_mlp, s.v_patch, s.v_image,
        s.t_hidden, s.t_layers, s.t_heads, s.t_mlp, s.t_vocab, s.t_ctx, s.proj_dim, s.eos_token_id, float(s.ln_eps), 1, 1)
    h = C.c_void_p()
    rc = lib.mmiss_encoder_create(C.byref(cfg), 0, C.byref(h))
    msg = (lib.mmiss_last_error() or b"").decode("utf-8", "replace")
    if rc == OK:
        lib.mmiss_encoder_destroy(h)
    return rc, msg


def _l14(**kw):
    import dataclasses
    from mmiss_amd.encoder import VIT_L14_336

    return dataclasses.replace(VIT_L14_336, v_layers=1, t_layers=1, t_vocab=1000, eos_token_id=999, **kw)   # (one layer: light where a GPU is present)


def test_named_shape_of_l14_at_336():
    from mmiss_amd.encoder import LONGCLIP_L14, VIT_L14_336, ClipShape

    s = VIT_L14_336
    assert s.v_tokens == 577 and (s.v_image, s.v_patch, s.t_ctx) == (336, 14, 77)
    for f in ("v_hidden", "v_layers", "v_heads", "v_mlp", "t_hidden", "t_layers", "t_heads", "t_mlp", "proj_dim"):
        assert getattr(s, f) == getattr(LONGCLIP_L14, f), f
    # what from_hf_config makes of the checkpoint's config.json (keys equal to the HF defaults omitted, as saved configs do)
    cfg = {"projection_dim": 768,
           "vision_config": {"hidden_size": 1024, "num_hidden_layers": 24, "num_attention_heads": 16, "intermediate_size": 4096,
                             "patch_size": 14, "image_size": 336},
           "text_config": {"hidden_size": 768, "num_attention_heads": 12, "intermediate_size": 3072}}
    assert ClipShape.from_hf_config(cfg) == s


def test_create_accepts_577_tokens_and_fails_only_at_the_device():
    import torch

    rc, msg = _create(_l14())
    assert rc != ERR_UNSUPPORTED, msg
    if torch.cuda.is_available():
        assert rc == OK, msg
    else:
        assert rc == ERR_HIP and "no HIP device" in msg, (rc, msg)


@pytest.mark.parametrize("kw", [dict(v_image=462), dict(t_ctx=1026)])   # 33 x 33 + 1 = 1090 vision tokens; 1026 text tokens
def test_create_refuses_more_than_1025_tokens(kw):
    rc, msg = _create(_l14(**kw))
    assert rc == ERR_UNSUPPORTED and "1025" in msg, (rc, msg)


def test_create_accepts_1025_tokens_as_far_as_the_shape_goes():
    rc, msg = _create(_l14(v_image=448, t_ctx=1025))
    assert rc in (OK, ERR_HIP), (rc, msg)


def test_tiled_attention_entry_is_exported():
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    assert hasattr(C.CDLL(_lib.LIB_PATH), "mmiss_dbg_attention_tiled")
    assert len(_lib.SIGNATURES["mmiss_dbg_attention_tiled"][1]) == 10


def test_tiled_attention_kernels_do_not_spill():
    """attention_tiled_kernel carries a query tile's softmax state and the next chunk's 16 staging registers across the key
    loop: scratch there would put memory traffic into the loop the chunking exists to keep fed. All three instantiations."""
    path = os.path.join(ROOT, "multimodal-image-similarity-search_amd", "csrc", "api_encoder.resources.txt")
    if not os.path.exists(path):
        pytest.skip("no resource report: the library was not built by csrc/Makefile in this tree")
    seen = set()
    for b in re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]:
        name = b.split()[0]
        if "attention_tiled_kernel" not in name:
            continue
        seen.add(name)
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        assert scratch == 0 and spill == 0, (name, scratch, spill)
    assert len(seen) == 3, seen   # <false, false>, <true, false>, <false, true>

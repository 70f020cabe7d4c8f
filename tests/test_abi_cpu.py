"""The C-ABI library loads on a machine without a GPU and exports every symbol include/*.h declares; the ctypes
prototypes cover the same set (no compute is called here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(mmiss_[a-z0-9_]+)\s*\(", text))


def test_library_exports_every_declared_symbol():
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libmmiss.so is not built: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _declared("mmiss.h") | _declared("mmiss_debug.h")
    assert len(declared) >= 35
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, f"declared in include/ but not exported: {missing}"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))


def test_loads_and_reports_no_device_without_a_gpu():
    import torch
    import mmiss_amd  # noqa: F401
    from mmiss_amd import _lib

    lib = _lib.load()
    assert lib.mmiss_abi_version() == 1
    if not torch.cuda.is_available():
        assert _lib.device_count() == 0


def test_compute_entry_points_fail_loudly_without_a_gpu():
    """No CPU fallback: creating an index or an encoder without a device is an error, not a silent slow path."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import mmiss_amd  # noqa: F401
    from mmiss_amd.encoder import ClipEncoder
    from mmiss_amd.index import FlatIndex, blend
    import numpy as np

    with pytest.raises(RuntimeError, match="no HIP device"):
        FlatIndex(512, "f32")
    with pytest.raises(RuntimeError, match="no HIP device"):
        ClipEncoder()
    with pytest.raises(RuntimeError, match="no HIP device"):
        blend(np.ones((1, 128), np.float32), np.ones((1, 128), np.float32), 0.5)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "multimodal-image-similarity-search_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f


def test_encoder_files_launch_through_launchers_only():
    """Every kernel the encoder runs is launched by the launch_* function beside it in its header (preconditions, profile
    record, error check), and the debug ABI calls the same function: neither file launches a kernel itself."""
    for f in ("api_encoder.hip", "api_encoder_debug.h"):
        text = open(os.path.join(ROOT, "multimodal-image-similarity-search_amd", "csrc", f)).read()
        assert "hipLaunchKernelGGL" not in text, f


def test_persistent_gemm_kernels_do_not_spill():
    """The persistent GEMM counts its own vector-memory operations (s_waitcnt vmcnt(N) with N = loads it leaves in flight):
    a register spill is a scratch load / store the count does not know about — correct only by over-waiting, and measured
    6 x slower. The build writes the compiler's per-kernel resource report next to the objects (csrc/Makefile)."""
    import re

    seen = 0
    for obj in ("api_encoder", "api_index"):
        path = os.path.join(ROOT, "multimodal-image-similarity-search_amd", "csrc", obj + ".resources.txt")
        if not os.path.exists(path):
            pytest.skip("no resource report: the library was not built by csrc/Makefile in this tree")
        text = open(path).read()
        for b in re.split(r"remark: [^\n]*Function Name: ", text)[1:]:
            name = b.split()[0]
            if not any(k in name for k in ("gemm256p_kernel", "gemm256s_kernel", "gemm160p_kernel", "gemm256p8_kernel", "attention_stream_kernel")):
                continue
            seen += 1
            scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
            spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
            assert scratch == 0 and spill == 0, (name, scratch, spill)
    assert seen >= 17, seen   # (round 5: + three extensions of the fp8 kernel, two forms of the streaming attention)


def _gfx950_disassembly(obj_name, tmp_path):
    """The gfx950 code object of csrc/<obj_name>.o, disassembled: {kernel symbol: [instruction text, ...]}."""
    import shutil
    import subprocess

    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    src = os.path.join(ROOT, "multimodal-image-similarity-search_amd", "csrc", obj_name + ".o")
    if not os.path.exists(src) or not os.path.exists(objdump):
        pytest.skip("no object file / no llvm-objdump: the library was not built by csrc/Makefile in this tree")
    work = str(tmp_path)
    shutil.copy(src, work)
    subprocess.check_call([objdump, "--offloading", obj_name + ".o"], cwd=work, stdout=subprocess.DEVNULL)   # writes the bundles next to the copy
    co = [f for f in os.listdir(work) if "gfx950" in f]
    assert len(co) == 1, os.listdir(work)
    text = subprocess.check_output([objdump, "-d", co[0]], cwd=work, text=True)
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    return kernels


def test_streaming_attention_owns_every_use_of_m0(tmp_path):
    """attention_stream.h issues its LDS-DMA pieces from inline asm that writes m0 (the LDS destination of `buffer_load ... lds`).
    m0 is reserved: hipcc ignores it in a clobber list, so nothing tells the compiler it changed. That is safe only while no
    other instruction of the kernel depends on m0 — enforced here on the ISA: every instruction that names m0 is the
    `s_mov_b32 m0` of one asm statement, followed by that statement's own `s_nop 0` and `buffer_load ... lds`; every LDS-DMA
    load has such a head; nothing with an implicit m0 operand (s_movrel, ds_gws, s_sendmsg, interpolation) appears."""
    kernels = _gfx950_disassembly("api_encoder", tmp_path)
    mine = {k: v for k, v in kernels.items() if "attention_stream_kernel" in k}
    assert len(mine) == 2, sorted(mine)          # bf16 and MXFP8 output
    for name, ins in mine.items():
        heads = dma = 0
        for i, text in enumerate(ins):
            op = text.split()[0]
            assert not op.startswith(("s_movrel", "v_movrel", "ds_gws", "s_sendmsg", "v_interp", "s_load_dword_m0")), (name, text)
            if op.startswith("buffer_load") and text.endswith(" lds"):
                dma += 1
                assert ins[i - 1] == "s_nop 0" and ins[i - 2].startswith("s_mov_b32 m0, "), (name, ins[i - 3:i + 1])
            if re.search(r"\bm0\b", text):
                assert op == "s_mov_b32" and text.startswith("s_mov_b32 m0, "), (name, text)      # never read, never written otherwise
                assert ins[i + 1] == "s_nop 0" and ins[i + 2].startswith("buffer_load") and ins[i + 2].endswith(" lds"), (name, ins[i:i + 3])
                heads += 1
        assert heads == dma and dma >= 8, (name, heads, dma)


def test_build_log_has_no_inline_asm_warnings():
    """`clobber list contains reserved registers` (-Winline-asm) was 24 warnings per build while attention_stream.h listed m0."""
    for obj in ("api_encoder", "api_index", "runtime"):
        path = os.path.join(ROOT, "multimodal-image-similarity-search_amd", "csrc", obj + ".resources.txt")
        if not os.path.exists(path):
            pytest.skip("no build log: the library was not built by csrc/Makefile in this tree")
        text = open(path).read()
        assert "-Winline-asm" not in text and "reserved registers" not in text, obj

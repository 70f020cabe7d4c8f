#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same machine code? For refactors of the kernel headers that must not change
the product: compares, kernel by kernel, the instruction sequences of csrc/api_encoder.o, csrc/api_index.o and csrc/preprocess_vfirst.o and the
compiler's resource figures (csrc/*.resources.txt) of an OLD and a NEW build.

    usage: python tools/codeobj_diff.py OLD/csrc NEW/csrc      (both built by `make -C .../csrc`; no GPU needed)

Kernels are matched by demangled name through RENAMES (old -> new, for kernels whose template or argument lists changed);
the match must be a bijection over all kernels of an object. Padding behind a kernel's last instruction (zeros — a single zero dword included —, or s_nop behind
an s_endpgm / s_branch) is not part of it. Kernels of the OLD build whose demangled name matches a pattern of
REMOVED are reported as "removed, expected" and not counted (for a refactor that retires kernels). ONE normalisation: the 32-bit literal of the s_add_u32 behind
an s_getpc_b64 is a PC-relative distance to read-only data and moves when anything earlier in the code object changes size;
kernels that needed it are listed. For a kernel whose instructions differ, the opcodes whose counts differ follow
(before -> after): equal counts say the same instructions in another order or with other registers. Exit status 0 = identical."""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ZERO_DWORD = "v_cndmask_b32_e32 v0, s0, v0, vcc"   # what the disassembler prints for 0x00000000

# (pattern on the OLD demangled name, replacement): for a refactor that changes kernels' template or argument lists. Empty
# between such refactors: a stale rule maps kernels that kept their names onto names that do not exist.
RENAMES = []

# patterns (re.search on the OLD demangled name) of kernels a refactor retires on purpose. Empty between such refactors, like RENAMES.
REMOVED = []


def removed(name):
    return any(re.search(pat, name) for pat in REMOVED)


def rename(name):
    for pat, rep in RENAMES:
        name = re.sub(pat, rep, name)
    return name


def disassembly(csrc, obj):
    """({demangled kernel name: [instruction text, ...]}, {mangled name: demangled name}) of the gfx950 code object in csrc/obj.o"""
    with tempfile.TemporaryDirectory() as work:
        subprocess.check_call(["cp", os.path.join(csrc, obj + ".o"), work])
        subprocess.check_call([LLVM + "/llvm-objdump", "--offloading", obj + ".o"], cwd=work, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(work) if "gfx950" in f]
        assert len(co) == 1, os.listdir(work)
        text = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--demangle", co[0]], cwd=work, text=True)
        raw = subprocess.check_output([LLVM + "/llvm-objdump", "-d", co[0]], cwd=work, text=True)
    head = re.compile(r"^[0-9a-f]+ <(.+)>:$", re.M)
    names = dict(zip(head.findall(raw), head.findall(text)))
    kernels, cur = {}, None
    for line in text.splitlines():
        m = head.match(line)
        if m:
            assert m.group(1) not in kernels, m.group(1)
            cur = kernels.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t") and line.strip() != "...":   # ("...": zero padding behind a kernel's end)
            cur.append(line.split("//")[0].strip())
    # alignment padding behind a kernel's end comes as s_nop as well, or as ONE zero dword (which decodes as ZERO_DWORD; only a longer
    # run of zeros prints as "..."): it moves with the kernel's place in the object
    for ins in kernels.values():
        n = len(ins)
        while n and (ins[n - 1].startswith("s_nop") or ins[n - 1] == ZERO_DWORD):
            n -= 1
        if n and ins[n - 1].split()[0] in ("s_endpgm", "s_branch"):
            del ins[n:]
    return kernels, names


def mask_pc_literals(ins):
    out, n = list(ins), 0
    for i, text in enumerate(ins):
        if text.startswith("s_getpc_b64"):
            for j in range(i + 1, min(i + 3, len(ins))):
                m = re.match(r"(s_add_u32 \S+ \S+ )0x[0-9a-f]+$", ins[j])
                if m:
                    out[j] = m.group(1) + "<pc-relative>"
                    n += 1
                    break
    return out, n


def opcode_count_differences(a, b):
    """'opcode before->after, ...' over the opcodes whose counts differ between instruction lists a and b"""
    ca, cb = (collections.Counter(text.split()[0] for text in ins if text) for ins in (a, b))
    return ", ".join(f"{op} {ca[op]}->{cb[op]}" for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op])


def resources(csrc, obj, names):
    """{demangled kernel name: {figure: value}} of the compiler's kernel-resource-usage remarks"""
    text = open(os.path.join(csrc, obj + ".resources.txt")).read()
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", text)[1:]:
        out[names[b.split()[0]]] = dict(re.findall(r"remark:\s+([A-Za-z][^:\n]*): (\S+) \[-Rpass", b))
    return out


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    bad = 0
    for obj in ("api_encoder", "api_index", "preprocess_vfirst"):
        (old, old_names), (new, new_names) = disassembly(old_dir, obj), disassembly(new_dir, obj)
        old_res, new_res = resources(old_dir, obj, old_names), resources(new_dir, obj, new_names)
        mapped = {}
        gone = sorted(k for k in old if removed(k) and rename(k) not in new)
        for k in old:
            if k in gone:
                continue
            assert rename(k) not in mapped, ("two old kernels map to one name", k)
            mapped[rename(k)] = k
        only_old = sorted(set(mapped) - set(new))
        only_new = sorted(set(new) - set(mapped))
        renamed = sorted(k for k in mapped if mapped[k] != k and k in new)
        masked, differ, res_differ = [], [], []
        for k in sorted(set(mapped) & set(new)):
            a, b = old[mapped[k]], new[k]
            if a != b:
                (ma, na), (mb, nb) = mask_pc_literals(a), mask_pc_literals(b)
                if ma == mb and na == nb:
                    masked.append(k)
                else:
                    differ.append(k)
            ra, rb = old_res.get(mapped[k]), new_res.get(k)
            if ra != rb or (ra is None) != (rb is None):
                res_differ.append((k, ra, rb))
        nres = sum(1 for k in new if k in new_res)
        print(f"{obj}: {len(old)} kernels before, {len(new)} after; {len(renamed)} matched under a new name; "
              f"{nres} with resource figures")
        for k in masked:
            print(f"  identical after masking PC-relative literals: {k}")
        for k in gone:
            print(f"  removed, expected: {k}")
        for k in only_old:
            print(f"  ONLY BEFORE: {mapped[k]}")
        for k in only_new:
            print(f"  ONLY AFTER: {k}")
        for k in differ:
            print(f"  INSTRUCTIONS DIFFER: {k} ({len(old[mapped[k]])} vs {len(new[k])})")
            print(f"    opcode counts: {opcode_count_differences(old[mapped[k]], new[k]) or 'equal'}")
        for k, ra, rb in res_differ:
            print(f"  RESOURCES DIFFER: {k}: {ra} vs {rb}")
        bad += len(only_old) + len(only_new) + len(differ) + len(res_differ)
    print("identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

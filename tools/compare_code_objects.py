#!/usr/bin/env python3
"""Compares the kernels of two gfx950 code objects: names, resource use (.vgpr_count, .sgpr_count, .vgpr_spill_count,
.group_segment_fixed_size, .private_segment_fixed_size from the AMDGPU metadata note) and the disassembly of every kernel,
symbol by symbol (the order in which a compiler emits them may differ).  Prints one line per differing name and the totals;
exit status 1 when anything differs.  Several B files stand for one translation unit split into these: every name must be in
exactly one of them.  The `s_nop 0` padding behind a symbol's last instruction (alignment in front of the
next symbol, the fill at the end of .text) is not compared: it depends on what stands behind a kernel in its unit.

usage: python tools/compare_code_objects.py A.co B.co [B2.co ...]
A code object comes out of a device-only compile in two steps:
    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -c search.hip -o search.dev.o
    clang-offload-bundler --unbundle --type=o --targets=hip-amdgcn-amd-amdhsa--gfx950 --input=search.dev.o --output=A.co
(a file that is still a bundle is unbundled here)."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(path, tmp):
    with open(path, "rb") as f:
        if f.read(24) != b"__CLANG_OFFLOAD_BUNDLE__":
            return path
    out = os.path.join(tmp, os.path.basename(path) + ".co")
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950",
        "--input=" + path, "--output=" + out)
    return out


def kernels(path):
    """{kernel name: {field: value}} from the metadata note"""
    res, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", path).splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.groups()
        if line.lstrip().startswith("- ") and line.startswith("  - "):  # a new entry of amdhsa.kernels
            cur = {}
        if cur is None:
            continue
        if key == ".name":
            res[val.strip("'\"")] = cur
        elif key in FIELDS:
            cur[key] = val
    return res


def disassembly(path):
    """{symbol: [instruction text]} -- addresses and encodings dropped, branch targets kept relative to their symbol"""
    res, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", path).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            cur = res.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":  # ("...": the zero padding behind a symbol)
            cur.append(re.sub(r"\s*//.*$", "", line.strip()))
    # s_nop 0 behind a symbol's last instruction is padding: alignment in front of the next symbol, or the fill at the end of
    # .text; which of the two a kernel gets, and how much, depends on what stands behind it in the unit, not on the kernel
    for insns in res.values():
        while insns and insns[-1] == "s_nop 0":
            insns.pop()
    return res


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        a = code_object(sys.argv[1], tmp)
        ka, da = kernels(a), disassembly(a)
        kb, db = {}, {}
        for p in sys.argv[2:]:
            b = code_object(p, tmp)
            kp, dp = kernels(b), disassembly(b)
            for name in sorted((set(kp) & set(kb)) | (set(dp) & set(db))):
                print(f"in more than one B: {name}")
                differ += 1
            kb.update(kp)
            db.update(dp)
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print(f"only in {'A' if name in ka else 'B'}: {name}")
        elif ka[name] != kb[name]:
            print(f"resources differ: {name}: {ka[name]} != {kb[name]}")
        elif da.get(name) is None or da.get(name) != db.get(name):
            print(f"disassembly differs: {name}")
        else:
            continue
        differ += 1
    for name in sorted((set(da) | set(db)) - set(ka) - set(kb)):  # device functions that were not inlined
        if da.get(name) != db.get(name):
            print(f"disassembly differs (not a kernel): {name}")
            differ += 1
    print(f"A: {len(ka)} kernels, B: {len(kb)} kernels, {differ} differing names")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Compare the gfx950 code of two builds kernel by kernel: registers, LDS and
scratch from the code object's metadata and the instruction count per mnemonic
from its disassembly (tools/disasm.sh).  No GPU needed.

  python tools/isa_table.py A/csrc B/csrc PATTERN file.o [file.o ...]

A and B are the directories holding the two builds' object files; PATTERN is a
regular expression over the demangled kernel names.  One row per kernel: "equal"
when metadata and every mnemonic count agree, else both sides and the mnemonics
that differ."""
from __future__ import annotations

import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
HERE = os.path.dirname(os.path.abspath(__file__))
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def code_object(obj, tmp):
    fb, co = os.path.join(tmp, "fb"), os.path.join(tmp, "co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(tmp, "dummy.o")],
                   check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fb}", f"--output={co}", "--unbundle"], check=True)
    return co


def kernels(obj):
    """{mangled name: (metadata tuple, Counter of mnemonics)}"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        notes = subprocess.run([f"{LLVM}/llvm-readobj", "--notes", co], check=True, capture_output=True, text=True).stdout
        dis = os.path.join(tmp, "dis")
        subprocess.run(["bash", os.path.join(HERE, "disasm.sh"), obj, dis], check=True)
        text = open(dis).read()
    meta = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = tuple(int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in META)
    out = {}
    for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^\S|\Z)", text, re.M | re.S):
        if m.group(1) in meta:
            # (a mnemonic starts the line; objdump's continuation lines of a long encoding do not)
            ops = collections.Counter(line.split()[0] for line in m.group(2).splitlines()
                                      if re.match(r"\t[a-z][a-z0-9_]*(\s|$)", line))
            out[m.group(1)] = (meta[m.group(1)], ops)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def main():
    a_dir, b_dir, pattern, objs = sys.argv[1], sys.argv[2], re.compile(sys.argv[3]), sys.argv[4:]
    print("# VGPRs / SGPRs / LDS bytes / scratch bytes, instructions; A = %s, B = %s" % (a_dir, b_dir))
    same = total = 0
    for o in objs:
        ka, kb = kernels(os.path.join(a_dir, o)), kernels(os.path.join(b_dir, o))
        names = demangle(sorted(set(ka) | set(kb)))
        for k, nice in sorted(names.items(), key=lambda kv: kv[1]):
            short = re.sub(r"^void sgm::(\(anonymous namespace\)::)?", "", nice).split("(")[0]
            if not pattern.search(short):
                continue
            total += 1
            if k not in ka or k not in kb:
                print(f"{o}: {short}: only in {'A' if k in ka else 'B'}")
                continue
            (ma, ca), (mb, cb) = ka[k], kb[k]
            fmt = lambda m, c: "%d/%d/%d/%d, %d" % (*m, sum(c.values()))
            if ma == mb and ca == cb:
                same += 1
                print(f"{o}: {short}: equal ({fmt(ma, ca)})")
            else:
                diff = " ".join(f"{op}:{ca[op]}->{cb[op]}" for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op])
                print(f"{o}: {short}: A {fmt(ma, ca)} | B {fmt(mb, cb)} | {diff or 'same counts'}")
    print(f"# {same} of {total} kernels equal")


if __name__ == "__main__":
    main()

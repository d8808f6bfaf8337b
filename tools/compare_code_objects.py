#!/usr/bin/env python3
"""Have the kernels of two builds of libhsw.so compiled to the same code?  Extracts every gfx950 code object from
both libraries (the clang offload bundles inside the fat binary), disassembles each with `llvm-objdump -d` and
compares the two builds symbol by symbol (instruction text with addresses and encodings, comments stripped).
Prints one line per kernel family and status, then every symbol that differs or exists on one side only.

usage: compare_code_objects.py <parent libhsw.so> <new libhsw.so> [--objdump=/opt/rocm/llvm/bin/llvm-objdump]
e.g.   git worktree add ../parent HEAD~1 && make -C ../parent/halo2-dynamic-sha256_amd/csrc -j8 && make -C halo2-dynamic-sha256_amd/csrc -j8
       python tools/compare_code_objects.py ../parent/halo2-dynamic-sha256_amd/libhsw.so halo2-dynamic-sha256_amd/libhsw.so
Exit status 0; the caller decides which families may differ."""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path):
    blob = open(path, "rb").read()
    out = []
    for m in re.finditer(MAGIC, blob):
        at = m.start()
        n = struct.unpack_from("<Q", blob, at + 24)[0]
        off = at + 32
        for _ in range(n):
            o, size, tl = struct.unpack_from("<QQQ", blob, off)
            off += 24
            triple = blob[off:off + tl].decode()
            off += tl
            if "gfx950" in triple and size:
                out.append(blob[at + o:at + o + size])
    return out


def symbols(path, objdump):
    syms = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, elf in enumerate(code_objects(path)):
            f = os.path.join(tmp, "co_%03d.elf" % i)
            open(f, "wb").write(elf)
            text = subprocess.run([objdump, "-d", f], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = m.group(1)
                    syms.setdefault(cur, [])
                elif cur and line.strip():
                    syms[cur].append(re.sub(r"\s*//.*$", "", line.rstrip()))
    return syms


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    objdump = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--objdump=")), "/opt/rocm/llvm/bin/llvm-objdump")
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = symbols(args[0], objdump), symbols(args[1], objdump)
    names = sorted(set(a) | set(b))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    dem = dict(zip(names, dem))
    count, other = collections.Counter(), []
    for k in names:
        status = "only-one-side" if (k not in a or k not in b) else "same" if a[k] == b[k] else "DIFFERENT"
        count[(status, re.sub(r"[<(].*", "", re.sub(r"^void ", "", dem[k])))] += 1
        if status != "same":
            other.append("%s  %s  (%d / %d lines)" % (status, dem[k], len(a.get(k, [])), len(b.get(k, []))))
    for (status, family), c in sorted(count.items()):
        print("%-14s %-40s %d" % (status, family, c))
    print("\n".join(other))


if __name__ == "__main__":
    main()

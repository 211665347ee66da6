#!/usr/bin/env python3
"""sha256 of every kernel's machine code in the gfx950 code object of one or two builds of libbore_hip.so.  CPU only.

With two libraries: which kernels both hold with the same bytes, which differ, which only one holds -- how
profiles/restart_helper/codeobj_identity.txt was made (a change that adds kernels moves every other one in the code
object, so the object's own hash says nothing; a kernel's bytes hold no absolute address, but a kernel that names a
__device__ variable holds its distance to it).

  python tools/codeobj_kernels.py A.so [B.so]
"""
import hashlib
import os
import subprocess
import sys
import tempfile

BIN = "/opt/rocm/llvm/bin"


def tool(name):
    p = os.path.join(BIN, name)
    return p if os.path.exists(p) else name


def kernels(lib):
    """{kernel symbol: sha256 of its bytes} of the gfx950 code object bundled in `lib`."""
    with tempfile.TemporaryDirectory() as tmp:
        fb, co = os.path.join(tmp, "fb.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", lib, os.path.join(tmp, "copy.so")], check=True)
        subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fb}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        data = open(co, "rb").read()
        sections = subprocess.run([tool("llvm-readelf"), "-S", "--wide", co], capture_output=True, text=True, check=True).stdout
        text = None
        for line in sections.splitlines():
            parts = line.replace("[", " ").replace("]", " ").split()
            if len(parts) > 5 and parts[1] == ".text":
                text = (int(parts[3], 16), int(parts[4], 16))   # address, file offset
        symbols = subprocess.run([tool("llvm-readelf"), "-s", "--wide", co], capture_output=True, text=True, check=True).stdout
        out = {}
        for line in symbols.splitlines():
            parts = line.split()
            if len(parts) == 8 and parts[3] == "FUNC" and parts[4] == "GLOBAL":
                addr, size, name = int(parts[1], 16), int(parts[2]), parts[7]
                off = addr - text[0] + text[1]
                out[name] = (hashlib.sha256(data[off:off + size]).hexdigest(), size)
        return out


def main():
    a = kernels(sys.argv[1])
    if len(sys.argv) < 3:
        for name in sorted(a):
            print(a[name][0][:16], a[name][1], name)
        return
    b = kernels(sys.argv[2])
    # (a template that gained a trailing `bool = false` parameter: B's `...Lb0EE...` is A's kernel of the name without it)
    for n in sorted(set(b) - set(a)):
        old = n.replace("Lb0EEv", "Ev", 1)
        if old != n and old in a and old not in b:
            print("RENAMED", old, "->", n)
            b[old] = b.pop(n)
    same =sorted(n for n in a if n in b and a[n] == b[n])
    differ = sorted(n for n in a if n in b and a[n] != b[n])
    print(f"kernels: {len(a)} in A, {len(b)} in B; same bytes {len(same)}, different {len(differ)}, "
          f"only in A {len(set(a) - set(b))}, only in B {len(set(b) - set(a))}")
    for n in differ:
        print("DIFFERENT", n, a[n][1], b[n][1])
    for n in sorted(set(a) - set(b)):
        print("ONLY IN A", n)
    for n in sorted(set(b) - set(a)):
        print("ONLY IN B", n, b[n][1])


if __name__ == "__main__":
    main()

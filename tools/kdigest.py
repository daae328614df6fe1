#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 code object inside a HIP object file / .so:

    tools/kdigest.py gwen_amd/build/layer.o [more files] > listing.tsv

Per file a `# <file name>: <n> kernels` line, then one line a kernel, sorted: <demangled name, without its parameter
list and namespace> TAB <code size> TAB <SHA-256 of the symbol's bytes in .text>.
Two builds whose listings are equal run the same device code, kernel for kernel -- the check for a change that is
meant to touch host code only (profiles/launcher_kernel_digests.tsv).  Same unbundling steps as tools/kres.sh; sizes
and hashes only, no instruction is looked at.
"""
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE).stdout.decode()


def kernels(path):
    """[(demangled name, size, sha256)] of the kernels of `path`'s gfx950 code object."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        _run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", path)
        _run(f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}",
             "--unbundle")
        sections = {}                                        # name -> (index, address, file offset)
        for line in _run(f"{LLVM}/llvm-readelf", "-S", "-W", co).splitlines():
            f = line.replace("[", " ").replace("]", " ").split()
            if len(f) >= 6 and f[0].isdigit() and f[1].startswith("."):
                sections[f[1]] = (int(f[0]), int(f[3], 16), int(f[4], 16))
        tidx, taddr, toff = sections[".text"]
        # a kernel is a function symbol of .text with a kernel descriptor NAME.kd beside it
        syms = [l.split() for l in _run(f"{LLVM}/llvm-readelf", "-s", "-W", co).splitlines()]
        syms = [f for f in syms if len(f) == 8 and f[0].rstrip(":").isdigit()]
        descriptors = {f[7][:-3] for f in syms if f[7].endswith(".kd")}
        found = sorted({(f[7], int(f[1], 16), int(f[2], 0)) for f in syms              # a set: .dynsym repeats .symtab
                        if f[3] == "FUNC" and f[6] == str(tidx) and f[7] in descriptors})
        names = subprocess.run(["c++filt", "--no-params"], check=True, input="\n".join(n for n, _, _ in found).encode(),
                               stdout=subprocess.PIPE).stdout.decode().splitlines()
        out = []
        with open(co, "rb") as fh:
            for (_, addr, size), name in zip(found, names):
                fh.seek(toff + addr - taddr)
                out.append((name.replace("(anonymous namespace)::", ""), size, hashlib.sha256(fh.read(size)).hexdigest()))
        return sorted(out)


def main(paths):
    for p in paths:
        found = kernels(p)
        print(f"# {os.path.basename(p)}: {len(found)} kernels")
        for name, size, sha in found:
            print(f"{name}\t{size}\t{sha}")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1:])

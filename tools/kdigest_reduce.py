#!/usr/bin/env python3
"""Reduce two tools/kdigest.py listings -- a parent build's and a change's -- to a file small enough to commit:

    tools/kdigest.py PARENT/layer.o PARENT/chain.o > parent.tsv
    tools/kdigest.py gwen_amd/build/layer.o gwen_amd/build/chain.o > change.tsv
    tools/kdigest_reduce.py parent.tsv change.tsv [kernel-name regex ...] > profiles/packw_kernel_digests.tsv

Per object: the number of kernels and the SHA-256 of its sorted listing lines '<name>\\t<size>\\t<sha256>'.  For the change
the digest is taken over the kernels whose packed-W flag is off (k_layer: last template argument; k_chain: the one before
the images), their names written without that argument -- so equal digests say that every kernel of the parent is in the
change byte for byte, and the script fails when they are not.  Then the listing lines of the kernels whose names match one
of the regular expressions, both trees.

    tools/kdigest_reduce.py --store parent.tsv change.tsv [regex ...] > profiles/store_kernel_digests.tsv

The same for the store mode (k_layer, k_gather: last template argument; k_chain: the one before the images): "off" is
ST = 1, whose kernels must be the parent's byte for byte; the column headers keep their names."""
import hashlib
import re
import sys


def load(path):
    out, obj = {}, None
    for line in open(path):
        if line.startswith("#"):
            obj = line[2:].split(":")[0]
            continue
        name, size, sha = line.rstrip("\n").split("\t")
        out[(obj, name)] = (size, sha)
    return out


STORE = False                          # --store: the flag is the store mode, off = 1


def flag_off_name(name):
    if STORE:
        m = re.match(r"(k_layer<.*|k_gather<.*), 1>$", name)
        if m:
            return m.group(1) + ">"
        m = re.match(r"(k_chain<.*), 1, (\d+)>$", name)
        return m.group(1) + ", " + m.group(2) + ">" if m else name
    m = re.match(r"(k_layer<.*), false>$", name)
    if m:
        return m.group(1) + ">"
    m = re.match(r"(k_chain<.*), false, (\d+)>$", name)
    return m.group(1) + ", " + m.group(2) + ">" if m else name


def packed(name):
    if STORE:
        return bool(re.search(r"(k_layer<.*|k_gather<.*), [2-4]>$|k_chain<.*, [2-4], \d+>$", name))
    return bool(re.search(r"k_layer<.*, true>$|k_chain<.*, true, \d+>$", name))


def main(parent_path, change_path, patterns):
    parent, change = load(parent_path), load(change_path)
    print("tree\tobject\tkernels\tkernels_pk_off\tkernels_pk_on\tsha256_of_listing_pk_off")
    for obj in sorted({o for o, _ in parent}, reverse=True):
        pa = sorted(f"{n}\t{s}\t{h}" for (o, n), (s, h) in parent.items() if o == obj)
        ch = sorted(f"{flag_off_name(n)}\t{s}\t{h}" for (o, n), (s, h) in change.items() if o == obj and not packed(n))
        on = sum(1 for (o, n) in change if o == obj and packed(n))
        ha, hb = (hashlib.sha256("\n".join(v).encode()).hexdigest() for v in (pa, ch))
        print(f"parent\t{obj}\t{len(pa)}\t{len(pa)}\t0\t{ha}")
        print(f"change\t{obj}\t{len(ch) + on}\t{len(ch)}\t{on}\t{hb}")
        if pa != ch:
            sys.exit(f"{obj}: the flag-off kernels of the change are not the parent's")
    print("tree\tobject\tkernel\tsize\tsha256")
    for tree, d in (("parent", parent), ("change", change)):
        for (o, n), (s, h) in sorted(d.items()):
            if any(re.match(p, n) for p in patterns):
                print(f"{tree}\t{o}\t{n}\t{s}\t{h}")


if __name__ == "__main__":
    if "--store" in sys.argv:
        STORE = True
        sys.argv.remove("--store")
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2], sys.argv[3:])

#!/usr/bin/env python3
"""Compare the device code of two builds, kernel by kernel.

    make -C gr-doa_amd asm ASM=/tmp/a          (on one tree)
    make -C gr-doa_amd asm ASM=/tmp/b          (on the other)
    python tools/compare_device_code.py /tmp/a /tmp/b

Each directory holds one device-only assembly file per translation unit (the Makefile's `asm` target).  A file is cut at its
function symbols (the compiler's "-- Begin function NAME" lines); a function with an .amdhsa_kernel descriptor is a kernel, and
its piece holds the instructions and the descriptor block (register counts, LDS, scratch).  Pieces are compared as text, under
the key "unit:NAME"; what a file holds outside its functions (the head and the metadata notes at the end) is compared as the
piece "unit:(file scope)".  Prints the number of kernels on each side, the names present on one side only and the names that
differ; exit status 0 only if both lists are empty.
"""
import re
import sys
from pathlib import Path

BEGIN = re.compile(r"^\s*\.\w+\s+(\S+)\s*;\s*-- Begin function \1\s*$")
TAIL = re.compile(r"^\s*\.(amdgpu_metadata|amdgcn_target)\b|^\s*\.section\s+\.(AMDGPU\.gpr_maximums|note|debug)")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$", re.M)


def pieces(path):
    """{name: text} of one assembly file, and the set of names that are kernels."""
    out, name, buf, scope = {}, None, [], []
    for line in path.read_text().splitlines(keepends=True):
        m = BEGIN.match(line)
        if m or (name is not None and TAIL.match(line)):
            if name is not None:
                out[name] = "".join(buf)
            name, buf = (m.group(1), []) if m else (None, [])
        (buf if name is not None else scope).append(line)
    if name is not None:
        out[name] = "".join(buf)
    kernels = {n for n, text in out.items() if KERNEL.search(text)}
    out["(file scope)"] = "".join(scope)
    return out, kernels


def load(directory):
    code, kernels = {}, set()
    for path in sorted(Path(directory).glob("*.s")):
        p, k = pieces(path)
        code.update({f"{path.stem}:{n}": text for n, text in p.items()})
        kernels.update(f"{path.stem}:{n}" for n in k)
    return code, kernels


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    (a, ka), (b, kb) = load(argv[1]), load(argv[2])
    if not a or not b:
        print("no *.s files in " + (argv[1] if not a else argv[2]), file=sys.stderr)
        return 2
    only = sorted(set(a) ^ set(b))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    print(f"kernels: {len(ka)} in {argv[1]}, {len(kb)} in {argv[2]}")
    print(f"on one side only: {len(only)}")
    for n in only:
        print(f"  {'A' if n in a else 'B'} only  {n}")
    print(f"differ: {len(differ)}")
    for n in differ:
        print(f"  {n}")
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

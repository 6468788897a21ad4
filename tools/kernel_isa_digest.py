#!/usr/bin/env python3
"""Per kernel of one csrc/ unit: the number of gfx950 instructions and a hash over them.

    python tools/kernel_isa_digest.py lidarcast.hip [-DLRC_VARIANTS] [--csrc DIR]

The unit is compiled device-only to assembly with the build's own flags (__graft_entry__.HIP_FLAGS), and for every kernel
symbol the instruction lines between its label and its .Lfunc_end are counted and hashed (SHA-256, first 16 hex digits), with
comments, directives and labels stripped.  Two trees whose lines agree compile a kernel to the same code; a refactor that must
not move a kernel shows that with a diff of two runs (--csrc points at the other tree's csrc/).  It hashes and nothing else.
One line per kernel, sorted by symbol: <instructions> <hash> <demangled name>."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as entry  # noqa: E402


def digest(source, defines=(), csrc=entry.CSRC):
    """{mangled kernel symbol: (instruction count, hash)} of csrc/<source>."""
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory(prefix="isa_digest_") as tmp:
        out = os.path.join(tmp, "t.s")
        subprocess.run([hipcc] + flags + list(defines) + ["--cuda-device-only", "-S", os.path.join(csrc, source), "-o", out],
                       check=True, cwd=csrc)
        with open(out) as fh:
            text = fh.read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M))
    res, name, lines = {}, None, []
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if name is None:
            if line.endswith(":") and line[:-1] in kernels:
                name, lines = line[:-1], []
            continue
        if line.startswith(".Lfunc_end"):
            res[name] = (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16])
            name = None
        elif line and not line.startswith(".") and not line.endswith(":"):
            # a branch target is .LBB<function number>_<block>: the function's place in the unit is not part of its code
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", line)))
    return res


def main(argv):
    csrc = entry.CSRC
    if "--csrc" in argv:
        i = argv.index("--csrc")
        csrc = os.path.abspath(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    if not argv or argv[0].startswith("-"):
        raise SystemExit(__doc__)
    source, defines = argv[0], argv[1:]
    res = digest(source, defines, csrc)
    try:      # readable names where binutils is there; the mangled ones otherwise
        pretty = subprocess.run(["c++filt"] + sorted(res), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        pretty = sorted(res)
    for sym, shown in zip(sorted(res), pretty):
        n, h = res[sym]
        print(f"{n:6d} {h} {shown.replace('(anonymous namespace)::', '')}")


if __name__ == "__main__":
    main(sys.argv[1:])

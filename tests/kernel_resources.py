"""What the compiler says a csrc/ unit's gfx950 kernels use: the unit compiled device-only with the build's own flags and
-Rpass-analysis=kernel-resource-usage, the remarks parsed per kernel.  A plain helper of the *resources* tests; a (unit, flags)
pair is compiled once per process, however many test files ask for it."""
import functools
import os
import re
import subprocess
import tempfile

from conftest import PKG

FIELDS = r"(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\])"


@functools.lru_cache(maxsize=None)
def _generators():
    """{name: value} of the ray generators, from their one table (csrc/lrc_gen.h)."""
    with open(os.path.join(PKG, "csrc", "lrc_gen.h")) as fh:
        found = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (kGen\w+) = (\d+);", fh.read())}
    assert found, "csrc/lrc_gen.h: no `constexpr int kGen... = n;` line found"
    return found


def trace_kernel_name(gen, qn, stats=False):
    """The mangled name of lidarcast.hip's trace_kernel<gen, 2, true, false, stats, qn>: ``gen`` is a generator's name in
    csrc/lrc_gen.h ("kGenPoses", ...); ``qn`` 1 = quantised nodes, 0 = float32 nodes."""
    assert gen in _generators(), f"{gen!r} is not a generator of csrc/lrc_gen.h: {sorted(_generators())}"
    return f"_ZN12_GLOBAL__N_112trace_kernelILi{_generators()[gen]}ELi2ELb1ELb0ELb{int(stats)}ELi{int(qn)}EEEvNS_11TraceParamsE"


@functools.lru_cache(maxsize=None)
def usage_of(source, drop_flags=("-shared",), asm=False):
    """{mangled kernel name: {"TotalSGPRs", "VGPRs", "ScratchSize", "Occupancy", "LDS": int}} of csrc/<source>, compiled with
    the build's flags less ``drop_flags``.  ``asm=True`` compiles to assembly text (-S) and returns (that dict, the text)."""
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f not in drop_flags]
    with tempfile.TemporaryDirectory(prefix="kernel_res_") as tmp:
        out = os.path.join(tmp, "t.s" if asm else "t.o")
        r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S" if asm else "-c", "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(PKG, "csrc", source), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        text = open(out).read() if asm else None
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
        if m and name:
            res[name][m.group(1).split()[0]] = int(m.group(2))
    return (res, text) if asm else res

"""CPU: the register budget of the product trace kernel, read from the compiler's kernel-resource-usage remarks as
test_pipe_lean_resources.py does.  It repeats that budget on purpose: the kernel's leading workgroups run the lean scatter
(scatter_tiles_xyzl_lean, now with streaming loads and stores) in the trace kernel's own registers, and every attempt to
give the tracing waves part of that work (profiles/pipe_fused_scatter.txt) moved this figure first."""
import os
import re
import subprocess

import pytest

from conftest import PKG

PRODUCT = "_ZN12_GLOBAL__N_112trace_kernelILi1ELi2ELb1ELb0ELb0ELi1EEEvNS_11TraceParamsE"   # <1, 2, true, false, false, 1>
FIELDS = r"(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\])"


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    out = tmp_path_factory.mktemp("fused_res") / "t.o"
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(PKG, "csrc", "lidarcast.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+" + FIELDS + r": (\d+)", line)
        if m and name:
            res[name].setdefault(m.group(1).split()[0], int(m.group(2)))     # the first block of a kernel: its own figures
    return res


def test_product_trace_kernel_budget(usage):
    u = usage[PRODUCT]
    assert u["VGPRs"] <= 64, u
    assert u["TotalSGPRs"] <= 80, u
    assert u["ScratchSize"] == 0, u
    assert u["Occupancy"] == 8, u

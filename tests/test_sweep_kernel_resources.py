"""CPU: the moving-sensor sweep instantiation of the trace kernel (GEN = 4, quantised nodes) keeps the budget of the
pose-batched scan it extends -- 64 VGPRs, at most 80 SGPRs, no scratch, 8 waves per SIMD -- read from the compiler's
kernel-resource-usage remarks as tests/test_trace_kernel_resources.py reads them."""
import os
import re
import subprocess

import pytest

from conftest import PKG

SWEEP_QUANTISED = "_ZN12_GLOBAL__N_112trace_kernelILi4ELi2ELb1ELb0ELb0ELi1EEEvNS_11TraceParamsE"   # <4, 2, true, false, false, 1>
SWEEP_FLOAT32 = "_ZN12_GLOBAL__N_112trace_kernelILi4ELi2ELb1ELb0ELb0ELi0EEEvNS_11TraceParamsE"     # <4, 2, true, false, false, 0>


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    out = tmp_path_factory.mktemp("sweep_res") / "t.o"
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
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split()[0]] = int(m.group(2))
    return res


def test_quantised_sweep_kernel_keeps_eight_waves(usage):
    u = usage[SWEEP_QUANTISED]
    assert u["VGPRs"] <= 64, u
    assert u["TotalSGPRs"] <= 80, u
    assert u["ScratchSize"] == 0, u
    assert u["Occupancy"] == 8, u


def test_float32_sweep_kernel_has_no_scratch(usage):
    u = usage[SWEEP_FLOAT32]
    assert u["VGPRs"] <= 64, u
    assert u["ScratchSize"] == 0, u

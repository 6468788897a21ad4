"""CPU: the seeded-noise instantiation of the trace kernel (GEN = 5, quantised nodes: Philox, the quantile table lookups and
the float64 row jitter in front of the traversal, the range draw behind it) keeps the budget of the pose-batched scan it
extends -- 64 VGPRs, at most 80 SGPRs, no scratch, 8 waves per SIMD -- read from the compiler's kernel-resource-usage remarks
as tests/test_sweep_kernel_resources.py reads them."""
import os
import re
import subprocess

import pytest

from conftest import PKG

NOISY_QUANTISED = "_ZN12_GLOBAL__N_112trace_kernelILi5ELi2ELb1ELb0ELb0ELi1EEEvNS_11TraceParamsE"   # <5, 2, true, false, false, 1>
NOISY_FLOAT32 = "_ZN12_GLOBAL__N_112trace_kernelILi5ELi2ELb1ELb0ELb0ELi0EEEvNS_11TraceParamsE"     # <5, 2, true, false, false, 0>


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    out = tmp_path_factory.mktemp("noise_res") / "t.o"
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


def test_quantised_noisy_kernel_keeps_eight_waves(usage):
    u = usage[NOISY_QUANTISED]
    assert u["VGPRs"] <= 64, u
    assert u["TotalSGPRs"] <= 80, u
    assert u["ScratchSize"] == 0, u
    assert u["Occupancy"] == 8, u


def test_float32_noisy_kernel_has_no_scratch(usage):
    u = usage[NOISY_FLOAT32]
    assert u["ScratchSize"] == 0, u

"""CPU: the beam instantiations of the trace kernel (GEN = 6: the float64 row offset in front of the traversal, the cross-lane
reduction to echoes and a second gen_ray behind it) use no scratch on either node route, and the quantised one keeps the
budget of the pose-batched scan it extends -- 64 VGPRs, 8 waves per SIMD -- read from the compiler's kernel-resource-usage
remarks as tests/test_noise_kernel_resources.py reads them.  The figures are printed (DESIGN.md section 5i records them)."""
import os
import re
import subprocess

import pytest

from conftest import PKG

ECHO_QUANTISED = "_ZN12_GLOBAL__N_112trace_kernelILi6ELi2ELb1ELb0ELb0ELi1EEEvNS_11TraceParamsE"   # <6, 2, true, false, false, 1>
ECHO_FLOAT32 = "_ZN12_GLOBAL__N_112trace_kernelILi6ELi2ELb1ELb0ELb0ELi0EEEvNS_11TraceParamsE"     # <6, 2, true, false, false, 0>


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    out = tmp_path_factory.mktemp("echo_res") / "t.o"
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
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res[name][m.group(1).split()[0]] = int(m.group(2))
    return res


def test_quantised_echo_kernel_keeps_eight_waves(usage):
    u = usage[ECHO_QUANTISED]
    print(f"\n[echo] trace_kernel<6, quantised nodes>: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["VGPRs"] <= 64, u
    assert u["Occupancy"] == 8, u
    assert u["LDS"] == 0, u            # no static LDS: the traversal stack is the launch's dynamic allocation, nothing beside it


def test_float32_echo_kernel_has_no_scratch(usage):
    u = usage[ECHO_FLOAT32]
    print(f"\n[echo] trace_kernel<6, float32 nodes>: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u

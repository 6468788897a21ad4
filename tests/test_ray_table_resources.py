"""CPU: the kernel that prepares the ray table of a fused pipeline submit (csrc/lidarcast.hip, ray_table_kernel), read from
the compiler's kernel-resource-usage remarks: no scratch.  The product trace kernel, which now carries the table's fast
path beside the per-ray set-up, is held to its budget by tests/test_trace_kernel_resources.py."""
import os
import re
import subprocess

import pytest

from conftest import PKG


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    out = tmp_path_factory.mktemp("ray_table_res") / "t.o"
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(PKG, "csrc", "lidarcast.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    res = {}
    name = None
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


def test_preparation_kernel_uses_no_scratch(usage):
    found = [u for n, u in usage.items() if "ray_table_kernel" in n]
    assert len(found) == 1, sorted(usage)
    assert found[0]["ScratchSize"] == 0, found[0]
    assert found[0]["Occupancy"] == 8, found[0]      # one-wave workgroups that fit beside the tracing waves

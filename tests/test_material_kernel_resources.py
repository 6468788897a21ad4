"""CPU: the material instantiations of the trace kernel (GEN = 7: a loop of segment steps and further traversals behind the
first one, the original ray formed again behind the loop) use no scratch and no static LDS on either node route -- read from
the compiler's kernel-resource-usage remarks as tests/test_echo_kernel_resources.py reads them.  VGPRs, SGPRs and occupancy are
printed, not fixed (DESIGN.md section 5j records them)."""
import os
import re
import subprocess

import pytest

from conftest import PKG

MATERIAL_QUANTISED = "_ZN12_GLOBAL__N_112trace_kernelILi7ELi2ELb1ELb0ELb0ELi1EEEvNS_11TraceParamsE"   # <7, 2, true, false, false, 1>
MATERIAL_FLOAT32 = "_ZN12_GLOBAL__N_112trace_kernelILi7ELi2ELb1ELb0ELb0ELi0EEEvNS_11TraceParamsE"     # <7, 2, true, false, false, 0>


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f != "-shared"]
    out = tmp_path_factory.mktemp("material_res") / "t.o"
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


@pytest.mark.parametrize("name, route", [(MATERIAL_QUANTISED, "quantised nodes"), (MATERIAL_FLOAT32, "float32 nodes")])
def test_material_kernel_has_no_scratch_and_no_static_lds(usage, name, route):
    assert name in usage, sorted(k for k in usage if "trace_kernel" in k)
    u = usage[name]
    print(f"\n[material] trace_kernel<7, {route}>: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u            # no static LDS: the traversal stack is the launch's dynamic allocation, nothing beside it

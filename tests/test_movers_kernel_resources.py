"""CPU: the two kernels of the moving objects (mover_rays_kernel: gen_ray, the ray in the mover's frame, the cull;
mover_merge_kernel: the running winner and, in the last pass, write_back with a given normal and triangle row) use no scratch
and no LDS -- read from the compiler's kernel-resource-usage remarks as tests/test_material_kernel_resources.py reads them.
VGPRs, SGPRs and occupancy are printed, not fixed (DESIGN.md section 5k records them)."""
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
    out = tmp_path_factory.mktemp("movers_res") / "t.o"
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


@pytest.mark.parametrize("kernel", ["mover_rays_kernel", "mover_merge_kernel"])
def test_mover_kernel_has_no_scratch_and_no_lds(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(k for k in usage if "mover" in k)
    u = usage[names[0]]
    print(f"\n[movers] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u

"""CPU: the per-frame object kernels (csrc/lrc_frameobj.hip) as compiled for gfx950 -- no scratch, at least seven waves per SIMD,
and the sensor-frame coordinate without any fused multiply-add (the bit-exactness of DESIGN.md section 5g rests on it):
read from the compiler's kernel-resource-usage remarks and from the accumulate kernel's ISA."""
import os
import re
import subprocess

import pytest

from conftest import PKG


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    import __graft_entry__ as entry
    hipcc = entry.HIPCC if os.path.exists(entry.HIPCC) else "hipcc"
    flags = [f for f in entry.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path_factory.mktemp("frameobj_res") / "t.s"
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(PKG, "csrc", "lrc_frameobj.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and name:
            res[name][m.group(1).split()[0]] = int(m.group(2))
    return res, out.read_text()


def _kernel(res, part):
    names = [n for n in res if part in n]
    assert len(names) == 1, (part, sorted(res))
    return names[0]


def test_kernels_have_no_scratch_and_seven_waves(compiled):
    res, _ = compiled
    for part in ("accumulate_kernel", "static_kernel", "export_kernel", "fill_boxes_kernel"):
        u = res[_kernel(res, part)]
        assert u["ScratchSize"] == 0, (part, u)
        # registers: 64 VGPRs allow eight waves per SIMD; the accumulate kernel's ~100 SGPRs (19 arguments and the twelve
        # pose scalars) cost it one of them
        assert u["Occupancy"] >= 7, (part, u)
    acc = res[_kernel(res, "accumulate_kernel")]
    assert acc["VGPRs"] <= 64, acc
    assert acc["LDS"] <= 9 * 1024, acc                      # the 128-row table; 160 KB per CU leave occupancy to the registers


def test_sensor_frame_arithmetic_is_not_contracted(compiled):
    res, asm = compiled
    name = _kernel(res, "accumulate_kernel")
    body = asm[asm.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    assert not re.search(r"v_fma(c|ak|mk)?_f64|v_pk_fma", body)
    assert re.search(r"\bv_mul_f64", body) and re.search(r"\bv_add_f64", body)      # the products and sums are there, apart

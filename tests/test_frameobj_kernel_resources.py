"""CPU: the per-frame object kernels (csrc/lrc_frameobj.hip) as compiled for gfx950 -- no scratch, at least seven waves per SIMD,
and the sensor-frame coordinate without any fused multiply-add (the bit-exactness of DESIGN.md section 5g rests on it):
read from the compiler's kernel-resource-usage remarks and from the accumulate kernel's ISA."""
import re

import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def compiled():
    return usage_of("lrc_frameobj.hip", ("-shared", "-fPIC"), asm=True)


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

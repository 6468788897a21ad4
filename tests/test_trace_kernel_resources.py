"""CPU: register and scratch budgets of the product trace kernels in csrc/lidarcast.hip, read from the compiler's
kernel-resource-usage remarks.  The quantised pose-batched kernel is sized for 8 waves per SIMD (its launch bound asks
for them): 64 VGPRs and at most 80 SGPRs -- 82..96 SGPRs admit only 7 waves although the remark still says 8."""
import pytest

from kernel_resources import trace_kernel_name, usage_of

QUANTISED = trace_kernel_name("kGenPoses", qn=1)
FLOAT32 = trace_kernel_name("kGenPoses", qn=0)


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


def test_quantised_trace_kernel_keeps_eight_waves(usage):
    u = usage[QUANTISED]
    assert u["VGPRs"] <= 64, u
    assert u["TotalSGPRs"] <= 80, u
    assert u["ScratchSize"] == 0, u
    assert u["Occupancy"] == 8, u


def test_float32_trace_kernel_registers_and_no_scratch(usage):
    # launch bound 1 (scenes without quantised images): not held to 8 waves, its SGPR count is not pinned
    u = usage[FLOAT32]
    assert u["VGPRs"] <= 64, u
    assert u["ScratchSize"] == 0, u

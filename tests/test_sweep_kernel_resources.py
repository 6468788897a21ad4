"""CPU: the moving-sensor sweep instantiation of the trace kernel (GEN = 4, quantised nodes) keeps the budget of the
pose-batched scan it extends -- 64 VGPRs, at most 80 SGPRs, no scratch, 8 waves per SIMD -- read from the compiler's
kernel-resource-usage remarks as tests/test_trace_kernel_resources.py reads them."""
import pytest

from kernel_resources import trace_kernel_name, usage_of

SWEEP_QUANTISED = trace_kernel_name("kGenSweeps", qn=1)
SWEEP_FLOAT32 = trace_kernel_name("kGenSweeps", qn=0)


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


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

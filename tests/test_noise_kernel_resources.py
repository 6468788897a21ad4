"""CPU: the seeded-noise instantiation of the trace kernel (GEN = 5, quantised nodes: Philox, the quantile table lookups and
the float64 row jitter in front of the traversal, the range draw behind it) keeps the budget of the pose-batched scan it
extends -- 64 VGPRs, at most 80 SGPRs, no scratch, 8 waves per SIMD -- read from the compiler's kernel-resource-usage remarks
as tests/test_sweep_kernel_resources.py reads them."""
import pytest

from kernel_resources import trace_kernel_name, usage_of

NOISY_QUANTISED = trace_kernel_name("kGenNoisy", qn=1)
NOISY_FLOAT32 = trace_kernel_name("kGenNoisy", qn=0)


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


def test_quantised_noisy_kernel_keeps_eight_waves(usage):
    u = usage[NOISY_QUANTISED]
    assert u["VGPRs"] <= 64, u
    assert u["TotalSGPRs"] <= 80, u
    assert u["ScratchSize"] == 0, u
    assert u["Occupancy"] == 8, u


def test_float32_noisy_kernel_has_no_scratch(usage):
    u = usage[NOISY_FLOAT32]
    assert u["ScratchSize"] == 0, u

"""CPU: the noisy-sweep instantiation of the trace kernel (GEN = 8: Philox, the quantile table lookups and the float64 row jitter
in front of the dgemm chain, the sweep rotation behind it, the centre and the range draw formed again behind the traversal) keeps
the budget of the two kernels it joins (GEN = 4 and GEN = 5) -- at most 64 VGPRs and 80 SGPRs, no scratch, 8 waves per SIMD over
quantised nodes; at most 64 VGPRs and no scratch over float32 nodes -- read from the compiler's kernel-resource-usage remarks as
tests/test_sweep_kernel_resources.py reads them."""
import pytest

from kernel_resources import trace_kernel_name, usage_of

NOISY_SWEEP_QUANTISED = trace_kernel_name("kGenNoisySweeps", qn=1)
NOISY_SWEEP_FLOAT32 = trace_kernel_name("kGenNoisySweeps", qn=0)


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


def test_quantised_noisy_sweep_kernel_keeps_eight_waves(usage):
    u = usage[NOISY_SWEEP_QUANTISED]
    assert u["VGPRs"] <= 64, u
    assert u["TotalSGPRs"] <= 80, u
    assert u["ScratchSize"] == 0, u
    assert u["Occupancy"] == 8, u


def test_float32_noisy_sweep_kernel_has_no_scratch(usage):
    u = usage[NOISY_SWEEP_FLOAT32]
    assert u["VGPRs"] <= 64, u
    assert u["ScratchSize"] == 0, u

"""CPU: the beam instantiations of the trace kernel (GEN = 6: the float64 row offset in front of the traversal, the cross-lane
reduction to echoes and a second gen_ray behind it) use no scratch on either node route, and the quantised one keeps the
budget of the pose-batched scan it extends -- 64 VGPRs, 8 waves per SIMD -- read from the compiler's kernel-resource-usage
remarks as tests/test_noise_kernel_resources.py reads them.  The figures are printed (DESIGN.md section 5i records them)."""
import pytest

from kernel_resources import trace_kernel_name, usage_of

ECHO_QUANTISED = trace_kernel_name("kGenEchoes", qn=1)
ECHO_FLOAT32 = trace_kernel_name("kGenEchoes", qn=0)


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


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

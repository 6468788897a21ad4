"""CPU: the register budget of the product trace kernel, read from the compiler's kernel-resource-usage remarks as
test_pipe_lean_resources.py does.  It repeats that budget on purpose: the kernel's leading workgroups run the lean scatter
(scatter_tiles_xyzl_lean, now with streaming loads and stores) in the trace kernel's own registers, and every attempt to
give the tracing waves part of that work (profiles/pipe_fused_scatter.txt) moved this figure first."""
import pytest

from kernel_resources import trace_kernel_name, usage_of

PRODUCT = trace_kernel_name("kGenPoses", qn=1)


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


def test_product_trace_kernel_budget(usage):
    u = usage[PRODUCT]
    assert u["VGPRs"] <= 64, u
    assert u["TotalSGPRs"] <= 80, u
    assert u["ScratchSize"] == 0, u
    assert u["Occupancy"] == 8, u

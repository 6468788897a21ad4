"""CPU: the kernels that form output rows from the 12-byte records of the scan pipeline's lean sets, read from the compiler's
kernel-resource-usage remarks -- the plain-form scatter (compact_scatter_lean_kernel) and the expansion behind lrc_pipe_records
(expand_lean_kernel) use no scratch, and the product trace kernel, whose leading workgroups now load records, table rows and
pose records and whose write-back stores the record, still fits 64 VGPRs, 80 SGPRs and 8 waves per SIMD with no scratch."""
import pytest

from kernel_resources import trace_kernel_name, usage_of

QUANTISED = trace_kernel_name("kGenPoses", qn=1)


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


@pytest.mark.parametrize("kernel", ["compact_scatter_lean_kernel", "expand_lean_kernel"])
def test_record_consumers_use_no_scratch(usage, kernel):
    found = [u for n, u in usage.items() if kernel in n]
    assert len(found) == 1, sorted(usage)
    assert found[0]["ScratchSize"] == 0, found[0]


def test_product_trace_kernel_budget_with_record_paths(usage):
    u = usage[QUANTISED]
    assert u["VGPRs"] <= 64, u
    assert u["TotalSGPRs"] <= 80, u
    assert u["ScratchSize"] == 0, u
    assert u["Occupancy"] == 8, u

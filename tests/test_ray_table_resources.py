"""CPU: the kernel that prepares the ray table of a fused pipeline submit (csrc/lidarcast.hip, ray_table_kernel), read from
the compiler's kernel-resource-usage remarks: no scratch.  The product trace kernel, which now carries the table's fast
path beside the per-ray set-up, is held to its budget by tests/test_trace_kernel_resources.py."""
import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


def test_preparation_kernel_uses_no_scratch(usage):
    found = [u for n, u in usage.items() if "ray_table_kernel" in n]
    assert len(found) == 1, sorted(usage)
    assert found[0]["ScratchSize"] == 0, found[0]
    assert found[0]["Occupancy"] == 8, found[0]      # one-wave workgroups that fit beside the tracing waves

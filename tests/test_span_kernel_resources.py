"""CPU: the two kernels of the animated movers under sweeps (k_span_slots: the span box and the gathered vertex record of a leaf
slot; span_trace_kernel: the per-ray-shape traversal with its stack in LDS) are found exactly once each and use no scratch -- read
from the compiler's kernel-resource-usage remarks as tests/test_deform_kernel_resources.py reads them.  VGPRs, SGPRs, LDS and
occupancy are printed, not fixed (DESIGN.md section 5s records them)."""
import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def usage():
    return usage_of("lrc_span.hip")


@pytest.mark.parametrize("kernel", ["k_span_slots", "span_trace_kernel"])
def test_span_kernel_has_no_scratch(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(usage)
    u = usage[names[0]]
    print(f"\n[span] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u


def test_the_traversal_stack_is_the_only_lds(usage):
    """[depth][lane] int32: 32 x 64 x 4 bytes; the slot kernel has none"""
    trace = usage[next(k for k in usage if "span_trace_kernel" in k)]
    slots = usage[next(k for k in usage if "k_span_slots" in k)]
    assert trace["LDS"] == 32 * 64 * 4, trace
    assert slots["LDS"] == 0, slots

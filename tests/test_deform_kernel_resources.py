"""CPU: the kernels of the deforming movers (csrc/lrc_deform.hip: k_blend, k_slots, k_level, k_tail) use no scratch, and the
blend and slot kernels no LDS -- read from the compiler's kernel-resource-usage remarks as
tests/test_movers_kernel_resources.py reads them.  VGPRs, SGPRs and occupancy are printed, not fixed (DESIGN.md section 5o
records them)."""
import pytest

from kernel_resources import usage_of

KERNELS = ["k_blend", "k_slots", "k_level", "k_tail"]


@pytest.fixture(scope="module")
def usage():
    return usage_of("lrc_deform.hip")


def test_the_unit_holds_exactly_these_kernels(usage):
    assert len(usage) == len(KERNELS), sorted(usage)


@pytest.mark.parametrize("kernel", KERNELS)
def test_deform_kernel_has_no_scratch(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(usage)
    u = usage[names[0]]
    print(f"\n[deform] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u
    if kernel in ("k_blend", "k_slots"):
        assert u["LDS"] == 0, u

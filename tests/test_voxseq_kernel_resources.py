"""CPU: the walk kernel of dynamic occupancy (csrc/lrc_voxseq.hip: seq_walk_kernel, one thread per ray, the walk of
csrc/lrc_voxwalk.h into the ray's frame slot) is found exactly once and uses no scratch -- read from the compiler's
kernel-resource-usage remarks as tests/test_mover_noise_kernel_resources.py reads them.  So do the kernels of its finalize.  VGPRs,
SGPRs and occupancy are printed, not fixed (DESIGN.md section 5u records them)."""
import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def usage():
    return usage_of("lrc_voxseq.hip")


def test_walk_kernel_is_found_once_and_has_no_scratch(usage):
    names = [k for k in usage if "seq_walk_kernel" in k]
    assert len(names) == 1, sorted(usage)
    u = usage[names[0]]
    print(f"\n[voxseq] seq_walk_kernel: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u


@pytest.mark.parametrize("kernel", ["seq_head_kernel", "seq_dense_kernel", "seq_label_vote_kernel", "seq_tail_kernel",
                                    "seq_mover_vote_kernel", "seq_counts_kernel"])
def test_finalize_kernels_have_no_scratch(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(usage)
    u = usage[names[0]]
    print(f"\n[voxseq] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u

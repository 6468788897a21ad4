"""CPU: the ray kernel of the non-rigid scene flow (nonrigid_target_kernel: the pair lookup among the kernel arguments, the
per-lane fetch of three indices and six vertices, the barycentric blend in float64, then the line of sight of flow_rays_kernel)
uses no scratch and no LDS, and its registers and occupancy are what DESIGN.md section 5p records -- read from the compiler's
kernel-resource-usage remarks for gfx950 as tests/test_flow_kernel_resources.py reads them.  A compiler that allocates
differently fails the pinned figures, not the kernel: then the figures here and in DESIGN.md are measured again."""
import pytest

from kernel_resources import usage_of

PINNED = {"nonrigid_target_kernel": {"VGPRs": 106, "TotalSGPRs": 49, "Occupancy": 4}}


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


def test_nonrigid_kernel_resources(usage):
    names = [k for k in usage if "nonrigid_target_kernel" in k]
    assert len(names) == 1, sorted(k for k in usage if "flow" in k or "nonrigid" in k)
    u = usage[names[0]]
    print(f"\n[nonrigid] nonrigid_target_kernel: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u
    assert {k: u[k] for k in PINNED["nonrigid_target_kernel"]} == PINNED["nonrigid_target_kernel"], u


def test_no_kernel_name_collides_with_the_flow_kernels(usage):
    """The flow resource tests find their kernels by substring: each name must still match exactly one kernel."""
    for name in ("flow_rays_kernel", "flow_object_rays_kernel", "flow_merge_kernel"):
        assert len([k for k in usage if name in k]) == 1, name

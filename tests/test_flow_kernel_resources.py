"""CPU: the three kernels of the scene flow (flow_rays_kernel: the target in float64, the line of sight, the range test;
flow_object_rays_kernel: the ray in a mover's next frame, the cull; flow_merge_kernel: the running minimum and the verdict) use no
scratch and no LDS, and their registers and occupancy are what DESIGN.md section 5m records -- read from the compiler's
kernel-resource-usage remarks for gfx950 as tests/test_movers_kernel_resources.py reads them.  A compiler that allocates
differently fails the pinned figures, not the kernels: then the figures here and in DESIGN.md are measured again."""
import pytest

from kernel_resources import usage_of

PINNED = {"flow_rays_kernel": {"VGPRs": 44, "TotalSGPRs": 58, "Occupancy": 8},
          "flow_object_rays_kernel": {"VGPRs": 25, "TotalSGPRs": 31, "Occupancy": 8},
          "flow_merge_kernel": {"VGPRs": 8, "TotalSGPRs": 14, "Occupancy": 8}}


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


@pytest.mark.parametrize("kernel", sorted(PINNED))
def test_flow_kernel_resources(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(k for k in usage if "flow" in k)
    u = usage[names[0]]
    print(f"\n[flow] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u
    assert {k: u[k] for k in PINNED[kernel]} == PINNED[kernel], u

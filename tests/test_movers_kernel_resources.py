"""CPU: the two kernels of the moving objects (mover_rays_kernel: gen_ray, the ray in the mover's frame, the cull;
mover_merge_kernel: the running winner and, in the last pass, write_back with a given normal and triangle row) use no scratch
and no LDS -- read from the compiler's kernel-resource-usage remarks as tests/test_material_kernel_resources.py reads them.
VGPRs, SGPRs and occupancy are printed, not fixed (DESIGN.md section 5k records them)."""
import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


@pytest.mark.parametrize("kernel", ["mover_rays_kernel", "mover_merge_kernel"])
def test_mover_kernel_has_no_scratch_and_no_lds(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(k for k in usage if "mover" in k)
    u = usage[names[0]]
    print(f"\n[movers] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u

"""CPU: the two kernels of the moving objects (mover_rays_kernel<false, false>: gen_ray, the ray in the mover's frame, the cull;
mover_merge_kernel<false, false>: the running winner and, in the last pass, write_back with a given normal and triangle row) use no scratch
and no LDS -- read from the compiler's kernel-resource-usage remarks as tests/test_material_kernel_resources.py reads them.
VGPRs, SGPRs and occupancy are printed, not fixed (DESIGN.md section 5k records them)."""
import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


# the instantiation by its mangled template arguments <SWEEP, NOISY>; the ids are the names the two kernels had before the family
KERNELS = [pytest.param("mover_rays_kernelILb0ELb0E", id="mover_rays_kernel"),
           pytest.param("mover_merge_kernelILb0ELb0E", id="mover_merge_kernel")]


@pytest.mark.parametrize("kernel", KERNELS)
def test_mover_kernel_has_no_scratch_and_no_lds(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(k for k in usage if "mover" in k)
    u = usage[names[0]]
    print(f"\n[movers] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u


@pytest.mark.parametrize("kernel", ["mover_rays_kernel", "mover_merge_kernel"])
def test_mover_kernel_templates_have_four_instantiations(usage, kernel):
    """The family is two templates over (SWEEP, NOISY): the unit holds exactly the four instantiations of each."""
    names = sorted(k for k in usage if kernel in k)
    assert len(names) == 4, names
    for sweep in (0, 1):
        for noisy in (0, 1):
            assert sum(f"{kernel}ILb{sweep}ELb{noisy}E" in k for k in names) == 1, names

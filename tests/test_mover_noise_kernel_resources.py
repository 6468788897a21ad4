"""CPU: the two kernels of the seeded sensor noise under movers (mover_rays_kernel<false, true>: gen_ray_noisy stored once with its live
byte, the stored world ray in a mover's frame, the cull; mover_merge_kernel<false, true>: the running winner on the clean ranges and, in
the last pass, the range draw and write_back with a given normal and triangle row on the stored world ray) are found exactly once
each and use no scratch and no LDS -- read from the compiler's kernel-resource-usage remarks as
tests/test_movers_kernel_resources.py reads them.  VGPRs, SGPRs and occupancy are printed, not fixed (DESIGN.md section 5r records
them)."""
import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


# the instantiation by its mangled template arguments <SWEEP, NOISY>; the ids are the names the two kernels had before the family
KERNELS = [pytest.param("mover_rays_kernelILb0ELb1E", id="mover_noisy_rays_kernel"),
           pytest.param("mover_merge_kernelILb0ELb1E", id="mover_noisy_merge_kernel")]


@pytest.mark.parametrize("kernel", KERNELS)
def test_mover_noise_kernel_has_no_scratch_and_no_lds(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(k for k in usage if "mover" in k)
    u = usage[names[0]]
    print(f"\n[mover noise] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u

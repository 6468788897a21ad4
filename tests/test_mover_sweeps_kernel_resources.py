"""CPU: the two kernels of the movers under moving-sensor sweeps (mover_rays_kernel<true, false>: gen_ray_sweep stored once, the stored
world ray in the frame the mover has at the ray's own firing fraction, the cull; mover_merge_kernel<true, false>: the running winner, the
normal turned by the pose at that fraction and, in the last pass, write_back with a given normal and triangle row about the
sweep's centre) are found exactly once each and use no scratch and no LDS -- read from the compiler's kernel-resource-usage
remarks as tests/test_movers_kernel_resources.py reads them.  VGPRs, SGPRs and occupancy are printed, not fixed (DESIGN.md section
5n records them)."""
import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


# the instantiation by its mangled template arguments <SWEEP, NOISY>; the ids are the names the two kernels had before the family
KERNELS = [pytest.param("mover_rays_kernelILb1ELb0E", id="mover_sweep_rays_kernel"),
           pytest.param("mover_merge_kernelILb1ELb0E", id="mover_sweep_merge_kernel")]


@pytest.mark.parametrize("kernel", KERNELS)
def test_mover_sweep_kernel_has_no_scratch_and_no_lds(usage, kernel):
    names = [k for k in usage if kernel in k]
    assert len(names) == 1, sorted(k for k in usage if "mover" in k)
    u = usage[names[0]]
    print(f"\n[mover sweeps] {kernel}: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u

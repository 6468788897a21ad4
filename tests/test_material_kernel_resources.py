"""CPU: the material instantiations of the trace kernel (GEN = 7: a loop of segment steps and further traversals behind the
first one, the original ray formed again behind the loop) use no scratch and no static LDS on either node route -- read from
the compiler's kernel-resource-usage remarks as tests/test_echo_kernel_resources.py reads them.  VGPRs, SGPRs and occupancy are
printed, not fixed (DESIGN.md section 5j records them)."""
import pytest

from kernel_resources import trace_kernel_name, usage_of

MATERIAL_QUANTISED = trace_kernel_name("kGenMaterials", qn=1)
MATERIAL_FLOAT32 = trace_kernel_name("kGenMaterials", qn=0)


@pytest.fixture(scope="module")
def usage():
    return usage_of("lidarcast.hip")


@pytest.mark.parametrize("name, route", [(MATERIAL_QUANTISED, "quantised nodes"), (MATERIAL_FLOAT32, "float32 nodes")])
def test_material_kernel_has_no_scratch_and_no_static_lds(usage, name, route):
    assert name in usage, sorted(k for k in usage if "trace_kernel" in k)
    u = usage[name]
    print(f"\n[material] trace_kernel<7, {route}>: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u            # no static LDS: the traversal stack is the launch's dynamic allocation, nothing beside it

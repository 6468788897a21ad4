"""CPU: the kernel of the skinned deforming movers (csrc/lrc_skin.hip: k_skin<false> for one key pose, k_skin<true> for two) uses
no scratch and no float64, and reads the staged bone tables from LDS -- read from the compiler's kernel-resource-usage remarks
and the gfx950 assembly as tests/test_deform_kernel_resources.py reads them.  The LDS is dynamic (48 * B bytes per pose, set at
the launch), so the remark's static LDS size is 0; VGPRs, SGPRs and occupancy are printed, not fixed (DESIGN.md section 5q
records them)."""
import re

import pytest

from kernel_resources import usage_of


@pytest.fixture(scope="module")
def built():
    return usage_of("lrc_skin.hip", asm=True)


def test_the_unit_holds_exactly_the_two_k_skin_instantiations(built):
    usage, _ = built
    assert len(usage) == 2, sorted(usage)
    assert sorted(re.search(r"k_skinILb([01])E", k).group(1) for k in usage) == ["0", "1"], sorted(usage)


@pytest.mark.parametrize("two", [0, 1])
def test_k_skin_has_no_scratch(built, two):
    usage, _ = built
    names = [k for k in usage if f"k_skinILb{two}E" in k]
    assert len(names) == 1, sorted(usage)
    u = usage[names[0]]
    print(f"\n[skin] k_skin<{'true' if two else 'false'}>: {u}")
    assert u["ScratchSize"] == 0, u
    assert u["LDS"] == 0, u              # dynamic: sized by B at the launch


def test_k_skin_reads_the_tables_from_lds_and_uses_no_float64(built):
    _, text = built
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\s", text, re.M)
    assert any(o.startswith("ds_read") or o.startswith("ds_load") for o in ops)
    assert ops.count("s_barrier") == 2                                    # one __syncthreads() per instantiation
    assert not [o for o in ops if o.startswith("flat_") or o.startswith("scratch_")], "generic or scratch accesses"
    assert not [o for o in ops if o.endswith("_f64")], "float64 arithmetic"

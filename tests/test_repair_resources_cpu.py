"""Scratch / spill / LDS budget of the shipped repair kernels (csrc/htp_repair.hip), read from the code object's
own metadata (tools/kernel_resources.py) -- CPU only: four kernels, pure copies and integer
logic, so none may need scratch or spill a register, and only the scan holds LDS (its 16 wavefront totals)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "headland_trajectory_planning_amd", "libhtp.so")
KERNELS = ("repair_scan_kernel", "repair_gather_kernel", "repair_decide_kernel", "repair_scatter_kernel")


@pytest.fixture(scope="module")
def repair_kernels():
    if not os.path.exists(LIB):
        pytest.fail("libhtp.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools.kernel_resources import kernels
    found = {}
    for name in KERNELS:
        hits = [v for k, v in kernels(LIB).items() if name in k]
        assert len(hits) == 1, (name, len(hits))
        found[name] = hits[0]
    return found


@pytest.mark.parametrize("name", KERNELS)
def test_repair_kernels_have_no_scratch_and_no_spills(repair_kernels, name):
    r = repair_kernels[name]
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, r
    assert r["vgpr_count"] <= 64, r                      # eight wavefronts per SIMD by registers: copies hide latency by occupancy
    assert r["group_segment_fixed_size"] == (64 if name == "repair_scan_kernel" else 0), r

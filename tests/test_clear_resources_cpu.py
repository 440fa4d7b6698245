"""Register, scratch and LDS budget of the shipped pose-clearance and turn-selection kernels (csrc/htp_clear.hip), read
from the code object's own metadata (tools/kernel_resources.py) -- CPU only.  DESIGN.md s.3.18 has the layout.

The budget: no private memory, no vector-register spill, at most 128 VGPRs (four wavefronts per SIMD by registers, as
the audit kernel has), and a fixed LDS that is exactly what the layout in clear_core.h adds up to:

    obstacle edge records   7 x 16 x 8 = 896 doubles
    body edge records       7 x  4 x 8 = 224
    polygon (first, count)  2 x (16 + 4) = 40
    placed poses            4 x 128 = 512      (x, y, cos, sin; the raw halfspace rows live here until the edges stand)
    given poses             3 x (128 + 1) + 1 = 388   (x, y, yaw of a chunk and the pose that closes its last gap; padded)
    per-pose keys           128
                            2188 doubles = 17504 bytes

Both kernels meet it.  Not part of the budget, pinned so that it cannot grow unseen: the clearance kernel spills
SGPR_SPILLS scalar registers into lanes of a VGPR (v_writelane / v_readlane, no memory traffic).  With sin / cos and
hypot of the planner libm inlined it was 219 (their double-double constants are scalar); they are called out of line,
as speed_core.h does.  What is left are the fourteen array pointers, the shape and the loop state of a path, live
across the chunk loop."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "headland_trajectory_planning_amd", "libhtp.so")

CLEAR_LDS = 8 * (896 + 224 + 40 + 512 + 388 + 128)      # 17504 bytes
SGPR_SPILLS = 81                                         # the shipped clearance kernel's


@pytest.fixture(scope="module")
def found():
    if not os.path.exists(LIB):
        pytest.fail("libhtp.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools.kernel_resources import kernels
    out = {}
    for name in ("pose_clearance_kernel", "turn_select_kernel"):
        hit = [v for k, v in kernels(LIB).items() if name in k]
        assert len(hit) == 1, name
        out[name] = hit[0]
    return out


@pytest.mark.parametrize("name", ["pose_clearance_kernel", "turn_select_kernel"])
def test_no_private_memory_no_vector_spill_and_four_wavefronts_per_simd(found, name):
    k = found[name]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] + k["agpr_count"] <= 128, k


def test_lds_is_what_the_layout_adds_up_to(found):
    assert CLEAR_LDS == 17504
    assert found["pose_clearance_kernel"]["group_segment_fixed_size"] == CLEAR_LDS, found["pose_clearance_kernel"]
    assert found["turn_select_kernel"]["group_segment_fixed_size"] == 0, found["turn_select_kernel"]


def test_scalar_spills_do_not_exceed_the_shipped_counts(found):
    assert found["pose_clearance_kernel"]["sgpr_spill_count"] <= SGPR_SPILLS, found["pose_clearance_kernel"]
    assert found["turn_select_kernel"]["sgpr_spill_count"] == 0, found["turn_select_kernel"]

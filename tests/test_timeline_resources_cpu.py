"""LDS / scratch / spill budget of the shipped trajectory-timeline kernel (csrc/htp_timeline.hip), read from the
code object's own metadata (tools/kernel_resources.py) -- CPU only: the fixed LDS is the tile
of 64 rows; the per-stage LDS (80 B per stage) is requested at launch, so the largest horizon the ABI accepts
must still fit 64 KB."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "headland_trajectory_planning_amd", "libhtp.so")

FIXED_LDS = 5120           # bytes: 64 rows x 10 columns
STAGE_LDS = 80             # bytes per stage: X 5, U 2, tau / h, node time, node arc length


@pytest.fixture(scope="module")
def timeline_kernel():
    if not os.path.exists(LIB):
        pytest.fail("libhtp.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools.kernel_resources import kernels
    hits = [v for k, v in kernels(LIB).items() if "obca_timeline_kernel" in k]
    assert len(hits) == 1                                 # exactly one timeline kernel
    return hits[0]


def test_timeline_kernel_has_no_scratch_and_no_spills(timeline_kernel):
    r = timeline_kernel
    assert r["group_segment_fixed_size"] == FIXED_LDS, r
    assert r["private_segment_fixed_size"] == 0, r       # no scratch: rows go through the LDS tile, no private arrays
    assert r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 128, r                     # four wavefronts per SIMD by registers


def test_timeline_lds_fits_a_workgroup_at_the_largest_horizon(timeline_kernel):
    hdr = open(os.path.join(ROOT, "include", "htp.h")).read()
    assert re.search(r"#define HTP_TIMELINE_MAX_N HTP_AUDIT_MAX_N\b", hdr)
    max_n = int(re.search(r"#define HTP_AUDIT_MAX_N (\d+)", hdr).group(1))
    core = open(os.path.join(ROOT, "headland_trajectory_planning_amd", "csrc", "timeline_core.h")).read()
    per_stage = int(re.search(r"lds_stage_doubles\(int N\) \{ return (\d+) \* N; \}", core).group(1))
    assert per_stage * 8 == STAGE_LDS
    assert timeline_kernel["group_segment_fixed_size"] + STAGE_LDS * max_n <= 64 * 1024

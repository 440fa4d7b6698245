"""LDS / scratch / spill budget of the shipped tracking-rollout kernel (csrc/htp_track.hip), read from the code
object's own metadata (tools/kernel_resources.py) -- CPU only: the fixed LDS holds the edge
records, the reference tile (in the area the raw halfspace rows use first) and the chunk's per-tick minima; the
per-stage LDS (72 B per stage) is requested at launch, so the largest horizon the ABI accepts must still fit 64 KB."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "headland_trajectory_planning_amd", "libhtp.so")
CSRC = os.path.join(ROOT, "headland_trajectory_planning_amd", "csrc")

FIXED_LDS = 13632          # bytes: 7 x (128 + 32) edge doubles, 40 polygon doubles, 480 tile doubles, 64 tick minima
STAGE_LDS = 72             # bytes per stage: X 5, U 2, tau / h, node time
VGPRS = 164                # the shipped binary's; three wavefronts per SIMD by registers, two by LDS at N = 80


@pytest.fixture(scope="module")
def track_kernel():
    if not os.path.exists(LIB):
        pytest.fail("libhtp.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools.kernel_resources import kernels
    hits = [v for k, v in kernels(LIB).items() if "obca_track_kernel" in k]
    assert len(hits) == 1                                 # exactly one track kernel
    return hits[0]


def test_track_kernel_has_no_scratch_no_spills_and_no_private_arrays(track_kernel):
    r = track_kernel
    assert r["group_segment_fixed_size"] == FIXED_LDS and FIXED_LDS % 16 == 0, r
    assert r["private_segment_fixed_size"] == 0, r       # no scratch, hence no private array and no spill to memory
    assert r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] == VGPRS, r
    core = open(os.path.join(CSRC, "track_core.h")).read()
    body = core[core.index("HTP_HD inline void run_problem"):]
    assert not re.search(r"\b(double|int|int32_t|State)\s+\w+\s*\[", body)       # nothing indexed lives in registers


def test_track_lds_fits_a_workgroup_at_the_largest_horizon(track_kernel):
    hdr = open(os.path.join(ROOT, "include", "htp.h")).read()
    assert re.search(r"#define HTP_TRACK_MAX_N HTP_AUDIT_MAX_N\b", hdr)
    max_n = int(re.search(r"#define HTP_AUDIT_MAX_N (\d+)", hdr).group(1))
    core = open(os.path.join(CSRC, "track_core.h")).read()
    per_stage = int(re.search(r"lds_stage_doubles\(int N\) \{ return (\d+) \* N; \}", core).group(1))
    assert per_stage * 8 == STAGE_LDS
    # the launch asks for exactly that formula
    hip = open(os.path.join(CSRC, "htp_track.hip")).read()
    assert "sizeof(double) * (size_t)track::lds_stage_doubles(sh.N)" in hip
    assert track_kernel["group_segment_fixed_size"] + STAGE_LDS * max_n == 48192 <= 64 * 1024

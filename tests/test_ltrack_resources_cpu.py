"""LDS / scratch / spill budget of the shipped kernel of the rollout under the LQR gains (csrc/htp_ltrack.hip), read
from the code object's own metadata (tools/kernel_resources.py) -- CPU only: the fixed LDS holds
the edge records, the tile of 65 rows of 17 doubles (reference row and law row; the raw halfspace rows use the area
first), the chunk's per-tick minima and its per-tick error maxima; the per-stage LDS (72 B per stage, the track's) is
requested at launch, so the largest horizon the ABI accepts must still fit 64 KB.  The gains stay in global memory."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "headland_trajectory_planning_amd", "libhtp.so")
CSRC = os.path.join(ROOT, "headland_trajectory_planning_amd", "csrc")

FIXED_LDS = 20176          # bytes: 7 x (128 + 32) edge doubles, 40 polygon doubles, 1106 tile doubles, 64 minima, 192 maxima
STAGE_LDS = 72             # bytes per stage: X 5, U 2, tau / h, node time
VGPRS = 169                # the shipped binary's; three wavefronts per SIMD by registers, as the track kernel's 164


@pytest.fixture(scope="module")
def ltrack_kernel():
    if not os.path.exists(LIB):
        pytest.fail("libhtp.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools.kernel_resources import kernels
    hits = [v for k, v in kernels(LIB).items() if "obca_ltrack_kernel" in k]
    assert len(hits) == 1                                 # exactly one ltrack kernel
    return hits[0]


def test_ltrack_kernel_has_no_scratch_no_spills_and_no_private_arrays(ltrack_kernel):
    r = ltrack_kernel
    assert r["group_segment_fixed_size"] == FIXED_LDS and FIXED_LDS % 16 == 0, r
    assert r["private_segment_fixed_size"] == 0, r       # no scratch, hence no private array and no spill to memory
    assert r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] == VGPRS, r
    core = open(os.path.join(CSRC, "ltrack_core.h")).read()
    body = core[core.index("HTP_HD inline void law_row"):]
    assert not re.search(r"\b(double|int|int32_t|State)\s+\w+\s*\[", body)       # nothing indexed lives in registers


def test_ltrack_lds_fits_a_workgroup_at_the_largest_horizon(ltrack_kernel):
    hdr = open(os.path.join(ROOT, "include", "htp.h")).read()
    max_n = int(re.search(r"#define HTP_AUDIT_MAX_N (\d+)", hdr).group(1))
    assert re.search(r"#define HTP_TRACK_MAX_N HTP_AUDIT_MAX_N\b", hdr) and max_n == 480
    core = open(os.path.join(CSRC, "ltrack_core.h")).read()
    per_stage = int(re.search(r"lds_stage_doubles\(int N\) \{ return (\d+) \* N; \}", core).group(1))
    assert per_stage * 8 == STAGE_LDS
    # the launch asks for exactly that formula
    hip = open(os.path.join(CSRC, "htp_ltrack.hip")).read()
    assert "sizeof(double) * (size_t)ltrack::lds_stage_doubles(sh.N)" in hip
    assert ltrack_kernel["group_segment_fixed_size"] + STAGE_LDS * max_n == 54736 <= 64 * 1024

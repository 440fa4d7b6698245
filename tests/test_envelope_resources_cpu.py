"""LDS / scratch / spill budget of the shipped trajectory-envelope kernel (csrc/htp_envelope.hip), read from the
code object's own metadata (tools/kernel_resources.py) -- CPU only: the fixed LDS holds the body
edges, a chunk of 256 poses and their bounding boxes; the two bitmaps (16 KB for a full grid) and the per-stage
part (64 B per stage) are requested at launch, so the largest horizon the ABI accepts with the largest grid must
still fit 64 KB."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "headland_trajectory_planning_amd", "libhtp.so")

FIXED_LDS = 12352          # bytes: edges 1792, polygons 64, poses 8192, boxes 2048, per-body extents 256
STAGE_LDS = 64             # bytes per stage: X 5, U 2, tau / h
BITMAP_LDS = 2 * 8192      # bytes: the current body's and the union's bitmap of a full grid
VGPRS = 124                # the shipped binary's


@pytest.fixture(scope="module")
def envelope_kernel():
    if not os.path.exists(LIB):
        pytest.fail("libhtp.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools.kernel_resources import kernels
    hits = [v for k, v in kernels(LIB).items() if "envelope" in k]
    assert len(hits) == 1                                 # exactly one envelope kernel
    return hits[0]


def test_envelope_kernel_has_no_scratch_and_no_spills(envelope_kernel):
    r = envelope_kernel
    assert r["group_segment_fixed_size"] == FIXED_LDS, r
    assert r["private_segment_fixed_size"] == 0, r       # no scratch: nothing polygon-shaped in private arrays
    assert r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 128, r                     # four wavefronts per SIMD by registers
    assert r["vgpr_count"] == VGPRS, r


def test_envelope_lds_fits_a_workgroup_at_the_largest_horizon_and_grid(envelope_kernel):
    hdr = open(os.path.join(ROOT, "include", "htp.h")).read()
    assert re.search(r"#define HTP_ENVELOPE_MAX_N HTP_AUDIT_MAX_N\b", hdr)
    max_n = int(re.search(r"#define HTP_AUDIT_MAX_N (\d+)", hdr).group(1))
    assert max_n >= 160
    cells = int(re.search(r"#define HTP_ENVELOPE_MAX_CELLS (\d+)", hdr).group(1))
    assert 2 * cells // 8 == BITMAP_LDS
    core = open(os.path.join(ROOT, "headland_trajectory_planning_amd", "csrc", "envelope_core.h")).read()
    per_stage = int(re.search(r"lds_stage_doubles\(int N\) \{ return (\d+) \* N; \}", core).group(1))
    assert per_stage * 8 == STAGE_LDS
    assert envelope_kernel["group_segment_fixed_size"] + BITMAP_LDS + STAGE_LDS * max_n <= 64 * 1024

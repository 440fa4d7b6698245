"""Register, scratch and LDS budget of the two shipped kernels of the sampled pose search (csrc/htp_sample.hip), read
from the code object's own metadata (tools/kernel_resources.py) -- CPU only.  The values are those of the shipped
binary (DESIGN.md s.3.16 says where the candidate kernel's private memory comes from)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "headland_trajectory_planning_amd", "libhtp.so")

SCENE_LDS = 4312     # bytes: 256 vertices (4096), 49 table entries (196), four scalars (16), padded to 8
WORDS_LDS = 3080     # bytes: 48 Reeds-Shepp words of 64 bytes, behind the Scene at a 16-byte boundary


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.fail("libhtp.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    from tools.kernel_resources import kernels
    found = kernels(LIB)
    cand = sorted((k, v) for k, v in found.items() if "classic_sample_kernel" in k)
    win = [v for k, v in found.items() if "classic_sample_winner_kernel" in k]
    assert len(cand) == 2 and len(win) == 1
    # the template argument in the mangled name: ILi2E the Reeds-Shepp words (1 << 1), ILi5E Dubins | circle-back
    assert "ILi2E" in cand[0][0] and "ILi5E" in cand[1][0]
    return {"words": cand[0][1], "rows": cand[1][1], "winner": win[0]}


def test_rows_kernel_has_no_private_memory(kernels):
    r = kernels["rows"]
    assert r["private_segment_fixed_size"] == 0, r       # polygons in LDS, corner arrays indexed by constants
    assert r["vgpr_spill_count"] == 0, r
    assert r["group_segment_fixed_size"] == SCENE_LDS, r  # the words' LDS is not part of this instance
    assert r["vgpr_count"] + r["agpr_count"] <= 256, r    # two wavefronts per SIMD by registers


def test_words_kernel_resources_are_the_shipped_ones(kernels):
    r = kernels["words"]
    # 208 bytes per lane: the run-time-indexed segment arrays of rs_core.h's word generator and sampler, which the
    # project's Reeds-Shepp kernels carry too; nothing polygon-shaped
    assert r["private_segment_fixed_size"] == 208, r
    assert r["vgpr_spill_count"] == 0, r
    assert r["group_segment_fixed_size"] == SCENE_LDS + WORDS_LDS, r
    assert r["vgpr_count"] <= 512, r                       # one wavefront per SIMD


def test_winner_kernel_is_small(kernels):
    r = kernels["winner"]
    assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 32, r

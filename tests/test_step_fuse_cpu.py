"""Conditions on the inputs of tests/test_gpu_step_fuse.py, from the serial host build with path counters
(csrc/obca_stats_hostsim.cpp): the cases really meet pivoted local blocks, the restoration phase and second-order
corrections, so the device test exercises the readers of the buffers the fused passes moved.  And the stand-alone
sanitizer program of the two smallest shapes (csrc/obca_step_asan.cpp) runs clean."""
import os
import subprocess

import pytest

import _step_cases as S


@pytest.fixture(scope="module")
def stats():
    return {name: S.solve_stats([S.instance(name)])[1][0] for name in S.CASES}


@pytest.mark.parametrize("name", list(S.CASES))
def test_cases_take_the_paths_they_are_for(stats, name):
    piv_max, piv_sweeps, soc, resto = (int(v) for v in stats[name])
    want = S.CASES[name][1]
    assert piv_max >= want.get("piv", 0), (name, piv_max)
    if want.get("piv", 0):
        assert piv_sweeps >= 1
    assert soc >= want.get("soc", 0), (name, soc)
    assert resto >= want.get("resto", 0), (name, resto)


def test_the_960_block_case_fills_more_than_one_pass2_trip(stats):
    assert int(stats["n80_m12"][0]) > 64


def test_host_solver_under_sanitizers(tmp_path):
    """HostLane solves of the two smallest shapes under -fsanitize=address,undefined (a program of its own)."""
    exe = str(tmp_path / "obca_step_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(S.CSRC, "obca_step_asan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]

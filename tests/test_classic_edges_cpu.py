"""The classic-turn planner (csrc/classic_core.h, classic_batch.h) at its edges, on the CPU: the host build
(_hostsim.classic_host) and the stand-alone sanitizer program (csrc/classic_asan.cpp: address, undefined and
float-cast-overflow, exactly-sized buffers, a child process) on the same batches of tests/_classic_cases.py.

Every status of the planner is produced: bad_input (non-finite parameters, a steering limit outside (0, 1.5) or too
small to steer with, a side the planners do not know, an unknown type, non-positive lengths, a body polygon of 2 or
MAXB + 1 vertices, an arc shorter than one step), overflow (each capacity check: arc_new's rows, dubins_full's rows
and samples, the fish-tail's word rows and turn-out scan), no_word, no_dubins and rs_error.  The expected statuses
come from the planner's definition, not from a run: see the case tables.  Outputs are pre-filled with sentinels, so
what a turn must leave untouched is checked exactly.  DESIGN.md s.3.6a.

rs_error: a seeded search of 4 000 pose pairs through the host build (uniform poses, row-like poses, axis-aligned
poses, and pairs 1e-9 / 1e-12 apart) found it only among the nearly coincident pairs (710 of 1 000); one of those,
rounded, is the case here."""
import numpy as np
import pytest

import _classic_cases as cc
from _hostsim import classic_host
from headland_trajectory_planning_amd import _native

S = _native.CT_STATUS


def _names(status):
    return [S.get(int(v), int(v)) for v in status]


def _run_both(cases, cap_path=cc.CAP_PATH, cap_samples=cc.CAP_SAMPLES):
    """(packed, host build's results with one turn of storage beyond the batch, the sanitizer program's results)."""
    pk = cc.pack(cases, cap_path, cap_samples)
    host = classic_host(pk, out=cc.sentinel_results(pk))
    san, rc, err = cc.run_asan(pk)
    assert rc == 0, f"the sanitizer program stopped (exit {rc}):\n{err[-3000:]}"
    B = pk.batch
    # the two builds of one source: the same bits, sentinels included
    assert np.array_equal(san.status, host.status[:B]) and np.array_equal(san.n_path, host.n_path[:B])
    assert np.array_equal(san.path.view(np.int64), host.path[:B].view(np.int64))
    # the turn of storage beyond the batch is untouched
    assert host.status[B] == cc.ISENTINEL and host.n_path[B] == cc.ISENTINEL and np.all(host.path[B] == cc.SENTINEL)
    return pk, host, san


@pytest.fixture(scope="module")
def edge():
    cases = cc.edge_batch()
    return (cases,) + _run_both(cases)


def test_every_case_ends_with_its_status(edge):
    cases, pk, host, _ = edge
    got = _names(host.status[:pk.batch])
    wrong = [(b, c[0], got[b], c[3]) for b, c in enumerate(cases) if got[b] != c[3]]
    assert not wrong, wrong
    for b, c in enumerate(cases):
        assert (host.n_path[b] > 0) == (c[3] == "ok"), (b, c[0], int(host.n_path[b]))
    assert {c[3] for c in cases} == {"ok", "overflow", "no_word", "bad_input", "rs_error", "no_dubins"}
    assert len(cases) <= 65     # the largest launch of the GPU tests


def test_output_contract(edge):
    cases, pk, host, _ = edge
    for b, c in enumerate(cases):
        n = int(host.n_path[b])
        if c[3] == "ok":        # rows of the path, then the caller's pre-fill
            assert np.all(np.isfinite(host.path[b, :n])) and np.all(host.path[b, n:] == cc.SENTINEL), (b, c[0])
        elif c[3] != "overflow":    # bad_input is rejected before anything is planned, no_word / rs_error / no_dubins
            assert np.all(host.path[b] == cc.SENTINEL), (b, c[0])     # before a row is written: the caller's block
    # 200 samples a turn are enough for every good turn (the GPU tests grow the scratch from there)
    small = classic_host(cc.pack(cases, cap_samples=200), out=cc.sentinel_results(pk))
    assert np.array_equal(small.status, host.status) and np.array_equal(small.n_path, host.n_path)
    assert np.array_equal(small.path.view(np.int64), host.path.view(np.int64))
    # good turns are the same whatever their neighbours are: each one alone gives the rows it has in the batch
    alone = 0
    for b, c in enumerate(cases):
        if c[3] == "ok":
            one = cc.pack([c])
            r = classic_host(one, out=cc.sentinel_results(one))
            assert r.n_path[0] == host.n_path[b] and np.array_equal(r.path[0], host.path[b]), (b, c[0])
            alone += 1
    assert alone == len(cc.good_cases()) + 2        # and the two wide-row turns


def _full(kind_case):
    """(n_path, rows) of one good case with generous capacities."""
    pk = cc.pack([kind_case])
    r = classic_host(pk)
    assert r.status[0] == 0
    return int(r.n_path[0]), r.rows(0)


@pytest.mark.parametrize("k", [0, 1, 2], ids=["circleback", "fishtail", "dubins"])
def test_cap_path_edges(k):
    case = cc.good_cases()[k]
    n, rows = _full(case)
    _, exact, _ = _run_both([case], cap_path=n)
    assert _names(exact.status[:1]) == ["ok"] and exact.n_path[0] == n
    assert np.array_equal(exact.path[0].view(np.int64), rows.view(np.int64))       # identical rows, none to spare
    _, short, _ = _run_both([case], cap_path=n - 1)
    assert _names(short.status[:1]) == ["overflow"] and short.n_path[0] == 0
    if k == 0:
        # forward arc [0, n1), reverse arc [n1, n2), Dubins lead [n2, n): with n - 1 rows the trailing dubins_full
        # overflows (both arcs are written), with n2 - 1 the second arc_new (the first arc is), with n1 - 1 the first
        d = rows[:, 4]
        n1 = int(np.argmax(d < 0))
        n2 = n1 + int(np.argmax(d[n1:] > 0))
        assert 2 < n1 < n2 < n and np.all(d[n1:n2] == -1.0)
        assert np.array_equal(short.path[0, :n2], rows[:n2]) and np.all(short.path[0, n2:] == cc.SENTINEL)
        _, mid, _ = _run_both([case], cap_path=n2 - 1)
        assert _names(mid.status[:1]) == ["overflow"]
        assert np.array_equal(mid.path[0, :n1], rows[:n1]) and np.all(mid.path[0, n1:] == cc.SENTINEL)
        _, low, _ = _run_both([case], cap_path=n1 - 1)
        assert _names(low.status[:1]) == ["overflow"] and np.all(low.path[0] == cc.SENTINEL)
        _, fit, _ = _run_both([case], cap_path=n2)          # both arcs fit exactly, the lead does not
        assert _names(fit.status[:1]) == ["overflow"] and np.array_equal(fit.path[0, :n2], rows[:n2])
    if k == 1:
        # lead-in [0, m), word rows [m, n): the turn has a lead-in (its exit pose lies inside the rows)
        _, lead, _ = _run_both([case], cap_path=20)
        assert _names(lead.status[:1]) == ["overflow"] and np.all(lead.path[0] == cc.SENTINEL)


def test_capacity_launches_as_the_device_gets_them():
    """The mixed launches of _classic_cases.capacity_launches (the GPU tests run the same): statuses as the counts
    say, an exactly filled block with its neighbour directly behind, through the host build and the sanitizer program."""
    launches = cc.capacity_launches()
    assert len(launches) == 10
    for name, cases, cap_path, cap_samples in launches:
        _, r, _ = _run_both(cases, cap_path, cap_samples)
        B = len(cases)
        assert _names(r.status[:B]) == [c[3] for c in cases], name
        for b, c in enumerate(cases):
            n = int(r.n_path[b])
            assert (n > 0) == (c[3] == "ok"), (name, b)
            if c[3] == "ok":
                assert np.all(np.isfinite(r.path[b, :n])) and np.all(r.path[b, n:] == cc.SENTINEL), (name, b)
    full = [la for la in launches if la[2] != cc.CAP_PATH and la[1][0][3] == "ok"]
    assert len(full) == 1       # the circle-back turn fills its block to the last row once, twice in that launch


def test_cap_samples_edge_at_the_minimum():
    """dubins_full's `while (x < L)` loop against cap_samples = 16, the entry's minimum: a Dubins turn whose step
    gives 16 samples fits, the same turn with 17 does not.  The counts come from the restated pydubins."""
    db = cc.base("db")
    s16, s17 = cc.step_for_samples(db, 16), cc.step_for_samples(db, 17)
    assert cc.dubins_samples(db, s16) == 16 and cc.dubins_samples(db, s17) == 17
    cases = [("16 samples", db, {cc.P_STEP: s16}, "ok"), ("17 samples", db, {cc.P_STEP: s17}, "overflow")]
    _, r, _ = _run_both(cases, cap_samples=16)
    assert _names(r.status[:2]) == ["ok", "overflow"] and r.n_path[0] > 0 and r.n_path[1] == 0
    _, r17, _ = _run_both(cases, cap_samples=17)
    assert _names(r17.status[:2]) == ["ok", "ok"]
    assert np.array_equal(r17.path[0], r.path[0])           # equal wherever both capacities suffice


def test_no_word_is_the_reference_none():
    """One large blocker across the headland, beyond the 45-degree turn-out arcs: the restated reference finds the
    offset poses of the unwalled turn and then no collision-free word (None); the planner says no_word.  The same
    wall far away changes nothing."""
    ft = cc.base("ft")
    open_start, open_end, open_path = cc.reference_fishtail()
    w_start, w_end, w_path = cc.reference_fishtail(cc.wall(ft, cc.WALL_GAP))
    assert np.array_equal(open_start, w_start) and np.array_equal(open_end, w_end)    # the offset poses exist
    assert open_path is not None and w_path is None
    cases = [c for c in cc.good_cases() if c[0] in ("ft", "ft far wall")] + [cc.planner_cases()[0]]
    r = classic_host(cc.pack(cases))
    assert _names(r.status) == ["ok", "ok", "no_word"]
    assert r.rows(0).shape == open_path.shape and np.max(np.abs(r.rows(0) - open_path)) <= 1e-11
    assert np.array_equal(r.rows(0), r.rows(1))


def test_no_dubins_where_the_reference_raises():
    """start == end at yaw 0 is the Dubins word of length 0 (no sample), 1 mm ahead a path with one sample: the
    restated get_dubins_path_full raises on both (no spline through fewer than two points), so there is no defined
    result to follow; the planner reports no_dubins."""
    from headland_trajectory_planning_amd.path_planner import safety_forward_path_plan as sfp
    for c in cc.planner_cases()[1:3]:
        t = c[1]
        assert cc.dubins_samples(t, 0.1) in (0, 1)
        with pytest.raises((IndexError, ValueError)):
            sfp.get_dubins_path_full(np.array(t["start"]), np.array(t["end"]), t["radius"])
        r = classic_host(cc.pack([c]))
        assert _names(r.status) == ["no_dubins"]


def test_wide_rows_boundary():
    """Rows 2R or more apart in the circle-back type are the Dubins type bit for bit; one ulp below 2R the circle-back
    construction runs (and ends bad_input, see _classic_cases.wide_cases) while the Dubins type still plans."""
    wide = cc.wide_cases()
    below = wide[2]
    cases = wide + [("db rows one ulp below 2R", below[1], {**below[2], cc.P_TYPE: 0.0}, "ok")]
    _, r, _ = _run_both(cases)
    assert _names(r.status[:4]) == [c[3] for c in cases]
    assert r.n_path[0] > 0 and np.array_equal(r.path[0].view(np.int64), r.path[1].view(np.int64))
    assert np.all(r.path[2] == cc.SENTINEL)


def test_tiny_step_through_the_sample_core():
    """The circle-back candidates of a turn with step 1e-9 are C_OVERFLOW (their arcs need 6e9 rows), the turn
    SMP_OVERFLOW, not C_PLANNER / none feasible as the wrapped int capacity test had it on the host; the good turns
    beside it keep their winners."""
    import _sample_host as sh
    turns = cc.sample_turns()
    r = sh.sample_host(_native.SamplePacked(turns, cap_samples=cc.SAMPLE_CAP))
    alone = [sh.sample_host(_native.SamplePacked([t], cap_samples=cc.SAMPLE_CAP)) for t in turns]
    assert r.status.tolist() == [_native.SMP_OK, _native.SMP_OVERFLOW, _native.SMP_OK]
    n = len(turns[1]["start_x"])
    assert np.all(r.cand_status[1, :n] == _native.SMP_C_OVERFLOW) and r.n_feasible[1] == 0
    for b in (0, 2):
        assert np.array_equal(r.winner[b], alone[b].winner[0]) and r.score[b] == alone[b].score[0]

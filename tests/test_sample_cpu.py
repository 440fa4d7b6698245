"""The sampled exit / entry pose search on the CPU: the signed ring distance on hand-computable cases, the serial host
build of csrc/sample_core.h against the numpy restatement (the host planners of path_planner/, candidate by
candidate), the reference's quirks one by one, the bad-input cases, and the stand-alone sanitizer program.
The reference itself (shapely, pydubins) is not run: the restatement is the oracle."""
import contextlib
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import _sample_host as sh  # noqa: E402
from headland_trajectory_planning_amd import _native  # noqa: E402
from headland_trajectory_planning_amd.path_planner import map_utils  # noqa: E402
from headland_trajectory_planning_amd.path_planner import safety_forward_path_plan as sfp  # noqa: E402
from headland_trajectory_planning_amd.path_planner.car_model import CarModel  # noqa: E402
from headland_trajectory_planning_amd.path_planner.geom import (Polygon, convex_contains_point, convex_intersects,  # noqa: E402
                                                                 place, ring_of, ring_signed_distance)
from headland_trajectory_planning_amd.path_planner.OGE_OBCA import orchard_environment_OBCA  # noqa: E402

N_ = _native

# (config, problem, type, n_start, n_end): config C carries the mower, A and B no implement
SCENES = [("C", 1, "dubins", 4, 4), ("C", 4, "dubins", 4, 3), ("B", 3, "dubins", 3, 4),
          ("A", 0, "reeds_shepp", 4, 4), ("C", 2, "reeds_shepp", 4, 4), ("B", 2, "reeds_shepp", 3, 3),
          ("B", 0, "circle_back", 4, 1), ("B", 1, "circle_back", 3, 1), ("C", 3, "circle_back", 4, 1)]


# ------------------------------------------------------------------ signed ring distance
SQUARE = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0]])
ELL = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 2.0], [2.0, 2.0], [2.0, 4.0], [0.0, 4.0]])   # reflex vertex (2, 2)
RING_CASES = [
    (SQUARE, (1.0, 2.0), 1.0),                       # inside, nearest to the edge x = 0
    (SQUARE, (2.0, 2.0), 2.0),                       # the centre
    (SQUARE, (5.0, 2.0), -1.0),                      # outside, nearest to the edge x = 4
    (SQUARE, (5.0, 5.0), -math.sqrt(2.0)),           # outside, nearest to the vertex (4, 4)
    (SQUARE, (-3.0, -4.0), -5.0),                    # outside, nearest to the vertex (0, 0)
    (SQUARE, (3.5, 3.75), 0.25),                     # inside, nearest to the edge y = 4
    (ELL, (1.5, 1.5), math.sqrt(0.5)),               # inside, nearest to the reflex vertex
    (ELL, (3.0, 3.0), -1.0),                         # in the notch: outside, nearest to the edges through (2, 2)
    (ELL, (2.5, 2.25), -0.25),                       # in the notch, nearest to the edge y = 2
    (ELL, (1.0, 3.0), 1.0),                          # inside the upright arm
    (ELL, (3.0, 1.0), 1.0),                          # inside the lying arm
    (ELL, (5.0, 3.0), -math.sqrt(2.0)),              # outside, nearest to the vertex (4, 2)
]


@pytest.mark.parametrize("impl", ["host", "numpy"])
def test_signed_ring_distance_closed_forms(impl):
    for ring, pt, want in RING_CASES:
        for r in (ring, ring[::-1].copy(), np.roll(ring, 2, axis=0)):   # orientation and start vertex do not matter
            got = sh.ring_distance(r, [pt])[0] if impl == "host" else float(ring_signed_distance(r, np.array(pt)))
            assert abs(got - want) <= 4e-16 * max(1.0, abs(want)), (pt, got, want)


# ------------------------------------------------------------------ host build against the numpy restatement
@pytest.fixture(scope="module")
def tables():
    """Every scene once: (request, turn, numpy status / score / winner) and the host build's results of one launch."""
    items = []
    with sh.oracle_rs():
        for cfg, pid, typ, ns, ne in SCENES:
            req, turn = sh.request(cfg, pid, typ, ns, ne)
            items.append((req, turn) + sh.np_tables(req, turn))
    res = sh.sample_host(N_.SamplePacked([t for _, t, *_ in items]))
    return items, res


def test_host_candidate_tables_equal_the_restatement(tables):
    items, res = tables
    assert any(len(req["car"].aux_polys) for req, *_ in items)
    for k, (req, turn, st, sc, win) in enumerate(items):
        n = len(st)
        assert n <= 16
        assert np.array_equal(res.cand_status[k, :n], st), (k, res.cand_status[k, :n], st)
        assert np.all(res.cand_status[k, n:] == N_.SMP_C_UNUSED)
        feas = st == N_.SMP_C_FEASIBLE
        assert np.all(np.isneginf(res.cand_score[k, :n][~feas])) and np.all(np.isneginf(res.cand_score[k, n:]))
        err = np.max(np.abs(res.cand_score[k, :n][feas] - sc[feas])) if feas.any() else 0.0
        print(f"turn {k} ({turn['type']}): {int(feas.sum())}/{n} feasible, score error {err:.3e}")
        assert err <= 1e-9
    assert sum(int((st == N_.SMP_C_FEASIBLE).any()) for _, _, st, _, _ in items) >= 6   # the scenes are not all blocked


def test_host_winner_equals_the_restatement(tables):
    items, res = tables
    for k, (req, turn, st, sc, win) in enumerate(items):
        ne = len(turn["end_x"])
        assert res.n_feasible[k] == int((st == N_.SMP_C_FEASIBLE).sum())
        if win < 0:
            assert res.status[k] == N_.SMP_NONE_FEASIBLE
            continue
        assert res.status[k] == N_.SMP_OK
        assert tuple(res.winner[k]) == (win // ne, win % ne), (k, res.winner[k], win)
        assert res.score[k] == res.cand_score[k, win]
        i, j = win // ne, win % ne
        want = [turn["start_x"][i], turn["start"][1], turn["start"][2], turn["end_x"][j], turn["end"][1],
                turn["end"][2], abs(turn["start_x"][i] - turn["start"][0]), abs(turn["end_x"][j] - turn["end"][0])]
        assert np.array_equal(res.poses[k], np.array(want))


def test_python_functions_return_what_the_search_returns(tables):
    """The three reference-shaped functions (full lists at a coarse accuracy) against the host build's search of the
    same request through sample_result_tuple: the same tuples."""
    items, _ = tables
    fn = {"dubins": sfp.sample_start_end_pose_for_dubins, "reeds_shepp": sfp.sample_start_end_pose_for_reeds_shepp,
          "circle_back": sfp.sample_start_end_pose_for_circle_back}
    for k in (0, 3, 6):
        req = dict(items[k][0], accuracy=1.5)
        turn = sfp.sample_turn(**req)
        res = sh.sample_host(N_.SamplePacked([turn]))
        got = sfp.sample_result_tuple(turn, int(res.status[0]), res.poses[0])
        args = {a: b for a, b in req.items() if a != "type"}
        with sh.oracle_rs(), contextlib.redirect_stdout(io.StringIO()):
            want = fn[req["type"]](**args)
        assert (got is None) == (want is None)
        if want is not None:
            assert len(got) == 4
            for a, b in zip(got, want):
                assert np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), (k, got, want)


# ------------------------------------------------------------------ reference quirks, each pinned
def _blocked(req, over):
    """The request with one more blocker: the rectangle `over` = (x0, x1, y0, y1)."""
    rows = req["map_tree_rows"]
    env = orchard_environment_OBCA(rows, [], tree_width=0.3, headland_width=6.0)
    x0, x1, y0, y1 = over
    env.obs_poly_list = env.obs_poly_list + [Polygon(np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]]))]
    return dict(req, config_env=env)


def test_equal_x_values_tie_and_the_lower_index_wins(tables):
    items, _ = tables
    req, turn, st, sc, win = items[0]
    ne = len(turn["end_x"])
    i, j = win // ne, win % ne
    t2 = dict(turn, start_x=np.array([turn["start_x"][i]] * 2), end_x=np.array([turn["end_x"][j]] * 2))
    res = sh.sample_host(N_.SamplePacked([t2]))
    assert np.all(res.cand_status[0] == N_.SMP_C_FEASIBLE)
    assert len(set(res.cand_score[0].tolist())) == 1 and res.cand_score[0, 0] == sc[win]   # an exact four-way tie
    assert tuple(res.winner[0]) == (0, 0) and res.status[0] == N_.SMP_OK
    _, sc2, win2 = sh.np_tables(req, t2)
    assert win2 == 0 and len(set(sc2.tolist())) == 1


def test_a_blocker_over_the_entry_leaves_none_feasible(tables):
    items, _ = tables
    req, turn = items[0][0], items[0][1]
    y = turn["end"][1]
    req2 = dict(_blocked(req, (turn["end"][0] - 40.0, turn["end"][0] + 3.0, y - 0.5, y + 0.5)), accuracy=1.5)
    turn2 = sfp.sample_turn(**req2)
    res = sh.sample_host(N_.SamplePacked([turn2]))
    n = len(turn2["start_x"]) * len(turn2["end_x"])
    assert res.status[0] == N_.SMP_NONE_FEASIBLE and res.n_feasible[0] == 0 and tuple(res.winner[0]) == (-1, -1)
    assert np.all(res.cand_status[0, :n] == N_.SMP_C_BLOCKED) and np.isneginf(res.score[0])
    assert np.all(np.isnan(res.poses[0]))
    assert sfp.sample_result_tuple(turn2, int(res.status[0]), res.poses[0]) is None
    args = {a: b for a, b in req2.items() if a != "type"}
    assert sfp.sample_start_end_pose_for_dubins(**args) is None


def test_circle_back_takes_the_first_feasible_offset_and_the_exhausted_loop_its_last_pose(tables):
    items, _ = tables
    req, turn, st, sc, win = items[6]
    # the first offsets blocked by a rectangle just outside the start row end: the first feasible index is not 0
    s = turn["start"]
    args = {a: b for a, b in req.items() if a != "type"}
    for over, exhausted in (((s[0] - 2.2, s[0] - 1.2, s[1] - 0.2, s[1] + 0.2), False),
                            ((s[0] - 40.0, s[0] + 3.0, s[1] - 0.2, s[1] + 0.2), True)):
        req2 = dict(_blocked(req, over), accuracy=1.0)
        turn2 = sfp.sample_turn(**req2)
        assert len(turn2["start_x"]) == 5 and turn2["past"] == -5.0
        res = sh.sample_host(N_.SamplePacked([turn2]))
        cs = res.cand_status[0, :5]
        with contextlib.redirect_stdout(io.StringIO()):
            want = sfp.sample_start_end_pose_for_circle_back(**dict(args, config_env=req2["config_env"], accuracy=1.0))
        got = sfp.sample_result_tuple(turn2, int(res.status[0]), res.poses[0])
        if exhausted:
            assert res.status[0] == N_.SMP_NONE_FEASIBLE and not (cs == N_.SMP_C_FEASIBLE).any()
            assert tuple(res.winner[0]) == (4, 0)                      # the last candidate is reported
            assert want[2] == 5.0 and np.array_equal(want[0], s + np.array([-4.0, 0, 0]))   # the reference's tuple
        else:
            first = int(np.nonzero(cs == N_.SMP_C_FEASIBLE)[0][0])
            assert res.status[0] == N_.SMP_OK and first > 0 and tuple(res.winner[0]) == (first, 0)
            assert (cs == N_.SMP_C_FEASIBLE).sum() > 1                 # not the best one: the first one
        for a, b in zip(got, want):
            assert np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), (got, want)


@pytest.mark.parametrize("side", [map_utils.NEAR_SIDE, map_utils.FAR_SIDE])
def test_x_lists_are_the_references_arange(tables, side):
    items, _ = tables
    req = items[0][0]
    rows, car, acc = req["map_tree_rows"], req["car"], 0.2
    turn = sfp.sample_turn(**dict(req, side=side, accuracy=acc))
    sb = map_utils.get_base_pose(req["start_row_id"], rows, min_offset=0.0, side=side, pose_type=map_utils.LEAVE_POSE)
    eb = map_utils.get_base_pose(req["end_row_id"], rows, min_offset=0.0, side=side, pose_type=map_utils.ENTER_POSE)
    so = sfp.get_car_outmost_pose(rows, req["start_row_id"], sb[2], car, side=side, pose_type=map_utils.LEAVE_POSE)
    eo = sfp.get_car_outmost_pose(rows, req["end_row_id"], eb[2], car, side=side, pose_type=map_utils.ENTER_POSE)
    if side == map_utils.NEAR_SIDE:
        out = min(so[0], eo[0])
        ws, we = np.arange(sb[0], out - acc, -acc), np.arange(eb[0], out - acc, -acc)
    else:
        out = max(so[0], eo[0])
        ws, we = np.arange(sb[0], out + acc, acc), np.arange(eb[0], out + acc, acc)
    assert len(ws) > 3 and len(we) > 3
    assert np.array_equal(turn["start_x"], ws) and np.array_equal(turn["end_x"], we)
    assert np.array_equal(turn["start"], sb) and np.array_equal(turn["end"], eb)
    pk = N_.SamplePacked([turn])
    assert pk.n_start[0] == len(ws) and pk.n_end[0] == len(we) and pk.cap_cand == len(ws) * len(we)
    assert np.array_equal(pk.start_x[0, :len(ws)], ws) and np.array_equal(pk.end_x[0, :len(we)], we)


def test_implements_are_checked_at_every_second_row_only(tables):
    """A blocker that only the implement placed at one ODD row touches: get_path_poly places implements at rows
    0, 2, 4, ..., so the candidate stays feasible.  The implement is wider than the tractor, so its outer rear corner
    is the vehicle's outermost point in the turn and no other placed polygon covers the spot just inside it."""
    items, _ = tables
    req, turn, st, sc, win = items[0]
    car = CarModel(max_steer=0.55, wheel_base=1.9, axle_to_front=2.85, axle_to_back=0.55, width=1.48,
                   aux_poly_features=[[[-2.0, 1.5], 3.0, 1.0]], with_aux=True)
    ne = len(turn["end_x"])
    sx, ex = turn["start_x"][win // ne], turn["end_x"][win % ne]
    s = np.array([sx, turn["start"][1], turn["start"][2]])
    e = np.array([ex, turn["end"][1], turn["end"][2]])
    path = sfp.get_dubins_path_full(s, e, 1.0 / car.curvature)[:, :3]
    body = place(ring_of(car.car_poly), path)
    impl = place(ring_of(car.aux_polys[0]), path)
    spot = None
    for k in range(11, len(path) // 2, 2):
        for v in range(4):
            c = impl[k].mean(axis=0)
            p = impl[k, v] + 5e-4 * (c - impl[k, v]) / np.linalg.norm(c - impl[k, v])
            others = [body[r] for r in range(len(path))] + [impl[r] for r in range(0, len(path), 2)]
            if convex_contains_point(impl[k], p[0], p[1]) and not any(convex_contains_point(q, p[0], p[1]) for q in others):
                spot = (k, p)
                break
        if spot:
            break
    assert spot is not None
    k, p = spot
    h = 1e-4
    blocker = np.array([[p[0] - h, p[1] - h], [p[0] + h, p[1] - h], [p[0] + h, p[1] + h], [p[0] - h, p[1] + h]])
    hits_body = convex_intersects(body, blocker)
    hits_impl = convex_intersects(impl, blocker)
    assert k % 2 == 1 and hits_impl[k] and not hits_impl[0::2].any() and not hits_body.any()
    field = np.array([[p[0] - 60.0, p[1] - 60.0], [p[0] + 60.0, p[1] - 60.0], [p[0] + 60.0, p[1] + 60.0],
                      [p[0] - 60.0, p[1] + 60.0]])
    t2 = dict(turn, start_x=np.array([sx]), end_x=np.array([ex]), aux=[ring_of(car.aux_polys[0])],
              body=ring_of(car.car_poly), blockers=[blocker], field=field)
    res = sh.sample_host(N_.SamplePacked([t2]))
    assert res.cand_status[0, 0] == N_.SMP_C_FEASIBLE and res.status[0] == N_.SMP_OK
    # ... and it is the parity that saves it: the same blocker under an even row collides
    q = impl[k + 1].mean(axis=0)
    t3 = dict(t2, blockers=[blocker - p + q])
    assert sh.sample_host(N_.SamplePacked([t3])).cand_status[0, 0] == N_.SMP_C_BLOCKED


# ------------------------------------------------------------------ bad input
def _mixed(tables):
    items, _ = tables
    return [dict(items[k][1]) for k in (0, 3, 6, 1)]


def test_bad_sizes_and_null_pointers_are_refused(tables):
    pk = N_.SamplePacked(_mixed(tables))
    good = N_.SampleResults(pk)
    for field, value in (("cap_samples", 15), ("cap_cand", 0), ("cap_s", 0), ("cap_e", 0), ("batch", -1),
                         ("max_groups", -1), ("nvert", -1), ("params", None), ("desc", None), ("poly_off", None),
                         ("vertices", None), ("start_x", None), ("end_x", None), ("n_start", None), ("n_end", None)):
        b = pk.struct()
        setattr(b, field, value)
        rc, msg = sh.raw_call(b, good.struct())
        assert rc == -1 and msg.startswith("sample:"), (field, rc, msg)
    for field in ("status", "winner", "poses", "score", "n_feasible", "cand_score", "cand_status"):
        r = good.struct()
        setattr(r, field, None)
        rc, msg = sh.raw_call(pk.struct(), r)
        assert rc == -1 and msg.startswith("sample:"), (field, rc, msg)
    assert sh.raw_call(None, good.struct())[0] == -1 and sh.raw_call(pk.struct(), None)[0] == -1
    b = pk.struct()
    bad = pk.desc.copy()
    bad[1, 5] = len(pk.poly_off) + 3
    b.desc = bad.ctypes.data
    rc, msg = sh.raw_call(b, good.struct())
    assert rc == -1 and "polygon ids" in msg


def test_bad_turns_end_as_statuses_and_leave_the_others_intact(tables):
    turns = _mixed(tables)
    clean = sh.sample_host(N_.SamplePacked(turns))
    assert np.all(clean.status == N_.SMP_OK)
    # turn 1: NaN in the base pose; turn 2: n_start = 0; turn 0: a NaN among its x samples
    bad = [dict(t) for t in turns]
    bad[1]["start"] = np.array([bad[1]["start"][0], np.nan, bad[1]["start"][2]])
    bad[2]["start_x"] = np.zeros(0)
    bad[0]["start_x"] = np.array([turns[0]["start_x"][0], np.nan, *turns[0]["start_x"][2:]])
    res = sh.sample_host(N_.SamplePacked(bad, cap_s=4, cap_e=4, cap_cand=16))
    assert res.status[1] == N_.SMP_BAD_INPUT and res.status[2] == N_.SMP_BAD_INPUT
    assert np.all(res.cand_status[1] == N_.SMP_C_UNUSED) and np.all(res.cand_status[2] == N_.SMP_C_UNUSED)
    assert tuple(res.winner[1]) == (-1, -1) and res.n_feasible[2] == 0
    ne = len(turns[0]["end_x"])
    assert np.all(res.cand_status[0, ne:2 * ne] == N_.SMP_C_BAD_INPUT)
    keep = np.r_[0:ne, 2 * ne:len(turns[0]["start_x"]) * ne]
    assert np.array_equal(res.cand_status[0, keep], clean.cand_status[0, keep])
    assert np.array_equal(res.cand_score[0, keep], clean.cand_score[0, keep])
    for name in sh.NAMES:   # the healthy turn of the batch: bit for bit what the clean batch gave
        assert np.array_equal(getattr(res, name)[3], getattr(clean, name)[3], equal_nan=True), name
    # n_start * n_end over the table capacity: OVERFLOW for that turn alone
    res = sh.sample_host(N_.SamplePacked(turns, cap_cand=12))
    assert res.status[0] == N_.SMP_OVERFLOW and res.status[1] == N_.SMP_OVERFLOW   # 16 candidates each
    assert np.all(res.cand_status[0] == N_.SMP_C_UNUSED)
    for k in (2, 3):
        assert res.status[k] == clean.status[k] and np.array_equal(res.winner[k], clean.winner[k])
        assert res.score[k] == clean.score[k]
    # cap_samples too small for a Dubins path: a candidate status and a turn status, never a loop
    res = sh.sample_host(N_.SamplePacked(turns, cap_samples=16))
    assert res.status[0] == N_.SMP_OVERFLOW and res.status[3] == N_.SMP_OVERFLOW
    n = len(turns[0]["start_x"]) * len(turns[0]["end_x"])
    assert np.all(res.cand_status[0, :n] == N_.SMP_C_OVERFLOW)
    # unknown type, a body that is no quadrilateral
    bad = [dict(t) for t in turns]
    bad[3]["body"] = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    pk = N_.SamplePacked(bad)
    pk.params[2, 0] = 7
    res = sh.sample_host(pk)
    assert res.status[2] == N_.SMP_BAD_INPUT and res.status[3] == N_.SMP_BAD_INPUT
    for k in (0, 1):
        assert np.array_equal(res.cand_score[k], clean.cand_score[k]) and np.array_equal(res.winner[k], clean.winner[k])


def test_results_do_not_depend_on_the_tables(tables):
    turns = _mixed(tables)
    pk = N_.SamplePacked(turns)
    a, b = sh.sample_host(pk, tables=True), sh.sample_host(pk, tables=False)
    for name in ("status", "winner", "poses", "score", "n_feasible"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name


def test_sanitizer_program_builds_and_exits_zero():
    exe = sh.build_asan()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "all checks passed" in out.stdout

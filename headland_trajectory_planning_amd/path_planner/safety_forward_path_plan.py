"""Row-exit / row-enter offsets and Dubins forward turns of
R/path_planner/safety_forward_path_plan.py (host side; the footprint checks
are the reference's env.check_path_feasibility)."""
import math

import numpy as np

from ..obca_py.util import calc_spline_course
from . import dubins
from .map_utils import ENTER_POSE, FAR_SIDE, LEAVE_POSE, NEAR_SIDE, get_base_pose  # noqa: F401
from .navigation_utils import get_dubins_path


def get_dubins_turn_dirs(start_pose, end_pose, turning_radius):
    """:25-34."""
    configs, _ = dubins.shortest_path(start_pose, end_pose, turning_radius).sample_many(0.1)
    start_turn_dir = -1 if configs[0][2] > start_pose[2] else 1
    end_turn_dir = -1 if configs[-1][2] > end_pose[2] else 1
    return start_turn_dir, end_turn_dir


def get_steer_dir_for_enter_calculation(start_pose, end_pose):
    """:37-45."""
    if end_pose[1] - start_pose[1] > 0:
        return np.sign(1 * math.cos(start_pose[2]))
    return np.sign(-1 * math.cos(start_pose[2]))


def get_offset_pose(init_pose, pose_type, turn_out_dir, car, config_env, steer_angle=0.55,
                    delta_yaw=math.radians(45), max_offset=5, accuracy=0.1):
    """:248-283: first offset (0, 0.1, ...) whose 45-degree turn-out arc is collision free."""
    init_x, init_y, init_yaw = init_pose[0], init_pose[1], init_pose[2]
    motion_dir = -1 if pose_type == ENTER_POSE else 1
    offset_dir = -1 if pose_type == ENTER_POSE else 1
    for dist in np.arange(0, max_offset + accuracy, accuracy):
        x = init_x + dist * np.cos(init_yaw) * offset_dir
        y = init_y + dist * np.sin(init_yaw) * offset_dir
        pose = np.array([x, y, init_yaw])
        path = car.calculate_motion_path(pose, [steer_angle * turn_out_dir, motion_dir], delta_yaw, accuracy)
        if config_env.check_path_feasibility(car, path, boundary_check=False):
            break
    if dist >= max_offset:
        print("no solution is available!! dist: %.2f, x: %.2f" % (dist, x))
    return dist, pose, path


def get_offset_poses_for_row_traversing(start_leave_pose_base, end_enter_pose_base, car, config_env,
                                        max_steer_angle=0.55, plt=None):
    """:48-84."""
    turn_dir = get_steer_dir_for_enter_calculation(start_leave_pose_base, end_enter_pose_base)
    leave_dist, start_off, leave_path = get_offset_pose(start_leave_pose_base, LEAVE_POSE, turn_dir, car, config_env,
                                                        steer_angle=max_steer_angle)
    print("backward distance for leaving is %.2f" % (leave_dist))
    enter_dist, end_off, enter_path = get_offset_pose(end_enter_pose_base, ENTER_POSE, turn_dir, car, config_env,
                                                      steer_angle=max_steer_angle)
    print("backward distance for entering is %.2f" % (enter_dist))
    if plt is not None:
        plt.plot(leave_path[:, 0], leave_path[:, 1])
        plt.plot(enter_path[:, 0], enter_path[:, 1])
    return start_off, end_off


def get_dubins_path_full(pose_start, pose_end, turning_radius, step_size=0.1):
    """:286-297 (re-splined at the default ds = 0.1, as the reference does)."""
    cfg = get_dubins_path(pose_start, pose_end, turning_radius, step_size=step_size)
    rx, ry, ryaw, rk, _ = calc_spline_course(cfg[:, 0], cfg[:, 1])
    return np.vstack([rx, ry, ryaw, rk, np.ones_like(rx)]).T


# ---------------------------------------------------------------- classic turns
# Reeds-Shepp words come from the HIP drop-in (libhtp.so htp_rs_all_paths_batch);
# there is no host fallback.  Tests may swap `rs_curves` for the CPU restatement.
from .. import reeds_shepp as rs_curves  # noqa: E402
from .geom import polyline_buffer_intersects, ring_of  # noqa: E402


def filter_consecutive_duplicate(array):
    """:19-22 (element 0 is compared with the last one, as in the reference)."""
    return np.array([elem for i, elem in enumerate(array) if (elem - array[i - 1]).any()])


def get_car_outmost_pose(tree_rows, row_id, base_yaw, car, side=NEAR_SIDE, pose_type=ENTER_POSE):
    """:87-129: the pose whose footprint (body + implements on the near side) just clears the row ends."""
    lower, upper = tree_rows[row_id, :, :], tree_rows[row_id + 1, :, :]
    if side == NEAR_SIDE:
        lo_end, up_end = lower[0, :], upper[0, :]
        outmost_x = min(lo_end[0], up_end[0])
        min_x, max_x = car.car_poly.bounds[0], car.car_poly.bounds[2]
        for aux in car.aux_polys:
            min_x = min(min_x, aux.bounds[0])
            max_x = max(max_x, aux.bounds[2])
        off = abs(min_x) if pose_type == LEAVE_POSE else abs(max_x)
        return np.array([outmost_x - off, (lo_end[1] + up_end[1]) / 2, base_yaw])
    lo_end, up_end = lower[1, :], upper[1, :]
    outmost_x = max(lo_end[0], up_end[0])
    off = car.AXLE_TO_BACK if pose_type == LEAVE_POSE else car.AXLE_TO_FRONT
    return np.array([outmost_x + off, (lo_end[1] + up_end[1]) / 2, base_yaw])


def get_start_end_pose_for_dubins(map_tree_rows, start_row_id, end_row_id, car, config_env, max_steer_angle=0.55,
                                  plt=None, side=NEAR_SIDE, extra_offset_enter_dist=0.0, extra_offset_leave_dist=0.0):
    """:132-198: offset poses whose 45-degree turn-out arcs clear the rows, re-run until the
    Dubins word's first/last turn directions agree with the arcs' directions."""
    start_base = get_base_pose(start_row_id, map_tree_rows, extra_offset_leave_dist, side=side, pose_type=LEAVE_POSE)
    end_base = get_base_pose(end_row_id, map_tree_rows, extra_offset_enter_dist, side=side, pose_type=ENTER_POSE)
    turn_dir = get_steer_dir_for_enter_calculation(start_base, end_base)
    leave_dir = enter_dir = turn_dir
    while True:
        leave_offset, start_off, leave_path = get_offset_pose(start_base, LEAVE_POSE, leave_dir, car, config_env,
                                                              steer_angle=max_steer_angle)
        enter_offset, end_off, enter_path = get_offset_pose(end_base, ENTER_POSE, enter_dir, car, config_env,
                                                            steer_angle=max_steer_angle)
        s_dir, e_dir = get_dubins_turn_dirs(start_off, end_off, 1.0 / car.curvature)
        if s_dir == leave_dir and e_dir == enter_dir:
            break
        leave_dir, enter_dir = s_dir, e_dir
    if plt is not None:
        plt.plot(leave_path[:, 0], leave_path[:, 1])
        plt.plot(enter_path[:, 0], enter_path[:, 1])
    return start_off, end_off, leave_offset, enter_offset


def get_start_end_pose_for_reeds_shepp(map_tree_rows, start_row_id, end_row_id, car, config_env,
                                       max_steer_angle=0.55, plt=None, side=NEAR_SIDE, extra_offset_enter_dist=0.0,
                                       extra_offset_leave_dist=0.0):
    """:300-364: both offset poses moved to one outmost x.  As in the reference, that x is taken
    from the start BASE pose and the end OFFSET pose."""
    start_base = get_base_pose(start_row_id, map_tree_rows, extra_offset_leave_dist, side=side, pose_type=LEAVE_POSE)
    end_base = get_base_pose(end_row_id, map_tree_rows, extra_offset_enter_dist, side=side, pose_type=ENTER_POSE)
    turn_dir = get_steer_dir_for_enter_calculation(start_base, end_base)
    _, start_off, leave_path = get_offset_pose(start_base, LEAVE_POSE, turn_dir, car, config_env,
                                               steer_angle=max_steer_angle)
    _, end_off, enter_path = get_offset_pose(end_base, ENTER_POSE, turn_dir, car, config_env,
                                             steer_angle=max_steer_angle)
    if side == NEAR_SIDE:
        outmost_x = np.min([start_base[0], end_off[0]])
    else:
        outmost_x = np.max([start_base[0], end_off[0]])
    start_off[0] = outmost_x
    end_off[0] = outmost_x
    leave_offset = abs(outmost_x - start_base[0])
    enter_offset = abs(outmost_x - end_base[0])
    if plt is not None:
        plt.plot(leave_path[:, 0], leave_path[:, 1])
        plt.plot(enter_path[:, 0], enter_path[:, 1])
    return start_off, end_off, leave_offset, enter_offset


def _rs_rows(p):
    return np.array([p.x, p.y, p.yaw, p.cs, p.directions], dtype=np.float64).T


def get_all_reeds_shepp_paths_full(pose_start, pose_end, turning_radius, step_size=0.1):
    """:367-392: every Reeds-Shepp word as rows [x, y, yaw, curvature, direction]."""
    paths = rs_curves.calc_all_paths(pose_start[0], pose_start[1], pose_start[2], pose_end[0], pose_end[1],
                                     pose_end[2], 1.0 / turning_radius, step_size)
    return [_rs_rows(p) for p in paths]


def get_circle_back_path_full(pose_start, pose_end, turning_radius, car, side=NEAR_SIDE, step_size=0.1):
    """:395-454: forward arc (radius Rf, angle theta), backward arc (Rb, pi - theta), Dubins lead-in;
    both radii grow by 5 % until the backward arc stays clear of the end pose's x.  Rows wider
    than 2R fall back to the plain Dubins turn."""
    w = abs(pose_start[1] - pose_end[1])
    turning_radius = max(turning_radius, 1.0 / car.curvature)
    if w >= turning_radius * 2:
        return get_dubins_path_full(pose_start, pose_end, turning_radius, step_size)
    Rf = Rb = turning_radius
    while True:
        theta = np.pi / 2 + np.arcsin((Rb + w - Rf) / (Rf + Rb))
        if side == NEAR_SIDE and pose_start[0] - (Rf + Rb) * np.cos(theta - np.pi / 2) < pose_end[0] - step_size:
            break
        if side == FAR_SIDE and pose_start[0] + (Rf + Rb) * np.cos(theta - np.pi / 2) > pose_end[0] + step_size:
            break
        Rf *= 1.05
        Rb *= 1.05
    turn_dir = get_steer_dir_for_enter_calculation(pose_start, pose_end)
    forward = car.calculate_motion_path_new(init_pose=pose_start, motion_dir=1, steer_dir=turn_dir,
                                            turning_radius=Rf, delta_yaw=theta, step_size=step_size)
    back = car.calculate_motion_path_new(init_pose=forward[-1, :3], motion_dir=-1, steer_dir=-turn_dir,
                                         turning_radius=Rb, delta_yaw=np.pi - theta, step_size=step_size)
    straight = get_dubins_path_full(back[-1, :3], pose_end, turning_radius, step_size)
    return np.vstack([forward, back, straight])


def classic_circle_back_turning_path(start_exit_pose, end_enter_pose, map_env, car_model, step_size=0.1, plt=None):
    """:793-882: the Reeds-Shepp word with the least backward length among those whose 0.3 m
    flat-capped corridor misses every row/obstacle polygon, then shifted along the exit heading
    until the footprints clear the rows (boundary_check=False), with Dubins lead-in/out when moved.

    Reference behaviour kept: the shift loop tests the path BEFORE moving it, so the returned path
    sits one step past the first feasible one; with no clear word it raises IndexError
    (`feasible_paths[0]` on an empty list)."""
    to_goal = rs_curves.calc_all_paths(start_exit_pose[0], start_exit_pose[1], start_exit_pose[2],
                                       end_enter_pose[0], end_enter_pose[1], end_enter_pose[2],
                                       car_model.curvature, step_size)
    rings = [ring_of(p) for p in map_env.obs_poly_list]
    feasible = []
    for p in to_goal:
        xy = np.array([p.x, p.y], dtype=np.float64).T
        if not any(polyline_buffer_intersects(xy, 0.3, Q) for Q in rings):
            feasible.append(p)
    if len(feasible) == 0:
        raise IndexError("list index out of range")
    optimal, best = None, 99999
    for p in feasible:
        lengths = np.array(p.lengths)
        cost = np.abs(lengths[lengths < 0].sum())
        if cost < best:
            optimal, best = p, cost
    turning_path = _rs_rows(optimal)
    ok = map_env.check_path_feasibility(car_model, turning_path[:, :3], boundary_check=False)
    offset = 0
    shift = np.array([[step_size * np.cos(start_exit_pose[2]), step_size * np.sin(start_exit_pose[2])]])
    while not ok:
        ok = map_env.check_path_feasibility(car_model, turning_path[:, :3], boundary_check=False)
        if plt is not None:
            plt.plot(turning_path[:, 0], turning_path[:, 1], "--", c="black", alpha=0.5)
        offset += step_size
        turning_path[:, :2] += shift
    if offset > step_size:
        radius = 1.0 / car_model.curvature
        leave = get_dubins_path_full(start_exit_pose, turning_path[0, :3], radius)
        turning_path = np.vstack([leave[:-1], turning_path])
        enter = get_dubins_path_full(turning_path[-1, :3], end_enter_pose, radius)
        turning_path = np.vstack([turning_path, enter])
    return turning_path


# ---------------------------------------------------------------- sampled exit / entry poses (:457-790)
# The three sample_start_end_pose_for_* functions below are the reference's loops evaluated on the host, like the
# planners above; sample_start_end_pose_batch runs the same search for many turns in one launch of
# htp_classic_sample_batch (csrc/sample_core.h).
def _sample_x_lists(map_tree_rows, start_row_id, end_row_id, car, side, accuracy, extra_offset_enter_dist,
                    extra_offset_leave_dist):
    """:470-519 / :571-620: the base poses and the np.arange lists of exit / entry x values."""
    start_base = get_base_pose(start_row_id, map_tree_rows, min_offset=extra_offset_leave_dist, side=side,
                               pose_type=LEAVE_POSE)
    end_base = get_base_pose(end_row_id, map_tree_rows, min_offset=extra_offset_enter_dist, side=side,
                             pose_type=ENTER_POSE)
    start_out = get_car_outmost_pose(map_tree_rows, start_row_id, start_base[2], car, side=side, pose_type=LEAVE_POSE)
    end_out = get_car_outmost_pose(map_tree_rows, end_row_id, end_base[2], car, side=side, pose_type=ENTER_POSE)
    if side == NEAR_SIDE:
        outmost_x = min(start_out[0], end_out[0])
        start_xs = np.arange(start_base[0], outmost_x - accuracy, -accuracy)
        end_xs = np.arange(end_base[0], outmost_x - accuracy, -accuracy)
    else:
        outmost_x = max(start_out[0], end_out[0])
        start_xs = np.arange(start_base[0], outmost_x + accuracy, accuracy)
        end_xs = np.arange(end_base[0], outmost_x + accuracy, accuracy)
    return start_base, end_base, start_xs, end_xs


def sample_start_end_pose_for_dubins(map_tree_rows, start_row_id, end_row_id, car, config_env, max_steer_angle=0.55,
                                     plt=None, side=NEAR_SIDE, accuracy=0.2, extra_offset_enter_dist=0.0,
                                     extra_offset_leave_dist=0.0):
    """:457-555: every (exit x, entry x) pair; the feasible Dubins turn furthest inside the field boundary wins
    (strict >: the first of equal scores).  None when no pair is feasible."""
    start_base, end_base, start_xs, end_xs = _sample_x_lists(map_tree_rows, start_row_id, end_row_id, car, side,
                                                             accuracy, extra_offset_enter_dist,
                                                             extra_offset_leave_dist)
    results = None
    current = -np.inf
    for sx in start_xs:
        for ex in end_xs:
            safe_start = np.array([sx, start_base[1], start_base[2]])
            safe_end = np.array([ex, end_base[1], end_base[2]])
            try:
                path = get_dubins_path_full(safe_start, safe_end, 1.0 / car.curvature)
            except (ValueError, IndexError, ZeroDivisionError):
                path = None   # the reference's `turning_path is None`
            if path is None:
                continue
            if config_env.check_path_feasibility(car, path[:, :3], boundary_check=False, aux_check=True):
                dist = config_env.get_min_distance_to_boundary(car, path[:, :3], with_aux=True)
                if dist > current:
                    current = dist
                    results = (safe_start, safe_end, abs(sx - start_base[0]), abs(ex - end_base[0]))
    return results


def sample_start_end_pose_for_reeds_shepp(map_tree_rows, start_row_id, end_row_id, car, config_env,
                                          max_steer_angle=0.55, plt=None, side=NEAR_SIDE, accuracy=0.2,
                                          extra_offset_enter_dist=0.0, extra_offset_leave_dist=0.0):
    """:558-656: as the Dubins variant, a pair scoring the best of its feasible Reeds-Shepp words."""
    start_base, end_base, start_xs, end_xs = _sample_x_lists(map_tree_rows, start_row_id, end_row_id, car, side,
                                                             accuracy, extra_offset_enter_dist,
                                                             extra_offset_leave_dist)
    results = None
    current = -np.inf
    for sx in start_xs:
        for ex in end_xs:
            safe_start = np.array([sx, start_base[1], start_base[2]])
            safe_end = np.array([ex, end_base[1], end_base[2]])
            paths = get_all_reeds_shepp_paths_full(safe_start, safe_end, 1.0 / car.curvature)
            best = -np.inf
            if len(paths) == 0:
                continue
            for path in paths:
                if config_env.check_path_feasibility(car, path[:, :3], boundary_check=False, aux_check=True):
                    dist = config_env.get_min_distance_to_boundary(car, path[:, :3], with_aux=True)
                    if dist > best:
                        best = dist
            if best > current:
                current = best
                results = (safe_start, safe_end, abs(sx - start_base[0]), abs(ex - end_base[0]))
    return results


def get_start_end_pose(map_tree_rows, start_row_id, end_row_id, side=NEAR_SIDE, extra_offset_enter_dist=0.4,
                       extra_offset_leave_dist=1.1):
    """:659-730: exit / entry poses at the outermost of the two row ends, moved out along the row heading."""
    N, M = start_row_id, end_row_id
    near_start = [(map_tree_rows[N, 0, 0] + map_tree_rows[N + 1, 0, 0]) / 2,
                  (map_tree_rows[N, 0, 1] + map_tree_rows[N + 1, 0, 1]) / 2]
    far_start = [(map_tree_rows[N, 1, 0] + map_tree_rows[N + 1, 1, 0]) / 2,
                 (map_tree_rows[N, 1, 1] + map_tree_rows[N + 1, 1, 1]) / 2]
    near_end = [(map_tree_rows[M, 0, 0] + map_tree_rows[M + 1, 0, 0]) / 2,
                (map_tree_rows[M, 0, 1] + map_tree_rows[M + 1, 0, 1]) / 2]
    far_end = [(map_tree_rows[M, 1, 0] + map_tree_rows[M + 1, 1, 0]) / 2,
               (map_tree_rows[M, 1, 1] + map_tree_rows[M + 1, 1, 1]) / 2]
    start_row_yaw = np.arctan2(far_start[1] - near_start[1], far_start[0] - near_start[0])
    end_row_yaw = np.arctan2(far_end[1] - near_end[1], far_end[0] - near_end[0])
    if side == NEAR_SIDE:
        start_x = min(map_tree_rows[N, 0, 0], map_tree_rows[N + 1, 0, 0])
        start_y = (map_tree_rows[N, 0, 1] + map_tree_rows[N + 1, 0, 1]) / 2
        start_pose = [start_x - extra_offset_leave_dist * np.cos(start_row_yaw),
                      start_y - extra_offset_leave_dist * np.sin(start_row_yaw), np.pi + start_row_yaw]
        end_x = min(map_tree_rows[M, 0, 0], map_tree_rows[M + 1, 0, 0])
        end_y = (map_tree_rows[M, 0, 1] + map_tree_rows[M + 1, 0, 1]) / 2
        end_pose = [end_x - extra_offset_enter_dist * np.cos(end_row_yaw),
                    end_y - extra_offset_enter_dist * np.sin(end_row_yaw), end_row_yaw]
    if side == FAR_SIDE:
        start_x = max(map_tree_rows[N, 1, 0], map_tree_rows[N + 1, 1, 0])
        start_y = (map_tree_rows[N, 1, 1] + map_tree_rows[N + 1, 1, 1]) / 2
        start_pose = [start_x + extra_offset_leave_dist * np.cos(start_row_yaw),
                      start_y + extra_offset_leave_dist * np.sin(start_row_yaw), start_row_yaw]
        end_x = max(map_tree_rows[M, 1, 0], map_tree_rows[M + 1, 1, 0])
        end_y = (map_tree_rows[M, 1, 1] + map_tree_rows[M + 1, 1, 1]) / 2
        end_pose = [end_x + extra_offset_enter_dist * np.cos(end_row_yaw),
                    end_y + extra_offset_enter_dist * np.sin(end_row_yaw), end_row_yaw + np.pi]
    return start_pose, end_pose


def _circle_back_offsets(side, accuracy):
    """:770-787: the offsets the while loop visits (accumulated by repeated addition, as the reference does) and
    the offset it holds once exhausted."""
    if not accuracy > 0:
        raise ValueError("accuracy must be positive (the reference's loop would not end)")
    step = -accuracy if side == NEAR_SIDE else accuracy
    offsets, current = [], 0.0
    while abs(current) < 5:
        offsets.append(current)
        current += step
    return np.array(offsets), current


def sample_start_end_pose_for_circle_back(map_tree_rows, start_row_id, end_row_id, car, config_env,
                                          max_steer_angle=0.55, plt=None, side=NEAR_SIDE, accuracy=0.2,
                                          extra_offset_enter_dist=0.0, extra_offset_leave_dist=0.0):
    """:733-790: the exit pose moved outwards in steps of `accuracy` until the circle-back turn clears the rows.
    Reference behaviour kept: when no offset below 5 m is feasible, the last pose tried is returned with the offset
    the loop holds after it."""
    start_base, end_base = get_start_end_pose(map_tree_rows, start_row_id, end_row_id, side,
                                              extra_offset_enter_dist, extra_offset_leave_dist)
    offsets, past = _circle_back_offsets(side, accuracy)
    current = past
    for off in offsets:
        start_off = start_base + np.array([off, 0, 0])
        path = get_circle_back_path_full(start_off, end_base, 1.0 / car.curvature, car, side)
        if config_env.check_path_feasibility(car, path[:, :3], boundary_check=False, aux_check=True):
            current = off
            break
    return (start_off, end_base, abs(current), 0.0)


SAMPLE_TYPES = ("dubins", "reeds_shepp", "circle_back")


def sample_turn(map_tree_rows, start_row_id, end_row_id, car, config_env, side=NEAR_SIDE, type="dubins",
                accuracy=0.2, extra_offset_enter_dist=0.0, extra_offset_leave_dist=0.0):
    """One request of sample_start_end_pose_batch as the device search takes it (_native.SamplePacked): base poses,
    the x lists built exactly as the host functions build them, car, polygons.  `past` is the circle-back loop's
    offset once exhausted."""
    if type not in SAMPLE_TYPES:
        raise ValueError("unknown sampling type %r" % (type,))
    past = 0.0
    if type == "circle_back":
        start_base, end_base = get_start_end_pose(map_tree_rows, start_row_id, end_row_id, side,
                                                  extra_offset_enter_dist, extra_offset_leave_dist)
        start_base, end_base = np.array(start_base, dtype=np.float64), np.array(end_base, dtype=np.float64)
        offsets, past = _circle_back_offsets(side, accuracy)
        start_xs = np.array([(start_base + np.array([off, 0, 0]))[0] for off in offsets])
        end_xs = np.array([end_base[0]])
    else:
        start_base, end_base, start_xs, end_xs = _sample_x_lists(map_tree_rows, start_row_id, end_row_id, car, side,
                                                                 accuracy, extra_offset_enter_dist,
                                                                 extra_offset_leave_dist)
    return dict(type=type, side=side, start=start_base, end=end_base, start_x=start_xs, end_x=end_xs,
                wheel_base=car.WHEEL_BASE, max_steer=car.MAX_STEER, radius=1.0 / car.curvature, step=0.1,
                body=ring_of(car.car_poly), aux=[ring_of(a) for a in car.aux_polys],
                blockers=[ring_of(q) for q in config_env.obs_poly_list], field=ring_of(config_env.field_range_poly),
                past=past)


def sample_result_tuple(turn, status, poses):
    """The reference's return value of one searched turn from the device outputs (status, poses[8])."""
    from .. import _native
    if turn["type"] == "circle_back":
        offset = poses[6] if status == _native.SMP_OK else abs(turn["past"])
        return (np.array(poses[0:3]), np.array(turn["end"], dtype=np.float64), float(offset), 0.0)
    if status != _native.SMP_OK:
        return None
    return (np.array(poses[0:3]), np.array(poses[3:6]), float(poses[6]), float(poses[7]))


def sample_start_end_pose_batch(requests, device=None, **opts):
    """The sampled pose search for many turns in one launch.  A request is a dict with the arguments of the
    sample_start_end_pose_for_* functions: map_tree_rows, start_row_id, end_row_id, car, config_env, and optionally
    side, type ("dubins" / "reeds_shepp" / "circle_back"), accuracy, extra_offset_enter_dist,
    extra_offset_leave_dist.  Returns, per request, what the function of its type returns (a tuple, or None).
    `device`: a _native.Context, a device index, or None for device 0.  A turn the kernel could not search (overflow,
    bad input) raises."""
    from .. import _native
    turns = [sample_turn(**r) for r in requests]
    if not turns:
        return []
    ctx = device if isinstance(device, _native.Context) else _native.Context(0 if device is None else int(device))
    res = ctx.classic_sample(_native.SamplePacked(turns, **opts), tables=False)
    out = []
    for k, t in enumerate(turns):
        st = int(res.status[k])
        if st not in (_native.SMP_OK, _native.SMP_NONE_FEASIBLE):
            raise RuntimeError("[htp] sampled pose search: turn %d ended %s" % (k, _native.SMP_STATUS[st]))
        out.append(sample_result_tuple(t, st, res.poses[k]))
    return out


# ------------------------------------------------------------------ speed profile and timed trajectory of a path
SPEED_KINDS = ("stop", "vmax", "alat", "steer_rate", "endpoint", "acc", "dec")
SPEED_LIMIT_DEFAULTS = dict(v_fwd=1.0, v_rev=1.0, acc=1.0, dec=1.0, a_lat=0.0, steer_rate=0.7, v0=0.0, v1=0.0)


def speed_limits(car, **limits):
    """The limits row of one path (include/htp.h HTP_SPD_L_*): wheelbase and max_steer from the car, the rest from
    `limits` over synth's values (max_velocity 1, max_accel 1, max_steer_rate 0.7), so a classic turn and an OBCA turn
    are timed under the same limits.  wheel_base / max_steer in `limits` override the car's."""
    for k in limits:
        if k not in SPEED_LIMIT_DEFAULTS and k not in ("wheel_base", "max_steer"):
            raise TypeError("speed_profile: unknown limit %r" % (k,))
    m = dict(SPEED_LIMIT_DEFAULTS, **limits)
    wb = m.get("wheel_base", getattr(car, "WHEEL_BASE", None))
    ms = m.get("max_steer", getattr(car, "MAX_STEER", None))
    return np.array([wb, m["v_fwd"], m["v_rev"], m["acc"], m["dec"], m["a_lat"], m["steer_rate"], ms, m["v0"],
                     m["v1"]], dtype=np.float64)


def _speed_interval(wi, wj, ds, dd, acc, dec, omega):
    """(dt, a, kind, t1, vm) of one interval; kind 0 ramp, 1 dwell, 2 hop."""
    vi, vj = math.sqrt(wi), math.sqrt(wj)
    if ds == 0.0:
        return (abs(dd) / omega if omega > 0.0 and dd != 0.0 else 0.0), 0.0, 1, 0.0, 0.0
    if vi + vj > 0.0:
        return 2.0 * ds / (vi + vj), (wj - wi) / (2.0 * ds), 0, 0.0, 0.0
    vm = math.sqrt(2.0 * acc * dec * ds / (acc + dec))
    t1 = vm / acc
    return t1 + vm / dec, acc, 2, t1, vm


def speed_profile(path, car, dt=0.0, cap_rows=None, libm=None, **limits):
    """The maximal speed profile of one path (rows x, y, yaw, k, dir) as include/htp.h defines it, in plain numpy with
    sequential recurrences: the statement the batched kernel is tested against.  Returns a dict: status ("ok" /
    "bad_input"), S, t, v (signed), accel, steer, steer_rate, cap, w, active [n], T, length, len_fwd, len_rev, stops,
    stop_nodes, dwell, peak_v, peak_lat, max_steer, time_kind [7], flags (set of "hop", "steer_exceeds", "truncated",
    "bad_time"), count and, with dt > 0, rows [min(count, cap_rows)][10] and stage.  `libm`: an object with atan and
    hypot (default: math); the tests pass the project's correctly rounded ones, which the kernel uses."""
    lm = math if libm is None else libm
    lim = speed_limits(car, **limits)
    L, vf, vr, acc, dec, alat, omega, max_steer, v0, v1 = [float(x) for x in lim]
    P = np.asarray(path, dtype=np.float64)
    bad = P.ndim != 2 or P.shape[0] < 2 or P.shape[1] < 5 or not np.all(np.isfinite(lim))
    bad = bad or not np.all(np.isfinite(P[:, :5])) or not np.all(np.abs(P[:, 4]) == 1.0)
    bad = bad or not (L > 0 and vf > 0 and vr > 0 and acc > 0 and dec > 0) or alat < 0 or omega < 0 or v0 < 0 or v1 < 0
    if bad:
        return dict(status="bad_input", count=0, flags=set())
    n = len(P)
    x, y, yaw, k, d = P[:, 0], P[:, 1], P[:, 2], P[:, 3], P[:, 4]
    ds = np.array([lm.hypot(x[i + 1] - x[i], y[i + 1] - y[i]) for i in range(n - 1)])
    S = np.concatenate([[0.0], np.cumsum(ds)])
    dl = np.array([lm.atan(L * k[i]) for i in range(n)])
    ddl = dl[1:] - dl[:-1]
    stop = np.zeros(n, bool)
    stop[:-1] = d[1:] != d[:-1]
    inf = math.inf
    c = np.zeros(n)
    kind = np.zeros(n, np.int32)
    for i in range(n):
        vmax, sr, endp = inf, inf, inf
        if i > 0:
            vmax = vf if d[i] > 0 else vr
            if omega > 0.0 and ddl[i - 1] != 0.0:
                sr = omega * ds[i - 1] / abs(ddl[i - 1])
        if i < n - 1:
            vmax = min(vmax, vf if d[i + 1] > 0 else vr)
            if omega > 0.0 and ddl[i] != 0.0:
                sr = min(sr, omega * ds[i] / abs(ddl[i]))
        al = math.sqrt(alat / abs(k[i])) if alat > 0.0 and k[i] != 0.0 else inf
        if i == 0:
            endp = v0
        if i == n - 1:
            endp = min(endp, v1)
        cands = [0.0 if stop[i] else inf, vmax, al, sr, endp]
        c[i] = min(cands)
        kind[i] = cands.index(c[i])
    c2 = c * c
    f = np.zeros(n)
    fb = np.full(n, inf)           # the forward bound of node i
    f[0] = c2[0]
    for i in range(n - 1):
        fb[i + 1] = f[i] + 2.0 * acc * ds[i]
        f[i + 1] = min(c2[i + 1], fb[i + 1])
    w = f.copy()
    bb = np.full(n, inf)           # the backward bound
    for i in range(n - 2, -1, -1):
        bb[i] = w[i + 1] + 2.0 * dec * ds[i]
        w[i] = min(f[i], bb[i])
    active = np.where(w == c2, kind, np.where(fb < bb, 5, 6)).astype(np.int32)
    iv = [_speed_interval(w[i], w[i + 1], ds[i], ddl[i], acc, dec, omega) for i in range(n - 1)]
    dts = np.array([q[0] for q in iv])
    t = np.concatenate([[0.0], np.cumsum(dts)])
    T = float(t[-1])
    g = np.concatenate([d[1:], d[-1:]])
    v = np.sqrt(w)
    a = np.array([q[1] for q in iv] + [0.0])
    rate = np.array([ddl[i] / dts[i] if dts[i] > 0.0 else 0.0 for i in range(n - 1)] + [0.0])
    len_f = len_r = dwell = 0.0
    tk = [0.0] * len(SPEED_KINDS)
    for i in range(n - 1):
        if d[i + 1] > 0:
            len_f += ds[i]
        else:
            len_r += ds[i]
        if iv[i][2] == 1:
            dwell += dts[i]
        tk[active[i]] += dts[i]
    hops = [q[4] for q in iv if q[2] == 2]
    flags = set()
    if hops:
        flags.add("hop")
    if np.max(np.abs(dl)) > max_steer:
        flags.add("steer_exceeds")
    out = dict(status="ok", S=S, t=t, v=g * v, accel=g * a, steer=dl, steer_rate=rate, cap=c, w=w, active=active,
               T=T, length=float(S[-1]), len_fwd=len_f, len_rev=len_r, stops=int(stop.sum()),
               stop_nodes=np.nonzero(stop)[0], dwell=dwell, peak_v=float(max([np.max(v)] + hops)),
               peak_lat=float(np.max(w * np.abs(k))), max_steer=float(np.max(np.abs(dl))), time_kind=np.array(tk),
               flags=flags, count=0)
    if dt > 0.0:
        quot = T / dt
        if not quot < 2.0 ** 30:
            flags.add("bad_time")
            return out
        nr = int(quot)
        while nr > 0 and (nr - 1) * dt >= T:
            nr -= 1
        while nr * dt < T:
            nr += 1
        out["count"] = nr + 1
        cap_rows = nr + 1 if cap_rows is None else int(cap_rows)
        if nr + 1 > cap_rows:
            flags.add("truncated")
        rows, stage = [], []
        for r in range(min(nr + 1, cap_rows)):
            if r == nr:
                q = iv[n - 2]
                rows.append([T, x[-1], y[-1], d[-1] * v[-1], yaw[-1], dl[-1], d[-1] * (-dec if q[2] == 2 else q[1]),
                             rate[n - 2], k[-1], S[-1]])
                stage.append(n - 1)
                continue
            s = r * dt
            i = int(np.searchsorted(t[:n - 1], s, side="right")) - 1
            dti, ai, kd, t1, vm = iv[i]
            tau = s - t[i]
            dist = vel = ac = 0.0
            if kd == 1:
                lam = tau / dti
            else:
                if kd == 0:
                    dist = v[i] * tau + 0.5 * ai * tau * tau
                    vel, ac = v[i] + ai * tau, ai
                elif tau < t1:
                    dist, vel, ac = 0.5 * acc * tau * tau, acc * tau, acc
                else:
                    t2 = tau - t1
                    dist = 0.5 * acc * t1 * t1 + vm * t2 - 0.5 * dec * t2 * t2
                    vel, ac = vm - dec * t2, -dec
                lam = dist / ds[i]
            lam = min(max(lam, 0.0), 1.0)
            dy = yaw[i + 1] - yaw[i]
            kk = k[i] + lam * (k[i + 1] - k[i])
            rows.append([s, x[i] + lam * (x[i + 1] - x[i]), y[i] + lam * (y[i + 1] - y[i]), d[i + 1] * vel,
                         yaw[i] + lam * (dy - 2.0 * math.pi * math.floor((dy + math.pi) / (2.0 * math.pi))),
                         lm.atan(L * kk), d[i + 1] * ac, rate[i], kk, S[i] + dist])
            stage.append(i)
        out["rows"] = np.array(rows).reshape(-1, 10)
        out["stage"] = np.array(stage, np.int32)
    return out


def speed_profile_batch(paths, car, device=None, dt=0.0, cap_rows=None, status=None, **limits):
    """The speed profile of many paths in one launch (htp_speed_profile_batch) -> _native.SpeedResults.  `paths`: a list
    of [n][5] arrays; `status`: optional per-path planner status, non-zero paths are skipped; `limits` as
    speed_profile (one set for the batch).  `device`: a _native.Context, a device index, or None for device 0."""
    from .. import _native
    ctx = device if isinstance(device, _native.Context) else _native.Context(0 if device is None else int(device))
    packed = _native.SpeedPacked(paths, [speed_limits(car, **limits)] * len(paths), dt=dt, cap_rows=cap_rows,
                                 status=status)
    return ctx.speed_profile(packed)


# ------------------------------------------------------------------ clearance of a pose sequence, best classic turn
def _polygon_vertices(poly):
    """Counter-clockwise vertices of a convex polygon given as vertices [m, 2] or as halfspaces (A [e, 2], b [e]) with
    rows of any order, possibly redundant -> [m, 2], or None when the halfspaces are empty, unbounded or degenerate."""
    if not isinstance(poly, tuple):
        v = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
        d, e = np.roll(v, -1, axis=0) - v, np.roll(v, -2, axis=0) - np.roll(v, -1, axis=0)
        return v if np.sum(d[:, 0] * e[:, 1] - d[:, 1] * e[:, 0]) > 0 else v[::-1].copy()
    A, b = np.asarray(poly[0], dtype=np.float64).reshape(-1, 2), np.asarray(poly[1], dtype=np.float64).reshape(-1)
    nrm = np.hypot(A[:, 0], A[:, 1])
    if not np.all(nrm > 0.0):
        return None
    A, b = A / nrm[:, None], b / nrm
    ang = np.sort(np.arctan2(A[:, 1], A[:, 0]))
    if len(ang) < 3 or np.max(np.diff(np.concatenate([ang, ang[:1] + 2.0 * math.pi]))) >= math.pi - 1e-9:
        return None                                   # the normals leave a half plane open: unbounded (or empty)
    pts = []
    for i in range(len(b)):
        for j in range(i + 1, len(b)):
            det = A[i, 0] * A[j, 1] - A[i, 1] * A[j, 0]
            if abs(det) <= 1e-12:
                continue
            p = np.array([(b[i] * A[j, 1] - b[j] * A[i, 1]) / det, (A[i, 0] * b[j] - A[j, 0] * b[i]) / det])
            if np.all(A @ p <= b + 1e-9) and not any(np.hypot(*(p - q)) <= 1e-9 for q in pts):
                pts.append(p)
    if len(pts) < 3:
        return None
    pts = np.array(pts)
    c = pts.mean(axis=0)
    return pts[np.argsort(np.arctan2(pts[:, 1] - c[1], pts[:, 0] - c[0]))]


def _polygon_signed_distance(P, Q):
    """Signed distance of two convex counter-clockwise polygons: the largest, over the edge normals of both, of the
    least projection gap; when that is positive they are disjoint and the distance is the least vertex-to-edge
    distance over both directions, otherwise it is minus the penetration depth."""
    sep, d2 = -math.inf, math.inf
    for F, V in ((P, Q), (Q, P)):
        e = np.roll(F, -1, axis=0) - F
        ln = np.hypot(e[:, 0], e[:, 1])
        u = e / ln[:, None]
        nrm = np.stack([u[:, 1], -u[:, 0]], axis=1)       # outward normals of a counter-clockwise polygon
        w = V[None, :, :] - F[:, None, :]                 # [edge, vertex, 2]
        pr = np.einsum("evk,ek->ev", w, nrm)
        al = np.einsum("evk,ek->ev", w, u)
        ex = np.maximum(np.maximum(-al, al - ln[:, None]), 0.0)
        sep = max(sep, float(np.max(np.min(pr, axis=1))))
        d2 = min(d2, float(np.min(pr * pr + ex * ex)))
    return math.sqrt(d2) if sep > 0.0 else sep


def pose_clearance(poses, obstacles, bodies, substeps=1, margin=None, libm=None, margin_tol=0.0):
    """The clearance of one pose sequence (rows x, y, yaw) against obstacle polygons, with the body polygons placed at
    every pose, as include/htp.h defines it ("Clearance of pose sequences"), in plain numpy: the statement the batched
    kernel is tested against.  obstacles / bodies: lists of vertices [m, 2] or of halfspaces (A, b).  Returns a dict:
    status ("ok" / "bad_input" / "bad_polytope"), clearance, clearance_node, max_gap, max_turn, worst (pose, substep,
    obstacle, body), pose_clearance [n], flags (set of "collision", "margin"), runner_up (test support: the least
    signed distance of an item that is greater than the clearance, i.e. how far `worst` is from a tie, so that the tests
    can draw scenes whose `worst` is decidable).  margin_tol is the kernel's option of that name.  `libm`: an object with sin, cos and
    hypot (default: math); the tests pass the project's correctly rounded ones, which the kernel uses."""
    lm = math if libm is None else libm
    P = np.asarray(poses, dtype=np.float64)
    S = int(substeps)
    if P.ndim != 2 or P.shape[0] < 1 or P.shape[1] < 3 or not np.all(np.isfinite(P[:, :3])):
        return dict(status="bad_input", flags=set())
    if margin is not None and not math.isfinite(margin):
        return dict(status="bad_input", flags=set())
    for poly in list(obstacles) + list(bodies):
        if isinstance(poly, tuple) and not (np.all(np.isfinite(poly[0])) and np.all(np.isfinite(poly[1]))):
            return dict(status="bad_input", flags=set())
    obs = [_polygon_vertices(o) for o in obstacles]
    bod = [_polygon_vertices(o) for o in bodies]
    if any(o is None for o in obs + bod):
        return dict(status="bad_polytope", flags=set())
    n = len(P)
    x, y, yaw = P[:, 0], P[:, 1], P[:, 2]
    best, node, worst = math.inf, math.inf, None
    gap = turn = 0.0
    per_pose = np.full(n, math.inf)
    every = []
    for i in range(n):
        dx = dy = dw = 0.0
        if i < n - 1:
            dx, dy, d = x[i + 1] - x[i], y[i + 1] - y[i], yaw[i + 1] - yaw[i]
            dw = d - 2.0 * math.pi * math.floor((d + math.pi) / (2.0 * math.pi))
            gap = max(gap, lm.hypot(dx, dy))
            turn = max(turn, abs(dw))
        for q in range(S if i < n - 1 else 1):
            lam = float(q) / float(S)
            px, py, pw = (x[i] + lam * dx, y[i] + lam * dy, yaw[i] + lam * dw) if q else (x[i], y[i], yaw[i])
            cs, sn = lm.cos(pw), lm.sin(pw)
            R = np.array([[cs, sn], [-sn, cs]])
            for m, O in enumerate(obs):
                for k, Bk in enumerate(bod):
                    d = _polygon_signed_distance(O, Bk @ R + [px, py])
                    every.append(d)
                    if d < best:
                        best, worst = d, (i, q, m, k)
                    if q == 0:
                        node = min(node, d)
                    per_pose[i] = min(per_pose[i], d)
    flags = set()
    if best < 0.0:
        flags.add("collision")
    if margin is not None and best < margin - margin_tol:
        flags.add("margin")
    return dict(status="ok", clearance=best, clearance_node=node, max_gap=gap, max_turn=turn, worst=worst,
                pose_clearance=per_pose, flags=flags, runner_up=min([v for v in every if v > best], default=math.inf))


def classic_turn_portfolio(packed, turns, car, types=("dubins", "circleback", "fishtail"), device=None, dt=0.1,
                           cap_rows=None, substeps=2, reject_steer_exceeds=True, cap_path=1024, **limits):
    """Per headland, the fastest classic turn that clears the obstacle set the solve is held to.  `packed`: the
    _native.PackedBatch the solve takes (its obstacles, bodies and min_dist as margin); `turns`: one ClassicPacked dict
    per problem (synth.classic_turn(meta)); every problem is planned as each of `types`: all C B turns in one
    htp_classic_turn_batch_device launch (candidate c of problem b at index c B + b), then the speed profile, the
    clearance of the planner's paths and the selection behind it on the same stream, with no host round trip between
    the launches.  A candidate that collides or misses the margin is rejected, and one that exceeds the steering bound
    unless reject_steer_exceeds is off; `limits` as speed_profile.  Returns a dict: types, winner [B] (index into
    types, -1: none), winner_type [B], T [B], clearance [B], rows (list of [count][10]), verdict [B, C], and per
    candidate [C, B] T_all, clearance_all, speed_status, clear_status, clear_flags, speed_flags; select is the
    _native.SelectResults behind winner, T, clearance and rows.  cap_path: rows of storage per planned turn."""
    import torch

    from .. import _native as N_
    ctx = device if isinstance(device, N_.Context) else N_.Context(0 if device is None else int(device))
    B, C = packed.batch, len(types)
    if len(turns) != B:
        raise ValueError("classic_turn_portfolio: one turn per problem of the batch")
    dev = torch.device("cuda", ctx.device)
    ck = N_.ClassicPacked([dict(t, type=typ) for typ in types for t in turns], cap_path=cap_path)
    sk = N_.SpeedPacked.resident(C * B, ck.cap_path, speed_limits(car, **limits), dt=dt, cap_rows=cap_rows)
    lk = N_.ClearPacked.resident(C * B, ck.cap_path, (packed.obs_edges, packed.body_edges), B,
                                 substeps=substeps, **N_.CLR_PATH_LAYOUT)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    t_in = {k: up(getattr(ck, k)) for k in ("params", "desc", "poly_off", "vertices")}
    t_sc = {k: up(getattr(packed, k)) for k in N_.CLR_SCENE_ARRAYS}
    t_sc.update(limits=up(sk.limits), scene=up(np.tile(np.arange(B, dtype=np.int32), C)),
                margin=up(packed.params[:, N_.P_DMIN]))
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)   # noqa: E731
    i32 = torch.int32
    t_turn = {"status": z(C * B, dtype=i32), "n_path": z(C * B, dtype=i32), "path": z(C * B, ck.cap_path, 5)}
    t_spd = {"status": z(C * B, dtype=i32), "flags": z(C * B, dtype=i32), "summary": z(C * B, N_.SPD_NSUM),
             "count": z(C * B, dtype=i32)}
    if sk.dt > 0.0:
        t_spd["rows"] = z(C * B, sk.cap_rows, 10)
    t_clr = {"status": z(C * B, dtype=i32), "flags": z(C * B, dtype=i32), "metrics": z(C * B, N_.CLR_NMETRIC),
             "worst": z(C * B, 4, dtype=i32)}
    sel = N_.SelectResults(B, C, sk.cap_rows if sk.dt > 0.0 else 0)
    t_sel = {k: up(getattr(sel, k)) for k in ("verdict", "winner", "score", "clearance", "out_rows", "out_count")
             if getattr(sel, k) is not None}
    ptr = lambda d: {k: v.data_ptr() for k, v in d.items()}   # noqa: E731
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    ctx.classic_turns_device(ck, ptr(t_in), ptr(t_turn), stream=s)
    ctx.speed_profile_device(sk, {"path": t_turn["path"].data_ptr(), "n_path": t_turn["n_path"].data_ptr(),
                                  "path_status": t_turn["status"].data_ptr(), "limits": t_sc["limits"].data_ptr()},
                             ptr(t_spd), stream=s)
    ctx.pose_clearance_device(lk, dict(ptr({k: t_sc[k] for k in N_.CLR_SCENE_ARRAYS + ("scene", "margin")}),
                                       poses=t_turn["path"].data_ptr(), n_poses=t_turn["n_path"].data_ptr(),
                                       pose_status=t_turn["status"].data_ptr()), ptr(t_clr), stream=s)
    sp = {"spd_status": t_spd["status"], "spd_flags": t_spd["flags"], "spd_summary": t_spd["summary"],
          "clr_status": t_clr["status"], "clr_flags": t_clr["flags"], "clr_metrics": t_clr["metrics"]}
    if sk.dt > 0.0:
        sp.update(rows=t_spd["rows"], count=t_spd["count"])
    ctx.turn_select_device(B, C, ptr(sp), ptr(t_sel), cap_rows=sk.cap_rows,
                           reject_speed_flags=["STEER_EXCEEDS"] if reject_steer_exceeds else 0,
                           reject_clear_flags=["COLLISION", "MARGIN"], stream=s)
    stream.synchronize()
    for k, v in t_sel.items():
        getattr(sel, k)[...] = v.cpu().numpy()
    host = lambda t: t.cpu().numpy().reshape((C, B) + tuple(t.shape[1:]))   # noqa: E731
    spd_status, summary = host(t_spd["status"]), host(t_spd["summary"])
    clr_status, metrics = host(t_clr["status"]), host(t_clr["metrics"])
    T_all = np.where(spd_status == N_.SPD_OK, summary[:, :, 0], np.nan)
    c_all = np.where(clr_status == N_.CLR_OK, metrics[:, :, 0], np.nan)
    return dict(types=tuple(types), winner=sel.winner, winner_type=[types[w] if w >= 0 else None for w in sel.winner],
                T=sel.score, clearance=sel.clearance, rows=[sel.rows(b) for b in range(B)] if sk.dt > 0.0 else None,
                verdict=sel.verdict, T_all=T_all, clearance_all=c_all, speed_status=spd_status,
                clear_status=clr_status, clear_flags=host(t_clr["flags"]), speed_flags=host(t_spd["flags"]),
                select=sel)

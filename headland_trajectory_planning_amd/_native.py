"""ctypes binding of libhtp.so (include/htp.h) and batch packing.

The product path REQUIRES the in-tree HIP library: `load()` raises if it is
missing -- there is no CPU fallback.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libhtp.so")
NPARAM = 24
(P_DT, P_Q00, P_Q01, P_Q10, P_Q11, P_R00, P_R01, P_R10, P_R11, P_W00, P_W11, P_WHEELBASE, P_MAXSTEER,
 P_MAXV, P_MAXACC, P_MAXSR, P_DMIN, P_XLO, P_XHI, P_YLO, P_YHI, P_HAS_INIT_CONTROL, P_HAS_INIT_DUAL) = range(23)

STATUS_STR = {0: "Solve_Succeeded", 1: "Solved_To_Acceptable_Level", 2: "Maximum_Iterations_Exceeded",
              3: "Restoration_Failed", 4: "Error_In_Step_Computation", 5: "Invalid_Problem_Definition",
              6: "Maximum_CpuTime_Exceeded", 7: "Infeasible_Problem_Detected", 8: "Search_Direction_Becomes_Too_Small"}

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


class ObcaBatch(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("N", ctypes.c_int32), ("M", ctypes.c_int32), ("K", ctypes.c_int32),
                ("time_opt", ctypes.c_int32), ("obs_edges", ctypes.c_void_p), ("body_edges", ctypes.c_void_p),
                ("traj", ctypes.c_void_p), ("obs_A", ctypes.c_void_p), ("obs_b", ctypes.c_void_p),
                ("body_G", ctypes.c_void_p), ("body_g", ctypes.c_void_p), ("params", ctypes.c_void_p),
                ("init_control", ctypes.c_void_p), ("init_mu", ctypes.c_void_p), ("init_lambda", ctypes.c_void_p)]


class ObcaResult(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("objective", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("iterations", ctypes.c_void_p), ("n_factor", ctypes.c_void_p), ("nlp_error", ctypes.c_void_p),
                ("n_resto", ctypes.c_void_p)]


class AuditOpts(ctypes.Structure):  # htp_obca_audit_opts
    _fields_ = [("substeps", ctypes.c_int32), ("margin_tol", ctypes.c_double), ("dyn_tol", ctypes.c_double),
                ("bound_tol", ctypes.c_double), ("term_tol", ctypes.c_double)]


class AuditResult(ctypes.Structure):  # htp_obca_audit_result
    _fields_ = [(n, ctypes.c_void_p) for n in ("metrics", "worst", "flags", "stage_clearance")]


AUDIT_METRICS = ("clearance", "clearance_node", "dyn_defect", "bound_excess", "init_miss", "term_miss",
                 "path_length", "total_time")
AUDIT_FLAGS = {"COLLISION": 1, "MARGIN": 2, "DYNAMICS": 4, "BOUNDS": 8, "TERMINAL": 16, "NONFINITE": 32,
               "BAD_POLYTOPE": 64}
AUDIT_MAX_SUBSTEPS = 16


def audit_opts(substeps=4, margin_tol=1e-4, dyn_tol=1e-4, bound_tol=1e-4, term_tol=0.0):
    """htp_obca_audit_opts; the default tolerances are IPOPT's constr_viol_tol, the worst unscaled violation a
    converged solve may carry (term_tol = 0: the terminal row is soft, so its miss raises no flag)."""
    return AuditOpts(int(substeps), float(margin_tol), float(dyn_tol), float(bound_tol), float(term_tol))


class AuditResults:
    """Host arrays of one audit: metrics [rows, 8] (AUDIT_METRICS), worst [rows, 4] (stage, substep, obstacle,
    body), flags [rows] (AUDIT_FLAGS bits), stage_clearance [rows, N] or None."""
    METRICS = AUDIT_METRICS
    FLAGS = AUDIT_FLAGS

    def __init__(self, rows, N, stage=True):
        self.metrics = np.zeros((rows, len(AUDIT_METRICS)))
        self.worst = np.zeros((rows, 4), dtype=np.int32)
        self.flags = np.zeros(rows, dtype=np.int32)
        self.stage_clearance = np.zeros((rows, N)) if stage else None

    def struct(self):
        r = AuditResult()
        r.metrics, r.worst, r.flags = self.metrics.ctypes.data, self.worst.ctypes.data, self.flags.ctypes.data
        r.stage_clearance = None if self.stage_clearance is None else self.stage_clearance.ctypes.data
        return r

    def metric(self, name):
        return self.metrics[:, AUDIT_METRICS.index(name)]

    def flag_names(self, k):
        return [n for n, bit in AUDIT_FLAGS.items() if int(self.flags[k]) & bit]

    def as_dict(self, k):
        d = {n: float(self.metrics[k, j]) for j, n in enumerate(AUDIT_METRICS)}
        d["worst"] = dict(zip(("stage", "substep", "obstacle", "body"), (int(v) for v in self.worst[k])))
        d["flags"] = self.flag_names(k)
        d["ok"] = int(self.flags[k]) == 0
        if self.stage_clearance is not None:
            d["stage_clearance"] = self.stage_clearance[k].copy()
        return d


class TimelineOpts(ctypes.Structure):  # htp_obca_timeline_opts
    _fields_ = [("dt", ctypes.c_double), ("cap", ctypes.c_int32)]


class TimelineResult(ctypes.Structure):  # htp_obca_timeline_result
    _fields_ = [(n, ctypes.c_void_p) for n in ("rows", "stage", "count", "flags", "duration")]


TIMELINE_COLUMNS = ("t", "x", "y", "v", "theta", "steer", "accel", "steer_rate", "curvature", "arc")
TIMELINE_FLAGS = {"TRUNCATED": 1, "NONFINITE": 2, "BAD_TIME": 4}
TIMELINE_MAX_N = 480


def timeline_opts(dt, cap):
    return TimelineOpts(float(dt), int(cap))


def timeline_cap(packed, x, dt):
    """Rows of storage that hold every problem of x [batch, n_var] at period dt: the longest duration's row count
    plus the quotient's rounding (problems the sampler rejects need none); at least 2."""
    N = packed.N
    h = packed.params[:, P_DT:P_DT + 1] * (x[:, packed.n_var - 5 - (N - 1):packed.n_var - 5] if packed.time_opt
                                            else np.ones((packed.batch, N - 1)))
    with np.errstate(all="ignore"):
        q = np.cumsum(h, axis=1)[:, -1] / float(dt)
    q = q[np.isfinite(q) & (q < 2.0 ** 30) & np.all(h > 0, axis=1)]
    return max(2, int(np.floor(q.max())) + 3) if q.size else 2


class TimelineResults:
    """Host arrays of one timeline: data [rows, cap, 10] (TIMELINE_COLUMNS), stage [rows, cap] or None, count
    [rows] (rows needed), flags [rows] (TIMELINE_FLAGS bits), duration [rows]."""
    COLUMNS = TIMELINE_COLUMNS
    FLAGS = TIMELINE_FLAGS

    def __init__(self, rows, cap, stage=True):
        self.cap = int(cap)
        self.data = np.zeros((rows, self.cap, len(TIMELINE_COLUMNS)))
        self.stage = np.zeros((rows, self.cap), dtype=np.int32) if stage else None
        self.count = np.zeros(rows, dtype=np.int32)
        self.flags = np.zeros(rows, dtype=np.int32)
        self.duration = np.zeros(rows)

    def struct(self):
        r = TimelineResult()
        r.rows, r.count, r.flags = self.data.ctypes.data, self.count.ctypes.data, self.flags.ctypes.data
        r.duration = self.duration.ctypes.data
        r.stage = None if self.stage is None else self.stage.ctypes.data
        return r

    def valid(self, k):
        return min(int(self.count[k]), self.cap)

    def flag_names(self, k):
        return [n for n, bit in TIMELINE_FLAGS.items() if int(self.flags[k]) & bit]

    def rows(self, k):
        """The written rows of problem k: a dict of the named column arrays, plus "stage" where it was asked for."""
        n = self.valid(k)
        d = {name: self.data[k, :n, j].copy() for j, name in enumerate(TIMELINE_COLUMNS)}
        if self.stage is not None:
            d["stage"] = self.stage[k, :n].copy()
        return d

    def as_dict(self, k):
        d = self.rows(k)
        d["duration"] = float(self.duration[k])
        d["flags"] = self.flag_names(k)
        return d


class EnvelopeOpts(ctypes.Structure):  # htp_obca_envelope_opts
    _fields_ = [("substeps", ctypes.c_int32), ("res", ctypes.c_double), ("W", ctypes.c_int32), ("H", ctypes.c_int32)]


class EnvelopeResult(ctypes.Structure):  # htp_obca_envelope_result
    _fields_ = [(n, ctypes.c_void_p) for n in ("extent", "where", "extent_body", "cells", "bitmap", "flags")]


ENVELOPE_SIDES = ("umin", "umax", "vmin", "vmax")
ENVELOPE_FLAGS = {"CLIPPED": 1, "NONFINITE": 2, "BAD_POLYTOPE": 4}
ENVELOPE_MAX_N = 480
ENVELOPE_MAX_CELLS = 65536


def envelope_opts(substeps=4, res=0.1, W=0, H=0):
    return EnvelopeOpts(int(substeps), float(res), int(W), int(H))


def body_radius(packed):
    """Largest distance of a body vertex from the body frame's origin, over the batch: the vertices are the pairwise
    intersections of a body's rows that satisfy all of its rows."""
    r = 0.0
    off = np.concatenate([[0], np.cumsum(packed.body_edges)])
    seen = set()
    for p in range(packed.batch):
        for k in range(packed.K):
            G, g = packed.body_G[p, off[k]:off[k + 1]], packed.body_g[p, off[k]:off[k + 1]]
            key = G.tobytes() + g.tobytes()
            if key in seen:               # a fleet of one machine: the same rows in every problem
                continue
            seen.add(key)
            for a in range(len(g)):
                for b in range(a + 1, len(g)):
                    A = np.array([G[a], G[b]])
                    if abs(np.linalg.det(A)) < 1e-12:
                        continue
                    v = np.linalg.solve(A, np.array([g[a], g[b]]))
                    if np.all(G @ v <= g + 1e-9 * (1.0 + np.abs(g))):
                        r = max(r, float(np.hypot(v[0], v[1])))
    return r


def envelope_default_frame(packed, x, res):
    """The frame Context.envelope uses when none is given -> (frames [batch, 3], W, H): phi = 0, origin = the
    problem's own nodes' minimum minus pad, pad = the largest body-vertex radius + res, and the smallest admissible
    W (a multiple of 32) and H that cover every problem's nodes' maximum plus pad.  Problems with a non-finite node
    take no part in the sizes (the envelope rejects them)."""
    if not (np.isfinite(res) and res > 0):
        raise ValueError(f"[htp] envelope: res must be finite and > 0, got {res}")
    B, N = packed.batch, packed.N
    xy = np.asarray(x)[:, :5 * N].reshape(B, N, 5)[:, :, :2]
    pad = body_radius(packed) + res
    lo, hi = xy.min(axis=1) - pad, xy.max(axis=1) + pad
    frames = np.zeros((B, 3))
    good = np.all(np.isfinite(lo) & np.isfinite(hi), axis=1)
    frames[good, :2] = lo[good]
    span = (hi - lo)[good].max(axis=0) if good.any() else np.array([res, res])
    W = max(32, 32 * int(np.ceil(np.ceil(span[0] / res) / 32.0)))
    H = max(1, int(np.ceil(span[1] / res)))
    if W * H > ENVELOPE_MAX_CELLS:
        need = float(np.sqrt(span[0] * span[1] / ENVELOPE_MAX_CELLS))
        raise ValueError(f"[htp] envelope: the default grid would be {W} x {H} cells at res = {res}, more than "
                         f"{ENVELOPE_MAX_CELLS}; use a coarser res (about {1.1 * need:.3g} or more) or give frames, W and H")
    return frames, W, H


class EnvelopeResults:
    """Host arrays of one envelope: extent [rows, 4] (ENVELOPE_SIDES), where [rows, 4, 3] (stage, substep, body),
    extent_body [rows, K, 4], cells [rows, K + 1] (the union last), flags [rows] (ENVELOPE_FLAGS bits), words
    [rows, H, W / 32] uint32 or None, and the frames, res, W and H they were computed in."""
    SIDES = ENVELOPE_SIDES
    FLAGS = ENVELOPE_FLAGS

    def __init__(self, rows, K, W=0, H=0, res=0.0, frames=None, bitmap=True):
        self.K, self.W, self.H, self.res = int(K), int(W), int(H), float(res)
        self.frames = None if frames is None else np.ascontiguousarray(frames, dtype=np.float64)
        self.extent = np.zeros((rows, 4))
        self.where = np.zeros((rows, 4, 3), dtype=np.int32)
        self.extent_body = np.zeros((rows, self.K, 4))
        self.cells = np.zeros((rows, self.K + 1), dtype=np.int32)
        self.flags = np.zeros(rows, dtype=np.int32)
        self.words = np.zeros((rows, self.H, self.W // 32), dtype=np.uint32) if (bitmap and self.W > 0) else None

    def struct(self):
        r = EnvelopeResult()
        r.extent, r.where, r.flags = self.extent.ctypes.data, self.where.ctypes.data, self.flags.ctypes.data
        r.extent_body, r.cells = self.extent_body.ctypes.data, self.cells.ctypes.data
        r.bitmap = None if self.words is None else self.words.ctypes.data
        return r

    def flag_names(self, k):
        return [n for n, bit in ENVELOPE_FLAGS.items() if int(self.flags[k]) & bit]

    def bitmap(self, k):
        """The union's occupancy of problem k as bool [H, W]: element [j, i] is cell (i, j)."""
        if self.words is None:
            raise ValueError("[htp] envelope: no bitmap was asked for")
        bits = (self.words[k][:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
        return bits.reshape(self.H, self.W).astype(bool)

    def as_dict(self, k):
        d = {n: float(self.extent[k, j]) for j, n in enumerate(ENVELOPE_SIDES)}
        d["depth"] = d["vmax"] - d["vmin"]
        d["where"] = {n: dict(zip(("stage", "substep", "body"), (int(v) for v in self.where[k, j])))
                      for j, n in enumerate(ENVELOPE_SIDES)}
        d["extent_body"] = self.extent_body[k].copy()
        d["flags"] = self.flag_names(k)
        if self.frames is not None:
            d["frame"] = self.frames[k].copy()
        if self.W > 0:
            d["cells"] = self.cells[k].copy()
            d["area"] = float(self.cells[k, -1]) * self.res * self.res
            d["res"], d["W"], d["H"] = self.res, self.W, self.H
            if self.words is not None:
                d["bitmap"] = self.bitmap(k)
        return d


class TrackOpts(ctypes.Structure):  # htp_obca_track_opts
    _fields_ = [("dt", ctypes.c_double), ("max_ticks", ctypes.c_int32), ("plant_substeps", ctypes.c_int32),
                ("k_lat", ctypes.c_double), ("k_yaw", ctypes.c_double), ("k_lon", ctypes.c_double),
                ("abort_dist", ctypes.c_double), ("margin_tol", ctypes.c_double), ("R", ctypes.c_int32),
                ("scenarios", ctypes.c_void_p)]


class TrackResult(ctypes.Structure):  # htp_obca_track_result
    _fields_ = [(n, ctypes.c_void_p) for n in ("metrics", "worst", "flags", "tally", "worst_scenario",
                                               "tick_clearance", "reference")]


TRACK_METRICS = ("clearance", "max_e_lat", "max_e_lon", "max_e_theta", "end_pos", "end_e_theta", "max_steer_dev",
                 "sat_share")
TRACK_FLAGS = {"COLLISION": 1, "MARGIN": 2, "SAT_STEER": 4, "SAT_RATE": 8, "SAT_ACC": 16, "DIVERGED": 32,
               "TRUNCATED": 64, "NONFINITE": 128, "BAD_POLYTOPE": 256, "BAD_TIME": 512}
TRACK_SCENARIO_COLUMNS = ("lat0", "lon0", "yaw0", "steer_bias", "slip", "yaw_gain")
TRACK_REFERENCE_COLUMNS = ("x", "y", "v", "theta", "steer")
TRACK_MAX_N = 480
TRACK_MAX_SCENARIOS = 4096
# Default gains, from the linearised error dynamics in include/htp.h: natural frequency |v| sqrt(k_lat / L), damping
# ratio k_yaw / (2 sqrt(k_lat L)).  k_lat = 0.5 /m and k_yaw = 2 give, at the wheelbases 1.9-3 m of the machines
# here, a damping ratio of 1.03-0.82, and at speeds of 1-2 m/s a natural frequency of 0.5-1 rad/s: at most a tenth of
# a radian per 0.1 s control tick, far inside what the one-tick hold of the steering set-point tolerates.  k_lon = 1 /s closes
# the along-track error with a 1 s time constant (k_lon dt = 0.1).
TRACK_DEFAULT_GAINS = dict(k_lat=0.5, k_yaw=2.0, k_lon=1.0)


def track_scenarios(R, seed, lat=0.05, lon=0.05, yaw=0.02, steer_bias=0.01, slip=0.03, yaw_gain=0.05):
    """A seeded table [R, 6] (TRACK_SCENARIO_COLUMNS) of normal draws with the given standard deviations through
    numpy.random.default_rng(seed): row 0 is the nominal scenario (0, 0, 0, 0, 0, 1); slip is clipped to [0, 0.5),
    yaw_gain is drawn around 1."""
    R = int(R)
    if R < 1:
        raise ValueError(f"[htp] track_scenarios: R must be >= 1, got {R}")
    rng = np.random.default_rng(seed)
    t = rng.normal(0.0, 1.0, (R, len(TRACK_SCENARIO_COLUMNS))) * np.array([lat, lon, yaw, steer_bias, slip, yaw_gain])
    t[:, 4] = np.clip(t[:, 4], 0.0, np.nextafter(0.5, 0.0))
    t[:, 5] += 1.0
    t[0] = [0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    return t


def track_opts(dt, max_ticks, scenarios_ptr, R, plant_substeps=2, k_lat=TRACK_DEFAULT_GAINS["k_lat"],
               k_yaw=TRACK_DEFAULT_GAINS["k_yaw"], k_lon=TRACK_DEFAULT_GAINS["k_lon"], abort_dist=2.0,
               margin_tol=1e-4):
    """htp_obca_track_opts.  scenarios_ptr: the address of R rows of 6 doubles (host or device, as the entry that
    takes it); the caller keeps the array alive.  abort_dist 2 m: a machine that far off its path has left the
    turn.  margin_tol as the audit's."""
    return TrackOpts(float(dt), int(max_ticks), int(plant_substeps), float(k_lat), float(k_yaw), float(k_lon),
                     float(abort_dist), float(margin_tol), int(R), scenarios_ptr)


def track_ticks(packed, x, dt):
    """Poses of storage that hold every problem of x [batch, n_var] at period dt (timeline_cap's count)."""
    return timeline_cap(packed, x, dt)


class TrackResults:
    """Host arrays of one tracking rollout: metrics [rows, R, 8] (TRACK_METRICS), worst [rows, R, 3] (tick, obstacle,
    body), flags [rows, R] (TRACK_FLAGS bits), tally [rows, 10] (scenarios per flag, in TRACK_FLAGS order),
    worst_scenario [rows], tick_clearance [rows, max_ticks] or None, reference [rows, max_ticks, 5] or None (both
    pre-filled with NaN: the poses a problem does not reach are never written), and the scenarios they belong to."""
    METRICS = TRACK_METRICS
    FLAGS = TRACK_FLAGS

    def __init__(self, rows, R, max_ticks, scenarios=None, ticks=True, reference=False):
        self.R, self.max_ticks = int(R), int(max_ticks)
        self.scenarios = scenarios
        self.metrics = np.zeros((rows, self.R, len(TRACK_METRICS)))
        self.worst = np.zeros((rows, self.R, 3), dtype=np.int32)
        self.flags = np.zeros((rows, self.R), dtype=np.int32)
        self.tally = np.zeros((rows, len(TRACK_FLAGS)), dtype=np.int32)
        self.worst_scenario = np.zeros(rows, dtype=np.int32)
        self.tick_clearance = np.full((rows, self.max_ticks), np.nan) if ticks else None
        self.reference = np.full((rows, self.max_ticks, len(TRACK_REFERENCE_COLUMNS)), np.nan) if reference else None

    def struct(self):
        r = TrackResult()
        for n in ("metrics", "worst", "flags", "tally", "worst_scenario"):
            setattr(r, n, getattr(self, n).ctypes.data)
        r.tick_clearance = None if self.tick_clearance is None else self.tick_clearance.ctypes.data
        r.reference = None if self.reference is None else self.reference.ctypes.data
        return r

    def metric(self, name):
        return self.metrics[:, :, TRACK_METRICS.index(name)]

    def flag_names(self, k, s):
        return [n for n, bit in TRACK_FLAGS.items() if int(self.flags[k, s]) & bit]

    def as_dict(self, k):
        d = {n: self.metrics[k, :, j].copy() for j, n in enumerate(TRACK_METRICS)}
        d["worst"] = self.worst[k].copy()
        d["flags"] = [self.flag_names(k, s) for s in range(self.R)]
        d["tally"] = {n: int(self.tally[k, j]) for j, n in enumerate(TRACK_FLAGS)}
        d["worst_scenario"] = int(self.worst_scenario[k])
        d["ok"] = not (int(np.bitwise_or.reduce(self.flags[k])) &
                       ~(TRACK_FLAGS["SAT_STEER"] | TRACK_FLAGS["SAT_RATE"] | TRACK_FLAGS["SAT_ACC"]))
        if self.scenarios is not None:
            d["scenarios"] = self.scenarios.copy()
        if self.tick_clearance is not None:
            d["tick_clearance"] = self.tick_clearance[k].copy()
        if self.reference is not None:
            d["reference"] = self.reference[k].copy()
        return d


class LqrOpts(ctypes.Structure):  # htp_obca_lqr_opts
    _fields_ = [(n, ctypes.c_double) for n in (
        "q_lon", "q_lat", "q_v", "q_th", "q_st", "qf", "r_a", "r_w", "sig0_lon", "sig0_lat", "sig0_v", "sig0_th",
        "sig0_st", "w_lon", "w_lat", "w_v", "w_th", "w_st", "k_sigma")]


class LqrResult(ctypes.Structure):  # htp_obca_lqr_result
    _fields_ = [(n, ctypes.c_void_p) for n in ("gains", "tube", "metrics", "worst", "flags", "cost_to_go",
                                               "linearisation")]


LQR_METRICS = ("max_sigma_lat", "max_sigma_lon", "max_sigma_theta", "end_sigma_lat", "max_gain", "trace_p0",
               "ratio_acc", "ratio_rate", "ratio_steer", "ratio_speed")
LQR_FLAGS = {"AUTHORITY_ACC": 1, "AUTHORITY_RATE": 2, "AUTHORITY_STEER": 4, "AUTHORITY_SPEED": 8, "SINGULAR": 16,
             "NONFINITE": 32, "BAD_TIME": 64, "BAD_LIMIT": 128}
LQR_TUBE_COLUMNS = ("sigma_lon", "sigma_lat", "sigma_v", "sigma_theta", "sigma_steer", "sigma_accel",
                    "sigma_steer_rate")
LQR_MAX_N = 480
# Defaults by Bryson's rule (a weight is one over the square of the deviation one is willing to accept): 0.1 m
# across and 0.2 m along the path, 0.2 m/s, 0.1 rad of heading and 0.2 rad of steering; the controls are weighted
# in units of their own limits (r = 1: a full-scale control costs as much as one accepted state deviation); the end
# state counts ten times.  sig0 are the sigmas of track_scenarios; w is a design choice: 1 cm of position and 0.01
# rad of heading random walk per root second.  k_sigma = 2: a flag where less than two sigma of headroom is left.
LQR_DEFAULTS = dict(q_lon=1.0 / 0.2 ** 2, q_lat=1.0 / 0.1 ** 2, q_v=1.0 / 0.2 ** 2, q_th=1.0 / 0.1 ** 2,
                    q_st=1.0 / 0.2 ** 2, qf=10.0, r_a=1.0, r_w=1.0, sig0_lon=0.05, sig0_lat=0.05, sig0_v=0.0,
                    sig0_th=0.02, sig0_st=0.0, w_lon=1e-4, w_lat=1e-4, w_v=0.0, w_th=1e-4, w_st=0.0, k_sigma=2.0)


def lqr_opts(**opts):
    """htp_obca_lqr_opts: LQR_DEFAULTS overridden by the keywords (the names of the struct's fields)."""
    unknown = set(opts) - set(LQR_DEFAULTS)
    if unknown:
        raise TypeError(f"[htp] lqr: unknown options {sorted(unknown)}")
    v = {**LQR_DEFAULTS, **opts}
    return LqrOpts(*(float(v[n]) for n, _ in LqrOpts._fields_))


class LqrResults:
    """Host arrays of one LQR pass: gains [rows, N-1, 2, 5] (u = U_i - K_i (s - X_i)), tube [rows, N, 7]
    (LQR_TUBE_COLUMNS), metrics [rows, 10] (LQR_METRICS), worst [rows, 2] (node of max_sigma_lat, stage of
    ratio_rate), flags [rows] (LQR_FLAGS bits), cost_to_go [rows, N, 15] or None (upper triangle of P_i, row-major),
    linearisation [rows, N-1, 35] or None (A_i, then B_i, row-major).  The arrays are pre-filled with NaN (worst
    with -1): what a flag leaves unwritten stays so."""
    METRICS = LQR_METRICS
    FLAGS = LQR_FLAGS

    def __init__(self, rows, N, cost_to_go=False, linearisation=False):
        self.N = int(N)
        self.gains = np.full((rows, self.N - 1, 2, 5), np.nan)
        self.tube = np.full((rows, self.N, len(LQR_TUBE_COLUMNS)), np.nan)
        self.metrics = np.full((rows, len(LQR_METRICS)), np.nan)
        self.worst = np.full((rows, 2), -1, dtype=np.int32)
        self.flags = np.zeros(rows, dtype=np.int32)
        self.cost_to_go = np.full((rows, self.N, 15), np.nan) if cost_to_go else None
        self.linearisation = np.full((rows, self.N - 1, 35), np.nan) if linearisation else None

    def struct(self):
        r = LqrResult()
        for n in ("gains", "tube", "metrics", "worst", "flags"):
            setattr(r, n, getattr(self, n).ctypes.data)
        r.cost_to_go = None if self.cost_to_go is None else self.cost_to_go.ctypes.data
        r.linearisation = None if self.linearisation is None else self.linearisation.ctypes.data
        return r

    def metric(self, name):
        return self.metrics[:, LQR_METRICS.index(name)]

    def flag_names(self, k):
        return [n for n, bit in LQR_FLAGS.items() if int(self.flags[k]) & bit]

    def P(self, k, i):
        """The cost-to-go matrix P_i of problem k as a full symmetric [5, 5]."""
        if self.cost_to_go is None:
            raise ValueError("[htp] lqr: no cost_to_go was asked for")
        m = np.zeros((5, 5))
        m[np.triu_indices(5)] = self.cost_to_go[k, i]
        return m + np.triu(m, 1).T

    def as_dict(self, k):
        d = {n: float(self.metrics[k, j]) for j, n in enumerate(LQR_METRICS)}
        d["gains"] = self.gains[k].copy()
        d["tube"] = {n: self.tube[k, :, j].copy() for j, n in enumerate(LQR_TUBE_COLUMNS)}
        d["worst"] = {"max_sigma_lat": int(self.worst[k, 0]), "ratio_rate": int(self.worst[k, 1])}
        d["flags"] = self.flag_names(k)
        d["ok"] = int(self.flags[k]) == 0
        if self.cost_to_go is not None:
            d["cost_to_go"] = self.cost_to_go[k].copy()
        if self.linearisation is not None:
            d["A"] = self.linearisation[k, :, :25].reshape(-1, 5, 5).copy()
            d["B"] = self.linearisation[k, :, 25:].reshape(-1, 5, 2).copy()
        return d


class LtrackOpts(ctypes.Structure):  # htp_obca_ltrack_opts
    _fields_ = [("dt", ctypes.c_double), ("max_ticks", ctypes.c_int32), ("plant_substeps", ctypes.c_int32),
                ("abort_dist", ctypes.c_double), ("margin_tol", ctypes.c_double), ("R", ctypes.c_int32),
                ("scenarios", ctypes.c_void_p), ("gains", ctypes.c_void_p)]


class LtrackResult(ctypes.Structure):  # htp_obca_ltrack_result
    _fields_ = [(n, ctypes.c_void_p) for n in ("metrics", "worst", "flags", "tally", "worst_scenario",
                                               "tick_clearance", "reference", "tick_error")]


LTRACK_ERROR_COLUMNS = ("e_lat", "e_lon", "e_theta")


def ltrack_opts(dt, max_ticks, scenarios_ptr, R, gains_ptr, plant_substeps=2, abort_dist=2.0, margin_tol=1e-4):
    """htp_obca_ltrack_opts: track_opts without the three fixed gains, with the address of the LQR gains
    [batch, N-1, 2, 5] (host or device, as the entry that takes it); the caller keeps both arrays alive."""
    return LtrackOpts(float(dt), int(max_ticks), int(plant_substeps), float(abort_dist), float(margin_tol), int(R),
                      scenarios_ptr, gains_ptr)


class LtrackResults(TrackResults):
    """TrackResults of a rollout under the LQR gains, plus tick_error [rows, max_ticks, 3] (LTRACK_ERROR_COLUMNS:
    per pose the largest |e_lat|, |e_lon|, |e_theta| over the scenarios that reached it) or None, pre-filled with NaN
    as the other per-tick arrays, and the gains [rows, N-1, 2, 5] the rollout ran under (None if they stayed on the
    device)."""

    def __init__(self, rows, R, max_ticks, scenarios=None, ticks=True, reference=False, errors=True, gains=None):
        super().__init__(rows, R, max_ticks, scenarios, ticks, reference)
        self.tick_error = np.full((rows, self.max_ticks, len(LTRACK_ERROR_COLUMNS)), np.nan) if errors else None
        self.gains = gains

    def struct(self):
        r = LtrackResult()
        for n in ("metrics", "worst", "flags", "tally", "worst_scenario"):
            setattr(r, n, getattr(self, n).ctypes.data)
        for n in ("tick_clearance", "reference", "tick_error"):
            setattr(r, n, None if getattr(self, n) is None else getattr(self, n).ctypes.data)
        return r

    def as_dict(self, k):
        d = super().as_dict(k)
        if self.tick_error is not None:
            d["tick_error"] = self.tick_error[k].copy()
        return d


class RepairOpts(ctypes.Structure):  # htp_obca_repair_opts
    _fields_ = [("rounds", ctypes.c_int32), ("pad", ctypes.c_double), ("max_raise", ctypes.c_double),
                ("audit", AuditOpts)]


class RepairState(ctypes.Structure):  # htp_obca_repair_state
    _fields_ = [(n, ctypes.c_void_p) for n in ("state", "rounds_used", "extra_iterations", "dmin_used")]


class RepairSlots(ctypes.Structure):  # htp_obca_repair_slots
    _fields_ = [("cap", ctypes.c_int32)] + [(n, ctypes.c_void_p) for n in (
        "count", "index", "adopted", "traj", "obs_A", "obs_b", "body_G", "body_g", "params", "params_audit",
        "init_control", "init_mu", "init_lambda")]


class RepairReport(ctypes.Structure):  # htp_obca_repair_report
    _fields_ = [("state", RepairState), ("round_counts", ctypes.c_void_p)]


REPAIR_STATES = {"CANDIDATE": 1, "IMPROVED": 2, "REPAIRED": 4, "RESOLVE_FAILED": 8, "GAVE_UP": 16}
REPAIR_MAX_ROUNDS = 8
REPAIR_STATE_ARRAYS = ("state", "rounds_used", "extra_iterations", "dmin_used")
REPAIR_SLOT_ARRAYS = ("traj", "obs_A", "obs_b", "body_G", "body_g", "params", "params_audit", "init_control",
                      "init_mu", "init_lambda")


def repair_opts(rounds=3, pad=0.01, max_raise=0.5, **audit):
    """htp_obca_repair_opts: 3 rounds, 1 cm on top of every raise, at most 0.5 m above the original margin
    (design choices, not tuned values) and the audit_opts of every audit."""
    return RepairOpts(int(rounds), float(pad), float(max_raise), audit_opts(**audit))


def _struct_of(cls, ptrs, **scalars):
    s = cls()
    for k, v in ptrs.items():
        setattr(s, k, v)
    for k, v in scalars.items():
        setattr(s, k, v)
    return s


class RepairStates:
    """Host arrays of the per-problem repair state; fresh = all zero (dmin_used counts only where rounds_used > 0)."""

    def __init__(self, batch):
        self.state = np.zeros(batch, dtype=np.int32)
        self.rounds_used = np.zeros(batch, dtype=np.int32)
        self.extra_iterations = np.zeros(batch, dtype=np.int32)
        self.dmin_used = np.zeros(batch)

    def struct(self):
        return _struct_of(RepairState, {n: getattr(self, n).ctypes.data for n in REPAIR_STATE_ARRAYS})

    def state_names(self, k):
        return [n for n, bit in REPAIR_STATES.items() if int(self.state[k]) & bit]


class RepairSlotArrays:
    """Host arrays of `cap` slots of a re-solve batch shaped like `packed` (htp_obca_repair_slots)."""

    def __init__(self, packed, cap, fill=0.0, ifill=0):
        self.shape_of = packed
        self.cap = int(cap)
        N = packed.N
        TEo, TEb = int(packed.obs_edges.sum()), int(packed.body_edges.sum())
        self.count = np.full(1, ifill, dtype=np.int32)
        self.index = np.full(self.cap, ifill, dtype=np.int32)
        self.adopted = np.full(self.cap, ifill, dtype=np.int32)
        dims = dict(traj=(N, 5), obs_A=(TEo, 2), obs_b=(TEo,), body_G=(TEb, 2), body_g=(TEb,), params=(NPARAM,),
                    params_audit=(NPARAM,), init_control=(N - 1, 2), init_mu=(N, packed.mu_count),
                    init_lambda=(N, packed.lam_count))
        for n in REPAIR_SLOT_ARRAYS:
            setattr(self, n, np.full((self.cap,) + dims[n], fill))

    def struct(self):
        ptrs = {n: getattr(self, n).ctypes.data for n in ("count", "index", "adopted") + REPAIR_SLOT_ARRAYS}
        return _struct_of(RepairSlots, ptrs, cap=self.cap)

    def used(self):
        return min(int(self.count[0]), self.cap)

    def packed(self, audit=False):
        """The written slots as a PackedBatch: what a solve takes, or (audit) the same judged by params_audit."""
        pk = PackedBatch.__new__(PackedBatch)
        pk.__dict__.update(self.shape_of.__dict__)
        pk.batch = self.used()
        for n in PackedBatch.INPUTS:
            setattr(pk, n, getattr(self, n)[:pk.batch])
        if audit:
            pk.params = self.params_audit[:pk.batch]
        return pk


class RepairReports(RepairStates):
    """Host arrays of one repair loop: the per-problem state and round_counts [8, 3] (selected, adopted, clean)."""

    def __init__(self, batch):
        super().__init__(batch)
        self.round_counts = np.zeros((REPAIR_MAX_ROUNDS, 3), dtype=np.int32)

    def report_struct(self):
        r = RepairReport()
        r.state = self.struct()
        r.round_counts = self.round_counts.ctypes.data
        return r

    def as_dict(self, k, min_dist):
        """`min_dist`: the problem's original margin, reported where no re-solve was merged."""
        return {"state": self.state_names(k), "rounds": int(self.rounds_used[k]),
                "min_dist_used": float(self.dmin_used[k]) if self.rounds_used[k] > 0 else float(min_dist),
                "extra_iterations": int(self.extra_iterations[k])}


class RsPaths(ctypes.Structure):
    _fields_ = [("cap_paths", ctypes.c_int64), ("cap_points", ctypes.c_int64), ("n_paths", ctypes.c_int64),
                ("n_points", ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in (
                    "path_offsets", "status", "lengths", "ctypes", "L", "point_offsets", "x", "y", "yaw", "cs",
                    "directions")]


class HaBatch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("batch", "npoly", "nvert", "nguide", "nmotion")] + \
        [(n, ctypes.c_void_p) for n in ("params", "desc", "poly_off", "vertices", "lane_len", "guide", "motions")] + \
        [(n, ctypes.c_int32) for n in ("max_nodes_cap", "cap_path", "cap_log")]


class HaResult(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("status", "counter", "n_path", "n_expanded", "n_pose", "x", "y", "yaw",
                                               "dir", "k", "expanded")]


class YpBatch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("batch", "npoly", "nvert", "naxis")] + \
        [(n, ctypes.c_void_p) for n in ("params", "desc", "poly_off", "vertices", "axis")] + [("cap_path", ctypes.c_int32)]


class YpResult(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("status", "cand", "n_path", "params", "n_pose", "path")]


YP_NPARAM, YP_NDESC = 16, 12
(YP_P_EX, YP_P_EY, YP_P_EYAW, YP_P_BDIR, YP_P_FDIR, YP_P_WB, YP_P_STEP, YP_P_R00, YP_P_R01, YP_P_R10, YP_P_R11,
 YP_P_TX, YP_P_TY, YP_P_YAW_ODOM) = range(14)
YP_STATUS = {0: "found", 1: "none", 2: "end_blocked", 3: "bad_input"}
YP_STATUS_BY_NAME = {v: k for k, v in YP_STATUS.items()}

HA_NPARAM, HA_NDESC = 16, 12
(HA_P_SX, HA_P_SY, HA_P_SYAW, HA_P_GX, HA_P_GY, HA_P_GYAW, HA_P_RES, HA_P_YAWRES, HA_P_WB, HA_P_MAXSTEER,
 HA_P_CURV, HA_P_DEFLEN, HA_P_MAXNODES) = range(13)
(HA_D_BODY, HA_D_BLK0, HA_D_BLK1, HA_D_LANE0, HA_D_LANE1, HA_D_FIELD, HA_D_GUIDE0, HA_D_GUIDE1, HA_D_MOT0,
 HA_D_MOT1, HA_D_KING) = range(11)
HA_STATUS = {0: "found", 1: "no_path", 2: "max_nodes", 3: "start_goal_blocked", 4: "rs_error", 5: "capacity",
             6: "bad_input", 7: "backtrack_error"}

RS_OK, RS_ASSERT, RS_OVERFLOW, RS_CAPACITY = 0, 1, 2, 3
RS_SEG = "LSR"  # HTP_RS_SEG_L / _S / _R


EXPORTS = ["htp_obca_sizes", "htp_create", "htp_destroy", "htp_last_error", "htp_set_option",
           "htp_obca_solve_batch", "htp_obca_solve_batch_device", "htp_last_kernel_ms", "htp_last_cycles",
           "htp_rs_all_paths_batch", "htp_rs_all_paths_batch_device", "htp_rs_last_ms",
           "htp_hastar_search_batch", "htp_hastar_search_batch_device", "htp_hastar_last_ms",
           "htp_ypark_search_batch", "htp_ypark_search_batch_device", "htp_ypark_last_ms",
           "htp_obca_points_sizes", "htp_obca_points_solve_batch", "htp_obca_points_solve_batch_device",
           "htp_init_ref_path_batch", "htp_init_ref_path_batch_device", "htp_init_ref_path_last_ms",
           "htp_queue_create", "htp_queue_destroy", "htp_queue_publish", "htp_queue_close", "htp_queue_published",
           "htp_queue_claimed", "htp_obca_solve_queue_device", "htp_obca_resident_waves",
           "htp_oge_obstacles_batch", "htp_oge_obstacles_batch_device", "htp_oge_last_ms",
           "htp_classic_turn_batch", "htp_classic_turn_batch_device", "htp_classic_last_ms",
           "htp_orchard_chain_device", "htp_chain_last_ms",
           "htp_obca_audit_batch", "htp_obca_audit_batch_device", "htp_obca_audit_last_ms",
           "htp_obca_timeline_batch", "htp_obca_timeline_batch_device", "htp_obca_timeline_last_ms",
           "htp_obca_repair_pack_batch", "htp_obca_repair_pack_batch_device", "htp_obca_repair_merge_batch",
           "htp_obca_repair_merge_batch_device", "htp_obca_repair_batch", "htp_obca_repair_batch_device",
           "htp_obca_repair_last_ms",
           "htp_obca_envelope_batch", "htp_obca_envelope_batch_device", "htp_obca_envelope_last_ms",
           "htp_obca_track_batch", "htp_obca_track_batch_device", "htp_obca_track_last_ms",
           "htp_obca_lqr_batch", "htp_obca_lqr_batch_device", "htp_obca_lqr_last_ms",
           "htp_obca_ltrack_batch", "htp_obca_ltrack_batch_device", "htp_obca_ltrack_last_ms",
           "htp_classic_sample_batch", "htp_classic_sample_batch_device", "htp_classic_sample_last_ms",
           "htp_speed_profile_batch", "htp_speed_profile_batch_device", "htp_speed_profile_last_ms",
           "htp_pose_clearance_batch", "htp_pose_clearance_batch_device", "htp_pose_clearance_last_ms",
           "htp_turn_select_batch", "htp_turn_select_batch_device", "htp_turn_select_last_ms"]


def _declare(lib):
    lib.htp_obca_sizes.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 2 + [ctypes.POINTER(ctypes.c_int64)] * 4
    lib.htp_obca_sizes.restype = ctypes.c_int
    lib.htp_create.argtypes = [ctypes.c_int32]
    lib.htp_create.restype = ctypes.c_void_p
    lib.htp_destroy.argtypes = [ctypes.c_void_p]
    lib.htp_destroy.restype = None
    lib.htp_last_error.argtypes = [ctypes.c_void_p]
    lib.htp_last_error.restype = ctypes.c_char_p
    lib.htp_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double]
    lib.htp_set_option.restype = ctypes.c_int
    lib.htp_obca_solve_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch), ctypes.POINTER(ObcaResult)]
    lib.htp_obca_solve_batch.restype = ctypes.c_int
    lib.htp_obca_solve_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch),
                                                ctypes.POINTER(ObcaResult), ctypes.c_void_p]
    lib.htp_obca_solve_batch_device.restype = ctypes.c_int
    lib.htp_init_ref_path_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(RpBatch), ctypes.POINTER(RpResult)]
    lib.htp_init_ref_path_batch.restype = ctypes.c_int
    lib.htp_init_ref_path_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RpBatch), ctypes.POINTER(RpResult),
                                                   ctypes.c_void_p]
    lib.htp_init_ref_path_batch_device.restype = ctypes.c_int
    lib.htp_init_ref_path_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_init_ref_path_last_ms.restype = ctypes.c_double
    lib.htp_obca_points_sizes.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int64)] * 4
    lib.htp_obca_points_sizes.restype = ctypes.c_int
    lib.htp_obca_points_solve_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaPointsBatch),
                                                ctypes.POINTER(ObcaResult)]
    lib.htp_obca_points_solve_batch.restype = ctypes.c_int
    lib.htp_obca_points_solve_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaPointsBatch),
                                                       ctypes.POINTER(ObcaResult), ctypes.c_void_p]
    lib.htp_obca_points_solve_batch_device.restype = ctypes.c_int
    lib.htp_last_kernel_ms.argtypes = [ctypes.c_void_p]
    lib.htp_last_kernel_ms.restype = ctypes.c_double
    lib.htp_last_cycles.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    lib.htp_last_cycles.restype = ctypes.c_int
    lib.htp_rs_all_paths_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(RsPaths)]
    lib.htp_rs_all_paths_batch.restype = ctypes.c_int
    lib.htp_rs_all_paths_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                  ctypes.POINTER(RsPaths), ctypes.c_void_p, ctypes.c_void_p]
    lib.htp_rs_all_paths_batch_device.restype = ctypes.c_int
    lib.htp_rs_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_rs_last_ms.restype = ctypes.c_double
    lib.htp_hastar_search_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(HaBatch), ctypes.POINTER(HaResult)]
    lib.htp_hastar_search_batch.restype = ctypes.c_int
    lib.htp_hastar_search_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(HaBatch), ctypes.POINTER(HaResult),
                                                   ctypes.c_void_p]
    lib.htp_hastar_search_batch_device.restype = ctypes.c_int
    lib.htp_hastar_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_hastar_last_ms.restype = ctypes.c_double
    lib.htp_ypark_search_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(YpBatch), ctypes.POINTER(YpResult)]
    lib.htp_ypark_search_batch.restype = ctypes.c_int
    lib.htp_ypark_search_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(YpBatch), ctypes.POINTER(YpResult),
                                                  ctypes.c_void_p]
    lib.htp_ypark_search_batch_device.restype = ctypes.c_int
    lib.htp_ypark_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_ypark_last_ms.restype = ctypes.c_double
    lib.htp_queue_create.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.htp_queue_create.restype = ctypes.c_void_p
    lib.htp_queue_destroy.argtypes = [ctypes.c_void_p]
    lib.htp_queue_destroy.restype = None
    lib.htp_queue_publish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    lib.htp_queue_publish.restype = ctypes.c_int
    lib.htp_queue_close.argtypes = [ctypes.c_void_p]
    lib.htp_queue_close.restype = ctypes.c_int
    lib.htp_queue_published.argtypes = [ctypes.c_void_p]
    lib.htp_queue_published.restype = ctypes.c_int64
    lib.htp_queue_claimed.argtypes = [ctypes.c_void_p]
    lib.htp_queue_claimed.restype = ctypes.c_int64
    lib.htp_obca_solve_queue_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch), ctypes.c_void_p,
                                                ctypes.POINTER(ObcaResult), ctypes.c_void_p, ctypes.c_int32,
                                                ctypes.c_double]
    lib.htp_obca_solve_queue_device.restype = ctypes.c_int
    lib.htp_obca_resident_waves.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch)]
    lib.htp_obca_resident_waves.restype = ctypes.c_int32
    lib.htp_oge_obstacles_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(OgeBatch), ctypes.POINTER(OgeResult)]
    lib.htp_oge_obstacles_batch.restype = ctypes.c_int
    lib.htp_oge_obstacles_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(OgeBatch),
                                                   ctypes.POINTER(OgeResult), ctypes.c_void_p]
    lib.htp_oge_obstacles_batch_device.restype = ctypes.c_int
    lib.htp_oge_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_oge_last_ms.restype = ctypes.c_double
    lib.htp_classic_turn_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(CtBatch), ctypes.POINTER(CtResult)]
    lib.htp_classic_turn_batch.restype = ctypes.c_int
    lib.htp_classic_turn_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(CtBatch), ctypes.POINTER(CtResult),
                                                  ctypes.c_void_p]
    lib.htp_classic_turn_batch_device.restype = ctypes.c_int
    lib.htp_classic_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_classic_last_ms.restype = ctypes.c_double
    lib.htp_orchard_chain_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ChainBatch), ctypes.c_void_p]
    lib.htp_orchard_chain_device.restype = ctypes.c_int
    lib.htp_chain_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_chain_last_ms.restype = ctypes.c_double
    lib.htp_libm_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 3 + \
        [ctypes.c_int64, ctypes.c_void_p]
    lib.htp_libm_batch_device.restype = ctypes.c_int
    if hasattr(lib, "htp_obca_audit_batch"):   # absent from libraries built before it (A/B variants of old kernels)
        lib.htp_obca_audit_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch), ctypes.c_void_p,
                                             ctypes.POINTER(AuditOpts), ctypes.POINTER(AuditResult)]
        lib.htp_obca_audit_batch.restype = ctypes.c_int
        lib.htp_obca_audit_batch_device.argtypes = lib.htp_obca_audit_batch.argtypes + [ctypes.c_void_p]
        lib.htp_obca_audit_batch_device.restype = ctypes.c_int
        lib.htp_obca_audit_last_ms.argtypes = [ctypes.c_void_p]
        lib.htp_obca_audit_last_ms.restype = ctypes.c_double
    if hasattr(lib, "htp_obca_timeline_batch"):   # likewise
        lib.htp_obca_timeline_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch), ctypes.c_void_p,
                                                ctypes.POINTER(TimelineOpts), ctypes.POINTER(TimelineResult)]
        lib.htp_obca_timeline_batch.restype = ctypes.c_int
        lib.htp_obca_timeline_batch_device.argtypes = lib.htp_obca_timeline_batch.argtypes + [ctypes.c_void_p]
        lib.htp_obca_timeline_batch_device.restype = ctypes.c_int
        lib.htp_obca_timeline_last_ms.argtypes = [ctypes.c_void_p]
        lib.htp_obca_timeline_last_ms.restype = ctypes.c_double
    if hasattr(lib, "htp_obca_repair_batch"):   # likewise
        P = ctypes.POINTER
        lib.htp_obca_repair_pack_batch.argtypes = [ctypes.c_void_p, P(ObcaBatch), P(ObcaResult), P(AuditResult),
                                                   P(RepairOpts), P(RepairState), P(RepairSlots)]
        lib.htp_obca_repair_merge_batch.argtypes = [ctypes.c_void_p, P(ObcaBatch), P(RepairSlots), P(ObcaResult),
                                                    P(AuditResult), P(ObcaResult), P(AuditResult), P(RepairState),
                                                    ctypes.c_void_p]
        lib.htp_obca_repair_batch.argtypes = [ctypes.c_void_p, P(ObcaBatch), P(ObcaResult), P(RepairOpts),
                                              P(AuditResult), P(RepairReport)]
        for n in ("pack_batch", "merge_batch", "batch"):
            f = getattr(lib, "htp_obca_repair_" + n)
            f.restype = ctypes.c_int
            g = getattr(lib, "htp_obca_repair_" + n + "_device")
            g.argtypes = f.argtypes + [ctypes.c_void_p]
            g.restype = ctypes.c_int
        lib.htp_obca_repair_last_ms.argtypes = [ctypes.c_void_p, _dp, _dp]
        lib.htp_obca_repair_last_ms.restype = ctypes.c_int
    if hasattr(lib, "htp_obca_envelope_batch"):   # likewise
        lib.htp_obca_envelope_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch), ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.POINTER(EnvelopeOpts),
                                                ctypes.POINTER(EnvelopeResult)]
        lib.htp_obca_envelope_batch.restype = ctypes.c_int
        lib.htp_obca_envelope_batch_device.argtypes = lib.htp_obca_envelope_batch.argtypes + [ctypes.c_void_p]
        lib.htp_obca_envelope_batch_device.restype = ctypes.c_int
        lib.htp_obca_envelope_last_ms.argtypes = [ctypes.c_void_p]
        lib.htp_obca_envelope_last_ms.restype = ctypes.c_double
    if hasattr(lib, "htp_obca_track_batch"):   # likewise
        lib.htp_obca_track_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch), ctypes.c_void_p,
                                             ctypes.POINTER(TrackOpts), ctypes.POINTER(TrackResult)]
        lib.htp_obca_track_batch.restype = ctypes.c_int
        lib.htp_obca_track_batch_device.argtypes = lib.htp_obca_track_batch.argtypes + [ctypes.c_void_p]
        lib.htp_obca_track_batch_device.restype = ctypes.c_int
        lib.htp_obca_track_last_ms.argtypes = [ctypes.c_void_p]
        lib.htp_obca_track_last_ms.restype = ctypes.c_double
    if hasattr(lib, "htp_obca_lqr_batch"):   # likewise
        lib.htp_obca_lqr_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch), ctypes.c_void_p,
                                           ctypes.POINTER(LqrOpts), ctypes.POINTER(LqrResult)]
        lib.htp_obca_lqr_batch.restype = ctypes.c_int
        lib.htp_obca_lqr_batch_device.argtypes = lib.htp_obca_lqr_batch.argtypes + [ctypes.c_void_p]
        lib.htp_obca_lqr_batch_device.restype = ctypes.c_int
        lib.htp_obca_lqr_last_ms.argtypes = [ctypes.c_void_p]
        lib.htp_obca_lqr_last_ms.restype = ctypes.c_double
    if hasattr(lib, "htp_obca_ltrack_batch"):   # likewise
        lib.htp_obca_ltrack_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ObcaBatch), ctypes.c_void_p,
                                              ctypes.POINTER(LtrackOpts), ctypes.POINTER(LtrackResult)]
        lib.htp_obca_ltrack_batch.restype = ctypes.c_int
        lib.htp_obca_ltrack_batch_device.argtypes = lib.htp_obca_ltrack_batch.argtypes + [ctypes.c_void_p]
        lib.htp_obca_ltrack_batch_device.restype = ctypes.c_int
        lib.htp_obca_ltrack_last_ms.argtypes = [ctypes.c_void_p]
        lib.htp_obca_ltrack_last_ms.restype = ctypes.c_double
    if hasattr(lib, "htp_mfma_f64_probe"):   # absent from libraries built before it (A/B variants of old kernels)
        lib.htp_mfma_f64_probe.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_void_p]
        lib.htp_mfma_f64_probe.restype = ctypes.c_int
    lib.htp_classic_sample_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(SmpIn), ctypes.POINTER(SmpResult)]
    lib.htp_classic_sample_batch.restype = ctypes.c_int
    lib.htp_classic_sample_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(SmpIn), ctypes.POINTER(SmpResult),
                                                    ctypes.c_void_p]
    lib.htp_classic_sample_batch_device.restype = ctypes.c_int
    lib.htp_classic_sample_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_classic_sample_last_ms.restype = ctypes.c_double
    lib.htp_speed_profile_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(SpdIn), ctypes.POINTER(SpdResult)]
    lib.htp_speed_profile_batch.restype = ctypes.c_int
    lib.htp_speed_profile_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(SpdIn), ctypes.POINTER(SpdResult),
                                                   ctypes.c_void_p]
    lib.htp_speed_profile_batch_device.restype = ctypes.c_int
    lib.htp_speed_profile_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_speed_profile_last_ms.restype = ctypes.c_double
    lib.htp_pose_clearance_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ClrIn), ctypes.POINTER(ClrResult)]
    lib.htp_pose_clearance_batch.restype = ctypes.c_int
    lib.htp_pose_clearance_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ClrIn), ctypes.POINTER(ClrResult),
                                                    ctypes.c_void_p]
    lib.htp_pose_clearance_batch_device.restype = ctypes.c_int
    lib.htp_pose_clearance_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_pose_clearance_last_ms.restype = ctypes.c_double
    lib.htp_turn_select_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(SelIn), ctypes.POINTER(SelResult)]
    lib.htp_turn_select_batch.restype = ctypes.c_int
    lib.htp_turn_select_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(SelIn), ctypes.POINTER(SelResult),
                                                 ctypes.c_void_p]
    lib.htp_turn_select_batch_device.restype = ctypes.c_int
    lib.htp_turn_select_last_ms.argtypes = [ctypes.c_void_p]
    lib.htp_turn_select_last_ms.restype = ctypes.c_double
    if hasattr(lib, "htp_bk_probe"):   # likewise
        lib.htp_bk_probe.argtypes = [ctypes.c_void_p] + BK_PROBE_ARGS + [ctypes.c_void_p]
        lib.htp_bk_probe.restype = ctypes.c_int
    return lib


# htp_bk_probe (csrc/bk_probe.h) after the context: variant, n, lane_stride, count, nrhs, then K0, rhs, K, ip, flags,
# x, x2; the test-only host builds of the same body take exactly these
BK_PROBE_ARGS = [ctypes.c_int32] * 3 + [ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 7
BK_SENTINEL = -7.25e300   # pre-fill of the probe's double outputs (ints: -77): what a form leaves untouched stays so


def bk_probe_sizes(variant, n):
    """Doubles per block of htp_bk_probe's input matrix and of its factor (bk_probe.h in_doubles / out_doubles)."""
    if variant == 6:
        return 9, 9
    if variant == 7:
        return 25, 15
    return n * (n + 1) // 2, n * (n + 1) // 2


def bk_probe_outputs(variant, n, rows, nrhs):
    """Sentinel-filled host outputs of `rows` blocks: K, ip, flags, x, x2."""
    _, vo = bk_probe_sizes(variant, n)
    return (np.full((rows, vo), BK_SENTINEL), np.full((rows, n), -77, np.int32), np.full((rows, 4), -77, np.int32),
            np.full((rows, nrhs, n), BK_SENTINEL), np.full((rows, nrhs, n), BK_SENTINEL))


# correctly rounded libm of the planner cores (csrc/htp_libm.h): function ids of htp_libm_batch_device
LIBM_FN = {"sin": 0, "cos": 1, "tan": 2, "atan": 3, "atan2": 4, "asin": 5, "acos": 6, "hypot": 7, "pow": 8, "log": 9,
           "fast_log": 10, "fast_sin": 11, "fast_cos": 12, "fast_tan": 13}
LIBM_BINARY = {"atan2", "hypot", "pow"}
CPU_LIB_PATH = os.path.join(HERE, "libhtp_cpu.so")
_CPU_LIB = None


def cpu_lib():
    """libhtp_cpu.so: the g++ build of the same cores (CPU baseline, workload generator, host twins)."""
    global _CPU_LIB
    if _CPU_LIB is None:
        if not os.path.exists(CPU_LIB_PATH):
            raise RuntimeError(f"[htp] CPU library not built: {CPU_LIB_PATH} (run __graft_entry__.build())")
        lib = ctypes.CDLL(CPU_LIB_PATH)
        lib.htp_cpu_libm_batch.argtypes = [ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_int64]
        lib.htp_cpu_libm_batch.restype = ctypes.c_int
        _CPU_LIB = lib
    return _CPU_LIB


def cpu_libm(name, x, y=None):
    """Host build of the planner libm: name in LIBM_FN, x (and y) float64 arrays -> float64 array."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    yy = np.ascontiguousarray(np.broadcast_to(y, x.shape), dtype=np.float64) if y is not None else None
    if name in LIBM_BINARY and yy is None:
        raise ValueError(f"[htp] {name} needs two arguments")
    out = np.empty_like(x)
    rc = cpu_lib().htp_cpu_libm_batch(LIBM_FN[name], x.ctypes.data, yy.ctypes.data if yy is not None else None,
                                      out.ctypes.data, x.size)
    if rc != 0:
        raise RuntimeError("[htp] htp_cpu_libm_batch failed")
    return out


_LIB = None


def core_sha():
    """Short hash of the OBCA solver sources (ties profiles/*_traffic.json to a solver version)."""
    import hashlib
    h = hashlib.sha256()
    for f in ("obca_core.h", "htp_common.h", "htp_obca.hip", "dyn_gen.h", "wave_ctx.h", "htp_fastm.h", "htp_libm.h"):
        with open(os.path.join(HERE, "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:12]


def load(path=LIB_PATH):
    """Load the in-tree HIP library; raise loudly if it is absent."""
    global _LIB
    if _LIB is not None and path == LIB_PATH:
        return _LIB
    if not os.path.exists(path):
        raise RuntimeError(f"[htp] HIP library not built: {path} (run __graft_entry__.build())")
    # torch wheels bundle their own libamdhip64.so.7 (same SONAME as /opt/rocm's).
    # Whichever is loaded first serves the whole process; loading torch's first
    # keeps torch.cuda working when callers import torch after this library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = _declare(ctypes.CDLL(path))
    if path == LIB_PATH:
        _LIB = lib
    return lib


def sizes(N, M, K, time_opt, obs_edges, body_edges, lib=None):
    lib = lib or load()
    eo = np.ascontiguousarray(obs_edges, dtype=np.int32)
    eb = np.ascontiguousarray(body_edges, dtype=np.int32)
    out = [ctypes.c_int64() for _ in range(4)]
    rc = lib.htp_obca_sizes(N, M, K, int(time_opt), eo.ctypes.data, eb.ctypes.data, *[ctypes.byref(v) for v in out])
    if rc != 0:
        raise ValueError("[OBCA] invalid problem shape")
    return tuple(v.value for v in out)


# ------------------------------------------------------------------ packing
def params_of(inst):
    p = np.zeros(NPARAM)
    Q, R, W = (np.asarray(inst[k], dtype=np.float64) for k in ("Q", "R", "W"))
    p[P_DT] = inst["dT"]
    p[P_Q00:P_Q11 + 1] = Q.reshape(-1)[:4]
    p[P_R00:P_R11 + 1] = R.reshape(-1)[:4]
    p[P_W00], p[P_W11] = W[0, 0], W[1, 1]
    p[P_WHEELBASE] = inst["wheelbase"]
    p[P_MAXSTEER] = inst["max_steer"]
    p[P_MAXV] = inst["max_velocity"]
    p[P_MAXACC] = inst["max_accel"]
    p[P_MAXSR] = inst["max_steer_rate"]
    dmin = inst.get("min_dist", 0.1)
    p[P_DMIN] = 0.1 if (dmin is None or dmin < 0) else dmin
    xb = inst.get("x_bound", [-np.inf, np.inf])
    yb = inst.get("y_bound", [-np.inf, np.inf])
    p[P_XLO], p[P_XHI], p[P_YLO], p[P_YHI] = xb[0], xb[1], yb[0], yb[1]
    p[P_HAS_INIT_CONTROL] = inst.get("init_control") is not None
    p[P_HAS_INIT_DUAL] = inst.get("init_mu") is not None
    return p


class PackedBatch:
    """Contiguous problem-major arrays for one batch (shared shape)."""

    def __init__(self, insts):
        i0 = insts[0]
        self.batch = len(insts)
        self.N = int(np.asarray(i0["init_traj"]).shape[0])
        self.M = len(i0["obs_A"])
        self.K = len(i0["body_G"])
        self.time_opt = int(np.asarray(i0["W"])[1, 1] != 0)
        self.obs_edges = np.array([a.shape[0] for a in i0["obs_A"]], dtype=np.int32)
        self.body_edges = np.array([a.shape[0] for a in i0["body_G"]], dtype=np.int32)
        for it in insts:
            if (np.asarray(it["init_traj"]).shape[0] != self.N
                    or [a.shape[0] for a in it["obs_A"]] != list(self.obs_edges)
                    or [a.shape[0] for a in it["body_G"]] != list(self.body_edges)
                    or int(np.asarray(it["W"])[1, 1] != 0) != self.time_opt):
                raise ValueError("[OBCA] all problems of a batch must share N, edge counts and time_opt")
        B = self.batch
        self.traj = np.ascontiguousarray(np.stack([np.asarray(it["init_traj"], dtype=np.float64) for it in insts]))
        self.obs_A = np.ascontiguousarray(np.stack([np.concatenate(it["obs_A"], axis=0) for it in insts]))
        self.obs_b = np.ascontiguousarray(np.stack([np.concatenate(it["obs_b"]) for it in insts]))
        self.body_G = np.ascontiguousarray(np.stack([np.concatenate(it["body_G"], axis=0) for it in insts]))
        self.body_g = np.ascontiguousarray(np.stack([np.concatenate(it["body_g"]) for it in insts]))
        self.params = np.ascontiguousarray(np.stack([params_of(it) for it in insts]))
        self.init_control = self._opt(insts, "init_control")
        self.init_mu = self._opt(insts, "init_mu")
        self.init_lambda = self._opt(insts, "init_lambda")
        TEo, TEb = int(self.obs_edges.sum()), int(self.body_edges.sum())
        self.mu_count, self.lam_count = TEb * self.M, TEo * self.K
        self.n_var = 5 * self.N + 2 * (self.N - 1) + self.N * (self.mu_count + self.lam_count) + \
            (self.N - 1) * self.time_opt + 5
        _ = B

    @staticmethod
    def _opt(insts, key):
        vals = [it.get(key) for it in insts]
        if all(v is None for v in vals):
            return None
        if any(v is None for v in vals):
            raise ValueError(f"[OBCA] {key} must be given for all or none of the problems")
        return np.ascontiguousarray(np.stack([np.asarray(v, dtype=np.float64) for v in vals]))

    def struct(self, ptrs=None):
        """ctypes htp_obca_batch over host arrays (or the given device pointers)."""
        def ptr(a):
            return None if a is None else a.ctypes.data
        b = ObcaBatch()
        b.batch, b.N, b.M, b.K, b.time_opt = self.batch, self.N, self.M, self.K, self.time_opt
        b.obs_edges, b.body_edges = self.obs_edges.ctypes.data, self.body_edges.ctypes.data
        src = ptrs or {}
        for name in ("traj", "obs_A", "obs_b", "body_G", "body_g", "params", "init_control", "init_mu", "init_lambda"):
            setattr(b, name, src[name] if name in src else ptr(getattr(self, name)))
        return b

    INPUTS = ("traj", "obs_A", "obs_b", "body_G", "body_g", "params", "init_control", "init_mu", "init_lambda")

    def chunk_struct(self, ptrs, lo, hi):
        """htp_obca_batch of problems [lo, hi) over base pointers `ptrs` (device or
        host) laid out like this batch's arrays (problem-major)."""
        b = self.struct(ptrs)
        b.batch = int(hi - lo)
        for name in self.INPUTS:
            a = getattr(self, name)
            base = ptrs[name] if name in ptrs else (None if a is None else a.ctypes.data)
            setattr(b, name, None if base is None else base + int(lo) * a.strides[0])
        return b

    @classmethod
    def concat(cls, parts):
        """One batch from same-shape PackedBatches (problem order kept)."""
        out = cls.__new__(cls)
        out.__dict__.update(parts[0].__dict__)
        out.batch = sum(p.batch for p in parts)
        for name in cls.INPUTS:
            a = [getattr(p, name) for p in parts]
            setattr(out, name, None if a[0] is None else np.ascontiguousarray(np.concatenate(a, axis=0)))
        return out


class ObcaPointsBatch(ctypes.Structure):  # htp_obca_points_batch
    _fields_ = [("batch", ctypes.c_int32), ("N", ctypes.c_int32), ("M", ctypes.c_int32),
                ("n_vertices", ctypes.c_int32), ("obs_edges", ctypes.c_void_p), ("traj", ctypes.c_void_p),
                ("obs_A", ctypes.c_void_p), ("obs_b", ctypes.c_void_p), ("vertices", ctypes.c_void_p),
                ("params", ctypes.c_void_p), ("init_control", ctypes.c_void_p)]


def points_params_of(inst):
    """HTP_P_* slots of a point-formulation instance (oracle/nlp_points.py format)."""
    p = np.zeros(NPARAM)
    p[P_DT] = inst["dT"]
    p[P_WHEELBASE] = inst["wheelbase"]
    p[P_MAXSTEER] = inst["max_steer"]
    p[P_MAXV] = inst["max_velocity"]
    p[P_MAXACC] = inst["max_accel"]
    p[P_MAXSR] = inst["max_steer_rate"]
    p[P_DMIN] = inst["min_dist"]
    xb = inst.get("x_bound", [-9999999, 9999999])
    yb = inst.get("y_bound", [-9999999, 9999999])
    p[P_XLO], p[P_XHI], p[P_YLO], p[P_YHI] = xb[0], xb[1], yb[0], yb[1]
    p[P_HAS_INIT_CONTROL] = inst.get("init_control") is not None
    return p


class PointsPackedBatch:
    """Contiguous problem-major arrays of a batch of point-formulation problems
    (R/obca_py/optimizer_points.py); all share N, obstacle edge counts and the
    number of hull vertices."""

    def __init__(self, insts):
        i0 = insts[0]
        self.batch = len(insts)
        self.N = int(np.asarray(i0["init_traj"]).shape[0])
        self.M = len(i0["obs_A"])
        self.n_vertices = int(np.asarray(i0["vertices"]).shape[0])
        self.obs_edges = np.array([a.shape[0] for a in i0["obs_A"]], dtype=np.int32)
        for it in insts:
            if (np.asarray(it["init_traj"]).shape[0] != self.N
                    or [a.shape[0] for a in it["obs_A"]] != list(self.obs_edges)
                    or np.asarray(it["vertices"]).shape[0] != self.n_vertices):
                raise ValueError("[OBCA points] all problems of a batch must share N, edge and vertex counts")
        self.traj = np.ascontiguousarray(np.stack([np.asarray(it["init_traj"], dtype=np.float64) for it in insts]))
        self.obs_A = np.ascontiguousarray(np.stack([np.concatenate(it["obs_A"], axis=0) for it in insts]))
        self.obs_b = np.ascontiguousarray(np.stack([np.concatenate(it["obs_b"]) for it in insts]))
        self.vertices = np.ascontiguousarray(np.stack([np.asarray(it["vertices"], dtype=np.float64) for it in insts]))
        self.params = np.ascontiguousarray(np.stack([points_params_of(it) for it in insts]))
        self.init_control = PackedBatch._opt(insts, "init_control")
        self.n_var = 5 * self.N + 2 * (self.N - 1) + self.N * int(self.obs_edges.sum())

    def struct(self, ptrs=None):
        def ptr(a):
            return None if a is None else a.ctypes.data
        b = ObcaPointsBatch()
        b.batch, b.N, b.M, b.n_vertices = self.batch, self.N, self.M, self.n_vertices
        b.obs_edges = self.obs_edges.ctypes.data
        src = ptrs or {}
        for name in ("traj", "obs_A", "obs_b", "vertices", "params", "init_control"):
            setattr(b, name, src[name] if name in src else ptr(getattr(self, name)))
        return b


class RpBatch(ctypes.Structure):  # htp_refpath_batch
    _fields_ = [("batch", ctypes.c_int32), ("cap_points", ctypes.c_int32), ("cap_rows", ctypes.c_int32),
                ("path_off", ctypes.c_void_p), ("xs", ctypes.c_void_p), ("ys", ctypes.c_void_p),
                ("dirs", ctypes.c_void_p), ("params", ctypes.c_void_p)]


class RpResult(ctypes.Structure):  # htp_refpath_result
    _fields_ = [("status", ctypes.c_void_p), ("n_rows", ctypes.c_void_p), ("traj", ctypes.c_void_p)]


RP_STATUS = {0: "ok", 1: "overflow", 2: "bad_segment", 3: "bad_input"}


class RefPathPacked:
    """CSR batch of warm-start paths for get_init_ref_path (R/obca_py/util.py:62-113).
    paths: list of (xs, ys, dirs) (yaw / curvature columns are not read by the reference);
    params: per path (WHEEL_BASE, desired_v, ds)."""

    def __init__(self, paths, params, cap_rows=None):
        self.batch = len(paths)
        lens = [len(p[0]) for p in paths]
        self.path_off = np.zeros(self.batch + 1, dtype=np.int32)
        self.path_off[1:] = np.cumsum(lens)
        cat = lambda k: np.ascontiguousarray(np.concatenate([np.asarray(p[k], dtype=np.float64) for p in paths])
                                             if paths else np.zeros(1))
        self.xs, self.ys, self.dirs = cat(0), cat(1), cat(2)
        self.params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(self.batch, 3))
        self.cap_points = max(1, max(lens) if lens else 1)
        if cap_rows is None:  # arc length <= polyline length: ceil(len/ds) + 1 rows per segment, + 1 per segment
            cap_rows = 1
            for p, prm in zip(paths, self.params):
                L = float(np.sum(np.hypot(np.diff(p[0]), np.diff(p[1]))))
                nseg = 1 + int(np.count_nonzero(np.diff(np.asarray(p[2])) != 0))
                cap_rows = max(cap_rows, int(np.ceil(L / prm[2])) + 2 * nseg + 2)
        self.cap_rows = int(cap_rows)

    def struct(self, ptrs=None):
        b = RpBatch()
        b.batch, b.cap_points, b.cap_rows = self.batch, self.cap_points, self.cap_rows
        src = ptrs or {}
        for name in ("path_off", "xs", "ys", "dirs", "params"):
            setattr(b, name, src[name] if name in src else getattr(self, name).ctypes.data)
        return b


class RefPathResults:
    def __init__(self, packed):
        self.status = np.zeros(packed.batch, dtype=np.int32)
        self.n_rows = np.zeros(packed.batch, dtype=np.int32)
        self.traj = np.zeros((packed.batch, packed.cap_rows, 5))

    def struct(self):
        return RpResult(self.status.ctypes.data, self.n_rows.ctypes.data, self.traj.ctypes.data)

    def path(self, b):
        return self.traj[b, :self.n_rows[b]].copy()


class HostResults:
    def __init__(self, batch, n_var):
        self.x = np.zeros((batch, n_var))
        self.objective = np.zeros(batch)
        self.status = np.zeros(batch, dtype=np.int32)
        self.iterations = np.zeros(batch, dtype=np.int32)
        self.n_factor = np.zeros(batch, dtype=np.int32)
        self.nlp_error = np.zeros(batch)
        self.n_resto = np.zeros(batch, dtype=np.int32)

    def struct(self):
        r = ObcaResult()
        for name in ("x", "objective", "status", "iterations", "n_factor", "nlp_error", "n_resto"):
            setattr(r, name, getattr(self, name).ctypes.data)
        return r


def _clean_ring(poly):
    """Vertices without the repeated closing vertex or consecutive duplicates."""
    a = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
    keep = [0]
    for i in range(1, a.shape[0]):
        if not np.array_equal(a[i], a[keep[-1]]):
            keep.append(i)
    a = a[keep]
    if a.shape[0] > 1 and np.array_equal(a[0], a[-1]):
        a = a[:-1]
    return a


def _ccw(a):
    area = np.sum(a[:, 0] * np.roll(a[:, 1], -1) - np.roll(a[:, 0], -1) * a[:, 1])
    return a if area > 0 else a[::-1].copy()


class HastarPacked:
    """htp_hastar_batch pools for a list of lowered hybrid A* problems (dicts
    made by path_planner.hybrid_a_star_search.lower_problem)."""

    def __init__(self, probs, cap_path=4096, cap_log=None):
        B = len(probs)
        polys, lane_len, guides, motions = [], [], [], []
        self.params = np.zeros((B, HA_NPARAM))
        self.desc = np.zeros((B, HA_NDESC), dtype=np.int32)
        ng = nm = 0
        for b, p in enumerate(probs):
            d = self.desc[b]
            d[HA_D_BODY] = len(polys)
            polys.append(_clean_ring(p["body"]))
            lane_len.append(0.0)
            d[HA_D_BLK0] = len(polys)
            for q in p["blockers"]:
                polys.append(_clean_ring(q))
                lane_len.append(0.0)
            d[HA_D_BLK1] = len(polys)
            d[HA_D_LANE0] = len(polys)
            for q, L in zip(p["lanes"], p["search_lengths"]):
                polys.append(_ccw(_clean_ring(q)))
                lane_len.append(float(L))
            d[HA_D_LANE1] = len(polys)
            if p["field"] is None:
                d[HA_D_FIELD] = -1
            else:
                d[HA_D_FIELD] = len(polys)
                polys.append(_clean_ring(p["field"]))
                lane_len.append(0.0)
            g = np.asarray(p["guide"], dtype=np.float64).reshape(-1, 4)
            d[HA_D_GUIDE0], d[HA_D_GUIDE1] = ng, ng + g.shape[0]
            guides.append(g)
            ng += g.shape[0]
            m = np.asarray(p["motions"], dtype=np.float64).reshape(-1, 2)
            d[HA_D_MOT0], d[HA_D_MOT1] = nm, nm + m.shape[0]
            motions.append(m)
            nm += m.shape[0]
            d[HA_D_KING] = 1 if p.get("king", True) else 0
            pr = self.params[b]
            pr[HA_P_SX:HA_P_SYAW + 1] = np.asarray(p["start"], dtype=np.float64)[:3]
            pr[HA_P_GX:HA_P_GYAW + 1] = np.asarray(p["goal"], dtype=np.float64)[:3]
            pr[HA_P_RES], pr[HA_P_YAWRES] = p["res"], p["yaw_res"]
            pr[HA_P_WB], pr[HA_P_MAXSTEER], pr[HA_P_CURV] = p["wheel_base"], p["max_steer"], p["curvature"]
            pr[HA_P_DEFLEN], pr[HA_P_MAXNODES] = p["default_search_length"], p["max_nodes"]
        self.batch = B
        self.poly_off = np.zeros(len(polys) + 1, dtype=np.int32)
        self.poly_off[1:] = np.cumsum([q.shape[0] for q in polys])
        self.vertices = np.ascontiguousarray(np.concatenate(polys, axis=0))
        self.lane_len = np.array(lane_len, dtype=np.float64)
        self.guide = np.ascontiguousarray(np.concatenate(guides, axis=0))
        self.motions = np.ascontiguousarray(np.concatenate(motions, axis=0))
        self.max_nodes_cap = int(max(int(p["max_nodes"]) for p in probs)) if B else 0
        self.cap_path = int(cap_path)
        self.cap_log = int(self.max_nodes_cap + 2 if cap_log is None else cap_log)

    def struct(self, ptrs=None):
        src = ptrs or {}
        b = HaBatch()
        b.batch, b.npoly, b.nvert = self.batch, len(self.poly_off) - 1, self.vertices.shape[0]
        b.nguide, b.nmotion = self.guide.shape[0], self.motions.shape[0]
        for n in ("params", "desc", "poly_off", "vertices", "lane_len", "guide", "motions"):
            setattr(b, n, src[n] if n in src else getattr(self, n).ctypes.data)
        b.max_nodes_cap, b.cap_path, b.cap_log = self.max_nodes_cap, self.cap_path, self.cap_log
        return b


class HastarResults:
    def __init__(self, packed):
        B, cp, cl = packed.batch, packed.cap_path, packed.cap_log
        self.status = np.zeros(B, np.int32)
        self.counter = np.zeros(B, np.int32)
        self.n_path = np.zeros(B, np.int32)
        self.n_expanded = np.zeros(B, np.int32)
        self.n_pose = np.zeros(B, np.int64)
        for n in ("x", "y", "yaw", "dir", "k"):
            setattr(self, n, np.zeros((B, cp)))
        self.expanded = np.zeros((B, cl, 3), np.int32)

    def struct(self):
        r = HaResult()
        for n in ("status", "counter", "n_path", "n_expanded", "n_pose", "x", "y", "yaw", "dir", "k", "expanded"):
            setattr(r, n, getattr(self, n).ctypes.data)
        return r

    def path(self, b):
        """(xs, ys, yaws, dirs, ks) of search b as lists (truncated to cap_path)."""
        n = min(int(self.n_path[b]), self.x.shape[1])
        return tuple(getattr(self, k)[b, :n].tolist() for k in ("x", "y", "yaw", "dir", "k"))

    def expansions(self, b):
        n = min(int(self.n_expanded[b]), self.expanded.shape[1])
        return [tuple(int(v) for v in r) for r in self.expanded[b, :n]]


class YparkPacked:
    """htp_ypark_batch pools for lowered Y-park searches (dicts made by
    path_planner.headland_path_planning.lower_ypark)."""

    def __init__(self, probs, cap_path=256):
        B = len(probs)
        polys, axis = [], []
        self.params = np.zeros((B, YP_NPARAM))
        self.desc = np.zeros((B, YP_NDESC), dtype=np.int32)
        for b, p in enumerate(probs):
            d = self.desc[b]
            d[0] = len(polys)
            polys.append(_clean_ring(p["body"]))
            d[1] = len(polys)
            for q in p["blockers"]:
                polys.append(_clean_ring(q))
            d[2] = len(polys)
            if p["field"] is None:
                d[3] = -1
            else:
                d[3] = len(polys)
                polys.append(_clean_ring(p["field"]))
            for a, key in enumerate(("backward_lengths", "forward_lengths", "backward_steers", "forward_steers")):
                vals = np.asarray(p[key], dtype=np.float64).reshape(-1)
                d[4 + 2 * a], d[5 + 2 * a] = len(axis), vals.size
                axis.extend(vals.tolist())
            self.params[b, :14] = [p["end_pose"][0], p["end_pose"][1], p["end_pose"][2], p["backward_steer_dir"],
                                   p["forward_steer_dir"], p["wheel_base"], p["step"], p["T"][0][0], p["T"][0][1],
                                   p["T"][1][0], p["T"][1][1], p["T"][0][3], p["T"][1][3], p["yaw_odom"]]
        self.batch = B
        self.poly_off = np.zeros(len(polys) + 1, dtype=np.int32)
        self.poly_off[1:] = np.cumsum([q.shape[0] for q in polys])
        self.vertices = np.ascontiguousarray(np.concatenate(polys, axis=0))
        self.axis = np.array(axis, dtype=np.float64)
        self.cap_path = int(cap_path)

    def struct(self, ptrs=None):
        src = ptrs or {}
        b = YpBatch()
        b.batch, b.npoly, b.nvert, b.naxis = self.batch, len(self.poly_off) - 1, self.vertices.shape[0], self.axis.size
        for n in ("params", "desc", "poly_off", "vertices", "axis"):
            setattr(b, n, src[n] if n in src else getattr(self, n).ctypes.data)
        b.cap_path = self.cap_path
        return b


class YparkResults:
    def __init__(self, packed):
        B = packed.batch
        self.status = np.zeros(B, np.int32)
        self.cand = np.zeros(B, np.int32)
        self.n_path = np.zeros(B, np.int32)
        self.params = np.zeros((B, 4))
        self.n_pose = np.zeros(B, np.int64)
        self.path = np.zeros((B, packed.cap_path, 5))

    def struct(self):
        r = YpResult()
        for n in ("status", "cand", "n_path", "params", "n_pose", "path"):
            setattr(r, n, getattr(self, n).ctypes.data)
        return r


# ------------------------------------------------------- orchard scene -> OBCA obstacles (htp_oge.hip)
OGE_NPARAM, OGE_MAXROWS, OGE_MAXPOLY, OGE_MAXV = 16, 32, 32, 12
OGE_STATUS = {0: "ok", 1: "bad_input", 2: "no_row_between", 3: "overflow", 4: "empty_side"}


class OgeBatch(ctypes.Structure):  # htp_oge_batch
    _fields_ = [("batch", ctypes.c_int32), ("max_rows", ctypes.c_int32), ("params", ctypes.c_void_p),
                ("row_draws", ctypes.c_void_p), ("eps_draws", ctypes.c_void_p)]


class OgeResult(ctypes.Structure):  # htp_oge_result
    _fields_ = [("status", ctypes.c_void_p), ("n_poly", ctypes.c_void_p), ("n_vert", ctypes.c_void_p),
                ("vertices", ctypes.c_void_p), ("n_facet", ctypes.c_void_p), ("A", ctypes.c_void_p),
                ("b", ctypes.c_void_p)]


class OgePacked:
    """Scenes for htp_oge_obstacles_batch.  A scene is a dict with nrows, row_width, row_length, slope,
    tree_width, headland_width, start, end, side (1 NEAR / -1 FAR) and the reference's random draws:
    row_draws (create_tree_rows, one per row) and eps_draws (create_headland_countour_lines, one per row)."""

    def __init__(self, scenes):
        B = len(scenes)
        self.batch = B
        self.max_rows = max(3, max((int(s["nrows"]) for s in scenes), default=3))
        if self.max_rows > OGE_MAXROWS:
            raise ValueError(f"[oge] at most {OGE_MAXROWS} tree rows per scene")
        self.params = np.zeros((B, OGE_NPARAM))
        self.row_draws = np.zeros((B, self.max_rows))
        self.eps_draws = np.zeros((B, self.max_rows))
        for b, s in enumerate(scenes):
            n = int(s["nrows"])
            self.params[b, :13] = [n, s["row_width"], s["row_length"], s["slope"], s["tree_width"],
                                   s["headland_width"], *np.asarray(s["start"], dtype=np.float64)[:3],
                                   *np.asarray(s["end"], dtype=np.float64)[:3], s.get("side", 1)]
            self.row_draws[b, :n] = s["row_draws"]
            self.eps_draws[b, :n] = s["eps_draws"]

    def struct(self, ptrs=None):
        p = ptrs or {}
        return OgeBatch(self.batch, self.max_rows, p.get("params", self.params.ctypes.data),
                        p.get("row_draws", self.row_draws.ctypes.data), p.get("eps_draws", self.eps_draws.ctypes.data))


class OgeResults:
    def __init__(self, batch, halfspaces=True):
        B = batch
        self.status = np.zeros(B, np.int32)
        self.n_poly = np.zeros(B, np.int32)
        self.n_vert = np.zeros((B, OGE_MAXPOLY), np.int32)
        self.vertices = np.zeros((B, OGE_MAXPOLY, OGE_MAXV, 2))
        self.n_facet = np.zeros((B, OGE_MAXPOLY), np.int32) if halfspaces else None
        self.A = np.zeros((B, OGE_MAXPOLY, OGE_MAXV, 2)) if halfspaces else None
        self.b = np.zeros((B, OGE_MAXPOLY, OGE_MAXV)) if halfspaces else None

    def struct(self):
        def ptr(a):
            return None if a is None else a.ctypes.data
        return OgeResult(self.status.ctypes.data, self.n_poly.ctypes.data, self.n_vert.ctypes.data,
                         self.vertices.ctypes.data, ptr(self.n_facet), ptr(self.A), ptr(self.b))

    def polygons(self, b):
        """Scene b's obstacle polygons [(n_v, 2) arrays] in the reference's order."""
        return [self.vertices[b, q, :self.n_vert[b, q]].copy() for q in range(int(self.n_poly[b]))]

    def halfspaces(self, b):
        """Scene b's [(A, b)] (compute_polytope_halfspaces of each polygon)."""
        out = []
        for q in range(int(self.n_poly[b])):
            f = int(self.n_facet[b, q])
            out.append((self.A[b, q, :f].copy(), self.b[b, q, :f].copy()))
        return out


# ------------------------------------------------------------ classic headland turns (htp_classic.hip)
CT_NPARAM = 12
CT_TYPES = {"dubins": 0, "circleback": 1, "fishtail": 2}
CT_STATUS = {0: "ok", 1: "overflow", 2: "no_word", 3: "bad_input", 4: "rs_error", 5: "no_dubins"}


class CtBatch(ctypes.Structure):  # htp_classic_batch
    _fields_ = [("batch", ctypes.c_int32), ("npoly", ctypes.c_int32), ("nvert", ctypes.c_int32),
                ("params", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("poly_off", ctypes.c_void_p),
                ("vertices", ctypes.c_void_p), ("cap_path", ctypes.c_int32), ("cap_samples", ctypes.c_int32)]


class CtResult(ctypes.Structure):  # htp_classic_result
    _fields_ = [("status", ctypes.c_void_p), ("n_path", ctypes.c_void_p), ("path", ctypes.c_void_p)]


class ClassicPacked:
    """Turns for htp_classic_turn_batch.  A turn is a dict: type ("dubins" / "circleback" / "fishtail"), side
    (map_utils NEAR_SIDE 1 / FAR_SIDE 2), start, end (x, y, yaw), wheel_base, max_steer, radius (the planners'
    turning-radius argument), step, body (car_poly ring), blockers (obs_poly_list rings; fish-tail only)."""

    def __init__(self, turns, cap_path=4096, cap_samples=4096):
        B = len(turns)
        self.batch, self.cap_path, self.cap_samples = B, int(cap_path), int(cap_samples)
        self.params = np.zeros((B, CT_NPARAM))
        self.desc = np.zeros((B, 3), np.int32)
        polys = []
        for b, t in enumerate(turns):
            self.params[b] = [CT_TYPES[t["type"]], t.get("side", 1), *np.asarray(t["start"], dtype=np.float64)[:3],
                              *np.asarray(t["end"], dtype=np.float64)[:3], t["wheel_base"], t["max_steer"],
                              t["radius"], t.get("step", 0.1)]
            self.desc[b, 0] = len(polys)
            polys.append(np.asarray(t["body"], dtype=np.float64).reshape(-1, 2))
            self.desc[b, 1] = len(polys)
            polys += [np.asarray(q, dtype=np.float64).reshape(-1, 2) for q in t.get("blockers", [])]
            self.desc[b, 2] = len(polys)
        self.poly_off = np.concatenate([[0], np.cumsum([len(q) for q in polys])]).astype(np.int32)
        self.vertices = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros((0, 2)))

    def struct(self, ptrs=None):
        p = ptrs or {}
        return CtBatch(self.batch, len(self.poly_off) - 1, self.vertices.shape[0],
                       p.get("params", self.params.ctypes.data), p.get("desc", self.desc.ctypes.data),
                       p.get("poly_off", self.poly_off.ctypes.data), p.get("vertices", self.vertices.ctypes.data),
                       self.cap_path, self.cap_samples)


class ClassicResults:
    def __init__(self, packed, rows=None):
        B = packed.batch if rows is None else int(rows)   # rows: storage for more turns than the batch has
        self.status = np.zeros(B, np.int32)
        self.n_path = np.zeros(B, np.int32)
        self.path = np.zeros((B, packed.cap_path, 5))

    def struct(self):
        return CtResult(self.status.ctypes.data, self.n_path.ctypes.data, self.path.ctypes.data)

    def rows(self, b):
        return self.path[b, :int(self.n_path[b])].copy()


# ------------------------------------------------------------ sampled exit / entry pose search (htp_sample.hip)
SMP_NDESC, SMP_NPOSE = 6, 8
SMP_MAX_POLY, SMP_MAX_VERT = 48, 256
SMP_TYPES = {"dubins": 0, "reeds_shepp": 1, "circle_back": 2}
SMP_OK, SMP_NONE_FEASIBLE, SMP_OVERFLOW, SMP_BAD_INPUT = 0, 1, 2, 3
SMP_STATUS = {0: "ok", 1: "none_feasible", 2: "overflow", 3: "bad_input"}
SMP_C_FEASIBLE, SMP_C_BLOCKED, SMP_C_PLANNER, SMP_C_OVERFLOW, SMP_C_BAD_INPUT, SMP_C_UNUSED = range(6)
SMP_C_STATUS = {0: "feasible", 1: "blocked", 2: "planner", 3: "overflow", 4: "bad_input", 5: "unused"}


class SmpIn(ctypes.Structure):  # htp_classic_sample_in
    _fields_ = [("batch", ctypes.c_int32), ("npoly", ctypes.c_int32), ("nvert", ctypes.c_int32),
                ("params", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("poly_off", ctypes.c_void_p),
                ("vertices", ctypes.c_void_p), ("start_x", ctypes.c_void_p), ("end_x", ctypes.c_void_p),
                ("n_start", ctypes.c_void_p), ("n_end", ctypes.c_void_p), ("cap_s", ctypes.c_int32),
                ("cap_e", ctypes.c_int32), ("cap_cand", ctypes.c_int32), ("cap_samples", ctypes.c_int32),
                ("max_groups", ctypes.c_int32)]


class SmpResult(ctypes.Structure):  # htp_classic_sample_result
    _fields_ = [("status", ctypes.c_void_p), ("winner", ctypes.c_void_p), ("poses", ctypes.c_void_p),
                ("score", ctypes.c_void_p), ("n_feasible", ctypes.c_void_p), ("cand_score", ctypes.c_void_p),
                ("cand_status", ctypes.c_void_p)]


class SamplePacked:
    """Turns for htp_classic_sample_batch.  A turn is a dict (path_planner.safety_forward_path_plan.sample_turn builds
    it): type ("dubins" / "reeds_shepp" / "circle_back"), side (map_utils NEAR_SIDE 1 / FAR_SIDE 2), start, end (the
    base poses x, y, yaw), start_x, end_x (the candidate lists), wheel_base, max_steer, radius, step, body (car_poly
    ring), aux (0-2 implement rings), blockers (obs_poly_list rings), field (the field ring).  Turns that share the
    very same polygon arrays (`is`) share their pool entries.  cap_s / cap_e / cap_cand default to the largest list
    and product of the batch; max_groups = 0 lets the library choose the candidate kernel's workgroup count."""

    def __init__(self, turns, cap_s=None, cap_e=None, cap_cand=None, cap_samples=1024, max_groups=0):
        B = len(turns)
        self.batch, self.cap_samples, self.max_groups = B, int(cap_samples), int(max_groups)
        sx = [np.asarray(t["start_x"], dtype=np.float64).reshape(-1) for t in turns]
        ex = [np.asarray(t["end_x"], dtype=np.float64).reshape(-1) for t in turns]
        self.cap_s = int(cap_s) if cap_s is not None else max([len(v) for v in sx] + [1])
        self.cap_e = int(cap_e) if cap_e is not None else max([len(v) for v in ex] + [1])
        self.cap_cand = int(cap_cand) if cap_cand is not None else max([len(a) * len(b) for a, b in zip(sx, ex)] + [1])
        self.params = np.zeros((B, CT_NPARAM))
        self.desc = np.full((B, SMP_NDESC), -1, np.int32)
        self.start_x = np.zeros((B, self.cap_s))
        self.end_x = np.zeros((B, self.cap_e))
        self.n_start = np.array([len(v) for v in sx], np.int32).reshape(B)
        self.n_end = np.array([len(v) for v in ex], np.int32).reshape(B)
        polys, seen = [], {}

        def add(q):
            if id(q) in seen:
                return seen[id(q)]
            polys.append(np.asarray(q, dtype=np.float64).reshape(-1, 2))
            seen[id(q)] = len(polys) - 1
            return len(polys) - 1
        self._keep = []   # the rings `seen` knows by id stay alive while packing
        for b, t in enumerate(turns):
            self.params[b] = [SMP_TYPES[t["type"]], t.get("side", 1), *np.asarray(t["start"], dtype=np.float64)[:3],
                              *np.asarray(t["end"], dtype=np.float64)[:3], t["wheel_base"], t["max_steer"],
                              t["radius"], t.get("step", 0.1)]
            self.start_x[b, :min(len(sx[b]), self.cap_s)] = sx[b][:self.cap_s]
            self.end_x[b, :min(len(ex[b]), self.cap_e)] = ex[b][:self.cap_e]
            aux = list(t.get("aux", []))
            if len(aux) > 2:
                raise ValueError("[htp] sample: at most two implements")
            self._keep += [t["body"], t["field"]] + aux
            self.desc[b, 0] = add(t["body"])
            for a, q in enumerate(aux):
                self.desc[b, 1 + a] = add(q)
            blk = t.get("blockers", [])
            key = id(blk)
            if key in seen:
                self.desc[b, 3], self.desc[b, 4] = seen[key]
            else:
                b0 = len(polys)
                polys += [np.asarray(q, dtype=np.float64).reshape(-1, 2) for q in blk]
                seen[key] = (b0, len(polys))
                self._keep.append(blk)
                self.desc[b, 3], self.desc[b, 4] = b0, len(polys)
            self.desc[b, 5] = add(t["field"])
        self.poly_off = np.concatenate([[0], np.cumsum([len(q) for q in polys])]).astype(np.int32)
        self.vertices = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros((0, 2)))

    def struct(self, ptrs=None):
        p = ptrs or {}

        def g(name):
            return p.get(name, getattr(self, name).ctypes.data)
        return SmpIn(self.batch, len(self.poly_off) - 1, self.vertices.shape[0], g("params"), g("desc"), g("poly_off"),
                     g("vertices"), g("start_x"), g("end_x"), g("n_start"), g("n_end"), self.cap_s, self.cap_e,
                     self.cap_cand, self.cap_samples, self.max_groups)


class SampleResults:
    """status [B] (SMP_*), winner [B, 2], poses [B, 8] (safe start, safe end, leave_offset, enter_offset), score [B],
    n_feasible [B]; with tables=True cand_score / cand_status [B, cap_cand] (-inf / SMP_C_*)."""

    def __init__(self, packed, tables=True):
        B = packed.batch
        self.status = np.zeros(B, np.int32)
        self.winner = np.zeros((B, 2), np.int32)
        self.poses = np.zeros((B, SMP_NPOSE))
        self.score = np.zeros(B)
        self.n_feasible = np.zeros(B, np.int32)
        self.cand_score = np.zeros((B, packed.cap_cand)) if tables else None
        self.cand_status = np.zeros((B, packed.cap_cand), np.int32) if tables else None

    def struct(self, ptrs=None):
        p = ptrs or {}

        def g(name):
            a = getattr(self, name)
            return p.get(name, None if a is None else a.ctypes.data)
        return SmpResult(g("status"), g("winner"), g("poses"), g("score"), g("n_feasible"), g("cand_score"),
                         g("cand_status"))


# ------------------------------------------------------------ speed profile of planner paths (htp_speed.hip)
SPD_NLIM, SPD_NNODE, SPD_NKIND, SPD_NSUM = 10, 7, 7, 16
SPD_OK, SPD_SKIPPED, SPD_BAD_INPUT = 0, 1, 2
SPD_STATUS = {0: "ok", 1: "skipped", 2: "bad_input"}
SPD_LIMITS = ("wheel_base", "v_fwd", "v_rev", "acc", "dec", "a_lat", "steer_rate", "max_steer", "v0", "v1")
SPD_NODE_COLUMNS = ("S", "t", "v", "accel", "steer", "steer_rate", "cap")
SPD_KINDS = ("stop", "vmax", "alat", "steer_rate", "endpoint", "acc", "dec")
SPD_SUMMARY = ("T", "length", "len_fwd", "len_rev", "stops", "dwell", "peak_v", "peak_lat", "max_steer") + tuple(
    "time_" + k for k in SPD_KINDS)
SPD_FLAGS = {"HOP": 1, "STEER_EXCEEDS": 2, "TRUNCATED": 4, "BAD_TIME": 8}


class SpdIn(ctypes.Structure):  # htp_speed_in
    _fields_ = [("batch", ctypes.c_int32), ("cap_path", ctypes.c_int32), ("path", ctypes.c_void_p),
                ("n_path", ctypes.c_void_p), ("path_status", ctypes.c_void_p), ("limits", ctypes.c_void_p),
                ("dt", ctypes.c_double), ("cap_rows", ctypes.c_int32), ("max_groups", ctypes.c_int32)]


class SpdResult(ctypes.Structure):  # htp_speed_result
    _fields_ = [("status", ctypes.c_void_p), ("flags", ctypes.c_void_p), ("summary", ctypes.c_void_p),
                ("node", ctypes.c_void_p), ("active", ctypes.c_void_p), ("count", ctypes.c_void_p),
                ("rows", ctypes.c_void_p), ("stage", ctypes.c_void_p)]


class SpeedPacked:
    """Paths for htp_speed_profile_batch.  paths: a list of [n][5] arrays (x, y, yaw, k, dir), or a ClassicResults whose
    path / n_path / status are taken as they are; limits: one row of SPD_LIMITS per path (or one for all);
    status: optional per-path planner status (non-zero: skipped); dt = 0: no fixed-period rows; cap_rows defaults to
    4096 when dt > 0; max_groups = 0 lets the library choose the workgroup count."""

    def __init__(self, paths, limits, cap_path=None, dt=0.0, cap_rows=None, status=None, max_groups=0):
        if isinstance(paths, ClassicResults):
            self.path, self.n_path = paths.path, paths.n_path
            status = paths.status if status is None else status
        else:
            arrs = [np.asarray(p, dtype=np.float64).reshape(-1, 5) for p in paths]
            cap = int(cap_path) if cap_path is not None else max([len(a) for a in arrs] + [2])
            self.path = np.zeros((len(arrs), cap, 5))
            self.n_path = np.array([len(a) for a in arrs], np.int32).reshape(len(arrs))
            for b, a in enumerate(arrs):
                self.path[b, :min(len(a), cap)] = a[:cap]
        self.batch, self.cap_path = self.path.shape[0], self.path.shape[1]
        lim = np.asarray(limits, dtype=np.float64)
        self.limits = np.ascontiguousarray(np.broadcast_to(lim.reshape(-1, SPD_NLIM), (self.batch, SPD_NLIM)))
        self.path_status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(self.batch)
        self.dt, self.max_groups = float(dt), int(max_groups)
        self.cap_rows = int(cap_rows) if cap_rows is not None else (4096 if self.dt > 0.0 else 0)

    @classmethod
    def resident(cls, batch, cap_path, limits, dt=0.0, cap_rows=None, max_groups=0):
        """The description of `batch` paths of `cap_path` rows that live on the device already (say, the buffers
        htp_classic_turn_batch_device filled): sizes, options and the host copy of the limits, no path arrays.  For
        Context.speed_profile_device only, which takes path / n_path / limits (and path_status) as device pointers."""
        self = cls.__new__(cls)
        self.batch, self.cap_path = int(batch), int(cap_path)
        self.path = self.n_path = self.path_status = None
        lim = np.asarray(limits, dtype=np.float64)
        self.limits = np.ascontiguousarray(np.broadcast_to(lim.reshape(-1, SPD_NLIM), (self.batch, SPD_NLIM)))
        self.dt, self.max_groups = float(dt), int(max_groups)
        self.cap_rows = int(cap_rows) if cap_rows is not None else (4096 if self.dt > 0.0 else 0)
        return self

    def struct(self, ptrs=None):
        p = ptrs or {}

        def g(name):
            a = getattr(self, name)
            return p.get(name, None if a is None else a.ctypes.data)
        return SpdIn(self.batch, self.cap_path, g("path"), g("n_path"), g("path_status"), g("limits"), self.dt,
                     self.cap_rows, self.max_groups)


class SpeedResults:
    """status [B] (SPD_*), flags [B] (SPD_FLAGS bits), summary [B, 16] (SPD_SUMMARY), count [B]; with nodes=True node
    [B, cap_path, 7] (SPD_NODE_COLUMNS) and active [B, cap_path] (index into SPD_KINDS); with dt > 0 rows
    [B, cap_rows, 10] (TIMELINE_COLUMNS) and stage.  `fill` pre-fills the doubles (ints: -77), so what the kernel leaves
    unwritten can be told."""

    def __init__(self, packed, nodes=True, stage=True, fill=0.0):
        B, cap, capr = packed.batch, packed.cap_path, packed.cap_rows
        ifill = 0 if fill == 0.0 else -77
        self.cap_rows = capr
        self.status = np.full(B, ifill, np.int32)
        self.flags = np.full(B, ifill, np.int32)
        self.summary = np.full((B, SPD_NSUM), fill)
        self.count = np.full(B, ifill, np.int32)
        self.node = np.full((B, cap, SPD_NNODE), fill) if nodes else None
        self.active = np.full((B, cap), ifill, np.int32) if nodes else None
        self.rows = np.full((B, capr, len(TIMELINE_COLUMNS)), fill) if packed.dt > 0.0 else None
        self.stage = np.full((B, capr), ifill, np.int32) if packed.dt > 0.0 and stage else None

    def struct(self, ptrs=None):
        p = ptrs or {}

        def g(name):
            a = getattr(self, name)
            return p.get(name, None if a is None else a.ctypes.data)
        return SpdResult(g("status"), g("flags"), g("summary"), g("node"), g("active"), g("count"), g("rows"),
                         g("stage"))

    def flag_names(self, k):
        return [n for n, bit in SPD_FLAGS.items() if int(self.flags[k]) & bit]

    def timeline(self, k):
        """The written fixed-period rows of path k."""
        return self.rows[k, :min(int(self.count[k]), self.cap_rows)].copy()

    def as_dict(self, k):
        d = {"status": SPD_STATUS[int(self.status[k])], "flags": self.flag_names(k), "count": int(self.count[k])}
        d.update({n: float(self.summary[k, j]) for j, n in enumerate(SPD_SUMMARY)})
        return d


# ------------------------------------------------------------ pose clearance and turn selection (htp_clear.hip)
CLR_NMETRIC, CLR_MAX_SUBSTEPS, SEL_MAX_CAND = 4, 16, 8
CLR_OK, CLR_SKIPPED, CLR_BAD_INPUT, CLR_BAD_POLYTOPE = 0, 1, 2, 3
CLR_STATUS = {0: "ok", 1: "skipped", 2: "bad_input", 3: "bad_polytope"}
CLR_FLAGS = {"COLLISION": 1, "MARGIN": 2, "TRUNCATED": 4}
CLR_METRICS = ("clearance", "clearance_node", "max_gap", "max_turn")
SEL_VERDICT = {"NOT_PLANNED": 1, "BAD": 2, "SPEED_FLAG": 4, "CLEAR_FLAG": 8, "TOO_LONG": 16, "NONFINITE": 32}
CLR_PATH_LAYOUT = dict(stride=5, cols=(0, 1, 2))        # planner paths x, y, yaw, k, dir
CLR_TIMELINE_LAYOUT = dict(stride=10, cols=(1, 2, 4))   # fixed-period rows t, x, y, v, theta, ...
CLR_SCENE_ARRAYS = ("obs_A", "obs_b", "body_G", "body_g")


class ClrIn(ctypes.Structure):  # htp_clear_in
    _fields_ = [("batch", ctypes.c_int32), ("cap_poses", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("col_x", ctypes.c_int32), ("col_y", ctypes.c_int32), ("col_yaw", ctypes.c_int32),
                ("poses", ctypes.c_void_p), ("n_poses", ctypes.c_void_p), ("pose_status", ctypes.c_void_p),
                ("scene", ctypes.c_void_p), ("n_scenes", ctypes.c_int32), ("M", ctypes.c_int32), ("K", ctypes.c_int32),
                ("obs_edges", ctypes.c_void_p), ("body_edges", ctypes.c_void_p), ("obs_A", ctypes.c_void_p),
                ("obs_b", ctypes.c_void_p), ("body_G", ctypes.c_void_p), ("body_g", ctypes.c_void_p),
                ("margin", ctypes.c_void_p), ("substeps", ctypes.c_int32), ("margin_tol", ctypes.c_double),
                ("max_groups", ctypes.c_int32)]


class ClrResult(ctypes.Structure):  # htp_clear_result
    _fields_ = [("status", ctypes.c_void_p), ("flags", ctypes.c_void_p), ("metrics", ctypes.c_void_p),
                ("worst", ctypes.c_void_p), ("pose_clearance", ctypes.c_void_p)]


class SelIn(ctypes.Structure):  # htp_select_in
    _fields_ = [("batch", ctypes.c_int32), ("C", ctypes.c_int32), ("spd_status", ctypes.c_void_p),
                ("spd_flags", ctypes.c_void_p), ("spd_summary", ctypes.c_void_p), ("rows", ctypes.c_void_p),
                ("count", ctypes.c_void_p), ("cap_rows", ctypes.c_int32), ("clr_status", ctypes.c_void_p),
                ("clr_flags", ctypes.c_void_p), ("clr_metrics", ctypes.c_void_p),
                ("reject_speed_flags", ctypes.c_int32), ("reject_clear_flags", ctypes.c_int32),
                ("t_max", ctypes.c_double)]


class SelResult(ctypes.Structure):  # htp_select_result
    _fields_ = [("verdict", ctypes.c_void_p), ("winner", ctypes.c_void_p), ("score", ctypes.c_void_p),
                ("clearance", ctypes.c_void_p), ("out_rows", ctypes.c_void_p), ("out_count", ctypes.c_void_p)]


def clear_scenes(scenes):
    """A scenes dict for ClearPacked from a list of (obstacles, bodies), each a list of halfspace pairs (A [e, 2],
    b [e]); every scene has the same edge counts."""
    obs0, bod0 = scenes[0]
    out = dict(obs_edges=np.array([len(b) for _, b in obs0], np.int32),
               body_edges=np.array([len(b) for _, b in bod0], np.int32))
    for name, which, part in (("obs_A", 0, 0), ("obs_b", 0, 1), ("body_G", 1, 0), ("body_g", 1, 1)):
        out[name] = np.ascontiguousarray(np.stack(
            [np.concatenate([np.asarray(h[part], dtype=np.float64) for h in sc[which]], axis=0) for sc in scenes]))
    return out


class ClearPacked:
    """Pose sequences and scenes for htp_pose_clearance_batch.  poses: a list of [n][stride] arrays, or one
    [B, cap, stride] array with n_poses; stride / cols: the layout (CLR_PATH_LAYOUT, CLR_TIMELINE_LAYOUT); scenes: a
    PackedBatch or a dict with obs_edges, body_edges, obs_A [n_scenes, TEo, 2], obs_b, body_G, body_g (clear_scenes);
    scene: per-path scene index (None: path p uses scene p); margin: None, a number or one per scene; status:
    optional per-path status (non-zero: skipped)."""

    def __init__(self, poses, scenes, scene=None, stride=5, cols=(0, 1, 2), n_poses=None, cap_poses=None, status=None,
                 substeps=1, margin=None, margin_tol=0.0, max_groups=0):
        self.stride, self.cols = int(stride), tuple(int(c) for c in cols)
        if isinstance(poses, np.ndarray) and poses.ndim == 3:
            self.poses = np.ascontiguousarray(poses, dtype=np.float64)
            self.n_poses = np.ascontiguousarray(n_poses, dtype=np.int32).reshape(self.poses.shape[0])
        else:
            arrs = [np.asarray(p, dtype=np.float64).reshape(-1, self.stride) for p in poses]
            cap = int(cap_poses) if cap_poses is not None else max([len(a) for a in arrs] + [1])
            self.poses = np.zeros((len(arrs), cap, self.stride))
            self.n_poses = np.array([len(a) for a in arrs], np.int32).reshape(len(arrs))
            for b, a in enumerate(arrs):
                self.poses[b, :min(len(a), cap)] = a[:cap]
        self.batch, self.cap_poses = self.poses.shape[0], self.poses.shape[1]
        self.pose_status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(self.batch)
        self._options(scenes, scene, substeps, margin, margin_tol, max_groups)

    def _options(self, scenes, scene, substeps, margin, margin_tol, max_groups):
        get = scenes.get if isinstance(scenes, dict) else (lambda k: getattr(scenes, k))
        self.obs_edges = np.ascontiguousarray(get("obs_edges"), dtype=np.int32)
        self.body_edges = np.ascontiguousarray(get("body_edges"), dtype=np.int32)
        for k in CLR_SCENE_ARRAYS:
            setattr(self, k, None if get(k) is None else np.ascontiguousarray(get(k), dtype=np.float64))
        self.M, self.K = len(self.obs_edges), len(self.body_edges)
        if self.obs_b is not None:
            self.n_scenes = int(self.obs_b.shape[0])
        else:
            self.n_scenes = int(get("n_scenes"))
        self.scene = None if scene is None else np.ascontiguousarray(scene, dtype=np.int32).reshape(self.batch)
        self.margin = None if margin is None else np.broadcast_to(
            np.asarray(margin, dtype=np.float64).reshape(-1), (self.n_scenes,)).copy()
        self.substeps, self.margin_tol, self.max_groups = int(substeps), float(margin_tol), int(max_groups)

    @classmethod
    def resident(cls, batch, cap_poses, edges, n_scenes, stride=5, cols=(0, 1, 2), substeps=1,
                 margin_tol=0.0, max_groups=0):
        """The description of `batch` sequences of `cap_poses` rows and `n_scenes` scenes that live on the device
        already: sizes, layout and options, no arrays.  edges: (obs_edges, body_edges).  For
        Context.pose_clearance_device only, which takes poses / n_poses / the scene arrays (and pose_status, scene,
        margin) as device pointers."""
        self = cls.__new__(cls)
        self.batch, self.cap_poses = int(batch), int(cap_poses)
        self.stride, self.cols = int(stride), tuple(int(c) for c in cols)
        self.poses = self.n_poses = self.pose_status = None
        self._options(dict(obs_edges=edges[0], body_edges=edges[1], obs_A=None, obs_b=None, body_G=None, body_g=None,
                           n_scenes=n_scenes), None, substeps, None, margin_tol, max_groups)
        return self

    def struct(self, ptrs=None):
        p = ptrs or {}

        def g(name):
            a = getattr(self, name)
            return p.get(name, None if a is None else a.ctypes.data)
        return ClrIn(self.batch, self.cap_poses, self.stride, self.cols[0], self.cols[1], self.cols[2], g("poses"),
                     g("n_poses"), g("pose_status"), g("scene"), self.n_scenes, self.M, self.K,
                     self.obs_edges.ctypes.data, self.body_edges.ctypes.data, g("obs_A"), g("obs_b"), g("body_G"),
                     g("body_g"), g("margin"), self.substeps, self.margin_tol, self.max_groups)


class ClearResults:
    """status [B] (CLR_*), flags [B] (CLR_FLAGS bits), metrics [B, 4] (CLR_METRICS), worst [B, 4] (pose, substep,
    obstacle, body); with poses=True pose_clearance [B, cap_poses].  `fill` pre-fills the doubles (ints: -77), so what
    the kernel leaves unwritten can be told."""

    def __init__(self, packed, poses=True, fill=0.0):
        B = packed.batch
        ifill = 0 if fill == 0.0 else -77
        self.status = np.full(B, ifill, np.int32)
        self.flags = np.full(B, ifill, np.int32)
        self.metrics = np.full((B, CLR_NMETRIC), fill)
        self.worst = np.full((B, 4), ifill, np.int32)
        self.pose_clearance = np.full((B, packed.cap_poses), fill) if poses else None

    def struct(self, ptrs=None):
        p = ptrs or {}

        def g(name):
            a = getattr(self, name)
            return p.get(name, None if a is None else a.ctypes.data)
        return ClrResult(g("status"), g("flags"), g("metrics"), g("worst"), g("pose_clearance"))

    def metric(self, name):
        return self.metrics[:, CLR_METRICS.index(name)]

    def flag_names(self, k):
        return [n for n, bit in CLR_FLAGS.items() if int(self.flags[k]) & bit]

    def as_dict(self, k):
        d = {"status": CLR_STATUS[int(self.status[k])], "flags": self.flag_names(k),
             "worst": dict(zip(("pose", "substep", "obstacle", "body"), (int(v) for v in self.worst[k])))}
        d.update({n: float(self.metrics[k, j]) for j, n in enumerate(CLR_METRICS)})
        return d


def select_flag_mask(names, table):
    """A mask of `table` (SPD_FLAGS / CLR_FLAGS) bits from flag names, or the int itself."""
    if isinstance(names, (int, np.integer)):
        return int(names)
    return int(sum(table[n] for n in names))


class SelectResults:
    """verdict [B, C] (SEL_VERDICT bits; 0: admissible), winner [B] (-1: none), score [B] (the winner's T or NaN),
    clearance [B]; with cap_rows > 0 out_rows [B, cap_rows, 10] and out_count [B]."""

    def __init__(self, batch, C, cap_rows=0, clearance=True, fill=0.0):
        ifill = 0 if fill == 0.0 else -77
        self.batch, self.C, self.cap_rows = int(batch), int(C), int(cap_rows)
        self.verdict = np.full((self.batch, self.C), ifill, np.int32)
        self.winner = np.full(self.batch, ifill, np.int32)
        self.score = np.full(self.batch, fill)
        self.clearance = np.full(self.batch, fill) if clearance else None
        self.out_rows = np.full((self.batch, self.cap_rows, len(TIMELINE_COLUMNS)), fill) if cap_rows else None
        self.out_count = np.full(self.batch, ifill, np.int32) if cap_rows else None

    def struct(self, ptrs=None):
        p = ptrs or {}

        def g(name):
            a = getattr(self, name)
            return p.get(name, None if a is None else a.ctypes.data)
        return SelResult(g("verdict"), g("winner"), g("score"), g("clearance"), g("out_rows"), g("out_count"))

    def flag_names(self, b, c):
        return [n for n, bit in SEL_VERDICT.items() if int(self.verdict[b, c]) & bit]

    def rows(self, b):
        """The copied rows of problem b's winner."""
        return self.out_rows[b, :min(int(self.out_count[b]), self.cap_rows)].copy()


def select_in(batch, C, ptr, cap_rows=0, reject_speed_flags=0, reject_clear_flags=0, t_max=0.0):
    """htp_select_in over the pointers `ptr` (name -> address; rows / count / clr_metrics optional)."""
    return SelIn(int(batch), int(C), ptr["spd_status"], ptr["spd_flags"], ptr["spd_summary"], ptr.get("rows"),
                 ptr.get("count"), int(cap_rows) if ptr.get("rows") else 0, ptr["clr_status"], ptr["clr_flags"],
                 ptr.get("clr_metrics"), select_flag_mask(reject_speed_flags, SPD_FLAGS),
                 select_flag_mask(reject_clear_flags, CLR_FLAGS), float(t_max))


class ChainBatch(ctypes.Structure):  # htp_chain_batch
    _fields_ = [("batch", ctypes.c_int32), ("N", ctypes.c_int32), ("M", ctypes.c_int32),
                ("scenes", OgeBatch), ("turns", CtBatch), ("margin", ctypes.c_void_p),
                ("n_vpoly", ctypes.c_int32), ("vpoly_nv", ctypes.c_int32 * 2), ("vpoly", ctypes.c_double * 32),
                ("dT", ctypes.c_double), ("wheel_base", ctypes.c_double), ("cap_rows", ctypes.c_int32),
                ("traj", ctypes.c_void_p), ("obs_A", ctypes.c_void_p), ("obs_b", ctypes.c_void_p),
                ("status", ctypes.c_void_p)]


class WorkQueue:
    """Host work queue of problem indices feeding one persistent solve launch
    (htp_queue_*: pinned, GPU-coherent host memory)."""

    def __init__(self, ctx, capacity):
        self.lib = ctx.lib
        self.q = self.lib.htp_queue_create(ctx.ctx, int(capacity))
        if not self.q:
            raise RuntimeError(f"[htp] htp_queue_create failed: {ctx.error()}")

    def publish(self, pids):
        a = np.ascontiguousarray(np.asarray(pids, dtype=np.int32))
        if self.lib.htp_queue_publish(self.q, a.ctypes.data, a.size) != 0:
            raise RuntimeError("[htp] htp_queue_publish failed (full, closed or index out of range)")

    def close(self):
        self.lib.htp_queue_close(self.q)

    def published(self):
        return int(self.lib.htp_queue_published(self.q))

    def claimed(self):
        return int(self.lib.htp_queue_claimed(self.q))

    def destroy(self):
        if self.q:
            self.lib.htp_queue_destroy(self.q)
            self.q = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Context:
    """Owns one htp_ctx (device workspace)."""

    def __init__(self, device=0, options=None, lib=None):
        self.lib = lib or load()
        self.device = int(device)
        self.ctx = self.lib.htp_create(int(device))
        if not self.ctx:
            raise RuntimeError("[htp] htp_create failed")
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        if self.lib.htp_set_option(self.ctx, name.encode(), float(value)) != 0:
            raise ValueError(f"[htp] unknown option {name}")

    def error(self):
        return self.lib.htp_last_error(self.ctx).decode()

    def solve(self, packed):
        res = HostResults(packed.batch, packed.n_var)
        b, r = packed.struct(), res.struct()
        rc = self.lib.htp_obca_solve_batch(self.ctx, ctypes.byref(b), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_solve_batch failed: {self.error()}")
        return res

    def libm(self, name, x, y=None):
        """The device build of the planner libm over host arrays (through device buffers) -> float64 array."""
        import torch
        dev = torch.device("cuda", self.device)
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
        yt = None
        if y is not None:
            yt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(y, np.shape(x)), dtype=np.float64)).to(dev)
        out = torch.empty_like(xt)
        s = torch.cuda.current_stream(dev)
        rc = self.lib.htp_libm_batch_device(self.ctx, LIBM_FN[name], xt.data_ptr(),
                                            yt.data_ptr() if yt is not None else None, out.data_ptr(), xt.numel(),
                                            ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_libm_batch_device failed: {self.error()}")
        s.synchronize()
        return out.cpu().numpy()

    def mfma_f64(self, A, B, C):
        """htp_mfma_f64_probe over host tiles A [n,16,4], B [n,4,16], C [n,16,16] -> D [n,16,16]."""
        import torch
        dev = torch.device("cuda", self.device)
        t = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev) for v in (A, B, C)]
        n = t[0].shape[0]
        if t[0].shape != (n, 16, 4) or t[1].shape != (n, 4, 16) or t[2].shape != (n, 16, 16):
            raise ValueError("[htp] mfma_f64: tiles must be [n,16,4], [n,4,16], [n,16,16]")
        out = torch.empty_like(t[2])
        s = torch.cuda.current_stream(dev)
        rc = self.lib.htp_mfma_f64_probe(self.ctx, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr(),
                                         n, ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_mfma_f64_probe failed: {self.error()}")
        s.synchronize()
        return out.cpu().numpy()

    def bk_probe(self, variant, n, K0, rhs, lane_stride=1, extra_rows=0):
        """htp_bk_probe over host blocks K0 [count, *] and right-hand sides rhs [count, nrhs, n] -> dict of host
        arrays K, ip, flags, x, x2.  The outputs are pre-filled with a sentinel and have `extra_rows` rows past
        `count`, which the kernel's inactive lanes must leave untouched."""
        import torch
        if not hasattr(self.lib, "htp_bk_probe"):
            raise RuntimeError("[htp] this libhtp.so has no htp_bk_probe")
        dev = torch.device("cuda", self.device)
        vi, _ = bk_probe_sizes(variant, n)
        K0 = np.array(K0, dtype=np.float64, order="C")   # copies: torch wants writable arrays
        rhs = np.array(rhs, dtype=np.float64, order="C")
        count, nrhs = K0.shape[0], rhs.shape[1]
        if K0.shape != (count, vi) or rhs.shape != (count, nrhs, n):
            raise ValueError(f"[htp] bk_probe: K0 must be [count, {vi}] and rhs [count, nrhs, {n}]")
        tin = [torch.from_numpy(v).to(dev) for v in (K0, rhs)]
        tout = [torch.from_numpy(v).to(dev) for v in bk_probe_outputs(variant, n, count + extra_rows, nrhs)]
        s = torch.cuda.current_stream(dev)
        rc = self.lib.htp_bk_probe(self.ctx, variant, n, lane_stride, count, nrhs, tin[0].data_ptr(),
                                   tin[1].data_ptr(), *[t.data_ptr() for t in tout], ctypes.c_void_p(s.cuda_stream))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_bk_probe failed: {self.error()}")
        s.synchronize()
        return dict(zip(("K", "ip", "flags", "x", "x2"), [t.cpu().numpy() for t in tout]))

    def solve_points(self, packed):
        """Batched optimizer_points.py solve (host buffers)."""
        res = HostResults(packed.batch, packed.n_var)
        b, r = packed.struct(), res.struct()
        rc = self.lib.htp_obca_points_solve_batch(self.ctx, ctypes.byref(b), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_points_solve_batch failed: {self.error()}")
        return res

    def classic_turns(self, packed, out=None):
        """Batched classic headland turns (host buffers) -> ClassicResults.  `out`: a ClassicResults to fill; what the
        kernel leaves unwritten (rows from n_path on, the rows of a rejected turn) stays as it was."""
        r = ClassicResults(packed) if out is None else out
        b, rs = packed.struct(), r.struct()
        if self.lib.htp_classic_turn_batch(self.ctx, ctypes.byref(b), ctypes.byref(rs)) != 0:
            raise RuntimeError(f"[htp] htp_classic_turn_batch failed: {self.error()}")
        return r

    def classic_turns_device(self, packed, dev_ptrs, out_ptrs, stream=None):
        """Device-resident classic turns on `stream`, not synchronised.  dev_ptrs: device pointers of the
        ClassicPacked arrays by name; out_ptrs: those of status, n_path and path.  The polygon ids are trusted."""
        b = packed.struct(dev_ptrs)
        r = CtResult(out_ptrs["status"], out_ptrs["n_path"], out_ptrs["path"])
        if self.lib.htp_classic_turn_batch_device(self.ctx, ctypes.byref(b), ctypes.byref(r), stream) != 0:
            raise RuntimeError(f"[htp] htp_classic_turn_batch_device failed: {self.error()}")

    def classic_last_ms(self):
        return self.lib.htp_classic_last_ms(self.ctx)

    def classic_sample(self, packed, tables=True, **opts):
        """Batched sampled exit / entry pose search (host buffers) -> SampleResults.  opts: max_groups (workgroups of
        the candidate kernel, 0 = the library's choice) and cap_samples override the packed values."""
        for k in opts:
            if k not in ("max_groups", "cap_samples"):
                raise TypeError(f"[htp] classic_sample: unknown option {k!r}")
        rs = SampleResults(packed, tables)
        b, r = packed.struct(), rs.struct()
        b.max_groups = int(opts.get("max_groups", packed.max_groups))
        b.cap_samples = int(opts.get("cap_samples", packed.cap_samples))
        if self.lib.htp_classic_sample_batch(self.ctx, ctypes.byref(b), ctypes.byref(r)) != 0:
            raise RuntimeError(f"[htp] htp_classic_sample_batch failed: {self.error()}")
        return rs

    def classic_sample_device(self, packed, dev_ptrs, out_ptrs, stream=None, **opts):
        """Device-resident search on `stream`, not synchronised.  dev_ptrs: device pointers of the SamplePacked arrays
        by name; out_ptrs: those of the SampleResults arrays (cand_score / cand_status optional, as a pair)."""
        b, r = packed.struct(dev_ptrs), SmpResult()
        b.max_groups = int(opts.get("max_groups", packed.max_groups))
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        if self.lib.htp_classic_sample_batch_device(self.ctx, ctypes.byref(b), ctypes.byref(r), stream) != 0:
            raise RuntimeError(f"[htp] htp_classic_sample_batch_device failed: {self.error()}")

    def classic_sample_last_ms(self):
        return self.lib.htp_classic_sample_last_ms(self.ctx)

    def speed_profile(self, packed, nodes=True, stage=True, out=None):
        """Batched speed profile and timed trajectory of planner paths (host buffers) -> SpeedResults.  `out`: a
        SpeedResults to fill; what the kernel leaves unwritten stays as it was."""
        r = SpeedResults(packed, nodes, stage) if out is None else out
        b, rs = packed.struct(), r.struct()
        if self.lib.htp_speed_profile_batch(self.ctx, ctypes.byref(b), ctypes.byref(rs)) != 0:
            raise RuntimeError(f"[htp] htp_speed_profile_batch failed: {self.error()}")
        return r

    def speed_profile_device(self, packed, dev_ptrs, out_ptrs, stream=None):
        """Device-resident speed profile on `stream`, not synchronised.  dev_ptrs: device pointers of path, n_path,
        limits and optionally path_status (e.g. the buffers htp_classic_turn_batch_device filled on the same stream);
        out_ptrs: those of the SpeedResults arrays (node, active, rows, stage optional)."""
        for k in ("path", "n_path", "limits"):
            if k not in dev_ptrs:
                raise KeyError(f"[htp] speed_profile_device: the device pointer of {k!r} is missing")
        b, r = packed.struct(dev_ptrs), SpdResult()
        if "path_status" not in dev_ptrs:
            b.path_status = None
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        if self.lib.htp_speed_profile_batch_device(self.ctx, ctypes.byref(b), ctypes.byref(r), stream) != 0:
            raise RuntimeError(f"[htp] htp_speed_profile_batch_device failed: {self.error()}")

    def speed_profile_last_ms(self):
        return self.lib.htp_speed_profile_last_ms(self.ctx)

    def pose_clearance(self, packed, poses=True, out=None):
        """Batched clearance of pose sequences against their scenes (host buffers) -> ClearResults.  `out`: a
        ClearResults to fill; what the kernel leaves unwritten stays as it was."""
        r = ClearResults(packed, poses) if out is None else out
        b, rs = packed.struct(), r.struct()
        if self.lib.htp_pose_clearance_batch(self.ctx, ctypes.byref(b), ctypes.byref(rs)) != 0:
            raise RuntimeError(f"[htp] htp_pose_clearance_batch failed: {self.error()}")
        return r

    def pose_clearance_device(self, packed, dev_ptrs, out_ptrs, stream=None):
        """Device-resident clearance on `stream`, not synchronised.  dev_ptrs: device pointers of poses, n_poses, obs_A,
        obs_b, body_G, body_g and optionally pose_status, scene and margin (e.g. the buffers
        htp_classic_turn_batch_device filled on the same stream); out_ptrs: those of the ClearResults arrays
        (pose_clearance optional)."""
        for k in ("poses", "n_poses") + CLR_SCENE_ARRAYS:
            if k not in dev_ptrs:
                raise KeyError(f"[htp] pose_clearance_device: the device pointer of {k!r} is missing")
        b, r = packed.struct(dev_ptrs), ClrResult()
        for k in ("pose_status", "scene", "margin"):
            if k not in dev_ptrs:
                setattr(b, k, None)
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        if self.lib.htp_pose_clearance_batch_device(self.ctx, ctypes.byref(b), ctypes.byref(r), stream) != 0:
            raise RuntimeError(f"[htp] htp_pose_clearance_batch_device failed: {self.error()}")

    def pose_clearance_last_ms(self):
        return self.lib.htp_pose_clearance_last_ms(self.ctx)

    def turn_select(self, speed, clear, C, reject_speed_flags=0, reject_clear_flags=0, t_max=0.0, rows=True, out=None):
        """The fastest admissible candidate per problem (host buffers) -> SelectResults.  speed: a SpeedResults and
        clear: a ClearResults of C * B paths, candidate c of problem b at index c B + b; reject_*_flags: a mask or a
        list of SPD_FLAGS / CLR_FLAGS names; rows: copy the winner's fixed-period rows when `speed` has them."""
        N = len(speed.status)
        if N % int(C) or len(clear.status) != N:
            raise ValueError("[htp] turn_select: speed and clear must hold C * B paths each")
        B = N // int(C)
        with_rows = bool(rows) and speed.rows is not None
        r = SelectResults(B, C, speed.cap_rows if with_rows else 0) if out is None else out
        ptr = {"spd_status": speed.status.ctypes.data, "spd_flags": speed.flags.ctypes.data,
               "spd_summary": speed.summary.ctypes.data, "clr_status": clear.status.ctypes.data,
               "clr_flags": clear.flags.ctypes.data, "clr_metrics": clear.metrics.ctypes.data}
        if with_rows:
            ptr.update(rows=speed.rows.ctypes.data, count=speed.count.ctypes.data)
        b, rs = select_in(B, C, ptr, speed.cap_rows, reject_speed_flags, reject_clear_flags, t_max), r.struct()
        if self.lib.htp_turn_select_batch(self.ctx, ctypes.byref(b), ctypes.byref(rs)) != 0:
            raise RuntimeError(f"[htp] htp_turn_select_batch failed: {self.error()}")
        return r

    def turn_select_device(self, batch, C, dev_ptrs, out_ptrs, cap_rows=0, reject_speed_flags=0, reject_clear_flags=0,
                           t_max=0.0, stream=None):
        """Device-resident selection on `stream`, not synchronised.  dev_ptrs: device pointers of spd_status, spd_flags,
        spd_summary, clr_status, clr_flags and optionally clr_metrics, rows and count (with cap_rows); out_ptrs: those
        of the SelectResults arrays."""
        b, r = select_in(batch, C, dev_ptrs, cap_rows, reject_speed_flags, reject_clear_flags, t_max), SelResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        if self.lib.htp_turn_select_batch_device(self.ctx, ctypes.byref(b), ctypes.byref(r), stream) != 0:
            raise RuntimeError(f"[htp] htp_turn_select_batch_device failed: {self.error()}")

    def turn_select_last_ms(self):
        return self.lib.htp_turn_select_last_ms(self.ctx)

    def oge_obstacles(self, packed, halfspaces=True):
        """Batched orchard scene -> OBCA obstacle polygons (+ halfspaces), host buffers -> OgeResults."""
        r = OgeResults(packed.batch, halfspaces)
        b, rs = packed.struct(), r.struct()
        if self.lib.htp_oge_obstacles_batch(self.ctx, ctypes.byref(b), ctypes.byref(rs)) != 0:
            raise RuntimeError(f"[htp] htp_oge_obstacles_batch failed: {self.error()}")
        return r

    def oge_last_ms(self):
        return self.lib.htp_oge_last_ms(self.ctx)

    def init_ref_path(self, packed):
        """Batched get_init_ref_path (host buffers) -> RefPathResults."""
        res = RefPathResults(packed)
        b, r = packed.struct(), res.struct()
        if self.lib.htp_init_ref_path_batch(self.ctx, ctypes.byref(b), ctypes.byref(r)) != 0:
            raise RuntimeError(f"[htp] htp_init_ref_path_batch failed: {self.error()}")
        return res

    def init_ref_path_last_ms(self):
        return self.lib.htp_init_ref_path_last_ms(self.ctx)

    def solve_device(self, packed, dev_ptrs, out_ptrs, stream=None, lo=None, hi=None):
        """Device-resident solve of `packed` (or of its problems [lo, hi)) on `stream`."""
        b = packed.struct(dev_ptrs) if lo is None else packed.chunk_struct(dev_ptrs, lo, hi)
        r = ObcaResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        rc = self.lib.htp_obca_solve_batch_device(self.ctx, ctypes.byref(b), ctypes.byref(r), stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_solve_batch_device failed: {self.error()}")

    def last_kernel_ms(self):
        return self.lib.htp_last_kernel_ms(self.ctx)

    def audit(self, packed, x, substeps=4, margin_tol=1e-4, dyn_tol=1e-4, bound_tol=1e-4, term_tol=0.0, stage=True):
        """Geometric audit of decision vectors x [batch, n_var] of `packed` (host buffers) -> AuditResults."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (packed.batch, packed.n_var):
            raise ValueError(f"[htp] audit: x must be [{packed.batch}, {packed.n_var}], got {x.shape}")
        res = AuditResults(packed.batch, packed.N, stage)
        b, r = packed.struct(), res.struct()
        o = audit_opts(substeps, margin_tol, dyn_tol, bound_tol, term_tol)
        rc = self.lib.htp_obca_audit_batch(self.ctx, ctypes.byref(b), x.ctypes.data, ctypes.byref(o), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_audit_batch failed: {self.error()}")
        return res

    def audit_device(self, packed, dev_ptrs, x_ptr, out_ptrs, stream=None, lo=None, hi=None, **opts):
        """Device-resident audit of `packed` (or of its problems [lo, hi)) on `stream`, not synchronised.  x_ptr:
        device pointer of the [batch, n_var] rows (e.g. a solve's out x); out_ptrs: device pointers metrics, worst,
        flags and optionally stage_clearance (torch tensors' data_ptr())."""
        b = packed.struct(dev_ptrs) if lo is None else packed.chunk_struct(dev_ptrs, lo, hi)
        r = AuditResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        o = audit_opts(**opts)
        rc = self.lib.htp_obca_audit_batch_device(self.ctx, ctypes.byref(b), x_ptr, ctypes.byref(o), ctypes.byref(r),
                                                  stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_audit_batch_device failed: {self.error()}")

    def audit_last_ms(self):
        return self.lib.htp_obca_audit_last_ms(self.ctx)

    def timeline(self, packed, x, dt, cap=None, stage=True):
        """Uniform-time sampling of decision vectors x [batch, n_var] of `packed` at period dt (host buffers) ->
        TimelineResults.  cap: rows of storage per problem; None derives it from x (timeline_cap), so that no
        problem is truncated."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (packed.batch, packed.n_var):
            raise ValueError(f"[htp] timeline: x must be [{packed.batch}, {packed.n_var}], got {x.shape}")
        if cap is None:
            if not (np.isfinite(dt) and dt > 0):
                raise ValueError(f"[htp] timeline: dt must be finite and > 0, got {dt}")
            cap = timeline_cap(packed, x, dt)
        res = TimelineResults(packed.batch, cap, stage)
        b, r = packed.struct(), res.struct()
        o = timeline_opts(dt, cap)
        rc = self.lib.htp_obca_timeline_batch(self.ctx, ctypes.byref(b), x.ctypes.data, ctypes.byref(o),
                                              ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_timeline_batch failed: {self.error()}")
        return res

    def timeline_device(self, packed, dev_ptrs, x_ptr, out_ptrs, dt, cap, stream=None, lo=None, hi=None):
        """Device-resident timeline of `packed` (or of its problems [lo, hi)) on `stream`, not synchronised.
        x_ptr: device pointer of the [batch, n_var] rows (e.g. a solve's out x); out_ptrs: device pointers rows
        [batch, cap, 10], count, flags and optionally stage [batch, cap] and duration (torch tensors' data_ptr())."""
        b = packed.struct(dev_ptrs) if lo is None else packed.chunk_struct(dev_ptrs, lo, hi)
        r = TimelineResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        o = timeline_opts(dt, cap)
        rc = self.lib.htp_obca_timeline_batch_device(self.ctx, ctypes.byref(b), x_ptr, ctypes.byref(o),
                                                     ctypes.byref(r), stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_timeline_batch_device failed: {self.error()}")

    def timeline_last_ms(self):
        return self.lib.htp_obca_timeline_last_ms(self.ctx)

    def envelope(self, packed, x, frames=None, res=0.1, W=None, H=None, substeps=4, bitmap=True):
        """Swept-footprint envelope of decision vectors x [batch, n_var] of `packed` (host buffers) ->
        EnvelopeResults.  frames [batch, 3] = (ox, oy, phi) with the grid W x H of side res; frames=None takes the
        default frame and grid (envelope_default_frame); W = H = 0 asks for the extent only."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (packed.batch, packed.n_var):
            raise ValueError(f"[htp] envelope: x must be [{packed.batch}, {packed.n_var}], got {x.shape}")
        if frames is None:
            frames, W0, H0 = envelope_default_frame(packed, x, res)
            W, H = (W0, H0) if W is None and H is None else (W, H)
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        if frames.shape != (packed.batch, 3):
            raise ValueError(f"[htp] envelope: frames must be [{packed.batch}, 3], got {frames.shape}")
        if W is None or H is None:
            raise ValueError("[htp] envelope: W and H must be given with frames (0, 0 for the extent only)")
        ok = W > 0 and H > 0 and W % 32 == 0 and W * H <= ENVELOPE_MAX_CELLS   # otherwise the library refuses
        res_ = EnvelopeResults(packed.batch, packed.K, W if ok else 0, H if ok else 0, res, frames, bitmap)
        b, r = packed.struct(), res_.struct()
        o = envelope_opts(substeps, res, W, H)
        rc = self.lib.htp_obca_envelope_batch(self.ctx, ctypes.byref(b), x.ctypes.data, frames.ctypes.data,
                                              ctypes.byref(o), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_envelope_batch failed: {self.error()}")
        return res_

    def envelope_device(self, packed, dev_ptrs, x_ptr, frame_ptr, out_ptrs, res=0.1, W=0, H=0, substeps=4,
                        stream=None, lo=None, hi=None):
        """Device-resident envelope of `packed` (or of its problems [lo, hi)) on `stream`, not synchronised.
        x_ptr: device pointer of the [batch, n_var] rows (e.g. a solve's out x); frame_ptr: device [batch, 3];
        out_ptrs: device pointers extent, where, flags and optionally extent_body, cells (required with a
        raster) and bitmap (torch tensors' data_ptr())."""
        b = packed.struct(dev_ptrs) if lo is None else packed.chunk_struct(dev_ptrs, lo, hi)
        r = EnvelopeResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        o = envelope_opts(substeps, res, W, H)
        rc = self.lib.htp_obca_envelope_batch_device(self.ctx, ctypes.byref(b), x_ptr, frame_ptr, ctypes.byref(o),
                                                     ctypes.byref(r), stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_envelope_batch_device failed: {self.error()}")

    def envelope_last_ms(self):
        return self.lib.htp_obca_envelope_last_ms(self.ctx)

    def track(self, packed, x, scenarios=None, dt=0.1, max_ticks=None, ticks=True, reference=False, R=64, seed=0,
              **opts):
        """Closed-loop tracking rollout of decision vectors x [batch, n_var] of `packed` under every scenario (host
        buffers) -> TrackResults.  scenarios [R, 6] (TRACK_SCENARIO_COLUMNS); None draws track_scenarios(R, seed).
        max_ticks: poses of storage per problem; None derives it from x (track_ticks), so that no problem is
        truncated.  Further keywords: plant_substeps, k_lat, k_yaw, k_lon, abort_dist, margin_tol (track_opts)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (packed.batch, packed.n_var):
            raise ValueError(f"[htp] track: x must be [{packed.batch}, {packed.n_var}], got {x.shape}")
        if scenarios is None:
            scenarios = track_scenarios(R, seed)
        scenarios = np.ascontiguousarray(scenarios, dtype=np.float64)
        if scenarios.ndim != 2 or scenarios.shape[1] != len(TRACK_SCENARIO_COLUMNS):
            raise ValueError(f"[htp] track: scenarios must be [R, 6], got {scenarios.shape}")
        if max_ticks is None:
            if not (np.isfinite(dt) and dt > 0):
                raise ValueError(f"[htp] track: dt must be finite and > 0, got {dt}")
            max_ticks = track_ticks(packed, x, dt)
        res = TrackResults(packed.batch, scenarios.shape[0], max(int(max_ticks), 0), scenarios, ticks, reference)
        b, r = packed.struct(), res.struct()
        o = track_opts(dt, max_ticks, scenarios.ctypes.data, scenarios.shape[0], **opts)
        rc = self.lib.htp_obca_track_batch(self.ctx, ctypes.byref(b), x.ctypes.data, ctypes.byref(o), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_track_batch failed: {self.error()}")
        return res

    def track_device(self, packed, dev_ptrs, x_ptr, scenarios_ptr, R, out_ptrs, dt, max_ticks, stream=None, lo=None,
                     hi=None, **opts):
        """Device-resident tracking rollout of `packed` (or of its problems [lo, hi)) on `stream`, not synchronised.
        x_ptr: device pointer of the [batch, n_var] rows (e.g. a solve's out x); scenarios_ptr: device [R, 6];
        out_ptrs: device pointers metrics [batch, R, 8], worst [batch, R, 3], flags [batch, R], tally [batch, 10],
        worst_scenario [batch] and optionally tick_clearance [batch, max_ticks] and reference [batch, max_ticks, 5]
        (torch tensors' data_ptr())."""
        b = packed.struct(dev_ptrs) if lo is None else packed.chunk_struct(dev_ptrs, lo, hi)
        r = TrackResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        o = track_opts(dt, max_ticks, scenarios_ptr, R, **opts)
        rc = self.lib.htp_obca_track_batch_device(self.ctx, ctypes.byref(b), x_ptr, ctypes.byref(o), ctypes.byref(r),
                                                  stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_track_batch_device failed: {self.error()}")

    def track_last_ms(self):
        return self.lib.htp_obca_track_last_ms(self.ctx)

    def lqr(self, packed, x, cost_to_go=False, linearisation=False, **opts):
        """Time-varying LQR gains and error tube about decision vectors x [batch, n_var] of `packed` (host buffers)
        -> LqrResults.  Keywords: the fields of htp_obca_lqr_opts (LQR_DEFAULTS)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (packed.batch, packed.n_var):
            raise ValueError(f"[htp] lqr: x must be [{packed.batch}, {packed.n_var}], got {x.shape}")
        res = LqrResults(packed.batch, packed.N, cost_to_go, linearisation)
        b, r, o = packed.struct(), res.struct(), lqr_opts(**opts)
        rc = self.lib.htp_obca_lqr_batch(self.ctx, ctypes.byref(b), x.ctypes.data, ctypes.byref(o), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_lqr_batch failed: {self.error()}")
        return res

    def lqr_device(self, packed, dev_ptrs, x_ptr, out_ptrs, stream=None, lo=None, hi=None, **opts):
        """Device-resident LQR pass of `packed` (or of its problems [lo, hi)) on `stream`, not synchronised.  x_ptr:
        device pointer of the [batch, n_var] rows (e.g. a solve's out x); out_ptrs: device pointers gains
        [batch, N-1, 2, 5], tube [batch, N, 7], metrics [batch, 10], worst [batch, 2], flags [batch] and optionally
        cost_to_go [batch, N, 15] and linearisation [batch, N-1, 35] (torch tensors' data_ptr())."""
        b = packed.struct(dev_ptrs) if lo is None else packed.chunk_struct(dev_ptrs, lo, hi)
        r = LqrResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        o = lqr_opts(**opts)
        rc = self.lib.htp_obca_lqr_batch_device(self.ctx, ctypes.byref(b), x_ptr, ctypes.byref(o), ctypes.byref(r),
                                                stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_lqr_batch_device failed: {self.error()}")

    def lqr_last_ms(self):
        return self.lib.htp_obca_lqr_last_ms(self.ctx)

    def ltrack(self, packed, x, gains=None, scenarios=None, dt=0.1, max_ticks=None, ticks=True, reference=False,
               errors=True, R=64, seed=0, plant_substeps=2, abort_dist=2.0, margin_tol=1e-4, **lqr_opts_):
        """Closed-loop rollout of decision vectors x [batch, n_var] of `packed` under their time-varying LQR gains and
        every scenario (host buffers) -> LtrackResults.  gains [batch, N-1, 2, 5] (LqrResults.gains); None runs
        lqr(packed, x, **lqr_opts_) first.  scenarios, dt, max_ticks, ticks, reference, R, seed as track's; errors
        asks for tick_error."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (packed.batch, packed.n_var):
            raise ValueError(f"[htp] ltrack: x must be [{packed.batch}, {packed.n_var}], got {x.shape}")
        if gains is None:
            gains = self.lqr(packed, x, **lqr_opts_).gains
        elif lqr_opts_:
            raise TypeError(f"[htp] ltrack: unknown options {sorted(lqr_opts_)} (LQR options need gains=None)")
        gains = np.ascontiguousarray(gains, dtype=np.float64)
        if gains.shape != (packed.batch, packed.N - 1, 2, 5):
            raise ValueError(f"[htp] ltrack: gains must be [{packed.batch}, {packed.N - 1}, 2, 5], got {gains.shape}")
        if scenarios is None:
            scenarios = track_scenarios(R, seed)
        scenarios = np.ascontiguousarray(scenarios, dtype=np.float64)
        if scenarios.ndim != 2 or scenarios.shape[1] != len(TRACK_SCENARIO_COLUMNS):
            raise ValueError(f"[htp] ltrack: scenarios must be [R, 6], got {scenarios.shape}")
        if max_ticks is None:
            if not (np.isfinite(dt) and dt > 0):
                raise ValueError(f"[htp] ltrack: dt must be finite and > 0, got {dt}")
            max_ticks = track_ticks(packed, x, dt)
        res = LtrackResults(packed.batch, scenarios.shape[0], max(int(max_ticks), 0), scenarios, ticks, reference,
                            errors, gains)
        b, r = packed.struct(), res.struct()
        o = ltrack_opts(dt, max_ticks, scenarios.ctypes.data, scenarios.shape[0], gains.ctypes.data, plant_substeps,
                        abort_dist, margin_tol)
        rc = self.lib.htp_obca_ltrack_batch(self.ctx, ctypes.byref(b), x.ctypes.data, ctypes.byref(o), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_ltrack_batch failed: {self.error()}")
        return res

    def ltrack_device(self, packed, dev_ptrs, x_ptr, gains_ptr, scenarios_ptr, R, out_ptrs, dt, max_ticks, stream=None,
                      lo=None, hi=None, **opts):
        """Device-resident rollout under the LQR gains of `packed` (or of its problems [lo, hi)) on `stream`, not
        synchronised.  x_ptr: device pointer of the [batch, n_var] rows (e.g. a solve's out x); gains_ptr: device
        [batch, N-1, 2, 5] (e.g. what lqr_device wrote on the same stream); scenarios_ptr: device [R, 6]; out_ptrs:
        those of track_device and optionally tick_error [batch, max_ticks, 3]."""
        b = packed.struct(dev_ptrs) if lo is None else packed.chunk_struct(dev_ptrs, lo, hi)
        r = LtrackResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        o = ltrack_opts(dt, max_ticks, scenarios_ptr, R, gains_ptr, **opts)
        rc = self.lib.htp_obca_ltrack_batch_device(self.ctx, ctypes.byref(b), x_ptr, ctypes.byref(o), ctypes.byref(r),
                                                   stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_ltrack_batch_device failed: {self.error()}")

    def ltrack_last_ms(self):
        return self.lib.htp_obca_ltrack_last_ms(self.ctx)

    def _repair_call(self, name, *args):
        if getattr(self.lib, name)(self.ctx, *args) != 0:
            raise RuntimeError(f"[htp] {name} failed: {self.error()}")

    def repair_pack(self, packed, res, aud, states, slots, pad=0.01, max_raise=0.5):
        """The pack step over host arrays: HostResults `res` and AuditResults `aud` of `packed`, RepairStates
        `states` (updated) and RepairSlotArrays `slots` (written) -> the number of candidates packed."""
        b, r, a, o = packed.struct(), res.struct(), aud.struct(), repair_opts(pad=pad, max_raise=max_raise)
        s, sl = states.struct(), slots.struct()
        self._repair_call("htp_obca_repair_pack_batch", ctypes.byref(b), ctypes.byref(r), ctypes.byref(a),
                          ctypes.byref(o), ctypes.byref(s), ctypes.byref(sl))
        return int(slots.count[0])

    def repair_merge(self, packed, slots, re, re_aud, res, aud, states, tally=None):
        """The merge step over host arrays: the re-solve `re` / `re_aud` of the packed slots into `res`, `aud` and
        `states` (all updated in place); tally: int32 [3] or None."""
        b, sl, r1, a1, r0, a0, s = (v.struct() for v in (packed, slots, re, re_aud, res, aud, states))
        self._repair_call("htp_obca_repair_merge_batch", ctypes.byref(b), ctypes.byref(sl), ctypes.byref(r1),
                          ctypes.byref(a1), ctypes.byref(r0), ctypes.byref(a0), ctypes.byref(s),
                          None if tally is None else tally.ctypes.data)

    def repair_pack_device(self, packed, dev_ptrs, out_ptrs, audit_ptrs, state_ptrs, slot_ptrs, cap, pad=0.01,
                           max_raise=0.5, stream=None):
        """Device-resident pack on `stream`, not synchronised.  Every *_ptrs is a dict of device pointers named as
        the fields of the C struct (out: x, status; audit: metrics, flags; state: the four arrays; slots: count,
        index, adopted and the ten arrays of `cap` slots)."""
        b, o = packed.struct(dev_ptrs), repair_opts(pad=pad, max_raise=max_raise)
        r, a = _struct_of(ObcaResult, out_ptrs), _struct_of(AuditResult, audit_ptrs)
        s, sl = _struct_of(RepairState, state_ptrs), _struct_of(RepairSlots, slot_ptrs, cap=int(cap))
        self._repair_call("htp_obca_repair_pack_batch_device", ctypes.byref(b), ctypes.byref(r), ctypes.byref(a),
                          ctypes.byref(o), ctypes.byref(s), ctypes.byref(sl), stream)

    def repair_merge_device(self, packed, dev_ptrs, slot_ptrs, cap, re_ptrs, re_audit_ptrs, out_ptrs, audit_ptrs,
                            state_ptrs, tally_ptr=None, stream=None):
        """Device-resident merge on `stream`, not synchronised (dicts as repair_pack_device)."""
        b, sl = packed.struct(dev_ptrs), _struct_of(RepairSlots, slot_ptrs, cap=int(cap))
        r1, a1 = _struct_of(ObcaResult, re_ptrs), _struct_of(AuditResult, re_audit_ptrs)
        r0, a0, s = _struct_of(ObcaResult, out_ptrs), _struct_of(AuditResult, audit_ptrs), _struct_of(RepairState, state_ptrs)
        self._repair_call("htp_obca_repair_merge_batch_device", ctypes.byref(b), ctypes.byref(sl), ctypes.byref(r1),
                          ctypes.byref(a1), ctypes.byref(r0), ctypes.byref(a0), ctypes.byref(s), tally_ptr, stream)

    def repair(self, packed, res, rounds=3, pad=0.01, max_raise=0.5, stage=True, **audit_opts_):
        """The repair loop over host arrays: HostResults `res` of `packed` is updated in place with the re-solves
        that were adopted -> (AuditResults of the adopted results, RepairReports).  Overwrites last_kernel_ms."""
        aud, rep = AuditResults(packed.batch, packed.N, stage), RepairReports(packed.batch)
        b, r, a, rp = packed.struct(), res.struct(), aud.struct(), rep.report_struct()
        o = repair_opts(rounds, pad, max_raise, **audit_opts_)
        self._repair_call("htp_obca_repair_batch", ctypes.byref(b), ctypes.byref(r), ctypes.byref(o), ctypes.byref(a),
                          ctypes.byref(rp))
        return aud, rep

    def repair_device(self, packed, dev_ptrs, out_ptrs, audit_ptrs, state_ptrs, round_counts_ptr, rounds=3, pad=0.01,
                      max_raise=0.5, stream=None, **audit_opts_):
        """The repair loop over device arrays on `stream` (it synchronises the stream once per round to read the
        count back; the last merge is left enqueued).  out_ptrs: the solve's seven result arrays, updated in place;
        audit_ptrs: metrics, worst, flags (and stage_clearance), written; state_ptrs and round_counts_ptr [8, 3]:
        the report, written."""
        b, r, a = packed.struct(dev_ptrs), _struct_of(ObcaResult, out_ptrs), _struct_of(AuditResult, audit_ptrs)
        rp = RepairReport()
        rp.state, rp.round_counts = _struct_of(RepairState, state_ptrs), round_counts_ptr
        o = repair_opts(rounds, pad, max_raise, **audit_opts_)
        self._repair_call("htp_obca_repair_batch_device", ctypes.byref(b), ctypes.byref(r), ctypes.byref(o),
                          ctypes.byref(a), ctypes.byref(rp), stream)

    def repair_last_ms(self):
        """(pack, merge) kernel times of the last pack and the last merge, ms."""
        pk, mg = ctypes.c_double(), ctypes.c_double()
        self.lib.htp_obca_repair_last_ms(self.ctx, ctypes.byref(pk), ctypes.byref(mg))
        return pk.value, mg.value

    def resident_waves(self, packed):
        v = self.lib.htp_obca_resident_waves(self.ctx, ctypes.byref(packed.struct()))
        if v <= 0:
            raise RuntimeError(f"[htp] htp_obca_resident_waves failed: {self.error()}")
        return v

    def solve_queue_device(self, packed, dev_ptrs, queue, out_ptrs, stream=None, waves=0, max_wait_s=60.0):
        """Persistent launch over the resident problems of `packed`, fed by `queue` (WorkQueue)."""
        b = packed.struct(dev_ptrs)
        r = ObcaResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        rc = self.lib.htp_obca_solve_queue_device(self.ctx, ctypes.byref(b), queue.q, ctypes.byref(r), stream,
                                                  int(waves), float(max_wait_s))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_obca_solve_queue_device failed: {self.error()}")

    def last_cycles(self, batch):
        """[batch, 8] shader-cycle counters: local sweeps, stage assembly,
        stage chain, KKT solves, total, errors+grad_lag, line search, update+re-eval."""
        out = np.zeros((batch, 8), dtype=np.int64)
        if self.lib.htp_last_cycles(self.ctx, out.ctypes.data, int(batch)) != 0:
            raise RuntimeError(self.error())
        return out

    def rs_all_paths(self, queries):
        """Reeds-Shepp calc_all_paths for a batch of queries [B, 8] =
        (sx, sy, syaw, gx, gy, gyaw, maxc, step_size); returns CSR numpy arrays
        (host buffers; a size query first, then the fill)."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float64).reshape(-1, 8))
        B = q.shape[0]
        out = {"path_offsets": np.zeros(B + 1, np.int64), "status": np.zeros(B, np.int32)}
        cap_p = cap_q = 0
        for _ in range(2):
            out.update(lengths=np.zeros((cap_p, 5)), ctypes=np.zeros((cap_p, 5), np.int8), L=np.zeros(cap_p),
                       point_offsets=np.zeros(cap_p + 1, np.int64), x=np.zeros(cap_q), y=np.zeros(cap_q),
                       yaw=np.zeros(cap_q), cs=np.zeros(cap_q), directions=np.zeros(cap_q, np.int8))
            st = RsPaths(cap_p, cap_q, 0, 0, *[out[k].ctypes.data for k in (
                "path_offsets", "status", "lengths", "ctypes", "L", "point_offsets", "x", "y", "yaw", "cs",
                "directions")])
            rc = self.lib.htp_rs_all_paths_batch(self.ctx, B, q.ctypes.data, ctypes.byref(st))
            if rc == 0:
                break
            if rc != RS_CAPACITY:
                raise RuntimeError(f"[htp] htp_rs_all_paths_batch failed: {self.error()}")
            cap_p, cap_q = int(st.n_paths), int(st.n_points)
        else:
            raise RuntimeError("[htp] htp_rs_all_paths_batch: capacity negotiation failed")
        out["n_paths"], out["n_points"] = int(st.n_paths), int(st.n_points)
        return out

    def rs_all_paths_device(self, batch, q_ptr, out_ptrs, caps, totals_ptr, stream=None):
        st = RsPaths(int(caps[0]), int(caps[1]), 0, 0, *[out_ptrs.get(k) for k in (
            "path_offsets", "status", "lengths", "ctypes", "L", "point_offsets", "x", "y", "yaw", "cs",
            "directions")])
        rc = self.lib.htp_rs_all_paths_batch_device(self.ctx, int(batch), q_ptr, ctypes.byref(st), totals_ptr, stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_rs_all_paths_batch_device failed: {self.error()}")

    def rs_last_ms(self):
        return self.lib.htp_rs_last_ms(self.ctx)

    def hastar(self, packed):
        """Hybrid A* searches of a HastarPacked batch (host buffers, synchronous)."""
        res = HastarResults(packed)
        b, r = packed.struct(), res.struct()
        rc = self.lib.htp_hastar_search_batch(self.ctx, ctypes.byref(b), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_hastar_search_batch failed: {self.error()}")
        return res

    def hastar_device(self, packed, dev_ptrs, out_ptrs, stream=None):
        b = packed.struct(dev_ptrs)
        r = HaResult()
        for k, v in out_ptrs.items():
            setattr(r, k, v)
        rc = self.lib.htp_hastar_search_batch_device(self.ctx, ctypes.byref(b), ctypes.byref(r), stream)
        if rc != 0:
            raise RuntimeError(f"[htp] htp_hastar_search_batch_device failed: {self.error()}")

    def hastar_last_ms(self):
        return self.lib.htp_hastar_last_ms(self.ctx)

    def ypark(self, packed):
        """Y-park grid searches of a YparkPacked batch (host buffers, synchronous)."""
        res = YparkResults(packed)
        b, r = packed.struct(), res.struct()
        rc = self.lib.htp_ypark_search_batch(self.ctx, ctypes.byref(b), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"[htp] htp_ypark_search_batch failed: {self.error()}")
        return res

    def ypark_last_ms(self):
        return self.lib.htp_ypark_last_ms(self.ctx)

    def close(self):
        if self.ctx:
            self.lib.htp_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

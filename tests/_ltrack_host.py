"""TEST-ONLY: ctypes access to the serial host build of the rollout under the LQR gains
(headland_trajectory_planning_amd/csrc/ltrack_hostsim.cpp -> build/libhtp_ltrack_host.so), the stand-alone sanitizer
program of the same core, a numpy restatement of the definition in include/htp.h and the batches the ltrack tests
share.  The product never loads it.  The problem builders, the reference signal, the plant and the signed distance
of the restatement are those of _track_host; the gains come from _lqr_host's host build."""
import ctypes
import os
import subprocess

import numpy as np

import _lqr_host as lh
import _track_host as tk
from _track_host import needed_ticks, parts, polygons  # noqa: F401  (re-exported to the tests)
from headland_trajectory_planning_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "headland_trajectory_planning_amd", "csrc")
SO = os.path.join(ROOT, "build", "libhtp_ltrack_host.so")
ASAN_EXE = os.path.join(ROOT, "build", "ltrack_asan")
_DEPS = ("ltrack_hostsim.cpp", "ltrack_batch.h", "ltrack_core.h", "track_core.h", "audit_core.h", "htp_common.h",
         "htp_libm.h")
SENTINEL = tk.SENTINEL
ISENTINEL = tk.ISENTINEL
F = _native.TRACK_FLAGS
NMET = len(_native.TRACK_METRICS)
NAMES = ("metrics", "worst", "flags", "tally", "worst_scenario", "tick_clearance", "reference", "tick_error")


def _deps(extra=()):
    return [os.path.join(CSRC, f) for f in _DEPS + tuple(extra)] + [os.path.join(ROOT, "include", "htp.h")]


def _fresh(out, deps):
    return os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps)


def build():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if _fresh(SO, _deps()):
        return SO
    subprocess.check_call(["g++", "-O2", "-fno-builtin", "-std=c++17", "-shared", "-fPIC", "-o", SO,
                           os.path.join(CSRC, "ltrack_hostsim.cpp")])
    return SO


def build_asan():
    """csrc/ltrack_asan.cpp (its own main) with -fsanitize=address,undefined: a plain executable."""
    os.makedirs(os.path.dirname(ASAN_EXE), exist_ok=True)
    if _fresh(ASAN_EXE, _deps(("ltrack_asan.cpp",))):
        return ASAN_EXE
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", ASAN_EXE,
                           os.path.join(CSRC, "ltrack_asan.cpp")])
    return ASAN_EXE


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.htp_hostsim_obca_ltrack.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_char_p, ctypes.c_int32]
        _lib.htp_hostsim_obca_ltrack.restype = ctypes.c_int
    return _lib


def raw_call(batch_struct, x_ptr, opts_struct, result_struct):
    """The C entry with possibly-null struct pointers -> (return code, message)."""
    msg = ctypes.create_string_buffer(256)

    def ref(s):
        return None if s is None else ctypes.cast(ctypes.pointer(s), ctypes.c_void_p)
    rc = lib().htp_hostsim_obca_ltrack(ref(batch_struct), x_ptr, ref(opts_struct), ref(result_struct), msg, 256)
    return rc, msg.value.decode()


def sentinel_results(rows, R, max_ticks, scenarios=None, ticks=True, reference=True, errors=True):
    """LtrackResults whose arrays carry the sentinels: what a run leaves untouched stays recognisable."""
    res = _native.LtrackResults(rows, R, max_ticks, scenarios, ticks, reference, errors)
    for a in (res.metrics, res.tick_clearance, res.reference, res.tick_error):
        if a is not None:
            a[...] = SENTINEL
    for a in (res.worst, res.flags, res.tally, res.worst_scenario):
        a[...] = ISENTINEL
    return res


def ltrack_host(packed, x, gains, scenarios, dt, max_ticks, rows=None, ticks=True, reference=True, errors=True, **opts):
    """The host build's rollout of `x` [batch, n_var] under `gains` [batch, N-1, 2, 5] -> _native.LtrackResults
    (pre-filled with the sentinels)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    gains = np.ascontiguousarray(gains, dtype=np.float64)
    scenarios = np.ascontiguousarray(scenarios, dtype=np.float64)
    assert x.shape == (packed.batch, packed.n_var), (x.shape, packed.batch, packed.n_var)
    assert gains.shape == (packed.batch, packed.N - 1, 2, 5), gains.shape
    res = sentinel_results(packed.batch if rows is None else rows, len(scenarios), max_ticks, scenarios, ticks,
                           reference, errors)
    o = _native.ltrack_opts(dt, max_ticks, scenarios.ctypes.data, len(scenarios), gains.ctypes.data, **opts)
    rc, msg = raw_call(packed.struct(), x.ctypes.data, o, res.struct())
    if rc != 0:
        raise RuntimeError(msg)
    return res


def host_gains(packed, x, **lqr_opts):
    """The host LQR build's gains of x, with NaN (not the sentinel) where the LQR wrote none."""
    res = lh.lqr_host(packed, x, cost_to_go=False, linearisation=False, **lqr_opts)
    g = res.gains.copy()
    g[g == lh.SENTINEL] = np.nan
    return g


# ------------------------------------------------------------------ numpy restatement of the definition
def np_ltrack(obstacles, bodies, X, U, tau, par, topt, gains, scen, dt, max_ticks, plant_substeps=2, abort_dist=2.0,
              margin_tol=1e-4):
    """One (finite, well-timed) problem from the definition -> dict(metrics [R, 8], worst [R, 3], flags [R],
    tick [np], err [np, 3], ref [np, 5], gap, poses): `gap` is the smallest distance of any compared quantity
    (clearance, position error, clamp argument) from its threshold."""
    P_ = _native
    dT, wb, dmin = par[P_.P_DT], par[P_.P_WHEELBASE], par[P_.P_DMIN]
    vmax, smax = abs(par[P_.P_MAXV]), abs(par[P_.P_MAXSTEER])
    amax, wmax = abs(par[P_.P_MAXACC]), abs(par[P_.P_MAXSR])
    N = len(X)
    ref, n = tk.np_reference(X, U, tau, dT, wb, dt, topt)
    h = dT * tau if topt else np.full(N - 1, dT)
    t = np.concatenate([[0.0], np.cumsum(h)])
    npose = min(n + 1, max_ticks)
    polybad = any(v is None for v in obstacles) or any(v is None for v in bodies)
    M, K, R = len(obstacles), len(bodies), len(scen)
    out = dict(metrics=np.full((R, NMET), np.nan), worst=np.full((R, 3), -1, np.int32), flags=np.zeros(R, np.int32),
               tick=np.full(npose, np.nan if polybad else np.inf), err=np.zeros((npose, 3)), gap=np.inf, poses=[])
    gaps = []
    for r, (lat0, lon0, yaw0, bias, slip, ygain) in enumerate(scen):
        if not np.all(np.isfinite(scen[r])):
            out["flags"][r] = F["NONFINITE"]
            out["poses"].append(None)
            continue
        c0, s0 = np.cos(X[0, 3]), np.sin(X[0, 3])
        q = np.array([(X[0, 0] + lon0 * c0) - lat0 * s0, (X[0, 1] + lon0 * s0) + lat0 * c0, X[0, 2], X[0, 3] + yaw0,
                      X[0, 4]])
        keep = 1.0 - slip
        clr, worst, fl = np.inf, (-1, -1, -1), 0
        mx = np.zeros(4)
        nctl = nsat = 0
        epos = eth = 0.0
        trace = []
        for k in range(npose):
            xr, yr, vr, thr, dr = ref[k]
            c, s = np.cos(thr), np.sin(thr)
            e_lon = c * (q[0] - xr) + s * (q[1] - yr)
            e_lat = c * (q[1] - yr) - s * (q[0] - xr)
            d = q[3] - thr
            e_th = np.arctan2(np.sin(d), np.cos(d))
            trace.append(q.copy())
            if not polybad:
                ct, st = np.cos(q[3]), np.sin(q[3])
                Rm = np.array([[ct, -st], [st, ct]])
                for m in range(M):
                    for b in range(K):
                        dist = tk.np_signed_distance(obstacles[m], bodies[b] @ Rm.T + q[:2])
                        out["tick"][k] = min(out["tick"][k], dist)
                        if dist < clr:
                            clr, worst = dist, (k, m, b)
            mx = np.maximum(mx, [abs(e_lat), abs(e_lon), abs(e_th), abs(q[4] - dr)])
            out["err"][k] = np.maximum(out["err"][k], [abs(e_lat), abs(e_lon), abs(e_th)])
            epos, eth = np.hypot(e_lon, e_lat), abs(e_th)
            gaps.append(abs(epos - abort_dist))
            if not epos <= abort_dist:
                fl |= F["DIVERGED"]
                break
            if k + 1 < npose:
                i = int(np.searchsorted(t[:N - 1], np.float64(k) * dt, side="right") - 1)
                Ki = gains[i]
                ci, si = np.cos(X[i, 3]), np.sin(X[i, 3])
                Rot = np.array([[ci, si], [-si, ci]])          # world -> frame of node i
                Kf = np.concatenate([Ki[:, :2] @ Rot.T, Ki[:, 2:]], axis=1)      # columns lon, lat, v, theta, delta
                fb = Kf @ np.array([e_lon, e_lat, q[2] - vr, e_th, q[4] - dr])
                vrn, drn = ref[k + 1, 2], ref[k + 1, 4]
                a_cmd = (vrn - vr) / dt - fb[0]
                w_cmd = (drn - dr) / dt - fb[1]
                v_des, _ = tk._clamp(q[2] + dt * a_cmd, vmax, gaps)
                a, ba = tk._clamp((v_des - q[2]) / dt, amax, gaps)
                d_des, bs = tk._clamp(q[4] + dt * w_cmd, smax, gaps)
                w, bw = tk._clamp((d_des - q[4]) / dt, wmax, gaps)
                fl |= (F["SAT_ACC"] if ba else 0) | (F["SAT_STEER"] if bs else 0) | (F["SAT_RATE"] if bw else 0)
                nctl += 1
                nsat += bool(ba or bs or bw)
                hp = dt / plant_substeps
                for _ in range(plant_substeps):
                    qm = q + (0.5 * hp) * tk._plant_f(q, a, w, wb, keep, bias, ygain)
                    q = q + hp * tk._plant_f(qm, a, w, wb, keep, bias, ygain)
                q[4] = min(max(q[4], -smax), smax)
        if n + 1 > max_ticks:
            fl |= F["TRUNCATED"]
        if polybad:
            fl |= F["BAD_POLYTOPE"]
            clr = np.nan
        else:
            gaps += [abs(clr), abs(clr - (dmin - margin_tol))]
            fl |= (F["COLLISION"] if clr < 0 else 0) | (F["MARGIN"] if clr < dmin - margin_tol else 0)
        out["metrics"][r] = [clr, mx[0], mx[1], mx[2], epos, eth, mx[3], nsat / nctl if nctl else 0.0]
        out["worst"][r] = worst
        out["flags"][r] = fl
        out["poses"].append(np.array(trace))
    out["gap"] = min(gaps) if gaps else np.inf
    out["ref"] = ref[:npose]
    return out


def np_ltrack_problem(pk, x, gains, p, scen, dt, max_ticks, **opts):
    X, U, tau = parts(pk, x)
    obs, bod = polygons(pk, p)
    return np_ltrack(obs, bod, X[p], U[p], tau[p], pk.params[p], pk.time_opt, gains[p], scen, dt, max_ticks, **opts)


# ------------------------------------------------------------------ the batches of the device-vs-host comparison
def ltrack_batch(seed, batch, N, time_opt, R, M, K, dt_over_dT):
    """_track_host.track_batch (problem 0 the longest; with room, problem 1 a NaN state and problem 2 a bad time,
    scenario 1 a NaN and scenario 2 diverging) with the host LQR build's gains of it; with room (batch >= 4) the
    last problem carries one NaN gain -> (PackedBatch, x, gains, scenarios, dt)."""
    pk, x, scen, dt = tk.track_batch(seed, batch, N, time_opt, R, M, K, dt_over_dT)
    gains = host_gains(pk, x)
    if batch >= 3:
        gains[2] = 0.25      # the LQR rejects the bad-time problem and leaves it no gains: finite ones reach BAD_TIME
    if batch >= 4:
        gains[batch - 1, (N - 1) // 2, 1, 3] = np.nan
    return pk, x, gains, scen, dt

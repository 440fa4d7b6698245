"""TEST-ONLY: ctypes access to the serial host build of the tracking rollout
(headland_trajectory_planning_amd/csrc/track_hostsim.cpp -> build/libhtp_track_host.so), the stand-alone sanitizer
program of the same core, a numpy restatement of the definition in include/htp.h and the batches the track tests
share.  The product never loads it.  The problem builders are those of _audit_host."""
import ctypes
import os
import subprocess

import numpy as np

from _audit_host import instance, ngon, random_batch, rect, x_of  # noqa: F401  (re-exported to the tests)
from _timeline_host import np_step, parts  # noqa: F401
from headland_trajectory_planning_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "headland_trajectory_planning_amd", "csrc")
SO = os.path.join(ROOT, "build", "libhtp_track_host.so")
ASAN_EXE = os.path.join(ROOT, "build", "track_asan")
_DEPS = ("track_hostsim.cpp", "track_batch.h", "track_core.h", "audit_core.h", "htp_common.h", "htp_libm.h")
SENTINEL = -7.25
ISENTINEL = -77
F = _native.TRACK_FLAGS
NMET = len(_native.TRACK_METRICS)


def _deps(extra=()):
    return [os.path.join(CSRC, f) for f in _DEPS + tuple(extra)] + [os.path.join(ROOT, "include", "htp.h")]


def _fresh(out, deps):
    return os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps)


def build():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if _fresh(SO, _deps()):
        return SO
    subprocess.check_call(["g++", "-O2", "-fno-builtin", "-std=c++17", "-shared", "-fPIC", "-o", SO,
                           os.path.join(CSRC, "track_hostsim.cpp")])
    return SO


def build_asan():
    """csrc/track_asan.cpp (its own main) with -fsanitize=address,undefined: a plain executable."""
    os.makedirs(os.path.dirname(ASAN_EXE), exist_ok=True)
    if _fresh(ASAN_EXE, _deps(("track_asan.cpp",))):
        return ASAN_EXE
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", ASAN_EXE,
                           os.path.join(CSRC, "track_asan.cpp")])
    return ASAN_EXE


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.htp_hostsim_obca_track.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_char_p, ctypes.c_int32]
        _lib.htp_hostsim_obca_track.restype = ctypes.c_int
    return _lib


def raw_call(batch_struct, x_ptr, opts_struct, result_struct):
    """The C entry with possibly-null struct pointers -> (return code, message)."""
    msg = ctypes.create_string_buffer(256)

    def ref(s):
        return None if s is None else ctypes.cast(ctypes.pointer(s), ctypes.c_void_p)
    rc = lib().htp_hostsim_obca_track(ref(batch_struct), x_ptr, ref(opts_struct), ref(result_struct), msg, 256)
    return rc, msg.value.decode()


def sentinel_results(rows, R, max_ticks, scenarios=None, ticks=True, reference=True):
    """TrackResults whose arrays carry the sentinels: what a run leaves untouched stays recognisable."""
    res = _native.TrackResults(rows, R, max_ticks, scenarios, ticks, reference)
    for a in (res.metrics, res.tick_clearance, res.reference):
        if a is not None:
            a[...] = SENTINEL
    for a in (res.worst, res.flags, res.tally, res.worst_scenario):
        a[...] = ISENTINEL
    return res


def track_host(packed, x, scenarios, dt, max_ticks, rows=None, ticks=True, reference=True, **opts):
    """The host build's rollout of `x` [batch, n_var] for a _native.PackedBatch -> _native.TrackResults (pre-filled
    with the sentinels)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    scenarios = np.ascontiguousarray(scenarios, dtype=np.float64)
    assert x.shape == (packed.batch, packed.n_var), (x.shape, packed.batch, packed.n_var)
    res = sentinel_results(packed.batch if rows is None else rows, len(scenarios), max_ticks, scenarios, ticks, reference)
    o = _native.track_opts(dt, max_ticks, scenarios.ctypes.data, len(scenarios), **opts)
    rc, msg = raw_call(packed.struct(), x.ctypes.data, o, res.struct())
    if rc != 0:
        raise RuntimeError(msg)
    return res


# ------------------------------------------------------------------ numpy restatement of the definition
def np_vertices(A, b):
    """Vertices of {A x <= b}, counter-clockwise: the pairwise intersections of the rows that satisfy all rows.
    Fewer than three: a bad polytope."""
    pts = []
    for i in range(len(b)):
        for j in range(i + 1, len(b)):
            Aij = np.array([A[i], A[j]])
            if abs(np.linalg.det(Aij)) < 1e-12:
                continue
            v = np.linalg.solve(Aij, np.array([b[i], b[j]]))
            if np.all(A @ v <= b + 1e-9) and not any(np.hypot(*(v - q)) < 1e-9 for q in pts):
                pts.append(v)
    if len(pts) < 3:
        return None
    pts = np.array(pts)
    c = pts.mean(axis=0)
    return pts[np.argsort(np.arctan2(pts[:, 1] - c[1], pts[:, 0] - c[0]))]


def _edges(V):
    d = np.roll(V, -1, axis=0) - V
    n = np.stack([d[:, 1], -d[:, 0]], axis=1)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return n, np.einsum("ij,ij->i", n, V)


def _point_segments(P, V):
    """Smallest distance from the points P to the closed edges of polygon V."""
    a, d = V, np.roll(V, -1, axis=0) - V
    best = np.inf
    for p in P:
        t = np.clip(np.einsum("ij,ij->i", p - a, d) / np.einsum("ij,ij->i", d, d), 0.0, 1.0)
        best = min(best, np.min(np.hypot(*(p - (a + t[:, None] * d)).T)))
    return best


def np_signed_distance(Vo, Vb):
    """Two convex polygons (world vertices): distance when disjoint, minus the penetration depth otherwise."""
    sep = -np.inf
    for V, W in ((Vo, Vb), (Vb, Vo)):
        n, off = _edges(V)
        sep = max(sep, np.max(np.min(W @ n.T - off[None, :], axis=0)))
    return min(_point_segments(Vb, Vo), _point_segments(Vo, Vb)) if sep > 0 else sep


def np_reference(X, U, tau, dT, wb, dt, topt):
    """(ref [n + 1, 5], n): ref(k), k = 0..n, from the definition."""
    N = len(X)
    h = dT * tau if topt else np.full(N - 1, dT)
    t = np.concatenate([[0.0], np.cumsum(h)])
    T = t[-1]
    n = 0
    while np.float64(n) * dt < T:
        n += 1
    ref = np.zeros((n + 1, 5))
    for k in range(n):
        s = np.float64(k) * dt
        i = int(np.searchsorted(t[:N - 1], s, side="right") - 1)
        ref[k] = np_step(X[i], U[i, 0], U[i, 1], wb, s - t[i], topt)
    ref[n] = X[-1]
    return ref, n


def _clamp(u, m, gaps):
    gaps.append(min(abs(u + m), abs(u - m)))
    return (-m if u < -m else (m if u > m else u)), (u < -m or u > m)


def _plant_f(q, a, w, wb, keep, bias, ygain):
    v = keep * q[2]
    return np.array([v * np.cos(q[3]), v * np.sin(q[3]), a, v * np.tan(q[4] + bias) / wb * ygain, w])


def np_track(obstacles, bodies, X, U, tau, par, topt, scen, dt, max_ticks, plant_substeps=2, k_lat=0.5, k_yaw=2.0,
             k_lon=1.0, abort_dist=2.0, margin_tol=1e-4, poses=False):
    """One (finite, well-timed) problem from the definition: obstacles / bodies as vertex arrays or None for a bad
    polytope -> dict(metrics [R, 8], worst [R, 3], flags [R], tick [np], gap, poses): `gap` is the smallest distance
    of any compared quantity (clearance, position error, clamp argument) from its threshold."""
    P_ = _native
    dT, wb, dmin = par[P_.P_DT], par[P_.P_WHEELBASE], par[P_.P_DMIN]
    vmax, smax = abs(par[P_.P_MAXV]), abs(par[P_.P_MAXSTEER])
    amax, wmax = abs(par[P_.P_MAXACC]), abs(par[P_.P_MAXSR])
    ref, n = np_reference(X, U, tau, dT, wb, dt, topt)
    npose = min(n + 1, max_ticks)
    polybad = any(v is None for v in obstacles) or any(v is None for v in bodies)
    M, K, R = len(obstacles), len(bodies), len(scen)
    out = dict(metrics=np.full((R, NMET), np.nan), worst=np.full((R, 3), -1, np.int32), flags=np.zeros(R, np.int32),
               tick=np.full(npose, np.nan if polybad else np.inf), gap=np.inf, poses=[])
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
                        dist = np_signed_distance(obstacles[m], bodies[b] @ Rm.T + q[:2])
                        out["tick"][k] = min(out["tick"][k], dist)
                        if dist < clr:
                            clr, worst = dist, (k, m, b)
            mx = np.maximum(mx, [abs(e_lat), abs(e_lon), abs(e_th), abs(q[4] - dr)])
            epos, eth = np.hypot(e_lon, e_lat), abs(e_th)
            gaps.append(abs(epos - abort_dist))
            if not epos <= abort_dist:
                fl |= F["DIVERGED"]
                break
            if k + 1 < npose:
                vrn, drn = ref[k + 1, 2], ref[k + 1, 4]
                g = -1.0 if vrn < 0 else 1.0
                v_des, _ = _clamp(vrn - k_lon * e_lon, vmax, gaps)
                a, ba = _clamp((v_des - q[2]) / dt, amax, gaps)
                d_des, bs = _clamp((drn - k_lat * e_lat) - (g * k_yaw) * e_th, smax, gaps)
                w, bw = _clamp((d_des - q[4]) / dt, wmax, gaps)
                fl |= (F["SAT_ACC"] if ba else 0) | (F["SAT_STEER"] if bs else 0) | (F["SAT_RATE"] if bw else 0)
                nctl += 1
                nsat += bool(ba or bs or bw)
                hp = dt / plant_substeps
                for _ in range(plant_substeps):
                    qm = q + (0.5 * hp) * _plant_f(q, a, w, wb, keep, bias, ygain)
                    q = q + hp * _plant_f(qm, a, w, wb, keep, bias, ygain)
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


def polygons(pk, p):
    """(obstacle vertex arrays, body vertex arrays) of problem p; None where a polygon is bad."""
    oo = np.concatenate([[0], np.cumsum(pk.obs_edges)])
    bo = np.concatenate([[0], np.cumsum(pk.body_edges)])
    return ([np_vertices(pk.obs_A[p, oo[m]:oo[m + 1]], pk.obs_b[p, oo[m]:oo[m + 1]]) for m in range(pk.M)],
            [np_vertices(pk.body_G[p, bo[k]:bo[k + 1]], pk.body_g[p, bo[k]:bo[k + 1]]) for k in range(pk.K)])


def np_track_problem(pk, x, p, scen, dt, max_ticks, **opts):
    X, U, tau = parts(pk, x)
    obs, bod = polygons(pk, p)
    return np_track(obs, bod, X[p], U[p], tau[p], pk.params[p], pk.time_opt, scen, dt, max_ticks, **opts)


def needed_ticks(pk, x, dt):
    """n + 1 of every problem by the numpy restatement (0 for the rejected ones)."""
    X, U, tau = parts(pk, x)
    out = []
    for p in range(pk.batch):
        dT = pk.params[p, _native.P_DT]
        h = dT * tau[p] if pk.time_opt else np.full(pk.N - 1, dT)
        if not (np.all(np.isfinite(X[p])) and np.all(np.isfinite(U[p])) and np.all(np.isfinite(h))) or np.any(h <= 0):
            out.append(0)
            continue
        T = np.cumsum(h)[-1]
        n = 0
        while np.float64(n) * dt < T:
            n += 1
        out.append(n + 1)
    return np.array(out)


# ------------------------------------------------------------------ the batches of the device-vs-host comparison
def drivable_batch(seed, batch, N, M, K, time_opt, dT=0.1, wheelbase=1.9, obs_edges=None, body_edges=None):
    """Seeded problems whose trajectories a vehicle can follow: the nodes are the NLP's own integrator run over
    small random controls (plus 1 mm of noise, so that the defect is not zero), even problems forward and odd ones
    in reverse, tau in [0.6, 1], and convex obstacles beside the path -> (PackedBatch, x)."""
    rng = np.random.default_rng(seed)
    obs_edges = list(obs_edges) if obs_edges is not None else [3 + (m % 4) for m in range(M)]
    body_edges = list(body_edges) if body_edges is not None else [4] * K
    insts, Xs, Us, Ts = [], [], [], []
    for p in range(batch):
        tau = rng.uniform(0.6, 1.0, N - 1) if time_opt else np.ones(N - 1)
        U = np.stack([rng.normal(0, 0.15, N - 1), rng.normal(0, 0.1, N - 1)], axis=1)
        X = np.zeros((N, 5))
        X[0] = [rng.normal(0, 1), rng.normal(0, 1), -0.8 if p % 2 else 0.8, rng.uniform(-3, 3), rng.normal(0, 0.1)]
        for i in range(N - 1):
            X[i + 1] = np_step(X[i], U[i, 0], U[i, 1], wheelbase, dT * tau[i], time_opt)
            X[i + 1, 2] = np.clip(X[i + 1, 2], -1.5, 1.5)
            X[i + 1, 4] = np.clip(X[i + 1, 4], -0.5, 0.5)
        X += rng.normal(0, 1e-3, X.shape)
        obstacles = []
        for m in range(M):
            i = int(rng.integers(0, N))
            side = rng.choice([-1.0, 1.0]) * rng.uniform(2.0, 4.0)
            c = X[i, :2] + side * np.array([-np.sin(X[i, 3]), np.cos(X[i, 3])])
            obstacles.append(ngon(c[0], c[1], rng.uniform(0.4, 1.0), obs_edges[m], rng.uniform(0, 6.28)))
        bodies = [ngon(0.8 * k, 0.0, 0.9, body_edges[k], 0.4 + k) for k in range(K)]
        insts.append(instance(X, obstacles, bodies, time_opt=time_opt, dT=dT, wheelbase=wheelbase))
        Xs.append(X)
        Us.append(U)
        Ts.append(tau)
    pk = _native.PackedBatch(insts)
    return pk, x_of(pk, np.stack(Xs), np.stack(Us), np.stack(Ts), fill=np.nan)


def track_batch(seed, batch, N, time_opt, R, M, K, dt_over_dT):
    """Seeded drivable problems and a seeded scenario table -> (PackedBatch, x, scenarios, dt).  Problem 0 is the
    longest, so that a max_ticks one short of what it needs truncates it alone; where the batch has room, problem
    1 carries a NaN state and problem 2 a zero time scale (time_opt) or a negative dT; where the table has room,
    scenario 1 carries a NaN and scenario 2 starts beyond any abort distance the tests use."""
    pk, x = drivable_batch(seed, batch, N, M, K, time_opt)
    dT = float(pk.params[0, _native.P_DT])
    o_tau = pk.n_var - 5 - (N - 1)
    if time_opt:
        x[0, o_tau:o_tau + N - 1] = 1.0
    else:
        pk.params[0, _native.P_DT] = 1.25 * dT
    if batch >= 3:
        x[1, 5 * (N // 2) + 1] = np.nan
        if time_opt:
            x[2, o_tau + (N - 1) // 2] = 0.0
        else:
            pk.params[2, _native.P_DT] = -dT
    scen = _native.track_scenarios(R, seed)
    if R >= 3:
        scen[1, 3] = np.nan
        scen[2, 0] = 25.0
    return pk, x, scen, dT * dt_over_dT

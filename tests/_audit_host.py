"""TEST-ONLY: ctypes access to the serial host build of the trajectory audit
(headland_trajectory_planning_amd/csrc/audit_hostsim.cpp -> build/libhtp_audit_host.so), plus the small
problem builders the audit tests share.  The product never loads it."""
import ctypes
import os
import subprocess

import numpy as np

from headland_trajectory_planning_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "headland_trajectory_planning_amd", "csrc")
SO = os.path.join(ROOT, "build", "libhtp_audit_host.so")
_DEPS = ("audit_hostsim.cpp", "audit_batch.h", "audit_core.h", "htp_common.h", "htp_libm.h")


def build():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    deps = [os.path.join(CSRC, f) for f in _DEPS] + [os.path.join(ROOT, "include", "htp.h")]
    if os.path.exists(SO) and os.path.getmtime(SO) >= max(os.path.getmtime(d) for d in deps):
        return SO
    subprocess.check_call(["g++", "-O2", "-fno-builtin", "-std=c++17", "-shared", "-fPIC", "-o", SO,
                           os.path.join(CSRC, "audit_hostsim.cpp")])
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.htp_hostsim_obca_audit.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_char_p, ctypes.c_int32]
        _lib.htp_hostsim_obca_audit.restype = ctypes.c_int
    return _lib


def raw_call(batch_struct, x_ptr, opts_struct, result_struct):
    """The C entry with possibly-null struct pointers -> (return code, message)."""
    msg = ctypes.create_string_buffer(256)

    def ref(s):
        return None if s is None else ctypes.cast(ctypes.pointer(s), ctypes.c_void_p)
    rc = lib().htp_hostsim_obca_audit(ref(batch_struct), x_ptr, ref(opts_struct), ref(result_struct), msg, 256)
    return rc, msg.value.decode()


def audit_host(packed, x, stage=True, rows=None, **opts):
    """The host build's audit of `x` [batch, n_var] for a _native.PackedBatch -> _native.AuditResults."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.shape == (packed.batch, packed.n_var), (x.shape, packed.batch, packed.n_var)
    res = _native.AuditResults(packed.batch if rows is None else rows, packed.N, stage)
    rc, msg = raw_call(packed.struct(), x.ctypes.data, _native.audit_opts(**opts), res.struct())
    if rc != 0:
        raise RuntimeError(msg)
    return res


# ------------------------------------------------------------------ problem builders
def halfspaces(vertices):
    """Counter-clockwise convex polygon -> (A, b) with A x <= b, rows of unit length, rounded to 7 decimals as the
    reference's cdd output is."""
    v = np.asarray(vertices, dtype=np.float64)
    d = np.roll(v, -1, axis=0) - v
    n = np.stack([d[:, 1], -d[:, 0]], axis=1)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return np.round(n, 7), np.round(np.einsum("ij,ij->i", n, v), 7)


def rect(cx, cy, w, h, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    pts = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]])
    return pts @ np.array([[c, s], [-s, c]]) + [cx, cy]


def ngon(cx, cy, r, n, phase=0.0):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)


def instance(traj, obstacles, bodies, time_opt=True, dT=0.1, min_dist=0.1, wheelbase=1.9, **kw):
    """An OBCA instance dict (the fields _native.PackedBatch reads) from vertex lists."""
    oh = [halfspaces(o) if not isinstance(o, tuple) else o for o in obstacles]
    bh = [halfspaces(o) if not isinstance(o, tuple) else o for o in bodies]
    inst = dict(init_traj=np.asarray(traj, dtype=np.float64), obs_A=[a for a, _ in oh], obs_b=[b for _, b in oh],
                body_G=[a for a, _ in bh], body_g=[b for _, b in bh], dT=dT, Q=np.eye(2), R=np.eye(2),
                W=np.diag([1.0, 1.0 if time_opt else 0.0]), wheelbase=wheelbase, max_steer=0.6, max_velocity=2.0,
                max_accel=1.0, max_steer_rate=0.8, min_dist=min_dist, x_bound=[-100.0, 100.0],
                y_bound=[-100.0, 100.0], init_control=None, init_mu=None, init_lambda=None)
    inst.update(kw)
    return inst


def x_of(packed, X, U, tau=None, fill=0.1):
    """Decision vectors in the optimizer's layout from X [B, N, 5], U [B, N-1, 2], tau [B, N-1]; duals = fill."""
    B, N = packed.batch, packed.N
    x = np.full((B, packed.n_var), fill)
    x[:, :5 * N] = np.asarray(X).reshape(B, -1)
    x[:, 5 * N:5 * N + 2 * (N - 1)] = np.asarray(U).reshape(B, -1)
    if packed.time_opt:
        x[:, -5 - (N - 1):-5] = np.ones((B, N - 1)) if tau is None else np.asarray(tau).reshape(B, -1)
    x[:, -5:] = 0.0
    return x


def random_batch(seed, batch, N, M, K, obs_edges=None, body_edges=None, time_opt=True, flags=True):
    """Seeded problems for the device-vs-host comparison: a noisy trajectory through a field of convex obstacles.
    With `flags`, problems 1.. carry a collision, a control kick, a bound excess, a NaN state and an infeasible
    obstacle in turn (where the batch is large enough) -> (PackedBatch, x)."""
    rng = np.random.default_rng(seed)
    obs_edges = list(obs_edges) if obs_edges is not None else [4] * M
    body_edges = list(body_edges) if body_edges is not None else [4] * K
    insts, Xs, Us, Ts = [], [], [], []
    for _ in range(batch):
        t = np.linspace(0.0, 1.0, N)
        th = 0.5 * np.pi * t + rng.normal(0, 0.05, N)
        X = np.stack([8.0 * t + rng.normal(0, 0.05, N), 3.0 * t ** 2 + rng.normal(0, 0.05, N),
                      0.8 + rng.normal(0, 0.05, N), th, rng.normal(0, 0.1, N)], axis=1)
        obstacles = [ngon(rng.uniform(-2, 10), rng.choice([-1, 1]) * rng.uniform(3.5, 7) + 1.5, rng.uniform(0.5, 1.5),
                          obs_edges[m], rng.uniform(0, 6.28)) for m in range(M)]
        bodies = [ngon(0.8 * k, 0.0, 0.9, body_edges[k], 0.4 + k) for k in range(K)]
        insts.append(instance(X + rng.normal(0, 1e-3, X.shape), obstacles, bodies, time_opt=time_opt))
        Xs.append(X)
        Us.append(rng.normal(0, 0.2, (N - 1, 2)))
        Ts.append(rng.uniform(0.6, 1.0, N - 1))
    if flags:
        for j, it in enumerate(insts):
            kind = j % 6
            if kind == 1:    # collision: an obstacle onto a stage
                i = (3 * j) % N
                m = j % M
                c = Xs[j][i, :2]
                it["obs_A"][m], it["obs_b"][m] = halfspaces(ngon(c[0], c[1], 0.7, obs_edges[m], 0.3))
            elif kind == 2:  # dynamics: irrelevant here (the noise already breaks them); bound excess instead
                Xs[j][(5 * j) % N, 2] = 2.5
            elif kind == 3:  # non-finite state
                Xs[j][(7 * j) % N, 1] = np.nan
            elif kind == 4:  # infeasible obstacle: two opposed rows that exclude each other
                m = j % M
                A, b = it["obs_A"][m].copy(), it["obs_b"][m].copy()
                A[1] = -A[0]
                b[1] = -b[0] - 1.0
                it["obs_A"][m], it["obs_b"][m] = A, b
            elif kind == 5:  # control beyond its bound
                Us[j][j % (N - 1), 0] = 1.7
    pk = _native.PackedBatch(insts)
    return pk, x_of(pk, np.stack(Xs), np.stack(Us), np.stack(Ts), fill=np.nan)

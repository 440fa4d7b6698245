"""GPU: the trajectory timeline kernel (csrc/htp_timeline.hip) against the serial host build of the same core
(tests/_timeline_host.py), bit for bit; through the device entry with an output base that is only 8-byte
aligned; chained behind a device-resident solve and audit on one stream; the untouched rows and problems; the
nullable outputs; and the Python surface (Context.timeline, obca_py.optimizer.timeline_batch /
solve_batch(timeline=...)).  Every batch with room for them carries a NaN problem and a BAD_TIME problem, and
every shape that can be cut (N > 2) is run with a cap one row short of what its longest problem needs."""
import contextlib
import io

import numpy as np
import pytest

import _audit_host as ah
import _timeline_host as th
from headland_trajectory_planning_amd import _native, synth

pytestmark = pytest.mark.gpu

F = _native.TIMELINE_FLAGS
NCOL = len(_native.TIMELINE_COLUMNS)


@pytest.fixture(scope="module")
def ctx():
    return _native.Context(0)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.int64), b.view(np.int64)
    return a.shape == b.shape and np.array_equal(a, b)


# N, time_opt, dt / dT, batch
SHAPES = [
    (2, True, 3.0, 3),          # dt > T: 2 rows, 62 idle lanes
    (7, False, 0.37, 7),        # Euler; a row count that is no multiple of 64 (a partial last chunk)
    (80, True, 0.25, 70),       # several chunks, mixed tau
    (480, True, 0.25, 2),       # the LDS limit
]
_cases = {}


def _case(N, topt, ratio, batch):
    """The batch of one shape, its cap and the host build's result: computed once, shared and left unchanged."""
    key = (N, topt, ratio, batch)
    if key not in _cases:
        pk, x, dt = th.timeline_batch(2000 + N, batch, N, topt, ratio)
        need = th.needed_rows(pk, x, dt)
        cap = int(need.max()) - 1 if N > 2 else 2
        _cases[key] = (pk, x, dt, cap, need, th.timeline_host(pk, x, dt, cap))
    return _cases[key]


def _device_inputs(torch, pk, dev):
    dev_in = {k: torch.from_numpy(getattr(pk, k)).to(dev) for k in pk.INPUTS if getattr(pk, k) is not None}
    return dev_in, {k: v.data_ptr() for k, v in dev_in.items()}


def _outs(torch, dev, rows, cap, offset=0, stage=True, duration=True):
    """Sentinel-filled device outputs; `rows` starts `offset` doubles into its allocation."""
    base = torch.full((rows * cap * NCOL + offset,), th.SENTINEL, dtype=torch.float64, device=dev)
    t = {"rows": base[offset:].view(rows, cap, NCOL),
         "count": torch.full((rows,), th.ISENTINEL, dtype=torch.int32, device=dev),
         "flags": torch.full((rows,), th.ISENTINEL, dtype=torch.int32, device=dev),
         "stage": torch.full((rows, cap), th.ISENTINEL, dtype=torch.int32, device=dev) if stage else None,
         "duration": torch.full((rows,), th.SENTINEL, dtype=torch.float64, device=dev) if duration else None}
    ptrs = {k: (None if v is None else v.data_ptr()) for k, v in t.items()}
    assert ptrs["rows"] == base.data_ptr() + 8 * offset
    return t, ptrs, base


def _assert_equals_host(outs, host, what):
    """Whole arrays, sentinels included: what the host build left untouched the device left untouched."""
    for name, ref in (("rows", host.data), ("stage", host.stage), ("count", host.count), ("flags", host.flags),
                      ("duration", host.duration)):
        assert _same_bits(outs[name].cpu().numpy(), ref), (what, name)


@pytest.mark.parametrize("N,topt,ratio,batch", SHAPES)
def test_device_equals_host_build(ctx, N, topt, ratio, batch):
    pk, x, dt, cap, need, host = _case(N, topt, ratio, batch)
    dev = ctx.timeline(pk, x, dt, cap=cap)
    assert _same_bits(dev.count, host.count) and _same_bits(dev.flags, host.flags)
    assert _same_bits(dev.duration, host.duration)
    assert np.array_equal(host.count, need)
    for p in range(batch):
        n = min(int(need[p]), cap)
        assert _same_bits(dev.data[p, :n], host.data[p, :n]) and np.array_equal(dev.stage[p, :n], host.stage[p, :n]), p
        assert np.all(dev.data[p, n:] == 0.0) and np.all(dev.stage[p, n:] == 0), p     # the caller's rows stay
        assert np.all(host.data[p, n:] == th.SENTINEL), p
    if N > 2:
        assert host.flags[0] == F["TRUNCATED"] and np.count_nonzero(host.flags & F["TRUNCATED"]) == 1
    if batch >= 3:
        assert host.flags[1] == F["NONFINITE"] and host.flags[2] == F["BAD_TIME"]
        assert host.count[1] == host.count[2] == 0
    assert np.count_nonzero(host.flags == 0) >= (1 if N > 2 and batch > 2 else 0)
    assert ctx.timeline_last_ms() > 0.0


@pytest.mark.parametrize("N,topt,ratio,batch", SHAPES)
@pytest.mark.parametrize("offset", [0, 1])
def test_device_entry_with_an_8_byte_aligned_base(ctx, N, topt, ratio, batch, offset):
    import torch
    pk, x, dt, cap, need, host = _case(N, topt, ratio, batch)
    dev = torch.device("cuda", 0)
    dev_in, ptrs = _device_inputs(torch, pk, dev)
    xd = torch.from_numpy(x).to(dev)
    outs, optr, base = _outs(torch, dev, batch, cap, offset=offset)
    assert (optr["rows"] % 16 == 8) == (offset == 1)
    stream = torch.cuda.Stream(dev)
    ctx.timeline_device(pk, ptrs, xd.data_ptr(), optr, dt, cap, stream=stream.cuda_stream)
    stream.synchronize()
    _assert_equals_host(outs, host, (N, offset))
    assert np.all(base.cpu().numpy()[:offset] == th.SENTINEL)      # the double in front of the rows
    del dev_in


def test_chained_behind_the_solve_and_the_audit_on_one_stream(ctx):
    import torch
    insts = [synth.make_instance(pid, N=10, M=3) for pid in range(4)]
    pk = _native.PackedBatch(insts)
    dev = torch.device("cuda", 0)
    dev_in, ptrs = _device_inputs(torch, pk, dev)
    B = pk.batch
    sol = {"objective": torch.zeros(B, dtype=torch.float64, device=dev),
           "status": torch.full((B,), -1, dtype=torch.int32, device=dev),
           "iterations": torch.zeros(B, dtype=torch.int32, device=dev),
           "n_factor": torch.zeros(B, dtype=torch.int32, device=dev),
           "nlp_error": torch.zeros(B, dtype=torch.float64, device=dev),
           "n_resto": torch.zeros(B, dtype=torch.int32, device=dev)}
    x = torch.zeros((B, pk.n_var), dtype=torch.float64, device=dev)
    sptr = {k: v.data_ptr() for k, v in sol.items()}
    sptr["x"] = x.data_ptr()
    aud = {"metrics": torch.zeros((B, len(_native.AUDIT_METRICS)), dtype=torch.float64, device=dev),
           "worst": torch.zeros((B, 4), dtype=torch.int32, device=dev),
           "flags": torch.zeros(B, dtype=torch.int32, device=dev)}
    dT = float(pk.params[0, _native.P_DT])
    dt, cap = dT / 4.0, 4 * pk.N + 4      # tau <= 1 (its bound): at most 4 (N - 1) regular rows and the final one
    outs, optr, _ = _outs(torch, dev, B, cap)
    stream = torch.cuda.Stream(dev)
    ctx.solve_device(pk, ptrs, sptr, stream=stream.cuda_stream)
    ctx.audit_device(pk, ptrs, x.data_ptr(), {k: v.data_ptr() for k, v in aud.items()}, stream=stream.cuda_stream,
                     substeps=4)
    ctx.timeline_device(pk, ptrs, x.data_ptr(), optr, dt, cap, stream=stream.cuda_stream)   # no host sync between
    stream.synchronize()
    assert np.all(sol["status"].cpu().numpy() >= 0)
    xh = x.cpu().numpy()
    host = th.timeline_host(pk, xh, dt, cap)
    _assert_equals_host(outs, host, "chained")
    assert np.all(host.flags == 0) and np.all(host.count >= 2)
    # the same doubles as the audit that ran in between: duration = total time, last arc = path length
    met = aud["metrics"].cpu().numpy()
    for p in range(B):
        n = int(host.count[p])
        assert _same_bits(host.duration[p], met[p, _native.AUDIT_METRICS.index("total_time")])
        assert _same_bits(host.data[p, n - 1, NCOL - 1], met[p, _native.AUDIT_METRICS.index("path_length")])
    del dev_in


def test_nullable_outputs_and_problems_beyond_a_sub_range(ctx):
    import torch
    pk, x, dt, cap, need, host = _case(7, False, 0.37, 7)
    dev = torch.device("cuda", 0)
    dev_in, ptrs = _device_inputs(torch, pk, dev)
    xd = torch.from_numpy(x).to(dev)
    stream = torch.cuda.Stream(dev)
    # stage = None, duration = None, three rows of storage beyond the batch
    extra = 3
    outs, optr, _ = _outs(torch, dev, pk.batch + extra, cap, stage=False, duration=False)
    ctx.timeline_device(pk, ptrs, xd.data_ptr(), optr, dt, cap, stream=stream.cuda_stream)
    stream.synchronize()
    for name, ref in (("rows", host.data), ("count", host.count), ("flags", host.flags)):
        got = outs[name].cpu().numpy()
        assert _same_bits(got[:pk.batch], ref), name
        assert np.all(got[pk.batch:] == (th.SENTINEL if name == "rows" else th.ISENTINEL)), name
    nostage = ctx.timeline(pk, x, dt, cap=cap, stage=False)
    assert nostage.stage is None and _same_bits(nostage.count, host.count) and "stage" not in nostage.rows(0)
    n0 = min(int(need[0]), cap)
    assert _same_bits(nostage.data[0, :n0], host.data[0, :n0])
    # a sub-range of the resident batch: problems [2, 6) into the first four output slots
    outs2, optr2, _ = _outs(torch, dev, pk.batch, cap)
    ctx.timeline_device(pk, ptrs, xd[2:].data_ptr(), optr2, dt, cap, stream=stream.cuda_stream, lo=2, hi=6)
    stream.synchronize()
    for name, ref in (("rows", host.data), ("stage", host.stage), ("count", host.count), ("flags", host.flags),
                      ("duration", host.duration)):
        got = outs2[name].cpu().numpy()
        assert _same_bits(got[:4], ref[2:6]), name
        assert np.all(got[4:] == (th.SENTINEL if got.dtype == np.float64 else th.ISENTINEL)), name
    assert host.flags[2] == F["BAD_TIME"] and host.flags[3] == 0
    del dev_in


def test_cap_none_and_api_errors(ctx):
    pk, x, dt, cap, need, host = _case(80, True, 0.25, 70)
    auto = ctx.timeline(pk, x, dt)                  # cap derived from x: nothing is truncated
    assert auto.cap >= need.max() and np.array_equal(auto.count, need)
    assert np.all(auto.flags & F["TRUNCATED"] == 0) and auto.flags[1] == F["NONFINITE"]
    for p in range(pk.batch):
        n = min(int(need[p]), cap)
        assert _same_bits(auto.data[p, :n], host.data[p, :n]), p
    assert auto.stage[0, need[0] - 1] == pk.N - 1 and _same_bits(auto.data[0, need[0] - 1, 1:6], x[0, 5 * (pk.N - 1):5 * pk.N])
    with pytest.raises(RuntimeError, match="cap"):
        ctx.timeline(pk, x, dt, cap=1)
    with pytest.raises(RuntimeError, match="dt"):
        ctx.timeline(pk, x, -1.0, cap=8)
    assert "[timeline]" in ctx.error()
    with pytest.raises(ValueError, match="dt"):
        ctx.timeline(pk, x, float("nan"))


def _optimizers(n=2):
    from headland_trajectory_planning_amd.obca_py.car_model_obca import CarModel
    from headland_trajectory_planning_amd.obca_py.optimizer import OBCAOptimizer
    out = []
    for pid in range(n):
        inst = synth.config_instance("A", pid)
        car = CarModel(max_steer=0.55, axle_to_back=0.55, width=1.48, with_aux=False)
        out.append(OBCAOptimizer(car=car, obstacles=[np.asarray(o) for o in inst["obstacles"]],
                                 init_traj=inst["init_traj"], dT=0.4, Q=np.diag([1.0, 1.0]), R=np.diag([0.1, 0.1]),
                                 W=np.diag([10.0, 0.1])))
    return out


def test_python_surface(ctx):
    from headland_trajectory_planning_amd.obca_py import optimizer as om
    opts = _optimizers()
    dt = 0.05                                       # 20 Hz
    with contextlib.redirect_stdout(io.StringIO()) as plain_out:
        plain = om.solve_batch(opts, max_cpu_time=0)
    with contextlib.redirect_stdout(io.StringIO()) as sampled_out:
        sampled = om.solve_batch(opts, max_cpu_time=0, timeline=dict(dt=dt))
    keys = {"dT", "weight", "x_opt", "y_opt", "v_opt", "theta_opt", "steer_angle_opt", "accel_opt", "steer_rate_opt",
            "mu_opt", "lambda_opt", "time_scale_opt", "slack_opt", "objective"}
    assert plain_out.getvalue() == sampled_out.getvalue()
    for (ok, sol), (ok2, sol2) in zip(plain, sampled):
        assert set(sol) == keys and set(sol2) == keys | {"timeline"} and ok == ok2
    # timeline_batch on the solution dicts == Context.timeline on the raw x == the entry solve_batch added
    pk = _native.PackedBatch([o.instance() for o in opts])
    raw = ctx.timeline(pk, ctx.solve(pk).x, dt)
    dicts = om.timeline_batch(opts, [s for _, s in plain], dt)
    single = opts[1].timeline(plain[1][1], dt)
    names = {*_native.TIMELINE_COLUMNS, "stage", "duration", "flags"}
    for k, d in enumerate(dicts):
        ref, ent = raw.as_dict(k), sampled[k][1]["timeline"]
        assert set(d) == set(ref) == set(ent) == names
        for name in (*_native.TIMELINE_COLUMNS, "stage"):
            assert _same_bits(d[name], ref[name]) and _same_bits(ent[name], ref[name]), (k, name)
        assert d["duration"] == ref["duration"] == ent["duration"] and d["flags"] == ref["flags"] == ent["flags"] == []
        n, N = len(d["t"]), opts[k].N
        assert n == raw.count[k] >= 2 and d["stage"][-1] == N - 1 and np.all(np.diff(d["t"]) > 0)
        assert np.array_equal(d["t"][:-1], dt * np.arange(n - 1)) and d["t"][-1] == d["duration"]
        assert d["x"][0] == plain[k][1]["x_opt"][0] and d["theta"][-1] == plain[k][1]["theta_opt"][-1]
    for name in (*_native.TIMELINE_COLUMNS, "stage"):
        assert _same_bits(single[name], dicts[1][name]), name

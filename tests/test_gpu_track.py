"""GPU: the tracking-rollout kernel (csrc/htp_track.hip) against the serial host build of the same core
(tests/_track_host.py), bit for bit on whole arrays, sentinels included; with max_ticks one short; with the x rows
one double off 16-byte alignment (the 16-byte loads; every output leaves through plain 8- and 4-byte stores);
chained behind a device-resident solve and audit on one stream; the nullable outputs and a sub-range; and the Python
surface (Context.track, obca_py.optimizer.track_batch / solve_batch(track=...)).  Every batch with room for them
carries a NaN problem and a BAD_TIME problem, every table with room a NaN scenario row and a diverging scenario."""
import contextlib
import io

import numpy as np
import pytest

import _track_host as tk
from headland_trajectory_planning_amd import _native, synth

pytestmark = pytest.mark.gpu

F = _native.TRACK_FLAGS
NAMES = ("metrics", "worst", "flags", "tally", "worst_scenario", "tick_clearance", "reference")


@pytest.fixture(scope="module")
def ctx():
    return _native.Context(0)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.int64), b.view(np.int64)
    return a.shape == b.shape and np.array_equal(a, b)


# N, time_opt, R, batch, M, K, dt / dT
SHAPES = [
    (2, True, 1, 3, 1, 1, 3.0),         # 63 idle lanes, dt > T: two poses
    (7, False, 65, 5, 2, 1, 0.37),      # a second pass of scenarios with one live lane, a partial tick chunk
    (80, True, 64, 8, 6, 2, 0.25),      # several tick chunks, mixed tau
    (480, True, 3, 2, 1, 1, 0.25),      # the LDS limit
]
CUTS = [(s, short) for s in SHAPES for short in (False, True) if not (short and s[0] == 2)]
_cases = {}


def _case(shape, short):
    """The batch of one shape, its max_ticks and the host build's result: computed once, shared, left unchanged."""
    key = (shape, short)
    if key not in _cases:
        N, topt, R, batch, M, K, ratio = shape
        pk, x, scen, dt = tk.track_batch(3000 + N, batch, N, topt, R, M, K, ratio)
        need = tk.needed_ticks(pk, x, dt)
        mt = int(need.max()) - (1 if short else 0)
        _cases[key] = (pk, x, scen, dt, mt, need, tk.track_host(pk, x, scen, dt, mt, rows=pk.batch + 1))
    return _cases[key]


def _device_inputs(torch, pk, dev):
    dev_in = {k: torch.from_numpy(getattr(pk, k)).to(dev) for k in pk.INPUTS if getattr(pk, k) is not None}
    return dev_in, {k: v.data_ptr() for k, v in dev_in.items()}


def _outs(torch, dev, rows, R, mt, ticks=True, reference=True):
    """Sentinel-filled device outputs."""
    def full(shape, dtype):
        return torch.full(shape, tk.SENTINEL if dtype == torch.float64 else tk.ISENTINEL, dtype=dtype, device=dev)
    t = {"metrics": full((rows, R, tk.NMET), torch.float64), "worst": full((rows, R, 3), torch.int32),
         "flags": full((rows, R), torch.int32), "tally": full((rows, len(F)), torch.int32),
         "worst_scenario": full((rows,), torch.int32),
         "tick_clearance": full((rows, mt), torch.float64) if ticks else None,
         "reference": full((rows, mt, 5), torch.float64) if reference else None}
    return t, {k: (None if v is None else v.data_ptr()) for k, v in t.items()}


def _shifted(torch, x, dev, offset):
    """x on the device, `offset` doubles into its allocation."""
    base = torch.full((x.size + offset,), tk.SENTINEL, dtype=torch.float64, device=dev)
    base[offset:] = torch.from_numpy(x.reshape(-1)).to(dev)
    return base, base.data_ptr() + 8 * offset


@pytest.mark.parametrize("shape,short", CUTS)
@pytest.mark.parametrize("offset", [0, 1])
def test_device_entry_equals_host_build(ctx, shape, short, offset):
    import torch
    pk, x, scen, dt, mt, need, host = _case(shape, short)
    dev = torch.device("cuda", 0)
    dev_in, ptrs = _device_inputs(torch, pk, dev)
    xbase, xptr = _shifted(torch, x, dev, offset)
    assert (xptr % 16 == 8) == (offset == 1)
    sd = torch.from_numpy(scen).to(dev)
    outs, optr = _outs(torch, dev, pk.batch + 1, len(scen), mt)      # one row of storage beyond the batch
    stream = torch.cuda.Stream(dev)
    ctx.track_device(pk, ptrs, xptr, sd.data_ptr(), len(scen), optr, dt, mt, stream=stream.cuda_stream)
    stream.synchronize()
    for name in NAMES:                 # whole arrays, sentinels included
        assert _same_bits(outs[name].cpu().numpy(), getattr(host, name)), (shape, short, name)
    # the shape exercises what it is there for
    N, topt, R, batch = shape[:4]
    live = [p for p in range(batch) if need[p] > 0]
    assert len(live) >= 1 and np.all(host.flags[batch:] == tk.ISENTINEL)
    if batch >= 3:
        assert np.all(host.flags[1] == F["NONFINITE"]) and np.all(host.flags[2] == F["BAD_TIME"])
    if R >= 3:
        assert host.flags[0, 1] == F["NONFINITE"] and host.flags[0, 2] & F["DIVERGED"]
        assert np.count_nonzero(host.flags[0] & F["DIVERGED"]) < R - 1
    assert bool(np.any(host.flags[0] & F["TRUNCATED"])) == short
    assert ctx.track_last_ms() > 0.0
    del dev_in, xbase


@pytest.mark.parametrize("shape,short", CUTS)
def test_host_entry_equals_host_build(ctx, shape, short):
    pk, x, scen, dt, mt, need, host = _case(shape, short)
    dev = ctx.track(pk, x, scen, dt, max_ticks=mt, reference=True)
    B = pk.batch
    for name in NAMES[:5]:
        assert _same_bits(getattr(dev, name), getattr(host, name)[:B]), (shape, short, name)
    for p in range(B):                 # the caller's entries at or beyond a problem's poses stay (NaN pre-fill)
        n = min(int(need[p]), mt)
        assert _same_bits(dev.tick_clearance[p, :n], host.tick_clearance[p, :n]), p
        assert _same_bits(dev.reference[p, :n], host.reference[p, :n]), p
        assert np.all(np.isnan(dev.tick_clearance[p, n:])) and np.all(np.isnan(dev.reference[p, n:])), p
        assert np.all(host.tick_clearance[p, n:] == tk.SENTINEL), p


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
    dt, mt = dT / 2.0, 2 * pk.N + 4        # tau <= 1 (its bound): at most 2 (N - 1) regular poses and the final one
    scen = _native.track_scenarios(9, 11)
    sd = torch.from_numpy(scen).to(dev)
    outs, optr = _outs(torch, dev, B, len(scen), mt)
    stream = torch.cuda.Stream(dev)
    ctx.solve_device(pk, ptrs, sptr, stream=stream.cuda_stream)
    ctx.audit_device(pk, ptrs, x.data_ptr(), {k: v.data_ptr() for k, v in aud.items()}, stream=stream.cuda_stream,
                     substeps=1)
    ctx.track_device(pk, ptrs, x.data_ptr(), sd.data_ptr(), len(scen), optr, dt, mt,
                     stream=stream.cuda_stream)   # no host sync between
    stream.synchronize()
    assert np.all(sol["status"].cpu().numpy() >= 0)
    host = tk.track_host(pk, x.cpu().numpy(), scen, dt, mt)
    for name in NAMES:
        assert _same_bits(outs[name].cpu().numpy(), getattr(host, name)), name
    assert not np.any(host.flags & (F["NONFINITE"] | F["BAD_TIME"] | F["TRUNCATED"] | F["BAD_POLYTOPE"]))
    # the rollout read the x the solve left on the device: ref(0) is its node 0
    assert _same_bits(outs["reference"].cpu().numpy()[:, 0], x.cpu().numpy()[:, :5])
    assert np.all(aud["flags"].cpu().numpy() & _native.AUDIT_FLAGS["NONFINITE"] == 0)
    del dev_in


def test_nullable_outputs_and_a_sub_range(ctx):
    import torch
    pk, x, scen, dt, mt, need, host = _case(SHAPES[1], False)
    dev = torch.device("cuda", 0)
    dev_in, ptrs = _device_inputs(torch, pk, dev)
    xd = torch.from_numpy(x).to(dev)
    sd = torch.from_numpy(scen).to(dev)
    stream = torch.cuda.Stream(dev)
    outs, optr = _outs(torch, dev, pk.batch, len(scen), mt, ticks=False, reference=False)
    ctx.track_device(pk, ptrs, xd.data_ptr(), sd.data_ptr(), len(scen), optr, dt, mt, stream=stream.cuda_stream)
    stream.synchronize()
    for name in NAMES[:5]:
        assert _same_bits(outs[name].cpu().numpy(), getattr(host, name)[:pk.batch]), name
    bare = ctx.track(pk, x, scen, dt, max_ticks=mt, ticks=False)
    assert bare.tick_clearance is None and bare.reference is None and "tick_clearance" not in bare.as_dict(0)
    assert _same_bits(bare.metrics, host.metrics[:pk.batch])
    # a sub-range of the resident batch: problems [2, 5) into the first three output slots
    outs2, optr2 = _outs(torch, dev, pk.batch, len(scen), mt)
    ctx.track_device(pk, ptrs, xd[2:].data_ptr(), sd.data_ptr(), len(scen), optr2, dt, mt, stream=stream.cuda_stream,
                     lo=2, hi=5)
    stream.synchronize()
    for name in NAMES:
        got = outs2[name].cpu().numpy()
        assert _same_bits(got[:3], getattr(host, name)[2:5]), name
        assert np.all(got[3:] == (tk.SENTINEL if got.dtype == np.float64 else tk.ISENTINEL)), name
    assert np.all(host.flags[2] == F["BAD_TIME"]) and host.flags[3, 0] & F["BAD_TIME"] == 0
    del dev_in


def test_api_errors_reach_the_caller(ctx):
    pk, x, scen, dt, mt, need, host = _case(SHAPES[0], False)
    with pytest.raises(RuntimeError, match="max_ticks"):
        ctx.track(pk, x, scen, dt, max_ticks=1)
    assert "[track]" in ctx.error()
    with pytest.raises(RuntimeError, match="gains"):
        ctx.track(pk, x, scen, dt, max_ticks=4, k_yaw=-1.0)
    with pytest.raises(ValueError, match="dt"):
        ctx.track(pk, x, scen, float("nan"))
    with pytest.raises(ValueError, match="scenarios"):
        ctx.track(pk, x, np.zeros((3, 5)), dt)


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
    topts = dict(R=8, seed=5, dt=0.2)
    with contextlib.redirect_stdout(io.StringIO()) as plain_out:
        plain = om.solve_batch(opts, max_cpu_time=0)
    with contextlib.redirect_stdout(io.StringIO()) as tracked_out:
        tracked = om.solve_batch(opts, max_cpu_time=0, track=topts)
    assert plain_out.getvalue() == tracked_out.getvalue()
    for (ok, sol), (ok2, sol2) in zip(plain, tracked):
        assert set(sol2) == set(sol) | {"track"} and ok == ok2
    # track_batch on the solution dicts == Context.track on the raw x == the entry solve_batch added
    pk = _native.PackedBatch([o.instance() for o in opts])
    raw = ctx.track(pk, ctx.solve(pk).x, **topts)
    dicts = om.track_batch(opts, [s for _, s in plain], **topts)
    single = opts[1].track(plain[1][1], **topts)
    names = {*_native.TRACK_METRICS, "worst", "flags", "tally", "worst_scenario", "ok", "scenarios", "tick_clearance"}
    for k, d in enumerate(dicts):
        ref, ent = raw.as_dict(k), tracked[k][1]["track"]
        assert set(d) == set(ref) == set(ent) == names
        for name in (*_native.TRACK_METRICS, "worst", "scenarios", "tick_clearance"):
            assert _same_bits(d[name], ref[name]) and _same_bits(ent[name], ref[name]), (k, name)
        assert d["flags"] == ref["flags"] == ent["flags"] and d["tally"] == ref["tally"] == ent["tally"]
        assert d["worst_scenario"] == ref["worst_scenario"] and len(d["flags"]) == 8
        assert np.array_equal(d["scenarios"], _native.track_scenarios(8, 5))
        assert sum(d["tally"].values()) == sum(len(f) for f in d["flags"])
        assert not any({"NONFINITE", "BAD_TIME", "TRUNCATED", "BAD_POLYTOPE"} & set(f) for f in d["flags"])
        assert np.all(np.isfinite(d["clearance"])) and d["worst_scenario"] == int(np.argmin(d["clearance"]))
    for name in _native.TRACK_METRICS:
        assert _same_bits(single[name], dicts[1][name]), name

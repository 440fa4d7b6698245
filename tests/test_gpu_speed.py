"""GPU: the speed-profile kernel (csrc/htp_speed.hip) against the serial host build of the same core
(tests/_speed_host.py), at the smallest shapes at which the kernel can go wrong: planner turns with cusps and dwells;
line-plus-arc paths of 2, 63, 64, 65 and 129 rows (the scans' 64-node chunk edge and the carried minimum); one mixed
launch with a NaN row, a skipped path, n_path of 0 and 1, a hop, and more paths than workgroups (the striding loop and
its scratch reuse); rows on and off, and too little row storage; the entry on resident buffers; the classic-turn
kernel and this one chained on one stream.

Bounds.  Integers (status, flags, count, active, stage) are equal exactly.  Both sides run one source with no
contraction, the same libm and IEEE sqrt and division, the minimum of the scans is exact and every sum is added in one
order, so the doubles are expected to be the same; what the test allows is the bound tests/test_speed_cpu.py derives
for two evaluations of the definition (tol_w on w and the cap, tol_t on t and T, 4 G tol_t on the rows and per-node
rates), computed here from the host build's profile.  The largest difference is printed."""
import numpy as np
import pytest

import _speed_host as sp
from headland_trajectory_planning_amd import _native, synth

pytestmark = pytest.mark.gpu
N_ = _native
LIMITS = dict(v_fwd=1.3, v_rev=0.8, acc=0.7, dec=0.9, a_lat=0.5, steer_rate=0.7)
INTS = ("status", "flags", "count", "active", "stage")
DOUBLES = ("summary", "node", "rows")


@pytest.fixture(scope="module")
def ctx():
    return _native.Context(0)


def _paths(name):
    turns = dict(sp.planner_paths())
    if name == "dubins":
        return [turns[k] for k in ("dubins_C1", "dubins_C4", "dubins_B3")], {}
    if name == "circle_back_fish_tail":      # the fish-tail's path is a Reeds-Shepp word
        return [turns["circle_back_C1"], turns["reeds_shepp_C1"]], {}
    if name == "chunk_edges":
        return [sp.line_arc(n) for n in (2, 63, 64, 65, 129)], LIMITS
    raise KeyError(name)


_host = {}


def _case(name, dt, cap_rows):
    """(packed, host build's results) of one batch: computed once, shared, left unchanged."""
    key = (name, dt, cap_rows)
    if key not in _host:
        if name == "mixed":
            good, nan = sp.line_arc(65), sp.line_arc(63)
            nan[40, 1] = np.nan
            hop = np.array([[0, 0, 0, 0, 1.0], [0.07, 0, 0, 0, 1.0]])
            paths = [good, nan, good, good[:0], good[:1], hop, sp.line_arc(129), sp.line(1.0), sp.circle(4.0, 3.0),
                     sp.line_arc(64), good, hop]
            pk = N_.SpeedPacked(paths, sp.limits(**LIMITS), dt=dt, cap_rows=cap_rows, max_groups=3,
                                status=[0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0])
        else:
            paths, lim = _paths(name)
            pk = N_.SpeedPacked(paths, sp.limits(**lim), dt=dt, cap_rows=cap_rows)
        _host[key] = (pk, sp.speed_host(pk, out=N_.SpeedResults(pk, fill=-7.25)))
    return _host[key]


def _assert_equal(dev, host, pk, name):
    for a in INTS:
        if getattr(host, a) is not None:
            assert np.array_equal(getattr(dev, a), getattr(host, a)), (name, a)
    worst = 0.0
    for b in range(pk.batch):
        if host.status[b] != N_.SPD_OK:
            for a in DOUBLES:
                if getattr(host, a) is not None:
                    assert np.array_equal(getattr(dev, a)[b], getattr(host, a)[b]), (name, a, b)   # the pre-fill
            continue
        n = int(pk.n_path[b])
        lim = pk.limits[b]
        hn, dn = host.node[b], dev.node[b]
        assert np.array_equal(dn[n:], hn[n:]), (name, b)                  # rows from n_path on: as they were
        tol_w, tol_t = sp.tolerances(hn[:n, 6], hn[:n, 2] ** 2, hn[:n, 1], host.summary[b, 1], lim[3], lim[4])
        G = max(1.0, lim[1], lim[3], lim[4], lim[6], lim[1] * float(np.max(np.abs(pk.path[b, :n, 3]))))
        tol = 4.0 * G * tol_t
        assert np.array_equal(dn[:n, 0], hn[:n, 0]) and np.array_equal(dn[:n, 4], hn[:n, 4]), (name, b)   # S, delta
        assert np.max(np.abs(dn[:n, 6] ** 2 - hn[:n, 6] ** 2)) <= tol_w, (name, b)
        assert np.max(np.abs(dn[:n, 2] ** 2 - hn[:n, 2] ** 2)) <= tol_w, (name, b)
        assert np.max(np.abs(dn[:n, 1] - hn[:n, 1])) <= tol_t, (name, b)
        assert np.max(np.abs(dn[:n] - hn[:n])) <= tol and np.max(np.abs(dev.summary[b] - host.summary[b])) <= tol, (name, b)
        worst = max(worst, float(np.max(np.abs(dn[:n] - hn[:n]))), float(np.max(np.abs(dev.summary[b] - host.summary[b]))))
        if host.rows is not None:
            m = min(int(host.count[b]), pk.cap_rows)
            assert np.array_equal(dev.rows[b, m:], host.rows[b, m:]), (name, b)
            assert np.max(np.abs(dev.rows[b, :m] - host.rows[b, :m])) <= tol, (name, b)
            worst = max(worst, float(np.max(np.abs(dev.rows[b, :m] - host.rows[b, :m]))))
    print(f"{name}: largest device-host difference of a double {worst:.3e}")


@pytest.mark.parametrize("name,dt,cap_rows", [("dubins", 0.25, 256), ("circle_back_fish_tail", 0.25, 256),
                                              ("chunk_edges", 0.1, 200), ("chunk_edges", 0.0, None),
                                              ("mixed", 0.25, 256), ("mixed", 0.25, 5)])
def test_device_equals_host_build(ctx, name, dt, cap_rows):
    pk, host = _case(name, dt, cap_rows)
    dev = ctx.speed_profile(pk, out=N_.SpeedResults(pk, fill=-7.25))
    _assert_equal(dev, host, pk, f"{name} dt={dt} cap_rows={cap_rows}")
    assert ctx.speed_profile_last_ms() > 0.0
    if name == "mixed":
        S = N_
        assert list(host.status) == [S.SPD_OK, S.SPD_BAD_INPUT, S.SPD_SKIPPED, S.SPD_BAD_INPUT, S.SPD_BAD_INPUT,
                                     S.SPD_OK] + [S.SPD_OK] * 6
        assert "HOP" in host.flag_names(5) and pk.max_groups == 3 and pk.batch == 12
        assert ("TRUNCATED" in host.flag_names(0)) == (cap_rows == 5) and host.count[0] > 5
        for g in (1, 64, 0):      # the workgroup count does not show in the result
            pk2 = N_.SpeedPacked(pk.path, pk.limits, dt=dt, cap_rows=cap_rows, max_groups=g, status=pk.path_status)
            pk2.n_path[:] = pk.n_path
            other = ctx.speed_profile(pk2, out=N_.SpeedResults(pk2, fill=-7.25))
            for a in INTS + DOUBLES:
                assert np.array_equal(getattr(other, a), getattr(dev, a)), (g, a)
    if name == "chunk_edges":
        assert list(pk.n_path) == [2, 63, 64, 65, 129] and np.all(host.status == 0)
        assert (host.rows is None) == (dt == 0.0) and (dt > 0.0 or np.all(host.count == 0))
    if name == "circle_back_fish_tail":
        assert host.summary[0, 5] > 0.0 and host.summary[0, 4] == 2 and host.summary[1, 4] >= 1    # dwell, cusps


def test_without_node_outputs_the_summary_is_the_same(ctx):
    pk, host = _case("dubins", 0.25, 256)
    dev = ctx.speed_profile(pk, nodes=False, stage=False)
    assert dev.node is None and dev.active is None and dev.stage is None
    staged = ctx.speed_profile(pk)
    for a in ("status", "flags", "count", "summary", "rows"):
        assert np.array_equal(getattr(dev, a), getattr(staged, a)), a


def test_device_entry_on_resident_buffers_equals_the_staged_entry(ctx):
    import torch
    pk, _ = _case("mixed", 0.25, 5)
    staged = ctx.speed_profile(pk, out=N_.SpeedResults(pk, fill=-7.25))
    dev = torch.device("cuda", 0)
    tin = {k: torch.from_numpy(getattr(pk, k)).to(dev) for k in ("path", "n_path", "path_status", "limits")}
    fresh = N_.SpeedResults(pk, fill=-7.25)
    names = ("status", "flags", "summary", "node", "active", "count", "rows", "stage")
    tout = {k: torch.from_numpy(getattr(fresh, k)).to(dev) for k in names}
    stream = torch.cuda.Stream(dev)
    ctx.speed_profile_device(pk, {k: v.data_ptr() for k, v in tin.items()}, {k: v.data_ptr() for k, v in tout.items()},
                             stream=stream.cuda_stream)
    stream.synchronize()
    for k, v in tout.items():
        assert np.array_equal(v.cpu().numpy(), getattr(staged, k)), k


def test_classic_turns_then_speed_profile_on_one_stream(ctx):
    import torch
    metas = [synth.config_instance(cfg, pid)["meta"] for cfg, n in (("C", 6), ("A", 2), ("B", 2)) for pid in range(n)]
    assert {m["turn"] for m in metas} == {"dubins", "circleback", "fishtail"}
    ck = N_.ClassicPacked([synth.classic_turn(m) for m in metas], cap_path=1024)
    turns = ctx.classic_turns(ck)
    pk = N_.SpeedPacked(turns, sp.limits(), dt=0.25, cap_rows=256)
    staged = ctx.speed_profile(pk, out=N_.SpeedResults(pk, fill=-7.25))
    assert np.all(staged.status == 0) and np.all(staged.summary[:, 0] > 5.0)
    dev = torch.device("cuda", 0)
    t_in = {k: torch.from_numpy(getattr(ck, k)).to(dev) for k in ("params", "desc", "poly_off", "vertices")}
    t_turn = {"status": torch.full((ck.batch,), -7, dtype=torch.int32, device=dev),
              "n_path": torch.zeros((ck.batch,), dtype=torch.int32, device=dev),
              "path": torch.zeros((ck.batch, ck.cap_path, 5), dtype=torch.float64, device=dev)}
    limits = torch.from_numpy(pk.limits).to(dev)
    fresh = N_.SpeedResults(pk, fill=-7.25)
    names = ("status", "flags", "summary", "node", "active", "count", "rows", "stage")
    tout = {k: torch.from_numpy(getattr(fresh, k)).to(dev) for k in names}
    stream = torch.cuda.Stream(dev)
    ctx.classic_turns_device(ck, {k: v.data_ptr() for k, v in t_in.items()}, {k: v.data_ptr() for k, v in t_turn.items()},
                             stream=stream.cuda_stream)
    ctx.speed_profile_device(pk, {"path": t_turn["path"].data_ptr(), "n_path": t_turn["n_path"].data_ptr(),
                                  "path_status": t_turn["status"].data_ptr(), "limits": limits.data_ptr()},
                             {k: v.data_ptr() for k, v in tout.items()}, stream=stream.cuda_stream)
    stream.synchronize()
    for k, v in tout.items():
        assert np.array_equal(v.cpu().numpy(), getattr(staged, k)), k


def test_api_errors_reach_the_caller(ctx):
    pk, _ = _case("dubins", 0.25, 256)
    bad = N_.SpeedPacked(pk.path, pk.limits, dt=0.25, cap_rows=1)
    with pytest.raises(RuntimeError, match=r"\[speed\] cap_rows"):
        ctx.speed_profile(bad)
    with pytest.raises(RuntimeError, match=r"\[speed\] dt"):
        ctx.speed_profile(N_.SpeedPacked(pk.path, pk.limits, dt=-1.0, cap_rows=8))
    with pytest.raises(RuntimeError, match=r"\[speed\] max_groups"):
        ctx.speed_profile(N_.SpeedPacked(pk.path, pk.limits, max_groups=-1))


def test_batched_python_entry(ctx):
    from headland_trajectory_planning_amd.path_planner import safety_forward_path_plan as sfp
    paths, _ = _paths("dubins")
    res = sfp.speed_profile_batch(paths, sp.Car, device=ctx, dt=0.25, cap_rows=256)
    _, host = _case("dubins", 0.25, 256)
    assert np.array_equal(res.status, host.status) and np.array_equal(res.count, host.count)
    assert np.max(np.abs(res.summary - host.summary)) <= 1e-11

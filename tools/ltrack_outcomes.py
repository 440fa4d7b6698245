#!/usr/bin/env python3
"""Solve a BASELINE config on the GPU and roll every returned trajectory twice under one table of disturbance
scenarios: under the fixed three-gain controller (htp_obca_track_batch_device) and under its own time-varying LQR
gains (htp_obca_lqr_batch_device, then htp_obca_ltrack_batch_device with the gains left on the device), all chained
behind htp_obca_solve_batch_device on one stream.  Writes profiles/ltrack_<config>.json: per law the share of
problems with a colliding or margin-losing scenario, the distribution of max |e_lat|, the saturation shares and the
DIVERGED counts; the tube check (scenarios with only lat / lon / yaw drawn at the LQR's sig0, the LQR's noise w set to
0: per problem the share of poses whose largest |e_lat| stays inside k_sigma x the tube's sigma_lat at the enclosing
node, split by whether the problem carries an AUTHORITY flag, and by each flag and its complement; beside it the same
share over the first second, the time of the first pose outside, the ratio at pose 0 (the table's largest draw) and
the share of poses whose tube is below a millimetre); and the ltrack kernel's time beside the track kernel's on the
same batch in the same run.

    python tools/ltrack_outcomes.py --config D --batch 4096            # R = 64, dt = 0.1 s, P = 2
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from headland_trajectory_planning_amd import _native  # noqa: E402

F = _native.TRACK_FLAGS
LF = _native.LQR_FLAGS
AUTHORITY = LF["AUTHORITY_ACC"] | LF["AUTHORITY_RATE"] | LF["AUTHORITY_STEER"] | LF["AUTHORITY_SPEED"]


def _dist(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    if not v.size:
        return None
    return {"n": int(v.size), "min": float(v.min()), "p10": float(np.percentile(v, 10)), "median": float(np.median(v)),
            "p90": float(np.percentile(v, 90)), "max": float(v.max()), "mean": float(v.mean())}


def _law_column(met, flags, tally, rolled):
    """The outcome of one law among the rolled problems."""
    n = int(rolled.sum())
    col = list(F)
    share = lambda name: float(np.count_nonzero(tally[rolled, col.index(name)]) / n) if n else None  # noqa: E731
    worst_lat = np.nanmax(np.where(np.isnan(met[:, :, 1]), -np.inf, met[:, :, 1]), axis=1)
    return {"share_any_scenario_collides": share("COLLISION"), "share_any_scenario_loses_margin": share("MARGIN"),
            "share_nominal_keeps_margin": float((rolled & ((flags[:, 0] & (F["COLLISION"] | F["MARGIN"])) == 0)).sum() / n)
            if n else None,
            "max_e_lat_m_per_scenario": _dist(met[rolled, :, 1].reshape(-1)),
            "max_e_lat_m_worst_scenario_per_problem": _dist(worst_lat[rolled]),
            "share_of_problems_saturating": {k: share(k) for k in ("SAT_STEER", "SAT_RATE", "SAT_ACC")},
            "share_of_rollouts_saturating": {k: float(tally[rolled, col.index(k)].sum() / (n * flags.shape[1])) if n
                                             else None for k in ("SAT_STEER", "SAT_RATE", "SAT_ACC")},
            "sat_share": _dist(met[rolled, :, 7].reshape(-1)),
            "diverged_rollouts": int(tally[rolled, col.index("DIVERGED")].sum()),
            "diverged_problems": int(np.count_nonzero(tally[rolled, col.index("DIVERGED")])),
            "worst_clearance_over_scenarios_m": _dist(np.nanmin(np.where(np.isnan(met[:, :, 0]), np.inf, met[:, :, 0]),
                                                                axis=1)[rolled])}


def _node_times(pk, xh):
    """t_i [B, N] as the kernels sum them."""
    B, N = pk.batch, pk.N
    dT = pk.params[:, _native.P_DT][:, None]
    if pk.time_opt:
        o = pk.n_var - 5 - (N - 1)          # tau sits behind X, U and the duals, in front of the five trailing doubles
        tau = xh[:, o:o + N - 1]
        h = dT * tau
    else:
        h = np.repeat(dT, N - 1, axis=1)
    return np.concatenate([np.zeros((B, 1)), np.cumsum(h, axis=1)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="D")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--scenarios", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--plant-substeps", type=int, default=2)
    ap.add_argument("--max-cpu-time", type=float, default=20.0)
    ap.add_argument("--repeat", type=int, default=3, help="launches timed per kernel (the minimum is reported too)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the generator forks a worker pool: before anything touches the GPU (bench.generate_own_slice)
    pk = bench.cached_own_slice(args.batch, args.config, 0, 1, 16, bench.DEFAULT_CACHE)

    import torch
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0, options={"max_cpu_time": args.max_cpu_time})
    dev_in = {k: torch.from_numpy(getattr(pk, k)).to(dev) for k in pk.INPUTS if getattr(pk, k) is not None}
    ptrs = {k: v.data_ptr() for k, v in dev_in.items()}
    B, N, R, P = pk.batch, pk.N, args.scenarios, args.plant_substeps
    sol = {"objective": torch.zeros(B, dtype=torch.float64, device=dev),
           "status": torch.full((B,), -1, dtype=torch.int32, device=dev),
           "iterations": torch.zeros(B, dtype=torch.int32, device=dev),
           "n_factor": torch.zeros(B, dtype=torch.int32, device=dev),
           "nlp_error": torch.zeros(B, dtype=torch.float64, device=dev),
           "n_resto": torch.zeros(B, dtype=torch.int32, device=dev)}
    x = torch.zeros((B, pk.n_var), dtype=torch.float64, device=dev)
    sptr = {k: v.data_ptr() for k, v in sol.items()}
    sptr["x"] = x.data_ptr()
    stream = torch.cuda.Stream(dev)

    def lqr_buffers():
        return {"gains": torch.full((B, N - 1, 2, 5), float("nan"), dtype=torch.float64, device=dev),
                "tube": torch.full((B, N, 7), float("nan"), dtype=torch.float64, device=dev),
                "metrics": torch.zeros((B, len(_native.LQR_METRICS)), dtype=torch.float64, device=dev),
                "worst": torch.zeros((B, 2), dtype=torch.int32, device=dev),
                "flags": torch.zeros(B, dtype=torch.int32, device=dev)}

    def roll_buffers(mt, errors):
        o = {"metrics": torch.zeros((B, R, len(_native.TRACK_METRICS)), dtype=torch.float64, device=dev),
             "worst": torch.zeros((B, R, 3), dtype=torch.int32, device=dev),
             "flags": torch.zeros((B, R), dtype=torch.int32, device=dev),
             "tally": torch.zeros((B, len(F)), dtype=torch.int32, device=dev),
             "worst_scenario": torch.zeros(B, dtype=torch.int32, device=dev),
             "tick_clearance": torch.full((B, mt), float("nan"), dtype=torch.float64, device=dev)}
        if errors:
            o["tick_error"] = torch.full((B, mt, 3), float("nan"), dtype=torch.float64, device=dev)
        return o

    with torch.cuda.stream(stream):
        lq = lqr_buffers()
    ctx.solve_device(pk, ptrs, sptr, stream=stream.cuda_stream)
    ctx.lqr_device(pk, ptrs, x.data_ptr(), {k: v.data_ptr() for k, v in lq.items()}, stream=stream.cuda_stream)
    stream.synchronize()
    solve_ms, lqr_ms = ctx.last_kernel_ms(), ctx.lqr_last_ms()
    status = sol["status"].cpu().numpy()
    xh = x.cpu().numpy()
    lflags = lq["flags"].cpu().numpy()

    scen = _native.track_scenarios(R, args.seed)
    mt = _native.track_ticks(pk, xh, args.dt)
    sd = torch.from_numpy(scen).to(dev)
    with torch.cuda.stream(stream):
        fixed, law = roll_buffers(mt, False), roll_buffers(mt, True)
    fptr, lptr = {k: v.data_ptr() for k, v in fixed.items()}, {k: v.data_ptr() for k, v in law.items()}
    track_ms, ltrack_ms = [], []
    for _ in range(max(1, args.repeat)):   # alternating, on the same batch in the same run
        ctx.track_device(pk, ptrs, x.data_ptr(), sd.data_ptr(), R, fptr, args.dt, mt, stream=stream.cuda_stream,
                         plant_substeps=P)
        ctx.ltrack_device(pk, ptrs, x.data_ptr(), lq["gains"].data_ptr(), sd.data_ptr(), R, lptr, args.dt, mt,
                          stream=stream.cuda_stream, plant_substeps=P)
        stream.synchronize()
        track_ms.append(ctx.track_last_ms())
        ltrack_ms.append(ctx.ltrack_last_ms())

    def host(o):
        return o["metrics"].cpu().numpy(), o["flags"].cpu().numpy(), o["tally"].cpu().numpy()
    fm, ff, ft = host(fixed)
    lm, lf, lt_ = host(law)
    ok = np.isin(status, (0, 1))
    reject = F["NONFINITE"] | F["BAD_TIME"] | F["BAD_POLYTOPE"]
    rolled = ok & ((ff[:, 0] & reject) == 0) & ((lf[:, 0] & reject) == 0)
    n_rolled = int(rolled.sum())
    ticks = np.count_nonzero(~np.isnan(law["tick_clearance"].cpu().numpy()), axis=1)

    # ---- both laws, problem by problem
    col = list(F)
    fc, lc = ft[:, col.index("COLLISION")] > 0, lt_[:, col.index("COLLISION")] > 0
    fmg, lmg = ft[:, col.index("MARGIN")] > 0, lt_[:, col.index("MARGIN")] > 0
    cross = {"collides_under_fixed_only": int((rolled & fc & ~lc).sum()),
             "collides_under_lqr_only": int((rolled & ~fc & lc).sum()),
             "collides_under_both": int((rolled & fc & lc).sum()),
             "loses_margin_under_fixed_only": int((rolled & fmg & ~lmg).sum()),
             "loses_margin_under_lqr_only": int((rolled & ~fmg & lmg).sum()),
             "loses_margin_under_both": int((rolled & fmg & lmg).sum())}

    # ---- the tube check: only lat / lon / yaw drawn, at the LQR's sig0; the LQR's noise off
    d = _native.LQR_DEFAULTS
    tscen = _native.track_scenarios(R, args.seed + 1, lat=d["sig0_lat"], lon=d["sig0_lon"], yaw=d["sig0_th"],
                                    steer_bias=0.0, slip=0.0, yaw_gain=0.0)
    td = torch.from_numpy(tscen).to(dev)
    with torch.cuda.stream(stream):
        lq0, tube_roll = lqr_buffers(), roll_buffers(mt, True)
    noise_off = dict(w_lon=0.0, w_lat=0.0, w_v=0.0, w_th=0.0, w_st=0.0)
    ctx.lqr_device(pk, ptrs, x.data_ptr(), {k: v.data_ptr() for k, v in lq0.items()}, stream=stream.cuda_stream,
                   **noise_off)
    ctx.ltrack_device(pk, ptrs, x.data_ptr(), lq0["gains"].data_ptr(), td.data_ptr(), R,
                      {k: v.data_ptr() for k, v in tube_roll.items()}, args.dt, mt, stream=stream.cuda_stream,
                      plant_substeps=P)
    stream.synchronize()
    tube = lq0["tube"].cpu().numpy()
    l0flags = lq0["flags"].cpu().numpy()
    terr = tube_roll["tick_error"].cpu().numpy()
    tflags = tube_roll["flags"].cpu().numpy()
    ttally = tube_roll["tally"].cpu().numpy()
    tn = _node_times(pk, xh)
    k_sigma = d["k_sigma"]
    trolled = rolled & ((tflags[:, 0] & reject) == 0) & ((l0flags & ~AUTHORITY) == 0)
    share_inside = np.full(B, np.nan)
    share_inside_1s = np.full(B, np.nan)
    worst_ratio = np.full(B, np.nan)
    ratio_pose0 = np.full(B, np.nan)
    holds_until_s = np.full(B, np.nan)
    share_tube_below_1mm = np.full(B, np.nan)
    for p in np.flatnonzero(trolled):
        npose = int(np.count_nonzero(~np.isnan(terr[p, :, 0])))
        if npose == 0:
            continue
        s = np.arange(npose, dtype=np.float64) * args.dt
        i = np.clip(np.searchsorted(tn[p, :N - 1], s, side="right") - 1, 0, N - 2)      # the enclosing node
        i = np.where(s >= tn[p, N - 1], N - 1, i)
        sig = tube[p, i, 1]
        inside = terr[p, :npose, 0] <= k_sigma * sig
        share_inside[p] = float(inside.mean())
        first_s = max(1, int(round(1.0 / args.dt)))
        share_inside_1s[p] = float(inside[:first_s].mean())
        holds_until_s[p] = float((np.argmin(inside) if not inside.all() else npose) * args.dt)   # the first pose outside
        ratio_pose0[p] = float(terr[p, 0, 0] / sig[0]) if sig[0] > 0 else np.nan
        share_tube_below_1mm[p] = float((k_sigma * sig < 1e-3).mean())
        with np.errstate(divide="ignore", invalid="ignore"):
            worst_ratio[p] = float(np.nanmax(np.where(sig > 0, terr[p, :npose, 0] / sig, np.nan)))
    flagged = trolled & ((l0flags & AUTHORITY) != 0)
    clean = trolled & ((l0flags & AUTHORITY) == 0)
    tsat = (ttally[:, col.index("SAT_STEER")] + ttally[:, col.index("SAT_RATE")] + ttally[:, col.index("SAT_ACC")]) > 0

    def tube_column(mask):
        n = int(mask.sum())
        v = share_inside[mask]
        return {"problems": n, "share_of_poses_inside": _dist(v),
                "problems_with_every_pose_inside": int(np.count_nonzero(v == 1.0)),
                "share_of_problems_with_every_pose_inside": float(np.count_nonzero(v == 1.0) / n) if n else None,
                "share_of_problems_with_a_saturating_rollout": float(tsat[mask].sum() / n) if n else None,
                "share_of_poses_inside_in_the_first_second": _dist(share_inside_1s[mask]),
                "tube_holds_until_s": _dist(holds_until_s[mask]),
                "e_lat_over_sigma_lat_at_pose_0": _dist(ratio_pose0[mask]),
                "share_of_poses_with_k_sigma_sigma_lat_below_1mm": _dist(share_tube_below_1mm[mask]),
                "worst_e_lat_over_sigma_lat": _dist(worst_ratio[mask])}
    by_flag = {}
    for name, bit in LF.items():
        if bit & AUTHORITY:
            by_flag[name] = tube_column(trolled & ((l0flags & bit) != 0))
            by_flag["without_" + name] = tube_column(trolled & ((l0flags & bit) == 0))

    k_min, y_min = min(ltrack_ms), min(track_ms)
    rec = {"config": args.config, "batch": B, "N": N, "M": pk.M, "K": pk.K, "time_opt": bool(pk.time_opt),
           "scenarios": R, "seed": args.seed, "dt": args.dt, "plant_substeps": P, "max_ticks": int(mt),
           "ticks_per_problem": _dist(ticks[rolled]),
           "ltrack_kernel_ms": ltrack_ms, "ltrack_kernel_ms_min": k_min,
           "track_kernel_ms": track_ms, "track_kernel_ms_min": y_min,
           "ltrack_over_track": k_min / y_min if y_min else None,
           "lqr_kernel_ms": lqr_ms, "solve_kernel_ms": solve_ms,
           "successful_solves": int(ok.sum()), "rolled": n_rolled,
           "lqr_flags_among_rolled": {name: int(np.count_nonzero(lflags[rolled] & bit)) for name, bit in LF.items()},
           "fixed_gains": _law_column(fm, ff, ft, rolled), "lqr": _law_column(lm, lf, lt_, rolled),
           "problem_by_problem": cross,
           "tube_check": {"scenario_sigmas": {"lat": d["sig0_lat"], "lon": d["sig0_lon"], "yaw": d["sig0_th"]},
                          "k_sigma": k_sigma, "lqr_noise": noise_off, "rolled": int(trolled.sum()),
                          "largest_draw_over_sigma": {"lat": float(np.abs(tscen[:, 0]).max() / d["sig0_lat"]),
                                                      "lon": float(np.abs(tscen[:, 1]).max() / d["sig0_lon"]),
                                                      "yaw": float(np.abs(tscen[:, 2]).max() / d["sig0_th"])},
                          "all": tube_column(trolled), "with_an_authority_flag": tube_column(flagged),
                          "without": tube_column(clean), "by_flag": by_flag},
           "fixed_gain_values": _native.TRACK_DEFAULT_GAINS, "lqr_weights": _native.LQR_DEFAULTS,
           "binary": _native.core_sha()}
    path = args.out or os.path.join(ROOT, "profiles", f"ltrack_{args.config}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()

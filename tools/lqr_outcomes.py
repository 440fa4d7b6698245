#!/usr/bin/env python3
"""Solve a BASELINE config on the GPU, audit it, sample it and compute the time-varying LQR about every returned
trajectory (htp_obca_audit_batch_device, htp_obca_timeline_batch_device and htp_obca_lqr_batch_device chained behind
htp_obca_solve_batch_device on one stream).  Writes profiles/lqr_<config>.json: the lqr kernel's time over three
launches next to the audit kernel's and the timeline kernel's of the same run, and among the successful solves the
share carrying each AUTHORITY flag, the distribution of the largest sigma_lat and of the four minimum ratios.

    python tools/lqr_outcomes.py --config D --batch 4096            # the default weights and sigmas
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


def _dist(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    if not v.size:
        return None
    return {"n": int(v.size), "min": float(v.min()), "p10": float(np.percentile(v, 10)), "median": float(np.median(v)),
            "p90": float(np.percentile(v, 90)), "max": float(v.max()), "mean": float(v.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="D")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dt", type=float, default=0.1, help="of the timeline")
    ap.add_argument("--substeps", type=int, default=4, help="of the audit")
    ap.add_argument("--max-cpu-time", type=float, default=20.0)
    ap.add_argument("--repeat", type=int, default=3, help="lqr launches timed (the minimum is reported too)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the generator forks a worker pool: before anything touches the GPU (bench.generate_own_slice)
    pk = bench.cached_own_slice(args.batch, args.config, 0, 1, 16, bench.DEFAULT_CACHE)

    import torch
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0, options={"max_cpu_time": args.max_cpu_time})
    dev_in = {k: torch.from_numpy(getattr(pk, k)).to(dev) for k in pk.INPUTS if getattr(pk, k) is not None}
    ptrs = {k: v.data_ptr() for k, v in dev_in.items()}
    B, N, S = pk.batch, pk.N, args.substeps
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
    stream = torch.cuda.Stream(dev)
    ctx.solve_device(pk, ptrs, sptr, stream=stream.cuda_stream)
    stream.synchronize()
    solve_ms = ctx.last_kernel_ms()
    status = sol["status"].cpu().numpy()
    xh = x.cpu().numpy()
    cap = _native.timeline_cap(pk, xh, args.dt)
    with torch.cuda.stream(stream):
        tml = {"rows": torch.zeros((B, cap, 10), dtype=torch.float64, device=dev),
               "count": torch.zeros(B, dtype=torch.int32, device=dev),
               "flags": torch.zeros(B, dtype=torch.int32, device=dev)}
        out = {"gains": torch.zeros((B, N - 1, 2, 5), dtype=torch.float64, device=dev),
               "tube": torch.zeros((B, N, 7), dtype=torch.float64, device=dev),
               "metrics": torch.zeros((B, len(_native.LQR_METRICS)), dtype=torch.float64, device=dev),
               "worst": torch.zeros((B, 2), dtype=torch.int32, device=dev),
               "flags": torch.zeros(B, dtype=torch.int32, device=dev)}
    optr = {k: v.data_ptr() for k, v in out.items()}
    audit_ms, timeline_ms, lqr_ms = [], [], []
    for _ in range(max(1, args.repeat)):     # the three one-wavefront-per-problem passes over the same X, U and tau
        ctx.audit_device(pk, ptrs, x.data_ptr(), {k: v.data_ptr() for k, v in aud.items()},
                         stream=stream.cuda_stream, substeps=S)
        ctx.timeline_device(pk, ptrs, x.data_ptr(), {k: v.data_ptr() for k, v in tml.items()}, args.dt, cap,
                            stream=stream.cuda_stream)
        ctx.lqr_device(pk, ptrs, x.data_ptr(), optr, stream=stream.cuda_stream)
        stream.synchronize()
        audit_ms.append(ctx.audit_last_ms())
        timeline_ms.append(ctx.timeline_last_ms())
        lqr_ms.append(ctx.lqr_last_ms())
    met = out["metrics"].cpu().numpy()
    flags = out["flags"].cpu().numpy()
    worst = out["worst"].cpu().numpy()

    F = _native.LQR_FLAGS
    M = _native.LQR_METRICS
    ok = np.isin(status, (0, 1))
    done = ok & ((flags & (F["NONFINITE"] | F["BAD_TIME"] | F["BAD_LIMIT"] | F["SINGULAR"])) == 0)
    n = int(done.sum())
    auth = ("AUTHORITY_ACC", "AUTHORITY_RATE", "AUTHORITY_STEER", "AUTHORITY_SPEED")
    any_auth = done & ((flags & 15) != 0)
    rec = {"config": args.config, "batch": B, "N": N, "M": pk.M, "K": pk.K, "time_opt": bool(pk.time_opt),
           "audit_substeps": S, "timeline_dt": args.dt, "timeline_cap": int(cap),
           "lqr_kernel_ms": lqr_ms, "lqr_kernel_ms_min": min(lqr_ms),
           "audit_kernel_ms": audit_ms, "audit_kernel_ms_min": min(audit_ms),
           "timeline_kernel_ms": timeline_ms, "timeline_kernel_ms_min": min(timeline_ms),
           "solve_kernel_ms": solve_ms,
           "lqr_over_audit": min(lqr_ms) / min(audit_ms) if min(audit_ms) else None,
           "lqr_over_timeline": min(lqr_ms) / min(timeline_ms) if min(timeline_ms) else None,
           "lqr_over_solve": min(lqr_ms) / solve_ms if solve_ms else None,
           "successful_solves": int(ok.sum()), "evaluated": n,
           "problems_with_flag_among_all": {name: int(np.count_nonzero(flags & bit)) for name, bit in F.items()},
           "share_with_flag_among_successful": {name: float(np.count_nonzero(flags[done] & F[name]) / n) if n else None
                                                for name in auth},
           "share_with_any_authority_flag": float(any_auth.sum() / n) if n else None,
           "max_sigma_lat_m": _dist(met[done, M.index("max_sigma_lat")]),
           "end_sigma_lat_m": _dist(met[done, M.index("end_sigma_lat")]),
           "max_sigma_theta_rad": _dist(met[done, M.index("max_sigma_theta")]),
           "max_gain": _dist(met[done, M.index("max_gain")]),
           "min_ratio": {name: _dist(met[done, M.index(name)]) for name in ("ratio_acc", "ratio_rate", "ratio_steer",
                                                                             "ratio_speed")},
           "stage_of_min_rate_ratio_over_N": _dist(worst[done, 1] / float(N - 1)),
           "options": _native.LQR_DEFAULTS, "binary": _native.core_sha()}
    path = args.out or os.path.join(ROOT, "profiles", f"lqr_{args.config}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()

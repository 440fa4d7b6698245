#!/usr/bin/env python3
"""Solve a BASELINE config on the GPU and sample every returned trajectory on the device at a fixed period
(htp_obca_timeline_batch_device chained behind htp_obca_solve_batch_device on one stream).  Writes
profiles/timeline_<config>.json: the timeline kernel's time over three launches, the rows and bytes it wrote,
the achieved write bandwidth, the time of a device-to-device copy of the same number of bytes on the same
machine, and the duration of the solve launch it ran behind; then the same at 4 dt and dt / 4, and a linear fit
of the kernel time over the rows written (time per row, time that does not depend on the rows).

    python tools/timeline_outcomes.py --config D --batch 4096            # dt = dT / 4
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="D")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dt", type=float, default=None, help="output period in seconds (default: dT / 4)")
    ap.add_argument("--max-cpu-time", type=float, default=20.0)
    ap.add_argument("--repeat", type=int, default=3, help="timeline launches timed (the minimum is reported too)")
    ap.add_argument("--no-sweep", dest="sweep", action="store_false",
                    help="skip the two further periods (4 dt, dt / 4) that separate the time per row from the rest")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the generator forks a worker pool: before anything touches the GPU (bench.generate_own_slice)
    pk = bench.cached_own_slice(args.batch, args.config, 0, 1, 16, bench.DEFAULT_CACHE)

    import torch
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0, options={"max_cpu_time": args.max_cpu_time})
    dev_in = {k: torch.from_numpy(getattr(pk, k)).to(dev) for k in pk.INPUTS if getattr(pk, k) is not None}
    ptrs = {k: v.data_ptr() for k, v in dev_in.items()}
    B, N = pk.batch, pk.N
    dT = float(pk.params[:, _native.P_DT].max())
    dt = args.dt if args.dt else dT / 4.0
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
    ctx.solve_device(pk, ptrs, sptr, stream=stream.cuda_stream)

    def measure(dt):
        """The timeline kernel at period dt on the solve's x (enqueued behind whatever the stream holds), and a
        plain device-to-device copy of as many bytes as it wrote, both timed over `repeat` launches."""
        cap = int((N - 1) * dT / dt * 1.01) + 4       # tau <= 1 is a bound of the NLP: nothing is truncated
        with torch.cuda.stream(stream):               # the fills are ordered before the kernel that overwrites them
            out = {"rows": torch.zeros((B, cap, len(_native.TIMELINE_COLUMNS)), dtype=torch.float64, device=dev),
                   "stage": torch.zeros((B, cap), dtype=torch.int32, device=dev),
                   "count": torch.zeros(B, dtype=torch.int32, device=dev),
                   "flags": torch.zeros(B, dtype=torch.int32, device=dev),
                   "duration": torch.zeros(B, dtype=torch.float64, device=dev)}
        optr = {k: v.data_ptr() for k, v in out.items()}
        kernel_ms = []
        for _ in range(max(1, args.repeat)):
            ctx.timeline_device(pk, ptrs, x.data_ptr(), optr, dt, cap, stream=stream.cuda_stream)
            stream.synchronize()
            kernel_ms.append(ctx.timeline_last_ms())
        count = out["count"].cpu().numpy()
        flags = out["flags"].cpu().numpy()
        rows = int(np.minimum(count, cap).sum())
        nbytes = rows * (8 * len(_native.TIMELINE_COLUMNS) + 4) + B * 16      # rows and stage; count, flags, duration
        copy_ms = []
        with torch.cuda.stream(stream):
            src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            dst.copy_(src)
            for _ in range(max(1, args.repeat)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                dst.copy_(src)
                e1.record(stream)
                e1.synchronize()
                copy_ms.append(e0.elapsed_time(e1))
        k_min, c_min = min(kernel_ms), min(copy_ms)
        return {"dt": dt, "cap": cap, "timeline_kernel_ms": kernel_ms, "timeline_kernel_ms_min": k_min,
                "rows_written": rows,
                "rows_per_problem_min_median_max": [int(count.min()), float(np.median(count)), int(count.max())],
                "bytes_written": nbytes, "write_GBps": nbytes / (k_min * 1e6) if k_min else None,
                "d2d_copy_ms": copy_ms, "d2d_copy_ms_min": c_min,
                "d2d_copy_GBps": nbytes / (c_min * 1e6) if c_min else None,
                "kernel_over_copy": k_min / c_min if c_min else None,
                "flags": {name: int(np.count_nonzero(flags & bit)) for name, bit in _native.TIMELINE_FLAGS.items()}}

    main_run = measure(dt)                             # the first launch runs behind the solve, no host sync between
    solve_ms = ctx.last_kernel_ms()
    # the same batch at four times and a quarter of the period: the time per row and the time that stays
    sweep = [measure(dt * f) for f in (4.0, 0.25)] if args.sweep else []
    pts = [main_run] + sweep
    fit = None
    if len(pts) >= 2:
        slope, fixed = np.polyfit([p["rows_written"] for p in pts], [p["timeline_kernel_ms_min"] for p in pts], 1)
        fit = {"ns_per_row": float(slope) * 1e6, "fixed_ms": float(fixed)}
    read_bytes = B * 8 * (5 * N + 2 * (N - 1) + (N - 1 if pk.time_opt else 0))
    rec = {"config": args.config, "batch": B, "N": N, "time_opt": bool(pk.time_opt), "dT": dT, **main_run,
           "bytes_read": read_bytes, "solve_kernel_ms": solve_ms,
           "kernel_over_solve": main_run["timeline_kernel_ms_min"] / solve_ms if solve_ms else None,
           "sweep": sweep, "linear_fit_over_rows": fit, "binary": _native.core_sha()}
    path = args.out or os.path.join(ROOT, "profiles", f"timeline_{args.config}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()

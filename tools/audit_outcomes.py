#!/usr/bin/env python3
"""Solve a BASELINE config on the GPU, audit every returned trajectory on the device (htp_obca_audit_batch_device
chained behind htp_obca_solve_batch_device on one stream) and tabulate the audit flags per solver status:
how many non-success outcomes are nevertheless collision-free and dynamically consistent, and how many
successes lose their margin between two nodes.  Writes profiles/audit_outcomes_<config>.json with the flag
table, the clearance quantiles per status and the two kernels' times from this run.

    python tools/audit_outcomes.py --config D --batch 4096 --substeps 4
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
    ap.add_argument("--substeps", type=int, default=4)
    ap.add_argument("--max-cpu-time", type=float, default=20.0)
    ap.add_argument("--repeat", type=int, default=3, help="audit launches timed (the minimum is reported too)")
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
    sol = {"objective": torch.zeros(B, dtype=torch.float64, device=dev),
           "status": torch.full((B,), -1, dtype=torch.int32, device=dev),
           "iterations": torch.zeros(B, dtype=torch.int32, device=dev),
           "n_factor": torch.zeros(B, dtype=torch.int32, device=dev),
           "nlp_error": torch.zeros(B, dtype=torch.float64, device=dev),
           "n_resto": torch.zeros(B, dtype=torch.int32, device=dev)}
    x = torch.zeros((B, pk.n_var), dtype=torch.float64, device=dev)
    sptr = {k: v.data_ptr() for k, v in sol.items()}
    sptr["x"] = x.data_ptr()
    out = {"metrics": torch.zeros((B, len(_native.AUDIT_METRICS)), dtype=torch.float64, device=dev),
           "worst": torch.zeros((B, 4), dtype=torch.int32, device=dev),
           "flags": torch.zeros(B, dtype=torch.int32, device=dev),
           "stage_clearance": torch.zeros((B, N), dtype=torch.float64, device=dev)}
    optr = {k: v.data_ptr() for k, v in out.items()}
    stream = torch.cuda.Stream(dev)
    ctx.solve_device(pk, ptrs, sptr, stream=stream.cuda_stream)
    ctx.audit_device(pk, ptrs, x.data_ptr(), optr, stream=stream.cuda_stream, substeps=args.substeps)
    stream.synchronize()
    solve_ms = ctx.last_kernel_ms()
    audit_ms = [ctx.audit_last_ms()]
    for _ in range(max(0, args.repeat - 1)):
        ctx.audit_device(pk, ptrs, x.data_ptr(), optr, stream=stream.cuda_stream, substeps=args.substeps)
        stream.synchronize()
        audit_ms.append(ctx.audit_last_ms())
    nodes_only = {k: torch.zeros_like(v) for k, v in out.items()}
    ctx.audit_device(pk, ptrs, x.data_ptr(), {k: v.data_ptr() for k, v in nodes_only.items()},
                     stream=stream.cuda_stream, substeps=1)
    stream.synchronize()
    nodes_ms = ctx.audit_last_ms()

    status = sol["status"].cpu().numpy()
    flags = out["flags"].cpu().numpy()
    metrics = out["metrics"].cpu().numpy()
    dmin = pk.params[:, _native.P_DMIN]
    table = {}
    for st in sorted(set(int(s) for s in status)):
        sel = status == st
        row = {"count": int(sel.sum()), "clean": int(np.count_nonzero(flags[sel] == 0))}
        for name, bit in _native.AUDIT_FLAGS.items():
            row[name] = int(np.count_nonzero(flags[sel] & bit))
        clr, node = metrics[sel, 0], metrics[sel, 1]
        fin = np.isfinite(clr)
        if fin.any():
            row["clearance_min_median_max"] = [float(v) for v in (clr[fin].min(), np.median(clr[fin]), clr[fin].max())]
            # the nodes keep the margin, the poses between them do not
            row["margin_lost_between_nodes"] = int(np.count_nonzero(
                (node[fin] >= dmin[sel][fin] - 1e-4) & (clr[fin] < dmin[sel][fin] - 1e-4)))
            row["largest_node_minus_dense_clearance"] = float(np.max(node[fin] - clr[fin]))
        row["dyn_defect_max"] = float(np.nanmax(metrics[sel, 2]))
        table[f"{st} {_native.STATUS_STR.get(st, '?')}"] = row
    rec = {"config": args.config, "batch": B, "N": N, "M": pk.M, "K": pk.K, "substeps": args.substeps,
           "tolerances": {"margin_tol": 1e-4, "dyn_tol": 1e-4, "bound_tol": 1e-4, "term_tol": 0.0},
           "solve_kernel_ms": solve_ms, "audit_kernel_ms": audit_ms, "audit_kernel_ms_min": min(audit_ms),
           "audit_nodes_only_ms": nodes_ms, "audit_over_solve": min(audit_ms) / solve_ms if solve_ms else None,
           "work_items_per_problem": N * args.substeps * pk.M * pk.K, "per_status": table,
           "binary": _native.core_sha()}
    path = args.out or os.path.join(ROOT, "profiles", f"audit_outcomes_{args.config}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()

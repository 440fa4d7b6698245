#!/usr/bin/env python3
"""Solve a BASELINE config on the GPU, audit it, and run the repair loop step by step on the device (pack,
htp_obca_solve_batch_device, htp_obca_audit_batch_device, merge: the steps of htp_obca_repair_batch_device, taken
apart here so that each can be timed).  Writes profiles/repair_<config>.json: per round the numbers selected,
adopted and clean, the iterations and the launch time of the re-solve beside those of the first solve, the pack
and merge kernel times beside a plain device copy (torch.Tensor.copy_) of the same bytes on the same stream; the
states at the end, the largest margin used and the objective ratio of the repaired turns.  The library's own loop
is then run on a copy of the first solve and must end in the same state.

    python tools/repair_outcomes.py --config D --batch 4096
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

S = _native.REPAIR_STATES
CLR = _native.AUDIT_METRICS.index("clearance")
FLAGGED = _native.AUDIT_FLAGS["COLLISION"] | _native.AUDIT_FLAGS["MARGIN"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="D")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pad", type=float, default=0.01)
    ap.add_argument("--max-raise", type=float, default=0.5)
    ap.add_argument("--substeps", type=int, default=4)
    ap.add_argument("--max-cpu-time", type=float, default=20.0)
    ap.add_argument("--repeat", type=int, default=3, help="copies timed (the minimum is reported)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    # the generator forks a worker pool: before anything touches the GPU (bench.generate_own_slice)
    pk = bench.cached_own_slice(args.batch, args.config, 0, 1, 16, bench.DEFAULT_CACHE)

    import torch
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0, options={"max_cpu_time": args.max_cpu_time})
    stream = torch.cuda.Stream(dev)
    B, N, nv = pk.batch, pk.N, pk.n_var
    f64, i32 = torch.float64, torch.int32

    def zeros(shape, dtype):
        with torch.cuda.stream(stream):
            return torch.zeros(shape, dtype=dtype, device=dev)

    def result(rows):
        t = {"x": zeros((rows, nv), f64), "objective": zeros(rows, f64), "status": zeros(rows, i32),
             "iterations": zeros(rows, i32), "n_factor": zeros(rows, i32), "nlp_error": zeros(rows, f64),
             "n_resto": zeros(rows, i32)}
        return t, {k: v.data_ptr() for k, v in t.items()}

    def audit(rows):
        t = {"metrics": zeros((rows, len(_native.AUDIT_METRICS)), f64), "worst": zeros((rows, 4), i32),
             "flags": zeros(rows, i32), "stage_clearance": zeros((rows, N), f64)}
        return t, {k: v.data_ptr() for k, v in t.items()}

    def copy_ms(nbytes):
        """A plain device copy of nbytes on the stream: the yardstick of pack and merge."""
        with torch.cuda.stream(stream):
            src = torch.zeros(max(1, nbytes), dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            dst.copy_(src)
            ms = []
            for _ in range(max(1, args.repeat)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                dst.copy_(src)
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        return min(ms)

    dev_in = {k: torch.from_numpy(getattr(pk, k)).to(dev) for k in pk.INPUTS if getattr(pk, k) is not None}
    ptrs = {k: v.data_ptr() for k, v in dev_in.items()}
    aopts = dict(substeps=args.substeps)
    out, optr = result(B)
    aud, aptr = audit(B)
    ctx.solve_device(pk, ptrs, optr, stream=stream.cuda_stream)
    ctx.audit_device(pk, ptrs, out["x"].data_ptr(), aptr, stream=stream.cuda_stream, **aopts)
    stream.synchronize()
    first_ms = ctx.last_kernel_ms()
    first = {k: v.clone() for k, v in out.items()}
    st0, it0, obj0 = (out[k].cpu().numpy().copy() for k in ("status", "iterations", "objective"))
    fl0, clr0 = aud["flags"].cpu().numpy().copy(), aud["metrics"][:, CLR].cpu().numpy().copy()
    ok0 = np.isin(st0, (0, 1))

    state = {n: zeros(B, f64 if n == "dmin_used" else i32) for n in _native.REPAIR_STATE_ARRAYS}
    sptr = {k: v.data_ptr() for k, v in state.items()}
    TEo, TEb = int(pk.obs_edges.sum()), int(pk.body_edges.sum())
    dims = dict(traj=5 * N, obs_A=2 * TEo, obs_b=TEo, body_G=2 * TEb, body_g=TEb, params=_native.NPARAM,
                params_audit=_native.NPARAM, init_control=2 * (N - 1), init_mu=N * pk.mu_count,
                init_lambda=N * pk.lam_count)
    slot_doubles = sum(dims.values())
    rounds = []
    cap = B
    for r in range(args.rounds):
        slots = {"count": zeros(1, i32), "index": zeros(cap, i32), "adopted": zeros(cap, i32)}
        slots.update({n: zeros((cap, d), f64) for n, d in dims.items()})
        slptr = {k: v.data_ptr() for k, v in slots.items()}
        # on a copy of the state: the first launch of a kernel loads its code, and a pack with one slot of
        # storage is the scan plus a single slot's copy, which splits the pack time into its two kernels
        trial = {k: v.clone() for k, v in state.items()}
        ctx.repair_pack_device(pk, ptrs, {k: optr[k] for k in ("x", "status")},
                               {k: aptr[k] for k in ("metrics", "flags")}, {k: v.data_ptr() for k, v in trial.items()},
                               slptr, 1, pad=args.pad, max_raise=args.max_raise, stream=stream.cuda_stream)
        stream.synchronize()
        ctx.repair_pack_device(pk, ptrs, {k: optr[k] for k in ("x", "status")},
                               {k: aptr[k] for k in ("metrics", "flags")}, {k: v.data_ptr() for k, v in trial.items()},
                               slptr, 1, pad=args.pad, max_raise=args.max_raise, stream=stream.cuda_stream)
        stream.synchronize()
        scan_ms = ctx.repair_last_ms()[0]
        ctx.repair_pack_device(pk, ptrs, {k: optr[k] for k in ("x", "status")},
                               {k: aptr[k] for k in ("metrics", "flags")}, sptr, slptr, cap, pad=args.pad,
                               max_raise=args.max_raise, stream=stream.cuda_stream)
        stream.synchronize()
        pack_ms = ctx.repair_last_ms()[0]
        n = int(slots["count"].cpu().numpy()[0])
        if n == 0:
            rounds.append({"round": r, "selected": 0})
            break
        sub = _native.PackedBatch.__new__(_native.PackedBatch)
        sub.__dict__.update(pk.__dict__)
        sub.batch = n
        again = {k: slptr[k] for k in ("traj", "obs_A", "obs_b", "body_G", "body_g", "params", "init_control",
                                      "init_mu", "init_lambda")}
        judged = dict(again, params=slptr["params_audit"])
        re, rptr = result(n)
        ra, raptr = audit(n)
        tally = zeros(3, i32)
        ctx.solve_device(sub, again, rptr, stream=stream.cuda_stream)
        ctx.audit_device(sub, judged, re["x"].data_ptr(), raptr, stream=stream.cuda_stream, **aopts)
        stream.synchronize()
        solve_ms = ctx.last_kernel_ms()
        ctx.repair_merge_device(pk, ptrs, slptr, cap, rptr, raptr, optr, aptr, sptr, tally.data_ptr(),
                                stream=stream.cuda_stream)
        stream.synchronize()
        merge_ms = ctx.repair_last_ms()[1]
        t = tally.cpu().numpy()
        idx = slots["index"][:n].cpu().numpy()
        it = re["iterations"].cpu().numpy()
        rst = re["status"].cpu().numpy()
        pack_bytes = 2 * 8 * n * slot_doubles                    # read and written
        merge_bytes = 2 * int(t[1]) * (8 * nv + 8 * (len(_native.AUDIT_METRICS) + N) + 64)
        pc, mc = copy_ms(pack_bytes // 2), copy_ms(merge_bytes // 2)
        rounds.append({"round": r, "selected": int(t[0]), "adopted": int(t[1]), "clean": int(t[2]),
                       "resolve_status": {_native.STATUS_STR[int(s)]: int(np.count_nonzero(rst == s)) for s in np.unique(rst)},
                       "resolve_iterations_mean": float(it.mean()), "first_iterations_mean_same_problems": float(it0[idx].mean()),
                       "resolve_launch_ms": solve_ms, "first_solve_launch_ms": first_ms,
                       "margin_max": float(slots["params"][:n, _native.P_DMIN].max().item()),
                       "pack_kernel_ms": pack_ms, "pack_with_one_slot_ms": scan_ms, "pack_bytes_moved": pack_bytes, "pack_copy_ms": pc,
                       "pack_over_copy": pack_ms / pc if pc else None,
                       "merge_kernel_ms": merge_ms, "merge_bytes_moved": merge_bytes, "merge_copy_ms": mc,
                       "merge_over_copy": merge_ms / mc if mc else None})
        cap = n                                                  # the candidates of a round are among the last one's

    stf = state["state"].cpu().numpy()
    dm = state["dmin_used"].cpu().numpy()
    ru = state["rounds_used"].cpu().numpy()
    objf, flf = out["objective"].cpu().numpy(), aud["flags"].cpu().numpy()
    repaired = (stf & S["REPAIRED"]) != 0
    ratio = objf[repaired] / obj0[repaired] if repaired.any() else np.zeros(0)
    flagged0 = ok0 & ((fl0 & FLAGGED) != 0)
    # the library's own loop from the same first solve
    for k in out:
        out[k].copy_(first[k])
    lstate = {n: zeros(B, f64 if n == "dmin_used" else i32) for n in _native.REPAIR_STATE_ARRAYS}
    lrc = zeros((_native.REPAIR_MAX_ROUNDS, 3), i32)
    laud, laptr = audit(B)
    stream.synchronize()
    torch.cuda.synchronize()
    import time
    t0 = time.perf_counter()
    ctx.repair_device(pk, ptrs, optr, laptr, {k: v.data_ptr() for k, v in lstate.items()}, lrc.data_ptr(),
                      rounds=args.rounds, pad=args.pad, max_raise=args.max_raise, stream=stream.cuda_stream, **aopts)
    stream.synchronize()
    loop_wall_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(lstate["state"].cpu().numpy(), stf) and np.array_equal(laud["flags"].cpu().numpy(), flf)
                and np.array_equal(out["objective"].cpu().numpy(), objf))
    rec = {"config": args.config, "batch": B, "N": N, "opts": {"rounds": args.rounds, "pad": args.pad,
                                                               "max_raise": args.max_raise, **aopts},
           "first_solve_launch_ms": first_ms, "first_iterations_mean": float(it0[ok0].mean()),
           "first_successes": int(ok0.sum()), "first_flagged_successes": int(flagged0.sum()),
           "first_collisions_among_successes": int((ok0 & ((fl0 & 1) != 0)).sum()),
           "rounds": rounds,
           "states_at_the_end": {n: int(np.count_nonzero(stf & b)) for n, b in S.items()},
           "still_flagged_successes": int((ok0 & ((flf & FLAGGED) != 0)).sum()),
           "collisions_left_among_successes": int((ok0 & ((flf & 1) != 0)).sum()),
           "margin_used_max": float(dm[ru > 0].max()) if (ru > 0).any() else None,
           "objective_ratio_repaired_median": float(np.median(ratio)) if ratio.size else None,
           "objective_ratio_repaired_max": float(ratio.max()) if ratio.size else None,
           "clearance_never_decreased": bool(np.all(aud["metrics"][:, CLR].cpu().numpy()[ok0] >= clr0[ok0])),
           "library_loop_wall_ms": loop_wall_ms, "library_loop_equals_the_steps": same,
           "library_loop_round_counts": lrc.cpu().numpy()[:args.rounds].tolist(), "binary": _native.core_sha()}
    path = args.out or os.path.join(ROOT, "profiles", f"repair_{args.config}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Run the sampled exit / entry pose search (htp_classic_sample_batch_device) over the orchards of a BASELINE config at
the reference's default accuracy = 0.2, once per type (Dubins, Reeds-Shepp, circle-back), and write
profiles/sample_outcomes_<config>.json: the kernels' time (htp_classic_sample_last_ms: candidate kernels + winner
kernel) over a warm-up and `--repeat` launches, candidates per turn, the share of feasible candidates, the statuses,
and -- on a subset of the turns -- how often the sampled winner differs from the first-clearing pose of
get_start_end_pose_for_dubins / _for_reeds_shepp and how much boundary distance it gains over that pose (the
first-clearing pose pair is scored by the same kernel, as a one-candidate turn).  The baseline is the host numpy
restatement (path_planner/safety_forward_path_plan.py, candidate by candidate) timed on the CPU over candidates drawn
from the same turns; the reference itself needs shapely and pydubins.

Two phases, so that the GPU is held only for the launches: everything the CPU can do (scenes, x lists, first-clearing
poses, the host baseline) is prepared first and may be kept in a file.

    python tools/sample_outcomes.py --config C --batch 4096 --prepare-only --prepared build/sample_prepared_C.pkl
    python tools/sample_outcomes.py --config C --batch 4096 --prepared build/sample_prepared_C.pkl
"""
import argparse
import contextlib
import io
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from headland_trajectory_planning_amd import _native, synth  # noqa: E402
from headland_trajectory_planning_amd.path_planner import safety_forward_path_plan as sfp  # noqa: E402
from headland_trajectory_planning_amd.path_planner.car_model import CarModel  # noqa: E402

TYPES = ("dubins", "reeds_shepp", "circle_back")
FIRST_CLEARING = {"dubins": sfp.get_start_end_pose_for_dubins, "reeds_shepp": sfp.get_start_end_pose_for_reeds_shepp}


class _HostWords:
    """calc_all_paths through the CPU build of csrc/rs_core.h (libhtp_cpu.so): the host planners' words without the GPU."""
    calc_all_paths = staticmethod(synth.host_rs_all_paths)


@contextlib.contextmanager
def _host_words():
    saved = sfp.rs_curves
    sfp.rs_curves = _HostWords
    try:
        yield
    finally:
        sfp.rs_curves = saved


def _dist(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    if not v.size:
        return None
    return {"n": int(v.size), "min": float(v.min()), "p10": float(np.percentile(v, 10)), "median": float(np.median(v)),
            "p90": float(np.percentile(v, 90)), "max": float(v.max()), "mean": float(v.mean())}


def _request(meta, implement):
    rows, env = synth._orchard_env(meta)
    veh, feat = synth.VEHICLE, synth.IMPLEMENTS[implement]
    car = CarModel(max_steer=veh["max_steer"], wheel_base=veh["wheelbase"], axle_to_front=veh["axle_to_front"],
                   axle_to_back=veh["axle_to_back"], width=veh["width"],
                   aux_poly_features=[feat] if feat is not None else [], with_aux=feat is not None)
    return dict(map_tree_rows=rows, start_row_id=int(meta["s_row"]), end_row_id=int(meta["e_row"]), car=car,
                config_env=env)


def _host_candidate(req, turn, sx, ex):
    """One candidate through the host planners: the body of the reference's loops -> score or None."""
    car, env = req["car"], req["config_env"]
    s = np.array([sx, turn["start"][1], turn["start"][2]])
    e = np.array([ex, turn["end"][1], turn["end"][2]])
    r = 1.0 / car.curvature
    if turn["type"] == "reeds_shepp":
        paths = sfp.get_all_reeds_shepp_paths_full(s, e, r)
    elif turn["type"] == "dubins":
        paths = [sfp.get_dubins_path_full(s, e, r)]
    else:
        paths = [sfp.get_circle_back_path_full(s, e, r, car, turn["side"])]
    best = None
    for p in paths:
        if env.check_path_feasibility(car, p[:, :3], boundary_check=False, aux_check=True):
            d = env.get_min_distance_to_boundary(car, p[:, :3], with_aux=True)
            best = d if best is None or d > best else best
    return best


def prepare(args):
    """Everything that needs no GPU: the turns of every type, the first-clearing poses of a subset, the host baseline."""
    own = bench.cached_own_slice(args.batch, args.config, 0, 1, 16, bench.DEFAULT_CACHE)
    metas = own.metas
    implement = synth.CONFIGS[args.config][3]
    reqs = [_request(m, implement) for m in metas]
    out = {"config": args.config, "batch": len(metas), "accuracy": args.accuracy, "turns": {}, "first": {}, "host": {}}
    rng = np.random.default_rng(0)
    subset = np.sort(rng.choice(len(metas), size=min(args.subset, len(metas)), replace=False))
    for typ in TYPES:
        turns = [sfp.sample_turn(**r, type=typ, accuracy=args.accuracy) for r in reqs]
        for t in turns:     # what travels: arrays and numbers only
            t["start"], t["end"] = np.asarray(t["start"], dtype=np.float64), np.asarray(t["end"], dtype=np.float64)
        out["turns"][typ] = turns
        if typ in FIRST_CLEARING:   # the poses the planners use today: the first offsets whose turn-out arcs clear the rows
            first = {}
            t0 = time.perf_counter()
            for k in subset:
                with contextlib.redirect_stdout(io.StringIO()):
                    s, e, _, _ = FIRST_CLEARING[typ](reqs[k]["map_tree_rows"], reqs[k]["start_row_id"],
                                                     reqs[k]["end_row_id"], reqs[k]["car"], reqs[k]["config_env"])
                first[int(k)] = (float(s[0]), float(e[0]))
            out["first"][typ] = first
            print(f"[prepare] {typ}: first-clearing poses of {len(first)} turns in {time.perf_counter() - t0:.1f} s", flush=True)
        # host baseline: candidates drawn evenly from the subset's turns, timed one by one
        n_time = args.host_candidates[typ]
        picks, t_sum = [], 0.0
        with _host_words(), contextlib.redirect_stdout(io.StringIO()):
            for q in range(n_time):
                k = int(subset[q % len(subset)])
                t = turns[k]
                i = int(rng.integers(0, len(t["start_x"])))
                j = int(rng.integers(0, len(t["end_x"])))
                t0 = time.perf_counter()
                d = _host_candidate(reqs[k], t, t["start_x"][i], t["end_x"][j])
                t_sum += time.perf_counter() - t0
                picks.append((k, i, j, d))
        out["host"][typ] = {"candidates_timed": n_time, "seconds": t_sum, "picks": picks}
        print(f"[prepare] {typ}: host restatement {t_sum / max(n_time, 1) * 1e3:.1f} ms per candidate", flush=True)
    out["subset"] = [int(k) for k in subset]
    return out


def run(prep, args):
    import torch
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    stream = torch.cuda.Stream(dev)
    names = ("params", "desc", "poly_off", "vertices", "start_x", "end_x", "n_start", "n_end")

    def launch(pk, repeat):
        tin = {k: torch.from_numpy(getattr(pk, k)).to(dev) for k in names}
        B, C = pk.batch, pk.cap_cand
        tout = {"status": torch.zeros(B, dtype=torch.int32, device=dev),
                "winner": torch.zeros((B, 2), dtype=torch.int32, device=dev),
                "poses": torch.zeros((B, _native.SMP_NPOSE), dtype=torch.float64, device=dev),
                "score": torch.zeros(B, dtype=torch.float64, device=dev),
                "n_feasible": torch.zeros(B, dtype=torch.int32, device=dev),
                "cand_score": torch.zeros((B, C), dtype=torch.float64, device=dev),
                "cand_status": torch.zeros((B, C), dtype=torch.int32, device=dev)}
        ms = []
        for _ in range(1 + repeat):          # the first launch warms up (allocations, code load) and is not reported
            ctx.classic_sample_device(pk, {k: v.data_ptr() for k, v in tin.items()},
                                      {k: v.data_ptr() for k, v in tout.items()}, stream=stream.cuda_stream)
            stream.synchronize()
            ms.append(ctx.classic_sample_last_ms())
        return {k: v.cpu().numpy() for k, v in tout.items()}, ms[0], ms[1:]

    report = {"config": prep["config"], "batch": prep["batch"], "accuracy": prep["accuracy"],
              "device": torch.cuda.get_device_name(0), "cap_samples": args.cap_samples, "types": {}}
    for typ in TYPES:
        turns = prep["turns"][typ]
        pk = _native.SamplePacked(turns, cap_samples=args.cap_samples)
        res, warm, ms = launch(pk, args.repeat)
        n_cand = pk.n_start.astype(np.int64) * pk.n_end
        used = res["cand_status"] != _native.SMP_C_UNUSED
        hist = {_native.SMP_C_STATUS[s]: int(np.count_nonzero(res["cand_status"][used] == s)) for s in range(5)}
        total = int(used.sum())
        host = prep["host"][typ]
        per_cand = host["seconds"] / max(host["candidates_timed"], 1)
        agree = [abs(d - res["cand_score"][k, i * pk.n_end[k] + j]) if d is not None else
                 float(res["cand_status"][k, i * pk.n_end[k] + j] == _native.SMP_C_FEASIBLE)
                 for k, i, j, d in host["picks"]]
        col = {"kernel_ms": {"warm_up": warm, "launches": ms, "min": min(ms), "median": float(np.median(ms))},
               "turn_status": {_native.SMP_STATUS[s]: int(np.count_nonzero(res["status"] == s)) for s in range(4)},
               "candidates_total": total, "candidates_per_turn": _dist(n_cand), "table_slots_per_turn": int(pk.cap_cand),
               "candidate_status": hist, "share_feasible": hist["feasible"] / max(total, 1),
               "feasible_per_turn": _dist(res["n_feasible"]),
               "winner_score_m": _dist(res["score"]),
               "candidates_per_second": total / (min(ms) * 1e-3),
               "host_restatement": {"candidates_timed": host["candidates_timed"], "ms_per_candidate": per_cand * 1e3,
                                    "estimated_s_for_the_batch_one_core": per_cand * total,
                                    "largest_difference_to_the_device_on_the_timed_candidates": float(max(agree)) if agree else None},
               "speedup_over_host_one_core": per_cand * total / (min(ms) * 1e-3)}
        if typ in prep["first"]:      # the first-clearing pose pairs, each scored by the kernel as a one-candidate turn
            first = prep["first"][typ]
            ks = sorted(first)
            ones = [dict(turns[k], start_x=np.array([first[k][0]]), end_x=np.array([first[k][1]])) for k in ks]
            r1, _, _ = launch(_native.SamplePacked(ones, cap_samples=args.cap_samples), 0)
            differs, gain, rescued, lost = 0, [], 0, 0
            for q, k in enumerate(ks):
                w = res["poses"][k]
                has_w, has_f = res["winner"][k, 0] >= 0, r1["n_feasible"][q] > 0
                if has_w and (abs(w[0] - first[k][0]) > 1e-9 or abs(w[3] - first[k][1]) > 1e-9):
                    differs += 1
                if has_w and has_f:
                    gain.append(res["score"][k] - r1["score"][q])
                rescued += int(has_w and not has_f)
                lost += int(has_f and not has_w)
            col["against_first_clearing_pose"] = {
                "turns_compared": len(ks), "share_winner_differs": differs / max(len(ks), 1),
                "first_clearing_pose_feasible_share": float(np.mean(r1["n_feasible"] > 0)),
                "sampled_has_winner_where_first_clearing_is_infeasible": rescued,
                "first_clearing_feasible_where_sampling_finds_none": lost,
                "boundary_distance_gain_m": _dist(gain)}
        report["types"][typ] = col
        print(f"[sample] {typ}: {total} candidates, {col['share_feasible']:.3f} feasible, kernel {min(ms):.2f} ms "
              f"(median {np.median(ms):.2f}), host {per_cand * 1e3:.1f} ms per candidate", flush=True)
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--accuracy", type=float, default=0.2)
    ap.add_argument("--subset", type=int, default=256, help="turns compared with the first-clearing poses")
    ap.add_argument("--cap-samples", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=3, help="timed launches per type after one warm-up launch")
    ap.add_argument("--host-dubins", type=int, default=200)
    ap.add_argument("--host-reeds-shepp", type=int, default=40)
    ap.add_argument("--host-circle-back", type=int, default=200)
    ap.add_argument("--prepared", default=None, help="file that keeps the CPU phase (read when present, else written)")
    ap.add_argument("--prepare-only", action="store_true")
    ap.add_argument("--limit", type=int, default=None, help="run only the first LIMIT turns of the prepared batch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.host_candidates = {"dubins": args.host_dubins, "reeds_shepp": args.host_reeds_shepp,
                            "circle_back": args.host_circle_back}
    if args.prepared and os.path.exists(args.prepared):
        with open(args.prepared, "rb") as fh:
            prep = pickle.load(fh)
        assert prep["config"] == args.config and prep["batch"] == args.batch and prep["accuracy"] == args.accuracy
    else:   # the generator forks a worker pool: before anything touches the GPU
        prep = prepare(args)
        if args.prepared:
            os.makedirs(os.path.dirname(os.path.abspath(args.prepared)), exist_ok=True)
            with open(args.prepared, "wb") as fh:
                pickle.dump(prep, fh)
    if args.prepare_only:
        return
    if args.limit is not None and args.limit < prep["batch"]:
        n = args.limit
        prep = dict(prep, batch=n, turns={t: v[:n] for t, v in prep["turns"].items()},
                    first={t: {k: p for k, p in v.items() if k < n} for t, v in prep["first"].items()},
                    host={t: dict(v, picks=[q for q in v["picks"] if q[0] < n]) for t, v in prep["host"].items()})
    report = run(prep, args)
    out = args.out or os.path.join(ROOT, "profiles", f"sample_outcomes_{args.config}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("[sample] wrote", out)


if __name__ == "__main__":
    main()

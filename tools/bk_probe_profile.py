"""Figures of the small-factorization probe (csrc/bk_probe.h) on the seeded blocks of tests/_bk_cases.py, written as
JSON: per block size the case counts per family, LAPACK's largest backward error eta per family and the bounds
derived from it; per (variant, n, lane stride) the form's largest eta, reconstruction error and forward error
against mpmath.lu_solve per family, and the 2 x 2 pivots and interchanges its pivot vectors hold.

  python tools/bk_probe_profile.py --cpu  [--out profiles/bk_probe_cpu.json]   both host builds
  python tools/bk_probe_profile.py --gpu  [--out profiles/bk_probe_gpu.json]   the device, and its bit comparison
                                                                               with the contracting host build
"""
import argparse
import collections
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import _bk_cases as bc  # noqa: E402

HOST_RUNS = [(0, 10, 1), (0, 4, 1), (0, 8, 1), (1, 4, 1), (1, 8, 1), (1, 10, 1), (1, 18, 1), (2, 10, 1), (3, 10, 1),
             (3, 18, 1), (3, 10, 64), (4, 10, 1), (4, 18, 1), (4, 10, 64), (5, 10, 1), (5, 10, 64)]
DEVICE_RUNS = [(0, 10, 1), (0, 4, 1), (0, 8, 1), (1, 4, 1), (1, 8, 1), (1, 10, 1), (1, 18, 1), (2, 10, 1), (3, 10, 64),
               (3, 10, 1), (3, 18, 1), (4, 10, 64), (4, 10, 1), (4, 18, 1), (5, 10, 64)]
CHOL_RUNS = [(6, 1, 1), (6, 2, 1), (6, 3, 1), (7, 5, 1)]


def _sci(d):
    return {k: float("%.3e" % v) for k, v in d.items()}


def cases_summary():
    out = {}
    for n in bc.BK_SIZES:
        cs = bc.bk_cases(n)
        bc.bk_reference(n)
        fam = collections.Counter(cs.kinds)
        sub = collections.Counter(f"{k}{s}" for k, s in zip(cs.kinds, cs.subs) if k in "deg")
        out[str(n)] = {"blocks": bc.N_BLOCKS, "per_family": dict(sorted(fam.items())),
                       "distinct_blocks": len({cs.K0[i].tobytes() for i in range(bc.N_BLOCKS)}),
                       "sub_kinds_d_e_g": dict(sorted(sub.items())), "lapack_eta_max": _sci(bc.lapack_eta(n)),
                       "bound": _sci(bc.bk_bounds(n))}
    return out


def bk_run_summary(v, n, out):
    cs, refs = bc.bk_cases(n), bc.bk_reference(n)
    out = {k: a[:bc.N_BLOCKS] for k, a in out.items()}
    if v == 0:   # the blocks whose unpivoted result the solver keeps
        sc = bc.score_bk(n, out, only=lambda i: (n == 10 and cs.kinds[i] == "b") or refs[i]["neg"] == 0)
    else:
        sc = bc.score_bk(n, out)
    fwd = {}
    for i, s in enumerate(sc):
        if s is not None:
            fwd[cs.kinds[i]] = max(fwd.get(cs.kinds[i], 0.0), bc.forward_error(refs[i], out["x"][i][0], cs.rhs[i], 0))
    two, inter = bc.pivot_stats(out["ip"])
    return {"eta_max": _sci(bc.family_max(n, sc, "eta")), "recon_max": _sci(bc.family_max(n, sc, "recon")),
            "forward_error_max": _sci(fwd), "two_by_two_pivots": two, "interchanges": inter,
            "blocks_scored": sum(s is not None for s in sc)}


def chol_run_summary(v, n, out):
    _, _, rhs, kinds = bc.chol_cases(n)
    refs = bc.chol_reference(n)
    res = {}
    for i, kind in enumerate(kinds):
        if refs[i] is None:
            continue
        back, fwd = bc.chol_factor_errors(refs[i], n, out["K"][i])
        e = max(bc.eta(refs[i], out["x"][i][k], rhs[i][k]) for k in range(bc.NRHS))
        w = res.setdefault(kind, {"factor_backward": 0.0, "eta": 0.0, "factor_vs_mpmath": 0.0})
        w["factor_backward"], w["eta"] = max(w["factor_backward"], back), max(w["eta"], e)
        w["factor_vs_mpmath"] = max(w["factor_vs_mpmath"], fwd)
    return {"per_kind": {k: _sci(w) for k, w in res.items()}, "lapack_eta_max": _sci(bc.lapack_chol_eta(n)),
            "bound": _sci(bc.chol_bounds(n)), "cases_per_kind": dict(collections.Counter(kinds))}


def ulp_diff(a, b):
    """Largest distance in units of the last place between two float64 arrays (finite entries)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    ia, ib = a[ok].view(np.int64), b[ok].view(np.int64)
    ia, ib = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia), np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return int(np.max(np.abs(ia - ib))) if ia.size else 0


def profile(runs, run_fn, label):
    res = {}
    for v, n, s in runs:
        out = run_fn(v, n, s)
        res[f"variant{v}_n{n}_stride{s}"] = chol_run_summary(v, n, out) if v >= 6 else bk_run_summary(v, n, out)
        print(label, v, n, s, "done", flush=True)
    return res


def inputs(v, n):
    if v >= 6:
        _, inp, rhs, _ = bc.chol_cases(n)
        return inp, rhs
    cs = bc.bk_cases(n)
    return cs.K0, cs.rhs


def device_vs_emulation(dev_fn, emu_fn):
    """Per device run, against the contracting host build (variant 5 against its variant 4, the LDS slice of
    variant 2 against its variant 1) and against the device's own packed form: pivots / flags equal, and the largest
    ulp distance of the factor and of the solutions."""
    res = {}
    for v, n, s in DEVICE_RUNS:
        ve = 4 if v == 5 else 1 if v == 2 else v
        d, e = dev_fn(v, n, s), emu_fn(ve, n, 1)
        N = bc.N_BLOCKS
        row = {"emulation_variant": ve, "pivots_equal": bool(np.array_equal(d["ip"][:N], e["ip"][:N])),
               "flags_equal": bool(np.array_equal(d["flags"][:N], e["flags"][:N])),
               "factor_ulp": ulp_diff(d["K"][:N], e["K"][:N]), "solution_ulp": ulp_diff(d["x"][:N], e["x"][:N])}
        if v >= 1 and n in (10, 18):
            p = dev_fn(1, n, 1)
            row["against_device_packed"] = {"pivots_equal": bool(np.array_equal(d["ip"][:N], p["ip"][:N])),
                                            "factor_ulp": ulp_diff(d["K"][:N], p["K"][:N]),
                                            "solution_ulp": ulp_diff(d["x"][:N], p["x"][:N])}
        res[f"variant{v}_n{n}_stride{s}"] = row
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import _hostsim as hs
    doc = {"cases": cases_summary()}
    if a.cpu:
        for name, fn in (("hostsim", hs.bk_probe_host), ("emusim", hs.bk_probe_emusim)):
            doc[name] = profile(HOST_RUNS + CHOL_RUNS, lambda v, n, s: fn(v, n, *inputs(v, n), lane_stride=s), name)
    if a.gpu:
        from headland_trajectory_planning_amd import _native
        ctx = _native.Context(0)
        cache = {}

        def dev(v, n, s):
            if (v, n, s) not in cache:
                cache[(v, n, s)] = ctx.bk_probe(v, n, *inputs(v, n), lane_stride=s)
            return cache[(v, n, s)]
        doc["device"] = profile(DEVICE_RUNS + CHOL_RUNS, dev, "device")
        doc["device_vs_emulation"] = device_vs_emulation(
            dev, lambda v, n, s: hs.bk_probe_emusim(v, n, *inputs(v, n), lane_stride=s))
    out = a.out or os.path.join(ROOT, "profiles", "bk_probe_gpu.json" if a.gpu else "bk_probe_cpu.json")
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", out)


if __name__ == "__main__":
    main()

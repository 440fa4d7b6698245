"""The small dense factorizations of csrc/obca_core.h on the device (htp_bk_probe: one block per lane, 64-lane
workgroups, the solver's LDS layout), one launch of 209 blocks per (variant, n): against the 200-bit mpmath
reference and LAPACK-derived bounds of tests/_bk_cases.py (see tests/test_bk_cpu.py for the rule), against the
contracting host build of the same body (htp_emusim_bk_probe) bit for bit, and the device forms against one
another.  Variant 5 (bk_factor_batch_p / bk_solve_batch_l, device only in the solver) is compared with the
emulation's variant 4: the substitution the solver's bit-exact emulation relies on.

Measured on the MI355X (profiles/bk_probe_gpu.json, tools/bk_probe_profile.py --gpu): every device form equals
the emulation in every pivot, flag and bit (0 ulp), and the forms equal one another at n = 10 and n = 18, so no
pair needed the weaker integer-plus-eta comparison.  Largest eta 1.6e-16 / 1.9e-16 / 2.7e-16 / 1.9e-16 and largest
reconstruction error 3.3e-16 / 2.5e-16 / 5.2e-16 / 5.7e-16 at n = 4 / 8 / 10 / 18, against bounds of 4.4e-16 ..
2.0e-15; the case counts and the pivots exercised are those of tests/test_bk_cpu.py.
"""
import functools

import numpy as np
import pytest

import _bk_cases as bc
import _hostsim as hs
from headland_trajectory_planning_amd import _native

pytestmark = pytest.mark.gpu

PIVOTED = [(1, 4, 1), (1, 8, 1), (1, 10, 1), (1, 18, 1), (2, 10, 1), (3, 10, 64), (3, 10, 1), (3, 18, 1),
           (4, 10, 64), (4, 10, 1), (4, 18, 1), (5, 10, 64)]
UNPIVOTED = [(0, 10, 1), (0, 4, 1), (0, 8, 1)]
CHOL = [(6, 1, 1), (6, 2, 1), (6, 3, 1), (7, 5, 1)]
EXTRA = 64 - 17 + 5   # sentinel rows: the partial wavefront's idle lanes and a few past the launch


@functools.lru_cache(maxsize=None)
def _ctx():
    return _native.Context(0)


def _inputs(v, n):
    if v >= 6:
        _, inp, rhs, _ = bc.chol_cases(n)
        return inp, rhs
    cs = bc.bk_cases(n)
    return cs.K0, cs.rhs


@functools.lru_cache(maxsize=None)
def device(v, n, s, reverse=False):
    K0, rhs = _inputs(v, n)
    if reverse:
        K0, rhs = K0[::-1], rhs[::-1]
    return _ctx().bk_probe(v, n, K0, rhs, lane_stride=s, extra_rows=EXTRA)


@functools.lru_cache(maxsize=None)
def emu(v, n):
    K0, rhs = _inputs(v, n)
    return hs.bk_probe_emusim(v, n, K0, rhs)


def _finite(n):
    cs = bc.bk_cases(n)   # the 2 x 2 pivot with determinant 0.0 leaves NaNs, whose payloads are not pinned
    return [i for i in range(bc.N_BLOCKS) if not (cs.kinds[i] == "g" and cs.subs[i] == 2)]


def _same(a, b, rows, tag, fields=("K", "x")):
    N = bc.N_BLOCKS
    assert np.array_equal(a["ip"][:N], b["ip"][:N]), tag
    assert np.array_equal(a["flags"][:N], b["flags"][:N]), tag
    for f in fields:
        assert np.array_equal(bc.bits(a[f][:N][rows]), bc.bits(b[f][:N][rows])), (tag, f)


def _check_bounds(n, scores, tag):
    bounds = bc.bk_bounds(n)
    for field in ("eta", "recon"):
        got = bc.family_max(n, scores, field)
        print(tag, field, {k: "%.2e" % v for k, v in got.items()}, "bound", {k: "%.2e" % bounds[k] for k in got})
        for kind, v in got.items():
            assert v <= bounds[kind], (tag, field, kind, v, bounds[kind])


def test_inertia_flags_and_idle_lanes():
    S = _native.BK_SENTINEL
    for v, n, s in PIVOTED + UNPIVOTED + CHOL:
        out, N = device(v, n, s), bc.N_BLOCKS
        # lanes past the block count (47 of them in the last wavefront) leave their rows untouched
        assert np.all(out["K"][N:] == S) and np.all(out["x"][N:] == S) and np.all(out["x2"][N:] == S), (v, n, s)
        assert np.all(out["ip"][N:] == -77) and np.all(out["flags"][N:] == -77), (v, n, s)
        if not (v == 4 or v == 7 or (v == 0 and n == 10)):
            assert np.all(out["x2"] == S), (v, n, s)
    for v, n, s in PIVOTED:
        cs, refs, out = bc.bk_cases(n), bc.bk_reference(n), device(v, n, s)
        for i in range(bc.N_BLOCKS):
            neg, zero, piv, ok = out["flags"][i]
            assert zero == int(cs.singular[i]), (v, n, s, i, cs.kinds[i], cs.subs[i], zero)
            assert (piv, ok) == (-1, -1)
            if not cs.singular[i]:
                assert neg == refs[i]["neg"], (v, n, s, i, cs.kinds[i], cs.subs[i], neg, refs[i]["neg"])
    for v, n, s in UNPIVOTED:
        cs, refs, out = bc.bk_cases(n), bc.bk_reference(n), device(v, n, s)
        for i in cs.of("b"):
            assert tuple(out["flags"][i][:3]) == (2, 0, 0 if n == 10 else 1), (n, i, out["flags"][i])
        for i in cs.of("c"):
            assert out["flags"][i][2] == 1, (n, i)
        for i in cs.of("a"):
            if refs[i]["neg"] == 0:
                assert tuple(out["flags"][i][:3]) == (0, 0, 0), (n, i)
        for i in cs.of("g"):
            assert out["flags"][i][1] == 1, (n, i, cs.subs[i])


def test_reconstruction_and_solve():
    for v, n, s in PIVOTED:
        _check_bounds(n, bc.score_bk(n, {k: a[:bc.N_BLOCKS] for k, a in device(v, n, s).items()}), (v, n, s))
    for v, n, s in UNPIVOTED:   # the blocks whose unpivoted result the solver keeps (tests/test_bk_cpu.py)
        cs, refs = bc.bk_cases(n), bc.bk_reference(n)
        out = {k: a[:bc.N_BLOCKS] for k, a in device(v, n, s).items()}
        _check_bounds(n, bc.score_bk(n, out, only=lambda i: (n == 10 and cs.kinds[i] == "b") or refs[i]["neg"] == 0),
                      (v, n, s))


def test_device_matches_emulation():
    for v, n, s in PIVOTED + UNPIVOTED:
        ve = 4 if v == 5 else 1 if v == 2 else v   # the emulation runs neither the _p / _l pair nor an LDS slice
        fields = ("K", "x", "x2") if (v == 4 or (v == 0 and n == 10)) else ("K", "x")
        _same(device(v, n, s), emu(ve, n), _finite(n), ("device", v, n, s, "emusim", ve), fields)
    for v, n, s in CHOL:
        _, _, _, kinds = bc.chol_cases(n)
        ok = [i for i, k in enumerate(kinds) if k.startswith("cond")]   # a failed chol3 leaves NaN / inf behind
        _same(device(v, n, s), emu(v, n), ok, ("device chol", n), ("K", "x", "x2") if v == 7 else ("K", "x"))


def test_device_forms_agree():
    for n, runs in ((10, [(2, 1), (3, 64), (3, 1), (4, 64), (4, 1), (5, 64)]), (18, [(3, 1), (4, 1)])):
        base = device(1, n, 1)
        for v, s in runs:
            _same(device(v, n, s), base, _finite(n), ("device", n, v, s, "against packed"))
            if v == 4:
                out = device(v, n, s)
                rows = _finite(n)
                assert np.array_equal(bc.bits(out["x2"][:bc.N_BLOCKS][rows]), bc.bits(out["x"][:bc.N_BLOCKS][rows]))


def test_lane_placement_does_not_matter():
    for v, n, s in PIVOTED + UNPIVOTED:
        a, b = device(v, n, s), device(v, n, s, True)
        N = bc.N_BLOCKS
        rows = _finite(n)
        assert np.array_equal(a["ip"][:N], b["ip"][:N][::-1]) and np.array_equal(a["flags"][:N], b["flags"][:N][::-1])
        for f in ("K", "x", "x2"):
            assert np.array_equal(bc.bits(a[f][:N][rows]), bc.bits(b[f][:N][::-1][rows])), (v, n, s, f)


def test_cholesky():
    for v, n, s in CHOL:
        A, inp, rhs, kinds = bc.chol_cases(n)
        refs, bounds, out = bc.chol_reference(n), bc.chol_bounds(n), device(v, n, s)
        for i, kind in enumerate(kinds):
            assert out["flags"][i][3] == (0 if refs[i] is None else 1), (n, i, kind, out["flags"][i])
            if refs[i] is None:
                continue
            back, _ = bc.chol_factor_errors(refs[i], n, out["K"][i])
            e = max(bc.eta(refs[i], out["x"][i][k], rhs[i][k]) for k in range(bc.NRHS))
            assert back <= bounds[kind] and e <= bounds[kind], (n, i, kind, back, e, bounds[kind])

"""The small dense factorizations of csrc/obca_core.h (unpivoted local LDL', the Bunch-Kaufman forms, chol3 /
chol5) through csrc/bk_probe.h in both host builds -- the serial one (g++) and the contracting one (clang with the
device's contraction) -- against a 200-bit mpmath reference on the seeded blocks of tests/_bk_cases.py.

Bound on the normwise backward error eta of a solve and on the reconstruction error of a factor, per family:
4 x the largest eta of LAPACK's own solve of the same blocks (scipy.linalg.solve assume_a="sym"; cho_solve for the
Cholesky helpers), at least n 2^-53; the factor 4 covers the different summation order of an equally stable
algorithm.  Nothing from the code under test enters it.  Measured (profiles/bk_probe_cpu.json lists every family,
size and form; written by tools/bk_probe_profile.py --cpu), n = 4 / 8 / 10 / 18, the worse of the two builds:
LAPACK's largest eta over the families 1.7e-16 / 2.5e-16 / 2.0e-16 / 2.5e-16, so bounds of 4.4e-16 .. 6.8e-16 /
8.9e-16 .. 9.8e-16 / 1.1e-15 / 2.0e-15; the pivoted forms' largest eta 2.1e-16 / 1.9e-16 / 2.7e-16 / 1.9e-16 and
largest reconstruction error 3.6e-16 / 3.2e-16 / 6.1e-16 / 5.7e-16 (every pivoted form of one build gives the same
bits, so the same figures); LocalBlock<4,4> unpivoted 5.4e-16 and 5.3e-16 at n = 10; chol3 / chol5 largest eta
2.2e-16 and largest factor error 3.1e-16 against bounds of 3.3e-16 .. 8.6e-16 (LAPACK's cho_solve 8.3e-17 .. 2.2e-16).
The 209 blocks of one size hold 19 a, 98 b (18 distinct + 80 filler lanes from a pool of 9), 18 c, 19 d, 19 e,
18 f, 18 g; the pivot vectors hold 128 / 146 / 188 / 293 two-by-two pivots and 153 / 223 / 299 / 559 interchanges.

LAPACK's dsytf2 is present in scipy.linalg.lapack, so the pivot vectors are compared with it.
"""
import functools

import numpy as np
import pytest

import _bk_cases as bc
import _hostsim as hs

BUILDS = {"hostsim": hs.bk_probe_host, "emusim": hs.bk_probe_emusim}
# (variant, n, lane_stride) of the pivoted forms; lane_stride 64 runs the device's interleaved LDS layout on the host
PIVOTED = [(1, 4, 1), (1, 8, 1), (1, 10, 1), (1, 18, 1), (2, 10, 1), (3, 10, 1), (3, 18, 1), (3, 10, 64),
           (4, 10, 1), (4, 18, 1), (4, 10, 64), (5, 10, 1), (5, 10, 64)]
UNPIVOTED = [(0, 10, 1), (0, 4, 1), (0, 8, 1)]


@functools.lru_cache(maxsize=None)
def run(build, variant, n, stride):
    cs = bc.bk_cases(n)
    return BUILDS[build](variant, n, cs.K0, cs.rhs, lane_stride=stride, extra_rows=3)


def _check_bounds(n, scores, tag):
    bounds = bc.bk_bounds(n)
    for field in ("eta", "recon"):
        got = bc.family_max(n, scores, field)
        print(tag, field, {k: "%.2e" % v for k, v in got.items()}, "bound", {k: "%.2e" % bounds[k] for k in got})
        for kind, v in got.items():
            assert v <= bounds[kind], (tag, field, kind, v, bounds[kind])


@pytest.mark.parametrize("build", BUILDS)
def test_inertia_and_flags(build):
    for v, n, s in PIVOTED:
        cs, refs, out = bc.bk_cases(n), bc.bk_reference(n), run(build, v, n, s)
        for i in range(bc.N_BLOCKS):
            neg, zero, piv, ok = out["flags"][i]
            assert zero == int(cs.singular[i]), (v, n, s, i, cs.kinds[i], cs.subs[i], zero)
            assert (piv, ok) == (-1, -1)
            if not cs.singular[i]:
                assert neg == refs[i]["neg"], (v, n, s, i, cs.kinds[i], cs.subs[i], neg, refs[i]["neg"])
        # rows past the block count, and x2 where the form has none, keep the sentinel
        assert np.all(out["K"][bc.N_BLOCKS:] == hs._native.BK_SENTINEL) and np.all(out["ip"][bc.N_BLOCKS:] == -77)
        assert np.all(out["flags"][bc.N_BLOCKS:] == -77) and np.all(out["x"][bc.N_BLOCKS:] == hs._native.BK_SENTINEL)
        if v != 4:
            assert np.all(out["x2"] == hs._native.BK_SENTINEL), (v, n, s)


@pytest.mark.parametrize("build", BUILDS)
def test_unpivoted_inertia_and_piv(build):
    for v, n, s in UNPIVOTED:
        cs, refs, out = bc.bk_cases(n), bc.bk_reference(n), run(build, v, n, s)
        for i in cs.of("b"):
            neg, zero, piv, _ = out["flags"][i]
            # LocalBlock looks at the multiplier pivots only; PtBlock has no equality rows, every pivot counts
            assert (neg, zero, piv) == (2, 0, 0 if n == 10 else 1), (n, i, neg, zero, piv)
        for i in cs.of("c"):
            assert out["flags"][i][2] == 1, (n, i)
        for i in cs.of("a"):
            if refs[i]["neg"] == 0:
                assert tuple(out["flags"][i][:3]) == (0, 0, 0), (n, i)
        for i in cs.of("g"):
            assert out["flags"][i][1] == 1, (n, i, cs.subs[i])


@pytest.mark.parametrize("build", BUILDS)
def test_reconstruction_and_solve(build):
    for v, n, s in PIVOTED:
        _check_bounds(n, bc.score_bk(n, run(build, v, n, s)), (build, v, n, s))
    # The unpivoted forms are scored on the blocks whose unpivoted result the solver keeps (`piv` false; every other
    # block is redone by the pivoted path): positive definite blocks, and for LocalBlock the saddle blocks too.
    # PtBlock has no equality rows, so a saddle block sets its `piv` (PtBlock<4> reconstructs family b to 5.7e-16).
    for v, n, s in UNPIVOTED:
        cs, refs, out = bc.bk_cases(n), bc.bk_reference(n), run(build, v, n, s)
        _check_bounds(n, bc.score_bk(n, out, only=lambda i: (n == 10 and cs.kinds[i] == "b") or refs[i]["neg"] == 0),
                      (build, v, n, s))
        if n == 10:   # LocalBlock::forward: unit lower L y = b
            bound = bc.bk_bounds(n)["b"]
            for i in cs.of("b")[:20]:
                L = np.tril(bc.unpack(out["K"][i], n), -1) + np.eye(n)
                for k in range(bc.NRHS):
                    e = bc.lower_solve_error(n, L, out["x2"][i][k], cs.rhs[i][k])
                    assert e <= bound, (build, i, k, e, bound)


@pytest.mark.parametrize("build", BUILDS)
def test_forms_agree_bit_for_bit(build):
    for n, others in ((10, [(2, 1), (3, 1), (4, 1), (5, 1), (3, 64), (4, 64), (5, 64)]), (18, [(3, 1), (4, 1)])):
        cs, base = bc.bk_cases(n), run(build, 1, n, 1)
        finite = [i for i in range(bc.N_BLOCKS) if not (cs.kinds[i] == "g" and cs.subs[i] == 2)]  # the others' NaNs
        for v, s in others:
            out = run(build, v, n, s)
            assert np.array_equal(out["ip"], base["ip"]), (build, n, v, s)
            assert np.array_equal(out["flags"][:, :2], base["flags"][:, :2]), (build, n, v, s)
            for f in ("K", "x"):
                assert np.array_equal(bc.bits(out[f][finite]), bc.bits(base[f][finite])), (build, n, v, s, f)
            if v == 4:   # bk_solve_batch_multi: each column sees bk_solve_batch's operations
                assert np.array_equal(bc.bits(out["x2"][finite]), bc.bits(out["x"][finite])), (build, n, s)


@pytest.mark.parametrize("build", BUILDS)
def test_pivots_match_lapack(build):
    from scipy.linalg import lapack
    for n in bc.BK_SIZES:
        cs, out = bc.bk_cases(n), run(build, 1, n, 1)
        for kind in "ade":
            for i in cs.of(kind):
                _, ipiv, info = lapack.dsytf2(cs.dense(i), lower=1)
                assert info == 0, (n, i, info)
                ours = out["ip"][i]   # 0-based: k, or -(kp + 1); LAPACK: 1-based k + 1, or -(kp + 1)
                assert np.array_equal(np.where(ours >= 0, ours + 1, ours), ipiv), (n, i, kind, ours, ipiv)
                # the families are what they claim, on LAPACK's pivots alone
                two, inter = bc.pivot_stats([np.where(ipiv > 0, ipiv - 1, ipiv)])
                if kind == "d" and cs.subs[i] < 2:
                    assert two == n // 2, (n, i, ipiv)
                if kind == "e":
                    assert (two, inter) == ((1, 0), (0, 1), (1, 1))[cs.subs[i]], (n, i, cs.subs[i], ipiv)
                    k = n - 3 if cs.subs[i] == 2 else n - 2
                    assert ipiv[k] != k + 1 and all(ipiv[j] == j + 1 for j in range(n) if j not in (k, k + 1))


@pytest.mark.parametrize("build", BUILDS)
def test_cholesky(build):
    for v, n in ((6, 1), (6, 2), (6, 3), (7, 5)):
        A, inp, rhs, kinds = bc.chol_cases(n)
        refs, bounds = bc.chol_reference(n), bc.chol_bounds(n)
        out = BUILDS[build](v, n, inp, rhs, extra_rows=3)
        assert np.all(out["flags"][bc.N_BLOCKS:] == -77) and np.all(out["x"][bc.N_BLOCKS:] == hs._native.BK_SENTINEL)
        worst = {}
        for i, kind in enumerate(kinds):
            assert out["flags"][i][3] == (0 if refs[i] is None else 1), (build, n, i, kind, out["flags"][i])
            if refs[i] is None:
                continue
            if v == 6:   # chol3 zeroes Lc and reads nothing outside the leading nv x nv block
                Lc = out["K"][i].reshape(3, 3)
                assert np.all(Lc[n:, :] == 0.0) and np.all(np.triu(Lc, 1) == 0.0), (n, i, Lc)
            back, fwd = bc.chol_factor_errors(refs[i], n, out["K"][i])
            e = max(bc.eta(refs[i], out["x"][i][k], rhs[i][k]) for k in range(bc.NRHS))
            w = worst.setdefault(kind, [0.0, 0.0, 0.0])
            w[:] = max(w[0], back), max(w[1], e), max(w[2], fwd)
            assert back <= bounds[kind] and e <= bounds[kind], (build, n, i, kind, back, e, bounds[kind])
            if v == 7:   # chol5_fwd: L y = b with the factor's own L
                L = bc.chol_factor_dense(n, out["K"][i])
                L[np.diag_indices(n)] = 1.0 / np.diag(L)
                for k in range(bc.NRHS):
                    assert bc.lower_solve_error(n, L, out["x2"][i][k], rhs[i][k]) <= bounds[kind], (build, i, k)
        print(build, "chol", n, {k: ["%.2e" % x for x in w] for k, w in worst.items()},
              "bound", {k: "%.2e" % b for k, b in bounds.items()})


def test_pivot_packing_round_trip():
    """piv_put / piv_get: every legal value (-n .. n - 1, n <= 10) in every slot, the other slots undisturbed"""
    n = 10
    rng = np.random.default_rng(5)
    for trial in range(4):
        base = [int(v) for v in rng.integers(-n, n, n)]
        w = 0
        for j, v in enumerate(base):
            w, _ = hs.bk_piv_roundtrip(w, j, v, n)
        for j in range(n):
            for v in range(-n, n):
                w2, slots = hs.bk_piv_roundtrip(w, j, v, n)
                want = list(base)
                want[j] = v
                assert list(slots) == want, (j, v, list(slots), want)
                assert w2 < 1 << 60

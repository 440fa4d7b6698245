"""TEST-ONLY: seeded blocks for the small dense factorizations of csrc/obca_core.h (csrc/bk_probe.h), their
high-precision reference (mpmath, 200 bits) and the scores the tests assert.  Nothing here looks at the code
under test: the families, the conditions on them and the bounds come from the reference and from LAPACK alone.

Families, per block size n (packed lower, 4 right-hand sides each):
  a  Q diag(lambda) Q' with a prescribed number of negative eigenvalues (instance i has i mod (n + 1) of them, so
     every split 0 .. n appears), |lambda| in [1e-2, 1e2]
  b  saddle [[H, C'], [C, 0]], H positive definite, C 2 x (n - 2) of full rank (the solver's own shape)
  c  b with one pivot of H's L D L' made slightly negative (-0.02 .. -0.1)
  d  zero diagonal: 0 a permuted direct sum of [[0, t], [t, 0]] (every Bunch-Kaufman step is 2 x 2, with an
     interchange), 1 the same with a 1e-3 zero-diagonal coupling (still every step 2 x 2), 2 dense zero-diagonal
  e  diagonally dominant but for the trailing rows: 0 the only 2 x 2 pivot at k = n - 2 without interchange,
     1 the only interchange at k = n - 2 (1 x 1 pivot), 2 a 2 x 2 pivot at k = n - 3 that interchanges the
     last two rows
  f  D A D with D = diag(2^e), e spread over [-7, 7] (both ends present): entries over 2^+-14.  A wider spread
     cannot meet the conditioning rule below (a symmetric row scaling over 2^+-30 puts the eigenvalues 2^-60
     apart), and that rule is the one that fails the generator.
  g  exactly singular: 0 a zero row and column, 1 the all-zero block, 2 a decoupled 2 x 2 pivot [[0, t], [t, 0]]
     with t = 2^-600, whose determinant t^2 underflows to exactly 0.0

Launch layout (209 = 64 * 3 + 17 blocks, one partial wavefront): blocks 0 .. 127 take kind (index mod 7); wavefront
2 is 63 saddle lanes and one d lane (lane 21); the partial wavefront is 16 saddle lanes and one e lane (lane 9).
The saddle filler lanes cycle through a pool of 9 distinct blocks, so neighbouring lanes always differ.
"""
import functools

import mpmath as mp
import numpy as np

PREC = 200
KINDS = "abcdefg"
N_BLOCKS = 64 * 3 + 17
NRHS = 4
BK_SIZES = (4, 8, 10, 18)
COND_MIN = 1e-9
SEED = 20261


def pack(A):
    n = A.shape[0]
    return np.array([A[r, c] for r in range(n) for c in range(r + 1)], dtype=np.float64)


def unpack(p, n):
    A = np.zeros((n, n))
    q = 0
    for r in range(n):
        for c in range(r + 1):
            A[r, c] = A[c, r] = p[q]
            q += 1
    return A


def _orth(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _sym(A):
    return (A + A.T) / 2


def _spectral(rng, n, negs, lo, hi):
    lam = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)
    lam[:negs] *= -1.0
    Q = _orth(rng, n)
    return _sym((Q * rng.permutation(lam)) @ Q.T)


def _C(rng, m):
    while True:
        C = rng.standard_normal((2, m))
        if m < 2 or np.linalg.svd(C, compute_uv=False)[-1] > 0.2:
            return C


def _saddle(rng, n, neg_pivot=None):
    m = n - 2
    if neg_pivot is None:
        G = rng.standard_normal((m, m))
        H = G @ G.T / m + 0.5 * np.eye(m)
    else:
        L = np.tril(0.3 * rng.standard_normal((m, m)), -1) + np.eye(m)
        d = rng.uniform(0.5, 2.0, m)
        d[neg_pivot] = -rng.uniform(0.02, 0.1)
        H = _sym((L * d) @ L.T)
    A = np.zeros((n, n))
    A[:m, :m] = H
    A[m:, :m] = _C(rng, m)
    A[:m, m:] = A[m:, :m].T
    return A


def _dominant(rng, n, off=1e-2):
    A = _sym(off * rng.standard_normal((n, n)))
    A[np.diag_indices(n)] = rng.uniform(1.0, 3.0, n) * rng.choice([-1.0, 1.0], n)
    return A


def _block(kind, n, i, rng):
    """-> (dense symmetric block, sub-kind)"""
    if kind == "a":
        return _spectral(rng, n, i % (n + 1), 1e-2, 1e2), i % (n + 1)
    if kind == "b":
        return _saddle(rng, n), 0
    if kind == "c":
        return _saddle(rng, n, neg_pivot=i % (n - 2)), i % (n - 2)
    if kind == "d":
        sub = i % 3
        if sub == 2:
            A = _sym(rng.standard_normal((n, n)))
        else:
            A = np.zeros((n, n)) if sub == 0 else _sym(1e-3 * rng.standard_normal((n, n)))
            p = rng.permutation(n)
            for q in range(0, n, 2):
                A[p[q], p[q + 1]] = A[p[q + 1], p[q]] = rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
        A[np.diag_indices(n)] = 0.0
        return A, sub
    if kind == "e":
        sub = i % 3
        A = _dominant(rng, n)
        s = rng.uniform(0.8, 1.2, 6) * rng.choice([-1.0, 1.0], 6)
        if sub == 0:
            A[n - 2:, n - 2:] = [[0.0, 1.5 * s[0]], [1.5 * s[0], 0.0]]
        elif sub == 1:
            A[n - 2:, n - 2:] = [[0.1 * s[1], 1.2 * s[0]], [1.2 * s[0], 2.5 * s[2]]]
        else:
            b, sm, t, d = 1.5 * s[0], 0.3 * s[1], 0.4 * s[2], s[3]
            A[n - 3:, n - 3:] = [[0.0, sm, b], [sm, d, t], [b, t, 0.0]]
        return A, sub
    if kind == "f":
        A0 = _spectral(rng, n, int(rng.integers(0, n + 1)), 1.0, 2.0)
        e = rng.integers(-7, 8, n)
        e[0], e[1] = 7, -7
        D = 2.0 ** rng.permutation(e)
        return A0 * D[:, None] * D[None, :], 0
    sub = i % 3
    if sub == 0:
        A = _spectral(rng, n, int(rng.integers(0, n + 1)), 1e-1, 1e1)
        j = (i // 3) % n
        A[j, :] = 0.0
        A[:, j] = 0.0
        return A, sub
    if sub == 1:
        return np.zeros((n, n)), sub
    A = _dominant(rng, n)
    p = (i // 3) % (n - 1)
    A[p:p + 2, :] = 0.0
    A[:, p:p + 2] = 0.0
    A[p, p + 1] = A[p + 1, p] = 2.0 ** -600
    return A, sub


def layout():
    """kind of each of the N_BLOCKS blocks, and whether it is a filler lane (drawn from the saddle pool)"""
    kinds = [KINDS[i % 7] for i in range(128)]
    filler = [False] * 128
    for lane in range(64):
        kinds.append("d" if lane == 21 else "b")
        filler.append(lane != 21)
    for lane in range(17):
        kinds.append("e" if lane == 9 else "b")
        filler.append(lane != 9)
    assert len(kinds) == N_BLOCKS
    return kinds, filler


class Cases:
    def __init__(self, n, K0, rhs, kinds, subs):
        self.n, self.K0, self.rhs, self.kinds, self.subs = n, K0, rhs, kinds, subs
        self.K0.setflags(write=False)
        self.rhs.setflags(write=False)

    def dense(self, i):
        return unpack(self.K0[i], self.n)

    def of(self, kind):
        return [i for i, k in enumerate(self.kinds) if k == kind]

    @property
    def singular(self):
        return [k == "g" for k in self.kinds]


@functools.lru_cache(maxsize=None)
def bk_cases(n):
    kinds, filler = layout()
    pool = [_block("b", n, j, np.random.default_rng([SEED, n, 7, j]))[0] for j in range(9)]
    count = {k: 0 for k in KINDS}
    K0, subs, nf = [], [], 0
    for idx, (kind, fill) in enumerate(zip(kinds, filler)):
        if fill:
            A, sub = pool[nf % 9], 0
            nf += 1
        else:
            A, sub = _block(kind, n, count[kind], np.random.default_rng([SEED, n, KINDS.index(kind), count[kind]]))
            count[kind] += 1
        assert np.array_equal(A, A.T), (n, idx, kind)
        K0.append(pack(A))
        subs.append(sub)
    rhs = np.random.default_rng([SEED, n, 99]).standard_normal((N_BLOCKS, NRHS, n))
    return Cases(n, np.array(K0), rhs, kinds, subs)


# ---------------------------------------------------------------------------------------------- reference (mpmath)
def _mpm(A):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(A)])


def _norm_inf(M):
    return max(sum(abs(M[r, c]) for c in range(M.cols)) for r in range(M.rows)) if M.rows else mp.mpf(0)


_ref_cache = {}


def block_ref(A, singular):
    """Reference of one block, memoised on its bytes: mp matrix, its inf-norm, eigenvalues / negative count /
    conditioning and the mpmath.lu_solve solutions' source (non-singular blocks only)."""
    key = (A.tobytes(), A.shape[0], singular)
    if key not in _ref_cache:
        with mp.workprec(PREC):
            M = _mpm(A)
            ref = {"M": M, "norm": _norm_inf(M)}
            if not singular:
                ev = mp.eigsy(M, eigvals_only=True)
                ev = [ev[i] for i in range(len(ev))]
                ref["neg"] = sum(1 for v in ev if v < 0)
                ref["ratio"] = float(min(abs(v) for v in ev) / max(abs(v) for v in ev))
            _ref_cache[key] = ref
    return _ref_cache[key]


@functools.lru_cache(maxsize=None)
def bk_reference(n):
    """Per block of bk_cases(n): the reference dict; asserts the generator's conditions (conditioning of every
    non-singular block, every family populated, every negative-count split present in family a)."""
    cs = bk_cases(n)
    refs = [block_ref(cs.dense(i), cs.singular[i]) for i in range(N_BLOCKS)]
    for kind in KINDS:
        assert cs.of(kind), f"family {kind} is empty at n = {n}"
    for i, r in enumerate(refs):
        if not cs.singular[i]:
            assert r["ratio"] >= COND_MIN, (n, i, cs.kinds[i], r["ratio"])
    assert {refs[i]["neg"] for i in cs.of("a")} == set(range(n + 1)), n
    assert all(refs[i]["neg"] == 2 for i in cs.of("b")), n
    return refs


def lu_reference(ref, rhs):
    """mpmath.lu_solve of the block's right-hand sides -> [nrhs][n] mp numbers (memoised in the block's reference)"""
    key = ("lu", rhs.tobytes())
    if key not in ref:
        with mp.workprec(PREC):
            ref[key] = [mp.lu_solve(ref["M"], _mpm(b).T) for b in rhs]
    return ref[key]


def eta(ref, x, b):
    """Normwise backward error |K x - b|_inf / (|K|_inf |x|_inf + |b|_inf) in mpmath; inf for a non-finite x."""
    if not np.all(np.isfinite(x)):
        return float("inf")
    with mp.workprec(PREC):
        xm, bm = _mpm(x).T, _mpm(b).T
        r = ref["M"] * xm - bm
        den = ref["norm"] * max(abs(v) for v in xm) + max(abs(v) for v in bm)
        return float(max(abs(v) for v in r) / den)


def forward_error(ref, x, rhs, k):
    with mp.workprec(PREC):
        xr = lu_reference(ref, rhs)[k]
        return float(max(abs(mp.mpf(float(x[j])) - xr[j]) for j in range(len(x))) / max(abs(v) for v in xr))


def recon_error(ref, n, Kf, ip):
    """|K0 - P1 L1 P2 L2 .. D .. L2' P2' L1' P1'|_inf / |K0|_inf in mpmath: the factor Kf (packed lower: unit L below
    the 1 x 1 / 2 x 2 diagonal blocks of D) with the interchanges in ip, LAPACK dsytf2's lower convention 0-based
    (ip[k] = kp: rows k, kp of the trailing matrix swapped; ip[k] = ip[k + 1] = -(kp + 1): rows k + 1, kp)."""
    if not np.all(np.isfinite(Kf)):
        return float("inf")
    with mp.workprec(PREC):
        F = _mpm(unpack(Kf, n))
        steps, k = [], 0
        while k < n:
            if ip[k] >= 0:
                steps.append((k, 1, int(ip[k])))
                k += 1
            else:
                assert k + 1 < n and ip[k + 1] == ip[k], (k, list(ip))
                steps.append((k, 2, -int(ip[k]) - 1))
                k += 2
        T = mp.zeros(n, n)   # trailing matrices, rebuilt from the last step to the first
        for k, w, kp in reversed(steps):
            for r in range(k, k + w):
                for c in range(k, r + 1):
                    T[r, c] = T[c, r] = F[r, c]
            for r in range(k + w, n):     # (L D)(r, :) and the Schur term L D L'
                ld = [sum(F[r, k + a] * F[k + a, k + c] for a in range(w)) for c in range(w)]
                for q in range(k + w, r + 1):
                    T[r, q] += sum(ld[c] * F[q, k + c] for c in range(w))
                    T[q, r] = T[r, q]
                for c in range(w):
                    T[r, k + c] = T[k + c, r] = ld[c]
            kk = k + w - 1
            if kp != kk:
                assert k <= kk < kp < n, (k, w, kp)
                for c in range(k, n):
                    T[kk, c], T[kp, c] = T[kp, c], T[kk, c]
                for r in range(k, n):
                    T[r, kk], T[r, kp] = T[r, kp], T[r, kk]
        return float(_norm_inf(T - ref["M"]) / ref["norm"])


def pivot_stats(ip):
    """(2 x 2 pivots, interchanges) of a batch of pivot vectors [count][n]"""
    two = inter = 0
    for row in np.asarray(ip):
        k = 0
        while k < len(row):
            if row[k] >= 0:
                inter += int(row[k] != k)
                k += 1
            else:
                two += 1
                inter += int(-row[k] - 1 != k + 1)
                k += 2
    return two, inter


def floor_bound(n):
    return n * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def lapack_eta(n):
    """Per family, the largest eta of LAPACK's symmetric-indefinite solve (scipy.linalg.solve, assume_a="sym") on
    the non-singular blocks of bk_cases(n) -> {kind: eta}"""
    import scipy.linalg
    cs, refs = bk_cases(n), bk_reference(n)
    out = {}
    for kind in KINDS[:-1]:
        worst, seen = 0.0, set()
        for i in cs.of(kind):
            if cs.K0[i].tobytes() in seen:
                continue
            seen.add(cs.K0[i].tobytes())
            X = scipy.linalg.solve(cs.dense(i), cs.rhs[i].T, assume_a="sym").T
            worst = max(worst, max(eta(refs[i], X[k], cs.rhs[i][k]) for k in range(NRHS)))
        out[kind] = worst
    return out


def bk_bounds(n):
    """The bound on eta and on the reconstruction error, per family: 4 x LAPACK's own worst eta, at least n 2^-53"""
    return {k: max(4.0 * v, floor_bound(n)) for k, v in lapack_eta(n).items()}


_score_cache = {}


def score_bk(n, out, check_recon=True, only=None):
    """Scores of one probe output on bk_cases(n) -> per block {"eta": max over the right-hand sides, "recon"};
    singular blocks (and those the predicate only(i) rejects) get none.  Memoised on the output bits (forms that
    agree bit for bit score the same)."""
    cs, refs = bk_cases(n), bk_reference(n)
    res = [None] * N_BLOCKS
    for i in range(N_BLOCKS):
        if cs.singular[i] or (only is not None and not only(i)):
            continue
        key = (n, cs.K0[i].tobytes(), cs.rhs[i].tobytes(), out["K"][i].tobytes(), out["ip"][i].tobytes(),
               out["x"][i].tobytes(), check_recon)
        if key not in _score_cache:
            s = {"eta": max(eta(refs[i], out["x"][i][k], cs.rhs[i][k]) for k in range(NRHS))}
            if check_recon:
                s["recon"] = recon_error(refs[i], n, out["K"][i], out["ip"][i])
            _score_cache[key] = s
        res[i] = _score_cache[key]
    return res


def family_max(n, scores, field):
    cs = bk_cases(n)
    out = {}
    for kind in KINDS[:-1]:
        v = [scores[i][field] for i in cs.of(kind) if scores[i] is not None and field in scores[i]]
        if v:
            out[kind] = max(v)
    return out


# ------------------------------------------------------------------------------------------------- Cholesky cases
CHOL_KINDS = ["cond1e%d" % k for k in range(9)] + ["neg", "semidef"]


@functools.lru_cache(maxsize=None)
def chol_cases(n):
    """N_BLOCKS symmetric n x n matrices (n = 1, 2, 3: chol3's nv; 5: chol5), kind (index mod 11): positive
    definite with condition number 1, 10, .. 1e8; one eigenvalue -1e-3 (the others in [0.5, 2]); exactly positive
    semidefinite (4 times the all-ones matrix, whose second pivot is exactly 0; n = 1: the zero matrix).
    -> (dense [count][n][n], probe input [count][9 or 25], rhs [count][NRHS][n], kinds)"""
    A, kinds = [], []
    for i in range(N_BLOCKS):
        kind = CHOL_KINDS[i % 11]
        rng = np.random.default_rng([SEED, 1000 + n, i])
        Q = _orth(rng, n)
        if kind == "neg":
            lam = rng.uniform(0.5, 2.0, n)
            lam[rng.integers(0, n)] = -1e-3
            M = _sym((Q * lam) @ Q.T) if n > 1 else np.array([[-1e-3]])
        elif kind == "semidef":
            M = np.full((n, n), 4.0) if n > 1 else np.zeros((1, 1))
        else:
            c = int(kind[6:])
            lam = 10.0 ** -np.linspace(0.0, c, n) if n > 1 else np.array([10.0 ** -rng.uniform(0, c + 1e-9)])
            M = _sym((Q * rng.permutation(lam)) @ Q.T) * 10.0 ** rng.uniform(-1, 1)
        A.append(M)
        kinds.append(kind)
    A = np.array(A)
    if n == 5:
        inp = A.reshape(N_BLOCKS, 25).copy()
    else:
        inp = np.full((N_BLOCKS, 3, 3), 99.0)   # entries outside the leading nv x nv block must not be read
        inp[:, :n, :n] = A
        inp = inp.reshape(N_BLOCKS, 9)
    rhs = np.random.default_rng([SEED, 1000 + n, 99]).standard_normal((N_BLOCKS, NRHS, n))
    for a in (A, inp, rhs):
        a.setflags(write=False)
    return A, inp, rhs, kinds


@functools.lru_cache(maxsize=None)
def chol_reference(n):
    """Per positive definite case: the block reference and mpmath.cholesky's factor; asserts that the cases are
    what they claim (positive definite ones factor in mpmath with the stated conditioning, the others do not)."""
    A, _, _, kinds = chol_cases(n)
    refs = []
    for i, kind in enumerate(kinds):
        if kind in ("neg", "semidef"):
            with mp.workprec(PREC):
                ev = mp.eigsy(_mpm(A[i]), eigvals_only=True)
                lo = min(ev[j] for j in range(n))
            assert (lo < 0 and abs(float(lo) + 1e-3) < 1e-9) if kind == "neg" else abs(lo) < mp.mpf(2) ** -150, (n, i, lo)
            refs.append(None)
            continue
        ref = block_ref(A[i], False)
        assert ref["neg"] == 0 and ref["ratio"] >= 10.0 ** -(int(kind[6:]) + 0.5), (n, i, kind, ref["ratio"])
        with mp.workprec(PREC):
            ref["chol"] = mp.cholesky(ref["M"])
        refs.append(ref)
    return refs


def chol_factor_dense(n, Lc):
    """The probe's factor (reciprocal pivots on the diagonal; chol3: 3 x 3 stride 3, chol5: packed lower) -> L"""
    L = np.zeros((n, n))
    for r in range(n):
        for c in range(r + 1):
            v = Lc[r * (r + 1) // 2 + c] if n == 5 else Lc[r * 3 + c]
            L[r, c] = v
    return L


def chol_factor_errors(ref, n, Lc):
    """(|L L' - A|_inf / |A|_inf, max |L - mpmath.cholesky(A)| / max |cholesky(A)|) with L's diagonal inverted in
    mpmath"""
    if not np.all(np.isfinite(Lc)):
        return float("inf"), float("inf")
    with mp.workprec(PREC):
        L = _mpm(chol_factor_dense(n, Lc))
        for j in range(n):
            L[j, j] = 1 / L[j, j]
        back = float(_norm_inf(L * L.T - ref["M"]) / ref["norm"])
        C = ref["chol"]
        fwd = float(max(abs(L[r, c] - C[r, c]) for r in range(n) for c in range(r + 1)) /
                    max(abs(C[r, c]) for r in range(n) for c in range(r + 1)))
    return back, fwd


@functools.lru_cache(maxsize=None)
def lapack_chol_eta(n):
    """Per kind, the largest eta of LAPACK's Cholesky solve (scipy.linalg.cho_factor / cho_solve) -> {kind: eta}"""
    import scipy.linalg
    A, _, rhs, kinds = chol_cases(n)
    refs = chol_reference(n)
    out = {}
    for i, kind in enumerate(kinds):
        if refs[i] is None:
            continue
        X = scipy.linalg.cho_solve(scipy.linalg.cho_factor(A[i], lower=True), rhs[i].T).T
        out[kind] = max(out.get(kind, 0.0), max(eta(refs[i], X[k], rhs[i][k]) for k in range(NRHS)))
    return out


def chol_bounds(n):
    return {k: max(4.0 * v, floor_bound(n)) for k, v in lapack_chol_eta(n).items()}


def lower_solve_error(n, L, y, b):
    """|L y - b|_inf / (|L|_inf |y|_inf + |b|_inf) in mpmath for a dense lower-triangular L (doubles)"""
    if not (np.all(np.isfinite(L)) and np.all(np.isfinite(y))):
        return float("inf")
    with mp.workprec(PREC):
        Lm, ym, bm = _mpm(L), _mpm(y).T, _mpm(b).T
        r = Lm * ym - bm
        return float(max(abs(v) for v in r) / (_norm_inf(Lm) * max(abs(v) for v in ym) + max(abs(v) for v in bm)))


def bits(a):
    """float64 array -> its bit patterns (NaN-safe equality)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

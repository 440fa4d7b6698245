"""The swept-footprint envelope (csrc/envelope_core.h) through its serial host build: the extent against a 50-digit
evaluation on crafted trajectories, the raster against a numpy restatement of the definition (brute force over all
cells, poses and bodies), areas against geometry, the flags, the argument checks of the C ABI, its agreement with
the audit's poses, the default frame of the Python layer and a sanitizer build of the same core."""
import ctypes
import subprocess

import numpy as np
import pytest

import _audit_host as ah
import _envelope_host as eh
from headland_trajectory_planning_amd import _native

F = _native.ENVELOPE_FLAGS
MP_TOL = 1e-9          # the project's bound against mpmath (the audit's and the timeline's)
UNDECIDED = 1e-9       # a cell with some |n . q - bb| below this is left out of the raster comparison
UNDECIDED_SHARE = 1e-3


def _one(X, U, bodies, tau=None, time_opt=True, dT=0.25, wheelbase=1.9):
    """PackedBatch and x of one crafted trajectory."""
    X, U = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64)
    pk = _native.PackedBatch([ah.instance(X, [ah.rect(500.0, 500.0, 1.0, 1.0)], bodies, time_opt=time_opt, dT=dT,
                                          wheelbase=wheelbase)])
    return pk, ah.x_of(pk, X[None], U[None], None if tau is None else np.asarray(tau)[None], fill=np.nan)


def _parked(x, y, th, bodies, N=2):
    """N identical nodes at rest: every pose is (x, y, th) exactly."""
    X = np.tile([x, y, 0.0, th, 0.0], (N, 1))
    return _one(X, np.zeros((N - 1, 2)), bodies)


BODY = ah.rect(0.7, 0.0, 3.0, 1.4)
IMPLEMENT = ah.rect(-1.6, 0.0, 1.2, 2.6)


def _crafted(kind):
    N = 6
    t = np.linspace(0.0, 1.0, N)
    U = np.stack([0.3 * np.cos(3 * t[:-1]), 0.4 * np.sin(5 * t[:-1])], axis=1)
    tau = 0.6 + 0.4 * t[:-1]
    topt, bodies, frame, off, v = True, [BODY], (-4.0, -3.0, 0.0), 0.0, 1.1
    th = 0.4 + 1.2 * t
    if kind == "theta_above_pi":
        th = 3.0 + 1.5 * t
    elif kind == "theta_below_minus_pi":
        th = -3.0 - 1.5 * t
    elif kind == "reverse":
        v = -0.9
    elif kind == "far":
        off, frame = 100.0, (93.0, 95.0, 0.0)
    elif kind == "euler":
        topt = False
    elif kind == "two_bodies":
        bodies = [BODY, IMPLEMENT]
    elif kind == "rotated":
        bodies, frame = [BODY, IMPLEMENT], (-2.0, 5.0, -0.7)
    elif kind == "rotated_far_euler":
        topt, off, frame, bodies = False, 100.0, (110.0, 90.0, 2.5), [BODY, IMPLEMENT]
    X = np.stack([off + 3.0 * t, off + 2.0 * t ** 2, np.full(N, v), th, 0.3 - 0.5 * t], axis=1)
    pk, x = _one(X, U, bodies, tau if topt else None, time_opt=topt)
    return pk, x, np.array([frame])


CRAFTED = ["plain", "theta_above_pi", "theta_below_minus_pi", "reverse", "far", "euler", "two_bodies", "rotated",
           "rotated_far_euler"]


# ------------------------------------------------------------------ extent
@pytest.mark.parametrize("kind", CRAFTED)
def test_extent_against_mpmath(kind):
    pk, x, fr = _crafted(kind)
    S = 4
    res = eh.envelope_host(pk, x, fr, substeps=S)
    assert res.flags[0] == 0
    ref = eh.mp_extent(pk, x, 0, fr[0], S)
    err = np.abs(res.extent[0] - ref).max()
    print(kind, "largest error", err)
    assert err <= MP_TOL
    nps = eh.np_envelope(pk, x, 0, fr[0], S)
    assert np.abs(res.extent_body[0] - nps["extent_body"]).max() <= MP_TOL
    for q in range(4):   # the restatement's choice wherever the runner-up is further than the bound away
        if nps["margin"][q] > MP_TOL:
            assert np.array_equal(res.where[0, q], nps["where"][q]), (q, res.where[0, q], nps["where"][q])
    # the extent is the hull of the per-body extents
    eb = res.extent_body[0]
    assert np.array_equal(res.extent[0], [eb[:, 0].min(), eb[:, 1].max(), eb[:, 2].min(), eb[:, 3].max()])


def test_where_ties_go_to_the_lowest_index():
    # four identical poses and two identical bodies: every side is attained by all of them
    pk, x = _parked(1.0, 2.0, 0.3, [BODY, BODY], N=3)
    res = eh.envelope_host(pk, x, np.array([[0.0, 0.0, 0.1]]), substeps=2)
    assert res.flags[0] == 0 and np.array_equal(res.where[0], np.zeros((4, 3), dtype=np.int32))
    assert np.array_equal(res.extent_body[0, 0], res.extent_body[0, 1])


def test_extent_body_may_be_null():
    pk, x, fr = _crafted("two_bodies")
    a = eh.envelope_host(pk, x, fr, substeps=3)
    b = eh.envelope_host(pk, x, fr, substeps=3, extent_body=False)
    assert np.all(b.extent_body == eh.SENTINEL)
    assert a.extent.tobytes() == b.extent.tobytes() and np.array_equal(a.where, b.where)


# ------------------------------------------------------------------ raster against the numpy restatement
def _compare_raster(pk, x, fr, S, res, W, H, allow_undecided=True):
    out = eh.envelope_host(pk, x, fr, res=res, W=W, H=H, substeps=S)
    for p in range(pk.batch):
        ref = eh.np_envelope(pk, x, p, fr[p], S, res, W, H)
        und = ref["slack"] < UNDECIDED
        occ = int(ref["union"].sum())
        print("problem", p, "occupied", occ, "undecided", int(und.sum()))
        assert occ > 0
        if allow_undecided:
            assert und.sum() <= UNDECIDED_SHARE * occ, (p, int(und.sum()), occ)   # a condition of the inputs
        else:
            und[...] = False
        bm = out.bitmap(p)
        assert np.array_equal(bm[~und], ref["union"][~und]), (p, int((bm != ref["union"])[~und].sum()))
        assert out.cells[p, -1] == bm.sum()
        for k in range(pk.K):
            lo, hi = int((ref["occ"][k] & ~und).sum()), int((ref["occ"][k] | und).sum())
            assert lo <= out.cells[p, k] <= hi, (p, k, lo, int(out.cells[p, k]), hi)
            if not und.any():
                assert out.cells[p, k] == lo
        assert bool(out.flags[p] & F["CLIPPED"]) == bool(
            out.extent[p, 0] < 0 or out.extent[p, 2] < 0 or out.extent[p, 1] > W * res or out.extent[p, 3] > H * res)
    return out


@pytest.mark.parametrize("seed,batch,N,K,topt,S,res,W,H,phi,edges", [
    (1, 1, 2, 1, True, 1, 0.1, 32, 1, 0.0, None),
    (2, 3, 7, 2, False, 3, 0.2, 64, 48, 0.4, None),
    (3, 2, 33, 2, True, 4, 0.07, 160, 130, -0.2, [5, 3]),
    (4, 1, 80, 2, True, 4, 0.05, 256, 256, 0.0, [4, 8]),
    (5, 2, 20, 4, True, 2, 0.11, 96, 70, 2.9, [3, 4, 6, 8]),
])
def test_raster_matches_the_numpy_restatement(seed, batch, N, K, topt, S, res, W, H, phi, edges):
    near = dict(back=1.0, down=0.05) if H == 1 else {}     # one row of cells: it has to cross the body
    pk, x, fr = eh.envelope_batch(seed, batch, N, K, topt, phi=phi, body_edges=edges, **near)
    _compare_raster(pk, x, fr, S, res, W, H)


def test_a_centre_exactly_on_an_edge_is_covered():
    """Sides at cell-centre coordinates, phi = 0, theta = 0, every number a short binary fraction: n . q - bb is an
    exact 0 on the boundary cells, `<= 0` covers them, and no cell is excluded from the comparison."""
    res = 0.25
    pk, x = _parked(2.125, 1.125, 0.0, [ah.rect(0.0, 0.0, 2.0, 1.0)])
    fr = np.zeros((1, 3))
    ref = eh.np_envelope(pk, x, 0, fr[0], 1, res, 32, 10)
    assert (ref["slack"][ref["union"]] == 0.0).sum() == 2 * 9 + 2 * 5 - 4   # the boundary cells are exact zeros
    out = _compare_raster(pk, x, fr, 1, res, 32, 10, allow_undecided=False)
    want = np.zeros((10, 32), dtype=bool)
    want[2:7, 4:13] = True
    assert np.array_equal(out.bitmap(0), want) and out.cells[0].tolist() == [45, 45] and out.flags[0] == 0


# ------------------------------------------------------------------ areas against geometry
def _area_bound(res, perimeter):
    # the symmetric difference of the region and its cells lies within res / sqrt(2) of the boundary
    return np.sqrt(2.0) * res * perimeter + np.pi * res * res / 2.0


@pytest.mark.parametrize("th", [0.0, 0.3, np.pi / 4, 1.9, -2.6])
def test_area_of_one_rectangle(th):
    w, l, res = 1.3, 2.7, 0.05
    pk, x = _parked(5.03, 4.98, th, [ah.rect(0.0, 0.0, l, w)])
    out = eh.envelope_host(pk, x, np.array([[0.013, -0.021, 0.0]]), res=res, W=224, H=224, substeps=1)
    assert out.flags[0] == 0
    area = out.cells[0, -1] * res * res
    print("heading", th, "area", area, "exact", w * l, "bound", _area_bound(res, 2 * (w + l)))
    assert abs(area - w * l) <= _area_bound(res, 2 * (w + l))


@pytest.mark.parametrize("th,topt", [(0.0, True), (0.7, True), (-2.2, False)])
def test_area_of_a_straight_drive(th, topt):
    w, l, res, N, dT, v = 1.3, 2.7, 0.05, 5, 0.5, 1.0
    L = (N - 1) * dT * v
    s = np.arange(N) * dT * v
    X = np.stack([4.0 + s * np.cos(th), 6.0 + s * np.sin(th), np.full(N, v),
                  np.full(N, th), np.zeros(N)], axis=1)
    pk, x = _one(X, np.zeros((N - 1, 2)), [ah.rect(0.0, 0.0, l, w)], time_opt=topt, dT=dT)
    out = eh.envelope_host(pk, x, np.array([[-0.017, 0.009, 0.0]]), res=res, W=224, H=256, substeps=16)
    assert out.flags[0] == 0, out.extent
    area = out.cells[0, -1] * res * res
    print("heading", th, "area", area, "exact", w * (l + L))
    assert abs(area - w * (l + L)) <= _area_bound(res, 2 * (w + l + L))


# ------------------------------------------------------------------ flags
SQUARE = ah.rect(0.0, 0.0, 1.0, 1.0)


@pytest.mark.parametrize("x0,y0,side", [(0.2, 1.6, 0), (3.1, 1.6, 1), (1.6, 0.3, 2), (1.6, 3.0, 3)])
def test_clipped_on_each_side(x0, y0, side):
    pk, x = _parked(x0, y0, 0.0, [SQUARE])
    out = eh.envelope_host(pk, x, np.zeros((1, 3)), res=0.1, W=32, H=32, substeps=1)
    ext = out.extent[0]
    over = [ext[0] < 0, ext[1] > 3.2, ext[2] < 0, ext[3] > 3.2]
    assert over == [q == side for q in range(4)] and out.flags[0] == F["CLIPPED"]
    assert 0 < out.cells[0, -1] < 100
    inside = eh.envelope_host(*_parked(1.6, 1.6, 0.0, [SQUARE]), np.zeros((1, 3)), res=0.1, W=32, H=32, substeps=1)
    assert inside.flags[0] == 0 and inside.cells[0, -1] == 100


def test_a_body_wholly_outside_the_grid():
    pk, x = _parked(-7.0, 9.0, 0.5, [SQUARE])
    out = eh.envelope_host(pk, x, np.array([[0.0, 0.0, 0.2]]), res=0.1, W=64, H=20, substeps=2)
    assert out.flags[0] == F["CLIPPED"] and out.cells[0].tolist() == [0, 0] and not out.words.any()
    assert np.abs(out.extent[0] - eh.mp_extent(pk, x, 0, [0.0, 0.0, 0.2], 2)).max() <= MP_TOL


def test_a_body_covering_the_whole_grid():
    pk, x = _parked(3.0, 2.0, 0.4, [ah.rect(0.0, 0.0, 30.0, 30.0)])
    out = eh.envelope_host(pk, x, np.array([[0.5, 0.5, -0.3]]), res=0.1, W=64, H=37, substeps=1)
    assert out.flags[0] == F["CLIPPED"] and out.cells[0].tolist() == [64 * 37] * 2
    assert np.all(out.words == 0xFFFFFFFF)


def _three(N=5):
    pk, x, fr = eh.envelope_batch(11, 3, N, 2, True, phi=0.3)
    return pk, x, fr


@pytest.mark.parametrize("source", ["X", "U", "tau", "frame", "body_row", "dT"])
def test_nonfinite(source):
    pk, x, fr = _three()
    good = eh.envelope_host(pk, x, fr, res=0.2, W=64, H=40, substeps=2)
    N = pk.N
    if source == "X":
        x[1, 5 * 2 + 3] = np.inf
    elif source == "U":
        x[1, 5 * N + 3] = np.nan
    elif source == "tau":
        x[1, pk.n_var - 5 - 1] = np.nan
    elif source == "frame":
        fr[1, 2] = np.nan
    elif source == "body_row":
        pk.body_g[1, 5] = -np.inf
    else:
        pk.params[1, _native.P_DT] = np.nan
    out = eh.envelope_host(pk, x, fr, res=0.2, W=64, H=40, substeps=2)
    assert out.flags[1] == F["NONFINITE"]
    assert np.all(np.isnan(out.extent[1])) and np.all(np.isnan(out.extent_body[1])) and np.all(out.where[1] == -1)
    assert not out.cells[1].any() and not out.words[1].any()
    for p in (0, 2):   # the neighbours are untouched
        for n in ("extent", "where", "extent_body", "cells", "flags", "words"):
            assert getattr(out, n)[p].tobytes() == getattr(good, n)[p].tobytes(), (p, n)


def test_values_that_are_not_read_may_be_nan():
    pk, x, fr = _three()
    good = eh.envelope_host(pk, x, fr, res=0.2, W=64, H=40, substeps=2)
    pk.traj[...] = np.nan
    pk.obs_A[...] = np.nan
    pk.params[:, _native.P_DMIN] = np.nan
    out = eh.envelope_host(pk, x, fr, res=0.2, W=64, H=40, substeps=2)
    assert eh.same_bits(out, good) == []


@pytest.mark.parametrize("kind", ["empty", "unbounded"])
def test_bad_polytope(kind):
    pk, x, fr = _three()
    if kind == "empty":        # two opposed rows that exclude each other
        pk.body_G[1, 1] = -pk.body_G[1, 0]
        pk.body_g[1, 1] = -pk.body_g[1, 0] - 1.0
    else:                      # all rows of body 1 face one way
        pk.body_G[1, 4:8] = [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.5]]
    out = eh.envelope_host(pk, x, fr, res=0.2, W=64, H=40, substeps=2)
    assert out.flags.tolist() == [0, F["BAD_POLYTOPE"], 0]
    assert np.all(np.isnan(out.extent[1])) and np.all(out.where[1] == -1)
    assert not out.cells[1].any() and not out.words[1].any() and out.cells[0, -1] > 0


def test_extent_only_writes_neither_cells_nor_bitmap():
    pk, x, fr = _three()
    full = eh.envelope_host(pk, x, fr, res=0.2, W=64, H=40, substeps=2)
    out = eh.envelope_host(pk, x, fr, res=float("nan"), W=0, H=0, substeps=2)    # res is not read
    assert np.all(out.cells == eh.ISENTINEL) and np.all(out.words == eh.WSENTINEL)
    assert out.extent.tobytes() == full.extent.tobytes() and np.array_equal(out.where, full.where)
    assert out.extent_body.tobytes() == full.extent_body.tobytes()
    assert not out.flags.any()                     # CLIPPED needs a grid
    x[2, 0] = np.nan
    out = eh.envelope_host(pk, x, fr, W=0, H=0, substeps=2)
    assert out.flags.tolist() == [0, 0, F["NONFINITE"]] and np.all(out.cells == eh.ISENTINEL)
    assert np.all(out.words == eh.WSENTINEL)


def test_bitmap_may_be_null():
    pk, x, fr = _three()
    full = eh.envelope_host(pk, x, fr, res=0.2, W=64, H=40, substeps=2)
    out = eh.envelope_host(pk, x, fr, res=0.2, W=64, H=40, substeps=2, bitmap=False)
    assert out.words is None and np.array_equal(out.cells, full.cells) and np.array_equal(out.flags, full.flags)


# ------------------------------------------------------------------ the poses are the audit's
@pytest.mark.parametrize("topt,S", [(True, 1), (True, 4), (False, 5)])
def test_same_poses_as_the_audit(topt, S):
    """Against a wall on the +x side the audit's clearance is the wall's offset minus the envelope's umax, and both
    name the same (stage, substep, body): one definition of the pose between two nodes."""
    N = 9
    t = np.linspace(0.0, 1.0, N)
    X = np.stack([3.0 * np.sin(2.0 * t), 2.0 * t, np.full(N, 1.3), 1.6 * (1 - t) - 0.4, 0.5 - t], axis=1)
    U = np.stack([0.3 * np.cos(3 * t[:-1]), 0.4 * np.sin(5 * t[:-1])], axis=1)
    wall = 9.0
    pk = _native.PackedBatch([ah.instance(X, [ah.rect(wall + 50.0, 0.0, 100.0, 400.0)], [BODY, IMPLEMENT],
                                          time_opt=topt, dT=0.4)])
    x = ah.x_of(pk, X[None], U[None], (0.6 + 0.4 * t[:-1])[None] if topt else None, fill=np.nan)
    aud = ah.audit_host(pk, x, substeps=S)
    env = eh.envelope_host(pk, x, np.zeros((1, 3)), substeps=S)
    assert abs(aud.metric("clearance")[0] - (wall - env.extent[0, 1])) <= 1e-12
    assert aud.worst[0, [0, 1, 3]].tolist() == env.where[0, 1].tolist()
    # (N - 1) S + 1 poses: the last index any side can name
    last = eh.envelope_host(*_one(X[::-1].copy(), U, [BODY], time_opt=False), np.array([[0.0, 0.0, np.pi / 2]]), substeps=S)
    assert np.all(last.where[0, :, 0] * S + last.where[0, :, 1] <= (N - 1) * S)


# ------------------------------------------------------------------ the C ABI's argument checks
def _args(W=64, H=40, res=0.2, S=2):
    pk, x, fr = _three()
    out = eh.sentinel_results(pk.batch, pk.K, 64, 40, 0.2, fr)
    return pk, x, fr, _native.envelope_opts(S, res, W, H), out


def _expect_error(b, xp, fp, o, r, word):
    rc, msg = eh.raw_call(b, xp, fp, o, r)
    assert rc == -1 and msg.startswith("[envelope]") and word in msg, (rc, msg)


def test_api_errors():
    pk, x, fr, o, out = _args()
    b, r = pk.struct(), out.struct()
    xp, fp = x.ctypes.data, fr.ctypes.data
    assert eh.raw_call(b, xp, fp, o, r)[0] == 0
    _expect_error(None, xp, fp, o, r, "null")
    _expect_error(b, xp, fp, None, r, "null")
    _expect_error(b, xp, fp, o, None, "null")
    _expect_error(b, None, fp, o, r, "null")
    _expect_error(b, xp, None, o, r, "null")
    for field in ("extent", "where", "flags", "cells"):
        r2 = out.struct()
        setattr(r2, field, None)
        _expect_error(b, xp, fp, o, r2, "null")
    for field in ("body_G", "body_g", "params", "body_edges"):
        b2 = pk.struct()
        setattr(b2, field, None)
        _expect_error(b2, xp, fp, o, r, "null")
    for n, word in ((1, "N must be >= 2"), (_native.ENVELOPE_MAX_N + 1, "HTP_ENVELOPE_MAX_N")):
        b2 = pk.struct()
        b2.N = n
        _expect_error(b2, xp, fp, o, r, word)
    for s in (0, _native.AUDIT_MAX_SUBSTEPS + 1):
        _expect_error(b, xp, fp, _native.envelope_opts(s, 0.2, 64, 40), r, "substeps")
    for e in (2, 9):
        edges = (ctypes.c_int32 * pk.K)(*([4] * (pk.K - 1) + [e]))
        b2 = pk.struct()
        b2.body_edges = ctypes.cast(edges, ctypes.c_void_p).value
        _expect_error(b2, xp, fp, o, r, "body edges")
    for res in (0.0, -0.1, float("nan"), float("inf")):
        _expect_error(b, xp, fp, _native.envelope_opts(2, res, 64, 40), r, "res")
    _expect_error(b, xp, fp, _native.envelope_opts(2, 0.2, 48, 40), r, "multiple of 32")
    _expect_error(b, xp, fp, _native.envelope_opts(2, 0.2, 256, 257), r, "65536")
    _expect_error(b, xp, fp, _native.envelope_opts(2, 0.2, 65536, 65536), r, "65536")
    _expect_error(b, xp, fp, _native.envelope_opts(2, 0.2, 64, 0), r, "both")
    _expect_error(b, xp, fp, _native.envelope_opts(2, 0.2, 0, 40), r, "both")
    _expect_error(b, xp, fp, _native.envelope_opts(2, 0.2, -32, -2), r, ">= 0")
    # nothing was written by a refused call
    fresh = eh.sentinel_results(pk.batch, pk.K, 64, 40, 0.2, fr)
    _expect_error(b, xp, fp, _native.envelope_opts(0, 0.2, 64, 40), fresh.struct(), "substeps")
    assert np.all(fresh.extent == eh.SENTINEL) and np.all(fresh.flags == eh.ISENTINEL)
    # the largest grid and the extent-only mode without cells are accepted
    assert eh.raw_call(b, xp, fp, _native.envelope_opts(2, 0.2, 0, 0), r)[0] == 0
    r2 = out.struct()
    r2.cells = None
    r2.bitmap = None
    assert eh.raw_call(b, xp, fp, _native.envelope_opts(2, 0.2, 0, 0), r2)[0] == 0


def test_empty_batch_returns_zero():
    pk, x, fr, o, out = _args()
    b = pk.struct()
    b.batch = 0
    assert eh.raw_call(b, None, None, o, out.struct()) == (0, "")
    assert np.all(out.flags == eh.ISENTINEL)


def test_largest_horizon_and_grid():
    pk, x, fr = eh.envelope_batch(21, 1, _native.ENVELOPE_MAX_N, 2, True)
    out = eh.envelope_host(pk, x, fr, res=0.06, W=256, H=256, substeps=2)
    assert out.flags[0] in (0, F["CLIPPED"]) and out.cells[0, -1] > 1000
    assert out.cells[0, -1] == out.bitmap(0).sum()


# ------------------------------------------------------------------ the Python layer's default frame
def test_default_frame_covers_the_swept_region():
    pk, x, _ = eh.envelope_batch(31, 3, 12, 2, True)
    res = 0.1
    frames, W, H = _native.envelope_default_frame(pk, x, res)
    assert W % 32 == 0 and W * H <= _native.ENVELOPE_MAX_CELLS and np.all(frames[:, 2] == 0.0)
    pad = _native.body_radius(pk) + res
    X = x[:, :5 * pk.N].reshape(3, pk.N, 5)
    assert np.allclose(frames[:, :2], X[:, :, :2].min(axis=1) - pad)
    span = (X[:, :, :2].max(axis=1) + pad - frames[:, :2]).max(axis=0)
    assert (W - 32) * res < span[0] <= W * res and (H - 1) * res < span[1] <= H * res   # the smallest admissible
    out = eh.envelope_host(pk, x, frames, res=res, W=W, H=H, substeps=1)
    assert not out.flags.any()                       # the nodes' poses lie inside: nothing is clipped
    bodies = eh.body_polys(pk, 0)
    assert abs(_native.body_radius(pk) - max(np.hypot(v[:, 0], v[:, 1]).max() for _, _, v in bodies)) <= 1e-6


def test_default_frame_names_a_coarser_res():
    pk, x, _ = eh.envelope_batch(31, 2, 12, 1, True)
    with pytest.raises(ValueError, match="coarser res"):
        _native.envelope_default_frame(pk, x, 0.01)
    with pytest.raises(ValueError, match="res must be finite"):
        _native.envelope_default_frame(pk, x, 0.0)


def test_results_bitmap_unpacks_bit_b_of_word_w():
    r = _native.EnvelopeResults(1, 1, 64, 3, 0.5)
    r.words[0, 1, 1] = (1 << 5) | (1 << 31)
    r.words[0, 2, 0] = 1
    bm = r.bitmap(0)
    assert bm.shape == (3, 64) and bm.dtype == bool
    assert sorted(zip(*np.nonzero(bm))) == [(1, 37), (1, 63), (2, 0)]
    r.cells[0] = [3, 3]
    d = r.as_dict(0)
    assert d["area"] == 0.75 and d["bitmap"].sum() == 3 and d["flags"] == []


# ------------------------------------------------------------------ sanitizer build
def test_host_core_under_asan_ubsan():
    """csrc/envelope_asan.cpp: a stand-alone executable (its own main) of the host build, over the shapes of the
    GPU test and the widest and tallest grids; any access beyond a buffer or undefined behaviour aborts it."""
    exe = eh.build_asan()
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert p.stdout.count(": ok") == 7, p.stdout

"""GPU tests of the SHOT local reference frames and descriptors (mvr_cloud_shot_lrf, mvr_cloud_shot, mvr_cloud_shot_at; rules
L1-L7 and H1-H9 in include/mvr_hip.h) against the numpy reference of tests/shot_ref.py on the cases of tests/shot_cases.py.

Frames are compared with the reference's own (numpy's eigh) where the reference says they are well conditioned -- eigen-gap >=
1e-3 and both sign votes decided; an undecided axis is compared up to its sign -- to one ulp of 1 in f32 (2^-23): the bar is
1e-8 before the rounding to f32, from n 2^-52 relative error of the covariance over a gap of 1e-3 at n <= 2 000.  The
descriptor is compared as the fixed-point SUMS the call returns, against the reference fed the GPU's own f32 frames: the two then
differ by the roundings of f64 libm calls (acos, atan2) and of the amounts alone, and a misplaced amount would move 0.1 to 1.
The rows are compared as the BITS of rule H8 on the returned sums.

Measured on an MI355X (profiles/shot_pytest_gpu.log, this file's own prints), |S_gpu - S_ref| per slot in amounts (2^32 units)
per neighbour of the query: 0 on the rows, the long row, the small clouds and the lattice under identity frames (12 000
neighbours on the z axis), one unit of 2^-32 in 1 to 7 slots of 258 396 to 808 589 on the view, the box, the skewed cloud and the
view with invalid points: worst 1.45e-12 (MEASURED_WORST); shot_cases.SUMS_BAR is 16 times that, rounded up to a power of ten, 1e-10.
Frames: no component off by more than an ulp of 1 on 4 949 / 2 974 / 1 471 fully compared queries, worst |f32 - f64| 2.98e-08 (the
rounding to f32); the same frame bits at every grid resolution on the box and the patch."""
import ctypes as C
import importlib

import numpy as np
import pytest

import pfh_cases as PC
import shot_cases as SC
import shot_ref as SR
from conftest import PKG

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ULP1 = 2.0 ** -23
MEASURED_WORST = 1.45e-12      # one unit of 2^-32 in one slot (the view with invalid points); 16 x -> 2.3e-11 -> SUMS_BAR = 1e-10


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F32 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def all_same(x, y):
    return all(same_bits(a, b) for a, b in zip(x, y))


def run(ctx, p, nrm, R, slot=0, **kw):
    """(rows, frames, sums, neighbor_count) of the self call"""
    ctx.upload(slot, p)
    if len(p):
        ctx.upload_normals(slot, nrm)
    out = ctx.shot(slot, R, return_lrf=True, return_sums=True, return_neighbors=True, **kw)
    assert out[0].shape == out[2].shape == (len(p), 352) and out[1].shape == (len(p), 9) and out[3].shape == (len(p),)
    assert out[2].dtype == np.uint64
    return out


_inputs, _gpu = {}, {}


def inputs(name, mvr, ctx):
    if name in _inputs:
        return _inputs[name]
    if name in ("view", "invalid", "patch"):
        base = "patch" if name == "patch" else "view"
        if base not in _inputs:
            p, _, R = SC.patch(mvr) if base == "patch" else SC.view(mvr)
            ctx.upload(2, p)
            ctx.estimate_normals(2, radius=PC.patch_normal_radius(p) if base == "patch" else SC.NORMAL_RADIUS)
            _inputs[base] = (p, ctx.download_normals(2), R)
        if name == "invalid":
            p, nrm, R = _inputs["view"]
            q, m, bad = SC.with_invalid(p, nrm)
            _inputs["invalid"] = (q, m, R)
    elif name == "long_row":
        _inputs[name] = SC.long_row(mvr)
    elif name.startswith("row_"):
        _inputs[name] = SC.row(int(name[4:]))
    else:
        _inputs[name] = getattr(SC, name)()
    return _inputs[name]


def gpu(name, mvr, ctx):
    if name not in _gpu:
        _gpu[name] = run(ctx, *inputs(name, mvr, ctx))
    return _gpu[name]


def valid_points(p, nrm):
    return np.isfinite(p[:, :3]).all(1) & np.isfinite(nrm[:, :3]).all(1)


def orthonormal(fr):
    """every finite frame: unit axes, orthogonal, right-handed, to 1e-6 in f32"""
    A = fr[np.isfinite(fr).all(1)].astype(F64).reshape(-1, 3, 3)
    G = A @ A.transpose(0, 2, 1)
    assert np.abs(G - np.eye(3)).max() <= 1e-6
    assert np.abs(np.cross(A[:, 2], A[:, 0]) - A[:, 1]).max() <= 1e-6      # y = z x x


def sums_close(name, p, nrm, q, R, got, valid_q, fma=False):
    """the comparison of the module docstring for the queries q (rows of `got`); returns the worst figure"""
    rows, fr, S, nb = got
    ref, n, contributors, on_axis = SR.sums(p, nrm, q, fr, R, fma=fma)
    n = np.where(valid_q, n, 0)
    ref[~valid_q] = 0
    assert np.array_equal(nb.astype(np.int64), n)
    few = n < SR.MIN_NEIGHBORS
    assert (S[few] == 0).all()
    ref[few] = 0
    diff = np.abs(S.astype(np.int64) - ref.astype(np.int64))
    per = diff.max(1) / SR.ONE / np.maximum(n, 1)
    worst = float(per.max()) if len(per) else 0.0
    print("%s: %d queries, %.1f neighbours (max %d), %d on the frame's z axis; |S_gpu - S_ref| per slot: worst %d units of 2^-32, worst per "
          "neighbour %.3g, slots that differ %d of %d" % (name, len(q), n.mean() if len(n) else 0, n.max() if len(n) else 0, int(on_axis.sum()),
                                                         int(diff.max()) if diff.size else 0, worst, int((diff > 0).sum()), int((ref > 0).sum())))
    assert worst <= SC.SUMS_BAR
    assert same_bits(rows, SR.rows_from_sums(S, nb, valid_q & np.isfinite(fr).all(1)))      # H8
    return worst


# ------------------------------------------------------------------ frames

@pytest.mark.parametrize("name", SC.FRAME_CASES)
def test_frames_against_the_reference(name, mvr, ctx):
    p, nrm, _ = inputs(name, mvr, ctx)
    R = SC.FRAME_RADIUS[name]
    ctx.upload(0, p)                                                       # no normals: a frame needs none
    fr, nl = ctx.shot_lrf(0, R, return_neighbors=True)
    ref = SR.frames(p, p, R)
    assert np.array_equal(nl.astype(np.int64), ref["n"])
    assert np.array_equal(np.isfinite(fr).all(1), ref["ok"]) and np.isnan(fr[~ref["ok"]]).all()
    orthonormal(fr)
    ok = ref["ok"] & (ref["gap"] >= SC.GAP)
    decided = SC.decided(ref)
    full = ok & decided.all(1)
    assert full.mean() >= SC.FRAME_SHARE
    g = fr.astype(F64).reshape(-1, 3, 3)
    want = ref["axes"].astype(F32).astype(F64)
    worst, checks = 0.0, []
    for c, axis in enumerate((0, 2)):                                      # x and z: as they are where the vote is decided, else up to sign
        d = np.abs(g[:, axis] - want[:, axis]).max(1)
        flip = np.abs(g[:, axis] + want[:, axis]).max(1)
        checks += [d[ok & decided[:, c]], np.minimum(d, flip)[ok & ~decided[:, c]]]
        worst = max(worst, float(np.abs(g[:, axis] - ref["axes"][:, axis])[ok & decided[:, c]].max()))
    checks.append(np.abs(g[:, 1] - want[:, 1]).max(1)[full])
    print("%s: %d frames, %d NaN, %d with gap >= %g, %d fully compared (%.3f), %d votes undecided; worst |f32 axis - f64 reference| %.3g; "
          "components off by more than an ulp of 1: %s" % (name, len(p), int((~ref["ok"]).sum()), int(ok.sum()), SC.GAP, int(full.sum()), full.mean(),
                                                        int((ok[:, None] & ~decided).sum()), worst, [int((c > ULP1).sum()) for c in checks]))
    assert all((c <= ULP1).all() for c in checks)
    again = ctx.shot_lrf(0, R)                                             # L7: bit-identical run to run
    assert same_bits(fr, again)


def test_lattice_frames_are_orthonormal_and_follow_the_vote(mvr, ctx):
    """cubic symmetry: three equal eigenvalues, any orthonormal basis is an eigenbasis -- the frame must still be one (L4), and
    its signs must follow L5 on its OWN axes"""
    p, nrm, R = inputs("lattice", mvr, ctx)
    ctx.upload(0, p)
    fr, nl = ctx.shot_lrf(0, R, return_neighbors=True)
    assert np.isfinite(fr).all() and (nl >= 8).all()
    orthonormal(fr)
    qi, pj = SR.pairs(p, p, R, np.ones(len(p), bool))
    qi, pj = qi[qi != pj], pj[qi != pj]                                      # (L2: not the query's own point)
    v = p[pj, :3].astype(F64) - p[qi, :3].astype(F64)
    for axis in (0, 2):
        a = fr.astype(F64).reshape(-1, 3, 3)[qi, axis]
        dots = (v[:, 0] * a[:, 0] + v[:, 1] * a[:, 1]) + v[:, 2] * a[:, 2]
        plus = np.bincount(qi, weights=dots >= 0, minlength=len(p))
        near = np.bincount(qi, weights=np.abs(dots) <= 1e-9 * np.linalg.norm(v, axis=1), minlength=len(p))
        assert (2 * plus + near >= nl).all()                               # never against a decided majority


def test_a_tie_of_the_vote_is_decided_by_the_weighted_sum(mvr, ctx):
    p, nrm, q, R = SC.tie()
    ref = SR.frames(p, q, R)
    assert (ref["margin"][0] == 0).all()                                   # (tests/test_shot_host.py: and the sums decide)
    ctx.upload(0, p); ctx.upload_normals(0, nrm)
    ctx.upload(9, q)
    rows, fr, nb = ctx.shot_at(9, 0, R, return_lrf=True, return_neighbors=True)
    assert nb[0] == len(p) and np.isfinite(rows).all()
    assert np.abs(fr[0].astype(F64) - ref["axes"][0].reshape(9).astype(F32).astype(F64)).max() <= ULP1
    print("tie: plus == n / 2 on both axes; tie sums %s; the frame is the reference's to %.3g"
          % (ref["tie_s"][0], np.abs(fr[0].astype(F64) - ref["axes"][0].reshape(9)).max()))


# ------------------------------------------------------------------ sums and rows

SUM_CASES = ["view", "box", "skew", "invalid", "long_row"] + ["row_%d" % n for n in SC.ROW_SIZES]


@pytest.mark.parametrize("name", SUM_CASES)
def test_sums_against_the_reference_fed_the_gpus_frames(name, mvr, ctx):
    p, nrm, R = inputs(name, mvr, ctx)
    got = gpu(name, mvr, ctx)
    valid = valid_points(p, nrm)
    sums_close(name, p, nrm, p, R, got, valid)
    rows, fr, S, nb = got
    assert np.isnan(rows[~valid]).all() and (nb[~valid] == 0).all() and np.isnan(fr[~valid]).all()
    if name.startswith("row_"):
        n = int(name[4:])
        assert (nb == (n if n >= 6 else 0)).all() and np.isfinite(rows).all() == (n >= 6)      # (fewer than 5 OTHER points: a NaN frame, count 0: H1)
    if name in ("view", "box", "skew"):
        assert (nb[valid & np.isfinite(fr).all(1)] >= 5).all() and np.isfinite(rows[nb >= 5]).all() and (S > 0).sum() > 50 * len(p)
        norm = np.linalg.norm(rows[nb >= 5].astype(F64), axis=1)
        assert np.abs(norm - 1.0).max() < 1e-6
    if name == "box":
        assert ((S > 0).any(0)).all()                                      # every one of the 352 slots is reached


def test_neighbours_on_the_axis_and_on_every_border(mvr, ctx):
    """the lattice under identity frames: acos(+-1), x == y == 0, |x| == |y|, d == R / 2, z == 0, all exact"""
    p, nrm, R = inputs("lattice", mvr, ctx)
    got = run(ctx, p, nrm, R, lrf=SC.identity_frames(len(p)))
    assert same_bits(got[1], SC.identity_frames(len(p)))
    sums_close("lattice", p, nrm, p, R, got, np.ones(len(p), bool))


def test_fma_distance(mvr, ctx):
    p, nrm, R = inputs("skew", mvr, ctx)
    got = run(ctx, p, nrm, R, fma=True)
    sums_close("skew, fma distance", p, nrm, p, R, got, np.ones(len(p), bool), fma=True)


@pytest.mark.parametrize("n", (4, 5, 6, 7))
def test_neighbourhoods_of_four_five_and_six(n, mvr, ctx):
    """n points, everybody everybody's neighbour: a frame sees the n - 1 OTHER points (L2: 4, 5 and 6 of them at n = 5, 6, 7), a row
    all n (H2: 4, 5 and 6 at n = 4, 5, 6, with frames passed in)"""
    p, nrm, R = SC.small(n)
    rows, fr, S, nb = run(ctx, p, nrm, R, slot=4)
    lone, nl = ctx.shot_lrf(4, R, return_neighbors=True)
    framed = n - 1 >= 5
    assert (nl == n - 1).all() and same_bits(lone, fr) and (nb == (n if framed else 0)).all()      # (a NaN frame: count 0, H1)
    assert np.isfinite(fr).all() == framed and np.isfinite(rows).all() == framed
    if not framed:
        assert np.isnan(fr).all() and np.isnan(rows).all() and (S == 0).all()
    else:
        orthonormal(fr)
        sums_close("small_%d" % n, p, nrm, p, R, (rows, fr, S, nb), np.ones(n, bool))
    # frames passed in: the descriptor's own rule n_i < 5 (H2), whatever the frame
    got = run(ctx, p, nrm, R, slot=4, lrf=SC.identity_frames(n))
    assert np.isfinite(got[0]).all() == (n >= 5) and (got[3] == n).all()
    sums_close("small_%d, identity frames" % n, p, nrm, p, R, got, np.ones(n, bool))


def test_a_query_with_only_copies_of_itself(mvr, ctx):
    p, nrm, R = SC.copies()
    rows, fr, S, nb = run(ctx, p, nrm, R, slot=4)
    lone, nl = ctx.shot_lrf(4, R, return_neighbors=True)
    assert (nl == 0).all() and np.isnan(fr).all() and np.isnan(rows).all() and (nb == 0).all()      # L2: no OTHER point
    rows, fr, S, nb = run(ctx, p, nrm, R, slot=4, lrf=SC.identity_frames(len(p)))
    assert (nb == len(p)).all() and (S == 0).all() and np.isnan(rows).all()                       # H2 / H8: d == 0 adds nothing, norm == 0


# ------------------------------------------------------------------ order freedom

@pytest.mark.parametrize("name", ["box", "patch"])
def test_sums_do_not_depend_on_grid_or_run(name, mvr, ctx):
    p, nrm, R = inputs(name, mvr, ctx)
    base = gpu(name, mvr, ctx)
    again = run(ctx, p, nrm, R, slot=0)
    assert all_same(base, again)                                           # without lrf_in: run to run, frames included
    fed = run(ctx, p, nrm, R, slot=3, lrf=base[1])                         # L6: its own frames passed in
    assert all_same(base, fed)
    ctx.upload(3, p); ctx.upload_normals(3, nrm)
    assert same_bits(ctx.shot(3, R), base[0])                              # the optional outputs change nothing
    try:
        for cp in SC.CELL_POINTS:
            ctx.tune(seq_cell_points=cp)
            got = run(ctx, p, nrm, R, slot=7, lrf=base[1])
            assert all_same(base, got), (name, cp)
            own = run(ctx, p, nrm, R, slot=7)                              # frames of another grid: equal to rounding
            both = np.isfinite(own[1]).all(1) & np.isfinite(base[1]).all(1)
            assert np.array_equal(own[3], base[3]) and np.array_equal(np.isfinite(own[1]).all(1), np.isfinite(base[1]).all(1))
            print("%s seq_cell_points=%d: the bits of the base with its frames passed in; own frames differ by at most %.3g"
                  % (name, cp, np.abs(own[1][both] - base[1][both]).max()))
    finally:
        ctx.tune(seq_cell_points=4)


@pytest.mark.parametrize("far", PC.PATCH_FARS)
def test_far_frames(far, mvr, ctx):
    p, nrm, R = inputs("patch", mvr, ctx)
    base = gpu("patch", mvr, ctx)
    q = PC.patch_moved(p, far)                                             # every coordinate an exact translation
    got = run(ctx, q, nrm, R, slot=5, lrf=base[1])
    assert all_same(base, got)
    print("patch %g mm from the origin: %d rows, the bits of the patch at the origin (frames passed in)" % (far, len(q)))


def test_lrf_radius_other_than_the_radius(mvr, ctx):
    p, nrm, R = inputs("box", mvr, ctx)
    Rl = 0.7 * R
    got = run(ctx, p, nrm, R, slot=3, lrf_radius=Rl)
    lone, nl = ctx.shot_lrf(3, Rl, return_neighbors=True)
    assert same_bits(got[1], lone) and not same_bits(got[1], gpu("box", mvr, ctx)[1])
    assert np.array_equal(got[3], gpu("box", mvr, ctx)[3]) and not np.array_equal(nl, got[3])
    sums_close("box, lrf_radius 0.7 R", p, nrm, p, R, got, np.ones(len(p), bool))
    ref = SR.frames(p, p, Rl)
    assert np.array_equal(nl.astype(np.int64), ref["n"])


def test_invalid_points_and_nan_frames(mvr, ctx):
    p, nrm, R = inputs("invalid", mvr, ctx)
    rows, fr, S, nb = gpu("invalid", mvr, ctx)
    valid = valid_points(p, nrm)
    assert (~valid).sum() > 20 and np.isnan(rows[~valid]).all() and (nb[~valid] == 0).all() and (S[~valid] == 0).all()
    g = run(ctx, p[valid], nrm[valid], R, slot=5, lrf=fr[valid])           # as if removed: the same frames, the same sums
    assert same_bits(g[0], rows[valid]) and np.array_equal(g[2], S[valid]) and np.array_equal(g[3], nb[valid])
    # a frame needs no normal: the frames alone, over the same points, see the points with a NaN normal
    ctx.upload(6, p)
    lone, nl = ctx.shot_lrf(6, R, return_neighbors=True)
    coords = np.isfinite(p[:, :3]).all(1)
    assert np.isfinite(lone[coords]).all() and np.isnan(lone[~coords]).all() and (nl[~coords] == 0).all()
    # a NaN row among the frames passed in
    f2 = fr.copy()
    pick = np.nonzero(valid)[0][[3, 700]]
    f2[pick[0], 4] = np.nan
    f2[pick[1]] = np.nan
    h = run(ctx, p, nrm, R, slot=5, lrf=f2)
    assert np.isnan(h[0][pick]).all() and (h[3][pick] == 0).all() and (h[2][pick] == 0).all() and same_bits(h[1], f2)
    keep = np.ones(len(p), bool); keep[pick] = False
    assert same_bits(h[0][keep], rows[keep]) and np.array_equal(h[2][keep], S[keep])


# ------------------------------------------------------------------ _at

def at(ctx, q_slot, s_slot, R, **kw):
    return ctx.shot_at(q_slot, s_slot, R, return_lrf=True, return_sums=True, return_neighbors=True, **kw)


def test_at_gives_the_bits_of_the_self_call(mvr, ctx):
    p, nrm, R = inputs("box", mvr, ctx)
    base = gpu("box", mvr, ctx)
    ctx.upload(0, p); ctx.upload_normals(0, nrm)
    idx = SC.at_indices(len(p))
    assert (np.diff(idx.astype(np.int64)) < 0).any() and len(np.unique(idx)) < len(idx)
    got = at(ctx, 0, 0, R, indices=idx)                                    # Q5 through indices: unsorted, repeated
    assert all_same([b[idx] for b in base], got)
    ctx.upload(9, p[idx])                                                  # Q5 through a copy in another slot (positions only)
    copy = at(ctx, 9, 0, R)
    assert all_same(got, copy)
    assert all_same(base, at(ctx, 0, 0, R))                                # Q8: the existing call
    fed = at(ctx, 9, 0, R, lrf=got[1])                                     # frames passed in, by row
    assert all_same(got, fed)
    try:
        ctx.tune(at_sort=0)
        assert all_same(got, at(ctx, 9, 0, R)) and all_same(got, at(ctx, 0, 0, R, indices=idx))
    finally:
        ctx.tune(at_sort=1)
    # a query off the surface, a non-finite query
    q = np.array([[500.0, 500.0, 500.0, 1.0], [np.nan, 0.0, 917.0, 1.0], p[7]], F32)
    ctx.upload(9, q)
    rows, fr, S, nb = at(ctx, 9, 0, R)
    assert list(nb) == [0, 0, base[3][7]] and np.isnan(rows[:2]).all() and np.isnan(fr[:2]).all() and (S[:2] == 0).all()
    assert same_bits(rows[2], base[0][7]) and same_bits(fr[2], base[1][7])
    # an empty surface, an empty query set
    ctx.upload(8, p[:0])
    rows, fr, S, nb = at(ctx, 9, 8, R)
    assert rows.shape == (3, 352) and np.isnan(rows).all() and np.isnan(fr).all() and (nb == 0).all()
    assert at(ctx, 8, 0, R)[0].shape == (0, 352) and at(ctx, 0, 0, R, indices=np.zeros(0, np.uint32))[0].shape == (0, 352)
    # an index out of range
    with pytest.raises(mvr.MvrError):
        at(ctx, 0, 0, R, indices=np.array([0, len(p)], np.uint32))
    assert same_bits(p, ctx.download(0)) and same_bits(nrm, ctx.download_normals(0))      # the slots are not modified


# ------------------------------------------------------------------ H9

def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def raw(mvr, ctx, slot, R, Rl, out, lrf, sums, nb, fma=0, lrf_in=None):
    prm = mvr.ShotParams(R, Rl, fma)
    return mvr._lib.mvr_cloud_shot(ctx._h, slot, C.byref(prm), ptr(lrf_in, C.c_float), ptr(out, C.c_float), ptr(lrf, C.c_float),
                                   ptr(sums, C.c_uint64), ptr(nb, C.c_uint32))


def test_refusals_with_nothing_written(mvr, ctx):
    p, nrm, R = SC.small(6)
    n = len(p)
    ctx.upload(5, p)                                                       # a new upload drops the normals
    out, lrf, sums, nb = np.full((n, 352), 9.0, F32), np.full((n, 9), 9.0, F32), np.full((n, 352), 9, np.uint64), np.full(n, 9, np.uint32)
    untouched = lambda: (out == 9.0).all() and (lrf == 9.0).all() and (sums == 9).all() and (nb == 9).all()
    assert raw(mvr, ctx, 5, R, 0.0, out, lrf, sums, nb) == mvr.E_ARG and untouched()      # no normals
    with pytest.raises(mvr.MvrError):
        ctx.shot(5, R)
    prm = mvr.ShotParams(R, 0.0, 0)
    assert mvr._lib.mvr_cloud_shot_lrf(ctx._h, 5, C.byref(prm), ptr(lrf, C.c_float), ptr(nb, C.c_uint32)) == mvr.OK      # frames need none
    assert np.isfinite(lrf).all() and (nb == n - 1).all()
    lrf[:] = 9.0; nb[:] = 9
    ctx.upload_normals(5, nrm)
    for r, rl in ((0.0, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (R, -1.0), (R, float("nan")), (R, float("inf"))):
        assert raw(mvr, ctx, 5, r, rl, out, lrf, sums, nb) == mvr.E_ARG and untouched(), (r, rl)
        prm = mvr.ShotParams(r, rl, 0)
        assert mvr._lib.mvr_cloud_shot_lrf(ctx._h, 5, C.byref(prm), ptr(lrf, C.c_float), ptr(nb, C.c_uint32)) == mvr.E_ARG and untouched()
        assert mvr._lib.mvr_cloud_shot_at(ctx._h, 5, None, 0, 5, C.byref(prm), None, ptr(out, C.c_float), ptr(lrf, C.c_float),
                                          ptr(sums, C.c_uint64), ptr(nb, C.c_uint32)) == mvr.E_ARG and untouched()
    assert raw(mvr, ctx, mvr.MAX_SLOTS, R, 0.0, out, lrf, sums, nb) == mvr.E_ARG and untouched()
    assert mvr._lib.mvr_cloud_shot(ctx._h, 5, None, None, ptr(out, C.c_float), None, None, None) == mvr.E_ARG and untouched()
    prm = mvr.ShotParams(R, 0.0, 0)
    bad = np.array([0, n], np.uint32)
    assert mvr._lib.mvr_cloud_shot_at(ctx._h, 5, ptr(bad, C.c_uint32), 2, 5, C.byref(prm), None, ptr(out, C.c_float), ptr(lrf, C.c_float),
                                      ptr(sums, C.c_uint64), ptr(nb, C.c_uint32)) == mvr.E_ARG and untouched()
    ctx.upload(6, p)                                                       # a surface without normals
    assert mvr._lib.mvr_cloud_shot_at(ctx._h, 5, None, 0, 6, C.byref(prm), None, ptr(out, C.c_float), ptr(lrf, C.c_float),
                                      ptr(sums, C.c_uint64), ptr(nb, C.c_uint32)) == mvr.E_ARG and untouched()
    assert raw(mvr, ctx, 5, R, 0.0, None, None, None, None) == mvr.OK      # all outputs NULL: the work, no copy
    assert raw(mvr, ctx, 5, R, 0.0, out, lrf, sums, nb) == mvr.OK and np.isfinite(out).all() and (nb == n).all()
    ctx.upload(5, p[:0])
    assert ctx.shot(5, R).shape == (0, 352) and ctx.shot_lrf(5, R).shape == (0, 9)      # an empty cloud is MVR_OK

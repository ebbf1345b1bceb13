"""GPU tests of mvr_pose_scores (rules S1-S2 in include/mvr_hip.h) against an anchor that passes through no new code: per pose
ctx.transform_f32 into a spare slot, ctx.nn against the target, the count of (double)d2 < max_dist^2 and math.fsum of those d2
divided by the count.  Inliers must be equal; the error within n * 2^-52 relative -- the bound of an f64 sum of n positive
terms added in any order (each of the n - 1 additions rounds by at most 2^-53 of a partial sum that never exceeds the total)."""
import importlib
import math

import numpy as np
import pytest

import align_cases as AC
from conftest import PKG

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DBL_MAX = np.finfo(F64).max
SRC, TGT, SPARE = 0, 1, 2


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def anchor(ctx, src, tgt, poses, max_dist, fma=False, spare=SPARE):
    """(inliers, error, d2 per pose) of the poses of slot src against slot tgt by transform_f32 + nn"""
    inl, err, all_d2 = [], [], []
    for T in poses:
        ctx.transform_f32(spare, src, T)
        _, d2 = ctx.nn(spare, tgt, fma=fma)
        d = d2.astype(F64)
        d = d[d < F64(max_dist) * F64(max_dist)]
        inl.append(len(d))
        err.append(math.fsum(d) / len(d) if len(d) else DBL_MAX)
        all_d2.append(d2)
    return np.array(inl, np.uint32), np.array(err), all_d2


def check(got, want, n):
    gi, ge = got
    wi, we = want[:2]
    assert np.array_equal(gi, wi), (gi, wi)
    none = wi == 0
    assert (ge[none] == DBL_MAX).all()
    rel = np.abs(ge[~none] - we[~none]) / we[~none]
    print("largest relative error of the mean: %.3g (bound %.3g)" % (rel.max() if len(rel) else 0.0, n * 2.0 ** -52))
    assert (rel <= n * 2.0 ** -52).all()


@pytest.fixture(scope="module")
def scene(ctx):
    s, t = AC.score_clouds()
    ctx.upload(SRC, s)
    ctx.upload(TGT, t)
    return s, t, AC.score_poses()


@pytest.mark.parametrize("fma", [False, True])
def test_37_poses_against_the_anchor(fma, ctx, scene):
    s, t, P = scene
    assert len(P) == 37
    want = anchor(ctx, SRC, TGT, P, AC.SCORE_MAX_DIST, fma)
    got = ctx.pose_scores(SRC, TGT, P, AC.SCORE_MAX_DIST, fma=fma)
    check(got, want, len(s))
    # the strict <: under `z + 2` the lattice points lie exactly at max_dist and are not inliers; one float nearer they are
    at = want[2][AC.SCORE_STRICT_POSE] == F32(AC.SCORE_MAX_DIST * AC.SCORE_MAX_DIST)
    assert at.sum() == AC.SCORE_LATTICE == len(s) // 5
    assert got[0][AC.SCORE_INSIDE_POSE] - got[0][AC.SCORE_STRICT_POSE] >= AC.SCORE_LATTICE * 0.9
    assert got[0][0] > 0.9 * len(s) and (got[0][3:7] == 0).all() and (got[1][3:7] == DBL_MAX).all()      # identity; far outside
    assert np.array_equal(ctx.download(SRC), s) and np.array_equal(ctx.download(TGT), t)               # neither slot is modified


def test_chunks_do_not_change_a_bit(ctx, scene):
    s, t, P = scene
    base = ctx.pose_scores(SRC, TGT, P, AC.SCORE_MAX_DIST)
    try:
        for chunk in (1, 5, 16, 36, 37, 1000):      # 37 poses: eight launches of five at most, three of sixteen, ...
            ctx.tune(score_chunk=chunk)
            got = ctx.pose_scores(SRC, TGT, P, AC.SCORE_MAX_DIST)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.uint64), base[1].view(np.uint64)), chunk
    finally:
        ctx.tune(score_chunk=256)
    again = ctx.pose_scores(SRC, TGT, P, AC.SCORE_MAX_DIST)
    assert np.array_equal(again[1].view(np.uint64), base[1].view(np.uint64))


def test_results_do_not_depend_on_the_grid_resolution(ctx, scene):
    """seq_cell_points 4 (the default), 1, 64 and 4096 change the cell edge of every grid built afterwards; source and target
    are uploaded again after each tune (the source's grid gives the blocks their points, the target's is walked).  The inliers
    are identical; the block sums follow the source's grid order, so the error is held to the anchor at each resolution"""
    s, t, P = scene
    want = anchor(ctx, SRC, TGT, P, AC.SCORE_MAX_DIST)
    try:
        base = None
        for cp in (4, 1, 64, 4096):
            ctx.tune(seq_cell_points=cp)
            ctx.upload(SRC, s)
            ctx.upload(TGT, t)
            got = ctx.pose_scores(SRC, TGT, P, AC.SCORE_MAX_DIST)
            if base is None:
                base = got
            assert np.array_equal(got[0], base[0]), cp
            check(got, want, len(s))
            print("seq_cell_points=%d: %d of %d errors differ in a bit from the default resolution's"
                  % (cp, int((got[1].view(np.uint64) != base[1].view(np.uint64)).sum()), len(P)))
    finally:
        ctx.tune(seq_cell_points=4)
        ctx.upload(SRC, s)
        ctx.upload(TGT, t)


def test_non_finite_source_points_are_no_inliers(ctx, scene, mvr):
    s, t, P = scene
    import mls_cases as K
    bad_s, bad = K.with_non_finite(s)
    ctx.upload(3, bad_s)
    ctx.upload(4, bad_s[np.isfinite(bad_s[:, :3]).all(1)])      # the anchor runs on the finite points: mvr_nn has no rule for the others
    want = anchor(ctx, 4, TGT, P[:12], AC.SCORE_MAX_DIST)
    got = ctx.pose_scores(3, TGT, P[:12], AC.SCORE_MAX_DIST)
    check(got, want, len(s))
    nan_pose = P[7].copy(); nan_pose[1, 2] = np.nan
    inf_pose = P[8].copy(); inf_pose[0, 3] = np.inf
    inl, err = ctx.pose_scores(SRC, TGT, np.stack([nan_pose, inf_pose, P[0]]), AC.SCORE_MAX_DIST)
    assert inl[0] == 0 and inl[1] == 0 and err[0] == DBL_MAX and err[1] == DBL_MAX and inl[2] > 0
    # non-finite target points are nobody's nearest point
    bad_t, _ = K.with_non_finite(t, seed=9)
    ctx.upload(5, bad_t)
    ctx.upload(6, bad_t[np.isfinite(bad_t[:, :3]).all(1)])
    check(ctx.pose_scores(SRC, 5, P[:12], AC.SCORE_MAX_DIST), anchor(ctx, SRC, 6, P[:12], AC.SCORE_MAX_DIST), len(s))


def test_empty_target_empty_source_and_no_poses(ctx, scene):
    s, t, P = scene
    ctx.upload(7, t[:0])
    inl, err = ctx.pose_scores(SRC, 7, P[:5], AC.SCORE_MAX_DIST)
    assert (inl == 0).all() and (err == DBL_MAX).all()
    want = anchor(ctx, SRC, 7, P[:2], AC.SCORE_MAX_DIST)
    assert (want[0] == 0).all()
    inl, err = ctx.pose_scores(7, TGT, P[:5], AC.SCORE_MAX_DIST)
    assert (inl == 0).all() and (err == DBL_MAX).all()
    inl, err = ctx.pose_scores(SRC, TGT, P[:0], AC.SCORE_MAX_DIST)
    assert inl.shape == (0,) and err.shape == (0,)
    # tiny clouds have no grid: one cell over the points
    ctx.upload(8, s[:3]); ctx.upload(9, t[:2])
    check(ctx.pose_scores(8, TGT, P[:3], AC.SCORE_MAX_DIST), anchor(ctx, 8, TGT, P[:3], AC.SCORE_MAX_DIST), 3)
    check(ctx.pose_scores(SRC, 9, P[:3], 60.0), anchor(ctx, SRC, 9, P[:3], 60.0), len(s))

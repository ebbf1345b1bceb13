"""GPU tests of mvr_align_prerejective (rules A1-A6 in include/mvr_hip.h), every run with its trace:
 (a) status, samples and matches of every iteration equal align_ref's replay fed with the GPU's own k-NN table, and that table
     equals align_ref.feature_knn of the same rows bit for bit (as every table of test_gpu_feature_knn.py does);
 (b) inliers / error of every scored iteration equal the anchor of test_gpu_pose_scores.py applied to the traced pose;
 (c) every traced pose agrees with numpy's Kabsch on the traced pairs within the bar of the estimator's own test
     (tests/test_gpu_configs.py:22, used at :29-32: rotation entries 1e-5, translation 1e-4 mm);
 (d) the result is A6 replayed over the trace: the same best iteration and the same bits of T;
 (e) runs with and without trace, repeated runs and every chunk size return identical results;
 (f) a guess that satisfies the threshold is returned as best_iteration -1 when no iteration beats it;
 (g) fewer eligible points than samples, k = 1, three and five samples.
And the recovery of a known pose end to end (voxel grid, normals and FPFH from the library on each cloud).

What was measured is in the docstring of test_recovery_of_a_known_pose."""
import importlib

import numpy as np
import pytest

import align_cases as AC
import align_ref as R
from conftest import PKG
from test_gpu_pose_scores import anchor

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_configs.py:22
S, T_, SPARE, FINITE = 10, 11, 12, 13


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def align(ctx, pair, **kw):
    s, t, sf, tf = pair
    ctx.upload(S, s)
    ctx.upload(T_, t)
    a = dict(max_iterations=AC.ALIGN_ITERS, nr_samples=3, k=AC.ALIGN_K, similarity=AC.ALIGN_SIMILARITY, max_dist=AC.ALIGN_MAX_DIST,
             inlier_fraction=AC.ALIGN_FRACTION, seed=AC.ALIGN_SEED, return_trace=True)
    a.update(kw)
    return ctx.align_prerejective(S, T_, sf, tf, **a), a


def same_result(a, b):
    return all(a[k] == b[k] for k in ("converged", "best_iteration", "inliers", "rejected", "scored")) and \
        np.float64(a["error"]).view(np.uint64) == np.float64(b["error"]).view(np.uint64) and \
        np.array_equal(a["T"].view(np.uint32), b["T"].view(np.uint32))


def same_trace(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in b)


def same_table(got, want):
    """a k-NN table of the GPU against align_ref.feature_knn of the same rows: indices and d2 bits, nothing excluded"""
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32))


def verify(ctx, pair, res, tr, a):
    """(a)-(d) on one traced run"""
    s, t, sf, tf = pair
    nr, iters = a["nr_samples"], a["max_iterations"]
    el = R.eligible(s, sf)
    if len(el) >= nr:
        idx, d2 = ctx.feature_knn(sf[el], tf, a["k"])
        same_table((idx, d2), R.feature_knn(sf[el], tf, a["k"]))     # the table the replay is fed is the reference's own
    else:
        idx = np.zeros((len(el), a["k"]), np.uint32)
    st, src, tgt = R.replay(s, t, el, idx, iters, nr, a["seed"], a["similarity"], a.get("fma", False))
    assert np.array_equal(tr["status"], st) and np.array_equal(tr["src"], src) and np.array_equal(tr["tgt"], tgt)      # (a)
    assert res["rejected"] == int((st == 0).sum()) and res["scored"] == int((st == 1).sum())
    scored = np.nonzero(st == 1)[0]
    if len(scored):
        fin = np.isfinite(s[:, :3]).all(1)                             # (the anchor's mvr_nn has no rule for non-finite queries: S1 gives them no inlier)
        if not fin.all():
            ctx.upload(FINITE, s[fin])
        inl, err, _ = anchor(ctx, S if fin.all() else FINITE, T_, tr["T"][scored], a["max_dist"], a.get("fma", False), spare=SPARE)      # (b)
        assert np.array_equal(tr["inliers"][scored], inl)
        some = inl > 0
        assert (tr["error"][scored][~some] == R.DBL_MAX).all()
        assert (np.abs(tr["error"][scored][some] - err[some]) <= len(s) * 2.0 ** -52 * err[some]).all()
        worst = [0.0, 0.0]
        for i in scored:                                                                                                # (c)
            K, sv = R.kabsch(s[src[i], :3], t[tgt[i], :3])
            dr, dt = np.abs(tr["T"][i][:3, :3] - K[:3, :3]).max(), np.abs(tr["T"][i][:3, 3] - K[:3, 3]).max()
            worst = [max(worst[0], dr), max(worst[1], dt)]
            assert dr <= ROT_TOL and dt <= TRANS_TOL, (i, dr, dt, sv)
            assert np.array_equal(tr["T"][i][3], [0, 0, 0, 1])
        print("Kabsch: rotation within %.2g, translation within %.2g over %d poses" % (worst[0], worst[1], len(scored)))
    rest = np.nonzero(st != 1)[0]
    assert (tr["inliers"][rest] == 0).all() and (tr["T"][rest] == 0).all()
    conv, best = R.select(st, tr["inliers"], tr["error"], len(s), a["inlier_fraction"])                                 # (d)
    assert res["converged"] == conv and res["best_iteration"] == best
    if conv:
        assert np.array_equal(res["T"].view(np.uint32), tr["T"][best].view(np.uint32))
        assert res["inliers"] == tr["inliers"][best] and res["error"] == tr["error"][best]
    else:
        assert np.array_equal(res["T"], np.eye(4, dtype=F32)) and res["inliers"] == 0 and res["error"] == R.DBL_MAX
    return st


@pytest.fixture(scope="module")
def base(ctx):
    pair = AC.align_pair()
    (res, tr), a = align(ctx, pair)
    return pair, res, tr, a


def test_trace_replay_scores_kabsch_and_selection(ctx, base):
    pair, res, tr, a = base
    st = verify(ctx, pair, res, tr, a)
    assert 0.25 <= (st == 0).mean() <= 0.75
    assert res["converged"] and res["inliers"] >= 0.6 * AC.ALIGN_NS                  # the 300 twins of the case
    x = pair[0][:, :3].astype(F64) @ res["T"][:3, :3].astype(F64).T + res["T"][:3, 3].astype(F64)
    y = pair[0][:, :3].astype(F64) @ AC.ALIGN_POSE[:3, :3].astype(F64).T + AC.ALIGN_POSE[:3, 3].astype(F64)
    assert np.linalg.norm(x - y, axis=1).max() < AC.ALIGN_MAX_DIST


def test_identical_results_with_and_without_trace_again_and_for_every_chunk(ctx, base):
    pair, res, tr, a = base
    (plain, _) = align(ctx, pair, return_trace=False)
    assert same_result(plain, res)
    try:
        for chunk in (1, 7, 64, 1000):
            ctx.tune(score_chunk=chunk)
            (r2, t2), _ = align(ctx, pair)
            assert same_result(r2, res), chunk
            assert same_trace(t2, tr), chunk
    finally:
        ctx.tune(score_chunk=256)
    for split in (1, 3):
        ctx.tune(feat_split=split)
        (r3, _) = align(ctx, pair, return_trace=False)
        ctx.tune(feat_split=0)
        assert same_result(r3, res)


def test_guess(ctx, base):
    pair, res, tr, a = base
    (g, gt), _ = align(ctx, pair, guess=res["T"])                 # the best pose itself: no iteration is strictly better
    assert g["converged"] and g["best_iteration"] == -1 and np.array_equal(g["T"].view(np.uint32), res["T"].view(np.uint32))
    assert g["inliers"] == res["inliers"] and g["error"] == res["error"]
    assert same_trace(gt, tr)      # the guess is not an iteration
    (b, _), _ = align(ctx, pair, guess=np.eye(4, dtype=F32))      # a guess below the inlier fraction changes nothing
    assert same_result(b, res)
    (z, _), _ = align(ctx, pair, guess=AC.ALIGN_POSE, max_iterations=0)
    assert z["converged"] and z["best_iteration"] == -1 and z["scored"] == 0 and np.array_equal(z["T"], AC.ALIGN_POSE)
    inl, err, _ = anchor(ctx, S, T_, [AC.ALIGN_POSE], a["max_dist"], spare=SPARE)
    assert z["inliers"] == inl[0] and abs(z["error"] - err[0]) <= AC.ALIGN_NS * 2.0 ** -52 * err[0]
    (w, _), _ = align(ctx, pair, guess=np.eye(4, dtype=F32), max_iterations=0)
    assert not w["converged"] and np.array_equal(w["T"], np.eye(4, dtype=F32)) and w["error"] == R.DBL_MAX


@pytest.mark.parametrize("nr,k,fma", [(3, 1, False), (5, 2, False), (5, 1, True), (8, 64, False)])
def test_other_sample_counts_and_randomness(nr, k, fma, ctx):
    pair = AC.align_pair()
    (res, tr), a = align(ctx, pair, nr_samples=nr, k=k, fma=fma)
    verify(ctx, pair, res, tr, a)


def test_invalid_points_and_rows(ctx):
    pair = AC.align_with_invalid()
    (res, tr), a = align(ctx, pair)
    st = verify(ctx, pair, res, tr, a)
    el = R.eligible(pair[0], pair[2])
    assert np.isin(tr["src"], el).all() and (st == 1).sum() > 20
    bad_t = np.nonzero(~np.isfinite(pair[3]).all(1))[0]
    assert not np.isin(tr["tgt"], bad_t).any()


def test_fewer_eligible_points_than_samples(ctx):
    s, t, sf, tf = AC.align_pair()
    sf = sf.copy()
    sf[2:, 0] = np.nan                                             # two eligible points
    (res, tr), a = align(ctx, (s, t, sf, tf))
    assert not res["converged"] and res["scored"] == 0 and res["rejected"] == 0 and res["best_iteration"] == -1
    assert (tr["status"] == 2).all() and (tr["src"] == R.NONE).all() and (tr["tgt"] == R.NONE).all()
    verify(ctx, (s, t, sf, tf), res, tr, a)
    # a target without one finite row: every list is empty, every iteration has status 2
    tf2 = np.full_like(tf, np.nan)
    (res, tr), a = align(ctx, (s, t, AC.align_pair()[2], tf2))
    assert not res["converged"] and (tr["status"] == 2).all() and (tr["tgt"] == R.NONE).all() and (tr["src"] != R.NONE).all()


# ------------------------------------------------------------------ recovery

def prepare(ctx, slot, pts):
    """voxel grid, normals and FPFH of the library on one cloud: (points, descriptors)"""
    ctx.upload(slot, pts)
    ctx.voxel_grid(slot, slot, AC.REC_LEAF)
    ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS)
    return ctx.download(slot), ctx.fpfh(slot, AC.REC_FPFH_RADIUS)


def test_recovery_of_a_known_pose(ctx, mvr):
    """The target is a synthetic view voxel-downsampled to a few thousand points, the source the same view moved by 70 degrees
    about a skew axis and a translation and then downsampled, so the clouds hold different points.  The aligner must converge and
    its pose must leave no source point further than max_dist from where the true inverse pose puts it.

    Parameters chosen with align_ref's replay on the CPU (reference voxel grid, normals and FPFH, 3 097 / 3 150 points, scores by
    a kd-tree): the object is a smooth blob, so with max_dist = 6 mm about half of the scored poses reach every point and the
    error alone decides.  At 4 000 iterations the best pose's worst displacement was 3.8 mm with k = 2 and 7.0 mm with k = 5 (a
    miss); at 20 000 iterations 2.9 mm (k = 2: 98.4 % polygon-rejected, 330 scored, 187 accepted, 14 of them within the bar) and
    3.4 mm (k = 5) -- hence 20 000 iterations and k = 2; four other seeds at those settings: 2.9, 2.5, 1.2 and 2.8 mm.  NOT measured on a GPU: no device was available when this was written."""
    s_raw, t_raw = AC.recovery_view(mvr)
    s, sf = prepare(ctx, 20, s_raw)
    t, tf = prepare(ctx, 21, t_raw)
    assert 1500 <= len(s) <= 9000 and 1500 <= len(t) <= 9000 and len(s) != len(t)
    res, tr = ctx.align_prerejective(20, 21, sf, tf, return_trace=True, **AC.REC_PARAMS)
    inv = np.linalg.inv(AC.REC_POSE.astype(F64))
    x = s[:, :3].astype(F64) @ res["T"][:3, :3].astype(F64).T + res["T"][:3, 3].astype(F64)
    y = s[:, :3].astype(F64) @ inv[:3, :3].T + inv[:3, 3]
    worst = float(np.linalg.norm(x - y, axis=1).max())
    print("recovery: %d / %d points, converged %d at iteration %d, %d inliers, error %.4f, rejected %d, scored %d, worst displacement %.3f mm"
          % (len(s), len(t), res["converged"], res["best_iteration"], res["inliers"], res["error"], res["rejected"], res["scored"], worst))
    assert res["converged"]
    assert worst <= AC.REC_MAX_DIST
    # the reference's replay of the first iterations of the same run, from the GPU's own table
    el = R.eligible(s, sf)
    idx, d2 = ctx.feature_knn(sf[el], tf, AC.REC_PARAMS["k"])
    # ... which is the reference's table of the same rows: the library's own FPFH signatures, real-valued, where the order and
    # the rounding of M1's sum show in the bits
    ri, rd = R.feature_knn(sf[el], tf, AC.REC_PARAMS["k"])
    same_table((idx, d2), (ri, rd))
    print("recovery: k-NN table of %d x %d signatures equals the reference's, %d entries" % (len(el), len(tf), idx.size))
    m = AC.REC_REPLAY
    st, src, tgt = R.replay(s, t, el, idx, m, 3, AC.REC_PARAMS["seed"], AC.REC_PARAMS["similarity"])
    assert np.array_equal(tr["status"][:m], st) and np.array_equal(tr["src"][:m], src) and np.array_equal(tr["tgt"][:m], tgt)

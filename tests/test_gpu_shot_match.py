"""GPU tests of the matcher and of the sample-consensus aligner on rows of 352 floats (SHOT; mvr_feature_knn and
mvr_align_prerejective_dim, rules M1-M3 and A1-A6 in include/mvr_hip.h) against tests/align_ref.py with its width set to 352: the
k-NN table bit for bit in idx and d2.  The 352-float kernel (csrc/mvr_shot.hip) keeps the partial sums of a tile of 16 target
rows per thread, 256 queries per block, and shares the split of the target (whole multiples of 64 rows) and the merge with the
33- and 125-float kernel: the shapes below stand one below, at and one above each of those edges.

Measured on an MI355X (profiles/shot_pytest_gpu.log, this file's own prints), on the pair of tests/test_gpu_align.py (3 097 / 3 150
points after the 4 mm voxel grid, 20 000 iterations, k = 2, seed 7), worst displacement of the recovered pose: FPFH at 20 mm
2.858 mm, PFH at 20 mm 3.128 mm, SHOT at 20 mm (101 neighbours) 172.6 mm -- 61 hypotheses scored, a wrong pose accepted -- and SHOT
at 40 mm (381 neighbours) 4.121 mm with 296 hypotheses scored.  The x axis of a SHOT frame is a vote (rule L5), and on this smooth
blob a vote over a hundred neighbours falls differently on the two differently sampled clouds; with k = 5 or another seed the
20 mm rows give 22 to 198 mm, the 30 mm rows 4.1 to 13.4 mm, the 40 mm rows 2.9 to 6.5 mm.  So the SHOT rows of this test are taken
at SHOT_RADIUS = 40 mm, twice the radius of the histogram descriptors, and their pose is held to the bar of that pair's own test
(align_cases.REC_MAX_DIST, 6 mm); the 20 mm figure is printed beside it.  The descriptor itself equals the reference slot for slot
at any radius (tests/test_gpu_shot.py)."""
import contextlib
import importlib

import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
from conftest import PKG

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DIM = 352
EDGE_NQ = (1, 255, 256, 257)                     # a block of 256 queries
EDGE_NT = (1, 15, 16, 17, 31, 33, 63, 64, 65, 129)      # a tile of 16 rows; 64 rows, the unit of a split
KS = (1, 2, 10, 64)
SPLIT_SHAPE = (257, 4161)                        # align_cases.KNN_SPLIT_SHAPE: feat_split 7 gives 7 x 640 rows, the last split 321
SPLITS = (1, 2, 3, 7, 64)
SHOT_RADIUS = 2.0 * AC.REC_FPFH_RADIUS         # see the module docstring


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def align_ref_width(dim):
    """align_ref.feature_knn / eligible reshape their tables to align_ref.DIM floats per row"""
    old, AR.DIM = AR.DIM, dim
    try:
        yield AR
    finally:
        AR.DIM = old


def ref_knn(q, t, k, dim=DIM):
    with align_ref_width(dim) as A:
        return A.feature_knn(q, t, k)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_table(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))


def quantised(rng, n, dim=DIM):
    """rows of small integers over 16: every term of M1 is exact, and many pairs tie in d2 exactly"""
    return (rng.integers(0, 3, (n, dim)) / 16.0).astype(F32)


def shot_like(rng, n, dim=DIM):
    """rows like SHOT signatures: non-negative, most of the mass in few slots, unit norm, real-valued"""
    r = rng.uniform(0, 1, (n, dim)) * rng.uniform(0, 1, (n, dim)) ** 8
    return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F32)


@pytest.mark.parametrize("nq", EDGE_NQ)
def test_tile_block_and_split_edges_on_rows_that_tie(nq, ctx):
    rng = np.random.default_rng(300 + nq)
    q = quantised(rng, nq)
    ties = 0
    for nt in EDGE_NT:
        t = quantised(rng, nt)
        want = ref_knn(q, t, 10)
        same_table(ctx.feature_knn(q, t, 10), want)
        d = want[1][:, :min(nt, 10)]
        ties += int((d[:, 1:] == d[:, :-1]).sum())
    assert ties > 0                                                        # the index decides somewhere (M2)


@pytest.mark.parametrize("k", KS)
def test_every_list_size_on_real_valued_rows(k, ctx):
    rng = np.random.default_rng(400 + k)
    q, t = shot_like(rng, 300), shot_like(rng, 700)
    same_table(ctx.feature_knn(q, t, k), ref_knn(q, t, k))


def test_the_result_does_not_depend_on_the_split(ctx):
    rng = np.random.default_rng(9)
    nq, nt = SPLIT_SHAPE
    q, t = quantised(rng, nq), quantised(rng, nt)
    want = ref_knn(q, t, 9)
    try:
        for split in (0,) + SPLITS:
            ctx.tune(feat_split=split)
            same_table(ctx.feature_knn(q, t, 9), want)
    finally:
        ctx.tune(feat_split=0)
    try:                                                                   # splits whose last one is one row, 15, 16 and 17 rows long
        ctx.tune(feat_split=2)
        for nt in (65, 79, 80, 81):
            same_table(ctx.feature_knn(q[:40], t[:nt], 2), ref_knn(q[:40], t[:nt], 2))
    finally:
        ctx.tune(feat_split=0)


def test_nan_rows_on_both_sides_and_targets_shorter_than_k(mvr, ctx):
    rng = np.random.default_rng(5)
    q, t = shot_like(rng, 300), shot_like(rng, 700)
    q[rng.choice(300, 20, replace=False), rng.integers(0, DIM, 20)] = np.nan
    t[rng.choice(700, 40, replace=False), rng.integers(0, DIM, 40)] = (np.nan, np.inf)[0]
    t[5, 351] = np.inf; t[6, 0] = -np.inf
    idx, d2 = ctx.feature_knn(q, t, 3)
    same_table((idx, d2), ref_knn(q, t, 3))
    assert (idx[np.isnan(q).any(1)] == AR.NONE).all() and not np.isin(idx, np.nonzero(~np.isfinite(t).all(1))[0]).any()
    q = shot_like(rng, 40)
    for nt in (1, 5, 15, 17, 63, 65):                                      # nt < k: the tails of the lists
        t = shot_like(rng, nt)
        same_table(ctx.feature_knn(q, t, 64), ref_knn(q, t, 64))
    idx, d2 = ctx.feature_knn(q, q[:0], 4)
    assert (idx == AR.NONE).all() and np.isinf(d2).all()
    assert ctx.feature_knn(q[:0], q, 4)[0].shape == (0, 4)


@pytest.mark.parametrize("dim", (33, 125))
def test_the_other_widths_give_the_bits_they_gave(dim, ctx):
    rng = np.random.default_rng(dim)
    q = (rng.uniform(0, 100, (300, dim)) * rng.uniform(0, 1, (300, dim)) ** 6).astype(F32)
    t = (rng.uniform(0, 100, (700, dim)) * rng.uniform(0, 1, (700, dim)) ** 6).astype(F32)
    same_table(ctx.feature_knn(q, t, 5), ref_knn(q, t, 5, dim))


def test_widths_that_are_still_refused(mvr, ctx):
    for dim in (351, 353, 344, 360, 1344):
        rows = np.ones((4, dim), F32)
        with pytest.raises(mvr.MvrError):
            ctx.feature_knn(rows, rows, 1)


def test_alignment_from_shot_rows(mvr, ctx):
    """the pair of tests/test_gpu_align.py's recovery test, aligned from FPFH, PFH and SHOT rows at the same settings: the trace of
    the SHOT run (rows at SHOT_RADIUS) is replayed decision for decision, its k-NN table equals the reference's on the first 200
    eligible rows, and its pose is held to that test's bar; the displacements are printed side by side, SHOT at 20 mm among them"""
    s_raw, t_raw = AC.recovery_view(mvr)
    inv = np.linalg.inv(AC.REC_POSE.astype(F64))
    rows = {}
    for slot, raw_pts in ((20, s_raw), (21, t_raw)):
        ctx.upload(slot, raw_pts)
        ctx.voxel_grid(slot, slot, AC.REC_LEAF)
        ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS)
        rows[slot] = (ctx.download(slot), ctx.fpfh(slot, AC.REC_FPFH_RADIUS), ctx.pfh(slot, radius=AC.REC_FPFH_RADIUS),
                      ctx.shot(slot, SHOT_RADIUS), ctx.shot(slot, AC.REC_FPFH_RADIUS))
    (s, sf33, sf125, sf352, sf_small), (t, tf33, tf125, tf352, tf_small) = rows[20], rows[21]
    assert sf352.shape == (len(s), DIM) and np.isfinite(sf352).all(1).mean() > 0.9
    y = s[:, :3].astype(F64) @ inv[:3, :3].T + inv[:3, 3]
    worst = {}
    for name, sf, tf in (("FPFH", sf33, tf33), ("PFH", sf125, tf125), ("SHOT at %g mm" % AC.REC_FPFH_RADIUS, sf_small, tf_small),
                         ("SHOT", sf352, tf352)):
        res, tr = ctx.align_prerejective(20, 21, sf, tf, return_trace=True, **AC.REC_PARAMS)
        x = s[:, :3].astype(F64) @ res["T"][:3, :3].astype(F64).T + res["T"][:3, 3].astype(F64)
        worst[name] = float(np.linalg.norm(x - y, axis=1).max())
        print("%s: %d / %d points, converged %d at iteration %d, %d inliers, error %.4f, rejected %d, scored %d, worst displacement "
              "%.3f mm; matching %.1f ms, hypotheses %.1f ms, scoring %.1f ms"
              % (name, len(s), len(t), res["converged"], res["best_iteration"], res["inliers"], res["error"], res["rejected"], res["scored"],
                 worst[name], ctx.stat("prerej_match_ms"), ctx.stat("prerej_hypotheses_ms"), ctx.stat("prerej_score_ms")))
    assert res["converged"] and worst["SHOT"] <= AC.REC_MAX_DIST
    with align_ref_width(DIM) as A:
        el = A.eligible(s, sf352)
    k = AC.REC_PARAMS["k"]
    idx, d2 = ctx.feature_knn(sf352[el], tf352, k)
    same_table((idx[:200], d2[:200]), ref_knn(sf352[el][:200], tf352, k))
    m = 300
    st, src, tgt = AR.replay(s, t, el, idx, m, 3, AC.REC_PARAMS["seed"], AC.REC_PARAMS["similarity"])
    assert np.array_equal(tr["status"][:m], st) and np.array_equal(tr["src"][:m], src) and np.array_equal(tr["tgt"][:m], tgt)
    conv, best = AR.select(tr["status"], tr["inliers"], tr["error"], len(s), AC.REC_PARAMS["inlier_fraction"])
    assert res["converged"] == conv and res["best_iteration"] == best
    # tables of two widths, or not one row per point
    for bad_s, bad_t in ((sf352, tf125), (sf352[:, :351], tf352[:, :351]), (sf352[:-1], tf352)):
        with pytest.raises(ValueError):
            ctx.align_prerejective(20, 21, bad_s, bad_t, **AC.REC_PARAMS)

"""GPU tests of the two outlier filters (mvr_cloud_statistical_outlier_removal, mvr_cloud_radius_outlier_removal; rules in
include/mvr_hip.h) against the numpy reference of tests/outlier_ref.py, and of their C++ layers (pcl::StatisticalOutlierRemoval,
pcl::RadiusOutlierRemoval, ScanCloud::removeStatisticalOutliers / removeRadiusOutliers).

Two correct implementations can only disagree on the inlier set when a mean distance lies within the f64 summation noise of the
threshold (about 1e-13 relative for 2e5 terms).  Every test that compares sets therefore first asserts, on the reference alone,
that no mean distance is within 1e-9 relative of the threshold: a condition on the input, not a tolerance on the result."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import outlier_ref as R
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MIN_GAP = 1e-9


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def with_outliers(view, n_out, seed=7, grow=5.0):
    """the view plus n_out points drawn uniformly from its bounding box grown by `grow` mm, shuffled; (points, injected mask)"""
    rng = np.random.default_rng(seed)
    lo, hi = view[:, :3].min(0) - grow, view[:, :3].max(0) + grow
    o = np.ones((n_out, 4), F32)
    o[:, :3] = rng.uniform(lo, hi, (n_out, 3)).astype(F32)
    p = np.concatenate([view, o])
    perm = rng.permutation(len(p))
    return np.ascontiguousarray(p[perm]), perm >= len(view)


@pytest.fixture(scope="module")
def main_case(mvr):
    """view 0 of synth_params(12, 2) at 200 000 points plus 2 000 injected outliers"""
    return with_outliers(mvr.synth_view(mvr.synth_params(12, 2), 0, 200000), 2000)


@pytest.fixture(scope="module")
def view20k(mvr):
    return mvr.synth_view(mvr.synth_params(12, 2), 0, 20000)


_ref_cache = {}


def ref_mean_dist(tag, p, k, fma=False):
    key = (tag, k, bool(fma))
    if key not in _ref_cache:
        _ref_cache[key] = R.mean_dist(p, k, fma)
    return _ref_cache[key]


def ref_statistical(tag, p, k, mul, negative=False, fma=False):
    """R.statistical with the mean distances taken from the cache"""
    md, nv = ref_mean_dist(tag, p, k, fma)
    st = R.statistics(md, nv, mul)
    fin = R.finite_mask(p)
    with np.errstate(invalid="ignore"):
        inl = fin & ~(md.astype(F64) > st["threshold"])
    gap = np.inf
    if nv and np.isfinite(st["threshold"]) and st["threshold"] != 0:
        gap = float(np.min(np.abs(md[fin].astype(F64) - st["threshold"])) / abs(st["threshold"]))
    sel = ~inl if negative else inl
    return dict(mean_dist=md, stats=st, inlier=inl, index=np.nonzero(sel)[0].astype(np.uint32), gap=gap)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rel(a, b):
    return abs(a - b) / abs(b)


def sor(ctx, p, k, mul, dst=1, src=0, normals=None, **kw):
    ctx.upload(src, p)
    if normals is not None:
        ctx.upload_normals(src, normals)
    n, idx, md, st = ctx.statistical_outlier_removal(dst, src, k, mul, return_index=True, return_dist=True, return_stats=True, **kw)
    out = ctx.download(dst)
    assert len(out) == n == len(idx)
    return out, idx, md, st


def ror(ctx, p, radius, min_nb, dst=1, src=0, normals=None, **kw):
    ctx.upload(src, p)
    if normals is not None:
        ctx.upload_normals(src, normals)
    n, idx, cnt = ctx.radius_outlier_removal(dst, src, radius, min_nb, return_index=True, return_counts=True, **kw)
    out = ctx.download(dst)
    assert len(out) == n == len(idx)
    return out, idx, cnt


def check_sor(p, got, ref, need_gap=True):
    out, idx, md, st = got
    if need_gap:
        assert ref["gap"] >= MIN_GAP, "the input puts a mean distance within %.1e of the threshold" % ref["gap"]
    assert same_bits(md, ref["mean_dist"])
    assert st["n_valid"] == ref["stats"]["n_valid"]
    for key in ("mean", "stddev", "threshold"):
        a, b = st[key], ref["stats"][key]
        print("%s: gpu %.17g reference %.17g" % (key, a, b))
        assert (np.isnan(a) and np.isnan(b)) or a == b or rel(a, b) <= 1e-12, (key, a, b)
    assert np.array_equal(idx, ref["index"])
    assert same_bits(out, p[ref["index"]])


# ------------------------------------------------------------------ mean distances

@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("k", [1, 8, 16, 50, 64])
def test_mean_dist_is_bit_identical_on_the_main_case(ctx, main_case, k, fma):
    p, _ = main_case
    ctx.upload(0, p)
    n, md = ctx.statistical_outlier_removal(1, 0, k, 1.0, fma=fma, return_dist=True)
    ref, nv = ref_mean_dist("main", p, k, fma)
    assert nv == len(p) and same_bits(md, ref)
    if k == 1:
        _, d2 = ctx.knn(0, 0, 2, fma=fma)
        assert same_bits(md, np.sqrt(d2[:, 1]))


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("k", [1, 8, 16, 50, 64])
def test_mean_dist_is_bit_identical_on_a_20k_view(ctx, view20k, k, fma):
    ctx.upload(0, view20k)
    n, md = ctx.statistical_outlier_removal(1, 0, k, 1.0, fma=fma, return_dist=True)
    ref, nv = ref_mean_dist("20k", view20k, k, fma)
    assert nv == len(view20k) and same_bits(md, ref)
    if k == 1:
        _, d2 = ctx.knn(0, 0, 2, fma=fma)
        assert same_bits(md, np.sqrt(d2[:, 1]))


# ------------------------------------------------------------------ inlier sets, indices, points, statistics

@pytest.mark.parametrize("k,mul", [(8, 1.0), (16, 2.0), (50, 1.0), (64, 3.0)])
def test_inliers_index_points_and_stats_on_the_main_case(ctx, main_case, k, mul):
    p, inj = main_case
    ref = ref_statistical("main", p, k, mul)
    got = sor(ctx, p, k, mul)
    print("mean_k %d, stddev_mul %g: threshold %.4f mm, %d of %d injected outliers removed, %d surface points removed, gap %.1e"
          % (k, mul, ref["stats"]["threshold"], int((~ref["inlier"] & inj).sum()), int(inj.sum()), int((~ref["inlier"] & ~inj).sum()), ref["gap"]))
    check_sor(p, got, ref)
    assert (got[0][:, 3] == 1).all()


def test_clean_view_with_a_small_gap(ctx, mvr):
    v = mvr.synth_view(mvr.synth_params(12, 2), 0, 200000)
    ref = ref_statistical("clean", v, 16, 2.0)
    print("clean view (16, 2.0): %d removed, gap %.1e" % (int((~ref["inlier"]).sum()), ref["gap"]))
    check_sor(v, sor(ctx, v, 16, 2.0), ref)


def test_anchor_outside_the_f32_path(ctx, main_case):
    """mean distances from the kd-tree's own f64 distances: 1e-6 relative, and the same inlier set at (8, 1.0), where the
    smallest gap to the threshold is 9e-3"""
    p, _ = main_case
    a = R.mean_dist_f64(p, 8)
    out, idx, md, st = sor(ctx, p, 8, 1.0)
    err = np.max(np.abs(md.astype(F64) - a) / a)
    print("largest relative difference to the f64 anchor: %.3g" % err)
    assert err <= 1e-6
    mean = a.sum() / len(a)
    thr = mean + 1.0 * np.sqrt(((a - mean) ** 2).sum() / (len(a) - 1))
    assert np.min(np.abs(a - thr)) / thr >= 1e-4
    assert np.array_equal(idx, np.nonzero(~(a > thr))[0])


# ------------------------------------------------------------------ radius filter

@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("radius,min_nb", [(1.0, 3), (2.0, 9)])
def test_radius_counts_on_a_20k_view(ctx, view20k, radius, min_nb, fma):
    ref = R.radius(view20k, radius, min_nb, fma=fma)
    out, idx, cnt = ror(ctx, view20k, radius, min_nb, fma=fma)
    print("radius %g: mean count %.2f, %d of %d kept" % (radius, cnt.mean(), len(idx), len(view20k)))
    assert np.array_equal(cnt, ref["count"])
    assert np.array_equal(idx, ref["index"]) and same_bits(out, view20k[ref["index"]])
    assert 0 < len(idx) < len(view20k)


def test_radius_counts_on_the_main_case(ctx, main_case):
    p, inj = main_case
    ref = R.radius(p, 0.45, 2)
    out, idx, cnt = ror(ctx, p, 0.45, 2)
    print("radius 0.45: mean count %.2f, %d injected and %d surface points removed"
          % (cnt.mean(), int((~ref["inlier"] & inj).sum()), int((~ref["inlier"] & ~inj).sum())))
    assert np.array_equal(cnt, ref["count"])
    assert np.array_equal(idx, ref["index"]) and same_bits(out, p[ref["index"]])


def test_lattice_neighbours_on_the_sphere_count(ctx):
    g = np.stack(np.meshgrid(np.arange(12), np.arange(9), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
    p = np.ones((len(g), 4), F32)
    p[:, :3] = g + np.array([-3.0, 10.0, 900.0])
    inner = ((g > 0) & (g < np.array([11, 8, 6]))).sum(1)
    out, idx, cnt = ror(ctx, p, 1.0, 6)
    assert np.array_equal(cnt, 3 + inner)                 # d2 == r2 exactly: counted
    assert np.array_equal(idx, np.nonzero(inner == 3)[0])
    assert np.array_equal(cnt, R.neighbor_counts(p, 1.0))
    # the statistical filter on the same lattice: every tie between equal distances
    for k in (1, 6, 7, 26):
        ctx.upload(0, p)
        n, md = ctx.statistical_outlier_removal(1, 0, k, 1.0, return_dist=True)
        assert same_bits(md, R.mean_dist(p, k)[0])


# ------------------------------------------------------------------ negative, in place, normals

def small_case(view20k):
    return with_outliers(view20k, 300, seed=11)[0]


def test_negative_is_the_exact_complement(ctx, view20k):
    p = small_case(view20k)
    ref = ref_statistical("small", p, 8, 1.0)
    assert ref["gap"] >= MIN_GAP
    out, idx, md, st = sor(ctx, p, 8, 1.0)
    nout, nidx, nmd, nst = sor(ctx, p, 8, 1.0, negative=True)
    assert np.array_equal(np.sort(np.concatenate([idx, nidx])), np.arange(len(p)))
    assert 0 < len(nidx) < len(idx) and np.array_equal(nidx, np.nonzero(~ref["inlier"])[0])
    assert same_bits(nout, p[nidx]) and same_bits(md, nmd) and st == nst
    out, idx, cnt = ror(ctx, p, 1.5, 4)
    nout, nidx, ncnt = ror(ctx, p, 1.5, 4, negative=True)
    assert np.array_equal(np.sort(np.concatenate([idx, nidx])), np.arange(len(p)))
    assert 0 < len(nidx) < len(idx) and same_bits(nout, p[nidx]) and np.array_equal(cnt, ncnt)


def test_in_place_equals_out_of_place_and_the_source_stays(ctx, view20k):
    p = small_case(view20k)
    a = sor(ctx, p, 16, 1.0, dst=1, src=0)
    assert same_bits(ctx.download(0), p)
    b = sor(ctx, p, 16, 1.0, dst=0, src=0)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and a[3] == b[3]
    a = ror(ctx, p, 1.5, 4, dst=1, src=0)
    assert same_bits(ctx.download(0), p)
    b = ror(ctx, p, 1.5, 4, dst=0, src=0)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert 0 < len(a[1]) < len(p)


def test_normals_follow_their_points(ctx, view20k):
    p = small_case(view20k)
    rng = np.random.default_rng(3)
    nr = rng.standard_normal((len(p), 4)).astype(F32)
    nr[:, 3] = 0
    for dst in (1, 0):
        out, idx, md, st = sor(ctx, p, 8, 1.0, dst=dst, normals=nr)
        assert 0 < len(idx) < len(p) and same_bits(ctx.download_normals(dst), nr[idx])
        out, idx, cnt = ror(ctx, p, 1.5, 4, dst=dst, normals=nr, negative=True)
        assert 0 < len(idx) < len(p) and same_bits(ctx.download_normals(dst), nr[idx])
    # a source without normals gives an output without
    ctx.upload(0, p)
    ctx.statistical_outlier_removal(1, 0, 8, 1.0)
    assert len(ctx.download_normals(1)) == 0


# ------------------------------------------------------------------ non-finite points

def test_non_finite_points_are_outliers(ctx, view20k):
    p = small_case(view20k).copy()
    rng = np.random.default_rng(5)
    bad = rng.choice(len(p), 60, replace=False)
    vals = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(bad):
        p[i, j % 3] = vals[(j // 3) % 3]
    p[bad[0], :3] = np.nan
    fin = R.finite_mask(p)
    assert (~fin).sum() == 60
    for k, mul in ((8, 1.0), (50, 2.0)):
        ref = R.statistical(p, k, mul)
        got = sor(ctx, p, k, mul)
        check_sor(p, got, ref)
        assert np.isnan(got[2][~fin]).all() and not np.isin(bad, got[1]).any()
        nout, nidx, nmd, nst = sor(ctx, p, k, mul, negative=True)
        assert np.isin(bad, nidx).all() and np.array_equal(nidx, np.nonzero(~ref["inlier"])[0])
        assert np.array_equal(bits(nout), bits(p[nidx]))
    ref = R.radius(p, 1.5, 4)
    out, idx, cnt = ror(ctx, p, 1.5, 4)
    assert np.array_equal(cnt, ref["count"]) and (cnt[~fin] == 0).all() and np.array_equal(idx, ref["index"])
    out, nidx, cnt = ror(ctx, p, 1.5, 4, negative=True)
    assert np.isin(bad, nidx).all() and np.array_equal(np.sort(np.concatenate([idx, nidx])), np.arange(len(p)))
    # nothing finite at all
    q = np.full((5, 4), np.nan, F32)
    out, idx, md, st = sor(ctx, q, 1, 1.0)
    assert len(idx) == 0 and np.isnan(md).all() and st["n_valid"] == 0
    out, idx, cnt = ror(ctx, q, 1.0, 0)
    assert len(idx) == 0 and (cnt == 0).all()
    out, idx, cnt = ror(ctx, q, 1.0, 0, negative=True)
    assert list(idx) == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------ edges

def cloud(xyz):
    p = np.ones((len(xyz), 4), F32)
    p[:, :3] = np.asarray(xyz, F32)
    return p


def test_empty_cloud(ctx, view20k):
    e = np.ones((0, 4), F32)
    ctx.upload(1, view20k)
    out, idx, md, st = sor(ctx, e, 8, 1.0)
    assert len(out) == 0 and len(md) == 0 and st["n_valid"] == 0 and np.isnan(st["threshold"]) and ctx.size(1) == 0
    ctx.upload(1, view20k)
    out, idx, cnt = ror(ctx, e, 1.0, 1)
    assert len(out) == 0 and len(cnt) == 0 and ctx.size(1) == 0


def test_fewer_points_than_mean_k(ctx):
    rng = np.random.default_rng(9)
    p = cloud(rng.uniform(-5, 5, (10, 3)) + [0, 0, 900])
    out, idx, md, st = sor(ctx, p, 10, 1.0)              # n - 1 < mean_k
    assert np.array_equal(idx, np.arange(10)) and np.isnan(md).all() and st["n_valid"] == 0
    assert np.isnan(st["mean"]) and np.isnan(st["stddev"]) and np.isnan(st["threshold"]) and same_bits(out, p)
    out, idx, md, st = sor(ctx, p, 10, 1.0, negative=True)
    assert len(idx) == 0
    check_sor(p, sor(ctx, p, 9, 0.5), R.statistical(p, 9, 0.5))          # n - 1 == mean_k
    for n in (1, 2, 3):                                   # too few points for a grid
        for k in (1, 2, 3):
            check_sor(p[:n], sor(ctx, p[:n], k, 1.0), R.statistical(p[:n], k, 1.0), need_gap=False)
        out, idx, cnt = ror(ctx, p[:n], 100.0, n - 1)
        assert list(cnt) == [n - 1] * n and len(idx) == n


def test_all_points_at_one_location(ctx):
    p = cloud([[1.5, -2.0, 900.0]] * 300)
    out, idx, md, st = sor(ctx, p, 16, 1.0)
    assert (md == 0).all() and st["stddev"] == 0 and st["mean"] == 0 and st["threshold"] == 0 and st["n_valid"] == 300
    assert np.array_equal(idx, np.arange(300))            # 0 > 0 is false
    out, idx, cnt = ror(ctx, p, 0.5, 299)
    assert (cnt == 299).all() and len(idx) == 300
    out, idx, cnt = ror(ctx, p, 0.5, 300)
    assert len(idx) == 0


def test_exact_duplicates_inside_a_cloud(ctx, view20k):
    p = view20k.copy()
    p[100:140] = p[7]                                     # 41 copies of one point, scattered by index
    p[5000:5003] = p[9000]
    for k in (1, 8, 40, 41, 64):
        ctx.upload(0, p)
        n, md = ctx.statistical_outlier_removal(1, 0, k, 1.0, return_dist=True)
        ref, _ = R.mean_dist(p, k)
        assert same_bits(md, ref)
        assert md[7] == 0 if k <= 40 else md[7] > 0
    out, idx, cnt = ror(ctx, p, 1.0, 3)
    assert np.array_equal(cnt, R.neighbor_counts(p, 1.0)) and cnt[7] >= 40


def test_one_far_point_on_a_line(ctx):
    """x = 0 .. 4 and 14, mean_k = 2: mean distances 1.5, 1, 1, 1, 1.5, 10.5; mean 2.75; sum of squared deviations 72.375"""
    p = cloud([[x, 3.0, 900.0] for x in (0, 1, 2, 3, 4, 14)])
    out, idx, md, st = sor(ctx, p, 2, 1.0)
    assert list(md) == [1.5, 1.0, 1.0, 1.0, 1.5, 10.5]
    assert st["n_valid"] == 6 and st["mean"] == 2.75 and rel(st["stddev"], np.sqrt(72.375 / 5)) < 1e-15
    assert rel(st["threshold"], 2.75 + np.sqrt(72.375 / 5)) < 1e-15
    assert list(idx) == [0, 1, 2, 3, 4] and same_bits(out, p[:5])
    assert list(sor(ctx, p, 2, 1.0, negative=True)[1]) == [5]
    assert list(sor(ctx, p, 2, -0.4)[1]) == [1, 2, 3]
    out, idx, cnt = ror(ctx, p, 1.0, 2)
    assert list(cnt) == [1, 2, 2, 2, 1, 0] and list(idx) == [1, 2, 3]


# ------------------------------------------------------------------ grids and bookkeeping

def test_a_cloud_transformed_after_upload(ctx, mvr, view20k):
    p = small_case(view20k)
    sp = mvr.synth_params(12, 2)
    piv, ax = mvr.synth_prior(sp)
    ctx.upload(0, p)
    ctx.statistical_outlier_removal(1, 0, 8, 1.0)         # a grid over the uploaded coordinates exists
    T = mvr.axis_rotation(piv, ax, mvr.turntable_angle(5, 12))
    T[:3, 3] += [400.0, -250.0, 90.0]
    ctx.transform(0, 0, T)
    moved = ctx.download(0)
    assert not same_bits(moved, p)
    n, idx, md, st = ctx.statistical_outlier_removal(1, 0, 8, 1.0, return_index=True, return_dist=True, return_stats=True)
    ref = R.statistical(moved, 8, 1.0)
    check_sor(moved, (ctx.download(1), idx, md, st), ref)
    n, idx, cnt = ctx.radius_outlier_removal(1, 0, 1.5, 4, return_index=True, return_counts=True)
    rr = R.radius(moved, 1.5, 4)
    assert np.array_equal(cnt, rr["count"]) and np.array_equal(idx, rr["index"])


def test_merged_object_of_twelve_views(ctx, mvr):
    sp = mvr.synth_params(12, 2)
    piv, ax = mvr.synth_prior(sp)
    pts = []
    for v in range(12):
        ctx.upload(0, mvr.synth_view(sp, v, 200000))
        ctx.transform(0, 0, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, 12)))
        pts.append(ctx.download(0))
    p = np.concatenate(pts)
    assert len(p) == 2400000
    ref = R.statistical(p, 16, 2.0)
    print("merged object (16, 2.0): threshold %.4f, %d removed, gap %.1e" % (ref["stats"]["threshold"], int((~ref["inlier"]).sum()), ref["gap"]))
    check_sor(p, sor(ctx, p, 16, 2.0), ref)


def test_two_runs_give_identical_bytes(ctx, main_case):
    p, _ = main_case
    a = sor(ctx, p, 16, 2.0)
    b = sor(ctx, p, 16, 2.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert [np.float64(a[3][k]).tobytes() for k in ("mean", "stddev", "threshold")] == [np.float64(b[3][k]).tobytes() for k in ("mean", "stddev", "threshold")]
    a = ror(ctx, p, 0.45, 2)
    b = ror(ctx, p, 0.45, 2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_filtered_slot_is_an_ordinary_cloud(ctx, mvr, main_case):
    p, _ = main_case
    sp = mvr.synth_params(12, 2)
    piv, ax = mvr.synth_prior(sp)
    ctx.upload(0, p)
    ctx.nn(0, 0)                                          # orderings / grids of the source exist
    n, idx = ctx.statistical_outlier_removal(0, 0, 16, 2.0, return_index=True)      # in place: none of them may be reused
    assert same_bits(ctx.download(0), p[idx])
    ctx.upload(5, p[idx])
    i0, d0 = ctx.nn(0, 0)
    i5, d5 = ctx.nn(5, 5)
    assert np.array_equal(i0, i5) and same_bits(d0, d5)
    ctx.upload(6, mvr.synth_view(sp, 1, 200000))
    ctx.transform(6, 6, mvr.axis_rotation(piv, ax, mvr.turntable_angle(1, 12)))
    T0, st0, rc0 = ctx.icp_align(6, 0, 7, mvr.icp_params())
    T5, st5, rc5 = ctx.icp_align(6, 5, 7, mvr.icp_params())
    assert rc0 == rc5 == 0 and st0["n_corr"] == st5["n_corr"] > 1000 and np.array_equal(bits(T0), bits(T5))
    # the radius filter's output likewise, out of place
    ctx.upload(0, p)
    n, idx = ctx.radius_outlier_removal(2, 0, 0.45, 2, return_index=True)
    ctx.upload(5, p[idx])
    T0, st0, rc0 = ctx.icp_align(6, 2, 7, mvr.icp_params())
    T5, st5, rc5 = ctx.icp_align(6, 5, 7, mvr.icp_params())
    assert rc0 == rc5 == 0 and st0["n_corr"] == st5["n_corr"] > 1000 and np.array_equal(bits(T0), bits(T5))


def test_bad_parameters_change_nothing(ctx, mvr, view20k):
    ctx.upload(0, view20k)
    ctx.upload(1, view20k[:100])
    for k, mul in ((0, 1.0), (65, 1.0), (8, np.nan), (8, np.inf)):
        with pytest.raises(mvr.MvrError):
            ctx.statistical_outlier_removal(1, 0, k, mul)
    for r, m in ((0.0, 1), (-1.0, 1), (np.nan, 1), (np.inf, 1), (1.0, -1)):
        with pytest.raises(mvr.MvrError):
            ctx.radius_outlier_removal(1, 0, r, m)
    with pytest.raises(mvr.MvrError):
        ctx.statistical_outlier_removal(mvr.MAX_SLOTS, 0, 8, 1.0)
    assert same_bits(ctx.download(0), view20k) and same_bits(ctx.download(1), view20k[:100])


# ------------------------------------------------------------------ C++ layers

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#define MVR_ALIAS_PCL
#include "mvr/registrator.hpp"
static void ints(const char *key, const std::vector<int> &v, bool last = false)
{
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ",%d" : "%d", v[i]);
  std::printf(last ? "]" : "], ");
}
static void cloud_bits(const char *key, const pcl::PointCloud<pcl::PointXYZ> &c)
{
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < c.size(); ++i) {
    const float f[3] = {c[i].x, c[i].y, c[i].z};
    for (int j = 0; j < 3; ++j) { uint32_t b; std::memcpy(&b, &f[j], 4); std::printf(i || j ? ",%u" : "%u", b); }
  }
  std::printf("], ");
}
int main()
{
  mvr_synth_params sp; mvr_synth_default(&sp, 12, 2);
  const size_t n = 40000;
  std::vector<float> xyzw(4 * n), nrm(4 * n);
  mvr_synth_view(&sp, 0, n, xyzw.data(), nrm.data());
  for (size_t i = 0; i < n; i += 200) xyzw[4 * i + 2] += 7.0f;      // a flying pixel every 200 points
  mvr::ScanCloud scan;
  for (size_t i = 0; i < n; ++i) {
    scan.points.push_back(mvr::PointXYZ(xyzw[4 * i], xyzw[4 * i + 1], xyzw[4 * i + 2]));
    mvr::io::RichPoint q; q.x = xyzw[4 * i]; q.y = xyzw[4 * i + 1]; q.z = xyzw[4 * i + 2];
    q.r = (uint8_t)(i % 251); q.g = (uint8_t)((i * 13) % 256); q.b = (uint8_t)(255 - i % 200);
    q.normal_x = nrm[4 * i]; q.normal_y = nrm[4 * i + 1]; q.normal_z = nrm[4 * i + 2]; q.curvature = (float)i;
    scan.rich.push_back(q);
  }
  std::printf("{");
  {
    pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(scan.points));
    pcl::StatisticalOutlierRemoval<pcl::PointXYZ> sor(true);
    std::printf("\"sor_defaults\": [%d, %g, %d], ", sor.getMeanK(), sor.getStddevMulThresh(), (int)sor.getNegative());
    sor.setInputCloud(cloud); sor.setMeanK(16); sor.setStddevMulThresh(2.0);
    pcl::PointCloud<pcl::PointXYZ> out;
    sor.filter(out);
    cloud_bits("sor", out);
    ints("sor_removed", *sor.getRemovedIndices());
    std::vector<int> idx;
    sor.filter(idx);
    ints("sor_idx", idx);
    sor.setNegative(true);
    sor.filter(idx);
    ints("sor_neg_idx", idx);
    ints("sor_neg_removed", *sor.getRemovedIndices());
    sor.setNegative(false);
    sor.filter(*cloud);                                    // in place, PCL's idiom
    cloud_bits("sor_inplace", *cloud);
    pcl::StatisticalOutlierRemoval<pcl::PointXYZ> none;
    none.filter(out);
    std::printf("\"sor_none\": %zu, \"sor_plain_removed\": %zu, ", out.size(), none.getRemovedIndices()->size());
    pcl::PointCloud<pcl::PointXYZ>::Ptr keep(new pcl::PointCloud<pcl::PointXYZ>(scan.points));
    pcl::StatisticalOutlierRemoval<pcl::PointXYZ> bad;
    bad.setInputCloud(keep); bad.setMeanK(0);
    bad.filter(*keep);
    bad.filter(out);
    std::printf("\"sor_bad_inplace\": %zu, \"sor_bad\": %zu, ", keep->size(), out.size());
  }
  {
    pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(scan.points));
    pcl::RadiusOutlierRemoval<pcl::PointXYZ> ror(true);
    std::printf("\"ror_defaults\": [%d, %d], ", ror.getMinNeighborsInRadius(), (int)ror.getNegative());
    ror.setInputCloud(cloud); ror.setRadiusSearch(1.2); ror.setMinNeighborsInRadius(3);
    pcl::PointCloud<pcl::PointXYZ> out;
    ror.filter(out);
    cloud_bits("ror", out);
    ints("ror_removed", *ror.getRemovedIndices());
    std::vector<int> idx;
    ror.filter(idx);
    ints("ror_idx", idx);
    ror.filter(*cloud);
    cloud_bits("ror_inplace", *cloud);
    pcl::RadiusOutlierRemoval<pcl::PointXYZ> bad;
    bad.setInputCloud(cloud); bad.setRadiusSearch(-1.0);
    bad.filter(out);
    std::printf("\"ror_bad\": %zu, ", out.size());
  }
  {
    mvr::ScanCloud a = scan, b = scan;
    const size_t ra = a.removeStatisticalOutliers(16, 2.0), rb = b.removeRadiusOutliers(1.2, 3);
    std::vector<int> ca, cb;
    bool ok = a.rich.size() == a.points.size() && b.rich.size() == b.points.size();
    for (size_t i = 0; i < a.rich.size(); ++i) { ca.push_back((int)a.rich[i].curvature); ok = ok && a.rich[i].x == a.points[i].x && a.rich[i].z == a.points[i].z; }
    for (size_t i = 0; i < b.rich.size(); ++i) { cb.push_back((int)b.rich[i].curvature); ok = ok && b.rich[i].y == b.points[i].y; }
    ints("scan_sor", ca);
    ints("scan_ror", cb);
    const size_t bad = a.removeStatisticalOutliers(100, 1.0) + a.removeRadiusOutliers(0.0, 1);
    std::printf("\"scan_sor_removed\": %zu, \"scan_ror_removed\": %zu, \"scan_rich_ok\": %d, \"scan_bad\": %zu, \"scan_after_bad\": %zu", ra, rb, (int)ok, bad, a.points.size());
  }
  std::printf("}\n");
  return 0;
}
"""


def test_cxx_outlier_filters_and_scan_members(ctx, mvr, built, tmp_path):
    built.build_hip()
    src = tmp_path / "outlier_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "outlier_driver"
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout)
    p = mvr.synth_view(mvr.synth_params(12, 2), 0, 40000)
    p[::200, 2] += F32(7.0)
    n = len(p)
    assert out["sor_defaults"] == [1, 0, 0] and out["ror_defaults"] == [1, 0]
    assert "No input dataset given" in r.stderr and out["sor_none"] == 0 and out["sor_plain_removed"] == 0
    assert "mean_k (0) must be in 1..64" in r.stderr and out["sor_bad_inplace"] == n and out["sor_bad"] == 0
    assert "must be finite and > 0" in r.stderr and out["ror_bad"] == 0
    # pcl::StatisticalOutlierRemoval == Context.statistical_outlier_removal == the reference
    ref = R.statistical(p, 16, 2.0)
    assert ref["gap"] >= MIN_GAP
    ctx.upload(0, p)
    m, idx = ctx.statistical_outlier_removal(1, 0, 16, 2.0, return_index=True)
    assert np.array_equal(idx, ref["index"]) and np.isin(np.arange(0, n, 200), np.nonzero(~ref["inlier"])[0]).mean() > 0.9
    removed = np.nonzero(~ref["inlier"])[0]
    assert np.array_equal(np.asarray(out["sor"], np.uint32).reshape(-1, 3), bits(ctx.download(1)[:, :3]))
    assert np.array_equal(np.asarray(out["sor_inplace"], np.uint32), np.asarray(out["sor"], np.uint32))
    assert np.array_equal(out["sor_idx"], idx) and np.array_equal(out["sor_removed"], removed)
    assert np.array_equal(out["sor_neg_idx"], removed) and np.array_equal(out["sor_neg_removed"], idx)
    # pcl::RadiusOutlierRemoval
    rr = R.radius(p, 1.2, 3)
    m, ridx = ctx.radius_outlier_removal(1, 0, 1.2, 3, return_index=True)
    assert np.array_equal(ridx, rr["index"]) and 0 < len(ridx) < n
    assert np.array_equal(np.asarray(out["ror"], np.uint32).reshape(-1, 3), bits(ctx.download(1)[:, :3]))
    assert np.array_equal(np.asarray(out["ror_inplace"], np.uint32), np.asarray(out["ror"], np.uint32))
    assert np.array_equal(out["ror_idx"], ridx) and np.array_equal(out["ror_removed"], np.nonzero(~rr["inlier"])[0])
    # ScanCloud: the rich records (their curvature holds the original index) follow the kept points
    assert out["scan_rich_ok"] == 1 and out["scan_bad"] == 0 and out["scan_after_bad"] == len(idx)
    assert np.array_equal(out["scan_sor"], idx) and out["scan_sor_removed"] == n - len(idx)
    assert np.array_equal(out["scan_ror"], ridx) and out["scan_ror_removed"] == n - len(ridx)

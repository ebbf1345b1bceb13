"""GPU tests of the exact k-NN search and of the normal estimation (mvr_knn, mvr_cloud_estimate_normals; include/mvr_hip.h)
against the numpy reference of tests/normals_ref.py, scipy's kd-tree, the synthetic generator's analytic normals,
point-to-plane ICP and the C++ layer (pcl::NormalEstimation, ScanCloud::estimateNormals)."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import normals_ref as R
from conftest import PKG, ROOT, rand_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def view200k(mvr):
    sp = mvr.synth_params(12, 2)
    return mvr.synth_view(sp, 0, 200000, normals=True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ k-NN exactness

def _clouds(rng):
    a = rand_cloud(rng, 2000, scale=20.0)
    b = rand_cloud(rng, 2000, scale=20.0)
    dup = a.copy()
    dup[1000:] = dup[rng.integers(0, 1000, 1000)]          # every point of the second half repeats one of the first
    dup[500:700, :3] = np.round(dup[500:700, :3])          # ... and some more ties on a lattice
    return a, b, dup


@pytest.mark.parametrize("k", [1, 3, 8, 16, 32, 64])
def test_knn_bit_identical_to_brute_force(ctx, k):
    rng = np.random.default_rng(100 + k)
    a, b, dup = _clouds(rng)
    for q, t in ((a, a), (dup, dup), (a, b)):
        ctx.upload(0, q); ctx.upload(1, t)
        qs, ts = (0, 0) if q is t else (0, 1)
        idx, d2 = ctx.knn(qs, ts, k)
        ei, ed = R.knn_brute(q, t, k)
        assert np.array_equal(idx, ei)
        assert np.array_equal(bits(d2), bits(ed))


def test_knn_more_than_the_target_holds(ctx):
    rng = np.random.default_rng(7)
    q = rand_cloud(rng, 300, scale=10.0)
    for nt in (0, 1, 3, 5, 40):
        t = rand_cloud(rng, nt, scale=10.0)
        ctx.upload(0, q); ctx.upload(1, t)
        idx, d2 = ctx.knn(0, 1, 64)
        ei, ed = R.knn_brute(q, t, 64)
        assert np.array_equal(idx, ei) and np.array_equal(bits(d2), bits(ed))
        assert (idx[:, nt:] == 0xFFFFFFFF).all() and np.isinf(d2[:, nt:]).all()


@pytest.mark.parametrize("fma", [False, True])
def test_knn_k1_is_nn(ctx, fma):
    rng = np.random.default_rng(11)
    a, b, dup = _clouds(rng)
    for q, t in ((a, b), (dup, dup), (b, a)):
        ctx.upload(0, q); ctx.upload(1, t)
        idx, d2 = ctx.knn(0, 1, 1, fma=fma)
        ni, nd = ctx.nn(0, 1, fma=fma)
        assert np.array_equal(idx[:, 0], ni) and np.array_equal(bits(d2[:, 0]), bits(nd))
        if fma:                                     # the lists are ordered by (d2, index) under the fma distance too
            i8, d8 = ctx.knn(0, 1, 8, fma=True)
            key = (d8.view(np.uint32).astype(np.uint64) << np.uint64(32)) | i8.astype(np.uint64)
            assert (key[:, 1:] > key[:, :-1]).all()
            assert np.array_equal(i8[:, 0], ni)


def test_knn_200k_against_kdtree(ctx, view200k):
    """k = 16 on a 200k view against scipy's kd-tree (f64 distances): the sets agree except where the k-th and the
    (k+1)-th neighbour are closer to each other than the f32 rounding of d2 -- and there are next to none of those."""
    p, _ = view200k
    ctx.upload(0, p)
    idx, d2 = ctx.knn(0, 0, 16)
    ki, kd = R.knn_kdtree(p, 17)
    ref = np.sort(ki[:, :16], 1)
    got = np.sort(idx.astype(np.int64), 1)
    diff = np.nonzero((ref != got).any(1))[0]
    for i in diff:
        # a boundary near-tie: the 16th and 17th kd-tree distances within the f32 rounding of d2
        assert abs(kd[i, 16] - kd[i, 15]) <= 4e-7 * kd[i, 16] + 1e-12, (i, kd[i, 14:17])
        assert set(got[i]) ^ set(ref[i]) <= {ki[i, 15], ki[i, 16]}
    assert len(diff) <= 20, len(diff)
    assert (d2[:, 0] == 0).all()                       # the point itself (or a lower-index duplicate of it)
    assert np.array_equal(p[idx[:, 0], :3], p[:, :3]) and (idx[:, 0] <= np.arange(len(p))).all()


# ------------------------------------------------------------------ normals against the numpy reference

def _compare_to_reference(nrm, curv, ref, rc, w, p, vp=(0.0, 0.0, 0.0)):
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    ok = ~np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(nrm[:, 0]), ~ok) and np.array_equal(np.isnan(curv), ~ok)
    good = ok & (gap >= 1e-4)
    assert good.sum() > 0.99 * ok.sum()
    ang = R.angle_between(nrm[good], ref[good], unsigned=True)
    assert ang.max() <= 1e-5, ang.max()
    assert np.abs(curv[ok].astype(np.float64) - rc[ok]).max() <= 1e-6
    # identical orientation wherever the flip is not decided by rounding
    v = np.asarray(vp, np.float64)[None, :] - p[:, :3].astype(np.float64)
    cs = np.sum(v * ref[:, :3], 1)
    sure = good & (np.abs(cs) > 1e-4 * np.linalg.norm(v, axis=1))
    assert (np.sum(nrm[sure, :3] * ref[sure, :3], 1) > 0).all()


def test_normals_k16_match_reference(ctx, view200k):
    p, _ = view200k
    ctx.upload(0, p)
    curv = ctx.estimate_normals(0, k=16, curvature=True)
    nrm = ctx.download_normals(0)
    assert nrm.shape == (len(p), 4) and (nrm[:, 3] == 0).all()
    idx, _ = ctx.knn(0, 0, 16)                       # the same neighbour sets (exactness of those: the tests above)
    ref, rc, w = R.normals_from_lists(p, idx)
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    assert gap.min() >= 1e-4                           # every point of this view meets the bar at k = 16 (1.8e-2 measured)
    _compare_to_reference(nrm, curv, ref, rc, w, p)


def test_normals_radius_match_reference(ctx, view200k):
    p, _ = view200k
    ctx.upload(0, p)
    curv = ctx.estimate_normals(0, radius=1.0, curvature=True)
    nrm = ctx.download_normals(0)
    flat, offs = R.radius_sets(p, 1.0)
    ref, rc, w = R.normals_from_sets(p, flat, offs)
    _compare_to_reference(nrm, curv, ref, rc, w, p)


def test_normals_viewpoint_and_fma(ctx):
    rng = np.random.default_rng(5)
    p = rand_cloud(rng, 3000, scale=30.0)
    ctx.upload(0, p)
    vp = (10.0, -500.0, 200.0)
    for fma in (False, True):
        curv = ctx.estimate_normals(0, k=12, viewpoint=vp, curvature=True, fma=fma)
        nrm = ctx.download_normals(0)
        idx, _ = ctx.knn(0, 0, 12, fma=fma)
        ref, rc, w = R.normals_from_lists(p, idx, viewpoint=vp)
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
        good = gap >= 1e-4
        assert R.angle_between(nrm[good], ref[good], unsigned=True).max() <= 1e-5
        assert np.abs(curv.astype(np.float64) - rc).max() <= 1e-6
        v = np.asarray(vp)[None, :] - p[:, :3].astype(np.float64)
        cs = np.sum(v * nrm[:, :3], 1)
        assert (cs > -1e-5 * np.linalg.norm(v, axis=1)).all()       # towards the viewpoint (up to the f32 rounding of the test)


def test_normals_nan_with_fewer_than_three_neighbours(ctx):
    rng = np.random.default_rng(3)
    # a sparse cloud: isolated points, pairs, triples and a dense blob; radius 1 mm
    iso = rand_cloud(rng, 50, scale=200.0)
    pair = np.repeat(rand_cloud(rng, 20, scale=200.0), 2, 0); pair[1::2, 0] += 0.5
    tri = np.repeat(rand_cloud(rng, 20, scale=200.0), 3, 0); tri[1::3, 0] += 0.5; tri[2::3, 1] += 0.5
    blob = rand_cloud(rng, 200, scale=0.3)
    p = np.concatenate([iso, pair, tri, blob]).astype(np.float32)
    ctx.upload(0, p)
    curv = ctx.estimate_normals(0, radius=1.0, curvature=True)
    nrm = ctx.download_normals(0)
    flat, offs = R.radius_sets(p, 1.0)
    ref, rc, w = R.normals_from_sets(p, flat, offs)
    cnt = np.diff(offs)
    assert (cnt < 3).sum() >= 90 and (cnt >= 3).sum() >= 200
    assert np.array_equal(np.isnan(nrm[:, 0]), cnt < 3) and np.array_equal(np.isnan(curv), cnt < 3)
    assert np.isnan(nrm[cnt < 3, :3]).all()
    # k < 3: NaN everywhere
    curv = ctx.estimate_normals(0, k=2, curvature=True)
    assert np.isnan(ctx.download_normals(0)[:, :3]).all() and np.isnan(curv).all()


def test_normals_degenerate_neighbourhood(ctx):
    """all neighbours at one point: some finite unit vector and curvature 0"""
    p = np.zeros((40, 4), np.float32); p[:, 3] = 1; p[:, :3] = (1.0, 2.0, 3.0)
    ctx.upload(0, p)
    curv = ctx.estimate_normals(0, k=8, curvature=True)
    nrm = ctx.download_normals(0)
    assert np.isfinite(nrm).all() and np.allclose(np.linalg.norm(nrm[:, :3], axis=1), 1.0, atol=1e-6)
    assert (curv == 0).all()


def test_normals_arguments(ctx, mvr):
    ctx.upload(0, rand_cloud(np.random.default_rng(1), 100))
    for kw in (dict(), dict(k=8, radius=1.0), dict(k=65), dict(k=-1), dict(radius=-1.0)):
        with pytest.raises(mvr.MvrError) as e:
            ctx.estimate_normals(0, **kw)
        assert e.value.status == mvr.E_ARG
    with pytest.raises(mvr.MvrError):
        ctx.estimate_normals([0, 0], k=8)
    with pytest.raises(mvr.MvrError):
        ctx.estimate_normals([0, 300], k=8)
    for k in (0, 65):
        with pytest.raises(mvr.MvrError):
            ctx.knn(0, 0, k)
    ctx.clear(5)
    assert ctx.estimate_normals(5, k=8) is None          # an empty slot: nothing to do


# ------------------------------------------------------------------ against the analytic normals

@pytest.mark.parametrize("kw, med, p99", [(dict(k=16), 5.0, 15.0), (dict(k=32), 2.5, 6.5),
                                          (dict(radius=1.0), 4.5, 14.0), (dict(radius=1.5), 2.0, 5.0)])
def test_normals_against_analytic(ctx, view200k, kw, med, p99):
    p, an = view200k
    ctx.upload(0, p)
    ctx.estimate_normals(0, **kw)
    nrm = ctx.download_normals(0)
    ok = ~np.isnan(nrm[:, 0])
    assert ok.all()
    ang = np.degrees(R.angle_between(nrm, an, unsigned=True))
    assert np.median(ang) < med and np.percentile(ang, 99) < p99, (np.median(ang), np.percentile(ang, 99))
    v = -p[:, :3].astype(np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    faces = np.sum(an[:, :3] * v, 1) > 0.2
    opposite = np.sum(np.sum(nrm[:, :3] * an[:, :3], 1)[faces] < 0)
    assert opposite < 1e-3 * faces.sum(), opposite


# ------------------------------------------------------------------ point-to-plane end to end

def test_point_to_plane_with_estimated_normals(ctx, mvr, view200k):
    """config-2 pair: target normals estimated on the GPU (slot 0) vs the numpy reference's normals uploaded (slot 3)"""
    tgt, _ = view200k
    sp = mvr.synth_params(12, 2)
    raw = mvr.synth_view(sp, 1, 200000)
    piv, ax = mvr.synth_prior(sp)
    prior = mvr.axis_rotation(piv, ax, mvr.turntable_angle(1, 12))
    ctx.upload(0, tgt)
    ctx.estimate_normals(0, k=16)
    idx, _ = ctx.knn(0, 0, 16)
    ref, _, _ = R.normals_from_lists(tgt, idx)
    ctx.upload(3, tgt); ctx.upload_normals(3, ref)
    ctx.upload(1, raw); ctx.transform(1, 1, prior)
    for kw in (dict(), dict(max_iter=4, teps=0.0, feps=-1e300)):
        T0, st0, rc0 = ctx.icp_align(1, 0, 2, mvr.icp_params(point_to_plane=True, **kw))
        T1, st1, rc1 = ctx.icp_align(1, 3, 4, mvr.icp_params(point_to_plane=True, **kw))
        assert rc0 == 0 and rc1 == 0
        assert st0["n_corr"] == st1["n_corr"] and st0["iterations"] == st1["iterations"] and st0["n_corr"] > 30000
        assert np.abs(T0[:3, :3] - T1[:3, :3]).max() < 1e-5 and np.abs(T0[:3, 3] - T1[:3, 3]).max() < 1e-4


# ------------------------------------------------------------------ bookkeeping

def test_multi_slot_call_equals_per_slot_calls(ctx, mvr):
    sp = mvr.synth_params(12, 2)
    views = [mvr.synth_view(sp, v, 20000 + 1000 * v) for v in range(3)]
    small = rand_cloud(np.random.default_rng(2), 3)
    for mode in (dict(k=16), dict(radius=1.0)):
        for s, v in enumerate(views + [small]):
            ctx.upload(10 + s, v)
        curv = ctx.estimate_normals([10, 11, 12, 13], curvature=True, **mode)
        many = [ctx.download_normals(10 + s) for s in range(4)]
        for s in range(4):
            c1 = ctx.estimate_normals(10 + s, curvature=True, **mode)
            assert np.array_equal(bits(ctx.download_normals(10 + s)), bits(many[s]))
            assert np.array_equal(bits(c1), bits(curv[s]))


def test_more_slots_than_one_launch_holds(ctx, mvr):
    sp = mvr.synth_params(20, 1)
    views = [mvr.synth_view(sp, v, 3000) for v in range(20)]
    for s, v in enumerate(views):
        ctx.upload(20 + s, v)
    curv = ctx.estimate_normals(list(range(20, 40)), k=10, curvature=True)
    for s, v in enumerate(views):
        idx, _ = ctx.knn(20 + s, 20 + s, 10)
        ref, rc, w = R.normals_from_lists(v, idx)
        good = (w[:, 1] - w[:, 0]) / w[:, 2] >= 1e-4
        assert R.angle_between(ctx.download_normals(20 + s)[good], ref[good], unsigned=True).max() <= 1e-5
        assert np.abs(curv[s].astype(np.float64) - rc).max() <= 1e-6


def test_transformed_normals_equal_estimate_after_transform(ctx, mvr, view200k):
    p, _ = view200k
    sp = mvr.synth_params(12, 2)
    piv, ax = mvr.synth_prior(sp)
    T = mvr.axis_rotation(piv, ax, mvr.turntable_angle(3, 12))
    ctx.upload(0, p)
    ctx.estimate_normals(0, k=16)
    ctx.transform(1, 0, T)                       # the normals ride along (rotated)
    moved = ctx.download_normals(1)
    ctx.copy(2, 1)
    ctx.estimate_normals(2, k=16)                # estimated in the new frame
    fresh = ctx.download_normals(2)
    i0, d0 = ctx.knn(0, 0, 17)
    i2, _ = ctx.knn(2, 2, 16)
    same = (np.sort(i0[:, :16], 1) == np.sort(i2, 1)).all(1)
    # where the sets differ, the 16th and 17th neighbour are a near-tie that the f32 rounding of the moved coordinates
    # (3e-5 mm at 900 mm) can swap -- and there are next to none of them (52 of 200 000 measured)
    gap = np.sqrt(d0[~same, 16].astype(np.float64)) - np.sqrt(d0[~same, 15].astype(np.float64))
    assert (gap <= 2e-4).all(), gap.max()
    assert (~same).sum() <= 1e-3 * len(p), (~same).sum()
    ang = R.angle_between(moved[same], fresh[same], unsigned=True)
    # the moved coordinates are f32 roundings of the motion (3e-5 mm at 900 mm): that alone turns a normal by up to a few
    # 1e-4 rad where the neighbourhood is nearly isotropic.  The same happens to the numpy reference on the same inputs, and
    # the GPU must not add to it: rotated original normals vs normals of the moved coordinates, GPU against reference
    R3 = np.asarray(T, np.float64)[:3, :3]
    ref0, _, w0 = R.normals_from_lists(p, i0[:, :16])
    ref2, _, _ = R.normals_from_lists(ctx.download(2), i2)
    ang_ref = R.angle_between(ref0[same, :3] @ R3.T, ref2[same], unsigned=True)
    assert np.median(ang) <= 1e-5 and (ang <= ang_ref + 2e-5).all(), (np.median(ang), (ang - ang_ref).max())
    # and the normals that rode along are the original ones, rotated
    orig = ctx.download_normals(0)
    assert R.angle_between(orig[:, :3].astype(np.float64) @ R3.T, moved, unsigned=True).max() <= 1e-6


def test_new_upload_drops_estimated_normals(ctx):
    p = rand_cloud(np.random.default_rng(4), 500, scale=10.0)
    ctx.upload(0, p)
    ctx.estimate_normals(0, k=8)
    assert len(ctx.download_normals(0)) == 500
    ctx.upload(0, p)
    assert len(ctx.download_normals(0)) == 0


# ------------------------------------------------------------------ C++ layer

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#define MVR_ALIAS_PCL
#include "mvr/registrator.hpp"
int main(int argc, char **argv)
{
  mvr_synth_params sp; mvr_synth_default(&sp, 12, 2);
  const size_t n = 20000;
  std::vector<float> xyzw(4 * n);
  mvr_synth_view(&sp, 0, n, xyzw.data(), nullptr);
  mvr::ScanCloud sc;
  for (size_t i = 0; i < n; ++i) sc.points.push_back(mvr::PointXYZ(xyzw[4 * i], xyzw[4 * i + 1], xyzw[4 * i + 2]));
  sc.estimateNormals(16);
  const std::string f = std::string(argv[1]) + "/scan.pcd";
  if (!sc.save(f)) return 2;
  mvr::io::RichCloud back;
  if (!mvr::io::loadPCDFile(f, back) || back.size() != n) return 3;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(sc.points));
  pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
  pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>());
  ne.setInputCloud(cloud); ne.setSearchMethod(tree); ne.setRadiusSearch(3.0);
  pcl::PointCloud<pcl::Normal> normals;
  ne.compute(normals);
  if (normals.size() != n) return 4;
  auto num = [](float v) { if (std::isnan(v)) std::printf("NaN"); else std::printf("%.9g", v); };
  auto row = [&](size_t i, float a, float b, float c, float d) { std::printf(i ? ", [" : "["); num(a); std::printf(", "); num(b); std::printf(", "); num(c); std::printf(", "); num(d); std::printf("]"); };
  std::printf("{\"pcd\": [");
  for (size_t i = 0; i < n; ++i) row(i, back[i].normal_x, back[i].normal_y, back[i].normal_z, back[i].curvature);
  std::printf("], \"ne\": [");
  for (size_t i = 0; i < n; ++i) row(i, normals[i].normal_x, normals[i].normal_y, normals[i].normal_z, normals[i].curvature);
  std::printf("]}\n");
  return 0;
}
"""


def test_scancloud_estimate_normals_save_round_trip(ctx, mvr, built, tmp_path):
    built.build_hip()
    src = tmp_path / "normals_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "normals_driver"
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout)
    sp = mvr.synth_params(12, 2)
    p = mvr.synth_view(sp, 0, 20000)
    ctx.upload(0, p)
    curv = ctx.estimate_normals(0, k=16, curvature=True)
    nrm = ctx.download_normals(0)
    pcd = np.asarray(out["pcd"], np.float32)
    assert np.array_equal(bits(pcd[:, :3]), bits(nrm[:, :3])) and np.array_equal(bits(pcd[:, 3]), bits(curv))
    curv = ctx.estimate_normals(0, radius=3.0, curvature=True)
    nrm = ctx.download_normals(0)
    ne = np.asarray(out["ne"], np.float32)
    assert np.array_equal(np.isnan(ne[:, 0]), np.isnan(nrm[:, 0]))
    ok = ~np.isnan(nrm[:, 0])
    assert np.array_equal(bits(ne[ok, :3]), bits(nrm[ok, :3])) and np.array_equal(bits(ne[ok, 3]), bits(curv[ok]))

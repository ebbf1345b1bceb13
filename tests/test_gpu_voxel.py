"""GPU tests of the voxel-grid downsampling (mvr_cloud_voxel_grid; rules in include/mvr_hip.h) against the numpy reference of
tests/voxel_ref.py, and of its C++ layers (pcl::VoxelGrid, ScanCloud::voxelDownsample, saveRegisteredPoints with a leaf)."""
import importlib
import json
import os
import subprocess
import time
import warnings

import numpy as np
import pytest

import voxel_ref as R
from conftest import PKG, ROOT, rand_cloud
from pcd_py import read_pcd

pytestmark = pytest.mark.gpu

F32 = np.float32


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


@pytest.fixture(scope="module")
def merged(mvr, ctx):
    """the twelve 200k views posed by their turntable prior and concatenated (2.4 M points), with their rotated normals"""
    sp = mvr.synth_params(12, 2)
    piv, ax = mvr.synth_prior(sp)
    pts, nrm = [], []
    for v in range(12):
        p, n = mvr.synth_view(sp, v, 200000, normals=True)
        ctx.upload(0, p)
        ctx.upload_normals(0, n)
        ctx.transform(0, 0, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, 12)))
        pts.append(ctx.download(0))
        nrm.append(ctx.download_normals(0))
    return np.concatenate(pts), np.concatenate(nrm)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulps(a, b):
    """distance in units in the last place between two f32 arrays of finite values"""
    ia, ib = bits(a).astype(np.int64), bits(b).astype(np.int64)
    ia = np.where(ia >= 2 ** 31, 2 ** 31 - ia, ia)
    ib = np.where(ib >= 2 ** 31, 2 ** 31 - ib, ib)
    return np.abs(ia - ib)


def run(ctx, p, leaf, min_points=0, normals=None, dst=1, src=0):
    ctx.upload(src, p)
    if normals is not None:
        ctx.upload_normals(src, normals)
    n, vmap = ctx.voxel_grid(dst, src, leaf, min_points=min_points, return_map=True)
    out = ctx.download(dst)
    nrm = ctx.download_normals(dst)
    assert len(out) == n
    return out, nrm, vmap


def check(out, nrm, vmap, ref, exact=False):
    assert len(out) == len(ref["pts"])
    assert np.array_equal(vmap, ref["voxel_of"])
    assert (out[:, 3] == 1).all()
    if exact:
        assert np.array_equal(bits(out), bits(ref["pts"]))
    else:
        assert ulps(out[:, :3], ref["pts"][:, :3]).max(initial=0) <= 1
    if ref["nrm"] is None:
        assert len(nrm) == 0
    else:
        assert len(nrm) == len(out) and (nrm[:, 3] == 0).all()
        ok = ~np.isnan(ref["nrm"][:, 0])
        assert np.array_equal(np.isnan(nrm[:, :3]), np.isnan(ref["nrm"][:, :3]))
        assert ulps(nrm[ok, :3], ref["nrm"][ok, :3]).max(initial=0) <= 2
        a, b = nrm[ok, :3].astype(np.float64), ref["nrm"][ok, :3].astype(np.float64)
        nz = np.linalg.norm(b, axis=1) > 0
        cosv = np.clip(np.sum(a[nz] * b[nz], 1) / (np.linalg.norm(a[nz], axis=1) * np.linalg.norm(b[nz], axis=1)), -1, 1)
        assert np.arccos(cosv).max(initial=0) <= 1e-6
        assert (np.linalg.norm(a[~nz], axis=1) == 0).all()


def unit_normals(rng, n):
    v = rng.standard_normal((n, 4))
    v[:, 3] = 0
    v[:, :3] /= np.linalg.norm(v[:, :3], axis=1, keepdims=True)
    return v.astype(F32)


# ------------------------------------------------------------------ structure and centroids

@pytest.mark.parametrize("leaf", [2.0, 5.0, 17.0, (1.0, 4.0, 9.5), (30.0, 0.75, 3.0)])
def test_structure_and_centroids_match_reference(ctx, leaf):
    rng = np.random.default_rng(int(np.sum(leaf) * 10))
    p = rand_cloud(rng, 50000, scale=40.0, centre=(-20.0, 35.0, 900.0))
    out, nrm, vmap = run(ctx, p, leaf)
    ref = R.voxel_grid(p, leaf)
    assert len(ref["pts"]) > 100
    check(out, nrm, vmap, ref)


def test_lattice_inputs_are_bit_identical(ctx):
    """coordinates that are multiples of 2^-8 mm: every summation order is exact, so the centroids agree bit for bit"""
    rng = np.random.default_rng(3)
    p = np.ones((300000, 4), F32)
    p[:, :3] = (rng.integers(-40000, 40000, (300000, 3)) / 256.0).astype(F32)
    for leaf in (1.0, 3.0, (0.5, 2.0, 8.0), 400.0):
        out, nrm, vmap = run(ctx, p, leaf)
        check(out, nrm, vmap, R.voxel_grid(p, leaf), exact=True)


def test_min_points(ctx):
    rng = np.random.default_rng(5)
    p = rand_cloud(rng, 40000, scale=10.0)
    nr = unit_normals(rng, 40000)
    for m in (0, 1, 2, 5, 20, 100000):
        out, nrm, vmap = run(ctx, p, 1.5, min_points=m, normals=nr)
        ref = R.voxel_grid(p, 1.5, min_points=m, normals=nr)
        check(out, nrm, vmap, ref)
        assert m < 100000 or len(out) == 0


# ------------------------------------------------------------------ normals

def test_normals_match_reference(ctx, view200k):
    p, nr = view200k
    for leaf in (0.5, 2.0, (1.0, 3.0, 0.7)):
        out, nrm, vmap = run(ctx, p, leaf, normals=nr)
        check(out, nrm, vmap, R.voxel_grid(p, leaf, normals=nr))


def test_normals_zero_sum_and_nan(ctx):
    p = np.ones((6, 4), F32)
    p[:, :3] = [[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [5.1, 0.1, 0.1], [5.2, 0.2, 0.2], [9.5, 0.5, 0.5], [9.6, 0.6, 0.6]]
    nr = np.zeros((6, 4), F32)
    nr[:, :3] = [[0, 0, 1], [0, 0, -1], [0, 1, 0], [np.nan, 0, 0], [0.6, 0.8, 0], [0.6, 0.8, 0]]
    out, nrm, vmap = run(ctx, p, 1.0, normals=nr)
    assert len(out) == 3 and list(vmap) == [0, 0, 1, 1, 2, 2]
    assert np.array_equal(nrm[0], F32([0, 0, 0, 0])) and not np.signbit(nrm[0, :3]).any()
    assert np.isnan(nrm[1, :3]).all()
    assert np.array_equal(nrm[2, :3], F32([0.6, 0.8, 0]))
    check(out, nrm, vmap, R.voxel_grid(p, 1.0, normals=nr))


# ------------------------------------------------------------------ edge cases

def test_non_finite_points_are_skipped(ctx):
    rng = np.random.default_rng(9)
    p = rand_cloud(rng, 20000, scale=15.0)
    bad = rng.choice(20000, 3000, replace=False)
    p[bad[:1000], 0] = np.nan
    p[bad[1000:2000], 1] = np.inf
    p[bad[2000:], 2] = -np.inf
    p[bad[2000:2010], :3] = 1e30          # finite, far away: widen the box
    nr = unit_normals(rng, 20000)
    out, nrm, vmap = run(ctx, p, 1e28, normals=nr)
    ref = R.voxel_grid(p, 1e28, normals=nr)
    check(out, nrm, vmap, ref)
    p[bad[2000:2010], :3] = -np.inf
    for leaf in (1.0, (2.0, 0.5, 1.0)):
        out, nrm, vmap = run(ctx, p, leaf, normals=nr)
        ref = R.voxel_grid(p, leaf, normals=nr)
        check(out, nrm, vmap, ref)
        assert (vmap[bad] == R.NONE).all()


def test_empty_and_all_nan(ctx):
    ctx.clear(0)
    n, vmap = ctx.voxel_grid(1, 0, 1.0, return_map=True)
    assert n == 0 and len(vmap) == 0 and ctx.size(1) == 0
    p = np.full((500, 4), np.nan, F32)
    out, nrm, vmap = run(ctx, p, 1.0)
    assert len(out) == 0 and (vmap == R.NONE).all() and len(nrm) == 0


def test_one_voxel_holding_every_point(ctx, merged):
    """2.4 M points in one voxel: the long-voxel path spreads it over many blocks"""
    p, nr = merged
    lattice = p.copy()                       # on the 2^-8 lattice, every coordinate in [1, 1e4): one voxel of leaf 1e4
    lattice[:, :3] = np.round((p[:, :3] - p[:, :3].min(0) + 1.0) * 256.0) / 256.0
    ctx.upload(0, lattice)
    ctx.upload_normals(0, nr)
    ctx.voxel_grid(1, 0, 1.0e4)             # warm
    t0 = time.perf_counter()
    n, vmap = ctx.voxel_grid(1, 0, 1.0e4, return_map=True)
    dt = time.perf_counter() - t0
    assert n == 1 and (vmap == 0).all()
    assert dt < 5.0, dt
    ref = R.voxel_grid(lattice, 1.0e4, normals=nr)
    check(ctx.download(1), ctx.download_normals(1), vmap, ref, exact=True)


def test_overflow_passthrough_is_a_copy(ctx, mvr):
    rng = np.random.default_rng(11)
    p = rand_cloud(rng, 5000, scale=300.0)
    p[::50, 1] = np.nan
    nr = unit_normals(rng, 5000)
    nr[7] = np.nan
    ctx.upload(0, p)
    ctx.upload_normals(0, nr)
    with pytest.warns(UserWarning, match="Integer indices would overflow"):
        n, vmap = ctx.voxel_grid(1, 0, 1e-4, return_map=True)
    assert n == 5000 and np.array_equal(vmap, np.arange(5000, dtype=np.uint32))
    assert np.array_equal(bits(ctx.download(1)), bits(p)) and np.array_equal(bits(ctx.download_normals(1)), bits(nr))
    assert R.voxel_grid(p, 1e-4)["passthrough"]
    import ctypes as C
    leaf = (C.c_float * 3)(1e-4, 1e-4, 1e-4)
    cnt, flag = C.c_size_t(), C.c_int()
    assert mvr._lib.mvr_cloud_voxel_grid(ctx._h, 2, 0, leaf, 0, C.byref(cnt), None, C.byref(flag)) == mvr.OK
    assert flag.value == 1 and cnt.value == 5000
    # in place, too
    with pytest.warns(UserWarning):
        assert ctx.voxel_grid(0, 0, 1e-4) == 5000
    assert np.array_equal(bits(ctx.download(0)), bits(p)) and np.array_equal(bits(ctx.download_normals(0)), bits(nr))


OVERFLOW_CASES = [
    # (points, leaf, passthrough): PCL's rule from both sides (d = (2^11, 2^10, 2^10 - 1) and (2^11, 2^10, 2^10)), one axis
    # at 2^31 and just below, and the 2^62 bound of the bound products
    ([[0, 0, 0], [2047, 1023, 1022], [5, 5, 5]], 1.0, False),
    ([[0, 0, 0], [2047, 1023, 1023], [np.nan, 1, 1]], 1.0, True),
    ([[0, 0, 0], [2.0 ** 31, 0, 0]], 1.0, True),
    ([[0, 0, 0], [2.0 ** 31 - 256, 0, 0], [7.5, 0, 0]], 1.0, False),
    ([[2.0 ** 62, 0, 0], [2.0 ** 62, 1, 1]], 1.0, True),
    ([[2.0 ** 61, 0, 0], [2.0 ** 61, 1, 1], [2.0 ** 61, 0.5, 0.5]], 1.0, False),
    ([[0, 0, 0], [2047, 1023, 1022]], (0.5, 0.5, 1.0), True),          # the same box at half the leaf on two axes
]


@pytest.mark.parametrize("case", range(len(OVERFLOW_CASES)))
def test_overflow_threshold_on_the_gpu(ctx, case):
    pts, leaf, expect = OVERFLOW_CASES[case]
    p = np.ones((len(pts), 4), F32)
    p[:, :3] = np.asarray(pts, np.float64).astype(F32)
    ref = R.voxel_grid(p, leaf)
    assert ref["passthrough"] == expect
    ctx.upload(0, p)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        n, vmap = ctx.voxel_grid(1, 0, leaf, return_map=True)
    assert any("Integer indices would overflow" in str(x.message) for x in w) == expect
    out = ctx.download(1)
    assert n == len(ref["pts"]) and np.array_equal(vmap, ref["voxel_of"])
    assert np.array_equal(bits(out), bits(ref["pts"]))


def test_index_beyond_32_bits(ctx):
    """a 46.34 m x 46.34 m patch at a 1 mm leaf with z across one face: d = (46340, 46340, 1) passes PCL's rule, but
    div = (46341, 46341, 2) puts the largest index above 2^32 -- the 64-bit key path"""
    rng = np.random.default_rng(21)
    n = 300000
    p = np.ones((n, 4), F32)
    p[:, 0] = rng.uniform(0.5, 46340.4, n)
    p[:, 1] = rng.uniform(0.5, 46340.4, n)
    p[:, 2] = rng.uniform(-0.25, 0.25, n)
    p[:4, :3] = [[0.5, 0.5, -0.25], [46340.4, 46340.4, 0.25], [46340.3, 46340.2, 0.2], [46340.1, 46339.9, 0.1]]
    p[1000:1010, 1] = np.nan
    nr = unit_normals(rng, n)
    passthrough, geo = R.overflow(p, 1.0)
    assert not passthrough and list(geo[2]) == [46341, 46341, 2]
    ref = R.voxel_grid(p, 1.0, normals=nr)
    assert int(ref["idx"].max()) >= 2 ** 32 and (ref["idx"] < 2 ** 32).any()
    out, nrm, vmap = run(ctx, p, 1.0, normals=nr)
    check(out, nrm, vmap, ref)
    out2, _, vmap2 = run(ctx, p, 1.0, min_points=2)
    check(out2, np.zeros((0, 4), F32), vmap2, R.voxel_grid(p, 1.0, min_points=2))


# ------------------------------------------------------------------ slots and arguments

def test_in_place_and_src_untouched(ctx):
    rng = np.random.default_rng(13)
    p = rand_cloud(rng, 30000, scale=20.0)
    nr = unit_normals(rng, 30000)
    out, nrm, vmap = run(ctx, p, 2.0, normals=nr, dst=1, src=0)
    assert np.array_equal(bits(ctx.download(0)), bits(p)) and np.array_equal(bits(ctx.download_normals(0)), bits(nr))
    n = ctx.voxel_grid(0, 0, 2.0)
    assert n == len(out)
    assert np.array_equal(bits(ctx.download(0)), bits(out)) and np.array_equal(bits(ctx.download_normals(0)), bits(nrm))


def test_bad_leaf_or_slot_changes_nothing(ctx, mvr):
    rng = np.random.default_rng(17)
    p, q = rand_cloud(rng, 1000, scale=5.0), rand_cloud(rng, 700, scale=5.0)
    ctx.upload(0, p)
    ctx.upload(1, q)
    for leaf in (0.0, -1.0, np.nan, np.inf, (1.0, 0.0, 1.0), (1.0, 1.0, -np.inf)):
        with pytest.raises(mvr.MvrError) as e:
            ctx.voxel_grid(1, 0, leaf)
        assert e.value.status == mvr.E_ARG
    for dst, src in ((300, 0), (1, -1), (-1, 0), (1, 256)):
        with pytest.raises(mvr.MvrError) as e:
            ctx.voxel_grid(dst, src, 1.0)
        assert e.value.status == mvr.E_ARG
    assert np.array_equal(bits(ctx.download(0)), bits(p)) and np.array_equal(bits(ctx.download(1)), bits(q))


def test_two_calls_are_bit_identical(ctx, merged):
    p, nr = merged
    a = run(ctx, p, 1.0, normals=nr)
    b = run(ctx, p, 1.0, normals=nr)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------------ full size

@pytest.mark.parametrize("leaf", [0.5, 1.0, 2.0])
def test_view200k_against_reference(ctx, view200k, leaf):
    p, nr = view200k
    out, nrm, vmap = run(ctx, p, leaf, normals=nr)
    check(out, nrm, vmap, R.voxel_grid(p, leaf, normals=nr))


def test_merged_24m_against_reference(ctx, merged):
    p, nr = merged
    out, nrm, vmap = run(ctx, p, 1.0, normals=nr)
    ref = R.voxel_grid(p, 1.0, normals=nr)
    assert len(out) < len(p) // 2
    check(out, nrm, vmap, ref)


# ------------------------------------------------------------------ the output is a fresh point set

def test_output_behaves_as_a_fresh_upload(ctx, mvr, view200k):
    p, nr = view200k
    sp = mvr.synth_params(12, 2)
    piv, ax = mvr.synth_prior(sp)
    ctx.upload(0, p)
    ctx.upload_normals(0, nr)
    ctx.nn(0, 0)                                 # orderings / grids of the source exist
    ctx.voxel_grid(0, 0, 1.0)                    # in place: what was built for the old set must not be reused
    out = ctx.download(0)
    ctx.upload(5, out)
    i0, d0 = ctx.nn(0, 0)
    i5, d5 = ctx.nn(5, 5)
    assert np.array_equal(i0, i5) and np.array_equal(bits(d0), bits(d5))
    k0, e0 = ctx.knn(0, 0, 8)
    k5, e5 = ctx.knn(5, 5, 8)
    assert np.array_equal(k0, k5) and np.array_equal(bits(e0), bits(e5))
    c0 = ctx.estimate_normals(0, k=16, curvature=True)
    c5 = ctx.estimate_normals(5, k=16, curvature=True)
    assert np.array_equal(bits(c0), bits(c5)) and np.array_equal(bits(ctx.download_normals(0)), bits(ctx.download_normals(5)))
    raw = mvr.synth_view(sp, 1, 200000)
    ctx.upload(6, raw)
    ctx.voxel_grid(6, 6, 1.0)
    ctx.transform(6, 6, mvr.axis_rotation(piv, ax, mvr.turntable_angle(1, 12)))
    T0, st0, rc0 = ctx.icp_align(6, 0, 7, mvr.icp_params())
    T5, st5, rc5 = ctx.icp_align(6, 5, 7, mvr.icp_params())
    assert rc0 == rc5 == 0 and st0["n_corr"] == st5["n_corr"] and np.array_equal(T0, T5)


# ------------------------------------------------------------------ C++ layers

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#define MVR_ALIAS_PCL
#include "mvr/registrator.hpp"
static void row(const char *key, const std::vector<float> &v, bool last = false)
{
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) { uint32_t b; std::memcpy(&b, &v[i], 4); std::printf(i ? ",%u" : "%u", b); }
  std::printf(last ? "]" : "], ");
}
int main(int argc, char **argv)
{
  const std::string dir = argv[1];
  mvr_synth_params sp; mvr_synth_default(&sp, 4, 2);
  const size_t n = 40000;
  std::vector<float> xyzw(4 * n), nrm(4 * n);
  mvr::TurntableModel model; model.views.resize(4);
  for (int v = 0; v < 4; ++v) {
    mvr_synth_view(&sp, v, n, xyzw.data(), nrm.data());
    mvr::ScanCloud &sc = model.views[v];
    sc.view = v;
    for (size_t i = 0; i < n; ++i) {
      sc.points.push_back(mvr::PointXYZ(xyzw[4 * i], xyzw[4 * i + 1], xyzw[4 * i + 2]));
      mvr::io::RichPoint q; q.x = xyzw[4 * i]; q.y = xyzw[4 * i + 1]; q.z = xyzw[4 * i + 2];
      q.r = (uint8_t)((i * 7 + v) % 256); q.g = (uint8_t)((i * 13) % 256); q.b = (uint8_t)(255 - i % 200);
      q.normal_x = nrm[4 * i]; q.normal_y = nrm[4 * i + 1]; q.normal_z = nrm[4 * i + 2]; q.curvature = (float)((i % 97) * 0.001);
      sc.rich.push_back(q);
    }
  }
  std::printf("{");
  // pcl::VoxelGrid on view 0
  {
    pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(model.views[0].points));
    pcl::VoxelGrid<pcl::PointXYZ> vg;
    vg.setInputCloud(cloud); vg.setLeafSize(1.0f, 1.5f, 0.75f); vg.setMinimumPointsNumberPerVoxel(2);
    pcl::PointCloud<pcl::PointXYZ> out;
    vg.filter(out);
    std::vector<float> v;
    for (size_t i = 0; i < out.size(); ++i) { v.push_back(out[i].x); v.push_back(out[i].y); v.push_back(out[i].z); }
    row("vg", v);
    pcl::VoxelGrid<pcl::PointXYZ> none;
    none.filter(out);
    std::printf("\"vg_none\": %zu, ", out.size());
    // in place, PCL's idiom: the input cloud is also the output
    pcl::PointCloud<pcl::PointXYZ>::Ptr same(new pcl::PointCloud<pcl::PointXYZ>(model.views[0].points));
    pcl::VoxelGrid<pcl::PointXYZ> vgi;
    vgi.setInputCloud(same); vgi.setLeafSize(1.0f, 1.5f, 0.75f); vgi.setMinimumPointsNumberPerVoxel(2);
    vgi.filter(*same);
    v.clear();
    for (size_t i = 0; i < same->size(); ++i) { v.push_back((*same)[i].x); v.push_back((*same)[i].y); v.push_back((*same)[i].z); }
    row("vg_inplace", v);
    // a bad leaf in place leaves the input as it was
    pcl::PointCloud<pcl::PointXYZ>::Ptr keep(new pcl::PointCloud<pcl::PointXYZ>(model.views[0].points));
    pcl::VoxelGrid<pcl::PointXYZ> bad;
    bad.setInputCloud(keep); bad.setLeafSize(1.0f, 0.0f, 1.0f);
    bad.filter(*keep);
    std::printf("\"vg_bad_inplace\": %zu, ", keep->size());
  }
  // ScanCloud::voxelDownsample on a copy of view 1 (rich)
  {
    mvr::ScanCloud sc = model.views[1];
    const size_t removed = sc.voxelDownsample(1.0f);
    std::vector<float> v;
    for (size_t i = 0; i < sc.rich.size(); ++i) {
      const mvr::io::RichPoint &q = sc.rich[i];
      float rgb[3] = {(float)q.r, (float)q.g, (float)q.b};
      v.insert(v.end(), {q.x, q.y, q.z, q.normal_x, q.normal_y, q.normal_z, q.curvature, rgb[0], rgb[1], rgb[2]});
    }
    row("scan", v);
    std::printf("\"scan_removed\": %zu, \"scan_points\": %zu, ", removed, sc.points.size());
  }
  // saveRegisteredPoints with and without a leaf
  {
    mvr::Registrator reg(&model);
    float piv[3]; double pv[3], ax[3];
    mvr_synth_prior(&sp, pv, ax);
    reg.setPivotPoint(pv[0], pv[1], pv[2]); reg.setAxisNormal(ax[0], ax[1], ax[2]); (void)piv;
    for (int v = 0; v < 4; ++v) { model.views[v].initRotation(reg); model.views[v].setRegisterState(true); }
    mvr::io::RichCloud full, ds;
    const size_t nf = reg.saveRegisteredPoints(0, dir + "/full", &full);
    const size_t nd = reg.saveRegisteredPoints(0, dir + "/ds", 1.0f, &ds);
    std::printf("\"full_n\": %zu, \"ds_n\": %zu, \"ds_out\": %zu", nf, nd, ds.size());
  }
  std::printf("}\n");
  return 0;
}
"""


def test_cxx_voxel_grid_scan_and_save(ctx, mvr, built, tmp_path):
    built.build_hip()
    src = tmp_path / "voxel_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "voxel_driver"
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    for d in ("full", "ds"):
        os.makedirs(tmp_path / d)
    r = subprocess.run([str(exe), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "No input dataset given" in r.stderr
    out = json.loads(r.stdout)
    assert out["vg_none"] == 0
    sp = mvr.synth_params(4, 2)
    views = [mvr.synth_view(sp, v, 40000, normals=True) for v in range(4)]
    # pcl::VoxelGrid == Context.voxel_grid, bit for bit
    ctx.upload(0, views[0][0])
    ctx.voxel_grid(1, 0, (1.0, 1.5, 0.75), min_points=2)
    vg = np.asarray(out["vg"], np.uint32).reshape(-1, 3)
    assert len(vg) > 1000 and np.array_equal(vg, bits(ctx.download(1)[:, :3]))
    assert np.array_equal(np.asarray(out["vg_inplace"], np.uint32).reshape(-1, 3), vg)
    assert out["vg_bad_inplace"] == 40000 and "must be finite and > 0" in r.stderr
    # ScanCloud::voxelDownsample on a rich cloud against the reference
    p, nr = views[1]
    i = np.arange(40000)
    rgb = np.stack([(i * 7 + 1) % 256, (i * 13) % 256, 255 - i % 200], 1).astype(np.uint8)
    curv = ((i % 97) * 0.001).astype(np.float64).astype(F32)
    ref = R.voxel_grid(p, 1.0, normals=nr)
    scan = np.asarray(out["scan"], np.uint32).view(F32).reshape(-1, 10)
    assert len(scan) == len(ref["pts"]) == out["scan_points"] and out["scan_removed"] == 40000 - len(scan)
    ctx.upload(0, p)
    ctx.upload_normals(0, nr)
    ctx.voxel_grid(1, 0, 1.0)
    assert np.array_equal(bits(scan[:, :3]), bits(ctx.download(1)[:, :3]))
    assert np.array_equal(bits(scan[:, 3:6]), bits(ctx.download_normals(1)[:, :3]))
    assert ulps(scan[:, :3], ref["pts"][:, :3]).max() <= 1
    er, ec = R.rich_average(ref["voxel_of"], len(scan), rgb, curv)
    assert np.array_equal(scan[:, 7:10].astype(np.uint8), er)
    assert np.array_equal(bits(scan[:, 6]), bits(ec))
    # saveRegisteredPoints(..., leaf): the existing overload's merged cloud put through voxel_grid
    _, full = read_pcd(str(tmp_path / "full" / "points.pcd"))
    _, ds = read_pcd(str(tmp_path / "ds" / "points.pcd"))
    assert out["full_n"] == len(full) == 160000 and out["ds_n"] == out["ds_out"] == len(ds) < len(full)
    fx = np.ones((len(full), 4), F32)
    fx[:, 0], fx[:, 1], fx[:, 2] = full["x"], full["y"], full["z"]
    fn = np.zeros((len(full), 4), F32)
    fn[:, 0], fn[:, 1], fn[:, 2] = full["normal_x"], full["normal_y"], full["normal_z"]
    ctx.upload(0, fx)
    ctx.upload_normals(0, fn)
    n, vmap = ctx.voxel_grid(1, 0, 1.0, return_map=True)
    assert n == len(ds)
    got = ctx.download(1)
    gn = ctx.download_normals(1)
    for k, c in enumerate("xyz"):
        assert np.array_equal(bits(ds[c]), bits(got[:, k]))
        assert np.array_equal(bits(ds["normal_" + c]), bits(gn[:, k]))
    frgb = np.ascontiguousarray(full["rgb"]).view(np.uint32)
    fr = np.stack([(frgb >> 16) & 255, (frgb >> 8) & 255, frgb & 255], 1).astype(np.uint8)
    er, ec = R.rich_average(vmap, n, fr, np.asarray(full["curvature"], F32))
    drgb = np.ascontiguousarray(ds["rgb"]).view(np.uint32)
    assert np.array_equal(np.stack([(drgb >> 16) & 255, (drgb >> 8) & 255, drgb & 255], 1).astype(np.uint8), er)
    assert np.array_equal(bits(np.asarray(ds["curvature"], F32)), bits(ec))

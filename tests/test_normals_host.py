"""CPU tests of the k-NN / normal estimation feature that need no device: the C-ABI rejects NULL arguments before touching
the GPU, the numpy reference (tests/normals_ref.py) is right on shapes with known normals, the PCL-style C++ shim compiles,
and every kernel of csrc/mvr_knn.hip keeps its k-best list in registers (no scratch memory)."""
import os
import re
import subprocess

import numpy as np

import normals_ref as R
from conftest import PKG, ROOT


def test_knn_and_normals_reject_null_arguments_before_touching_the_gpu(mvr):
    import ctypes as C
    L, NULL = mvr._lib, None
    idx, d2 = (C.c_uint32 * 8)(), (C.c_float * 8)()
    assert L.mvr_knn(NULL, 0, 1, 4, 0, idx, d2) == mvr.E_ARG
    slots = (C.c_int * 2)(0, 1)
    p = mvr.NormalParams(8, 0.0, (C.c_float * 3)(0, 0, 0), 0)
    assert L.mvr_cloud_estimate_normals(NULL, 2, slots, C.byref(p), NULL) == mvr.E_ARG
    assert mvr.MAX_KNN == 64


def test_reference_plane_gives_the_exact_normal():
    rng = np.random.default_rng(1)
    uv = rng.uniform(-5, 5, (400, 2))
    n = np.array([1.0, 2.0, -2.0]) / 3.0
    a = np.cross(n, [1.0, 0, 0]); a /= np.linalg.norm(a)
    b = np.cross(n, a)
    p = np.ones((400, 4), np.float32)
    p[:, :3] = (uv[:, :1] * a + uv[:, 1:] * b + np.array([3.0, -1.0, 50.0])).astype(np.float32)
    idx, _ = R.knn_brute(p, p, 12)
    nrm, curv, _ = R.normals_from_lists(p, idx)
    assert R.angle_between(nrm, np.tile(n, (400, 1)), unsigned=True).max() < 1e-5
    assert np.abs(curv).max() < 1e-6
    # towards the origin (the default viewpoint): n . (0 - p) >= 0
    assert (np.sum(nrm[:, :3] * -p[:, :3], 1) >= 0).all()


def test_reference_sphere_gives_radial_normals():
    rng = np.random.default_rng(2)
    d = rng.standard_normal((20000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = np.array([0.0, 0.0, 100.0])
    p = np.ones((20000, 4), np.float32); p[:, :3] = (c + 20.0 * d).astype(np.float32)
    flat, offs = R.radius_sets(p, 2.0)
    nrm, curv, _ = R.normals_from_sets(p, flat, offs, viewpoint=c)
    ang = np.degrees(R.angle_between(nrm, d, unsigned=True))
    assert np.median(ang) < 1.0 and ang.max() < 5.0, (np.median(ang), ang.max())
    # viewpoint at the centre: every normal points inwards
    assert (np.sum(nrm[:, :3] * d, 1) < 0).all()
    assert (curv > 0).all() and (curv < 0.05).all()


def test_reference_flip_is_strict():
    p = np.array([[0, 0, 10, 1], [0, 0, 10, 1], [5, 0, 0, 1]], np.float32)
    nf = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 1]], np.float32)      # cos = -10, +10, 0
    out = R.flip_towards(p, nf, (0, 0, 0))
    assert np.array_equal(out, np.array([[0, 0, -1], [0, 0, -1], [0, 0, 1]], np.float32))


def test_reference_fewer_than_three_neighbours_is_nan():
    p = np.array([[0, 0, 0, 1], [0.5, 0, 0, 1], [50, 0, 0, 1], [60, 0, 0, 1], [60.2, 0, 0, 1], [60, 0.2, 0, 1]], np.float32)
    flat, offs = R.radius_sets(p, 1.0)
    nrm, curv, _ = R.normals_from_sets(p, flat, offs)
    assert np.isnan(nrm[:3, :3]).all() and np.isnan(curv[:3]).all()
    assert np.isfinite(nrm[3:]).all() and np.isfinite(curv[3:]).all()


SNIPPET = r"""
#include "mvr/registrator.hpp"
void estimate(pcl::PointCloud<pcl::PointXYZ>::Ptr cloud, pcl::PointCloud<pcl::Normal> &normals)
{
  pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
  ne.setInputCloud(cloud);
  pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>());
  ne.setSearchMethod(tree);
  ne.setKSearch(16);
  ne.setRadiusSearch(0.0);
  ne.setViewPoint(0.f, 0.f, 0.f);
  ne.compute(normals);
  const pcl::Normal &n = normals.points[0];
  (void)(n.normal_x + n.normal_y + n.normal_z + n.curvature + n.normal[0]);
  mvr::ScanCloud scan;
  scan.estimateNormals(16);
  scan.estimateNormals(0, 1.5);
}
static_assert(sizeof(pcl::Normal) == 32, "pcl::Normal layout");
"""


def test_pcl_style_normal_estimation_compiles(tmp_path):
    src = tmp_path / "ne.cpp"
    src.write_text(SNIPPET)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DMVR_ALIAS_PCL", "-I" + os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_knn_kernels_use_no_scratch(built, tmp_path):
    src = os.path.join(ROOT, PKG, "csrc", "mvr_knn.hip")
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "-c", src, "-o", str(tmp_path / "knn.o"),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    kernels = [n for n in names if "kernel" in n]
    assert len(kernels) == 18, names                   # k-NN and k-mode normals x KMAX 8/16/32/64 x fma, radius normals x fma
    assert len(scratch) == len(names) and all(s == 0 for s in scratch), list(zip(names, scratch))

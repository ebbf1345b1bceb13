"""CPU tests of the voxel-grid feature that need no device: the C-ABI rejects NULL arguments before touching the GPU, the
numpy reference (tests/voxel_ref.py) gets hand-computed cases right (negative coordinates, faces, anisotropic leaves,
min_points, PCL's overflow threshold from both sides), the PCL-style C++ code compiles, and the kernels of
csrc/mvr_voxel.hip use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import voxel_ref as R
from conftest import PKG, ROOT

F32 = np.float32


def cloud(xyz):
    p = np.ones((len(xyz), 4), F32)
    p[:, :3] = np.asarray(xyz, F32)
    return p


def test_voxel_grid_rejects_null_arguments_before_touching_the_gpu(mvr):
    L = mvr._lib
    leaf = (C.c_float * 3)(1.0, 1.0, 1.0)
    n, flag = C.c_size_t(7), C.c_int(7)
    assert L.mvr_cloud_voxel_grid(None, 0, 0, leaf, 0, C.byref(n), None, C.byref(flag)) == mvr.E_ARG
    assert L.mvr_cloud_voxel_grid(None, 0, 1, None, 0, None, None, None) == mvr.E_ARG
    assert n.value == 7 and flag.value == 7              # nothing written on a rejected call
    assert "mvr_cloud_voxel_grid" in mvr.SIGNATURES


def test_reference_negative_coordinates():
    p = cloud([[-0.5, 0, 0], [-1.5, 0, 0], [0.5, 0, 0], [-0.25, 0, 0], [-3.0, -2.0, -1.0]])
    r = R.voxel_grid(p, 1.0)
    # x voxels: floor(-0.5) = -1, floor(-1.5) = -2, 0, -1, -3; y: 0 / -2, z: 0 / -1 -> min_b = (-3, -2, -1), div = (4, 3, 2)
    # idx = (x + 3) + (y + 2) * 4 + (z + 1) * 12: (-3,-2,-1) -> 0; -2 -> 1 + 8 + 12 = 21; -1 -> 22 (two points); 0 -> 23
    assert list(r["idx"]) == [0, 21, 22, 23]
    assert np.array_equal(r["pts"][:, 0], F32([-3.0, -1.5, -0.375, 0.5]))
    assert list(r["voxel_of"]) == [2, 1, 3, 2, 0]
    assert (r["pts"][:, 3] == 1).all()


def test_reference_points_on_faces_go_to_the_upper_voxel():
    one = F32(1.0)
    below, above = np.nextafter(one, F32(0)), np.nextafter(one, F32(2))
    p = cloud([[0.0, 0, 0], [below, 0, 0], [one, 0, 0], [above, 0, 0], [2.0, 0, 0]])
    r = R.voxel_grid(p, 1.0)
    assert list(r["voxel_of"]) == [0, 0, 1, 1, 2]
    assert list(r["counts"]) == [2, 2, 1]
    # leaf 0.5 (inv = 2 exactly): the face at 0.5
    half = F32(0.5)
    p = cloud([[np.nextafter(half, F32(0)), 0, 0], [half, 0, 0], [0.0, 0, 0]])
    assert list(R.voxel_grid(p, 0.5)["voxel_of"]) == [0, 1, 0]


def test_reference_anisotropic_leaf_and_min_points():
    p = cloud([[0.2, 0.2, 0.2], [0.9, 1.9, 3.9], [1.1, 0.2, 0.2], [0.2, 2.1, 0.2], [0.2, 0.2, 4.1], [0.3, 0.3, 0.3]])
    r = R.voxel_grid(p, (1.0, 2.0, 4.0))
    # max_p = (1.1, 2.1, 4.1) -> max_b = (1, 1, 1), div = (2, 2, 2): idx = i + 2 j + 4 k
    assert list(r["idx"]) == [0, 1, 2, 4]
    assert list(r["counts"]) == [3, 1, 1, 1]
    assert list(r["voxel_of"]) == [0, 0, 1, 2, 3, 0]
    r2 = R.voxel_grid(p, (1.0, 2.0, 4.0), min_points=2)
    assert list(r2["voxel_of"]) == [0, 0, R.NONE, R.NONE, R.NONE, 0] and len(r2["pts"]) == 1
    assert np.allclose(r2["pts"][0, :3], np.mean(p[[0, 1, 5], :3].astype(np.float64), 0))
    assert len(R.voxel_grid(p, 1.0, min_points=7)["pts"]) == 0


def test_reference_overflow_threshold_from_both_sides():
    """d = (2^11, 2^10, 2^10 - 1): 2^31 - 2^21 voxels, below INT32_MAX; d = (2^11, 2^10, 2^10) = 2^31: the input passes through
    (2^31 - 1 is prime, and no f32 product reaches it on one axis)"""
    below = cloud([[0, 0, 0], [2047, 1023, 1022], [5, 5, 5]])
    passthrough, geo = R.overflow(below, 1.0)
    assert not passthrough and list(geo[2]) == [2048, 1024, 1023]
    r = R.voxel_grid(below, 1.0)
    assert not r["passthrough"] and list(r["idx"]) == [0, 5 + 5 * 2048 + 5 * 2048 * 1024, 2047 + 1023 * 2048 + 1022 * 2048 * 1024]
    at = cloud([[0, 0, 0], [2047, 1023, 1023], [np.nan, 1, 1]])
    r = R.voxel_grid(at, 1.0)
    assert r["passthrough"] and list(r["voxel_of"]) == [0, 1, 2] and np.array_equal(r["pts"][:2], at[:2])
    # one axis whose product reaches 2^31 on its own
    assert R.overflow(cloud([[0, 0, 0], [2.0 ** 31, 0, 0]]), 1.0)[0]
    assert not R.overflow(cloud([[0, 0, 0], [2.0 ** 31 - 256, 0, 0]]), 1.0)[0]


def test_reference_non_finite_points_belong_to_no_voxel():
    p = cloud([[0.5, 0.5, 0.5], [np.nan, 0, 0], [1.5, 0.5, 0.5], [np.inf, 1e9, 1e9], [0.25, 0.25, -np.inf]])
    r = R.voxel_grid(p, 1.0)
    assert list(r["voxel_of"]) == [0, R.NONE, 1, R.NONE, R.NONE]
    assert len(R.voxel_grid(cloud([[np.nan, 0, 0]]), 1.0)["pts"]) == 0


SNIPPET = r"""
#include "mvr/registrator.hpp"
void downsample(pcl::PointCloud<pcl::PointXYZ>::Ptr cloud, pcl::PointCloud<pcl::PointXYZ> &out, mvr::Registrator &reg)
{
  pcl::VoxelGrid<pcl::PointXYZ> vg;
  vg.setInputCloud(cloud);
  vg.setLeafSize(1.0f, 1.0f, 2.0f);
  vg.setMinimumPointsNumberPerVoxel(2);
  unsigned int m = vg.getMinimumPointsNumberPerVoxel();
  (void)m;
  vg.filter(out);
  mvr::ScanCloud scan;
  size_t removed = scan.voxelDownsample(0.5f);
  removed += scan.voxelDownsample(1.0f, 3);
  (void)removed;
  mvr::io::RichCloud merged;
  reg.saveRegisteredPoints(0, "out", 1.0f, &merged);
  reg.saveRegisteredPoints(0, "out", 1.0f);
  reg.saveRegisteredPoints(0, "out", &merged);
  reg.saveRegisteredPoints(0, "out");
}
"""


def test_pcl_style_voxel_grid_compiles(tmp_path):
    src = tmp_path / "vg.cpp"
    src.write_text(SNIPPET)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DMVR_ALIAS_PCL", "-I" + os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_voxel_kernels_use_no_scratch(built, tmp_path):
    src = os.path.join(ROOT, PKG, "csrc", "mvr_voxel.hip")
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "-c", src, "-o", str(tmp_path / "voxel.o"),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    usage = [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)))
             for b in blocks]
    own = [(n, s) for n, s in usage if "vox_" in n]
    # box x 2, map, key / head x 2 key widths, voxel x 2 key widths x 2 (normals), piece / long / out x 2 (normals)
    assert len(own) == 17, own
    assert all(s == 0 for _, s in own), own

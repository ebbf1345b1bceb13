"""CPU tests of the outlier filters that need no device: the C-ABI rejects bad arguments before touching the GPU and writes
nothing, the numpy reference (tests/outlier_ref.py) gets hand-computed cases right, the PCL-style C++ code compiles, the
kernels of csrc/mvr_outlier.hip use no scratch memory, and the distance-only list of the mean-distance kernel needs fewer
registers than the (d2, index) list of knn_kernel."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import outlier_ref as R
from conftest import PKG, ROOT

F32 = np.float32


def cloud(xyz):
    p = np.ones((len(xyz), 4), F32)
    p[:, :3] = np.asarray(xyz, F32)
    return p


# ------------------------------------------------------------------ argument checks

def _outputs():
    n = C.c_size_t(7)
    idx = (C.c_uint32 * 4)(9, 9, 9, 9)
    val = (C.c_float * 4)(9, 9, 9, 9)
    cnt = (C.c_uint32 * 4)(9, 9, 9, 9)
    return n, idx, val, cnt


def _untouched(n, idx, val, cnt):
    return n.value == 7 and list(idx) == [9] * 4 and list(val) == [9.0] * 4 and list(cnt) == [9] * 4


def test_outlier_filters_reject_bad_arguments_before_touching_the_gpu(mvr):
    L = mvr._lib
    assert "mvr_cloud_statistical_outlier_removal" in mvr.SIGNATURES and "mvr_cloud_radius_outlier_removal" in mvr.SIGNATURES
    # a context that is not one: any use of it, or any GPU work, would crash -- the argument checks come first
    fake = C.create_string_buffer(256)
    ctx = C.cast(fake, C.c_void_p)
    st = mvr.SorStats(1.0, 2.0, 3.0, 4)
    n, idx, val, cnt = _outputs()
    good = mvr.SorParams(8, 1.0, 0, 0)
    sor = L.mvr_cloud_statistical_outlier_removal
    assert sor(None, 0, 1, C.byref(good), C.byref(n), idx, val, C.byref(st)) == mvr.E_ARG
    assert sor(ctx, 0, 1, None, C.byref(n), idx, val, C.byref(st)) == mvr.E_ARG
    for k in (0, -1, mvr.MAX_KNN + 1, 1 << 20):
        assert sor(ctx, 0, 1, C.byref(mvr.SorParams(k, 1.0, 0, 0)), C.byref(n), idx, val, C.byref(st)) == mvr.E_ARG
    for m in (math.nan, math.inf, -math.inf):
        assert sor(ctx, 0, 1, C.byref(mvr.SorParams(8, m, 0, 0)), C.byref(n), idx, val, C.byref(st)) == mvr.E_ARG
    for d, s in ((-1, 0), (0, -1), (mvr.MAX_SLOTS, 0), (0, mvr.MAX_SLOTS)):
        assert sor(ctx, d, s, C.byref(good), C.byref(n), idx, val, C.byref(st)) == mvr.E_ARG
    ror = L.mvr_cloud_radius_outlier_removal
    rgood = mvr.RorParams(1.0, 2, 0, 0)
    assert ror(None, 0, 1, C.byref(rgood), C.byref(n), idx, cnt) == mvr.E_ARG
    assert ror(ctx, 0, 1, None, C.byref(n), idx, cnt) == mvr.E_ARG
    for r in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert ror(ctx, 0, 1, C.byref(mvr.RorParams(r, 2, 0, 0)), C.byref(n), idx, cnt) == mvr.E_ARG
    assert ror(ctx, 0, 1, C.byref(mvr.RorParams(1.0, -1, 0, 0)), C.byref(n), idx, cnt) == mvr.E_ARG
    for d, s in ((-1, 0), (0, -1), (mvr.MAX_SLOTS, 0), (0, mvr.MAX_SLOTS)):
        assert ror(ctx, d, s, C.byref(rgood), C.byref(n), idx, cnt) == mvr.E_ARG
    assert _untouched(n, idx, val, cnt)
    assert (st.mean, st.stddev, st.threshold, st.n_valid) == (1.0, 2.0, 3.0, 4)
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the reference, by hand

def test_reference_line_with_one_far_point():
    """x = 0, 1, 2, 3, 4 and 14; mean_k = 2.  Mean distances: 1.5, 1, 1, 1, 1.5, (10 + 11) / 2 = 10.5; their mean is 16.5 / 6 =
    2.75 and the squared deviations sum to 2 * 1.5625 + 3 * 3.0625 + 60.0625 = 72.375"""
    p = cloud([[x, 0, 0] for x in (0, 1, 2, 3, 4, 14)])
    r = R.statistical(p, 2, 1.0)
    assert list(r["mean_dist"]) == [1.5, 1.0, 1.0, 1.0, 1.5, 10.5]
    st = r["stats"]
    assert st["n_valid"] == 6 and st["mean"] == 2.75
    assert abs(st["stddev"] - math.sqrt(72.375 / 5)) < 1e-15
    assert abs(st["threshold"] - (2.75 + math.sqrt(72.375 / 5))) < 1e-15
    assert list(r["index"]) == [0, 1, 2, 3, 4]
    assert list(R.statistical(p, 2, 1.0, negative=True)["index"]) == [5]
    # a negative multiplier is allowed: threshold = 2.75 - 0.4 * 3.80... = 1.228...: only the three inner points stay
    assert list(R.statistical(p, 2, -0.4)["index"]) == [1, 2, 3]


def test_reference_duplicates_count_at_zero_distance():
    p = cloud([[0, 0, 0], [0, 0, 0], [0, 0, 0], [3, 4, 0]])
    md, nv = R.mean_dist(p, 2)
    assert nv == 4 and list(md) == [0.0, 0.0, 0.0, 5.0]
    md, _ = R.mean_dist(p, 3)
    assert np.array_equal(md, F32([5 / 3, 5 / 3, 5 / 3, 5.0]))
    # all points at one location: every mean distance 0, stddev 0, threshold 0 and 0 > 0 is false
    r = R.statistical(cloud([[1, 2, 3]] * 5), 3, 1.0)
    assert list(r["mean_dist"]) == [0.0] * 5 and r["stats"]["stddev"] == 0.0 and r["stats"]["threshold"] == 0.0
    assert list(r["index"]) == [0, 1, 2, 3, 4]


def test_reference_too_few_points_and_one_valid_point():
    p = cloud([[0, 0, 0], [1, 0, 0], [5, 0, 0]])
    r = R.statistical(p, 3, 1.0)                         # n - 1 < mean_k
    assert np.isnan(r["mean_dist"]).all() and r["stats"]["n_valid"] == 0 and math.isnan(r["stats"]["threshold"])
    assert list(r["index"]) == [0, 1, 2] and len(R.statistical(p, 3, 1.0, negative=True)["index"]) == 0
    r = R.statistical(p, 2, 0.0)                         # n - 1 == mean_k
    assert list(r["mean_dist"]) == [3.0, 2.5, 4.5] and r["stats"]["n_valid"] == 3
    assert abs(r["stats"]["mean"] - 10 / 3) < 1e-15 and list(r["index"]) == [0, 1]
    r = R.statistical(np.ones((0, 4), F32), 1, 1.0)
    assert len(r["index"]) == 0 and r["stats"]["n_valid"] == 0


def test_reference_non_finite_points_are_outliers_and_nobodys_neighbour():
    p = cloud([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0.5, np.inf, 0], [2, 0, 0], [0, 0, -np.inf]])
    r = R.statistical(p, 1, 5.0)
    md = r["mean_dist"]
    assert np.array_equal(np.isnan(md), [False, True, False, True, False, True])
    assert list(md[[0, 2, 4]]) == [1.0, 1.0, 1.0] and r["stats"]["n_valid"] == 3
    assert list(r["index"]) == [0, 2, 4] and list(R.statistical(p, 1, 5.0, negative=True)["index"]) == [1, 3, 5]
    rr = R.radius(p, 1.0, 1)
    assert list(rr["count"]) == [1, 0, 2, 0, 1, 0] and list(rr["index"]) == [0, 2, 4]
    assert list(R.radius(p, 1.0, 2, negative=True)["index"]) == [0, 1, 3, 4, 5]
    # two finite points and mean_k = 2: nobody has a mean distance, the finite points stay
    r = R.statistical(p[:4], 2, 1.0)
    assert list(r["index"]) == [0, 2] and r["stats"]["n_valid"] == 0


def test_reference_radius_counts_the_boundary():
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    p = cloud(g)
    cnt = R.neighbor_counts(p, 1.0)                      # neighbours at d2 == r2 exactly: they count
    inner = ((g > 0) & (g < 3)).sum(1)
    assert np.array_equal(cnt, 3 + inner)
    assert np.array_equal(R.neighbor_counts(p, 0.999), np.zeros(64, np.uint32))
    r = R.radius(p, 1.0, 6)
    assert len(r["index"]) == 8 and np.array_equal(r["index"], np.nonzero(inner == 3)[0])
    assert len(R.radius(p, 1.0, 0)["index"]) == 64


def test_reference_fma_distance_is_one_rounding():
    """dx = 2^-12, dy = 1 + 2^-12: dx*dx = 2^-24 and dy*dy = 1 + 2^-11 + 2^-24 exactly.  Rounded per operation, dy*dy is a tie
    and goes to the even 1 + 2^-11, and adding 2^-24 is the same tie again.  The fma adds 2^-24 to the exact product:
    1 + 2^-11 + 2^-23, one ulp more."""
    a = F32([[0, 0, 0]])
    b = F32([[2.0 ** -12, 1 + 2.0 ** -12, 0]])
    assert R.d2_f32(a, b)[0] == F32(1 + 2.0 ** -11)
    assert R.d2_f32(a, b, fma=True)[0] == F32(1 + 2.0 ** -11 + 2.0 ** -23)
    # the last step of the chain likewise
    b = F32([[2.0 ** -12, 0, 1 + 2.0 ** -12]])
    assert R.d2_f32(a, b)[0] == F32(1 + 2.0 ** -11)
    assert R.d2_f32(a, b, fma=True)[0] == F32(1 + 2.0 ** -11 + 2.0 ** -23)


# ------------------------------------------------------------------ the C++ names

SNIPPET = r"""
#include "mvr/registrator.hpp"
size_t clean(pcl::PointCloud<pcl::PointXYZ>::Ptr cloud, pcl::PointCloud<pcl::PointXYZ> &out, std::vector<int> &idx)
{
  pcl::StatisticalOutlierRemoval<pcl::PointXYZ> sor(true);
  sor.setInputCloud(cloud);
  sor.setMeanK(50);
  sor.setStddevMulThresh(1.0);
  sor.setNegative(false);
  int k = sor.getMeanK(); double m = sor.getStddevMulThresh(); bool neg = sor.getNegative();
  (void)k; (void)m; (void)neg;
  sor.filter(out);
  sor.filter(*cloud);
  sor.filter(idx);
  size_t removed = sor.getRemovedIndices()->size();
  pcl::RadiusOutlierRemoval<pcl::PointXYZ> ror;
  ror.setInputCloud(cloud);
  ror.setRadiusSearch(0.8);
  ror.setMinNeighborsInRadius(2);
  ror.setNegative(true);
  double r = ror.getRadiusSearch(); int mn = ror.getMinNeighborsInRadius();
  (void)r; (void)mn;
  ror.filter(out);
  ror.filter(idx);
  pcl::RadiusOutlierRemoval<pcl::PointXYZ> ror2(true);
  removed += ror2.getRemovedIndices()->size();
  mvr::ScanCloud scan;
  removed += scan.removeStatisticalOutliers(16, 2.0);
  removed += scan.removeRadiusOutliers(1.5, 4);
  return removed;
}
"""


def test_pcl_style_outlier_removal_compiles(tmp_path):
    src = tmp_path / "outlier.cpp"
    src.write_text(SNIPPET)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DMVR_ALIAS_PCL", "-I" + os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


# ------------------------------------------------------------------ the kernels' resources

def _usage(built, tmp_path, name):
    """[(kernel, VGPRs, scratch bytes per lane)] from the compiler's remarks for one source file (device code only)"""
    src = os.path.join(ROOT, PKG, "csrc", name)
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / (name + ".o")),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    return [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
             int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))) for b in blocks]


@pytest.fixture(scope="module")
def outlier_usage(built, tmp_path_factory):
    return _usage(built, tmp_path_factory.mktemp("outl"), "mvr_outlier.hip")


def test_outlier_kernels_use_no_scratch(outlier_usage):
    own = [(n, s) for n, _, s in outlier_usage if "outl_" in n]
    # finite, mean distance x KMAX 8/16/32/64 x fma, count x fma, sum x 2 passes, final x 2 passes, flag x 2 filters
    assert len(own) == 17, own
    assert all(s == 0 for _, s in own), own
    # the hipCUB selection kernels the file instantiates as well
    assert all(s == 0 for _, _, s in outlier_usage), [(n, s) for n, _, s in outlier_usage if s]


def test_distance_only_list_needs_fewer_registers_than_the_knn_list(built, outlier_usage, tmp_path):
    knn = _usage(built, tmp_path, "mvr_knn.hip")
    for kmax in (8, 16, 32, 64):
        for fma in (0, 1):
            mine = [v for n, v, _ in outlier_usage if "outl_mean_dist_kernelILi%dELb%d" % (kmax, fma) in n]
            theirs = [v for n, v, _ in knn if "10knn_kernelILi%dELb%d" % (kmax, fma) in n]
            assert len(mine) == 1 and len(theirs) == 1, (kmax, fma, mine, theirs)
            print("KMAX %d fma %d: mean-distance kernel %d VGPRs, knn_kernel %d" % (kmax, fma, mine[0], theirs[0]))
            if kmax == 64:
                assert mine[0] < theirs[0], (kmax, fma, mine, theirs)
